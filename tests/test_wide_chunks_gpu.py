"""dcf_eval_device at LAMBDA >= 32 over more points than one head/tail pass takes.

A key's points run in passes of 2^22 (dcf_hip.hip kWideChunk at N <= 31): the CW digest and the
shared-prefix table are made for the first pass and read again by every later one, while xs, ys and
the t-vector scratch start afresh.  Every case evaluates m = 2^22 + 70 points (a second pass of one
64-point unit and a partial one), both parties, and checks
  - rows [0, 2^22) byte for byte against eval_device of xs[:2^22] alone, rows [2^22, m) against
    eval_device of xs[2^22:] alone (check_chunks);
  - the sentinel rows on either side of ys;
  - both parties against the CPU oracle on the first and last 64 rows, the 128 rows around the pass
    boundary and 256 seeded random rows, and the key against the oracle's gen;
  - y0 ^ y1 == beta * [x < alpha] (GtBeta: >) on every row.
x = alpha sits at row 0 and at row 2^22, its neighbours in the last byte beside the boundary.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_multikey_dispatch_gpu import want_reconstruction
from tests.test_range_gpu import PAD, SENTINEL

pytestmark = pytest.mark.gpu

CHUNK = 1 << 22     # points per pass
M = CHUNK + 70


@dataclass(frozen=True)
class Case:
    id: str
    kind: str       # "hirose" / "mmo"
    lam: int
    nb: int
    bound: int
    depth: int      # the shared-prefix depth the call must plan
    levels: int = -1  # dcf_prg_set_prefix_levels


CASES = [
    # masked head, no tail; the automatic table (min(log2(m) - 1, 8N - 1) = 15) serves both passes
    Case("hirose32-n2-table15", "hirose", 32, 2, 0, 15),
    # 4-bit tail below the same table
    Case("hirose48-n2-tail4", "hirose", 48, 2, 1, 15),
    # paired-slot tail, table off: both passes walk from the root
    Case("hirose128-n1-tail2-no-table", "hirose", 128, 1, 0, 0, levels=0),
    # eval_mmo_wide's own pass loop (the MMO PRG builds no table)
    Case("mmo32-n2", "mmo", 32, 2, 1, 0),
]
CASE_IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


def check_chunks(ys, first, second, what):
    """The whole call's rows against its two passes evaluated alone, byte for byte (device tensors)."""
    import torch
    for name, got, want, base in (("first pass", ys[:CHUNK], first, 0), ("second pass", ys[CHUNK:], second, CHUNK)):
        assert got.shape == want.shape, (what, name, got.shape, want.shape)
        if not torch.equal(got, want):
            bad = torch.nonzero((got != want).any(dim=1)).flatten()[:8] + base
            raise AssertionError((what, name, "differs from the pass evaluated alone, rows", bad.tolist()))


def oracle_rows(rng):
    return np.unique(np.concatenate([np.arange(64), np.arange(M - 64, M), np.arange(CHUNK - 64, CHUNK + 64),
                                     rng.integers(0, M, size=256)]))


@dataclass
class Result:
    case: Case
    ys: list       # per party: (M, lam) device tensor, the whole call
    first: list    # per party: eval_device of xs[:CHUNK] alone
    second: list   # per party: eval_device of xs[CHUNK:] alone
    rows: np.ndarray
    want: list     # per party: the oracle's outputs on `rows`
    rec: np.ndarray  # (M, lam) expected y0 ^ y1


@lru_cache(maxsize=1)
def compute(dcf, case):
    """Gen, the three evals of each party and the host-side expectations.  One result is kept: the
    self-test and the first case share it."""
    import torch
    lam, nb = case.lam, case.nb
    rng = np.random.default_rng([0xC4C4, CASE_IDS.index(case.id)])
    if case.kind == "mmo":
        keys = [rng.bytes(16) for _ in range(4 * lam // 16)]
        prg, Po = dcf.Aes128MatyasMeyerOseasPrg(keys, lam), O.OracleMmoPrg(keys, lam)
    else:
        keys = [rng.bytes(32) for _ in range(18)]
        prg, Po = dcf.Aes256HirosePrg(keys, lam), O.OraclePrg(keys, lam)
    prg.set_prefix_levels(case.levels)
    # the plan first: the table really is there (or really is not)
    assert prg.eval_prefix_levels(nb, 1, M) == case.depth, (case.id, prg.eval_prefix_levels(nb, 1, M))
    assert prg.eval_plan(nb, 1, M).engine == dcf.Engine.WIDE_PER_KEY
    d = dcf.DcfImpl(nb, lam, prg)
    alpha, beta, s0, s1 = rng.bytes(nb), rng.bytes(lam), rng.bytes(lam), rng.bytes(lam)
    ok = O.gen(Po, alpha, beta, s0, s1, case.bound)
    k = d.gen(dcf.CmpFn(alpha, beta), [s0, s1], dcf.BoundState(case.bound))
    cwb = dcf.share_to_cwb(k, nb, lam)
    raw = ok.cw_s.tobytes() + ok.cw_v.tobytes() + ok.cw_t.tobytes()
    assert cwb == raw + bytes((-len(raw)) % 16) + ok.cw_np1.tobytes(), (case.id, "gen differs from the oracle")
    a = np.frombuffer(alpha, np.uint8)
    xs = rng.integers(0, 256, size=(M, nb), dtype=np.uint8)
    xs[[0, CHUNK - 1, CHUNK, CHUNK + 1]] = a
    xs[CHUNK - 1:CHUNK, -1] -= 1  # wraps mod 256, like the neighbours the other suites plant
    xs[CHUNK + 1:CHUNK + 2, -1] += 1
    T = lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()  # noqa: E731
    cwb_d, xd = T(cwb), torch.from_numpy(xs).cuda()
    rows = oracle_rows(rng)
    pts = np.ascontiguousarray(xs[rows])
    res = Result(case, [], [], [], rows, [], None)
    for b, s in ((0, s0), (1, s1)):
        sd = T(s)
        buf = torch.full((M + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
        d.eval_device(bool(b), cwb_d, sd, xd, ys=buf[PAD:PAD + M])
        torch.cuda.synchronize()
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + M:] == SENTINEL).all()), \
            (case.id, "neighbours of ys written", "party", b)
        res.ys.append(buf[PAD:PAD + M])
        res.first.append(d.eval_device(bool(b), cwb_d, sd, xd[:CHUNK]))
        res.second.append(d.eval_device(bool(b), cwb_d, sd, xd[CHUNK:]))
        res.want.append(O.eval_(Po, b, ok, s, pts, nthreads=8))
    torch.cuda.synchronize()
    res.rec = want_reconstruction(xs, a[None, :], np.frombuffer(beta, np.uint8)[None, :], M, case.bound)
    return res


def check(res):
    case = res.case
    for b in (0, 1):
        check_chunks(res.ys[b], res.first[b], res.second[b], (case.id, "party", b))
    ys = [y.cpu().numpy() for y in res.ys]
    for b in (0, 1):
        bad = np.flatnonzero((ys[b][res.rows] != res.want[b]).any(axis=1))
        assert bad.size == 0, (case.id, "oracle", "party", b, "rows", res.rows[bad[:8]])
    bad = np.flatnonzero(((ys[0] ^ ys[1]) != res.rec).any(axis=1))
    assert bad.size == 0, (case.id, "reconstruction", "first rows", bad[:8])
    assert not (ys[0][[0, CHUNK]] ^ ys[1][[0, CHUNK]]).any()  # f(alpha) = 0 under both bounds


# ---- the comparison's own test comes first ----

def test_chunk_comparison_rejects_a_one_byte_corruption(dcf):
    """A correct result: one byte flipped in row 2^22 fails the second pass's comparison, one in row
    2^22 - 1 the first pass's; untouched, both pass."""
    res = compute(dcf, CASES[0])
    y, first, second = res.ys[1], res.first[1], res.second[1]
    check_chunks(y, first, second, "clean")
    for row, name in ((CHUNK, "second pass"), (CHUNK - 1, "first pass")):
        bad = y.clone()
        bad[row, res.case.lam - 1] ^= 0x10
        with pytest.raises(AssertionError, match=name) as e:
            check_chunks(bad, first, second, "corrupted")
        assert str(row) in str(e.value)
        del bad


# ---- the cases ----

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_second_pass(dcf, case):
    check(compute(dcf, case))
