"""dcf_eval_multikey_device on both sides of every branch plan_eval takes for K > 1.

Every case names the route it was written for (engine, key mode, per-key top trees); the runner
asks dcf_eval_plan first and asserts that route, so a case cannot drift onto another kernel unseen.
The boundaries that depend on the device (small against stream: K * P = 2 * CUs * 1024) are found
by bisection on dcf_eval_plan, never from constants: the cases sit at m - 1 and m, and
test_every_edge_is_an_edge asserts that the plan differs across each edge.  A threshold that moves
keeps the cases on its two sides; an edge that disappears fails.

The runner (run_case) gens K keys with gen_batch_device, evaluates both parties into a ys with PAD
sentinel rows on either side, synchronises and checks
  - the sentinels;
  - y0 ^ y1 == beta[k] * [x < alpha[k]] (GtBeta: >) on EVERY row;
  - both parties bit for bit against the CPU oracle on the sampled keys (sample_keys) and rows
    (sample_rows), and the CWB of those keys against the oracle's gen.
Points (make_points): every key's first rows hold alpha[k], alpha[k] +- 1 in the last byte and
tests/test_stream_update_emulation.py's patterned points (all-0xFF, all-0x00, alternating, runs of
ones ending at the word edges); its last rows hold the patterned points again in reverse, so the
row beside the next key's first row is all-0xFF (right steps only) and the rows before it carry
the long runs.  A key with fewer rows than that list takes the list round robin, key k starting
where key k - 1 stopped, so K keys of 1 point still cover alpha, its neighbours and the patterns.
"""
from dataclasses import dataclass, replace
from functools import lru_cache

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_range_gpu import PAD, SENTINEL
from tests.test_stream_update_emulation import patterned

pytestmark = pytest.mark.gpu

MAX_ORACLE_KEYS = 80   # sampled keys of a case with K > 64, at most
MAX_ORACLE_ROWS = 128  # sampled rows of a key with more points than this
TREE_LEVELS = 5        # depth of the multi-key stream engine's per-key top trees (include/dcf_hip.h)


@dataclass(frozen=True)
class Case:
    """One multi-key shape and the route it is written for.  K may be ("small_edge", d): the
    smallest K whose plan is not `small` at this (PRG, N, P, mode), plus d (resolve)."""
    id: str
    kind: str = "hirose"
    lam: int = 16
    nb: int = 2
    K: object = 5
    P: int = 64
    mode: object = None    # None: the PRG's default (Hirose: automatic; MMO: DCF_EVAL_TTABLE)
    levels: int = -1
    bound: int = 0
    engine: str = "PAIR"   # dcf_amd.Engine member the plan must name
    small: object = None   # the plan's `small`, where the case is about it
    trees: object = None   # per-key top trees: the depth dcf_prg_last_eval_phases reports (5 / 0)
    depth: object = None   # the plan's prefix_levels, where the case is about it


def key_mode_of(P):
    return 1 if P % 64 == 0 else 2


KM_P = (1, 31, 32, 33, 63, 64, 65, 127, 128, 192 + 1)


def _key_mode_cases():
    """K = 5, N = 2 and 16, P on both sides of every multiple of 64 up to 192: the lockstep T-table
    walk (mode 1), the pair walk (automatic mode) and the MMO kernel, each under key modes 1 and 2."""
    out = []
    for nb in (2, 16):
        for i, P in enumerate(KM_P):
            b = (i + nb // 16) % 2
            out.append(Case(f"km-ttable-n{nb}-P{P}", nb=nb, P=P, mode=1, bound=b, engine="TTABLE"))
            out.append(Case(f"km-pair-n{nb}-P{P}", nb=nb, P=P, mode=0, bound=1 - b, engine="PAIR", small=True))
            out.append(Case(f"km-mmo-n{nb}-P{P}", kind="mmo", nb=nb, P=P, bound=b, engine="MMO16"))
    return out


def _top_tree_cases():
    """Stream engine (mode 4), per-key top trees on each side of ppk >= 32 and of prefix_levels != 0,
    at N = 1 (8 levels: the tree ends 3 above the leaves), for K = 3 and K = 130 (more than a wave
    of keys in k_mk_prefix16); then every instance eval_stream picks below the trees: N = 16 and
    N = 4 with a power-of-two and a generic P, x in registers (N = 8) and in memory (N = 3)."""
    out = []
    for K in (3, 130):
        out += [Case(f"trees-P31-K{K}", K=K, P=31, mode=4, engine="STREAM", trees=0),
                Case(f"trees-P32-K{K}", K=K, P=32, mode=4, bound=1, engine="STREAM", trees=TREE_LEVELS),
                Case(f"trees-levels0-K{K}", K=K, P=64, mode=4, levels=0, bound=1, engine="STREAM", trees=0),
                Case(f"trees-auto-K{K}", K=K, P=64, mode=4, engine="STREAM", trees=TREE_LEVELS),
                Case(f"trees-n1-K{K}", nb=1, K=K, P=64, mode=4, bound=K % 2, engine="STREAM", trees=TREE_LEVELS)]
    for nb, P in ((16, 64), (16, 33), (4, 64), (4, 33), (8, 64), (3, 64)):
        out.append(Case(f"stream-n{nb}-P{P}", nb=nb, K=3, P=P, mode=4, bound=P % 2, engine="STREAM", trees=TREE_LEVELS))
    return out


def _small_edge_cases():
    """Automatic mode, N = 2: the largest K that is `small` (pair walk) and the next (stream), at
    P = 64 (key mode 1) and P = 33 (key mode 2); the same K * P at N = 32 (stream) and N = 33
    (T-table); the MMO kernel on both sides (its plan is `small` only in automatic mode)."""
    out = []
    for P in (64, 33):
        out += [Case(f"edge-pair-P{P}", K=("small_edge", -1), P=P, mode=0, bound=P % 2, engine="PAIR", small=True),
                Case(f"edge-stream-P{P}", K=("small_edge", 0), P=P, mode=0, bound=1 - P % 2, engine="STREAM", small=False,
                     trees=TREE_LEVELS)]
    out += [Case("edge-n32-stream", nb=32, K=("small_edge", 0), P=64, mode=0, engine="STREAM", small=False, trees=TREE_LEVELS),
            Case("edge-n33-ttable", nb=33, K=("small_edge", 0), P=64, mode=0, bound=1, engine="TTABLE", small=False),
            Case("edge-mmo-small", kind="mmo", K=("small_edge", -1), P=64, mode=0, engine="MMO16", small=True),
            Case("edge-mmo-past-lt", kind="mmo", K=("small_edge", 0), P=64, mode=0, engine="MMO16", small=False),
            Case("edge-mmo-past-gt", kind="mmo", K=("small_edge", 0), P=64, mode=0, bound=1, engine="MMO16", small=False)]
    return out


def _wide_cases():
    """LAMBDA >= 32, N = 1 unless the depth needs more levels: the batched passes against the per-key
    passes at P = 32768 / 32769, one pass of 4096 keys against two, the second pass's tail grid rows
    at LAMBDA = 48, a forced depth and the MMO PRG (both key by key)."""
    out = []
    for lam in (32, 48):
        b = lam // 16 % 2
        out += [Case(f"wide{lam}-batch-P32768", lam=lam, nb=1, K=2, P=32768, bound=b, engine="WIDE_BATCH"),
                Case(f"wide{lam}-perkey-P32769", lam=lam, nb=1, K=2, P=32769, bound=1 - b, engine="WIDE_PER_KEY"),
                Case(f"wide{lam}-K4096", lam=lam, nb=1, K=4096, P=2, bound=1 - b, engine="WIDE_BATCH"),
                Case(f"wide{lam}-K4097", lam=lam, nb=1, K=4097, P=2, bound=b, engine="WIDE_BATCH"),
                Case(f"wide{lam}-depth8", lam=lam, nb=2, K=3, P=300, levels=8, bound=b, engine="WIDE_PER_KEY", depth=8)]
    out += [Case("wide48-K4097-P9", lam=48, nb=1, K=4097, P=9, bound=1, engine="WIDE_BATCH"),
            Case("wide32-mmo", kind="mmo", lam=32, nb=1, K=3, P=70, engine="WIDE_PER_KEY")]
    return out


CASES = _key_mode_cases() + _top_tree_cases() + _small_edge_cases() + _wide_cases()
assert len({c.id for c in CASES}) == len(CASES)

# Engines a call with K > 1 can reach (all but the single-key latency kernels), and those whose
# kernel is instantiated per key mode.
MULTIKEY_ENGINES = {"WIDE_BATCH", "WIDE_PER_KEY", "MMO16", "PAIR", "STREAM", "TTABLE"}
KEY_MODE_ENGINES = {"MMO16", "PAIR", "TTABLE"}


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


@lru_cache(maxsize=None)
def _aes_keys(kind, lam):
    rng = np.random.default_rng([0xD15, lam, int(kind == "mmo")])
    if kind == "mmo":
        return tuple(rng.bytes(16) for _ in range(4 * lam // 16))
    return tuple(rng.bytes(32) for _ in range(2 if lam == 16 else 18))


@lru_cache(maxsize=None)
def oracle_prg(kind, lam):
    keys = list(_aes_keys(kind, lam))
    return O.OracleMmoPrg(keys, lam) if kind == "mmo" else O.OraclePrg(keys, lam)


def new_prg(dcf, case):
    """A fresh dcf_prg under the case's settings (nothing leaks from case to case)."""
    keys = list(_aes_keys(case.kind, case.lam))
    prg = (dcf.Aes128MatyasMeyerOseasPrg if case.kind == "mmo" else dcf.Aes256HirosePrg)(keys, case.lam)
    if case.mode is not None:
        prg.set_eval_mode(case.mode)
    prg.set_prefix_levels(case.levels)
    return prg


def small_edge(prg, nb, P):
    """The smallest K >= 2 whose plan is not `small`, by bisection on dcf_eval_plan."""
    lo, hi = 2, 1 << 26
    assert prg.eval_plan(nb, lo, P).small and not prg.eval_plan(nb, hi, P).small, "no small / not-small edge in K"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if prg.eval_plan(nb, mid, P).small else (lo, mid)
    return hi


def resolve(dcf, case, prg=None):
    """The case with its K as a number."""
    if isinstance(case.K, tuple):
        tag, d = case.K
        assert tag == "small_edge"
        # the edge is a property of K * P alone: looked up at the case's PRG and mode, N = 2
        return replace(case, K=small_edge(prg or new_prg(dcf, case), 2, case.P) + d)
    return case


# ---- points, samples, expectations (host only) ----

def make_points(nb, alpha, P, rng):
    """(K * P, nb) points, key-major, as the module docstring lays them out."""
    K = alpha.shape[0]
    pat = np.stack([np.frombuffer(x, np.uint8) for x in patterned(nb)])  # [0] all-0xFF, [1] all-0x00
    H = 3 + len(pat)
    head = np.empty((K, H, nb), np.uint8)
    head[:, 0] = alpha
    head[:, 1] = alpha
    head[:, 1, -1] += 1  # wraps mod 256, like the neighbours the other suites plant
    head[:, 2] = alpha
    head[:, 2, -1] -= 1
    head[:, 3:] = pat
    xs = rng.integers(0, 256, size=(K, P, nb), dtype=np.uint8)
    if P >= H:
        xs[:, :H] = head
        for i in range(min(P - H, len(pat))):
            xs[:, P - 1 - i] = pat[i]
    else:
        idx = (np.arange(K)[:, None] * P + np.arange(P)[None, :]) % H
        xs[:] = head[np.arange(K)[:, None], idx]
    return xs.reshape(K * P, nb)


def sample_keys(K, P, rng):
    """Every key when K <= 64.  Otherwise key 0 and key K - 1, the keys on either side of a wave
    boundary (the keys of rows 64 j - 1 and 64 j: with P % 64 != 0 a wave straddles them) for the
    first 8, the last 8 and 8 seeded random boundaries, and 16 seeded random keys: at most
    MAX_ORACLE_KEYS."""
    if K <= 64:
        return np.arange(K)
    nwaves = (K * P + 63) // 64
    js = np.unique(np.concatenate([np.arange(1, min(9, nwaves)), np.arange(max(1, nwaves - 8), nwaves),
                                   rng.integers(1, nwaves, size=8)]))
    edge = np.concatenate([(64 * js - 1) // P, (64 * js) // P])
    keys = np.unique(np.concatenate([[0, K - 1], edge, rng.integers(0, K, size=16)]))
    assert keys.size <= MAX_ORACLE_KEYS and keys.max() < K
    return keys


def sample_rows(P, rng):
    """Every row of a key of up to MAX_ORACLE_ROWS points; else the first and last 48 (the planted
    points) and 32 seeded random rows."""
    if P <= MAX_ORACLE_ROWS:
        return np.arange(P)
    return np.unique(np.concatenate([np.arange(48), np.arange(P - 48, P), rng.integers(48, P - 48, size=32)]))


def want_reconstruction(xs, alpha, beta, P, bound):
    """beta[k] * [x < alpha[k]] (bound 0) / [x > alpha[k]] (bound 1) for every row, big-endian."""
    A = np.repeat(alpha, P, axis=0)
    diff = xs != A
    has = diff.any(1)
    first = diff.argmax(1)
    r = np.arange(xs.shape[0])
    lt = has & (xs[r, first] < A[r, first])
    on = lt if bound == 0 else has & ~lt
    return np.where(on[:, None], np.repeat(beta, P, axis=0), 0).astype(np.uint8)


@dataclass
class Expect:
    """What a case's outputs are compared with; the oracle's rows are computed once."""
    case: Case
    xs: np.ndarray
    keys: np.ndarray   # sampled keys
    rows: np.ndarray   # sampled rows of each sampled key
    want: dict         # (party, key) -> (len(rows), lam) oracle outputs
    rec: np.ndarray    # (K * P, lam) expected y0 ^ y1

    def check_oracle(self, ys):
        P = self.case.P
        for b in (0, 1):
            for k in self.keys:
                got = ys[b][k * P + self.rows]
                bad = np.flatnonzero((got != self.want[b, int(k)]).any(axis=1))
                assert bad.size == 0, (self.case.id, "oracle", "party", b, "key", int(k), "rows", self.rows[bad[:8]])

    def check_reconstruction(self, ys):
        bad = np.flatnonzero(((ys[0] ^ ys[1]) != self.rec).any(axis=1))
        assert bad.size == 0, (self.case.id, "reconstruction", "first rows", bad[:8], "of keys", bad[:8] // self.case.P)

    def check(self, ys):
        self.check_reconstruction(ys)
        self.check_oracle(ys)


def _assert_plan(prg, case, dcf):
    plan = prg.eval_plan(case.nb, case.K, case.P)
    what = (case.id, plan)
    assert plan.unsupported is None, what
    if case.engine is not None:
        assert plan.engine == dcf.Engine[case.engine], what
    assert plan.key_mode == (0 if case.K == 1 else key_mode_of(case.P)), what
    assert plan.prefix_levels == prg.eval_prefix_levels(case.nb, case.K, case.P), what
    if case.small is not None:
        assert plan.small == case.small, what
    if case.depth is not None:
        assert plan.prefix_levels == case.depth, what
    return plan


def run_case(dcf, case, seed=None):
    """Gen, both parties' eval and every check of the module docstring.  Returns (Expect, [y0, y1])
    with the outputs on the host.  A case with engine None (the fuzz list of tests/test_gpu_fuzz.py)
    takes whatever route its shape has: where the plan calls its engine setting unsupported, the
    case runs in automatic mode instead."""
    import torch
    prg = new_prg(dcf, case)
    case = resolve(dcf, case, prg)
    nb, lam, K, P = case.nb, case.lam, case.K, case.P
    if case.engine is None and prg.eval_plan(nb, K, P).unsupported:
        prg.set_eval_mode(0)
    plan = _assert_plan(prg, case, dcf)
    print(f"{case.id}: N={nb} LAMBDA={lam} K={K} P={P} -> {plan.engine.name} key_mode={plan.key_mode} "
          f"small={plan.small} prefix_levels={plan.prefix_levels}")
    rng = np.random.default_rng([0xD15BA7C4, CASE_IDS.index(case.id)] if seed is None else seed)
    r = lambda *s: rng.integers(0, 256, size=s, dtype=np.uint8)  # noqa: E731
    alpha, beta, s0, s1 = r(K, nb), r(K, lam), r(K, lam), r(K, lam)
    xs = make_points(nb, alpha, P, rng)
    T = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    d = dcf.DcfImpl(nb, lam, prg)
    cwb = d.gen_batch_device(T(alpha), T(beta), T(s0), T(s1), dcf.BoundState(case.bound))
    if case.trees is not None:
        prg.set_phase_timing(True)  # dcf_prg_last_eval_phases then reports the top trees' depth
    xd, ys = T(xs), []
    for b, s in ((0, s0), (1, s1)):
        buf = torch.full((K * P + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
        d.eval_multikey_device(bool(b), cwb, T(s), xd, P, ys=buf[PAD:PAD + K * P])
        torch.cuda.synchronize()
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + K * P:] == SENTINEL).all()), \
            (case.id, "neighbours of ys written", "party", b)
        if case.trees is not None:
            assert prg.last_eval_phases()[2] == case.trees, (case.id, "top trees", prg.last_eval_phases())
        ys.append(buf[PAD:PAD + K * P].cpu().numpy())
        del buf
    keys, rows = sample_keys(K, P, rng), sample_rows(P, rng)
    Po, n = oracle_prg(case.kind, lam), 8 * nb
    c = cwb.cpu().numpy()
    off = dcf.cwb_np1_offset(nb, lam, K)
    cw_s = c[:n * K * lam].reshape(n, K, lam)
    cw_v = c[n * K * lam:2 * n * K * lam].reshape(n, K, lam)
    cw_t = c[2 * n * K * lam:2 * n * K * lam + n * K].reshape(n, K)
    np1 = c[off:off + K * lam].reshape(K, lam)
    want = {}
    for k in map(int, keys):
        ok = O.gen(Po, alpha[k].tobytes(), beta[k].tobytes(), s0[k].tobytes(), s1[k].tobytes(), case.bound)
        assert (np.array_equal(cw_s[:, k], np.asarray(ok.cw_s).reshape(n, lam)) and
                np.array_equal(cw_v[:, k], np.asarray(ok.cw_v).reshape(n, lam)) and
                np.array_equal(cw_t[:, k], np.asarray(ok.cw_t).reshape(n)) and
                np.array_equal(np1[k], np.asarray(ok.cw_np1).reshape(lam))), (case.id, "gen differs from the oracle", "key", k)
        pts = np.ascontiguousarray(xs[k * P + rows])
        for b, s in ((0, s0), (1, s1)):
            want[b, k] = O.eval_(Po, b, ok, s[k].tobytes(), pts, nthreads=8)
    exp = Expect(case, xs, keys, rows, want, want_reconstruction(xs, alpha, beta, P, case.bound))
    exp.check(ys)
    return exp, ys


CASE_IDS = [c.id for c in CASES]


# ---- the runner's own test comes first ----

def test_runner_rejects_a_one_byte_corruption(dcf):
    """A correct result of K = 130 keys of 33 points (more keys than are sampled): one byte flipped
    in a sampled row fails the oracle comparison; one byte flipped in a row of an unsampled key
    passes it (nothing looks there) and fails the all-rows reconstruction."""
    case = next(c for c in CASES if c.id == "trees-P32-K130")
    exp, ys = run_case(dcf, replace(case, P=33, trees=None))
    K, P, lam = case.K, 33, case.lam
    unsampled = np.setdiff1d(np.arange(K), exp.keys)
    assert unsampled.size > 0 and exp.keys.size > 2
    exp.check(ys)

    def corrupted(party, row, byte):
        out = [y.copy() for y in ys]
        out[party][row, byte] ^= 0x10
        return out

    k = int(exp.keys[exp.keys.size // 2])
    bad = corrupted(1, k * P + int(exp.rows[-1]), lam - 1)
    with pytest.raises(AssertionError, match="oracle"):
        exp.check_oracle(bad)
    u = int(unsampled[unsampled.size // 2])
    bad = corrupted(0, u * P + 17, 3)
    exp.check_oracle(bad)
    with pytest.raises(AssertionError, match="reconstruction"):
        exp.check_reconstruction(bad)
    with pytest.raises(AssertionError):
        exp.check(bad)


def test_points_hold_alpha_its_neighbours_and_the_patterns():
    """make_points (host only): with room, every key's first rows are alpha, alpha +- 1, the
    patterns, and its last row is all-0xFF; without, K keys together still cover the list."""
    rng = np.random.default_rng(1)
    for nb in (1, 2, 16):
        pat = [np.frombuffer(x, np.uint8) for x in patterned(nb)]
        H = 3 + len(pat)
        alpha = rng.integers(0, 256, size=(7, nb), dtype=np.uint8)
        for P in (H, H + 1, 2 * H + 5):
            xs = make_points(nb, alpha, P, rng).reshape(7, P, nb)
            for k in range(7):
                assert np.array_equal(xs[k, 0], alpha[k]) and np.array_equal(xs[k, 1, :-1], alpha[k, :-1])
                assert xs[k, 1, -1] == (int(alpha[k, -1]) + 1) % 256 and xs[k, 2, -1] == (int(alpha[k, -1]) - 1) % 256
                assert all(np.array_equal(xs[k, 3 + i], p) for i, p in enumerate(pat))
                if P > H:
                    assert (xs[k, P - 1] == 0xFF).all()
        alphas = rng.integers(0, 256, size=(H, nb), dtype=np.uint8)
        xs = make_points(nb, alphas, 1, rng)
        assert np.array_equal(xs[0], alphas[0]) and (xs[3] == 0xFF).all() and (xs[4] == 0).all()
    assert set(sample_keys(64, 5, rng)) == set(range(64))
    ks = sample_keys(130, 33, rng)
    assert {0, 129, 63 // 33, 64 // 33}.issubset(ks) and ks.size < 130


# ---- the cases ----

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_multikey_route(dcf, case):
    run_case(dcf, case)


def _plans(dcf, a, b):
    pa, pb = new_prg(dcf, a), new_prg(dcf, b)
    a, b = resolve(dcf, a, pa), resolve(dcf, b, pb)
    return (a, pa.eval_plan(a.nb, a.K, a.P)), (b, pb.eval_plan(b.nb, b.K, b.P))


def _case(cid):
    return next(c for c in CASES if c.id == cid)


EDGES = [  # (case below, case above, the plan field that must differ)
    ("edge-pair-P64", "edge-stream-P64", "engine"), ("edge-pair-P33", "edge-stream-P33", "engine"),
    ("edge-pair-P64", "edge-stream-P64", "small"), ("edge-mmo-small", "edge-mmo-past-lt", "small"),
    ("edge-n32-stream", "edge-n33-ttable", "engine"),
    ("wide32-batch-P32768", "wide32-perkey-P32769", "engine"), ("wide48-batch-P32768", "wide48-perkey-P32769", "engine"),
    ("km-ttable-n2-P63", "km-ttable-n2-P64", "key_mode"), ("km-ttable-n2-P64", "km-ttable-n2-P65", "key_mode"),
    ("km-pair-n16-P127", "km-pair-n16-P128", "key_mode"), ("km-mmo-n2-P128", "km-mmo-n2-P193", "key_mode"),
]


@pytest.mark.parametrize("lo,hi,field", EDGES, ids=[f"{a}|{b}|{f}" for a, b, f in EDGES])
def test_every_edge_is_an_edge(dcf, lo, hi, field):
    """The two cases of a pair differ in the plan field the edge is about; a bisected pair sits on
    consecutive K (or N)."""
    (a, pa), (b, pb) = _plans(dcf, _case(lo), _case(hi))
    print(f"edge {field}: {a.id} (N={a.nb} K={a.K} P={a.P}) -> {pa} | {b.id} (N={b.nb} K={b.K} P={b.P}) -> {pb}")
    assert getattr(pa, field) != getattr(pb, field), (pa, pb)
    if isinstance(_case(lo).K, tuple) and isinstance(_case(hi).K, tuple) and a.nb == b.nb:
        assert b.K == a.K + 1


def test_unsupported_plans_launch_nothing(dcf):
    """Forced DCF_EVAL_STREAM with K = 2 at N = 33: dcf_eval_plan and the eval call both return
    DCF_ERR_UNSUPPORTED with the plan's text, and ys keeps its sentinels.  N = 32 is supported.
    The other two reasons (2^31 points per key on the stream engine, more than 2^32 64-point units
    on the T-table engine) through dcf_eval_plan alone: no buffers."""
    import torch
    lib = dcf.load()
    case = Case("unsupported", nb=33, K=2, P=64, mode=4, engine="STREAM")
    prg = new_prg(dcf, case)
    plan = prg.eval_plan(33, 2, 64)
    assert plan.engine == dcf.Engine.STREAM and plan.unsupported == "multi-key stream eval: N <= 32", plan
    assert prg.eval_plan(32, 2, 64).unsupported is None
    assert lib.dcf_eval_plan(prg.handle, 33, 2, 64, None, None, None, None) == -7
    assert prg.eval_plan(33, 1, 128).unsupported is None  # one key: any N
    d = dcf.DcfImpl(33, 16, prg)
    buf = torch.full((128 + 2 * PAD, 16), SENTINEL, dtype=torch.uint8, device="cuda")
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")  # noqa: E731
    with pytest.raises(dcf.DcfError) as e:
        d.eval_multikey_device(False, z(dcf.cwb_bytes(33, 16, 2)), z(2, 16), z(128, 33), 64, ys=buf[PAD:PAD + 128])
    assert e.value.code == -7 and "multi-key stream eval: N <= 32" in str(e.value)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    plan = prg.eval_plan(2, 2, 1 << 31)
    assert plan.engine == dcf.Engine.STREAM and plan.unsupported == "multi-key stream eval: 2^31 points per key or more", plan
    assert prg.eval_plan(2, 2, (1 << 31) - 1).unsupported is None
    prg.set_eval_mode(1)
    plan = prg.eval_plan(2, 2, 1 << 37)
    assert plan.engine == dcf.Engine.TTABLE and plan.unsupported == "more than 2^32 64-point units", plan
    assert prg.eval_plan(2, 2, 1 << 36).unsupported is None
    # argument errors leave the outputs alone
    import ctypes
    e_ = ctypes.c_int(-5)
    assert lib.dcf_eval_plan(None, 2, 2, 64, ctypes.byref(e_), None, None, None) == -1 and e_.value == -5
    assert lib.dcf_eval_plan(prg.handle, 0, 2, 64, ctypes.byref(e_), None, None, None) == -4 and e_.value == -5


# ---- the coverage assertion comes last ----

def test_cases_cover_every_multikey_engine_and_key_mode(dcf):
    """The plans of CASES (recomputed: a prg per case, no kernel) name every engine a call with
    K > 1 can reach, and each engine whose kernel is instantiated per key mode under modes 1 and 2."""
    seen = {}
    for case in CASES:
        prg = new_prg(dcf, case)
        c = resolve(dcf, case, prg)
        assert c.K > 1
        plan = prg.eval_plan(c.nb, c.K, c.P)
        seen.setdefault(plan.engine.name, set()).add(plan.key_mode)
    print("engines and key modes reached:", {e: sorted(m) for e, m in sorted(seen.items())})
    assert set(seen) == MULTIKEY_ENGINES, seen
    for e in KEY_MODE_ENGINES:
        assert seen[e] == {1, 2}, (e, seen[e])
