"""dcf_gen_batch_device and dcf_gen on both sides of every branch plan_gen takes.

Every case names the route it was written for (dcf_gen_route, the work-counter flag, the launch
count); the runner asks dcf_gen_plan first and asserts that route, so a case cannot drift onto
another kernel unseen.  The boundaries that depend on the device (quad against lane at
K = CUs * 512, the work counter from CUs * 2048 lanes) are found by bisection on dcf_gen_plan, never
from constants, and test_every_edge_is_an_edge asserts that the plan differs across each edge.

The runner (run_case) gens K keys into a 16-byte-aligned slice of a sentinel-filled buffer, with PAD
sentinel bytes on both sides, synchronises once and checks
  - both guards, and the padding bytes between cw_t and cw_np1 (the device entry point writes the
    four parts of the key block and nothing else);
  - that alpha, beta, s0_0 and s0_1 are unchanged;
  - cw_s, cw_v, cw_t and cw_np1 bit for bit against the CPU oracle's gen: every key when
    K <= ALL_KEYS_MAX, else the keys of sample_keys (at most MAX_ORACLE_KEYS);
  - when K > ALL_KEYS_MAX: all four parts of EVERY key against a gen of the same inputs in
    consecutive slices of SLICE keys (4096 on the WIDE route: one launch with key_base = 0), whose
    sampled keys are compared with the oracle too;
  - two-party reconstruction on EVERY key: eval_multikey_device of both parties at alpha, alpha - 1,
    alpha + 1 (big-endian, clamped at the ends of the domain) and a random point must give
    y0 ^ y1 == beta[k] * [x < alpha[k]] (GtBeta: >).
Inputs (make_inputs): seeded random, the first keys overwritten with the edge patterns of
edge_inputs (alpha all-0x00, all-0xFF, 0xAA.., 0x55.., 0x80 00.., 00..01 and
tests/test_stream_update_emulation.py's patterned alphas; beta all-zero and all-0xFF; one key with
s0_0 == s0_1); a case with fewer keys than patterns takes them round robin from an offset of its own.
"""
import ctypes
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_multikey_dispatch_gpu import oracle_prg, want_reconstruction, _aes_keys
from tests.test_range_gpu import PAD, SENTINEL
from tests.test_stream_update_emulation import patterned

pytestmark = pytest.mark.gpu

ALL_KEYS_MAX = 4200     # cases of up to this many keys compare every key with the oracle
MAX_ORACLE_KEYS = 2048  # sampled keys of a larger case, at most (the oracle's gen: 32-52 us per key)
SLICE = 2048            # keys per slice of the second gen of a larger case (Hirose LAMBDA = 16, N <= 32: the row route)
WIDE_LAUNCH = 4096      # keys per launch of the WIDE route (include/dcf_hip.h, dcf_gen_plan)
P_EVAL = 4              # points per key of the reconstruction check


@dataclass(frozen=True)
class Case:
    """One gen shape and the route it is written for.  K may be a (tag, d) pair resolved on the
    device (resolve): "Eq" the largest K on the quad route, "Ec" the smallest K on the lane route
    with the work counter, "grid" CUs * 1024 (one key per lane of a full grid), each plus d."""
    id: str
    kind: str = "hirose"
    lam: int = 16
    nb: int = 1
    K: object = 1
    bound: int = 0
    route: str = "ROW"     # dcf_amd.GenRoute member the plan must name
    counter: bool = False  # the plan's work-counter flag
    launches: int = 1      # the plan's launch count


def _row_col_cases():
    """Hirose LAMBDA = 16: one wave per key up to 2048 keys, 16 lanes per key up to 16384, on both
    sides of 16 keys (a workgroup of waves) and 64 keys (a workgroup of 16-lane groups); N = 5 makes
    the last chunk of alpha partial; N = 33 (8N > 256) leaves the latency kernels for the quad route."""
    out = []
    for nb in (1, 32, 5):
        for i, K in enumerate((1, 15, 16, 17, 63, 64, 65, 2047, 2048)):
            out.append(Case(f"row-n{nb}-K{K}", nb=nb, K=K, bound=(i + nb) % 2, route="ROW"))
        for i, K in enumerate((2049, 16383, 16384)):
            out.append(Case(f"col-n{nb}-K{K}", nb=nb, K=K, bound=(i + nb) % 2, route="COL"))
    out += [Case("quad-n33-K1", nb=33, K=1, bound=1, route="QUAD"),
            Case("quad-n33-K70", nb=33, K=70, bound=0, route="QUAD")]
    return out


def _quad_lane_cases():
    """k_gen16<4> and k_gen16<1>: past the column kernel at N = 1, 3, 7 (alpha's last chunk
    partial); a last partial wave (16 keys per wave) at N = 40; the one K at which the quad route
    takes the work counter; the first K on the lane route; one lane past a full grid without the
    counter (the grid-stride loop's second trip); both sides of the lane route's counter threshold,
    the upper one with a partial final unit."""
    out = [Case(f"quad-n{nb}-K16385", nb=nb, K=16385, bound=i % 2, route="QUAD") for i, nb in enumerate((1, 3, 7))]
    out += [Case(f"quad-n40-K{K}", nb=40, K=K, bound=i % 2, route="QUAD") for i, K in enumerate((15, 16, 17, 33))]
    out += [Case("quad-counter-Eq", K=("Eq", 0), bound=1, route="QUAD", counter=True),
            Case("lane-n1-Eq+1", K=("Eq", 1), bound=0, route="LANE"),
            Case("lane-n5-Eq+1", nb=5, K=("Eq", 1), bound=1, route="LANE"),
            Case("lane-stride-grid+1", K=("grid", 1), bound=0, route="LANE"),
            Case("lane-Ec-1", K=("Ec", -1), bound=1, route="LANE"),
            Case("lane-counter-Ec+63", K=("Ec", 63), bound=0, route="LANE", counter=True)]
    return out


def _mmo16_cases():
    """k_gen16_mmo: around a wave of keys and past a workgroup of them, at N = 1, 5 and 16; one key
    past a full grid (a workgroup's second trip)."""
    out = []
    for nb in (1, 5, 16):
        for i, K in enumerate((1, 63, 64, 65, 1025)):
            out.append(Case(f"mmo16-n{nb}-K{K}", kind="mmo", nb=nb, K=K, bound=(i + nb) % 2, route="MMO16"))
    out.append(Case("mmo16-grid+1", kind="mmo", K=("grid", 1), bound=1, route="MMO16"))
    return out


def _wide_cases():
    """k_gen_wide: one, two and three launches of 4096 keys (key_base 0, 4096, 8192; scratch rows by
    blockIdx.x); three 16-byte pieces; one piece per thread and thread 0's second trip; N = 33."""
    out = [Case(f"wide32-K{K}", lam=32, K=K, bound=i % 2, route="WIDE", launches=n)
           for i, (K, n) in enumerate(((1, 1), (4095, 1), (4096, 1), (4097, 2), (8193, 3)))]
    out += [Case("wide48-K4097", lam=48, K=4097, bound=1, route="WIDE", launches=2),
            Case("wide16384-K3", lam=16384, K=3, bound=0, route="WIDE"),
            Case("wide16400-K2", lam=16400, K=2, bound=1, route="WIDE"),
            Case("wide64-n33-K5", lam=64, nb=33, K=5, bound=0, route="WIDE")]
    return out


def _mmo_wide_cases():
    """k_mmo_wide_gen head and tail: around a group of 64 keys; three blocks; the second trip of
    both grids (more than 16 * CUs groups for the head, more than 64 * CUs items for the tail).
    That last case takes about 25 s on a 256-CU part, nearly all of it in the reconstruction check:
    multi-key eval with the MMO PRG at LAMBDA >= 32 runs key by key (WIDE_PER_KEY), four launches
    per key over CUs * 1024 + 1 keys; its gen, guards, oracle sample and sliced gen take under 1 s."""
    out = [Case(f"mmowide32-K{K}", kind="mmo", lam=32, K=K, bound=i % 2, route="MMO_WIDE", launches=2)
           for i, K in enumerate((1, 63, 64, 65))]
    out += [Case("mmowide48-K130", kind="mmo", lam=48, K=130, bound=1, route="MMO_WIDE", launches=2),
            Case("mmowide80-grid+1", kind="mmo", lam=80, K=("grid", 1), bound=0, route="MMO_WIDE", launches=2)]
    return out


CASES = _row_col_cases() + _quad_lane_cases() + _mmo16_cases() + _wide_cases() + _mmo_wide_cases()
CASE_IDS = [c.id for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


def new_prg(dcf, kind, lam):
    keys = list(_aes_keys(kind, lam))
    return (dcf.Aes128MatyasMeyerOseasPrg if kind == "mmo" else dcf.Aes256HirosePrg)(keys, lam)


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bisect(pred, lo, hi):
    """The smallest K in (lo, hi] with pred(K), given not pred(lo) and pred(hi)."""
    assert not pred(lo) and pred(hi), ("no edge between", lo, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


@lru_cache(maxsize=None)
def _edges(dcf):
    """(E_q, E_c) of the module docstring, by bisection on dcf_gen_plan at N = 1."""
    prg = new_prg(dcf, "hirose", 16)
    col_max = _bisect(lambda K: prg.gen_plan(1, K).route != dcf.GenRoute.COL, 2049, 1 << 20) - 1
    first_lane = _bisect(lambda K: prg.gen_plan(1, K).route == dcf.GenRoute.LANE, col_max + 1, 1 << 28)
    e_c = _bisect(lambda K: prg.gen_plan(1, K).counter, first_lane, 1 << 30)
    return first_lane - 1, e_c


def resolve(dcf, case):
    """The case's K as a number."""
    if isinstance(case.K, tuple):
        tag, d = case.K
        e_q, e_c = _edges(dcf)
        return {"Eq": e_q, "Ec": e_c, "grid": 1024 * cus()}[tag] + d
    return case.K


# ---- inputs, samples (host only) ----

def edge_inputs(nb, lam):
    """The edge patterns as (field, row) entries: field "alpha" / "beta" with the bytes of that row,
    or ("same", None): s0_1 takes s0_0's bytes."""
    alphas = [bytes(nb), b"\xff" * nb, b"\xaa" * nb, b"\x55" * nb, b"\x80" + bytes(nb - 1), bytes(nb - 1) + b"\x01"]
    alphas += [bytes(x) for x in patterned(nb)]
    out = [("alpha", np.frombuffer(a, np.uint8)) for a in alphas]
    out += [("beta", np.zeros(lam, np.uint8)), ("beta", np.full(lam, 0xFF, np.uint8)), ("same", None)]
    return out


def make_inputs(case, K, rng):
    """alpha (K, N), beta, s0_0, s0_1 (K, LAMBDA) and the keys that took an edge pattern."""
    nb, lam = case.nb, case.lam
    r = lambda *s: rng.integers(0, 256, size=s, dtype=np.uint8)  # noqa: E731
    alpha, beta, s0, s1 = r(K, nb), r(K, lam), r(K, lam), r(K, lam)
    edges = edge_inputs(nb, lam)
    off = CASE_IDS.index(case.id) if case.id in CASE_IDS else 0
    planted = np.arange(min(K, len(edges)))
    for k in planted:
        field, row = edges[(off + k) % len(edges)] if K < len(edges) else edges[k]
        if field == "alpha":
            alpha[k] = row
        elif field == "beta":
            beta[k] = row
        else:
            s1[k] = s0[k]
    return alpha, beta, s0, s1, planted


def keys_per_workgroup(route, K, ncus):
    """Keys a workgroup of the route holds (one trip): the latency kernels spread a small batch over
    the CUs, at most 16 waves / 64 lane groups per workgroup; a 1024-lane workgroup of quads, of
    lanes, of the MMO kernels (16 groups of 64 keys in the wide head); one key on WIDE."""
    per = -(-K // ncus)
    return {"ROW": max(1, min(16, per)), "COL": max(1, min(64, per)), "QUAD": 256, "LANE": 1024, "MMO16": 1024,
            "WIDE": 1, "MMO_WIDE": 1024}[route]


def sample_keys(route, K, planted, ncus, rng):
    """Every key up to ALL_KEYS_MAX.  Otherwise at most MAX_ORACLE_KEYS: the first and last 130
    keys, the planted keys, on the WIDE route the keys around every launch boundary
    (k % 4096 in {4094, 4095, 0, 1}), the keys either side of every multiple of the route's
    per-workgroup key count (evenly thinned if they alone would pass half the cap), the rest random."""
    if K <= ALL_KEYS_MAX:
        return np.arange(K)
    must = [np.arange(130), np.arange(K - 130, K), planted]
    if route == "WIDE":
        b = np.arange(WIDE_LAUNCH, K + 2, WIDE_LAUNCH)
        must.append(np.concatenate([b - 2, b - 1, b, b + 1]))
    else:
        m = np.arange(1, (K - 1) // keys_per_workgroup(route, K, ncus) + 1) * keys_per_workgroup(route, K, ncus)
        if 2 * m.size > MAX_ORACLE_KEYS // 2:
            m = m[np.linspace(0, m.size - 1, MAX_ORACLE_KEYS // 4).astype(np.int64)]
        must.append(np.concatenate([m - 1, m]))
    keys = np.unique(np.concatenate(must))
    keys = keys[(keys >= 0) & (keys < K)]
    assert keys.size <= MAX_ORACLE_KEYS
    fill = rng.integers(0, K, size=MAX_ORACLE_KEYS - keys.size)
    return np.unique(np.concatenate([keys, fill]))


def neighbours(alpha, d):
    """alpha + d (d = +-1) as N-byte big-endian integers, clamped at the ends of the domain."""
    out = alpha.astype(np.int16)
    carry = np.full(alpha.shape[0], d, np.int16)
    for j in reversed(range(alpha.shape[1])):
        v = out[:, j] + carry
        out[:, j] = v & 0xFF
        carry = np.where(v > 255, 1, np.where(v < 0, -1, 0)).astype(np.int16)
    out = out.astype(np.uint8)
    out[carry != 0] = alpha[carry != 0]
    return out


def make_points(alpha, rng):
    """(K * P_EVAL, N): per key alpha, alpha - 1, alpha + 1 and a random point."""
    K, nb = alpha.shape
    xs = np.empty((K, P_EVAL, nb), np.uint8)
    xs[:, 0], xs[:, 1], xs[:, 2] = alpha, neighbours(alpha, -1), neighbours(alpha, +1)
    xs[:, 3] = rng.integers(0, 256, size=(K, nb), dtype=np.uint8)
    return xs.reshape(K * P_EVAL, nb)


# ---- the key block's four parts ----

def cwb_parts(dcf, cwb, nb, lam, K):
    """Views (cw_s (8N, K, LAMBDA), cw_v, cw_t (8N, K), cw_np1 (K, LAMBDA), padding) of a K-key CWB
    (a flat torch tensor or numpy array)."""
    n = 8 * nb
    a, b, off = n * K * lam, 2 * n * K * lam + n * K, dcf.cwb_np1_offset(nb, lam, K)
    assert cwb.shape == (dcf.cwb_bytes(nb, lam, K),) and b <= off < b + 16 and off % 16 == 0
    return (cwb[:a].reshape(n, K, lam), cwb[a:2 * a].reshape(n, K, lam), cwb[2 * a:b].reshape(n, K),
            cwb[off:off + K * lam].reshape(K, lam), cwb[b:off])


PART_NAMES = ("cw_s", "cw_v", "cw_t", "cw_np1")


def assert_key_is_oracle(parts, k, ok, what=()):
    """All four parts of key column k of host-side `parts` (cwb_parts) equal the oracle key `ok`."""
    s, v, t, np1 = parts[:4]
    n, lam = s.shape[0], s.shape[2]
    for name, got, want in (("cw_s", s[:, k], np.asarray(ok.cw_s).reshape(n, lam)),
                            ("cw_v", v[:, k], np.asarray(ok.cw_v).reshape(n, lam)),
                            ("cw_t", t[:, k], np.asarray(ok.cw_t).reshape(n)),
                            ("cw_np1", np1[k], np.asarray(ok.cw_np1).reshape(lam))):
        assert np.array_equal(got, want), (*what, name, "differs from the oracle", "key", int(k))


def gather_keys(parts, keys):
    """The columns `keys` of device-side parts, on the host (same shapes with K = len(keys))."""
    import torch
    idx = torch.as_tensor(np.asarray(keys), device=parts[0].device)
    s, v, t, np1 = parts[:4]
    return tuple(x.cpu().numpy() for x in (s[:, idx], v[:, idx], t[:, idx], np1[idx]))


def guarded_gen(dcf, d, K, dev_in, bound):
    """gen_batch_device into a 16-byte-aligned slice of a SENTINEL-filled buffer with PAD bytes on
    either side.  Returns (whole buffer, the CWB slice)."""
    import torch
    size = dcf.cwb_bytes(d.n_bytes, d.lam, K)
    buf = torch.full((size + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[PAD:PAD + size]
    assert out.data_ptr() % 16 == 0
    d.gen_batch_device(*dev_in, dcf.BoundState(bound), cwb_out=out)
    return buf, out


def check_guards(case_id, buf, parts):
    size = buf.numel() - 2 * PAD
    assert bool((buf[:PAD] == SENTINEL).all()), (case_id, "bytes before cwb_out written")
    assert bool((buf[PAD + size:] == SENTINEL).all()), (case_id, "bytes after cwb_out written")
    assert bool((parts[4] == SENTINEL).all()), (case_id, "padding between cw_t and cw_np1 written")


def check_oracle(case, Po, host_in, parts_h, keys, cols, what):
    """Keys `keys` (columns `cols` of the host-side parts) against the oracle's gen."""
    alpha, beta, s0, s1 = host_in
    for k, c in zip(map(int, keys), cols):
        ok = O.gen(Po, alpha[k].tobytes(), beta[k].tobytes(), s0[k].tobytes(), s1[k].tobytes(), case.bound)
        assert_key_is_oracle(parts_h, c, ok, (case.id, what, "key", k))


def check_slices(dcf, d, case, K, dev_in, parts, step):
    """Gen the same inputs in consecutive slices of `step` keys and compare all four parts of every
    key of the big call with its slice.  Returns the slices' parts assembled as one K-key set."""
    import torch
    n, lam = 8 * d.n_bytes, d.lam
    s2 = torch.empty((n, K, lam), dtype=torch.uint8, device="cuda")
    v2, t2, p2 = torch.empty_like(s2), torch.empty((n, K), dtype=torch.uint8, device="cuda"), \
        torch.empty((K, lam), dtype=torch.uint8, device="cuda")
    for k0 in range(0, K, step):
        k1 = min(K, k0 + step)
        buf, out = guarded_gen(dcf, d, k1 - k0, [x[k0:k1] for x in dev_in], case.bound)
        sl = cwb_parts(dcf, out, d.n_bytes, lam, k1 - k0)
        s2[:, k0:k1], v2[:, k0:k1], t2[:, k0:k1], p2[k0:k1] = sl[:4]
        if k0 == 0 or k1 == K:
            torch.cuda.synchronize()
            check_guards(case.id + f" slice at {k0}", buf, sl)
    torch.cuda.synchronize()
    for name, big, small in zip(PART_NAMES, parts, (s2, v2, t2, p2)):
        if not torch.equal(big, small):
            ne = big != small  # per key: cw_s / cw_v (8N, K, LAMBDA), cw_t (8N, K), cw_np1 (K, LAMBDA)
            per_key = {"cw_s": lambda: ne.any(2).any(0), "cw_v": lambda: ne.any(2).any(0), "cw_t": lambda: ne.any(0),
                       "cw_np1": lambda: ne.any(1)}[name]()
            bad = torch.nonzero(per_key).flatten()[:8].tolist()
            raise AssertionError((case.id, name, "differs from the sliced gen", "first keys", bad))
    return s2, v2, t2, p2


def check_reconstruction(dcf, d, case, K, host_in, dev_in, cwb, rng):
    """Both parties' eval_multikey_device over P_EVAL points per key: y0 ^ y1 on every row."""
    import torch
    alpha, beta = host_in[0], host_in[1]
    xs = make_points(alpha, rng)
    xd = torch.from_numpy(xs).cuda()
    y0 = d.eval_multikey_device(False, cwb, dev_in[2], xd, P_EVAL)
    y1 = d.eval_multikey_device(True, cwb, dev_in[3], xd, P_EVAL)
    torch.cuda.synchronize()
    rec = (y0 ^ y1).cpu().numpy()
    bad = np.flatnonzero((rec != want_reconstruction(xs, alpha, beta, P_EVAL, case.bound)).any(axis=1))
    assert bad.size == 0, (case.id, "reconstruction", "first rows", bad[:8], "of keys", bad[:8] // P_EVAL)


def assert_plan(dcf, prg, case, K):
    plan = prg.gen_plan(case.nb, K)
    what = (case.id, K, plan)
    assert plan.route == dcf.GenRoute[case.route], what
    assert plan.counter == case.counter, what
    assert plan.launches == case.launches, what
    return plan


def run_case(dcf, case):
    import torch
    prg = new_prg(dcf, case.kind, case.lam)
    K = resolve(dcf, case)
    nb, lam = case.nb, case.lam
    plan = assert_plan(dcf, prg, case, K)
    print(f"{case.id}: N={nb} LAMBDA={lam} K={K} bound={case.bound} -> {plan}")
    rng = np.random.default_rng([0x6E17, CASE_IDS.index(case.id)])
    *host_in, planted = make_inputs(case, K, rng)
    dev_in = [torch.from_numpy(a).cuda() for a in host_in]
    d = dcf.DcfImpl(nb, lam, prg)
    buf, cwb = guarded_gen(dcf, d, K, dev_in, case.bound)
    torch.cuda.synchronize()
    parts = cwb_parts(dcf, cwb, nb, lam, K)
    check_guards(case.id, buf, parts)
    for name, h, t in zip(("alpha", "beta", "s0_0", "s0_1"), host_in, dev_in):
        assert np.array_equal(t.cpu().numpy(), h), (case.id, name, "changed by gen")
    keys = sample_keys(case.route, K, planted, cus(), rng)
    Po = oracle_prg(case.kind, lam)
    check_oracle(case, Po, host_in, gather_keys(parts, keys), keys, range(keys.size), "gen")
    if K > ALL_KEYS_MAX:
        sliced = check_slices(dcf, d, case, K, dev_in, parts, WIDE_LAUNCH if case.route == "WIDE" else SLICE)
        check_oracle(case, Po, host_in, gather_keys(sliced, keys), keys, range(keys.size), "sliced gen")
        del sliced
    check_reconstruction(dcf, d, case, K, host_in, dev_in, cwb, rng)


# ---- host-only tests of the runner's helpers ----

def test_inputs_and_samples():
    """make_inputs plants every edge pattern when K allows and a rotating part of them otherwise;
    neighbours clamps; sample_keys holds the keys the module docstring lists."""
    rng = np.random.default_rng(3)
    case = Case("x", nb=5, lam=16)
    edges = edge_inputs(5, 16)
    alpha, beta, s0, s1, planted = make_inputs(case, 100, rng)
    assert planted.size == len(edges) and not alpha[0].any() and (alpha[1] == 0xFF).all()
    assert alpha[4].tolist() == [0x80, 0, 0, 0, 0] and alpha[5].tolist() == [0, 0, 0, 0, 1]
    na = sum(f == "alpha" for f, _ in edges)
    assert not beta[na].any() and (beta[na + 1] == 0xFF).all() and np.array_equal(s0[na + 2], s1[na + 2])
    assert not np.array_equal(s0[na + 1], s1[na + 1])
    a = np.array([[0, 0], [0xFF, 0xFF], [0x12, 0xFF], [0x13, 0x00]], np.uint8)
    assert neighbours(a, +1).tolist() == [[0, 1], [0xFF, 0xFF], [0x13, 0x00], [0x13, 0x01]]
    assert neighbours(a, -1).tolist() == [[0, 0], [0xFF, 0xFE], [0x12, 0xFE], [0x12, 0xFF]]
    assert sample_keys("ROW", 4200, planted, 256, rng).size == 4200
    ks = set(sample_keys("WIDE", 8193, planted, 256, rng).tolist())
    assert {0, 129, 8063, 8192, 4094, 4095, 4096, 4097, 8190, 8191}.issubset(ks) and len(ks) <= MAX_ORACLE_KEYS
    ks = set(sample_keys("LANE", 262145, planted, 256, rng).tolist())
    assert all({1024 * j - 1, 1024 * j}.issubset(ks) for j in range(1, 257)) and len(ks) <= MAX_ORACLE_KEYS
    ks = set(sample_keys("QUAD", 131072, planted, 256, rng).tolist())
    assert {255, 256, 131071 - 256, 131072 - 256}.issubset(ks) and len(ks) <= MAX_ORACLE_KEYS


# ---- the cases ----

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gen_route(dcf, case):
    run_case(dcf, case)


def _case(cid):
    return next(c for c in CASES if c.id == cid)


EDGES = [  # (case below, case above, the plan field that must differ, consecutive K)
    ("row-n1-K2048", "col-n1-K2049", "route", True), ("row-n32-K2048", "col-n32-K2049", "route", True),
    ("col-n1-K16384", "quad-n1-K16385", "route", True), ("col-n5-K16384", "quad-n3-K16385", "route", False),
    ("row-n32-K1", "quad-n33-K1", "route", False), ("row-n32-K1", "quad-n33-K1", "host_tiny", False),
    ("row-n32-K65", "quad-n33-K70", "route", False),
    ("quad-counter-Eq", "lane-n1-Eq+1", "route", True), ("quad-counter-Eq", "lane-n1-Eq+1", "counter", True),
    ("quad-n1-K16385", "quad-counter-Eq", "counter", False),
    ("lane-Ec-1", "lane-counter-Ec+63", "counter", False),
    ("wide32-K4096", "wide32-K4097", "launches", True), ("wide32-K4097", "wide32-K8193", "launches", False),
    ("mmo16-n1-K1", "mmowide32-K1", "route", False), ("row-n1-K1", "wide32-K1", "route", False),
    ("row-n1-K1", "mmo16-n1-K1", "route", False),
]


@pytest.mark.parametrize("lo,hi,field,adjacent", EDGES, ids=[f"{a}|{b}|{f}" for a, b, f, _ in EDGES])
def test_every_edge_is_an_edge(dcf, lo, hi, field, adjacent):
    """The two cases of a pair differ in the plan field the edge is about; the bisected edges sit on
    consecutive K: quad | lane at E_q | E_q + 1, and the lane route's counter at E_c - 1 | E_c."""
    a, b = _case(lo), _case(hi)
    Ka, Kb = resolve(dcf, a), resolve(dcf, b)
    pa = new_prg(dcf, a.kind, a.lam).gen_plan(a.nb, Ka)
    pb = new_prg(dcf, b.kind, b.lam).gen_plan(b.nb, Kb)
    print(f"edge {field}: {a.id} (N={a.nb} K={Ka}) -> {pa} | {b.id} (N={b.nb} K={Kb}) -> {pb}")
    assert getattr(pa, field) != getattr(pb, field), (pa, pb)
    if adjacent:
        assert Kb == Ka + 1
    if lo == "lane-Ec-1":
        prg = new_prg(dcf, "hirose", 16)
        assert not prg.gen_plan(1, Ka).counter and prg.gen_plan(1, Ka + 1).counter
        assert prg.gen_plan(1, Ka + 1).route == dcf.GenRoute.LANE


def test_device_edges_sit_where_the_header_says(dcf):
    """The bisected edges against include/dcf_hip.h's description: quad up to CUs * 512 keys, the
    counter from CUs * 2048 lanes; the quad route takes the counter at exactly one K."""
    e_q, e_c = _edges(dcf)
    n = cus()
    print(f"CUs={n} E_q={e_q} E_c={e_c}")
    assert e_q == 512 * n and e_c == 2048 * n
    prg = new_prg(dcf, "hirose", 16)
    assert not prg.gen_plan(1, e_q - 1).counter and prg.gen_plan(1, e_q).counter
    assert 1024 * n + 1 < e_c - 1  # the stride-loop case lies below the counter


def test_gen_plan_argument_errors(dcf):
    """null prg -> DCF_ERR_ARG, n_bytes == 0 -> DCF_ERR_N, outputs untouched; NULL outputs are fine."""
    lib = dcf.load()
    prg = new_prg(dcf, "hirose", 16)
    r = ctypes.c_int(-5)
    assert lib.dcf_gen_plan(None, 1, 1, ctypes.byref(r), None, None, None) == -1 and r.value == -5
    assert lib.dcf_gen_plan(prg.handle, 0, 1, ctypes.byref(r), None, None, None) == -4 and r.value == -5
    assert lib.dcf_gen_plan(prg.handle, 1, 1, None, None, None, None) == 0
    assert lib.dcf_gen_plan(prg.handle, 1, 1, ctypes.byref(r), None, None, None) == 0 and r.value == dcf.GenRoute.ROW


# ---- the host entry point ----

HOST_CASES = [("hirose", 16, 32, True, "ROW"), ("hirose", 16, 33, False, "QUAD"), ("mmo", 16, 4, False, "MMO16"),
              ("hirose", 64, 2, False, "WIDE"), ("mmo", 48, 2, False, "MMO_WIDE")]


@pytest.mark.parametrize("kind,lam,nb,tiny,route", HOST_CASES, ids=[f"{k}-lam{l}-n{n}" for k, l, n, _, _ in HOST_CASES])
def test_host_gen(dcf, kind, lam, nb, tiny, route):
    """dcf_gen through the mapped tiny buffer (Hirose LAMBDA = 16, N <= 32) and through the staged
    copies: all four parts against the oracle, the padding bytes 0, and the same bytes out of
    gen_batch_device with K = 1 (its padding aside, which that call leaves alone)."""
    import torch
    prg, Po = new_prg(dcf, kind, lam), oracle_prg(kind, lam)
    plan = prg.gen_plan(nb, 1)
    assert plan.host_tiny == tiny and plan.route == dcf.GenRoute[route], plan
    d = dcf.DcfImpl(nb, lam, prg)
    rng = np.random.default_rng([0x6057, lam, nb])
    lib = dcf.load()
    size = dcf.cwb_bytes(nb, lam, 1)
    for bound in (0, 1):
        a, b, s0, s1 = (rng.integers(0, 256, size=(1, w), dtype=np.uint8) for w in (nb, lam, lam, lam))
        out = np.full(size + 2 * PAD, SENTINEL, np.uint8)
        rc = lib.dcf_gen(prg.handle, nb, a.ctypes.data, b.ctypes.data, s0.ctypes.data, s1.ctypes.data, bound,
                         ctypes.c_void_p(out.ctypes.data + PAD))
        assert rc == 0
        assert (out[:PAD] == SENTINEL).all() and (out[PAD + size:] == SENTINEL).all()
        host = out[PAD:PAD + size]
        parts = cwb_parts(dcf, host, nb, lam, 1)
        ok = O.gen(Po, a.tobytes(), b.tobytes(), s0.tobytes(), s1.tobytes(), bound)
        assert_key_is_oracle(parts, 0, ok, (kind, lam, nb, "dcf_gen"))
        assert not parts[4].any(), "dcf_gen's padding bytes read 0"
        buf, dev = guarded_gen(dcf, d, 1, [torch.from_numpy(x).cuda() for x in (a, b, s0, s1)], bound)
        torch.cuda.synchronize()
        dparts = cwb_parts(dcf, dev, nb, lam, 1)
        check_guards((kind, lam, nb), buf, dparts)
        dh = dev.cpu().numpy()
        dh[2 * 8 * nb * lam + 8 * nb:dcf.cwb_np1_offset(nb, lam, 1)] = 0
        assert np.array_equal(dh, host), (kind, lam, nb, "gen_batch_device with K = 1 differs from dcf_gen")


# ---- the coverage assertion comes last ----

def test_cases_cover_every_route_and_counter_state(dcf):
    """The plans of CASES (recomputed, no kernel) name every gen route, the quad and lane routes
    with and without the work counter, and the WIDE route with 1, 2 and 3 launches."""
    seen = set()
    for case in CASES:
        plan = new_prg(dcf, case.kind, case.lam).gen_plan(case.nb, resolve(dcf, case))
        seen.add((plan.route.name, plan.counter, plan.launches))
    print(sorted(seen))
    assert {r for r, _, _ in seen} == {r.name for r in dcf.GenRoute}
    for r in ("QUAD", "LANE"):
        assert {(r, False, 1), (r, True, 1)} <= seen
    assert {("WIDE", False, n) for n in (1, 2, 3)} <= seen
