"""Sequences of calls on ONE long-lived dcf_prg, every output guarded.

A dcf_prg leases its workspaces from a LIFO pool, so a single caller gets the same workspace back
for every call, with the buffers of all earlier calls already grown and still holding their bytes:
the shared-prefix table / per-key top trees / MMO level rows in d_pfx, the LAMBDA >= 32, range and
MMO full-domain layouts in d_ws (full-domain eval lays out a range call's, but for its two own
paths), the work counter and block count in d_ctr, the grow-only digests, the staging buffers.  The other GPU tests build a fresh prg per case; these keep one and change the path, the
depth, the size and the stream from call to call, so state that leaks from call k into call k + 1
shows as wrong bytes, a written guard row or a wrong block count.

Every step draws a fresh key, runs one entry point with its output inside sentinel rows (device:
torch.full; host: numpy), compares with the CPU oracle bit for bit (all rows up to 4096, else
_sample's edges and random rows), checks y0 ^ y1 on all rows where both parties run and, where the
library documents one, the AES block count of the call.  The pool, the hand-written ladders and the
seeded generator are plain data (tests/test_call_sequences.py checks them without a GPU).

Longer one-off runs: DCF_SEQ_STEPS steps per sequence from DCF_SEQ_SEED (as DCF_FUZZ_* in
test_gpu_fuzz.py).  A failure names the configuration, the seed, the step index and the step."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_fuzz import _lt
from tests.test_range_gpu import PAD, SENTINEL, _cwb, _dev, _points, _sample, host_chunk
from tests.test_range_multikey_gpu import _cwbk, _nroots

pytestmark = pytest.mark.gpu

FLAT_PAD = 256  # sentinel bytes on either side of a flat CWB output (keeps the inner pointer 16-byte aligned)
CUS = 256       # compute units of an MI355X (dcf_prg::cus); the engine thresholds below depend on it
STREAM_MIN = CUS * 1024 * 2  # points from which auto mode runs the stream engine (524288)

# configuration -> (PRG, LAMBDA, the N a sequence draws from)
CONFIGS = {
    "hirose16": ("hirose", 16, (4, 16)),
    "mmo16": ("mmo", 16, (4, 16)),
    "hirose64": ("hirose", 64, (2, 5, 16, 40)),
    "hirose128": ("hirose", 128, (2, 5, 16, 40)),
    "hirose272": ("hirose", 272, (2, 5, 16, 40)),
    "mmo32": ("mmo", 32, (2, 5, 16, 40)),  # no tree path: range eval materialises the points
}

ALL_BUFFERS = frozenset({"d_pfx", "d_ws", "d_ctr", "d_dig", "d_kdig", "d_tctr", "stage"})
# step kind -> the workspace buffers a call of that kind may lay out ("stage": d_stage / h_stage /
# h_tiny / h_mid).  The ladders below are checked against this table (tests/test_call_sequences.py).
STEP_BUFFERS = {
    "host_eval": frozenset({"d_ctr", "d_pfx", "d_ws", "d_dig", "d_tctr", "stage"}),
    "eval_device": frozenset({"d_ctr", "d_pfx", "d_ws", "d_dig", "d_tctr"}),
    "eval_multikey": frozenset({"d_ctr", "d_pfx", "d_kdig", "d_ws", "d_dig", "d_tctr"}),
    "gen_batch": frozenset({"d_ws"}),
    # the fast path's table, the MMO levels' nodes, else a range call's
    "full_domain": frozenset({"d_ctr", "d_pfx", "d_ws", "d_dig", "d_tctr"}),
    "range_device": frozenset({"d_ctr", "d_ws", "d_dig", "d_tctr"}),
    "range_host": frozenset({"d_ctr", "d_ws", "d_dig", "d_tctr", "stage"}),
    "range_multikey": frozenset({"d_ctr", "d_ws"}),
    "host_gen": frozenset({"stage"}),
    "gen_many": frozenset({"stage"}),
    "set_prefix_levels": frozenset(),
    "set_eval_mode": frozenset(),
    "set_prefix_max_bytes": frozenset(),
    "trim": ALL_BUFFERS,  # frees them all
}
SETTINGS = ("set_prefix_levels", "set_eval_mode", "set_prefix_max_bytes", "trim")

# The shapes of the pool: both sides of every engine threshold of dcf_hip.hip (kEvalRow2Max 2048,
# kEvalRowMax 8192, kEvalOctMax 32768, the pair walk below STREAM_MIN with its depth-18 table from
# 32769; kGenRowMax 2048, kGenColMax 16384; kRangeDirectMax 4096; multi-key top trees from 32 points
# per key, a power-of-two and a generic instance; multi-key range h = 4 at 64 x 64).  A random
# sequence draws a few of them; sweep() below runs every one, under every engine setting that
# changes its kernel, once per configuration.
EVAL16_M = (1, 2048, 2049, 8192, 8193, 32768, 32769, 40000)
EVAL16_FORCED_M = 3001  # eval_device under mode 1 and under mode 4 with forced depths
MK16 = ((200, 32), (65, 48), (10, 13))
GEN16_K = (5, 2048, 2049, 16384, 16385)
RANGE16 = (4095, 4096, 5000)
WIDE_M = (70, 5000)
WIDE_MK = ((40, 17),)
WIDE_GEN_K = (5, 70)
WIDE_RANGE = (100, 5000)
PREFIX_LEVELS = (-1, 0, 1, 9, 15, 19, 21)
EVAL_MODES = (0, 1, 4)
PREFIX_CAPS = (0, 1 << 20)


@dataclass(frozen=True)
class Step:
    kind: str
    args: tuple = ()  # sorted (name, value) pairs

    def get(self, name, default=None):
        return dict(self.args).get(name, default)

    def __str__(self):
        return f"{self.kind}({', '.join(f'{k}={v}' for k, v in self.args)})"


def S(kind, **args) -> Step:
    assert kind in STEP_BUFFERS, kind
    return Step(kind, tuple(sorted(args.items())))


def pool(config):
    """The step kinds a configuration supports, each with the shapes a random sequence draws from."""
    _, lam, nbs = CONFIGS[config]
    if lam == 16:
        p = {
            "host_eval": [dict(m=m) for m in EVAL16_M],
            "eval_device": [dict(m=m) for m in EVAL16_M + (EVAL16_FORCED_M,)],
            "eval_multikey": [dict(K=K, P=P) for K, P in MK16],
            "gen_batch": [dict(K=K) for K in GEN16_K],
            "full_domain": [dict(nb=nb, bound=b) for nb in (1, 2) for b in (0, 1)],
            "range_device": [dict(count=c) for c in RANGE16],
            "range_host": [dict(count=c) for c in RANGE16],
            "range_multikey": [dict(K=64, count=64)],
        }
    else:
        p = {
            "host_eval": [dict(m=m) for m in WIDE_M],
            "eval_device": [dict(m=m) for m in WIDE_M],
            "eval_multikey": [dict(K=K, P=P) for K, P in WIDE_MK],
            "gen_batch": [dict(K=K) for K in WIDE_GEN_K],
            "full_domain": [dict(nb=1, bound=b) for b in (0, 1)],
            "range_device": [dict(count=c) for c in WIDE_RANGE],
            "range_host": [dict(count=c) for c in WIDE_RANGE],
        }
    p["host_gen"] = [dict()]
    p["gen_many"] = [dict(m=9)]
    p["set_prefix_levels"] = [dict(levels=v) for v in PREFIX_LEVELS]
    p["set_eval_mode"] = [dict(mode=v) for v in EVAL_MODES]
    p["set_prefix_max_bytes"] = [dict(cap=v) for v in PREFIX_CAPS]
    p["trim"] = [dict()]
    return p


def _sequence(config, seed, steps, settings=True):
    """`steps` steps for one configuration, a function of (config, seed, steps, settings) alone.
    Every kind of the pool comes once while there is room, the rest are drawn uniformly, and the
    whole is shuffled; a shape is drawn uniformly from the kind's list, N from the configuration's.
    At LAMBDA = 16 one eval step per sequence (the first drawn with room for it) is the 524288-point
    stream step; every other shape has at most 40000 points."""
    _, lam, nbs = CONFIGS[config]
    rng = np.random.default_rng([seed, sorted(CONFIGS).index(config), steps])
    p = pool(config)
    kinds = [k for k in p if settings or k not in SETTINGS]
    deck = list(kinds) if steps >= len(kinds) else []
    deck += [kinds[int(i)] for i in rng.integers(0, len(kinds), size=steps - len(deck))]
    rng.shuffle(deck)
    out, stream_left = [], 1 if lam == 16 else 0
    for kind in deck:
        args = dict(p[kind][int(rng.integers(0, len(p[kind])))])
        if "nb" not in args and kind not in SETTINGS and kind != "gen_many":
            args["nb"] = int(nbs[int(rng.integers(0, len(nbs)))])
        if kind in ("host_eval", "eval_device") and stream_left and rng.random() < 0.5:
            args["m"], stream_left = STREAM_MIN, 0
        out.append(S(kind, **args))
    return out


def sweep(config):
    """Every (kind, shape) of the pool once on one prg, N dealt round-robin from the configuration's:
    in auto mode first; then every value of the settings with an eval behind it — mode 4 (LAMBDA = 16:
    stream engine, per-key top trees for every multi-key shape), eval_device below every depth of
    PREFIX_LEVELS (3001 points; LAMBDA >= 32: 5000), mode 1 (k_eval16) for one and for many keys, the
    cap on the automatic depth, and trim with a fresh allocation after it."""
    _, lam, nbs = CONFIGS[config]
    out, i = [], 0
    for kind, shapes in pool(config).items():
        if kind in SETTINGS:
            continue
        for args in shapes:
            args = dict(args)
            if "nb" not in args and kind != "gen_many":
                args["nb"], i = nbs[i % len(nbs)], i + 1
            out.append(S(kind, **args))
    big, small = (EVAL16_FORCED_M, 1) if lam == 16 else (WIDE_M[1], WIDE_M[0])
    mk = [S("eval_multikey", nb=nbs[j % len(nbs)], K=K, P=P) for j, (K, P) in enumerate(MK16)] if lam == 16 else []
    out += [S("set_eval_mode", mode=4)] + mk
    for j, levels in enumerate((9, 21, 0, 1, 15, 19, -1)):  # PREFIX_LEVELS, ending on automatic
        out += [S("set_prefix_levels", levels=levels), S("eval_device", nb=nbs[j % len(nbs)], m=big)]
    out += [S("set_eval_mode", mode=1), S("eval_device", nb=nbs[-1], m=big)] + mk[1:2]
    out += [S("set_eval_mode", mode=0), S("set_prefix_max_bytes", cap=1 << 20),
            S("eval_device", nb=nbs[-1], m=40000 if lam == 16 else big), S("set_prefix_max_bytes", cap=0),
            S("trim"), S("eval_device", nb=nbs[0], m=small)]
    return out


def eval_chunk(nb, lam):
    """Points per chunk of the staged host eval: the 128 MiB of host_chunk, shared by x and y."""
    return host_chunk(lam) * lam // (nb + lam)


# ---- hand-written ladders: the order of the steps is the point ----

def _depth(levels, nb, m=3001):
    return [S("set_prefix_levels", levels=levels), S("eval_device", nb=nb, m=m)]


def pfx_ladder_hirose16(nb):
    """d_pfx: deep table, shallow table, the per-key top trees over it, the depth-first build
    (D >= 19), the full-domain build, one level, the automatic depths (the pair walk's 18), the cap,
    trim, and a fresh allocation."""
    return ([S("set_eval_mode", mode=4)] + _depth(21, nb) + _depth(9, nb) + [S("eval_multikey", nb=nb, K=200, P=32)] +
            _depth(19, nb) + [S("full_domain", nb=2, bound=1)] + _depth(1, nb) +
            [S("set_prefix_levels", levels=-1), S("eval_device", nb=nb, m=3001),
             S("set_eval_mode", mode=0), S("eval_device", nb=nb, m=40000),
             S("set_prefix_max_bytes", cap=1 << 20), S("eval_device", nb=nb, m=40000),
             S("trim"), S("set_eval_mode", mode=4)] + _depth(15, nb))


def pfx_ladder_mmo16(nb):
    """d_pfx under the MMO PRG (the table and the rows of the level above it, level-by-level build).
    The library caps a forced depth at 28 for either PRG (kPrefixMaxForced, as prefix_depth() below) and at 8N - 1; tests/test_mmo.py
    goes up to 24; 23 is the deepest here (0.55 GB)."""
    return (_depth(1, nb) + _depth(15, nb) + _depth(23, nb) + [S("eval_multikey", nb=nb, K=200, P=32)] + _depth(8, nb) +
            [S("trim")] + _depth(15, nb))


def pfx_ladder_hirose64(nb):
    """d_pfx as the LAMBDA >= 32 table of 80-byte rows."""
    return (_depth(16, nb, 5000) + _depth(1, nb, 5000) + _depth(21, nb, 5000) +
            [S("eval_multikey", nb=nb, K=40, P=17)] + _depth(8, nb, 5000) + [S("trim")] + _depth(16, nb, 70))


WS_LADDER = [  # d_ws, Hirose LAMBDA = 128
    S("eval_device", nb=16, m=5000), S("range_device", nb=16, count=5000), S("full_domain", nb=1, bound=0),
    S("eval_multikey", nb=16, K=40, P=17), S("gen_batch", nb=16, K=70), S("eval_device", nb=40, m=70),
    S("range_device", nb=16, count=100),
]

CTR_LADDER = [  # d_ctr, Hirose LAMBDA = 16: the block count is read after every step
    S("eval_device", nb=16, m=9000),                                    # oct: the kernel zeroes the counter itself
    S("eval_device", nb=16, m=STREAM_MIN),                              # stream: work counter + block count
    S("set_eval_mode", mode=1), S("eval_device", nb=16, m=777),         # k_eval16: work counter, counts no blocks
    S("set_eval_mode", mode=0), S("range_device", nb=16, count=5000),   # range tree: block count
    S("eval_device", nb=16, m=1),                                       # row2
    S("set_eval_mode", mode=4), S("eval_multikey", nb=16, K=200, P=32),  # stream + top trees on the aux stream
]


def staging_ladder():
    """Host entry points only: tiny (h_tiny), mid (h_mid), staged in two chunks (d_stage / h_stage,
    the second chunk a pair walk with its own table), host range, tiny again, host gen, gen_many."""
    return [S("host_eval", nb=16, m=1000), S("host_eval", nb=16, m=40000),
            S("host_eval", nb=16, m=eval_chunk(16, 16) + 40000), S("range_host", nb=16, count=5000),
            S("host_eval", nb=16, m=1), S("host_gen", nb=16), S("gen_many", m=9)]


DEFERRED = [S("eval_device", nb=16, m=3001), S("range_device", nb=16, count=5000), S("eval_multikey", nb=16, K=200, P=32)]

LADDERS = {  # name -> (configuration, the buffer it is named for, steps)
    "pfx_hirose16_n4": ("hirose16", "d_pfx", pfx_ladder_hirose16(4)),
    "pfx_hirose16_n16": ("hirose16", "d_pfx", pfx_ladder_hirose16(16)),
    "pfx_mmo16": ("mmo16", "d_pfx", pfx_ladder_mmo16(16)),
    "pfx_hirose64": ("hirose64", "d_pfx", pfx_ladder_hirose64(16)),
    "ws_hirose128": ("hirose128", "d_ws", WS_LADDER),
    "ctr_hirose16": ("hirose16", "d_ctr", CTR_LADDER),
    "staging_hirose16": ("hirose16", "stage", staging_ladder()),
}


# ---- what a step lays out, as plain arithmetic (mirrors dcf_hip.hip; used for the block counts
# here and for the ladder checks of tests/test_call_sequences.py) ----

@dataclass
class Settings:
    mode: int = 0
    levels: int = -1
    cap: int = 0

    def apply(self, step):
        if step.kind == "set_eval_mode":
            self.mode = step.get("mode")
        elif step.kind == "set_prefix_levels":
            self.levels = step.get("levels")
        elif step.kind == "set_prefix_max_bytes":
            self.cap = step.get("cap")


def engine(config, st, step):
    """The kernel family an eval step runs (dcf_hip.hip plan_eval), None for other steps."""
    kind, lam, _ = CONFIGS[config]
    if step.kind not in ("host_eval", "eval_device", "eval_multikey"):
        return None
    K = step.get("K", 1)
    total = K * step.get("P", step.get("m", 0))
    if lam > 16:
        return "wide"
    if kind == "mmo":
        return "mmo"
    nb = step.get("nb")
    if st.mode == 0 and st.levels <= 0 and K == 1 and total <= 32768 and nb <= 32:
        return "lat"      # k_eval16_row2 / _row / _oct: the kernel zeroes d_ctr, eval_launch does not
    if st.mode == 0 and total < STREAM_MIN:
        return "pair"     # k_eval16_pair: no counter
    if st.mode == 1 or (st.mode == 0 and K > 1 and nb > 32):
        return "ttable"   # k_eval16: work counter, no block count
    return "stream"       # k_eval16_stream: work counter and block count


def prefix_depth(config, st, step):
    """Shared-prefix depth of a single-key eval step (dcf_eval_prefix_levels), ignoring the cap."""
    kind, lam, _ = CONFIGS[config]
    nb, m = step.get("nb"), step.get("m", 0)
    if step.kind not in ("host_eval", "eval_device") or st.levels == 0 or (kind == "mmo" and lam > 16):
        return 0
    cap = 8 * nb - 1
    if st.levels > 0:
        return min(st.levels, 28 if lam == 16 else 30, cap)
    lg = max(m, 1).bit_length() - 1
    if lam > 16:
        d = min(lg - 1, 22)
    elif kind == "mmo":
        d = min(lg - 1, 27) if m >= STREAM_MIN else 0
    else:
        e = engine(config, st, step)
        d = min(lg, 27) if e == "stream" else ((18 if lg < 18 else 19) if e == "pair" and m > 32768 else 0)
    return min(d, cap) if d >= 8 else 0


def fd_route(config, step):
    """The path of a full_domain step: "fast" (Hirose, LAMBDA = 16, the table build's 8N - 4 levels at
    least 12), "levels" (MMO, LAMBDA = 16: a launch per level between two node buffers in d_ws), else
    "range": a range_device step over the whole domain."""
    kind, lam, _ = CONFIGS[config]
    if lam == 16 and kind == "mmo":
        return "levels"
    return "fast" if lam == 16 and 8 * step.get("nb") - 4 >= 12 else "range"


def extent(config, st, step, buffer):
    """Bytes (to the leading term) a step lays out in `buffer`; None when it does not use it."""
    kind, lam, _ = CONFIGS[config]
    k, nb = step.kind, step.get("nb")
    if k == "full_domain" and fd_route(config, step) == "range":
        return extent(config, st, S("range_device", nb=nb, count=1 << (8 * nb)), buffer)
    if buffer not in STEP_BUFFERS[k] or k == "trim":
        return None
    if buffer == "d_pfx":
        if k in ("host_eval", "eval_device"):
            d = prefix_depth(config, st, step)
            return ((80 if lam > 16 else 32) << d) if d else None
        if k == "eval_multikey" and lam == 16 and kind == "hirose":
            trees = engine(config, st, step) == "stream" and st.levels != 0 and 8 * nb > 5 and step.get("P") >= 32
            return step.get("K") * 1024 if trees else None
        if k == "eval_multikey" and lam > 16 and kind == "hirose" and st.levels > 0:  # key by key, a table each
            return 80 << min(st.levels, 30, 8 * nb - 1)
        if k == "full_domain" and fd_route(config, step) == "fast":
            return 32 << (8 * nb - 4)
        return None
    if buffer == "d_ws":
        if k == "full_domain":  # the fast path lays out its table alone
            return 2 * 33 * (1 << (8 * nb)) if fd_route(config, step) == "levels" else None
        if k in ("range_device", "range_host", "range_multikey"):
            return step.get("count") * step.get("K", 1) * (4 if lam == 16 else 64 + 20)
        if lam > 16 and k in ("host_eval", "eval_device"):
            return step.get("m") * 64
        if lam > 16 and k == "eval_multikey":
            return step.get("K") * step.get("P") * 64
        if lam > 16 and k == "gen_batch":
            return min(step.get("K"), 4096) * 3 * lam
        return None
    if buffer == "stage":
        if k == "host_eval":
            return min(step.get("m"), eval_chunk(nb, lam)) * (nb + lam)
        if k == "range_host":
            return step.get("count") * lam
        if k == "host_gen":
            return 2 * 8 * nb * lam
        return step.get("m") * (5 * lam + 2)  # gen_many
    return 0  # d_ctr, the digests, d_tctr: no size to speak of


def stage_path(config, st, step):
    """Which staging buffer a host step goes through."""
    kind, lam, _ = CONFIGS[config]
    if step.kind == "host_eval":
        nb, m = step.get("nb"), step.get("m")
        if engine(config, st, step) == "lat" and m * (nb + lam) + 8 * 8 * nb * lam <= 1 << 20:
            return "h_tiny"
        if lam == 16 and st.mode == 0 and m < STREAM_MIN and m * (nb + lam) <= 64 << 20:
            return "h_mid"
        return "staged x+y"
    return {"range_host": "staged y", "host_gen": "h_tiny" if kind == "hirose" and lam == 16 else "staged gen",
            "gen_many": "staged seeds"}.get(step.kind)


# ---- running a step ----

@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    assert torch.cuda.get_device_properties(0).multi_processor_count == CUS
    import dcf_amd
    return dcf_amd


class DevGuard:
    """rows x width bytes on the device between PAD sentinel rows."""

    def __init__(self, rows, width):
        import torch
        self.buf = torch.full((rows + 2 * PAD, width), SENTINEL, dtype=torch.uint8, device="cuda")
        self.rows = rows
        self.inner = self.buf[PAD:PAD + rows]

    def intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.rows:] == SENTINEL).all())


class FlatDevGuard:
    """n bytes on the device between FLAT_PAD sentinel bytes."""

    def __init__(self, n):
        import torch
        self.buf = torch.full((n + 2 * FLAT_PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.n = n
        self.inner = self.buf[FLAT_PAD:FLAT_PAD + n]

    def intact(self):
        return bool((self.buf[:FLAT_PAD] == SENTINEL).all()) and bool((self.buf[FLAT_PAD + self.n:] == SENTINEL).all())


class HostGuard:
    """rows x width bytes of host memory between PAD sentinel rows; the inner slice is contiguous."""

    def __init__(self, rows, width):
        self.buf = np.full((rows + 2 * PAD, width), SENTINEL, np.uint8)
        self.rows = rows
        self.inner = self.buf[PAD:PAD + rows]
        assert self.inner.flags["C_CONTIGUOUS"]

    def intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.rows:] == SENTINEL).all())


@dataclass
class Ctx:
    dcf: object
    lib: object
    config: str
    prg: object = None
    P: object = None
    st: Settings = field(default_factory=Settings)
    base_bytes: int = 0

    @property
    def lam(self):
        return CONFIGS[self.config][1]

    def d(self, nb):
        return self.dcf.DcfImpl(nb, self.lam, self.prg)


def make_ctx(dcf, hip_lib, config, seed):
    kind, lam, _ = CONFIGS[config]
    rng = np.random.default_rng([seed, 0xC7])
    if kind == "mmo":
        keys = [rng.bytes(16) for _ in range(4 * lam // 16)]
        prg, P = dcf.Aes128MatyasMeyerOseasPrg(keys, lam), O.OracleMmoPrg(keys, lam)
    else:
        keys = [rng.bytes(32) for _ in range(2 if lam == 16 else 18)]
        prg, P = dcf.Aes256HirosePrg(keys, lam), O.OraclePrg(keys, lam)
    ctx = Ctx(dcf, hip_lib, config, prg, P)
    ctx.base_bytes = prg.device_bytes()
    assert prg.workspaces() == 0
    return ctx


def _key(ctx, rng, nb, bound, alpha=None):
    lam = ctx.lam
    alpha = rng.bytes(nb) if alpha is None else alpha
    beta, seeds = rng.bytes(lam), [rng.bytes(lam), rng.bytes(lam)]
    return O.gen(ctx.P, alpha, beta, seeds[0], seeds[1], bound), alpha, beta, seeds


def _xs(rng, m, nb, alpha):
    """Random points with alpha planted at row 0 and, in a batch of more than 8, its neighbours."""
    xs = rng.integers(0, 256, size=(m, nb), dtype=np.uint8)
    a = np.frombuffer(alpha, np.uint8)
    xs[0] = a
    if m > 8:
        xs[1:8] = a
        xs[1:8, -1] = (a[-1] + np.array([1, 255, 2, 254, 128, 3, 253], np.uint8)) & 0xFF
    return xs


def _rows(m, rng):
    return np.arange(m) if m <= 4096 else _sample(m, rng)


def _want_rec(xs, alpha, beta, bound):
    a = np.frombuffer(alpha, np.uint8)
    on = _lt(xs, a) if bound == 0 else (~_lt(xs, a)) & (xs != a).any(1)
    return np.where(on[:, None], np.frombuffer(beta, np.uint8)[None, :], 0).astype(np.uint8)


def _range_rec(rec, beta, off, count, bound):
    """rec (count, lam) numpy = y0 ^ y1 over x0 + i; alpha = x0 + off inside the range."""
    on = np.arange(count) < off if bound == 0 else np.arange(count) > off
    bt = np.frombuffer(beta, np.uint8)
    return bool((rec[on] == bt).all()) and not rec[~on].any()


def _np(y):
    return y if isinstance(y, np.ndarray) else y.cpu().numpy()


def _stream_bounds(n, depth, points, trees=0):
    """AES blocks of a stream-engine walk below a table of `depth` levels: every remaining level of
    every point encrypts A, B or both, and a right step at t = 0 can spare the next level's block
    (tests/test_gpu_parity.py test_stream_b_reuse_vs_oracle), so between half a block and two blocks
    per level and point; `trees`: the blocks of the multi-key top trees, counted exactly.
    The header gives no formula for this engine, so the band is 4x wide.  What it catches: a count
    left over from a call at least 4x larger per point-level (the 524288-point step before a small
    one, a range call's count), a count never zeroed, and any count at all after an engine that
    counts nothing (the (0, 0) of _eval_blocks).  What it cannot: two calls of similar size added
    up, which may still lie inside it — tests/test_stream_update_gpu.py pins that engine's count
    exactly, on a fresh prg."""
    return trees + (n - depth) * points // 2, trees + 2 * (n - depth) * points


def _assert_plan(ctx, step, nb, K, ppk):
    """dcf_eval_plan names the engine the rule above predicts for this eval step (the rule stays:
    it predicts the buffers), the key mode of the shape, and dcf_eval_prefix_levels' depth."""
    E = ctx.dcf.Engine
    total = K * ppk
    want = {"wide": (E.WIDE_BATCH, E.WIDE_PER_KEY), "mmo": (E.MMO16,), "pair": (E.PAIR,), "ttable": (E.TTABLE,),
            "stream": (E.STREAM,), "lat": (E.ROW2 if total <= 2048 else E.ROW if total <= 8192 else E.OCT,)}
    plan = ctx.prg.eval_plan(nb, K, ppk)
    assert plan.engine in want[engine(ctx.config, ctx.st, step)], ("eval_plan", plan, engine(ctx.config, ctx.st, step))
    assert plan.unsupported is None and plan.key_mode == (0 if K == 1 else 1 if ppk % 64 == 0 else 2), ("eval_plan", plan)
    assert plan.prefix_levels == ctx.prg.eval_prefix_levels(nb, K, ppk), ("eval_plan", plan)
    if CONFIGS[ctx.config][1] == 16 and CONFIGS[ctx.config][0] == "hirose":
        assert plan.small == (ctx.st.mode == 0 and total < STREAM_MIN), ("eval_plan", plan)


def _eval_blocks(ctx, step, nb, K, ppk):
    """What dcf_prg_last_eval_blocks must read after this eval step, as (lo, hi), or None."""
    e = engine(ctx.config, ctx.st, step)
    if e in ("lat", "pair", "ttable", "mmo"):
        return 0, 0  # engines that count nothing: the count of the call before must be gone
    if e != "stream":
        return None
    if K == 1:
        return _stream_bounds(8 * nb, ctx.prg.eval_prefix_levels(nb, 1, ppk), ppk)
    trees = ctx.st.levels != 0 and 8 * nb > 5 and ppk >= 32
    # k_mk_prefix16: 4 threads per key, 2 + 7 PRG calls of 2 blocks each
    return _stream_bounds(8 * nb, 5 if trees else 0, K * ppk, 72 * K if trees else 0)


def _range_blocks(ctx, nb, K, x0, count, h):
    kind, lam, _ = CONFIGS[ctx.config]
    n, roots = 8 * nb, _nroots(x0, count, h)
    if nb > 16 or (kind == "mmo" and lam > 16):
        return None  # the materialising path documents no count
    if lam > 16:  # kernels_range_wide.h: exact
        b = 4 * n * count if h == 0 else roots * (4 * (n - h) + 4 * ((1 << h) - 1))
        return b, b
    if kind == "mmo":  # exact
        b = 2 * n * K * count if h == 0 else K * roots * (2 * (n - h) + 4 * ((1 << h) - 1))
        return b, b
    # Hirose LAMBDA = 16: the bounds of test_range_multikey_gpu._check_blocks
    return 2 * K * (count - 1), K * roots * (2 * (n - h) + 2 * ((1 << h) - 1))


@dataclass
class Pending:
    """A launched step: check() compares everything once the streams are synchronized; blocks is the
    (lo, hi) dcf_prg_last_eval_blocks must lie in right after the step, or None."""
    check: object
    blocks: object = None


def _check_eval(ctx, what, ok, alpha, beta, seeds, bound, xs, outs, rng):
    rows = _rows(len(xs), rng)

    def check():
        ys = []
        for b, g in enumerate(outs):
            assert g.intact(), ("neighbours of ys written", "party", b) + what
            y = _np(g.inner)
            want = O.eval_(ctx.P, b, ok, seeds[b], xs[rows], nthreads=8)
            bad = np.flatnonzero((y[rows] != want).any(axis=1))
            assert bad.size == 0, what + ("party", b, "first mismatching rows", rows[bad[:8]])
            ys.append(y)
        assert np.array_equal(ys[0] ^ ys[1], _want_rec(xs, alpha, beta, bound)), ("reconstruction",) + what
    return check


def step_eval_device(ctx, rng, step):
    import torch
    nb, m, lam = step.get("nb"), step.get("m"), ctx.lam
    bound = int(rng.integers(0, 2))
    _assert_plan(ctx, step, nb, 1, m)
    ok, alpha, beta, seeds = _key(ctx, rng, nb, bound)
    xs = _xs(rng, m, nb, alpha)
    xd, cwb, d = torch.from_numpy(xs).cuda(), _dev(_cwb(ok)), ctx.d(nb)
    outs = []
    for b in (0, 1):
        g = DevGuard(m, lam)
        d.eval_device(bool(b), cwb, _dev(seeds[b]), xd, ys=g.inner)
        outs.append(g)
    return Pending(_check_eval(ctx, (str(step),), ok, alpha, beta, seeds, bound, xs, outs, rng),
                   _eval_blocks(ctx, step, nb, 1, m))


def step_host_eval(ctx, rng, step):
    nb, m, lam = step.get("nb"), step.get("m"), ctx.lam
    bound = int(rng.integers(0, 2))
    _assert_plan(ctx, step, nb, 1, m)
    ok, alpha, beta, seeds = _key(ctx, rng, nb, bound)
    xs = _xs(rng, m, nb, alpha)
    d, outs = ctx.d(nb), []
    for b in (0, 1):
        g = HostGuard(m, lam)
        d.eval(bool(b), ctx.dcf.cwb_to_share(_cwb(ok), nb, lam, [seeds[b]]), xs, ys=g.inner)
        outs.append(g)
    chunk = eval_chunk(nb, lam)
    # a chunked call's count is its last chunk's (eval_launch zeroes it per chunk): not asserted
    blocks = _eval_blocks(ctx, step, nb, 1, m) if m <= chunk or stage_path(ctx.config, ctx.st, step) != "staged x+y" else None
    return Pending(_check_eval(ctx, (str(step),), ok, alpha, beta, seeds, bound, xs, outs, rng), blocks)


def step_eval_multikey(ctx, rng, step):
    import torch
    nb, K, P, lam = step.get("nb"), step.get("K"), step.get("P"), ctx.lam
    _assert_plan(ctx, step, nb, K, P)
    keys = [_key(ctx, rng, nb, 0) for _ in range(K)]
    xs = rng.integers(0, 256, size=(K * P, nb), dtype=np.uint8)
    xs[::P] = np.stack([np.frombuffer(k[1], np.uint8) for k in keys])
    cwb, xd, d = _dev(_cwbk([k[0] for k in keys], nb, lam)), torch.from_numpy(xs).cuda(), ctx.d(nb)
    outs = []
    for b in (0, 1):
        g = DevGuard(K * P, lam)
        s0s = _dev(b"".join(k[3][b] for k in keys)).view(K, lam)
        d.eval_multikey_device(bool(b), cwb, s0s, xd, P, ys=g.inner)
        outs.append(g)
    what = (str(step),)

    def check():
        ys = []
        for b, g in enumerate(outs):
            assert g.intact(), ("neighbours of ys written", "party", b) + what
            y = _np(g.inner)
            for k, (ok, _, _, seeds) in enumerate(keys):
                sl = slice(k * P, (k + 1) * P)
                assert np.array_equal(y[sl], O.eval_(ctx.P, b, ok, seeds[b], xs[sl], nthreads=8)), what + ("party", b, "key", k)
            ys.append(y)
        want = np.concatenate([_want_rec(xs[k * P:(k + 1) * P], a, bt, 0) for k, (_, a, bt, _) in enumerate(keys)])
        assert np.array_equal(ys[0] ^ ys[1], want), ("reconstruction",) + what
    return Pending(check, _eval_blocks(ctx, step, nb, K, P))


def step_gen_batch(ctx, rng, step):
    import torch
    nb, K, lam = step.get("nb"), step.get("K"), ctx.lam
    bound = int(rng.integers(0, 2))
    A = rng.integers(0, 256, size=(K, nb), dtype=np.uint8)
    B, S0, S1 = (rng.integers(0, 256, size=(K, lam), dtype=np.uint8) for _ in range(3))
    nbytes = ctx.dcf.cwb_bytes(nb, lam, K)
    g = FlatDevGuard(nbytes)
    ctx.d(nb).gen_batch_device(*(torch.from_numpy(a).cuda() for a in (A, B, S0, S1)), ctx.dcf.BoundState(bound), cwb_out=g.inner)
    # every key up to 4096, else the first and last 1024 and 1024 random ones
    picks = np.arange(K) if K <= 4096 else _sample(K, rng, edge=1024, rand=1024)
    what = (str(step), "bound", bound)

    def check():
        assert g.intact(), ("neighbours of cwb_out written",) + what
        c, n = _np(g.inner), 8 * nb
        off = ctx.dcf.cwb_np1_offset(nb, lam, K)
        oks = [O.gen(ctx.P, A[k].tobytes(), B[k].tobytes(), S0[k].tobytes(), S1[k].tobytes(), bound) for k in picks]
        parts = {"cw_s": (c[:n * K * lam].reshape(n, K, lam), 1), "cw_v": (c[n * K * lam:2 * n * K * lam].reshape(n, K, lam), 1),
                 "cw_t": (c[2 * n * K * lam:2 * n * K * lam + n * K].reshape(n, K), 1), "cw_np1": (c[off:off + K * lam].reshape(K, lam), 0)}
        for name, (got, axis) in parts.items():
            want = np.stack([getattr(ok, name) for ok in oks], axis=axis)
            diff = np.take(got, picks, axis=axis) != want
            bad = np.flatnonzero(diff.reshape(diff.shape[0], len(picks), -1).any(axis=(0, 2)) if axis else diff.reshape(len(picks), -1).any(axis=1))
            assert bad.size == 0, what + (name, "first mismatching keys", picks[bad[:8]])
    return Pending(check)


def step_full_domain(ctx, rng, step):
    nb, bound, lam = step.get("nb"), step.get("bound"), ctx.lam
    count = 1 << (8 * nb)
    ok, alpha, beta, seeds = _key(ctx, rng, nb, bound)
    cwb, d, outs = _dev(_cwb(ok)), ctx.d(nb), []
    for b in (0, 1):
        g = DevGuard(count, lam)
        d.eval_full_domain_device(bool(b), cwb, _dev(seeds[b]), ys=g.inner)
        outs.append(g)
    rows = _rows(count, rng)
    xs = _points(nb, 0, rows)
    what = (str(step),)

    def check():
        ys = []
        for b, g in enumerate(outs):
            assert g.intact(), ("neighbours of ys written", "party", b) + what
            y = _np(g.inner)
            bad = np.flatnonzero((y[rows] != O.eval_(ctx.P, b, ok, seeds[b], xs, nthreads=8)).any(axis=1))
            assert bad.size == 0, what + ("party", b, "first mismatching x", rows[bad[:8]])
            ys.append(y)
        assert _range_rec(ys[0] ^ ys[1], beta, int.from_bytes(alpha, "big"), count, bound), ("reconstruction",) + what
    # full-domain eval's own paths document no count; every other shape is a range call over [0, count)
    blocks = _range_blocks(ctx, nb, 1, 0, count, d.range_subtree_levels(count)) if fd_route(ctx.config, step) == "range" else None
    return Pending(check, blocks)


def _unaligned_x0(rng, nb):
    """An odd x0 in the lower half of the domain (room for the count above it), at most 128 bits."""
    return ((int.from_bytes(rng.bytes(min(nb, 16)), "big") >> 1) | 1)


def _step_range(ctx, rng, step, host):
    nb, count, lam = step.get("nb"), step.get("count"), ctx.lam
    x0, bound, off = _unaligned_x0(rng, nb), int(rng.integers(0, 2)), int(rng.integers(0, count))
    ok, alpha, beta, seeds = _key(ctx, rng, nb, bound, alpha=(x0 + off).to_bytes(nb, "big"))
    d, outs = ctx.d(nb), []
    cwb = None if host else _dev(_cwb(ok))
    for b in (0, 1):
        if host:
            g = HostGuard(count, lam)
            d.eval_range(bool(b), ctx.dcf.cwb_to_share(_cwb(ok), nb, lam, [seeds[b]]), x0, count, ys=g.inner)
        else:
            g = DevGuard(count, lam)
            d.eval_range_device(bool(b), cwb, _dev(seeds[b]), x0, count, ys=g.inner)
        outs.append(g)
    rows = _rows(count, rng)
    xs = _points(nb, x0, rows)
    what = (str(step), "x0", hex(x0), "alpha at row", off, "bound", bound)

    def check():
        ys = []
        for b, g in enumerate(outs):
            assert g.intact(), ("neighbours of ys written", "party", b) + what
            y = _np(g.inner)
            bad = np.flatnonzero((y[rows] != O.eval_(ctx.P, b, ok, seeds[b], xs, nthreads=8)).any(axis=1))
            assert bad.size == 0, what + ("party", b, "first mismatching i", rows[bad[:8]])
            ys.append(y)
        assert _range_rec(ys[0] ^ ys[1], beta, off, count, bound), ("reconstruction",) + what
    return Pending(check, _range_blocks(ctx, nb, 1, x0, count, d.range_subtree_levels(count)))


def step_range_device(ctx, rng, step):
    return _step_range(ctx, rng, step, host=False)


def step_range_host(ctx, rng, step):
    return _step_range(ctx, rng, step, host=True)


def step_range_multikey(ctx, rng, step):
    nb, K, count, lam = step.get("nb"), step.get("K"), step.get("count"), ctx.lam
    x0 = _unaligned_x0(rng, nb)
    offs = [int(rng.integers(0, count)) for _ in range(K)]
    keys = [_key(ctx, rng, nb, k % 2, alpha=(x0 + offs[k]).to_bytes(nb, "big")) for k in range(K)]
    cwb, d, outs = _dev(_cwbk([k[0] for k in keys], nb, lam)), ctx.d(nb), []
    for b in (0, 1):
        g = DevGuard(K * count, lam)
        s0s = _dev(b"".join(k[3][b] for k in keys)).view(K, lam)
        d.eval_range_multikey_device(bool(b), cwb, s0s, x0, count, ys=g.inner.view(K, count, lam))
        outs.append(g)
    xs = _points(nb, x0, range(count))
    what = (str(step), "x0", hex(x0))

    def check():
        ys = []
        for b, g in enumerate(outs):
            assert g.intact(), ("neighbours of ys written", "party", b) + what
            y = _np(g.inner).reshape(K, count, lam)
            for k, (ok, _, _, seeds) in enumerate(keys):
                assert np.array_equal(y[k], O.eval_(ctx.P, b, ok, seeds[b], xs, nthreads=8)), what + ("party", b, "key", k)
            ys.append(y)
        rec = ys[0] ^ ys[1]
        for k in range(K):
            assert _range_rec(rec[k], keys[k][2], offs[k], count, k % 2), ("reconstruction", "key", k) + what
    return Pending(check, _range_blocks(ctx, nb, K, x0, count, d.range_multikey_subtree_levels(K, count)))


def step_host_gen(ctx, rng, step):
    nb, lam = step.get("nb"), ctx.lam
    bound = int(rng.integers(0, 2))
    alpha, beta, s0, s1 = rng.bytes(nb), rng.bytes(lam), rng.bytes(lam), rng.bytes(lam)
    n = ctx.dcf.cwb_bytes(nb, lam, 1)
    buf = np.full(n + 2 * FLAT_PAD, SENTINEL, np.uint8)
    rc = ctx.lib.dcf_gen(ctx.prg.handle, nb, alpha, beta, s0, s1, bound, ctypes.c_void_p(buf.ctypes.data + FLAT_PAD))
    assert rc == 0, (str(step), rc)
    what = (str(step), "bound", bound)

    def check():
        assert (buf[:FLAT_PAD] == SENTINEL).all() and (buf[FLAT_PAD + n:] == SENTINEL).all(), ("neighbours of cwb_out written",) + what
        assert buf[FLAT_PAD:FLAT_PAD + n].tobytes() == _cwb(O.gen(ctx.P, alpha, beta, s0, s1, bound)), what
    return Pending(check)


def step_gen_many(ctx, rng, step):
    m, lam = step.get("m"), ctx.lam
    seeds = [rng.bytes(lam) for _ in range(m)]
    g = HostGuard(m, 4 * lam + 2)
    rc = ctx.lib.dcf_prg_gen(ctx.prg.handle, b"".join(seeds), m, ctypes.c_void_p(g.inner.ctypes.data))
    assert rc == 0, (str(step), rc)
    what = (str(step),)

    def check():
        assert g.intact(), ("neighbours of out written",) + what
        for i, sd in enumerate(seeds):
            (sl, vl, tl), (sr, vr, tr) = ctx.P.gen(sd)
            assert g.inner[i].tobytes() == sl + vl + sr + vr + bytes([tl, tr]), what + ("seed", i)
    return Pending(check)


def step_setting(ctx, rng, step):
    prg = ctx.prg
    if step.kind == "set_prefix_levels":
        prg.set_prefix_levels(step.get("levels"))
    elif step.kind == "set_eval_mode":
        prg.set_eval_mode(step.get("mode"))
    elif step.kind == "set_prefix_max_bytes":
        prg.set_prefix_max_bytes(step.get("cap"))
    else:  # trim: every workspace is idle between the steps of a sequence
        n = prg.workspaces()
        assert prg.trim() == n, (str(step), n)
        assert prg.workspaces() == 0 and prg.host_pinned_bytes() == 0
        assert prg.device_bytes() == ctx.base_bytes, (prg.device_bytes(), ctx.base_bytes)
    ctx.st.apply(step)
    return None


STEPS = {
    "host_eval": step_host_eval, "eval_device": step_eval_device, "eval_multikey": step_eval_multikey,
    "gen_batch": step_gen_batch, "full_domain": step_full_domain, "range_device": step_range_device,
    "range_host": step_range_host, "range_multikey": step_range_multikey, "host_gen": step_host_gen,
    "gen_many": step_gen_many, "set_prefix_levels": step_setting, "set_eval_mode": step_setting,
    "set_prefix_max_bytes": step_setting, "trim": step_setting,
}
assert set(STEPS) == set(STEP_BUFFERS)


def run_sequence(ctx, steps, seed, label):
    """Each step in turn on ctx.prg: launch, synchronize, compare, read the block count."""
    import torch
    rng = np.random.default_rng([seed, 0x5E9])
    for i, step in enumerate(steps):
        try:
            pend = STEPS[step.kind](ctx, rng, step)
            if pend is None:
                continue
            torch.cuda.synchronize()
            pend.check()
            if pend.blocks is not None:
                blocks, (lo, hi) = ctx.prg.last_eval_blocks(), pend.blocks
                print(f"{label} step {i} {step}: {blocks} blocks, expected [{lo}, {hi}]")
                assert lo <= blocks <= hi, ("block count", blocks, "expected", lo, hi)
        except (AssertionError, ctx.dcf.DcfError) as e:
            raise AssertionError(f"{label} ({ctx.config}, seed {seed}) step {i} {step}: {e}") from e


# ---- the tests ----

@pytest.mark.parametrize("name", sorted(LADDERS))
def test_ladder(dcf, hip_lib, name):
    config, _, steps = LADDERS[name]
    run_sequence(make_ctx(dcf, hip_lib, config, 11), steps, 11, name)


def _queue(ctx, steps, rng, streams, host_after):
    """The steps queued back to back with no synchronize, step i on streams[i] (None: the current
    stream), then (host_after) a host eval straight after them; one synchronize; every check."""
    import torch
    pend = []
    for step, s in zip(steps, streams):
        if s is None:
            pend.append(STEPS[step.kind](ctx, rng, step))
        else:
            with torch.cuda.stream(s):
                pend.append(STEPS[step.kind](ctx, rng, step))
    if host_after:
        pend.append(step_host_eval(ctx, rng, S("host_eval", nb=16, m=40000)))
    torch.cuda.synchronize()
    for p in pend:
        p.check()


@pytest.mark.parametrize("host_after", [False, True], ids=["device_only", "host_eval_after"])
def test_deferred_synchronization(dcf, hip_lib, host_after):
    """eval_device below a depth-21 table, a range tree and a multi-key eval with top trees queued
    with no synchronize between them, on one stream and then on three: each call gets the workspace
    of the one before (LIFO pool) and overwrites its d_pfx / d_ws / d_ctr, ordered only by
    Workspace::done and the aux fork / join."""
    import torch
    ctx = make_ctx(dcf, hip_lib, "hirose16", 12)
    for st in (S("set_eval_mode", mode=4), S("set_prefix_levels", levels=21)):
        step_setting(ctx, None, st)
    rng = np.random.default_rng(12)
    try:
        _queue(ctx, DEFERRED, rng, [None] * 3, host_after)
        _queue(ctx, DEFERRED, rng, [torch.cuda.Stream() for _ in range(3)], host_after)
    except AssertionError as e:
        raise AssertionError(f"deferred (hirose16, seed 12, host_after={host_after}): {e}") from e


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_sweep(dcf, hip_lib, config):
    """Every shape of the pool, under every engine it can select, once on one long-lived prg."""
    run_sequence(make_ctx(dcf, hip_lib, config, 14), sweep(config), 14, "sweep")


DEFAULT_STEPS, DEFAULT_SEEDS = 24, (1, 2)
SEQ_STEPS = int(os.environ.get("DCF_SEQ_STEPS", DEFAULT_STEPS))
SEQ_SEEDS = [int(os.environ["DCF_SEQ_SEED"], 0)] if "DCF_SEQ_SEED" in os.environ else list(DEFAULT_SEEDS)


@pytest.mark.parametrize("seed", SEQ_SEEDS)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_random_sequence(dcf, hip_lib, config, seed):
    run_sequence(make_ctx(dcf, hip_lib, config, seed), _sequence(config, seed, SEQ_STEPS), seed, "random")


@pytest.mark.parametrize("config", ["hirose16", "hirose128"])
def test_threads_share_one_prg(dcf, hip_lib, config):
    """Four host threads, each with its own 8-step sequence (no settings steps: a setter racing a call
    is allowed, but then no test could know which engine ran), every other thread on a side stream;
    everything is compared after the pool has joined."""
    import torch
    ctx = make_ctx(dcf, hip_lib, config, 13)

    def job(t):
        rng = np.random.default_rng([13, t])
        steps = _sequence(config, 100 + t, 8, settings=False)
        stream = torch.cuda.Stream() if t % 2 else None
        pend = []
        for step in steps:
            if stream is None:
                pend.append(STEPS[step.kind](ctx, rng, step))
            else:
                with torch.cuda.stream(stream):
                    pend.append(STEPS[step.kind](ctx, rng, step))
        return steps, pend

    with ThreadPoolExecutor(4) as ex:
        res = list(ex.map(job, range(4)))
    torch.cuda.synchronize()
    assert ctx.prg.workspaces() >= 2  # calls really overlapped
    for t, (steps, pend) in enumerate(res):
        for i, (step, p) in enumerate(zip(steps, pend)):
            try:
                p.check()
            except AssertionError as e:
                raise AssertionError(f"threads ({config}, seed {100 + t}) thread {t} step {i} {step}: {e}") from e
