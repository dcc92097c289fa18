"""dcf_eval_plan against the rules include/dcf_hip.h documents, for single-key shapes and for the
agreement with dcf_eval_prefix_levels.  A dcf_prg reads its device's compute-unit count, so these
need a device; no kernel is launched.  The thresholds that depend on that count are checked as
"exactly one change of engine between 2^17 and 2^21 points", never against a number."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the grid of tests/test_abi.py test_multikey_launch_split_keeps_indices_32_bit
GRID_NB = (1, 4, 16, 17, 32, 64, 159)
GRID_PPK = (1, 32, 64, 255, 256, 4096, 1 << 20, 1 << 30, (1 << 31) + 5)


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


def _prg(dcf, kind="hirose", lam=16):
    rng = np.random.default_rng(0xE7A1)
    if kind == "mmo":
        return dcf.Aes128MatyasMeyerOseasPrg([rng.bytes(16) for _ in range(4 * lam // 16)], lam)
    return dcf.Aes256HirosePrg([rng.bytes(32) for _ in range(2 if lam == 16 else 18)], lam)


def test_latency_kernel_ladder(dcf):
    """One key, automatic mode, N <= 32: ROW2 <= 2048 < ROW <= 8192 < OCT <= 32768 < PAIR."""
    E, prg = dcf.Engine, _prg(dcf)
    ladder = [(1, E.ROW2), (2048, E.ROW2), (2049, E.ROW), (8192, E.ROW), (8193, E.OCT), (32768, E.OCT), (32769, E.PAIR)]
    for nb in (1, 16, 32):
        for m, want in ladder:
            plan = prg.eval_plan(nb, 1, m)
            assert plan.engine == want and plan.key_mode == 0 and plan.small and plan.unsupported is None, (nb, m, plan)
            if want != E.PAIR:
                assert plan.prefix_levels == 0, (nb, m, plan)


def test_n33_never_takes_a_latency_kernel(dcf):
    E, prg = dcf.Engine, _prg(dcf)
    for nb in (33, 40, 256):
        for m in (1, 2048, 2049, 8192, 8193, 32768):
            assert prg.eval_plan(nb, 1, m).engine == E.PAIR, (nb, m)
    assert prg.eval_plan(32, 1, 1).engine == E.ROW2


def test_forced_modes(dcf):
    """DCF_EVAL_TTABLE / _STREAM name their engine for every size, one key or many, and are never
    `small`; the MMO PRG and LAMBDA >= 32 ignore the setting."""
    E, prg = dcf.Engine, _prg(dcf)
    shapes = [(16, 1, 1), (16, 1, 40000), (16, 1, 1 << 21), (2, 5, 64), (2, 5, 33), (33, 1, 70), (16, 1 << 14, 64)]
    for mode, want in ((1, E.TTABLE), (4, E.STREAM)):
        prg.set_eval_mode(mode)
        for nb, K, P in shapes:
            plan = prg.eval_plan(nb, K, P)
            assert plan.engine == want and not plan.small and plan.unsupported is None, (mode, nb, K, P, plan)
            assert plan.key_mode == (0 if K == 1 else 1 if P % 64 == 0 else 2)
    mmo, wide, wide_mmo = _prg(dcf, "mmo"), _prg(dcf, lam=32), _prg(dcf, "mmo", 32)
    for mode in (0, 1, 4):
        for p in (mmo, wide, wide_mmo):
            p.set_eval_mode(mode)
        for nb, K, P in shapes:
            assert mmo.eval_plan(nb, K, P).engine == E.MMO16, (mode, nb, K, P)
            assert wide.eval_plan(nb, K, P).engine == (E.WIDE_BATCH if K > 1 else E.WIDE_PER_KEY), (mode, nb, K, P)
            assert wide_mmo.eval_plan(nb, K, P).engine == E.WIDE_PER_KEY, (mode, nb, K, P)
            if K * P <= 40000:  # far below two points per lane of any device
                assert mmo.eval_plan(nb, K, P).small == (mode == 0), (mode, nb, K, P)
            assert mode == 0 or not mmo.eval_plan(nb, K, P).small
            assert not wide.eval_plan(nb, K, P).small


def test_forced_depth_disables_the_latency_kernels(dcf):
    """dcf_prg_set_prefix_levels(k > 0): the pair walk below a table of that depth (at most 8N - 1)
    where automatic mode ran a latency kernel; 0 (off) keeps the latency kernels."""
    E, prg = dcf.Engine, _prg(dcf)
    prg.set_prefix_levels(9)
    for nb, m, depth in ((16, 1, 9), (16, 1000, 9), (16, 32768, 9), (1, 100, 7)):
        plan = prg.eval_plan(nb, 1, m)
        assert plan.engine == E.PAIR and plan.prefix_levels == depth, (nb, m, plan)
    prg.set_prefix_levels(0)
    assert prg.eval_plan(16, 1, 1000).engine == E.ROW2 and prg.eval_plan(16, 1, 32768).engine == E.OCT
    assert prg.eval_plan(16, 1, 40000).prefix_levels == 0
    prg.set_prefix_levels(-1)
    assert prg.eval_plan(16, 1, 1000).engine == E.ROW2


def test_prefix_levels_agree_with_dcf_eval_prefix_levels(dcf):
    """Both exports read the same plan: every (N, P) of the ABI test's grid, one key and three,
    each PRG, each engine setting, automatic / off / forced depths.  A shape the plan calls
    unsupported still fills prefix_levels."""
    n = 0
    for kind, lam in (("hirose", 16), ("mmo", 16), ("hirose", 32), ("mmo", 32)):
        prg = _prg(dcf, kind, lam)
        for mode in (0, 1, 4):
            prg.set_eval_mode(mode)
            for levels in (-1, 0, 9, 21):
                prg.set_prefix_levels(levels)
                for nb in GRID_NB:
                    for ppk in GRID_PPK:
                        for K in (1, 3):
                            plan = prg.eval_plan(nb, K, ppk)
                            assert plan.prefix_levels == prg.eval_prefix_levels(nb, K, ppk), (kind, lam, mode, levels, nb, K, ppk, plan)
                            assert plan.key_mode == (0 if K == 1 else 1 if ppk % 64 == 0 else 2)
                            n += 1
    assert n == 4 * 3 * 4 * len(GRID_NB) * len(GRID_PPK) * 2


def test_one_change_of_engine_between_2_17_and_2_21_points(dcf):
    """Automatic mode, one key, N = 16: the pair walk at 2^17 points, the stream engine at 2^21,
    and one m* between them such that every probe below m* is the pair walk (and `small`) and every
    probe from m* on the stream engine (and not).  m* is where two points per lane of the device
    are reached; it is found by bisection and printed, not compared with a number."""
    E, prg = dcf.Engine, _prg(dcf)
    lo, hi = 1 << 17, 1 << 21
    assert prg.eval_plan(16, 1, lo).engine == E.PAIR and prg.eval_plan(16, 1, hi).engine == E.STREAM
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if prg.eval_plan(16, 1, mid).engine == E.PAIR else (lo, mid)
    edge = hi
    print(f"pair walk -> stream engine at {edge} points")
    rng = np.random.default_rng(3)
    probes = np.unique(np.concatenate([[1 << 17, 1 << 21, edge - 1, edge], np.arange(1 << 17, (1 << 21) + 1, 1 << 14),
                                       rng.integers(1 << 17, 1 << 21, size=256)]))
    for m in map(int, probes):
        plan = prg.eval_plan(16, 1, m)
        assert plan.engine == (E.PAIR if m < edge else E.STREAM) and plan.small == (m < edge), (m, edge, plan)
    # the multi-key plan turns at the same total
    assert prg.eval_plan(2, edge // 64 - 1, 64).engine == E.PAIR and prg.eval_plan(2, -(-edge // 64), 64).engine == E.STREAM
