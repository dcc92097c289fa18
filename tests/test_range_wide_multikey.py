"""Multi-key range eval over the Hirose PRG at LAMBDA >= 32, the parts that need no GPU: the block
height of dcf_eval_range_wide_multikey_subtree_levels and the launch-group size of
dcf_eval_range_wide_keys_per_launch (pure arithmetic), the argument checks of the entry point that
return before any device access, and the mirrors of the two functions."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 2, 4, 16)
KS = (1, 2, 3, 63, 64, 67, 4096, 4099, 1 << 16, 1 << 20)
LAMS = (32, 48, 128)
COUNTS = sorted({c for e in range(0, 40) for c in ((1 << e) - 1, 1 << e, (1 << e) + 1) if c > 0} |
                {63, 64, 65, 100, 256, 1000, 4095, 4096, 4173, 32768, 32769, 32773})
PER = 1 << 22  # dcf_eval_range_wide_points_per_launch at N <= 16


def single_rule(nb: int, count: int) -> int:
    if count < 1 << 12:
        return 0
    return min(8 * nb, 14, max(8, count.bit_length() - 1 - 8))


def multikey_rule(nb: int, K: int, count: int) -> int:
    if count < 64 or K * count < 1 << 12:
        return 0
    return min(8 * nb, 14, count.bit_length() - 1 - 2)


def rule(nb: int, K: int, count: int) -> int:
    """include/dcf_hip.h: the single-key height from 2^12 points per key, the multi-key height below."""
    return single_rule(nb, count) if count >= 1 << 12 else multikey_rule(nb, K, count)


def keys_rule(nb: int, K: int, count: int) -> int:
    """include/dcf_hip.h: the most whole keys within the four bounds, at least 1; 1 above 32768 points."""
    h = rule(nb, K, count)
    span = ((count >> h) + 2) << h
    if count > 32768 or span > PER:
        return 1
    return max(1, min(PER // span, 4096, 32768 // -(-count // 4096), (0xFFFFFFFF // 4) // (8 * nb)))


def _counts(nb):
    return [c for c in COUNTS if nb >= 8 or c <= 1 << (8 * nb)]


@pytest.mark.parametrize("nb", NS)
@pytest.mark.parametrize("K", KS)
def test_height_rule(hip_lib, nb, K):
    f = hip_lib.dcf_eval_range_wide_multikey_subtree_levels
    for c in _counts(nb):
        h = f(nb, K, c)
        assert h == rule(nb, K, c), (nb, K, c, h)
        if c >= 1 << 12:
            assert h == hip_lib.dcf_eval_range_subtree_levels(nb, c), (nb, K, c, h)
        else:
            assert h == hip_lib.dcf_eval_range_multikey_subtree_levels(nb, K, c), (nb, K, c, h)
        assert h == 0 or 4 <= h <= min(8 * nb, 14), (nb, K, c, h)


def test_height_rule_values(hip_lib):
    """The values themselves (the shapes of tests/test_range_wide_multikey_gpu.py among them), so a
    change of rule() and library together still shows."""
    f = hip_lib.dcf_eval_range_wide_multikey_subtree_levels
    assert f(1, 67, 256) == 6 and f(1, 15, 256) == 0 and f(1, 16, 256) == 6
    assert f(2, 5, 1000) == 7 and f(2, 4, 1000) == 0
    assert f(16, 64, 65) == 4
    assert f(2, 3, 63) == 0
    assert (f(2, 64, 63), f(2, 63, 65), f(2, 64, 64)) == (0, 0, 4)
    assert f(4, 2, (1 << 12) + 77) == 8 and f(2, 3, 5000) == 8
    assert f(2, 1, 4095) == 0 and f(2, 2, 4095) == 9 and f(2, 1, 4096) == 8  # not monotone in count across 2^12
    assert f(1, 4099, 64) == 4
    assert f(4, 2, 32768 + 5) == 8
    assert f(4, 1 << 20, 1 << 22) == 14
    assert f(0, 5, 1000) == 0 and f(17, 5, 1000) == 0 and f(2, 0, 1000) == 0 and f(2, 5, 0) == 0


@pytest.mark.parametrize("nb", NS)
@pytest.mark.parametrize("lam", LAMS)
def test_keys_per_launch(hip_lib, nb, lam):
    f = hip_lib.dcf_eval_range_wide_keys_per_launch
    per = hip_lib.dcf_eval_range_wide_points_per_launch(nb, lam)
    assert per == PER
    for K in KS:
        for c in _counts(nb):
            keys = f(nb, lam, K, c)
            h = hip_lib.dcf_eval_range_wide_multikey_subtree_levels(nb, K, c)
            assert keys == keys_rule(nb, K, c), (nb, lam, K, c, keys)
            assert 1 <= keys <= 4096, (nb, lam, K, c, keys)
            span = ((c >> h) + 2) << h
            if keys > 1:
                assert keys * span <= per, (nb, lam, K, c, keys)
                assert keys * -(-c // 4096) <= 32768 and 4 * keys * 8 * nb < 1 << 32
                # and no smaller than it has to be
                assert keys == 4096 or (keys + 1) * span > per, (nb, lam, K, c, keys)
            if c > 32768:
                assert keys == 1, (nb, lam, K, c, keys)


def test_keys_per_launch_values(hip_lib):
    f = hip_lib.dcf_eval_range_wide_keys_per_launch
    assert f(1, 32, 4099, 64) == 4096                    # 96 leaves per key: the key bound
    assert f(1, 128, 1 << 16, 256) == 4096               # 384 leaves per key
    assert f(2, 32, 4096, 1000) == (1 << 22) // ((7 + 2) << 7) == 3640
    assert f(4, 48, 2, (1 << 12) + 77) == (1 << 22) // ((16 + 2) << 8) == 910
    assert f(4, 32, 2, 32768) == (1 << 22) // ((128 + 2) << 8) == 126
    assert f(4, 32, 2, 32768 + 5) == 1
    assert f(4, 32, 2, 1 << 30) == 1
    for args in ((0, 32, 5, 100), (17, 32, 5, 100), (2, 32, 0, 100), (2, 16, 5, 100), (2, 0, 5, 100), (2, 32, 5, 0)):
        assert f(*args) == 0, args


def test_argument_checks_without_gpu(hip_lib):
    """The entry point's checks on the shapes of this path (N <= 16): they return before the prg is
    looked at, so nothing is launched."""
    x0 = ctypes.create_string_buffer(16)
    buf = ctypes.create_string_buffer(64)
    f = hip_lib.dcf_eval_range_multikey_device
    assert f(None, 2, 3, 0, buf, buf, x0, 100, buf, None) == -1  # null prg
    fake = ctypes.cast(buf, ctypes.c_void_p)  # never dereferenced: the checks below come first
    assert f(fake, 0, 3, 0, buf, buf, x0, 100, buf, None) == -4   # n_bytes == 0
    assert f(fake, 2, 3, 2, buf, buf, x0, 100, buf, None) == -1   # bad party
    assert f(fake, 2, 3, -1, buf, buf, x0, 100, buf, None) == -1
    assert f(fake, 2, 3, 0, None, buf, x0, 100, buf, None) == -1
    assert f(fake, 2, 3, 0, buf, None, x0, 100, buf, None) == -1
    assert f(fake, 2, 3, 0, buf, buf, None, 100, buf, None) == -1
    assert f(fake, 2, 0, 0, buf, buf, x0, 100, None, None) == 0   # no keys: nothing to do
    assert f(fake, 2, 3, 0, buf, buf, x0, 0, None, None) == 0     # no points
    assert f(fake, 2, 3, 0, buf, buf, x0, 100, None, None) == -1  # null ys with work to do
    assert f(fake, 2, 3, 0, buf, buf, (ctypes.c_char * 2)(0xFF, 0xF0), 17, buf, None) == -1  # x0 + count > 2^16
    assert f(fake, 1, 67, 0, buf, buf, (ctypes.c_char * 1)(1), 256, buf, None) == -1


def test_mirrors():
    import dcf_amd
    from dcf_amd import _lib
    for name in ("range_wide_multikey_subtree_levels", "range_wide_keys_per_launch"):
        assert callable(getattr(dcf_amd.DcfImpl, name))
    hpp = open(os.path.join(ROOT, "include", "dcf.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "dcf-hip", "src", "lib.rs")).read()
    for name in ("dcf_eval_range_wide_multikey_subtree_levels", "dcf_eval_range_wide_keys_per_launch"):
        assert name in _lib.EXPORTS and name in hpp and name in rs, name


def test_python_mirror_values(hip_lib):
    """DcfImpl passes its own N and LAMBDA; no prg is touched."""
    import dcf_amd

    class NoPrg:
        lam = 128
    d = object.__new__(dcf_amd.DcfImpl)
    d.n_bytes, d.lam, d.prg = 1, 128, NoPrg()
    assert d.range_wide_multikey_subtree_levels(67, 256) == 6
    assert d.range_wide_keys_per_launch(1 << 16, 256) == 4096
    d.lam = 16
    assert d.range_wide_keys_per_launch(1 << 16, 256) == 0
