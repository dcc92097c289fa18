"""Multi-key contiguous-range eval, the parts that need no GPU: the block-height rule of
dcf_eval_range_multikey_subtree_levels and the launch-group size of dcf_eval_range_keys_per_launch
(pure arithmetic), and argument checks that return before any device access."""
import ctypes

import pytest

NS = (1, 2, 4, 16)
KS = (1, 3, 1 << 12, 1 << 20)
COUNTS = sorted({c for e in range(0, 64) for c in ((1 << e) - 1, 1 << e, (1 << e) + 1) if 0 < c < 1 << 64})


def rule(nb: int, K: int, count: int) -> int:
    """include/dcf_hip.h: h = 0 when count < 64 or K * count < 2^12, else min(8N, 14, floor(log2 count) - 2)."""
    if count < 64 or K * count < 1 << 12:
        return 0
    return min(8 * nb, 14, count.bit_length() - 1 - 2)


@pytest.mark.parametrize("nb", NS)
@pytest.mark.parametrize("K", KS)
def test_height_rule_constraints_and_monotone(hip_lib, nb, K):
    prev = 0
    for c in COUNTS:
        if nb < 8 and c > 1 << (8 * nb):
            break
        h = hip_lib.dcf_eval_range_multikey_subtree_levels(nb, K, c)
        assert h == rule(nb, K, c), (nb, K, c, h)
        assert h == 0 or 4 <= h <= min(8 * nb, 14), (nb, K, c, h)
        if h:
            assert 4 * (1 << h) <= c, (nb, K, c, h)  # 2^h <= count / 4
        assert h >= prev, (nb, K, c, h, prev)
        prev = h


def test_height_rule_values(hip_lib):
    """The values themselves, so a change of rule() and library together still shows."""
    f = hip_lib.dcf_eval_range_multikey_subtree_levels
    assert f(1, 1 << 20, 256) == 6      # N = 1 whole domain: 4 blocks of 64 leaves per key
    assert f(2, 1 << 12, 1 << 16) == 14
    assert f(16, 1 << 12, 1 << 12) == 10
    assert f(16, 100, 15) == 0 and f(16, 100, 63) == 0 and f(16, 100, 64) == 4
    assert f(16, 3, 300) == 0           # 900 outputs in all: direct walk
    assert f(1, 1, 256) == 0 and f(1, 16, 256) == 6
    assert f(0, 5, 1000) == 0 and f(2, 0, 1000) == 0


@pytest.mark.parametrize("nb", NS)
@pytest.mark.parametrize("K", KS)
def test_keys_per_launch(hip_lib, nb, K):
    for c in COUNTS:
        if nb < 8 and c > 1 << (8 * nb):
            break
        per = hip_lib.dcf_eval_range_keys_per_launch(nb, K, c)
        h = hip_lib.dcf_eval_range_multikey_subtree_levels(nb, K, c)
        assert per >= 1, (nb, K, c)
        one = ((c >> h) + 2) << h  # the most leaves one key can expand
        if one <= 1 << 28:
            assert per * one <= 1 << 28, (nb, K, c, per)
            assert (per + 1) * one > 1 << 28, (nb, K, c, per)  # and no smaller than it has to be
        else:
            assert per == 1


def test_keys_per_launch_16_bit_domain(hip_lib):
    for K in (1, 1 << 12, (1 << 12) + 1, 1 << 20):
        assert 1 <= hip_lib.dcf_eval_range_keys_per_launch(2, K, 1 << 16) <= 1 << 12


def test_argument_checks_without_gpu(hip_lib):
    x0 = ctypes.create_string_buffer(16)
    buf = ctypes.create_string_buffer(64)
    f = hip_lib.dcf_eval_range_multikey_device
    assert f(None, 16, 1, 0, buf, buf, x0, 1, buf, None) == -1  # null prg
    fake = ctypes.cast(buf, ctypes.c_void_p)  # never dereferenced: the checks below come first
    assert f(fake, 0, 1, 0, buf, buf, x0, 1, buf, None) == -4   # n_bytes == 0
    assert f(fake, 16, 1, 2, buf, buf, x0, 1, buf, None) == -1  # bad party
    assert f(fake, 16, 1, 0, None, buf, x0, 1, buf, None) == -1
    assert f(fake, 16, 1, 0, buf, None, x0, 1, buf, None) == -1
    assert f(fake, 16, 1, 0, buf, buf, None, 1, buf, None) == -1
    assert f(fake, 257, 1, 0, buf, buf, x0, 1, buf, None) == -7  # N > 256
    assert f(fake, 16, 0, 0, buf, buf, x0, 1, None, None) == 0   # no keys: nothing to do
    assert f(fake, 16, 1, 0, buf, buf, x0, 0, None, None) == 0   # no points
    assert f(fake, 16, 1, 0, buf, buf, x0, 1, None, None) == -1  # null ys with work to do
    hi = (ctypes.c_char * 16)(*([0xFF] * 16))
    assert f(fake, 16, 1, 0, buf, buf, hi, 2, buf, None) == -1   # x0 + count > 2^128
    assert f(fake, 1, 1, 0, buf, buf, (ctypes.c_char * 1)(200), 57, buf, None) == -1


def test_python_mirror_has_the_entry_points():
    import dcf_amd
    for name in ("eval_range_multikey_device", "range_multikey_subtree_levels", "range_keys_per_launch"):
        assert callable(getattr(dcf_amd.DcfImpl, name))
