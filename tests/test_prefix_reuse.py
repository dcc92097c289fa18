"""Policy arithmetic of the cross-call shared-prefix table (include/dcf_hip.h): when a table is
deepened and how deep it may grow, through the helpers the library itself calls.  No GPU."""
from fractions import Fraction


def _calls(depth, m):
    """ceil(2^(D+1) / (1.257 m)), exactly."""
    q = Fraction(2 ** (depth + 1) * 1000, 1257 * m)
    return max(1, -(-q.numerator // q.denominator))


def test_deepen_thresholds(hip_lib):
    f = hip_lib.dcf_prefix_deepen_calls
    m = 1 << 28
    assert [f(d, m) for d in (27, 28, 29, 30)] == [1, 2, 4, 7]
    for m in (1, 3, 524_289, (1 << 20) - 1000, 1 << 24, (1 << 28) + 5, 1 << 33):
        for d in range(0, 31):
            assert f(d, m) == _calls(d, m), (d, m)
    # a level's pay-back time doubles with the depth, and a larger batch pays back sooner
    assert f(20, 1 << 19) == 4 and f(19, 1 << 19) == 2 and f(19, (1 << 20) - 1000) == 1
    # never: no points, no depth left below one x word
    assert f(27, 0) == 0 and f(31, 1 << 28) == 0 and f(-1, 1 << 28) == 0


def test_depth_caps(hip_lib):
    g = hip_lib.dcf_prefix_reuse_max_depth
    big = 1 << 50
    # depth <= 31 and < 8N
    assert g(16, big, 0) == 31 and g(4, big, 0) == 31 and g(2, big, 0) == 15 and g(0, big, 0) == 0
    # table bytes (32 * 2^D) <= 1/8 of the device: 288 GiB -> D = 30 (34.4 GB), 256 GiB -> 29... exactly at the edge
    assert g(16, 288 << 30, 0) == 30
    assert g(16, 8 * (32 << 30), 0) == 30 and g(16, 8 * (32 << 30) - 8, 0) == 29
    assert g(16, 8 * 32, 0) == 0 and g(16, 8 * 64, 0) == 1
    # the byte cap counts what a one-call build of that depth takes (table + build buffers):
    # 65 * 2^19 at D = 19 (include/dcf_hip.h), so a cap that admits the first call's table alone
    # admits no growth
    d19 = 32 * 2 ** 19 + 2 * 256 * 33 * 1024
    assert g(16, big, d19) == 19 and g(16, big, d19 - 1) == 18
    assert g(16, big, 40_000_000) == 19
    assert g(16, 8 * (32 << 20), 1 << 40) == 20  # the smaller of the two limits holds
