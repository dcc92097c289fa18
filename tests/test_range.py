"""Contiguous-range eval, the parts that need no GPU: the block-height rule of
dcf_eval_range_subtree_levels (pure arithmetic) and argument checks that return before any
device access."""
import ctypes

import pytest

NS = (1, 4, 16)
COUNTS = (1, 2, 33, (1 << 12) + 1, (1 << 17) + 3, 1 << 28)


def rule(nb: int, count: int) -> int:
    """include/dcf_hip.h: h = 0 below 2^12 points, else min(8N, 14, max(8, floor(log2 count) - 8))."""
    if count < 1 << 12:
        return 0
    return min(8 * nb, 14, max(8, count.bit_length() - 1 - 8))


@pytest.mark.parametrize("nb", NS)
def test_subtree_levels_matches_documented_rule(hip_lib, nb):
    for count in COUNTS:
        assert hip_lib.dcf_eval_range_subtree_levels(nb, count) == rule(nb, count), (nb, count)
    # the values themselves, so a change of rule() and library together still shows
    want = {1: (0, 0, 0, 8, 8, 8), 4: (0, 0, 0, 8, 9, 14), 16: (0, 0, 0, 8, 9, 14)}[nb]
    assert tuple(hip_lib.dcf_eval_range_subtree_levels(nb, c) for c in COUNTS) == want


@pytest.mark.parametrize("nb", NS)
def test_subtree_levels_bounded_and_monotone(hip_lib, nb):
    counts = sorted({c for e in range(0, 64) for c in ((1 << e) - 1, 1 << e, (1 << e) + 1) if 0 < c < 1 << 64})
    prev = 0
    for c in counts:
        h = hip_lib.dcf_eval_range_subtree_levels(nb, c)
        assert 0 <= h <= 8 * nb, (nb, c, h)
        assert h >= prev, (nb, c, h, prev)
        prev = h


def test_subtree_levels_work_bound_shape(hip_lib):
    """The shape the GPU work-bound test uses: any h in [9, log2(count) - 3] keeps the blocks per
    output under 3 there (2 for the tree, 2 (128 - h) / 2^h for the root paths, <= 4 * 2^h / count
    for the two clipped edge blocks)."""
    count = (1 << 17) + 3
    h = hip_lib.dcf_eval_range_subtree_levels(16, count)
    assert 9 <= h <= 14
    assert 2 + 2 * (128 - h) / 2 ** h + 4 * 2 ** h / count < 3


def test_introspection_exports_match_recorded_table(hip_lib, golden):
    """The six exports read a plan (plan_range); tests/golden/range_plan_table.json holds what they
    returned over this grid when each computed its own arithmetic, recorded from that build."""
    t = golden("range_plan_table")
    g = t["grid"]
    assert g == {"n_bytes": [1, 2, 4, 16, 17], "count": [1, 63, 64, 4095, 4096, 1 << 20, (1 << 28) + 1],
                 "num_keys": [1, 2, 41, 4096], "lambda": [16, 32, 64]}
    assert len(t["rows"]) == len(g["n_bytes"]) * len(g["count"]) * len(g["num_keys"]) * len(g["lambda"])
    assert {tuple(r[:4]) for r in t["rows"]} == {(nb, c, K, lam) for nb in g["n_bytes"] for c in g["count"]
                                                  for K in g["num_keys"] for lam in g["lambda"]}
    for nb, c, K, lam, *want in t["rows"]:
        got = [hip_lib.dcf_eval_range_subtree_levels(nb, c),
               hip_lib.dcf_eval_range_wide_points_per_launch(nb, lam),
               hip_lib.dcf_eval_range_multikey_subtree_levels(nb, K, c),
               hip_lib.dcf_eval_range_keys_per_launch(nb, K, c),
               hip_lib.dcf_eval_range_wide_multikey_subtree_levels(nb, K, c),
               hip_lib.dcf_eval_range_wide_keys_per_launch(nb, lam, K, c)]
        assert got == want, (nb, c, K, lam, t["columns"][4:])


def test_range_argument_checks_without_gpu(hip_lib):
    assert hip_lib.dcf_eval_range_subtree_levels(0, 100) == 0
    x0 = ctypes.create_string_buffer(16)
    assert hip_lib.dcf_eval_range_device(None, 16, 0, None, None, x0, 1, None, None) == -1
    assert hip_lib.dcf_eval_range(None, 16, 0, None, 0, None, x0, 1, None, 16) == -1


def test_python_mirror_rejects_bad_x0():
    import dcf_amd

    class FakePrg:
        lam = 16

    d = dcf_amd.DcfImpl(2, 16, FakePrg())
    assert d._x0(65000) == (65000).to_bytes(2, "big")
    assert d._x0(b"\x01\x02") == b"\x01\x02"
    with pytest.raises(dcf_amd.DcfError):
        d._x0(1 << 16)
    with pytest.raises(ValueError):
        d._x0(b"\x01\x02\x03")
