"""Seeded random-shape sweep of range eval (GPU), the sibling of tests/test_gpu_fuzz.py for
dcf_eval_range_device and dcf_eval_range_multikey_device: the dispatch splits on the PRG, LAMBDA,
N <= 16 or not, the two height rules, K and the launch groups, and the hand-picked cases name only
some combinations.  Every case is checked bit for bit against the CPU oracle on the points
(x0 + i).to_bytes(N, "big") — every row up to 8193 points, _sample rows above — with both parties,
the sentinel rows on either side of ys and reconstruction on all rows (the runners of
tests/test_range_points_gpu.py).  The shapes come from a fixed seed, so a failure names a
reproducible case id."""
import os

import numpy as np
import pytest

from tests.test_range_points_gpu import LOW, run_mk, run_range

pytestmark = pytest.mark.gpu

LAMS = [16, 16, 16, 32, 48, 128]
COUNTS = [1, 63, 64, 65, 1000, 4095, 4096, 5000, 8193, 70001]
X0S = ["random", "aligned", "domain-end", "limb64", "zero"]
ALPHAS = ["inside", "below", "above", "first", "last"]
MAX_OUTPUTS = 1 << 18  # K * count of a multi-key case

# Extended sweeps (one-off GPU runs; the default is the suite's fixed list): DCF_RANGE_FUZZ_CASES /
# DCF_RANGE_FUZZ_MK_CASES cases from DCF_RANGE_FUZZ_SEED / DCF_RANGE_FUZZ_MK_SEED.
_ENV = os.environ.get


def _big(rng, nbytes) -> int:
    return int.from_bytes(rng.bytes(nbytes), "big")


def _shape(rng, K):
    """(lam, nb, kind, count, x0, x0 kind): count clipped to the domain and to MAX_OUTPUTS / K."""
    lam = int(rng.choice(LAMS))
    nb = int(rng.integers(1, 21))
    kind = "mmo" if rng.random() < 0.25 else "hirose"
    dom = 1 << (8 * nb)
    count = min(int(rng.choice([c for c in COUNTS if K * c <= MAX_OUTPUTS])), dom)
    how = str(rng.choice(X0S))
    if nb > 16 and count > 1 and rng.random() < 1 / 3:  # the low 128 bits wrap inside the range
        how = "wrap"
        x0 = ((_big(rng, nb - 16) >> 1) << 128) + LOW - int(rng.integers(1, count))
    elif how == "aligned":  # a multiple of the tallest block, 2^14, so of 2^h under either height rule
        a = min(14, 8 * nb)
        x0 = (_big(rng, nb + 1) % (((dom - count) >> a) + 1)) << a
    elif how == "domain-end":
        x0 = dom - count
    elif how == "limb64" and nb > 8:  # the range crosses the 64-bit limb of the 128-bit add
        x0 = (1 << 64) - (count + 1) // 2
    elif how == "zero":
        x0 = 0
    else:
        how = "random"
        x0 = _big(rng, nb + 1) % (dom - count + 1)
    assert 0 <= x0 and x0 + count <= dom
    return lam, nb, kind, count, x0, how


def _alpha_off(rng, where, x0, count, dom):
    """Row of alpha relative to x0: inside the range, below or above it, or on its first or last row."""
    if where == "below" and x0 > 0:
        return -1 - _big(rng, 40) % x0
    if where == "above" and x0 + count < dom:
        return count + _big(rng, 40) % (dom - x0 - count)
    if where == "first":
        return 0
    if where == "last":
        return count - 1
    return int(rng.integers(0, count))


def _cases(n=int(_ENV("DCF_RANGE_FUZZ_CASES", "48")), seed=int(_ENV("DCF_RANGE_FUZZ_SEED", "0xA27E"), 0)):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        lam, nb, kind, count, x0, how = _shape(rng, 1)
        where = str(rng.choice(ALPHAS))
        off = _alpha_off(rng, where, x0, count, 1 << (8 * nb))
        out.append((i, lam, nb, kind, int(rng.integers(0, 2)), count, x0, how, where, off))
    return out


def _mk_cases(n=int(_ENV("DCF_RANGE_FUZZ_MK_CASES", "24")), seed=int(_ENV("DCF_RANGE_FUZZ_MK_SEED", "0xA2BE"), 0)):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        K = int(rng.choice([1, 2, 3, 67]))
        out.append((i, K) + _shape(rng, K))
    return out


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


@pytest.mark.parametrize("case", _cases(),
                         ids=lambda c: f"c{c[0]}-lam{c[1]}-n{c[2]}-{c[3]}-b{c[4]}-m{c[5]}-x0{c[7]}-alpha{c[8]}")
def test_fuzz_range_vs_oracle(dcf, case):
    i, lam, nb, kind, bound, count, x0, _, _, off = case
    run_range(dcf, nb, x0, count, 0x5EED0 + i, bounds=(bound,), kind=kind, lam=lam, alpha_offs=(off,))


@pytest.mark.parametrize("case", _mk_cases(), ids=lambda c: f"k{c[0]}-K{c[1]}-lam{c[2]}-n{c[3]}-{c[4]}-m{c[5]}-x0{c[7]}")
def test_fuzz_range_multikey_vs_oracle(dcf, case):
    """Key k's alpha lies inside the range, outside it or on an edge and its bound alternates (run_mk);
    every key also against eval_range_device of that key alone."""
    i, K, lam, nb, kind, count, x0, _ = case
    run_mk(dcf, nb, x0, count, K, 0x3EED0 + i, kind=kind, lam=lam)
