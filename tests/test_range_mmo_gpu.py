"""Range eval over the Matyas-Meyer-Oseas AES-128 PRG on the GPU (kernels_range_mmo.h and the
RangeMmo instances of kernels_range.h), one key and K keys: dcf_eval_range_device / dcf_eval_range / dcf_eval_range_multikey_device against the CPU
oracle on the points (x0 + i).to_bytes(N, "big"), bit for bit, on keys from the oracle's gen over
OracleMmoPrg.  Every case evaluates both parties, checks the 64 sentinel rows on either side of ys,
that the parties' outputs reconstruct the comparison function on all rows, and the AES-128 block
count of the call: the per-point walk does not count, so a call that misses the tree path reports 0.

The shapes are the smallest that reach each stage: h = 0 (the roots kernel writes y), h = 4 (tail
straight from the roots), h = 8..10 (breadth-first levels) and h = 14 (ten levels)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_range_gpu import PAD, SENTINEL, _cwb, _dev, _points, _sample, host_chunk, run_host_chunked
from tests.test_range_multikey_gpu import _alpha, _cwbk, _nroots

pytestmark = pytest.mark.gpu

LAM = 16


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


def _prgs(dcf, rng):
    keys = [rng.bytes(16) for _ in range(4)]
    return dcf.Aes128MatyasMeyerOseasPrg(keys, LAM), O.OracleMmoPrg(keys, LAM)


def _odd_x0(seed):
    return (int.from_bytes(np.random.default_rng(seed).bytes(16), "big") >> 1) | 1


def check_blocks(blocks, nb, K, x0, count, h):
    """h = 0: every point walks 8N levels of 2 blocks.  h > 0: any expansion needs 2 per output; the
    three stages execute K nroots (2 (8N - h) + 4 (2^h - 1)), clipped leaves included."""
    print(f"N={nb} K={K} count={count} h={h}: {blocks} blocks = {blocks / (K * count):.3f} per output")
    if h == 0:
        assert blocks == 2 * 8 * nb * K * count, (blocks, nb, K, count)
    else:
        upper = K * _nroots(x0, count, h) * (2 * (8 * nb - h) + 4 * ((1 << h) - 1))
        assert 2 * K * count <= blocks <= upper, (blocks, upper)


def run_range(dcf, nb, x0, count, seed, bounds=(0,), expect_h=None):
    """Both parties of a fresh key per bound, alpha inside [x0, x0 + count).  Returns the prg, the
    DcfImpl, the last key's (cwb, party-1 seed, party-1 ys) on the device and the last block count."""
    import torch
    rng = np.random.default_rng(seed)
    prg, P = _prgs(dcf, rng)
    d = dcf.DcfImpl(nb, LAM, prg)
    h = d.range_subtree_levels(count)
    if expect_h is not None:
        assert h == expect_h, (nb, count, h)
    last = blocks = None
    for bound in bounds:
        off = int(rng.integers(0, count))
        alpha, beta = (x0 + off).to_bytes(nb, "big"), rng.bytes(LAM)
        seeds = [rng.bytes(LAM), rng.bytes(LAM)]
        ok = O.gen(P, alpha, beta, seeds[0], seeds[1], bound)
        cwb = _dev(_cwb(ok))
        idx = _sample(count, rng)
        xs = _points(nb, x0, idx)
        ys = []
        for b in (0, 1):
            buf = torch.full((count + 2 * PAD, LAM), SENTINEL, dtype=torch.uint8, device="cuda")
            y = d.eval_range_device(bool(b), cwb, _dev(seeds[b]), x0, count, ys=buf[PAD:PAD + count])
            torch.cuda.synchronize()
            assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + count:] == SENTINEL).all()), \
                ("neighbours of ys written", nb, x0, count, b)
            blocks = prg.last_eval_blocks()
            check_blocks(blocks, nb, 1, x0, count, h)
            got = y[torch.from_numpy(idx).cuda()].cpu().numpy()
            want = O.eval_(P, b, ok, seeds[b], xs, nthreads=8)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (nb, hex(x0), count, bound, b, "first mismatching i", idx[bad[:8]])
            ys.append(y)
        rec = ys[0] ^ ys[1]
        bt = _dev(beta)
        lo, hi = (rec[:off], rec[off:]) if bound == 0 else (rec[off + 1:], rec[:off + 1])
        assert bool((lo == bt).all()) and not bool(hi.any()), ("reconstruction", nb, hex(x0), count, bound)
        last = (cwb, _dev(seeds[1]), ys[1])
    return prg, d, last, blocks


def run_mk(dcf, nb, x0, count, K, seed, expect_h):
    """K fresh oracle keys with alphas inside, outside and on the edges of the range, both bounds,
    both parties; every index of every key against the oracle."""
    import torch
    rng = np.random.default_rng(seed)
    prg, P = _prgs(dcf, rng)
    d = dcf.DcfImpl(nb, LAM, prg)
    oks, alphas, betas, seeds = [], [], [], []
    bounds = [(k // 2 + k) % 2 for k in range(K)]
    for k in range(K):
        a = _alpha(k, nb, x0, count, rng)
        beta, sd = rng.bytes(LAM), [rng.bytes(LAM), rng.bytes(LAM)]
        oks.append(O.gen(P, a.to_bytes(nb, "big"), beta, sd[0], sd[1], bounds[k]))
        alphas.append(a)
        betas.append(beta)
        seeds.append(sd)
    cwb = _dev(_cwbk(oks, nb, LAM))
    idx = np.arange(count)
    xs = _points(nb, x0, idx)
    h = d.range_multikey_subtree_levels(K, count)
    assert h == expect_h, (nb, K, count, h)
    ys = []
    for b in (0, 1):
        s0 = _dev(b"".join(sd[b] for sd in seeds)).view(K, LAM)
        buf = torch.full((K * count + 2 * PAD, LAM), SENTINEL, dtype=torch.uint8, device="cuda")
        y = d.eval_range_multikey_device(bool(b), cwb, s0, x0, count, ys=buf[PAD:PAD + K * count].view(K, count, LAM))
        torch.cuda.synchronize()
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + K * count:] == SENTINEL).all()), \
            ("neighbours of ys written", nb, x0, count, K, b)
        check_blocks(prg.last_eval_blocks(), nb, K, x0, count, h)
        got = y.cpu().numpy()
        for k in range(K):
            want = O.eval_(P, b, oks[k], seeds[k][b], xs, nthreads=8)
            bad = np.flatnonzero((got[k] != want).any(axis=1))
            assert bad.size == 0, (nb, hex(x0), count, K, "key", k, "party", b, "first mismatching i", bad[:8])
        ys.append(y)
    rec = (ys[0] ^ ys[1]).cpu().numpy()
    for k in range(K):
        off = alphas[k] - x0
        m = idx < min(max(off, 0), count) if bounds[k] == 0 else idx > min(max(off, -1), count)
        bt = np.frombuffer(betas[k], np.uint8)
        assert (rec[k][m] == bt).all() and not rec[k][~m].any(), ("reconstruction", nb, hex(x0), count, "key", k)


# ---- one key ----

@pytest.mark.parametrize("count", [4095, 4096])
def test_direct_walk_to_tree_threshold(dcf, count):
    """h steps from 0 (the roots kernel writes y) to 8 (blocks of 256) at 2^12 points."""
    run_range(dcf, 16, _odd_x0(7), count, 2000 + count, bounds=(0, 1), expect_h=0 if count < 4096 else 8)


def test_many_blocks_unaligned_both_ends(dcf):
    """2^17 + 3 points: 257 or 258 blocks of 512 leaves, 5 breadth-first levels; at most
    258 * (2 * 119 + 4 * 511) = 588 756 blocks, 4.49 per output (the per-point walk: 256)."""
    count = (1 << 17) + 3
    *_, blocks = run_range(dcf, 16, _odd_x0(17), count, 2017, bounds=(0, 1), expect_h=9)
    assert blocks <= 5 * count


def test_ten_levels(dcf):
    run_range(dcf, 16, _odd_x0(22), (1 << 22) + 5, 2022, expect_h=14)


def test_carry_across_64_bit_boundary_in_the_root_prefixes(dcf):
    run_range(dcf, 16, (1 << 72) - 700, 5000, 2072, expect_h=8)


def test_straddling_the_midpoint(dcf):
    run_range(dcf, 16, (1 << 127) - 3000, 6000, 2127, expect_h=8)


def test_last_block_ends_the_domain(dcf):
    run_range(dcf, 16, (1 << 128) - 4500, 4500, 2128, expect_h=8)


def test_whole_domain_equals_full_domain_eval(dcf):
    import torch
    _, d, (cwb, s1, y1), _ = run_range(dcf, 2, 0, 1 << 16, 2002, expect_h=8)
    full = d.eval_full_domain_device(True, cwb, s1)
    torch.cuda.synchronize()
    assert torch.equal(y1, full)


def test_equals_eval_device_on_materialised_points(dcf):
    import torch
    nb, count, x0 = 8, 5000, (1 << 40) - 1234
    _, d, (cwb, s1, y1), _ = run_range(dcf, nb, x0, count, 2040, expect_h=8)
    xs = torch.from_numpy(_points(nb, x0, range(count)).copy()).cuda()
    pointwise = d.eval_device(True, cwb, s1, xs)
    torch.cuda.synchronize()
    assert torch.equal(y1, pointwise)


def test_host_entry_point(dcf):
    nb, count = 16, 70001
    rng = np.random.default_rng(2070)
    prg, P = _prgs(dcf, rng)
    d = dcf.DcfImpl(nb, LAM, prg)
    x0 = (int.from_bytes(rng.bytes(16), "big") >> 1) | 1
    off = int(rng.integers(0, count))
    alpha, beta, seeds = (x0 + off).to_bytes(nb, "big"), rng.bytes(LAM), [rng.bytes(LAM), rng.bytes(LAM)]
    ok = O.gen(P, alpha, beta, seeds[0], seeds[1], 0)
    xs = _points(nb, x0, range(count))
    ys = []
    for b in (0, 1):
        k = dcf.cwb_to_share(_cwb(ok), nb, LAM, [seeds[b]])
        y = d.eval_range(bool(b), k, x0, count)
        check_blocks(prg.last_eval_blocks(), nb, 1, x0, count, d.range_subtree_levels(count))
        assert np.array_equal(y, O.eval_(P, b, ok, seeds[b], xs, nthreads=8)), b
        ys.append(y)
    rec = ys[0] ^ ys[1]
    assert (rec[:off] == np.frombuffer(beta, np.uint8)).all() and not rec[off:].any()


def test_host_entry_point_chunked(dcf):
    """One chunk of 2^23 outputs and 3 points from an odd x0: the last chunk is 3 points at h = 14.
    One party."""
    run_host_chunked(dcf, "mmo", LAM, 16, _odd_x0(2071), host_chunk(LAM) + 3, 2071, walk=2, node=4, bound=1)


# ---- K keys ----

def test_multikey_whole_8_bit_domain(dcf):
    run_mk(dcf, 1, 0, 256, 67, 2100, expect_h=6)


def test_multikey_tail_straight_from_the_roots(dcf):
    """h = 4: no level launch between the roots and the tail."""
    run_mk(dcf, 2, 0x01F0, 64, 67, 2101, expect_h=4)


def test_multikey_unaligned_n16(dcf):
    run_mk(dcf, 16, _odd_x0(2102), 4101, 3, 2102, expect_h=10)


def test_multikey_unaligned_n4(dcf):
    run_mk(dcf, 4, 0x00FFF123, 3001, 3, 2103, expect_h=9)


@pytest.mark.parametrize("count,K", [(33, 200), (1000, 3)])
def test_multikey_direct_walk(dcf, count, K):
    """h = 0 by both clauses of the height rule: count below 64, and fewer than 2^12 outputs in all."""
    run_mk(dcf, 16, _odd_x0(count), count, K, 2200 + count, expect_h=0)
