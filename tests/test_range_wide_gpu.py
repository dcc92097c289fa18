"""Range eval over the Hirose PRG at LAMBDA >= 32 on the GPU (kernels_range_wide.h):
dcf_eval_range_device / dcf_eval_range / dcf_eval_range_multikey_device against the CPU oracle on
the points (x0 + i).to_bytes(N, "big"), bit for bit, on keys from the oracle's gen.  Every case runs
both parties with alpha inside the range, checks the 64 sentinel rows on either side of ys, that the
parties' outputs reconstruct the comparison function on all rows, and the AES-256 block count of the
call (dcf_prg_last_eval_blocks):
  h > 0:  2 count <= blocks <= nroots (4 (8N - h) + 4 (2^h - 1))   per launch group
  h = 0:  2 * 8N * count <= blocks <= 4 * 8N * count

The shapes are the smallest that reach each stage: h = 0 (the roots kernel writes y and the
t-vectors), h = 8 (six breadth-first levels above the two-level register tail), h = 9 with both
edge blocks clipped, h = 14, no tail (LAMBDA = 32), the 4-bit tail (48) and the paired-slot tail
(128), and two launch groups."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_range_gpu import PAD, SENTINEL, _cwb, _dev, _points, _prgs, _sample, host_chunk, run_host_chunked
from tests.test_range_multikey_gpu import _cwbk, _nroots

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


def _odd_x0(seed, bits=128):
    return ((int.from_bytes(np.random.default_rng(seed).bytes(16), "big") >> 1) | 1) >> (128 - bits)


def _groups(x0, count, per):
    return [(x0 + o, min(per, count - o)) for o in range(0, count, per)]


def check_blocks(blocks, nb, x0, count, h, per):
    print(f"N={nb} count={count} h={h}: {blocks} blocks = {blocks / count:.3f} per output")
    n = 8 * nb
    if h == 0:
        assert 2 * n * count <= blocks <= 4 * n * count, (blocks, nb, count)
    else:
        upper = sum(_nroots(x, c, h) * (4 * (n - h) + 4 * ((1 << h) - 1)) for x, c in _groups(x0, count, per))
        assert 2 * count <= blocks <= upper, (blocks, upper)


def run_range(dcf, nb, lam, x0, count, seed, bounds=(0,), expect_h=None, extra_idx=None):
    """Both parties of a fresh key per bound, alpha inside [x0, x0 + count).  Returns the prg, the
    DcfImpl, the last key's (ok, oracle prg, cwb, seeds, party-1 ys on the device) and the last
    block count."""
    import torch
    rng = np.random.default_rng(seed)
    prg, P = _prgs(dcf, "hirose", lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    h = d.range_subtree_levels(count)
    if expect_h is not None:
        assert h == expect_h, (nb, count, h)
    per = d.range_wide_points_per_launch()
    assert per > 0
    last = blocks = None
    for bound in bounds:
        off = int(rng.integers(0, count))
        alpha, beta = (x0 + off).to_bytes(nb, "big"), rng.bytes(lam)
        seeds = [rng.bytes(lam), rng.bytes(lam)]
        ok = O.gen(P, alpha, beta, seeds[0], seeds[1], bound)
        cwb = _dev(_cwb(ok))
        idx = _sample(count, rng)
        if extra_idx is not None:
            idx = np.unique(np.concatenate([idx, extra_idx]))
        xs = _points(nb, x0, idx)
        ys = []
        for b in (0, 1):
            buf = torch.full((count + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
            y = d.eval_range_device(bool(b), cwb, _dev(seeds[b]), x0, count, ys=buf[PAD:PAD + count])
            torch.cuda.synchronize()
            assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + count:] == SENTINEL).all()), \
                ("neighbours of ys written", nb, lam, x0, count, b)
            blocks = prg.last_eval_blocks()
            check_blocks(blocks, nb, x0, count, h, per)
            got = y[torch.from_numpy(idx).cuda()].cpu().numpy()
            want = O.eval_(P, b, ok, seeds[b], xs, nthreads=8)
            bad = np.flatnonzero((got[:, :32] != want[:, :32]).any(axis=1))
            assert bad.size == 0, ("bytes [0,32)", nb, lam, hex(x0), count, bound, b, "first mismatching i", idx[bad[:8]])
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, ("bytes [32,lam)", nb, lam, hex(x0), count, bound, b, "first mismatching i", idx[bad[:8]])
            ys.append(y)
        rec = ys[0] ^ ys[1]
        bt = _dev(beta)
        lo, hi = (rec[:off], rec[off:]) if bound == 0 else (rec[off + 1:], rec[:off + 1])
        assert bool((lo == bt).all()) and not bool(hi.any()), ("reconstruction", nb, lam, hex(x0), count, bound)
        last = (ok, P, cwb, seeds, ys[1])
        del buf, rec
    return prg, d, last, blocks


@pytest.mark.parametrize("count", [4095, 4096])
def test_threshold_no_tail(dcf, count):
    """LAMBDA = 32: h steps from 0 (leaf mode: the roots kernel writes y) to 8 at 2^12 points."""
    run_range(dcf, 16, 32, _odd_x0(7), count, 3000 + count, bounds=(0, 1), expect_h=0 if count < 4096 else 8)


def test_work_bound(dcf):
    """LAMBDA = 32, N = 16, 2^17 + 3 points from an odd x0: h = 9, seven breadth-first levels, both
    edge blocks clipped; at most 258 (4 * 119 + 4 * 511) = 650 160 blocks, 4.96 per output.  The
    per-point head needs about 250 per output at this shape (2.5 per level below the shared prefix;
    measured on the parent commit: 245 at 2^16 points, 241 at 2^20), so this fails without the tree
    path."""
    count = (1 << 17) + 3
    *_, blocks = run_range(dcf, 16, 32, _odd_x0(17), count, 3017, bounds=(0, 1), expect_h=9)
    assert blocks <= 8 * count


def test_paired_slot_tail_and_carry_in_the_root_prefixes(dcf):
    """LAMBDA = 128 (k_eval_wide_tail2), N = 16, 2^12 + 77 points: x0 just below a multiple of
    2^(64 + 8), so the root prefixes x0 >> 8 carry across the 64-bit limb inside the range."""
    run_range(dcf, 16, 128, (5 << 72) - 700, (1 << 12) + 77, 3072, bounds=(0, 1), expect_h=8)


def test_four_bit_tail_whole_domain(dcf):
    """LAMBDA = 48 (k_eval_wide_tail), N = 2, the whole domain: h = 8, the last block ends the domain;
    every row against the oracle, and against eval_device on the materialised points."""
    import torch
    nb, lam, count = 2, 48, 1 << 16
    _, d, (ok, P, cwb, seeds, y1), _ = run_range(dcf, nb, lam, 0, count, 3048, bounds=(0, 1), expect_h=8,
                                                 extra_idx=np.arange(count))
    xs = torch.from_numpy(_points(nb, 0, range(count)).copy()).cuda()
    pointwise = d.eval_device(True, cwb, _dev(seeds[1]), xs)
    torch.cuda.synchronize()
    assert torch.equal(y1, pointwise)


def test_leaf_mode_with_a_tail(dcf):
    """LAMBDA = 128, N = 1, the whole domain: h = 0, the roots kernel writes the t-vectors itself."""
    run_range(dcf, 1, 128, 0, 256, 3001, bounds=(0, 1), expect_h=0)


def test_ten_levels(dcf):
    """LAMBDA = 32, N = 4, 2^22 + 5 points from an odd x0: h = 14."""
    run_range(dcf, 4, 32, 0x5A3C7B1, (1 << 22) + 5, 3022, expect_h=14)


def test_launch_group_split(dcf):
    """LAMBDA = 48, N = 4: 2^12 + 3 points more than one launch group holds; rows on both sides of the
    group boundary are compared, and the block count is the sum of both groups."""
    import dcf_amd
    rng = np.random.default_rng(3)
    prg, _ = _prgs(dcf_amd, "hirose", 48, rng)
    per = dcf_amd.DcfImpl(4, 48, prg).range_wide_points_per_launch()
    assert per == 1 << 22
    count = per + (1 << 12) + 3
    around = np.arange(per - 4096, per + 4096)
    run_range(dcf, 4, 48, 0x0123457, count, 3448, expect_h=14, extra_idx=around)


def test_host_entry_point(dcf):
    nb, lam, count = 16, 32, 70001
    rng = np.random.default_rng(3070)
    prg, P = _prgs(dcf, "hirose", lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    x0 = _odd_x0(3071)
    off = int(rng.integers(0, count))
    alpha, beta, seeds = (x0 + off).to_bytes(nb, "big"), rng.bytes(lam), [rng.bytes(lam), rng.bytes(lam)]
    ok = O.gen(P, alpha, beta, seeds[0], seeds[1], 0)
    cwb = _dev(_cwb(ok))
    h, per = d.range_subtree_levels(count), d.range_wide_points_per_launch()
    ys = []
    for b in (0, 1):
        k = dcf.cwb_to_share(_cwb(ok), nb, lam, [seeds[b]])
        y = d.eval_range(bool(b), k, x0, count)
        check_blocks(prg.last_eval_blocks(), nb, x0, count, h, per)
        ydev = d.eval_range_device(bool(b), cwb, _dev(seeds[b]), x0, count)
        assert np.array_equal(y, ydev.cpu().numpy()), b
        ys.append(y)
    rec = ys[0] ^ ys[1]
    assert (rec[:off] == np.frombuffer(beta, np.uint8)).all() and not rec[off:].any()


@pytest.mark.parametrize("extra", [4099, 5])
def test_host_entry_point_chunked(dcf, extra):
    """LAMBDA = 48, N = 4: a chunk is 2 796 202 outputs, no multiple of a block of 2^13, so the second
    chunk (4099 or 5 points) starts mid-block; each chunk is one launch group.  One party."""
    nb, lam = 4, 48
    count = host_chunk(lam) + extra
    assert host_chunk(lam) == 2796202
    per = dcf.DcfImpl(nb, lam, _prgs(dcf, "hirose", lam, np.random.default_rng(3))[0]).range_wide_points_per_launch()
    assert per >= host_chunk(lam)
    run_host_chunked(dcf, "hirose", lam, nb, 0x0123457, count, 3500 + extra, walk=4, node=4, bound=extra % 2, group=per)


def test_multikey_equals_single_key_calls(dcf):
    """eval_range_multikey_device at LAMBDA = 32 goes key by key through the single-key path."""
    import torch
    nb, lam, K, count, x0 = 2, 32, 3, 5000, 0x1F37
    rng = np.random.default_rng(3300)
    prg, P = _prgs(dcf, "hirose", lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    oks, seeds = [], []
    for k in range(K):
        sd = [rng.bytes(lam), rng.bytes(lam)]
        alpha = x0 + int(rng.integers(0, count))
        oks.append(O.gen(P, alpha.to_bytes(nb, "big"), rng.bytes(lam), sd[0], sd[1], k % 2))
        seeds.append(sd)
    cwbk = _dev(_cwbk(oks, nb, lam))
    h, per = d.range_subtree_levels(count), d.range_wide_points_per_launch()
    assert h == 8
    xs = _points(nb, x0, range(count))
    for b in (0, 1):
        s0 = _dev(b"".join(sd[b] for sd in seeds)).view(K, lam)
        buf = torch.full((K * count + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
        y = d.eval_range_multikey_device(bool(b), cwbk, s0, x0, count, ys=buf[PAD:PAD + K * count].view(K, count, lam))
        torch.cuda.synchronize()
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + K * count:] == SENTINEL).all())
        blocks = prg.last_eval_blocks()
        single = 0
        for k in range(K):
            yk = d.eval_range_device(bool(b), _dev(_cwb(oks[k])), _dev(seeds[k][b]), x0, count)
            torch.cuda.synchronize()
            single += prg.last_eval_blocks()
            check_blocks(prg.last_eval_blocks(), nb, x0, count, h, per)
            assert torch.equal(y[k], yk), (k, b)
            assert np.array_equal(yk.cpu().numpy(), O.eval_(P, b, oks[k], seeds[k][b], xs, nthreads=8)), (k, b)
        assert blocks == single, (blocks, single)
