"""Multi-key range eval over the Hirose PRG at LAMBDA >= 32, N <= 16 on the GPU: one tree expansion
over the keys of a launch group (kernels_range_wide.h under the per-lane key policy) against the
CPU oracle on the points (x0 + i).to_bytes(N, "big"), bit for bit, on keys from the oracle's gen
packed into the K-key layout.  The keys of a case have alphas inside the range, outside it and on
both of its edges (_alpha) and alternating bounds; both parties run; 64 sentinel rows sit on either
side of ys; the parties' outputs must reconstruct every key's comparison function on every row;
every checked key is compared with eval_range_device of that key alone; and the AES-256 block count
of the call (dcf_prg_last_eval_blocks) must equal, exactly,
  sum over launch groups of keys * nroots * (4 (8N - h) + 4 (2^h - 1)),   4 * 8N * K * count at h = 0.

The shapes are the smallest that reach each stage; the first two fail on the key-by-key path this
one replaces, which walks every point from the root below 2^12 points per key."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_range_gpu import PAD, SENTINEL, _cwb, _dev, _points, _prgs, _sample
from tests.test_range_multikey_gpu import _alpha, _cwbk, _nroots
from tests.test_range_points_gpu import _check_rec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


def tree_blocks(nb, x0, count, h, keys):
    return keys * _nroots(x0, count, h) * (4 * (8 * nb - h) + 4 * ((1 << h) - 1))


def expected_blocks(d, nb, K, x0, count):
    """The formula of include/dcf_hip.h from the two arithmetic functions."""
    h, per = d.range_wide_multikey_subtree_levels(K, count), d.range_wide_keys_per_launch(K, count)
    if h == 0:
        return 4 * 8 * nb * K * count
    if count > 32768:  # the keys one after another, in groups of points
        pts = d.range_wide_points_per_launch()
        return K * sum(tree_blocks(nb, x0 + o, min(pts, count - o), h, 1) for o in range(0, count, pts))
    return sum(tree_blocks(nb, x0, count, h, min(per, K - k0)) for k0 in range(0, K, per))


def make_keys(P, nb, lam, x0, count, K, rng):
    oks, alphas, betas, seeds = [], [], [], []
    bounds = [(k // 2 + k) % 2 for k in range(K)]
    for k in range(K):
        a = _alpha(k, nb, x0, count, rng)
        beta, sd = rng.bytes(lam), [rng.bytes(lam), rng.bytes(lam)]
        oks.append(O.gen(P, a.to_bytes(nb, "big"), beta, sd[0], sd[1], bounds[k]))
        alphas.append(a)
        betas.append(beta)
        seeds.append(sd)
    return oks, alphas, betas, seeds, bounds


def check_rec_all(rec, betas, alphas, bounds, x0, count):
    """rec = y0 ^ y1, (K, count, lam) on the device: beta * [x < alpha] or [x > alpha] on every row of every key."""
    import torch
    K, lam = rec.shape[0], rec.shape[2]
    off = torch.tensor([a - x0 for a in alphas], dtype=torch.float64, device="cuda").clamp(-1, count)[:, None]
    idx = torch.arange(count, dtype=torch.float64, device="cuda")[None, :]
    lt = torch.tensor([b == 0 for b in bounds], device="cuda")[:, None]
    on = torch.where(lt, idx < off, idx > off)
    bt = _dev(b"".join(betas)).view(K, 1, lam)
    want = torch.where(on[:, :, None], bt, torch.zeros_like(bt))
    bad = (rec != want).any(dim=2).nonzero()
    assert bad.numel() == 0, ("reconstruction", "first mismatching (key, i)", bad[:8].tolist())


def launch(d, b, cwb, s0, x0, count, K, lam):
    """One call into a guarded buffer; returns (buffer, ys view)."""
    import torch
    buf = torch.full((K * count + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
    y = d.eval_range_multikey_device(bool(b), cwb, s0, x0, count, ys=buf[PAD:PAD + K * count].view(K, count, lam))
    return buf, y


def intact(buf, K, count):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + K * count:] == SENTINEL).all())


def run_mk(dcf, nb, lam, x0, count, K, seed, h, blocks=None, check_keys=None, single_blocks=False):
    """K fresh oracle keys, both parties.  h: the height the call must take; blocks: its block count
    when the docstring of the test states it (else the formula); check_keys: the keys compared with
    the oracle and the single-key call (default: all).  Returns the DcfImpl and the block count."""
    import torch
    rng = np.random.default_rng(seed)
    prg, P = _prgs(dcf, "hirose", lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    assert d.range_wide_multikey_subtree_levels(K, count) == h, (nb, K, count)
    want_blocks = expected_blocks(d, nb, K, x0, count)
    if blocks is not None:
        assert want_blocks == blocks, (want_blocks, blocks)
    oks, alphas, betas, seeds, bounds = make_keys(P, nb, lam, x0, count, K, rng)
    cwb = _dev(_cwbk(oks, nb, lam))
    rows = _sample(count, rng)
    xs = _points(nb, x0, rows)
    rows_dev = torch.from_numpy(rows).cuda()
    check_keys = range(K) if check_keys is None else check_keys
    ys, got_blocks = [], None
    for b in (0, 1):
        s0 = _dev(b"".join(sd[b] for sd in seeds)).view(K, lam)
        buf, y = launch(d, b, cwb, s0, x0, count, K, lam)
        torch.cuda.synchronize()
        assert y.shape == (K, count, lam)
        assert intact(buf, K, count), ("neighbours of ys written", nb, lam, x0, count, K, b)
        got_blocks = prg.last_eval_blocks()
        print(f"N={nb} lam={lam} K={K} count={count} h={h}: {got_blocks} blocks = {got_blocks / (K * count):.3f} per output")
        assert got_blocks == want_blocks, (got_blocks, want_blocks)
        single = 0
        for k in check_keys:
            got = y[k][rows_dev].cpu().numpy()
            want = O.eval_(P, b, oks[k], seeds[k][b], xs, nthreads=8)
            bad = np.flatnonzero((got[:, :32] != want[:, :32]).any(axis=1))
            assert bad.size == 0, ("bytes [0,32)", nb, lam, hex(x0), count, K, "key", k, "party", b, "first mismatching i", rows[bad[:8]])
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, ("bytes [32,lam)", nb, lam, hex(x0), count, K, "key", k, "party", b, "first mismatching i", rows[bad[:8]])
            yk = d.eval_range_device(bool(b), _dev(_cwb(oks[k])), _dev(seeds[k][b]), x0, count)
            assert torch.equal(y[k], yk), ("single-key call", k, b)
            if single_blocks:
                torch.cuda.synchronize()
                single += prg.last_eval_blocks()
        if single_blocks:
            assert got_blocks == single, (got_blocks, single)
        ys.append(y)
    check_rec_all(ys[0] ^ ys[1], betas, alphas, bounds, x0, count)
    return d, got_blocks


def test_tree_below_2_12_points_paired_slot_tail(dcf):
    """N = 1, LAMBDA = 128, the whole domain, 67 keys: h = 6, 4 roots per key, the levels below them
    and the paired-slot tail for bytes [32, 128).  67 * 4 * (4 * 2 + 4 * 63) = 69 680 blocks; the
    key-by-key path walks every point: 4 * 8 * 256 * 67 = 548 864."""
    run_mk(dcf, 1, 128, 0, 256, 67, 5100, h=6, blocks=69680)


def test_no_t_vectors_both_edge_blocks_clipped(dcf):
    """N = 2, LAMBDA = 32, 1000 points from an odd x0, 5 keys: h = 7, blocks of 128 leaves, the first
    and the last clipped.  The key-by-key path needs 64 blocks per output, this one under 5."""
    x0, count, K = 0x1F37, 1000, 5
    _, blocks = run_mk(dcf, 2, 32, x0, count, K, 5101, h=7, blocks=K * _nroots(x0, count, 7) * (4 * 9 + 4 * 127))
    assert blocks < 5 * K * count


def test_four_bit_tail_bits_across_a_word_and_carry_across_the_limb(dcf):
    """N = 16, LAMBDA = 48, 65 points from 2^64 - 33, 64 keys: 4160 outputs in all, h = 4.  The root
    prefixes carry across the 64-bit limb; w0 = 7, so the subtree's rows 125 .. 128 fall into words
    7 and 8 of the t-vector; the 4-bit tail writes bytes [32, 48)."""
    d, _ = run_mk(dcf, 16, 48, (1 << 64) - 33, 65, 64, 5102, h=4)
    assert (128 - 4 + 1) >> 4 == 7 and 128 >> 4 == 8


def test_leaf_mode_over_several_keys(dcf):
    """N = 2, LAMBDA = 128, 3 keys x 63 points: h = 0, the roots kernel walks the 189 (key, point) pairs."""
    run_mk(dcf, 2, 128, 0x0FE1, 63, 3, 5103, h=0, blocks=4 * 16 * 3 * 63)


@pytest.mark.parametrize("K,count,h", [(64, 63, 0), (63, 65, 0), (64, 64, 4)])
def test_both_sides_of_the_thresholds(dcf, K, count, h):
    """N = 2, LAMBDA = 32: under 64 points per key, under 2^12 outputs in all, and exactly at both."""
    run_mk(dcf, 2, 32, 0x2A55, count, K, 5104 + K + count, h=h)


def test_count_at_least_2_12_keeps_the_single_key_blocks(dcf):
    """N = 4, LAMBDA = 48, 2 keys x (2^12 + 77) points from an odd x0: the single-key height 8, and
    exactly the blocks of the two single-key calls."""
    run_mk(dcf, 4, 48, 0x0123457, (1 << 12) + 77, 2, 5105, h=8, single_blocks=True)


def test_key_groups(dcf):
    """N = 1, LAMBDA = 32, 64 points, 4099 keys: a launch group holds 4096, so the last 3 keys are a
    group of their own, at a 64-bit key offset.  Oracle and single-key call on the keys on both sides
    of the boundary, key 0 and 32 sampled keys; reconstruction on all; the blocks of both groups."""
    K, count, x0 = 4099, 64, 0x55
    rng = np.random.default_rng(5106)
    keys = sorted({0, *range(4090, 4099), *(int(k) for k in rng.integers(1, 4090, size=32))})
    d, blocks = run_mk(dcf, 1, 32, x0, count, K, 5106, h=4, check_keys=keys)
    assert d.range_wide_keys_per_launch(K, count) == 4096 == K - 3
    assert blocks == tree_blocks(1, x0, count, 4, 4096) + tree_blocks(1, x0, count, 4, 3)


def test_one_key_above_32768_points(dcf):
    """N = 4, LAMBDA = 32, 2 keys x (32768 + 5) points: the keys run one after another through the
    single-key kernels, each read in place from the 2-key block."""
    d, _ = run_mk(dcf, 4, 32, 0x00ABCDE, 32768 + 5, 2, 5107, h=8, single_blocks=True)
    assert d.range_wide_keys_per_launch(2, 32768 + 5) == 1 and d.range_wide_keys_per_launch(2, 32768) > 1


def test_long_lived_prg(dcf):
    """One prg at LAMBDA = 128, N = 2: the multi-key range (67 keys x 256), eval_device and
    eval_range_device of 5000 points (a single-key digest and workspace in between), then the
    multi-key range again with 200 keys on another stream — the digest and the workspace grow again.
    Nothing waits until the end; every output is then compared with the oracle."""
    import torch
    nb, lam, count, x0 = 2, 128, 256, 0x3F01
    rng = np.random.default_rng(5108)
    prg, P = _prgs(dcf, "hirose", lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    b = 1
    mk = []
    for K in (67, 200):
        oks, _, _, seeds, _ = make_keys(P, nb, lam, x0, count, K, rng)
        mk.append((K, oks, seeds, _dev(_cwbk(oks, nb, lam)), _dev(b"".join(sd[b] for sd in seeds)).view(K, lam)))
    m = 5000
    ok1, _, _, seeds1, _ = make_keys(P, nb, lam, 1000, m, 1, rng)
    cwb1, s1 = _dev(_cwb(ok1[0])), _dev(seeds1[0][b])
    xs_pts = np.frombuffer(rng.bytes(m * nb), np.uint8).reshape(m, nb)
    xs_dev = torch.from_numpy(xs_pts.copy()).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()  # the inputs are in place; from here on nothing waits

    K, _, _, cwb, s0 = mk[0]
    buf_a, y_a = launch(d, b, cwb, s0, x0, count, K, lam)
    buf_e = torch.full((m + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
    d.eval_device(bool(b), cwb1, s1, xs_dev, ys=buf_e[PAD:PAD + m])
    buf_r = torch.full((m + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
    d.eval_range_device(bool(b), cwb1, s1, 1000, m, ys=buf_r[PAD:PAD + m])
    K2, _, _, cwb2, s02 = mk[1]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        buf_b, y_b = launch(d, b, cwb2, s02, x0, count, K2, lam)
    torch.cuda.synchronize()

    xs = _points(nb, x0, range(count))
    for (K, oks, seeds, _, _), buf, y in ((mk[0], buf_a, y_a), (mk[1], buf_b, y_b)):
        assert intact(buf, K, count), K
        got = y.cpu().numpy()
        for k in range(K):
            want = O.eval_(P, b, oks[k], seeds[k][b], xs, nthreads=8)
            assert np.array_equal(got[k], want), (K, "key", k)
    for buf, pts in ((buf_e, xs_pts), (buf_r, _points(nb, 1000, range(m)))):
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + m:] == SENTINEL).all())
        want = O.eval_(P, b, ok1[0], seeds1[0][b], pts, nthreads=8)
        assert np.array_equal(buf[PAD:PAD + m].cpu().numpy(), want)
