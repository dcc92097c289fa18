"""Range fold on the GPU: dcf_eval_range_fold_device and dcf_eval_range_fold_multikey_device against
the CPU oracle's eval over the points, masked by the table and XORed in numpy.  Keys come from the
oracle's gen (alphas inside the range, outside it and on its edges, both bounds), both parties run,
`out` sits between 64 sentinel rows, the two parties' folds must XOR to the fold of beta & w[i] over
the points the comparison function selects (computed from alpha, beta and w alone), and on the fused
path the AES block count must equal that of the range call of the same shape.

The single-key h = 0 counts are 1 and 63 at N = 1 and 4095 at N = 2 (an 8-bit domain has 256 points)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_range_multikey_gpu import _alpha, _cwb1, _cwbk, _dev, _points, _prgs, _single_cwb

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 64, 0xA5


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


def _xor_rows(a):
    return np.bitwise_xor.reduce(a, axis=0) if len(a) else np.zeros(a.shape[1:], np.uint8)


def dev_fold(y):
    """XOR of the rows of a (n, lam) uint8 device tensor, by halving."""
    import torch
    y = y.view(torch.int64)
    acc = torch.zeros_like(y[0])
    n = y.shape[0]
    while n > 1:
        if n & 1:
            acc ^= y[n - 1]
        n //= 2
        y = y[:n] ^ y[n:2 * n]
    return (acc ^ y[0]).view(torch.uint8) if n else acc.view(torch.uint8)


def run_fold(dcf, nb, x0, count, K, seed, kind="hirose", lam=16, mask=True, multikey=None, expect_h=None,
             fused=None, prgs=None, prefill=SENTINEL):
    """K fresh oracle keys over [x0, x0 + count) and one table, both parties.  multikey: the K-key
    entry point (default: K > 1).  expect_h: the block height the shape must have.  fused: whether
    the call must report the range call's block count."""
    import torch
    rng = np.random.default_rng(seed)
    prg, P = prgs if prgs else _prgs(dcf, kind, lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    multikey = K > 1 if multikey is None else multikey
    h = d.range_multikey_subtree_levels(K, count) if multikey else d.range_subtree_levels(count)
    if expect_h is not None:
        assert h == expect_h, (nb, K, count, h)
    if fused is None:
        fused = lam == 16 and nb <= 16 and h > 0
    oks, alphas, betas, seeds = [], [], [], []
    bounds = [(k // 2 + k + seed) % 2 for k in range(K)]
    for k in range(K):
        a = _alpha(k + seed % 4, nb, x0, count, rng)
        beta, sd = rng.bytes(lam), [rng.bytes(lam), rng.bytes(lam)]
        oks.append(O.gen(P, a.to_bytes(nb, "big"), beta, sd[0], sd[1], bounds[k]))
        alphas.append(a)
        betas.append(beta)
        seeds.append(sd)
    cwb = _dev(_cwbk(oks, nb, lam)) if multikey else _dev(_cwb1(oks[0]))
    idx = np.arange(count)
    xs = _points(nb, x0, idx)
    w = rng.integers(0, 256, size=(count, lam), dtype=np.uint8) if mask else np.full((count, lam), 0xFF, np.uint8)
    w_d = torch.from_numpy(w).cuda() if mask else None
    outs = []
    for b in (0, 1):
        s0 = _dev(b"".join(sd[b] for sd in seeds)).view(K, lam)
        buf = torch.full((K + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
        buf[PAD:PAD + K] = prefill
        if multikey:
            got = d.eval_range_fold_multikey_device(bool(b), cwb, s0, x0, count, w_d, out=buf[PAD:PAD + K])
        else:
            got = d.eval_range_fold_device(bool(b), cwb, s0[0], x0, count, w_d, out=buf[PAD])
        torch.cuda.synchronize()
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + K:] == SENTINEL).all()), \
            ("neighbours of out written", nb, hex(x0), count, K, b)
        if fused:
            blocks = prg.last_eval_blocks()
            if multikey:
                d.eval_range_multikey_device(bool(b), cwb, s0, x0, count)
            else:
                d.eval_range_device(bool(b), cwb, s0[0], x0, count)
            torch.cuda.synchronize()
            want_blocks = prg.last_eval_blocks()
            print(f"N={nb} K={K} count={count} h={h}: {blocks} blocks, range call {want_blocks}")
            assert blocks == want_blocks and blocks > 0, (blocks, want_blocks)
        got = got.cpu().numpy().reshape(K, lam)
        for k in range(K):
            ys = O.eval_(P, b, oks[k], seeds[k][b], xs, nthreads=8)
            want = _xor_rows(ys & w)
            assert np.array_equal(got[k], want), (nb, hex(x0), count, K, "key", k, "party", b, got[k], want)
        outs.append(got)
    rec = outs[0] ^ outs[1]
    for k in range(K):
        off = alphas[k] - x0
        m = idx < min(max(off, 0), count) if bounds[k] == 0 else idx > min(max(off, -1), count)
        want = _xor_rows(w[m] & np.frombuffer(betas[k], np.uint8))
        assert np.array_equal(rec[k], want), ("reconstruction", nb, hex(x0), count, "key", k)
    return prg, P, d


# ---- one key, Hirose, lambda = 16 ----

@pytest.mark.parametrize("mask", [True, False])
def test_one_key_h8_both_edges_clipped(dcf, mask):
    """N = 2, x0 = 0x0123, 4096 + 37 points: h = 8, four level launches, both edge blocks clipped."""
    run_fold(dcf, 2, 0x0123, 4096 + 37, 1, 2100 + mask, mask=mask, expect_h=8)


def test_one_key_carry_across_the_limb(dcf):
    run_fold(dcf, 16, (1 << 64) - 1000, 5000, 1, 2110, expect_h=8)


@pytest.mark.parametrize("nb,count", [(1, 1), (1, 63), (2, 4095)])
def test_one_key_direct_walk(dcf, nb, count):
    """h = 0: the root walk writes y, k_fold_rows folds it."""
    run_fold(dcf, nb, 0, count, 1, 2120 + count, expect_h=0)


def test_one_key_whole_24_bit_domain_and_memory(dcf):
    """N = 3, the whole domain: against eval_full_domain_device masked and folded on the device.  The
    fold holds the device memory the range call of that shape holds: no count * lambda buffer."""
    import torch
    nb, lam, count = 3, 16, 1 << 24
    rng = np.random.default_rng(2130)
    keys = [rng.bytes(32) for _ in range(2)]
    prg, P = dcf.Aes256HirosePrg(keys, lam), O.OraclePrg(keys, lam)
    d = dcf.DcfImpl(nb, lam, prg)
    assert d.range_subtree_levels(count) == 14
    alpha, beta, sd = rng.bytes(nb), rng.bytes(lam), [rng.bytes(lam), rng.bytes(lam)]
    cwb = _dev(_cwb1(O.gen(P, alpha, beta, sd[0], sd[1], 0)))
    g = torch.Generator(device="cuda").manual_seed(2130)
    w = torch.randint(0, 256, (count, lam), dtype=torch.uint8, device="cuda", generator=g)
    outs = []
    for b in (0, 1):
        s0 = _dev(sd[b])
        buf = torch.full((1 + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
        got = d.eval_range_fold_device(bool(b), cwb, s0, 0, count, w, out=buf[PAD])
        torch.cuda.synchronize()
        blocks = prg.last_eval_blocks()
        if b == 0:
            held = prg.device_bytes()
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + 1:] == SENTINEL).all())
        full = d.eval_full_domain_device(bool(b), cwb, s0)
        assert torch.equal(got, dev_fold(full & w)), b
        outs.append(got.clone())
        del full
    a = int.from_bytes(alpha, "big")
    want = dev_fold(w[:a] & _dev(beta)) if a else torch.zeros(lam, dtype=torch.uint8, device="cuda")
    assert torch.equal(outs[0] ^ outs[1], want)
    other = dcf.Aes256HirosePrg(keys, lam)
    dcf.DcfImpl(nb, lam, other).eval_range_device(True, cwb, _dev(sd[1]), 0, count)
    torch.cuda.synchronize()
    assert blocks == other.last_eval_blocks()
    print(f"device bytes: fold {held}, range call {other.device_bytes()}; outputs would be {count * lam}")
    assert held == other.device_bytes() and held < count * lam


# ---- K keys, Hirose, lambda = 16 ----

def test_keys_direct_walk(dcf):
    run_fold(dcf, 2, 0x0310, 50, 3, 2200, expect_h=0)


def test_keys_h4_a_wave_spans_13_keys(dcf):
    """64 keys x 64 points from x0 = 5 mod 16: h = 4, no level launch, 5 nodes per key."""
    run_fold(dcf, 2, 0x1235, 64, 64, 2210, expect_h=4)


def test_keys_partial_last_wave_and_straddled_waves(dcf):
    run_fold(dcf, 1, 100, 67, 129, 2220, expect_h=4)


def test_keys_h7(dcf):
    run_fold(dcf, 2, 0x2345, 1000, 37, 2230, expect_h=7)


def test_keys_without_mask(dcf):
    run_fold(dcf, 2, 0x2345, 300, 20, 2240, mask=False, expect_h=6)


# ---- the other PRG shapes ----

def test_mmo_three_keys(dcf):
    run_fold(dcf, 4, 0x00FFF123, 3001, 3, 2300, kind="mmo", expect_h=9)


def test_mmo_one_key(dcf):
    run_fold(dcf, 4, 0x00ABCDEF, (1 << 13) + 1, 1, 2310, kind="mmo", expect_h=8)


def test_hirose_lambda_32(dcf):
    run_fold(dcf, 2, 0x01F0, 777, 1, 2320, lam=32, fused=False)


def test_hirose_lambda_64_two_keys(dcf):
    run_fold(dcf, 2, 0x0456, 5000, 2, 2330, lam=64, fused=False)


def test_mmo_lambda_32_whole_domain(dcf):
    run_fold(dcf, 1, 0, 256, 1, 2340, kind="mmo", lam=32, fused=False)


def test_n17_across_the_wrap_of_the_low_bytes(dcf):
    run_fold(dcf, 17, (1 << 128) - 150, 300, 1, 2350, fused=False)


# ---- launch groups: against the library's own range output folded on the device ----

def test_one_key_two_launch_groups(dcf):
    """count = 2^28 + 3 from an unaligned x0 at N = 4: two launch groups fold into the one row."""
    import torch
    nb, lam, count, x0 = 4, 16, (1 << 28) + 3, 12345
    rng = np.random.default_rng(2400)
    prg, _ = _prgs(dcf, "hirose", lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    g = torch.Generator(device="cuda").manual_seed(2400)
    r = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    alpha, s1 = r(1, nb), r(1, lam)
    alpha[:, 0] = 0x08  # inside the range
    cwb = d.gen_batch_device(alpha, r(1, lam), r(1, lam), s1, dcf.BoundState.GtBeta)
    buf = torch.full((1 + 2 * PAD, lam), 0xFF, dtype=torch.uint8, device="cuda")
    got = d.eval_range_fold_device(True, cwb, s1[0], x0, count, None, out=buf[PAD])
    torch.cuda.synchronize()
    blocks = prg.last_eval_blocks()
    assert bool((buf[:PAD] == 0xFF).all()) and bool((buf[PAD + 1:] == 0xFF).all())
    y = d.eval_range_device(True, cwb, s1[0], x0, count)
    torch.cuda.synchronize()
    assert blocks == prg.last_eval_blocks()
    assert torch.equal(got, dev_fold(y))


def test_keys_two_launch_groups(dcf):
    """N = 2 whole domain, one key more than a launch group holds, a 1 MiB table: the keys at the
    seam and at both ends against the single-key fold."""
    import torch
    nb, lam, count = 2, 16, 1 << 16
    rng = np.random.default_rng(2410)
    prg, _ = _prgs(dcf, "hirose", lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    per = d.range_keys_per_launch(1 << 12, count)
    K = per + 1
    assert 2 <= K <= (1 << 12) + 1
    g = torch.Generator(device="cuda").manual_seed(2410)
    r = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    alpha, beta, s0, s1 = r(K, nb), r(K, lam), r(K, lam), r(K, lam)
    cwb = d.gen_batch_device(alpha, beta, s0, s1, dcf.BoundState.LtBeta)
    w = r(count, lam)
    buf = torch.full((K + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
    got = d.eval_range_fold_multikey_device(True, cwb, s1, 0, count, w, out=buf[PAD:PAD + K])
    torch.cuda.synchronize()
    blocks = prg.last_eval_blocks()
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + K:] == SENTINEL).all())
    for k in (0, per - 1, per, K - 1):
        c1 = _single_cwb(cwb, nb, lam, K, k, dcf)
        assert torch.equal(got[k], d.eval_range_fold_device(True, c1, s1[k], 0, count, w)), k
    # party 0 reconstructs on the first key of the second group
    c1 = _single_cwb(cwb, nb, lam, K, per, dcf)
    a = int.from_bytes(bytes(alpha[per].cpu().numpy()), "big")
    want = dev_fold(w[:a] & beta[per]) if a else torch.zeros(lam, dtype=torch.uint8, device="cuda")
    assert torch.equal(got[per] ^ d.eval_range_fold_device(False, c1, s0[per], 0, count, w), want)
    y = d.eval_range_multikey_device(True, cwb, s1, 0, count)
    torch.cuda.synchronize()
    assert blocks == prg.last_eval_blocks()
    assert torch.equal(got[K - 1], dev_fold(y[K - 1] & w))


# ---- the other checks ----

def test_overwrite_and_two_calls_on_one_prg(dcf):
    """out pre-filled with 0xFF gives the fold, not an accumulation; a second call on the same prg
    with other keys (fused, then the row-folding path, then fused) is right as well."""
    rng = np.random.default_rng(2500)
    prgs = _prgs(dcf, "hirose", 16, rng)
    run_fold(dcf, 2, 0x0123, 5000, 1, 2501, prgs=prgs, prefill=0xFF, expect_h=8)
    run_fold(dcf, 2, 0x0123, 5000, 1, 2502, prgs=prgs, prefill=0xFF, expect_h=8)
    run_fold(dcf, 2, 0x0777, 200, 1, 2503, prgs=prgs, prefill=0xFF, expect_h=0)
    run_fold(dcf, 2, 0x0400, 700, 9, 2504, prgs=prgs, prefill=0xFF, expect_h=7)
    run_fold(dcf, 2, 0x0400, 700, 9, 2505, prgs=prgs, prefill=0xFF, expect_h=7)


def test_count_zero_writes_zeros(dcf):
    import torch
    rng = np.random.default_rng(2510)
    prg, _ = _prgs(dcf, "hirose", 16, rng)
    d = dcf.DcfImpl(2, 16, prg)
    K = 3
    cwb1, cwbk = _dev(bytes(dcf.cwb_bytes(2, 16, 1))), _dev(bytes(dcf.cwb_bytes(2, 16, K)))
    buf = torch.full((K + 2 * PAD, 16), SENTINEL, dtype=torch.uint8, device="cuda")
    d.eval_range_fold_device(False, cwb1, _dev(bytes(16)), 0xFFFF, 0, None, out=buf[PAD])
    torch.cuda.synchronize()
    assert not bool(buf[PAD].any()) and bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + 1:] == SENTINEL).all())
    buf[:] = SENTINEL
    d.eval_range_fold_multikey_device(False, cwbk, _dev(bytes(16 * K)).view(K, 16), 7, 0, None, out=buf[PAD:PAD + K])
    torch.cuda.synchronize()
    assert not bool(buf[PAD:PAD + K].any())
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + K:] == SENTINEL).all())


def test_errors(dcf, hip_lib):
    import torch
    rng = np.random.default_rng(2520)
    prg, _ = _prgs(dcf, "hirose", 16, rng)
    K = 3
    for nb, x0, count in ((16, (1 << 128) - 10, 11), (1, 200, 57)):
        d = dcf.DcfImpl(nb, 16, prg)
        cwb, s0s = _dev(bytes(dcf.cwb_bytes(nb, 16, K))), _dev(bytes(16 * K)).view(K, 16)
        with pytest.raises(dcf.DcfError) as e:
            d.eval_range_fold_multikey_device(False, cwb, s0s, x0, count)
        assert e.value.code == -1  # DCF_ERR_ARG: the range would wrap
        with pytest.raises(dcf.DcfError) as e:
            d.eval_range_fold_device(False, _dev(bytes(dcf.cwb_bytes(nb, 16, 1))), s0s[0], x0, count)
        assert e.value.code == -1
    cwb, s0s = _dev(bytes(dcf.cwb_bytes(16, 16, K))), _dev(bytes(16 * K))
    out = torch.full((K, 16), SENTINEL, dtype=torch.uint8, device="cuda")
    w = torch.zeros((8, 16), dtype=torch.uint8, device="cuda")
    x0 = (5).to_bytes(16, "big")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f = hip_lib.dcf_eval_range_fold_multikey_device
    assert f(prg.handle, 16, 0, 0, p(cwb), p(s0s), x0, 8, p(w), p(out), None) == 0  # no keys: nothing written
    assert f(prg.handle, 16, K, 2, p(cwb), p(s0s), x0, 8, p(w), p(out), None) == -1
    assert f(prg.handle, 16, K, -1, p(cwb), p(s0s), x0, 8, p(w), p(out), None) == -1
    assert f(prg.handle, 0, K, 0, p(cwb), p(s0s), x0, 8, p(w), p(out), None) == -4
    assert f(prg.handle, 257, K, 0, p(cwb), p(s0s), x0, 8, p(w), p(out), None) == -7
    assert f(prg.handle, 16, K, 0, None, p(s0s), x0, 8, p(w), p(out), None) == -1
    assert f(prg.handle, 16, K, 0, p(cwb), None, x0, 8, p(w), p(out), None) == -1
    assert f(prg.handle, 16, K, 0, p(cwb), p(s0s), None, 8, p(w), p(out), None) == -1
    assert f(prg.handle, 16, K, 0, p(cwb), p(s0s), x0, 8, p(w), None, None) == -1
    f1 = hip_lib.dcf_eval_range_fold_device
    assert f1(prg.handle, 16, 2, p(cwb), p(s0s), x0, 8, p(w), p(out), None) == -1
    assert f1(prg.handle, 0, 0, p(cwb), p(s0s), x0, 8, p(w), p(out), None) == -4
    assert f1(prg.handle, 16, 0, p(cwb), p(s0s), x0, 8, p(w), None, None) == -1
    assert f1(None, 16, 0, p(cwb), p(s0s), x0, 8, p(w), p(out), None) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
