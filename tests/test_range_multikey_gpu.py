"""Multi-key contiguous-range eval on the GPU: dcf_eval_range_multikey_device against the CPU
oracle on the points (x0 + i).to_bytes(N, "big"), bit for bit, on keys from the oracle's gen packed
into the K-key layout.  The keys of a case have different alphas (inside the range, outside it, on
its edges) and both bounds.  Every case also checks the 64 sentinel rows on either side of ys, that
the two parties' outputs reconstruct every key's comparison function, and on the tree path the
AES block count."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 64, 0xA5


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


def _cwb1(ok) -> bytes:
    """One oracle key in the single-key layout."""
    raw = ok.cw_s.tobytes() + ok.cw_v.tobytes() + ok.cw_t.tobytes()
    return raw + bytes((-len(raw)) % 16) + ok.cw_np1.tobytes()


def _cwbk(oks, nb, lam) -> bytes:
    """K oracle keys in the K-key layout: [n][K][lam], [n][K][lam], [n][K], pad to 16, cw_np1[K][lam]."""
    n = 8 * nb
    s = np.stack([np.asarray(ok.cw_s).reshape(n, lam) for ok in oks], axis=1)
    v = np.stack([np.asarray(ok.cw_v).reshape(n, lam) for ok in oks], axis=1)
    t = np.stack([np.asarray(ok.cw_t).reshape(n) for ok in oks], axis=1)
    raw = s.tobytes() + v.tobytes() + t.tobytes()
    return raw + bytes((-len(raw)) % 16) + b"".join(np.asarray(ok.cw_np1).tobytes() for ok in oks)


def _dev(b: bytes):
    import torch
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()


def _points(nb, x0, idx):
    return np.frombuffer(b"".join((x0 + int(i)).to_bytes(nb, "big") for i in idx), np.uint8).reshape(-1, nb)


def _prgs(dcf, kind, lam, rng):
    if kind == "mmo":
        keys = [rng.bytes(16) for _ in range(4 * lam // 16)]
        return dcf.Aes128MatyasMeyerOseasPrg(keys, lam), O.OracleMmoPrg(keys, lam)
    keys = [rng.bytes(32) for _ in range(2 if lam == 16 else 18)]
    return dcf.Aes256HirosePrg(keys, lam), O.OraclePrg(keys, lam)


def _alpha(k, nb, x0, count, rng) -> int:
    """Key k's alpha: inside the range, outside it (below, else above), or on one of its edges."""
    end, dom = x0 + count, 1 << (8 * nb)
    where = k % 4
    if where == 1 and (x0 > 0 or end < dom):
        lo, hi = (0, x0) if x0 > 0 and (k % 8 == 1 or end == dom) else (end, dom)
        return lo + int.from_bytes(rng.bytes(nb + 1), "big") % (hi - lo)
    if where == 2:
        return x0 if k % 8 == 2 else end - 1
    return x0 + int(rng.integers(0, count))


def _nroots(x0, count, h):
    return (((x0 % (1 << h)) + count - 1) >> h) + 1


def _check_blocks(blocks, nb, K, x0, count, h):
    """2 K (count - 1) <= blocks <= K nroots (2 (8N - h) + 2 (2^h - 1)): any binary expansion needs
    the lower side; the upper is what the three stages execute, clipped leaves included."""
    upper = K * _nroots(x0, count, h) * (2 * (8 * nb - h) + 2 * ((1 << h) - 1))
    print(f"N={nb} K={K} count={count} h={h}: {blocks} blocks = {blocks / (K * count):.3f} per output, bound {upper}")
    assert 2 * K * (count - 1) <= blocks <= upper, (blocks, upper)


def run_mk(dcf, nb, x0, count, K, seed, kind="hirose", lam=16, expect_h=None, both=False):
    """K fresh oracle keys, both parties.  Returns the prg, the DcfImpl, the oracle keys, the K-key
    CWB, the party-1 seeds (device) and the party-1 outputs (K, count, lam); with `both`, the seeds
    and the outputs of both parties, and each party's block count behind them."""
    import torch
    rng = np.random.default_rng(seed)
    prg, P = _prgs(dcf, kind, lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    oks, alphas, betas, seeds = [], [], [], []
    for k in range(K):
        a = _alpha(k, nb, x0, count, rng)
        beta, sd = rng.bytes(lam), [rng.bytes(lam), rng.bytes(lam)]
        oks.append(O.gen(P, a.to_bytes(nb, "big"), beta, sd[0], sd[1], (k // 2 + k) % 2))
        alphas.append(a)
        betas.append(beta)
        seeds.append(sd)
    bounds = [(k // 2 + k) % 2 for k in range(K)]
    cwb = _dev(_cwbk(oks, nb, lam))
    idx = np.arange(count)
    xs = _points(nb, x0, idx)
    h = d.range_multikey_subtree_levels(K, count)
    tree = kind == "hirose" and lam == 16 and nb <= 16
    if expect_h is not None:
        assert (h > 0) == expect_h, (nb, K, count, h)
    ys, s0s, blocks = [], [], []
    for b in (0, 1):
        s0 = _dev(b"".join(sd[b] for sd in seeds)).view(K, lam)
        buf = torch.full((K * count + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
        y = d.eval_range_multikey_device(bool(b), cwb, s0, x0, count, ys=buf[PAD:PAD + K * count].view(K, count, lam))
        torch.cuda.synchronize()
        assert y.shape == (K, count, lam)
        blocks.append(prg.last_eval_blocks())
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + K * count:] == SENTINEL).all()), \
            ("neighbours of ys written", nb, x0, count, K, b)
        if tree and h:
            _check_blocks(prg.last_eval_blocks(), nb, K, x0, count, h)
        got = y.cpu().numpy()
        for k in range(K):
            want = O.eval_(P, b, oks[k], seeds[k][b], xs, nthreads=8)
            bad = np.flatnonzero((got[k] != want).any(axis=1))
            assert bad.size == 0, (nb, hex(x0), count, K, "key", k, "party", b, "first mismatching i", bad[:8])
        ys.append(y)
        s0s.append(s0)
    rec = (ys[0] ^ ys[1]).cpu().numpy()
    for k in range(K):
        off = alphas[k] - x0
        m = idx < min(max(off, 0), count) if bounds[k] == 0 else idx > min(max(off, -1), count)
        bt = np.frombuffer(betas[k], np.uint8)
        assert (rec[k][m] == bt).all() and not rec[k][~m].any(), ("reconstruction", nb, hex(x0), count, "key", k)
    return (prg, d, oks, cwb, s0s, ys, blocks) if both else (prg, d, oks, cwb, s0s[1], ys[1])


# ---- h = 0: every point walked on its own ----

@pytest.mark.parametrize("count", [1, 3, 15])
def test_direct_walk_many_keys(dcf, count):
    x0 = (int.from_bytes(np.random.default_rng(count).bytes(16), "big") >> 1) | 1
    run_mk(dcf, 16, x0, count, 100, 1100 + count, expect_h=False)


def test_direct_walk_carry_across_64_bit_boundary(dcf):
    run_mk(dcf, 16, (1 << 64) - 5, 300, 3, 1120, expect_h=False)


# ---- tree path ----

@pytest.mark.parametrize("K", [1, 2, 3, 65, 130])
def test_whole_8_bit_domain_equals_full_domain_eval(dcf, K):
    """Blocks of 64 leaves, 4 per key: a wave of the levels and of the tail holds several keys (K <= 3:
    fewer than 2^12 outputs in all, the direct walk)."""
    import torch
    _, d, oks, _, s1, y1 = run_mk(dcf, 1, 0, 256, K, 1200 + K, expect_h=K >= 16)
    for k in range(K):
        full = d.eval_full_domain_device(True, _dev(_cwb1(oks[k])), s1[k])
        assert torch.equal(y1[k], full), k
    torch.cuda.synchronize()


def test_unaligned_both_ends_odd_roots_n2(dcf):
    """An odd number of keys, each clipped at both ends (x0 = 1000 into its first block, the last
    block 4536 leaves short of its end); the N = 16 case below has K * nroots odd as well."""
    run_mk(dcf, 2, 1000, 60000, 5, 1300, expect_h=True)


def test_unaligned_both_ends_odd_roots_n16(dcf):
    x0 = (int.from_bytes(np.random.default_rng(1301).bytes(16), "big") >> 1) | 1
    count, K = 4097, 3
    _, d, *_ = run_mk(dcf, 16, x0, count, K, 1301, expect_h=True)
    assert (K * _nroots(x0, count, d.range_multikey_subtree_levels(K, count))) % 2 == 1


def test_carry_in_the_root_prefixes(dcf):
    run_mk(dcf, 16, (1 << 72) - 700, 5000, 7, 1400, expect_h=True)


def test_ending_at_the_domain_end(dcf):
    run_mk(dcf, 16, (1 << 128) - 4500, 4500, 2, 1401, expect_h=True)


def test_against_the_existing_paths(dcf):
    import torch
    nb, count, x0, K = 8, 5000, (1 << 40) - 1234, 4
    _, d, oks, cwb, s1, y1 = run_mk(dcf, nb, x0, count, K, 1500, expect_h=True)
    xs = torch.from_numpy(_points(nb, x0, range(count)).copy()).cuda().repeat(K, 1)
    pointwise = d.eval_multikey_device(True, cwb, s1, xs, count)
    for k in range(K):
        single = d.eval_range_device(True, _dev(_cwb1(oks[k])), s1[k], x0, count)
        assert torch.equal(y1[k], single), k
    torch.cuda.synchronize()
    assert torch.equal(y1.reshape(K * count, 16), pointwise)


K1_CASES = [  # engine, PRG, N, lambda, x0, count, (single-key h, multi-key h) or None where no tree runs
    ("tree16", "hirose", 2, 16, 1001, 5000, (8, 10)),
    ("tree16", "mmo", 2, 16, 1001, 5000, (8, 10)),
    ("wide", "hirose", 2, 32, 1001, 5000, (8, 8)),
    ("wide", "hirose", 2, 64, 1001, 5000, (8, 8)),
    ("points", "hirose", 17, 16, (1 << 128) - 101, 300, None),
    ("points", "mmo", 2, 32, 1001, 300, None),
]


@pytest.mark.parametrize("engine,kind,nb,lam,x0,count,hs", K1_CASES, ids=[f"{c[0]}-{c[1]}-{c[3]}" for c in K1_CASES])
def test_one_key_multikey_call_equals_the_single_key_call(dcf, engine, kind, nb, lam, x0, count, hs):
    """K = 1 through eval_range_multikey_device (run_mk: both parties, sentinels, the oracle on every
    index) against eval_range_device on the same key, byte for byte, on each engine.  On the lambda =
    16 tree path the two entry points use different heights and the multi-key call's blocks are those
    of h = 10; at lambda >= 32 the heights agree and so do the block counts."""
    import torch
    seed = 1600 + 16 * nb + lam
    prg, d, oks, _, s0s, ys, blocks = run_mk(dcf, nb, x0, count, 1, seed, kind=kind, lam=lam, both=True)
    _, P = _prgs(dcf, kind, lam, np.random.default_rng(seed))  # the oracle prg of run_mk's keys
    if hs:
        wide = d.range_wide_multikey_subtree_levels(1, count) if engine == "wide" else d.range_multikey_subtree_levels(1, count)
        assert (d.range_subtree_levels(count), wide) == hs
    cwb1 = _dev(_cwb1(oks[0]))
    xs = _points(nb, x0, np.arange(count))
    for b in (0, 1):
        buf = torch.full((count + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
        y = d.eval_range_device(bool(b), cwb1, s0s[b][0], x0, count, ys=buf[PAD:PAD + count])
        torch.cuda.synchronize()
        single_blocks = prg.last_eval_blocks()
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + count:] == SENTINEL).all()), (engine, kind, b)
        assert torch.equal(y, ys[b][0]), (engine, kind, lam, b)
        want = O.eval_(P, b, oks[0], s0s[b][0].cpu().numpy().tobytes(), xs, nthreads=8)
        assert np.array_equal(y.cpu().numpy(), want), (engine, kind, lam, b)
        if engine == "tree16" and kind == "hirose":
            _check_blocks(blocks[b], nb, 1, x0, count, hs[1])
        elif engine == "tree16":
            from tests.test_range_mmo_gpu import check_blocks
            check_blocks(blocks[b], nb, 1, x0, count, hs[1])
        elif engine == "wide":
            assert blocks[b] == single_blocks, (lam, b, blocks[b], single_blocks)


def _single_cwb(cwb, nb, lam, K, k, dcf):
    """Key k of a K-key CWB (device tensor) in the single-key layout."""
    import torch
    n = 8 * nb
    s = cwb[:n * K * lam].view(n, K, lam)[:, k].reshape(-1)
    v = cwb[n * K * lam:2 * n * K * lam].view(n, K, lam)[:, k].reshape(-1)
    t = cwb[2 * n * K * lam:2 * n * K * lam + n * K].view(n, K)[:, k]
    off = dcf.cwb_np1_offset(nb, lam, K)
    np1 = cwb[off + k * lam:off + (k + 1) * lam]
    raw = torch.cat([s, v, t])
    return torch.cat([raw, torch.zeros((-raw.numel()) % 16, dtype=torch.uint8, device=cwb.device), np1]).contiguous()


def test_launch_split(dcf):
    """N = 2 whole domain with one key more than a launch group holds: the second group starts at a
    64-bit key offset.  Keys from gen_batch_device; the keys at the seam and at both ends against
    the single-key range eval."""
    import torch
    nb, lam, count = 2, 16, 1 << 16
    rng = np.random.default_rng(1600)
    prg, _ = _prgs(dcf, "hirose", lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    per = d.range_keys_per_launch(1 << 12, count)
    K = per + 1
    assert 2 <= K <= (1 << 12) + 1
    g = torch.Generator(device="cuda").manual_seed(1600)
    r = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    alpha, beta, s0, s1 = r(K, nb), r(K, lam), r(K, lam), r(K, lam)
    cwb = d.gen_batch_device(alpha, beta, s0, s1, dcf.BoundState.LtBeta)
    h = d.range_multikey_subtree_levels(K, count)
    buf = torch.full((K * count + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
    y = d.eval_range_multikey_device(True, cwb, s1, 0, count, ys=buf[PAD:PAD + K * count].view(K, count, lam))
    torch.cuda.synchronize()
    blocks = prg.last_eval_blocks()
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + K * count:] == SENTINEL).all())
    for k in (0, per - 1, per, K - 1):
        c1 = _single_cwb(cwb, nb, lam, K, k, dcf)
        assert torch.equal(y[k], d.eval_range_device(True, c1, s1[k], 0, count)), k
        if k == 0:  # one key through the same entry point, the same height: its block count
            assert d.range_multikey_subtree_levels(1, count) == h
            d.eval_range_multikey_device(True, c1, s1[:1], 0, count)
            torch.cuda.synchronize()
            one = prg.last_eval_blocks()
    _check_blocks(blocks, nb, K, 0, count, h)
    assert blocks == K * one, (blocks, K, one)
    # and party 0 reconstructs on the first key of the second group
    c1 = _single_cwb(cwb, nb, lam, K, per, dcf)
    rec = y[per] ^ d.eval_range_device(False, c1, s0[per], 0, count)
    a = int.from_bytes(bytes(alpha[per].cpu().numpy()), "big")
    assert bool((rec[:a] == beta[per]).all()) and not bool(rec[a:].any())


def test_one_key_larger_than_a_launch(dcf):
    """count = 2^28 + 3 from an unaligned x0 at N = 4: one key alone exceeds a launch group, so the
    keys run one after another, 2^28 outputs at a time (the second part starts mid-block)."""
    import torch
    nb, lam, count, K, x0 = 4, 16, (1 << 28) + 3, 2, 12345
    rng = np.random.default_rng(1650)
    prg, _ = _prgs(dcf, "hirose", lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    assert d.range_keys_per_launch(K, count) == 1 and d.range_multikey_subtree_levels(K, count) == 14
    g = torch.Generator(device="cuda").manual_seed(1650)
    r = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    alpha, s1 = r(K, nb), r(K, lam)
    alpha[:, 0] = 0x08  # inside the range
    cwb = d.gen_batch_device(alpha, r(K, lam), r(K, lam), s1, dcf.BoundState.GtBeta)
    buf = torch.full((K * count + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
    y = d.eval_range_multikey_device(True, cwb, s1, x0, count, ys=buf[PAD:PAD + K * count].view(K, count, lam))
    torch.cuda.synchronize()
    blocks = prg.last_eval_blocks()
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + K * count:] == SENTINEL).all())
    # two parts per key: at most (count >> 14) + 4 roots of 18 levels and count + 4 * 2^14 leaves
    assert 2 * K * (count - 1) <= blocks <= K * (2 * (count + (4 << 14)) + ((count >> 14) + 4) * 2 * (32 - 14))
    single = torch.empty((count, lam), dtype=torch.uint8, device="cuda")
    for k in range(K):
        d.eval_range_device(True, _single_cwb(cwb, nb, lam, K, k, dcf), s1[k], x0, count, single)
        assert torch.equal(y[k], single), k


# ---- the other PRG shapes (written for the key-by-key materialising path, which these shapes have
# since left; that path is covered by tests/test_range_points_gpu.py) ----

def test_mmo_tree_path_three_keys(dcf):
    """MMO PRG, LAMBDA = 16, N = 4, 3 keys x 3001 points: the MMO kernels of the K-key tree path, h = 9."""
    run_mk(dcf, 4, 0x00FFF123, 3001, 3, 1700, kind="mmo")


def test_hirose_lambda_32_key_by_key(dcf):
    """Hirose PRG, LAMBDA = 32, N = 2, 2 keys x 777 points: k_rangemk_gather, then each key through
    the single-key LAMBDA >= 32 tree path in leaf mode (h = 0)."""
    run_mk(dcf, 2, 0x01F0, 777, 2, 1701, lam=32)


# ---- errors ----

def test_errors(dcf, hip_lib):
    import torch
    rng = np.random.default_rng(1800)
    prg, _ = _prgs(dcf, "hirose", 16, rng)
    K = 3
    for nb, x0, count in ((16, (1 << 128) - 10, 11), (1, 200, 57)):
        d = dcf.DcfImpl(nb, 16, prg)
        cwb, s0s = _dev(bytes(dcf.cwb_bytes(nb, 16, K))), _dev(bytes(16 * K)).view(K, 16)
        with pytest.raises(dcf.DcfError) as e:
            d.eval_range_multikey_device(False, cwb, s0s, x0, count)
        assert e.value.code == -1  # DCF_ERR_ARG: the range would wrap
    cwb, s0s = _dev(bytes(dcf.cwb_bytes(16, 16, K))), _dev(bytes(16 * K))
    ys = torch.full((K * 8, 16), SENTINEL, dtype=torch.uint8, device="cuda")
    x0 = (5).to_bytes(16, "big")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f = hip_lib.dcf_eval_range_multikey_device
    assert f(prg.handle, 16, 0, 0, p(cwb), p(s0s), x0, 8, p(ys), None) == 0
    assert f(prg.handle, 16, K, 0, p(cwb), p(s0s), x0, 0, p(ys), None) == 0
    torch.cuda.synchronize()
    assert bool((ys == SENTINEL).all())
    assert f(prg.handle, 16, K, 2, p(cwb), p(s0s), x0, 8, p(ys), None) == -1
    assert f(prg.handle, 16, K, -1, p(cwb), p(s0s), x0, 8, p(ys), None) == -1
    assert f(prg.handle, 0, K, 0, p(cwb), p(s0s), x0, 8, p(ys), None) == -4
    assert f(prg.handle, 16, K, 0, p(cwb), p(s0s), None, 8, p(ys), None) == -1
    assert f(prg.handle, 16, K, 0, p(cwb), p(s0s), x0, 8, None, None) == -1
    torch.cuda.synchronize()
    assert bool((ys == SENTINEL).all())
