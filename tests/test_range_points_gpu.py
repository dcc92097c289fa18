"""The materialising path of range eval on the GPU: the shapes with no tree path (every N > 16, and
the MMO PRG at LAMBDA >= 32) write the points x0 + i to a device buffer, 2^22 at a time
(k_range_points), and run dcf_eval_device's path on them; K keys go key by key through
k_rangemk_gather.  For N > 16 the host splits the range at the one row where the low 128 bits of x
wrap (range_parse: first, top, top1).

The reference is the CPU oracle on the points (x0 + i).to_bytes(N, "big"), which Python builds with
big-integer arithmetic, on keys from the oracle's gen, bit for bit.  Every case runs both parties,
checks the 64 sentinel rows on either side of ys and that the parties' outputs reconstruct the
comparison function on all rows.  No block counts: include/dcf_hip.h documents none for this path."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_range_gpu import PAD, SENTINEL, _cwb, _dev, _points, _prgs, _sample
from tests.test_range_multikey_gpu import _alpha, _cwbk

pytestmark = pytest.mark.gpu

LOW = 1 << 128  # the kernels add in the low 16 bytes; the bytes above them come from the host
PASS = 1 << 22  # points per pass of the materialising path (include/dcf_hip.h: "2^22 at a time")


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


def _rand(seed, nbytes) -> int:
    return int.from_bytes(np.random.default_rng(seed).bytes(nbytes), "big")


def _check_rec(rec, beta_dev, off, count, bound, what):
    """rec = y0 ^ y1 (device, all rows) against beta * [x < alpha] / [x > alpha]; alpha = x0 + off,
    which may lie outside the range."""
    if bound == 0:
        cut = min(max(off, 0), count)
        on, rest = rec[:cut], rec[cut:]
    else:
        cut = min(max(off + 1, 0), count)
        on, rest = rec[cut:], rec[:cut]
    assert bool((on == beta_dev).all()) and not bool(rest.any()), ("reconstruction",) + what


def run_range(dcf, nb, x0, count, seed, bounds=(0,), kind="hirose", lam=16, alpha_offs=(None,), idx=None, impl=None):
    """A fresh key per (bound, alpha offset), both parties: sentinels, the rows idx (default:
    _sample, every row of a short range) against the oracle, reconstruction on all rows.  impl: a
    (prg, oracle prg, DcfImpl) to run on instead of a new one.  Returns that triple and the last
    key's (ok, cwb, seeds, [y0, y1])."""
    import torch
    rng = np.random.default_rng(seed)
    prg, P, d = impl or (*_prgs(dcf, kind, lam, rng), None)
    d = d or dcf.DcfImpl(nb, lam, prg)
    last = None
    for bound in bounds:
        for alpha_off in alpha_offs:
            off = int(rng.integers(0, count)) if alpha_off is None else alpha_off
            alpha, beta = (x0 + off).to_bytes(nb, "big"), rng.bytes(lam)
            seeds = [rng.bytes(lam), rng.bytes(lam)]
            ok = O.gen(P, alpha, beta, seeds[0], seeds[1], bound)
            cwb = _dev(_cwb(ok))
            rows = _sample(count, rng) if idx is None else idx
            xs = _points(nb, x0, rows)
            what = (nb, lam, kind, hex(x0), count, "bound", bound, "alpha at row", off)
            ys = []
            for b in (0, 1):
                buf = torch.full((count + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
                y = d.eval_range_device(bool(b), cwb, _dev(seeds[b]), x0, count, ys=buf[PAD:PAD + count])
                torch.cuda.synchronize()
                assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + count:] == SENTINEL).all()), \
                    ("neighbours of ys written", b) + what
                got = y[torch.from_numpy(rows).cuda()].cpu().numpy()
                want = O.eval_(P, b, ok, seeds[b], xs, nthreads=8)
                bad = np.flatnonzero((got != want).any(axis=1))
                assert bad.size == 0, what + ("party", b, "first mismatching i", rows[bad[:8]])
                ys.append(y)
            _check_rec(ys[0] ^ ys[1], _dev(beta), off, count, bound, what)
            last = (ok, cwb, seeds, ys)
            del buf
    return (prg, P, d), last


# ---- the split at the row where the low 128 bits wrap ----

WRAP17 = (0x41 << 128) + LOW - 300  # N = 17: rows 0..299 carry top byte 0x41, rows 300.. carry 0x42


def test_wrap_of_the_low_128_bits_inside_the_range(dcf):
    """N = 17, LAMBDA = 16, 777 rows, both bounds; alpha on each side of the wrap, on the last row
    before it and on the first after it."""
    assert _points(17, WRAP17, [299, 300])[:, 0].tolist() == [0x41, 0x42]
    run_range(dcf, 17, WRAP17, 777, 4100, bounds=(0, 1), alpha_offs=(120, 555, 299, 300))


def test_carry_rippling_through_several_top_bytes(dcf):
    """N = 20: top bytes 00 FF FF FF for rows 0..4, 01 00 00 00 from row 5 on."""
    x0 = (0x00FFFFFF << 128) + LOW - 5
    pts = _points(20, x0, [4, 5])
    assert pts[0, :4].tolist() == [0, 0xFF, 0xFF, 0xFF] and pts[1, :4].tolist() == [1, 0, 0, 0]
    run_range(dcf, 20, x0, 64, 4101, bounds=(0, 1), alpha_offs=(None, 4, 5))


@pytest.mark.parametrize("nb,back,count", [(18, 77, 77), (17, 1, 1)])
def test_domain_end_above_16_bytes(dcf, nb, back, count):
    """N = 18 from 2^144 - 77 and N = 17 from 2^136 - 1: the last `count` points of the domain
    succeed (the low bits do not wrap: top1 is not used); one point more carries out of the top
    bytes: DCF_ERR_ARG from both entry points, nothing written."""
    import torch
    x0 = (1 << (8 * nb)) - back
    (prg, P, d), (ok, cwb, seeds, _) = run_range(dcf, nb, x0, count, 4102 + nb, bounds=(0, 1))
    buf = torch.full((count + 1 + 2 * PAD, 16), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(dcf.DcfError) as e:
        d.eval_range_device(True, cwb, _dev(seeds[1]), x0, count + 1, ys=buf[PAD:PAD + count + 1])
    assert e.value.code == -1  # DCF_ERR_ARG
    s0s = _dev(seeds[1] + seeds[1]).view(2, 16)
    with pytest.raises(dcf.DcfError) as e:
        d.eval_range_multikey_device(True, _dev(_cwbk([ok, ok], nb, 16)), s0s, x0, count + 1)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


def test_widest_n(dcf):
    """N = 256 (240 top bytes): random top bytes, the lowest of them 0xFF so the carry ripples into
    the byte above, low 128 bits 2^128 - 40, 100 rows."""
    top = _rand(4105, 240) | 0xFF
    x0 = (top << 128) + LOW - 40
    pts = _points(256, x0, [39, 40])
    assert pts[0, 239] == 0xFF and pts[1, 239] == 0 and int(pts[1, 238]) == (int(pts[0, 238]) + 1) & 0xFF
    run_range(dcf, 256, x0, 100, 4105, bounds=(0, 1), alpha_offs=(None, 39, 40))


def test_n_257_is_unsupported(dcf):
    import torch
    rng = np.random.default_rng(4106)
    prg, _ = _prgs(dcf, "hirose", 16, rng)
    d = dcf.DcfImpl(257, 16, prg)
    buf = torch.full((8 + 2 * PAD, 16), SENTINEL, dtype=torch.uint8, device="cuda")
    ys = buf[PAD:PAD + 8]
    with pytest.raises(dcf.DcfError) as e:
        d.eval_range_device(False, _dev(bytes(dcf.cwb_bytes(257, 16, 1))), _dev(bytes(16)), 5, 8, ys=ys)
    assert e.value.code == -7  # DCF_ERR_UNSUPPORTED
    with pytest.raises(dcf.DcfError) as e:
        d.eval_range_multikey_device(False, _dev(bytes(dcf.cwb_bytes(257, 16, 2))), _dev(bytes(32)).view(2, 16), 5, 4,
                                     ys=ys.view(2, 4, 16))
    assert e.value.code == -7
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


def test_no_wrap_equals_eval_device_on_materialised_points(dcf):
    """N = 24, 5000 rows, bit 127 of x0 clear (no wrap): bytes 0..7 of a point come from the host's
    top bytes, 8..15 from the high and 16..23 from the low limb of the 128-bit add."""
    import torch
    nb, count = 24, 5000
    x0 = _rand(4107, nb) & ~(1 << 127)
    (_, _, d), (_, cwb, seeds, ys) = run_range(dcf, nb, x0, count, 4107, bounds=(0, 1))
    xs = torch.from_numpy(_points(nb, x0, range(count)).copy()).cuda()
    pointwise = d.eval_device(True, cwb, _dev(seeds[1]), xs)
    torch.cuda.synchronize()
    assert torch.equal(ys[1], pointwise)


@pytest.mark.parametrize("lam", [32, 128])
def test_hirose_wide_lambda_above_16_bytes(dcf, lam):
    """Hirose PRG at LAMBDA >= 32 has a tree path only for N <= 16: N = 17, the wrap inside."""
    run_range(dcf, 17, WRAP17, 600, 4200 + lam, bounds=(0, 1), lam=lam, alpha_offs=(None, 299, 300))


@pytest.mark.parametrize("lam", [32, 64])
def test_mmo_wide_lambda(dcf, lam):
    """The MMO PRG at LAMBDA >= 32 has no tree path at any N: N = 2 across 0x01FF -> 0x0200 and two
    more byte carries, and N = 16 across the 64-bit limb."""
    run_range(dcf, 2, 0x01F0, 777, 4300 + lam, bounds=(0, 1), kind="mmo", lam=lam)
    run_range(dcf, 16, (1 << 64) - 5, 300, 4400 + lam, bounds=(0, 1), kind="mmo", lam=lam)


@pytest.mark.parametrize("first,bound", [(123457, 0), (PASS, 1), (PASS + 500, 0)],
                         ids=["wrap-in-pass-0", "wrap-at-pass-1", "wrap-in-pass-1"])
def test_more_than_one_pass(dcf, first, bound):
    """N = 17, 2^22 + 1001 rows: two passes.  The wrap row `first` lies inside pass 0 (two
    k_range_points launches, then one), exactly at 2^22 (one launch each, pass 1 starts on top1) or
    at 2^22 + 500 (pass 1 is two launches).  Oracle: the first and last 4096 rows, 2048 on each
    side of `first` and of row 2^22, and 4096 random rows; reconstruction on all rows."""
    count = PASS + 1001
    x0 = (0x7E << 128) + LOW - first
    rng = np.random.default_rng(4500 + first)
    idx = np.unique(np.concatenate([np.arange(4096), np.arange(count - 4096, count),
                                    np.arange(first - 2048, min(first + 2048, count)),
                                    np.arange(PASS - 2048, min(PASS + 2048, count)),
                                    rng.integers(0, count, size=4096)]))
    assert _points(17, x0, [first - 1, first])[:, 0].tolist() == [0x7E, 0x7F]
    run_range(dcf, 17, x0, count, 4500 + first, bounds=(bound,), idx=idx)


# ---- K keys, key by key (rangemk_fallback, k_rangemk_gather) ----

def run_mk(dcf, nb, x0, count, K, seed, kind="hirose", lam=16):
    """K fresh oracle keys with alphas inside, outside and on the edges of the range (_alpha),
    alternating bounds, both parties: every key against the oracle (_sample rows: every row of a
    short range) and against eval_range_device of that key alone, sentinels, reconstruction."""
    import torch
    rng = np.random.default_rng(seed)
    prg, P = _prgs(dcf, kind, lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    bounds = [(k // 2 + k) % 2 for k in range(K)]
    oks, alphas, betas, seeds = [], [], [], []
    for k in range(K):
        a = _alpha(k, nb, x0, count, rng)
        beta, sd = rng.bytes(lam), [rng.bytes(lam), rng.bytes(lam)]
        oks.append(O.gen(P, a.to_bytes(nb, "big"), beta, sd[0], sd[1], bounds[k]))
        alphas.append(a)
        betas.append(beta)
        seeds.append(sd)
    cwb = _dev(_cwbk(oks, nb, lam))
    rows = _sample(count, rng)
    xs = _points(nb, x0, rows)
    ys = []
    for b in (0, 1):
        s0 = _dev(b"".join(sd[b] for sd in seeds)).view(K, lam)
        buf = torch.full((K * count + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
        y = d.eval_range_multikey_device(bool(b), cwb, s0, x0, count, ys=buf[PAD:PAD + K * count].view(K, count, lam))
        torch.cuda.synchronize()
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + K * count:] == SENTINEL).all()), \
            ("neighbours of ys written", nb, lam, kind, K, b)
        got = y.cpu().numpy()
        for k in range(K):
            want = O.eval_(P, b, oks[k], seeds[k][b], xs, nthreads=8)
            bad = np.flatnonzero((got[k][rows] != want).any(axis=1))
            assert bad.size == 0, (nb, lam, kind, hex(x0), count, K, "key", k, "party", b, "first mismatching i", rows[bad[:8]])
            single = d.eval_range_device(bool(b), _dev(_cwb(oks[k])), _dev(seeds[k][b]), x0, count)
            assert torch.equal(y[k], single), ("single-key call", k, b)
        ys.append(y)
    rec = ys[0] ^ ys[1]
    for k in range(K):
        _check_rec(rec[k], _dev(betas[k]), alphas[k] - x0, count, bounds[k], (nb, lam, kind, "key", k))


def test_multikey_wrap_inside(dcf):
    run_mk(dcf, 17, WRAP17, 777, 3, 4600)


def test_multikey_mmo_lambda_32(dcf):
    run_mk(dcf, 2, 0x01F0, 777, 3, 4601, kind="mmo", lam=32)


def test_multikey_two_keys_hirose_lambda_64(dcf):
    run_mk(dcf, 17, WRAP17, 600, 2, 4602, lam=64)


# ---- host buffers; calls that follow on the same prg ----

def test_host_entry_point(dcf):
    """dcf_eval_range at N = 17, 3000 rows, the wrap inside: the oracle and eval_range_device."""
    nb, lam, count, x0 = 17, 16, 3000, (0xC3 << 128) + LOW - 1234
    rng = np.random.default_rng(4700)
    prg, P = _prgs(dcf, "hirose", lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    off = int(rng.integers(0, count))
    alpha, beta, seeds = (x0 + off).to_bytes(nb, "big"), rng.bytes(lam), [rng.bytes(lam), rng.bytes(lam)]
    ok = O.gen(P, alpha, beta, seeds[0], seeds[1], 1)
    xs = _points(nb, x0, range(count))
    ys = []
    for b in (0, 1):
        buf = np.full((count + 2 * PAD, lam), SENTINEL, np.uint8)
        y = d.eval_range(bool(b), dcf.cwb_to_share(_cwb(ok), nb, lam, [seeds[b]]), x0, count, ys=buf[PAD:PAD + count])
        assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + count:] == SENTINEL).all(), b
        assert np.array_equal(y, O.eval_(P, b, ok, seeds[b], xs, nthreads=8)), b
        ydev = d.eval_range_device(bool(b), _dev(_cwb(ok)), _dev(seeds[b]), x0, count)
        assert np.array_equal(y, ydev.cpu().numpy()), b
        ys.append(y.copy())
    rec = ys[0] ^ ys[1]
    assert (rec[off + 1:] == np.frombuffer(beta, np.uint8)).all() and not rec[:off + 1].any()


def test_following_calls_on_the_same_prg_stay_exact(dcf):
    """After an N = 17 call (its own points buffer, eval's workspace), an N = 16 tree-path range
    call and a plain eval_device on the same dcf_prg — one workspace, taken and returned LIFO."""
    import torch
    impl, _ = run_range(dcf, 17, WRAP17, 777, 4800)
    prg, P, _ = impl
    x0 = (_rand(4801, 16) >> 1) | 1
    d16 = dcf.DcfImpl(16, 16, prg)
    assert d16.range_subtree_levels(5000) == 8
    _, (ok, cwb, seeds, ys) = run_range(dcf, 16, x0, 5000, 4802, impl=(prg, P, d16))
    xs = np.random.default_rng(4803).integers(0, 256, size=(1000, 16), dtype=np.uint8)
    xs[0] = np.frombuffer((x0 + 17).to_bytes(16, "big"), np.uint8)
    for b in (0, 1):
        y = d16.eval_device(bool(b), cwb, _dev(seeds[b]), torch.from_numpy(xs).cuda())
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().numpy(), O.eval_(P, b, ok, seeds[b], xs, nthreads=8)), b
        assert torch.equal(y[0], ys[b][17])
    run_range(dcf, 17, WRAP17, 777, 4804, impl=(prg, P, dcf.DcfImpl(17, 16, prg)))
