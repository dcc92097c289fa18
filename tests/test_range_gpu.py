"""Contiguous-range eval on the GPU: dcf_eval_range_device / dcf_eval_range against the CPU oracle
on the points (x0 + i).to_bytes(N, "big"), bit for bit, on keys from the oracle's gen.  Every case
also checks the 64 sentinel rows on either side of ys and, with alpha inside the range, that the
two parties' outputs reconstruct the comparison function."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_range_multikey_gpu import _nroots

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 64, 0xA5


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


def _cwb(ok) -> bytes:
    raw = ok.cw_s.tobytes() + ok.cw_v.tobytes() + ok.cw_t.tobytes()
    return raw + bytes((-len(raw)) % 16) + ok.cw_np1.tobytes()


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


def _sample(count, rng, edge=4096, rand=4096):
    """Every index of a short range; the first and last `edge` and `rand` random ones of a long one."""
    if count <= 2 * edge + rand:
        return np.arange(count)
    return np.unique(np.concatenate([np.arange(edge), np.arange(count - edge, count),
                                     rng.integers(edge, count - edge, size=rand)]))


def run_range(dcf, nb, x0, count, seed, bounds=(0,), kind="hirose", lam=16, alpha_off=None):
    """Both parties of a fresh key per bound, alpha inside [x0, x0 + count).  Returns the prg, the
    DcfImpl and the last key's (cwb, party-1 seed, party-1 ys) on the device."""
    import torch
    rng = np.random.default_rng(seed)
    prg, P = _prgs(dcf, kind, lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    last = None
    for bound in bounds:
        off = int(rng.integers(0, count)) if alpha_off is None else alpha_off
        alpha, beta = (x0 + off).to_bytes(nb, "big"), rng.bytes(lam)
        seeds = [rng.bytes(lam), rng.bytes(lam)]
        ok = O.gen(P, alpha, beta, seeds[0], seeds[1], bound)
        cwb = _dev(_cwb(ok))
        idx = _sample(count, rng)
        xs = _points(nb, x0, idx)
        ys = []
        for b in (0, 1):
            buf = torch.full((count + 2 * PAD, lam), SENTINEL, dtype=torch.uint8, device="cuda")
            y = d.eval_range_device(bool(b), cwb, _dev(seeds[b]), x0, count, ys=buf[PAD:PAD + count])
            torch.cuda.synchronize()
            assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + count:] == SENTINEL).all()), \
                ("neighbours of ys written", nb, x0, count, b)
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
    return prg, d, last


@pytest.mark.parametrize("count", [1, 2, 3, 31, 33, 1000])
def test_small_counts(dcf, count):
    x0 = int.from_bytes(np.random.default_rng(count).bytes(16), "big") >> 1
    run_range(dcf, 16, x0, count, 100 + count)


@pytest.mark.parametrize("count", [4095, 4096])
def test_direct_walk_to_tree_threshold(dcf, count):
    """h steps from 0 (every point walked) to 8 (blocks of 256) at 2^12 points."""
    x0 = (int.from_bytes(np.random.default_rng(7).bytes(16), "big") >> 1) | 1
    _, d, _ = run_range(dcf, 16, x0, count, 200 + count, bounds=(0, 1))
    assert d.range_subtree_levels(count) == (0 if count < 4096 else 8)


def test_carry_across_64_bit_boundary(dcf):
    run_range(dcf, 16, (1 << 64) - 5, 300, 301, bounds=(0, 1))


def test_carry_across_64_bit_boundary_in_the_root_prefixes(dcf):
    """Tree path: the block prefixes x0 >> 8 themselves carry from 2^56 - 1 into bit 56 and, with
    x0 just below 2^72, across the 64-bit limb of the 128-bit prefix add."""
    run_range(dcf, 16, (1 << 72) - 700, 5000, 302)


def test_straddling_the_midpoint(dcf):
    run_range(dcf, 16, (1 << 127) - 100, 257, 303, bounds=(0, 1))
    run_range(dcf, 16, (1 << 127) - 3000, 6000, 304)  # the same on the tree path


def test_ending_at_the_domain_end(dcf):
    run_range(dcf, 16, (1 << 128) - 77, 77, 305, bounds=(0, 1))
    run_range(dcf, 2, 65000, 536, 306, bounds=(0, 1))
    run_range(dcf, 16, (1 << 128) - 4500, 4500, 307)  # tree path, last block ends the domain


@pytest.fixture(scope="module")
def many_blocks(dcf):
    """N = 16, random odd x0, 2^17 + 3 points, both bounds: oracle on the first 4096, the last 4096
    and 4096 random indices, reconstruction on all (run_range).  Shared with the work bound."""
    import torch
    count = (1 << 17) + 3
    x0 = (int.from_bytes(np.random.default_rng(17).bytes(16), "big") >> 1) | 1
    prg, d, _ = run_range(dcf, 16, x0, count, 400, bounds=(0, 1))
    torch.cuda.synchronize()
    return count, prg.last_eval_blocks(), d.range_subtree_levels(count)


def test_many_blocks_unaligned_both_ends(many_blocks):
    assert many_blocks[2] == 9  # 257 or 258 blocks of 512 leaves: several workgroups, 5 breadth-first levels


def test_work_bound(many_blocks):
    """dcf_prg_last_eval_blocks <= 4 * count at N = 16, count = 2^17 + 3: 2 blocks per output for
    the tree, 2 (128 - h) / 2^h for the root paths, at most 4 * 2^h in all for the two clipped edge
    blocks — under 3 per output for any h in [9, 14].  The per-point path needs >= 111."""
    count, blocks, _ = many_blocks
    print(f"range eval blocks: {blocks} = {blocks / count:.3f} per output")
    assert 0 < blocks <= 4 * count


def test_full_lds_node_buffer(dcf):
    """2^22 + 5 points: h = 14, ten breadth-first levels fill the 1024-node LDS buffer."""
    x0 = (int.from_bytes(np.random.default_rng(22).bytes(16), "big") >> 1) | 1
    _, d, _ = run_range(dcf, 16, x0, (1 << 22) + 5, 500)
    assert d.range_subtree_levels((1 << 22) + 5) == 14


@pytest.mark.parametrize("nb", [1, 2])
def test_whole_domain_equals_full_domain_eval(dcf, nb):
    import torch
    _, d, (cwb, s1, y1) = run_range(dcf, nb, 0, 1 << (8 * nb), 600 + nb)
    full = d.eval_full_domain_device(True, cwb, s1)
    torch.cuda.synchronize()
    assert torch.equal(y1, full)


def test_equals_eval_device_on_materialised_points(dcf):
    import torch
    nb, count, x0 = 8, 5000, (1 << 40) - 1234
    _, d, (cwb, s1, y1) = run_range(dcf, nb, x0, count, 700)
    xs = torch.from_numpy(_points(nb, x0, range(count)).copy()).cuda()
    pointwise = d.eval_device(True, cwb, s1, xs)
    torch.cuda.synchronize()
    assert torch.equal(y1, pointwise)


def test_errors(dcf, hip_lib):
    import torch
    rng = np.random.default_rng(800)
    prg, _ = _prgs(dcf, "hirose", 16, rng)
    d16, d1 = dcf.DcfImpl(16, 16, prg), dcf.DcfImpl(1, 16, prg)
    for d, x0, count in ((d16, (1 << 128) - 10, 11), (d1, 200, 57)):
        cwb, s0 = _dev(bytes(dcf.cwb_bytes(d.n_bytes, 16, 1))), _dev(bytes(16))
        with pytest.raises(dcf.DcfError) as e:
            d.eval_range_device(False, cwb, s0, x0, count)
        assert e.value.code == -1  # DCF_ERR_ARG: the range would wrap
    cwb, s0 = _dev(bytes(dcf.cwb_bytes(16, 16, 1))), _dev(bytes(16))
    ys = torch.full((8, 16), SENTINEL, dtype=torch.uint8, device="cuda")
    x0 = (5).to_bytes(16, "big")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert hip_lib.dcf_eval_range_device(prg.handle, 16, 0, p(cwb), p(s0), x0, 0, p(ys), None) == 0
    torch.cuda.synchronize()
    assert bool((ys == SENTINEL).all())
    assert hip_lib.dcf_eval_range_device(prg.handle, 16, 2, p(cwb), p(s0), x0, 1, p(ys), None) == -1
    assert hip_lib.dcf_eval_range_device(prg.handle, 0, 0, p(cwb), p(s0), x0, 1, p(ys), None) == -4
    assert hip_lib.dcf_eval_range_device(prg.handle, 16, 0, p(cwb), p(s0), None, 1, p(ys), None) == -1
    hk, hy = bytes(dcf.cwb_bytes(16, 16, 1)), np.zeros((8, 16), np.uint8)
    hp = ctypes.c_void_p(hy.ctypes.data)
    assert hip_lib.dcf_eval_range(prg.handle, 16, 0, hk, len(hk), bytes(16), x0, 8, hp, 8 * 16 - 1) == -5
    assert hip_lib.dcf_eval_range(prg.handle, 16, 0, hk, len(hk), bytes(16), x0, 7, hp, 8 * 16) == -5
    assert hip_lib.dcf_eval_range(prg.handle, 16, 0, hk, len(hk) - 16, bytes(16), x0, 8, hp, 8 * 16) == -8
    assert not hy.any()


# ---- the other tree paths at h = 0 (written for the materialising path, which these shapes have
# since left; that path is covered by tests/test_range_points_gpu.py) ----

def test_mmo_direct_walk(dcf):
    """MMO PRG, LAMBDA = 16, N = 4, 3001 points: below 2^12, so k_range_roots16_mmo walks every point."""
    run_range(dcf, 4, 0x00FFF123, 3001, 900, bounds=(0, 1), kind="mmo")


def test_hirose_lambda_32_direct_walk(dcf):
    """Hirose PRG, LAMBDA = 32, N = 2, 777 points: leaf mode of the LAMBDA >= 32 tree path
    (k_range_roots_wide writes y)."""
    run_range(dcf, 2, 0x01F0, 777, 901, bounds=(0, 1), lam=32)  # crosses 0x01FF -> 0x0200 and two more byte carries


def test_host_entry_point(dcf):
    nb, lam, count = 16, 16, 70001
    rng = np.random.default_rng(1000)
    prg, P = _prgs(dcf, "hirose", lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    x0 = (int.from_bytes(rng.bytes(16), "big") >> 1) | 1
    off = int(rng.integers(0, count))
    alpha, beta, seeds = (x0 + off).to_bytes(nb, "big"), rng.bytes(lam), [rng.bytes(lam), rng.bytes(lam)]
    ok = O.gen(P, alpha, beta, seeds[0], seeds[1], 0)
    xs = _points(nb, x0, range(count))
    ys = []
    for b in (0, 1):
        k = dcf.cwb_to_share(_cwb(ok), nb, lam, [seeds[b]])
        y = d.eval_range(bool(b), k, x0, count)
        assert np.array_equal(y, O.eval_(P, b, ok, seeds[b], xs, nthreads=8)), b
        ys.append(y)
    rec = ys[0] ^ ys[1]
    assert (rec[:off] == np.frombuffer(beta, np.uint8)).all() and not rec[off:].any()


def host_chunk(lam):
    """Outputs per chunk of dcf_eval_range: include/dcf_hip.h, "outputs come back in chunks of up to
    128 MiB through the prg's staging pool" (at least 256 outputs)."""
    return max(256, (128 << 20) // lam)


def run_host_chunked(dcf, kind, lam, nb, x0, count, seed, walk, node, parties=(1,), bound=0, alpha_off=None, group=1 << 28):
    """dcf_eval_range over more than one chunk.  Every chunk after the first starts where the one
    before ended, mid-block, at the height h of the whole count; the last may be a few points.
    Per party: the host result against eval_range_device over the same range (all rows, on the
    device), against the oracle on _sample rows and 2048 rows on each side of the chunk boundary,
    and the call's block count: at least 2 per output and at most the sum over the chunks (and
    the launch groups of `group` outputs inside a chunk) of the documented bound of a launch,
    nroots (walk (8N - h) + node (2^h - 1)) — so the count is neither reset nor doubled between
    chunks.  Both parties given: reconstruction on all rows."""
    import torch
    chunk = host_chunk(lam)
    assert chunk < count
    rng = np.random.default_rng(seed)
    prg, P = _prgs(dcf, kind, lam, rng)
    d = dcf.DcfImpl(nb, lam, prg)
    h = d.range_subtree_levels(count)
    assert h > 0
    off = int(rng.integers(0, count)) if alpha_off is None else alpha_off
    alpha, beta, seeds = (x0 + off).to_bytes(nb, "big"), rng.bytes(lam), [rng.bytes(lam), rng.bytes(lam)]
    ok = O.gen(P, alpha, beta, seeds[0], seeds[1], bound)
    cwb = _dev(_cwb(ok))
    idx = np.unique(np.concatenate([_sample(count, rng), np.arange(chunk - 2048, min(chunk + 2048, count))]))
    xs = _points(nb, x0, idx)
    launches = [(x0 + o + g, min(group, n - g)) for o in range(0, count, chunk)
                for n in [min(chunk, count - o)] for g in range(0, n, group)]
    upper = sum(_nroots(x, n, h) * (walk * (8 * nb - h) + node * ((1 << h) - 1)) for x, n in launches)
    ys = []
    for b in parties:
        y = d.eval_range(bool(b), dcf.cwb_to_share(_cwb(ok), nb, lam, [seeds[b]]), x0, count)
        blocks = prg.last_eval_blocks()
        print(f"{kind} lam={lam} N={nb} count={count} h={h}: {len(launches)} launches, {blocks} blocks, bound {upper}")
        assert 2 * count <= blocks <= upper, (blocks, 2 * count, upper)
        yh = torch.from_numpy(y).cuda()
        ydev = d.eval_range_device(bool(b), cwb, _dev(seeds[b]), x0, count)
        torch.cuda.synchronize()
        assert torch.equal(yh, ydev), ("host and device entry points differ", b)
        want = O.eval_(P, b, ok, seeds[b], xs, nthreads=8)
        bad = np.flatnonzero((y[idx] != want).any(axis=1))
        assert bad.size == 0, (kind, lam, nb, hex(x0), count, b, "first mismatching i", idx[bad[:8]])
        ys.append(yh)
        del ydev, y
    if len(ys) == 2:
        rec = ys[0] ^ ys[1]
        lo, hi = (rec[:off], rec[off:]) if bound == 0 else (rec[off + 1:], rec[:off + 1])
        assert bool((lo == _dev(beta)).all()) and not bool(hi.any()), ("reconstruction", kind, lam, nb, count)


def test_host_entry_point_chunked(dcf):
    """Hirose, LAMBDA = 16, N = 16, odd x0, one chunk and 3 points: h = 14, and the last chunk is 3
    points at h = 14 (a shape the device entry point has only at h = 0); alpha in that chunk."""
    count = host_chunk(16) + 3
    x0 = (int.from_bytes(np.random.default_rng(1001).bytes(16), "big") >> 1) | 1
    run_host_chunked(dcf, "hirose", 16, 16, x0, count, 1001, walk=2, node=2, parties=(0, 1), alpha_off=count - 2)
