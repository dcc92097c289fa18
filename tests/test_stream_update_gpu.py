"""k_eval16_stream's mask-form level update on the GPU, byte for byte against the oracle, both
parties, through the stream engine (DCF_EVAL_STREAM), and its own AES block count against the
word-for-word emulation of tests/test_stream_update_emulation.py: the count shows that run reuse
is taken, or not, in the instance that ran.  RUN mirrors the per-family defaults of
dcf_amd/csrc/kernels_stream.h (DCF_REUSE_RUN_*); a changed default shows up here as a count that
matches the other emulation."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import pyref
from tests.test_stream_update_emulation import _w, patterned, stream_eval

pytestmark = pytest.mark.gpu

EVAL_STREAM = 4  # DCF_EVAL_STREAM (include/dcf_hip.h)
M = 3 * 256 + 17  # several 256-point units and a partial one
# Run reuse per instance family: x words in registers, one key (N = 16) / one key, x in one word
# (N = 4) / multi-key; x loaded per word (N no multiple of 4).
RUN = {"sk": True, "sk4": True, "xw": True}


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


def _points(rng, nb, m):
    """The first 64 points the patterned x values (repeated to 64), the rest seeded random."""
    pat = patterned(nb)
    xs = rng.integers(0, 256, size=(m, nb), dtype=np.uint8)
    for i in range(64):
        xs[i] = np.frombuffer(pat[i % len(pat)], np.uint8)
    return xs


def _prefix_state(prg, party, s0, cws, x, depth):
    """(s, v, t) after `depth` levels of lib.rs:163-190: the prefix table's row for x."""
    zero = bytes(16)
    xor = lambda *a: bytes(np.bitwise_xor.reduce([np.frombuffer(b, np.uint8) for b in a]))  # noqa: E731
    s, t, v = bytes(s0), bool(party), zero
    for i in range(depth):
        cs, cv, ctl, ctr = cws[i]
        (sl, vl, tl), (sr, vr, tr) = prg.gen(s)
        right = (x[i // 8] >> (7 - i % 8)) & 1
        sn, vn, tn, ct = (sr, vr, tr, ctr) if right else (sl, vl, tl, ctl)
        v = xor(v, vn, cv if t else zero)
        s = xor(sn, cs if t else zero)
        t = bool(tn) ^ (t & bool(ct))
    return _w(s), _w(v), int(t)


@pytest.mark.parametrize("party", [0, 1])
@pytest.mark.parametrize("nb,prefix,family", [(16, 0, "sk"), (16, 5, "sk"), (4, 5, "sk4"), (1, 0, "xw"), (3, 0, "xw")])
def test_single_key_bytes_and_block_count(dcf, nb, prefix, family, party):
    rng = np.random.default_rng(0x5700 + 16 * nb + prefix)
    keys = [rng.bytes(32) for _ in range(2)]
    prg, Po = dcf.Aes256HirosePrg(keys, 16), O.OraclePrg(keys, 16)
    prg.set_eval_mode(EVAL_STREAM)
    prg.set_prefix_levels(prefix)
    d = dcf.DcfImpl(nb, 16, prg)
    pprg, aes = pyref.HirosePrg(keys, 16), pyref.Aes256Ecb(keys[0])
    depth = prg.eval_prefix_levels(nb, 1, M)
    assert depth == prefix
    run = RUN[family]
    ones = bytes([0xFF]) * nb

    def emulate(xb, run):
        if depth:
            s, v, t = _prefix_state(pprg, party, s0s[party], cws, xb, depth)
            return stream_eval(aes, s, v, t, depth, xb, cws, np1, run, fresh=False)
        # at the root the x-in-registers instance takes its first x word from the queue (fresh)
        return stream_eval(aes, _w(s0s[party]), [0] * 4, party, 0, xb, cws, np1, run, fresh=family != "xw")

    for _ in range(256):
        alpha, beta = rng.bytes(nb), rng.bytes(16)
        s0s = [bytearray(rng.bytes(16)), bytearray(rng.bytes(16))]
        s0s[0][15] |= 1   # party 0: a root seed with its masked bit set never reuses at the root
        s0s[1][15] &= 0xFE
        s0s = [bytes(s) for s in s0s]
        cws, np1 = pyref.gen(pprg, alpha, beta, s0s, nb % 2)
        # a key on whose all-ones path this party meets a run at t = 0 (whether one exists depends
        # on the key's t bits along that path: at N = 1 most keys have none)
        if not run or emulate(ones, True)[1] < emulate(ones, False)[1]:
            break
    else:
        raise AssertionError("no key with a t = 0 run on the all-ones path in 256 draws")
    ok = O.gen(Po, alpha, beta, s0s[0], s0s[1], nb % 2)
    k = d.gen(dcf.CmpFn(alpha, beta), s0s, dcf.BoundState(nb % 2))
    xs = _points(rng, nb, M)
    got = d.eval(bool(party), dcf.Share([s0s[party]], k.cws, k.cw_np1), xs)
    blocks = prg.last_eval_blocks()
    want = O.eval_(Po, party, ok, s0s[party], xs, nthreads=8)
    assert np.array_equal(got, want), (nb, prefix, party)

    emu = [emulate(x.tobytes(), run) for x in xs]
    assert [e[0] for e in emu] == [w.tobytes() for w in want]
    # the walk's blocks alone: the device count leaves out a single key's prefix table build
    # (include/dcf_hip.h, dcf_prg_last_eval_blocks), whose 2^(D+1) - 2 blocks the bench adds itself
    total = sum(e[1] for e in emu)
    print(f"N={nb} prefix={depth} party={party} run={run}: kernel blocks {blocks}, emulation {total}")
    assert blocks == total
    if run:  # really taken: fewer blocks than the single-step form on the all-ones points
        idx = [i for i in range(64) if xs[i].tobytes() == ones]
        off = sum(emulate(ones, False)[1] for i in idx)
        on = sum(emu[i][1] for i in idx)
        print(f"  all-ones points: {on} blocks with run reuse, {off} without")
        assert idx and on < off


@pytest.mark.parametrize("nb", [16, 4])
@pytest.mark.parametrize("K,P", [(3, 64), (5, 5), (2, 256)])
def test_multikey_bytes(dcf, nb, K, P):
    """Key-major digest offsets: few keys, the last level of one key next to the first of the next;
    per-key top trees (P >= 32) and the root start (P = 5)."""
    import torch
    rng = np.random.default_rng(0x3700 + 1000 * nb + 10 * K + P)
    keys = [rng.bytes(32) for _ in range(2)]
    prg, Po = dcf.Aes256HirosePrg(keys, 16), O.OraclePrg(keys, 16)
    prg.set_eval_mode(EVAL_STREAM)
    d = dcf.DcfImpl(nb, 16, prg)
    r = lambda shape: rng.integers(0, 256, size=shape, dtype=np.uint8)  # noqa: E731
    alpha, beta, s0, s1 = r((K, nb)), r((K, 16)), r((K, 16)), r((K, 16))
    T = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    cwb = d.gen_batch_device(T(alpha), T(beta), T(s0), T(s1), dcf.BoundState(1))
    xs = r((K * P, nb))
    pat = patterned(nb)
    for key in range(K):
        for i in range(min(P, len(pat))):
            xs[key * P + i] = np.frombuffer(pat[(i + key) % len(pat)], np.uint8)
    y0 = d.eval_multikey_device(False, cwb, T(s0), T(xs), P)
    y1 = d.eval_multikey_device(True, cwb, T(s1), T(xs), P)
    torch.cuda.synchronize()
    y0h, y1h = y0.cpu().numpy(), y1.cpu().numpy()
    for key in range(K):
        ok = O.gen(Po, alpha[key].tobytes(), beta[key].tobytes(), s0[key].tobytes(), s1[key].tobytes(), 1)
        sl = slice(key * P, (key + 1) * P)
        assert np.array_equal(y0h[sl], O.eval_(Po, 0, ok, s0[key].tobytes(), xs[sl])), key
        assert np.array_equal(y1h[sl], O.eval_(Po, 1, ok, s1[key].tobytes(), xs[sl])), key
