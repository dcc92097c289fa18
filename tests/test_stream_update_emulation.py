"""CPU emulation of the mask-form level update of k_eval16_stream (dcf_amd/csrc/kernels_stream.h,
stream_run: from the d words through the reuse section to L.lev = nl) against the second oracle
restatement (oracle/pyref.py, lib.rs:163-204).  Word for word the kernel's mask algebra: every
condition is a 0 / ~0 word, every word of s and v is updated by the same three-input expressions
(bop3), kMaskLast enters through word 3's masks only.  run=True is the run-reuse form (a whole run
of right steps at t = 0 without an AES slot), run=False the single reused step.  stream_eval also
returns the number of AES blocks the stream encrypts for the point, which the GPU test
(test_stream_update_gpu.py) sets against the kernel's own count."""
import random

import pytest

from oracle import pyref

M3 = 0xFEFFFFFF  # kMaskLast: bit 0 of byte 15 in little-endian word 3
F = 0xFFFFFFFF


def _w(b: bytes):
    return [int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(4)]


def _b(w):
    return b"".join(x.to_bytes(4, "little") for x in w)


def _bswap(x):
    return int.from_bytes(x.to_bytes(4, "little"), "big")


def _sar31(x):  # (int32)x >> 31
    return F if x >> 31 else 0


def _neg(x):
    return (-x) & F


def _clz(x):  # __clz: 32 for 0
    return 32 - x.bit_length()


def stream_eval(aes, s, v, t, lev, x, cws, np1, run, fresh=True):
    """One point from state (s, v, t) at level `lev` (0: the root, with `fresh` as the kernel's
    x-in-registers instance without a prefix table sets it; > 0: a prefix-table row).  Returns
    (y, blocks)."""
    nb = len(x)
    nlev = 8 * nb
    raw = x + bytes((-nb) % 4) + bytes(16)
    xw = [int.from_bytes(raw[4 * k:4 * k + 4], "little") if 4 * k < nb else 0 for k in range(4)]
    cw = [(_w(c[0]), _w(c[1]), int(c[2]) | (int(c[3]) << 1)) for c in cws]
    cw.append(([0] * 4, [0] * 4, 0))  # the unclamped next-level load at the last level: never used
    s, v, t = list(s), list(v), int(t)
    ph, cur = 0, 0
    if not fresh:  # stream_start below a prefix: word 0 consumed, shifted past the prefix bits
        assert lev < 32
        cur = (_bswap(xw[0]) << lev) & F
        xw[0], xw[1], xw[2] = xw[1], xw[2], xw[3]
    enc = lambda w: _w(aes.encrypt(_b(w)))  # noqa: E731
    blocks = 0

    def next_word():
        nonlocal cur
        cur = _bswap(xw[0])
        xw[0], xw[1], xw[2] = xw[1], xw[2], xw[3]

    while lev < nlev:
        blocks += 1
        cs, cv, ct = cw[lev]
        cs2, cv2, ct2 = cw[lev + 1]
        st = enc([w ^ ((ph - 1) & F) for w in s])
        fm = 0
        if fresh:
            fm = F
            next_word()
            fresh = False
        pm = _neg(ph)
        xm = _sar31(cur)
        tm = _neg(t)
        am = F & (pm | xm)  # alive
        adv = am & 1
        inv = ~pm & F
        ik = ~(pm | xm) & F
        itm, apm, atm = tm & ~pm & F, am & pm, am & tm
        ikw = [ik, ik, ik, ik & M3]
        invw = [inv, inv, inv, inv & M3]
        apmw = [apm, apm, apm, apm & M3]
        s3bad = F if (s[3] >> 24) & 1 else 0
        rm = (am & ~pm & ~tm & F) & ~s3bad & ~fm & F
        d = [st[j] ^ s[j] ^ inv for j in range(4)]
        d0 = d[0]
        for j in range(4):
            vj = v[j] ^ (st[j] & ikw[j])
            vj = vj ^ (invw[j] & ~s[j] & F)
            v[j] = vj ^ (cv[j] & itm)
            sj = s[j]
            if j == 3:
                sj &= (~am & F) | M3
            sj = sj ^ (st[j] & apmw[j])
            s[j] = sj ^ (cs[j] & atm)
        tb = d0 ^ (t & (ct >> (xm & 1)))
        t = (t & ~adv) | (tb & adv)
        nl = lev + adv
        cur = (cur << adv) & F
        if adv and (nl & 31) == 0:
            next_word()
        # reuse
        t1, tm1 = t, _neg(t)
        ones = _clz(~cur & F) if run else cur >> 31
        klim = (rm & (tm1 ^ 32) & 33) if run else (rm & 1)
        k = min(ones, nlev - nl, klim)
        ko = F if k & 1 else 0
        nl += k
        cur = (cur << k) & F
        cross = k != 0 and (nl & 31) == 0
        below = _sar31((nl - nlev) & F)
        xm2 = _sar31(cur)
        lm0 = (rm & below) & ~xm2 & ~((tm1 & ko) if run else ko) & F
        lm = 0 if cross else lm0
        vm2, sm = tm1 & (ko | lm), tm1 & ko
        kow = [ko, ko, ko, ko & M3]
        lmw = [lm, lm, lm, lm & M3]
        for j in range(4):
            vj = v[j] ^ (kow[j] & ~s[j] & F)
            vj = vj ^ (d[j] & lmw[j])
            v[j] = vj ^ (cv2[j] & vm2)
            s[j] = s[j] ^ (cs2[j] & sm)
        c = sm & 1
        t = (t1 & ~c) | ((d0 ^ (ct2 >> 1)) & c)
        ph = (adv ^ 1) | (lm & 1)
        if cross:
            next_word()
        assert nl <= nlev, (nl, nlev)
        assert t in (0, 1) and ph in (0, 1)
        lev = nl
    np_ = _w(np1)
    return _b([v[j] ^ s[j] ^ (np_[j] if t else 0) for j in range(4)]), blocks


def root_eval(aes, party, s0, cws, np1, x, run):
    return stream_eval(aes, _w(s0), [0, 0, 0, 0], party, 0, x, cws, np1, run)


def ones_until(nb, end):
    """x of nb bytes: zero bits, then a run of ones that ends exactly at bit `end` (Msb0, inclusive),
    a zero after it; the run starts 9 bits earlier (or at bit 0)."""
    n = 8 * nb
    bits = [0] * n
    for i in range(max(0, end - 8), end + 1):
        bits[i] = 1
    return bytes(sum(bits[8 * b + i] << (7 - i) for i in range(8)) for b in range(nb))


def patterned(nb):
    """The update's edge patterns: all ones, all zeros, alternating (both phases), and runs of ones
    that end exactly at bits 30, 31, 32, 33, 63, 64, 126, 127 (those inside 8 * nb bits)."""
    xs = [b"\xff" * nb, bytes(nb), b"\xaa" * nb, b"\x55" * nb]
    for e in (30, 31, 32, 33, 63, 64, 126, 127):
        if e < 8 * nb:
            xs.append(ones_until(nb, e))
            # the same run preceded by ones from bit 0: one long run across the words
            n = 8 * nb
            bits = [1] * (e + 1) + [0] * (n - e - 1)
            xs.append(bytes(sum(bits[8 * b + i] << (7 - i) for i in range(8)) for b in range(nb)))
    return xs


@pytest.mark.parametrize("bound", [0, 1], ids=["LtBeta", "GtBeta"])
@pytest.mark.parametrize("nb", range(1, 17))
def test_update_matches_oracle(nb, bound):
    rnd = random.Random(0x5EED00 + 2 * nb + bound)
    lam = 16
    keys = [rnd.randbytes(32) for _ in range(2)]
    prg = pyref.HirosePrg(keys, lam)
    aes = pyref.Aes256Ecb(keys[0])
    alpha, beta = rnd.randbytes(nb), rnd.randbytes(lam)
    s0s = [rnd.randbytes(lam), rnd.randbytes(lam)]
    cws, np1 = pyref.gen(prg, alpha, beta, s0s, bound)
    xs = patterned(nb) + [alpha] + [rnd.randbytes(nb) for _ in range(200)]
    for party in (0, 1):
        ref = pyref.eval_(prg, bool(party), s0s[party], cws, np1, xs)
        tot = {}
        for run in (False, True):
            got = [root_eval(aes, party, s0s[party], cws, np1, x, run) for x in xs]
            assert [g[0] for g in got] == ref, (party, run)
            tot[run] = [g[1] for g in got]
            # every slot is a used block: at most B and A per level, at least one per x word
            assert all(-(-nb // 4) <= b <= 16 * nb for b in tot[run])
        # run reuse never encrypts more (how much less it encrypts at t = 0 is pinned below)
        assert all(a <= b for a, b in zip(tot[True], tot[False]))


def test_run_reuse_counts_on_all_ones():
    """All-ones x from a masked seed at t = 0 and lsb(B ^ ~s) = 0: the run form needs one block per
    x word after the root step, the single-step form one per two levels."""
    rnd = random.Random(0xA110)
    lam, nb = 16, 16
    keys = [rnd.randbytes(32) for _ in range(2)]
    prg = pyref.HirosePrg(keys, lam)
    aes = pyref.Aes256Ecb(keys[0])
    s0s = [rnd.randbytes(lam), rnd.randbytes(lam)]
    cws, np1 = pyref.gen(prg, rnd.randbytes(nb), rnd.randbytes(lam), s0s, 0)
    x = b"\xff" * nb
    for _ in range(64):  # a seed with the masked bit clear whose B keeps t = 0
        s = _w(rnd.randbytes(15) + bytes([rnd.getrandbits(8) & 0xFE]))
        b0 = _w(aes.encrypt(_b([w ^ F for w in s])))[0] ^ s[0] ^ F
        if b0 & 1 == 0:
            break
    else:
        raise AssertionError("no such seed in 64 draws")
    y1, n1 = stream_eval(aes, s, [0] * 4, 0, 0, x, cws, np1, True)
    y0, n0 = stream_eval(aes, s, [0] * 4, 0, 0, x, cws, np1, False)
    assert y0 == y1
    assert (n1, n0) == (5, 65)  # root step (never reuses: the x word is fresh), then 1 + 3 / 64
