"""The range-eval tree path of the Hirose PRG at LAMBDA >= 32 restated in Python on OraclePrg.gen,
without a GPU (kernels_range_wide.h): the root walk, the breadth-first levels on 80-byte rows
(s[0:32) | v[0:32) | t, q0, q1), the clipped leaves of the depth-first tail, the assembly of a leaf's
t-vector row from its root's prefix and the two words q0, q1 that the subtree's bits fall into, and
bytes [32, LAMBDA) as the GF(2) combination of W rows that the tail kernels compute from that row
(kernels_wide.h).

It pins the row form and the nibble positions of the subtree's t bits: row r of the t-sequence is
bit 8 ((r >> 2) & 3) + (r & 3) of word r >> 4.  Bytes [0, 32) and [32, LAMBDA) are compared with the
oracle's eval separately, and the executed AES-256 blocks with the formula the device counter is
held to."""
import numpy as np
import pytest

from oracle import oracle as O

TAIL, TW = 2, 16  # register depth of the tail, words of a t-vector row
M32 = (1 << 256) - 1


def rule(nb: int, count: int) -> int:
    """include/dcf_hip.h: h = 0 below 2^12 points, else min(8N, 14, max(8, floor(log2 count) - 8))."""
    if count < 1 << 12:
        return 0
    return min(8 * nb, 14, max(8, count.bit_length() - 1 - 8))


def _i(b) -> int:
    return int.from_bytes(bytes(b), "little")


def tbit(row: int) -> int:
    return 8 * ((row >> 2) & 3) + (row & 3)


class Emu:
    """One key, one party.  A node is (s, v, t, q0, q1): s and v the first 32 bytes as little-endian
    integers.  `blocks` counts what the kernels execute: 4 per stepped node."""

    def __init__(self, P, ok, s0: bytes, party: int, nb: int):
        self.P, self.ok, self.party, self.s0, self.blocks = P, ok, party, s0, 0
        self.lam, self.n = P.lam, 8 * nb
        self.cs = [_i(r[:32]) for r in ok.cw_s]
        self.cv = [_i(r[:32]) for r in ok.cw_v]
        self.ct = [int(t) for t in ok.cw_t]
        self.np1 = _i(ok.cw_np1[:32])

    def _children(self, s: int, v: int, t: int, lev: int):
        """Bytes [0, 32) of both children: they depend on bytes [0, 32) of the seed alone."""
        m = M32 if t else 0
        outs = self.P.gen(s.to_bytes(32, "little") + bytes(self.lam - 32))
        self.blocks += 4
        return [(_i(cs[:32]) ^ (m & self.cs[lev]), v ^ _i(cv[:32]) ^ (m & self.cv[lev]),
                 int(ct) ^ (t & (self.ct[lev] >> side) & 1)) for side, (cs, cv, ct) in enumerate(outs)]

    def roots(self, pfx: int, nwalk: int, nroots: int):
        """Nodes of level nwalk with prefixes pfx .. pfx + nroots - 1 and their t-vector prefixes
        (rows 0 .. nwalk, TW words, the rest zero)."""
        nodes, pre = [], []
        for p in range(pfx, pfx + nroots):
            s, v, t = _i(self.s0[:32]), 0, self.party
            row, tacc = [0] * TW, self.party
            for lev in range(nwalk):
                s, v, t = self._children(s, v, t, lev)[(p >> (nwalk - 1 - lev)) & 1]
                r = lev + 1
                tacc |= t << tbit(r)
                if r & 15 == 15:
                    row[r >> 4], tacc = tacc, 0
            if nwalk & 15 != 15:
                row[nwalk >> 4] = tacc
            nodes.append((s, v, t, tacc, 0))
            pre.append(row)
        return nodes, pre

    def _kids(self, node, lev: int, w0: int):
        s, v, t, q0, q1 = node
        out = []
        for cs, cv, ct in self._children(s, v, t, lev):
            r = lev + 1
            hi = (r >> 4) != w0
            assert (r >> 4) - w0 in (0, 1)
            out.append((cs, cv, ct, q0 if hi else q0 | ct << tbit(r), q1 | ct << tbit(r) if hi else q1))
        return out

    def level(self, nodes, lev: int, w0: int):
        return [kid for node in nodes for kid in self._kids(node, lev, w0)]

    def leaf(self, node):
        s, v, t = node[:3]
        return (v ^ s ^ (self.np1 if t else 0)).to_bytes(32, "little")

    def tail(self, nodes, pre, lev0: int, w0: int, rsh: int, skip: int, count: int):
        """The last TAIL levels below each node, depth-first; leaf g of the launch is output g - skip,
        kept only below count (32-bit arithmetic, as the kernel's).  Returns y[0:32) and the t rows."""
        ys, tv = [None] * count, [None] * count
        for j, node in enumerate(nodes):
            stack = [(node, 0, j << TAIL)]
            while stack:
                nd, k, g = stack.pop()
                kids = self._kids(nd, lev0 + k, w0)
                if k + 1 == TAIL:
                    for side, kid in enumerate(kids):
                        o = (g + side - skip) & 0xFFFFFFFF
                        if o < count:
                            ys[o] = self.leaf(kid)
                            row = list(pre[j >> rsh])
                            row[w0] = kid[3]
                            if w0 + 1 < TW:
                                row[w0 + 1] = kid[4]
                            tv[o] = row
                else:
                    stack.append((kids[1], k + 1, g + (1 << (TAIL - 1 - k))))
                    stack.append((kids[0], k + 1, g))
        return ys, tv

    def wide_tail(self, tv):
        """y[32, LAMBDA) from the t rows (kernels_wide.h): s0 with the PRG's cleared bit, XOR W_r over
        the rows r with t_r = 1; W_r = cw_v[r] ^ (r + 1 even ? cw_s[r] : 0) below n, cw_np1 at n, and the
        cleared bit takes cw_s at r + 1 == n only."""
        n, lam, ok = self.n, self.lam, self.ok
        W = np.zeros((n + 1, lam), np.uint8)
        for r in range(n):
            W[r] = ok.cw_v[r] ^ (ok.cw_s[r] if (r + 1) % 2 == 0 else 0)
            bit = (ok.cw_v[r][lam - 1] ^ (ok.cw_s[r][lam - 1] if r + 1 == n else 0)) & 1
            W[r][lam - 1] = (W[r][lam - 1] & 0xFE) | bit
        W[n] = ok.cw_np1
        c = np.frombuffer(self.s0, np.uint8).copy()
        c[lam - 1] &= 0xFE
        out = np.zeros((len(tv), lam - 32), np.uint8)
        for o, row in enumerate(tv):
            y = c.copy()
            for r in range(n + 1):
                if (row[r >> 4] >> tbit(r)) & 1:
                    y ^= W[r]
            assert not any(row[(n >> 4) + 1:]), "words past row 8N are zero"
            out[o] = y[32:]
        return out


def range_eval(P, ok, s0, party, nb, x0, count):
    n, h = 8 * nb, rule(nb, count)
    e = Emu(P, ok, s0, party, nb)
    if h == 0:  # leaf mode: the roots are the points and their prefixes the whole t rows
        nodes, tv = e.roots(x0, n, count)
        ys = [e.leaf(nd) for nd in nodes]
        assert e.blocks == 4 * n * count
    else:
        assert h >= TAIL
        w0 = (n - h + 1) >> 4
        skip = x0 & ((1 << h) - 1)
        nroots = ((skip + count - 1) >> h) + 1
        nodes, pre = e.roots(x0 >> h, n - h, nroots)
        for k in range(h - TAIL):
            nodes = e.level(nodes, n - h + k, w0)
        ys, tv = e.tail(nodes, pre, n - TAIL, w0, h - TAIL, skip, count)
        assert e.blocks == nroots * (4 * (n - h) + 4 * ((1 << h) - 1))
        assert 2 * count <= e.blocks
    head = np.frombuffer(b"".join(ys), np.uint8).reshape(count, 32)
    return head, (e.wide_tail(tv) if P.lam > 32 else None), h


CASES = [
    # nb, lam, x0, count, h: an unaligned x0 at N = 16 whose range crosses 2^h boundaries
    (16, 32, (0x5A17 << 100) | 0x3F9D, 4200, 8),
    (16, 128, (0x5A17 << 100) | 0x3F9D, 4200, 8),
    (1, 128, 0, 256, 0),               # a whole N = 1 domain: leaf mode with a tail
    (1, 32, 0, 256, 0),
    (2, 48, 65536 - 4500, 4500, 8),    # the last block ends the domain; row 8N = 16 opens word 1
    (3, 64, (1 << 24) - 4100, 4100, 8),  # 8N = 24: the subtree's rows 17 .. 24 lie in one word
]


@pytest.mark.parametrize("nb,lam,x0,count,h", CASES)
def test_three_stages_and_t_vectors_match_the_oracle(nb, lam, x0, count, h):
    rng = np.random.default_rng(3100 + nb + lam)
    P = O.OraclePrg([rng.bytes(32) for _ in range(18)], lam)
    xs = np.frombuffer(b"".join((x0 + i).to_bytes(nb, "big") for i in range(count)), np.uint8).reshape(-1, nb)
    for bound in (0, 1):
        alpha = x0 + int(rng.integers(0, count))
        beta, seeds = rng.bytes(lam), [rng.bytes(lam), rng.bytes(lam)]
        ok = O.gen(P, alpha.to_bytes(nb, "big"), beta, seeds[0], seeds[1], bound)
        for b in (0, 1):
            head, tail, got_h = range_eval(P, ok, seeds[b], b, nb, x0, count)
            assert got_h == h
            want = O.eval_(P, b, ok, seeds[b], xs, nthreads=4)
            bad = np.flatnonzero((head != want[:, :32]).any(axis=1))
            assert bad.size == 0, ("bytes [0,32)", hex(x0), count, bound, b, "first mismatching i", bad[:8])
            if lam > 32:
                bad = np.flatnonzero((tail != want[:, 32:]).any(axis=1))
                assert bad.size == 0, ("bytes [32,lam)", hex(x0), count, bound, b, "first mismatching i", bad[:8])
