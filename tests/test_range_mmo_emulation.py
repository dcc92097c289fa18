"""The MMO range-eval tree path restated in Python on OracleMmoPrg.gen, without a GPU: the root walk
(two blocks per level), the breadth-first level expansion on packed 32-byte rows with t in bit 24
of the seed's last word, and the clipped leaves of the depth-first tail (kernels_range_mmo.h and
the RangeMmo instances of kernels_range.h).

It pins the row format: every child seed has bit 0 of byte 15 cleared by the PRG and cw_s is the XOR
of two such seeds, so that bit is free in every row the stages write; v is not clean, so t cannot
ride there.  The outputs are compared with the oracle's eval bit for bit and the executed AES-128
blocks with the formula the device counter is held to."""
import numpy as np
import pytest

from oracle import oracle as O

LAM, TAIL = 16, 4
T_BIT = 1 << 120  # bit 0 of byte 15: bit 24 of word 3 of the row's first 16 bytes, read little-endian
ONES = (1 << 128) - 1


def rule(nb: int, count: int) -> int:
    """include/dcf_hip.h: h = 0 below 2^12 points, else min(8N, 14, max(8, floor(log2 count) - 8))."""
    if count < 1 << 12:
        return 0
    return min(8 * nb, 14, max(8, count.bit_length() - 1 - 8))


def _i(b) -> int:
    return int.from_bytes(bytes(b), "little")


class Emu:
    """One key, one party; 16-byte values as little-endian integers, a row as the pair (s with t in
    T_BIT, v).  `blocks` counts what the kernels execute: 2 per walk step, 4 per expanded node."""

    def __init__(self, P, ok, s0: bytes, party: int):
        self.P, self.party, self.s0, self.blocks = P, party, s0, 0
        self.cs = [_i(r) for r in ok.cw_s]
        self.cv = [_i(r) for r in ok.cw_v]
        self.ct = [int(t) for t in ok.cw_t]
        self.np1 = _i(ok.cw_np1)
        assert not any(c & T_BIT for c in self.cs)  # the row-format argument: cw_s never touches the t bit

    def _children(self, s: int, v: int, t: int, lev: int):
        m = ONES if t else 0
        return [(_i(cs) ^ (m & self.cs[lev]), v ^ _i(cv) ^ (m & self.cv[lev]), int(ct) ^ (t & (self.ct[lev] >> side) & 1))
                for side, (cs, cv, ct) in enumerate(self.P.gen(s.to_bytes(16, "little")))]

    @staticmethod
    def pack(s, v, t):
        assert not s & T_BIT, "a seed below s0 carries the t bit"
        return s | (T_BIT if t else 0), v

    @staticmethod
    def unpack(row):
        return row[0] & ~T_BIT, row[1], 1 if row[0] & T_BIT else 0

    def roots(self, pfx: int, nwalk: int, nroots: int):
        """Rows of the nodes of level nwalk with prefixes pfx .. pfx + nroots - 1, bits Msb-first."""
        assert nwalk >= 1
        rows = []
        for p in range(pfx, pfx + nroots):
            s, v, t = _i(self.s0), 0, self.party
            for lev in range(nwalk):
                s, v, t = self._children(s, v, t, lev)[(p >> (nwalk - 1 - lev)) & 1]
                self.blocks += 2  # the side's s and v blocks
            rows.append(self.pack(s, v, t))
        return rows

    def level(self, rows, lev: int):
        """in[j] -> out[2j], out[2j + 1]."""
        out = []
        for row in rows:
            out += [self.pack(*kid) for kid in self._children(*self.unpack(row), lev)]
            self.blocks += 4
        return out

    def tail(self, rows, lev0: int, skip: int, count: int) -> np.ndarray:
        """The last TAIL levels below each row, depth-first; leaf g of the launch is output g - skip,
        kept only below count (32-bit arithmetic, as the kernel's)."""
        ys = [bytes(LAM)] * count
        for j, row in enumerate(rows):
            stack = [(row, 0, j << TAIL)]  # the stack holds rows, as the kernel's registers do
            while stack:
                node, k, g = stack.pop()
                kids = self._children(*self.unpack(node), lev0 + k)
                self.blocks += 4
                if k + 1 == TAIL:
                    for side, (ls, lv, lt) in enumerate(kids):
                        o = (g + side - skip) & 0xFFFFFFFF
                        if o < count:
                            ys[o] = (lv ^ ls ^ (self.np1 if lt else 0)).to_bytes(LAM, "little")
                else:
                    stack.append((self.pack(*kids[1]), k + 1, g + (1 << (TAIL - 1 - k))))
                    stack.append((self.pack(*kids[0]), k + 1, g))
        return np.frombuffer(b"".join(ys), np.uint8).reshape(count, LAM)


def range_eval(P, ok, s0, party, nb, x0, count):
    h = rule(nb, count)
    assert h >= TAIL
    e = Emu(P, ok, s0, party)
    skip = x0 & ((1 << h) - 1)
    nroots = ((skip + count - 1) >> h) + 1
    rows = e.roots(x0 >> h, 8 * nb - h, nroots)
    for k in range(h - TAIL):
        rows = e.level(rows, 8 * nb - h + k)
    ys = e.tail(rows, 8 * nb - TAIL, skip, count)
    assert e.blocks == nroots * (2 * (8 * nb - h) + 4 * ((1 << h) - 1))
    return ys, e.blocks, h


@pytest.mark.parametrize("x0,count", [(0x1F37, 5000), (0, 1 << 16)])
def test_three_stages_match_the_oracle(x0, count):
    nb = 2
    rng = np.random.default_rng(2300 + count)
    keys = [rng.bytes(16) for _ in range(4)]
    P = O.OracleMmoPrg(keys, LAM)
    xs = np.frombuffer(b"".join((x0 + i).to_bytes(nb, "big") for i in range(count)), np.uint8).reshape(-1, nb)
    alphas = (x0 + int(rng.integers(0, count)), x0, x0 + count - 1)  # inside and on both edges
    for k, alpha in enumerate(alphas):
        beta, seeds = rng.bytes(LAM), [rng.bytes(LAM), rng.bytes(LAM)]
        ok = O.gen(P, alpha.to_bytes(nb, "big"), beta, seeds[0], seeds[1], k % 2)
        # both parties on the short range; one per key on the whole domain (each costs 2^16 PRG calls)
        for b in ((0, 1) if count < (1 << 13) else (k % 2,)):
            ys, blocks, h = range_eval(P, ok, seeds[b], b, nb, x0, count)
            assert h == 8
            assert 2 * count <= blocks <= 5 * count
            want = O.eval_(P, b, ok, seeds[b], xs, nthreads=4)
            bad = np.flatnonzero((ys != want).any(axis=1))
            assert bad.size == 0, (hex(x0), count, "key", k, "party", b, "first mismatching i", bad[:8])


def test_v_rows_are_not_clean():
    """Why t rides in the seed row: cw_v carries beta, so bit 0 of byte 15 of a v row is data."""
    rng = np.random.default_rng(2400)
    P = O.OracleMmoPrg([rng.bytes(16) for _ in range(4)], LAM)
    hit = False
    for _ in range(8):
        ok = O.gen(P, rng.bytes(2), rng.bytes(LAM), rng.bytes(LAM), rng.bytes(LAM), 0)
        assert not (ok.cw_s[:, 15] & 1).any()
        hit |= bool((ok.cw_v[:, 15] & 1).any())
    assert hit
