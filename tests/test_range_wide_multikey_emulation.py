"""The multi-key indexing of the LAMBDA >= 32 range tree (kernels_range_wide.h under RangeDigKeys)
restated in Python around the single-key emulation of tests/test_range_wide_emulation.py, without
a GPU: every node buffer holds the keys of a launch group one after another, each in leaf order, so
node j of a level with `per` nodes per key belongs to key j // per; root r of key `key` is row
key * nroots + r of the t-vector prefixes, which the tail finds again as j >> rsh; leaf g of a key
is that key's output g - skip, kept only below count, at row key * count + (g - skip) of ys and of
the t-vector buffer.  Every row of every key is compared with the oracle's eval of that key, and
the executed AES-256 blocks with keys * nroots * (4 (8N - h) + 4 (2^h - 1))."""
import numpy as np

from oracle import oracle as O
from tests.test_range_wide_emulation import TAIL, TW, Emu


def rule(nb: int, K: int, count: int) -> int:
    """include/dcf_hip.h, dcf_eval_range_wide_multikey_subtree_levels."""
    if count >= 1 << 12:
        return min(8 * nb, 14, max(8, count.bit_length() - 1 - 8))
    if count < 64 or K * count < 1 << 12:
        return 0
    return min(8 * nb, 14, count.bit_length() - 1 - 2)


def group_eval(emus, nb, x0, count, h):
    """One launch group: emus[key] steps the nodes of key `key`.  Returns the group's ys rows
    (bytes [0, 32)) and t-vector rows, keys * count of each."""
    n, keys = 8 * nb, len(emus)
    w0 = (n - h + 1) >> 4
    skip = x0 & ((1 << h) - 1)
    nroots = ((skip + count - 1) >> h) + 1
    # roots: lane r of keys * nroots walks root r - key * nroots of key r // nroots
    nodes, tpre = [None] * (keys * nroots), [None] * (keys * nroots)
    for r in range(keys * nroots):
        key = r // nroots
        (nodes[r],), (tpre[r],) = emus[key].roots((x0 >> h) + r - key * nroots, n - h, 1)
    # levels: parent j of keys * per, children rows 2j and 2j + 1
    for k in range(h - TAIL):
        per = nroots << k
        out = [None] * (2 * len(nodes))
        for j, node in enumerate(nodes):
            out[2 * j], out[2 * j + 1] = emus[j // per]._kids(node, n - h + k, w0)
        nodes = out
    # tail: node j is node j - key * per of key j // per; its root's prefix is row j >> rsh of tpre
    per, rsh = nroots << (h - TAIL), h - TAIL
    assert len(nodes) == keys * per
    ys, tv = [None] * (keys * count), [None] * (keys * count)
    for j, node in enumerate(nodes):
        key = j // per
        assert j >> rsh == key * nroots + ((j - key * per) >> rsh)
        # Emu.tail on this one node: its first leaf is g = (j - key * per) << TAIL of the key, so the
        # node counts as node 0 with that much less to skip (32-bit, as the kernel's o0)
        o0 = (((j - key * per) << TAIL) - skip) & 0xFFFFFFFF
        y1, t1 = emus[key].tail([node], [tpre[j >> rsh]], n - TAIL, w0, 31, (-o0) & 0xFFFFFFFF, count)
        for i in range(count):
            if y1[i] is not None:
                assert ys[key * count + i] is None, "a leaf is written once"
                ys[key * count + i], tv[key * count + i] = y1[i], t1[i]
    assert all(y is not None for y in ys), "every output of every key is written"
    return ys, tv, nroots


def test_three_keys_key_major_rows_match_the_oracle():
    nb, lam, K, count, x0 = 2, 48, 3, 100, 0x1F37
    h = 4  # the height a call of 41 such keys takes; the indexing is the same for 3
    assert rule(nb, 41, count) == h and rule(nb, 40, count) == 0
    rng = np.random.default_rng(3900)
    P = O.OraclePrg([rng.bytes(32) for _ in range(18)], lam)
    xs = np.frombuffer(b"".join((x0 + i).to_bytes(nb, "big") for i in range(count)), np.uint8).reshape(-1, nb)
    alphas = [x0 + 17, x0 - 1, x0 + count - 1]  # inside, outside, on the last point
    oks, seeds = [], []
    for k in range(K):
        sd = [rng.bytes(lam), rng.bytes(lam)]
        oks.append(O.gen(P, alphas[k].to_bytes(nb, "big"), rng.bytes(lam), sd[0], sd[1], k % 2))
        seeds.append(sd)
    for b in (0, 1):
        emus = [Emu(P, oks[k], seeds[k][b], b, nb) for k in range(K)]
        ys, tv, nroots = group_eval(emus, nb, x0, count, h)
        assert nroots == 7 and x0 % 16 == 7 and (x0 + count) % 16 != 0  # both edge blocks clipped
        assert sum(e.blocks for e in emus) == K * nroots * (4 * (8 * nb - h) + 4 * ((1 << h) - 1))
        for k in range(K):
            want = O.eval_(P, b, oks[k], seeds[k][b], xs, nthreads=4)
            head = np.frombuffer(b"".join(ys[k * count:(k + 1) * count]), np.uint8).reshape(count, 32)
            bad = np.flatnonzero((head != want[:, :32]).any(axis=1))
            assert bad.size == 0, ("bytes [0,32)", "key", k, "party", b, "first mismatching i", bad[:8])
            rows = tv[k * count:(k + 1) * count]
            assert all(len(r) == TW for r in rows)
            tail = emus[k].wide_tail(rows)
            bad = np.flatnonzero((tail != want[:, 32:]).any(axis=1))
            assert bad.size == 0, ("bytes [32,lam)", "key", k, "party", b, "first mismatching i", bad[:8])
