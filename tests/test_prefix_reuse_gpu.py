"""The cross-call shared-prefix table of dcf_eval_device (include/dcf_hip.h): kept while the key
material is unchanged, rebuilt when the key buffer is rewritten in place, deepened by the policy
of tests/test_prefix_reuse.py.  Every output is compared with the oracle on sampled rows and, in
full, with a fresh prg that builds its own table in the same call; the device's AES block count
is pinned exactly: the walk at the depth really used, plus the build or deepening that really ran.

Shapes: the smallest that take the table path on the stream engine (more than CUS * 1024 * 2
points), N = 16 and N = 4 (x in one word, rows staged through the LDS)."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

SMALL = 256 * 1024 * 2          # below this the small-batch pair path runs (no cross-call table)
M_LATE = SMALL + 1000           # D = 19; deepened after 2 calls at 19, 4 at 20
M_SOON = (1 << 20) - 1000       # D = 19; deepened after 1 call at 19, 2 at 20


@pytest.fixture(scope="module")
def dcf(hip_lib):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import dcf_amd
    return dcf_amd


def table_blocks(depth):
    return 2 ** (depth + 1) - 2


class Rig:
    """One long-lived prg under test, the oracle's prg and one batch of points per call."""

    def __init__(self, dcf, nb, m, seed, levels=-1):
        import torch
        self.dcf, self.nb, self.m, self.torch = dcf, nb, m, torch
        self.rng = np.random.default_rng(seed)
        self.keys = [self.rng.bytes(32) for _ in range(2)]
        self.prg, self.Po = dcf.Aes256HirosePrg(self.keys, 16), O.OraclePrg(self.keys, 16)
        if levels != -1:
            self.prg.set_prefix_levels(levels)
        self.prg.set_phase_timing(True)
        self.d = dcf.DcfImpl(nb, 16, self.prg)
        self.d0 = self.prg.eval_prefix_levels(nb, 1, m)

    def T(self, b):
        return self.torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()

    def key(self, alpha=None, beta=None, s0s=None):
        """(oracle key, cwb bytes, [s0, s1], alpha)."""
        alpha = alpha or self.rng.bytes(self.nb)
        beta = beta or self.rng.bytes(16)
        s0s = s0s or [self.rng.bytes(16), self.rng.bytes(16)]
        ok = O.gen(self.Po, alpha, beta, s0s[0], s0s[1], 1)
        k = self.d.gen(self.dcf.CmpFn(alpha, beta), s0s, self.dcf.BoundState(1))
        return ok, self.dcf.share_to_cwb(k, self.nb, 16), s0s, alpha

    def points(self, alpha=None):
        xs = self.rng.integers(0, 256, size=(self.m, self.nb), dtype=np.uint8)
        xs[0], xs[-1] = 0, 0xFF
        if alpha is not None:
            xs[1] = np.frombuffer(alpha, np.uint8)
        return xs

    def walk(self, party, cwb, s0, xs_t, depth):
        """The same eval on a fresh prg at forced depth, where the block count is the walk's alone
        (include/dcf_hip.h, dcf_prg_last_eval_blocks); and its output."""
        prg = self.dcf.Aes256HirosePrg(self.keys, 16)
        prg.set_prefix_levels(depth)
        ys = self.dcf.DcfImpl(self.nb, 16, prg).eval_device(bool(party), cwb.clone(), s0.clone(), xs_t)
        self.torch.cuda.synchronize()
        return ys, prg.last_eval_blocks()

    def check(self, what, party, ok, seed, xs, ys, ys_ref):
        assert self.torch.equal(ys, ys_ref), what
        rows = np.r_[0:64, self.rng.integers(0, self.m, size=1024), self.m - 64:self.m]
        want = O.eval_(self.Po, party, ok, seed, xs[rows], nthreads=8)
        idx = self.torch.from_numpy(rows.astype(np.int64)).cuda()
        assert np.array_equal(ys[idx].cpu().numpy(), want), what

    def call(self, what, party, ok, seed, cwb, s0, xs=None):
        """One eval_device call on the long-lived prg: (blocks, depth used, the walk's blocks at
        that depth), outputs checked."""
        xs = self.points() if xs is None else xs
        xs_t = self.torch.from_numpy(xs).cuda()
        ys = self.d.eval_device(bool(party), cwb, s0, xs_t)
        self.torch.cuda.synchronize()
        blocks, depth = self.prg.last_eval_blocks(), self.prg.last_eval_phases()[2]
        ys_ref, walk = self.walk(party, cwb, s0, xs_t, depth)
        self.check(what, party, ok, seed, xs, ys, ys_ref)
        print(what, "blocks", blocks, "depth", depth, "walk", walk, "extra", blocks - walk)
        return blocks, depth, walk


def policy_depths(hip_lib, d0, m, calls, dmax=31):
    """Depth of each of `calls` calls with one key: +1 at the start of a call once
    dcf_prefix_deepen_calls calls have walked at the current depth."""
    out, depth, walked = [], d0, 0
    for i in range(calls):
        if i and depth < dmax and walked >= hip_lib.dcf_prefix_deepen_calls(depth, m):
            depth, walked = depth + 1, 0
        out.append(depth)
        walked += 1
    return out


@pytest.mark.parametrize("nb,m", [(16, M_SOON), (16, M_LATE), (4, M_SOON)])
def test_reuse_and_deepening(dcf, hip_lib, nb, m):
    """Same key, fresh points every call: no rebuild after the first call, one level deeper at the
    call the threshold predicts, the counts exact."""
    r = Rig(dcf, nb, m, 0x9E00 + nb + m % 7)
    ok, cwb, s0s, alpha = r.key()
    cwb_t, s0_t = r.T(cwb), r.T(s0s[0])
    ncalls = 4  # M_SOON: the second deepening runs in place, in the room the first one's allocation left
    want = policy_depths(hip_lib, r.d0, m, ncalls)
    assert r.d0 == 19 and want == ([19, 20, 20, 21] if m == M_SOON else [19, 19, 20, 20])
    got = [r.call(("reuse", nb, m, i), 0, ok, s0s[0], cwb_t, s0_t, r.points(alpha)) for i in range(ncalls)]
    assert [g[1] for g in got] == want
    for i, (blocks, depth, walk) in enumerate(got):
        extra = table_blocks(r.d0) if i == 0 else 2 ** depth if depth != got[i - 1][1] else 0
        assert blocks == walk + extra, (i, blocks, walk, extra)
    if m == M_SOON:  # every later call below the first by the table's blocks or more: nothing was rebuilt
        assert all(g[0] <= got[0][0] - table_blocks(r.d0) for g in got[1:]), [g[0] for g in got]


def test_key_rewritten_in_place(dcf, hip_lib):
    """The cwb and s0 tensors stay, their bytes change: a difference in table material (a level
    below the depth, the party, s0) rebuilds at the first call's depth inside the call; a
    difference above level 31 alone does not."""
    nb, m = 16, M_LATE
    r = Rig(dcf, nb, m, 0x9E77)
    ok, cwb, s0s, alpha = r.key()
    cwb_t, s0_t = r.T(cwb), r.T(s0s[0])
    xs = r.points(alpha)
    b, depth, walk = r.call("first", 0, ok, s0s[0], cwb_t, s0_t, xs)
    assert depth == r.d0 and b == walk + table_blocks(r.d0)
    b, depth, walk = r.call("same", 0, ok, s0s[0], cwb_t, s0_t, xs)
    assert depth == r.d0 and b == walk

    def flipped(a, bit):
        a = bytearray(a)
        a[bit // 8] ^= 0x80 >> (bit % 8)
        return bytes(a)

    def first_cw_difference(c0, c1):
        n = 8 * nb
        s = [np.frombuffer(c, np.uint8)[:16 * n].reshape(n, 16) for c in (c0, c1)]
        return int(np.flatnonzero((s[0] != s[1]).any(axis=1))[0])

    # alpha differs at bit 3: the correction words differ from level 3 (< depth) on.  (This is
    # also the call at whose start the host deepens: the deepening must find the other key and
    # leave it to the build.)
    beta = r.rng.bytes(16)
    alpha2 = flipped(alpha, 3)
    ok2, cwb2, _, _ = r.key(alpha2, beta, s0s)
    assert first_cw_difference(cwb, cwb2) <= 3
    cwb_t.copy_(r.T(cwb2))
    xs[1] = np.frombuffer(alpha2, np.uint8)
    b, depth, walk = r.call("level 3", 0, ok2, s0s[0], cwb_t, s0_t, xs)
    assert depth == r.d0 and b == walk + table_blocks(r.d0)
    b, was, walk = r.call("level 3 again", 0, ok2, s0s[0], cwb_t, s0_t, xs)
    assert b == walk + (2 ** was if was != depth else 0)
    # alpha differs at bit 40 only: levels >= 40 > 31 differ, none of them table material
    alpha3 = flipped(alpha2, 40)
    ok3, cwb3, _, _ = r.key(alpha3, beta, s0s)
    assert first_cw_difference(cwb2, cwb3) == 40
    cwb_t.copy_(r.T(cwb3))
    xs[1] = np.frombuffer(alpha3, np.uint8)
    b, depth, walk = r.call("level 40", 0, ok3, s0s[0], cwb_t, s0_t, xs)
    assert depth >= was and b == walk + (2 ** depth if depth != was else 0), (b, walk, depth, was)  # no rebuild
    d_now = depth
    # the party alone
    b, depth, walk = r.call("party", 1, ok3, s0s[0], cwb_t, s0_t, xs)
    assert depth == r.d0 and b == walk + table_blocks(r.d0), (b, walk, depth, d_now)
    # s0 alone
    s0n = r.rng.bytes(16)
    s0_t.copy_(r.T(s0n))
    b, depth, walk = r.call("s0", 1, ok3, s0n, cwb_t, s0_t, xs)
    assert depth == r.d0 and b == walk + table_blocks(r.d0)


def test_key_changes_where_the_host_deepens(dcf, hip_lib):
    """Pointers equal, key rewritten exactly at the call whose start deepens the table: the
    deepening finds another key's rows and does nothing, the build runs at the first call's depth."""
    nb, m = 16, M_SOON
    r = Rig(dcf, nb, m, 0x9E33)
    assert policy_depths(hip_lib, r.d0, m, 2) == [19, 20]
    ok, cwb, s0s, alpha = r.key()
    cwb_t, s0_t = r.T(cwb), r.T(s0s[0])
    xs = r.points(alpha)
    b, depth, walk = r.call("first", 0, ok, s0s[0], cwb_t, s0_t, xs)
    assert depth == 19 and b == walk + table_blocks(19)
    ok2, cwb2, s0s2, alpha2 = r.key()
    cwb_t.copy_(r.T(cwb2))
    s0_t.copy_(r.T(s0s2[0]))
    xs[1] = np.frombuffer(alpha2, np.uint8)
    b, depth, walk = r.call("changed at the deepening call", 0, ok2, s0s2[0], cwb_t, s0_t, xs)
    assert depth == 19 and b == walk + table_blocks(19)
    b, depth, walk = r.call("after", 0, ok2, s0s2[0], cwb_t, s0_t, xs)
    assert depth in (19, 20) and b == walk + (2 ** 20 if depth == 20 else 0)


def test_forced_depth_and_depth_zero(dcf, hip_lib):
    nb, m = 16, M_LATE
    r = Rig(dcf, nb, m, 0x9E44, levels=12)
    ok, cwb, s0s, alpha = r.key()
    cwb_t, s0_t = r.T(cwb), r.T(s0s[0])
    xs = r.points(alpha)
    got = [r.call(("forced", i), 0, ok, s0s[0], cwb_t, s0_t, xs) for i in range(6)]
    assert [g[1] for g in got] == [12] * 6  # never deepened
    assert all(g[0] == g[2] for g in got)    # a forced depth reports the walk alone
    held = r.prg.device_bytes()
    r.prg.set_prefix_levels(0)  # no table, no state: every call walks from the root
    got = [r.call(("off", i), 0, ok, s0s[0], cwb_t, s0_t, xs) for i in range(2)]
    assert [g[1] for g in got] == [0, 0] and got[0][0] == got[1][0] == got[0][2]
    assert r.prg.device_bytes() == held
    r.prg.set_prefix_levels(12)  # the setter reset the state: the first call builds again
    b, depth, walk = r.call("forced again", 0, ok, s0s[0], cwb_t, s0_t, xs)
    assert depth == 12 and b == walk


def test_two_streams_one_prg(dcf):
    """Same key, two calls queued on two streams without synchronising in between (as the deferred
    checks of tests/test_call_sequences_gpu.py): the second call reuses the table the first one is
    still building."""
    import torch
    nb, m = 16, M_SOON
    r = Rig(dcf, nb, m, 0x9E55)
    ok, cwb, s0s, alpha = r.key()
    cwb_t, s0_t = r.T(cwb), r.T(s0s[0])
    xs = [r.points(alpha), r.points(alpha)]
    xt = [torch.from_numpy(x).cuda() for x in xs]
    torch.cuda.synchronize()
    streams, ys = [torch.cuda.Stream(), torch.cuda.Stream()], []
    for s, x in zip(streams, xt):
        with torch.cuda.stream(s):
            ys.append(r.d.eval_device(False, cwb_t, s0_t, x))
    torch.cuda.synchronize()
    for i in range(2):
        ref, _ = r.walk(0, cwb_t, s0_t, xt[i], 19)
        r.check(("stream", i), 0, ok, s0s[0], xs[i], ys[i], ref)


def test_byte_cap_stops_growth(dcf, hip_lib):
    """dcf_prg_set_prefix_max_bytes below what a table one level deeper takes: the depth stays."""
    nb, m = 16, M_SOON
    r = Rig(dcf, nb, m, 0x9E66)
    r.prg.set_prefix_max_bytes(40_000_000)
    assert r.prg.eval_prefix_levels(nb, 1, m) == 19
    assert hip_lib.dcf_prefix_reuse_max_depth(nb, 1 << 50, 40_000_000) == 19
    ok, cwb, s0s, alpha = r.key()
    cwb_t, s0_t = r.T(cwb), r.T(s0s[0])
    xs = r.points(alpha)
    got = [r.call(("cap", i), 0, ok, s0s[0], cwb_t, s0_t, xs) for i in range(4)]
    assert [g[1] for g in got] == [19] * 4
    assert got[0][0] == got[0][2] + table_blocks(19) and all(g[0] == g[2] for g in got[1:])
