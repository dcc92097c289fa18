"""The inputs of tests/test_call_sequences_gpu.py, checked without a GPU: the seeded generator is
deterministic and covers its pool, and every hand-written ladder contains the transitions it is
named for — judged from STEP_BUFFERS, the table of (step kind -> buffers it uses) kept next to the
pool, so that an edit cannot thin a ladder unnoticed."""
import pytest

from tests.test_call_sequences_gpu import (ALL_BUFFERS, CONFIGS, DEFAULT_SEEDS, DEFAULT_STEPS, DEFERRED, EVAL16_FORCED_M,
                                           LADDERS, MK16, SETTINGS, STEP_BUFFERS, STREAM_MIN, Settings, _sequence, engine,
                                           eval_chunk, extent, pool, prefix_depth, stage_path, sweep)

# the suite's defaults as literals: DCF_SEQ_SEED / DCF_SEQ_STEPS (one-off GPU runs) do not reach these checks
SEQ_SEEDS, SEQ_STEPS = DEFAULT_SEEDS, DEFAULT_STEPS
assert (SEQ_SEEDS, SEQ_STEPS) == ((1, 2), 24)


def test_generator_is_deterministic():
    for config in CONFIGS:
        for seed in (1, 2, 77):
            a, b = _sequence(config, seed, 24), _sequence(config, seed, 24)
            assert a == b and len(a) == 24
            assert _sequence(config, seed + 1, 24) != a
        assert not any(s.kind in SETTINGS for s in _sequence(config, 5, 40, settings=False))


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_default_seeds_cover_the_pool(config):
    steps = [s for seed in SEQ_SEEDS for s in _sequence(config, seed, SEQ_STEPS)]
    for kind in pool(config):
        assert sum(s.kind == kind for s in steps) >= 2, (config, kind)
    lam = CONFIGS[config][1]
    for seed in SEQ_SEEDS:
        big = [s for s in _sequence(config, seed, SEQ_STEPS) if max(s.get("m", 0), s.get("count", 0)) > 40000]
        assert len(big) <= (1 if lam == 16 else 0) and all(s.get("m") == STREAM_MIN for s in big)
        assert all(s.get("K", 1) * max(s.get("P", 0), s.get("count", 0)) <= 40000 for s in _sequence(config, seed, SEQ_STEPS))
    if lam == 16:  # the stream step really occurs
        assert any(s.get("m") == STREAM_MIN for s in steps), config
    for s in steps:  # N from the configuration's list; full domain brings its own (1 or 2)
        assert s.get("nb") is None or s.get("nb") in CONFIGS[config][2] + ((1, 2) if s.kind == "full_domain" else ())


def _reached(config):
    """{(kind, shape without N, engine, prefix depth)} over everything the default suite runs on
    this configuration: its ladders, the default random sequences and the sweep."""
    runs = [steps for c, _, steps in LADDERS.values() if c == config]
    runs += [_sequence(config, seed, SEQ_STEPS) for seed in SEQ_SEEDS] + [sweep(config)]
    out = set()
    for steps in runs:
        st = Settings()
        for s in steps:
            st.apply(s)
            shape = tuple(kv for kv in s.args if kv[0] != "nb" or s.kind == "full_domain")
            out.add((s.kind, shape, engine(config, st, s), prefix_depth(config, st, s)))
    return out


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_every_shape_and_engine_of_the_pool_is_run(config):
    got = _reached(config)
    for kind, shapes in pool(config).items():
        for args in shapes:
            assert any(g[0] == kind and g[1] == tuple(sorted(args.items())) for g in got), (config, kind, args)
    if config != "hirose16":
        return
    hit = lambda kind, engine, depth=None, **shape: any(  # noqa: E731
        g[0] == kind and g[1] == tuple(sorted(shape.items())) and g[2] == engine and depth in (None, g[3]) for g in got)
    for m in (1, 2048, 2049, 8192, 8193, 32768):  # row2 | row | oct, both edges of each, on both entry points
        assert hit("eval_device", "lat", m=m) and hit("host_eval", "lat", m=m), m
    for m in (32769, 40000):  # the pair walk, the first shape with its automatic table
        assert hit("eval_device", "pair", 18, m=m) and hit("host_eval", "pair", 18, m=m), m
    assert hit("eval_device", "stream", m=STREAM_MIN)
    assert hit("eval_device", "ttable", m=EVAL16_FORCED_M)
    for depth in (9, 21):
        assert hit("eval_device", "stream", depth, m=EVAL16_FORCED_M), depth
    for K, P in MK16:  # the pair kernel in auto mode, the stream engine (top trees from 32 points per key) in mode 4
        assert hit("eval_multikey", "pair", K=K, P=P) and hit("eval_multikey", "stream", K=K, P=P), (K, P)
    assert any(g[0] == "eval_multikey" and g[2] == "ttable" for g in got)


def test_every_pool_kind_is_in_the_buffer_table():
    for config in CONFIGS:
        assert set(pool(config)) <= set(STEP_BUFFERS)
    assert set().union(*STEP_BUFFERS.values()) == ALL_BUFFERS


def _walk(name):
    """[(step, path label, bytes)] of the ladder's steps that lay something out in its buffer."""
    config, buffer, steps = LADDERS[name]
    st, out = Settings(), []
    for s in steps:
        if s.kind in SETTINGS:
            st.apply(s)
            if s.kind == "trim":
                out.append((s, "trim", 0))
            continue
        e = extent(config, st, s, buffer)
        if e is None:
            continue
        label = stage_path(config, st, s) if buffer == "stage" else f"{s.kind}/{engine(config, st, s)}"
        out.append((s, label, e))
    return config, buffer, out


def _pairs(seq):
    return [(a, b) for a, b in zip(seq, seq[1:]) if a[1] != "trim" and b[1] != "trim"]


@pytest.mark.parametrize("name", sorted(n for n in LADDERS if LADDERS[n][1] != "d_ctr"))
def test_ladder_grows_shrinks_and_switches_paths(name):
    config, buffer, seq = _walk(name)
    pairs = _pairs(seq)
    assert any(b[2] > a[2] for a, b in pairs), (name, "no call larger than the one before")
    assert any(b[2] < a[2] for a, b in pairs), (name, "no call smaller than the one before")
    if name != "pfx_mmo16":  # under the MMO PRG d_pfx has one user, the single-key table
        assert any(b[1] != a[1] for a, b in pairs), (name, "no switch of path")
    # the largest layout is not the last: something smaller runs over its remains
    assert max(range(len(seq)), key=lambda i: seq[i][2]) < len(seq) - 1


@pytest.mark.parametrize("name", sorted(n for n in LADDERS if LADDERS[n][1] == "d_pfx"))
def test_prefix_ladders(name):
    config, _, seq = _walk(name)
    labels = [lab for _, lab, _ in seq]
    if name != "pfx_mmo16":
        assert any(lab.startswith("eval_multikey") for lab in labels), "per-key top trees / per-key tables between two tables"
    i = labels.index("trim")
    assert 0 < i < len(labels) - 1, "trim in mid-sequence, and a fresh allocation after it"
    st, depths = Settings(), []
    for s in LADDERS[name][2]:
        st.apply(s)
        if s.kind == "eval_device":
            depths.append(prefix_depth(config, st, s))
    if name.startswith("pfx_hirose16"):
        assert any(lab.startswith("full_domain") for lab in labels)
        assert {21, 9, 19, 1, 15, 18} <= set(depths), depths  # both sides of the depth-first build (D >= 19), auto 18
        assert "eval_device/pair" in labels and "eval_device/stream" in labels
    if name == "pfx_mmo16":
        assert [d for d in depths if d][:4] == [1, 15, 23, 8]
    if name == "pfx_hirose64":
        assert [d for d in depths if d][:4] == [16, 1, 21, 8]


def test_counter_ladder():
    """d_ctr has no size; its transitions are between the ways a call treats the counter."""
    config, _, seq = _walk("ctr_hirose16")
    how = {"lat": "kernel zeroes", "stream": "counts", "None": "counts", "ttable": "memset only", "pair": "memset only"}
    kinds = [how[lab.split("/")[1]] for _, lab, _ in seq]
    pairs = list(zip(kinds, kinds[1:]))
    assert ("counts", "memset only") in pairs      # a stale block count must read 0
    assert ("counts", "kernel zeroes") in pairs
    assert ("kernel zeroes", "counts") in pairs
    assert ("memset only", "counts") in pairs
    assert any(lab.startswith("range_device") for _, lab, _ in seq) and any(lab.startswith("eval_multikey/stream") for _, lab, _ in seq)
    ms = [s.get("m") for s, _, _ in seq if s.kind == "eval_device"]
    assert max(ms) == STREAM_MIN and ms.index(STREAM_MIN) < len(ms) - 1  # a large call, then smaller ones


def test_staging_ladder():
    config, _, seq = _walk("staging_hirose16")
    labels = [lab for _, lab, _ in seq]
    assert labels[:3] == ["h_tiny", "h_mid", "staged x+y"] and labels[3] == "staged y" and labels[4] == "h_tiny"
    two = seq[2][0]
    assert eval_chunk(16, 16) < two.get("m") <= 2 * eval_chunk(16, 16)  # exactly two chunks
    assert {"h_tiny", "staged seeds"} <= set(labels[5:])
    assert all("stage" in STEP_BUFFERS[s.kind] for s, _, _ in seq) and len(seq) == len(LADDERS["staging_hirose16"][2])


def test_deferred_queue_switches_every_buffer():
    kinds = [s.kind for s in DEFERRED]
    assert kinds == ["eval_device", "range_device", "eval_multikey"]
    assert "d_pfx" in STEP_BUFFERS[kinds[0]] & STEP_BUFFERS[kinds[2]] and "d_ws" in STEP_BUFFERS[kinds[1]]
    assert all("d_ctr" in STEP_BUFFERS[k] for k in kinds)
