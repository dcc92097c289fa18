"""bench.py's roofline arithmetic (no GPU): block counts and peaks the JSON line reports."""
import importlib.util
import os

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_reference_block_counts(bench):
    # prg.rs:48-53 once per level (lib.rs:176): 2 AES-256 blocks at LAMBDA = 16, 4 at LAMBDA >= 32
    assert bench.blocks_per_eval(16, 16) == 256
    assert bench.blocks_per_eval(4, 16) == 64
    assert bench.blocks_per_eval(16, 16384) == 512


def test_peaks(bench):
    # T-table: 256 CUs x 32 ds_read_b32 lookups/clk x 2.4 GHz / 224 lookups per block
    assert bench.PEAK_TT_BLOCKS == pytest.approx(256 * 32 * 2.4e9 / 224)
    assert bench.engine_peak("stream") == bench.PEAK_TT_BLOCKS
    assert bench.engine_peak("mmo") == pytest.approx(256 * 2.4e9 / (160 / 32 + 11 / 16))
    assert bench.engine_peak("ttable") == bench.engine_peak("ttable-small") == bench.PEAK_TT_BLOCKS


def test_wide_roofline_bound(bench):
    m, lam = 1 << 22, 16384
    r = bench.wide_roofline(m, 16, lam, kern_s=0.05, exec_bpe=320, bpe=512, kernel="k", engine="stream-head")
    t_min = m * 320 / bench.PEAK_TT_BLOCKS + m * lam / bench.HBM_WRITE_BPS
    assert r["peak"] == pytest.approx(m / t_min / 1e6)
    assert r["frac"] == pytest.approx(t_min / 0.05)
    assert r["unit"] == "M evals/s" and r["bound"] == "lds+hbm"


def test_dump_outputs_sample(bench, tmp_path):
    # --dump-outputs: whole arrays when they fit, else a fixed, sorted, distinct row sample; float32
    import numpy as np
    import torch
    assert bench.sample_rows(100, 100) is None
    for rows, keep in ((101, 100), (1 << 28, 1 << 18), ((1 << 32) - 5, 750_000)):
        idx = bench.sample_rows(rows, keep)
        assert idx.shape == (keep,) and idx[0] >= 0 and idx[-1] < rows and (np.diff(idx) > 0).all()
        assert np.array_equal(idx, bench.sample_rows(rows, keep))
    rng = np.random.default_rng(5)
    small = rng.integers(0, 256, (33, 16), dtype=np.uint8)
    big = rng.integers(0, 256, (bench.DUMP_BUDGET // 64, 16), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), {"small": torch.from_numpy(small), "big": big})
    got = np.load(tmp_path / "small.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small)
    got = np.load(tmp_path / "big.npy")
    keep = bench.DUMP_BUDGET // 2 // 64
    assert got.dtype == np.float32 and np.array_equal(got, big[bench.sample_rows(len(big), keep)])
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64_000_000


def test_plain_run_is_the_default(bench):
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full and a.dump_outputs is None and a.steps == 3 and a.workload == "c3"
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_zero_bits_below_prefix(bench):
    # the stream engine's A blocks: 0 bits of x below a shared prefix of `skip` levels
    import numpy as np
    import torch
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, (777, 5), dtype=np.uint8)
    for skip in (0, 1, 7, 8, 9, 15, 24, 33, 39):
        want = int((np.unpackbits(x, axis=1)[:, skip:] == 0).sum())
        assert bench.zero_bits(torch.from_numpy(x), skip) == want, skip
