"""Range fold without a GPU: the two entry points are declared, mirrored and exported, their
argument checks return before the prg is looked at, and the K-key segmented wave reduce of the
folding tail (kernels_range.h range_fold_keys), restated in numpy, reproduces the per-key XOR."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

NAMES = ("dcf_eval_range_fold_device", "dcf_eval_range_fold_multikey_device")


def test_declared_mirrored_and_exported(hip_lib):
    from dcf_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dcf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"^[A-Za-z_][\w \*]*?\b(dcf_\w+)\s*\(", src, flags=re.M))
    syms = subprocess.check_output(["nm", "-D", "--defined-only", hip_lib._name]).decode()
    exported = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert name in exported, name
        assert getattr(hip_lib, name).argtypes is not None


def test_mirrors():
    import dcf_amd
    for name in ("eval_range_fold_device", "eval_range_fold_multikey_device"):
        assert callable(getattr(dcf_amd.DcfImpl, name))
    hpp = open(os.path.join(ROOT, "include", "dcf.hpp")).read()
    ffi = open(os.path.join(ROOT, "rust", "dcf-hip", "src", "ffi.rs")).read()
    rs = open(os.path.join(ROOT, "rust", "dcf-hip", "src", "lib.rs")).read()
    for name in NAMES:
        assert name in hpp and name in ffi and name in rs, name


def test_argument_checks_without_gpu(hip_lib):
    """These return before the prg is looked at, so nothing is launched."""
    x0 = ctypes.create_string_buffer(16)
    buf = ctypes.create_string_buffer(64)
    fake = ctypes.cast(buf, ctypes.c_void_p)  # never dereferenced: the checks below come first
    one, many = hip_lib.dcf_eval_range_fold_device, hip_lib.dcf_eval_range_fold_multikey_device
    for f, k in ((one, ()), (many, (3,))):
        call = lambda prg, nb, party, cwb, s0, x, count, w, out: f(prg, nb, *k, party, cwb, s0, x, count, w, out, None)
        assert call(None, 2, 0, buf, buf, x0, 100, buf, buf) == -1   # null prg
        assert call(fake, 0, 0, buf, buf, x0, 100, buf, buf) == -4   # n_bytes == 0
        assert call(fake, 2, 2, buf, buf, x0, 100, buf, buf) == -1   # bad party
        assert call(fake, 2, -1, buf, buf, x0, 100, None, buf) == -1
        assert call(fake, 2, 0, None, buf, x0, 100, buf, buf) == -1  # null cwb / s0 / x0
        assert call(fake, 2, 0, buf, None, x0, 100, buf, buf) == -1
        assert call(fake, 2, 0, buf, buf, None, 100, buf, buf) == -1
        assert call(fake, 2, 0, buf, buf, x0, 100, buf, None) == -1  # null out with work to do
        assert call(fake, 257, 0, buf, buf, x0, 100, buf, buf) == -7  # N > 256
        assert call(fake, 2, 0, buf, buf, (ctypes.c_char * 2)(0xFF, 0xF0), 17, buf, buf) == -1  # x0 + count > 2^16
        assert call(fake, 1, 0, buf, buf, (ctypes.c_char * 1)(1), 256, None, buf) == -1
        assert call(fake, 16, 0, buf, buf, (ctypes.c_char * 16)(*([0xFF] * 16)), 2, buf, buf) == -1  # wraps 2^128
    assert many(fake, 2, 0, 0, buf, buf, x0, 100, buf, None, None) == 0  # no keys: nothing to do


# ---- the lane logic of the K-key fold, as the tail kernel has it ----

def _shfl_up(v, d):
    """__shfl_up over a 64-lane wave: lanes below d keep their own value."""
    out = v.copy()
    out[d:] = v[:-d]
    return out


def wave_fold(keys, acc):
    """range_fold_keys over one wave: keys (64,), non-decreasing; acc (64, 4) uint32.  Returns the
    updates {key: 4 words} the last lane of each run of equal keys issues."""
    lane = np.arange(64)
    acc = acc.copy()
    d = 1
    while d < 64:
        ok, o = _shfl_up(keys, d), _shfl_up(acc, d)
        take = (lane >= d) & (ok == keys)
        acc[take] ^= o[take]
        d <<= 1
    nk = np.append(keys[1:], keys[-1])  # __shfl_down(key, 1): lane 63 keeps its own
    last = (lane == 63) | (nk != keys)
    updates = {}
    for l in np.flatnonzero(last):
        assert int(keys[l]) not in updates, "one update per (wave, key)"
        updates[int(keys[l])] = acc[l]
    return updates


@pytest.mark.parametrize("per", [1, 5, 6, 64, 65])
@pytest.mark.parametrize("base", [0, 64, 192, 1000 * 64])
def test_segmented_wave_reduce(per, base):
    """64 lanes on nodes base .. base + 63, key = j // per (RangeKeys::key): the updates of a wave are
    the per-key XOR of its lanes, one per key; idle lanes (clamped to the last node, nothing folded)
    change nothing."""
    rng = np.random.default_rng(per * 7919 + base)
    for nnodes in (base + 64, base + 37, base + 1):
        j = base + np.arange(64)
        live = j < nnodes
        keys = (np.where(live, j, nnodes - 1) // per).astype(np.uint32)
        acc = rng.integers(0, 1 << 32, size=(64, 4), dtype=np.uint64).astype(np.uint32)
        acc[~live] = 0
        got = wave_fold(keys, acc)
        want = {}
        for l in range(64):
            want[int(keys[l])] = want.get(int(keys[l]), np.zeros(4, np.uint32)) ^ acc[l]
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), (per, base, nnodes, k)


def test_waves_of_a_launch_combine_to_the_per_key_fold():
    """All waves of a launch (units of 64 nodes, any order) XORed into `out`: the fold of every key,
    for keys that straddle wave boundaries (per = 5, 65) and keys inside one wave."""
    rng = np.random.default_rng(11)
    for per in (1, 5, 6, 64, 65):
        nnodes = 7 * per + 3 * 64
        nnodes -= nnodes % per
        leaves = rng.integers(0, 1 << 32, size=(nnodes, 4), dtype=np.uint64).astype(np.uint32)
        out = np.zeros((nnodes // per, 4), np.uint32)
        for base in rng.permutation(np.arange(0, nnodes, 64)):
            j = base + np.arange(64)
            live = j < nnodes
            jj = np.where(live, j, nnodes - 1)
            acc = np.where(live[:, None], leaves[jj], 0).astype(np.uint32)
            for k, v in wave_fold((jj // per).astype(np.uint32), acc).items():
                out[k] ^= v
        want = np.bitwise_xor.reduce(leaves.reshape(nnodes // per, per, 4), axis=1)
        assert np.array_equal(out, want), per
