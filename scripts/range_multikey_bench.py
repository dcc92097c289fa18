"""Multi-key contiguous-range eval (dcf_eval_range_multikey_device) on one MI355X, Hirose or MMO PRG
(--prg), LAMBDA = 16 or --lam, keys from gen_batch_device.

Shapes:
  n1     N = 1  whole domain (256 points),            K = 2^20
  n2     N = 2  whole domain (2^16 points),           K = 2^12
  n16    N = 16 count = 2^12 at a random odd x0,      K = 2^12
  w1a    N = 1  whole domain,                         K = 2^12   (the LAMBDA >= 32 shapes: --lam 128
  w1b    N = 1  whole domain,                         K = 2^16    for w1a / w1b, --lam 32 for w2)
  w2     N = 2  count = 1000 at a random odd x0,      K = 2^12
For each: outputs/s, AES blocks per output (dcf_prg_last_eval_blocks, counted on the device) and the
executed blocks/s as a fraction of the T-table LDS bound (256 CUs x 32 lookups/clk x 2.4 GHz over the
lookups of a block: 224 for AES-256, 87.77e9 blocks/s, Hirose; 160 for AES-128, 122.88e9, MMO).  Baselines in the same
process on the same keys:
  loop       K single-key eval_range_device calls on the keys' single-key CWBs — what a caller had
             before the multi-key entry point; at most --loop-keys (2^12) keys are looped and the time is
             scaled to K;
  pointwise  eval_multikey_device on the materialised points.

Every figure is the median of REPS >= 10 repetitions timed one by one with HIP events after WARMUP
untimed ones; min and max are kept beside it.  Prints one JSON document and writes it to --out
(default profiles/range_multikey_bench.json, range_multikey_bench_mmo.json with --prg mmo).

  python scripts/range_multikey_bench.py [--prg hirose|mmo] [--lam 16] [--out FILE] [--reps 10] [--warmup 3]
                                         [--shapes n1,n2,n16] [--loop-keys 4096] [--max-keys K]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dcf_amd  # noqa: E402

LDS_LOOKUPS_PER_S = 256 * 32 * 2.4e9  # VERDICT.md Weak #2
LDS_PER_BLOCK = {"hirose": 224, "mmo": 160}  # T-table lookups of an AES-256 / AES-128 block

SHAPES = {  # name: (N, count or None for the whole domain, K)
    "n1": (1, None, 1 << 20),
    "n2": (2, None, 1 << 12),
    "n16": (16, 1 << 12, 1 << 12),
    "w1a": (1, None, 1 << 12),
    "w1b": (1, None, 1 << 16),
    "w2": (2, 1000, 1 << 12),
}


def timed(f, reps, warmup):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def single_cwbs(cwb, nb, lam, K, keys):
    """The first `keys` keys of a K-key CWB as rows of single-key CWBs, (keys, cwb_bytes(nb, lam, 1))."""
    n = 8 * nb
    s = cwb[:n * K * lam].view(n, K, lam)[:, :keys].permute(1, 0, 2).reshape(keys, -1)
    v = cwb[n * K * lam:2 * n * K * lam].view(n, K, lam)[:, :keys].permute(1, 0, 2).reshape(keys, -1)
    t = cwb[2 * n * K * lam:2 * n * K * lam + n * K].view(n, K)[:, :keys].t()
    off = dcf_amd.cwb_np1_offset(nb, lam, K)
    np1 = cwb[off:off + K * lam].view(K, lam)[:keys]
    out = torch.zeros((keys, dcf_amd.cwb_bytes(nb, lam, 1)), dtype=torch.uint8, device=cwb.device)
    raw = torch.cat([s, v, t], dim=1)
    out[:, :raw.shape[1]] = raw
    out[:, dcf_amd.cwb_np1_offset(nb, lam, 1):] = np1
    return out


def points(x0: int, count: int, nb: int):
    """(x0 + i) as big-endian N-byte rows on the device (count <= 2^16: built on the host)."""
    b = b"".join((x0 + i).to_bytes(nb, "big") for i in range(count))
    return torch.from_numpy(np.frombuffer(b, np.uint8).reshape(count, nb).copy()).cuda()


def spread_apart(fast, slow):
    """True when every repetition of `fast` beat every repetition of `slow`."""
    return fast["max_ms"] < slow["min_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prg", choices=("hirose", "mmo"), default="hirose")
    ap.add_argument("--lam", type=int, default=16, help="LAMBDA (a multiple of 16)")
    ap.add_argument("--out")
    ap.add_argument("--loop-keys", type=int, default=1 << 12)
    ap.add_argument("--max-keys", type=int, help="cap every shape's K (a library whose path runs key by key)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="n1,n2,n16")
    a = ap.parse_args()
    assert a.reps >= 10, "median of at least 10 repetitions"
    a.out = a.out or os.path.join("profiles", "range_multikey_bench.json" if a.prg == "hirose"
                                  else f"range_multikey_bench_{a.prg}.json")
    LDS_BOUND_BLOCKS_PER_S, LOOP_KEYS_MAX = LDS_LOOKUPS_PER_S / LDS_PER_BLOCK[a.prg], a.loop_keys
    lam = a.lam
    rng = np.random.default_rng(0x7B)
    if a.prg == "mmo":
        prg = dcf_amd.Aes128MatyasMeyerOseasPrg([rng.bytes(16) for _ in range(4 * lam // 16)], lam)
    else:
        prg = dcf_amd.Aes256HirosePrg([rng.bytes(32) for _ in range(2 if lam == 16 else 18)], lam)
    wide = a.prg == "hirose" and lam >= 32  # the LAMBDA >= 32 tree path has its own height and group size
    res = {"device": torch.cuda.get_device_name(0), "prg": a.prg, "lambda": lam, "library": dcf_amd.load().dcf_version().decode(),
           "lds_bound_blocks_per_s": LDS_BOUND_BLOCKS_PER_S, "loop_keys_max": LOOP_KEYS_MAX, "shapes": []}
    g = torch.Generator(device="cuda").manual_seed(0x7B)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)  # noqa: E731

    for name in a.shapes.split(","):
        nb, count, K = SHAPES[name]
        K = min(K, a.max_keys or K)
        d = dcf_amd.DcfImpl(nb, lam, prg)
        if count is None:
            x0, count = 0, 1 << (8 * nb)
        elif nb == 16:
            x0 = (int.from_bytes(rng.bytes(8), "big") << 64) | (int.from_bytes(rng.bytes(7), "big") | 1)
        else:
            x0 = int(rng.integers(0, ((1 << (8 * nb)) - count) // 2)) * 2 + 1
        alpha, s0 = rnd(K, nb), rnd(K, lam)
        if nb == 16:  # alphas inside the range
            alpha = points(x0, count, nb)[torch.randint(0, count, (K,), device="cuda", generator=g)].contiguous()
        cwb = d.gen_batch_device(alpha, rnd(K, lam), s0, rnd(K, lam), dcf_amd.BoundState.LtBeta)
        total = K * count
        ys = torch.empty((K, count, lam), dtype=torch.uint8, device="cuda")
        t = timed(lambda: d.eval_range_multikey_device(False, cwb, s0, x0, count, ys), a.reps, a.warmup)
        blocks = prg.last_eval_blocks()

        lk = min(K, LOOP_KEYS_MAX)
        c1 = single_cwbs(cwb, nb, lam, K, lk)
        yl = torch.empty((lk, count, lam), dtype=torch.uint8, device="cuda")

        def loop():
            for k in range(lk):
                d.eval_range_device(False, c1[k], s0[k], x0, count, yl[k])

        tl = timed(loop, a.reps, a.warmup)
        loop_equal = bool(torch.equal(yl, ys[:lk]))
        del yl
        scale = K / lk
        loop_scaled = {k: (v * scale if k.endswith("_ms") else v) for k, v in tl.items()}

        xs = points(x0, count, nb).repeat(K, 1)
        yp = torch.empty((total, lam), dtype=torch.uint8, device="cuda")
        tp = timed(lambda: d.eval_multikey_device(False, cwb, s0, xs, count, yp), a.reps, a.warmup)
        pointwise_equal = bool(torch.equal(yp, ys.view(total, lam)))
        del xs, yp

        sec = t["median_ms"] * 1e-3
        row = {"shape": name, "n_bytes": nb, "num_keys": K, "count": count, "x0": hex(x0),
               "subtree_levels": (d.range_wide_multikey_subtree_levels if wide and nb <= 16
                                  else d.range_multikey_subtree_levels)(K, count),
               "keys_per_launch": (d.range_wide_keys_per_launch if wide and nb <= 16 else d.range_keys_per_launch)(K, count),
               "multikey": t, "outputs_per_s": total / sec,
               "blocks": blocks, "blocks_per_output": blocks / total, "blocks_per_s": blocks / sec,
               "lds_bound_frac": blocks / sec / LDS_BOUND_BLOCKS_PER_S,
               "loop_keys": lk, "loop_measured": tl, "loop_scaled_to_K": loop_scaled,
               "loop_single_subtree_levels": d.range_subtree_levels(count),
               "loop_outputs_per_s": total / (loop_scaled["median_ms"] * 1e-3),
               "speedup_vs_loop": loop_scaled["median_ms"] / t["median_ms"],
               "faster_than_loop_beyond_spread": spread_apart(t, loop_scaled), "loop_outputs_equal": loop_equal,
               "pointwise": tp, "pointwise_evals_per_s": total / (tp["median_ms"] * 1e-3),
               "speedup_vs_pointwise": tp["median_ms"] / t["median_ms"],
               "faster_than_pointwise_beyond_spread": spread_apart(t, tp), "pointwise_outputs_equal": pointwise_equal}
        res["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del ys, cwb, c1
        torch.cuda.empty_cache()

    out = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out + "\n")
    print(out, flush=True)


if __name__ == "__main__":
    main()
