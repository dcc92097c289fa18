"""Contiguous-range eval (dcf_eval_range_device) on one MI355X, Hirose or MMO PRG (--prg), LAMBDA = 16
or --lam (the Hirose PRG at LAMBDA >= 32 takes 18 keys; blocks are then the AES-256 blocks of bytes [0, 32)).

  (a) N = 16, count = 2^16, 2^20, 2^24, 2^28 at a random unaligned x0: outputs/s and AES blocks
      per output (dcf_prg_last_eval_blocks, counted on the device);
  (b) the same ranges through eval_device on the materialised points, in the same process;
  (c) N = 4 over the whole domain next to eval_full_domain_device, in the same run;
  (d) the executed blocks/s of (a) as a fraction of the T-table LDS bound: 256 CUs x 32 lookups/clk
      x 2.4 GHz over the lookups of a block, 224 for AES-256 (87.77e9 blocks/s, Hirose) and 160 for
      AES-128 (122.88e9, MMO);
  (e) K keys over one small range (--multikey LOG2_K,COUNT, default 2^20 keys x 256 points at N = 1)
      through eval_range_multikey_device.

--fold times the range fold instead (eval_range_fold_device for (a), eval_range_fold_multikey_device
for (e), under a random table of count rows; "fold_checksum" is the folded value) and leaves (b)
and (c) out, so a --fold run and a plain run on the same shapes stand side by side.

Every figure is the median of REPS >= 10 repetitions timed one by one with HIP events after
WARMUP untimed ones; min and max are kept beside it.  Prints one JSON document and writes it to
--out (default profiles/range_bench.json, range_bench_mmo.json with --prg mmo).

  python scripts/range_bench.py [--prg hirose|mmo] [--lam 16] [--log2-counts 16,20,24,28] [--out FILE]
                                [--reps 10] [--warmup 3] [--skip-full-domain] [--skip-pointwise]
                                [--fold] [--multikey 20,256 | --skip-multikey]

--skip-pointwise leaves (b) out (at LAMBDA = 16384 and 2^22 points its outputs are a second 64 GiB);
every range row carries a checksum of its outputs, so two libraries can be compared run to run.
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


def points(x0: int, count: int, nb: int, chunk: int = 1 << 24):
    """(x0 + i) as big-endian N-byte rows on the device; x0's low 64 bits stay below 2^62."""
    lo, hi = x0 & ((1 << 64) - 1), (x0 >> 64).to_bytes(max(nb - 8, 0), "big")
    assert lo + count < 1 << 62
    xs = torch.empty((count, nb), dtype=torch.uint8, device="cuda")
    if nb > 8:
        xs[:, :nb - 8] = torch.tensor(list(hi), dtype=torch.uint8, device="cuda")
    for o in range(0, count, chunk):
        n = min(chunk, count - o)
        v = torch.arange(o, o + n, dtype=torch.int64, device="cuda") + lo
        for k in range(min(nb, 8)):
            xs[o:o + n, nb - 1 - k] = ((v >> (8 * k)) & 255).to(torch.uint8)
    return xs


def key(d, nb, lam, rng, alpha: int):
    T = lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()  # noqa: E731
    s0, s1 = rng.bytes(lam), rng.bytes(lam)
    k = d.gen(dcf_amd.CmpFn(alpha.to_bytes(nb, "big"), rng.bytes(lam)), [s0, s1], dcf_amd.BoundState.LtBeta)
    return T(dcf_amd.share_to_cwb(k, nb, lam)), T(s0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prg", choices=("hirose", "mmo"), default="hirose")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-full-domain", action="store_true")
    ap.add_argument("--skip-pointwise", action="store_true")
    ap.add_argument("--lam", type=int, default=16)
    ap.add_argument("--log2-counts", default="16,20,24,28")
    ap.add_argument("--fold", action="store_true")
    ap.add_argument("--multikey", default="20,256")
    ap.add_argument("--skip-multikey", action="store_true")
    a = ap.parse_args()
    if a.fold:
        a.skip_full_domain = a.skip_pointwise = True
    assert a.reps >= 10, "median of at least 10 repetitions"
    stem = "range_fold_bench" if a.fold else "range_bench"
    a.out = a.out or os.path.join("profiles", f"{stem}.json" if a.prg == "hirose" else f"{stem}_{a.prg}.json")
    LDS_BOUND_BLOCKS_PER_S = LDS_LOOKUPS_PER_S / LDS_PER_BLOCK[a.prg]
    lam = a.lam
    rng = np.random.default_rng(0x7A)
    if a.prg == "mmo":
        prg = dcf_amd.Aes128MatyasMeyerOseasPrg([rng.bytes(16) for _ in range(4 * lam // 16)], lam)
    else:
        prg = dcf_amd.Aes256HirosePrg([rng.bytes(32) for _ in range(2 if lam == 16 else 18)], lam)
    res = {"device": torch.cuda.get_device_name(0), "prg": a.prg, "lambda": lam, "fold": a.fold,
           "library": dcf_amd.load().dcf_version().decode(),
           "lds_bound_blocks_per_s": LDS_BOUND_BLOCKS_PER_S, "ranges": []}

    nb = 16
    d = dcf_amd.DcfImpl(nb, lam, prg)
    x0 = (int.from_bytes(rng.bytes(8), "big") << 64) | (int.from_bytes(rng.bytes(7), "big") | 1)
    for e in (int(v) for v in a.log2_counts.split(",")):
        count = 1 << e
        cwb, s0 = key(d, nb, lam, rng, x0 + count // 3)
        if a.fold:
            w = torch.randint(0, 256, (count, lam), dtype=torch.uint8, device="cuda")
            ys = torch.empty((lam,), dtype=torch.uint8, device="cuda")
            t = timed(lambda: d.eval_range_fold_device(False, cwb, s0, x0, count, w, ys), a.reps, a.warmup)
        else:
            ys = torch.empty((count, lam), dtype=torch.uint8, device="cuda")
            t = timed(lambda: d.eval_range_device(False, cwb, s0, x0, count, ys), a.reps, a.warmup)
        blocks = prg.last_eval_blocks()
        row = {"n_bytes": nb, "count": count, "subtree_levels": d.range_subtree_levels(count),
               "range": t, "range_outputs_per_s": count / (t["median_ms"] * 1e-3),
               "blocks": blocks, "blocks_per_output": blocks / count,
               "blocks_per_s": blocks / (t["median_ms"] * 1e-3),
               "lds_bound_frac": blocks / (t["median_ms"] * 1e-3) / LDS_BOUND_BLOCKS_PER_S,
               "fold_checksum" if a.fold else "ys_checksum": int(ys.view(torch.int64).sum().item())}
        if a.fold:
            del w
        if not a.skip_pointwise:
            xs = points(x0, count, nb)
            yp = torch.empty((count, lam), dtype=torch.uint8, device="cuda")
            tp = timed(lambda: d.eval_device(False, cwb, s0, xs, yp), a.reps, a.warmup)
            row.update({"pointwise": tp, "pointwise_evals_per_s": count / (tp["median_ms"] * 1e-3),
                        "speedup": tp["median_ms"] / t["median_ms"], "outputs_equal": bool(torch.equal(ys, yp))})
            del xs, yp
        res["ranges"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del ys
        torch.cuda.empty_cache()

    if not a.skip_multikey:
        nb = 1
        lk, count = (int(v) for v in a.multikey.split(","))
        K = 1 << lk
        d = dcf_amd.DcfImpl(nb, lam, prg)
        g = torch.Generator(device="cuda").manual_seed(0x7A)
        r = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)  # noqa: E731
        s0 = r(K, lam)
        cwb = d.gen_batch_device(r(K, nb), r(K, lam), s0, r(K, lam), dcf_amd.BoundState.LtBeta)
        if a.fold:
            w = r(count, lam)
            ys = torch.empty((K, lam), dtype=torch.uint8, device="cuda")
            t = timed(lambda: d.eval_range_fold_multikey_device(False, cwb, s0, 0, count, w, ys), a.reps, a.warmup)
        else:
            ys = torch.empty((K, count, lam), dtype=torch.uint8, device="cuda")
            t = timed(lambda: d.eval_range_multikey_device(False, cwb, s0, 0, count, ys), a.reps, a.warmup)
        blocks = prg.last_eval_blocks()
        res["multikey"] = {"n_bytes": nb, "keys": K, "count": count,
                           "subtree_levels": d.range_multikey_subtree_levels(K, count), "range": t,
                           "range_outputs_per_s": K * count / (t["median_ms"] * 1e-3), "blocks": blocks,
                           "blocks_per_output": blocks / (K * count),
                           "fold_checksum" if a.fold else "ys_checksum": int(ys.view(torch.int64).sum().item())}
        print(json.dumps(res["multikey"]), file=sys.stderr, flush=True)
        del ys, cwb
        torch.cuda.empty_cache()

    if not a.skip_full_domain:
        nb = 4
        d = dcf_amd.DcfImpl(nb, lam, prg)
        count = 1 << 32
        cwb, s0 = key(d, nb, lam, rng, count // 3)
        ys = torch.empty((count, lam), dtype=torch.uint8, device="cuda")
        tf = timed(lambda: d.eval_full_domain_device(False, cwb, s0, ys), a.reps, a.warmup)
        sample = torch.randint(0, count, (1 << 20,), device="cuda")
        ref = ys[sample].clone()
        tr = timed(lambda: d.eval_range_device(False, cwb, s0, 0, count, ys), a.reps, a.warmup)
        blocks = prg.last_eval_blocks()
        res["full_domain_n4"] = {
            "count": count, "full_domain": tf, "range": tr,
            "full_domain_outputs_per_s": count / (tf["median_ms"] * 1e-3),
            "range_outputs_per_s": count / (tr["median_ms"] * 1e-3),
            "range_over_full_domain_ms": tr["median_ms"] / tf["median_ms"],
            "range_inside_full_domain_spread": tf["min_ms"] <= tr["median_ms"] <= tf["max_ms"],
            "range_blocks_per_output": blocks / count,
            "range_lds_bound_frac": blocks / (tr["median_ms"] * 1e-3) / LDS_BOUND_BLOCKS_PER_S,
            "sample_equal": bool(torch.equal(ys[sample], ref))}
    out = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out + "\n")
    print(out, flush=True)


if __name__ == "__main__":
    main()
