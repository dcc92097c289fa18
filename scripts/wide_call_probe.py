"""One small wide call (lambda = 32, N = 2, 300 points): device-call latency, host enqueue and end to end."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dcf_amd
lam, nb, m = 32, 2, 300
rng = np.random.default_rng(11)
prg = dcf_amd.Aes256HirosePrg([rng.bytes(32) for _ in range(18)], lam)
d = dcf_amd.DcfImpl(nb, lam, prg)
s0, s1 = rng.bytes(lam), rng.bytes(lam)
k = d.gen(dcf_amd.CmpFn(rng.bytes(nb), rng.bytes(lam)), [s0, s1], dcf_amd.BoundState.LtBeta)
T = lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()
cwb, sd = T(dcf_amd.share_to_cwb(k, nb, lam)), T(s0)
xs = torch.from_numpy(rng.integers(0, 256, (m, nb), dtype=np.uint8)).cuda()
ys = torch.empty((m, lam), dtype=torch.uint8, device="cuda")
out = []
for rep in range(5):
    n = 2000
    for _ in range(50): d.eval_device(False, cwb, sd, xs, ys)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n): d.eval_device(False, cwb, sd, xs, ys)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out.append({"enqueue_us": (t1 - t0) / n * 1e6, "call_us": (t2 - t0) / n * 1e6})
# one call at a time: launch + wait
lat = []
for _ in range(300):
    t0 = time.perf_counter(); d.eval_device(False, cwb, sd, xs, ys); torch.cuda.synchronize(); lat.append(time.perf_counter() - t0)
print(json.dumps({"lambda": lam, "n_bytes": nb, "points": m, "reps": out,
                  "call_us_median": float(np.median([r["call_us"] for r in out])),
                  "enqueue_us_median": float(np.median([r["enqueue_us"] for r in out])),
                  "sync_call_us_median": float(np.median(lat) * 1e6)}), flush=True)
