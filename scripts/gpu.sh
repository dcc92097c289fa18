# One parameterised script for every GPU-box step (replaces the round 1-5 one-shot lease scripts).
# Run on the box through gpurun, e.g.
#   gpurun --timeout 1200 -- 'bash scripts/gpu.sh r06a suite && bash scripts/gpu.sh r06a bench c3 c4'
#   bash scripts/gpu.sh TAG SUB-COMMAND [args]    (TAG names the output directory gpurun_out/<TAG>)
# Sub-commands:
#   suite   [pytest args]           GPU suite (-m gpu, or the given tests) + smoke()
#   bench   W... [-- bench args]    bench lines of workloads W (c1 c2 c3 c4 c5 fd lat mmo; "all");
#                                   --full lines; c3 with the driver's steps (--gpus 1 --steps 20 --warmup 5)
#   trace                           C3 bench line + a rocprofv3 kernel trace of the same workload in the
#                                   same lease, reduced by scripts/lease_c3.py to prof_c3.md
#   profile W [bench args]          kernel trace + FETCH_SIZE / WRITE_SIZE / SQ PMC passes (one pass
#                                   each, MI355X_MICROARCH.md) of one workload, reduced to prof_<W>.md;
#                                   TRAFFIC="<kernels> <W> <points> <N> <lambda> <prefix> <alg bytes>"
#                                   also writes pmc_traffic_<W>.json
#   ab      W REPS VARIANT... [-- bench args]  alternating same-box runs of library builds
#                                   (VARIANT "default" = dcf_amd/libdcf_hip.so, else
#                                   dcf_amd/libdcf_hip_<VARIANT>.so from scripts/build_variant.sh),
#                                   one summary line per run appended to ab.txt
#   abtest  VARIANT... [-- pytest args]  parity of each variant build on the GPU suite subset
#   pmc     W "COUNTERS" [bench args]    one extra PMC pass (mean per dispatch per kernel printed)
#   range   [range_bench args]      scripts/range_bench.py: range eval vs eval_device on the same points and
#                                   vs full-domain eval at N = 4 -> range_bench.json (copy to profiles/)
#   rangemk [range_multikey_bench args]  scripts/range_multikey_bench.py: K keys over one range vs a loop of
#                                   single-key range calls and vs multi-key point eval -> range_multikey_bench.json
set -o pipefail
export TMPDIR=/tmp
TAG=$1; CMD=$2; shift 2
O=gpurun_out/$TAG
mkdir -p $O

libof() { if [ "$1" = default ]; then echo $PWD/dcf_amd/libdcf_hip.so; else echo $PWD/dcf_amd/libdcf_hip_$1.so; fi; }

steps_of() {  # default steps / warmup per workload (a few seconds of GPU time each)
  case $1 in
    c1) echo "--workload c1 --steps 300 --warmup 100";;
    c2) echo "--workload c2 --steps 60 --warmup 20";;
    c3) echo "--gpus 1 --steps 20 --warmup 5";;
    c4) echo "--workload c4 --steps 10 --warmup 3";;
    c5) echo "--workload c5 --steps 3 --warmup 1";;
    fd) echo "--workload fd --steps 3 --warmup 1";;
    lat) echo "--workload lat";;
    mmo) echo "--prg mmo --steps 3 --warmup 1";;
    *) echo "--workload $1";;
  esac
}

summary() {  # one line per bench JSON
  python - "$1" "$2" "$3" <<'EOF'
import json, sys
f, w, tag = sys.argv[1:4]
d = json.loads(open(f).read().strip().splitlines()[-1])
r = d.get("roofline") or {}
print(w, tag, "value=%.4g" % d["value"], "ms=%.4f" % d["ms_per_step"], "frac=%s" % (round(r["frac"], 4) if "frac" in r else None),
      "eval_only=%s" % (round(r["eval_only"]["frac"], 4) if "eval_only" in r else None),
      "cpu=%s" % ((d.get("cpu_baseline") or {}).get("value")), "phases=%s" % (d.get("phases") or d.get("phases_ms")))
EOF
}

case $CMD in
suite)
  ARGS=${*:-tests -m gpu}
  timeout -k 10 900 python -u -m pytest $ARGS -x -v --timeout 300 --timeout-method thread > $O/pytest_gpu.log 2>&1 \
    || { tail -60 $O/pytest_gpu.log; exit 1; }
  tail -1 $O/pytest_gpu.log
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1 \
    || { tail -20 $O/smoke.log; exit 1; }
  tail -1 $O/smoke.log
  ;;
bench)
  WS=(); while [ $# -gt 0 ] && [ "$1" != -- ]; do WS+=("$1"); shift; done; [ "$1" = -- ] && shift
  [ "${WS[0]}" = all ] && WS=(c3 c1 c2 c4 c5 fd lat mmo)
  for w in "${WS[@]}"; do
    timeout -k 10 600 python bench.py $(steps_of $w) --full "$@" > $O/bench_$w.json 2> $O/bench_$w.err \
      || { tail -20 $O/bench_$w.err; exit 1; }
    summary $O/bench_$w.json $w "" | tee -a $O/bench.txt
  done
  ;;
trace)
  timeout -k 10 600 python bench.py $(steps_of c3) > $O/bench_c3.json 2> $O/bench_c3.err || { tail -20 $O/bench_c3.err; exit 1; }
  summary $O/bench_c3.json c3 ""
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/trace -o trace -- python3 bench.py --steps 5 --warmup 2 --no-cpu \
    --no-compare > $O/bench_trace.log 2>&1 || { tail -20 $O/bench_trace.log; exit 1; }
  python scripts/lease_c3.py $O > $O/prof_c3.md && rm -rf $O/trace && head -12 $O/prof_c3.md
  ;;
profile)
  W=$1; shift
  B="bench.py $(steps_of $W | sed -e 's/--steps [0-9]*/--steps 2/' -e 's/--warmup [0-9]*/--warmup 1/') --no-cpu --no-compare $*"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/trace_$W -o trace -- python $B > $O/trace_$W.log 2>&1 \
    || { tail -5 $O/trace_$W.log; exit 1; }
  grep "^{\"metric" $O/trace_$W.log > $O/bench_prof_$W.json || true
  timeout -s KILL 240 rocprofv3 --pmc FETCH_SIZE -d $O/pmc_fetch_$W -o pmc -- python $B > $O/pmc_fetch_$W.log 2>&1 \
    || { tail -5 $O/pmc_fetch_$W.log; exit 1; }
  timeout -s KILL 240 rocprofv3 --pmc WRITE_SIZE -d $O/pmc_write_$W -o pmc -- python $B > $O/pmc_write_$W.log 2>&1 \
    || { tail -5 $O/pmc_write_$W.log; exit 1; }
  timeout -s KILL 240 rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAVE_CYCLES \
    SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU SQ_INSTS_SALU GRBM_GUI_ACTIVE -d $O/pmc_sq_$W -o pmc -- python $B \
    > $O/pmc_sq_$W.log 2>&1 || { tail -5 $O/pmc_sq_$W.log; exit 1; }
  python scripts/prof_summary.py $O --suffix _$W > $O/prof_$W.md || exit 1
  if [ -n "$TRAFFIC" ]; then
    python scripts/prof_summary.py $O --suffix _$W --traffic $O/pmc_traffic_$W.json $TRAFFIC > /dev/null || exit 1
  fi
  rm -rf $O/trace_$W $O/pmc_fetch_$W $O/pmc_write_$W $O/pmc_sq_$W
  echo "profiled $W"; head -20 $O/prof_$W.md
  ;;
pmc)  # one extra PMC pass of one workload: pmc W "COUNTERS" [bench args] (<= 8 SQ_, 4 TCC_, 2 TA_ ... per pass)
  W=$1; C=$2; shift 2
  B="bench.py $(steps_of $W | sed -e 's/--steps [0-9]*/--steps 2/' -e 's/--warmup [0-9]*/--warmup 1/') --no-cpu --no-compare $*"
  N=pmc_x_${W}_$(echo $C | md5sum | cut -c1-6)
  timeout -s KILL 240 rocprofv3 --pmc $C -d $O/$N -o pmc -- python $B > $O/$N.log 2>&1 || { tail -5 $O/$N.log; exit 1; }
  python - "$O/$N" <<'PY'
import glob, sqlite3, sys
from collections import defaultdict
sys.path.insert(0, "scripts")
from prof_summary import short
agg = defaultdict(lambda: defaultdict(list))
for db in glob.glob(sys.argv[1] + "/**/*.db", recursive=True):
    for k, c, v in sqlite3.connect(db).execute("select kernel_name, counter_name, value from counters_collection"):
        agg[short(k)][c].append(v)
for k, cs in agg.items():
    if k.startswith("k_"):
        print(k, " ".join(f"{c}={sum(v) / len(v):.4g}" for c, v in sorted(cs.items())))
PY
  rm -rf $O/$N
  ;;
ab)
  W=$1; REPS=$2; shift 2
  VS=(); while [ $# -gt 0 ] && [ "$1" != -- ]; do VS+=("$1"); shift; done; [ "$1" = -- ] && shift
  for rep in $(seq 1 $REPS); do
    for v in "${VS[@]}"; do
      DCF_HIP_LIB=$(libof $v) timeout -k 10 300 python bench.py $(steps_of $W) --no-cpu --no-compare "$@" \
        > $O/${W}_${v}_$rep.json 2> $O/${W}_${v}_$rep.err || { tail -20 $O/${W}_${v}_$rep.err; exit 1; }
      summary $O/${W}_${v}_$rep.json $W "$v/$rep" | tee -a $O/ab.txt
    done
  done
  ;;
abtest)
  VS=(); while [ $# -gt 0 ] && [ "$1" != -- ]; do VS+=("$1"); shift; done; [ "$1" = -- ] && shift
  for v in "${VS[@]}"; do
    DCF_HIP_LIB=$(libof $v) timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread \
      "$@" > $O/pytest_$v.log 2>&1 || { tail -60 $O/pytest_$v.log; exit 1; }
    echo "$v $(tail -1 $O/pytest_$v.log)"
  done
  ;;
range)  # contiguous-range eval vs the per-point route and full-domain eval: range [range_bench args]
  timeout -k 10 900 python scripts/range_bench.py --out $O/range_bench.json "$@" > $O/range_bench.log 2> $O/range_bench.err \
    || { tail -20 $O/range_bench.err; exit 1; }
  python - $O/range_bench.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
for r in d["ranges"]:
    print("range N=%d count=2^%d h=%d %.4g out/s %.3f blocks/out lds=%.3f pointwise %.4g ev/s speedup %.1fx equal=%s" % (
        r["n_bytes"], r["count"].bit_length() - 1, r["subtree_levels"], r["range_outputs_per_s"], r["blocks_per_output"],
        r["lds_bound_frac"], r["pointwise_evals_per_s"], r["speedup"], r["outputs_equal"]))
f = d.get("full_domain_n4")
if f:
    print("N=4 whole domain: range %.4g out/s, full-domain %.4g out/s (%.3f-%.3f ms), range/full %.3f, inside spread %s" % (
        f["range_outputs_per_s"], f["full_domain_outputs_per_s"], f["full_domain"]["min_ms"], f["full_domain"]["max_ms"],
        f["range_over_full_domain_ms"], f["range_inside_full_domain_spread"]))
PY
  ;;
rangemk)  # multi-key range eval vs a loop of single-key range calls and vs multi-key point eval
  timeout -k 10 900 python scripts/range_multikey_bench.py --out $O/range_multikey_bench.json "$@" \
    > $O/range_multikey_bench.log 2> $O/range_multikey_bench.err || { tail -20 $O/range_multikey_bench.err; exit 1; }
  python - $O/range_multikey_bench.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
for r in d["shapes"]:
    print("rangemk N=%d K=2^%d count=2^%d h=%d %.4g out/s (%.3f-%.3f ms) %.3f blocks/out lds=%.3f loop %.1fx (beyond spread %s) "
          "pointwise %.1fx equal=%s/%s" % (
              r["n_bytes"], r["num_keys"].bit_length() - 1, r["count"].bit_length() - 1, r["subtree_levels"],
              r["outputs_per_s"], r["multikey"]["min_ms"], r["multikey"]["max_ms"], r["blocks_per_output"],
              r["lds_bound_frac"], r["speedup_vs_loop"], r["faster_than_loop_beyond_spread"], r["speedup_vs_pointwise"],
              r["loop_outputs_equal"], r["pointwise_outputs_equal"]))
PY
  ;;
*)
  echo "unknown sub-command $CMD"; exit 2;;
esac
