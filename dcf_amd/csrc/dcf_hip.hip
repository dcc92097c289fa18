// dcf_hip.hip — MI355X (gfx950, CDNA4) DCF evaluator: HIP kernels + C ABI.
//
// Replaces the hot path of the `dcf` crate (xymeng16/dcf v0.2.2):
//   DcfImpl::eval  (lib.rs:163-204)   -> k_eval16 (one lane per (key, point))
//   DcfImpl::gen   (lib.rs:86-161)    -> k_gen16  (batched; a lane quad or one lane per key)
//   Aes256HirosePrg::gen (prg.rs:42-73) inlined into both (hirose16)
// The C ABI is declared in include/dcf_hip.h.  No CPU fallback: every compute
// entry point runs a kernel or returns an error.
//
// AES-256 on CDNA4 (no AES instructions): T-table rounds with the four 1 KiB
// tables replicated 32 ways in LDS so that lane l of every 32-lane half-wave
// always reads bank l (ds_read_b32 banks are (addr/4) mod 32 per half-wave,
// MI355X_MICROARCH.md §LDS) — conflict-free for any data.  Layout (128 KiB):
//   addr(T, b, lane) = (T>>1)*64K + b*256 + (T&1)*128 + (lane&31)*4
// so one v_perm_b32 builds the address from the state byte and a per-lane
// constant: byte0 = lane slot (T even: (l&31)*4, T odd: 128+(l&31)*4),
// byte1 = state byte b, byte2 = 64K half select.  One VALU op + one LDS read
// per lookup; 16 lookups per round.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <optional>
#include <thread>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "dcf_hip.h"

#define DCF_VERSION "dcf_amd 0.2.0 (gfx950)"

#include "aes_lds.h"
#include "kernels16.h"
#include "kernels_lat.h"
#include "kernels_wide.h"
#include "kernels_stream.h"
#include "kernels_mmo.h"
#include "kernels_mmo_wide.h"
#include "kernels_wide_stream.h"
#include "kernels_range.h"
#include "kernels_range_mmo.h"
#include "kernels_range_wide.h"

namespace {

// ------------------------------------------------------------------------
// Host plumbing
// ------------------------------------------------------------------------
thread_local std::string t_err;

int fail(int code, const std::string& msg) {
  t_err = msg;
  return code;
}

// On failure the runtime's per-thread last error is cleared as well, so a later call on
// this thread does not report a stale error (e.g. an OOM) from its own launch check.
#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      (void)hipGetLastError();                                                          \
      return fail(DCF_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_));        \
    }                                                                                   \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) return;
    ok = (prev == dev) || (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (ok && hipGetDevice(&cur) == hipSuccess && cur != prev && prev >= 0) (void)hipSetDevice(prev);
  }
};

uint64_t grid_for(uint64_t work_items, int cus) {
  uint64_t blocks = (work_items + kBlock - 1) / kBlock;
  const uint64_t cap = (uint64_t)cus;  // one 128 KiB-LDS workgroup per CU, persistent loop
  if (blocks > cap) blocks = cap;
  return blocks ? blocks : 1;
}

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
};

}  // namespace

constexpr size_t kCtrBytes = 16;  // d_ctr: work counter (u32), then the stream engine's block count (u64)

// Per-call mutable state of a dcf_prg (the reference's `Dcf::eval(&self, ...)` is reentrant and
// its PRG is `Sync`, lib.rs:34,52: one DcfImpl may be shared by many threads).  Every compute
// entry point leases one workspace from the prg's pool for its duration, so concurrent calls
// on one prg — from several host threads, or device calls queued on different streams — never
// share a buffer.  The pool is LIFO, so a single caller keeps reusing one workspace whose
// buffers have already grown.  Device calls return before their kernels finish: the lease
// records `done` on the caller's stream, and the next lease of this workspace on another
// stream waits for that event on the device (hipStreamWaitEvent) before touching a buffer.
struct Workspace {
  uint32_t* d_ctr = nullptr;  // work counter / device-counted AES blocks (dcf_prg_last_eval_blocks)
  uint8_t* d_ws = nullptr;    // stream-ordered scratch (LAMBDA >= 32 paths, full domain)
  size_t ws_bytes = 0;
  uint8_t* d_dig = nullptr;   // LAMBDA >= 32 stream head: compact CW digest of the current key
  uint32_t dig_levels = 0;
  uint8_t* d_kdig = nullptr;  // LAMBDA = 16 multi-key stream eval: key-major CW digest
  size_t kdig_bytes = 0;
  uint8_t* d_pfx = nullptr;   // shared-prefix table + its build buffers / per-key top trees
  size_t pfx_bytes = 0;
  uint8_t* d_mkey = nullptr;  // dcf_eval_multi_gpu_device: this device's copy of the key (CWB + s0)
  size_t mkey_bytes = 0;
  uint32_t* d_tctr = nullptr; // LAMBDA >= 32 paired-slot tail with LDS-filling tables: per-workgroup block counters
  size_t tctr_bytes = 0;
  uint8_t* d_fold = nullptr;  // range fold, the shapes without a folding tail: a pass of range outputs (and one gathered key)
  size_t fold_bytes = 0;
  // Host-pointer entry points: three non-blocking streams (copy-in, compute, copy-out), their
  // events and staging (pinned host + device), grown on demand and kept.
  hipStream_t hs[3] = {nullptr, nullptr, nullptr};
  hipEvent_t hev[6] = {};     // in[2], kernel[2], out[2] (double-buffered chunks)
  uint8_t* h_stage = nullptr; // pinned
  size_t h_stage_bytes = 0;
  uint8_t* d_stage = nullptr;
  size_t d_stage_bytes = 0;
  uint8_t* h_tiny = nullptr;  // small host calls: pinned, device-mapped, coherent (read/written by the kernel)
  size_t tiny_bytes = 0;
  uint8_t* h_mid = nullptr;   // mid-size host evals: pinned, device-mapped, coarse-grained (x in, y out)
  size_t mid_bytes = 0;
  // Ordering of the device work of successive leases (see above).
  hipEvent_t done = nullptr;
  hipStream_t done_stream = nullptr;
  // Multi-key LAMBDA = 16 eval: a second stream for the per-key top trees, built while the
  // key-major digest is written on the call's stream (fork / join events).
  hipStream_t aux = nullptr;
  hipEvent_t aux_ev[2] = {};
  bool pending = false;
  uint32_t host_streams = 0;  // hs[] the current host call queued work on (bit i = hs[i])
  // dcf_prg_set_phase_timing: events around the last eval's preparation and walk kernels.
  hipEvent_t tev[3] = {};
  bool timed = false;
  uint32_t last_prefix = 0;
  // Cross-call shared-prefix table (dcf_eval_device, one key, LAMBDA = 16 Hirose; reuse_prefix):
  // the device state (valid depth + the key material the table in d_pfx was built from,
  // kernels16.h) and the host's hints.  The verdict "same key" lives on the device only; the host
  // knows what it asked for, not what the device found.
  uint32_t* d_pst = nullptr;
  bool last_prefix_dev = false;  // last_prefix is the host's guess: d_pst[0] holds the depth walked
  struct PrefixHints {
    bool valid = false;          // d_pfx holds this path's table (any other user of d_pfx clears it)
    const void* cwb = nullptr;
    const void* s0 = nullptr;
    int party = 0;
    size_t n_bytes = 0;
    uint32_t req = 0;            // first-call depth asked for (prefix_depth of the call)
    uint32_t base = 0;           // first-call depth built (a rebuild goes back to it)
    uint32_t depth = 0;          // depth the table should have now
    uint64_t calls = 0;          // calls walked at `depth`
    bool grow = true;            // false once an allocation for a deeper table failed
    uint64_t epoch = 0;          // the prg's settings epoch the hints belong to
  } ph;
};

struct dcf_prg {
  int kind = 0;               // 0: Aes256HirosePrg (prg.rs), 1: Aes128MatyasMeyerOseasPrg (kernels_mmo.h)
  int device = 0;
  int cus = 256;
  size_t lambda = 0;
  size_t cipher_n = 0;
  std::vector<RoundKeys> rk;  // Aes256::new per key (prg.rs:28-31)
  uint4* d_rk128 = nullptr;   // MMO: AES-128 schedules (4 * LAMBDA/16 x 11 round keys)
  size_t rk128_count = 0;     // ... how many
  uint4* d_rk2 = nullptr;     // LAMBDA >= 32 stream head: AES-256 schedules of ciphers 0 and 17
  uint4* d_rk0 = nullptr;     // LAMBDA = 16 stream eval: AES-256 schedule of cipher 0 (15 x 16 B)
  uint32_t* d_tab = nullptr;  // T0..T3 (4 KiB) on the device
  std::vector<uint8_t> key_blob;  // the PRG keys as given (multi-GPU calls check every prg holds the same)
  // Settings (read once per call; atomics so a setter racing a call is not a data race).
  std::atomic<int> eval_mode{DCF_EVAL_AUTO};
  std::atomic<int> prefix_levels{-1};     // shared-prefix table depth: -1 auto, 0 off
  std::atomic<size_t> prefix_cap{0};      // dcf_prg_set_prefix_max_bytes (0 = none)
  std::atomic<int> timing{0};             // dcf_prg_set_phase_timing
  std::atomic<uint64_t> epoch{1};         // bumped by the setters that reset the cross-call table state
  size_t total_mem = 0;                   // the device's memory (cap on the cross-call table: 1/8 of it)
  // Workspace pool (see Workspace).
  std::mutex pool_mu;
  std::vector<Workspace*> all_ws, free_ws;
  std::atomic<Workspace*> last_ws{nullptr};  // the workspace of the last eval call to return
};

namespace {

// The prg's settings as one call sees them: read once, when the call leases its workspace (the
// setters may race a call; no decision inside a call reads a setting twice).
struct Cfg {
  int mode, prefix_levels;
  size_t prefix_cap;
  bool timing;
  uint64_t epoch;
};
Cfg snapshot(const dcf_prg* p) {
  // (the epoch first: a setter bumps it after storing, so a call never pairs a new epoch with an old setting)
  const uint64_t epoch = p->epoch.load();
  return Cfg{p->eval_mode.load(), p->prefix_levels.load(), p->prefix_cap.load(), p->timing.load() != 0, epoch};
}

// A workspace leased for one call.  `st` is the stream the call's device work is queued on
// (for host entry points: the workspace's own compute stream, set by host_lease()).
struct Lease {
  dcf_prg* p;
  const Cfg c;  // the call's settings
  Workspace* w = nullptr;
  hipStream_t st = nullptr;
  bool ordered = false;
  bool drained = false;  // a host call synchronized its streams: nothing left to order after
  bool reuse = false;    // dcf_eval_device: the shared-prefix table may outlive the call (reuse_prefix)
  Lease(dcf_prg* prg) : p(prg), c(snapshot(prg)) {
    {
      std::lock_guard<std::mutex> g(p->pool_mu);
      if (!p->free_ws.empty()) {
        w = p->free_ws.back();
        p->free_ws.pop_back();
      }
    }
    if (!w) {
      w = new Workspace();
      std::lock_guard<std::mutex> g(p->pool_mu);
      p->all_ws.push_back(w);
    }
  }
  // Queue the call's device work on `stream`, after this workspace's previous device work.
  int order(hipStream_t stream) {
    st = stream;
    ordered = true;
    if (w->pending && w->done_stream != st) {
      const hipError_t e = hipStreamWaitEvent(st, w->done, 0);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(DCF_ERR_HIP, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e));
      }
    }
    return DCF_OK;
  }
  ~Lease() {
    if (drained) {
      w->pending = false;
    } else if (ordered) {
      if (!w->done) (void)hipEventCreateWithFlags(&w->done, hipEventDisableTiming);
      if (w->done && hipEventRecord(w->done, st) == hipSuccess) {
        w->done_stream = st;
        w->pending = true;
      } else {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(st);  // cannot order the next user: drain instead
        w->pending = false;
      }
    }
    std::lock_guard<std::mutex> g(p->pool_mu);
    p->free_ws.push_back(w);
  }
  Lease(const Lease&) = delete;
  Lease& operator=(const Lease&) = delete;
};

constexpr int kPrefixNoMem = -100;            // build_prefix: table allocation failed (internal)
constexpr uint64_t kWideChunk = 1ull << 22;   // points per head/tail pass (t-vector scratch 256 MiB at N <= 31)
// Points per LAMBDA >= 32 head/tail pass for t-vectors of tw words: kWideChunk up to N = 31 (16
// words), fewer for longer t-sequences so the scratch stays ~256 MiB.
uint64_t wide_chunk_points(uint32_t tw) {
  return std::max<uint64_t>(16384, kWideChunk * 16 / std::max<uint32_t>(tw, 16u));
}
constexpr uint64_t kGenChunk = 4096;          // keys per wide-gen launch (scratch 3*LAMBDA per key)
constexpr uint32_t kTailPts = 4096;          // points per tail workgroup (one table build each)

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Grow a workspace buffer to `need` bytes (contents not kept).  The old buffer may still be
// read by this workspace's earlier work on `st`, so that drains first.
int grow(uint8_t** buf, size_t* have, size_t need, hipStream_t st) {
  if (*have >= need) return DCF_OK;
  if (*buf) {
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipFree(*buf));
    *buf = nullptr;
    *have = 0;
  }
  HIP_TRY(hipMalloc(buf, need));
  *have = need;
  return DCF_OK;
}

int ensure_ws(Workspace* w, size_t bytes, hipStream_t st) { return grow(&w->d_ws, &w->ws_bytes, bytes, st); }

int ensure_ctr(Workspace* w) {
  if (!w->d_ctr) HIP_TRY(hipMalloc(&w->d_ctr, kCtrBytes));
  return DCF_OK;
}

// Where the parts of a K-key CWB lie (include/dcf_hip.h), the one fact every engine shares:
//   cw_s[8N][K][LAMBDA] | cw_v[8N][K][LAMBDA] | cw_t[8N][K] | pad to 16 B | cw_np1[K][LAMBDA]
// B: const uint8_t for a block that is read (KeyBlock), uint8_t for gen's cwb_out (KeyBlockOut).
template <class B>
struct KeyBlockT {
  using U4 = std::conditional_t<std::is_const<B>::value, const uint4, uint4>;
  B *cws, *cwv, *cwt, *np1;
  uint32_t nlev, lam;
  uint64_t K;
  KeyBlockT(B* cwb, size_t n_bytes, size_t lambda, size_t num_keys)
      : cws(cwb), cwv(cwb + 8 * n_bytes * num_keys * lambda), cwt(cwb + 2 * 8 * n_bytes * num_keys * lambda),
        np1(cwb + dcf_cwb_np1_offset(n_bytes, lambda, num_keys)), nlev((uint32_t)(8 * n_bytes)),
        lam((uint32_t)lambda), K(num_keys) {}
  // LAMBDA = 16: a row is one uint4
  U4* s4() const { return reinterpret_cast<U4*>(cws); }
  U4* v4() const { return reinterpret_cast<U4*>(cwv); }
  U4* np14() const { return reinterpret_cast<U4*>(np1); }
  // The block from key k0 on, for the kernels that find key k's row of a level at [level * K + k].
  KeyBlockT from(uint64_t k0) const {
    KeyBlockT b = *this;
    b.cws += k0 * lam;
    b.cwv += k0 * lam;
    b.cwt += k0;
    b.np1 += k0 * lam;
    return b;
  }
};
using KeyBlock = KeyBlockT<const uint8_t>;
using KeyBlockOut = KeyBlockT<uint8_t>;

// Phase timing (dcf_prg_set_phase_timing): event i of the lease's workspace on its stream.
void phase_mark(dcf_prg*, Lease& L, int i) {
  if (!L.c.timing) return;
  Workspace* w = L.w;
  if (!w->tev[i] && hipEventCreate(&w->tev[i]) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  if (hipEventRecord(w->tev[i], L.st) != hipSuccess) (void)hipGetLastError();
  if (i == 0) w->timed = false;
  if (i == 2) w->timed = true;
}

// Workgroups of the single-launch table builds (k_prefix_build16, k_wpfx_build): 2^S
// subtrees under level S, each expanded by one workgroup.
uint32_t prefix_split(uint32_t levels) { return levels > 18u ? 8u : (levels > 10u ? levels - 10u : 0u); }

// Depth-first tail of k_prefix_build16: the last H <= kPfxDfsMax levels, once the workgroup's
// level holds at least one node per thread (2^10 = kBlock).
// Full-domain eval's fast path (Hirose, from N = 2): the last kFdTail levels in registers, depth-first
// (k_fd_dfs16; 5 levels: 128 VGPRs + scratch spills), the levels above by one k_prefix_build16 launch.
// Range eval, and with it every other full-domain shape: the same tail below its breadth-first
// levels (k_range_tail16).
constexpr uint32_t kFdTail = 4;
uint32_t prefix_dfs_levels(uint32_t levels, uint32_t S) {
  const uint32_t cap = kPfxDfsMax;
  return levels >= S + 10u + 1u ? std::min<uint32_t>(cap, levels - S - 10u) : 0u;
}

// Shared-prefix depth for a single-key stream eval of `total` points (kernels_stream.h
// PrefixTable): the top tree has 2^D nodes (33 B each, built with 2^(D+1) AES blocks)
// and saves every point D levels.  Auto: D = log2(total) - 1 (table build < 1 block per
// point; Hirose: log2(total)), at most kPrefixMax = 27 (a 4.3 GB table of 32-B rows beside 0.55 GB of build
// buffers since r06; prefix_table_bytes), none below 8, always < 8N.  If the buffers cannot be
// allocated in auto mode, eval retries 2 levels shallower down to 8, then runs without a
// table (identical bytes; see try_prefix).  Measured (r01i, C2: 2^24 points, N = 4):
// D = 12 / 16 / 20 / 24 -> 2.00 / 2.29 / 2.62 / 2.83 G evals/s (1.44 without);
// C3 (2^28, N = 16): D = 16 / 24 / 26 -> 450 / 477 / ~482 M (397 M without; r01q/r).
// auto cap.  C3 sweeps (2^28 points): r01q 24 519, 25 521, 26 524, 27 524 M evals/s; r05y (today's
// walk, 2 runs, ms per step) 25 495.5 / 495.5, 26 491.6 / 492.0, 27 489.3 / 488.8, 28 488.9 / 488.8
constexpr uint32_t kPrefixMax = 27;
constexpr uint32_t kPrefixMaxForced = 28;  // dcf_prg_set_prefix_levels (Hirose 9.7 GB, MMO 2^28 x 48 B = 12.9 GB)
// Nodes per workgroup region of k_prefix_build16's two ping-pong buffers (log2): the widest
// level a workgroup writes there.  With a depth-first tail of H levels the breadth-first part
// stops at level D - H, so that is 2^(D-H-S) nodes (at D = 27: 553 MB of buffers beside the
// 4.3 GB table, r06; it was 2^(D-1-S), 4.4 GB); without one the last level goes straight to
// the table and the widest buffered level is D - 1.
uint32_t prefix_region_log2(uint32_t d, uint32_t S) {
  const uint32_t H = prefix_dfs_levels(d, S);
  return d - std::max<uint32_t>(H, 1u) - S;
}

// Device bytes of a shared-prefix table of depth d (table + build buffers, as build_prefix /
// build_wide_prefix allocate them).  MMO, LAMBDA = 16: an upper bound — the depth rules and the
// dcf_prg_set_prefix_max_bytes cap decide on the 66 B per row of the build's first layout; the rows
// build_prefix allocates (the table and the level above it) take 48.
size_t hirose16_table_bytes(uint32_t d) {  // Hirose, LAMBDA = 16: k_prefix_build16's table + buffers
  const uint32_t S = prefix_split(d);
  return ((((size_t)32 << d) + 255) & ~(size_t)255) +
         2 * ((size_t)1 << S) * ((((size_t)33 << prefix_region_log2(d, S)) + 255) & ~(size_t)255);
}
size_t prefix_table_bytes(const dcf_prg* p, uint32_t d) {
  if (d == 0) return 0;
  if (p->lambda > 16) return (((size_t)80 << d) + 255) + 2 * ((size_t)80 << (d - 1u));
  if (p->kind == 1) return 2 * ((((size_t)33 << d) + 255) & ~(size_t)255) + 256;
  return hirose16_table_bytes(d);
}

// Auto depth under the dcf_prg_set_prefix_max_bytes cap: shallower until it fits (none below 8).
uint32_t capped_depth(const dcf_prg* p, const Cfg& c, uint32_t d) {
  if (!c.prefix_cap) return d;
  while (d >= 8u && prefix_table_bytes(p, d) > c.prefix_cap) --d;
  return d >= 8u ? d : 0u;
}

// The forced depth (at most max_forced), else the automatic depth d (none below 8, at most
// max_auto, under the cap); always < 8N.
uint32_t depth_rule(const dcf_prg* p, const Cfg& c, size_t n_bytes, uint32_t d, uint32_t max_auto, uint32_t max_forced) {
  const uint32_t top = (uint32_t)(8 * n_bytes - 1);
  if (c.prefix_levels > 0) return std::min(std::min((uint32_t)c.prefix_levels, max_forced), top);
  if (d < 8u) return 0;
  return std::min(capped_depth(p, c, std::min(std::min(d, max_auto), top)), top);
}

uint32_t prefix_depth(const dcf_prg* p, const Cfg& c, size_t n_bytes, uint64_t num_keys, uint64_t total) {
  if (p->lambda != 16 || num_keys != 1 || c.prefix_levels == 0) return 0;
  // Hirose (one-launch build, k_prefix_build16): D = log2(total), r02g sweep C2 (2^24
  // points) D = 22/23/24/25 -> 3.97/4.08/4.13/3.93 G evals/s; MMO (a launch per level): log2 - 1
  const uint32_t lg = 63u - (uint32_t)__builtin_clzll(total | 1u);
  return depth_rule(p, c, n_bytes, p->kind == 0 ? lg : (lg > 1u ? lg - 1u : 0u), kPrefixMax, kPrefixMaxForced);
}

// Tiny batches run the latency kernels of kernels_lat.h (one AES column per lane).  Thresholds:
// scripts/lat_sweep.py / row_threshold.py (DESIGN.md §4 "Latency kernels", profiles/AB_LOG.md).
#ifndef DCF_EVAL_OCT_MAX
#define DCF_EVAL_OCT_MAX 32768
#endif
constexpr uint64_t kEvalOctMax = DCF_EVAL_OCT_MAX;  // points (one key) up to which auto-mode eval runs k_eval16_oct
                                         // (r03a, us per device call: 32768 oct 187 vs pair 273; 100k 623 vs 485)
constexpr uint64_t kEvalRowMax = 8192;   // points up to which auto-mode eval runs k_eval16_row (32 lanes per point)
#ifndef DCF_EVAL_ROW2_MAX
#define DCF_EVAL_ROW2_MAX 2048
#endif
constexpr uint64_t kEvalRow2Max = DCF_EVAL_ROW2_MAX;  // ... k_eval16_row2 (64 lanes per point, two levels per
// chain on right steps) up to this many points (r06i, us per device call, row2 vs row: 1 point 75.7 vs
// 97.6, 256 81.9 vs 108.1, 2048 87.4 vs 97.7, 4096 105.1 vs 100.3)

// Shared-prefix depth for the small-batch pair path (k_eval16_pair: one key, fewer points than
// two per lane of the GPU, more than the latency kernels take).  Forced: dcf_prg_set_prefix_levels.
// Auto: 18 below 2^18 points, 19 from there (at most 8N - 1; none below 8 or up to kEvalOctMax
// points) — the build is one
// launch of k_prefix_build16 (row-AES root path, depth-first tail) whose blocks cost far less than
// the walk's latency-bound levels they save.  r06 sweep (one key, both parties, ms per step;
// `scripts/c1_prefix_sweep.sh`, profiles/r06/r06v_*): N = 16 100k points 0.895 without a table,
// 0.851 / 0.850 / 0.860 at D = 17 / 18 / 19; 250k 1.878 vs 1.704 at 18; 500k 3.736 vs 3.299 at 19;
// N = 4 100k 0.249 vs 0.200 at 18, 400k 0.966 vs 0.530 at 19; N = 8 100k 0.464 vs 0.413 at 18.
// (Round 3 measured no gain at D = 14-16 on C1, before the build's row-AES root path and
// depth-first tail.)
uint32_t small_prefix_depth(const dcf_prg* p, const Cfg& c, size_t n_bytes, uint64_t total) {
  if (p->lambda != 16 || p->kind != 0 || c.prefix_levels == 0) return 0;
  const uint32_t cap = (uint32_t)(8 * n_bytes - 1);
  if (c.prefix_levels > 0) return std::min<uint32_t>(std::min((uint32_t)c.prefix_levels, kPrefixMaxForced), cap);
  // none up to kEvalOctMax points: the latency kernels walk from the root there, and at N > 32 (the
  // pair walk) a table's fixed build latency would cost more than a few thousand points save
  if (total <= kEvalOctMax) return 0;
  const uint32_t lg = 63u - (uint32_t)__builtin_clzll(total | 1u);
  const uint32_t d = capped_depth(p, c, std::min<uint32_t>(lg < 18u ? 18u : 19u, cap));
  return d >= 8u ? d : 0u;
}

// Shared-prefix depth for the LAMBDA >= 32 stream head over m points of one key
// (kernels_wide_stream.h WidePrefix): 80 B per node, 4 AES blocks per parent.
// Auto: log2(m) - 1, at most 22 (two 336 MB node buffers at 2^22), none below 8.
constexpr uint32_t kWidePrefixMax = 22;
uint32_t wide_prefix_depth(const dcf_prg* p, const Cfg& c, size_t n_bytes, uint64_t m) {
  if (p->lambda <= 16 || p->kind != 0 || c.prefix_levels == 0 || m == 0) return 0;
  const uint32_t lg = 63u - (uint32_t)__builtin_clzll(m | 1u);
  return depth_rule(p, c, n_bytes, lg > 1u ? lg - 1u : 0u, kWidePrefixMax, 30u);
}

// The multi-key shapes eval_wide_batch takes: several keys of few points each (larger keys amortise their own
// launches: eval_wide per key), Hirose PRG, no forced prefix depth (that runs the per-key passes, a table each).
constexpr uint64_t kWideBatchPpk = 32768;
constexpr uint64_t kWideBatchKeys = 4096;  // keys per pass: tail grid rows (keys x <= 8 ranges) <= 32768
bool wide_batched(const dcf_prg* p, const Cfg& c, uint64_t num_keys, uint64_t ppk) {
  return num_keys > 1 && ppk > 0 && p->kind == 0 && ppk <= kWideBatchPpk && c.prefix_levels <= 0;
}

// ---- One plan per eval call: plan_eval() alone tests the eval path's thresholds;
// eval_launch, eval_body, host_eval and dcf_eval_prefix_levels read the plan ----
enum class Engine {
  WideBatch, WidePerKey,  // LAMBDA >= 32: eval_wide_batch / eval_wide or eval_mmo_wide key by key
  Mmo16,                  // k_eval16_mmo, whatever the engine setting
  Row2, Row, Oct,         // the latency kernels (kernels_lat.h)
  Pair, Stream, TTable,   // k_eval16_pair / k_eval16_stream / k_eval16
};
struct EvalPlan {
  Engine engine = Engine::TTable;
  // The one-call shared-prefix depth asked for (what dcf_eval_prefix_levels returns), 0 where the
  // engine builds no shared table; the multi-key stream engine's top trees (kMkPfxLevels) are none.
  uint32_t depth = 0;
  int key_mode = 0;    // how a lockstep kernel finds a point's key: 0 one key, 1 ppk % 64 == 0, 2 any
  // LAMBDA = 16, auto mode, fewer points than two per lane of the GPU: set whatever the engine (MMO and the
  // latency kernels too, not only Pair); beyond plan_eval only host_eval's mid path reads it
  bool small = false;
  const char* unsupported = nullptr;  // why eval_body fails the call (DCF_ERR_UNSUPPORTED), before any device work
  // a latency kernel: it zeroes d_ctr itself, and a host call passes through the mapped tiny buffer
  bool latency() const { return engine == Engine::Row2 || engine == Engine::Row || engine == Engine::Oct; }
};

EvalPlan plan_eval(const dcf_prg* p, const Cfg& c, size_t n_bytes, uint64_t num_keys, uint64_t ppk) {
  EvalPlan pl;
  const uint64_t total = num_keys * ppk;
  const bool few = total < (uint64_t)p->cus * kBlock * 2;
  pl.key_mode = num_keys == 1 ? 0 : ppk % 64 == 0 ? 1 : 2;
  pl.small = p->lambda == 16 && c.mode == DCF_EVAL_AUTO && few;
  if (p->lambda > 16) {  // batched keys build no table; per-key passes do (Hirose only)
    pl.engine = wide_batched(p, c, num_keys, ppk) ? Engine::WideBatch : Engine::WidePerKey;
    if (pl.engine == Engine::WidePerKey) pl.depth = wide_prefix_depth(p, c, n_bytes, ppk);
    return pl;
  }
  if (p->kind == 1) {  // one key (prefix_depth); auto depth: none for small batches (latency-bound:
    pl.engine = Engine::Mmo16;  // the table's D launches cost what it saves)
    if (c.prefix_levels > 0 || !few) pl.depth = prefix_depth(p, c, n_bytes, num_keys, total);
    return pl;
  }
  if (c.mode == DCF_EVAL_AUTO && num_keys == 1 && total <= kEvalOctMax && 8 * n_bytes <= kColMaxLevels &&
      c.prefix_levels <= 0) {
    pl.engine = total <= kEvalRow2Max ? Engine::Row2 : total <= kEvalRowMax ? Engine::Row : Engine::Oct;
    return pl;
  }
  // Auto: small batches (fewer points than two per lane of the GPU) are latency-bound: one
  // point's 8N levels run back to back, so the lockstep walk (A and B of a level in one AES
  // pass: 8N passes) beats the stream engine (~12N passes); it runs on a lane pair per point
  // (k_eval16_pair: the even lane encrypts A, the odd lane B), spread over every CU with
  // workgroups just big enough (C1).  Larger batches: the stream engine, single key or many
  // (C3 r01: 407 M evals/s vs 332 M lockstep T-table; C5 with the key-major digest).  DCF_EVAL_TTABLE
  // forces the lockstep walk (k_eval16: A and B every level), which auto takes for many keys at N > 32.
  if (pl.small) {
    pl.engine = Engine::Pair;
    if (num_keys == 1) pl.depth = small_prefix_depth(p, c, n_bytes, total);
    return pl;
  }
  const bool stream = c.mode == DCF_EVAL_STREAM || (c.mode == DCF_EVAL_AUTO && (num_keys == 1 || n_bytes <= 32));
  pl.engine = stream ? Engine::Stream : Engine::TTable;
  if (stream && num_keys > 1 && n_bytes > 32) pl.unsupported = "multi-key stream eval: N <= 32";
  else if (stream && num_keys > 1 && ppk >= (1ull << 31)) pl.unsupported = "multi-key stream eval: 2^31 points per key or more";
  else if (stream) pl.depth = prefix_depth(p, c, n_bytes, num_keys, total);  // (one key only)
  else if ((total + 63) / 64 > 0xFFFFFFFFull) pl.unsupported = "more than 2^32 64-point units";
  return pl;
}

// ---- One plan per range call: plan_range() alone tests the range paths' thresholds;
// range_run and its engines, the fold and the dcf_eval_range_* introspection exports read the plan ----
constexpr uint64_t kRangeDirectMax = 1ull << 12;    // single-key rule: counts below this walk every point (h = 0)
constexpr uint64_t kRangeMkDirectMax = 1ull << 12;  // multi-key rule: fewer outputs than this in the whole call: h = 0
constexpr uint64_t kRangeLaunch = 1ull << 28;  // outputs per launch group of the tree paths (32-bit node and leaf indices)
constexpr uint32_t kRangeCtrs = 16;            // work counters of a launch group: one per level launch and the tail's last
#ifndef DCF_RANGEMK_WIDE
#define DCF_RANGEMK_WIDE 1  // A/B knob: 0 runs K keys at lambda >= 32 one after another under the single-key rule
#endif

enum class RangeEngine {
  Tree16,  // lambda = 16, N <= 16, either PRG: range_group (kernels_range.h, kernels_range_mmo.h)
  Wide,    // Hirose, lambda >= 32, N <= 16: range_wide_group (kernels_range_wide.h)
  Points,  // everything else: the points are materialised and run through eval
};
// The two height rules of include/dcf_hip.h: dcf_eval_range_device, dcf_eval_range and the single-key fold plan
// under OneKey, the multi-key entry points under MultiKey (count = 5000, one key: h = 8 and h = 10).
enum class RangeRule { OneKey, MultiKey };

// The one workspace allocation of a Wide launch group of `keys` keys of n outputs each: [t-vectors, 64 B
// per output (lambda > 32; + 256 B as eval_wide: a tail's clamped t loads run past the last row) |
// two ping-pong buffers of the 80-byte nodes of the level above the register tail | the roots'
// t-vector prefixes, 64 B each (lambda > 32) | kRangeCtrs work counters].  The paired-slot tail's
// per-workgroup counters are a buffer of their own (Workspace::d_tctr), not part of this.
struct RangeWideWs {
  size_t tv, buf, pre, total;
};
RangeWideWs range_wide_ws(uint64_t n, uint32_t h, size_t lam, uint64_t keys, uint32_t tail) {
  RangeWideWs r;
  const uint64_t maxroots = keys * ((n >> h) + 2);
  n *= keys;
  r.tv = lam > 32 ? align256(n * kTWords * 4) + 256 : 0;
  r.buf = h ? align256((maxroots * 80) << (h - tail)) : 0;
  r.pre = h && lam > 32 ? align256(maxroots * kTWords * 4) : 0;
  r.total = r.tv + 2 * r.buf + r.pre + kRangeCtrs * sizeof(uint32_t);
  return r;
}

// Workspace of a Tree16 launch group: two ping-pong buffers of *buf_bytes each — the rows (32 B) of the
// level above the tail, for `keys` keys with n <= 2^28 outputs each (4 B per output in all) — then
// kRangeCtrs work counters.  h = 0 needs none.
size_t range_ws_bytes(uint64_t keys, uint64_t n, uint32_t h, size_t* buf_bytes) {
  *buf_bytes = h ? align256((keys * ((n >> h) + 2) * 32) << (h - kFdTail)) : 0;
  return h ? 2 * *buf_bytes + kRangeCtrs * sizeof(uint32_t) : 0;
}

struct RangePlan {
  RangeEngine engine = RangeEngine::Points;
  uint32_t h = 0;        // height of the aligned blocks (whatever the engine: Points does not read it)
  // Launch groups hold whole keys, `keys` of them at most, each key's whole count; otherwise (keys = 1)
  // the keys run one after another, `per` outputs of one key to a group.
  bool grouped = false;
  uint64_t keys = 1;
  uint64_t gkeys = 1;    // keys of a group in this call: min(keys, the keys planned for)
  uint64_t per = 0;      // kRangeLaunch, or the t-vector buffer's bound on the Wide engine
  bool per_lane = false;  // the kernels' key policy: RangeKeys / RangeDigKeys, not RangeOneKey
  uint32_t tail = 0;     // Wide: register depth of the tail
  bool fused = false;    // a fold of this shape runs in the tree path's tail (Tree16, h > 0)
  size_t lam = 0;
  uint64_t count = 0;    // points per key of the call planned
  // The workspace of a driver call over cnt <= count points of each key (a host chunk and a fold pass
  // size it for their own points, the height staying the call's).
  size_t tree_ws(uint64_t cnt, size_t* buf_bytes) const {
    return range_ws_bytes(gkeys, std::min(cnt, per), h, buf_bytes);
  }
  RangeWideWs wide_ws(uint64_t cnt) const { return range_wide_ws(std::min(cnt, per), h, lam, gkeys, tail); }
};

// `kind`, `lam`: the prg's.  The heights and groups are those of a call of num_keys keys (a pass of an
// unfused multi-key fold plans on its own keys) of `count` points each.
RangePlan plan_range(int kind, size_t lam, size_t n_bytes, uint64_t num_keys, uint64_t count, RangeRule rule) {
  RangePlan pl;
  pl.lam = lam;
  pl.count = count;
  pl.engine = kind == 0 && lam >= 32 && n_bytes <= 16 ? RangeEngine::Wide
              : lam == 16 && n_bytes <= 16            ? RangeEngine::Tree16
                                                      : RangeEngine::Points;
  const bool wide = pl.engine == RangeEngine::Wide;
  const bool multi = rule == RangeRule::MultiKey && (!wide || DCF_RANGEMK_WIDE);
  // The height (the rules are documented in include/dcf_hip.h).  One key: 0 below 2^12 points.  K keys:
  // 2^h <= count / 4 (h >= kFdTail = 4 needs count >= 64), 0 below 2^12 outputs in the whole call; on the
  // Wide engine the single-key rule from 2^12 points per key, where a key has at least 16 blocks of its own.
  const uint32_t lg = 63u - (uint32_t)__builtin_clzll(count | 1u);
  if (!multi || (wide && count >= kRangeDirectMax))
    pl.h = count < kRangeDirectMax ? 0u : std::min<uint32_t>(kRangeMaxH, std::max<uint32_t>(8u, lg - 8u));
  else  // K * count < 2^12 <=> K < ceil(2^12 / count)
    pl.h = count < (4ull << kFdTail) || num_keys < (kRangeMkDirectMax + count - 1) / count
               ? 0u
               : std::min<uint32_t>(kRangeMaxH, lg - 2u);
  pl.h = (uint32_t)std::min<uint64_t>(pl.h, 8 * (uint64_t)n_bytes);
  // Whole keys per launch group: every key has at most (count >> h) + 2 blocks of 2^h leaves.
  const uint64_t maxroots = (count >> pl.h) + 2, span = maxroots << pl.h;
  if (wide) {  // a group's bound is the t-vector buffer's, as eval_wide bounds its passes, and 2^28
    pl.per = std::min<uint64_t>(wide_chunk_points(t_words((uint32_t)(8 * n_bytes))), kRangeLaunch);
    pl.grouped = multi && count <= kWideBatchPpk && span <= pl.per;
    if (pl.grouped) {
      const uint64_t rpk = std::max<uint64_t>(1, (count + kTailPts - 1) / kTailPts);  // launch_tail's grid rows per key
      const uint64_t kdig = std::max<uint64_t>(1, (0xFFFFFFFFull / 4u) / (8 * n_bytes));  // as eval_wide_batch
      pl.keys = std::max<uint64_t>(1, std::min<uint64_t>({pl.per / span, kWideBatchKeys, 8 * kWideBatchKeys / rpk, kdig}));
    }
    pl.per_lane = pl.grouped;
    pl.tail = pl.grouped ? kRangeWideTailKeys : kRangeWideTail;
  } else {
    pl.per = kRangeLaunch;
    pl.grouped = multi && maxroots <= (kRangeLaunch >> pl.h);  // else one key alone is more than a launch
    if (pl.grouped) pl.keys = std::max<uint64_t>(1, kRangeLaunch / span);
    pl.per_lane = multi;
    pl.fused = pl.engine == RangeEngine::Tree16 && pl.h > 0;
  }
  pl.gkeys = std::min<uint64_t>(pl.keys, std::max<uint64_t>(num_keys, 1));
  return pl;
}

// Expand the top `levels` levels of one key's tree for the wide stream head (the CW
// digest w->d_dig must hold this key) into WidePrefix rows in w->d_pfx, in one launch
// (k_wpfx_build): [table 2^D x 80 B | 2 x 2^S regions of 2^(D-1-S) nodes].
int build_wide_prefix(dcf_prg* p, Workspace* w, uint32_t nlev, int party, const uint8_t* s0, uint32_t levels,
                      WidePrefix* out, hipStream_t st) {
  const uint32_t S = prefix_split(levels);
  const uint32_t R = 1u << (levels - 1u - S);
  const size_t tab_bytes = (((size_t)80 << levels) + 255) & ~(size_t)255;
  const size_t region = (size_t)80 * R;
  const size_t need = tab_bytes + 2 * ((size_t)1 << S) * region;
  w->ph.valid = false;  // d_pfx changes hands
  if (int rc = grow(&w->d_pfx, &w->pfx_bytes, need, st)) return rc;
  uint4* table = (uint4*)w->d_pfx;
  uint4* ba = (uint4*)(w->d_pfx + tab_bytes);
  uint4* bb = (uint4*)(w->d_pfx + tab_bytes + ((size_t)1 << S) * region);
  hipLaunchKernelGGL(p->lambda == 32 ? k_wpfx_build<true> : k_wpfx_build<false>, dim3(1u << S), dim3(kBlock), 0, st,
                     p->d_tab, p->d_rk2, (const uint4*)w->d_dig, w->d_dig + (size_t)nlev * 64, s0, (uint32_t)party, S,
                     levels, ba, bb, R, table);
  HIP_TRY(hipGetLastError());
  *out = WidePrefix{table, levels};
  return DCF_OK;
}

// Make w->d_pfx at least `need` bytes (contents not kept; the caller has cleared w->ph.valid).
// Unlike grow(), a failed allocation does not fail the call: *oom holds its error, d_pfx is
// empty, and the caller walks with a shallower table or none.
int reserve_pfx(Workspace* w, size_t need, hipStream_t st, hipError_t* oom) {
  *oom = hipSuccess;
  if (w->pfx_bytes >= need) return DCF_OK;
  if (w->d_pfx) {
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipFree(w->d_pfx));
    w->d_pfx = nullptr;
    w->pfx_bytes = 0;
  }
  *oom = hipMalloc(&w->d_pfx, need);
  if (*oom == hipSuccess) {
    w->pfx_bytes = need;
  } else {
    (void)hipGetLastError();
    w->d_pfx = nullptr;
  }
  return DCF_OK;
}

// Expand the top `levels` levels of the key's tree (s = s0, v = 0, t = party at the root) into
// PrefixTable rows in w->d_pfx.  Hirose: one launch (k_prefix_build16).  MMO: the range path's kernels
// on rows — the two nodes of level 1 walked from s0 (the root itself is no row: s0 is not masked),
// then one k_range_level16 launch per level.
// pst (reuse_prefix, Hirose only): the gated build, which runs only if the device state word says
// that no table is valid; reuse_prefix sets the hints again afterwards.
int build_prefix(dcf_prg* p, Workspace* w, int party, const KeyBlock& kb, const uint8_t* s0, uint32_t levels,
                 PrefixTable* out, hipStream_t st, const uint32_t* pst = nullptr) {
  const uint4 *cws = kb.s4(), *cwv = kb.v4(), *np1 = kb.np14();
  const uint8_t* cwt = kb.cwt;
  w->ph.valid = false;  // d_pfx changes hands
  // Hirose: [table 2^D x 32 B | 2 x 2^S regions of 2^(D-1-S) nodes]
  // MMO: [table | the rows of level D - 1 | kPfxCtrs work counters, one per level launch | a block count]
  const uint32_t S = prefix_split(levels);
  const uint32_t R = 1u << prefix_region_log2(levels, S);
  const size_t region = align256((size_t)R * 33);
  const size_t tab_bytes = align256((size_t)32 << levels), half_bytes = align256((size_t)16 << levels);
  constexpr size_t kPfxCtrs = 32;  // > kPrefixMaxForced
  const size_t need = p->kind == 0 ? tab_bytes + 2 * ((size_t)1 << S) * region
                                   : tab_bytes + half_bytes + (kPfxCtrs + 2) * sizeof(uint32_t);
  hipError_t oom;
  if (int rc = reserve_pfx(w, need, st, &oom)) return rc;
  if (oom != hipSuccess) return fail(kPrefixNoMem, std::string("prefix table: hipMalloc: ") + hipGetErrorString(oom));
  *out = PrefixTable{(const uint4*)w->d_pfx, levels};
  if (p->kind == 0) {  // one launch: k_prefix_build16 (gated by the state word where there is one)
    uint8_t* ba = w->d_pfx + tab_bytes;
    const uint32_t H = prefix_dfs_levels(levels, S);
    hipLaunchKernelGGL(pst ? k_prefix_build16<true> : k_prefix_build16<false>, dim3(1u << S), dim3(kBlock), 0, st,
                       p->d_tab, p->rk[0], cws, cwv, cwt, (const uint4*)s0, (uint32_t)party, S, levels, H, ba,
                       ba + ((size_t)1 << S) * region, (uint64_t)region, R, (uint4*)w->d_pfx, p->d_rk0, pst);
    HIP_TRY(hipGetLastError());
    return DCF_OK;
  }
  // Level l goes to the table's buffer when D - l is even and to the other one when it is odd, so
  // level D lands in the table.  The kernels count their AES blocks: into a word of the build's own,
  // since a table is no part of what dcf_prg_last_eval_blocks reports for the call.
  uint4* cur = (uint4*)(w->d_pfx + ((levels - 1u) % 2u ? tab_bytes : 0));
  uint4* nxt = (uint4*)(w->d_pfx + ((levels - 1u) % 2u ? 0 : tab_bytes));
  uint32_t* ctrs = (uint32_t*)(w->d_pfx + tab_bytes + half_bytes);
  unsigned long long* blocks = reinterpret_cast<unsigned long long*>(ctrs + kPfxCtrs);
  HIP_TRY(hipMemsetAsync(ctrs, 0, (kPfxCtrs + 2) * sizeof(uint32_t), st));
  hipLaunchKernelGGL((k_range_roots16_mmo<false, RangeOneKey>), dim3(1), dim3(kBlock), 0, st, p->d_tab, p->d_rk128, cws,
                     cwv, cwt, np1, (const uint4*)s0, RangeOneKey{}, (uint32_t)party, RangeX{0, 0}, 1u, (uint64_t)2,
                     cur, blocks);
  HIP_TRY(hipGetLastError());
  for (uint32_t lev = 1; lev < levels; ++lev) {  // the 2^lev parents of level lev
    const uint32_t parents = 1u << lev;
    hipLaunchKernelGGL((k_range_level16<RangeMmo, RangeOneKey>), dim3((unsigned)grid_for(parents, p->cus)),
                       dim3(kBlock), 0, st, p->d_tab, p->d_rk128, cws, cwv, cwt, RangeOneKey{}, lev, parents,
                       (const uint4*)cur, nxt, ctrs + lev, blocks);
    HIP_TRY(hipGetLastError());
    std::swap(cur, nxt);
  }
  return DCF_OK;
}

// build_prefix at depth d; in auto mode (prefix_levels < 0) an allocation failure retries
// two levels shallower, down to 8, and then evaluates without a table (same output bytes).
// d = 0: no table.  The depth built goes to w->last_prefix.
int try_prefix(dcf_prg* p, const Cfg& c, Workspace* w, int party, const KeyBlock& kb, const uint8_t* s0, uint32_t d,
               PrefixTable* out, hipStream_t st, const uint32_t* pst = nullptr) {
  *out = PrefixTable{nullptr, 0u};
  while (d) {
    const int rc = build_prefix(p, w, party, kb, s0, d, out, st, pst);
    if (rc == DCF_OK) w->last_prefix = out->levels;
    if (rc != kPrefixNoMem) return rc;
    if (c.prefix_levels >= 0) return fail(DCF_ERR_HIP, t_err);  // a forced depth must fit
    d = d >= 10u ? d - 2u : 0u;
  }
  *out = PrefixTable{nullptr, 0u};
  return DCF_OK;
}

// ---- Cross-call shared-prefix table (dcf_eval_device: one key, LAMBDA = 16, Hirose, N = 16 / 4) ----
// All of a call's table work depends on the key alone, and the real use (one key, points arriving
// batch after batch) keeps the key: the table is kept across calls, not rebuilt while the key
// material is unchanged (decided on the device, k_prefix_check), and once its build is sunk it is
// deepened one level at a time, each level sparing every later point one level of the walk.
//
// Deepening D -> D + 1 costs 2^(D+1) blocks once and spares a call of m points 1.257 m blocks (the
// walk's blocks per level): it has paid for itself after
// ceil(2^(D+1) / (1.257 m)) calls, and the host deepens at the start of a call once that many calls
// have walked at D.
constexpr uint64_t kWalkMilliBlocksPerLevel = 1257;

}  // namespace

uint64_t dcf_prefix_deepen_calls(int depth, size_t points) {
  if (depth < 0 || depth >= (int)kPfxKeyLevels || points == 0) return 0;
  const uint64_t num = (1000ull << (depth + 1)), den = kWalkMilliBlocksPerLevel * (uint64_t)points;
  return std::max<uint64_t>(1, (num + den - 1) / den);
}

int dcf_prefix_reuse_max_depth(size_t n_bytes, size_t device_bytes, size_t cap_bytes) {
  if (n_bytes == 0) return 0;
  uint32_t d = (uint32_t)std::min<size_t>(kPfxKeyLevels, 8 * n_bytes - 1);
  // the dcf_prg_set_prefix_max_bytes cap keeps its meaning: what a table of that depth takes when
  // one call builds it (table + build buffers), although a deepened table has no build buffers
  while (d && ((((size_t)32 << d) > device_bytes / 8) || (cap_bytes && hirose16_table_bytes(d) > cap_bytes))) --d;
  return (int)d;
}

namespace {

void launch_commit(Workspace* w, hipStream_t st, uint32_t expect, uint32_t depth, uint32_t other, uint64_t blocks) {
  hipLaunchKernelGGL(k_prefix_commit, dim3(1), dim3(1), 0, st, w->d_pst, w->d_ctr, expect, depth, other, blocks);
}

// The table of a dcf_eval_device call of `total` points whose one-call depth is d (prefix_depth).
// *out: the table and the depth the host expects; the walk reads the real depth from w->d_pst.
// out->levels = 0: no table could be allocated, the walk starts at the root.
int reuse_prefix(dcf_prg* p, const Cfg& c, Workspace* w, int party, const KeyBlock& kb, const uint8_t* s0, uint32_t d,
                 uint64_t total, PrefixTable* out, hipStream_t st) {
  const size_t n_bytes = kb.nlev / 8;
  const uint8_t* cwb = kb.cws;  // the block's start: what the hints remember
  const uint4 *cws = kb.s4(), *cwv = kb.v4();
  const uint8_t* cwt = kb.cwt;
  Workspace::PrefixHints& h = w->ph;
  // dcf_prg_last_eval_blocks: at automatic depth the table is the library's own choice and part of
  // what the call encrypts, so the build / deepening that really ran is counted; a forced depth
  // reports the walk alone, as every other path does
  const uint64_t counted = c.prefix_levels < 0 ? 1u : 0u;
  if (!w->d_pst) {
    HIP_TRY(hipMalloc(&w->d_pst, kPfxStateBytes));  // (written whole by the first, forced, check)
    h.valid = false;
  }
  const uint32_t nlev = std::min<uint32_t>(kPfxKeyLevels, (uint32_t)(8 * n_bytes - 1));
  const bool same = h.valid && h.cwb == cwb && h.s0 == s0 && h.party == party && h.n_bytes == n_bytes &&
                    h.req == d && h.epoch == c.epoch && w->d_pfx &&
                    w->pfx_bytes >= std::max(prefix_table_bytes(p, h.base), (size_t)32 << h.depth);
  auto check = [&](uint32_t force) {
    hipLaunchKernelGGL(k_prefix_check, dim3(1), dim3(256), 0, st, (const uint8_t*)cws, (const uint8_t*)cwv, cwt, s0,
                       (uint32_t)party, (uint32_t)n_bytes, nlev, force, w->d_pst);
  };
  if (!same) {
    // First call, or changed hints: one call's path — same depth rule, same allocation, a build
    // that runs whatever the state said.
    check(1u);
    HIP_TRY(hipGetLastError());
    if (int rc = try_prefix(p, c, w, party, kb, s0, d, out, st, w->d_pst)) return rc;
    if (!out->levels) return DCF_OK;  // (h.valid is false: build_prefix cleared it)
    launch_commit(w, st, 0u, out->levels, 0xFFFFFFFFu, counted * ((2ull << out->levels) - 2));
    HIP_TRY(hipGetLastError());
    h = Workspace::PrefixHints{};
    h.valid = true;
    h.cwb = cwb;
    h.s0 = s0;
    h.party = party;
    h.n_bytes = n_bytes;
    h.req = d;
    h.base = h.depth = out->levels;
    h.calls = 1;
    h.epoch = c.epoch;
    return DCF_OK;
  }
  check(0u);
  HIP_TRY(hipGetLastError());
  // Deepen (auto depth only: a forced depth keeps the skip of identical rebuilds alone).
  const uint32_t dmax = (uint32_t)dcf_prefix_reuse_max_depth(n_bytes, p->total_mem, c.prefix_cap);
  if (c.prefix_levels < 0 && h.grow && h.depth < dmax && h.calls >= dcf_prefix_deepen_calls((int)h.depth, total)) {
    auto deepen = [&](uint64_t lo, uint64_t hi, uint4* dst) {
      const unsigned grid = (unsigned)std::min<uint64_t>((hi - lo + kBlock - 1) / kBlock, (uint64_t)p->cus);
      hipLaunchKernelGGL(k_prefix_deepen16, dim3(grid), dim3(kBlock), 0, st, p->d_tab, p->rk[0], cws, cwv, cwt, h.depth,
                         lo, hi, (const uint4*)w->d_pfx, dst, p->d_rk0, w->d_pst);
    };
    if (((size_t)32 << std::min(h.depth + 2u, dmax)) <= w->pfx_bytes) {
      // room in the allocation for this level and the next: in place, from the high end
      // (kernels16.h).  A deepening always leaves room for one more level, so the first one — the
      // caller has just shown that the key repeats — takes the larger allocation, and the
      // allocations fall on every other deepening.
      for (uint32_t j = h.depth; j-- > 0;) deepen(1ull << j, 2ull << j, (uint4*)w->d_pfx);
      deepen(0, 1, (uint4*)w->d_pfx);
      launch_commit(w, st, h.depth, h.depth + 1u, 0xFFFFFFFFu, 2ull << h.depth);
      HIP_TRY(hipGetLastError());
      ++h.depth;
      h.calls = 0;
    } else {
      // A larger allocation, with room for the level after this one as well (an allocation of this
      // size and the wait below cost as much as a level saves a call: every other deepening pays
      // them), else for this level alone.  The old table may still be read by this workspace's
      // earlier work on other streams, which st waits for: the same discipline as every growth of
      // d_pfx, but the old buffer lives on until the new rows are written from it.
      uint8_t* fresh = nullptr;
      size_t need = 0;
      for (uint32_t ahead = std::min(h.depth + 2u, dmax); ahead > h.depth && !fresh; --ahead) {
        need = std::max((size_t)32 << ahead, prefix_table_bytes(p, h.base));
        if (hipMalloc(&fresh, need) != hipSuccess) {
          (void)hipGetLastError();  // never fatal
          fresh = nullptr;
        }
      }
      if (!fresh) {
        h.grow = false;  // the table stays at this depth
      } else {
        deepen(0, 1ull << h.depth, (uint4*)fresh);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) {
          launch_commit(w, st, h.depth, h.depth + 1u, 0u, 2ull << h.depth);
          e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
          (void)hipGetLastError();
          (void)hipStreamSynchronize(st);
          (void)hipFree(fresh);
          h.valid = false;
          return fail(DCF_ERR_HIP, std::string("prefix table deepening: ") + hipGetErrorString(e));
        }
        (void)hipFree(w->d_pfx);
        w->d_pfx = (uint8_t*)fresh;
        w->pfx_bytes = need;
        ++h.depth;
        h.calls = 0;
      }
    }
  }
  // The key changed under the same pointers (state 0 after the check, or after a deepening that
  // found another depth than the host expected): rebuild at the first-call depth; else nothing runs.
  const Workspace::PrefixHints keep = h;  // (build_prefix clears the hints)
  if (int rc = build_prefix(p, w, party, kb, s0, keep.base, out, st, w->d_pst)) return rc;
  launch_commit(w, st, 0u, keep.base, 0xFFFFFFFFu, counted * ((2ull << keep.base) - 2));
  HIP_TRY(hipGetLastError());
  h = keep;
  ++h.calls;
  *out = PrefixTable{(const uint4*)w->d_pfx, h.depth};
  return DCF_OK;
}

// One tail pass, y[32, LAMBDA) from the head's t-vectors: cnt points of cnt / ppk consecutive keys key,
// key + 1, ... of the block (ppk points each, s0: their s0s back to back; one key: ppk = cnt).
struct WideTail {
  KeyBlock kb;
  uint64_t key;
  const uint8_t* s0;
  uint32_t* tvec;
  uint64_t cnt, ppk;
  uint8_t* ys;
  int party;
  hipStream_t st;
  int cus;
  Workspace* w;
};

// The 4-bit tail; grid rows = keys x ranges per key.
template <int TW, int NCH = 0, bool ACC = false>
int launch_tail(const WideTail& t, uint32_t c0 = 0, uint32_t ncp = 0) {
  static_assert(TW == 32 || TW == 64 || TW == 128 || TW == 256, "tile width");
  const uint32_t nlev = t.kb.nlev, lam = t.kb.lam;
  const uint64_t cnt = t.cnt, ppk = t.ppk;
  if (ncp == 0) ncp = (nlev + 1 + 3) / 4;
  const size_t lds = (size_t)ncp * 16 * TW;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_eval_wide_tail<TW, NCH, ACC>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // Points per workgroup: each workgroup builds its tile's tables once, then streams its
  // kTailPts points (r02i A/B on C4: 41.1-41.3 ms vs 41.7-42.3 with ranges sized to 1, 2 or 4
  // workgroups per CU).
  const uint64_t tiles = (lam + TW - 1) / TW;
  const uint64_t rpk = (ppk + kTailPts - 1) / kTailPts;
  const dim3 grid((unsigned)tiles, (unsigned)((cnt / ppk) * rpk));
  hipLaunchKernelGGL((k_eval_wide_tail<TW, NCH, ACC>), grid, dim3(kBlock), lds, t.st, t.kb.cws, t.kb.cwv, t.kb.np1, t.s0,
                     nlev, lam, t.kb.K, t.key, (const uint32_t*)t.tvec, cnt, kTailPts, t.ys, t_words(nlev), ppk,
                     (uint32_t)rpk, c0, ncp);
  HIP_TRY(hipGetLastError());
  return DCF_OK;
}

// More chunks than one 32-byte-tile table set holds (N >= 160): passes of kTailPassChunks chunks,
// each after the first adding its rows' share to the y the previous pass wrote.
constexpr uint32_t kTailPassChunks = 320;  // 320 x 16 entries x 32 B = 160 KiB
int launch_tail_passes(const WideTail& t) {
  const uint32_t nch = (t.kb.nlev + 1 + 3) / 4;
  for (uint32_t c0 = 0; c0 < nch; c0 += kTailPassChunks) {
    const uint32_t ncp = std::min(kTailPassChunks, nch - c0);
    if (int rc = c0 == 0 ? launch_tail<32>(t, 0, ncp) : launch_tail<32, 0, true>(t, c0, ncp)) return rc;
  }
  return DCF_OK;
}

// Paired-slot tail (k_eval_wide_tail2, 128-byte tiles, 6/5-bit chunks in LDS): the t-vectors are
// repacked into chunk bytes in place, then the tail runs as launch_tail does.  (8-bit chunks in
// global memory beside the LDS tables, read through the vector L1 / L2, measured 11-24 % slower on
// C4: profiles/AB_LOG.md r04d.)
template <int R6, int R5, int ROW0>
int launch_tail2(const WideTail& t) {
  using L = Tail2Layout<R6, R5, ROW0>;
  const uint32_t nlev = t.kb.nlev, lam = t.kb.lam;
  const uint64_t cnt = t.cnt, ppk = t.ppk;
  hipStream_t st = t.st;
  Workspace* w = t.w;
  if (nlev + 1 > L::rows()) return fail(DCF_ERR_UNSUPPORTED, "tail2 layout too small");
  const uint64_t tiles = (lam + 127) / 128;
  hipLaunchKernelGGL((k_tvec_chunks<R6, R5, ROW0>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, t.tvec, nlev,
                     cnt);
  HIP_TRY(hipGetLastError());
  const size_t lds = L::lds_bytes();
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_eval_wide_tail2<R6, R5, ROW0>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // One workgroup per CU at a time, kTail2Rounds rounds of them: the batch split into
  // rounds x cus / tiles ranges, so the tiles of a range build their tables once and walk its
  // points together (the rows being written at any time stay few), at least 32768 points per
  // workgroup.  Several rounds let the dispatcher even out the CUs' speeds (one round: the last
  // workgroup ended ~1 ms after the first, profiles/r04b_c4_timeline_dynamic_tail.json).  C4 A/B
  // (r04t / r04u, 3 alternating runs per box): rounds 1 / 2 / 4 / 8 32.33-32.53 / 32.46-32.73 /
  // 32.28-32.43 / 32.16-32.27 ms; on a second box 8 / 16 / 32 / 64 (= 32768-point ranges)
  // 33.08-33.12 / 33.12-33.41 / 33.24-33.28 / 33.69-33.99 ms.
  // Several keys (ppk < cnt): each key's points are ranges of their own (its own tables).
  constexpr uint64_t kTail2Rounds = 8;
  const uint64_t ranges = std::max<uint64_t>(1, (uint64_t)t.cus * kTail2Rounds / tiles);
  const uint64_t per = std::max<uint64_t>(32768, (((cnt + ranges - 1) / ranges) + 255) & ~(uint64_t)255);
  const uint64_t rpk = (ppk + per - 1) / per;
  const dim3 grid((unsigned)tiles, (unsigned)((cnt / ppk) * rpk));
  uint32_t* gctr = nullptr;
  if (L::GCTR) {  // one block counter per workgroup (each workgroup resets its own)
    uint8_t* b = reinterpret_cast<uint8_t*>(w->d_tctr);
    if (int rc = grow(&b, &w->tctr_bytes, (size_t)grid.x * grid.y * kT2CtrStride * sizeof(uint32_t), st)) return rc;
    w->d_tctr = reinterpret_cast<uint32_t*>(b);
    gctr = w->d_tctr;
  }
  hipLaunchKernelGGL((k_eval_wide_tail2<R6, R5, ROW0>), grid, dim3(kBlock), lds, st, t.kb.cws, t.kb.cwv, t.kb.np1, t.s0,
                     nlev, lam, t.kb.K, t.key, t.tvec, cnt, (uint32_t)per, t.ys, ppk, (uint32_t)rpk, (uint32_t)t.party,
                     gctr);
  HIP_TRY(hipGetLastError());
  return DCF_OK;
}

// The tail for n = nlev levels: the paired-slot tail when one of its instances covers the
// n + 1 rows with fewer LDS reads than the 4-bit tail's ceil((n + 1) / 4), else the 4-bit one.
int run_tail(const WideTail& t) {
  const uint32_t nrows = t.kb.nlev + 1, nch = (nrows + 3) / 4;
  if (t.kb.lam % 128 == 0) {
    // Paired-slot layouts with row 0 folded into the constant (t_0 = party): the first that covers
    // rows 1 .. n, in increasing reads per 16 bytes of y (2 (R6 + R5)), used when it beats the
    // 4-bit tail's ceil((n + 1) / 4).  (r04 layouts, row 0 in the tables: N = 16 took (5, 7), 24 reads.)
#define DCF_T2(A, B) \
  if (nrows <= Tail2Layout<A, B, 1>::rows() && 2u * (A + B) < nch) return launch_tail2<A, B, 1>(t);
#ifndef DCF_T2_ROW0
#define DCF_T2_ROW0 1
#endif
    if (!DCF_T2_ROW0) {  // A/B knob: the r04 layouts (row 0 in the tables)
      if (nrows <= Tail2Layout<5, 7>::rows() && nrows > Tail2Layout<3, 3>::rows() && 24u < nch)
        return launch_tail2<5, 7, 0>(t);
    }
    DCF_T2(0, 1)   // N = 1: 8 rows, 2 reads (4-bit: 3)
    DCF_T2(2, 0)   // N = 2, 3: 16 / 24 rows, 4 reads (5 / 7)
    DCF_T2(1, 2)   // N = 4: 32 rows, 6 reads (9)
    DCF_T2(4, 0)   // N = 5, 6: 40 / 48 rows, 8 reads (11 / 13)
    DCF_T2(3, 2)   // N = 7: 56 rows, 10 reads (15)
    DCF_T2(6, 0)   // N = 8, 9: 64 / 72 rows, 12 reads (17 / 19)
    DCF_T2(5, 2)   // N = 10: 80 rows, 14 reads (21)
    DCF_T2(8, 0)   // N = 11, 12: 88 / 96 rows, 16 reads (23 / 25)
    DCF_T2(7, 2)   // N = 13: 104 rows, 18 reads (27)
    DCF_T2(10, 0)  // N = 14, 15: 112 / 120 rows, 20 reads (29 / 31), 160 KiB of tables
    DCF_T2(9, 2)   // N = 16: 128 rows, 22 reads (33), 160 KiB of tables
    DCF_T2(8, 4)   // N = 17: 136 rows, 24 reads (35), 160 KiB of tables
#undef DCF_T2
  }
  // 4-bit tail: the widest tile whose tables (nch x 16 entries x TW bytes) fit the LDS
  if (nch == 33) return launch_tail<256, 33>(t);
  if (nch <= 40) return launch_tail<256>(t);
  if (nch <= 80) return launch_tail<128>(t);
  if (nch <= 160) return launch_tail<64>(t);
  if (nch <= kTailPassChunks) return launch_tail<32>(t);
  return launch_tail_passes(t);
}

// The CW digest of the wide stream head (bytes [0,32) of each level's cw_s / cw_v, then the cw_t bytes): 65 B
// per level and key in w->d_dig.  dig_levels: the levels the buffer holds.
constexpr size_t kDigLevelBytes = 65;
int ensure_dig(Workspace* w, uint64_t levels, hipStream_t st) {
  if (w->dig_levels >= levels) return DCF_OK;
  size_t have = (size_t)w->dig_levels * kDigLevelBytes;
  const int rc = grow(&w->d_dig, &have, (size_t)levels * kDigLevelBytes, st);
  w->dig_levels = (uint32_t)(have / kDigLevelBytes);
  return rc;
}

// The digest of keys [k0, k0 + nk) of the block, key-major, the cw_t bytes behind the nk keys' rows.
int launch_digest(Workspace* w, const KeyBlock& kb, uint64_t k0, uint64_t nk, hipStream_t st) {
  hipLaunchKernelGGL(k_cw_digest, dim3((unsigned)((4 * kb.nlev * nk + 255) / 256)), dim3(256), 0, st, kb.cws, kb.cwv,
                     kb.cwt, kb.nlev, kb.lam, kb.K, k0, (uint32_t)nk, (uint4*)w->d_dig,
                     w->d_dig + (size_t)nk * kb.nlev * 64);
  HIP_TRY(hipGetLastError());
  return DCF_OK;
}

// One head/tail pass over the points of `t` (xs: theirs), whose keys' digest is in w->d_dig: the pass's work
// counter, the stream head (one point per lane, one 1024-thread workgroup per CU: the T-tables fill the LDS;
// 2.5 AES blocks per level instead of 4), then the tail when LAMBDA > 32.  mk: a point's key is
// t.key + point / t.ppk (the batched engine), else every point is key t.key's and may start below wpf.
int wide_pass(dcf_prg* p, const WideTail& t, const uint8_t* xs, bool mk, const WidePrefix& wpf) {
  Workspace* w = t.w;
  const uint32_t nlev = t.kb.nlev, lam = t.kb.lam, n_bytes = nlev / 8;
  HIP_TRY(hipMemsetAsync(w->d_ctr, 0, 8, t.st));  // (the block count beside it stays)
  const uint64_t units = (t.cnt + kWideUnit - 1) / kWideUnit;
  const uint64_t blocks = std::min<uint64_t>((units + 15) / 16, (uint64_t)p->cus);
  const uint8_t* dig_t = w->d_dig + (size_t)(t.cnt / t.ppk) * nlev * 64;
  const bool xreg = n_bytes % 4 == 0 && n_bytes <= 16;
#define DCF_WH(MH, XR) \
  { k_eval_wide_head_stream<1, MH, XR, false, kBlock>, k_eval_wide_head_stream<1, MH, XR, true, kBlock> }
  static constexpr decltype(&k_eval_wide_head_stream<1, false, false, false, kBlock>) kHead[2][2][2] = {
      {DCF_WH(false, false), DCF_WH(false, true)}, {DCF_WH(true, false), DCF_WH(true, true)}};  // [MASK_HEAD][XREG][MK]
#undef DCF_WH
  hipLaunchKernelGGL(kHead[lam == 32][xreg][mk], dim3((unsigned)blocks), dim3(kBlock), 0, t.st, p->d_tab, p->d_rk2,
                     (const uint4*)w->d_dig, dig_t, t.kb.np1, t.s0, (uint32_t)t.party, xs, n_bytes, lam, t.kb.K, t.key,
                     t.cnt, w->d_ctr, t.ys, t.tvec, wpf, t_words(nlev), (uint32_t)t.ppk);
  HIP_TRY(hipGetLastError());
  return lam > 32 ? run_tail(t) : DCF_OK;
}

// The t-vector scratch of a pass of `points` points; + 256 B: a multi-pass tail's t loads run up to 64 B past
// the last row (never used).
size_t wide_tvec_bytes(uint64_t points, uint32_t tw) { return align256(points * tw * 4) + 256; }

// Dcf::eval at LAMBDA >= 32 for key `key` of the block (see kernels_wide.h): the key's digest and, at depth
// d > 0 (the plan's wide_prefix_depth), its shared-prefix table once, then the m points in passes that share both.
// The caller (eval_launch) has zeroed the workspace's block count once for the whole call.
int eval_wide(dcf_prg* p, uint32_t d, Workspace* w, const KeyBlock& kb, uint64_t key, int party, const uint8_t* s0,
              const uint8_t* xs, uint64_t m, uint8_t* ys, hipStream_t st) {
  const uint32_t tw = t_words(kb.nlev);  // t-vector words per point
  const uint64_t chunk = std::min<uint64_t>(m, wide_chunk_points(tw));
  if (int rc = ensure_ws(w, wide_tvec_bytes(chunk, tw), st)) return rc;
  if (int rc = ensure_dig(w, kb.nlev, st)) return rc;
  if (int rc = launch_digest(w, kb, key, 1, st)) return rc;
  WidePrefix wpf{nullptr, 0u};
  if (d)
    if (int rc = build_wide_prefix(p, w, kb.nlev, party, s0, d, &wpf, st)) return rc;
  w->last_prefix = d;
  for (uint64_t off = 0; off < m; off += chunk) {
    const uint64_t cnt = std::min<uint64_t>(chunk, m - off);
    const WideTail t{kb, key, s0, (uint32_t*)w->d_ws, cnt, cnt, ys + off * kb.lam, party, st, p->cus, w};
    if (int rc = wide_pass(p, t, xs + off * (kb.nlev / 8), false, wpf)) return rc;
  }
  return DCF_OK;
}

// Dcf::eval at LAMBDA >= 32 for keys 0 .. K - 1, ppk points each (key-major xs / ys, s0s[K][LAMBDA]),
// several keys per pass: one key-major CW digest, one stream-head launch (each point's key =
// point / ppk) and one tail launch whose workgroups build the tables of their own key.  For the
// shapes of wide_batched() (ppk <= kWideBatchPpk).  No shared prefix; the MMO PRG keeps the
// per-key path.
int eval_wide_batch(dcf_prg* p, Workspace* w, const KeyBlock& kb, uint64_t ppk, int party, const uint8_t* s0s,
                    const uint8_t* xs, uint8_t* ys, hipStream_t st) {
  const uint32_t nlev = kb.nlev, lam = kb.lam, tw = t_words(nlev);
  // keys per pass; the digest's uint4 index 4 * (key * nlev + level) and dig_levels are 32-bit
  const uint64_t kdig = std::max<uint64_t>(1, (0xFFFFFFFFull / 4u) / nlev);
  const uint64_t kp =
      std::max<uint64_t>(1, std::min<uint64_t>({kb.K, wide_chunk_points(tw) / ppk, kWideBatchKeys, kdig}));
  if (int rc = ensure_ws(w, wide_tvec_bytes(kp * ppk, tw), st)) return rc;
  if (int rc = ensure_dig(w, kp * nlev, st)) return rc;
  const WidePrefix none{nullptr, 0u};
  for (uint64_t k0 = 0; k0 < kb.K; k0 += kp) {
    const uint64_t nk = std::min<uint64_t>(kp, kb.K - k0);
    if (int rc = launch_digest(w, kb, k0, nk, st)) return rc;
    const WideTail t{kb, k0, s0s + k0 * lam, (uint32_t*)w->d_ws, nk * ppk, ppk, ys + k0 * ppk * lam, party, st, p->cus, w};
    if (int rc = wide_pass(p, t, xs + k0 * ppk * (nlev / 8), true, none)) return rc;
  }
  return DCF_OK;
}

// Dcf::eval with the MMO PRG at LAMBDA >= 32 for key `key` (kernels_mmo_wide.h): per pass
// of up to kWideChunk points, the head walks block 0 (y[0:16), t-vector), then the tail
// walks blocks 1..nb-1 given the t-vectors.
int eval_mmo_wide(dcf_prg* p, Workspace* w, const KeyBlock& kb, uint64_t key, int party, const uint8_t* s0,
                  const uint8_t* xs, uint64_t m, uint8_t* ys, hipStream_t st) {
  const uint32_t lam = kb.lam, nb = lam / 16u, n_bytes = kb.nlev / 8;
  const uint32_t tw = mmo_t_words(kb.nlev);
  const uint64_t chunk = std::min<uint64_t>(m, wide_chunk_points(2 * tw));
  if (int rc = ensure_ws(w, chunk * tw * 4, st)) return rc;
  uint32_t* tvec = reinterpret_cast<uint32_t*>(w->d_ws);
  for (uint64_t off = 0; off < m; off += chunk) {
    const uint64_t cnt = std::min<uint64_t>(chunk, m - off);
    const uint64_t groups = (cnt + 63) / 64;
    const dim3 gh((unsigned)std::min<uint64_t>((groups + 15) / 16, (uint64_t)p->cus));
    hipLaunchKernelGGL(k_mmo_wide_eval<true>, gh, dim3(kBlock), 0, st, p->d_tab, p->d_rk128, kb.cws, kb.cwv, kb.cwt,
                       kb.np1, s0, (uint32_t)party, xs + off * n_bytes, n_bytes, lam, kb.K, key, cnt, tvec,
                       ys + off * lam);
    HIP_TRY(hipGetLastError());
    if (nb > 1) {
      const uint64_t items = groups * (nb - 1);
      const dim3 gt((unsigned)std::min<uint64_t>((items + 15) / 16, 4 * (uint64_t)p->cus));
      hipLaunchKernelGGL(k_mmo_wide_eval<false>, gt, dim3(kBlock), 0, st, p->d_tab, p->d_rk128, kb.cws, kb.cwv, kb.cwt,
                         kb.np1, s0, (uint32_t)party, xs + off * n_bytes, n_bytes, lam, kb.K, key, cnt, tvec,
                         ys + off * lam);
      HIP_TRY(hipGetLastError());
    }
  }
  return DCF_OK;
}

// Batched Dcf::gen with the MMO PRG at LAMBDA >= 32 (kernels_mmo_wide.h): per pass of keys,
// the head over block 0 of both parties (t-CWs, per-level t bits), then the tail.
int gen_mmo_wide(dcf_prg* p, Workspace* w, const KeyBlockOut& kb, const uint8_t* alpha, const uint8_t* beta,
                 const uint8_t* s0_0, const uint8_t* s0_1, int bound, bool tail, hipStream_t st) {
  const uint32_t lam = kb.lam, nb = lam / 16u, nlev = kb.nlev, n_bytes = nlev / 8;
  const uint64_t K = kb.K;
  uint8_t *cws = kb.cws, *cwv = kb.cwv, *cwt = kb.cwt, *np1 = kb.np1;
  if (int rc = ensure_ws(w, (size_t)K * nlev * 4, st)) return rc;
  uint32_t* tinfo = reinterpret_cast<uint32_t*>(w->d_ws);
  const uint64_t groups = (K + 63) / 64;
  const dim3 gh((unsigned)std::min<uint64_t>((groups + 15) / 16, (uint64_t)p->cus));
  hipLaunchKernelGGL(k_mmo_wide_gen<true>, gh, dim3(kBlock), 0, st, p->d_tab, p->d_rk128, alpha, beta, s0_0, s0_1,
                     (uint32_t)bound, (uint32_t)n_bytes, lam, K, cws, cwv, cwt, np1, tinfo);
  HIP_TRY(hipGetLastError());
  if (tail) {  // blocks past the first (plan_gen: the call's second launch)
    const uint64_t items = groups * (nb - 1);
    const dim3 gt((unsigned)std::min<uint64_t>((items + 15) / 16, 4 * (uint64_t)p->cus));
    hipLaunchKernelGGL(k_mmo_wide_gen<false>, gt, dim3(kBlock), 0, st, p->d_tab, p->d_rk128, alpha, beta, s0_0,
                       s0_1, (uint32_t)bound, (uint32_t)n_bytes, lam, K, cws, cwv, cwt, np1, tinfo);
    HIP_TRY(hipGetLastError());
  }
  return DCF_OK;
}

}  // namespace

extern "C" {

const char* dcf_version(void) { return DCF_VERSION; }

const char* dcf_last_error(void) { return t_err.c_str(); }

size_t dcf_cwb_np1_offset(size_t n_bytes, size_t lambda, size_t num_keys) {
  const size_t n = 8 * n_bytes;
  return ((2 * n * num_keys * lambda + n * num_keys) + 15) & ~(size_t)15;
}

size_t dcf_cwb_bytes(size_t n_bytes, size_t lambda, size_t num_keys) {
  return dcf_cwb_np1_offset(n_bytes, lambda, num_keys) + num_keys * lambda;
}

int dcf_hirose_prg_new(const uint8_t* keys, size_t cipher_n, size_t lambda, int device, dcf_prg** out) {
  if (!keys || !out) return fail(DCF_ERR_ARG, "null argument");
  *out = nullptr;
  if (lambda == 0 || lambda % 16 != 0) return fail(DCF_ERR_LAMBDA, "lambda must be a positive multiple of 16");
  const size_t need = (lambda / 16 >= 2) ? 18 : 1;
  if (cipher_n < need)
    return fail(DCF_ERR_CIPHER_N, "cipher_n too small: the Hirose PRG reads ciphers[i*16+j] (prg.rs:51)");
  std::call_once(g_aes_once, aes_init_tables);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(DCF_ERR_ARG, "bad device ordinal");
  DeviceGuard dg(device);
  if (!dg.ok) return fail(DCF_ERR_HIP, "hipSetDevice failed");
  dcf_prg* p = new dcf_prg();
  p->device = device;
  p->lambda = lambda;
  p->cipher_n = cipher_n;
  p->rk.resize(cipher_n);
  for (size_t i = 0; i < cipher_n; i++) aes256_expand_words(keys + 32 * i, &p->rk[i]);
  p->key_blob.assign(keys, keys + 32 * cipher_n);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) {
    p->cus = prop.multiProcessorCount;
    p->total_mem = prop.totalGlobalMem;
  }
  hipError_t e = hipMalloc(&p->d_tab, sizeof(g_tab));
  if (e == hipSuccess) e = hipMemcpy(p->d_tab, g_tab, sizeof(g_tab), hipMemcpyHostToDevice);
  // device copies of the schedules the kernels read per round: cipher 0 (LAMBDA = 16 stream /
  // pair / table-build kernels) and, at LAMBDA >= 32, ciphers 0 and 17 (the wide stream head)
  if (e == hipSuccess) e = hipMalloc(&p->d_rk0, sizeof(RoundKeys));
  if (e == hipSuccess) e = hipMemcpy(p->d_rk0, &p->rk[0], sizeof(RoundKeys), hipMemcpyHostToDevice);
  if (e == hipSuccess && lambda > 16) {
    e = hipMalloc(&p->d_rk2, 2 * sizeof(RoundKeys));
    if (e == hipSuccess) e = hipMemcpy(p->d_rk2, &p->rk[0], sizeof(RoundKeys), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_rk2 + 15, &p->rk[17], sizeof(RoundKeys), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    dcf_prg_free(p);
    return fail(DCF_ERR_HIP, std::string("table upload: ") + hipGetErrorString(e));
  }
  *out = p;
  return DCF_OK;
}

int dcf_mmo_prg_new(const uint8_t* keys, size_t cipher_n, size_t lambda, int device, dcf_prg** out) {
  if (!keys || !out) return fail(DCF_ERR_ARG, "null argument");
  *out = nullptr;
  if (lambda == 0 || lambda % 16 != 0) return fail(DCF_ERR_LAMBDA, "lambda must be a positive multiple of 16");
  if (cipher_n < 4 * (lambda / 16)) return fail(DCF_ERR_CIPHER_N, "MMO PRG needs 4 * lambda / 16 AES-128 keys");
  std::call_once(g_aes_once, aes_init_tables);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(DCF_ERR_ARG, "bad device ordinal");
  DeviceGuard dg(device);
  if (!dg.ok) return fail(DCF_ERR_HIP, "hipSetDevice failed");
  dcf_prg* p = new dcf_prg();
  p->kind = 1;
  p->device = device;
  p->lambda = lambda;
  p->cipher_n = cipher_n;
  p->eval_mode = DCF_EVAL_TTABLE;
  p->key_blob.assign(keys, keys + 16 * cipher_n);
  // schedule b * nb + j for output b (s_L, v_L, s_R, v_R) and 16-byte block j (kernels_mmo_wide.h)
  const size_t nsched = 4 * (lambda / 16);
  std::vector<uint32_t> w(nsched * 44);
  for (size_t i = 0; i < nsched; i++) aes128_expand_words(keys + 16 * i, w.data() + 44 * i);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    p->cus = prop.multiProcessorCount;
  hipError_t e = hipMalloc(&p->d_tab, sizeof(g_tab));
  if (e == hipSuccess) e = hipMemcpy(p->d_tab, g_tab, sizeof(g_tab), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&p->d_rk128, w.size() * 4);
  if (e == hipSuccess) e = hipMemcpy(p->d_rk128, w.data(), w.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) p->rk128_count = nsched;
  if (e != hipSuccess) {
    dcf_prg_free(p);
    return fail(DCF_ERR_HIP, std::string("table upload: ") + hipGetErrorString(e));
  }
  *out = p;
  return DCF_OK;
}

int dcf_prg_kind(const dcf_prg* p) { return p ? p->kind : -1; }

static void free_workspace(Workspace* w) {
  for (hipStream_t s : w->hs)  // host-path work still queued (an error return drains these too)
    if (s) (void)hipStreamSynchronize(s);
  if (w->aux) (void)hipStreamSynchronize(w->aux);
  if (w->pending) (void)hipEventSynchronize(w->done);  // the last device call's kernels
  for (void* b : {(void*)w->d_ctr, (void*)w->d_ws, (void*)w->d_dig, (void*)w->d_kdig, (void*)w->d_pfx,
                  (void*)w->d_mkey, (void*)w->d_stage, (void*)w->d_tctr, (void*)w->d_pst, (void*)w->d_fold})
    if (b) (void)hipFree(b);
  if (w->h_stage) (void)hipHostFree(w->h_stage);
  if (w->h_tiny) (void)hipHostFree(w->h_tiny);
  if (w->h_mid) (void)hipHostFree(w->h_mid);
  for (hipStream_t s : w->hs)
    if (s) (void)hipStreamDestroy(s);
  if (w->aux) (void)hipStreamDestroy(w->aux);
  for (hipEvent_t e : w->aux_ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : w->hev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : w->tev)
    if (e) (void)hipEventDestroy(e);
  if (w->done) (void)hipEventDestroy(w->done);
  delete w;
}

void dcf_prg_free(dcf_prg* p) {
  if (!p) return;
  {
    DeviceGuard dg(p->device);
    for (Workspace* w : p->all_ws) free_workspace(w);
    for (void* b : {(void*)p->d_tab, (void*)p->d_rk128, (void*)p->d_rk2, (void*)p->d_rk0})
      if (b) (void)hipFree(b);
  }
  delete p;
}

size_t dcf_prg_lambda(const dcf_prg* p) { return p ? p->lambda : 0; }

int dcf_prg_set_eval_mode(dcf_prg* p, int mode) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  if (mode != DCF_EVAL_AUTO && mode != DCF_EVAL_TTABLE && mode != DCF_EVAL_STREAM)
    return fail(DCF_ERR_ARG, "bad eval mode (DCF_EVAL_AUTO, DCF_EVAL_TTABLE or DCF_EVAL_STREAM)");
  p->eval_mode = mode;
  ++p->epoch;  // the cross-call table state starts afresh
  return DCF_OK;
}

int dcf_prg_set_prefix_levels(dcf_prg* p, int levels) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  if (levels < -1) return fail(DCF_ERR_ARG, "prefix levels must be -1 (auto), 0 (off) or > 0");
  p->prefix_levels = levels;
  ++p->epoch;  // the cross-call table state starts afresh
  return DCF_OK;
}

int dcf_eval_prefix_levels(const dcf_prg* p, size_t n_bytes, size_t num_keys, size_t points_per_key) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  if (n_bytes == 0) return fail(DCF_ERR_N, "n_bytes must be > 0");
  return (int)plan_eval(p, snapshot(p), n_bytes, num_keys, points_per_key).depth;
}

// The public image of Engine (include/dcf_hip.h); no default: a new Engine value fails to compile here.
static int public_engine(Engine e) {
  switch (e) {
    case Engine::WideBatch: return DCF_ENGINE_WIDE_BATCH;
    case Engine::WidePerKey: return DCF_ENGINE_WIDE_PER_KEY;
    case Engine::Mmo16: return DCF_ENGINE_MMO16;
    case Engine::Row2: return DCF_ENGINE_ROW2;
    case Engine::Row: return DCF_ENGINE_ROW;
    case Engine::Oct: return DCF_ENGINE_OCT;
    case Engine::Pair: return DCF_ENGINE_PAIR;
    case Engine::Stream: return DCF_ENGINE_STREAM;
    case Engine::TTable: return DCF_ENGINE_TTABLE;
  }
  return -1;
}

int dcf_eval_plan(const dcf_prg* p, size_t n_bytes, size_t num_keys, size_t points_per_key, int* engine,
                  int* key_mode, int* prefix_levels, int* small) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  if (n_bytes == 0) return fail(DCF_ERR_N, "n_bytes must be > 0");
  const EvalPlan pl = plan_eval(p, snapshot(p), n_bytes, num_keys, points_per_key);
  if (engine) *engine = public_engine(pl.engine);
  if (key_mode) *key_mode = pl.key_mode;
  if (prefix_levels) *prefix_levels = (int)pl.depth;
  if (small) *small = pl.small ? 1 : 0;
  return pl.unsupported ? fail(DCF_ERR_UNSUPPORTED, pl.unsupported) : DCF_OK;
}

int dcf_prg_set_prefix_max_bytes(dcf_prg* p, size_t max_bytes) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  p->prefix_cap = max_bytes;
  ++p->epoch;
  return DCF_OK;
}

size_t dcf_prg_device_bytes(const dcf_prg* p) {
  if (!p) return 0;
  size_t b = 0;
  if (p->d_tab) b += sizeof(g_tab);
  if (p->d_rk128) b += p->rk128_count * 44 * 4;
  if (p->d_rk2) b += 2 * sizeof(RoundKeys);
  if (p->d_rk0) b += sizeof(RoundKeys);
  std::lock_guard<std::mutex> g(const_cast<dcf_prg*>(p)->pool_mu);
  for (const Workspace* w : p->all_ws) {
    if (w->d_ctr) b += kCtrBytes;
    if (w->d_pst) b += kPfxStateBytes;
    b += (size_t)w->dig_levels * kDigLevelBytes + w->kdig_bytes + w->ws_bytes + w->pfx_bytes +
         w->d_stage_bytes + w->mkey_bytes + w->tctr_bytes + w->fold_bytes;
  }
  return b;
}

size_t dcf_prg_host_pinned_bytes(const dcf_prg* p) {
  if (!p) return 0;
  size_t b = 0;
  std::lock_guard<std::mutex> g(const_cast<dcf_prg*>(p)->pool_mu);
  for (const Workspace* w : p->all_ws) b += w->h_stage_bytes + w->tiny_bytes + w->mid_bytes;
  return b;
}

int dcf_prg_workspaces(const dcf_prg* p) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  std::lock_guard<std::mutex> g(const_cast<dcf_prg*>(p)->pool_mu);
  return (int)p->all_ws.size();
}

// The measurement hooks read the last eval's workspace only while no call holds it: under the
// pool lock (a lease takes that lock to pop the workspace), after the workspace's last device
// work has finished.
static bool ws_idle(const dcf_prg* p, const Workspace* w) {
  return std::find(p->free_ws.begin(), p->free_ws.end(), w) != p->free_ws.end();
}

int dcf_prg_last_eval_blocks(dcf_prg* p, uint64_t* blocks) {
  if (!p || !blocks) return fail(DCF_ERR_ARG, "null argument");
  *blocks = 0;
  Workspace* w = nullptr;
  {  // take the workspace out of the pool (as a lease does), so the drain below holds no lock
    std::lock_guard<std::mutex> g(p->pool_mu);
    w = p->last_ws.load();
    if (!w || !w->d_ctr) return DCF_OK;
    auto it = std::find(p->free_ws.begin(), p->free_ws.end(), w);
    if (it == p->free_ws.end()) return fail(DCF_ERR_ARG, "the last eval's workspace is in use by another call");
    p->free_ws.erase(it);
  }
  int rc = DCF_OK;
  {
    DeviceGuard dg(p->device);
    hipError_t e = w->pending ? hipEventSynchronize(w->done) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpy(blocks, w->d_ctr + 2, sizeof(uint64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      rc = fail(DCF_ERR_HIP, std::string("dcf_prg_last_eval_blocks: ") + hipGetErrorString(e));
    } else {
      w->pending = false;  // drained
    }
  }
  std::lock_guard<std::mutex> g(p->pool_mu);
  p->free_ws.push_back(w);
  return rc;
}

int dcf_prg_set_phase_timing(dcf_prg* p, int on) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  if (on != 0 && on != 1) return fail(DCF_ERR_ARG, "on must be 0 or 1");
  p->timing = on;
  ++p->epoch;  // a timed call shows a whole call's split: the cross-call table state starts afresh
  return DCF_OK;
}

int dcf_prg_last_eval_phases(dcf_prg* p, float* prep_ms, float* walk_ms, int* prefix_levels) {
  if (!p || !prep_ms || !walk_ms) return fail(DCF_ERR_ARG, "null argument");
  *prep_ms = *walk_ms = 0.f;
  if (prefix_levels) *prefix_levels = 0;
  std::lock_guard<std::mutex> g(p->pool_mu);
  Workspace* w = p->last_ws.load();
  if (!w || !w->timed) return fail(DCF_ERR_ARG, "no timed eval yet (dcf_prg_set_phase_timing)");
  if (!ws_idle(p, w)) return fail(DCF_ERR_ARG, "the last eval's workspace is in use by another call");
  DeviceGuard dg(p->device);
  HIP_TRY(hipEventElapsedTime(prep_ms, w->tev[0], w->tev[1]));
  HIP_TRY(hipEventElapsedTime(walk_ms, w->tev[1], w->tev[2]));
  if (prefix_levels) *prefix_levels = (int)w->last_prefix;
  if (prefix_levels && w->last_prefix_dev && w->d_pst) {  // the depth the walk really read (cross-call table)
    uint32_t depth = 0;
    HIP_TRY(hipMemcpy(&depth, w->d_pst, sizeof(depth), hipMemcpyDeviceToHost));
    *prefix_levels = (int)depth;
    if (w->ph.valid && depth && depth != w->ph.depth) {  // the key changed in place: the host's guess catches up
      w->ph.depth = depth;
      w->ph.calls = 1;
    }
  }
  return DCF_OK;
}

int dcf_prg_trim(dcf_prg* p) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  std::vector<Workspace*> idle;
  {
    std::lock_guard<std::mutex> g(p->pool_mu);
    idle.swap(p->free_ws);
    for (Workspace* w : idle) p->all_ws.erase(std::find(p->all_ws.begin(), p->all_ws.end(), w));
    Workspace* last = p->last_ws.load();
    if (std::find(idle.begin(), idle.end(), last) != idle.end()) p->last_ws.store(nullptr);
  }
  DeviceGuard dg(p->device);
  for (Workspace* w : idle) free_workspace(w);  // waits for each one's last device work
  return (int)idle.size();
}

// Tiny host calls (the latency kernels' batch sizes): inputs and outputs through one pinned,
// device-mapped buffer that the kernel reads and writes itself — one launch, no copy commands.
constexpr size_t kTinyBytes = 1ull << 20;
// Small gen batches run the latency kernels of kernels_lat.h as well (eval's thresholds: plan_eval).
constexpr uint64_t kGenRowMax = 2048;    // keys up to which gen runs k_gen16_row (one wave per key; pipelined, r03t3:
                                         // 2048 keys 110 vs 148 us col, 4096 keys 149 vs 147, 8192 277 vs 165)
constexpr uint64_t kGenColMax = 16384;   // keys up to which gen runs k_gen16_col (r03a: 4096 keys 232 vs 562 us quads)
// Items per workgroup of the latency kernels: a small batch spread over the CUs (one wave per
// CU while it lasts), at most `cap` (a full 1024-thread workgroup).
static uint32_t per_wg(uint64_t items, int cus, uint32_t cap) {
  const uint64_t per = (items + (uint64_t)cus - 1) / (uint64_t)cus;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cap, per));
}
// ---- One plan per gen call: plan_gen() alone tests the gen path's thresholds;
// gen_launch, host_gen and dcf_gen_plan read the plan ----
enum class GenRoute {
  Row, Col,    // Hirose LAMBDA = 16, 8N <= 256: k_gen16_row (one wave per key) / k_gen16_col (16 lanes per key)
  Quad, Lane,  // Hirose LAMBDA = 16 otherwise: k_gen16<4> / k_gen16<1>
  Mmo16,       // k_gen16_mmo
  Wide,        // Hirose LAMBDA >= 32: k_gen_wide, one workgroup per key, kGenChunk keys per launch
  MmoWide,     // MMO LAMBDA >= 32: k_mmo_wide_gen head, then its tail over the blocks past the first
};
struct GenPlan {
  GenRoute route = GenRoute::Lane;
  bool counter = false;   // Quad / Lane: 64-lane units come from the work counter (else a grid-stride loop)
  uint64_t items = 0;     // Quad / Lane: lanes of the call (4 or 1 per key)
  uint64_t chunk = 0;     // Wide: keys per launch (scratch rows of 3 * LAMBDA bytes)
  uint64_t launches = 1;  // kernel launches of the call
  // dcf_gen of this N passes through the mapped tiny buffer: what a lone key runs on a latency kernel
  bool host_tiny = false;
};
// Where dcf_gen lays one key's inputs and CWB in its host / device buffer pair (256-byte aligned parts).
struct GenStage {
  size_t oa, ob, o0, o1, ok, cwb_len, total;
  GenStage(size_t nb, size_t lam)
      : oa(0), ob(align256(nb)), o0(ob + align256(lam)), o1(o0 + align256(lam)), ok(o1 + align256(lam)),
        cwb_len(dcf_cwb_bytes(nb, lam, 1)), total(ok + align256(cwb_len)) {}
};

static GenPlan plan_gen(const dcf_prg* p, size_t n_bytes, uint64_t num_keys) {
  GenPlan pl;
  const size_t lam = p->lambda;
  const bool col = p->kind == 0 && lam == 16 && 8 * n_bytes <= kColMaxLevels;  // the latency kernels' shapes
  pl.host_tiny = col && GenStage(n_bytes, lam).total <= kTinyBytes;
  if (p->kind == 1) {
    pl.route = lam > 16 ? GenRoute::MmoWide : GenRoute::Mmo16;
    if (pl.route == GenRoute::MmoWide) pl.launches = lam / 16 > 1 ? 2 : 1;
    return pl;
  }
  if (lam > 16) {  // keys in chunks (scratch 3 * LAMBDA per key)
    pl.route = GenRoute::Wide;
    pl.chunk = num_keys < kGenChunk ? num_keys : kGenChunk;
    pl.launches = pl.chunk ? (num_keys + pl.chunk - 1) / pl.chunk : 0;
    return pl;
  }
  if (col && num_keys <= kGenColMax) {
    // The smallest batches: one wave per key, one table lookup per lane and AES round (a lone key's
    // level is one 16-lane AES chain).  Small batches (a single key through the C ABI: benches/dcf.rs
    // bench_gen) are latency-bound: 16 lanes per key, one AES column each.
    pl.route = num_keys <= kGenRowMax ? GenRoute::Row : GenRoute::Col;
    return pl;
  }
  // Large batches: 64-lane units from the work counter (waves drift apart, as in k_eval16).
  // Lanes per key: a quad while the batch leaves lanes idle (a key's 8N levels take a quarter of
  // the AES latency: single gen 826 -> 266 us), one lane per key for large batches (2^20 keys:
  // 7.5-7.6 ms with one lane, 8.0 with quads — the four lanes repeat the level update).
  const bool quad = num_keys <= (uint64_t)p->cus * kBlock / 2;
  pl.route = quad ? GenRoute::Quad : GenRoute::Lane;
  pl.items = num_keys * (quad ? 4u : 1u);
  pl.counter = pl.items >= (uint64_t)p->cus * kBlock * 2 && (pl.items + 63) / 64 <= 0xFFFFFFFFull;
  return pl;
}

// The public image of GenRoute (include/dcf_hip.h); no default: a new GenRoute value fails to compile here.
static int public_gen_route(GenRoute r) {
  switch (r) {
    case GenRoute::Row: return DCF_GEN_ROW;
    case GenRoute::Col: return DCF_GEN_COL;
    case GenRoute::Quad: return DCF_GEN_QUAD;
    case GenRoute::Lane: return DCF_GEN_LANE;
    case GenRoute::Mmo16: return DCF_GEN_MMO16;
    case GenRoute::Wide: return DCF_GEN_WIDE;
    case GenRoute::MmoWide: return DCF_GEN_MMO_WIDE;
  }
  return -1;
}

int dcf_gen_plan(const dcf_prg* p, size_t n_bytes, size_t num_keys, int* route, int* counter, uint64_t* launches,
                 int* host_tiny) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  if (n_bytes == 0) return fail(DCF_ERR_N, "n_bytes must be > 0");
  const GenPlan pl = plan_gen(p, n_bytes, num_keys);
  if (route) *route = public_gen_route(pl.route);
  if (counter) *counter = pl.counter ? 1 : 0;
  if (launches) *launches = pl.launches;
  if (host_tiny) *host_tiny = pl.host_tiny ? 1 : 0;
  return DCF_OK;
}

static int gen_launch(dcf_prg* p, Lease& L, const GenPlan& plan, size_t n_bytes, size_t num_keys,
                      const uint8_t* alpha, const uint8_t* beta, const uint8_t* s0_0, const uint8_t* s0_1, int bound,
                      uint8_t* cwb_out) {
  Workspace* w = L.w;
  hipStream_t st = L.st;
  const size_t lam = p->lambda;
  const KeyBlockOut kb(cwb_out, n_bytes, lam, num_keys);
  uint8_t *cws = kb.cws, *cwv = kb.cwv, *cwt = kb.cwt, *np1 = kb.np1;
  switch (plan.route) {
    case GenRoute::MmoWide: return gen_mmo_wide(p, w, kb, alpha, beta, s0_0, s0_1, bound, plan.launches > 1, st);
    case GenRoute::Mmo16:  // Aes128MatyasMeyerOseasPrg (LAMBDA = 16)
      hipLaunchKernelGGL(k_gen16_mmo, dim3((unsigned)grid_for(num_keys, p->cus)), dim3(kBlock), 0, st, p->d_tab,
                         p->d_rk128, alpha, (const uint4*)beta, (const uint4*)s0_0, (const uint4*)s0_1, (uint32_t)bound,
                         (uint32_t)n_bytes, (uint64_t)num_keys, (uint4*)cws, (uint4*)cwv, cwt, (uint4*)np1);
      break;
    case GenRoute::Wide: {  // one workgroup per key
      if (int rc = ensure_ws(w, plan.chunk * 3 * lam, st)) return rc;
      for (uint64_t k0 = 0; k0 < num_keys; k0 += plan.chunk) {
        const uint64_t cnt = (num_keys - k0 < plan.chunk) ? num_keys - k0 : plan.chunk;
        hipLaunchKernelGGL(k_gen_wide, dim3((unsigned)cnt), dim3(kBlock), 0, st, p->d_tab, p->d_rk2, alpha,
                           beta, s0_0, s0_1, (uint32_t)bound, (uint32_t)n_bytes, (uint64_t)num_keys, k0, (uint32_t)lam,
                           cws, cwv, cwt, np1, w->d_ws);
        HIP_TRY(hipGetLastError());
      }
      return DCF_OK;
    }
    case GenRoute::Row: {
      const uint32_t kpw = per_wg(num_keys, p->cus, kBlock / 64);
      hipLaunchKernelGGL(k_gen16_row, dim3((unsigned)((num_keys + kpw - 1) / kpw)), dim3(kBlock), 0, st, p->d_tab,
                         p->rk[0], alpha, beta, s0_0, s0_1, (uint32_t)bound, (uint32_t)n_bytes, kpw,
                         (uint64_t)num_keys, cws, cwv, cwt, np1);
      break;
    }
    case GenRoute::Col: {
      const uint32_t kpw = per_wg(num_keys, p->cus, kBlock / 16);
      hipLaunchKernelGGL(k_gen16_col, dim3((unsigned)((num_keys + kpw - 1) / kpw)), dim3(kBlock), 0, st, p->d_tab,
                         p->rk[0], alpha, beta, s0_0, s0_1, (uint32_t)bound, (uint32_t)n_bytes, kpw,
                         (uint64_t)num_keys, cws, cwv, cwt, np1);
      break;
    }
    case GenRoute::Quad:
    case GenRoute::Lane: {
      uint32_t* ctr = nullptr;
      if (plan.counter) {
        if (int rc = ensure_ctr(w)) return rc;
        HIP_TRY(hipMemsetAsync(w->d_ctr, 0, kCtrBytes, st));
        ctr = w->d_ctr;
      }
      // Round keys in SGPRs (22 / 26 SGPR spills into VGPR lanes in the one-lane / quad instances):
      // per-round keys from the device copy spill none but gen ran 1-1.5 % slower (C5 r05l).
#define DCF_GEN16(LN)                                                                                                  \
  hipLaunchKernelGGL(k_gen16<LN>, dim3((unsigned)grid_for(plan.items, p->cus)), dim3(kBlock), 0, st, p->d_tab,         \
                     p->rk[0], alpha, (const uint4*)beta, (const uint4*)s0_0, (const uint4*)s0_1, (uint32_t)bound,     \
                     (uint32_t)n_bytes, (uint64_t)num_keys, (uint4*)cws, (uint4*)cwv, cwt, (uint4*)np1, ctr)
      if (plan.route == GenRoute::Quad) DCF_GEN16(4);
      else DCF_GEN16(1);
#undef DCF_GEN16
      break;
    }
  }
  HIP_TRY(hipGetLastError());
  return DCF_OK;
}

int dcf_gen_batch_device(dcf_prg* p, size_t n_bytes, size_t num_keys, const uint8_t* alpha, const uint8_t* beta,
                         const uint8_t* s0_0, const uint8_t* s0_1, int bound, uint8_t* cwb_out, void* stream) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  if (n_bytes == 0) return fail(DCF_ERR_N, "n_bytes must be > 0");
  if (bound != DCF_BOUND_LT_BETA && bound != DCF_BOUND_GT_BETA) return fail(DCF_ERR_ARG, "bad bound");
  if (num_keys == 0) return DCF_OK;
  if (!alpha || !beta || !s0_0 || !s0_1 || !cwb_out) return fail(DCF_ERR_ARG, "null buffer");
  DeviceGuard dg(p->device);
  Lease L(p);
  if (int rc = L.order((hipStream_t)stream)) return rc;
  return gen_launch(p, L, plan_gen(p, n_bytes, num_keys), n_bytes, num_keys, alpha, beta, s0_0, s0_1, bound, cwb_out);
}

// ---- Dcf::eval: one function per engine of the plan; first the A/B knobs of eval_stream's instance ladder ----
#ifndef DCF_SK_PFX
#define DCF_SK_PFX 1
#endif
// Single key below a shared-prefix table (C2 / C3 shapes): the instance whose starts all take the
// table row (PFX), so the fresh-x-word path (4 selects per stream and step) is compiled out; 87 ->
// 74 SGPRs.  r05v A/B (same box, 3 alternating runs): C3 491.3-491.7 vs 493.1-493.9 ms, C2
// 3.354-3.360 vs 3.391-3.396 ms (round 2's attempt at this split lost to a register-allocation flip).
constexpr bool kSkPfx = DCF_SK_PFX;
#ifndef DCF_STG
#define DCF_STG 1
#endif
// N <= 4 single key below the table (C2): prefix rows staged two iterations ahead into LDS by DMA
// (kernels_stream.h STG) instead of gathered at each point start.
constexpr bool kStg = DCF_STG;
#ifndef DCF_MK_NBC16
#define DCF_MK_NBC16 1
#endif
constexpr bool kMkNbc16 = DCF_MK_NBC16;  // A/B knob: the N = 16 multi-key top-tree instance
#ifndef DCF_MK_PK2
#define DCF_MK_PK2 1
#endif
// ... and of it, for a power-of-two points per key (C5: 64), point -> key by a shift instead of
// the division sequence (65 fewer VALU in the kernel)
constexpr bool kMkPk2 = DCF_MK_PK2;
#ifndef DCF_MK_NBC4
#define DCF_MK_NBC4 1
#endif
constexpr bool kMkNbc4 = DCF_MK_NBC4;  // A/B knob: the N = 4 multi-key top-tree instance (C5 at N = 4)

// Multi-key stream eval: keys per launch.  The kernel's work distribution, point and digest-row
// indices are 32-bit (kernels_stream.h StreamLane): a launch covers < 2^31 points, and its digest
// rows key * 8N + level index uint4 pairs (2 * row < 2^31), so at most 2^30 / 8N keys.
static uint64_t mk_keys_per_launch(size_t n_bytes, uint64_t ppk) {
  return std::max<uint64_t>(1, std::min<uint64_t>({1ull << 24, (1ull << 31) / ppk, (1ull << 30) / (8 * n_bytes)}));
}

size_t dcf_eval_keys_per_launch(size_t n_bytes, size_t points_per_key) {
  if (n_bytes == 0 || points_per_key == 0) return 0;
  return (size_t)mk_keys_per_launch(n_bytes, points_per_key);
}

// One eval call: num_keys keys x ppk points each, key-major, and the parts of its CWB (eval_launch).
struct EvalArgs {
  size_t n_bytes, num_keys, ppk;
  uint64_t total;  // num_keys * ppk
  int party;
  const uint8_t *cwb, *s0s, *xs;
  uint8_t* ys;
  KeyBlock kb;
};

// LAMBDA >= 32, head/tail pipeline: keys with few points batched, else per key.
static int eval_wide_engine(dcf_prg* p, Lease& L, const EvalPlan& plan, const EvalArgs& a) {
  const size_t lam = p->lambda;
  phase_mark(p, L, 1);
  if (plan.engine == Engine::WideBatch) return eval_wide_batch(p, L.w, a.kb, a.ppk, a.party, a.s0s, a.xs, a.ys, L.st);
  for (uint64_t k = 0; k < a.num_keys; ++k) {
    const uint8_t *s0 = a.s0s + k * lam, *xs = a.xs + k * a.ppk * a.n_bytes;
    uint8_t* ys = a.ys + k * a.ppk * lam;
    if (int rc = p->kind == 1 ? eval_mmo_wide(p, L.w, a.kb, k, a.party, s0, xs, a.ppk, ys, L.st)
                              : eval_wide(p, plan.depth, L.w, a.kb, k, a.party, s0, xs, a.ppk, ys, L.st))
      return rc;
  }
  return DCF_OK;
}

// MMO at LAMBDA = 16: lockstep, two blocks per level (the side's s and v), any engine setting.
static int eval_mmo16(dcf_prg* p, Lease& L, const EvalPlan& plan, const EvalArgs& a) {
  static constexpr decltype(&k_eval16_mmo<0>) kKernel[3] = {k_eval16_mmo<0>, k_eval16_mmo<1>, k_eval16_mmo<2>};
  PrefixTable pf{nullptr, 0u};
  if (int rc = try_prefix(p, L.c, L.w, a.party, a.kb, a.s0s, plan.depth, &pf, L.st))
    return rc;
  phase_mark(p, L, 1);
  hipLaunchKernelGGL(kKernel[plan.key_mode], dim3((unsigned)grid_for(a.total, p->cus)), dim3(kBlock), 0, L.st,
                     p->d_tab, p->d_rk128, a.kb.s4(), a.kb.v4(), a.kb.cwt, a.kb.np14(), (const uint4*)a.s0s, (uint32_t)a.party, a.xs,
                     (uint32_t)a.n_bytes, (uint64_t)a.num_keys, (uint64_t)a.ppk, (uint4*)a.ys, pf);
  HIP_TRY(hipGetLastError());
  return DCF_OK;
}

// The latency kernels (kernels_lat.h; each zeroes d_ctr itself), {kernel, lanes per point}.  row2, the very
// smallest batches: one wave per point, two levels per AES chain on right steps (rows 2 / 3 encrypt the right
// successor's blocks alongside the level's own).  row, the smallest: one table lookup per lane and AES round (a
// lone point's level is one 16-lane AES chain).  oct: tiny batches (a single point through the C ABI:
// benches/dcf.rs bench_eval) are latency-bound: one AES column per lane, A and B side by side.
static int eval_latency(dcf_prg* p, Lease& L, const EvalPlan& plan, const EvalArgs& a) {
  static constexpr std::pair<decltype(&k_eval16_oct), uint32_t> kLat[3] = {
      {k_eval16_row2, 64}, {k_eval16_row, 32}, {k_eval16_oct, 8}};
  const auto& lat = kLat[plan.engine == Engine::Row2 ? 0 : plan.engine == Engine::Row ? 1 : 2];
  phase_mark(p, L, 1);
  const uint32_t ppw = per_wg(a.total, p->cus, kBlock / lat.second);
  hipLaunchKernelGGL(lat.first, dim3((unsigned)((a.total + ppw - 1) / ppw)), dim3(kBlock), 0, L.st, p->d_tab, p->rk[0],
                     a.cwb, a.s0s, (uint32_t)a.party, a.xs, (uint32_t)a.n_bytes, ppw, a.total, a.ys, L.w->d_ctr);
  HIP_TRY(hipGetLastError());
  return DCF_OK;
}

// The pair walk (why and when: plan_eval); one key walks below its own table (small_prefix_depth).
static int eval_pair(dcf_prg* p, Lease& L, const EvalPlan& plan, const EvalArgs& a) {
  static constexpr decltype(&k_eval16_pair<0>) kKernel[3] = {k_eval16_pair<0>, k_eval16_pair<1>, k_eval16_pair<2>};
  const uint64_t total = a.total;
  PrefixTable spf{nullptr, 0u};
  if (int rc = try_prefix(p, L.c, L.w, a.party, a.kb, a.s0s, plan.depth, &spf, L.st))
    return rc;
  phase_mark(p, L, 1);
  // Whole waves per workgroup.  r06c (C1, same box, 4 alternating runs): rounding the lanes to a
  // pair instead, so that all 256 CUs get a workgroup (782 lanes, the last wave partial) rather than
  // 241 (13 whole waves), ran 0.913-0.915 vs 0.894-0.895 ms per step.
  uint64_t threads = (total * 2 + p->cus - 1) / p->cus;
  threads = std::min<uint64_t>(((threads + 63) / 64) * 64, kBlock);
  const dim3 g2((unsigned)((total * 2 + threads - 1) / threads)), b2((unsigned)threads);
  // (r06i: a per-lane block schedule for one key, k_eval16_pair2 — ~100 instead of 128 AES passes
  // per wave by simulation — ran 31 % slower on C1 and was removed; AB_LOG round 6)  Table: mode 0 only.
  hipLaunchKernelGGL(kKernel[plan.key_mode], g2, b2, 0, L.st, p->d_tab, p->rk[0], a.kb.s4(), a.kb.v4(), a.kb.cwt, a.kb.np14(),
                     (const uint4*)a.s0s, (uint32_t)a.party, a.xs, (uint32_t)a.n_bytes, (uint64_t)a.num_keys,
                     (uint64_t)a.ppk, (uint4*)a.ys, p->d_rk0, plan.key_mode == 0 ? spf : PrefixTable{nullptr, 0u});
  HIP_TRY(hipGetLastError());
  return DCF_OK;
}

// Stream engine, several keys: the per-key top trees (*pf; none: the walk starts at the root) and
// the key-major CW digest in w->d_kdig.
static int stream_multikey_prep(dcf_prg* p, Lease& L, const EvalArgs& a, PrefixTable* pf) {
  Workspace* w = L.w;
  hipStream_t st = L.st;
  const size_t n = 8 * a.n_bytes, num_keys = a.num_keys;
  if (L.c.prefix_levels != 0 && n > kMkPfxLevels && a.ppk >= 32 && num_keys <= (1ull << (31 - kMkPfxLevels))) {
    // per-key top trees (k_mk_prefix16: 32 rows per key); no room -> walk from the root (same bytes)
    const size_t need = (size_t)num_keys * (32u << kMkPfxLevels);
    w->ph.valid = false;  // d_pfx changes hands
    hipError_t oom;
    if (int rc = reserve_pfx(w, need, st, &oom)) return rc;
    if (w->pfx_bytes >= need) {
      *pf = PrefixTable{(const uint4*)w->d_pfx, kMkPfxLevels};
      w->last_prefix = kMkPfxLevels;
    }
  }
  // The top trees (k_mk_prefix16: LDS-bound AES, 128 KiB of LDS per workgroup) on the
  // workspace's second stream while the key-major digest (kernels_stream.h: memory-bound,
  // 17 KiB per workgroup, so one fits beside a top-tree workgroup on a CU) is written on the
  // call's stream; the walk waits for both.
  if (int rc = grow(&w->d_kdig, &w->kdig_bytes, (size_t)num_keys * n * 33, st)) return rc;
  const bool fork = pf->levels != 0;
  // Once the top trees are queued on aux, every exit from this function — the normal one and an
  // error return — joins aux into the call's stream (the walk and the lease's `done` event must
  // cover them: the next user of this workspace overwrites d_pfx / d_ctr); if the join cannot
  // be queued, aux is drained on the host instead.
  struct AuxJoin {
    Workspace* w;
    hipStream_t st;
    bool armed = false;
    ~AuxJoin() {
      if (!armed) return;
      if (hipEventRecord(w->aux_ev[1], w->aux) != hipSuccess || hipStreamWaitEvent(st, w->aux_ev[1], 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(w->aux);
      }
    }
  } join{w, st};
  if (fork) {
    if (!w->aux) HIP_TRY(hipStreamCreateWithFlags(&w->aux, hipStreamNonBlocking));
    for (auto& e : w->aux_ev)
      if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(w->aux_ev[0], st));
    HIP_TRY(hipStreamWaitEvent(w->aux, w->aux_ev[0], 0));
    join.armed = true;
    hipLaunchKernelGGL(k_mk_prefix16<true>, dim3((unsigned)(((num_keys << kMkPfxRoot) + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, w->aux, p->d_tab, p->rk[0], a.kb.s4(), a.kb.v4(), a.kb.cwt, (const uint4*)a.s0s,
                       (uint32_t)a.party, (uint64_t)num_keys, (uint4*)w->d_pfx, p->d_rk0, w->d_ctr);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_cw_keymajor, dim3((unsigned)((num_keys + kKmKeys - 1) / kKmKeys), (unsigned)((n + kKmLevs - 1) / kKmLevs)),
                     dim3(kKmThreads), 0, st, a.kb.s4(), a.kb.v4(), a.kb.cwt, (uint32_t)n, (uint64_t)num_keys, (uint4*)w->d_kdig,
                     w->d_kdig + (size_t)num_keys * n * 32);
  HIP_TRY(hipGetLastError());
  return DCF_OK;  // (the join runs here, as `join` leaves scope: the walk waits for the top trees)
}

// Stream engine, one key: the shared-prefix table of the plan's depth.  The cross-call table
// (reuse_prefix; last_prefix_dev: the walk reads its depth from d_pst): dcf_eval_device calls that
// run a single-key table-start instance.
static int stream_table(dcf_prg* p, Lease& L, const EvalPlan& plan, const EvalArgs& a, PrefixTable* pf) {
  if (!(plan.depth && L.reuse && kSkPfx && (a.n_bytes == 16 || a.n_bytes == 4) && a.total < (1ull << 31)))
    return try_prefix(p, L.c, L.w, a.party, a.kb, a.s0s, plan.depth, pf, L.st);
  if (int rc = reuse_prefix(p, L.c, L.w, a.party, a.kb, a.s0s, plan.depth, a.total, pf, L.st)) return rc;
  L.w->last_prefix = pf->levels;
  L.w->last_prefix_dev = pf->levels != 0;
  return DCF_OK;
}

// Stream engine: table preparation (several keys: top trees and digest; one key: the table), then the
// walk.  One launch covers < 2^31 points (multi-key: mk_keys_per_launch whole keys).  Larger batches run
// as several launches over consecutive points / whole keys, sharing the table and the digest.
static int eval_stream(dcf_prg* p, Lease& L, const EvalPlan& plan, const EvalArgs& a) {
  constexpr int NS = 2;  // streams per lane
  Workspace* w = L.w;
  hipStream_t st = L.st;
  PrefixTable pf{nullptr, 0u};
  if (int rc = a.num_keys > 1 ? stream_multikey_prep(p, L, a, &pf) : stream_table(p, L, plan, a, &pf)) return rc;
  phase_mark(p, L, 1);
  const size_t n_bytes = a.n_bytes, n = 8 * n_bytes, ppk = a.ppk;
  const uint64_t total = a.total;
  const uint32_t* pst = w->last_prefix_dev ? w->d_pst : nullptr;  // cross-call table: its depth
  const bool xreg = n_bytes % 4 == 0 && n_bytes <= 16, multi = a.num_keys > 1;
  // several keys: the key-major digest of stream_multikey_prep
  const uint4* scs = multi ? (const uint4*)w->d_kdig : a.kb.s4();
  const uint8_t* sct = multi ? w->d_kdig + (size_t)a.num_keys * n * 32 : a.kb.cwt;
  const uint64_t kpl = multi ? mk_keys_per_launch(n_bytes, ppk) : 1;
  const uint64_t ppl = multi ? kpl * ppk : (1ull << 31);  // points per launch
  for (uint64_t c0 = 0; c0 < total; c0 += ppl) {
    const uint64_t cnt = std::min<uint64_t>(ppl, total - c0), k0 = multi ? c0 / ppk : 0, kc = multi ? cnt / ppk : 1;
    // each walk's work counter starts at 0 (the block count beside it keeps the per-key top
    // trees' blocks): eval_launch zeroed it for the first launch (the table builds and the
    // digest do not touch it), so a one-launch eval has no fill between the build and the walk
    if (c0 > 0) HIP_TRY(hipMemsetAsync(w->d_ctr, 0, 8, st));
    const uint64_t units = (cnt + kStreamUnit - 1) / kStreamUnit;
    const uint64_t blocks = std::min<uint64_t>((units + 15) / 16, (uint64_t)p->cus);
    const uint4* lcs = multi ? scs + k0 * 2 * n : scs;
    const uint8_t* lct = multi ? sct + k0 * n : sct;
    const uint4* lnp1 = a.kb.np14() + k0;
    const uint8_t* lxs = a.xs + c0 * n_bytes;
    uint8_t* lys = a.ys + c0 * 16;
    const uint8_t* ls0 = a.s0s + k0 * 16;
    const PrefixTable lpf = (multi && pf.levels) ? PrefixTable{pf.sv + 2 * (k0 << pf.levels), pf.levels} : pf;
#define DCF_STREAM(XR, MK, PF, NBC, PK2, STG)                                                                        \
  hipLaunchKernelGGL((k_eval16_stream<NS, XR, MK, PF, NBC, PK2, STG>), dim3((unsigned)blocks), dim3(kBlock), 0, st,   \
                     p->d_tab, p->rk[0], lcs, a.kb.v4(), lct, lnp1, (const uint4*)ls0, (uint32_t)a.party, lxs,          \
                     (uint32_t)n_bytes, (uint64_t)kc, (uint64_t)ppk, (uint64_t)cnt, w->d_ctr, (uint4*)lys, lpf,       \
                     p->d_rk0, pst)
    // multi-key: an instance for "per-key top trees present" (no root-seed start path: 48 -> 33
    // SGPR spills; C5 r03c A/B 414.6 / 413.7 vs 408.5 / 408.1 M evals/s), and of it one with the
    // x width fixed at N = 16 (C5: 33 -> 18 SGPR spills, 121 -> 119 VGPRs, r05k).  Single key, x in
    // registers: N = 16 (C1 / C3) and N = 4 (C2) with the x width fixed at compile time (a
    // point's start loads x without width branches: C2 starts a point every ~13 AES slots).
    if (multi && lpf.levels) {
      if (xreg && n_bytes == 16 && kMkNbc16 && kMkPk2 && (ppk & (ppk - 1)) == 0) DCF_STREAM(true, true, true, 16, true, false);
      else if (xreg && n_bytes == 16 && kMkNbc16) DCF_STREAM(true, true, true, 16, false, false);
      else if (xreg && n_bytes == 4 && kMkNbc4 && (ppk & (ppk - 1)) == 0) DCF_STREAM(true, true, true, 4, true, false);
      else if (xreg) DCF_STREAM(true, true, true, 0, false, false);
      else DCF_STREAM(false, true, true, 0, false, false);
    } else if (multi) {
      if (xreg) DCF_STREAM(true, true, false, 0, false, false);
      else DCF_STREAM(false, true, false, 0, false, false);
    } else if (xreg && n_bytes == 16 && lpf.levels && kSkPfx) {
      DCF_STREAM(true, false, true, 16, false, false);  // every start below the shared prefix: no fresh-x-word path
    } else if (xreg && n_bytes == 16) {
      DCF_STREAM(true, false, false, 16, false, false);
    } else if (xreg && n_bytes == 4 && lpf.levels && kSkPfx && kStg) {
      DCF_STREAM(true, false, true, 4, false, true);  // rows staged two iterations ahead (C2)
    } else if (xreg && n_bytes == 4 && lpf.levels && kSkPfx) {
      DCF_STREAM(true, false, true, 4, false, false);
    } else if (xreg && n_bytes == 4) {
      DCF_STREAM(true, false, false, 4, false, false);
    } else if (xreg) {
      DCF_STREAM(true, false, false, 0, false, false);
    } else {
      DCF_STREAM(false, false, false, 0, false, false);
    }
#undef DCF_STREAM
    HIP_TRY(hipGetLastError());
  }
  return DCF_OK;
}

// Lockstep T-table walk (k_eval16), 64-point units from the work counter.
static int eval_ttable(dcf_prg* p, Lease& L, const EvalPlan& plan, const EvalArgs& a) {
  static constexpr decltype(&k_eval16<0>) kKernel[3] = {k_eval16<0>, k_eval16<1>, k_eval16<2>};
  phase_mark(p, L, 1);
  hipLaunchKernelGGL(kKernel[plan.key_mode], dim3((unsigned)grid_for(a.total, p->cus)), dim3(kBlock), 0, L.st,
                     p->d_tab, p->rk[0], a.kb.s4(), a.kb.v4(), a.kb.cwt, a.kb.np14(), (const uint4*)a.s0s, (uint32_t)a.party, a.xs,
                     (uint32_t)a.n_bytes, (uint64_t)a.num_keys, (uint64_t)a.ppk, (uint4*)a.ys, L.w->d_ctr);
  HIP_TRY(hipGetLastError());
  return DCF_OK;
}

// Dcf::eval of the call `a` by the engine of its plan.  Phase mark 1 (dcf_prg_set_phase_timing) sits in
// every engine before the walk kernel, after any table / digest preparation.
static int eval_body(dcf_prg* p, Lease& L, const EvalPlan& plan, const EvalArgs& a) {
  if (plan.unsupported) return fail(DCF_ERR_UNSUPPORTED, plan.unsupported);
  switch (plan.engine) {
    case Engine::WideBatch:
    case Engine::WidePerKey: return eval_wide_engine(p, L, plan, a);
    case Engine::Mmo16: return eval_mmo16(p, L, plan, a);
    case Engine::Pair: return eval_pair(p, L, plan, a);
    case Engine::Stream: return eval_stream(p, L, plan, a);
    case Engine::TTable: return eval_ttable(p, L, plan, a);
    default: return eval_latency(p, L, plan, a);  // Row2, Row, Oct
  }
}

// Dcf::eval of K keys x ppk points on the lease's stream (arguments checked by the caller; the
// range and multi-GPU drivers come through here as well).  Phase marks: 0 at entry, 2 at the end.
static int eval_launch(dcf_prg* p, Lease& L, size_t n_bytes, size_t num_keys, size_t ppk, int party,
                       const uint8_t* cwb, const uint8_t* s0s, const uint8_t* xs, uint8_t* ys) {
  if (int rc = ensure_ctr(L.w)) return rc;
  const EvalPlan plan = plan_eval(p, L.c, n_bytes, num_keys, ppk);
  // the block count (dcf_prg_last_eval_blocks) covers the whole call: zeroed once here (the
  // latency kernels zero it themselves: one command less on a ~100 us call)
  if (!plan.latency()) HIP_TRY(hipMemsetAsync(L.w->d_ctr, 0, kCtrBytes, L.st));
  L.w->last_prefix = 0;
  L.w->last_prefix_dev = false;
  phase_mark(p, L, 0);
  const EvalArgs a{n_bytes, num_keys, ppk, (uint64_t)num_keys * ppk, party, cwb, s0s, xs, ys,
                   KeyBlock(cwb, n_bytes, p->lambda, num_keys)};
  const int rc = eval_body(p, L, plan, a);
  phase_mark(p, L, 2);
  p->last_ws.store(L.w);
  return rc;
}

static int check_eval_args(dcf_prg* p, size_t n_bytes, int party, uint64_t total, const void* cwb, const void* s0s,
                           const void* xs, const void* ys) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  if (n_bytes == 0) return fail(DCF_ERR_N, "n_bytes must be > 0");
  if (party != 0 && party != 1) return fail(DCF_ERR_ARG, "party must be 0 or 1");
  if (total && (!cwb || !s0s || !xs || !ys)) return fail(DCF_ERR_ARG, "null buffer");
  return DCF_OK;
}

int dcf_eval_device(dcf_prg* p, size_t n_bytes, int party, const uint8_t* cwb, const uint8_t* s0,
                    const uint8_t* xs, size_t m, uint8_t* ys, void* stream) {
  if (int rc = check_eval_args(p, n_bytes, party, m, cwb, s0, xs, ys)) return rc;
  if (m == 0) return DCF_OK;
  DeviceGuard dg(p->device);
  Lease L(p);
  L.reuse = true;
  if (int rc = L.order((hipStream_t)stream)) return rc;
  return eval_launch(p, L, n_bytes, 1, m, party, cwb, s0, xs, ys);
}

int dcf_eval_multikey_device(dcf_prg* p, size_t n_bytes, size_t num_keys, size_t points_per_key, int party,
                             const uint8_t* cwb, const uint8_t* s0s, const uint8_t* xs, uint8_t* ys,
                             void* stream) {
  const uint64_t total = (uint64_t)num_keys * points_per_key;
  if (int rc = check_eval_args(p, n_bytes, party, total, cwb, s0s, xs, ys)) return rc;
  if (total == 0) return DCF_OK;
  DeviceGuard dg(p->device);
  Lease L(p);
  if (int rc = L.order((hipStream_t)stream)) return rc;
  return eval_launch(p, L, n_bytes, num_keys, points_per_key, party, cwb, s0s, xs, ys);
}

// ---- host-pointer path: per-workspace streams and staging, chunked pipeline ----

// Points per chunk of the host eval pipeline: ~128 MiB of x + y per buffer (C3 shape: 4 Mi
// points, an 8 ms kernel against ~3 ms of PCIe each way, so the copies hide behind it).
constexpr size_t kHostChunkBytes = 128ull << 20;
constexpr size_t kHostMidBytes = 64ull << 20;  // x + y of a mid-size host eval through the mapped buffer

static int ensure_host_path(Workspace* w) {
  if (w->hs[0]) return DCF_OK;
  hipStream_t hs[3] = {nullptr, nullptr, nullptr};
  for (auto& s : hs) HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  for (auto& e : w->hev)
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (int i = 0; i < 3; ++i) w->hs[i] = hs[i];
  return DCF_OK;
}

static int ensure_stage(Workspace* w, size_t hbytes, size_t dbytes) {
  if (w->h_stage_bytes < hbytes) {
    if (w->h_stage) HIP_TRY(hipHostFree(w->h_stage));
    w->h_stage = nullptr;
    w->h_stage_bytes = 0;
    HIP_TRY(hipHostMalloc((void**)&w->h_stage, hbytes, hipHostMallocDefault));
    w->h_stage_bytes = hbytes;
  }
  if (w->d_stage_bytes < dbytes) {
    if (w->d_stage) HIP_TRY(hipFree(w->d_stage));
    w->d_stage = nullptr;
    w->d_stage_bytes = 0;
    HIP_TRY(hipMalloc(&w->d_stage, dbytes));
    w->d_stage_bytes = dbytes;
  }
  return DCF_OK;
}

// The tiny-call buffer: coherent (the kernel's stores are visible once the stream has passed
// it) and mapped into the device's address space.  Returns its device address.
static int ensure_tiny(Workspace* w, uint8_t** dptr) {
  if (!w->h_tiny) {
    HIP_TRY(hipHostMalloc((void**)&w->h_tiny, kTinyBytes, hipHostMallocMapped | hipHostMallocCoherent));
    w->tiny_bytes = kTinyBytes;
  }
  HIP_TRY(hipHostGetDevicePointer((void**)dptr, w->h_tiny, 0));
  return DCF_OK;
}

// The mid-size host buffer: mapped into the device's address space, coarse-grained (the GPU may
// cache it; the host reads the outputs only after the stream has passed the kernel; fine-grained
// measured the same, r03y2 C1 host path 143-148 vs 141-146 M evals/s).  Grown on demand and kept.
// Returns its device address.
static int ensure_mid(Workspace* w, size_t bytes, uint8_t** dptr) {
  if (w->mid_bytes < bytes) {
    if (w->h_mid) HIP_TRY(hipHostFree(w->h_mid));
    w->h_mid = nullptr;
    w->mid_bytes = 0;
    HIP_TRY(hipHostMalloc((void**)&w->h_mid, bytes,
                          hipHostMallocMapped | hipHostMallocNonCoherent));
    w->mid_bytes = bytes;
  }
  HIP_TRY(hipHostGetDevicePointer((void**)dptr, w->h_mid, 0));
  return DCF_OK;
}

// Every host entry point ends here: wait for the workspace's own streams only (never the
// whole device), also after an error, so no queued copy still targets the staging buffers.
static int host_finish(Lease& L, int rc) {
  Workspace* w = L.w;
  bool ok = true;
  for (int i = 0; i < 3; ++i) {
    if (!w->hs[i] || !((w->host_streams >> i) & 1u)) continue;
    const hipError_t e = hipStreamSynchronize(w->hs[i]);
    if (e != hipSuccess) {
      ok = false;
      (void)hipGetLastError();
      if (rc == DCF_OK) rc = fail(DCF_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    }
  }
  w->host_streams = 0;
  L.drained = ok;
  return rc;
}

// A lease for a host entry point: its workspace's streams exist and the compute stream is
// ordered after the workspace's earlier device work (a *_device call on any stream).
static int host_lease(Lease& L) {
  if (int rc = ensure_host_path(L.w)) return rc;
  L.w->host_streams = 2u;  // the compute stream; the chunked eval pipeline adds copy-in / copy-out
  return L.order(L.w->hs[1]);
}

// A host entry point's frame: the prg's device, a host lease, body(L), host_finish.
extern "C++" template <class Body>
static int host_call(dcf_prg* p, Body body) {
  DeviceGuard dg(p->device);
  if (!dg.ok) return fail(DCF_ERR_HIP, "hipSetDevice failed");
  Lease L(p);
  int rc = host_lease(L);
  if (rc == DCF_OK) rc = body(L);
  return host_finish(L, rc);
}

// The checks the host evals share ahead of their points (as check_eval_args for the device ones): `null_arg`
// (the entry's own pointers), N, party, and the size of the one key against the prg's LAMBDA.
static int check_host_key(bool null_arg, size_t n_bytes, int party, const dcf_prg* p, size_t cwb_len) {
  if (null_arg) return fail(DCF_ERR_ARG, "null argument");
  if (n_bytes == 0) return fail(DCF_ERR_N, "n_bytes must be > 0");
  if (party != 0 && party != 1) return fail(DCF_ERR_ARG, "party must be 0 or 1");
  if (cwb_len != dcf_cwb_bytes(n_bytes, p->lambda, 1))
    return fail(DCF_ERR_KEY, "key size does not match 8*N levels (lib.rs:165)");
  return DCF_OK;
}

// Dcf::eval over host buffers (caller: DeviceGuard held, arguments checked, m > 0).
// Tiny batches: one launch of a latency kernel (k_eval16_row / k_eval16_oct) that reads the key and points from, and writes
// the outputs to, the workspace's mapped pinned buffer.  Otherwise chunks of `chunk` points
// flow through two staging slots on three streams: copy-in (pinned -> device), compute
// (eval_launch), copy-out (device -> pinned); the host copies chunk c's x into pinned memory
// and chunk c-1's y out of it while the GPU works on chunk c, so PCIe transfers overlap the
// kernels of neighbouring chunks.  The GPU never touches caller memory.
static int host_eval(dcf_prg* p, Lease& L, size_t nb, int party, const uint8_t* cwb, size_t cwb_len,
                     const uint8_t* s0, const uint8_t* xs, uint64_t m, uint8_t* ys) {
  Workspace* w = L.w;
  const size_t lam = p->lambda;
  const size_t ko = 0, so0 = align256(cwb_len), xo = so0 + 256, yo = xo + align256(m * nb);
  const EvalPlan plan = plan_eval(p, L.c, nb, 1, m);  // of the whole batch: which host path
  if (plan.latency() && yo + m * lam <= kTinyBytes) {
    uint8_t* d = nullptr;
    if (int rc = ensure_tiny(w, &d)) return rc;
    uint8_t* h = w->h_tiny;
    memcpy(h + ko, cwb, cwb_len);
    memcpy(h + so0, s0, lam);
    memcpy(h + xo, xs, m * nb);
    if (int rc = eval_launch(p, L, nb, 1, m, party, d + ko, d + so0, d + xo, d + yo)) return rc;
    HIP_TRY(hipStreamSynchronize(L.st));
    memcpy(ys, h + yo, m * lam);
    return DCF_OK;
  }
  // Mid-size batches (the small-batch kernels' range, LAMBDA = 16): the kernel reads x from and
  // writes y to a mapped pinned buffer, so the call is one host copy in, a 4 KiB key copy, one
  // launch, one stream sync and one host copy out — no staging DMAs or chunk events (a C1-size
  // call is one chunk, its copies cannot overlap its kernel anyway).  The key goes to device
  // memory first: the walk reads a correction word per level.
  if (plan.small && m * (nb + lam) <= kHostMidBytes) {
    const size_t kb = align256(cwb_len) + align256(lam);
    const size_t mx = align256(m * nb), need = kb + mx + m * lam;
    uint8_t* d = nullptr;
    if (int rc = ensure_mid(w, need, &d)) return rc;
    if (int rc = ensure_stage(w, 0, kb)) return rc;
    uint8_t* h = w->h_mid;
    memcpy(h, cwb, cwb_len);
    memcpy(h + align256(cwb_len), s0, lam);
    memcpy(h + kb, xs, m * nb);
    HIP_TRY(hipMemcpyAsync(w->d_stage, h, kb, hipMemcpyHostToDevice, L.st));
    if (int rc = eval_launch(p, L, nb, 1, m, party, w->d_stage, w->d_stage + align256(cwb_len), d + kb, d + kb + mx))
      return rc;
    HIP_TRY(hipStreamSynchronize(L.st));
    memcpy(ys, h + kb + mx, m * lam);
    return DCF_OK;
  }
  w->host_streams = 7u;
  const uint64_t chunk = std::min<uint64_t>(m, std::max<uint64_t>(256, kHostChunkBytes / (nb + lam)));
  const int nbuf = m > chunk ? 2 : 1;
  const size_t kb = align256(cwb_len) + align256(lam);
  const size_t xb = align256(chunk * nb), yb = align256(chunk * lam);
  if (int rc = ensure_stage(w, nbuf * (xb + yb), kb + nbuf * (xb + yb))) return rc;
  uint8_t* dk = w->d_stage;
  uint8_t* ds0 = dk + align256(cwb_len);
  uint8_t *dx[2], *dy[2], *hx[2], *hy[2];
  for (int b = 0; b < nbuf; ++b) {
    dx[b] = dk + kb + b * xb;
    dy[b] = dk + kb + nbuf * xb + b * yb;
    hx[b] = w->h_stage + b * xb;
    hy[b] = w->h_stage + nbuf * xb + b * yb;
  }
  hipStream_t si = w->hs[0], sc = w->hs[1], so = w->hs[2];
  hipEvent_t *ev_in = w->hev, *ev_k = w->hev + 2, *ev_out = w->hev + 4;
  HIP_TRY(hipMemcpyAsync(dk, cwb, cwb_len, hipMemcpyHostToDevice, sc));
  HIP_TRY(hipMemcpyAsync(ds0, s0, lam, hipMemcpyHostToDevice, sc));
  const uint64_t nch = (m + chunk - 1) / chunk;
  for (uint64_t c = 0; c <= nch; ++c) {
    if (c < nch) {
      const int b = (int)(c & (nbuf - 1));
      const uint64_t off = c * chunk, cnt = std::min<uint64_t>(chunk, m - off);
      if (c >= 2) HIP_TRY(hipEventSynchronize(ev_in[b]));  // chunk c-2's H2D has read hx[b]
      memcpy(hx[b], xs + off * nb, cnt * nb);
      if (c >= 2) HIP_TRY(hipStreamWaitEvent(si, ev_k[b], 0));  // chunk c-2's kernel is done with dx[b]
      HIP_TRY(hipMemcpyAsync(dx[b], hx[b], cnt * nb, hipMemcpyHostToDevice, si));
      HIP_TRY(hipEventRecord(ev_in[b], si));
      HIP_TRY(hipStreamWaitEvent(sc, ev_in[b], 0));
      if (c >= 2) HIP_TRY(hipStreamWaitEvent(sc, ev_out[b], 0));  // chunk c-2's D2H is done with dy[b]
      if (int rc = eval_launch(p, L, nb, 1, cnt, party, dk, ds0, dx[b], dy[b])) return rc;
      HIP_TRY(hipEventRecord(ev_k[b], sc));
      HIP_TRY(hipStreamWaitEvent(so, ev_k[b], 0));
      HIP_TRY(hipMemcpyAsync(hy[b], dy[b], cnt * lam, hipMemcpyDeviceToHost, so));
      HIP_TRY(hipEventRecord(ev_out[b], so));
    }
    if (c >= 1) {  // drain chunk c-1 while chunk c is in flight
      const uint64_t pc = c - 1;
      const int b = (int)(pc & (nbuf - 1));
      const uint64_t off = pc * chunk, cnt = std::min<uint64_t>(chunk, m - off);
      HIP_TRY(hipEventSynchronize(ev_out[b]));
      memcpy(ys + off * lam, hy[b], cnt * lam);
    }
  }
  return DCF_OK;
}

// Dcf::gen for one key over host buffers, on the workspace's compute stream.  Tiny path (the
// column kernel): inputs and the CWB through the mapped pinned buffer, one launch.
static int host_gen(dcf_prg* p, Lease& L, size_t nb, const uint8_t* alpha, const uint8_t* beta, const uint8_t* s0_0,
                    const uint8_t* s0_1, int bound, uint8_t* cwb_out) {
  Workspace* w = L.w;
  const size_t lam = p->lambda;
  const GenStage g(nb, lam);
  const size_t oa = g.oa, ob = g.ob, o0 = g.o0, o1 = g.o1, ok = g.ok, cwb_len = g.cwb_len, total = g.total;
  const GenPlan plan = plan_gen(p, nb, 1);
  const bool tiny = plan.host_tiny;
  uint8_t *h = nullptr, *d = nullptr;
  if (tiny) {
    if (int rc = ensure_tiny(w, &d)) return rc;
    h = w->h_tiny;
  } else {
    if (int rc = ensure_stage(w, total, total)) return rc;
    h = w->h_stage;
    d = w->d_stage;
  }
  memcpy(h + oa, alpha, nb);
  memcpy(h + ob, beta, lam);
  memcpy(h + o0, s0_0, lam);
  memcpy(h + o1, s0_1, lam);
  hipStream_t sc = L.st;
  if (!tiny) HIP_TRY(hipMemcpyAsync(d, h, ok, hipMemcpyHostToDevice, sc));
  if (!tiny) HIP_TRY(hipMemsetAsync(d + ok, 0, cwb_len, sc));  // the CWB's padding bytes read 0
  int rc = gen_launch(p, L, plan, nb, 1, d + oa, d + ob, d + o0, d + o1, bound, d + ok);
  if (rc) return rc;
  if (!tiny) HIP_TRY(hipMemcpyAsync(h + ok, d + ok, cwb_len, hipMemcpyDeviceToHost, sc));
  HIP_TRY(hipStreamSynchronize(sc));
  memcpy(cwb_out, h + ok, cwb_len);
  if (tiny) {  // the CWB's padding bytes (between cw_t and cw_np1) read 0, as on the staged path
    const KeyBlockOut kb(cwb_out, nb, lam, 1);
    memset(kb.cwt + kb.nlev, 0, kb.np1 - (kb.cwt + kb.nlev));
  }
  return DCF_OK;
}

// Prg::gen for m seeds over host buffers (test hook), on the workspace's compute stream.
static int host_prg_gen(dcf_prg* p, Lease& L, const uint8_t* seeds, size_t m, uint8_t* out) {
  Workspace* w = L.w;
  const size_t lam = p->lambda, row = 4 * lam + 2;
  const size_t so = align256(m * lam), total = so + align256(m * row);
  if (int rc = ensure_stage(w, total, total)) return rc;
  uint8_t *h = w->h_stage, *d = w->d_stage;
  hipStream_t sc = L.st;
  memcpy(h, seeds, m * lam);
  HIP_TRY(hipMemcpyAsync(d, h, m * lam, hipMemcpyHostToDevice, sc));
  if (p->kind == 1 && lam > 16)
    hipLaunchKernelGGL(k_prg_mmo_wide, dim3((unsigned)grid_for(m * (lam / 16), p->cus)), dim3(kBlock), 0, sc,
                       p->d_tab, p->d_rk128, (const uint8_t*)d, (uint64_t)m, (uint32_t)lam, d + so);
  else if (p->kind == 1)
    hipLaunchKernelGGL(k_prg16_mmo, dim3((unsigned)grid_for(m, p->cus)), dim3(kBlock), 0, sc, p->d_tab, p->d_rk128,
                       (const uint4*)d, (uint64_t)m, d + so);
  else if (lam == 16)
    hipLaunchKernelGGL(k_prg16, dim3((unsigned)grid_for(m, p->cus)), dim3(kBlock), 0, sc, p->d_tab, p->rk[0],
                       (const uint4*)d, (uint64_t)m, d + so);
  else
    hipLaunchKernelGGL(k_prg_wide, dim3((unsigned)std::min<uint64_t>((m * (lam / 16) + 255) / 256, 65535)),
                       dim3(256), 0, sc, p->d_tab, p->d_rk2, (const uint8_t*)d, (uint64_t)m, (uint32_t)lam,
                       d + so);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h + so, d + so, m * row, hipMemcpyDeviceToHost, sc));
  HIP_TRY(hipStreamSynchronize(sc));
  memcpy(out, h + so, m * row);
  return DCF_OK;
}

// ---- serde / bincode wire format of Share (lib.rs:217-340) ----
// bincode 1.x `serialize` (the crate's declared dep, Cargo.toml:44): little-endian,
// u64 length prefix per Vec, struct fields in declaration order, bool as one byte.

size_t dcf_share_bincode_bytes(size_t n_bytes, size_t lambda, size_t num_s0s) {
  const size_t n = 8 * n_bytes;
  return 8 + num_s0s * (8 + lambda) + 8 + n * (2 * (8 + lambda) + 2) + 8 + lambda;
}

static void put_u64(uint8_t*& o, uint64_t v) {
  for (int i = 0; i < 8; i++) *o++ = (uint8_t)(v >> (8 * i));
}

int dcf_share_to_bincode(size_t n_bytes, size_t lambda, const uint8_t* cwb, const uint8_t* s0s, size_t num_s0s,
                         uint8_t* out, size_t out_len) {
  if (!cwb || !out || (num_s0s && !s0s)) return fail(DCF_ERR_ARG, "null argument");
  if (n_bytes == 0) return fail(DCF_ERR_N, "n_bytes must be > 0");
  if (lambda == 0 || lambda % 16) return fail(DCF_ERR_LAMBDA, "lambda must be a positive multiple of 16");
  if (out_len != dcf_share_bincode_bytes(n_bytes, lambda, num_s0s)) return fail(DCF_ERR_LEN, "bad out_len");
  const size_t n = 8 * n_bytes;
  uint8_t* o = out;
  put_u64(o, num_s0s);  // s0s: Vec<Vec<u8>> (lib.rs:291-292)
  for (size_t i = 0; i < num_s0s; i++) {
    put_u64(o, lambda);
    memcpy(o, s0s + i * lambda, lambda);
    o += lambda;
  }
  put_u64(o, n);  // cws: Vec<Cw> (lib.rs:293), Cw = (s, v, tl, tr) (lib.rs:222-227)
  for (size_t i = 0; i < n; i++) {
    put_u64(o, lambda);
    memcpy(o, cwb + i * lambda, lambda);
    o += lambda;
    put_u64(o, lambda);
    memcpy(o, cwb + (n + i) * lambda, lambda);
    o += lambda;
    const uint8_t t = cwb[2 * n * lambda + i];
    *o++ = t & 1;
    *o++ = (t >> 1) & 1;
  }
  put_u64(o, lambda);  // cw_np1 (lib.rs:294)
  memcpy(o, cwb + dcf_cwb_np1_offset(n_bytes, lambda, 1), lambda);
  return DCF_OK;
}

int dcf_share_from_bincode(size_t n_bytes, size_t lambda, const uint8_t* in, size_t in_len, uint8_t* cwb_out,
                           uint8_t* s0s_out, size_t max_s0s, size_t* num_s0s) {
  if (!in || !cwb_out || !num_s0s) return fail(DCF_ERR_ARG, "null argument");
  if (n_bytes == 0) return fail(DCF_ERR_N, "n_bytes must be > 0");
  if (lambda == 0 || lambda % 16) return fail(DCF_ERR_LAMBDA, "lambda must be a positive multiple of 16");
  const size_t n = 8 * n_bytes;
  size_t pos = 0;
  auto u64 = [&](uint64_t* v) {
    if (in_len - pos < 8) return false;
    *v = 0;
    for (int i = 0; i < 8; i++) *v |= (uint64_t)in[pos + i] << (8 * i);
    pos += 8;
    return true;
  };
  auto arr = [&](uint8_t* dst) {  // Vec<u8> that must hold exactly lambda bytes (copy_from_slice, lib.rs:251)
    uint64_t len;
    if (!u64(&len) || len != lambda || in_len - pos < lambda) return false;
    if (dst) memcpy(dst, in + pos, lambda);
    pos += lambda;
    return true;
  };
  uint64_t ns;
  if (!u64(&ns)) return fail(DCF_ERR_KEY, "truncated Share (s0s length)");
  if (ns > max_s0s && s0s_out) return fail(DCF_ERR_LEN, "more seeds than s0s_out holds");
  for (uint64_t i = 0; i < ns; i++)
    if (!arr(s0s_out ? s0s_out + i * lambda : nullptr)) return fail(DCF_ERR_KEY, "bad seed in s0s");
  uint64_t ncw;
  if (!u64(&ncw)) return fail(DCF_ERR_KEY, "truncated Share (cws length)");
  if (ncw != n) return fail(DCF_ERR_KEY, "cws.len() != N * 8 (lib.rs:165)");
  memset(cwb_out, 0, dcf_cwb_bytes(n_bytes, lambda, 1));
  for (size_t i = 0; i < n; i++) {
    if (!arr(cwb_out + i * lambda) || !arr(cwb_out + (n + i) * lambda)) return fail(DCF_ERR_KEY, "bad Cw.s / Cw.v");
    if (in_len - pos < 2 || in[pos] > 1 || in[pos + 1] > 1) return fail(DCF_ERR_KEY, "bad Cw bool (bincode bool is 0/1)");
    cwb_out[2 * n * lambda + i] = (uint8_t)(in[pos] | (in[pos + 1] << 1));
    pos += 2;
  }
  if (!arr(cwb_out + dcf_cwb_np1_offset(n_bytes, lambda, 1))) return fail(DCF_ERR_KEY, "bad cw_np1");
  if (pos != in_len) return fail(DCF_ERR_KEY, "trailing bytes after Share");
  *num_s0s = (size_t)ns;
  return DCF_OK;
}

// ---- contiguous-range eval (kernels_range.h; DESIGN.md "Range eval") ----

constexpr uint64_t kRangeChunk = 1ull << 22;  // points per pass of the materialising path

// The introspection exports: fields of a plan (the heights and the Tree16 groups do not depend on the
// PRG; the Wide ones are those of the Hirose PRG at `lambda`, 0 for a shape that engine does not take).
int dcf_eval_range_subtree_levels(size_t n_bytes, uint64_t count) {
  return n_bytes ? (int)plan_range(0, 16, n_bytes, 1, count, RangeRule::OneKey).h : 0;
}

uint64_t dcf_eval_range_wide_points_per_launch(size_t n_bytes, size_t lambda) {
  if (!n_bytes) return 0;
  const RangePlan pl = plan_range(0, lambda, n_bytes, 1, 1, RangeRule::OneKey);
  return pl.engine == RangeEngine::Wide ? pl.per : 0;
}

int dcf_eval_range_multikey_subtree_levels(size_t n_bytes, size_t num_keys, uint64_t count) {
  return n_bytes && num_keys ? (int)plan_range(0, 16, n_bytes, num_keys, count, RangeRule::MultiKey).h : 0;
}

size_t dcf_eval_range_keys_per_launch(size_t n_bytes, size_t num_keys, uint64_t count) {
  if (!n_bytes || !count) return 1;
  return (size_t)plan_range(0, 16, n_bytes, num_keys ? num_keys : 1, count, RangeRule::MultiKey).keys;
}

int dcf_eval_range_wide_multikey_subtree_levels(size_t n_bytes, size_t num_keys, uint64_t count) {
  if (!n_bytes || !num_keys || !count) return 0;
  const RangePlan pl = plan_range(0, 32, n_bytes, num_keys, count, RangeRule::MultiKey);
  return pl.engine == RangeEngine::Wide ? (int)pl.h : 0;
}

size_t dcf_eval_range_wide_keys_per_launch(size_t n_bytes, size_t lambda, size_t num_keys, uint64_t count) {
  if (!n_bytes || !num_keys || !count) return 0;
  const RangePlan pl = plan_range(0, lambda, n_bytes, num_keys, count, RangeRule::MultiKey);
  return pl.engine == RangeEngine::Wide ? (size_t)pl.keys : 0;
}

// x0 as the kernels take it: the low 16 bytes as a 128-bit value and the bytes above them.  Points
// [0, first) of the range have top bytes `top`; the rest (only when the low 128 bits wrap, N > 16)
// have `top1` = top + 1 and low bits counted from zero.
struct RangeArg {
  RangeX x;
  RangeTop top, top1;
  uint64_t first;
};

static int range_parse(size_t nb, const uint8_t* x0, uint64_t count, RangeArg* A) {  // (nb <= 256: RangeCall::check)
  const size_t low = std::min<size_t>(nb, 16), nt = nb - low;
  memset(A, 0, sizeof(*A));
  memcpy(A->top.b, x0, nt);
  for (size_t b = 0; b < low; ++b) {
    const size_t pos = low - 1 - b;
    const uint64_t v = x0[nt + b];
    if (pos < 8) A->x.lo |= v << (8 * pos);
    else A->x.hi |= v << (8 * (pos - 8));
  }
  A->first = count;
  const RangeX last = range_add(A->x, count - 1);
  const bool wrapped = last.hi < A->x.hi || (last.hi == A->x.hi && last.lo < A->x.lo);
  const size_t bits = 8 * nb;
  const bool fits = bits >= 128 || (bits <= 64 ? (last.hi == 0 && (bits == 64 || (last.lo >> bits) == 0))
                                                : (last.hi >> (bits - 64)) == 0);
  if (!fits || (wrapped && nt == 0)) return fail(DCF_ERR_ARG, "x0 + count exceeds 2^(8N)");
  if (wrapped) {  // N > 16: the top bytes step once, after 2^128 - x (x.hi is all ones here)
    A->top1 = A->top;
    size_t b = nt;
    while (b > 0 && ++A->top1.b[b - 1] == 0) --b;
    if (b == 0) return fail(DCF_ERR_ARG, "x0 + count exceeds 2^(8N)");
    A->first = 0 - A->x.lo;
  }
  return DCF_OK;
}

// What every range entry point does ahead of its own work, in two steps with the entry's own
// early-outs between them.  check(): the arguments (as check_eval_args; the prg is not looked into,
// and ys / out may be null when there is nothing to write, so the callers look at them after their
// counts).  open(): x0 parsed (count > 0), the prg's device, and a workspace leased and ordered on
// `stream` — host: on its own compute stream; once L is set the caller ends with host_finish.
struct RangeCall {
  RangeArg A;
  std::optional<DeviceGuard> dg;
  std::optional<Lease> L;
  static int check(dcf_prg* p, size_t n_bytes, int party, const void* cwb, const void* s0s, const void* x0) {
    if (!p) return fail(DCF_ERR_ARG, "null prg");
    if (n_bytes == 0) return fail(DCF_ERR_N, "n_bytes must be > 0");
    if (party != 0 && party != 1) return fail(DCF_ERR_ARG, "party must be 0 or 1");
    if (!cwb || !s0s || !x0) return fail(DCF_ERR_ARG, "null argument");
    if (n_bytes > 16 + kRangeTopMax) return fail(DCF_ERR_UNSUPPORTED, "range eval: N <= 256");
    return DCF_OK;
  }
  int open(dcf_prg* p, size_t n_bytes, const uint8_t* x0, uint64_t count, void* stream, bool host = false) {
    if (count)
      if (int rc = range_parse(n_bytes, x0, count, &A)) return rc;
    dg.emplace(p->device);
    if (host && !dg->ok) return fail(DCF_ERR_HIP, "hipSetDevice failed");
    L.emplace(p);
    return host ? host_lease(*L) : L->order((hipStream_t)stream);
  }
};

// Points [off, off + cnt) of the range as N-byte strings at xs.
static int range_points(const RangeArg& A, size_t nb, uint64_t off, uint64_t cnt, uint8_t* xs, hipStream_t st) {
  for (uint64_t done = 0; done < cnt;) {
    const uint64_t i = off + done;
    const bool hi = i >= A.first;
    const uint64_t n = hi ? cnt - done : std::min<uint64_t>(cnt - done, A.first - i);
    const RangeX x = hi ? RangeX{i - A.first, 0} : range_add(A.x, i);
    hipLaunchKernelGGL(k_range_points, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, st,
                       (uint32_t)nb, x, hi ? A.top1 : A.top, n, xs + done * nb);
    HIP_TRY(hipGetLastError());
    done += n;
  }
  return DCF_OK;
}

// The blocks of 2^h leaves (h >= 1) that cover the n points from xa: the range starts `skip` leaves
// into the first, whose root has the (8N - h)-bit prefix pfx; nroots <= (n >> h) + 2 of them, with
// m breadth-first levels between a root and the `tail` levels of the register tail.
struct RangeGeom {
  uint64_t skip, nroots;
  RangeX pfx;
  uint32_t m;
};
static RangeGeom range_geom(const RangeX xa, uint64_t n, uint32_t h, uint32_t tail) {
  const uint64_t skip = xa.lo & ((1ull << h) - 1);
  return {skip, ((skip + n - 1) >> h) + 1, RangeX{(xa.lo >> h) | (xa.hi << (64 - h)), xa.hi >> h}, h - tail};
}

// What a tree-path call does ahead of its launch groups and after them: the workspace of ws_bytes
// (0: none), the block count zeroed (zero_blocks: first part of a call), phase mark 0 — the caller
// sets mark 1 after what it builds once per call — and mark 2 at the end.
static int range_begin(dcf_prg* p, Lease& L, size_t ws_bytes, bool zero_blocks) {
  Workspace* w = L.w;
  if (int rc = ensure_ctr(w)) return rc;
  if (ws_bytes)
    if (int rc = ensure_ws(w, ws_bytes, L.st)) return rc;
  if (zero_blocks) HIP_TRY(hipMemsetAsync(w->d_ctr, 0, kCtrBytes, L.st));
  w->last_prefix = 0;
  phase_mark(p, L, 0);
  return DCF_OK;
}
static int range_end(dcf_prg* p, Lease& L) {
  phase_mark(p, L, 2);
  p->last_ws.store(L.w);
  return DCF_OK;
}

// One launch group of the tree path (lambda = 16, N <= 16): keys [key0, key0 + keys) of a K-key
// block over the n <= 2^28 points from xa, keys * n <= 2^28; the outputs of key key0 + k go to rows
// [k * n, (k + 1) * n) of ys (several keys in a group: n is the call's count).  PRG: the prg's PRG
// policy, RangeHirose or RangeMmo.  KP: the kernels' key policy — RangeOneKey takes key0 = 0,
// keys = K = 1.  The caller has sized the workspace (RangePlan::tree_ws) and zeroed the block count.
// OUT: the tail's output policy; under RangeFold (h > 0 only) ys is row key0 of the call's `out`,
// 16 bytes per key, zeroed by the caller, and op holds the group's rows of the table.
extern "C++" template <class PRG, class KP, class OUT>
static int range_group(dcf_prg* p, Lease& L, const KeyBlock& kb, int party, const uint8_t* s0s, uint64_t key0,
                       uint64_t keys, const RangeX xa, uint64_t n, uint32_t h, size_t buf_bytes, uint8_t* ys,
                       const OUT op) {
  using Idx = typename KP::Idx;
  hipStream_t st = L.st;
  Workspace* w = L.w;
  const uint32_t nlev = kb.nlev;
  const size_t K = kb.K;
  const KeyBlock g0 = kb.from(key0);  // the group's first key
  const uint4 *cws = g0.s4(), *cwv = g0.v4(), *np1 = g0.np14();
  const uint8_t* cwt = g0.cwt;
  const uint4* s0 = (const uint4*)s0s + key0;
  unsigned long long* blocks = reinterpret_cast<unsigned long long*>(w->d_ctr) + 1;
  const typename PRG::Arg rk = PRG::arg(p);
  const auto roots_grid = [&](uint64_t total) {
    return dim3((unsigned)std::min<uint64_t>((uint64_t)p->cus, (total + PRG::kRootsPer - 1) / PRG::kRootsPer));
  };
  if (h == 0) {  // every point is its own root: the root walk writes y
    if (OUT::kFold) return fail(DCF_ERR_ARG, "range fold: the root walk has no fold");
    const uint64_t total = keys * n;
    hipLaunchKernelGGL((PRG::template roots<true, KP>()), roots_grid(total), dim3(kBlock), 0, st, p->d_tab, rk, cws, cwv,
                       cwt, np1, s0, KP::make(K, (uint32_t)n), (uint32_t)party, xa, nlev, (Idx)total, (uint4*)ys, blocks);
    HIP_TRY(hipGetLastError());
    return DCF_OK;
  }
  const RangeGeom g = range_geom(xa, n, h, kFdTail);
  uint32_t* ctrs = (uint32_t*)(w->d_ws + 2 * buf_bytes);
  uint4* cur = (uint4*)w->d_ws;
  uint4* nxt = (uint4*)(w->d_ws + buf_bytes);
  HIP_TRY(hipMemsetAsync(ctrs, 0, kRangeCtrs * sizeof(uint32_t), st));
  const uint64_t total = keys * g.nroots;
  hipLaunchKernelGGL((PRG::template roots<false, KP>()), roots_grid(total), dim3(kBlock), 0, st, p->d_tab, rk, cws, cwv,
                     cwt, np1, s0, KP::make(K, (uint32_t)g.nroots), (uint32_t)party, g.pfx, nlev - h, (Idx)total, cur,
                     blocks);
  HIP_TRY(hipGetLastError());
  for (uint32_t k = 0; k < g.m; ++k) {  // level 8N - h + k: nroots << k parents per key
    const uint64_t parents = total << k;
    hipLaunchKernelGGL((k_range_level16<PRG, KP>), dim3((unsigned)grid_for(parents, p->cus)), dim3(kBlock), 0, st,
                       p->d_tab, rk, cws, cwv, cwt, KP::make(K, (uint32_t)(g.nroots << k)), nlev - h + k,
                       (uint32_t)parents, (const uint4*)cur, nxt, ctrs + k, blocks);
    HIP_TRY(hipGetLastError());
    std::swap(cur, nxt);
  }
  const uint64_t nnodes = total << g.m;
  hipLaunchKernelGGL((k_range_tail16<(int)kFdTail, PRG, KP, OUT>), dim3((unsigned)grid_for(nnodes, p->cus)), dim3(kBlock),
                     0, st, p->d_tab, rk, cws, cwv, cwt, np1, KP::make(K, (uint32_t)(g.nroots << g.m)), nlev - kFdTail,
                     (uint32_t)nnodes, (const uint4*)cur, (uint32_t)g.skip, (uint32_t)n, (uint4*)ys,
                     ctrs + kRangeCtrs - 1, blocks, op);
  HIP_TRY(hipGetLastError());
  return DCF_OK;
}

// ---- range eval over the Hirose PRG at lambda >= 32 (kernels_range_wide.h; DESIGN.md "Range eval, λ ≥ 32") ----

// One launch group: keys [key0, key0 + keys) of a K-key block over the n points from xa; the outputs
// of key key0 + k go to rows [k * n, (k + 1) * n) of ys (several keys in a group: n is the call's
// count).  MASK: lambda = 32, the kernels' form without t-vectors.  KP: the kernels' key policy —
// RangeOneKey takes keys = 1 (any key0 of any K: the key is read in place).  The caller has sized
// the workspace (RangePlan::wide_ws), built the CW digest of the group's keys (dig_t behind its
// keys * 8N * 64 bytes) and zeroed the block count.
extern "C++" template <bool MASK, class KP>
static int range_wide_group(dcf_prg* p, Lease& L, const KeyBlock& kb, int party, const uint8_t* s0s, uint64_t key0,
                            uint64_t keys, const RangeX xa, uint64_t n, uint32_t h, const RangeWideWs& ws, uint8_t* ys) {
  hipStream_t st = L.st;
  Workspace* w = L.w;
  const uint32_t lam = kb.lam, nlev = kb.nlev;
  const uint4* np1k = kb.from(key0).np14();  // the group's first key
  const uint8_t* s0 = s0s + key0 * lam;
  const uint4* dig = (const uint4*)w->d_dig;
  const uint8_t* dig_t = w->d_dig + (size_t)keys * nlev * 64;
  unsigned long long* blocks = reinterpret_cast<unsigned long long*>(w->d_ctr) + 1;
  uint32_t* tvec = MASK ? nullptr : reinterpret_cast<uint32_t*>(w->d_ws);
  const auto roots_grid = [&](uint64_t roots) { return dim3((unsigned)std::min<uint64_t>((uint64_t)p->cus, (roots + 63) / 64)); };
  if (h == 0) {  // every point is its own root: the root walk writes y[0:32) and the t-vector
    const uint64_t total = keys * n;
    hipLaunchKernelGGL((k_range_roots_wide<true, MASK, KP>), roots_grid(total), dim3(kBlock), 0, st, p->d_tab, p->d_rk2, dig,
                       dig_t, np1k, (const uint4*)s0, KP::make(nlev, (uint32_t)n), (uint32_t)party, xa, nlev, (uint32_t)total,
                       (uint4*)nullptr, tvec, ys, lam, blocks);
    HIP_TRY(hipGetLastError());
  } else {
    constexpr uint32_t tail = KP::kPerLane ? kRangeWideTailKeys : kRangeWideTail;  // register depth of the tail
    const RangeGeom g = range_geom(xa, n, h, tail);
    const uint32_t w0 = (nlev - h + 1) >> 4;  // the t-vector word of the first row below the roots
    uint4* cur = (uint4*)(w->d_ws + ws.tv);
    uint4* nxt = (uint4*)(w->d_ws + ws.tv + ws.buf);
    uint32_t* tpre = MASK ? nullptr : (uint32_t*)(w->d_ws + ws.tv + 2 * ws.buf);
    uint32_t* ctrs = (uint32_t*)(w->d_ws + ws.tv + 2 * ws.buf + ws.pre);
    HIP_TRY(hipMemsetAsync(ctrs, 0, kRangeCtrs * sizeof(uint32_t), st));
    const uint64_t total = keys * g.nroots;
    hipLaunchKernelGGL((k_range_roots_wide<false, MASK, KP>), roots_grid(total), dim3(kBlock), 0, st, p->d_tab, p->d_rk2, dig,
                       dig_t, np1k, (const uint4*)s0, KP::make(nlev, (uint32_t)g.nroots), (uint32_t)party, g.pfx, nlev - h,
                       (uint32_t)total, cur, tpre, (uint8_t*)nullptr, lam, blocks);
    HIP_TRY(hipGetLastError());
    for (uint32_t k = 0; k < g.m; ++k) {  // level 8N - h + k: nroots << k parents per key
      const uint64_t parents = total << k;
      hipLaunchKernelGGL((k_range_level_wide<MASK, KP>), dim3((unsigned)grid_for(parents, p->cus)), dim3(kBlock), 0, st,
                         p->d_tab, p->d_rk2, dig, dig_t, KP::make(nlev, (uint32_t)(g.nroots << k)), nlev - h + k, w0,
                         (uint32_t)parents, (const uint4*)cur, nxt, ctrs + k, blocks);
      HIP_TRY(hipGetLastError());
      std::swap(cur, nxt);
    }
    const uint64_t nnodes = total << g.m;
    const uint32_t nq = ((nlev >> 4) + 1 + 3) / 4;  // uint4s holding rows 0 .. 8N of a t-vector
    hipLaunchKernelGGL((k_range_tail_wide<(int)tail, MASK, KP>), dim3((unsigned)grid_for(nnodes, p->cus)),
                       dim3(kBlock), 0, st, p->d_tab, p->d_rk2, dig, dig_t, np1k, KP::make(nlev, (uint32_t)(g.nroots << g.m)),
                       nlev - tail, w0, (uint32_t)nnodes, (const uint4*)cur, (uint32_t)g.skip, (uint32_t)n, ys, lam,
                       (uint4*)tvec, (const uint4*)tpre, g.m, nq, ctrs + kRangeCtrs - 1, blocks);
    HIP_TRY(hipGetLastError());
  }
  if (!MASK)  // y[32, lambda) from the t-vectors (the existing tail kernels)
    return run_tail(WideTail{kb, key0, s0, tvec, keys * n, n, ys, party, st, p->cus, w});
  return DCF_OK;
}

// ---- the drivers: a plan over keys [key0, key0 + nkeys) of a K-key block, points [off, off + cnt) of
// the range, one function per engine; a single key is the K = 1 case (DESIGN.md "Range eval") ----

// Tree16, on L.st: launch groups of pl.gkeys whole keys, or the keys one after another in groups of
// 2^28 outputs.  RangeStore: into ys, the output of point `off` of key key0.  RangeFold (pl.fused):
// ys is row key0 of the call's `out`, 16 bytes per key, zeroed by the caller — the groups of one key
// fold into the same row — and op holds the table from point `off`.
extern "C++" template <class OUT>
static int range_tree(dcf_prg* p, Lease& L, const RangePlan& pl, size_t nb, size_t K, uint64_t key0, uint64_t nkeys,
                      int party, const uint8_t* cwb, const uint8_t* s0s, const RangeArg& A, uint64_t off, uint64_t cnt,
                      uint8_t* ys, bool zero_blocks, const OUT op) {
  size_t buf_bytes;
  const size_t ws = pl.tree_ws(cnt, &buf_bytes);
  if (int rc = range_begin(p, L, ws, zero_blocks)) return rc;
  phase_mark(p, L, 1);
  const bool mmo = p->kind != 0;
  const auto group =
      pl.per_lane ? (mmo ? range_group<RangeMmo, RangeKeys, OUT> : range_group<RangeHirose, RangeKeys, OUT>)
                  : (mmo ? range_group<RangeMmo, RangeOneKey, OUT> : range_group<RangeHirose, RangeOneKey, OUT>);
  const uint64_t row = OUT::kFold ? 1 : cnt;  // rows of ys per key
  const KeyBlock kb(cwb, nb, p->lambda, K);
  for (uint64_t k0 = key0; k0 < key0 + nkeys; k0 += pl.gkeys) {
    const uint64_t nk = std::min<uint64_t>(pl.gkeys, key0 + nkeys - k0);
    for (uint64_t o = 0; o < cnt; o += pl.per) {  // several keys to a group, or h = 0: cnt <= per, one pass
      const uint64_t n = std::min<uint64_t>(pl.per, cnt - o);
      if (int rc = group(p, L, kb, party, s0s, k0, nk, range_add(A.x, off + o), n, pl.h, buf_bytes,
                         ys + ((k0 - key0) * row + (OUT::kFold ? 0 : o)) * 16, op.at(o)))
        return rc;
    }
  }
  return range_end(p, L);
}

// Wide, on L.st: launch groups of pl.gkeys whole keys under the per-lane key policy, or the keys one
// after another through the single-key kernels, each read in place from the K-key block, pl.per
// outputs to a group.  No materialised points, no gather, no buffer of the call's own, no stream wait.
static int range_wide(dcf_prg* p, Lease& L, const RangePlan& pl, size_t nb, size_t K, uint64_t key0, uint64_t nkeys,
                      int party, const uint8_t* cwb, const uint8_t* s0s, const RangeArg& A, uint64_t off, uint64_t cnt,
                      uint8_t* ys, bool zero_blocks) {
  hipStream_t st = L.st;
  Workspace* w = L.w;
  const uint32_t lam = (uint32_t)p->lambda;
  const KeyBlock kb(cwb, nb, lam, K);
  const RangeWideWs ws = pl.wide_ws(cnt);
  if (int rc = ensure_dig(w, pl.gkeys * kb.nlev, st)) return rc;
  if (int rc = range_begin(p, L, ws.total, zero_blocks)) return rc;
  const bool once = nkeys == 1;  // a call's only key: its digest is built once, ahead of mark 1
  if (once)
    if (int rc = launch_digest(w, kb, key0, 1, st)) return rc;
  phase_mark(p, L, 1);
  const auto group =
      pl.per_lane ? (lam == 32 ? range_wide_group<true, RangeDigKeys> : range_wide_group<false, RangeDigKeys>)
                  : (lam == 32 ? range_wide_group<true, RangeOneKey> : range_wide_group<false, RangeOneKey>);
  for (uint64_t k0 = key0; k0 < key0 + nkeys; k0 += pl.gkeys) {
    const uint64_t nk = std::min<uint64_t>(pl.gkeys, key0 + nkeys - k0);
    if (!once)
      if (int rc = launch_digest(w, kb, k0, nk, st)) return rc;
    for (uint64_t o = 0; o < cnt; o += pl.per) {  // several keys to a group, or h = 0: cnt <= per, one pass
      const uint64_t n = std::min<uint64_t>(pl.per, cnt - o);
      if (int rc = group(p, L, kb, party, s0s, k0, nk, range_add(A.x, off + o), n, pl.h, ws,
                         ys + ((k0 - key0) * cnt + o) * lam))
        return rc;
    }
  }
  return range_end(p, L);
}

// Key k of a K-key block into the single-key layout: the key at dk, its s0 at ds0 (the caller has
// zeroed the key's padding).
static int range_gather(dcf_prg* p, Lease& L, size_t nb, size_t K, uint64_t k, const uint8_t* cwb, const uint8_t* s0s,
                        uint8_t* dk, uint8_t* ds0) {
  const KeyBlock src(cwb, nb, p->lambda, K), dst(dk, nb, p->lambda, 1);
  hipLaunchKernelGGL(k_rangemk_gather, dim3(8), dim3(256), 0, L.st, cwb, src.np1, s0s, src.K, k, src.nlev, src.lam,
                     (uint32_t)(dst.np1 - dk), dk, ds0);
  HIP_TRY(hipGetLastError());
  return DCF_OK;
}

// Points (no tree-sharing path): key by key, the points materialised kRangeChunk at a time and run
// through eval.  One key is read in place; a key of a K-key block is gathered into the single-key
// layout first.  eval owns the workspace, so the points and the gathered key get buffers of the
// call's own, freed on return.
static int range_materialise(dcf_prg* p, Lease& L, size_t nb, size_t K, uint64_t key0, uint64_t nkeys, int party,
                             const uint8_t* cwb, const uint8_t* s0s, const RangeArg& A, uint64_t off, uint64_t cnt,
                             uint8_t* ys) {
  hipStream_t st = L.st;
  const size_t lam = p->lambda, kb = align256(dcf_cwb_bytes(nb, lam, 1));
  DevBuf xs, key;
  const uint64_t chunk = std::min<uint64_t>(cnt, kRangeChunk);
  HIP_TRY(xs.alloc(chunk * nb));
  uint8_t* dk = nullptr;
  if (K > 1) {
    HIP_TRY(key.alloc(kb + lam));
    dk = (uint8_t*)key.p;
    HIP_TRY(hipMemsetAsync(dk, 0, kb + lam, st));
  }
  for (uint64_t k = key0; k < key0 + nkeys; ++k) {
    if (dk)
      if (int rc = range_gather(p, L, nb, K, k, cwb, s0s, dk, dk + kb)) return rc;
    for (uint64_t o = 0; o < cnt; o += chunk) {
      const uint64_t n = std::min<uint64_t>(chunk, cnt - o);
      if (int rc = range_points(A, nb, off + o, n, (uint8_t*)xs.p, st)) return rc;
      if (int rc = eval_launch(p, L, nb, 1, n, party, dk ? dk : cwb, dk ? dk + kb : s0s, (const uint8_t*)xs.p,
                               ys + ((k - key0) * cnt + o) * lam))
        return rc;
    }
  }
  HIP_TRY(hipStreamSynchronize(st));  // xs and key are freed on return
  return DCF_OK;
}

// The plan over keys [key0, key0 + nkeys) of the K-key block at cwb / s0s — no more keys than it was
// made for — and points [off, off + cnt) of the range, on L.st: into ys, the output of point `off`
// of key key0 (RangeFold: see range_tree).  A point sub-range takes one key.  zero_blocks: first
// part of a call.
extern "C++" template <class OUT>
static int range_run(dcf_prg* p, Lease& L, const RangePlan& pl, size_t nb, size_t K, uint64_t key0, uint64_t nkeys,
                     int party, const uint8_t* cwb, const uint8_t* s0s, const RangeArg& A, uint64_t off, uint64_t cnt,
                     uint8_t* ys, bool zero_blocks, const OUT op) {
  if ((off != 0 || cnt != pl.count) && nkeys != 1)
    return fail(DCF_ERR_ARG, "range eval: a point sub-range takes one key");
  if (OUT::kFold && !pl.fused) return fail(DCF_ERR_ARG, "range fold: the shape has no folding tail");
  switch (pl.engine) {
    case RangeEngine::Tree16:
      return range_tree(p, L, pl, nb, K, key0, nkeys, party, cwb, s0s, A, off, cnt, ys, zero_blocks, op);
    case RangeEngine::Wide:
      return range_wide(p, L, pl, nb, K, key0, nkeys, party, cwb, s0s, A, off, cnt, ys, zero_blocks);
    case RangeEngine::Points:
      return range_materialise(p, L, nb, K, key0, nkeys, party, cwb, s0s, A, off, cnt, ys);
  }
  return fail(DCF_ERR_ARG, "range eval: no engine");
}

int dcf_eval_range_device(dcf_prg* p, size_t n_bytes, int party, const uint8_t* cwb, const uint8_t* s0,
                          const uint8_t* x0, uint64_t count, uint8_t* ys, void* stream) {
  if (int rc = RangeCall::check(p, n_bytes, party, cwb, s0, x0)) return rc;
  if (count == 0) return DCF_OK;
  if (!ys) return fail(DCF_ERR_ARG, "null buffer");
  RangeCall c;
  if (int rc = c.open(p, n_bytes, x0, count, stream)) return rc;
  const RangePlan pl = plan_range(p->kind, p->lambda, n_bytes, 1, count, RangeRule::OneKey);
  return range_run(p, *c.L, pl, n_bytes, 1, 0, 1, party, cwb, s0, c.A, 0, count, ys, true, RangeStore{});
}

// Full domain over the MMO PRG at LAMBDA = 16: the root, then 8N breadth-first level launches
// (k_fd_level16_mmo) between two SoA node buffers in d_ws — s (16 B), v (16 B), t (1 B) per node,
// the widest level held 2^(8N - 1) — the last of which writes y.  The one user of that node format:
// kept because the range route (16 launch groups with a register tail at N = 4) measured 204.0 ms
// against these launches' 192.0 (profiles/r17).
static int full_domain_mmo16(dcf_prg* p, Lease& L, size_t n_bytes, int party, const uint8_t* cwb, const uint8_t* s0,
                             uint8_t* ys) {
  hipStream_t st = L.st;
  const uint32_t nlev = (uint32_t)(8 * n_bytes);
  const size_t nodeb = 33;
  const uint64_t maxnodes = (1ull << nlev) / 2;
  const KeyBlock kb(cwb, n_bytes, 16, 1);
  // + one work counter per launch (64-node units, see next_wave_base) after the nodes
  const size_t ctr_off = (2 * maxnodes * nodeb + 64 + 255) & ~(size_t)255;
  if (int rc = ensure_ws(L.w, ctr_off + 64 * sizeof(uint32_t), st)) return rc;
  uint8_t* w = L.w->d_ws;
  uint32_t* ctrs = (uint32_t*)(w + ctr_off);
  HIP_TRY(hipMemsetAsync(ctrs, 0, 64 * sizeof(uint32_t), st));
  uint4* s_a = (uint4*)w;
  uint4* v_a = s_a + maxnodes;
  uint8_t* t_a = (uint8_t*)(v_a + maxnodes);
  uint4* s_b = (uint4*)(w + maxnodes * nodeb + 16 - (maxnodes * nodeb) % 16);
  uint4* v_b = s_b + maxnodes;
  uint8_t* t_b = (uint8_t*)(v_b + maxnodes);
  hipLaunchKernelGGL(k_fd_root16, dim3(1), dim3(64), 0, st, (const uint4*)s0, (uint32_t)party, s_a, v_a, t_a);
  HIP_TRY(hipGetLastError());
  for (uint32_t lev = 0; lev < nlev; ++lev) {
    const uint64_t parents = 1ull << lev;
    hipLaunchKernelGGL(k_fd_level16_mmo, dim3((unsigned)grid_for(parents, p->cus)), dim3(kBlock), 0, st, p->d_tab,
                       p->d_rk128, kb.s4(), kb.v4(), kb.cwt, kb.np14(), lev, nlev, parents, s_a, v_a, t_a, s_b, v_b, t_b,
                       (uint4*)ys, ctrs + lev);
    HIP_TRY(hipGetLastError());
    std::swap(s_a, s_b);
    std::swap(v_a, v_b);
    std::swap(t_a, t_b);
  }
  return DCF_OK;
}

// The whole domain is the range [0, 2^(8N)), and but for two shapes full-domain eval is that range
// call.  Hirose, LAMBDA = 16, from N = 2: levels 0 .. 8N - kFdTail - 1 in ONE launch of the
// shared-prefix table build (k_prefix_build16: workgroup subtrees, no level launches), then the
// register depth-first tail on its rows (k_fd_dfs16), which the range driver's root walk and level
// launches do not match (DESIGN.md "Range eval": 1.26x at N = 4); when its table cannot be
// allocated, it is a range call as well.  MMO, LAMBDA = 16: full_domain_mmo16.
int dcf_eval_full_domain_device(dcf_prg* p, size_t n_bytes, int party, const uint8_t* cwb, const uint8_t* s0,
                                uint8_t* ys, void* stream) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  if (n_bytes == 0) return fail(DCF_ERR_N, "n_bytes must be > 0");
  if (n_bytes > 4) return fail(DCF_ERR_UNSUPPORTED, "full-domain eval: N <= 4 (2^32 outputs)");
  if (party != 0 && party != 1) return fail(DCF_ERR_ARG, "party must be 0 or 1");
  if (!cwb || !s0 || !ys) return fail(DCF_ERR_ARG, "null buffer");
  DeviceGuard dg(p->device);
  Lease L(p);
  if (int rc = L.order((hipStream_t)stream)) return rc;
  hipStream_t st = L.st;
  const uint32_t nlev = (uint32_t)(8 * n_bytes);
  const size_t lam = p->lambda;
  if (p->kind == 0 && lam == 16 && nlev >= kFdTail + 12) {
    const uint32_t lev_end = nlev - kFdTail;
    const KeyBlock kb(cwb, n_bytes, lam, 1);
    PrefixTable pf{nullptr, 0u};
    const int brc = build_prefix(p, L.w, party, kb, s0, lev_end, &pf, st);
    if (brc != DCF_OK && brc != kPrefixNoMem) return brc;
    if (brc == DCF_OK) {
      const uint64_t nodes = 1ull << lev_end;
      if (int rc2 = ensure_ctr(L.w)) return rc2;
      HIP_TRY(hipMemsetAsync(L.w->d_ctr, 0, kCtrBytes, st));
      hipLaunchKernelGGL(k_fd_dfs16<kFdTail>, dim3((unsigned)grid_for(nodes, p->cus)), dim3(kBlock), 0, st, p->d_tab,
                         p->rk[0], kb.s4(), kb.v4(), kb.cwt, kb.np14(), lev_end, nodes, pf.sv, (uint4*)ys, L.w->d_ctr);
      HIP_TRY(hipGetLastError());
      return DCF_OK;
    }
  }
  if (p->kind == 1 && lam == 16) return full_domain_mmo16(p, L, n_bytes, party, cwb, s0, ys);
  const uint64_t npts = 1ull << nlev;
  RangeArg A{};  // x0 = 0
  A.first = npts;
  const RangePlan pl = plan_range(p->kind, lam, n_bytes, 1, npts, RangeRule::OneKey);
  return range_run(p, L, pl, n_bytes, 1, 0, 1, party, cwb, s0, A, 0, npts, ys, true, RangeStore{});
}

// The range over host buffers: chunks of outputs through the workspace's staging buffers on its
// compute stream, one after the other (the key goes to the device once; one plan, of the whole count).
static int host_range(dcf_prg* p, Lease& L, size_t nb, int party, const uint8_t* cwb, size_t cwb_len,
                      const uint8_t* s0, const RangeArg& A, uint64_t count, uint8_t* ys) {
  Workspace* w = L.w;
  const size_t lam = p->lambda;
  const uint64_t chunk = std::min<uint64_t>(count, std::max<uint64_t>(256, kHostChunkBytes / lam));
  const size_t kb = align256(cwb_len) + align256(lam), yb = align256(chunk * lam);
  if (int rc = ensure_stage(w, yb, kb + yb)) return rc;
  uint8_t* dk = w->d_stage;
  uint8_t* ds0 = dk + align256(cwb_len);
  uint8_t* dy = dk + kb;
  HIP_TRY(hipMemcpyAsync(dk, cwb, cwb_len, hipMemcpyHostToDevice, L.st));
  HIP_TRY(hipMemcpyAsync(ds0, s0, lam, hipMemcpyHostToDevice, L.st));
  const RangePlan pl = plan_range(p->kind, lam, nb, 1, count, RangeRule::OneKey);
  for (uint64_t off = 0; off < count; off += chunk) {
    const uint64_t n = std::min<uint64_t>(chunk, count - off);
    if (int rc = range_run(p, L, pl, nb, 1, 0, 1, party, dk, ds0, A, off, n, dy, off == 0, RangeStore{})) return rc;
    HIP_TRY(hipMemcpyAsync(w->h_stage, dy, n * lam, hipMemcpyDeviceToHost, L.st));
    HIP_TRY(hipStreamSynchronize(L.st));
    memcpy(ys + off * lam, w->h_stage, n * lam);
  }
  return DCF_OK;
}

int dcf_eval_range(dcf_prg* p, size_t n_bytes, int party, const uint8_t* cwb, size_t cwb_len, const uint8_t* s0,
                   const uint8_t* x0, uint64_t count, uint8_t* ys, size_t ys_len) {
  if (int rc = RangeCall::check(p, n_bytes, party, cwb, s0, x0)) return rc;
  if (int rc = check_host_key(false, n_bytes, party, p, cwb_len)) return rc;  // (the key's size: the rest is checked)
  const size_t lam = p->lambda;
  if (ys_len % lam != 0 || ys_len / lam != count) return fail(DCF_ERR_LEN, "ys length != count * lambda");
  if (count == 0) return DCF_OK;
  if (!ys) return fail(DCF_ERR_ARG, "null buffer");
  RangeCall c;
  int rc = c.open(p, n_bytes, x0, count, nullptr, true);
  if (!c.L) return rc;  // failed ahead of the lease
  if (rc == DCF_OK) rc = host_range(p, *c.L, n_bytes, party, cwb, cwb_len, s0, c.A, count, ys);
  return host_finish(*c.L, rc);
}

// K keys over one range (DESIGN.md "Multi-key range eval"): the heights and groups of the multi-key rule.
int dcf_eval_range_multikey_device(dcf_prg* p, size_t n_bytes, size_t num_keys, int party, const uint8_t* cwb,
                                   const uint8_t* s0s, const uint8_t* x0, uint64_t count, uint8_t* ys, void* stream) {
  if (int rc = RangeCall::check(p, n_bytes, party, cwb, s0s, x0)) return rc;
  if (num_keys == 0 || count == 0) return DCF_OK;
  if (!ys) return fail(DCF_ERR_ARG, "null buffer");
  RangeCall c;
  if (int rc = c.open(p, n_bytes, x0, count, stream)) return rc;
  const RangePlan pl = plan_range(p->kind, p->lambda, n_bytes, num_keys, count, RangeRule::MultiKey);
  return range_run(p, *c.L, pl, n_bytes, num_keys, 0, num_keys, party, cwb, s0s, c.A, 0, count, ys, true, RangeStore{});
}

// ---- range fold (kernels_range.h; DESIGN.md "Range fold") ----

constexpr uint64_t kFoldPassRows = 1ull << 22;    // outputs per pass of the row-folding path ...
constexpr uint64_t kFoldPassBytes = 256ull << 20;  // ... and their bytes, whichever is smaller

static uint64_t fold_pass_rows(size_t lam) { return std::max<uint64_t>(1, std::min(kFoldPassRows, kFoldPassBytes / lam)); }

// out[key] ^= XOR_i rows[key * cnt + i] & w[i] for nk keys (k_fold_rows), on st.
static int fold_rows(const dcf_prg* p, const uint8_t* rows, const uint8_t* w, uint64_t nk, uint64_t cnt, uint8_t* out,
                     hipStream_t st) {
  const uint32_t q = (uint32_t)(p->lambda / 16);
  const uint64_t elems = cnt * q;
  // enough threads for one 8-element column walk each, at least one per column, a few waves per CU at most
  const uint64_t gy = std::min<uint64_t>(nk, 65535);
  const uint64_t want = std::max<uint64_t>((elems + 7) / 8, q);
  const uint64_t gx = std::max<uint64_t>(1, std::min<uint64_t>((want + 255) / 256, std::max<uint64_t>(1, 8ull * p->cus / gy)));
  const uint64_t gx_min = ((uint64_t)q + 255) / 256;  // the stride is at least q
  const uint64_t g = std::max(gx, gx_min);
  const uint32_t stride = (uint32_t)(g * 256 / q * q);
  hipLaunchKernelGGL(k_fold_rows, dim3((unsigned)g, (unsigned)gy), dim3(256), 0, st, (const uint4*)rows, (const uint4*)w,
                     (uint32_t)nk, cnt, q, stride, (uint32_t*)out);
  HIP_TRY(hipGetLastError());
  return DCF_OK;
}

// One key without a folding tail (pl: its single-key plan): the range in passes of fold_pass_rows
// outputs into the workspace's fold buffer (behind `reserve` bytes of it that the caller uses), each
// folded into `out` (zeroed by the caller).  zero_blocks: first part of a call.
static int fold_passes(dcf_prg* p, Lease& L, const RangePlan& pl, size_t nb, int party, const uint8_t* cwb,
                       const uint8_t* s0, const RangeArg& A, uint64_t count, const uint8_t* w, uint8_t* out,
                       size_t reserve, bool zero_blocks) {
  const size_t lam = p->lambda;
  const uint64_t pass = std::min<uint64_t>(count, fold_pass_rows(lam));
  uint8_t* ys = L.w->d_fold + reserve;
  for (uint64_t o = 0; o < count; o += pass) {
    const uint64_t n = std::min<uint64_t>(pass, count - o);
    if (int rc = range_run(p, L, pl, nb, 1, 0, 1, party, cwb, s0, A, o, n, ys, zero_blocks && o == 0, RangeStore{}))
      return rc;
    if (int rc = fold_rows(p, ys, w ? w + o * lam : nullptr, 1, n, out, L.st)) return rc;
  }
  return DCF_OK;
}

static int ensure_fold(Workspace* w, size_t bytes, hipStream_t st) { return grow(&w->d_fold, &w->fold_bytes, bytes, st); }

int dcf_eval_range_fold_device(dcf_prg* p, size_t n_bytes, int party, const uint8_t* cwb, const uint8_t* s0,
                               const uint8_t* x0, uint64_t count, const uint8_t* w, uint8_t* out, void* stream) {
  if (int rc = RangeCall::check(p, n_bytes, party, cwb, s0, x0)) return rc;
  if (!out) return fail(DCF_ERR_ARG, "null buffer");
  RangeCall c;
  if (int rc = c.open(p, n_bytes, x0, count, stream)) return rc;
  Lease& L = *c.L;
  const size_t lam = p->lambda;
  HIP_TRY(hipMemsetAsync(out, 0, lam, L.st));
  if (count == 0) return DCF_OK;
  const RangePlan pl = plan_range(p->kind, lam, n_bytes, 1, count, RangeRule::OneKey);
  if (pl.fused)
    return range_run(p, L, pl, n_bytes, 1, 0, 1, party, cwb, s0, c.A, 0, count, out, true, RangeFold{(const uint4*)w});
  if (int rc = ensure_fold(L.w, std::min<uint64_t>(count, fold_pass_rows(lam)) * lam, L.st)) return rc;
  return fold_passes(p, L, pl, n_bytes, party, cwb, s0, c.A, count, w, out, 0, true);
}

int dcf_eval_range_fold_multikey_device(dcf_prg* p, size_t n_bytes, size_t num_keys, int party, const uint8_t* cwb,
                                        const uint8_t* s0s, const uint8_t* x0, uint64_t count, const uint8_t* w,
                                        uint8_t* out, void* stream) {
  if (int rc = RangeCall::check(p, n_bytes, party, cwb, s0s, x0)) return rc;
  if (num_keys == 0) return DCF_OK;
  if (!out) return fail(DCF_ERR_ARG, "null buffer");
  RangeCall c;
  if (int rc = c.open(p, n_bytes, x0, count, stream)) return rc;
  Lease& L = *c.L;
  const RangeArg& A = c.A;
  const size_t lam = p->lambda, K = num_keys;
  HIP_TRY(hipMemsetAsync(out, 0, K * lam, L.st));
  if (count == 0) return DCF_OK;
  const RangePlan all = plan_range(p->kind, lam, n_bytes, K, count, RangeRule::MultiKey);
  if (all.fused)
    return range_run(p, L, all, n_bytes, K, 0, K, party, cwb, s0s, A, 0, count, out, true, RangeFold{(const uint4*)w});
  const uint64_t rows = fold_pass_rows(lam);
  if (count <= rows) {  // passes of whole keys, each planned as a call of its own keys
    const uint64_t per = std::min<uint64_t>(K, rows / count);
    if (int rc = ensure_fold(L.w, per * count * lam, L.st)) return rc;
    for (uint64_t k0 = 0; k0 < K; k0 += per) {
      const uint64_t nk = std::min<uint64_t>(per, K - k0);
      const RangePlan pl = plan_range(p->kind, lam, n_bytes, nk, count, RangeRule::MultiKey);
      if (int rc = range_run(p, L, pl, n_bytes, K, k0, nk, party, cwb, s0s, A, 0, count, L.w->d_fold, k0 == 0, RangeStore{}))
        return rc;
      if (int rc = fold_rows(p, L.w->d_fold, w, nk, count, out + k0 * lam, L.st)) return rc;
    }
    return DCF_OK;
  }
  // a key is more than a pass: key by key, each gathered into the single-key layout ahead of the pass
  const size_t kb = align256(dcf_cwb_bytes(n_bytes, lam, 1)), reserve = kb + align256(lam);
  if (int rc = ensure_fold(L.w, reserve + rows * lam, L.st)) return rc;
  uint8_t* dk = L.w->d_fold;
  HIP_TRY(hipMemsetAsync(dk, 0, reserve, L.st));
  const RangePlan one = plan_range(p->kind, lam, n_bytes, 1, count, RangeRule::OneKey);
  for (uint64_t k = 0; k < K; ++k) {
    if (int rc = range_gather(p, L, n_bytes, K, k, cwb, s0s, dk, dk + kb)) return rc;
    if (int rc = fold_passes(p, L, one, n_bytes, party, dk, dk + kb, A, count, w, out + k * lam, reserve, k == 0)) return rc;
  }
  return DCF_OK;
}

int dcf_gen(dcf_prg* p, size_t n_bytes, const uint8_t* alpha, const uint8_t* beta, const uint8_t* s0_0,
            const uint8_t* s0_1, int bound, uint8_t* cwb_out) {
  if (!p || !alpha || !beta || !s0_0 || !s0_1 || !cwb_out) return fail(DCF_ERR_ARG, "null argument");
  if (n_bytes == 0) return fail(DCF_ERR_N, "n_bytes must be > 0");
  if (bound != DCF_BOUND_LT_BETA && bound != DCF_BOUND_GT_BETA) return fail(DCF_ERR_ARG, "bad bound");
  return host_call(p, [&](Lease& L) { return host_gen(p, L, n_bytes, alpha, beta, s0_0, s0_1, bound, cwb_out); });
}

int dcf_eval(dcf_prg* p, size_t n_bytes, int party, const uint8_t* cwb, size_t cwb_len, const uint8_t* s0,
             const uint8_t* xs, size_t m, uint8_t* ys, size_t ys_len) {
  if (int rc = check_host_key(!p || !cwb || !s0, n_bytes, party, p, cwb_len)) return rc;
  if (ys_len != m * p->lambda) return fail(DCF_ERR_LEN, "ys length != m * lambda");
  if (m == 0) return DCF_OK;
  if (!xs || !ys) return fail(DCF_ERR_ARG, "null buffer");
  return host_call(p, [&](Lease& L) { return host_eval(p, L, n_bytes, party, cwb, cwb_len, s0, xs, m, ys); });
}

int dcf_prg_gen(dcf_prg* p, const uint8_t* seeds, size_t m, uint8_t* out) {
  if (!p) return fail(DCF_ERR_ARG, "null prg");
  if (m == 0) return DCF_OK;
  if (!seeds || !out) return fail(DCF_ERR_ARG, "null buffer");
  return host_call(p, [&](Lease& L) { return host_prg_gen(p, L, seeds, m, out); });
}

// ---- multi-GPU (SURVEY §8(b) dcf_eval_multi_gpu; the reference spreads Dcf::eval over
// every host core inside one call, lib.rs:194-199) ----

static int check_group(dcf_prg* const* prgs, size_t G) {
  if (!prgs || G == 0) return fail(DCF_ERR_ARG, "prgs must hold at least one dcf_prg");
  for (size_t g = 0; g < G; ++g) {
    if (!prgs[g]) return fail(DCF_ERR_ARG, "null dcf_prg in prgs");
    for (size_t h = 0; h < g; ++h)
      if (prgs[h] == prgs[g]) return fail(DCF_ERR_ARG, "a dcf_prg appears twice in prgs (one thread per prg)");
    if (prgs[g]->kind != prgs[0]->kind || prgs[g]->lambda != prgs[0]->lambda ||
        prgs[g]->key_blob != prgs[0]->key_blob)
      return fail(DCF_ERR_ARG, "prgs disagree on the PRG (kind, lambda or keys)");
  }
  return DCF_OK;
}

int dcf_eval_multi_gpu(dcf_prg* const* prgs, size_t G, size_t n_bytes, int party, const uint8_t* cwb,
                       size_t cwb_len, const uint8_t* s0, const uint8_t* xs, size_t m, uint8_t* ys, size_t ys_len) {
  if (int rc = check_group(prgs, G)) return rc;
  if (int rc = check_host_key(!cwb || !s0, n_bytes, party, prgs[0], cwb_len)) return rc;
  const size_t lam = prgs[0]->lambda;
  if (ys_len != m * lam) return fail(DCF_ERR_LEN, "ys length != m * lambda");
  if (m == 0) return DCF_OK;
  if (!xs || !ys) return fail(DCF_ERR_ARG, "null buffer");
  std::vector<int> rcs(G, DCF_OK);
  std::vector<std::string> errs(G);
  auto run = [&](size_t g) {
    size_t start, cnt;
    dcf_point_slice(m, G, g, &start, &cnt);
    if (cnt == 0) return;
    rcs[g] = host_call(prgs[g], [&](Lease& L) {
      return host_eval(prgs[g], L, n_bytes, party, cwb, cwb_len, s0, xs + start * n_bytes, cnt, ys + start * lam);
    });
    if (rcs[g]) errs[g] = t_err;
  };
  std::vector<std::thread> th;
  for (size_t g = 1; g < G; ++g) th.emplace_back(run, g);
  run(0);
  for (auto& t : th) t.join();
  for (size_t g = 0; g < G; ++g)
    if (rcs[g]) return fail(rcs[g], "device slice " + std::to_string(g) + ": " + errs[g]);
  return DCF_OK;
}

int dcf_eval_multi_gpu_device(dcf_prg* const* prgs, size_t G, size_t n_bytes, int party, const uint8_t* cwb,
                              size_t cwb_len, const uint8_t* s0, const uint8_t* const* xs, const size_t* ms,
                              uint8_t* const* ys, void* const* streams, uint8_t* gather_ys) {
  if (int rc = check_group(prgs, G)) return rc;
  if (int rc = check_host_key(!cwb || !s0 || !xs || !ms || !ys, n_bytes, party, prgs[0], cwb_len)) return rc;
  const size_t lam = prgs[0]->lambda;
  const int dev0 = prgs[0]->device;
  size_t off = 0;
  for (size_t g = 0; g < G; ++g) {
    dcf_prg* p = prgs[g];
    DeviceGuard dg(p->device);
    if (!dg.ok) return fail(DCF_ERR_HIP, "hipSetDevice failed");
    Lease L(p);
    if (int rc = L.order(streams ? (hipStream_t)streams[g] : nullptr)) return rc;
    hipStream_t st = L.st;
    Workspace* w = L.w;
    // the key to this device, once per call (4.2 KB at N = LAMBDA = 16): the "broadcast"
    const size_t kb = align256(cwb_len) + align256(lam);
    if (int rc = grow(&w->d_mkey, &w->mkey_bytes, kb, st)) return rc;
    HIP_TRY(hipMemcpyAsync(w->d_mkey, cwb, cwb_len, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w->d_mkey + align256(cwb_len), s0, lam, hipMemcpyHostToDevice, st));
    if (ms[g]) {
      if (!xs[g] || !ys[g]) return fail(DCF_ERR_ARG, "null slice buffer");
      int rc = eval_launch(p, L, n_bytes, 1, ms[g], party, w->d_mkey, w->d_mkey + align256(cwb_len), xs[g], ys[g]);
      if (rc) return rc;
      if (gather_ys) {  // slice g -> its rows of the gather buffer on prgs[0]'s device, over xGMI
        if (p->device != dev0) {
          // direct peer writes when the devices can map each other; hipMemcpyPeerAsync stages the
          // copy itself when they cannot, so a refused peer mapping is not an error
          const hipError_t e = hipDeviceEnablePeerAccess(dev0, 0);
          if (e != hipSuccess) (void)hipGetLastError();
          HIP_TRY(hipMemcpyPeerAsync(gather_ys + off * lam, dev0, ys[g], p->device, ms[g] * lam, st));
        } else {
          HIP_TRY(hipMemcpyAsync(gather_ys + off * lam, ys[g], ms[g] * lam, hipMemcpyDeviceToDevice, st));
        }
      }
    }
    off += ms[g];
  }
  return DCF_OK;
}

#ifdef DCF_CLOCK_STAMPS
// Diagnostic builds only (not in include/dcf_hip.h): the in-kernel clock stamps of slot `slot`
// (0 = k_eval_wide_tail2 main loop, 1 = k_eval_wide_head_stream walk, 2 = k_eval16_stream, 3 = k_eval16_oct,
// 4 = k_eval_wide_tail2 entry (phase 0 only), 5 = k_eval_wide_head_stream entry (phase 0 only)) of the last launch:
// per workgroup {memtime, realtime} at start and end, kClkGroups x 4 u64.
int dcf_debug_clock_stamps(int device, int slot, unsigned long long* out, size_t n) {
  if (!out || slot < 0 || slot >= (int)kClkSlots || n < (size_t)kClkGroups * 4) return fail(DCF_ERR_ARG, "bad argument");
  DeviceGuard dg(device);
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_clk_stamps), (size_t)kClkGroups * 4 * 8,
                              (size_t)slot * kClkGroups * 4 * 8, hipMemcpyDeviceToHost));
  return DCF_OK;
}
int dcf_debug_clock_reset(int device) {
  DeviceGuard dg(device);
  static std::vector<unsigned long long> z((size_t)kClkSlots * kClkGroups * 4, 0);
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_clk_stamps), z.data(), z.size() * 8, 0, hipMemcpyHostToDevice));
  return DCF_OK;
}
#endif

void dcf_point_slice(size_t total, size_t G, size_t g, size_t* start, size_t* count) {
  if (!start || !count) return;
  if (G == 0 || g >= G) {
    *start = total;
    *count = 0;
    return;
  }
  const size_t base = total / G, rem = total % G;
  *start = g * base + (g < rem ? g : rem);
  *count = base + (g < rem ? 1 : 0);
}

}  // extern "C"
