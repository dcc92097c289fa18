/*
 * dcf_hip.h — C ABI of the MI355X (gfx950) DCF evaluator.
 *
 * Drop-in boundary for the hot path of the `dcf` crate (xymeng16/dcf v0.2.2):
 * the `Dcf<N, LAMBDA>` operator (lib.rs:24-35) implemented by `DcfImpl`
 * (lib.rs:63-205) over the `Aes256HirosePrg` plugin (prg.rs:22-74).  Every
 * entry point is plain C: pointers, sizes, int status codes.  A Rust crate binds
 * it with `extern "C"` declarations (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   n_bytes   `N` of `Dcf<N, LAMBDA>` / `CmpFn<N, LAMBDA>` (lib.rs:39): domain
 *             size in bytes; the tree has n = 8 * n_bytes levels (lib.rs:93).
 *   lambda    `LAMBDA` (lib.rs:40): seed and output size in bytes; must be a
 *             multiple of 16 (prg.rs:17-18).
 *   party     `b` of `Dcf::eval` (lib.rs:34): 0 = false, 1 = true.
 *   bound     `BoundState` (lib.rs:342-349): 0 = LtBeta, 1 = GtBeta.
 *   seeds     `Share::s0s` (lib.rs:278).  gen takes both; eval takes the one the
 *             reference reads, `k.s0s[0]` (lib.rs:168), as `s0`.
 *
 * Key layout ("correction-word block", CWB) for K keys, n = 8 * n_bytes
 * (replaces `Share { cws: Vec<Cw>, cw_np1 }`, lib.rs:208-214 and 275-283),
 * structure-of-arrays so a wave reads one level of 64 keys coalesced:
 *   offset 0                 cw_s  [n][K][lambda]   Cw::s
 *   offset n*K*lambda        cw_v  [n][K][lambda]   Cw::v
 *   offset 2*n*K*lambda      cw_t  [n][K]  u8       bit0 = Cw::tl, bit1 = Cw::tr
 *   offset dcf_cwb_np1_offset cw_np1[K][lambda]     Share::cw_np1
 * (the cw_np1 offset is 2*n*K*lambda + n*K rounded up to 16).  K = 1 is the
 * single-key layout.  Size: dcf_cwb_bytes().
 *
 * Errors: the reference panics where this ABI returns a code —
 *   DCF_ERR_KEY      assert_eq!(k.cws.len(), N * 8)           lib.rs:165
 *   DCF_ERR_CIPHER_N self.ciphers[i * 16 + j] out of range     prg.rs:51
 *   DCF_ERR_LEN      xs.len() != ys.len() (the reference silently truncates
 *                    via zip, lib.rs:196-198)
 * Nothing aborts the process.
 *
 * Memory: `*_device` entry points take device pointers and a hipStream_t (as
 * void*, NULL = the legacy default stream) and are asynchronous; the library
 * keeps no reference to caller buffers once the stream has passed the call.
 * Host entry points take host pointers and are synchronous: they run on three
 * streams the dcf_prg owns (copy-in, compute, copy-out) through pinned staging
 * buffers pooled on the dcf_prg, in chunks whose PCIe copies overlap the
 * kernels of neighbouring chunks, and they wait for those streams only (never
 * the whole device).  The GPU never reads or writes caller host memory.
 *
 * Threading (the reference's `Dcf::eval(&self, ...)` over a `Prg: Sync`, lib.rs:34,52):
 * every compute entry point may be called on ONE dcf_prg from any number of host
 * threads at once, and its device calls may be queued on different streams at once.
 * Each call leases a workspace (work counter, scratch, shared-prefix table, host
 * streams and staging) from a pool on the prg, so concurrent calls share no mutable
 * buffer; a workspace re-used on another stream first waits (on the device, with an
 * event) for the device work of its previous call, so a host call queued after a
 * *_device call on the same prg is ordered after it without any synchronization by the
 * caller.  The pool grows to the number of calls in flight at once and is freed with
 * the prg (dcf_prg_workspaces, dcf_prg_device_bytes, dcf_prg_host_pinned_bytes report
 * it).  The setters (dcf_prg_set_*) may race calls: a call reads each setting once.
 * Multi-GPU: one dcf_prg per device (all built from the same keys) and
 * dcf_eval_multi_gpu / _device below, or one process per device; the path shards by
 * points/keys with no collective.
 */
#ifndef DCF_HIP_H
#define DCF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_OK 0
#define DCF_ERR_ARG -1        /* null pointer, bad enum */
#define DCF_ERR_LAMBDA -2     /* lambda == 0 or lambda % 16 != 0 (prg.rs:17-18) */
#define DCF_ERR_CIPHER_N -3   /* too few ciphers for lambda (reference panics, prg.rs:51) */
#define DCF_ERR_N -4          /* n_bytes == 0 */
#define DCF_ERR_LEN -5        /* length mismatch (reference truncates, lib.rs:196) */
#define DCF_ERR_HIP -6        /* HIP runtime error; see dcf_last_error() */
#define DCF_ERR_UNSUPPORTED -7 /* shape not implemented by any kernel */
#define DCF_ERR_KEY -8        /* malformed key (lib.rs:165) */

#define DCF_BOUND_LT_BETA 0
#define DCF_BOUND_GT_BETA 1

/* AES engine for LAMBDA = 16 eval (dcf_prg_set_eval_mode); results are identical.  Values 2, 3
 * and 5 (bitsliced, hybrid and stream-hybrid engines, rounds 1-4) are retired: every A/B measured
 * them slower than the stream engine (profiles/AB_LOG.md), and setting them returns DCF_ERR_ARG. */
#define DCF_EVAL_AUTO 0      /* library's choice: STREAM for one key or N <= 32, TTABLE for many keys at N > 32 */
#define DCF_EVAL_TTABLE 1    /* LDS T-table AES, lockstep walk (A and B every level), one lane per point */
#define DCF_EVAL_STREAM 4    /* LDS T-table AES, per-lane block scheduling: a right step encrypts B only */

/* Opaque: an Aes256HirosePrg (prg.rs:22-24) whose AES-256 schedules live on one
 * device, i.e. `DcfImpl::new(Aes256HirosePrg::new(keys))` (lib.rs:74, prg.rs:27). */
typedef struct dcf_prg dcf_prg;

/* Version string of this library. */
const char* dcf_version(void);

/* Last error message of the calling thread ("" if none). */
const char* dcf_last_error(void);

/* Aes256HirosePrg::<LAMBDA, CIPHER_N>::new(keys) (prg.rs:27-33) on `device`.
 * keys: cipher_n * 32 bytes.  Needs cipher_n >= 1 for lambda == 16 and
 * cipher_n >= 18 for lambda >= 32 (the diagonal zip reads ciphers 0 and 17,
 * prg.rs:48-51). */
int dcf_hirose_prg_new(const uint8_t* keys, size_t cipher_n, size_t lambda, int device, dcf_prg** out);
/* Aes128MatyasMeyerOseasPrg::<LAMBDA, CIPHER_N>::new(keys) on `device` — the PRG
 * BASELINE.json's north_star names; the reference crate has no such PRG, so the
 * definition is ours (parity UNPINNED by the reference; DESIGN.md §4 "MMO"):
 *   out_b[j] = AES128_{keys[b * LAMBDA/16 + j]}(seed_j) ^ seed_j for b = s_L, v_L,
 *   s_R, v_R and every 16-byte block j (one key per output and block: "multi-block
 *   MMO" at LAMBDA >= 32), t_L / t_R = Lsb0 bit 0 of byte 0 of s_L / s_R, then bit 0
 *   of byte LAMBDA-1 cleared in all four outputs (the Hirose convention of prg.rs:63-68).
 * keys: cipher_n * 16 bytes, cipher_n >= 4 * lambda / 16 (else DCF_ERR_CIPHER_N).
 * Every gen / eval / prg entry point below accepts either PRG (LAMBDA >= 32: no
 * shared-prefix table). */
int dcf_mmo_prg_new(const uint8_t* keys, size_t cipher_n, size_t lambda, int device, dcf_prg** out);

/* 0 = Aes256HirosePrg, 1 = Aes128MatyasMeyerOseasPrg, -1 = null. */
int dcf_prg_kind(const dcf_prg* prg);

void dcf_prg_free(dcf_prg* prg);
size_t dcf_prg_lambda(const dcf_prg* prg);

/* Select the AES engine used by eval at LAMBDA = 16 (DCF_EVAL_AUTO / _TTABLE / _STREAM; the
 * LAMBDA >= 32 head and the MMO PRG have one engine each and ignore it).  Tuning and test knob
 * only: every engine returns identical bytes. */
int dcf_prg_set_eval_mode(dcf_prg* prg, int mode);

/* Shared prefix for single-key eval at LAMBDA = 16 (Hirose PRG: stream engine, and the
 * automatic engine's small-batch path; Aes128MatyasMeyerOseasPrg: every
 * engine setting) and, per key, for the LAMBDA >= 32
 * stream head (bytes [0,32) of the walk and the t-vector rows, 80 B per node).
 * Every point's walk (lib.rs:174-189) passes through the node of the key's GGM
 * tree named by its first D bits, and that node's (s, v, t) depends on nothing
 * else, so eval expands the top D levels once (2^(D+1) AES blocks, 32 B per node)
 * and starts each point at level D from its node:
 * D fewer levels per point, identical output bytes.
 *   levels = -1: automatic (the default): D = log2(points) (Aes128MatyasMeyerOseasPrg:
 *                log2(points) - 1), at most 27 (LAMBDA >= 32: log2(points) - 1, at most
 *                22), none below 8; Hirose small batches (32768 < points < 2^19 on the
 *                pair walk): 18 below 2^18 points, 19 above (1.7e7 / 3.4e7 B with the build buffers), at most
 *                8N - 1; none for Aes128MatyasMeyerOseasPrg small batches or up to 32768 points;
 *   levels =  0: off;  levels > 0: that depth (capped at 28 (LAMBDA >= 32: 30) and
 *                at 8N - 1).
 * The table and its build buffers are one allocation of the call's workspace; they stay
 * resident on the prg (sized by the largest D used) until dcf_prg_trim / dcf_prg_free, and
 * dcf_prg_device_bytes counts them.  Bytes at depth D:
 *   Hirose, LAMBDA = 16:  32 * 2^D (rows) + the one-launch build's two node buffers,
 *                         2 * 33 * 2^(D-H) with H = min(4, D - 18) levels built depth-first
 *                         (33 * 2^D when D <= 18) — 4.85e9 B at D = 27 (2^28 points, the auto
 *                         cap), 2.42e9 at 26, 0.61e9 at 24 (C2);
 *   MMO, LAMBDA = 16:     48 * 2^D (level-by-level build on rows: the table and the level above
 *                         it) — 6.44e9 B at D = 27; dcf_prg_set_prefix_max_bytes still counts
 *                         2 * 33 * 2^D, the build's earlier layout, so a cap picks the depth it picked;
 *   LAMBDA >= 32:         160 * 2^D (80-B rows + the build's two node buffers) — 0.34e9 at 21.
 * Multi-key stream eval (LAMBDA = 16, >= 32 points per key, 8N > 6 levels):
 * each key's own top tree of depth 5 (32 rows of 32 B per key, 36 PRG calls per key)
 * unless levels = 0; if its buffer cannot be allocated the points walk from the root. */
int dcf_prg_set_prefix_levels(dcf_prg* prg, int levels);
/* The prefix depth D a dcf_eval* call of this shape would use (0 = none). */
int dcf_eval_prefix_levels(const dcf_prg* prg, size_t n_bytes, size_t num_keys, size_t points_per_key);

/* The kernel family an eval call runs (dcf_eval_plan). */
typedef enum dcf_engine {
  DCF_ENGINE_WIDE_BATCH = 0,   /* LAMBDA >= 32, Hirose: several keys per pass of the stream head */
  DCF_ENGINE_WIDE_PER_KEY = 1, /* LAMBDA >= 32: the stream head (Hirose) or the MMO walk, key by key */
  DCF_ENGINE_MMO16 = 2,        /* Aes128MatyasMeyerOseasPrg at LAMBDA = 16, whatever the engine setting */
  DCF_ENGINE_ROW2 = 3,         /* latency kernels, one key in automatic mode: up to 2048 points, */
  DCF_ENGINE_ROW = 4,          /*   up to 8192, */
  DCF_ENGINE_OCT = 5,          /*   up to 32768 */
  DCF_ENGINE_PAIR = 6,         /* lockstep walk on a lane pair per point (small batches, automatic mode) */
  DCF_ENGINE_STREAM = 7,       /* DCF_EVAL_STREAM's engine */
  DCF_ENGINE_TTABLE = 8        /* DCF_EVAL_TTABLE's engine */
} dcf_engine;
/* The plan of a dcf_eval* call of this shape under the prg's current settings: what
 * dcf_eval_device (num_keys = 1, points_per_key = m), dcf_eval_multikey_device and the host entry
 * points decide before they launch anything.  Pure arithmetic on the prg's configuration and its
 * device's compute-unit count; nothing is launched.  Any of the four outputs may be NULL.
 *   engine         a dcf_engine.  LAMBDA >= 32: WIDE_BATCH for 2 or more keys of at most 32768
 *                  points each with the Hirose PRG and no forced prefix depth, else WIDE_PER_KEY.
 *                  LAMBDA = 16: MMO16 for that PRG; Hirose in automatic mode with one key, N <= 32
 *                  and no forced depth: ROW2 up to 2048 points, ROW up to 8192, OCT up to 32768;
 *                  otherwise PAIR while `small`; otherwise STREAM (DCF_EVAL_STREAM, or automatic
 *                  mode with one key or N <= 32) or TTABLE (DCF_EVAL_TTABLE, or automatic mode with
 *                  several keys at N > 32).
 *   key_mode       how a lockstep kernel finds a point's key: 0 one key, 1 points_per_key % 64 == 0
 *                  (a wave holds one key), 2 any other points_per_key.
 *   prefix_levels  what dcf_eval_prefix_levels returns for the shape.
 *   small          1 at LAMBDA = 16 in automatic mode when the call has fewer points than two per
 *                  lane of the device (num_keys * points_per_key < 2 * compute units * 1024).
 * Returns DCF_OK, or DCF_ERR_UNSUPPORTED where the eval call itself would fail before any device
 * work (multi-key stream eval at N > 32 or with 2^31 or more points per key; more than 2^32 64-point
 * units on the T-table engine): dcf_last_error carries the reason and the outputs are still filled.
 * null prg -> DCF_ERR_ARG, n_bytes == 0 -> DCF_ERR_N (outputs untouched). */
int dcf_eval_plan(const dcf_prg* prg, size_t n_bytes, size_t num_keys, size_t points_per_key, int* engine,
                  int* key_mode, int* prefix_levels, int* small);
/* The kernel family a gen call runs (dcf_gen_plan). */
typedef enum dcf_gen_route {
  DCF_GEN_ROW = 0,     /* Hirose, LAMBDA = 16, N <= 32, up to 2048 keys: one wave per key */
  DCF_GEN_COL = 1,     /*   up to 16384 keys: 16 lanes per key */
  DCF_GEN_QUAD = 2,    /* Hirose, LAMBDA = 16 otherwise: a lane quad per key up to compute units * 512 keys, */
  DCF_GEN_LANE = 3,    /*   one lane per key beyond */
  DCF_GEN_MMO16 = 4,   /* Aes128MatyasMeyerOseasPrg at LAMBDA = 16: one lane per key */
  DCF_GEN_WIDE = 5,    /* Hirose, LAMBDA >= 32: one workgroup per key, launches of 4096 keys */
  DCF_GEN_MMO_WIDE = 6 /* Aes128MatyasMeyerOseasPrg at LAMBDA >= 32: a head launch over block 0, a tail over the rest */
} dcf_gen_route;
/* The plan of a dcf_gen_batch_device call of num_keys keys (and of dcf_gen: num_keys = 1): what
 * the call decides before it launches anything.  Pure arithmetic on the prg's configuration and
 * its device's compute-unit count; nothing is launched.  Any of the four outputs may be NULL.
 *   route      a dcf_gen_route, as listed above.
 *   counter    1 when the QUAD or LANE route hands its 64-lane units out from a work counter: the
 *              call has at least compute units * 2048 lanes (4 per key on QUAD, 1 on LANE); below
 *              that, and on every other route, 0 (a grid-stride loop or a fixed grid).
 *   launches   kernel launches of the call: ceil(num_keys / 4096) on WIDE, 2 on MMO_WIDE (1 if
 *              LAMBDA were 16), 1 on every other route.
 *   host_tiny  1 when dcf_gen of this N passes its inputs and the CWB through the mapped 1 MiB
 *              buffer (one launch, no copy commands: the ROW / COL shapes) instead of the staged
 *              copies; it does not depend on num_keys and is meaningful at num_keys = 1.
 * null prg -> DCF_ERR_ARG, n_bytes == 0 -> DCF_ERR_N (outputs untouched). */
int dcf_gen_plan(const dcf_prg* prg, size_t n_bytes, size_t num_keys, int* route, int* counter, uint64_t* launches,
                 int* host_tiny);
/* Keys per kernel launch of a LAMBDA = 16 multi-key stream eval (dcf_eval_multikey_device and
 * the host entry points with several keys): min(2^24, 2^31 / points_per_key, 2^30 / 8N), at
 * least 1 — the engine's point, work and CW-digest-row indices are 32-bit, so a larger call runs
 * as consecutive launches over whole keys.  Pure arithmetic (no device access). */
size_t dcf_eval_keys_per_launch(size_t n_bytes, size_t points_per_key);
/* Cap on the device memory the AUTOMATIC prefix depth may allocate (table + build
 * buffers, which stay resident on the prg until dcf_prg_trim / dcf_prg_free; sizes above):
 * the auto depth is lowered until they fit, and no table is built below depth 8.  0 = no cap
 * (the default: 4.85e9 B at the auto cap D = 27, Hirose LAMBDA = 16).  Forced depths ignore
 * it.  Output bytes never change. */
int dcf_prg_set_prefix_max_bytes(dcf_prg* prg, size_t max_bytes);

/* Cross-call shared-prefix table.  dcf_eval_device calls with one key, LAMBDA = 16, the Hirose
 * PRG and N = 16 or N = 4 on the stream engine keep their table on the prg (per workspace) after
 * the call.  The next such call with the same cwb / s0 pointers, party, N and point-count class
 * compares, on the device and byte for byte, the key material a table is built from (party, N,
 * s0, cw_s / cw_v / cw_t of levels [0, min(31, 8N - 1))) with a copy kept beside the table:
 *   - equal: no rebuild.  At automatic depth the table is also deepened by one level at the start
 *     of a call once dcf_prefix_deepen_calls(D, m) calls have walked at depth D, up to
 *     dcf_prefix_reuse_max_depth(N, device memory, dcf_prg_set_prefix_max_bytes cap); a failed
 *     allocation keeps the depth.  A forced depth (dcf_prg_set_prefix_levels(k > 0)) is never deepened.
 *   - different (the key buffer was rewritten in place): the table is rebuilt at the first call's
 *     depth inside the same call.  Correction words of deeper levels and cw_np1 are not table
 *     material and may change freely.
 * The call stays asynchronous (no host read of the verdict); a call that deepens waits for its
 * stream once, to free the smaller table.  Output bytes never change.  dcf_prg_set_prefix_levels,
 * dcf_prg_set_eval_mode, dcf_prg_set_prefix_max_bytes and dcf_prg_set_phase_timing (so that a
 * timed call shows a whole call's table / walk split) make the next call start afresh;
 * dcf_prg_trim / dcf_prg_free release the table.  Other entry points (host pointers, multi-key,
 * range, full domain, multi-GPU) build their tables per call as before.
 *
 * dcf_prefix_deepen_calls: calls of m points after which deepening D -> D + 1 has paid for
 * itself, ceil(2^(D+1) / (1.257 m)) (2^(D+1) blocks once against 1.257 m per call), at least 1;
 * 0 = never (D outside [0, 31), m = 0).  m = 2^28: 1 at D = 27, 2 at 28, 4 at 29, 7 at 30.
 * dcf_prefix_reuse_max_depth: the deepest table reuse may grow to: min(31, 8N - 1), lowered until
 * the table's 32 * 2^D bytes fit 1/8 of device_bytes, and what a one-call build of that depth
 * takes (the sizes listed at dcf_prg_set_prefix_levels) fits cap_bytes (0 = no cap).
 * Both are pure arithmetic (no device access). */
uint64_t dcf_prefix_deepen_calls(int depth, size_t points);
int dcf_prefix_reuse_max_depth(size_t n_bytes, size_t device_bytes, size_t cap_bytes);
/* Device memory this dcf_prg currently holds (tables, prefix tables, scratch, staging, over
 * all of its workspaces). */
size_t dcf_prg_device_bytes(const dcf_prg* prg);
/* Pinned host memory this dcf_prg holds for the host-pointer entry points (per workspace: up
 * to two 128 MiB x + y chunks of the eval pipeline, sized to the largest call, a 1 MiB mapped
 * buffer for tiny calls and a mapped buffer of up to 64 MiB for mid-size evals: ~321 MiB per
 * workspace at most, one workspace per call in flight), kept until dcf_prg_trim / dcf_prg_free. */
size_t dcf_prg_host_pinned_bytes(const dcf_prg* prg);
/* Number of workspaces in the prg's pool (the most calls that were in flight at once). */
int dcf_prg_workspaces(const dcf_prg* prg);
/* Free every workspace no call holds right now (their device scratch, prefix tables, pinned
 * staging); calls in flight keep theirs.  The next call allocates afresh.  Returns the number
 * of workspaces freed. */
int dcf_prg_trim(dcf_prg* prg);

/* AES blocks the last eval call on this prg (the last one to return, from any thread)
 * encrypted for live points (LAMBDA = 16: the DCF_EVAL_STREAM engine;
 * LAMBDA >= 32: the stream head over all of the call's keys and passes; not counting a
 * shared-prefix table build, except the multi-key per-key top trees, whose blocks are
 * included, and the cross-call table of dcf_eval_device (above) at automatic depth: there the
 * count includes the blocks of the build (2^(D+1) - 2) or deepening (2^(D+1)) that really ran in
 * this call, decided on the device — none on a call that reused the table; at a forced depth the
 * walk alone), counted on the device; 0 for engines that do not count.
 * Measurement hook for the bench; call after the eval's stream has been synchronized.  0
 * before any eval; DCF_ERR_ARG while that call's workspace is leased by another call (the
 * hook never reads a workspace in use). */
int dcf_prg_last_eval_blocks(dcf_prg* prg, uint64_t* blocks);

/* Phase timing of eval calls (measurement hook, off by default).  When on, every eval call
 * records HIP events on its stream at entry, before its walk kernel(s) (after any shared-
 * prefix table, per-key top trees or CW digest/rows were built) and at the end.
 * dcf_prg_last_eval_phases reads the last eval call's split (call after synchronizing its
 * stream): prep_ms = table / digest preparation, walk_ms = the walk kernels, prefix_levels =
 * the shared-prefix depth it used (0 = none; for the cross-call table of dcf_eval_device the
 * depth the walk read from the device state, which after an in-place key change is the first
 * call's depth again).  DCF_ERR_ARG if no timed eval has run, or while
 * that call's workspace is leased by another call. */
int dcf_prg_set_phase_timing(dcf_prg* prg, int on);
int dcf_prg_last_eval_phases(dcf_prg* prg, float* prep_ms, float* walk_ms, int* prefix_levels);

/* CWB layout helpers (see above). */
size_t dcf_cwb_bytes(size_t n_bytes, size_t lambda, size_t num_keys);
size_t dcf_cwb_np1_offset(size_t n_bytes, size_t lambda, size_t num_keys);

/* ---- host-pointer, synchronous (mirror Dcf::gen / Dcf::eval) ---- */

/* Dcf::gen (lib.rs:26-31, impl lib.rs:86-161) for one key.
 * alpha: n_bytes, beta / s0_0 / s0_1: lambda, cwb_out: dcf_cwb_bytes(n_bytes, lambda, 1). */
int dcf_gen(dcf_prg* prg, size_t n_bytes, const uint8_t* alpha, const uint8_t* beta, const uint8_t* s0_0,
            const uint8_t* s0_1, int bound, uint8_t* cwb_out);

/* Dcf::eval (lib.rs:34, impl lib.rs:163-204).  xs: m * n_bytes (x_i contiguous),
 * ys: m * lambda (overwritten, lib.rs:171).  cwb: one key, s0: k.s0s[0]. */
int dcf_eval(dcf_prg* prg, size_t n_bytes, int party, const uint8_t* cwb, size_t cwb_len, const uint8_t* s0,
             const uint8_t* xs, size_t m, uint8_t* ys, size_t ys_len);

/* Aes256HirosePrg::gen (prg.rs:42-73) for m seeds (test hook for PRG vectors).
 * seeds: m * lambda; out: m * (4 * lambda + 2) = s_l | v_l | s_r | v_r | t_l | t_r. */
int dcf_prg_gen(dcf_prg* prg, const uint8_t* seeds, size_t m, uint8_t* out);

/* ---- device-pointer, asynchronous on `stream` ---- */

/* Batched Dcf::gen: K independent keys (the kernel route: dcf_gen_plan).
 * alpha: K * n_bytes, beta / s0_0 / s0_1: K * lambda (row k = key k),
 * cwb_out: dcf_cwb_bytes(n_bytes, lambda, K).
 * beta, s0_0, s0_1 and cwb_out must be 16-byte aligned: the kernels read and write them as uint4.
 * The call writes cw_s, cw_v, cw_t and cw_np1 and nothing else: the padding bytes between cw_t
 * and cw_np1 ([2 * 8N * K * lambda + 8N * K, dcf_cwb_np1_offset)) keep what the buffer held.
 * (dcf_gen returns them as zeros.) */
int dcf_gen_batch_device(dcf_prg* prg, size_t n_bytes, size_t num_keys, const uint8_t* alpha, const uint8_t* beta,
                         const uint8_t* s0_0, const uint8_t* s0_1, int bound, uint8_t* cwb_out, void* stream);

/* Dcf::eval of one key over m points (x_i contiguous, n_bytes each). */
int dcf_eval_device(dcf_prg* prg, size_t n_bytes, int party, const uint8_t* cwb, const uint8_t* s0,
                    const uint8_t* xs, size_t m, uint8_t* ys, void* stream);

/* Dcf::eval for K keys x P points each: point j of key k is xs[k*P + j],
 * its output ys[k*P + j]; s0s: K * lambda (k.s0s[0] of each key). */
int dcf_eval_multikey_device(dcf_prg* prg, size_t n_bytes, size_t num_keys, size_t points_per_key, int party,
                             const uint8_t* cwb, const uint8_t* s0s, const uint8_t* xs, uint8_t* ys, void* stream);

/* ---- multi-GPU (one call drives G devices) ----
 * The reference spreads Dcf::eval over every host core inside one call (rayon,
 * lib.rs:194-199); these spread it over G GPUs.  prgs[g] is a dcf_prg on the
 * device that evaluates slice g; all G must be built from the same keys (and
 * kind, lambda) — checked, DCF_ERR_ARG otherwise — and be distinct.  Points are
 * split into G contiguous slices, slice g = dcf_point_slice(m, G, g): the first
 * m % G slices hold one extra point.  Every (key, point) is independent, so no
 * collective runs during evaluation. */

/* Contiguous slice [start, start + count) of `total` items for slice g of G. */
void dcf_point_slice(size_t total, size_t G, size_t g, size_t* start, size_t* count);

/* Dcf::eval (lib.rs:163-204) of one key over host buffers on G devices: slice g
 * of xs goes to prgs[g]'s device (one host thread per device, each running the
 * pipelined host path above) and its outputs land directly in the matching rows
 * of ys.  Synchronous; same arguments and errors as dcf_eval. */
int dcf_eval_multi_gpu(dcf_prg* const* prgs, size_t G, size_t n_bytes, int party, const uint8_t* cwb,
                       size_t cwb_len, const uint8_t* s0, const uint8_t* xs, size_t m, uint8_t* ys, size_t ys_len);

/* Device-resident variant.  cwb (cwb_len bytes) and s0 are HOST pointers: the key
 * is copied to every device once per call (the broadcast; 4.2 KB at N = LAMBDA =
 * 16).  xs[g] / ys[g]: ms[g] points / outputs on prgs[g]'s device; streams[g]:
 * that device's stream (streams may be NULL = each device's default stream).
 * gather_ys: NULL, or a buffer on prgs[0]'s device of (sum of ms) * lambda bytes
 * that receives every slice's outputs in slice order (hipMemcpyPeerAsync over
 * xGMI, queued on streams[g] after slice g's eval).  Asynchronous: the caller
 * synchronizes every streams[g] before reading ys or gather_ys. */
int dcf_eval_multi_gpu_device(dcf_prg* const* prgs, size_t G, size_t n_bytes, int party, const uint8_t* cwb,
                              size_t cwb_len, const uint8_t* s0, const uint8_t* const* xs, const size_t* ms,
                              uint8_t* const* ys, void* const* streams, uint8_t* gather_ys);

/* ---- key wire format (host only, no GPU) ----
 * `Share` as serialised by serde + bincode 1.x `bincode::serialize` (lib.rs:217-340;
 * Cargo.toml:44): little-endian, u64 length before every Vec, fields in
 * declaration order, bool = one byte 0/1:
 *   u64 |s0s|, |s0s| x (u64 lambda, lambda bytes)
 *   u64 8N,    8N x (u64 lambda, Cw.s, u64 lambda, Cw.v, u8 tl, u8 tr)
 *   u64 lambda, cw_np1
 * from_bincode writes the single-key CWB and the seeds; a Vec of the wrong
 * length (the reference's copy_from_slice panics, lib.rs:251), a bool byte > 1,
 * cws.len() != 8N (lib.rs:165), truncation or trailing bytes -> DCF_ERR_KEY. */
size_t dcf_share_bincode_bytes(size_t n_bytes, size_t lambda, size_t num_s0s);
int dcf_share_to_bincode(size_t n_bytes, size_t lambda, const uint8_t* cwb, const uint8_t* s0s, size_t num_s0s,
                         uint8_t* out, size_t out_len);
int dcf_share_from_bincode(size_t n_bytes, size_t lambda, const uint8_t* in, size_t in_len, uint8_t* cwb_out,
                           uint8_t* s0s_out, size_t max_s0s, size_t* num_s0s);

/* Full-domain eval: ys[x] = Dcf::eval(party, k, x) for every x in
 * [0, 2^(8N)), x read big-endian (Msb0, lib.rs:181) — i.e. the output of
 * dcf_eval_device over all points in increasing order.  ys: 2^(8N) * lambda
 * bytes.  The key's tree is expanded once (lambda = 16: 2 AES blocks per leaf
 * instead of 16N per point), by a path of its own for lambda = 16 (Hirose from N = 2,
 * Aes128MatyasMeyerOseasPrg) and otherwise as dcf_eval_range_device over x0 = 0,
 * count = 2^(8N), whose block count it then reports; N <= 4. */
int dcf_eval_full_domain_device(dcf_prg* prg, size_t n_bytes, int party, const uint8_t* cwb, const uint8_t* s0,
                                uint8_t* ys, void* stream);

/* Contiguous-range eval (the other half of SURVEY §8 f4): ys[i] = Dcf::eval(party, k, x0 + i) for
 * i in [0, count), x0 + i the N-byte big-endian integer (Msb0, lib.rs:181) — the bytes
 * dcf_eval_device returns over those points in that order, for any x0 and count (no alignment, no
 * power of two), either PRG, every lambda, N <= 256.  cwb, s0 and ys (count * lambda bytes) are
 * device pointers; x0 is a HOST pointer to n_bytes bytes, read before the call returns and passed
 * to the kernels by value.  Asynchronous on `stream`.
 *   Hirose PRG, lambda = 16, N <= 16: the range is covered by the aligned blocks of 2^h leaves that
 *   intersect it (h = dcf_eval_range_subtree_levels); each block's root (level 8N - h) is walked
 *   from s0 and its subtree expanded once, 2 AES blocks per output instead of 16N, and leaves
 *   outside the range are not stored.  A call of more than 2^28 outputs runs as consecutive
 *   launches of 2^28 each (node and leaf indices are 32-bit within a launch, 64-bit across them);
 *   the workspace holds two buffers of the nodes four levels above the leaves, 4 B per output of
 *   a launch in all.
 *   dcf_prg_last_eval_blocks then reports the AES blocks of the root paths, the interior
 *   expansion and the tail, clipped leaves of the edge blocks included.
 *   MMO PRG, lambda = 16, N <= 16: the same blocks, heights, launches, workspace and level and
 *   tail kernels under the MMO policy, with its own root walk (kernels_range_mmo.h); a node's two children cost four AES-128 blocks and a step of a
 *   root walk two, so 4 AES-128 blocks per output plus 2 (8N - h) per root instead of 32N per
 *   point, and h = 0 walks every point in one launch.  Asynchronous on `stream` like the Hirose
 *   path: no materialised points, no stream wait.  dcf_prg_last_eval_blocks then reports the
 *   executed AES-128 blocks: nroots (2 (8N - h) + 4 (2^h - 1)) per launch, clipped leaves
 *   included, and 2 * 8N * count at h = 0.
 *   Hirose PRG, lambda >= 32, N <= 16 (kernels_range_wide.h): the same blocks and heights over the
 *   head state of that PRG — only bytes [0,32) of a node see AES, under ciphers 0 and 17, and a
 *   node's two children cost the four blocks A, B, C, D of kernels_wide.h.  The roots are walked one
 *   lane each (all four blocks per level), the levels below are expanded breadth-first, one launch
 *   each, on 80-byte rows, and the last 3 levels depth-first in registers (a wide node is 19
 *   words): 4 AES-256 blocks per output instead of 2.5 * 8N per point.  The tail writes y[0:32) of
 *   every leaf inside the range and, when lambda > 32, the leaf's t-vector (its root's prefix plus
 *   the subtree's bits), from which the existing tail kernels write y[32, lambda).  h = 0
 *   (count < 2^12): the root walk is the point walk and writes y[0:32) and the t-vector itself.
 *   A call runs as consecutive launch groups of dcf_eval_range_wide_points_per_launch outputs
 *   (32-bit indices within a group, 64-bit offsets across them).  One workspace allocation holds a
 *   group's t-vectors (64 B per output, lambda > 32), the two node buffers (80 B per node of the
 *   level three above the leaves), the roots' t-vector prefixes and the work counters; the CW
 *   digest is built once per call.  Asynchronous on `stream` like the lambda = 16 paths: no
 *   materialised points, no buffer of the call's own, no stream wait.  dcf_prg_last_eval_blocks
 *   then reports the executed AES-256 blocks of roots, levels and tail, clipped leaves included:
 *     sum over groups of nroots * (4 (8N - h) + 4 (2^h - 1)),
 *     nroots = (((x mod 2^h) + n - 1) >> h) + 1 for a group of n outputs from x,
 *   and 4 * 8N * count at h = 0.
 *   Otherwise (the MMO PRG at lambda >= 32, N > 16) the points are materialised on the device,
 *   2^22 at a time, and dcf_eval_device's path runs on them; that path waits for the stream
 *   before returning.
 * Errors, nothing launched: x0 + count > 2^(8N) -> DCF_ERR_ARG; bad party / null pointer ->
 * DCF_ERR_ARG; n_bytes == 0 -> DCF_ERR_N; N > 256 -> DCF_ERR_UNSUPPORTED.  count == 0 -> DCF_OK,
 * nothing written. */
int dcf_eval_range_device(dcf_prg* prg, size_t n_bytes, int party, const uint8_t* cwb, const uint8_t* s0,
                          const uint8_t* x0, uint64_t count, uint8_t* ys, void* stream);

/* The same over host buffers, synchronous: outputs come back in chunks of up to 128 MiB through the
 * prg's staging pool on its compute stream.  ys_len != count * lambda -> DCF_ERR_LEN; cwb_len not
 * one key's -> DCF_ERR_KEY (as dcf_eval). */
int dcf_eval_range(dcf_prg* prg, size_t n_bytes, int party, const uint8_t* cwb, size_t cwb_len, const uint8_t* s0,
                   const uint8_t* x0, uint64_t count, uint8_t* ys, size_t ys_len);

/* Height h of the aligned blocks the tree path of dcf_eval_range* uses for this shape (pure
 * arithmetic, no device access):
 *   count < 2^12:  h = 0 — every point is walked on its own (32 lanes per point);
 *   otherwise:     h = min(8N, 14, max(8, floor(log2(count)) - 8)).
 * At least 2^8 blocks cover a range, so the root walk and the first levels below it have a few
 * hundred nodes to spread over the CUs; h stops at 14: ten breadth-first levels (one launch each)
 * above a 4-level register tail.  Root paths cost 2 (8N - h) / 2^h AES blocks per output (< 0.94 at N = 16), the two
 * clipped edge blocks at most 4 * 2^h blocks in all. */
int dcf_eval_range_subtree_levels(size_t n_bytes, uint64_t count);

/* Outputs per launch group of the Hirose lambda >= 32 tree path of dcf_eval_range* (pure
 * arithmetic, no device access): the points whose t-vectors fill the 256 MiB the point walk's
 * passes use (2^22 at N <= 16), and at most 2^28.  0 for a shape that path does not take
 * (n_bytes == 0, n_bytes > 16, lambda < 32). */
uint64_t dcf_eval_range_wide_points_per_launch(size_t n_bytes, size_t lambda);

/* Multi-key contiguous-range eval: K keys over one range, ys[(k * count + i) * lambda ..] =
 * Dcf::eval(party, key k, x0 + i) — dcf_eval_range_device of every key of a K-key block in one
 * call (lookup-table / spline protocols, batched comparison gates: many keys over one small
 * domain or window).  cwb is the K-key correction-word block as dcf_gen_batch_device writes it and
 * dcf_eval_multikey_device reads it ([n][K][lambda], [n][K][lambda], [n][K], cw_np1[K][lambda] at
 * dcf_cwb_np1_offset(n_bytes, lambda, K)); s0s: K * lambda bytes; ys: K * count * lambda bytes;
 * all device pointers.  x0 is a HOST pointer to n_bytes big-endian bytes, read before the call
 * returns.  Asynchronous on `stream`.
 *   Hirose PRG, lambda = 16, N <= 16: every key's range is covered by the same
 *   nroots = (((x0 mod 2^h) + count - 1) >> h) + 1 aligned blocks of 2^h leaves
 *   (h = dcf_eval_range_multikey_subtree_levels).  The K * nroots roots are walked from their keys'
 *   seeds, the levels below are expanded breadth-first over all keys at once (one launch per
 *   level, the keys one after another in every node buffer, each in leaf order) and the last 4
 *   levels depth-first in registers: 2 AES blocks per output plus 2 (8N - h) per root.  Correction
 *   words are read per lane at [level][key].  Node and output indices are 32-bit within a launch
 *   group of dcf_eval_range_keys_per_launch whole keys (keys * (nroots << h) <= 2^28; only the key
 *   offset is 64-bit across groups); when one key alone exceeds 2^28 outputs the keys run one after
 *   another, 2^28 outputs per group.  The workspace holds two buffers of the nodes four levels
 *   above the leaves of a group (at most 2 x 512 MiB).  dcf_prg_last_eval_blocks then reports the
 *   AES blocks of the root paths, the interior levels and the tail, clipped leaves included, summed
 *   over all keys and groups.
 *   MMO PRG, lambda = 16, N <= 16: the same blocks, heights, launch groups and workspace with the
 *   MMO kernels: 4 AES-128 blocks per output plus 2 (8N - h) per root, h = 0 in one launch over all
 *   (key, point) pairs.  Asynchronous on `stream` like the Hirose path: no key-by-key gather, no
 *   stream wait.  dcf_prg_last_eval_blocks then reports the executed AES-128 blocks,
 *   keys * nroots (2 (8N - h) + 4 (2^h - 1)) per group, and 2 * 8N * K * count at h = 0.
 *   Hirose PRG, lambda >= 32, N <= 16 (kernels_range_wide.h under a per-lane key policy): one tree
 *   expansion over the keys of a launch group, blocks of height
 *   h = dcf_eval_range_wide_multikey_subtree_levels.  The keys * nroots roots are walked one lane
 *   each from their keys' seeds, the levels below are expanded breadth-first over all keys at once
 *   on 80-byte rows (the keys one after another in every node buffer, each in leaf order; node j of
 *   a level with `per` nodes per key is node j - key * per of key j / per) and the last level in
 *   registers; the correction words come per lane from the key-major CW digest of the group.  Leaf
 *   g of a key is its output g - skip: y[0:32) and, when lambda > 32, the t-vector go to row
 *   key * count + (g - skip) of the group, from which the existing tail kernels write
 *   y[32, lambda) with count points per key.  h = 0: one root walk over the keys * count (key,
 *   point) pairs.  Indices are 32-bit within a launch group of
 *   dcf_eval_range_wide_keys_per_launch whole keys; only the key offset is 64-bit.  When count >
 *   32768, or one key alone exceeds a group, the keys run one after another through the
 *   single-key kernels, each read in place from the K-key block, in dcf_eval_range_device's
 *   launch groups.  One workspace allocation holds a group's t-vectors, node buffers (80 B per
 *   two outputs), root prefixes and counters; the digest is keys * 8N * 65 bytes.  Asynchronous on
 *   `stream`: no gather, no buffer of the call's own, no stream wait.  dcf_prg_last_eval_blocks
 *   then reports the executed AES-256 blocks, exactly
 *     sum over groups of keys * nroots * (4 (8N - h) + 4 (2^h - 1)),   4 * 8N * K * count at h = 0.
 *   Otherwise (the MMO PRG at lambda >= 32, N > 16) — key by key: each key is gathered into the
 *   single-key layout in a buffer of the call's own and run through dcf_eval_range_device's path;
 *   the call waits for the stream before it returns.
 * Errors, nothing launched: null prg / cwb / s0s / x0, null ys with work to do, bad party ->
 * DCF_ERR_ARG; n_bytes == 0 -> DCF_ERR_N; N > 256 -> DCF_ERR_UNSUPPORTED; x0 + count > 2^(8N) ->
 * DCF_ERR_ARG.  num_keys == 0 or count == 0 -> DCF_OK, nothing written. */
int dcf_eval_range_multikey_device(dcf_prg* prg, size_t n_bytes, size_t num_keys, int party, const uint8_t* cwb,
                                   const uint8_t* s0s, const uint8_t* x0, uint64_t count, uint8_t* ys, void* stream);

/* Height h of the aligned blocks the tree path of dcf_eval_range_multikey_device uses (pure
 * arithmetic, no device access; 0 for n_bytes == 0 or num_keys == 0):
 *   count < 64 or num_keys * count < 2^12:  h = 0 — every point is walked on its own;
 *   otherwise:                              h = min(8N, 14, floor(log2(count)) - 2).
 * So h = 0 or 4 <= h <= min(8N, 14), and 2^h <= count / 4: a key has at least 4 blocks and its two
 * clipped edge blocks waste at most count / 2 leaves.  The parallelism comes from K * nroots, so
 * the blocks are as tall as that allows (root paths cost 2 (8N - h) blocks per 2^h leaves); below
 * 2^12 outputs in the whole call the direct walk's single launch wins.  It is not the single-key
 * rule at num_keys = 1. */
int dcf_eval_range_multikey_subtree_levels(size_t n_bytes, size_t num_keys, uint64_t count);

/* Whole keys per launch group of that path: the most keys with keys * (((count >> h) + 2) << h) <=
 * 2^28 (every key has at most (count >> h) + 2 blocks), at least 1; num_keys enters through h
 * only.  1 also when one key alone exceeds a launch. */
size_t dcf_eval_range_keys_per_launch(size_t n_bytes, size_t num_keys, uint64_t count);

/* Height h of the aligned blocks dcf_eval_range_multikey_device uses on the Hirose PRG at
 * lambda >= 32, N <= 16 (pure arithmetic, no device access):
 *   count >= 2^12:  dcf_eval_range_subtree_levels(n_bytes, count) — a key has at least 16 blocks of
 *                   its own, and the call executes exactly the blocks of the K single-key calls;
 *   count <  2^12:  dcf_eval_range_multikey_subtree_levels(n_bytes, num_keys, count) — where the
 *                   single-key rule would walk every point of every key from the root.
 * 0 for a shape that path does not take (n_bytes == 0, n_bytes > 16, num_keys == 0) and for
 * count == 0. */
int dcf_eval_range_wide_multikey_subtree_levels(size_t n_bytes, size_t num_keys, uint64_t count);

/* Whole keys per launch group of that path at that height h: the most keys such that
 *   keys * (((count >> h) + 2) << h) <= dcf_eval_range_wide_points_per_launch(n_bytes, lambda)
 *     (every key has at most (count >> h) + 2 blocks: the t-vector bound, 2^22),
 *   keys <= 4096, and keys * ceil(count / 4096) <= 32768 (the grid rows of the kernels that write
 *     y[32, lambda): one row per key and 4096 points, as dcf_eval_multikey_device keeps them),
 *   4 * keys * 8N < 2^32 (the CW digest's 32-bit index),
 * at least 1; num_keys enters through h only.  1 when count > 32768 or one key alone exceeds a
 * group: the keys then run one after another.  0 for a shape that path does not take
 * (n_bytes == 0, n_bytes > 16, num_keys == 0, lambda < 32) and for count == 0. */
size_t dcf_eval_range_wide_keys_per_launch(size_t n_bytes, size_t lambda, size_t num_keys, uint64_t count);

/* Range fold: the XOR of a key's range outputs, each masked by its row of a public table,
 *   out = XOR over i in [0, count) of ( Dcf::eval(party, k, x0 + i) AND w[i] ),
 * one lambda-byte value instead of the count * lambda bytes of dcf_eval_range_device.  The two
 * parties' values XOR to the XOR of beta & w[i] over the i with x0 + i < alpha (LtBeta; > alpha for
 * GtBeta): the prefix-XOR of the table up to the secret alpha when beta is all-ones.  cwb, s0, w
 * (count * lambda bytes, row i masks point x0 + i; NULL: no mask, the plain XOR of the outputs) and
 * out (lambda bytes, OVERWRITTEN, not accumulated into) are device pointers, 16-byte aligned; x0 is a
 * HOST pointer to n_bytes big-endian bytes, read before the call returns.  Asynchronous on
 * `stream`.
 *   Fused — lambda = 16, N <= 16, either PRG, count >= 2^12 (h = dcf_eval_range_subtree_levels
 *   > 0): dcf_eval_range_device's tree path with the same blocks, heights, launch groups of 2^28
 *   outputs, workspace (4 B per output of a group), root and level kernels; only the tail kernel
 *   differs: it loads w[i] for each leaf inside the range, XORs the masked leaf into four words of
 *   the lane, combines the lanes of a wave by shuffles and updates `out` with one 4-word atomic XOR
 *   per wave.  `out` is zeroed on the stream once per call and all groups fold into it; no buffer
 *   of count * lambda bytes exists.  dcf_prg_last_eval_blocks then reports exactly what
 *   dcf_eval_range_device reports for the shape: per group
 *     nroots (2 (8N - h) + 2 (2^h - 1)) AES-256 blocks (Hirose),
 *     nroots (2 (8N - h) + 4 (2^h - 1)) AES-128 blocks (MMO),
 *     nroots = (((x mod 2^h) + n - 1) >> h) + 1 for a group of n outputs from x.
 *   Otherwise (count < 2^12, lambda >= 32, N > 16): dcf_eval_range_device's path for the shape
 *   runs in passes of min(2^22, 256 MiB / lambda) outputs into a buffer of the workspace (at most
 *   256 MiB, kept with the workspace, counted by dcf_prg_device_bytes) and k_fold_rows XORs each
 *   pass's masked rows into `out`.  No stream wait, except for the MMO PRG at lambda >= 32 and for
 *   N > 16, where the range path itself waits for the stream in every pass.
 * Errors, nothing launched: those of dcf_eval_range_device (x0 + count > 2^(8N), bad party, null
 * prg / cwb / s0 / x0 -> DCF_ERR_ARG; n_bytes == 0 -> DCF_ERR_N; N > 256 -> DCF_ERR_UNSUPPORTED);
 * null out -> DCF_ERR_ARG.  count == 0 -> DCF_OK, out = lambda zero bytes (the empty XOR). */
int dcf_eval_range_fold_device(dcf_prg* prg, size_t n_bytes, int party, const uint8_t* cwb, const uint8_t* s0,
                               const uint8_t* x0, uint64_t count, const uint8_t* w, uint8_t* out, void* stream);

/* The same for the K keys of a K-key block (as dcf_eval_range_multikey_device takes it) over one
 * range and one table: out[k] = XOR_i ( Dcf::eval(party, key k, x0 + i) AND w[i] ), K * lambda
 * bytes, overwritten.  All keys share w; a per-key rotation of the table is not offered.
 *   Fused — lambda = 16, N <= 16, either PRG, h = dcf_eval_range_multikey_subtree_levels > 0:
 *   dcf_eval_range_multikey_device's tree path, same launch groups of
 *   dcf_eval_range_keys_per_launch whole keys and same workspace, with the folding tail.  The lanes
 *   of a wave differ in their key (node j of a level with `per` nodes per key has key j / per, so
 *   the keys are non-decreasing over the lanes): after its 16 leaves each lane enters a segmented
 *   XOR scan over the runs of equal key, and the last lane of each run updates out[key] — one
 *   4-word atomic XOR per (wave, key).  When one key alone exceeds 2^28 outputs, its groups fold
 *   into the same row; the table offset across groups is 64-bit.  Needs K * lambda bytes of output
 *   and the range call's workspace, nothing else.  dcf_prg_last_eval_blocks reports what
 *   dcf_eval_range_multikey_device reports: keys * nroots (2 (8N - h) + B (2^h - 1)) per group,
 *   B = 2 (Hirose, AES-256) or 4 (MMO, AES-128).
 *   Otherwise (h = 0, lambda >= 32, N > 16): dcf_eval_range_multikey_device's path for the shape
 *   over passes of whole keys — as many as fit min(2^22, 256 MiB / lambda) outputs — into the
 *   workspace's fold buffer, each folded by k_fold_rows; a key of more outputs than a pass is
 *   gathered into the single-key layout and run as dcf_eval_range_fold_device's passes.  No stream
 *   wait, except for the MMO PRG at lambda >= 32 and for N > 16 (as the range call).
 * Errors as above (null s0s -> DCF_ERR_ARG).  num_keys == 0 -> DCF_OK, nothing written;
 * count == 0 -> DCF_OK, out = K * lambda zero bytes. */
int dcf_eval_range_fold_multikey_device(dcf_prg* prg, size_t n_bytes, size_t num_keys, int party, const uint8_t* cwb,
                                        const uint8_t* s0s, const uint8_t* x0, uint64_t count, const uint8_t* w,
                                        uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DCF_HIP_H */
