// kernels_range.h — contiguous-range eval: ys[i] = Dcf::eval(b, k, x0 + i), i in [0, count), for one
// key, and ys[k * count + i] = Dcf::eval(b, key k, x0 + i) for K keys over one range.
// Included by dcf_hip.hip only (after kernels16.h and kernels_lat.h).
//
// Consecutive points share almost their whole GGM path, so the Hirose LAMBDA = 16 path covers the
// range by the aligned blocks of 2^h leaves that intersect it and expands each block's subtree
// once: 2 AES blocks per output instead of 16N per point (DESIGN.md "Range eval", "Multi-key range
// eval").  Every key's range is covered by the same nroots blocks; every node buffer holds the keys
// of a launch group one after another, each in leaf order, so node j of a level with d nodes per
// key belongs to key j / d and key k's outputs are contiguous.
//   k_range_roots16   the roots of those blocks — the nodes of level 8N - h whose prefixes run
//                     from x0 >> h upwards — each walked from s0 on a 32-lane half-wave (RowPrg, as
//                     k_prefix_build16's root path); the path bits come from the 128-bit value
//                     prefix + root index.  h = 0 (LEAF): the "roots" are the points themselves and
//                     the kernel writes y (small counts).
//   k_range_level16   the h - kFdTail levels below the roots, breadth-first over all blocks at
//                     once, one launch per level, on 32-byte PrefixTable rows: the nodes of
//                     all blocks stay consecutive, in leaf order, in two ping-pong buffers.  The
//                     child rules are fd_children's (kernels16.h) or mmo_children's.  The MMO
//                     prefix-table build (build_prefix) is this kernel from level 1 down.
//   k_range_tail16    the register depth-first tail of k_fd_dfs16 (the full-domain fast path's,
//                     kernels16.h) on those nodes; a leaf's output index is its distance from x0
//                     and leaves outside the range are not stored.
// Each is a template on the key policy, RangeOneKey or RangeKeys, and is instantiated for both.
// k_range_tail16 is also a template on the output policy: RangeStore writes every leaf inside the
// range, RangeFold XORs the leaves, each masked by its row of a public table, into one LAMBDA-byte
// value per key and stores nothing per leaf (DESIGN.md "Range fold").
// k_range_level16 and k_range_tail16 are also templates on the PRG policy: RangeHirose here,
// RangeMmo in kernels_range_mmo.h, which has the MMO PRG's own root walk (k_range_roots16_mmo)
// as well.  kernels_range_wide.h has the three stages over the Hirose PRG's head state at
// LAMBDA >= 32, for one key.
//   k_range_points    the points x0 + i as N-byte big-endian strings, for the MMO PRG at
//                     LAMBDA >= 32 and for N > 16, which have no tree-sharing path (the existing
//                     eval runs on them).
//   k_rangemk_gather  key k of a K-key block as a single-key block (the same slow path, key by key).
//   k_fold_rows       the fold of rows that a range call has written: the shapes without a folding
//                     tail (h = 0, LAMBDA >= 32, N > 16).
// The pointers the kernels get are already advanced to the first key of the launch group; K stays
// the row stride.  All node, key and output indices of a tree launch are 32-bit (the host keeps
// keys * (nroots << h) <= 2^28).
#pragma once

#include "aes_lds.h"
#include "kernels16.h"
#include "kernels_lat.h"

namespace {

// An unsigned 128-bit value: the low 16 bytes of a big-endian x.
struct RangeX {
  uint64_t lo, hi;
};
__host__ __device__ __forceinline__ RangeX range_add(const RangeX a, const uint64_t i) {
  RangeX r;
  r.lo = a.lo + i;
  r.hi = a.hi + (r.lo < a.lo ? 1u : 0u);  // the carry crosses the 64-bit boundary
  return r;
}
__host__ __device__ __forceinline__ uint32_t range_bit(const RangeX a, const uint32_t i) {  // i < 128
  return (uint32_t)((i < 64u ? a.lo >> i : a.hi >> (i - 64u)) & 1u);
}

constexpr uint32_t kRangeMaxH = 14;  // at most 10 breadth-first levels above the tail
constexpr uint32_t kRangeTopMax = 240;  // bytes of x above the low 16 (N <= 256)

// Bytes [0, N - 16) of a point wider than 128 bits (big-endian, as given): constant over a launch.
struct RangeTop {
  uint8_t b[kRangeTopMax];
};

// n / d for n < 2^28 without a division: q = (n * mul) >> sh with sh = 28 + ceil(log2 d) and
// mul = ceil(2^sh / d) <= 2^29 + 1 (round-up method: mul * d - 2^sh < d <= 2^(sh - 28), so the
// quotient is exact for every n < 2^28).  Built on the host once per launch.
struct RangeDiv {
  uint32_t d, mul, sh;
};
__host__ inline RangeDiv range_div_make(const uint32_t d) {  // 1 <= d <= 2^28
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  RangeDiv r;
  r.d = d;
  r.sh = 28u + l;
  r.mul = (uint32_t)(((1ull << r.sh) + d - 1u) / d);
  return r;
}
__host__ __device__ __forceinline__ uint32_t range_div(const RangeDiv dv, const uint32_t n) {
  return (uint32_t)(((uint64_t)n * dv.mul) >> dv.sh);
}

// Key policies: the key of node (or root) j of a level with `per` nodes per key, j's index within
// that key, and the row of the key block that holds the key's correction words of level lev.
//   kPerLane   the lanes of a wave may differ in their key, so correction words, seeds and cw_np1
//              are per-lane loads inside the work loop; otherwise they are uniform, loaded once
//              ahead of it and held in scalars.
//   Idx        the root kernel's index type (a single-key direct walk takes the caller's count).
struct RangeOneKey {
  static constexpr bool kPerLane = false;
  using Idx = uint64_t;
  static RangeOneKey make(uint64_t, uint32_t) { return {}; }
  template <class T>
  __device__ __forceinline__ uint32_t key(T) const { return 0u; }
  template <class T>
  __device__ __forceinline__ T node(T j, uint32_t) const { return j; }
  __device__ __forceinline__ uint64_t cw(uint32_t lev, uint32_t) const { return lev; }
};
// Key j / per of the group; its words are a broadcast within one key, coalesced across neighbours.
struct RangeKeys {
  static constexpr bool kPerLane = true;
  using Idx = uint32_t;
  uint64_t K;  // keys in the block: the row stride
  RangeDiv per;
  static RangeKeys make(uint64_t K, uint32_t per) { return {K, range_div_make(per)}; }
  __device__ __forceinline__ uint32_t key(uint32_t j) const { return range_div(per, j); }
  __device__ __forceinline__ uint32_t node(uint32_t j, uint32_t key) const { return j - key * per.d; }
  __device__ __forceinline__ uint64_t cw(uint32_t lev, uint32_t key) const { return (uint64_t)lev * K + key; }
};

// Root r (32 lanes each) of `total` = keys * per: the node of level `nwalk` of key kp.key(r) whose
// nwalk-bit prefix is pfx + kp.node(r), walked from (s0s[key], 0, party) with RowPrg, bits
// Msb-first.  LEAF = false: PrefixTable-style row (s with t in bit 0 of byte 15, then v) to
// out[2r], out[2r + 1]; the caller keeps nwalk >= 1, so s is masked there.  LEAF = true
// (nwalk = 8N, per = count, so r = key * count + i): y = v ^ s ^ t * cw_np1 (lib.rs:192) to out[r].
// blocks: the call's AES block count (dcf_prg_last_eval_blocks), 2 per level and root.
template <bool LEAF, class KP>
__global__ __launch_bounds__(kBlock, 1) void k_range_roots16(
    const uint32_t* __restrict__ tab, const RoundKeys rk, const uint4* __restrict__ cw_s,
    const uint4* __restrict__ cw_v, const uint8_t* __restrict__ cw_t, const uint4* __restrict__ cw_np1,
    const uint4* __restrict__ s0s, const KP kp, const uint32_t party, const RangeX pfx, const uint32_t nwalk,
    const typename KP::Idx total, uint4* __restrict__ out, unsigned long long* __restrict__ blocks) {
  using Idx = typename KP::Idx;
  __shared__ uint32_t lds[kLdsWords];
  lds_fill_tables(lds, tab);
  RowPrg rp;
  rp.init(rk);
  const uint32_t a = rp.a;
  const uint32_t s0a = KP::kPerLane ? 0u : reinterpret_cast<const uint32_t*>(s0s)[a];
  const uint32_t npa = KP::kPerLane ? 0u : reinterpret_cast<const uint32_t*>(cw_np1)[a];
  constexpr uint32_t kPer = kBlock / 32;  // roots per workgroup pass
  for (Idx base = (Idx)blockIdx.x * kPer; base < total; base += (Idx)gridDim.x * kPer) {
    const Idx r = base + (threadIdx.x >> 5);
    const bool live = r < total;
    const Idx rr = live ? r : total - 1u;
    const uint32_t key = kp.key(rr);
    const RangeX p = range_add(pfx, kp.node(rr, key));
    uint32_t s = KP::kPerLane ? reinterpret_cast<const uint32_t*>(s0s + key)[a] : s0a, v = 0u, t = party;
    for (uint32_t lev = 0; lev < nwalk; ++lev) {
      const uint64_t c = kp.cw(lev, key);
      const uint32_t cs = reinterpret_cast<const uint32_t*>(cw_s + c)[a];
      const uint32_t cv = reinterpret_cast<const uint32_t*>(cw_v + c)[a], ct = cw_t[c];
      uint32_t sl, vl, tl, sr, vr, tr;
      rp.children(lds, s, v, t, cs, cv, ct, sl, vl, tl, sr, vr, tr);
      const bool right = range_bit(p, nwalk - 1u - lev) != 0u;
      s = right ? sr : sl;
      v = right ? vr : vl;
      t = right ? tr : tl;
    }
    if (threadIdx.x == 0) atomicAdd(blocks, 2ull * nwalk * (unsigned long long)min((Idx)kPer, total - base));
    if (live && (threadIdx.x & 31u) < 4u) {  // row 0, lanes 0..3: columns 0..3
      if (LEAF) {
        const uint32_t np = KP::kPerLane ? reinterpret_cast<const uint32_t*>(cw_np1 + key)[a] : npa;
        reinterpret_cast<uint32_t*>(out + r)[a] = v ^ s ^ ((0u - t) & np);
      } else {
        uint32_t* o = reinterpret_cast<uint32_t*>(out + 2ull * r);
        o[a] = a == 3u ? ((s & kMaskLast) | (t << 24)) : s;
        o[4u + a] = v;
      }
    }
  }
}

// PRG policies of the level and tail kernels: what differs between the Hirose PRG (here) and the
// MMO PRG (RangeMmo, kernels_range_mmo.h).
//   Arg        the kernels' key argument, and arg(p) its value for a dcf_prg (the host's type)
//   keys()     the kernel's set-up of the keys, ahead of lds_fill_tables; what children() takes
//   children   both children of a node under the correction words of its level
//   kBlocks    AES blocks per node
//   kPacked    the tail keeps t in the node's word 3 under every key policy, not only per-lane keys
//   roots()    the PRG's root kernel; kRootsPer roots fill a workgroup before a second one pays
struct RangeHirose {
  using Arg = RoundKeys;  // by value: SGPRs
  static constexpr unsigned long long kBlocks = 2;
  static constexpr bool kPacked = false;
  static constexpr uint64_t kRootsPer = kBlock / 32;  // a pass of half-waves (RowPrg)
  template <class Prg>
  static Arg arg(const Prg* p) { return p->rk[0]; }
  template <bool LEAF, class KP>
  static auto roots() { return k_range_roots16<LEAF, KP>; }
  static __device__ __forceinline__ const RoundKeys& keys(const RoundKeys& rk) { return rk; }
  template <class... A>
  static __device__ __forceinline__ void children(A&&... a) { fd_children(a...); }
};

// Interior, one launch per level, on PrefixTable-style rows: the parents of level
// `lev` — rows in[2j], in[2j + 1] of all blocks of all keys, consecutive in leaf order — become the
// children rows out[4j .. 4j + 3], one lane per parent, waves claiming units of parents from
// ctr[0].  blocks: the call's AES block count, PRG::kBlocks per parent.
template <class PRG, class KP>
__global__ __launch_bounds__(kBlock, 1) void k_range_level16(
    const uint32_t* __restrict__ tab, const typename PRG::Arg rk, const uint4* __restrict__ cw_s,
    const uint4* __restrict__ cw_v, const uint8_t* __restrict__ cw_t, const KP kp, const uint32_t lev,
    const uint32_t nparents, const uint4* __restrict__ in, uint4* __restrict__ out, uint32_t* __restrict__ ctr,
    unsigned long long* __restrict__ blocks) {
  __shared__ uint32_t lds[kLdsWords];
  const auto& ks = PRG::keys(rk);
  lds_fill_tables(lds, tab);  // its barrier also publishes the keys
  const uint32_t lc = lane_const();
  uint32_t csw[4], cvw[4], ct = 0u;
  if constexpr (!KP::kPerLane) ct = fd_cw(cw_s, cw_v, cw_t, kp.cw(lev, 0u), csw, cvw);
  const uint32_t unit = fd_unit(nparents);
  uint32_t nlive = 0;  // parents this wave expanded: one atomic per wave, after its last unit
  for (uint64_t base = next_unit_base_n(ctr, ~0ull, unit); base < nparents;
       base = next_unit_base_n(ctr, base, unit)) {
    const uint32_t j = (uint32_t)base + (threadIdx.x & 63u);
    const bool live = j < nparents;
    const uint32_t jj = live ? j : nparents - 1u;
    nlive += (uint32_t)__popcll(__ballot(live));
    if constexpr (KP::kPerLane) ct = fd_cw(cw_s, cw_v, cw_t, kp.cw(lev, kp.key(jj)), csw, cvw);
    const uint4 a = in[2ull * jj], b = in[2ull * jj + 1u];
    const uint32_t s[4] = {a.x, a.y, a.z, a.w & kMaskLast}, v[4] = {b.x, b.y, b.z, b.w};
    uint32_t sl[4], vl[4], sr[4], vr[4], tl, tr;
    PRG::children(lds, lc, ks, csw, cvw, ct, s, v, (a.w >> 24) & 1u, sl, vl, tl, sr, vr, tr);
    if (!live) continue;
    uint4* o = out + 4ull * j;
    o[0] = make_uint4(sl[0], sl[1], sl[2], (sl[3] & kMaskLast) | (tl << 24));
    o[1] = make_uint4(vl[0], vl[1], vl[2], vl[3]);
    o[2] = make_uint4(sr[0], sr[1], sr[2], (sr[3] & kMaskLast) | (tr << 24));
    o[3] = make_uint4(vr[0], vr[1], vr[2], vr[3]);
  }
  if ((threadIdx.x & 63u) == 0 && nlive) atomicAdd(blocks, PRG::kBlocks * nlive);
}

// Output policies of the tail kernel: what becomes of leaf o (its distance from x0) of a key.
//   RangeStore  y goes to row o of the key's outputs.
//   RangeFold   y & w[o] is XORed into four accumulator words of the lane (w: the table of the
//               launch group, one row per output, shared by all keys; null: no mask).  The words
//               of a wave are combined without LDS (the workgroup's LDS is the tables) and XORed
//               into the key's row of `out` with one 4-word atomic update per wave (one key) or
//               per run of equal keys in the wave (per-lane keys).  The host zeroes `out` on the
//               stream once per call; XOR is associative and commutative, so the result is exact
//               whatever the order of the updates.
//   at(o)       the policy of the launch group that starts at output o of the call.
struct RangeStore {
  static constexpr bool kFold = false;
  RangeStore at(uint64_t) const { return {}; }
};
struct RangeFold {
  static constexpr bool kFold = true;
  const uint4* w;
  RangeFold at(uint64_t o) const { return {w ? w + o : nullptr}; }
  __device__ __forceinline__ uint4 mask(uint32_t o) const { return w ? w[o] : make_uint4(~0u, ~0u, ~0u, ~0u); }
};

// acc ^= y & m, y = v ^ s ^ t * cw_np1 (nt = 0 - t).
__device__ __forceinline__ void range_fold_leaf(uint32_t (&acc)[4], const uint32_t (&v)[4], const uint32_t (&s)[4],
                                                const uint32_t nt, const uint4 np, const uint4 m) {
  acc[0] ^= (v[0] ^ s[0] ^ (nt & np.x)) & m.x;
  acc[1] ^= (v[1] ^ s[1] ^ (nt & np.y)) & m.y;
  acc[2] ^= (v[2] ^ s[2] ^ (nt & np.z)) & m.z;
  acc[3] ^= (v[3] ^ s[3] ^ (nt & np.w)) & m.w;
}

// One key: the XOR of the wave's 64 accumulators (butterfly) into out[0..3], by lane 0.
__device__ __forceinline__ void range_fold_wave(uint32_t (&acc)[4], uint32_t* __restrict__ out) {
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] ^= __shfl_xor(acc[e], d);
  if ((threadIdx.x & 63u) == 0 && (acc[0] | acc[1] | acc[2] | acc[3]))
#pragma unroll
    for (int e = 0; e < 4; ++e) atomicXor(out + e, acc[e]);
}

// Per-lane keys, non-decreasing over the lanes of the wave (node j has key j / per): an inclusive
// segmented XOR scan over the runs of equal key (lane l takes lane l - d while that lane has l's
// key; the keys are ordered, so then every lane between has it too), after which the last lane of
// each run holds the run's XOR and updates out[4 key ..].  Clears acc.
__device__ __forceinline__ void range_fold_keys(uint32_t (&acc)[4], const uint32_t key, uint32_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t ok = __shfl_up(key, d);
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = __shfl_up(acc[e], d);
    if (lane >= d && ok == key)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] ^= o[e];
  }
  const uint32_t nk = __shfl_down(key, 1u);
  if ((lane == 63u || nk != key) && (acc[0] | acc[1] | acc[2] | acc[3]))
#pragma unroll
    for (int e = 0; e < 4; ++e) atomicXor(out + 4ull * key + e, acc[e]);
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = 0u;
}

// Tail: k_fd_dfs16's register depth-first expansion of the last H levels from the rows of level
// lev0 = 8N - H, one lane per node, waves claiming units of nodes from ctr[0] (the stack logic is
// written out here as there: a function template shared by the two compiled to 3 % more VALU work
// in the expansion loop and measured 3 % slower, profiles/AB_LOG.md round 8).  Node j is node kp.node(j) of key kp.key(j); its leaves are g = (node << H) ..
// (node << H) + 2^H - 1 of that key, counted from the first root's first leaf; the range starts
// `skip` leaves in and holds `count`, so leaf g is the key's output g - skip, stored at
// ys[key * count + g - skip] only when g - skip is below count (32-bit: a launch covers at most
// 2^28 outputs; g < skip wraps far above).
// PACKED (per-lane correction words, and the MMO PRG always): the node and the stack slots stay in
// the rows' form, 8 words with t in bit 24 of word 3, the bit s has cleared; the words take the
// registers that a separate t (9-word nodes) has otherwise.
// OUT: RangeStore as above; RangeFold: ys is the launch group's first row of `out` (16 bytes per
// key), the leaves below count are folded and nothing else is written.
// blocks: the call's AES block count, PRG::kBlocks (2^H - 1) per node — clipped leaves included.
template <int H, class PRG, class KP, class OUT>
__global__ __launch_bounds__(kBlock, 1) void k_range_tail16(
    const uint32_t* __restrict__ tab, const typename PRG::Arg rk, const uint4* __restrict__ cw_s,
    const uint4* __restrict__ cw_v, const uint8_t* __restrict__ cw_t, const uint4* __restrict__ cw_np1,
    const KP kp, const uint32_t lev0, const uint32_t nnodes, const uint4* __restrict__ rows, const uint32_t skip,
    const uint32_t count, uint4* __restrict__ ys, uint32_t* __restrict__ ctr,
    unsigned long long* __restrict__ blocks, const OUT op) {
  static_assert(H >= 2 && H <= 4, "register depth-first tail of 2..4 levels");
  constexpr bool PACKED = PRG::kPacked || KP::kPerLane;
  __shared__ uint32_t lds[kLdsWords];
  const auto& ks = PRG::keys(rk);
  lds_fill_tables(lds, tab);
  const uint32_t lc = lane_const();
  const uint4 np0 = KP::kPerLane ? make_uint4(0u, 0u, 0u, 0u) : cw_np1[0];
  const uint32_t unit = fd_unit(nnodes);
  uint32_t nlive = 0;  // nodes this wave expanded: one atomic per wave, after its last unit
  [[maybe_unused]] uint32_t acc[4] = {0u, 0u, 0u, 0u};  // RangeFold: the lane's masked leaves
  for (uint64_t base = next_unit_base_n(ctr, ~0ull, unit); base < nnodes;
       base = next_unit_base_n(ctr, base, unit)) {
    const uint32_t j = (uint32_t)base + (threadIdx.x & 63u);
    const bool live = j < nnodes;
    const uint32_t jj = live ? j : nnodes - 1u;
    nlive += (uint32_t)__popcll(__ballot(live));
    const uint32_t key = kp.key(jj);
    constexpr int W = PACKED ? 8 : 9;
    uint32_t stk[H - 1][W];  // pending right children, by depth
    uint32_t n[W];
    {
      const uint4 sv = rows[2ull * jj], vv = rows[2ull * jj + 1u];
      n[0] = sv.x; n[1] = sv.y; n[2] = sv.z; n[3] = PACKED ? sv.w : sv.w & kMaskLast;
      n[4] = vv.x; n[5] = vv.y; n[6] = vv.z; n[7] = vv.w;
      if constexpr (!PACKED) n[8] = (sv.w >> 24) & 1u;
    }
    // output of the node's first leaf within its key; idle lanes: none
    const uint32_t o0 = live ? (kp.node(jj, key) << H) - skip : 0x80000000u;
    for (uint32_t i = 0; i < (1u << (H - 1)); ++i) {
      uint32_t k = 0;
      if (i) {  // resume at the right child saved at depth H - 2 - ctz(i) (wave-uniform)
        const uint32_t d = (uint32_t)(H - 2) - (uint32_t)__builtin_ctz(i);
#pragma unroll
        for (uint32_t q = 0; q + 1 < (uint32_t)H; ++q)
          if (q == d)
#pragma unroll
            for (int e = 0; e < W; ++e) n[e] = stk[q][e];
        k = d + 1u;
      }
      for (;; ++k) {  // expand depth k (level lev0 + k)
        const uint64_t c = kp.cw(lev0 + k, key);
        const uint4 cs = cw_s[c], cv = cw_v[c];
        const uint32_t csw[4] = {cs.x, cs.y, cs.z, cs.w}, cvw[4] = {cv.x, cv.y, cv.z, cv.w};
        const uint32_t s[4] = {n[0], n[1], n[2], PACKED ? n[3] & kMaskLast : n[3]}, v[4] = {n[4], n[5], n[6], n[7]};
        uint32_t t;
        if constexpr (PACKED) t = (n[3] >> 24) & 1u;
        else t = n[8];
        uint32_t sl[4], vl[4], sr[4], vr[4], tl, tr;
        PRG::children(lds, lc, ks, csw, cvw, cw_t[c], s, v, t, sl, vl, tl, sr, vr, tr);
        if (k + 1u == (uint32_t)H) {  // leaves 2i, 2i + 1 of the node: y = v ^ s ^ t * cw_np1 (lib.rs:192)
          const uint32_t ol = o0 + 2u * i, orr = ol + 1u;
          const uint32_t ml = 0u - tl, mr = 0u - tr;
          const uint4 np = KP::kPerLane ? cw_np1[key] : np0;
          if constexpr (OUT::kFold) {
            if (ol < count) range_fold_leaf(acc, vl, sl, ml, np, op.mask(ol));
            if (orr < count) range_fold_leaf(acc, vr, sr, mr, np, op.mask(orr));
          } else {
            uint4* const yk = ys + (uint64_t)key * count;
            if (ol < count)
              yk[ol] = make_uint4(vl[0] ^ sl[0] ^ (ml & np.x), vl[1] ^ sl[1] ^ (ml & np.y),
                                  vl[2] ^ sl[2] ^ (ml & np.z), vl[3] ^ sl[3] ^ (ml & np.w));
            if (orr < count)
              yk[orr] = make_uint4(vr[0] ^ sr[0] ^ (mr & np.x), vr[1] ^ sr[1] ^ (mr & np.y),
                                   vr[2] ^ sr[2] ^ (mr & np.z), vr[3] ^ sr[3] ^ (mr & np.w));
          }
          break;
        }
#pragma unroll
        for (uint32_t q = 0; q + 1 < (uint32_t)H; ++q)
          if (q == k) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              stk[q][e] = PACKED && e == 3 ? ((sr[3] & kMaskLast) | (tr << 24)) : sr[e];
              stk[q][4 + e] = vr[e];
            }
            if constexpr (!PACKED) stk[q][8] = tr;
          }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          n[e] = PACKED && e == 3 ? ((sl[3] & kMaskLast) | (tl << 24)) : sl[e];
          n[4 + e] = vl[e];
        }
        if constexpr (!PACKED) n[8] = tl;
      }
    }
    // idle lanes have the last node's key and folded nothing
    if constexpr (OUT::kFold && KP::kPerLane) range_fold_keys(acc, key, reinterpret_cast<uint32_t*>(ys));
  }
  if constexpr (OUT::kFold && !KP::kPerLane) range_fold_wave(acc, reinterpret_cast<uint32_t*>(ys));
  if ((threadIdx.x & 63u) == 0 && nlive) atomicAdd(blocks, PRG::kBlocks * ((1u << H) - 1u) * nlive);
}

// Points x0 + i, i in [0, count), as N-byte big-endian strings: the
// add carries across all 16 low bytes; bytes above them come from `top` (the host splits a range
// at the one place where the low 128 bits wrap).
__global__ void k_range_points(const uint32_t nbytes, const RangeX x0, const RangeTop top, const uint64_t count,
                               uint8_t* __restrict__ xs) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const RangeX x = range_add(x0, i);
    uint8_t* o = xs + i * nbytes;
    for (uint32_t b = 0; b < nbytes; ++b) {
      const uint32_t pos = nbytes - 1u - b;  // significance of byte b
      o[b] = pos < 8u ? (uint8_t)(x.lo >> (8u * pos)) : (pos < 16u ? (uint8_t)(x.hi >> (8u * (pos - 8u))) : top.b[b]);
    }
  }
}

// Key `key` of a K-key correction-word block as a single-key block at `out` (np1 at byte `np1_off`
// of it) and its seed at s0_out: nlev rows of lam bytes of cw_s and cw_v, nlev bytes of cw_t.
__global__ void k_rangemk_gather(const uint8_t* __restrict__ cwb, const uint8_t* __restrict__ np1,
                                 const uint8_t* __restrict__ s0s, const uint64_t K, const uint64_t key,
                                 const uint32_t nlev, const uint32_t lam, const uint32_t np1_off,
                                 uint8_t* __restrict__ out, uint8_t* __restrict__ s0_out) {
  const uint32_t rows = nlev * lam;  // bytes of one key's cw_s (and cw_v)
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < 2u * rows + nlev + 2u * lam;
       i += gridDim.x * blockDim.x) {
    if (i < 2u * rows) {  // cw_s then cw_v: byte b of level lev
      const uint32_t part = i / rows, lev = (i % rows) / lam, b = i % lam;
      out[i] = cwb[((uint64_t)part * nlev * K + (uint64_t)lev * K + key) * lam + b];
    } else if (i < 2u * rows + nlev) {
      const uint32_t lev = i - 2u * rows;
      out[i] = cwb[2ull * nlev * K * lam + (uint64_t)lev * K + key];
    } else if (i < 2u * rows + nlev + lam) {
      const uint32_t b = i - (2u * rows + nlev);
      out[np1_off + b] = np1[key * lam + b];
    } else {
      const uint32_t b = i - (2u * rows + nlev + lam);
      s0_out[b] = s0s[key * lam + b];
    }
  }
}

// The fold of rows a range call has written (the shapes without a folding tail): for each of nk
// keys, out[key] ^= XOR over i < count of rows[key * count + i] & w[i], on rows of q uint4s
// (LAMBDA = 16 q).  A key's rows and the table are both count * q uint4s in the same order, so
// thread g of the S = stride threads of a grid row takes elements g, g + S, ... of both; S is a
// multiple of q, so they all lie in column g % q (the host keeps S >= q).  q a power of two up to
// 64: a workgroup starts at a multiple of 64, so lanes l and l ^ d share a column for d >= q, and
// the wave's partial sums meet in its lanes below q (the butterfly of range_fold_wave, stopped at
// q) before the atomic update; any other q: every thread updates `out` itself.  w null: no mask.
// `out` has been zeroed by the call.  blockIdx.y strides over the keys.
__global__ __launch_bounds__(256) void k_fold_rows(const uint4* __restrict__ rows, const uint4* __restrict__ w,
                                                   const uint32_t nk, const uint64_t count, const uint32_t q,
                                                   const uint32_t stride, uint32_t* __restrict__ out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n = count * q;
  const bool pow2 = q <= 64u && (q & (q - 1u)) == 0u;
  for (uint32_t key = blockIdx.y; key < nk; key += gridDim.y) {
    const uint4* r = rows + (uint64_t)key * n;
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    if (g < stride)
      for (uint64_t e = g; e < n; e += stride) {
        const uint4 y = r[e], m = w ? w[e] : make_uint4(~0u, ~0u, ~0u, ~0u);
        acc[0] ^= y.x & m.x;
        acc[1] ^= y.y & m.y;
        acc[2] ^= y.z & m.z;
        acc[3] ^= y.w & m.w;
      }
    if (pow2)
      for (uint32_t d = 32; d >= q; d >>= 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] ^= __shfl_xor(acc[e], d);
    if ((!pow2 || (threadIdx.x & 63u) < q) && (acc[0] | acc[1] | acc[2] | acc[3])) {
      uint32_t* o = out + 4ull * ((uint64_t)key * q + g % q);
#pragma unroll
      for (int e = 0; e < 4; ++e) atomicXor(o + e, acc[e]);
    }
  }
}

}  // namespace
