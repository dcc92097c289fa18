// kernels_range_wide.h — contiguous-range eval over the Hirose PRG at LAMBDA >= 32:
// ys[i] = Dcf::eval(b, k, x0 + i), i in [0, count), for one key, and ys[k * count + i] for the keys
// of a launch group over one range.  Included by dcf_hip.hip only (after kernels_range.h and
// kernels_wide_stream.h).
//
// The three stages of kernels_range.h over the LAMBDA >= 32 head state (kernels_wide.h): only bytes
// [0,32) of a node ever see AES, so a node is s[0:32), v[0:32), t — and the t bits of the levels
// between its block's root and itself, because bytes [32, LAMBDA) of a leaf's output are linear in
// its whole t-sequence.  A node's two children cost the four blocks A = E0(s_lo), B = E0(~s_lo),
// C = E17(s_hi), D = E17(~s_hi); every stage encrypts all four for every node it steps (the root
// walk too: one lane per root runs the four as one interleaved AES chain per level, where the
// direction's two or three blocks would save LDS reads that a root walk of a few waves does not
// miss).  The correction words come from the CW digest of k_cw_digest.
//
// Each kernel is a template on the key policy, as the stages of kernels_range.h are: RangeOneKey
// (uniform correction words, seed and cw_np1, loaded ahead of the work loop into scalars) or
// RangeDigKeys (below: the keys of a launch group one after another in every node buffer, each in
// leaf order, everything of the key a per-lane load inside the work loop).
//
// Node row (80 B, five uint4, the row of WidePrefix): s[0:32) | v[0:32) | {t, q0, q1, 0}.  q0 and
// q1 are words W0 and W0 + 1 of the leaf's t-vector row as far as they are known at this node,
// W0 = (8N - h + 1) >> 4 being the word of the first row below the block roots: the h <= 14 rows
// 8N - h + 1 .. 8N of the subtree lie in those two words (nibble format of kernels_wide.h: row r is
// bit 8 ((r >> 2) & 3) + (r & 3) of word r >> 4).  Words below W0 are the same for all 2^h leaves
// of a block and are kept per root (`tpre`, 64 B per root, words past the root's level zero).
//   k_range_roots_wide  the roots (level 8N - h, prefixes x0 >> h upwards) walked from
//                       (s0, 0, party), one lane per root, bits from the 128-bit pfx + root index;
//                       writes the node row and the root's t-vector prefix.  LEAF (h = 0): the
//                       roots are the points; it finishes with cw_np1 and writes y[0:32) and the
//                       complete t-vector row.
//   k_range_level_wide  one breadth-first level: parents in[5j ..], children out[10j ..], one lane
//                       per parent, waves claiming units of parents from ctr[0].
//   k_range_tail_wide   register depth-first tail over the last H levels: leaf g of the launch is
//                       output g - skip, stored only below count: y[0:32) at ys + o * LAMBDA and,
//                       when LAMBDA > 32, the t-vector row o (the root's prefix with words W0,
//                       W0 + 1 from the leaf) — the row k_eval_wide_head_stream writes for that
//                       point, for k_eval_wide_tail / k_eval_wide_tail2 to turn into y[32, LAMBDA).
// Every t-vector row is written as whole uint4s, zero past row 8N.  All node, root and output
// indices of a launch are 32-bit (the host keeps a launch group <= 2^28 outputs; a group of several
// keys <= 2^22 leaves, clipped ones included).  blocks: the call's AES-256 block count, 4 per stepped
// node, one atomic per wave.
// MASK (LAMBDA = 32: no t-vectors) is chosen once per call on the host (range_wide_group<MASK>),
// which takes a group's blocks from the same range_geom as the LAMBDA = 16 path.
#pragma once

#include "aes_lds.h"
#include "kernels_range.h"
#include "kernels_wide.h"
#include "kernels_wide_stream.h"

namespace {

// Register depth of the tail.  A wide node is 19 words (s, v, t, q0, q1) where the LAMBDA = 16
// node is 9, so two levels (one stacked node, 38 words of tree state) take the registers that four
// take there; three levels (57 words) spill at 128 VGPRs.  DCF_RANGE_WIDE_TAIL: A/B knob.
#ifndef DCF_RANGE_WIDE_TAIL
#define DCF_RANGE_WIDE_TAIL 2
#endif
constexpr uint32_t kRangeWideTail = DCF_RANGE_WIDE_TAIL;
// Under per-lane keys the correction words of a level are 17 VGPRs where one key's are scalars, and
// the two-level tail spills (8 to 14 VGPRs in every form tried: the digest row loaded behind the
// blocks, the node's placement formed again at the leaves, 32-bit digest offsets).  Without the
// stacked node it does not: the groups of several keys run one breadth-first level more and a
// tail of one level, the two leaves of a node.
constexpr uint32_t kRangeWideTailKeys = 1;
constexpr uint32_t kRwWords = 19;  // s[8] | v[8] | t | q0 | q1

// RangeKeys for the key-major CW digest k_cw_digest writes for the nk keys of a launch group:
// cw(lev, key) is the digest row key * nlev + lev (dig[4 row + q], dig_t[row]; 4 row < 2^32 is the
// host's bound on a group's keys).  Seeds and cw_np1 are read at [key], LAMBDA bytes apart.
struct RangeDigKeys {
  static constexpr bool kPerLane = true;
  uint32_t nlev;
  RangeDiv per;
  static RangeDigKeys make(uint64_t nlev, uint32_t per) { return {(uint32_t)nlev, range_div_make(per)}; }
  __device__ __forceinline__ uint32_t key(uint32_t j) const { return range_div(per, j); }
  __device__ __forceinline__ uint32_t node(uint32_t j, uint32_t key) const { return j - key * per.d; }
  __device__ __forceinline__ uint32_t cw(uint32_t lev, uint32_t key) const { return key * nlev + lev; }
};

// The four blocks of a node: st = A = E0(s_lo), B = E0(~s_lo), C = E17(s_hi), D = E17(~s_hi).
// QUAD: one interleaved chain of four (latency: the root walk, the level kernel); else A, B then
// C, D (half the AES state in registers: the tail).
template <bool QUAD>
__device__ __forceinline__ void rw_blocks(const uint32_t* lds, const uint32_t lc, const uint32_t rks_a,
                                          const uint32_t* n, uint32_t (&st)[4][4]) {
  // the empty asm makes the schedules' address opaque per call: the round keys are loop-invariant
  // LDS reads otherwise, and hoisting them out of a level loop takes 120 VGPRs (spills)
  uint32_t kb = rks_a;
  asm volatile("" : "+v"(kb));
  if (QUAD) {
    const uint32_t ka[4] = {kb, kb, kb + 368u, kb + 368u};  // cipher 17 sits 23 slots on
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      st[0][j] = n[j];
      st[1][j] = ~n[j];
      st[2][j] = n[4 + j];
      st[3][j] = ~n[4 + j];
    }
    aes_tt_lka<14, 4, false>(st, ka, lds, lc);
  } else {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      uint32_t w[2][4];
      if (h) asm volatile("" : "+v"(kb) : "v"(st[0][0]));  // C, D after A, B: their keys are read then
      const uint32_t ka[2] = {kb + 368u * h, kb + 368u * h};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[0][j] = n[4 * h + j];
        w[1][j] = ~n[4 * h + j];
      }
      aes_tt_lka<14, 2, false>(w, ka, lds, lc);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        st[2 * h][j] = w[0][j];
        st[2 * h + 1][j] = w[1][j];
      }
    }
  }
}

// LATE (per-lane correction words: they are VGPRs, 17 of them, where a uniform key's are scalars):
// the four blocks first, and the digest row `c` made to depend on their last word, so that the
// compiler cannot issue the row's loads ahead of the AES chain and hold them across it — the
// chain is where the kernels' register demand peaks.
template <bool QUAD>
__device__ __forceinline__ void rw_blocks_first(const uint32_t* lds, const uint32_t lc, const uint32_t rks_a,
                                                const uint32_t* n, uint32_t (&st)[4][4], uint32_t& c) {
  rw_blocks<QUAD>(lds, lc, rks_a, n, st);
  asm volatile("" : "+v"(c) : "v"(st[3][3]));
}

// uint4 q of digest row c.  LATE: the byte offset 64 c + 16 q is formed in 32 bits (the host keeps a
// group's digest below 2^32 bytes), which leaves the address one register on top of a scalar base.
template <bool LATE>
__device__ __forceinline__ uint4 rw_dig(const uint4* __restrict__ dig, const uint32_t c, const uint32_t q) {
  if constexpr (LATE) return *reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(dig) + (64u * c + 16u * q));
  else return dig[4u * c + q];
}

// Both children of a node at level `lev` from the four blocks, bytes [0,32) exactly as
// k_eval_wide_head_stream steps them (prg.rs:42-73, lib.rs:177-180); MASK: LAMBDA == 32, byte 31 holds
// the bit the PRG clears.  n / l / r: kRwWords words each (l may be n); words 17 and 18 (q0, q1) are the
// caller's.  Here and in rw_step / rw_leaves `lev` only names the digest row: KP::cw(level, key).
template <bool MASK, bool QUAD, bool LATE = false>
__device__ __forceinline__ void rw_children(const uint32_t* lds, const uint32_t lc, const uint32_t rks_a,
                                            const uint4* __restrict__ dig, const uint8_t* __restrict__ dig_t,
                                            const uint32_t lev, const uint32_t* n, uint32_t* l, uint32_t* r) {
  uint32_t st[4][4];
  uint32_t c = lev;
  if constexpr (LATE) rw_blocks_first<QUAD>(lds, lc, rks_a, n, st, c);
  const uint4 c0 = rw_dig<LATE>(dig, c, 0u), c1 = rw_dig<LATE>(dig, c, 1u), c2 = rw_dig<LATE>(dig, c, 2u), c3 = rw_dig<LATE>(dig, c, 3u);
  const uint32_t ct = dig_t[c];
  const uint32_t csw[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const uint32_t cvw[8] = {c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
  if constexpr (!LATE) rw_blocks<QUAD>(lds, lc, rks_a, n, st);
  const uint32_t t = n[16], tm = 0u - t;
  const uint32_t tl = ((st[0][0] ^ n[0]) & 1u) ^ (t & ct & 1u);           // lsb(A ^ s)[0]
  const uint32_t tr = ((st[1][0] ^ ~n[0]) & 1u) ^ (t & (ct >> 1) & 1u);   // lsb(B ^ ~s)[0]
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t m = (MASK && j == 3) ? kMaskLast : 0xFFFFFFFFu;
    const uint32_t slo = n[j], shi = n[4 + j], vlo = n[8 + j], vhi = n[12 + j];
    const uint32_t xs_lo = tm & csw[j], xs_hi = tm & csw[4 + j], xv_lo = tm & cvw[j], xv_hi = tm & cvw[4 + j];
    l[j] = st[0][j] ^ slo ^ xs_lo;                       // s_L[0:16) = A ^ s
    r[j] = slo ^ xs_lo;                                  // s_R[0:16) = s
    l[8 + j] = vlo ^ st[1][j] ^ ~slo ^ xv_lo;            // v ^= B ^ ~s
    r[8 + j] = vlo ^ ~slo ^ xv_lo;                       // v ^= ~s
    l[4 + j] = (shi & m) ^ xs_hi;                        // s_L[16:32) = s
    r[4 + j] = ((st[2][j] ^ shi) & m) ^ xs_hi;           // s_R[16:32) = C ^ s
    l[12 + j] = vhi ^ (~shi & m) ^ xv_hi;                // v ^= ~s
    r[12 + j] = vhi ^ ((st[3][j] ^ ~shi) & m) ^ xv_hi;   // v ^= D ^ ~s
  }
  l[16] = tl;
  r[16] = tr;
}

// One step of a walk: node n (words 0 .. 16) becomes its left or right child, in place.
template <bool MASK, bool LATE = false>
__device__ __forceinline__ void rw_step(const uint32_t* lds, const uint32_t lc, const uint32_t rks_a,
                                        const uint4* __restrict__ dig, const uint8_t* __restrict__ dig_t,
                                        const uint32_t lev, uint32_t* n, const bool right) {
  uint32_t st[4][4];
  uint32_t c = lev;
  if constexpr (LATE) rw_blocks_first<true>(lds, lc, rks_a, n, st, c);
  const uint4 c0 = rw_dig<LATE>(dig, c, 0u), c1 = rw_dig<LATE>(dig, c, 1u), c2 = rw_dig<LATE>(dig, c, 2u), c3 = rw_dig<LATE>(dig, c, 3u);
  const uint32_t ct = dig_t[c];
  const uint32_t csw[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const uint32_t cvw[8] = {c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
  if constexpr (!LATE) rw_blocks<true>(lds, lc, rks_a, n, st);
  const uint32_t t = n[16], tm = 0u - t, rm = right ? 0xFFFFFFFFu : 0u;
  n[16] = (((right ? st[1][0] ^ ~n[0] : st[0][0] ^ n[0])) & 1u) ^ (t & (ct >> (rm & 1u)) & 1u);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t m = (MASK && j == 3) ? kMaskLast : 0xFFFFFFFFu;
    const uint32_t slo = n[j], shi = n[4 + j];
    n[j] = slo ^ (~rm & st[0][j]) ^ (tm & csw[j]);                                       // left: A ^ s
    n[8 + j] ^= ~slo ^ (~rm & st[1][j]) ^ (tm & cvw[j]);                                 // left: B ^ ~s
    n[4 + j] = ((shi ^ (rm & st[2][j])) & m) ^ (tm & csw[4 + j]);                        // right: C ^ s
    n[12 + j] ^= ((~shi ^ (rm & st[3][j])) & m) ^ (tm & cvw[4 + j]);                     // right: D ^ ~s
  }
}

// The two leaves under a node of the last level `lev`: y[0:32) = v ^ s ^ t * cw_np1 (lib.rs:192) of
// each child and its t, without forming the children (s ^ ~s cancels: 18 words out instead of 34).
template <bool MASK, bool LATE = false>
__device__ __forceinline__ void rw_leaves(const uint32_t* lds, const uint32_t lc, const uint32_t rks_a,
                                          const uint4* __restrict__ dig, const uint8_t* __restrict__ dig_t,
                                          const uint32_t lev, const uint32_t* n, const uint32_t (&np)[8],
                                          uint32_t (&yl)[8], uint32_t (&yr)[8], uint32_t& tl, uint32_t& tr) {
  uint32_t st[4][4];
  uint32_t c = lev;
  if constexpr (LATE) rw_blocks_first<false>(lds, lc, rks_a, n, st, c);
  const uint4 c0 = rw_dig<LATE>(dig, c, 0u), c1 = rw_dig<LATE>(dig, c, 1u), c2 = rw_dig<LATE>(dig, c, 2u), c3 = rw_dig<LATE>(dig, c, 3u);
  const uint32_t ct = dig_t[c];
  const uint32_t cw[8] = {c0.x ^ c2.x, c0.y ^ c2.y, c0.z ^ c2.z, c0.w ^ c2.w,
                          c1.x ^ c3.x, c1.y ^ c3.y, c1.z ^ c3.z, c1.w ^ c3.w};  // cw_s ^ cw_v
  if constexpr (!LATE) rw_blocks<false>(lds, lc, rks_a, n, st);
  const uint32_t t = n[16], tm = 0u - t;
  tl = ((st[0][0] ^ n[0]) & 1u) ^ (t & ct & 1u);
  tr = ((st[1][0] ^ ~n[0]) & 1u) ^ (t & (ct >> 1) & 1u);
  const uint32_t ml = 0u - tl, mr = 0u - tr;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t m = (MASK && j == 3) ? kMaskLast : 0xFFFFFFFFu;
    // s_L ^ v_L = (A ^ s) ^ (v ^ B ^ ~s), s_R ^ v_R = s ^ (v ^ ~s) on [0:16); on [16:32) the same with
    // C, D and the sides swapped, under the mask; both ^ t (cw_s ^ cw_v)
    const uint32_t lo = ~n[8 + j] ^ (tm & cw[j]), hi = n[12 + j] ^ (tm & cw[4 + j]);
    yl[j] = lo ^ st[0][j] ^ st[1][j] ^ (ml & np[j]);
    yr[j] = lo ^ (mr & np[j]);
    yl[4 + j] = hi ^ m ^ (ml & np[4 + j]);
    yr[4 + j] = hi ^ (~(st[2][j] ^ st[3][j]) & m) ^ (mr & np[4 + j]);
  }
}

// Row `row` (lev + 1) of the t-vector into the node's words q0 / q1 (word (row >> 4) - w0 of the two).
__device__ __forceinline__ void rw_tbit(uint32_t* nd, const uint32_t row, const uint32_t w0, const uint32_t q0,
                                        const uint32_t q1) {
  const uint32_t bit = nd[16] << (8u * ((row >> 2) & 3u) + (row & 3u));
  const bool hi = (row >> 4) != w0;  // uniform
  nd[17] = hi ? q0 : q0 | bit;
  nd[18] = hi ? q1 | bit : q1;
}

__device__ __forceinline__ void rw_load(uint32_t* n, const uint4* __restrict__ row) {
  const uint4 a = row[0], b = row[1], c = row[2], d = row[3], e = row[4];
  n[0] = a.x; n[1] = a.y; n[2] = a.z; n[3] = a.w; n[4] = b.x; n[5] = b.y; n[6] = b.z; n[7] = b.w;
  n[8] = c.x; n[9] = c.y; n[10] = c.z; n[11] = c.w; n[12] = d.x; n[13] = d.y; n[14] = d.z; n[15] = d.w;
  n[16] = e.x; n[17] = e.y; n[18] = e.z;
}
__device__ __forceinline__ void rw_store(uint4* __restrict__ row, const uint32_t* n) {
  row[0] = make_uint4(n[0], n[1], n[2], n[3]);
  row[1] = make_uint4(n[4], n[5], n[6], n[7]);
  row[2] = make_uint4(n[8], n[9], n[10], n[11]);
  row[3] = make_uint4(n[12], n[13], n[14], n[15]);
  row[4] = make_uint4(n[16], n[17], n[18], 0u);
}

// y[0:32) = v ^ s ^ t * cw_np1 (lib.rs:192) of leaf `n` to y4.
__device__ __forceinline__ void rw_leaf_y(uint4* __restrict__ y4, const uint32_t* n, const uint4 np0, const uint4 np1) {
  const uint32_t tn = 0u - n[16];
  y4[0] = make_uint4(n[8] ^ n[0] ^ (tn & np0.x), n[9] ^ n[1] ^ (tn & np0.y), n[10] ^ n[2] ^ (tn & np0.z),
                     n[11] ^ n[3] ^ (tn & np0.w));
  y4[1] = make_uint4(n[12] ^ n[4] ^ (tn & np1.x), n[13] ^ n[5] ^ (tn & np1.y), n[14] ^ n[6] ^ (tn & np1.z),
                     n[15] ^ n[7] ^ (tn & np1.w));
}

#define DCF_RW_PROLOGUE()                                                                       \
  __shared__ uint32_t lds[kLdsWords];                                                           \
  __shared__ uint4 rks[23 + 15]; /* cipher 0 at slot 0, cipher 17 at slot 23 (k_wpfx_build) */  \
  if (threadIdx.x < 30) rks[threadIdx.x < 15 ? threadIdx.x : threadIdx.x + 8] = rk2[threadIdx.x]; \
  lds_fill_tables(lds, tab); /* its barrier publishes rks */                                    \
  const uint32_t rks_a = (uint32_t)(size_t)(__attribute__((address_space(3))) uint4*)rks;       \
  const uint32_t lc = lane_const()

// Root r of `total` = keys * per: the node of level `nwalk` of key kp.key(r) whose nwalk-bit prefix
// is pfx + kp.node(r), one lane per root, waves taking 64 roots at a time in grid order, walked from
// that key's seed (s0 and cw_np1 start at the group's first key).  Row r of `nodes`, and
// (trows != null) its t-vector prefix to row r of trows: rows 0 .. nwalk, the remaining words zero.
// LEAF (nwalk = 8N, pfx = the first point, per = count, so r = key * count + i): no node row;
// y[0:32) to ys + r * lam, and trows is the launch's t-vector buffer.
template <bool LEAF, bool MASK, class KP>
__global__ __launch_bounds__(kBlock, 1) void k_range_roots_wide(
    const uint32_t* __restrict__ tab, const uint4* __restrict__ rk2, const uint4* __restrict__ dig,
    const uint8_t* __restrict__ dig_t, const uint4* __restrict__ cw_np1, const uint4* __restrict__ s0, const KP kp,
    const uint32_t party, const RangeX pfx, const uint32_t nwalk, const uint32_t total, uint4* __restrict__ nodes,
    uint32_t* __restrict__ trows, uint8_t* __restrict__ ys, const uint32_t lam,
    unsigned long long* __restrict__ blocks) {
  DCF_RW_PROLOGUE();
  const uint32_t kq = lam >> 4;  // uint4s between two keys' seeds (and cw_np1s)
  uint4 sa, sb;
  if constexpr (!KP::kPerLane) sa = s0[0], sb = s0[1];
  uint32_t nlive = 0;
  const uint32_t stride = gridDim.x * (kBlock / 64u) * 64u;
  for (uint32_t base = (blockIdx.x + gridDim.x * (threadIdx.x >> 6)) * 64u; base < total; base += stride) {
    const uint32_t r = base + (threadIdx.x & 63u);
    const bool live = r < total;
    nlive += (uint32_t)__popcll(__ballot(live));
    const uint32_t rr = live ? r : total - 1u;
    const uint32_t key = kp.key(rr);
    const RangeX p = range_add(pfx, kp.node(rr, key));
    uint32_t* trow = trows ? trows + (uint64_t)rr * kTWords : nullptr;
    if constexpr (KP::kPerLane) sa = s0[key * kq], sb = s0[key * kq + 1u];
    uint32_t n[kRwWords] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, party, 0u, 0u};
    uint32_t tacc = party;  // row 0 of the t-vector is t_0 = party
    for (uint32_t lev = 0; lev < nwalk; ++lev) {
      rw_step<MASK, KP::kPerLane>(lds, lc, rks_a, dig, dig_t, (uint32_t)kp.cw(lev, key), n, range_bit(p, nwalk - 1u - lev) != 0u);
      const uint32_t row = lev + 1u;
      tacc |= n[16] << (8u * ((row >> 2) & 3u) + (row & 3u));
      if ((row & 15u) == 15u) {  // word row >> 4 is complete
        if (trow && live) trow[row >> 4] = tacc;
        tacc = 0u;
      }
    }
    if (trow && live) {
      uint32_t w = nwalk >> 4;
      if ((nwalk & 15u) != 15u) trow[w] = tacc;
      for (++w; w < (uint32_t)kTWords; ++w) trow[w] = 0u;
    }
    if (!live) continue;
    if (LEAF) {
      const uint4* np = KP::kPerLane ? cw_np1 + key * kq : cw_np1;
      rw_leaf_y(reinterpret_cast<uint4*>(ys + (uint64_t)r * lam), n, np[0], np[1]);
    } else {
      n[17] = tacc;  // word (nwalk + 1) >> 4 so far (zero when the walk just completed a word)
      n[18] = 0u;
      rw_store(nodes + 5ull * r, n);
    }
  }
  if ((threadIdx.x & 63u) == 0 && nlive) atomicAdd(blocks, 4ull * nwalk * nlive);
}

// One breadth-first level: the parents of level `lev`, rows in[5j ..] of all blocks of all keys in
// leaf order (parent j: key kp.key(j)), become the children rows out[10j ..], out[10j + 5 ..].
// w0: the t-vector word of q0.
template <bool MASK, class KP>
__global__ __launch_bounds__(kBlock, 1) void k_range_level_wide(
    const uint32_t* __restrict__ tab, const uint4* __restrict__ rk2, const uint4* __restrict__ dig,
    const uint8_t* __restrict__ dig_t, const KP kp, const uint32_t lev, const uint32_t w0, const uint32_t nparents,
    const uint4* __restrict__ in, uint4* __restrict__ out, uint32_t* __restrict__ ctr,
    unsigned long long* __restrict__ blocks) {
  DCF_RW_PROLOGUE();
  const uint32_t unit = fd_unit(nparents);
  uint32_t nlive = 0;
  for (uint64_t base = next_unit_base_n(ctr, ~0ull, unit); base < nparents;
       base = next_unit_base_n(ctr, base, unit)) {
    const uint32_t j = (uint32_t)base + (threadIdx.x & 63u);
    const bool live = j < nparents;
    nlive += (uint32_t)__popcll(__ballot(live));
    uint32_t n[kRwWords], l[kRwWords], r[kRwWords];
    const uint32_t jj = live ? j : nparents - 1u;
    rw_load(n, in + 5ull * jj);
    rw_children<MASK, true>(lds, lc, rks_a, dig, dig_t, (uint32_t)kp.cw(lev, kp.key(jj)), n, l, r);
    rw_tbit(l, lev + 1u, w0, n[17], n[18]);
    rw_tbit(r, lev + 1u, w0, n[17], n[18]);
    if (!live) continue;
    rw_store(out + 10ull * j, l);
    rw_store(out + 10ull * j + 5u, r);
  }
  if ((threadIdx.x & 63u) == 0 && nlive) atomicAdd(blocks, 4ull * nlive);
}

// Tail: register depth-first expansion of the last H levels from the rows of level lev0 = 8N - H,
// one lane per node (the stack logic of k_range_tail16).  Node j's leaves are g = (j << H) ..
// + 2^H - 1, counted from the first root's first leaf; leaf g is output g - skip, stored only below
// count (32-bit: g < skip wraps far above).  tvec != null (LAMBDA > 32): row o of tvec gets the
// leaf's t-vector, nq uint4s: the prefix of its root (row j >> rsh of tpre) with words w0, w0 + 1
// from the leaf.  Several keys (kp): node j is node kp.node(j) of key kp.key(j), its leaves are
// counted within that key, and the key's output o is row key * count + o of ys and of tvec; the
// nodes being key-major, j >> rsh is row key * nroots + root of tpre as the roots kernel wrote it.
// The digest rows and cw_np1 of the lane's key are loaded where they are used, level by level, never
// held across a level (19-word nodes leave no registers for them).
template <int H, bool MASK, class KP>
__global__ __launch_bounds__(kBlock, 1) void k_range_tail_wide(
    const uint32_t* __restrict__ tab, const uint4* __restrict__ rk2, const uint4* __restrict__ dig,
    const uint8_t* __restrict__ dig_t, const uint4* __restrict__ cw_np1, const KP kp, const uint32_t lev0,
    const uint32_t w0, const uint32_t nnodes, const uint4* __restrict__ rows, const uint32_t skip, const uint32_t count,
    uint8_t* __restrict__ ys, const uint32_t lam, uint4* __restrict__ tvec, const uint4* __restrict__ tpre,
    const uint32_t rsh, const uint32_t nq, uint32_t* __restrict__ ctr, unsigned long long* __restrict__ blocks) {
  static_assert(H >= (KP::kPerLane ? 1 : 2) && H <= 4, "register depth-first tail of 2..4 levels (per-lane keys: from 1)");
  DCF_RW_PROLOGUE();
  const uint32_t unit = fd_unit(nnodes);
  uint32_t nlive = 0;
  uint32_t np[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if constexpr (!KP::kPerLane) {
    const uint4 np0 = cw_np1[0], np1 = cw_np1[1];
    np[0] = np0.x; np[1] = np0.y; np[2] = np0.z; np[3] = np0.w;
    np[4] = np1.x; np[5] = np1.y; np[6] = np1.z; np[7] = np1.w;
  }
  // leaf at output o of the key whose outputs start at row ob: y[0:32) and the t-vector row (its
  // root's prefix, words w0 and w0 + 1 = q0, q1)
  auto leaf = [&](const uint32_t ob, const uint32_t oo, const uint32_t (&y)[8], const uint32_t q0, const uint32_t q1,
                  const uint32_t root) {
    if (oo >= count) return;
    const uint32_t o = ob + oo;
    uint4* y4 = reinterpret_cast<uint4*>(ys + (uint64_t)o * lam);
    y4[0] = make_uint4(y[0], y[1], y[2], y[3]);
    y4[1] = make_uint4(y[4], y[5], y[6], y[7]);
    if (tvec == nullptr) return;
    for (uint32_t q = 0; q < nq; ++q) {
      uint4 p = tpre[4ull * root + q];
      const uint32_t b = 4u * q;  // uniform selects
      p.x = b == w0 ? q0 : (b == w0 + 1u ? q1 : p.x);
      p.y = b + 1u == w0 ? q0 : (b == w0 ? q1 : p.y);
      p.z = b + 2u == w0 ? q0 : (b + 1u == w0 ? q1 : p.z);
      p.w = b + 3u == w0 ? q0 : (b + 2u == w0 ? q1 : p.w);
      tvec[4ull * o + q] = p;
    }
  };
  for (uint64_t base = next_unit_base_n(ctr, ~0ull, unit); base < nnodes;
       base = next_unit_base_n(ctr, base, unit)) {
    const uint32_t j = (uint32_t)base + (threadIdx.x & 63u);
    const bool live = j < nnodes;
    const uint32_t jj = live ? j : nnodes - 1u;
    nlive += (uint32_t)__popcll(__ballot(live));
    uint32_t stk[H > 1 ? H - 1 : 1][kRwWords];  // pending right children, by depth (H = 1: none)
    uint32_t n[kRwWords];
    rw_load(n, rows + 5ull * jj);
    // Where node jv's outputs go: its key, the row of the key's first output, the output of the
    // node's first leaf within the key (idle lanes: none) and the row of its root's prefix.
    struct Where {
      uint32_t key, ob, o0, root;
    };
    const auto where = [&](const uint32_t jv) {
      const uint32_t key = kp.key(jv);
      return Where{key, KP::kPerLane ? key * count : 0u,
                   live ? ((uint32_t)kp.node(jv, key) << H) - skip : 0x80000000u, jv >> rsh};
    };
    // One key: held across the node.  Per-lane keys: only jj is; the rest is formed again from it
    // behind the last blocks, where the registers are free (rw_blocks_first).
    Where wh = where(jj);
    for (uint32_t i = 0; i < (1u << (H - 1)); ++i) {
      uint32_t k = 0;
      if (i) {  // resume at the right child saved at depth H - 2 - ctz(i) (wave-uniform)
        const uint32_t d = (uint32_t)(H - 2) - (uint32_t)__builtin_ctz(i);
#pragma unroll
        for (uint32_t q = 0; q + 1 < (uint32_t)H; ++q)
          if (q == d)
#pragma unroll
            for (uint32_t e = 0; e < kRwWords; ++e) n[e] = stk[q][e];
        k = d + 1u;
      }
      for (;; ++k) {  // expand depth k (level lev0 + k)
        if (k + 1u == (uint32_t)H) {  // leaves 2i, 2i + 1 of the node
          uint32_t yl[8], yr[8], tt[2][kRwWords];
          rw_leaves<MASK, KP::kPerLane>(lds, lc, rks_a, dig, dig_t, (uint32_t)kp.cw(lev0 + k, kp.key(jj)), n, np, yl, yr, tt[0][16], tt[1][16]);
          if constexpr (KP::kPerLane) {  // np was zero: the key's cw_np1 now, loaded behind the blocks as the digest row is
            uint32_t jv = jj;
            asm volatile("" : "+v"(jv) : "v"(yl[0]));
            wh = where(jv);
            const uint32_t a = wh.key * (lam >> 4);  // lam / 16 uint4s between two keys' cw_np1s
            const uint4 np0 = cw_np1[a], np1 = cw_np1[a + 1u];
            const uint32_t npk[8] = {np0.x, np0.y, np0.z, np0.w, np1.x, np1.y, np1.z, np1.w};
            const uint32_t ml = 0u - tt[0][16], mr = 0u - tt[1][16];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              yl[e] ^= ml & npk[e];
              yr[e] ^= mr & npk[e];
            }
          }
          rw_tbit(tt[0], lev0 + k + 1u, w0, n[17], n[18]);
          rw_tbit(tt[1], lev0 + k + 1u, w0, n[17], n[18]);
          leaf(wh.ob, wh.o0 + 2u * i, yl, tt[0][17], tt[0][18], wh.root);
          leaf(wh.ob, wh.o0 + 2u * i + 1u, yr, tt[1][17], tt[1][18], wh.root);
          break;
        }
        uint32_t l[kRwWords], r[kRwWords];
        rw_children<MASK, false, KP::kPerLane>(lds, lc, rks_a, dig, dig_t, (uint32_t)kp.cw(lev0 + k, kp.key(jj)), n, l, r);
        rw_tbit(l, lev0 + k + 1u, w0, n[17], n[18]);
        rw_tbit(r, lev0 + k + 1u, w0, n[17], n[18]);
#pragma unroll
        for (uint32_t q = 0; q + 1 < (uint32_t)H; ++q)
          if (q == k)
#pragma unroll
            for (uint32_t e = 0; e < kRwWords; ++e) stk[q][e] = r[e];
#pragma unroll
        for (uint32_t e = 0; e < kRwWords; ++e) n[e] = l[e];
      }
    }
  }
  if ((threadIdx.x & 63u) == 0 && nlive) atomicAdd(blocks, 4ull * ((1u << H) - 1u) * nlive);
}

#undef DCF_RW_PROLOGUE

}  // namespace
