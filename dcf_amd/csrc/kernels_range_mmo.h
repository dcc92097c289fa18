// kernels_range_mmo.h — contiguous-range eval over the Matyas-Meyer-Oseas AES-128 PRG at
// LAMBDA = 16: the three stages of kernels_range.h (roots, breadth-first levels, register
// depth-first tail) as siblings of the Hirose kernels, on the same key policies (RangeOneKey,
// RangeKeys), block layout, 32-byte node rows, launch groups and clipping; range_group picks the set
// by the PRG.  Included by dcf_hip.hip only (after kernels_mmo.h and kernels_range.h).
//
// An MMO node costs four AES-128 blocks for both children (mmo_prg4), a walk step two (the side's
// s and v schedules, as mmo_eval_one): 4 blocks per output below the roots plus 2 (8N - h) per
// root.  Every kernel holds the T-tables and the four schedules in LDS, one workgroup per CU.
//
// Rows keep t in bit 24 of the seed's last word (bit 0 of byte 15), as the Hirose rows do: the PRG
// clears that bit in every child seed and cw_s is the XOR of two child seeds, so it is clear in
// every seed below the key's s0; v is not clean (cw_v carries beta), so t stays with s.  The caller
// keeps nwalk >= 1, so the raw s0 never lands in a row.
#pragma once

#include "aes_lds.h"
#include "kernels16.h"
#include "kernels_mmo.h"
#include "kernels_range.h"

namespace {

// Both children of (s, v, t) under the correction words of their level (lib.rs:176-189 with x bit
// 0 and 1, as k_fd_level16_mmo): four blocks.
__device__ __forceinline__ void mmo_children(const uint32_t* lds, uint32_t lc, const uint4* rks,
                                             const uint32_t (&csw)[4], const uint32_t (&cvw)[4], uint32_t ct,
                                             const uint32_t (&s)[4], const uint32_t (&v)[4], uint32_t t,
                                             uint32_t (&sl)[4], uint32_t (&vl)[4], uint32_t& tl, uint32_t (&sr)[4],
                                             uint32_t (&vr)[4], uint32_t& tr) {
  uint32_t o[4][4], tl0, tr0;
  mmo_prg4(lds, lc, rks, s, o, tl0, tr0);
  const uint32_t tm = 0u - t;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sl[k] = o[0][k] ^ (tm & csw[k]);
    vl[k] = v[k] ^ o[1][k] ^ (tm & cvw[k]);
    sr[k] = o[2][k] ^ (tm & csw[k]);
    vr[k] = v[k] ^ o[3][k] ^ (tm & cvw[k]);
  }
  tl = tl0 ^ (t & ct & 1u);
  tr = tr0 ^ (t & (ct >> 1) & 1u);
}

// Root r of `total` = keys * per, one lane each: the node of level `nwalk` of key kp.key(r) whose
// nwalk-bit prefix is pfx + kp.node(r), walked from (s0s[key], 0, party) with the two-block step of
// mmo_eval_one, bits Msb-first.  Waves take 64 roots at a time, the waves of different workgroups
// first, so a few hundred roots walk on as many CUs.  LEAF as k_range_roots16: false writes the row
// (s with t in bit 24 of word 3, then v) to out[2r], out[2r + 1]; true (nwalk = 8N, per = count)
// writes y = v ^ s ^ t * cw_np1 (lib.rs:192) to out[r].
// blocks: the call's AES block count (dcf_prg_last_eval_blocks), 2 per level and root.
template <bool LEAF, class KP>
__global__ __launch_bounds__(kBlock, 1) void k_range_roots16_mmo(
    const uint32_t* __restrict__ tab, const uint4* __restrict__ rk128, const uint4* __restrict__ cw_s,
    const uint4* __restrict__ cw_v, const uint8_t* __restrict__ cw_t, const uint4* __restrict__ cw_np1,
    const uint4* __restrict__ s0s, const KP kp, const uint32_t party, const RangeX pfx, const uint32_t nwalk,
    const typename KP::Idx total, uint4* __restrict__ out, unsigned long long* __restrict__ blocks) {
  using Idx = typename KP::Idx;
  __shared__ uint32_t lds[kLdsWords];
  __shared__ uint4 rks[4 * kMmoRk];
  lds_fill_rk128(rks, rk128);
  lds_fill_tables(lds, tab);  // its barrier also publishes rks
  const uint32_t lc = lane_const();
  uint32_t nlive = 0;  // roots this wave walked: one atomic per wave, after its last pass
  const uint64_t stride = 64ull * gridDim.x * (kBlock / 64);
  for (uint64_t base = 64ull * (blockIdx.x + (uint64_t)gridDim.x * (threadIdx.x >> 6)); base < total; base += stride) {
    const uint64_t r = base + (threadIdx.x & 63u);
    const bool live = r < total;
    const Idx rr = (Idx)(live ? r : total - 1u);
    nlive += (uint32_t)__popcll(__ballot(live));
    const uint32_t key = kp.key(rr);
    const RangeX p = range_add(pfx, kp.node(rr, key));
    const uint4 sv = s0s[key];
    uint32_t s[4] = {sv.x, sv.y, sv.z, sv.w}, v[4] = {0u, 0u, 0u, 0u}, t = party;
    for (uint32_t lev = 0; lev < nwalk; ++lev) {
      const uint32_t xb = range_bit(p, nwalk - 1u - lev);
      const uint4* const rk[2] = {rks + kMmoRk * (2u * xb), rks + kMmoRk * (2u * xb + 1u)};
      uint32_t st[2][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) st[0][j] = st[1][j] = s[j];
      if (DCF_MMO_PRIO) __builtin_amdgcn_s_setprio(1);
      aes128_tt<2>(st, rk, lds, lc);  // the side's s and v blocks
      if (DCF_MMO_PRIO) __builtin_amdgcn_s_setprio(0);
      uint32_t csw[4], cvw[4];
      const uint32_t ct = fd_cw(cw_s, cw_v, cw_t, kp.cw(lev, key), csw, cvw);
      const uint32_t tm = 0u - t;
      const uint32_t tn = ((st[0][0] ^ s[0]) & 1u) ^ (t & (ct >> xb) & 1u);  // lib.rs:179-180
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t msk = (j == 3) ? kMaskLast : 0xFFFFFFFFu;
        v[j] ^= ((st[1][j] ^ s[j]) & msk) ^ (tm & cvw[j]);  // lib.rs:182/186
        s[j] = ((st[0][j] ^ s[j]) & msk) ^ (tm & csw[j]);   // lib.rs:177-178, 183/187
      }
      t = tn;
    }
    if (!live) continue;
    if (LEAF) {
      const uint4 np = cw_np1[key];
      const uint32_t tm = 0u - t;
      out[r] = make_uint4(v[0] ^ s[0] ^ (tm & np.x), v[1] ^ s[1] ^ (tm & np.y), v[2] ^ s[2] ^ (tm & np.z),
                          v[3] ^ s[3] ^ (tm & np.w));
    } else {
      out[2ull * r] = make_uint4(s[0], s[1], s[2], (s[3] & kMaskLast) | (t << 24));
      out[2ull * r + 1u] = make_uint4(v[0], v[1], v[2], v[3]);
    }
  }
  if ((threadIdx.x & 63u) == 0 && nlive) atomicAdd(blocks, 2ull * nwalk * nlive);
}

// Interior, one launch per level (k_range_level16 with the MMO PRG): the parents of level `lev` —
// rows in[2j], in[2j + 1] of all blocks of all keys, consecutive in leaf order — become the children
// rows out[4j .. 4j + 3], one lane per parent, waves claiming units of parents from ctr[0].
// blocks: the call's AES block count, 4 per parent.
template <class KP>
__global__ __launch_bounds__(kBlock, 1) void k_range_level16_mmo(
    const uint32_t* __restrict__ tab, const uint4* __restrict__ rk128, const uint4* __restrict__ cw_s,
    const uint4* __restrict__ cw_v, const uint8_t* __restrict__ cw_t, const KP kp, const uint32_t lev,
    const uint32_t nparents, const uint4* __restrict__ in, uint4* __restrict__ out, uint32_t* __restrict__ ctr,
    unsigned long long* __restrict__ blocks) {
  __shared__ uint32_t lds[kLdsWords];
  __shared__ uint4 rks[4 * kMmoRk];
  lds_fill_rk128(rks, rk128);
  lds_fill_tables(lds, tab);
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
    mmo_children(lds, lc, rks, csw, cvw, ct, s, v, (a.w >> 24) & 1u, sl, vl, tl, sr, vr, tr);
    if (!live) continue;
    uint4* o = out + 4ull * j;
    o[0] = make_uint4(sl[0], sl[1], sl[2], (sl[3] & kMaskLast) | (tl << 24));
    o[1] = make_uint4(vl[0], vl[1], vl[2], vl[3]);
    o[2] = make_uint4(sr[0], sr[1], sr[2], (sr[3] & kMaskLast) | (tr << 24));
    o[3] = make_uint4(vr[0], vr[1], vr[2], vr[3]);
  }
  if ((threadIdx.x & 63u) == 0 && nlive) atomicAdd(blocks, 4ull * nlive);
}

// Tail: k_range_tail16's register depth-first expansion of the last H levels from the rows of
// level lev0 = 8N - H with the MMO PRG, one lane per node, waves claiming units of nodes from
// ctr[0].  Node j is node kp.node(j) of key kp.key(j); its leaves are g = (node << H) ..
// (node << H) + 2^H - 1 of that key, counted from the first root's first leaf; the range starts
// `skip` leaves in and holds `count`, so leaf g is the key's output g - skip, stored at
// ys[key * count + g - skip] only when g - skip is below count (32-bit: a launch covers at most
// 2^28 outputs; g < skip wraps far above).  The node and the stack slots stay in the rows' form for
// both key policies, 8 words with t in bit 24 of word 3.
// blocks: the call's AES block count, 4 (2^H - 1) per node — clipped leaves included.
template <int H, class KP>
__global__ __launch_bounds__(kBlock, 1) void k_range_tail16_mmo(
    const uint32_t* __restrict__ tab, const uint4* __restrict__ rk128, const uint4* __restrict__ cw_s,
    const uint4* __restrict__ cw_v, const uint8_t* __restrict__ cw_t, const uint4* __restrict__ cw_np1,
    const KP kp, const uint32_t lev0, const uint32_t nnodes, const uint4* __restrict__ rows, const uint32_t skip,
    const uint32_t count, uint4* __restrict__ ys, uint32_t* __restrict__ ctr,
    unsigned long long* __restrict__ blocks) {
  static_assert(H >= 2 && H <= 4, "register depth-first tail of 2..4 levels");
  __shared__ uint32_t lds[kLdsWords];
  __shared__ uint4 rks[4 * kMmoRk];
  lds_fill_rk128(rks, rk128);
  lds_fill_tables(lds, tab);
  const uint32_t lc = lane_const();
  const uint32_t unit = fd_unit(nnodes);
  uint32_t nlive = 0;  // nodes this wave expanded: one atomic per wave, after its last unit
  for (uint64_t base = next_unit_base_n(ctr, ~0ull, unit); base < nnodes;
       base = next_unit_base_n(ctr, base, unit)) {
    const uint32_t j = (uint32_t)base + (threadIdx.x & 63u);
    const bool live = j < nnodes;
    const uint32_t jj = live ? j : nnodes - 1u;
    nlive += (uint32_t)__popcll(__ballot(live));
    const uint32_t key = kp.key(jj);
    uint32_t stk[H - 1][8];  // pending right children, by depth
    uint32_t n[8];
    {
      const uint4 sv = rows[2ull * jj], vv = rows[2ull * jj + 1u];
      n[0] = sv.x; n[1] = sv.y; n[2] = sv.z; n[3] = sv.w;
      n[4] = vv.x; n[5] = vv.y; n[6] = vv.z; n[7] = vv.w;
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
            for (int e = 0; e < 8; ++e) n[e] = stk[q][e];
        k = d + 1u;
      }
      for (;; ++k) {  // expand depth k (level lev0 + k)
        uint32_t csw[4], cvw[4];
        const uint32_t ct = fd_cw(cw_s, cw_v, cw_t, kp.cw(lev0 + k, key), csw, cvw);
        const uint32_t s[4] = {n[0], n[1], n[2], n[3] & kMaskLast}, v[4] = {n[4], n[5], n[6], n[7]};
        uint32_t sl[4], vl[4], sr[4], vr[4], tl, tr;
        mmo_children(lds, lc, rks, csw, cvw, ct, s, v, (n[3] >> 24) & 1u, sl, vl, tl, sr, vr, tr);
        if (k + 1u == (uint32_t)H) {  // leaves 2i, 2i + 1 of the node: y = v ^ s ^ t * cw_np1 (lib.rs:192)
          const uint32_t ol = o0 + 2u * i, orr = ol + 1u;
          const uint32_t ml = 0u - tl, mr = 0u - tr;
          const uint4 np = cw_np1[key];
          uint4* const yk = ys + (uint64_t)key * count;
          if (ol < count)
            yk[ol] = make_uint4(vl[0] ^ sl[0] ^ (ml & np.x), vl[1] ^ sl[1] ^ (ml & np.y),
                                vl[2] ^ sl[2] ^ (ml & np.z), vl[3] ^ sl[3] ^ (ml & np.w));
          if (orr < count)
            yk[orr] = make_uint4(vr[0] ^ sr[0] ^ (mr & np.x), vr[1] ^ sr[1] ^ (mr & np.y),
                                 vr[2] ^ sr[2] ^ (mr & np.z), vr[3] ^ sr[3] ^ (mr & np.w));
          break;
        }
#pragma unroll
        for (uint32_t q = 0; q + 1 < (uint32_t)H; ++q)
          if (q == k) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              stk[q][e] = e == 3 ? ((sr[3] & kMaskLast) | (tr << 24)) : sr[e];
              stk[q][4 + e] = vr[e];
            }
          }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          n[e] = e == 3 ? ((sl[3] & kMaskLast) | (tl << 24)) : sl[e];
          n[4 + e] = vl[e];
        }
      }
    }
  }
  if ((threadIdx.x & 63u) == 0 && nlive) atomicAdd(blocks, 4ull * ((1u << H) - 1u) * nlive);
}

}  // namespace
