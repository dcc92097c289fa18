// kernels_range_mmo.h — contiguous-range eval over the Matyas-Meyer-Oseas AES-128 PRG at
// LAMBDA = 16: what the three stages of kernels_range.h (roots, breadth-first levels, register
// depth-first tail) need for it — mmo_children, the root walk k_range_roots16_mmo (another
// algorithm than the Hirose half-wave walk) and the PRG policy RangeMmo, under which
// k_range_level16 and k_range_tail16 run the MMO PRG on the same key policies (RangeOneKey,
// RangeKeys), block layout, 32-byte node rows, launch groups and clipping; range_group<PRG, KP> is
// the host side of both PRGs.  Included by dcf_hip.hip only (after kernels_mmo.h and kernels_range.h).
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

// Both children of (s, v, t) under the correction words of their level: four blocks, o = s_L, v_L,
// s_R, v_R of mmo_prg4 (already masked), then lib.rs:176-189 with x bit 0 and 1 and tm = t ? ~0 : 0:
//   s_l = o[0] ^ tm & cw_s    v_l = v ^ o[1] ^ tm & cw_v    t_l = t_L ^ t & cw_tl   (_r: o[2], o[3], t_R, cw_tr)
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

// The MMO PRG under k_range_level16 and k_range_tail16 (the members are described at RangeHirose):
// the four AES-128 schedules arrive as a device pointer and are staged into LDS, a node costs four
// blocks, and the tail keeps the packed 8-word node under both key policies.
struct RangeMmo {
  using Arg = const uint4*;
  static constexpr unsigned long long kBlocks = 4;
  static constexpr bool kPacked = true;
  static constexpr uint64_t kRootsPer = 64;  // one wave of lanes
  template <class Prg>
  static Arg arg(const Prg* p) { return p->d_rk128; }
  template <bool LEAF, class KP>
  static auto roots() { return k_range_roots16_mmo<LEAF, KP>; }
  static __device__ __forceinline__ const uint4* keys(const uint4* rk128) {
    __shared__ uint4 rks[4 * kMmoRk];
    lds_fill_rk128(rks, rk128);
    return rks;
  }
  template <class... A>
  static __device__ __forceinline__ void children(A&&... a) { mmo_children(a...); }
};

}  // namespace
