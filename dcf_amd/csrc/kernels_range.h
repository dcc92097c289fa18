// kernels_range.h — contiguous-range eval: ys[i] = Dcf::eval(b, k, x0 + i), i in [0, count).
// Included by dcf_hip.hip only (after kernels16.h and kernels_lat.h).
//
// Consecutive points share almost their whole GGM path, so the Hirose LAMBDA = 16 path covers the
// range by the aligned blocks of 2^h leaves that intersect it and expands each block's subtree
// once: 2 AES blocks per output instead of 16N per point (DESIGN.md "Range eval").
//   k_range_roots16   the roots of those blocks — the nodes of level 8N - h whose prefixes run
//                     from x0 >> h upwards — each walked from s0 on a 32-lane half-wave (RowPrg, as
//                     k_prefix_build16's root path); the path bits come from the 128-bit value
//                     prefix + root index.  h = 0: the "roots" are the points themselves and the
//                     kernel writes y (small counts).
//   k_range_level16   the h - kRangeTail levels below the roots, breadth-first over all blocks at
//                     once, one launch per level (as k_fd_level16, on 32-byte rows): the nodes of
//                     all blocks stay consecutive, in leaf order, in two ping-pong buffers.
//   k_range_tail16    the register depth-first tail of k_fd_dfs16 on those nodes; a leaf's output
//                     index is its distance from x0 and leaves outside the range are not stored.
//   k_range_points    the points x0 + i as N-byte big-endian strings, for the PRGs / LAMBDA without
//                     a tree-sharing path (the existing eval runs on them).
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

constexpr uint32_t kRangeTail = 4;   // depth-first register tail (kFdTail)
constexpr uint32_t kRangeMaxH = 14;  // at most 10 breadth-first levels above the tail
constexpr uint32_t kRangeTopMax = 240;  // bytes of x above the low 16 (N <= 256)

// Bytes [0, N - 16) of a point wider than 128 bits (big-endian, as given): constant over a launch.
struct RangeTop {
  uint8_t b[kRangeTopMax];
};

// Root r (32 lanes each) is the node of level `nwalk` whose nwalk-bit prefix is pfx + r: walked
// from (s0, 0, party) with RowPrg, bits Msb-first.  LEAF = false: PrefixTable-style row (s with t
// in bit 0 of byte 15, then v) to out[2r], out[2r + 1]; the caller keeps nwalk >= 1, so s is
// masked there.  LEAF = true (nwalk = 8N): y = v ^ s ^ t * cw_np1 (lib.rs:192) to out[r].
// blocks: the call's AES block count (dcf_prg_last_eval_blocks), 2 per level and root.
template <bool LEAF>
__global__ __launch_bounds__(kBlock, 1) void k_range_roots16(
    const uint32_t* __restrict__ tab, const RoundKeys rk, const uint4* __restrict__ cw_s,
    const uint4* __restrict__ cw_v, const uint8_t* __restrict__ cw_t, const uint4* __restrict__ cw_np1,
    const uint4* __restrict__ s0, const uint32_t party, const RangeX pfx, const uint32_t nwalk,
    const uint64_t nroots, uint4* __restrict__ out, unsigned long long* __restrict__ blocks) {
  __shared__ uint32_t lds[kLdsWords];
  lds_fill_tables(lds, tab);
  RowPrg rp;
  rp.init(rk);
  const uint32_t a = rp.a;
  const uint32_t s0a = reinterpret_cast<const uint32_t*>(s0)[a];
  const uint32_t npa = reinterpret_cast<const uint32_t*>(cw_np1)[a];
  constexpr uint32_t kPer = kBlock / 32;  // roots per workgroup pass
  for (uint64_t base = (uint64_t)blockIdx.x * kPer; base < nroots; base += (uint64_t)gridDim.x * kPer) {
    const uint64_t r = base + (threadIdx.x >> 5);
    const bool live = r < nroots;
    const RangeX p = range_add(pfx, live ? r : nroots - 1);
    uint32_t s = s0a, v = 0u, t = party;
    for (uint32_t lev = 0; lev < nwalk; ++lev) {
      const uint32_t cs = reinterpret_cast<const uint32_t*>(cw_s + lev)[a];
      const uint32_t cv = reinterpret_cast<const uint32_t*>(cw_v + lev)[a], ct = cw_t[lev];
      uint32_t sl, vl, tl, sr, vr, tr;
      rp.children(lds, s, v, t, cs, cv, ct, sl, vl, tl, sr, vr, tr);
      const bool right = range_bit(p, nwalk - 1u - lev) != 0u;
      s = right ? sr : sl;
      v = right ? vr : vl;
      t = right ? tr : tl;
    }
    if (threadIdx.x == 0)
      atomicAdd(blocks, 2ull * nwalk * (unsigned long long)min((uint64_t)kPer, nroots - base));
    if (live && (threadIdx.x & 31u) < 4u) {  // row 0, lanes 0..3: columns 0..3
      if (LEAF) {
        reinterpret_cast<uint32_t*>(out + r)[a] = v ^ s ^ ((0u - t) & npa);
      } else {
        uint32_t* o = reinterpret_cast<uint32_t*>(out + 2u * r);
        o[a] = a == 3u ? ((s & kMaskLast) | (t << 24)) : s;
        o[4u + a] = v;
      }
    }
  }
}

// Interior, one launch per level (k_fd_level16 on PrefixTable-style rows): the parents of level
// `lev` — rows in[2j], in[2j + 1] of all blocks, consecutive in leaf order — become the children
// rows out[4j .. 4j + 3], one lane per parent, waves claiming units of parents from ctr[0].
// blocks: the call's AES block count, 2 per parent.
__global__ __launch_bounds__(kBlock, 1) void k_range_level16(
    const uint32_t* __restrict__ tab, const RoundKeys rk, const uint4* __restrict__ cw_s,
    const uint4* __restrict__ cw_v, const uint8_t* __restrict__ cw_t, const uint32_t lev,
    const uint32_t nparents, const uint4* __restrict__ in, uint4* __restrict__ out, uint32_t* __restrict__ ctr,
    unsigned long long* __restrict__ blocks) {
  __shared__ uint32_t lds[kLdsWords];
  lds_fill_tables(lds, tab);
  const uint32_t lc = lane_const();
  const uint4 cs = cw_s[lev], cv = cw_v[lev];
  const uint32_t csw[4] = {cs.x, cs.y, cs.z, cs.w}, cvw[4] = {cv.x, cv.y, cv.z, cv.w};
  const uint32_t ct = cw_t[lev];
  const uint32_t unit = fd_unit(nparents);
  uint32_t nlive = 0;  // parents this wave expanded: one atomic per wave, after its last unit
  for (uint64_t base = next_unit_base_n(ctr, ~0ull, unit); base < nparents;
       base = next_unit_base_n(ctr, base, unit)) {
    const uint32_t j = (uint32_t)base + (threadIdx.x & 63u);
    const bool live = j < nparents;
    const uint32_t jj = live ? j : nparents - 1u;
    nlive += (uint32_t)__popcll(__ballot(live));
    const uint4 a = in[2ull * jj], b = in[2ull * jj + 1u];
    const uint32_t s[4] = {a.x, a.y, a.z, a.w & kMaskLast}, v[4] = {b.x, b.y, b.z, b.w};
    uint32_t sl[4], vl[4], sr[4], vr[4], tl, tr;
    fd_children(lds, lc, rk, csw, cvw, ct, s, v, (a.w >> 24) & 1u, sl, vl, tl, sr, vr, tr);
    if (!live) continue;
    uint4* o = out + 4ull * j;
    o[0] = make_uint4(sl[0], sl[1], sl[2], (sl[3] & kMaskLast) | (tl << 24));
    o[1] = make_uint4(vl[0], vl[1], vl[2], vl[3]);
    o[2] = make_uint4(sr[0], sr[1], sr[2], (sr[3] & kMaskLast) | (tr << 24));
    o[3] = make_uint4(vr[0], vr[1], vr[2], vr[3]);
  }
  if ((threadIdx.x & 63u) == 0 && nlive) atomicAdd(blocks, 2ull * nlive);
}

// Tail: k_fd_dfs16's register depth-first expansion of the last H levels from the rows of level
// lev0 = 8N - H, one lane per node, waves claiming units of nodes from ctr[0].  Node j's leaves
// are g = (j << H) .. (j << H) + 2^H - 1, counted from the first root's first leaf; the range
// starts `skip` leaves in and holds `count`, so leaf g is output g - skip and is stored only when
// that is below count (32-bit: a launch covers at most 2^28 outputs; g < skip wraps far above).
// blocks: the call's AES block count, 2 (2^H - 1) per node — clipped leaves included.
template <int H>
__global__ __launch_bounds__(kBlock, 1) void k_range_tail16(
    const uint32_t* __restrict__ tab, const RoundKeys rk, const uint4* __restrict__ cw_s,
    const uint4* __restrict__ cw_v, const uint8_t* __restrict__ cw_t, const uint4* __restrict__ cw_np1,
    const uint32_t lev0, const uint32_t nnodes, const uint4* __restrict__ rows, const uint32_t skip,
    const uint32_t count, uint4* __restrict__ ys, uint32_t* __restrict__ ctr,
    unsigned long long* __restrict__ blocks) {
  static_assert(H >= 2 && H <= 4, "register depth-first tail of 2..4 levels");
  __shared__ uint32_t lds[kLdsWords];
  lds_fill_tables(lds, tab);
  const uint32_t lc = lane_const();
  const uint4 np = cw_np1[0];
  const uint32_t unit = fd_unit(nnodes);
  uint32_t nlive = 0;  // nodes this wave expanded: one atomic per wave, after its last unit
  for (uint64_t base = next_unit_base_n(ctr, ~0ull, unit); base < nnodes;
       base = next_unit_base_n(ctr, base, unit)) {
    const uint32_t j = (uint32_t)base + (threadIdx.x & 63u);
    const bool live = j < nnodes;
    const uint32_t jj = live ? j : nnodes - 1u;
    nlive += (uint32_t)__popcll(__ballot(live));
    uint32_t stk[H - 1][9];  // pending right children: s[4] | v[4] | t, by depth
    uint32_t n[9];
    {
      const uint4 sv = rows[2ull * jj], vv = rows[2ull * jj + 1u];
      n[0] = sv.x; n[1] = sv.y; n[2] = sv.z; n[3] = sv.w & kMaskLast;
      n[4] = vv.x; n[5] = vv.y; n[6] = vv.z; n[7] = vv.w;
      n[8] = (sv.w >> 24) & 1u;
    }
    const uint32_t o0 = live ? (jj << H) - skip : 0x80000000u;  // output of the node's first leaf; idle lanes: none
    for (uint32_t i = 0; i < (1u << (H - 1)); ++i) {
      uint32_t k = 0;
      if (i) {  // resume at the right child saved at depth H - 2 - ctz(i) (wave-uniform)
        const uint32_t d = (uint32_t)(H - 2) - (uint32_t)__builtin_ctz(i);
#pragma unroll
        for (uint32_t q = 0; q + 1 < (uint32_t)H; ++q)
          if (q == d)
#pragma unroll
            for (int e = 0; e < 9; ++e) n[e] = stk[q][e];
        k = d + 1u;
      }
      for (;; ++k) {  // expand depth k (level lev0 + k)
        const uint4 cs = cw_s[lev0 + k], cv = cw_v[lev0 + k];
        const uint32_t csw[4] = {cs.x, cs.y, cs.z, cs.w}, cvw[4] = {cv.x, cv.y, cv.z, cv.w};
        const uint32_t s[4] = {n[0], n[1], n[2], n[3]}, v[4] = {n[4], n[5], n[6], n[7]};
        uint32_t sl[4], vl[4], sr[4], vr[4], tl, tr;
        fd_children(lds, lc, rk, csw, cvw, cw_t[lev0 + k], s, v, n[8], sl, vl, tl, sr, vr, tr);
        if (k + 1u == (uint32_t)H) {  // leaves 2i, 2i + 1 of the node: y = v ^ s ^ t * cw_np1 (lib.rs:192)
          const uint32_t ol = o0 + 2u * i, orr = ol + 1u;
          const uint32_t ml = 0u - tl, mr = 0u - tr;
          if (ol < count)
            ys[ol] = make_uint4(vl[0] ^ sl[0] ^ (ml & np.x), vl[1] ^ sl[1] ^ (ml & np.y),
                                vl[2] ^ sl[2] ^ (ml & np.z), vl[3] ^ sl[3] ^ (ml & np.w));
          if (orr < count)
            ys[orr] = make_uint4(vr[0] ^ sr[0] ^ (mr & np.x), vr[1] ^ sr[1] ^ (mr & np.y),
                                 vr[2] ^ sr[2] ^ (mr & np.z), vr[3] ^ sr[3] ^ (mr & np.w));
          break;
        }
#pragma unroll
        for (uint32_t q = 0; q + 1 < (uint32_t)H; ++q)
          if (q == k) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              stk[q][e] = sr[e];
              stk[q][4 + e] = vr[e];
            }
            stk[q][8] = tr;
          }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          n[e] = sl[e];
          n[4 + e] = vl[e];
        }
        n[8] = tl;
      }
    }
  }
  if ((threadIdx.x & 63u) == 0 && nlive) atomicAdd(blocks, 2ull * ((1u << H) - 1u) * nlive);
}

// Points x0 + i, i in [0, count), as N-byte big-endian strings (a sibling of k_domain_points): the
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

}  // namespace
