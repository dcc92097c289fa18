// kernels_range_mk.h — multi-key contiguous-range eval: ys[k * count + i] = Dcf::eval(b, key k, x0 + i)
// for K keys over one range.  Included by dcf_hip.hip only (after kernels_range.h).
//
// The three stages of kernels_range.h with one more dimension (DESIGN.md "Multi-key range eval").
// Every key's range is covered by the same nroots aligned blocks of 2^h leaves; every node buffer
// holds the keys of a launch group one after another, each in leaf order, so node j of a level with
// d nodes per key belongs to key j / d and key k's outputs are contiguous.  The correction words
// come from the K-key block ([lev][key] rows), read per lane at lev * K + key: a broadcast within
// one key, coalesced across neighbouring keys.  The single-key kernels are untouched.
//   k_rangemk_roots16   keys * nroots roots, one per 32-lane half-wave on RowPrg; root r belongs to
//                       key r / nroots and its path bits come from pfx + r % nroots.  h = 0 (LEAF):
//                       the roots are the points and the kernel writes y.
//   k_rangemk_level16   one launch per level over keys * (nroots << k) parents, one lane per parent.
//   k_rangemk_tail16    the 4-level register depth-first tail; the per-key skip / count clip leaves.
//   k_rangemk_gather    key k of a K-key block as a single-key block (the slow path of the PRGs /
//                       LAMBDA / N without a tree-sharing path).
// The pointers the kernels get are already advanced to the first key of the launch group; K stays
// the row stride.  All node, key and output indices of a launch are 32-bit (the host keeps
// keys * (nroots << h) <= 2^28).
#pragma once

#include "kernels_range.h"

namespace {

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

// Root r of `total` = keys * nroots: the node of level `nwalk` of key r / nroots whose prefix is
// pfx + r % nroots, walked from (s0s[key], 0, party) as k_range_roots16 walks its roots.  The
// quotient is one multiply per root, outside the level loop.  Rows / outputs as k_range_roots16,
// at index r (LEAF: nroots = count, so r = key * count + i).
template <bool LEAF>
__global__ __launch_bounds__(kBlock, 1) void k_rangemk_roots16(
    const uint32_t* __restrict__ tab, const RoundKeys rk, const uint4* __restrict__ cw_s,
    const uint4* __restrict__ cw_v, const uint8_t* __restrict__ cw_t, const uint4* __restrict__ cw_np1,
    const uint4* __restrict__ s0s, const uint64_t K, const uint32_t party, const RangeX pfx, const uint32_t nwalk,
    const RangeDiv nroots, const uint32_t total, uint4* __restrict__ out, unsigned long long* __restrict__ blocks) {
  __shared__ uint32_t lds[kLdsWords];
  lds_fill_tables(lds, tab);
  RowPrg rp;
  rp.init(rk);
  const uint32_t a = rp.a;
  constexpr uint32_t kPer = kBlock / 32;  // roots per workgroup pass
  for (uint32_t base = blockIdx.x * kPer; base < total; base += gridDim.x * kPer) {
    const uint32_t r = base + (threadIdx.x >> 5);
    const bool live = r < total;
    const uint32_t rr = live ? r : total - 1u;
    const uint32_t key = range_div(nroots, rr);
    const RangeX p = range_add(pfx, rr - key * nroots.d);
    uint32_t s = reinterpret_cast<const uint32_t*>(s0s + key)[a], v = 0u, t = party;
    for (uint32_t lev = 0; lev < nwalk; ++lev) {
      const uint64_t c = (uint64_t)lev * K + key;
      const uint32_t cs = reinterpret_cast<const uint32_t*>(cw_s + c)[a];
      const uint32_t cv = reinterpret_cast<const uint32_t*>(cw_v + c)[a], ct = cw_t[c];
      uint32_t sl, vl, tl, sr, vr, tr;
      rp.children(lds, s, v, t, cs, cv, ct, sl, vl, tl, sr, vr, tr);
      const bool right = range_bit(p, nwalk - 1u - lev) != 0u;
      s = right ? sr : sl;
      v = right ? vr : vl;
      t = right ? tr : tl;
    }
    if (threadIdx.x == 0) atomicAdd(blocks, 2ull * nwalk * (unsigned long long)min(kPer, total - base));
    if (live && (threadIdx.x & 31u) < 4u) {  // row 0, lanes 0..3: columns 0..3
      if (LEAF) {
        const uint32_t npa = reinterpret_cast<const uint32_t*>(cw_np1 + key)[a];
        reinterpret_cast<uint32_t*>(out + r)[a] = v ^ s ^ ((0u - t) & npa);
      } else {
        uint32_t* o = reinterpret_cast<uint32_t*>(out + 2ull * r);
        o[a] = a == 3u ? ((s & kMaskLast) | (t << 24)) : s;
        o[4u + a] = v;
      }
    }
  }
}

// Interior level `lev` (k_range_level16 over several keys): parent j of nparents = keys * per.d
// belongs to key j / per.d; its children rows go to out[4j .. 4j + 3], which keeps the keys one
// after another in leaf order.  The level's correction words are per-lane loads at lev * K + key.
__global__ __launch_bounds__(kBlock, 1) void k_rangemk_level16(
    const uint32_t* __restrict__ tab, const RoundKeys rk, const uint4* __restrict__ cw_s,
    const uint4* __restrict__ cw_v, const uint8_t* __restrict__ cw_t, const uint64_t K, const uint32_t lev,
    const RangeDiv per, const uint32_t nparents, const uint4* __restrict__ in, uint4* __restrict__ out,
    uint32_t* __restrict__ ctr, unsigned long long* __restrict__ blocks) {
  __shared__ uint32_t lds[kLdsWords];
  lds_fill_tables(lds, tab);
  const uint32_t lc = lane_const();
  const uint64_t row = (uint64_t)lev * K;
  const uint32_t unit = fd_unit(nparents);
  uint32_t nlive = 0;  // parents this wave expanded: one atomic per wave, after its last unit
  for (uint64_t base = next_unit_base_n(ctr, ~0ull, unit); base < nparents;
       base = next_unit_base_n(ctr, base, unit)) {
    const uint32_t j = (uint32_t)base + (threadIdx.x & 63u);
    const bool live = j < nparents;
    const uint32_t jj = live ? j : nparents - 1u;
    nlive += (uint32_t)__popcll(__ballot(live));
    const uint64_t c = row + range_div(per, jj);
    const uint4 cs = cw_s[c], cv = cw_v[c];
    const uint32_t csw[4] = {cs.x, cs.y, cs.z, cs.w}, cvw[4] = {cv.x, cv.y, cv.z, cv.w};
    const uint32_t ct = cw_t[c];
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

// Tail (k_range_tail16 over several keys): node j of nnodes = keys * per.d is node j % per.d of key
// j / per.d; its leaves are g = (j % per.d << H) .. + 2^H - 1 of that key, leaf g is the key's
// output g - skip, stored at ys[key * count + g - skip] only when g - skip < count (g < skip wraps
// far above).  The correction words of depth k are per-lane loads at (lev0 + k) * K + key.
template <int H>
__global__ __launch_bounds__(kBlock, 1) void k_rangemk_tail16(
    const uint32_t* __restrict__ tab, const RoundKeys rk, const uint4* __restrict__ cw_s,
    const uint4* __restrict__ cw_v, const uint8_t* __restrict__ cw_t, const uint4* __restrict__ cw_np1,
    const uint64_t K, const uint32_t lev0, const RangeDiv per, const uint32_t nnodes,
    const uint4* __restrict__ rows, const uint32_t skip, const uint32_t count, uint4* __restrict__ ys,
    uint32_t* __restrict__ ctr, unsigned long long* __restrict__ blocks) {
  static_assert(H >= 2 && H <= 4, "register depth-first tail of 2..4 levels");
  __shared__ uint32_t lds[kLdsWords];
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
    const uint32_t key = range_div(per, jj);
    // Nodes stay in the rows' form (t in bit 24 of word 3, the bit s has cleared): the per-lane
    // correction words take the registers the single-key tail has for a separate t.
    uint32_t stk[H - 1][8];  // pending right children: s[4] with t | v[4], by depth
    uint32_t n[8];
    {
      const uint4 sv = rows[2ull * jj], vv = rows[2ull * jj + 1u];
      n[0] = sv.x; n[1] = sv.y; n[2] = sv.z; n[3] = sv.w;
      n[4] = vv.x; n[5] = vv.y; n[6] = vv.z; n[7] = vv.w;
    }
    // output of the node's first leaf within its key; idle lanes: none
    const uint32_t o0 = live ? ((jj - key * per.d) << H) - skip : 0x80000000u;
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
        const uint64_t c = (uint64_t)(lev0 + k) * K + key;
        const uint4 cs = cw_s[c], cv = cw_v[c];
        const uint32_t csw[4] = {cs.x, cs.y, cs.z, cs.w}, cvw[4] = {cv.x, cv.y, cv.z, cv.w};
        const uint32_t s[4] = {n[0], n[1], n[2], n[3] & kMaskLast}, v[4] = {n[4], n[5], n[6], n[7]};
        uint32_t sl[4], vl[4], sr[4], vr[4], tl, tr;
        fd_children(lds, lc, rk, csw, cvw, cw_t[c], s, v, (n[3] >> 24) & 1u, sl, vl, tl, sr, vr, tr);
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
  if ((threadIdx.x & 63u) == 0 && nlive) atomicAdd(blocks, 2ull * ((1u << H) - 1u) * nlive);
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

}  // namespace
