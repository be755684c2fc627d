// Query minimum length by END position (dg_query_min_len_end, `dicey mappability -q -l -E`): per position p of a query buffer
// the smallest k in [min_k, limit(p)] at which the k-mer that ENDS there, w_k = Q[p-k+1, p+1), has at most t places in the genome within e
// mismatches and with its last a bases exact, both strands: the 3' end stays where it is and the oligo grows at its 5' end.
//
// The buffer, the lane layout and the probe order are k_qminlen's (query_min_len.hpp); the search of one probe is k_qmap_anch's
// (query_anchor.hpp: mm_strand<E> on an AnchLane, unchanged).  What is new is the direction:
//   limit    brun(p), the A/C/G/T bytes that end at p, read off the bitmap of k_acgt_bits towards word 0 and cut at max_k: the nearest clear
//            bit at or in front of p (the word shifted left by 63 - (p & 63), __clzll), at most max_k/64 + 2 words, none in front of word 0
//            (the first record starts at buffer offset 0 with no '\n' in front of it: word 0 exhausted means the run starts at 0).
//            limit < min_k: QMAP_INVALID.
//   probe    c.p = p + 1 - k, c.k = k, c.cap = t + 1, c.total = 0.  Forward strand: steps [0, a) are anchored.  Other strand: steps
//            [k - a, k), recomputed per probe because k changes.  a <= min_k <= k (the host checks), so both ranges lie inside the pattern
//            and hold the same bases Q[p-a+1, p] at every k.  The probe passes when total <= t.
//   order    value_k(p) never rises with k (w_{k+1} = x w_k: a window within e of w_{k+1} with its last a bases exact has its k-suffix
//            within e of w_k with the same bases exact, one position to the right; on the other strand its k-prefix, at the same start;
//            both maps are injective).  So limit(p) first (a fail gives 0), then min_k, a gallop 2, 4, 8 ... upward, a bisection.
// One probe loop around one strand loop: one copy of the search in the kernel, no stack, no runtime-indexed array (map_mm.hpp's rules).
// Pattern reads: every probe has min_k <= k <= limit(p) <= brun(p), so [p + 1 - k, p + 1) lies inside the record: its start is at or behind
// the record's start, which is >= 0.  mm_pat_code reads bytes of that range only.  mm_pat8 reads the aligned words that overlap
// [start + j, start + j + 8) with j < k on the forward strand, so they end below p + 1 + 15 <= qn + 14 (p <= qn - 2: the last byte is a
// '\n'), inside the rest of the 64-byte block and the 64 bytes of slack behind qn; on the other strand it reads from start + k - m
// (m <= k: never in front of the start, so never in front of the buffer for the first record at offset 0) to below p + 1 + 8.
#pragma once
#include "query_anchor.hpp"
#include "query_min_len.hpp"

namespace dg {

// buffer positions [p0, p1): out[p] = the smallest k in [min_k, limit(p)] whose k-mer ending at p has an anchored total <= t, 0 when there
// is none, QMAP_INVALID where limit(p) < min_k.  acgt: the bitmap of k_acgt_bits over the buffer.  anchor <= min_k (the host checks)
template <int E>
__global__ void __launch_bounds__(256) k_qminlen_end(FmView f, const u8* q, const u64* acgt, u32 min_k, u32 max_k, u32 anchor, int forward_only, u32 W,
                                                    u32 t, u64 p0, u64 p1, u32* out, QminlenCounters* ctr) {
  const u64 i = p0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  AnchLane c;
  mm_lane_init(c, q, i, min_k, W, t + 1);
  u32 ok = 0, probes = 0;
  if (i < p1) {
    // limit(p): the last byte that is not A/C/G/T at or in front of p, no further than max_k away
    u64 w = i >> 6;
    const u64 z = ~acgt[w] << (63 - (i & 63));  // (the shifted-in low bits are 0: they end nothing)
    u32 lim = z ? (u32)__clzll((long long)z) : (u32)(i & 63) + 1;
    if (!z)
      while (lim < max_k && w > 0) {  // word 0 is the last one: nothing lies in front of the buffer
        const u64 z1 = ~acgt[--w];
        if (z1) {
          lim += (u32)__clzll((long long)z1);
          break;
        }
        lim += 64;
      }
    if (lim > max_k) lim = max_k;
    u32 v = QMAP_INVALID;
    if (lim >= min_k) {
      ok = 1;
      v = 0;
      const u32 strands = forward_only ? 1u : 2u;
      // k_qminlen's probe loop, spelled out a second time on purpose: shared as a helper it compiles differently ("One
      // search, folded").  lo fails (min_k - 1: nothing to probe there), hi passes once the first probe, at lim, has; step 0 marks that first probe
      u32 lo = min_k - 1, hi = lim, step = 0, k = lim;
#pragma nounroll
      for (;;) {  // (a loop: one copy of the search in the kernel)
        c.p = i + 1 - k;
        c.k = k;
        c.total = 0;
#pragma nounroll
        for (u32 s = 0; s < strands && c.total < c.cap; ++s) {
          mm_set_strand(c, s != 0, anchor);
          mm_strand<E>(f, c);
        }
        ++probes;
        const bool pass = c.total <= t;
        if (step == 0) {
          if (!pass) break;  // still not specific at limit(p)
          step = 1;
        } else if (pass) {
          hi = k;
        } else {
          lo = k;
          step <<= 1;
        }
        if (hi - lo <= 1) {
          v = hi;
          break;
        }
        k = lo + step < hi ? lo + step : lo + (hi - lo) / 2;  // the gallop while it stays below hi, then the bisection
      }
    }
    out[i] = v;
  }
  wave_add(&ctr->valid, ok);  // (every lane of the wavefront is here)
  wave_add(&ctr->probes, probes);
  mm_flush(ctr, c);
}

}  // namespace dg
