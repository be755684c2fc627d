// Query minimum length (dg_query_min_len, `dicey mappability -q -l`): per position of a query buffer the smallest k in
// [min_k, limit(p)] at which the k-mer that starts there has at most t places in the genome within e mismatches, both strands.
//
// The buffer, the lane layout and the search are k_qmap's (query_map.hpp): one lane per buffer position, mm_strand<E> per strand with the
// pattern read through MmLane::pat.  What is new is that the lane looks for its k itself.  value_k(p) never rises with k (a window within
// e of the (k+1)-mer has its k-prefix within e of the k-mer at the same start; on the other strand the window one to the right; both maps
// are injective), so "value_k(p) <= t" is false up to some k and true from there on, and any order of probes finds that k exactly:
//   limit    run(p), the A/C/G/T bytes from p, read off the bitmap of k_acgt_bits and cut at max_k: at most max_k/64 + 2 words, none at or
//            behind word nw (the buffer ends with a '\n', so a run ends inside the data words anyway).  limit < min_k: QMINLEN_INVALID.
//   probes   a probe sets c.k, c.cap = t + 1 and c.total = 0, runs k_qmap's strand loop and passes when total <= t.  First limit(p): a
//            fail gives 0 (long k-mers are cheap: the narrow-interval finish ends the search right behind the table whatever k is).
//            Then min_k, then a gallop upward from min_k in steps 2, 4, 8 ... and a bisection of the bracket it leaves: answers sit a
//            few characters above log4(n), close to min_k, far from max_k.
// One probe loop around one strand loop: one copy of the search in the kernel, no stack, no runtime-indexed array (map_mm.hpp's rules).
// Pattern reads: every probe has min_k <= k <= limit(p) <= run(p), so [p, p + k) lies inside the record.  mm_pat_code reads bytes of
// [p, p + k) only.  mm_pat8 reads the aligned words that overlap [p + j, p + j + 8) with j < k on the forward strand, and on the reverse
// strand from p + k - m (m <= k: never in front of p, so never in front of the buffer for the first record at offset 0, the smallest probe
// k = min_k and a record of exactly min_k bytes included) to below p + k + 8.  p + k <= qn - 1 (the record's '\n'), and the buffer has the
// rest of its 64-byte block and 64 bytes of slack behind qn: the bounds are k_qmap's.
#pragma once
#include "query_map.hpp"

namespace dg {

struct QminlenCounters {  // device record, one wave_add per field and wavefront
  unsigned long long valid, probes, steps, table_reads, verified_rows;
};

// buffer positions [p0, p1): out[p] = the smallest k in [min_k, limit(p)] whose k-mer has a total <= t, 0 when there is none, QMAP_INVALID
// where limit(p) < min_k.  acgt: the bitmap of k_acgt_bits over the buffer, nw words.
template <int E>
__global__ void __launch_bounds__(256) k_qminlen(FmView f, const u8* q, const u64* acgt, u64 nw, u32 min_k, u32 max_k, int forward_only, u32 W, u32 t,
                                                u64 p0, u64 p1, u32* out, QminlenCounters* ctr) {
  const u64 i = p0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  MmLane c;
  mm_lane_init(c, q, i, min_k, W, t + 1);
  u32 ok = 0, probes = 0;
  if (i < p1) {
    // limit(p): the first byte that is not A/C/G/T at or behind p, no further than max_k away
    u64 w = i >> 6;
    u32 lim = 0;
    if (w < nw) {
      const u64 z = ~acgt[w] >> (i & 63);  // (the shifted-in high bits are 0: they end nothing)
      lim = z ? (u32)__ffsll((long long)z) - 1 : 64 - (u32)(i & 63);
      if (!z)
        for (++w; lim < max_k && w < nw; ++w) {
          const u64 z1 = ~acgt[w];
          if (z1) {
            lim += (u32)__ffsll((long long)z1) - 1;
            break;
          }
          lim += 64;
        }
    }
    if (lim > max_k) lim = max_k;
    u32 v = QMAP_INVALID;
    if (lim >= min_k) {
      ok = 1;
      v = 0;
      const u32 strands = forward_only ? 1u : 2u;
      // lo fails (min_k - 1: nothing to probe there), hi passes once the first probe, at lim, has; step 0 marks that first probe
      u32 lo = min_k - 1, hi = lim, step = 0, k = lim;
#pragma nounroll
      for (;;) {  // (a loop: one copy of the search in the kernel)
        c.k = k;
        c.total = 0;
#pragma nounroll
        for (u32 s = 0; s < strands && c.total < c.cap; ++s) {
          mm_set_strand(c, s != 0);
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
