// Minimum unique length with mismatches (dg_min_unique_mm, `dicey mappability -u -w`): per text position the smallest k in
// 1..limit(p) at which the k-mer that starts there is the ONLY valid window of the text within e substitutions of it and of its reverse
// complement, e in {1, 2}: (k,e)-mappability over all k at once.
//
//   value_{e,k}(p)  what dg_mappability_mm writes at p for this k and e (max_count = 0); w_k itself is counted, so it is >= 1
//   mul_e(p)        the smallest k in 1..limit(p) with value_{e,k}(p) == 1, 0 when there is none
// A window within 0 mismatches is within e, so value_{e,k} >= value_{0,k} and mul_e(p) >= mul_0(p), and mul_0(p) == 0 (nothing unique
// up to the limit even exactly) gives mul_e(p) == 0.  The two exact passes (min_unique.hpp) run first and leave L0 = mul_0(p) in out[p]:
// a lower bound a few characters below the answer, and every position that can never be unique is settled before a search is spent.
//   lane     one per text position p (coalesced reads and writes of out[], no suffix-array read).  rank_order (the development build's
//            DICEY_MU_MM_RANK_ORDER, for the measurement of DESIGN.md §10): lane i takes p = SA[i] instead; neighbours then share their
//            first ~log4 n characters, so their table entries and early Occ lines, and the writes scatter: 12 % faster on the i.i.d.
//            genome, 1.8 x slower on the repeats genome, where the lanes of a repeat then sit in the same workgroups and finish last.
//            L0 == 0 is final.  Otherwise limit(p) = min(run(p), max_k) from the text bytes, eight at a time from p + L0 on (the first
//            L0 are A/C/G/T: the exact pass checked them).  The bytes are the lines the lane's pattern reads touch next; a bitmap would
//            cost a pass and n/8 bytes to save at most max_k/8 - max_k/64 word reads per candidate.
//   probes   the schedule of probe_schedule.hpp with lo = L0 - 1, hi = limit(p): first limit(p), a fail writes 0; then L0, a pass keeps
//            the value; then the gallop upward and the bisection.  A probe is k_qminlen's: c.k = k, c.total = 0, cap = 2, mm_strand<E>
//            per strand, and it passes when the total is <= 1.  value_{e,k} never rises with k (query_min_len.hpp has the argument; a
//            valid (k+1)-window has a valid k-prefix and a valid k-suffix), so any order of probes finds the answer exactly.
//   writer   the lane overwrites out[p], its own slot, which no other lane of the launch reads or writes (in rank order: SA is a
//            permutation).
// One probe loop around one strand loop: one copy of the search in the kernel, no stack, no runtime-indexed array (map_mm.hpp's rules).
// Pattern reads: every probe has 1 <= k <= limit(p) <= run(p), so [p, p + k) holds A/C/G/T only and ends in front of the '\n' that closes
// its sequence; mm_pat8 reads what k_heads_mm reads for a valid k-mer at p.  The limit scan stops at the first word with another byte:
// at the latest the one with that '\n' (or the sentinel), inside the text and its slack.
#pragma once
#include "map_mm.hpp"
#include "probe_schedule.hpp"

namespace dg {

struct MuMmCounters {  // device record, one wave_add per field and wavefront
  unsigned long long candidates, probes, steps, table_reads, verified_rows;
};

// positions [r0, r1) (r1 <= n; the sentinel's slot holds 0): out[p] holds mul_0 and receives mul_e.  rank_order: ranks [r0, r1) instead
template <int E>
__global__ void __launch_bounds__(256) k_mu_mm(FmView f, u32 max_k, int forward_only, u32 W, int rank_order, u64 r0, u64 r1, u32* out,
                                               MuMmCounters* ctr) {
  const u64 i = r0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  MmLane c;
  mm_lane_init(c, f.text, 0, 1, W, 2);
  u32 cand = 0, probes = 0;
  if (i < r1) {
    const u64 p = rank_order ? f.sa[i] : i;
    const u32 L0 = out[p];
    if (L0 != 0) {
      cand = 1;
      c.p = p;
      // limit(p): the first byte that is not A/C/G/T at or behind p + L0, no further than max_k from p (L0 <= limit(p) <= max_k)
      u32 lim = max_k;
      for (u32 j = L0; j < max_k; j += 8) {
        const u64 bad = ~mm_acgt_bytes(text8(f.text, p + j)) & MM_HIGH;
        if (bad) {
          const u32 at = j + ((u32)__ffsll((long long)bad) - 1) / 8;
          if (at < lim) lim = at;
          break;
        }
      }
      const u32 strands = forward_only ? 1u : 2u;
      ProbeSchedule s = probe_begin(L0 - 1, lim);
#pragma nounroll
      do {  // (a loop: one copy of the search in the kernel)
        const u32 k = probe_next(s);
        c.k = k;
        c.total = 0;
#pragma nounroll
        for (u32 t = 0; t < strands && c.total < c.cap; ++t) {
          mm_set_strand(c, t != 0);
          mm_strand<E>(f, c);
        }
        ++probes;
        probe_update(s, k, c.total <= 1);
      } while (!probe_done(s));
      out[p] = probe_answer(s);
    }
  }
  wave_add(&ctr->candidates, cand);  // (every lane of the wavefront is here)
  wave_add(&ctr->probes, probes);
  mm_flush(ctr, c);
}

}  // namespace dg
