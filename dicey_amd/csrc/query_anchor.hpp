// Anchored query mappability (dg_query_map_anchored, `dicey mappability -q -a`): the counts of k_qmap (query_map.hpp) with the
// LAST a bases of the k-mer w, its 3' end, matched exactly.
//
//   fwd(p) = #{valid windows u of the text : Hamming(u, w) <= e and u[k-a, k) == w[k-a, k)}
//   rev(p) = #{valid windows u of the text : Hamming(u, revcomp(w)) <= e and u[0, a) == revcomp(w)[0, a)}
// Backward-search step t consumes pattern index k-1-t, so the anchored bases are the steps [0, a) of the forward pattern and the steps
// [k-a, k) of revcomp(w): one step range [t0, t1) per strand, which the search exploits rather than filters by:
//   levels   no sibling is spawned at a step inside [t0, t1);
//   table    substitutions are placed only at table steps outside [t0, t1): with F free steps among the table's K a strand reads
//            1 + 3F + 9F(F-1)/2 entries at e = 2 (forward with a >= K: one entry);
//   narrow   a mismatching byte whose pattern index lies in [k-t1, k-t0) rejects the row, as a byte outside A/C/G/T does: a byte mask
//            per 8-byte word, which may begin and end inside the word.
// The search itself is map_mm.hpp's, run on an AnchLane: the three conditions are its Lane::anchored branches, and mm_strands sets the
// strand's [t0, t1).  Pattern and text reads are those of k_qmap: same positions, same k.
#pragma once
#include "query_map.hpp"

namespace dg {

// buffer positions [p0, p1): out[p] = the saturated (and capped) anchored total of the k-mer at p, QMAP_INVALID where no k-mer of A/C/G/T
// starts.  anchor <= k (the host checks)
template <int E>
__global__ void __launch_bounds__(256) k_qmap_anch(FmView f, const u8* q, const u64* valid, u32 k, u32 anchor, int forward_only, u32 W, u32 cap, u64 p0,
                                                  u64 p1, u32* out, QmapCounters* ctr) {
  const u64 i = p0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  AnchLane c;
  mm_lane_init(c, q, i, k, W, cap);
  u32 ok = 0, early = 0;
  if (i < p1) {
    u32 v = QMAP_INVALID;
    if (bit_at(valid, i)) {
      ok = 1;
      const u32 strands = forward_only ? 1u : 2u;
#pragma nounroll
      for (u32 s = 0; s < strands && !(cap && c.total >= cap); ++s) {  // (a loop: one copy of the search in the kernel)
        mm_set_strand(c, s != 0, anchor);
        mm_strand<E>(f, c);
      }
      early = cap && c.total >= cap;
      v = c.total > QMAP_MAX ? QMAP_MAX : (u32)c.total;
      if (cap && v > cap) v = cap;
    }
    out[i] = v;
  }
  wave_add(&ctr->valid, ok);  // (every lane of the wavefront is here)
  mm_flush(ctr, c);
  wave_add(&ctr->early_exits, early);
}

}  // namespace dg
