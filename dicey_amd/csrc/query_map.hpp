// Query mappability (dg_query_map, `dicey mappability -q`): (k,e) counts for the k-mers of sequences that are NOT in the index.
//
// The queries are one device buffer laid out like the index text, REC1 '\n' REC2 '\n' ..., with the text's zero slack behind, so that
// k_acgt_bits / k_valid_bits (text_bits.hpp) give the valid bit of every buffer position unchanged: a record boundary ends a k-mer the
// way a sequence boundary does.  One lane per buffer position runs both strands of its k-mer through mm_strand<E> (map_mm.hpp): K-mer table,
// levels, narrow-interval check against the TEXT; only the pattern comes from the query buffer (MmLane::pat).  There are no groups of equal
// k-mers to share a search and w itself is in the count only when the genome holds it, so 0 is a value and invalid positions carry
// DG_QMAP_INVALID.
#pragma once
#include "map_mm.hpp"

namespace dg {

struct QmapCounters {  // device record, one wave_add per field and wavefront
  unsigned long long valid, steps, table_reads, verified_rows, early_exits;
};

static constexpr u32 QMAP_INVALID = 0xFFFFFFFFu, QMAP_MAX = 0xFFFFFFFEu;

// buffer positions [p0, p1): out[p] = the saturated (and capped) total of the k-mer at p, QMAP_INVALID where no k-mer of A/C/G/T starts
template <int E>
__global__ void __launch_bounds__(256) k_qmap(FmView f, const u8* q, const u64* valid, u32 k, int forward_only, u32 W, u32 cap, u64 p0, u64 p1,
                                             u32* out, QmapCounters* ctr) {
  const u64 i = p0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  MmLane c;
  mm_lane_init(c, q, i, k, W, cap);
  u32 ok = 0, early = 0;
  if (i < p1) {
    u32 v = QMAP_INVALID;
    if (bit_at(valid, i)) {
      ok = 1;
      const u32 strands = forward_only ? 1u : 2u;
#pragma nounroll
      for (u32 s = 0; s < strands && !(cap && c.total >= cap); ++s) {  // (a loop: one copy of the search in the kernel)
        mm_set_strand(c, s != 0);
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
