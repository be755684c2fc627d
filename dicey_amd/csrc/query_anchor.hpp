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
// Pattern and text reads are those of k_qmap: same positions, same k.  Included by mappability.hip behind query_map.hpp.
#pragma once
#include "query_map.hpp"

namespace dg {

struct AnchLane : MmLane {  // and the steps of the current strand at which the text must show the pattern's own character
  u32 t0, t1;
};

DG_DEV bool anch_step(const AnchLane& c, u32 t) { return t >= c.t0 && t < c.t1; }

// 0xFF in every byte b of the word at pattern index j whose index j + b lies in [i0, i1)
DG_DEV u64 anch_byte_mask(u32 j, u32 i0, u32 i1) {
  const u32 s = i0 > j ? i0 - j : 0u;
  const u32 e = i1 > j ? (i1 - j < 8u ? i1 - j : 8u) : 0u;
  if (s >= e) return 0;  // (so s <= 7)
  const u64 below_e = e == 8u ? ~0ULL : (1ULL << (8 * e)) - 1;
  return below_e & ~((1ULL << (8 * s)) - 1);
}

// mm_verify with the anchored index range [k - t1, k - t0): a mismatch inside it rejects the row
DG_DEV void anch_verify(const FmView& f, AnchLane& c, u32 t, u32 lo, u32 hi, u32 budget) {
  const u32 m = c.k - t;
  const u32 i0 = c.k - c.t1, i1 = c.k - c.t0;
  for (u32 r = lo; r < hi; ++r) {
    if (c.cap && c.total >= c.cap) return;
    const u64 s = f.sa[r];
    ++c.rows;
    if (s < m) continue;  // the window would start before the text
    const u64 q = s - m;
    u32 mism = 0;
    bool ok = true;
    for (u32 j = 0; j < m && ok; j += 8) {
      const u64 y = text8(f.text, q + j);
      u64 x = y ^ mm_pat8(f, c, m, j);
      if (m - j < 8) x &= (1ULL << (8 * (m - j))) - 1;
      const u64 nz = mm_nonzero_bytes(x);
      if (nz) {
        mism += (u32)__popcll(nz);
        ok = mism <= budget && (nz & (~mm_acgt_bytes(y) | anch_byte_mask(j, i0, i1))) == 0;
      }
    }
    c.total += ok;
  }
}

// mm_search whose levels spawn no sibling at an anchored step
template <int B>
DG_DEV void anch_search(const FmView& f, AnchLane& c, u32 t, u32 lo, u32 hi) {
  while (t < c.k && lo < hi) {
    if (c.cap && c.total >= c.cap) return;
    if (hi - lo <= c.W) {
      anch_verify(f, c, t, lo, hi, (u32)B);
      return;
    }
    const OccLine A = occ_load(f.occ, lo >> 7);
    const OccLine Z = (lo >> 7) == (hi >> 7) ? A : occ_load(f.occ, hi >> 7);
    u32 nlo[4], nhi[4];
#pragma unroll
    for (u32 a = 0; a < 4; ++a) {
      nlo[a] = f.C4[a] + occ_in_line(A, lo & 127, a);
      nhi[a] = f.C4[a] + occ_in_line(Z, hi & 127, a);
    }
    ++c.steps;
    const u32 pc = mm_pat_code(f, c, t);
    if constexpr (B > 0) {
      if (!anch_step(c, t)) {
        for (u32 d = 1; d < 4; ++d) {  // the sibling counter of this level
          const u32 a = (pc + d) & 3u;
          const u32 l = sel4(a, nlo[0], nlo[1], nlo[2], nlo[3]), h = sel4(a, nhi[0], nhi[1], nhi[2], nhi[3]);
          if (l < h) anch_search<B - 1>(f, c, t + 1, l, h);
        }
      }
    }
    lo = sel4(pc, nlo[0], nlo[1], nlo[2], nlo[3]);
    hi = sel4(pc, nhi[0], nhi[1], nhi[2], nhi[3]);
    ++t;
  }
  if (lo < hi) c.total += hi - lo;
}

// mm_strand whose table start places substitutions at free table steps only
template <int E>
DG_DEV void anch_strand(const FmView& f, AnchLane& c) {
  if (!(f.K && c.k >= f.K)) {
    anch_search<E>(f, c, 0, 0, (u32)f.n);
    return;
  }
  const u32 K = f.K;
  u64 code = 0;
  for (u32 t = 0; t < K; ++t) code |= (u64)mm_pat_code(f, c, t) << (2 * t);
  {
    const KtabEntry e0 = ktab_entry(f, code);
    ++c.tab;
    if (e0.lo < e0.hi) anch_search<E>(f, c, K, e0.lo, e0.hi);
  }
  if constexpr (E >= 1) {
    for (u32 i = 0; i < K; ++i) {
      if (anch_step(c, i)) continue;
      for (u64 a = 1; a < 4; ++a) {
        if (c.cap && c.total >= c.cap) return;
        const u64 code1 = code ^ (a << (2 * i));
        const KtabEntry e1 = ktab_entry(f, code1);
        ++c.tab;
        if (e1.lo < e1.hi) anch_search<E - 1>(f, c, K, e1.lo, e1.hi);
        if constexpr (E >= 2) {
          for (u32 j = 0; j < i; ++j) {
            if (anch_step(c, j)) continue;
            for (u64 b = 1; b < 4; ++b) {
              if (c.cap && c.total >= c.cap) return;
              const KtabEntry e2 = ktab_entry(f, code1 ^ (b << (2 * j)));
              ++c.tab;
              if (e2.lo < e2.hi) anch_search<E - 2>(f, c, K, e2.lo, e2.hi);
            }
          }
        }
      }
    }
  }
}

// buffer positions [p0, p1): out[p] = the saturated (and capped) anchored total of the k-mer at p, QMAP_INVALID where no k-mer of A/C/G/T
// starts.  anchor <= k (the host checks)
template <int E>
__global__ void __launch_bounds__(256) k_qmap_anch(FmView f, const u8* q, const u64* valid, u32 k, u32 anchor, int forward_only, u32 W, u32 cap, u64 p0,
                                                  u64 p1, u32* out, QmapCounters* ctr) {
  const u64 i = p0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  AnchLane c;
  c.pat = q;
  c.p = i;
  c.k = k;
  c.rev = false;
  c.W = W;
  c.cap = cap;
  c.total = 0;
  c.steps = c.tab = c.rows = 0;
  c.t0 = c.t1 = 0;
  u32 ok = 0, early = 0;
  if (i < p1) {
    u32 v = QMAP_INVALID;
    if (bit_at(valid, i)) {
      ok = 1;
      const u32 strands = forward_only ? 1u : 2u;
#pragma nounroll
      for (u32 s = 0; s < strands && !(cap && c.total >= cap); ++s) {  // (a loop: one copy of the search in the kernel)
        c.rev = s != 0;
        c.t0 = s ? k - anchor : 0u;  // step t consumes pattern index k-1-t: w's last a bases are revcomp(w)'s first a
        c.t1 = s ? k : anchor;
        anch_strand<E>(f, c);
      }
      early = cap && c.total >= cap;
      v = c.total > QMAP_MAX ? QMAP_MAX : (u32)c.total;
      if (cap && v > cap) v = cap;
    }
    out[i] = v;
  }
  wave_add(&ctr->valid, ok);  // (every lane of the wavefront is here)
  wave_add(&ctr->steps, c.steps);
  wave_add(&ctr->table_reads, c.tab);
  wave_add(&ctr->verified_rows, c.rows);
  wave_add(&ctr->early_exits, early);
}

}  // namespace dg
