// Degenerate query mappability (dg_query_map_iupac, `dicey mappability -q -I`): the counts of k_qmap / k_qmap_anch for
// records whose letters are A, C, G, T and the eleven IUPAC codes R Y S W K M B D H V N, each standing for a set S(c) of bases.
//
//   deg(w)  = the product of |S(w_j)| over the k-mer w
//   dist(u, w) = #{ j : u_j not in S(w_j) }
//   fwd(p)  = #{valid windows u of the text : dist(u, w) <= e and u_j in S(w_j) for the LAST a indices j}
//   rev(p)  = the same against revcomp(w), whose sets are the complemented sets in reverse order and whose anchored indices are the FIRST a
// Every window counts once, however many expansions of w it is close to: the lane walks the concrete expansions v of w with an odometer
// over the degenerate indices and runs map_mm.hpp's search once per v on a SetLane, where
//   - a letter of S(w_j) other than v_j is never substituted: that window belongs to the expansion that shows it;
//   - a letter outside S(w_j) is substituted at cost 1 only where v_j is the lowest code of S(w_j), the canonical member, and j is not
//     anchored.
// A window u is therefore reached from the one expansion with v_j = u_j where u_j is in the set and v_j canonical where it is not, at
// cost dist(u, w).  k <= 64 keeps an expansion in registers: the degenerate indices, the two bit planes of the member chosen at each
// and the indices open to a substitution are one 64-bit word each.  Positions with deg(w) > max_degeneracy are not searched.
#pragma once
#include "query_map.hpp"

namespace dg {

struct QiupacCounters {  // device record, one wave_add per field and wavefront
  unsigned long long valid, steps, table_reads, verified_rows, early_exits, too_degenerate, degenerate, expansions;
};

// b is one of the 15 letters: a bit per letter from 'A' on
DG_DEV bool iupac_letter(u32 b) {
  constexpr u32 L = 1u << 0 | 1u << 1 | 1u << 2 | 1u << 3 | 1u << 6 | 1u << 7 | 1u << 10 | 1u << 12 | 1u << 13 | 1u << 17 | 1u << 18 | 1u << 19 |
                    1u << 21 | 1u << 22 | 1u << 24;  // A B C D G H K M N R S T V W Y
  const u32 x = b - 'A';
  return x < 25u && ((L >> x) & 1u);
}

// k_acgt_bits for the 15 letters: bit j of word w = T[64w + j] is A/C/G/T or an IUPAC code (positions >= n and the padding words are 0)
__global__ void k_iupac_bits(const u8* text, u64 n, u64* bits, u64 nw) {
  const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nw) return;
  u64 m = 0;
  const u64 p0 = w * 64;
  if (p0 < n) {
    const uint4* q = reinterpret_cast<const uint4*>(text + p0);
#pragma unroll
    for (u32 c = 0; c < 4; ++c) {
      const uint4 v = q[c];
      const u32 wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (u32 j = 0; j < 16; ++j) {
        const u32 b = (wd[j >> 2] >> (8 * (j & 3))) & 255u;
        m |= (u64)iupac_letter(b) << (c * 16 + j);
      }
    }
    if (n - p0 < 64) m &= (1ULL << (n - p0)) - 1;
  }
  bits[w] = m;
}

// deg(w) of the k-mer at p of q (15 letters only, k <= 64), or limit + 1 once it passes limit (<= 4096); degw: its degenerate indices
DG_DEV u32 iupac_degeneracy(const u8* q, u64 p, u32 k, u32 limit, u64& degw) {
  u32 deg = 1;
  degw = 0;
  for (u32 j = 0; j < k; j += 8) {
    const u64 x = text8(q, p + j);
    const u32 m = k - j < 8 ? k - j : 8u;
    for (u32 b = 0; b < m; ++b) {
      const u32 n = (u32)__popc(iupac_set((u32)(x >> (8 * b)) & 255u));
      degw |= (u64)(n > 1) << (j + b);
      deg = deg * n > limit ? limit + 1 : deg * n;  // (at most 4097 * 4)
    }
  }
  return deg;
}

// the lane's next searches are of the expansions of its k-mer w or, with rev, of revcomp(w), the first one first: the canonical member at
// every degenerate index.  degw: w's degenerate indices; anchor: the last `anchor` bases of w, revcomp(w)'s first, take no substitution
DG_DEV void iupac_set_strand(SetLane& c, bool rev, u32 anchor, u64 degw) {
  c.rev = rev;
  c.deg = rev ? __brevll(degw) >> (64 - c.k) : degw;
  c.sel0 = c.sel1 = 0;
  const auto below = [](u32 n) { return n >= 64 ? ~0ULL : (1ULL << n) - 1; };
  c.allow = rev ? below(c.k) & ~below(anchor) : below(c.k - anchor);  // anchored: the pattern's first `anchor` indices, else its last
}

// the odometer: the next expansion (the member index of the lowest degenerate index runs fastest); false once every one has been seen.
// The caller takes the indices that no longer show the canonical member out of c.allow
DG_DEV bool iupac_next(SetLane& c) {
  for (u64 d = c.deg; d; d &= d - 1) {
    const u32 i = (u32)__builtin_ctzll(d);
    const u64 bit = 1ULL << i;
    const u32 n = (u32)__popc(iupac_set(c.pat[c.rev ? c.p + c.k - 1 - i : c.p + i]));
    const u32 idx = ((c.sel0 & bit) ? 1u : 0u) + ((c.sel1 & bit) ? 2u : 0u) + 1u;
    if (idx < n) {
      c.sel0 = (c.sel0 & ~bit) | ((idx & 1u) ? bit : 0);
      c.sel1 = (c.sel1 & ~bit) | ((idx & 2u) ? bit : 0);
      return true;
    }
    c.sel0 &= ~bit;  // back to the canonical member, and on to the next index
    c.sel1 &= ~bit;
  }
  return false;
}

// buffer positions [p0, p1): out[p] = the saturated (and capped) total of the degenerate k-mer at p, QMAP_INVALID where no k-mer of the 15
// letters starts or its degeneracy is above maxdeg.  10 <= k <= 64, anchor <= k, 1 <= maxdeg <= 4096 (the host checks)
template <int E>
__global__ void __launch_bounds__(256) k_qmap_iupac(FmView f, const u8* q, const u64* valid, u32 k, u32 anchor, u32 maxdeg, int forward_only, u32 W,
                                                   u32 cap, u64 p0, u64 p1, u32* out, QiupacCounters* ctr) {
  const u64 i = p0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  SetLane c;
  mm_lane_init(c, q, i, k, W, cap);
  u32 ok = 0, early = 0, too = 0, degen = 0, nexp = 0;
  if (i < p1) {
    u32 v = QMAP_INVALID;
    if (bit_at(valid, i)) {
      u64 degw;
      const u32 deg = iupac_degeneracy(q, i, k, maxdeg, degw);
      if (deg > maxdeg) {
        too = 1;
      } else {
        ok = 1;
        degen = deg > 1;
        const u32 strands = forward_only ? 1u : 2u;
#pragma nounroll
        for (u32 s = 0; s < strands && !(cap && c.total >= cap); ++s) {  // (loops: one copy of the search in the kernel)
          iupac_set_strand(c, s != 0, anchor, degw);
          const u64 open = c.allow;  // every index that is not anchored
#pragma nounroll
          do {
            ++nexp;
            mm_strand<E>(f, c);
            if (cap && c.total >= cap) break;
            if (!iupac_next(c)) break;
            c.allow = open & ~(c.sel0 | c.sel1);
          } while (true);
        }
        early = cap && c.total >= cap;
        v = c.total > QMAP_MAX ? QMAP_MAX : (u32)c.total;
        if (cap && v > cap) v = cap;
      }
    }
    out[i] = v;
  }
  wave_add(&ctr->valid, ok);  // (every lane of the wavefront is here)
  mm_flush(ctr, c);
  wave_add(&ctr->early_exits, early);
  wave_add(&ctr->too_degenerate, too);
  wave_add(&ctr->degenerate, degen);
  wave_add(&ctr->expansions, nexp);
}

}  // namespace dg
