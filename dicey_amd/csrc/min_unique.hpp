// Minimum unique length: the shortest k-mer that starts at a position and is unique in the genome (`dicey mappability -u`,
// dg_min_unique).
//
// Index text T with the sentinel at n-1, position p in [0, n-1), max_k in 10..1000.
//   run(p)     the number of consecutive A/C/G/T bytes from p: 0 when T[p] is anything else; N, IUPAC letters, the '\n' between
//              sequences and the sentinel all end a run
//   limit(p)   min(run(p), max_k)
//   value_k(p) the exact mappability of mappability.hip: count(w) + count(revcomp(w)) for w = T[p, p+k), sdsl::count semantics
//              (forward_only: count(w) alone); a reverse-complement palindrome therefore never has value 1 at its own length
//   mul(p)     the smallest k in 1..limit(p) with value_k(p) == 1; 0 when there is none (the position is not A/C/G/T, or the k-mer is
//              still repeated at limit(p))
// Both strand counts fall monotonically as k grows, so mul(p) = max(1 + maxlcp(p), first k with count(revcomp(w_k)) == 0) wherever
// both numbers are <= limit(p); maxlcp(p) is the longer common prefix, in raw text bytes, of suffix p with its two neighbours in
// suffix-array order.  Values below 10 are legal (small genomes).
//   forward  k_mu_lcp: one thread per rank i, lcp[i] = min(max_k, common prefix of T[SA[i-1]..] and T[SA[i]..]), 8 bytes at a time;
//            lcp[0] = lcp[n] = 0.  Two different suffixes differ at the latest where the later one meets the sentinel, so no read goes
//            past the text's slack.
//   reverse  k_mu_walk: one thread per rank i, F = 1 + max(lcp[i], lcp[i+1]).  F > max_k or run(p) < F (the first F bytes, eight
//            per word): 0.  Else revcomp(w_k) read from its last character to its first is T[p], T[p+1], ... complemented: ONE backward
//            search that consumes one character per step is the reverse count of every k in turn.  It starts at the K-mer table entry of
//            the first K characters when those are all A/C/G/T and max_k >= K; an EMPTY entry says the first empty k is <= K — F >= K:
//            F is the answer and nothing more is read; F < K: the walk starts over from the full interval to find that k exactly.  The
//            walk ends at the first empty interval (answer max(F, steps consumed)), at a byte outside A/C/G/T or after max_k characters
//            (answer 0: still on the other strand at limit(p)).  The value goes to out[SA[i]] from the same kernel.
// The walk is the one k_heads takes at k = max_k (left at the first empty interval), per rank instead of per group head and only
// where F <= limit(p): no narrow-interval finish on the text is built on top of it (DESIGN.md §10 has the reasoning and the figures).
#pragma once
#include "map_mm.hpp"  // mm_acgt_bytes
#include "text_bits.hpp"

namespace dg {

__global__ void __launch_bounds__(256) k_mu_lcp(FmView f, u32 max_k, u64 r0, u64 r1, u16* lcp) {
  const u64 i = r0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r1) return;  // r1 <= n + 1: rank n is the closing 0
  u32 l = 0;
  if (i > 0 && i < f.n) {
    const u64 a = f.sa[i - 1], b = f.sa[i];
    l = max_k;
    for (u32 j = 0; j < max_k; j += 8) {
      const u64 x = text8(f.text, a + j) ^ text8(f.text, b + j);
      if (x) {
        l = j + ((u32)__ffsll((long long)x) - 1) / 8;
        break;
      }
    }
    if (l > max_k) l = max_k;
  }
  lcp[i] = (u16)l;
}

// the m bytes from p are all A/C/G/T
DG_DEV bool mu_acgt_run(const u8* t, u64 p, u32 m) {
  for (u32 j = 0; j < m; j += 8) {
    u64 bad = ~mm_acgt_bytes(text8(t, p + j)) & MM_HIGH;
    if (m - j < 8) bad &= (1ULL << (8 * (m - j))) - 1;
    if (bad) return false;
  }
  return true;
}

__global__ void __launch_bounds__(256) k_mu_walk(FmView f, u32 max_k, int forward_only, u64 r0, u64 r1, const u16* lcp, u32* out,
                                                unsigned long long* steps) {
  const u64 i = r0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  u32 n_ext = 0;
  if (i < r1) {
    const u64 p = f.sa[i];
    const u32 la = lcp[i], lb = lcp[i + 1];
    const u32 F = 1 + (la > lb ? la : lb);
    u32 v = 0;
    if (F <= max_k && mu_acgt_run(f.text, p, F)) {
      v = F;
      if (!forward_only) {
        u32 lo = 0, hi = (u32)f.n, t = 0;
        u64 chunk = 0;
        bool walk = true;
        if (f.K && max_k >= f.K && mu_acgt_run(f.text, p, f.K)) {
          u64 code = 0;
          for (u32 j = 0; j < f.K; ++j) {
            if ((j & 7) == 0) chunk = text8(f.text, p + j);
            code |= (u64)(3u - acgt_code((u32)(chunk >> (8 * (j & 7))) & 255u)) << (2 * j);
          }
          const KtabEntry e = ktab_entry(f, code);
          if (e.lo < e.hi) {
            lo = e.lo;
            hi = e.hi;
            t = f.K;
          } else if (F >= f.K) {
            walk = false;  // the other strand is gone at some k <= K <= F
          }
        }
        if (walk) {
          // v = 0 unless the interval empties: at a byte outside A/C/G/T or after max_k characters the other strand still matches
          v = 0;
          if (t & 7) chunk = text8(f.text, p + (t & ~7u));
          for (; t < max_k; ++t) {
            if ((t & 7) == 0) chunk = text8(f.text, p + t);
            const u32 b = (u32)(chunk >> (8 * (t & 7))) & 255u;
            if (!(b == 'A' || b == 'C' || b == 'G' || b == 'T')) break;
            bs_extend_code_narrow(f, lo, hi, 3u - acgt_code(b));
            ++n_ext;
            if (lo >= hi) {
              v = F > t + 1 ? F : t + 1;
              break;
            }
          }
        }
      }
    }
    out[p] = v;
  }
  wave_add(steps, n_ext);  // (every lane of the wavefront is here)
}

}  // namespace dg
