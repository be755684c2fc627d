// (k,e)-mappability, e in {1, 2}: the per-head search of `dicey mappability -e` (mappability.hip phase 3).
//
// For the k-mer w of a group head the kernel counts the valid windows of the text within Hamming distance e of w and, unless
// forward_only, of revcomp(w).  A window is an occurrence of one string u over A/C/G/T, so the count is the sum of the suffix-array
// interval widths of all u within distance e of the pattern: a backward search with a mismatch budget.
//   levels   mm_search<B> follows ONE string with B substitutions left.  A step reads the Occ lines of lo and hi once and forms the
//            intervals of all four characters; the pattern's character continues the level, each non-empty other one is a child with
//            budget B - 1 that runs to completion first (mm_search<B - 1>, inlined: e + 1 nested loops whose depth / lo / hi / sibling
//            counter live in registers — no stack, no runtime-indexed array).
//   table    the first K characters consumed are one K-mer table read; the strings with <= e substitutions inside them are further
//            reads (3K for one substitution, 9 K (K-1) / 2 for two).
//   narrow   an interval of at most W rows is finished on the text: the remaining characters in front of SA[r] against the rest of the
//            pattern, 8 bytes at a time, with the remaining budget.  A mismatching byte outside A/C/G/T (N, IUPAC, '\n') or a start
//            before position 0 rejects the row.  On a mostly unique genome that ends the search right behind the table, whatever k is.
// Included by mappability.hip behind text8 / acgt_code / bit_at.
#pragma once
#include "devfm.hpp"

namespace dg {

struct MmCounters {  // device record, one wave_add per field and wavefront
  unsigned long long heads, steps, table_reads, verified_rows, early_exits;
};

struct MmLane {  // one lane's search of one k-mer w: its constants and the running results
  const u8* pat;  // the buffer w is read from: the text for a group head, the query buffer for k_qmap (query_map.hpp).  8-byte reads of
                  // it touch only the aligned words that overlap [p, p + k + 8): never in front of an 8-aligned buffer, and behind its
                  // last k-mer inside the text's slack.  Windows are always read from f.text
  u64 p;          // position of w in pat
  u32 k;
  bool rev;   // the pattern is revcomp(w)
  u32 W;      // intervals of at most W rows are verified on the text (0: never)
  u32 cap;    // max_count (0: none): the search may stop once total reaches it
  u64 total;  // both strands
  u32 steps, tab, rows;
};

// the pattern's character met at backward-search step t (its LAST character at t = 0), as a code 0..3.  revcomp(w) from its last
// character to its first is w from its first to its last, complemented.
DG_DEV u32 mm_pat_code(const FmView& f, const MmLane& c, u32 t) {
  const u32 b = c.pat[c.rev ? c.p + t : c.p + c.k - 1 - t];
  const u32 x = acgt_code(b);
  return c.rev ? 3u - x : x;
}

static constexpr u64 MM_ONES = 0x0101010101010101ULL, MM_LOW7 = 0x7F7F7F7F7F7F7F7FULL, MM_HIGH = 0x8080808080808080ULL;
// 0x80 in every byte of x that is not zero (exact: no carry leaves a byte)
DG_DEV u64 mm_nonzero_bytes(u64 x) { return (((x & MM_LOW7) + MM_LOW7) | x) & MM_HIGH; }
// 0x80 in every byte of y that is A, C, G or T
DG_DEV u64 mm_acgt_bytes(u64 y) {
  return (~mm_nonzero_bytes(y ^ (MM_ONES * 'A')) | ~mm_nonzero_bytes(y ^ (MM_ONES * 'C')) | ~mm_nonzero_bytes(y ^ (MM_ONES * 'G')) |
          ~mm_nonzero_bytes(y ^ (MM_ONES * 'T'))) & MM_HIGH;
}
// complement of eight A/C/G/T bytes: A 0x41 <-> T 0x54 (xor 0x15), C 0x43 <-> G 0x47 (xor 0x04); bit 1 tells the pairs apart
DG_DEV u64 mm_complement_bytes(u64 x) {
  const u64 cg = (x >> 1) & MM_ONES;
  return x ^ (cg * 0x04) ^ ((cg ^ MM_ONES) * 0x15);
}

// the first m characters of the pattern from index j on, eight per word (byte i = pattern[j + i]); bytes at or behind m are undefined
DG_DEV u64 mm_pat8(const FmView& f, const MmLane& c, u32 m, u32 j) {
  if (!c.rev) return text8(c.pat, c.p + j);
  // pattern[i] = complement of w[k - 1 - i]: the eight bytes that end at w[k - 1 - j], reversed; near the pattern's end the word is
  // read from w[k - m] on (never in front of w) and shifted
  const u32 rem = m - j;
  if (rem >= 8) return mm_complement_bytes(__builtin_bswap64(text8(c.pat, c.p + c.k - 8 - j)));
  return mm_complement_bytes(__builtin_bswap64(text8(c.pat, c.p + c.k - m)) >> (8 * (8 - rem)));
}

// rows [lo, hi) hold the suffixes that start with the t characters consumed so far: count those whose k - t characters in front spell
// the rest of the pattern with at most `budget` substitutions
DG_DEV void mm_verify(const FmView& f, MmLane& c, u32 t, u32 lo, u32 hi, u32 budget) {
  const u32 m = c.k - t;
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
        ok = mism <= budget && (nz & ~mm_acgt_bytes(y)) == 0;
      }
    }
    c.total += ok;
  }
}

// the string whose last t characters have the interval [lo, hi), extended to the pattern's full length with at most B substitutions
template <int B>
DG_DEV void mm_search(const FmView& f, MmLane& c, u32 t, u32 lo, u32 hi) {
  while (t < c.k && lo < hi) {
    if (c.cap && c.total >= c.cap) return;
    if (hi - lo <= c.W) {
      mm_verify(f, c, t, lo, hi, (u32)B);
      return;
    }
    // one pair of Occ lines gives the ranks of all four characters
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
      for (u32 d = 1; d < 4; ++d) {  // the sibling counter of this level
        const u32 a = (pc + d) & 3u;
        const u32 l = sel4(a, nlo[0], nlo[1], nlo[2], nlo[3]), h = sel4(a, nhi[0], nhi[1], nhi[2], nhi[3]);
        if (l < h) mm_search<B - 1>(f, c, t + 1, l, h);
      }
    }
    lo = sel4(pc, nlo[0], nlo[1], nlo[2], nlo[3]);
    hi = sel4(pc, nhi[0], nhi[1], nhi[2], nhi[3]);
    ++t;
  }
  if (lo < hi) c.total += hi - lo;
}

// one strand of one head: the table start, then the levels
template <int E>
DG_DEV void mm_strand(const FmView& f, MmLane& c) {
  if (!(f.K && c.k >= f.K)) {
    mm_search<E>(f, c, 0, 0, (u32)f.n);
    return;
  }
  const u32 K = f.K;
  u64 code = 0;
  for (u32 t = 0; t < K; ++t) code |= (u64)mm_pat_code(f, c, t) << (2 * t);
  {
    const KtabEntry e0 = ktab_entry(f, code);
    ++c.tab;
    if (e0.lo < e0.hi) mm_search<E>(f, c, K, e0.lo, e0.hi);
  }
  if constexpr (E >= 1) {
    for (u32 i = 0; i < K; ++i)
      for (u64 a = 1; a < 4; ++a) {
        if (c.cap && c.total >= c.cap) return;
        const u64 code1 = code ^ (a << (2 * i));
        const KtabEntry e1 = ktab_entry(f, code1);
        ++c.tab;
        if (e1.lo < e1.hi) mm_search<E - 1>(f, c, K, e1.lo, e1.hi);
        if constexpr (E >= 2) {
          for (u32 j = 0; j < i; ++j)
            for (u64 b = 1; b < 4; ++b) {
              if (c.cap && c.total >= c.cap) return;
              const KtabEntry e2 = ktab_entry(f, code1 ^ (b << (2 * j)));
              ++c.tab;
              if (e2.lo < e2.hi) mm_search<E - 2>(f, c, K, e2.lo, e2.hi);
            }
        }
      }
  }
}

// ranks [r0, r1): every group head among them gets the saturated total of its k-mer in its slot of `start`
template <int E>
__global__ void __launch_bounds__(256) k_heads_mm(FmView f, u32 k, int forward_only, u32 W, u32 cap, u64 r0, u64 r1, const u64* hd, u32* start,
                                                 MmCounters* ctr) {
  const u64 i = r0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  MmLane c;
  c.pat = f.text;
  c.p = 0;
  c.k = k;
  c.rev = false;
  c.W = W;
  c.cap = cap;
  c.total = 0;
  c.steps = c.tab = c.rows = 0;
  u32 head = 0, early = 0;
  if (i < r1 && bit_at(hd, i)) {
    head = 1;
    c.p = f.sa[i];
    const u32 strands = forward_only ? 1u : 2u;
#pragma nounroll
    for (u32 s = 0; s < strands && !(cap && c.total >= cap); ++s) {  // (a loop: one copy of the search in the kernel)
      c.rev = s != 0;
      mm_strand<E>(f, c);
    }
    early = cap && c.total >= cap;
    start[i] = c.total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)c.total;
  }
  wave_add(&ctr->heads, head);  // (every lane of the wavefront is here)
  wave_add(&ctr->steps, c.steps);
  wave_add(&ctr->table_reads, c.tab);
  wave_add(&ctr->verified_rows, c.rows);
  wave_add(&ctr->early_exits, early);
}

}  // namespace dg
