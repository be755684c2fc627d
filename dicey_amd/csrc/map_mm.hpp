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
// Anchored (dg_query_map_anchored, query_anchor.hpp): the same search on an AnchLane, whose steps [t0, t1) must show the pattern's own
// character.  Lane::anchored is a compile-time trait, and every anchored condition below is written `Lane::anchored && ...` or as an
// `if constexpr`: on an MmLane the front end then drops it before anything is inlined.  A helper that merely returns false there is folded
// later and moves blocks of the e >= 1 kernels (DESIGN.md §10 has the instruction counts).  The kernels set the lane up with mm_lane_init
// and mm_set_strand and flush it with mm_flush; the strand loop itself stays in each kernel (§10 again).
// Degenerate (dg_query_map_iupac, query_iupac.hpp): the same search on a SetLane, whose k-mer w holds IUPAC codes.  The lane follows one
// concrete expansion v of w at a time, and the letters a substitution may NOT take at a pattern index are a 4-bit mask (mm_barred): the
// other members of the code's set always, every letter where v does not show the set's lowest member or the index is anchored.  Each
// window is then reached from exactly one expansion.  Lane::sets is a compile-time trait written like Lane::anchored.
#pragma once
#include "text_bits.hpp"

namespace dg {

struct MmCounters {  // device record, one wave_add per field and wavefront
  unsigned long long heads, steps, table_reads, verified_rows, early_exits;
};

struct MmLane {  // one lane's search of one k-mer w: its constants and the running results
  static constexpr bool anchored = false, sets = false;
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

struct AnchLane : MmLane {  // and the steps of the current strand at which the text must show the pattern's own character
  static constexpr bool anchored = true;
  u32 t0, t1;
};

// and w may hold IUPAC codes (k <= 64): the lane searches the expansion v of w that `sel` names.  All masks are over the indices of the
// CURRENT strand's pattern (bit i = pattern[i]; revcomp(w)[i] is w[k-1-i] with its set complemented)
struct SetLane : MmLane {
  static constexpr bool anchored = false, sets = true;
  u64 deg;         // the pattern's degenerate indices
  u64 sel0, sel1;  // bit planes of the member v shows there: 0 = the set's lowest code, the canonical member
  u64 allow;       // indices at which a letter outside the set may be substituted: not anchored, and v shows the canonical member
};

// the 4-bit set of an IUPAC letter over the codes of acgt_code (bit 0 = A, 1 = C, 2 = G, 3 = T); 0 for every other byte, U and lower
// case included.  The letters 'A'..'Y' are two words of nibbles
DG_DEV u32 iupac_set(u32 b) {
  constexpr u64 lo = 0x1ULL | 0xEULL << 4 | 0x2ULL << 8 | 0xDULL << 12 | 0x4ULL << 24 | 0xBULL << 28 | 0xCULL << 40 | 0x3ULL << 48 | 0xFULL << 52;
  constexpr u64 hi = 0x5ULL << 4 | 0x6ULL << 8 | 0x8ULL << 12 | 0x7ULL << 20 | 0x9ULL << 24 | 0xAULL << 32;  // from 'Q' on
  const u32 x = b - 'A';
  if (x > 24u) return 0;
  return (u32)((x < 16u ? lo >> (4 * x) : hi >> (4 * (x - 16u))) & 15u);
}

// the set at pattern index i of the lane's current strand, and the code v shows there
DG_DEV u32 mm_set_at(const SetLane& c, u32 i, u32& pc) {
  u32 S = iupac_set(c.pat[c.rev ? c.p + c.k - 1 - i : c.p + i]);
  if (c.rev) S = __brev(S) >> 28;  // the complement of code x is 3 - x
  u32 m = S;
  const u32 idx = (u32)((c.sel0 >> i) & 1ULL) | (u32)((c.sel1 >> i) & 1ULL) << 1;
  if (idx >= 1) m &= m - 1;
  if (idx >= 2) m &= m - 1;
  if (idx >= 3) m &= m - 1;
  pc = (u32)__ffs((int)m) - 1u;
  return S;
}
// the letters no substitution at pattern index i may take, S being the set there
DG_DEV u32 mm_barred(const SetLane& c, u32 i, u32 S) { return ((c.allow >> i) & 1ULL) ? S : 15u; }

// step t (pattern index k - 1 - t) takes no substitution by letter a (never on a lane without sets; callers write `Lane::sets &&` in front)
template <class Lane>
DG_DEV bool mm_step_bars(const Lane& c, u32 t, u32 a) {
  if constexpr (Lane::sets) {
    u32 pc;
    const u32 S = mm_set_at(c, c.k - 1 - t, pc);
    return (mm_barred(c, c.k - 1 - t, S) >> a) & 1u;
  } else return false;
}

// step t is anchored: no substitution there (never on a plain lane; callers write `Lane::anchored &&` in front, see the header)
template <class Lane>
DG_DEV bool mm_fixed_step(const Lane& c, u32 t) {
  if constexpr (Lane::anchored) return t >= c.t0 && t < c.t1;
  else return false;
}

// 0xFF in every byte b of the word at pattern index j whose index j + b lies in [i0, i1)
DG_DEV u64 anch_byte_mask(u32 j, u32 i0, u32 i1) {
  const u32 s = i0 > j ? i0 - j : 0u;
  const u32 e = i1 > j ? (i1 - j < 8u ? i1 - j : 8u) : 0u;
  if (s >= e) return 0;  // (so s <= 7)
  const u64 below_e = e == 8u ? ~0ULL : (1ULL << (8 * e)) - 1;
  return below_e & ~((1ULL << (8 * s)) - 1);
}

// the pattern's character met at backward-search step t (its LAST character at t = 0), as a code 0..3.  revcomp(w) from its last
// character to its first is w from its first to its last, complemented.
DG_DEV u32 mm_pat_code(const FmView& f, const MmLane& c, u32 t) {
  const u32 b = c.pat[c.rev ? c.p + t : c.p + c.k - 1 - t];
  const u32 x = acgt_code(b);
  return c.rev ? 3u - x : x;
}

DG_DEV u32 mm_pat_code(const FmView& f, const SetLane& c, u32 t) {
  u32 pc;
  (void)mm_set_at(c, c.k - 1 - t, pc);
  return pc;
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

// 0x80 in byte b for every bit b of the low eight of x
DG_DEV u64 mm_bits_to_bytes(u64 x) { return mm_nonzero_bytes(((x & 255ULL) * MM_ONES) & 0x8040201008040201ULL); }

// the degenerate indices among the first n of the word at pattern index j, one bit each (none on a lane without sets)
template <class Lane>
DG_DEV u64 mm_set_bytes(const Lane& c, u32 j, u32 n) {
  if constexpr (Lane::sets) return (c.deg >> j) & (n < 8 ? (1ULL << n) - 1 : 255ULL);
  else return 0;
}

// SetLane, the bytes `nz` flags (0x80 each) among the first n of the word at pattern index j, whose text bytes are y; mism counts them all
// already.  A degenerate index is flagged unless the text shows the very same IUPAC byte, which is no occurrence; where the text shows v's
// letter it is taken off the count; a text letter inside the set but not v's belongs to another expansion; one outside costs its 1 where
// mm_barred lets it.  A word without a degenerate index takes the anchored lane's byte masks.  False: the row is rejected
DG_DEV bool mm_set_word(const SetLane& c, u32 j, u32 n, u64 y, u64 nz, u32& mism, u32 budget) {
  const u64 deg8 = mm_set_bytes(c, j, n);
  if (deg8 == 0) {
    const u64 free8 = mm_bits_to_bytes(c.allow >> j);
    return mism <= budget && (nz & (~mm_acgt_bytes(y) | ~free8)) == 0;
  }
  if (mm_bits_to_bytes(deg8) & ~nz) return false;
  for (u64 z = nz; z; z &= z - 1) {
    const u32 b = (u32)__builtin_ctzll(z) >> 3;
    const u32 Y = iupac_set((u32)(y >> (8 * b)) & 255u);
    if (__popc(Y) != 1) return false;  // the text shows no A/C/G/T there
    u32 pc;
    const u32 S = mm_set_at(c, j + b, pc);
    if (Y == 1u << pc) {
      --mism;
      continue;
    }
    if (mm_barred(c, j + b, S) & Y) return false;
  }
  return mism <= budget;
}

// rows [lo, hi) hold the suffixes that start with the t characters consumed so far: count those whose k - t characters in front spell
// the rest of the pattern with at most `budget` substitutions.  Anchored: a mismatching byte whose pattern index lies in the anchored
// range [k - t1, k - t0) rejects the row, as a byte outside A/C/G/T does
template <class Lane>
DG_DEV void mm_verify(const FmView& f, Lane& c, u32 t, u32 lo, u32 hi, u32 budget) {
  const u32 m = c.k - t;
  [[maybe_unused]] u32 i0 = 0, i1 = 0;  // the anchored index range
  if constexpr (Lane::anchored) i0 = c.k - c.t1, i1 = c.k - c.t0;
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
      if (nz || (Lane::sets && mm_set_bytes(c, j, m - j))) {  // (a degenerate index that is not flagged: the text shows the same IUPAC byte)
        mism += (u32)__popcll(nz);
        // (both forms leave the byte masks behind the budget test: they are formed only while the row is still within budget)
        if constexpr (Lane::sets) ok = mm_set_word(c, j, m - j, y, nz, mism, budget);
        else if constexpr (Lane::anchored) ok = mism <= budget && (nz & (~mm_acgt_bytes(y) | anch_byte_mask(j, i0, i1))) == 0;
        else ok = mism <= budget && (nz & ~mm_acgt_bytes(y)) == 0;
      }
    }
    c.total += ok;
  }
}

// the string whose last t characters have the interval [lo, hi), extended to the pattern's full length with at most B substitutions
// (no sibling is spawned at an anchored step)
template <int B, class Lane>
DG_DEV void mm_search(const FmView& f, Lane& c, u32 t, u32 lo, u32 hi) {
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
      if (!(Lane::anchored && mm_fixed_step(c, t))) {
        for (u32 d = 1; d < 4; ++d) {  // the sibling counter of this level
          const u32 a = (pc + d) & 3u;
          if (Lane::sets && mm_step_bars(c, t, a)) continue;
          const u32 l = sel4(a, nlo[0], nlo[1], nlo[2], nlo[3]), h = sel4(a, nhi[0], nhi[1], nhi[2], nhi[3]);
          if (l < h) mm_search<B - 1>(f, c, t + 1, l, h);
        }
      }
    }
    lo = sel4(pc, nlo[0], nlo[1], nlo[2], nlo[3]);
    hi = sel4(pc, nhi[0], nhi[1], nhi[2], nhi[3]);
    ++t;
  }
  if (lo < hi) c.total += hi - lo;
}

// one strand of one head: the table start (substitutions at its free steps only), then the levels
template <int E, class Lane>
DG_DEV void mm_strand(const FmView& f, Lane& c) {
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
    for (u32 i = 0; i < K; ++i) {
      if (Lane::anchored && mm_fixed_step(c, i)) continue;
      for (u64 a = 1; a < 4; ++a) {
        if (Lane::sets && mm_step_bars(c, i, (u32)((code >> (2 * i)) ^ a) & 3u)) continue;
        if (c.cap && c.total >= c.cap) return;
        const u64 code1 = code ^ (a << (2 * i));
        const KtabEntry e1 = ktab_entry(f, code1);
        ++c.tab;
        if (e1.lo < e1.hi) mm_search<E - 1>(f, c, K, e1.lo, e1.hi);
        if constexpr (E >= 2) {
          for (u32 j = 0; j < i; ++j) {
            if (Lane::anchored && mm_fixed_step(c, j)) continue;
            for (u64 b = 1; b < 4; ++b) {
              if (Lane::sets && mm_step_bars(c, j, (u32)((code >> (2 * j)) ^ b) & 3u)) continue;
              if (c.cap && c.total >= c.cap) return;
              const KtabEntry e2 = ktab_entry(f, code1 ^ (b << (2 * j)));
              ++c.tab;
              if (e2.lo < e2.hi) mm_search<E - 2>(f, c, K, e2.lo, e2.hi);
            }
          }
        }
      }
    }
  }
}

// a lane at position p of `pat` with nothing counted yet
template <class Lane>
DG_DEV void mm_lane_init(Lane& c, const u8* pat, u64 p, u32 k, u32 W, u32 cap) {
  c.pat = pat;
  c.p = p;
  c.k = k;
  c.rev = false;
  c.W = W;
  c.cap = cap;
  c.total = 0;
  c.steps = c.tab = c.rows = 0;
  if constexpr (Lane::anchored) c.t0 = c.t1 = 0;
  if constexpr (Lane::sets) c.deg = c.sel0 = c.sel1 = c.allow = 0;
}

// the lane's next mm_strand is of its k-mer w or, with rev, of revcomp(w).  On an anchored lane the last `anchor` bases of w are exact:
// step t consumes pattern index k-1-t, so they are the steps [0, anchor) of w and, being revcomp(w)'s first bases, its steps [k - anchor, k)
template <class Lane>
DG_DEV void mm_set_strand(Lane& c, bool rev, u32 anchor = 0) {
  c.rev = rev;
  if constexpr (Lane::anchored) {
    c.t0 = rev ? c.k - anchor : 0u;
    c.t1 = rev ? c.k : anchor;
  }
}

// the lane's search counters into a device record (every lane of the wavefront must be here)
template <class Counters>
DG_DEV void mm_flush(Counters* ctr, const MmLane& c) {
  wave_add(&ctr->steps, c.steps);
  wave_add(&ctr->table_reads, c.tab);
  wave_add(&ctr->verified_rows, c.rows);
}

// ranks [r0, r1): every group head among them gets the saturated total of its k-mer in its slot of `start`
template <int E>
__global__ void __launch_bounds__(256) k_heads_mm(FmView f, u32 k, int forward_only, u32 W, u32 cap, u64 r0, u64 r1, const u64* hd, u32* start,
                                                 MmCounters* ctr) {
  const u64 i = r0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
  MmLane c;
  mm_lane_init(c, f.text, 0, k, W, cap);
  u32 head = 0, early = 0;
  if (i < r1 && bit_at(hd, i)) {
    head = 1;
    c.p = f.sa[i];
    const u32 strands = forward_only ? 1u : 2u;
#pragma nounroll
    for (u32 s = 0; s < strands && !(cap && c.total >= cap); ++s) {  // (a loop: one copy of the search in the kernel)
      mm_set_strand(c, s != 0);
      mm_strand<E>(f, c);
    }
    early = cap && c.total >= cap;
    start[i] = c.total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)c.total;
  }
  wave_add(&ctr->heads, head);  // (every lane of the wavefront is here)
  mm_flush(ctr, c);
  wave_add(&ctr->early_exits, early);
}

}  // namespace dg
