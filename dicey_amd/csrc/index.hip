// dg_index_open / dg_index_close / dg_index_stats: load the sdsl csa_wt<> file unchanged into HBM and derive the
// search layouts on the device.  Replaces load_from_checked_file (reference src/hunter.h:253-260, src/silica.h:340-347).
#include <chrono>
#include <memory>

#include "dev_mem.hpp"
#include "devfm.hpp"
#include "index_plan.hpp"
#include "index_internal.hpp"
#include <rocprim/device/device_scan.hpp>

#include "sdsl_file.hpp"

namespace dg {

std::string& last_error() {
  static thread_local std::string e;
  return e;
}
int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  last_error() = buf;
  return code;
}

// ------------------------------------------------------------------------------------------------------------
// Derivation kernels (load time).  All are one-thread-one-chain; no inter-thread communication.
// ------------------------------------------------------------------------------------------------------------

// Thread h decodes BWT[64h, 64h+64) through the wavelet tree into three plane words and per-symbol counts.
__global__ void k_decode_bwt(FmView f, OccBlock* occ, u32* half_cnt, u64 nhalf) {
  u64 h = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= nhalf) return;
  u64 p0 = 0, p1 = 0, p2 = 0;
  u32 c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  u64 base = h << 6;
  for (u32 j = 0; j < 64; ++j) {
    u64 i = base + j;
    if (i >= f.n) break;
    u32 sym;
    (void)wt_inverse_select(f, i, sym);
    u32 code = code_of_byte(sym);
    p0 |= (u64)(code & 1) << j;
    p1 |= (u64)((code >> 1) & 1) << j;
    p2 |= (u64)(code >> 2) << j;
    c0 += code == 0;
    c1 += code == 1;
    c2 += code == 2;
    c3 += code == 3;
  }
  OccBlock* b = occ + (h >> 1);
  u32 w = (u32)(h & 1);
  b->pl[0][w] = p0;
  b->pl[1][w] = p1;
  b->pl[2][w] = p2;
  half_cnt[h] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);  // each <= 64
}

// Thread t sums HALF_PER_CHUNK half-block counts -> chunk totals (host scans the chunk totals).
static constexpr u32 HALF_PER_CHUNK = 64;
__global__ void k_chunk_totals(const u32* half_cnt, u64 nhalf, u32* chunk_tot /*[nchunk][4]*/, u64 nchunk) {
  u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nchunk) return;
  u32 s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  u64 b = t * HALF_PER_CHUNK, e = b + HALF_PER_CHUNK < nhalf ? b + HALF_PER_CHUNK : nhalf;
  for (u64 h = b; h < e; ++h) {
    u32 v = half_cnt[h];
    s0 += v & 255;
    s1 += (v >> 8) & 255;
    s2 += (v >> 16) & 255;
    s3 += v >> 24;
  }
  chunk_tot[t * 4 + 0] = s0;
  chunk_tot[t * 4 + 1] = s1;
  chunk_tot[t * 4 + 2] = s2;
  chunk_tot[t * 4 + 3] = s3;
}
// chunk_base = exclusive scan of chunk_tot; writes the running counts into every block header
__global__ void k_block_counts(const u32* half_cnt, u64 nhalf, const u32* chunk_base, u64 nchunk, OccBlock* occ,
                               u64 nblk) {
  u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nchunk) return;
  u32 s0 = chunk_base[t * 4], s1 = chunk_base[t * 4 + 1], s2 = chunk_base[t * 4 + 2], s3 = chunk_base[t * 4 + 3];
  u64 b = t * HALF_PER_CHUNK, e = b + HALF_PER_CHUNK;
  for (u64 h = b; h < e; ++h) {
    if (!(h & 1) && (h >> 1) < nblk) {
      OccBlock* ob = occ + (h >> 1);
      ob->cnt[0] = s0;
      ob->cnt[1] = s1;
      ob->cnt[2] = s2;
      ob->cnt[3] = s3;
    }
    if (h < nhalf) {
      u32 v = half_cnt[h];
      s0 += v & 255;
      s1 += (v >> 8) & 255;
      s2 += (v >> 16) & 255;
      s3 += v >> 24;
    }
  }
}

// Text from ISA samples: sample k is ISA[64k]; walking LF from it yields T[64k-1], T[64k-2], ...
// Thread 0 starts at ISA[0] and therefore produces the tail T[n-1] .. T[64*(ns-1)].
__global__ void k_derive_text(FmView f, u8* text) {
  u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= f.n_isa_samp) return;
  u64 i = packed_get(f.isa_samp, f.samp_width, k);
  u64 hi, lo;  // writes text[lo, hi)
  if (k == 0) {
    hi = f.n;
    lo = (f.n_isa_samp - 1) * 64;
  } else {
    hi = k * 64;
    lo = hi - 64;
  }
  for (u64 p = hi; p > lo;) {
    u32 sym;
    i = lf_step(f, i, sym);
    text[--p] = (u8)sym;
  }
}

// The same walk also knows the rank of every suffix it passes: after the LF step that produced T[p], i is the rank of
// suffix p.  isa[p] = i is written next to text[p] (consecutive p per lane), and the suffix array is obtained from it by
// a sort (derive_sa_by_sort) instead of a second walk with scattered stores.
__global__ void k_derive_text_isa(FmView f, u8* text, u32* isa) {
  u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= f.n_isa_samp) return;
  u64 i = packed_get(f.isa_samp, f.samp_width, k);
  u64 hi, lo;  // writes [lo, hi)
  if (k == 0) {
    hi = f.n;
    lo = (f.n_isa_samp - 1) * 64;
  } else {
    hi = k * 64;
    lo = hi - 64;
  }
  for (u64 p = hi; p > lo;) {
    u32 sym;
    i = lf_step(f, i, sym);
    --p;
    text[p] = (u8)sym;
    isa[p] = (u32)i;
  }
}
// the file's own SA samples must agree with the suffix array derived from its ISA samples
__global__ void k_check_sa_samples(FmView f, const u32* sa, u32* bad) {
  u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= f.n_sa_samp) return;
  if (packed_get(f.sa_samp, f.samp_width, j) != sa[j * 32]) atomicAdd(bad, 1u);
}

// Full SA from SA samples: SA[LF(i)] = SA[i] - 1.  Thread j owns the LF chain that leaves index 32j and stops at
// the next index that is itself sampled; LF is a permutation, so every unsampled index is written exactly once.
__global__ void k_derive_sa(FmView f, u32* sa) {
  u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= f.n_sa_samp) return;
  u64 v = packed_get(f.sa_samp, f.samp_width, j);
  u64 i = j * 32;
  sa[i] = (u32)v;
  for (;;) {
    u32 sym;
    i = lf_step(f, i, sym);
    if ((i & 31) == 0) break;
    v = v ? v - 1 : f.n - 1;
    sa[i] = (u32)v;
  }
}

// Self-check on a pseudo-random sample of SA indices: BWT[i] == T[SA[i]-1], and suffix SA[i] <= suffix SA[i+1]
// on their first 48 bytes.  Catches a mis-parsed file before any query is answered.
__global__ void k_selfcheck(FmView f, u64 nsample, u32* bad) {
  u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nsample) return;
  u64 x = (t + 1) * 0x9E3779B97F4A7C15ULL;
  x ^= x >> 29;
  x *= 0xBF58476D1CE4E5B9ULL;
  x ^= x >> 32;
  u64 i = x % f.n;
  u32 sym;
  (void)lf_step(f, i, sym);
  u64 p = f.sa[i];
  u64 prev = p ? p - 1 : f.n - 1;
  bool ok = f.text[prev] == (u8)sym && p < f.n;
  if (i + 1 < f.n) {
    u64 q = f.sa[i + 1];
    for (u32 k = 0; k < 48; ++k) {
      u64 a = p + k, b = q + k;
      if (a >= f.n || b >= f.n) break;
      u8 ca = f.text[a], cb = f.text[b];
      if (ca != cb) {
        ok = ok && ca < cb;
        break;
      }
    }
  }
  if (!ok) atomicAdd(bad, 1u);
}

// K-mer table: thread i looks at the K-mer that starts suffix SA[i]; the first / last suffix of each run of equal K-mers
// writes the interval bounds.  K-mers that run into a separator, an N or the end of the text have no entry.
// the K-mer and the K2-mer (K2 > K, or 0) that start at text position p (K, K2 <= 24).  The text arrives as four aligned
// 64-bit words (24 characters at any byte offset; the buffer is padded) in one round trip — a byte loop that may stop at the
// first other letter cannot have its loads hoisted, so it waited for memory once per character (r02: 0.45-0.70 s of table
// fill).  Which bytes are A/C/G/T is an exact zero-byte test against the four letters; ((b >> 1) ^ (b >> 2)) & 3 maps
// A,C,G,T to 0..3; the 2-bit fields of a byte-swapped word are squeezed together so that the first character ends up on top.
DG_DEV u64 acgt_flags(u64 w) {  // 0x80 in every byte that is one of A, C, G, T
  u64 f = 0;
  const u64 lo7 = 0x7F7F7F7F7F7F7F7FULL;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const u64 v = w ^ ((u64)(k == 0 ? 'A' : k == 1 ? 'C' : k == 2 ? 'G' : 'T') * 0x0101010101010101ULL);
    f |= ~(((v & lo7) + lo7) | v | lo7);
  }
  return f;
}
DG_DEV u32 pack8(u64 w) {  // 8 characters (first one in the lowest byte) -> 16 bits, first character in bits 15-14
  w = __builtin_bswap64(w);
  u64 x = ((w >> 1) ^ (w >> 2)) & 0x0303030303030303ULL;
  x = (x | (x >> 6)) & 0x000F000F000F000FULL;
  x = (x | (x >> 12)) & 0x000000FF000000FFULL;
  x = (x | (x >> 24)) & 0xFFFFULL;
  return (u32)x;
}
DG_DEV void kmer_codes_at(const FmView& f, u64 p, u32 K, u32 K2, u64& code, u64& code2) {
  const u64 none = 1ULL << 63;
  const u64* src = reinterpret_cast<const u64*>(f.text + (p & ~7ULL));
  const u32 sh = (u32)(p & 7) * 8;
  const u64 w0 = src[0], w1 = src[1], w2 = src[2], w3 = src[3];
  const u64 b0 = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
  const u64 b1 = sh ? (w1 >> sh) | (w2 << (64 - sh)) : w1;
  const u64 b2 = sh ? (w2 >> sh) | (w3 << (64 - sh)) : w2;
  // bit i of `valid` <=> character i is A/C/G/T
  const u64 gather = 0x0102040810204080ULL, ones = 0x0101010101010101ULL;
  const u32 v0 = (u32)((((acgt_flags(b0) >> 7) & ones) * gather) >> 56), v1 = (u32)((((acgt_flags(b1) >> 7) & ones) * gather) >> 56),
            v2 = (u32)((((acgt_flags(b2) >> 7) & ones) * gather) >> 56);
  const u32 valid = v0 | (v1 << 8) | (v2 << 16);
  u32 got = (u32)__builtin_ctz(~valid | (1u << 24));  // characters before the first other letter, at most 24
  const u64 room = f.n - 1 - p;                        // characters before the sentinel (p < n - 1 for every suffix but the last)
  if (p >= f.n - 1) got = 0;
  else if (got > room) got = (u32)room;
  const u64 acc = (u64)pack8(b0) << 32 | (u64)pack8(b1) << 16 | (u64)pack8(b2);  // 24 characters, the first on top (bits 47-46)
  code = got >= K ? acc >> (2 * (24 - K)) : none;
  code2 = (K2 && got >= K2) ? acc >> (2 * (24 - K2)) : none;
}

// ---- presence filter (FmView::kf) ----
// copy 0 (in-line bits = the low 9 code bits = address order of the table): one coalesced pass over the table
__global__ void __launch_bounds__(256) k_kf_from_table(const uint2* tab, u64 entries, u32* out) {  // entries: multiple of 64
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < entries; i += stride) {  // a launch holds < 2^32 threads
    const uint2 e = tab[i];
    const unsigned long long m = __ballot(e.x < e.y);
    if ((threadIdx.x & 63) == 0) *reinterpret_cast<unsigned long long*>(out + (i >> 5)) = m;
  }
}
// any copy, one lane per output word, straight from the table: small tables, and the lane-independent debugging build
__global__ void k_kf_generic(const uint2* tab, u32 bits, u32 s, u32* out, u64 nwords) {
  const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwords) return;
  const u64 line = w >> 4;
  u32 v = 0;
  for (u32 i = 0; i < 32; ++i) {
    const u64 inl = ((w & 15) << 5) | i;
    const u64 code = (line & ((1ULL << s) - 1)) | (inl << s) | ((line >> s) << (s + 9));
    if (code >> bits) continue;
    const uint2 e = tab[code];
    v |= (u32)(e.x < e.y) << i;
  }
  out[w] = v;
}
// copy with in-line bits [s, s+9), s >= 8, from copy 0: a workgroup owns the 2^17 codes that share everything but those
// nine bits and the low eight; lane M reads the 256 bits of its in-line value (32 contiguous bytes of copy 0), the
// 512 x 256 bit matrix is turned by ballots and leaves as 256 consecutive lines of the new copy.
__global__ void __launch_bounds__(512) k_kf_transpose(const u32* r0, u32* out, u32 s) {
  __shared__ unsigned long long tile[256][8];  // [line][wavefront]: 64 in-line bits each
  const u64 T = blockIdx.x;
  const u64 lowpart = (T & ((1ULL << (s - 8)) - 1)) << 8, high = T >> (s - 8);
  const u32 M = threadIdx.x, wave = M >> 6, lane = M & 63;
  const u64 src_bit = lowpart | ((u64)M << s) | (high << (s + 9));
  const uint4* src = reinterpret_cast<const uint4*>(r0 + (src_bit >> 5));
  const uint4 a = src[0], b = src[1];
  const u32 word[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  unsigned long long keep[4] = {0, 0, 0, 0};
#pragma unroll
  for (int wi = 0; wi < 8; ++wi)
#pragma unroll
    for (int bit = 0; bit < 32; ++bit) {
      const unsigned long long m = __ballot((word[wi] >> bit) & 1u);
      const int l = wi * 32 + bit;
      if ((int)lane == (l & 63)) keep[l >> 6] = m;
    }
#pragma unroll
  for (int k = 0; k < 4; ++k) tile[64 * k + lane][wave] = keep[k];
  __syncthreads();
  const u64 line0 = lowpart | (high << s);
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(out + line0 * 16);
  const unsigned long long* flat = &tile[0][0];
  for (u32 k = threadIdx.x; k < 256 * 8; k += 512) dst[k] = flat[k];
}

// any copy, one lane per output word, from copy 0 (in-line bits = the low nine code bits, i.e. bit address = code): the long
// filter has no table to read
__global__ void k_kf_generic0(const u32* r0, u32 bits, u32 s, u32* out, u64 nwords) {
  const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwords) return;
  const u64 line = w >> 4;
  u32 v = 0;
  for (u32 i = 0; i < 32; ++i) {
    const u64 inl = ((w & 15) << 5) | i;
    const u64 code = (line & ((1ULL << s) - 1)) | (inl << s) | ((line >> s) << (s + 9));
    if (code >> bits) continue;
    v |= ((r0[code >> 5] >> (code & 31)) & 1u) << i;
  }
  out[w] = v;
}

// Number of copies, their in-line bit fields (spread evenly over the code) and, per window position, the copy to ask.
static void kf_layout(KFilter& kf, u32 k) {
  const u32 bits = 2 * k;
  u32 nr = bits <= 9 ? 1u : (bits - 9 + 7) / 8 + 1;
  if (nr > 4) nr = 4;
  kf.k = k;
  kf.nr = nr;
  for (u32 r = 0; r < 4; ++r) kf.s[r] = (nr > 1 && r < nr) ? (r * (bits - 9) + (nr - 1) / 2) / (nr - 1) : 0u;
  kf.pick = 0;
  for (u32 t = 0; t < 32; ++t) {
    u32 best = 0;
    int best_score = -1000;
    for (u32 r = 0; r < nr; ++r) {
      const int lo = (int)kf.s[r], hi = lo + 9, b0 = 2 * (int)t;
      const int covered = (b0 >= lo && b0 < hi) + (b0 + 1 >= lo && b0 + 1 < hi);
      const int off = 2 * b0 + 1 - (2 * lo + 8);  // twice the distance of the character from the field's centre
      const int score = covered * 100 - (off < 0 ? -off : off);
      if (score > best_score) {
        best_score = score;
        best = r;
      }
    }
    kf.pick |= (u64)best << (2 * t);
  }
}

// Copies of a presence filter.  Copy 0 comes from the table (tab != nullptr: one ballot pass) or is already in place
// (copy0: the long filter, whose bits the table-fill kernel sets); the others are bit-matrix transposes of copy 0.
static int build_filter(dg_index* ix, KFilter& kf, u32 k, const uint2* tab, u32* copy0) {
  const u32 bits = 2 * k;
  if (bits < 17 || exp_env("DICEY_NO_KMER_FILTER")) return DG_OK;  // a table this small is cache resident anyway
  const u64 entries = 1ULL << bits, nwords = entries >> 5;
  kf_layout(kf, k);
  const u32 nr = kf.nr;
  kf.nr = 0;  // until the copies exist
  const u32 TB = 256;
  for (u32 r = 0; r < nr; ++r) {
    const u32 s = kf.s[r];
    u32* bm = nullptr;
    if (r == 0 && copy0) bm = copy0;
    else DG_TRY(ix->own((void**)&bm, plan::filter_copy_bytes(k)));
    if (r == 0 && copy0) {
      // filled by the caller
    } else if (r == 0) {
      hipLaunchKernelGGL(k_kf_from_table, dim3((u32)std::min<u64>(entries / TB, 1u << 20)), dim3(TB), 0, ix->stream, tab, entries, bm);
    } else if (s < 8) {
      if (tab) hipLaunchKernelGGL(k_kf_generic, dim3(ceil_div(nwords, TB)), dim3(TB), 0, ix->stream, tab, bits, s, bm, nwords);
      else hipLaunchKernelGGL(k_kf_generic0, dim3(ceil_div(nwords, TB)), dim3(TB), 0, ix->stream, (const u32*)kf.cp[0], bits, s, bm, nwords);
    } else {
      hipLaunchKernelGGL(k_kf_transpose, dim3((u32)(entries >> 17)), dim3(512), 0, ix->stream, kf.cp[0], bm, s);
    }
    kf.cp[r] = bm;
  }
  DG_HIP(hipStreamSynchronize(ix->stream));
  DG_HIP(hipGetLastError());
  kf.nr = nr;
  return DG_OK;
}

// The table fill, one text gather per lane: the K-mers of the neighbouring suffixes come from the neighbouring lanes (the first /
// last lane of a wavefront read theirs).  kf2: copy 0 of the long presence filter (bit address = K2-mer code), zeroed by the caller;
// nullptr = none
__global__ void __launch_bounds__(256) k_kmer_table_wave(FmView f, uint2* tab, u32 K, u32 K2, u32* kf2) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const u64 none = 1ULL << 63;
  u64 me = none, me2 = none, x2;
  if (i < f.n) kmer_codes_at(f, f.sa[i], K, kf2 ? K2 : 0u, me, me2);
  const u32 lane = threadIdx.x & 63;
  u32 plo = __shfl_up((u32)me, 1), phi = __shfl_up((u32)(me >> 32), 1);
  u32 nlo = __shfl_down((u32)me, 1), nhi = __shfl_down((u32)(me >> 32), 1);
  u64 prev = (u64)phi << 32 | plo, next = (u64)nhi << 32 | nlo;
  const u64 prev2 = (u64)__shfl_up((u32)(me2 >> 32), 1) << 32 | __shfl_up((u32)me2, 1);
  if (i >= f.n || (me >> 63)) return;
  if (lane == 0) {
    prev = none;
    if (i) kmer_codes_at(f, f.sa[i - 1], K, 0u, prev, x2);
  }
  if (lane == 63) {
    next = none;
    if (i + 1 < f.n) kmer_codes_at(f, f.sa[i + 1], K, 0u, next, x2);
  }
  if (prev != me) tab[me].x = (u32)i;
  if (next != me) tab[me].y = (u32)(i + 1);
  // suffixes are sorted, so equal K2-mers are neighbours: the first lane of a run sets the bit
  if (kf2 && !(me2 >> 63) && (lane == 0 || prev2 != me2)) atomicOr(&kf2[me2 >> 5], 1u << (me2 & 31));
}

// FmView::nrun_min: the length of the text's shortest run of 'N', capped at 64 (r05).  A lane per text position; the lane of a run's
// first character looks at most 63 characters ahead.  A query character outside A,C,G,T is searched as 'N' (util.h:208-219) and
// matches only an 'N' of the text: a neighbourhood string whose N-block has other characters on both sides needs a run of exactly
// that length — k_search prunes such strings when no run is that short (hunt_search.hpp).
__global__ void __launch_bounds__(256) k_nrun_min(const u8* text, u64 n, u32* out) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
    if (text[i] != 'N' || (i && text[i - 1] == 'N')) continue;
    u32 len = 1;
    while (len < 64 && i + len < n && text[i + len] == 'N') ++len;
    if (len < 64) atomicMin(out, len);
  }
}

// FmView::pre5: the five characters in front of every suffix, in suffix-array order (one text gather per lane) — and, with the same
// gather, FmView::sax: {SA[i], context word} (devfm.hpp: the two characters in front of the suffix and the thirteen characters
// T[p+16 .. p+28], two bits each, bit 31 when any of them is not A/C/G/T or lies outside the text).  sax == nullptr: pre5 only.
__global__ void __launch_bounds__(256) k_pre5(const u32* sa, const u8* text, u64 n, u16* out, uint2* sax) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64 p = sa[i];
  u32 v = 0;
#pragma unroll
  for (u32 k = 1; k <= 5; ++k) {
    u32 c = 7u;
    if (p >= k) {
      const u32 b = text[p - k];
      c = b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 7u;
    }
    v |= c << (3 * (k - 1));
  }
  out[i] = (u16)v;
  if (!sax) return;
  const u32 c1 = v & 7u, c2 = (v >> 3) & 7u;
  u32 ctx = (c1 & 3u) | ((c2 & 3u) << 2);
  bool esc = c1 > 3u || c2 > 3u;
  const u64 q = p + SAX_POST_OFF;
  if (q + SAX_POST_N > n) esc = true;  // (text[n - 1] is the sentinel: it escapes by itself)
  else {
    // thirteen bytes from q, read as three aligned 64-bit words (the text block is 64-byte aligned and 64 bytes longer than n)
    const u64* tw = reinterpret_cast<const u64*>(text) + (q >> 3);
    const u32 sh = (u32)(q & 7u) * 8u;
    const u64 a = tw[0], b = tw[1], c = tw[2];
    const u64 w0 = sh ? (a >> sh) | (b << (64u - sh)) : a, w1 = sh ? (b >> sh) | (c << (64u - sh)) : b;
#pragma unroll
    for (u32 j = 0; j < SAX_POST_N; ++j) {
      const u32 ch = (u32)((j < 8 ? w0 >> (8 * j) : w1 >> (8 * (j - 8))) & 255u);
      const u32 code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 7u;
      esc = esc || code > 3u;
      ctx |= (code & 3u) << (4 + 2 * j);
    }
  }
  sax[i] = make_uint2((u32)p, esc ? (ctx | SAX_ESCAPE) : ctx);
}

// FmView::plv, one level: the flags "text position below x" of every suffix-array index as 64-bit words (seven per 64-byte
// line of the rank directory, one wavefront per line), the line's count aside ...
__global__ void __launch_bounds__(256) k_plv_bits(const u32* sa, u64 n, u64 x, u64* dir, u32* cnt, u64 nlines) {
  const u64 line = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
  const u32 lane = threadIdx.x & 63;
  if (line >= nlines) return;  // (the same for a whole wavefront)
  u32 total = 0;
  u64 mine = 0;
  for (u32 j = 0; j < 7; ++j) {
    const u64 i = line * FmView::PLV_LINE + 64 * j + lane;
    const unsigned long long w = __ballot(i < n && (u64)sa[i] < x);
    if (lane == j) mine = w;
    total += (u32)__popcll(w);
  }
  if (lane < 7) dir[line * 8 + 1 + lane] = mine;
  if (lane == 0) cnt[line] = total;
}
// ... and, behind the exclusive scan of the counts: the count before every line, and the flagged suffixes' records in their order
__global__ void __launch_bounds__(256) k_plv_fill(const uint2* sax, const u32* before, u64* dir, uint2* rec, u64 nlines) {
  const u64 line = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
  const u32 lane = threadIdx.x & 63;
  if (line >= nlines) return;
  u64 base = before[line];
  if (lane == 0) dir[line * 8] = base;
  for (u32 j = 0; j < 7; ++j) {
    const u64 w = dir[line * 8 + 1 + j];
    if ((w >> lane) & 1ULL) rec[base + (u64)__popcll(w & ((1ULL << lane) - 1ULL))] = sax[line * FmView::PLV_LINE + 64 * j + lane];
    base += (u64)__popcll(w);
  }
}

// The table's final entry format (FmView::ktab): (lo, hi) as the fill pass left them -> (lo, width | pre5[lo] << 16) for widths below
// 2^16, (lo, 0x80000000 | width) above.  pre: nullptr when the preceding characters were not built (the field then reads 0x7FFF,
// which the search kernels never consult without FmView::pre5).
__global__ void __launch_bounds__(256) k_ktab_pack(uint2* tab, u64 entries, const u16* pre) {
  // (grid-stride: a launch of entries / 256 workgroups is 2^32 threads for the order-16 table, one more than HIP takes)
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < entries; i += (u64)gridDim.x * blockDim.x) {
    const uint2 e = tab[i];
    const u32 w = e.y - e.x;  // (absent K-mers are (0, 0))
    u32 y;
    if (w >= 65536u) y = 0x80000000u | w;
    else y = w | ((w && pre ? (u32)pre[e.x] & 0x7FFFu : 0x7FFFu) << 16);
    tab[i].y = y;
  }
}

// Block minima of the suffix array, fan-out 8 (FmView::samin): one lane per block, two 16-byte loads.
__global__ void __launch_bounds__(256) k_block_min8(const u32* in, u64 n_in, u32* out, u64 n_out, u64 n_out_padded) {
  const u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_out_padded) return;
  u32 m = 0xFFFFFFFFu;
  if (b < n_out) {
    const u64 i0 = b * 8;
    if (i0 + 8 <= n_in) {
      const uint4 x = *reinterpret_cast<const uint4*>(in + i0), y = *reinterpret_cast<const uint4*>(in + i0 + 4);
      m = min(min(min(x.x, x.y), min(x.z, x.w)), min(min(y.x, y.y), min(y.z, y.w)));
    } else {
      for (u64 i = i0; i < n_in; ++i) m = min(m, in[i]);
    }
  }
  out[b] = m;
}

struct PhaseClock {  // DICEY_TIMING=1: host wall clock of the load phases on stderr
  bool on = std::getenv("DICEY_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void lap(const char* what) {
    if (!on) return;
    auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "dicey timing: %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};

// ------------------------------------------------------------------------------------------------------------
// The open as stages (derive_layouts below is their list).  A stage owns its temporaries through a scratch local to it; what stays is
// the index's from dg_index::own / try_own on; the decisions between the launches are index_plan.hpp's.  A stage returns with the
// stream synchronised, so the free bytes the next one asks for are the ones it left.
// ------------------------------------------------------------------------------------------------------------
static_assert(sizeof(OccBlock) == 64 && plan::MAXPLV == FmView::MAXPLV && plan::PLV_LINE == FmView::PLV_LINE, "index_plan.hpp");
static constexpr u32 TB = 256;

// Occ blocks from the decoded BWT; C[] of the file must agree with what the decoded BWT holds
static int stage_occ(dg_index* ix, const SdslCsa& c) {
  FmView& f = ix->view;
  const u64 nblk = plan::occ_blocks(f.n), nhalf = nblk * 2;
  const u64 nchunk = (nhalf + HALF_PER_CHUNK - 1) / HALF_PER_CHUNK;
  OccBlock* occ = nullptr;
  u32 *half_cnt = nullptr, *chunk = nullptr;
  DG_TRY(ix->own((void**)&occ, nblk * sizeof(OccBlock)));
  DG_HIP(hipMemsetAsync(occ, 0, nblk * sizeof(OccBlock), ix->stream));
  StreamScratch tmp(ix->stream);  // gone before the text is allocated
  DG_TRY(tmp.big((void**)&half_cnt, nhalf * 4));
  DG_TRY(tmp.small((void**)&chunk, nchunk * 16));
  hipLaunchKernelGGL(k_decode_bwt, dim3(ceil_div(nhalf, TB)), dim3(TB), 0, ix->stream, f, occ, half_cnt, nhalf);
  hipLaunchKernelGGL(k_chunk_totals, dim3(ceil_div(nchunk, TB)), dim3(TB), 0, ix->stream, half_cnt, nhalf, chunk, nchunk);
  std::vector<u32> tot(nchunk * 4);
  DG_HIP(hipMemcpyAsync(tot.data(), chunk, nchunk * 16, hipMemcpyDeviceToHost, ix->stream));
  DG_HIP(hipStreamSynchronize(ix->stream));
  u64 run[4] = {0, 0, 0, 0};
  for (u64 t = 0; t < nchunk; ++t)
    for (int s = 0; s < 4; ++s) {
      u32 v = tot[t * 4 + s];
      tot[t * 4 + s] = (u32)run[s];
      run[s] += v;
    }
  static const u8 acgt[4] = {'A', 'C', 'G', 'T'};
  for (int s = 0; s < 4; ++s) {
    u32 cc = c.char2comp[acgt[s]];
    u64 expect = cc ? c.C[cc + 1] - c.C[cc] : 0;  // comp 0 is the sentinel: the byte is absent
    if (run[s] != expect)
      return fail(DG_EFORMAT, "index self-check: decoded BWT holds %llu '%c' but C[] says %llu", (unsigned long long)run[s],
                  acgt[s], (unsigned long long)expect);
    f.C4[s] = cc ? (u32)c.C[cc] : 0u;
  }
  DG_HIP(hipMemcpyAsync(chunk, tot.data(), nchunk * 16, hipMemcpyHostToDevice, ix->stream));
  hipLaunchKernelGGL(k_block_counts, dim3(ceil_div(nchunk, TB)), dim3(TB), 0, ix->stream, half_cnt, nhalf, chunk, nchunk, occ,
                     nblk);
  f.occ = occ;
  DG_HIP(hipStreamSynchronize(ix->stream));
  return DG_OK;
}

// Text and suffix array: in one walk with the inverse suffix array, which is then sorted (large indexes), or in two independent walks
static int stage_text_sa(dg_index* ix) {
  FmView& f = ix->view;
  const u64 n = f.n;
  u8* text = nullptr;
  u32* sa = nullptr;
  DG_TRY(ix->own((void**)&text, plan::text_bytes(n)));
  DG_TRY(ix->own((void**)&sa, plan::sa_bytes(n)));
  bool sorted_sa = false;
  if (n > (1u << 16)) {
    int rc = DG_ENOMEM;  // (no room for isa, like no room for the sort: the two walks)
    {  // text and inverse suffix array in one walk, suffix array by sorting (isa[p], p); isa is gone before the table is sized
      StreamScratch tmp(ix->stream);
      u32* isa = nullptr;
      if (tmp.big((void**)&isa, plan::sa_bytes(n)) == DG_OK) {
        hipLaunchKernelGGL(k_derive_text_isa, dim3(ceil_div(f.n_isa_samp, TB)), dim3(TB), 0, ix->stream, f, text, isa);
        rc = derive_sa_by_sort(ix->stream, isa, n, sa);
      } else (void)hipGetLastError();
    }
    if (rc == DG_OK) {
      DevWord bad(ix->stream);
      u32 hbad = 0;
      DG_TRY(bad.init(0));
      hipLaunchKernelGGL(k_check_sa_samples, dim3(ceil_div(f.n_sa_samp, TB)), dim3(TB), 0, ix->stream, f, (const u32*)sa, bad.p);
      DG_TRY(bad.read(&hbad));
      if (hbad) return fail(DG_EFORMAT, "index self-check: %u suffix-array samples of the file disagree with its inverse samples", hbad);
      sorted_sa = true;
    } else if (rc != DG_ENODEV && rc != DG_ENOMEM) return rc;
  }
  if (!sorted_sa) {  // the two independent walks (small indexes, low memory, debugging builds)
    hipLaunchKernelGGL(k_derive_text, dim3(ceil_div(f.n_isa_samp, TB)), dim3(TB), 0, ix->stream, f, text);
    hipLaunchKernelGGL(k_derive_sa, dim3(ceil_div(f.n_sa_samp, TB)), dim3(TB), 0, ix->stream, f, sa);
  }
  f.text = text;
  f.sa = sa;
  DG_HIP(hipStreamSynchronize(ix->stream));
  DG_HIP(hipGetLastError());
  return DG_OK;
}

// the shortest run of 'N' (one streaming pass over the text)
static int stage_nrun(dg_index* ix) {
  FmView& f = ix->view;
  DevWord dmin(ix->stream);
  u32 h_min = 64;
  DG_TRY(dmin.init(h_min));
  hipLaunchKernelGGL(k_nrun_min, dim3((u32)std::min<u64>(ceil_div(f.n, TB), 1u << 16)), dim3(TB), 0, ix->stream, f.text, f.n, dmin.p);
  DG_TRY(dmin.read(&h_min));
  f.nrun_min = exp_env("DICEY_NO_NRUN_PRUNE") ? 0u : h_min;
  return DG_OK;
}

struct TableBuild {
  uint2* tab = nullptr;  // (lo, hi) pairs until stage_table_pack
  u32* f2 = nullptr;     // copy 0 of the long filter: its bits are set by the pass that fills the table
  plan::TableOrders o{0, 0};
};
// The K-mer table in its orders (plan::table_orders) and, with it, copy 0 of the long filter
static int stage_table(dg_index* ix, u32 flags, PhaseClock& pc, TableBuild& t) {
  FmView& f = ix->view;
  plan::TableFacts tf;
  tf.n = f.n;
  tf.flags = flags;
  size_t free_b = 0, total_b = 0;
  tf.have_mem = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
  tf.free_b = free_b;
  if (const char* ek = std::getenv("DICEY_KMER_K")) tf.env_k = std::atoi(ek);  // tuning knobs: force the table order (8..17) ...
  if (const char* ek = std::getenv("DICEY_KMER_K2")) {                         // ... / the long filter's (0 = none)
    tf.env_k2_set = true;
    tf.env_k2 = std::atoi(ek);
  }
  tf.no_filter = exp_env("DICEY_NO_KMER_FILTER");
  t.o = plan::table_orders(tf);
  pc.lap("table order (hipMemGetInfo)");
  DG_TRY(ix->own((void**)&t.tab, plan::table_bytes(t.o.K)));
  pc.lap("table hipMalloc");
  DG_HIP(hipMemsetAsync(t.tab, 0, plan::table_bytes(t.o.K), ix->stream));
  if (t.o.K2) {
    DG_TRY(ix->own((void**)&t.f2, plan::filter_copy_bytes(t.o.K2)));
    DG_HIP(hipMemsetAsync(t.f2, 0, plan::filter_copy_bytes(t.o.K2), ix->stream));
  }
  hipLaunchKernelGGL(k_kmer_table_wave, dim3(ceil_div(f.n, TB)), dim3(TB), 0, ix->stream, f, t.tab, t.o.K, t.o.K2, t.f2);
  DG_HIP(hipStreamSynchronize(ix->stream));
  DG_HIP(hipGetLastError());
  f.ktab = t.tab;
  f.K = t.o.K;
  return DG_OK;
}

// The characters in front of every suffix (2 n bytes): built with the table, i.e. for handles that search batches.  With the same
// gather: the suffix array with context (8 n bytes, FmView::sax) for the locate job kernels — handles that have the block minima (i.e.
// the top-k locate) and the room; DICEY_NO_SAX leaves it out (the tests run both ways: hits of repeat-rich strings then read their
// context from the text as before r06)
static int stage_pre5_sax(dg_index* ix, u32 flags) {
  FmView& f = ix->view;
  const u64 n = f.n;
  u16* pre = nullptr;
  uint2* sax = nullptr;
  if (!ix->try_own((void**)&pre, plan::pre5_bytes(n))) return DG_OK;
  if (!(flags & DG_OPEN_COMPACT) && !exp_env("DICEY_NO_SAX") && !exp_env("DICEY_NO_SA_MINIMA")) {
    size_t free_b = 0, total_b = 0;
    const bool have = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    if (!(plan::sax_fits(n, have, free_b) && ix->try_own((void**)&sax, plan::sax_bytes(n)))) (void)hipGetLastError();
  }
  hipLaunchKernelGGL(k_pre5, dim3(ceil_div(n, TB)), dim3(TB), 0, ix->stream, f.sa, f.text, n, pre, sax);
  DG_HIP(hipStreamSynchronize(ix->stream));
  DG_HIP(hipGetLastError());
  f.pre5 = pre;
  f.sax = sax;
  return DG_OK;
}

// Prefix levels over the records (FmView::plv): X = 2^16, 2^18, ... below n — 64 n / 448 bytes of directory and 8 X bytes of records per
// level (GRCh38: 8 levels, 3.5 + 11.5 GB); DICEY_NO_PLV leaves them out (tests: every repeat-rich string then walks the block minima).
// A level's two blocks are the index's only once the level is complete: the first level that does not fit, or whose scan fails, ends
// the list and leaves nothing behind (its scratch synchronises the stream before it releases them).
static int stage_prefix_levels(dg_index* ix) {
  FmView& f = ix->view;
  const u64 n = f.n, nlines = plan::plv_lines(n);
  StreamScratch tmp(ix->stream);
  u32 *cnt = nullptr, *before = nullptr;
  void* scan = nullptr;
  size_t scan_bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, scan_bytes, (const u32*)nullptr, (u32*)nullptr, 0u, nlines, rocprim::plus<u32>(), ix->stream);
  if (tmp.small((void**)&cnt, nlines * 4) == DG_OK && tmp.small((void**)&before, nlines * 4) == DG_OK &&
      tmp.small(&scan, scan_bytes ? scan_bytes : 16) == DG_OK) {
    for (const u64 x : plan::plv_sizes(n)) {
      size_t free_b = 0, total_b = 0;
      const bool have = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
      if (!plan::plv_level_fits(n, x, have, free_b)) break;
      StreamScratch level(ix->stream);
      u64* dir = nullptr;
      uint2* rec = nullptr;
      if (level.big((void**)&dir, plan::plv_dir_bytes(n)) != DG_OK || level.big((void**)&rec, plan::plv_rec_bytes(x)) != DG_OK) break;
      hipLaunchKernelGGL(k_plv_bits, dim3(ceil_div(nlines, 4)), dim3(256), 0, ix->stream, f.sa, n, x, dir, cnt, nlines);
      if (rocprim::exclusive_scan(scan, scan_bytes, (const u32*)cnt, before, 0u, nlines, rocprim::plus<u32>(), ix->stream) != hipSuccess) break;
      hipLaunchKernelGGL(k_plv_fill, dim3(ceil_div(nlines, 4)), dim3(256), 0, ix->stream, f.sax, (const u32*)before, dir, rec, nlines);
      DG_HIP(hipStreamSynchronize(ix->stream));
      DG_HIP(hipGetLastError());
      level.keep();
      ix->adopt(dir, plan::plv_dir_bytes(n));
      ix->adopt(rec, plan::plv_rec_bytes(x));
      f.plv[f.nplv++] = {dir, rec, x};
    }
  }
  (void)hipGetLastError();
  return DG_OK;
}

// every reader of (lo, hi) pairs is done (the filters were derived from them): the entries take their final form
static int stage_table_pack(dg_index* ix, const TableBuild& t) {
  const u64 entries = 1ULL << (2 * t.o.K);
  hipLaunchKernelGGL(k_ktab_pack, dim3((u32)std::min<u64>(ceil_div(entries, TB), 1u << 20)), dim3(TB), 0, ix->stream, t.tab, entries, ix->view.pre5);
  DG_HIP(hipStreamSynchronize(ix->stream));
  DG_HIP(hipGetLastError());
  return DG_OK;
}

// block minima over the suffix array for the top-k locate (0.57 n bytes; one streaming pass over SA)
static int stage_block_minima(dg_index* ix) {
  FmView& f = ix->view;
  u64 cnt = f.n;
  const u32* prev = f.sa;
  while (cnt > 8 && f.nlev < FmView::MAXLEV) {
    const u64 nout = (cnt + 7) / 8, npad = ((nout + 7) & ~7ULL) + 8;
    u32* lv = nullptr;
    DG_TRY(ix->own((void**)&lv, npad * 4));
    hipLaunchKernelGGL(k_block_min8, dim3(ceil_div(npad, TB)), dim3(TB), 0, ix->stream, prev, cnt, lv, nout, npad);
    f.samin[f.nlev++] = lv;
    prev = lv;
    cnt = nout;
  }
  DG_HIP(hipStreamSynchronize(ix->stream));
  DG_HIP(hipGetLastError());
  return DG_OK;
}

static int stage_selfcheck(dg_index* ix) {
  FmView& f = ix->view;
  DevWord bad(ix->stream);
  u32 hbad = 0;
  DG_TRY(bad.init(0));
  const u64 ns = f.n < (1u << 20) ? f.n : (1u << 20);
  hipLaunchKernelGGL(k_selfcheck, dim3(ceil_div(ns, TB)), dim3(TB), 0, ix->stream, f, ns, bad.p);
  DG_TRY(bad.read(&hbad));
  if (hbad) return fail(DG_EFORMAT, "index self-check failed on %u of %llu sampled suffixes", hbad, (unsigned long long)ns);
  return DG_OK;
}

static int derive_layouts(dg_index* ix, const SdslCsa& c, u32 flags) {
  FmView& f = ix->view;
  PhaseClock pc;
  DG_TRY(stage_occ(ix, c));
  pc.lap("occ blocks");
  DG_TRY(stage_text_sa(ix));
  pc.lap("text + suffix array");
  DG_TRY(stage_nrun(ix));
  pc.lap("shortest N run");
  if (!(flags & DG_OPEN_NO_KMER_TABLE)) {
    TableBuild t;
    DG_TRY(stage_table(ix, flags, pc, t));
    pc.lap("table fill");
    DG_TRY(build_filter(ix, f.kf, t.o.K, t.tab, nullptr));
    pc.lap("presence filter");
    if (t.o.K2) {
      DG_TRY(build_filter(ix, f.kf2, t.o.K2, nullptr, t.f2));
      pc.lap("long presence filter");
    }
    if (!(flags & DG_OPEN_NO_PRE5) && !exp_env("DICEY_NO_PRE5")) {
      DG_TRY(stage_pre5_sax(ix, flags));
      if (f.pre5) pc.lap(f.sax ? "preceding characters + suffix array with context" : "preceding characters");
      if (f.sax && !exp_env("DICEY_NO_PLV")) {
        DG_TRY(stage_prefix_levels(ix));
        pc.lap("prefix levels of the suffix array");
      }
    }
    DG_TRY(stage_table_pack(ix, t));
    pc.lap("table entries packed");
  }
  f.samin[0] = f.sa;
  f.nlev = 1;
  if (!exp_env("DICEY_NO_SA_MINIMA")) {
    DG_TRY(stage_block_minima(ix));
    pc.lap("suffix-array block minima");
  }
  if (!(flags & DG_OPEN_NO_SELFCHECK)) {
    DG_TRY(stage_selfcheck(ix));
    pc.lap("self-check");
  }
  return DG_OK;
}

template <class T>
static int upload(dg_index* ix, const void* src, size_t bytes, const T** dst) {
  void* d = nullptr;
  DG_TRY(ix->own(&d, bytes + 64));  // +64: packed_get may touch one word past the last element
  DG_HIP(hipMemsetAsync((char*)d + bytes, 0, 64, ix->stream));
  DG_HIP(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ix->stream));
  *dst = (const T*)d;
  return DG_OK;
}

static int open_impl(const char* path, int device, u32 flags, dg_index* ix) {
  auto t0 = std::chrono::steady_clock::now();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(DG_ENODEV, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(DG_EINVAL, "device %d out of range (have %d)", device, ndev);
  DG_HIP(hipSetDevice(device));
  ix->device = device;
  DG_HIP(hipStreamCreate(&ix->stream));
  PhaseClock pc;
  SdslCsa c;
  DG_TRY(sdsl_open(path, c));
  pc.lap("file map + parse");
  if (c.n > 0xFFFFFFFFULL) return fail(DG_ELIMIT, "index has %llu symbols; this build keeps 32-bit suffix-array entries", (unsigned long long)c.n);
  ix->file_bytes = c.len;
  FmView& f = ix->view;
  std::memset(&f, 0, sizeof f);
  f.n = c.n;
  DG_TRY(upload(ix, c.bv.w, c.bv.nwords * 8, &f.bv));
  DG_TRY(upload(ix, c.rank.w, c.rank.nwords * 8, &f.rk));
  DG_TRY(upload(ix, c.sa_samples.w, c.sa_samples.nwords * 8, &f.sa_samp));
  DG_TRY(upload(ix, c.isa_samples.w, c.isa_samples.nwords * 8, &f.isa_samp));
  f.samp_width = c.sa_samples.width;
  f.n_sa_samp = c.sa_samples.bits / c.sa_samples.width;
  f.n_isa_samp = c.isa_samples.bits / c.isa_samples.width;
  auto t = std::make_unique<WtTables>();
  std::memset(t.get(), 0, sizeof *t);
  for (size_t v = 0; v < c.nodes.size(); ++v) {
    t->node_pos[v] = c.nodes[v].bv_pos;
    t->node_rank[v] = c.nodes[v].bv_pos_rank;
    t->child[v][0] = c.nodes[v].child[0];
    t->child[v][1] = c.nodes[v].child[1];
  }
  std::memcpy(t->path, c.path, sizeof t->path);
  std::memcpy(t->c_to_leaf, c.c_to_leaf, sizeof t->c_to_leaf);
  for (size_t i = 0; i < c.C.size(); ++i) t->C[i] = c.C[i];
  std::memcpy(t->char2comp, c.char2comp, 256);
  for (size_t i = 0; i < c.comp2char.size(); ++i) t->comp2char[i] = c.comp2char[i];
  t->sigma = c.sigma;
  for (int b = 0; b < 256; ++b) ix->code_len[b] = (c.c_to_leaf[b] == 0xFFFF) ? 0u : (u32)(c.path[b] >> 56);
  ix->sigma = c.sigma;
  DG_TRY(upload(ix, t.get(), sizeof *t, &f.wt));
  DG_HIP(hipStreamSynchronize(ix->stream));  // the copy has read *t
  t.reset();
  pc.lap("upload of the sdsl sections");
  static const u8 soc[8] = {'A', 'C', 'G', 'T', 'N', '\n', 0, 0};
  std::memcpy(f.sym_of_code, soc, 8);
  auto t1 = std::chrono::steady_clock::now();
  DG_TRY(derive_layouts(ix, c, flags));
  auto t2 = std::chrono::steady_clock::now();
  ix->derive_seconds = std::chrono::duration<double>(t2 - t1).count();
  ix->load_seconds = std::chrono::duration<double>(t2 - t0).count();
  return DG_OK;
}

}  // namespace dg

using namespace dg;

dg_index::~dg_index() {
  stop_worker();
  if (lanes[0]) {  // the owner of the internal lanes (they only point at its hints record)
    for (dg_index*& l : lanes) {
      delete l;
      l = nullptr;
    }
    SharedHints* sh = shared_hints.exchange(nullptr);
    if (sh)
      for (hipEvent_t e : sh->ev_base)
        if (e) (void)hipEventDestroy(e);
    delete sh;
  }
  for (void* p : owned) dg::big_free(p, stream);
  if (stream) (void)hipStreamSynchronize(stream);
  for (auto& w : ws) w.release();
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);

  if (pinned) (void)hipHostFree(pinned);
  if (stream) (void)hipStreamDestroy(stream);
}

extern "C" {

const char* dg_last_error(void) { return dg::last_error().c_str(); }
int dg_abi_version(void) { return DG_ABI_VERSION; }

// Host only (no device is touched): the file's sections accounted for byte by byte, their invariants against each other, and —
// DG_FM9_CHECK_DEEP — the big sections read through (rank words against the bit vector, the tree's node sizes and rank offsets,
// C[] against the leaf sizes, sample values).  The report is one JSON object; on DG_EFORMAT its "error" (= dg_last_error()) names
// the first section that is off.
int dg_fm9_check(const char* fm9_path, uint32_t flags, char* report, size_t report_cap) {
  if (report && report_cap) report[0] = 0;
  if (!fm9_path) return fail(DG_EINVAL, "dg_fm9_check: null path");
  SdslCsa c;
  int rc = sdsl_open(fm9_path, c);
  if (rc == DG_OK && (flags & DG_FM9_CHECK_DEEP)) {
    rc = sdsl_check_deep(c);
    if (rc != DG_OK) fail(rc, "%s: %s", fm9_path, c.why.c_str());
  }
  if (report && report_cap) {
    std::string j = "{\"ok\":";
    j += rc == DG_OK ? "true" : "false";
    j += ",\"deep\":";
    j += (flags & DG_FM9_CHECK_DEEP) ? "true" : "false";
    j += ",\"file_bytes\":" + std::to_string(c.len);
    if (c.base && rc != DG_EIO) {
      j += std::string(",\"layout\":\"") + (c.checked_layout ? "store_to_checked_file" : "store_to_file") + "\"";
      j += ",\"n\":" + std::to_string(c.n) + ",\"sigma\":" + std::to_string(c.wt_sigma);
      j += ",\"sa_sample_width\":" + std::to_string((unsigned)c.sa_samples.width);
      j += ",\"sections\":[";
      for (size_t i = 0; i < c.sections.size(); ++i) {
        if (i) j += ",";
        j += std::string("{\"name\":\"") + c.sections[i].name + "\",\"offset\":" + std::to_string(c.sections[i].offset) + ",\"bytes\":" + std::to_string(c.sections[i].bytes) + "}";
      }
      j += "]";
    }
    if (rc != DG_OK) {
      std::string e = last_error();
      for (char& ch : e)
        if (ch == '"' || ch == '\\' || (unsigned char)ch < 32) ch = ' ';
      j += ",\"error\":\"" + e + "\"";
    }
    j += "}";
    std::snprintf(report, report_cap, "%s", j.c_str());
  }
  return rc;
}
int dg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int dg_index_open(const char* fm9_path, int device, uint32_t flags, dg_index** out) {
  if (!fm9_path || !out) return fail(DG_EINVAL, "dg_index_open: null argument");
  *out = nullptr;
  dg_index* ix = new dg_index;
  int rc = open_impl(fm9_path, device, flags, ix);
  if (rc != DG_OK) {
    delete ix;
    return rc;
  }
  *out = ix;
  return DG_OK;
}

int dg_index_share(dg_index* src, dg_index** out) {
  if (!src || !out) return fail(DG_EINVAL, "dg_index_share: null argument");
  *out = nullptr;
  DG_HIP(hipSetDevice(src->device));
  dg_index* ix = new dg_index;
  ix->device = src->device;
  ix->view = src->view;  // the index arrays stay owned by `src`
  ix->sigma = src->sigma;
  std::memcpy(ix->code_len, src->code_len, sizeof ix->code_len);
  ix->file_bytes = src->file_bytes;
  ix->hbm_bytes = 0;
  ix->hints = src->hints.inherited();
  // DICEY_EXP_PRIO (measurement aid, r06): the shares of an index — its internal lanes — get stream priorities in turn (highest,
  // lowest, highest, ...) while the index's own stream stays at the default, so that the lanes' search kernels do not share the chip
  // evenly (which keeps the lanes in step: DESIGN "lanes")
  static std::atomic<unsigned> n_shares{0};
  hipError_t se = hipSuccess;
  if (exp_env("DICEY_EXP_PRIO")) {
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    se = hipStreamCreateWithPriority(&ix->stream, hipStreamDefault, (n_shares.fetch_add(1) & 1u) ? least : greatest);
  } else se = hipStreamCreate(&ix->stream);
  if (se != hipSuccess) {
    delete ix;
    return fail(DG_EHIP, "dg_index_share: cannot create a stream");
  }
  *out = ix;
  return DG_OK;
}

void* dg_index_stream(dg_index* ix) { return ix ? (void*)ix->stream : nullptr; }

void dg_index_close(dg_index* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  delete ix;
}

int dg_index_stats(const dg_index* ix, dg_index_stats_t* out) {
  if (!ix || !out) return fail(DG_EINVAL, "dg_index_stats: null argument");
  std::memset(out, 0, sizeof *out);
  out->n = ix->view.n;
  out->sigma = ix->sigma;
  std::memcpy(out->code_len, ix->code_len, sizeof out->code_len);
  out->file_bytes = ix->file_bytes;
  out->hbm_bytes = ix->hbm_bytes;
  out->load_seconds = ix->load_seconds;
  out->derive_seconds = ix->derive_seconds;
  return DG_OK;
}

#ifdef DG_EXPERIMENTS
// Development builds only (experiments.hpp; not in include/dicey_gpu.h, not exported by the product): the derived layouts as they lie
// in HBM, for tests/test_gpu_index_layout.py, which holds every entry against tests/index_layout_ref.py.
enum dgx_layout : uint32_t {
  DGX_L_OCC = 0,   // OccBlock[plan::occ_blocks(n)]
  DGX_L_TEXT,      // u8[n]
  DGX_L_SA,        // u32[n]
  DGX_L_KTAB,      // uint2[4^K], packed (FmView::ktab)
  DGX_L_KF,        // copy `level` of kf: u32[4^k / 32]
  DGX_L_KF2,       // copy `level` of kf2
  DGX_L_PRE5,      // u16[n]
  DGX_L_SAX,       // uint2[n]
  DGX_L_PLV_DIR,   // prefix level `level`: u64[8 * plan::plv_lines(n)]
  DGX_L_PLV_REC,   // prefix level `level`: uint2[x]
  DGX_L_SAMIN      // block minima, level `level` >= 1: u32[((nout + 7) & ~7) + 8] — the 0xFFFFFFFF padding belongs to the layout
};
struct dgx_filter_info {
  uint32_t k, nr, s[4];
  uint64_t pick;
};
struct dgx_layout_info {
  uint64_t bytes;  // of the layout asked for, without the allocation's slack; 0 = this handle does not have it
  uint64_t n;
  uint64_t x;      // DGX_L_PLV_*: the level's X, else 0
  uint32_t C4[4];
  uint32_t K, nrun_min, nlev, nplv;
  uint32_t pre5_null, sax_null;
  dgx_filter_info kf, kf2;
};
int dgx_index_layout(dg_index* ix, uint32_t what, uint32_t level, void* host_out, uint64_t cap_bytes, dgx_layout_info* info) {
  if (!ix || !info) return fail(DG_EINVAL, "dgx_index_layout: null argument");
  const FmView& f = ix->view;
  std::memset(info, 0, sizeof *info);
  info->n = f.n;
  std::memcpy(info->C4, f.C4, sizeof info->C4);
  info->K = f.K;
  info->nrun_min = f.nrun_min;
  info->nlev = f.nlev;
  info->nplv = f.nplv;
  info->pre5_null = f.pre5 == nullptr;
  info->sax_null = f.sax == nullptr;
  const KFilter* kfs[2] = {&f.kf, &f.kf2};
  dgx_filter_info* out[2] = {&info->kf, &info->kf2};
  for (int i = 0; i < 2; ++i) {
    out[i]->k = kfs[i]->k;
    out[i]->nr = kfs[i]->nr;
    std::memcpy(out[i]->s, kfs[i]->s, sizeof out[i]->s);
    out[i]->pick = kfs[i]->pick;
  }
  const void* src = nullptr;
  u64 bytes = 0;
  switch (what) {
    case DGX_L_OCC: src = f.occ, bytes = plan::occ_blocks(f.n) * sizeof(OccBlock); break;
    case DGX_L_TEXT: src = f.text, bytes = f.n; break;
    case DGX_L_SA: src = f.sa, bytes = f.n * 4; break;
    case DGX_L_KTAB: src = f.K ? f.ktab : nullptr, bytes = f.K ? plan::table_bytes(f.K) : 0; break;
    case DGX_L_KF:
    case DGX_L_KF2: {
      const KFilter& kf = what == DGX_L_KF ? f.kf : f.kf2;
      if (level < kf.nr) src = kf.cp[level], bytes = plan::filter_bits_bytes(kf.k);
      break;
    }
    case DGX_L_PRE5: src = f.pre5, bytes = f.n * 2; break;
    case DGX_L_SAX: src = f.sax, bytes = f.n * 8; break;
    case DGX_L_PLV_DIR:
    case DGX_L_PLV_REC:
      if (level < f.nplv) {
        info->x = f.plv[level].x;
        if (what == DGX_L_PLV_DIR) src = f.plv[level].dir, bytes = plan::plv_lines(f.n) * 64;
        else src = f.plv[level].rec, bytes = f.plv[level].x * 8;
      }
      break;
    case DGX_L_SAMIN:
      if (level >= 1 && level < f.nlev) {
        u64 cnt = f.n, npad = 0;
        for (u32 l = 1; l <= level; ++l) {  // stage_block_minima's sizes
          cnt = (cnt + 7) / 8;
          npad = ((cnt + 7) & ~7ULL) + 8;
        }
        src = f.samin[level], bytes = npad * 4;
      }
      break;
    default: return fail(DG_EINVAL, "dgx_index_layout: unknown layout %u", what);
  }
  if (!src) bytes = 0;
  info->bytes = bytes;
  DG_HIP(hipSetDevice(ix->device));
  DG_HIP(hipStreamSynchronize(ix->stream));
  if (host_out && bytes) DG_HIP(hipMemcpy(host_out, src, (size_t)std::min<u64>(bytes, cap_bytes), hipMemcpyDeviceToHost));
  return DG_OK;
}
#endif

}  // extern "C"
