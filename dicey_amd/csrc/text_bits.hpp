// What every mappability kernel reads of a text laid out like the index text (mappability.hip, map_mm.hpp, min_unique.hpp, query_*.hpp):
// 8 text bytes from any position, the 2-bit code of a base, and the A/C/G/T and valid-k-mer bitmaps.
#pragma once
#include "devfm.hpp"

namespace dg {

__host__ __device__ inline bool bit_at(const u64* b, u64 i) { return (b[i >> 6] >> (i & 63)) & 1ULL; }

// 8 text bytes from any position (little endian: byte p in bits 0-7); the text buffer has 64 bytes of slack behind n
DG_DEV u64 text8(const u8* t, u64 p) {
  const u64* w = reinterpret_cast<const u64*>(t + (p & ~7ULL));
  const u32 s = (u32)(p & 7) * 8;
  const u64 lo = w[0];
  return s ? (lo >> s) | (w[1] << (64 - s)) : lo;
}
// 2-bit code of an A/C/G/T byte: A 0x41 -> 0, C 0x43 -> 1, G 0x47 -> 2, T 0x54 -> 3
DG_DEV u32 acgt_code(u32 b) { return ((b >> 1) ^ (b >> 2)) & 3u; }

// bit j of word w = T[64w + j] is A/C/G/T (positions >= n, the sentinel and the padding words are 0)
__global__ void k_acgt_bits(const u8* text, u64 n, u64* acgt, u64 nw) {
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
        const bool ok = b == 'A' || b == 'C' || b == 'G' || b == 'T';
        m |= (u64)ok << (c * 16 + j);
      }
    }
    if (n - p0 < 64) m &= (1ULL << (n - p0)) - 1;
  }
  acgt[w] = m;
}

// bit p = the k characters from p are all A/C/G/T (so p + k <= n - 1: the sentinel is not).  Words w + 1 .. w + ceil(k/64) + 1 are
// read; the caller pads the bitmap with that many zero words.
__global__ void k_valid_bits(const u64* acgt, u64 nw_data, u32 k, u64* valid) {
  const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nw_data) return;
  // first non-A/C/G/T position at or after 64 (w + 1), or far enough that no bit of this word cares
  u64 nz = (w + 1) * 64 + k + 64;
  const u32 look = (k + 63) / 64 + 1;
  for (u32 j = 1; j <= look; ++j) {
    const u64 z = ~acgt[w + j];
    if (z) {
      nz = (w + j) * 64 + (u64)__ffsll((long long)z) - 1;
      break;
    }
  }
  const u64 z0 = ~acgt[w];
  u64 v = 0;
  for (int b = 63; b >= 0; --b) {
    const u64 p = w * 64 + (u64)b;
    if ((z0 >> b) & 1ULL) nz = p;
    v |= (u64)(nz - p >= k) << b;
  }
  valid[w] = v;
}

DG_DEV bool kmer_equal(const u8* t, u64 a, u64 b, u32 k) {
  for (u32 j = 0; j < k; j += 8) {
    u64 x = text8(t, a + j) ^ text8(t, b + j);
    if (k - j < 8) x &= (1ULL << (8 * (k - j))) - 1;
    if (x) return false;
  }
  return true;
}

}  // namespace dg
