// Per-base tracks over a dg_map that is already resident (mappability.hip: dg_map_cover, dg_map_min_cover).  Every other member of the
// family gives a value per k-mer START; these two give a value per BASE, the form Umap and ENCODE publish.
//
// Cover count.  src is a count map made at length k, t = at_most >= 1:
//   spec(q)    = 1 iff 1 <= src(q) <= t                                  (t = 1: the k-mer that starts at q is unique)
//   cover_t(p) = #{q : max(0, p-k+1) <= q <= p, spec(q) = 1}             (the specific k-mers that lie over base p, 0..k)
// written as min(cover, max_count) when max_count > 0 (1: the single-read track; cover / k is the multi-read one).  src is 0 at every
// start whose k-mer crosses a sequence end, an N or the text's end, so no boundary rule is needed.  The work per base does not grow with k:
//   k_spec_bits  one pass over src; a wavefront ballots spec into one 64-bit word per 64 positions (the bit order of k_acgt_bits)
//   scan         rocprim exclusive scan of the words' popcounts: dir[w] = set bits in front of word w (u32: n < 2^32)
//   k_cover      one lane per base: cover(p) = rank(p+1) - rank(max(0, p-k+1)), rank(x) = dir[x >> 6] + popc(word[x >> 6] & low bits)
//
// Minimum covering length.  src is a length map made with max_k (mul or mul_e of include/dicey_gpu.h, any strand setting):
//   mcl(p) = min{max(src(q), p-q+1) : p-max_k+1 <= q <= p, q >= 0, src(q) != 0, run(q) >= p-q+1}, 0 when the set is empty
// the length of the shortest unique valid window of at most max_k bases that contains base p: a window that starts at q with length
// m >= src(q) inside q's run is unique, because value never rises with the length.
//   k_min_cover  a workgroup owns a tile of consecutive bases.  It stages the tile's cells and the max_k - 1 in front of them in LDS, one
//                u16 per position (bit 15: the base is A/C/G/T, low bits: src), all loads going out together; positions in front of the
//                text are cells of 0.  A lane then walks d = 1, 2, ... back from its base, in LDS only, and stops at the first cell that is
//                not A/C/G/T, at max_k, or once d >= best: the loop is bounded by the answer.
//
// What ties the two together: for every k in 10..max_k and every p that lies in at least one VALID k-window,
//   cover_1 at k is >= 1 at p   <=>   mcl(p) != 0 && mcl(p) <= k.
// =>: a unique valid k-window at q over p has 0 != src(q) <= k, run(q) >= k >= p-q+1 and p-q+1 <= k, so max(src(q), p-q+1) <= k.
// <=: mcl(p) = m <= k names a unique valid window U of m bases over p.  p lies in a valid k-window V, so the A/C/G/T run around p holds
// at least k bases, and U, which lies in the same run, can be grown inside it to a valid k-window W over p.  W is unique: every place
// within e mismatches of W, on either strand, holds at the matching offset a place within e mismatches of U, and U has one.
// The restriction is needed: a base in an A/C/G/T run shorter than k can have mcl(p) <= k while no k-window covers it.
//
// The arithmetic is in functions over plain arrays, shared with a host program (tests/host/map_cover_main.cpp) that runs them against
// the numpy model without a GPU, as band_bits.hpp, cap_enum.hpp and probe_schedule.hpp do.
#pragma once
#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DG_MC __host__ __device__ __forceinline__
#else
#define DG_MC inline
#endif

namespace dg {

static constexpr uint32_t COVER_CELL_ACGT = 0x8000u;  // the position is A/C/G/T
static constexpr uint32_t COVER_CELL_LEN = 0x7FFFu;   // its length of the source map (at most 1000)
static constexpr uint32_t COVER_TILE_MAX = 2048;      // positions per workgroup tile
static constexpr uint32_t COVER_MAX_K = 1000;

// set bits among positions [0, x): words[w] bit j is position 64 w + j, dir[w] the set bits in front of word w
DG_MC uint32_t cover_rank(const uint32_t* dir, const uint64_t* words, uint64_t x) {
  const uint64_t w = x >> 6;
  return dir[w] + (uint32_t)__builtin_popcountll(words[w] & ((1ULL << (x & 63)) - 1));
}

// set bits among the starts max(0, p-k+1) .. p
DG_MC uint32_t cover_count(const uint32_t* dir, const uint64_t* words, uint64_t p, uint32_t k) {
  const uint64_t lo = p + 1 >= k ? p + 1 - k : 0;
  return cover_rank(dir, words, p + 1) - cover_rank(dir, words, lo);
}

DG_MC uint16_t cover_cell(uint32_t len, bool acgt) { return (uint16_t)((len & COVER_CELL_LEN) | (acgt ? COVER_CELL_ACGT : 0u)); }

// mcl of the position whose cell is cells[i]; the cell of position p - d + 1 is cells[i - d + 1], and nothing in front of cells[0] is read
DG_MC uint32_t cover_walk(const uint16_t* cells, uint32_t i, uint32_t max_k) {
  const uint32_t lim = max_k < i + 1 ? max_k : i + 1;
  uint32_t best = 0xFFFFFFFFu;
  for (uint32_t d = 1; d <= lim && d < best; ++d) {
    const uint32_t c = cells[i + 1 - d];
    if (!(c & COVER_CELL_ACGT)) break;
    const uint32_t L = c & COVER_CELL_LEN;
    if (L) {
      const uint32_t m = L > d ? L : d;
      if (m < best) best = m;
    }
  }
  return best == 0xFFFFFFFFu ? 0u : best;
}

}  // namespace dg

#ifdef __HIPCC__
#include "devfm.hpp"

namespace dg {

// Counters of a pass.  A counter that every wavefront adds to is one address for tens of millions of atomics, and the pass then runs at the
// rate of that address, not of HBM: so a workgroup adds ONCE (its wavefronts' sums meet in LDS), and the workgroups spread over
// COVER_SLOTS counters a cache line apart, which the host adds up.
static constexpr u32 COVER_SLOTS = 16, COVER_SLOT_STRIDE = 16;  // 16 x u64 = 128 bytes between two slots
struct CoverCounters {
  unsigned long long specific[COVER_SLOTS * COVER_SLOT_STRIDE], covered[COVER_SLOTS * COVER_SLOT_STRIDE];
};
static constexpr u32 COVER_PER_BLOCK = 4096;  // positions per k_cover workgroup: 16 per lane

// every thread of a 256-thread workgroup calls this, once per counter and with its own 4 words of LDS
DG_DEV void block_add(unsigned long long* slots, u32 v, u32* part) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const u32 t = part[0] + part[1] + part[2] + part[3];
    if (t) atomicAdd(&slots[(blockIdx.x % COVER_SLOTS) * COVER_SLOT_STRIDE], (unsigned long long)t);
  }
}

struct PopcWord {  // the scan's input: set bits of a word
  __device__ __host__ u32 operator()(u64 w) const { return (u32)__builtin_popcountll(w); }
};

// 256 threads: 4 wavefronts of 4 words each, the 4 loads of a lane issued together.  n1 = n - 1: the sentinel is no position.  The number
// of set bits needs no counter: the scan leaves it in the directory entry of the last word, a padding word
__global__ void __launch_bounds__(256) k_spec_bits(const u32* src, u64 n1, u32 at_most, u64* words, u64 nw) {
  const u32 lane = threadIdx.x & 63;
  const u64 w0 = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  u32 v[4];
#pragma unroll
  for (u32 j = 0; j < 4; ++j) {
    const u64 p = (w0 + j) * 64 + lane;
    v[j] = p < n1 ? src[p] : 0u;
  }
#pragma unroll
  for (u32 j = 0; j < 4; ++j) {
    const u64 m = __ballot(v[j] - 1u < at_most);  // 1 <= v <= at_most (0 wraps above every at_most: at most 0xFFFFFFFD)
    if (lane == 0 && w0 + j < nw) words[w0 + j] = m;
  }
}

// COVER_PER_BLOCK positions per workgroup, lane after lane (stores of a wavefront are one 256-byte stretch); out[n-1], the sentinel's
// entry, is 0
__global__ void __launch_bounds__(256) k_cover(const u64* words, const u32* dir, u64 n, u32 k, u32 max_count, u32* out, CoverCounters* ctr) {
  __shared__ u32 part[4];
  const u64 p0 = (u64)blockIdx.x * COVER_PER_BLOCK + threadIdx.x;
  u32 cov = 0;
#pragma unroll 4
  for (u32 j = 0; j < COVER_PER_BLOCK / 256; ++j) {
    const u64 p = p0 + (u64)j * 256;
    if (p >= n) break;
    u32 c = p + 1 < n ? cover_count(dir, words, p, k) : 0u;
    if (max_count && c > max_count) c = max_count;
    out[p] = c;
    cov += c != 0;
  }
  block_add(ctr->covered, cov, part);
}

// tile <= COVER_TILE_MAX positions per workgroup, max_k <= COVER_MAX_K: (tile + max_k - 1) cells of LDS, 6 KB at most
__global__ void __launch_bounds__(256) k_min_cover(const u32* src, const u8* text, u64 n, u32 max_k, u32 tile, u32* out, CoverCounters* ctr) {
  __shared__ u16 cells[COVER_TILE_MAX + COVER_MAX_K];
  __shared__ u32 part[8];
  const u64 t0 = (u64)blockIdx.x * tile, n1 = n - 1;
  const u32 halo = max_k - 1, ncell = halo + tile;
  u32 spec = 0, cov = 0;
#pragma unroll 4
  for (u32 j = threadIdx.x; j < ncell; j += 256) {
    const u64 g = t0 + j;  // the position + halo
    const bool in = g >= halo && g - halo < n1;
    const u64 q = in ? g - halo : 0;  // every load is unconditional, so that they go out together
    const u32 v = src[q], b = text[q];
    const bool acgt = b == 'A' || b == 'C' || b == 'G' || b == 'T';
    cells[j] = in ? cover_cell(v, acgt) : (u16)0;
    spec += in && j >= halo && v != 0;
  }
  __syncthreads();
  for (u32 j = threadIdx.x; j < tile; j += 256) {
    const u64 p = t0 + j;
    if (p >= n) break;
    const u32 r = p < n1 ? cover_walk(cells, halo + j, max_k) : 0u;
    out[p] = r;
    cov += r != 0;
  }
  block_add(ctr->specific, spec, part);  // (every thread of the workgroup is here)
  block_add(ctr->covered, cov, part + 4);
}

}  // namespace dg
#endif
