// What an index open decides before it allocates, and the byte size of every resident layout: plain integers and pure functions, no HIP.
// index.hip gathers the facts (hipMemGetInfo, the open flags, the environment), calls a rule and builds what it decided; a host harness
// (tests/host) holds the same rules against a model of them without a GPU.  Every comparison with the free bytes is strict.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/dicey_gpu.h"

namespace dg {
namespace plan {

using u32 = uint32_t;
using u64 = uint64_t;

// bytes of the layouts (+64: the kernels read whole words past the last element)
inline u64 occ_blocks(u64 n) { return (n >> 7) + 1; }                          // 64-byte blocks of 128 BWT symbols
inline u64 text_bytes(u64 n) { return n + 64; }
inline u64 sa_bytes(u64 n) { return n * 4 + 64; }                              // the suffix array, and the inverse one it is sorted from
inline u64 table_bytes(u32 K) { return 8ULL << (2 * K); }                      // (lo, hi) per K-mer
inline u64 filter_bits_bytes(u32 k) { return (1ULL << (2 * k)) >> 3; }         // one bit per k-mer ...
inline u64 filter_copy_bytes(u32 k) { return filter_bits_bytes(k) + 64; }      // ... in each of up to four permuted copies
inline u64 pre5_bytes(u64 n) { return n * 2 + 64; }
inline u64 sax_bytes(u64 n) { return n * 8 + 64; }
static constexpr u32 MAXPLV = 8, PLV_LINE = 448;                               // = FmView::MAXPLV, FmView::PLV_LINE
inline u64 plv_lines(u64 n) { return n / PLV_LINE + 1; }
inline u64 plv_dir_bytes(u64 n) { return plv_lines(n) * 64; }
inline u64 plv_rec_bytes(u64 x) { return x * 8 + 64; }
static constexpr u64 ROOM = 4ULL << 30;                                        // what an optional layout leaves free

struct TableFacts {
  u64 n = 0;
  bool have_mem = false;    // hipMemGetInfo succeeded ...
  u64 free_b = 0;           // ... and reported this many free bytes
  u32 flags = 0;            // DG_OPEN_*
  int env_k = 0;            // DICEY_KMER_K: forces the table order; 0 = not set (a value outside 8..17 is ignored)
  bool env_k2_set = false;  // DICEY_KMER_K2: forces the long filter's order ...
  int env_k2 = 0;           // ... (K, 20], anything else = none
  bool no_filter = false;   // DICEY_NO_KMER_FILTER
};
struct TableOrders {
  u32 K, K2;  // K2 = 0: no long filter
};
// K = ceil(log4 n) clamped to [8,16]: about one expected occurrence per K-mer; 16 -> 34 GB, which is what the 288 GB of HBM are for.
// What the rest of the HBM is spent on (DESIGN.md "long filter"): one character more for the table when the device has room (K = 17,
// 137 GB, on a 3.1 Gb genome: one interval extension fewer per surviving string), and a presence filter of order K2 = ceil(log4 n) + 2
// in four permuted copies (4 x 8.6 GB at K2 = 18) in front of everything — a random 18-mer of a 3.1 Gb genome occurs with p = 0.04, a
// 16-mer with 0.51, a 17-mer with 0.17.  r02 measured K / K2 = 16/19, 16/18 and 17/18 on the bench workloads; 17/18 is
// the fastest at both distances.
inline TableOrders table_orders(const TableFacts& t) {
  u32 K = 8, K2 = 0;
  while (K < 16 && (1ULL << (2 * K)) < t.n) ++K;
  const u64 slack = std::min<u64>(48ULL << 30, t.n * 16 + (64u << 20));
  const u64 f2_b = 4 * filter_bits_bytes(K + 2);
  u64 need = table_bytes(K) + slack;
  if (t.have_mem && t.free_b > need + f2_b) {
    K2 = K + 2;
    need += f2_b;
  }
  if ((t.flags & DG_OPEN_BIG_TABLE) && t.have_mem && (1ULL << (2 * K)) < t.n * 2 && t.free_b > need - table_bytes(K) + table_bytes(K + 1)) ++K;
  if (t.env_k >= 8 && t.env_k <= 17) {
    K = (u32)t.env_k;
    if (K2 && K2 <= K) K2 = K + 1;
  }
  if (t.env_k2_set) K2 = (t.env_k2 > (int)K && t.env_k2 <= 20) ? (u32)t.env_k2 : 0u;
  if (t.no_filter || 2 * K2 < 17) K2 = 0;
  return {K, K2};
}

// the suffix array with context (8 n bytes) beside the preceding characters (2 n, already allocated when this is asked)
inline bool sax_fits(u64 n, bool have_mem, u64 free_b) { return have_mem && free_b > n * 8 + n * 2 + ROOM; }

// prefix levels: X = 2^16, 2^18, ... below n, at most MAXPLV of them; one more is built while its directory and records leave ROOM
inline std::vector<u64> plv_sizes(u64 n) {
  std::vector<u64> xs;
  for (u64 x = 1ULL << 16; x < n && xs.size() < MAXPLV; x <<= 2) xs.push_back(x);
  return xs;
}
inline bool plv_level_fits(u64 n, u64 x, bool have_mem, u64 free_b) { return have_mem && !(free_b < plv_lines(n) * 64 + x * 8 + ROOM); }

}  // namespace plan
}  // namespace dg
