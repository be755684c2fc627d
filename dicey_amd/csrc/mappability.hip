// `dicey mappability`: exact-match k-mer uniqueness of every text position, computed on the resident index.
//
// value(p) = count(w) + count(revcomp(w)) for w = T[p, p+k) when w lies inside the text and holds only A/C/G/T, else 0
// (count = sdsl::count, overlapping occurrences included; a reverse-complement palindrome counts twice per occurrence, the
// both-strand total `padlock` uses).  Phases, all on the index's stream, handing data over only at kernel boundaries:
//   1. valid bitmap   k_acgt_bits (1 bit per position: A/C/G/T) -> k_valid_bits (the run of A/C/G/T from p is >= k long)
//   2. forward counts suffixes with equal k-prefixes are adjacent in the suffix array: k_fwd_boundaries marks, per rank, where
//                     a group of equal k-mers starts (one comparison of two neighbouring suffixes); a max-scan gives every rank
//                     its group's first rank, a min-scan over the reversed ranks its group's last one (rocprim, as build.hip)
//   3. reverse strand k_heads: one backward search of revcomp(w) per group head (K-mer table first, left at the first empty
//                     interval); the head's slot of the start array then holds the group's total
//   4. scatter        k_scatter: every rank reads its head's total (a broadcast in rank order) and writes it at SA[i]
// With e = 1 or 2 mismatches (dg_mappability_mm, (k,e)-mappability) phases 1, 2 and 4 are the same and phase 3 is k_heads_mm (map_mm.hpp):
// per group head a backward search with a mismatch budget of w and of revcomp(w), launched per chunk of head ranks.
// Transient HBM: the start array (4n) and three bitmaps (3n/8) beside the result (4n), which the end scan uses first.
// dg_min_unique (min_unique.hpp) answers the inverse question on the same handle type: per position the smallest k at which the value
// is 1, from one pass over neighbouring suffixes and one backward search per rank.  dg_min_unique_mm (min_unique_mm.hpp) asks the same
// with up to two mismatches: the two exact passes, then one lane per position that probes lengths from the exact answer upward.
// dg_query_map (query_map.hpp) runs phase 1 on a buffer of query records laid out like the text and then one search per valid position
// of it: the (k,e) counts of k-mers that are not in the index.  dg_query_min_len (query_min_len.hpp) looks, on the same buffer, for the
// smallest k at which that count is at most t.  dg_query_map_anchored (query_anchor.hpp) is dg_query_map with the last a bases of every
// k-mer matched exactly.  dg_query_min_len_end (query_min_len_end.hpp) looks for the smallest k by the oligo's LAST base, anchored.
// dg_query_map_iupac (query_iupac.hpp) is dg_query_map_anchored for records with IUPAC codes, each letter a set of bases.
// dg_map_cover and dg_map_min_cover (map_cover.hpp) turn a resident map of values per k-mer START into one of values per BASE: the
// specific k-mers that lie over each base, and the shortest unique window that contains it.  Streaming passes over the map, no search.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "dev_mem.hpp"  // StreamScratch: the transient device buffers of one call
#include "devfm.hpp"
#include "experiments.hpp"
#include "index_internal.hpp"
#include "map_cover.hpp"        // per-base tracks of a resident map (dg_map_cover, dg_map_min_cover)
#include "map_mm.hpp"           // k_heads' sibling for e >= 1 mismatches
#include "min_unique.hpp"         // the kernels of dg_min_unique
#include "min_unique_mm.hpp"      // and the search with a mismatch budget on top of them (dg_min_unique_mm)
#include "query_anchor.hpp"       // k_qmap with the k-mer's last bases matched exactly (dg_query_map_anchored)
#include "query_iupac.hpp"        // k_qmap_anch for k-mers with IUPAC codes, one search per expansion (dg_query_map_iupac)
#include "query_map.hpp"          // the same search per position of a query buffer (dg_query_map)
#include "query_min_len.hpp"      // and the search for the smallest specific k per position (dg_query_min_len)
#include "query_min_len_end.hpp"  // the smallest specific k of the anchored k-mer that ENDS at a position (dg_query_min_len_end)
#include "text_bits.hpp"          // text8, acgt_code, the A/C/G/T and valid bitmaps

struct dg_map {
  int device = 0;
  hipStream_t stream = nullptr;  // own stream: the map may be read after its index handle has moved on to other work
  uint64_t n = 0;                // index n; values cover positions [0, n-1)
  uint32_t* out = nullptr;       // u32[n] (the entry at n-1, the sentinel, is 0)
  dg_map_stats_t st{};
  dg_map_mm_stats_t mm{};  // all zero for an exact map
  dg_mu_mm_stats_t mu{};   // all zero unless dg_min_unique_mm searched with mismatches
  dg_cover_stats_t cv{};   // all zero unless dg_map_cover or dg_map_min_cover made the map
  uint32_t kind = DG_MAP_KIND_COUNT;  // what the values are: dg_map_cover and dg_map_min_cover ask
  uint32_t max_count = 0;             // the clamp the values were written with (0: none)
  dg::DevBuf run_flags, run_pos, run_val, run_cnt;  // dg_map_runs workspaces (grow-only)
  ~dg_map() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (out) dg::big_free(out, stream);
    run_flags.release();
    run_pos.release();
    run_val.release();
    run_cnt.release();
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }
};

namespace dg {

// per rank i: bd bit i = a group of equal k-mers starts at rank i (every rank whose suffix has no valid k-mer is a group of its own),
// hd bit i = that, and the k-mer at SA[i] is valid.  Launched with 256 threads per block: a wavefront's 64 ranks are one word.
__global__ void __launch_bounds__(256) k_fwd_boundaries(FmView f, const u64* valid, u32 k, u64* bd, u64* hd) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < f.n;
  bool boundary = true, head = false;
  if (in) {
    const u64 p = f.sa[i];
    const bool vi = bit_at(valid, p);
    if (vi && i > 0) {
      const u64 q = f.sa[i - 1];
      if (bit_at(valid, q)) boundary = !kmer_equal(f.text, q, p, k);
    }
    head = vi && boundary;
  }
  const u64 mb = __ballot(boundary), mh = __ballot(head);
  if ((threadIdx.x & 63) == 0 && i < f.n) {
    bd[i >> 6] = mb;
    hd[i >> 6] = mh;
  }
}

struct StartKey {  // rank i -> i where a group starts, else 0 (max-scan: the group's first rank)
  const u64* bd;
  __device__ __host__ u32 operator()(u32 i) const { return bit_at(bd, i) ? i : 0u; }
};
struct EndKey {  // j -> rank i = n-1-j if i is the last rank of its group, else ~0 (min-scan over j: the group's last rank)
  const u64* bd;
  u64 n;
  __device__ __host__ u32 operator()(u32 j) const {
    const u64 i = n - 1 - j;
    return (i + 1 == n || bit_at(bd, i + 1)) ? (u32)i : 0xFFFFFFFFu;
  }
};
struct MaxU32 {
  __device__ __host__ u32 operator()(u32 a, u32 b) const { return a > b ? a : b; }
};
struct MinU32 {
  __device__ __host__ u32 operator()(u32 a, u32 b) const { return a < b ? a : b; }
};

// group heads: the forward count is the group's size; the reverse count one backward search of revcomp(w).  Reading revcomp(w) from
// its last character to its first is reading w from its first character to its last, complemented.  The head's slot of `start`
// (which holds the head's own rank) receives the saturated total.
__global__ void __launch_bounds__(256) k_heads(FmView f, u32 k, int forward_only, const u64* hd, u32* start, const u32* end_rev,
                                              unsigned long long* steps) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  u32 n_ext = 0;
  if (i < f.n && bit_at(hd, i)) {
    const u64 fw = (u64)end_rev[f.n - 1 - i] - i + 1;
    u64 rv = 0;
    if (!forward_only) {
      const u64 p = f.sa[i];
      u32 lo = 0, hi = (u32)f.n, t = 0;
      u64 chunk = 0;
      if (f.K && k >= f.K) {
        u64 code = 0;
        for (; t < f.K; ++t) {
          if ((t & 7) == 0) chunk = text8(f.text, p + t);
          code |= (u64)(3u - acgt_code((u32)(chunk >> (8 * (t & 7))) & 255u)) << (2 * t);
        }
        const KtabEntry e = ktab_entry(f, code);
        lo = e.lo;
        hi = e.hi;
      }
      if (t < k && lo < hi) chunk = text8(f.text, p + (t & ~7u));
      for (; t < k && lo < hi; ++t, ++n_ext) {
        if ((t & 7) == 0) chunk = text8(f.text, p + t);
        bs_extend_code_narrow(f, lo, hi, 3u - acgt_code((u32)(chunk >> (8 * (t & 7))) & 255u));
      }
      rv = lo < hi ? hi - lo : 0;
    }
    const u64 tot = fw + rv;
    start[i] = tot > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)tot;
  }
  wave_add(steps, n_ext);  // (every lane of the wavefront is here)
}

// out[SA[i]] = the total of i's group (heads hold it in their own slot; members hold their head's rank), 0 for invalid ranks
__global__ void k_scatter(FmView f, const u64* hd, const u32* start, u32 max_count, u32* out) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= f.n) return;
  const u32 s = start[i];
  u32 v = 0;
  if (bit_at(hd, i)) v = s;
  else if (s != (u32)i) v = start[s];
  if (max_count && v > max_count) v = max_count;
  out[f.sa[i]] = v;
}

// run boundaries of [a, b) inside the requested range [lo, hi): a run is a maximal stretch of equal non-zero values
__global__ void k_run_flags(const u32* out, u64 lo, u64 hi, u64 a, u64 len, u8* fs, u8* fe) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= len) return;
  const u64 p = a + t;
  const u32 v = out[p];
  fs[t] = v && (p == lo || out[p - 1] != v);
  fe[t] = v && (p + 1 == hi || out[p + 1] != v);
}
__global__ void k_run_values(const u32* out, u64 a, const u32* starts, const unsigned long long* cnt, u32* val) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cnt[0]) return;
  val[t] = out[a + starts[t]];
}

// default ranks per k_heads_mm launch and default W (rows verified on the text): DESIGN.md §10 has the measurements behind both
static constexpr u64 MM_HEAD_CHUNK = 1ULL << 24;
static constexpr u32 MM_NARROW = 8;

// f(std::integral_constant<int, e>{}): the search kernels are templates on the mismatch count (e <= 2: every entry point checks)
template <class F>
static void with_mismatches(u32 e, F&& f) {
  if (e == 0) f(std::integral_constant<int, 0>{});
  else if (e == 1) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 2>{});
}

// the events of a call with N phases, one of them a chunked search: N + 1 events around the phases and, with DICEY_TIMING, one in front of
// every launch of the search, for the longest one.  Every event is owned from the moment it exists: a failed creation releases the others
template <int N>
struct ChunkTimer {
  hipEvent_t ev[N + 1] = {};
  std::vector<hipEvent_t> lev;
  const bool timing = std::getenv("DICEY_TIMING") != nullptr;
  ~ChunkTimer() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : lev) (void)hipEventDestroy(e);
  }
  int init() {
    for (auto& e : ev) DG_HIP(hipEventCreate(&e));
    return DG_OK;
  }
  int launch(hipStream_t st) {  // in front of every launch of the search
    if (!timing) return DG_OK;
    hipEvent_t e;
    DG_HIP(hipEventCreate(&e));
    lev.push_back(e);
    DG_HIP(hipEventRecord(e, st));
    return DG_OK;
  }
  // once the stream has been synchronised.  search: the phase the launches lie in (the last one ends where that phase does)
  int read(float ms[N], int search, float* longest) {
    for (int j = 0; j < N; ++j) DG_HIP(hipEventElapsedTime(&ms[j], ev[j], ev[j + 1]));
    *longest = 0;
    for (size_t j = 0; j < lev.size(); ++j) {
      float t = 0;
      DG_HIP(hipEventElapsedTime(&t, lev[j], j + 1 < lev.size() ? lev[j + 1] : ev[search + 1]));
      *longest = std::max(*longest, t);
    }
    return DG_OK;
  }
};

static int map_impl(dg_index* ix, const dg_map_params* prm, u32 mismatches, dg_map* m) {
  const FmView& f = ix->view;
  const u64 n = f.n;
  const u32 k = prm->k;
  hipStream_t st = ix->stream;
  const u64 nw_data = (n + 63) / 64, nw = nw_data + (k + 63) / 64 + 4;
  const size_t bm_bytes = nw * 8;
  // scan scratch sizes first: everything is allocated before the first kernel runs
  rocprim::counting_iterator<u32> cnt0(0);
  auto sk = rocprim::make_transform_iterator(cnt0, StartKey{nullptr});
  auto ek = rocprim::make_transform_iterator(cnt0, EndKey{nullptr, n});
  size_t scan1 = 0, scan2 = 0;
  DG_HIP(rocprim::inclusive_scan(nullptr, scan1, sk, (u32*)nullptr, (size_t)n, MaxU32(), st));
  DG_HIP(rocprim::inclusive_scan(nullptr, scan2, ek, (u32*)nullptr, (size_t)n, MinU32(), st));
  const size_t scan_bytes = std::max(scan1, scan2) + 256;
  const u64 need = n * 4 + 256 + n * 4 + 256 + 3 * bm_bytes + scan_bytes + 64;
  size_t free_b = 0, total_b = 0;
  DG_HIP(hipMemGetInfo(&free_b, &total_b));
  if ((u64)free_b < need + (64ULL << 20))
    return fail(DG_ENOMEM, "dg_mappability: needs %llu MB of device memory, %llu MB free", (unsigned long long)(need >> 20),
                (unsigned long long)(free_b >> 20));
  StreamScratch b(st);
  void *b_start = nullptr, *b_bm = nullptr, *b_scan = nullptr, *b_steps = nullptr;
  DG_HIP(big_alloc((void**)&m->out, n * 4 + 256, st));
  DG_TRY(b.big(&b_start, n * 4 + 256));
  DG_TRY(b.big(&b_bm, 3 * bm_bytes));
  DG_TRY(b.small(&b_scan, scan_bytes));
  DG_TRY(b.small(&b_steps, sizeof(MmCounters)));
  u64* acgt = (u64*)b_bm;  // becomes the boundary bitmap once the valid bitmap is made
  u64* valid = acgt + nw;
  u64* hd = valid + nw;
  u64* bd = acgt;
  u32* start = (u32*)b_start;
  u32* end_rev = m->out;
  ChunkTimer<4> tm;  // valid | forward | reverse (the chunked search when e >= 1) | scatter
  DG_TRY(tm.init());
  const u32 TB = 256;
  DG_HIP(hipMemsetAsync(b_steps, 0, sizeof(MmCounters), st));
  DG_HIP(hipEventRecord(tm.ev[0], st));
  hipLaunchKernelGGL(k_acgt_bits, dim3(ceil_div(nw, TB)), dim3(TB), 0, st, f.text, n, acgt, nw);
  DG_HIP(hipMemsetAsync(valid + nw_data, 0, (nw - nw_data) * 8, st));
  hipLaunchKernelGGL(k_valid_bits, dim3(ceil_div(nw_data, TB)), dim3(TB), 0, st, (const u64*)acgt, nw_data, k, valid);
  DG_HIP(hipEventRecord(tm.ev[1], st));
  hipLaunchKernelGGL(k_fwd_boundaries, dim3(ceil_div(n, TB)), dim3(TB), 0, st, f, (const u64*)valid, k, bd, hd);
  DG_HIP(rocprim::inclusive_scan(b_scan, scan1, rocprim::make_transform_iterator(cnt0, StartKey{bd}), start, (size_t)n, MaxU32(), st));
  DG_HIP(rocprim::inclusive_scan(b_scan, scan2, rocprim::make_transform_iterator(cnt0, EndKey{bd, n}), end_rev, (size_t)n, MinU32(), st));
  DG_HIP(hipEventRecord(tm.ev[2], st));
  u64 launches = 0;
  if (mismatches == 0) {
    hipLaunchKernelGGL(k_heads, dim3(ceil_div(n, TB)), dim3(TB), 0, st, f, k, prm->forward_only, (const u64*)hd, start, (const u32*)end_rev,
                       (unsigned long long*)b_steps);
  } else {
    // head ranks in chunks, one launch each: no single launch holds the device for long
    u64 chunk = MM_HEAD_CHUNK;
    u32 W = MM_NARROW;
    if (const char* e = exp_env("DICEY_MAP_HEAD_CHUNK")) chunk = std::max<u64>(1, std::strtoull(e, nullptr, 10));
    if (const char* e = exp_env("DICEY_MAP_NARROW")) W = (u32)std::min<u64>(std::strtoull(e, nullptr, 10), 0xFFFFFFFFull);
    MmCounters* ctr = (MmCounters*)b_steps;
    for (u64 r0 = 0; r0 < n; r0 += chunk, ++launches) {
      const u64 r1 = std::min(n, r0 + chunk);
      DG_TRY(tm.launch(st));
      with_mismatches(mismatches, [&](auto E) {
        if constexpr (E.value > 0)  // (e = 0 is k_heads above)
          hipLaunchKernelGGL(k_heads_mm<E.value>, dim3(ceil_div(r1 - r0, TB)), dim3(TB), 0, st, f, k, prm->forward_only, W, prm->max_count, r0, r1,
                             (const u64*)hd, start, ctr);
      });
    }
  }
  DG_HIP(hipEventRecord(tm.ev[3], st));
  hipLaunchKernelGGL(k_scatter, dim3(ceil_div(n, TB)), dim3(TB), 0, st, f, (const u64*)hd, (const u32*)start, prm->max_count, m->out);
  DG_HIP(hipEventRecord(tm.ev[4], st));
  MmCounters hc{};
  if (mismatches == 0) DG_HIP(hipMemcpyAsync(&m->st.rev_steps, b_steps, 8, hipMemcpyDeviceToHost, st));
  else DG_HIP(hipMemcpyAsync(&hc, b_steps, sizeof hc, hipMemcpyDeviceToHost, st));
  DG_HIP(hipStreamSynchronize(st));
  DG_HIP(hipGetLastError());
  float ms[4] = {0, 0, 0, 0}, longest = 0;
  DG_TRY(tm.read(ms, 2, &longest));
  m->st.ms_valid = ms[0];
  m->st.ms_forward = ms[1];
  m->st.ms_reverse = ms[2];
  m->st.ms_scatter = ms[3];
  m->st.ms_total = (double)ms[0] + (double)ms[1] + (double)ms[2] + (double)ms[3];  // in double: exactly the sum of the reported parts
  m->st.transient_bytes = n * 4 + 256 + 3 * bm_bytes + scan_bytes;
  if (mismatches) {
    m->st.rev_steps = hc.steps;
    m->mm.heads = hc.heads;
    m->mm.steps = hc.steps;
    m->mm.table_reads = hc.table_reads;
    m->mm.verified_rows = hc.verified_rows;
    m->mm.early_exits = hc.early_exits;
    m->mm.launches = launches;
    m->mm.ms_search = ms[2];
    if (tm.timing && launches)
      std::fprintf(stderr, "dicey timing: mappability e=%u: %llu launches of the head search, %.1f ms in all, longest %.1f ms\n", mismatches,
                   (unsigned long long)launches, ms[2], longest);
  }
  return DG_OK;
}

// default ranks per launch of the two passes (the same reasoning as MM_HEAD_CHUNK: no launch holds a shared device for long)
static constexpr u64 MU_CHUNK = 1ULL << 24;
// default positions per k_mu_mm launch at e = 2, where a lane runs 5 to 7 searches of 1 + 3K + 9K(K-1)/2 table reads each: a launch of 2^24
// takes 9 to 19 s on the 64 Mb genomes.  e = 1 keeps 2^24 (0.3 to 0.7 s): shorter launches cost more than they give, each one waits for
// its slowest workgroup (DESIGN.md §10 has the measurements)
static constexpr u64 MU_MM_CHUNK2 = 1ULL << 22;

// who: the entry point's name for messages.  mismatches = 0: the two exact passes (dg_min_unique).  e = 1, 2: k_mu_mm behind them, positions in
// chunks of launches; it reads mul_0 from the result array and overwrites it, and kernel boundaries separate the passes
static int min_unique_impl(const char* who, dg_index* ix, u32 max_k, int forward_only, u32 mismatches, dg_map* m) {
  const FmView& f = ix->view;
  const u64 n = f.n;
  // the INDEX handle's stream, as map_impl: the passes read the index and are ordered with the handle's other work; the map's own stream
  // serves dg_map_values / dg_map_runs afterwards (the final synchronize below is the hand-over)
  hipStream_t st = ix->stream;
  const u64 lcp_bytes = (n + 1) * 2 + 256;
  const u64 need = n * 4 + 256 + lcp_bytes + 64;
  size_t free_b = 0, total_b = 0;
  DG_HIP(hipMemGetInfo(&free_b, &total_b));
  if ((u64)free_b < need + (64ULL << 20))
    return fail(DG_ENOMEM, "%s: needs %llu MB of device memory, %llu MB free", who, (unsigned long long)(need >> 20),
                (unsigned long long)(free_b >> 20));
  StreamScratch b(st);
  void *b_lcp = nullptr, *b_steps = nullptr, *b_mm = nullptr;
  DG_HIP(big_alloc((void**)&m->out, n * 4 + 256, st));
  DG_TRY(b.big(&b_lcp, lcp_bytes));
  DG_TRY(b.small(&b_steps, 8));
  if (mismatches) DG_TRY(b.small(&b_mm, sizeof(MuMmCounters)));
  u64 chunk = MU_CHUNK, mm_chunk = mismatches >= 2 ? MU_MM_CHUNK2 : MU_CHUNK;
  u32 W = MM_NARROW;
  if (const char* e = exp_env("DICEY_MAP_HEAD_CHUNK")) chunk = mm_chunk = std::max<u64>(1, std::strtoull(e, nullptr, 10));
  if (const char* e = exp_env("DICEY_MAP_NARROW")) W = (u32)std::min<u64>(std::strtoull(e, nullptr, 10), 0xFFFFFFFFull);
  ChunkTimer<2> tm;  // forward (k_mu_lcp) | reverse (the chunked walk)
  DG_TRY(tm.init());
  const int rank_order = exp_env("DICEY_MU_MM_RANK_ORDER") != nullptr;  // lanes by rank instead of by text position (a measurement aid)
  ChunkTimer<1> ts;  // the chunked search with mismatches behind them
  if (mismatches) DG_TRY(ts.init());
  const u32 TB = 256;
  DG_HIP(hipMemsetAsync(b_steps, 0, 8, st));
  if (mismatches) DG_HIP(hipMemsetAsync(b_mm, 0, sizeof(MuMmCounters), st));
  DG_HIP(hipEventRecord(tm.ev[0], st));
  for (u64 r0 = 0; r0 < n + 1; r0 += chunk) {  // ranks 0..n: lcp[n] closes the array
    const u64 r1 = std::min(n + 1, r0 + chunk);
    hipLaunchKernelGGL(k_mu_lcp, dim3(ceil_div(r1 - r0, TB)), dim3(TB), 0, st, f, max_k, r0, r1, (u16*)b_lcp);
  }
  DG_HIP(hipEventRecord(tm.ev[1], st));
  u64 launches = 0;
  for (u64 r0 = 0; r0 < n; r0 += chunk, ++launches) {
    const u64 r1 = std::min(n, r0 + chunk);
    DG_TRY(tm.launch(st));
    hipLaunchKernelGGL(k_mu_walk, dim3(ceil_div(r1 - r0, TB)), dim3(TB), 0, st, f, max_k, forward_only, r0, r1, (const u16*)b_lcp, m->out,
                       (unsigned long long*)b_steps);
  }
  DG_HIP(hipEventRecord(tm.ev[2], st));
  u64 mm_launches = 0;
  MuMmCounters hc{};
  if (mismatches) {
    DG_HIP(hipEventRecord(ts.ev[0], st));
    for (u64 r0 = 0; r0 < n; r0 += mm_chunk, ++mm_launches) {
      const u64 r1 = std::min(n, r0 + mm_chunk);
      DG_TRY(ts.launch(st));
      with_mismatches(mismatches, [&](auto E) {
        if constexpr (E.value > 0)  // (e = 0 ends with the walk above)
          hipLaunchKernelGGL(k_mu_mm<E.value>, dim3(ceil_div(r1 - r0, TB)), dim3(TB), 0, st, f, max_k, forward_only, W, rank_order, r0, r1,
                             m->out, (MuMmCounters*)b_mm);
      });
    }
    DG_HIP(hipEventRecord(ts.ev[1], st));
    DG_HIP(hipMemcpyAsync(&hc, b_mm, sizeof hc, hipMemcpyDeviceToHost, st));
  }
  DG_HIP(hipMemcpyAsync(&m->st.rev_steps, b_steps, 8, hipMemcpyDeviceToHost, st));
  DG_HIP(hipStreamSynchronize(st));
  DG_HIP(hipGetLastError());
  float ms[2] = {0, 0}, longest = 0;
  DG_TRY(tm.read(ms, 1, &longest));
  m->st.ms_valid = 0;
  m->st.ms_forward = ms[0];
  m->st.ms_reverse = ms[1];
  m->st.ms_scatter = 0;  // the walk writes the value itself
  m->st.ms_total = (double)ms[0] + (double)ms[1];  // in double: exactly the sum of the reported parts
  m->st.transient_bytes = lcp_bytes;
  if (tm.timing && launches)
    std::fprintf(stderr, "dicey timing: min unique max_k=%u: %llu launches of the walk, %.1f ms in all, longest %.1f ms\n", max_k,
                 (unsigned long long)launches, ms[1], longest);
  if (mismatches) {
    float mss[1] = {0}, mm_longest = 0;
    DG_TRY(ts.read(mss, 0, &mm_longest));
    m->mu.candidates = hc.candidates;
    m->mu.probes = hc.probes;
    m->mu.steps = hc.steps;
    m->mu.table_reads = hc.table_reads;
    m->mu.verified_rows = hc.verified_rows;
    m->mu.launches = mm_launches;
    m->mu.ms_search = mss[0];
    m->st.ms_total = (double)ms[0] + (double)ms[1] + (double)mss[0];  // in double: exactly ms_forward + ms_reverse + ms_search
    if (ts.timing && mm_launches)
      std::fprintf(stderr, "dicey timing: min unique max_k=%u e=%u: %llu launches of the search, %.1f ms in all, longest %.1f ms\n", max_k, mismatches,
                   (unsigned long long)mm_launches, mss[0], mm_longest);
  }
  return DG_OK;
}

// default positions per k_qmap launch (the same reasoning as MM_HEAD_CHUNK; DESIGN.md §10 has the measurement)
static constexpr u64 QMAP_CHUNK = 1ULL << 20;
// default positions per k_qminlen launch: a lane does several probes one after the other (DESIGN.md §10 has the measurement)
static constexpr u64 QMINLEN_CHUNK = 1ULL << 18;

// the records as REC1 '\n' REC2 '\n' ...: record i at off[i] - off[0] + i, a '\n' behind each
static std::vector<u8> query_pack(const uint8_t* seqs, const uint64_t* off, size_t nseq) {
  const u64 base = off[0];
  std::vector<u8> hq(off[nseq] - base + nseq);
  for (size_t i = 0; i < nseq; ++i) {
    const u64 len = off[i + 1] - off[i];
    if (len) std::memcpy(&hq[off[i] - base + i], seqs + off[i], len);
    hq[off[i + 1] - base + i] = '\n';
  }
  return hq;
}
// and the values of the buffer's positions back in the caller's layout (the '\n' positions dropped)
static void query_unpack(const std::vector<u32>& vals, const uint64_t* off, size_t nseq, uint32_t* values) {
  const u64 base = off[0];
  for (size_t i = 0; i < nseq; ++i) {
    const u64 len = off[i + 1] - off[i];
    if (len) std::memcpy(values + off[i], &vals[off[i] - base + i], len * 4);
  }
}

// the checks dg_query_map and dg_query_min_len share behind their parameter block: the size limit, then the handle and the pointers.
// need_device: a process without a HIP device is told so (DG_ENODEV) before the handle it cannot have is looked at
static int query_args_check(const char* who, dg_index* ix, const uint8_t* seqs, const uint64_t* off, size_t nseq, const uint32_t* values,
                            bool need_device) {
  const u64 total = (off && nseq) ? off[nseq] : 0;
  if (total >= (1ULL << 31) || (u64)nseq >= (1ULL << 31) || total + nseq >= (1ULL << 31))
    return fail(DG_ELIMIT, "%s: %llu query bytes in %llu records: 2^31 or more with their separators", who, (unsigned long long)total,
                (unsigned long long)nseq);
  if (need_device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(DG_ENODEV, "%s: no HIP device available", who);
  }
  if (!ix || (nseq && !off) || (total && (!seqs || !values))) return fail(DG_EINVAL, "%s: null argument", who);
  for (size_t i = 0; i < nseq; ++i)
    if (off[i] > off[i + 1]) return fail(DG_EINVAL, "%s: offsets decrease at record %llu", who, (unsigned long long)i);
  if (ix->view.n < 2 || ix->view.n > 0xFFFFFFFFull) return fail(DG_ELIMIT, "%s: index of %llu suffixes", who, (unsigned long long)ix->view.n);
  if (ix->any_lane_busy()) return fail(DG_EINVAL, "%s: a dg_hunt_submit batch is in flight on this handle (dg_hunt_wait first)", who);
  return DG_OK;
}

// The device side of a query buffer: the bytes in whole 64-byte blocks with the text's slack behind, one u32 per position, `nbm` bitmaps
// of nw words each (the A/C/G/T bitmap first, the valid bitmap second) and a counter record.  alloc() checks the free memory and allocates
// everything; upload() queues the copy and k_acgt_bits or, for records with IUPAC codes, k_iupac_bits.
struct QueryDev {
  StreamScratch mem;
  u64 qn = 0, nw_data = 0, nw = 0, q_bytes = 0;
  void *q = nullptr, *out = nullptr, *bm = nullptr, *ctr = nullptr;
  explicit QueryDev(hipStream_t s) : mem(s) {}
  // k: the longest k-mer looked at, which sizes the zero words behind the bitmap's data
  int alloc(const char* who, u64 qn_, u32 k, u32 nbm, size_t ctr_bytes) {
    qn = qn_;
    nw_data = (qn + 63) / 64;
    nw = nw_data + (k + 63) / 64 + 4;
    const size_t bm_bytes = nw * 8;
    q_bytes = nw_data * 64 + 64;  // whole 64-byte blocks for k_acgt_bits, then the text's slack
    const u64 need = q_bytes + qn * 4 + 256 + nbm * bm_bytes + 64;
    size_t free_b = 0, total_b = 0;
    DG_HIP(hipMemGetInfo(&free_b, &total_b));
    if ((u64)free_b < need + (64ULL << 20))
      return fail(DG_ENOMEM, "%s: needs %llu MB of device memory, %llu MB free", who, (unsigned long long)(need >> 20),
                  (unsigned long long)(free_b >> 20));
    DG_TRY(mem.big(&q, q_bytes));
    DG_TRY(mem.big(&out, qn * 4 + 256));
    DG_TRY(mem.big(&bm, nbm * bm_bytes));
    DG_TRY(mem.small(&ctr, ctr_bytes));
    return DG_OK;
  }
  u64* acgt() const { return (u64*)bm; }
  u64* valid() const { return acgt() + nw; }
  int upload(const std::vector<u8>& hq, bool iupac) {
    hipStream_t st = mem.st;
    DG_HIP(hipMemsetAsync((u8*)q + (qn & ~63ULL), 0, q_bytes - (qn & ~63ULL), st));  // the tail of the last block and the slack
    DG_HIP(hipMemcpyAsync(q, hq.data(), qn, hipMemcpyHostToDevice, st));
    if (iupac) hipLaunchKernelGGL(k_iupac_bits, dim3(ceil_div(nw, 256)), dim3(256), 0, st, (const u8*)q, qn, acgt(), nw);
    else hipLaunchKernelGGL(k_acgt_bits, dim3(ceil_div(nw, 256)), dim3(256), 0, st, (const u8*)q, qn, acgt(), nw);
    return DG_OK;
  }
};

// what tells the two query searches apart on the host, beside their kernels and counters
struct QueryKind {
  u32 nbm;            // bitmaps: 2 when k_valid_bits runs (one k for all positions), 1 when a lane finds its own limit
  u64 chunk;          // default positions per launch
  const char* chunk_env;
  bool iupac;         // the first bitmap is of the 15 IUPAC letters, not of A/C/G/T alone
};
static constexpr QueryKind QUERY_MAP = {2, QMAP_CHUNK, "DICEY_QMAP_CHUNK", false}, QUERY_MIN_LEN = {1, QMINLEN_CHUNK, "DICEY_QMINLEN_CHUNK", false},
                           QUERY_MAP_IUPAC = {2, QMAP_CHUNK, "DICEY_QMAP_CHUNK", true};

// The driver of every dg_query_* call.  hq: the records as REC1 '\n' REC2 '\n' ... (qn bytes); vals: u32[qn], one value per buffer
// position; k: the longest k-mer looked at; label: what the DICEY_TIMING line calls the search.  launch(b, W, p0, p1, grid, block) queues the
// kernel for positions [p0, p1).  Fills *hc with the device counters and the fields every stats struct has; the caller adds its own.
template <class Counters, class Stats, class Launch>
static int query_run(const char* who, dg_index* ix, const QueryKind& kind, u32 k, const char* label, const std::vector<u8>& hq, std::vector<u32>& vals,
                     Counters* hc, Stats* stt, Launch launch) {
  const u64 qn = hq.size();
  hipStream_t st = ix->stream;
  QueryDev b(st);
  DG_TRY(b.alloc(who, qn, k, kind.nbm, sizeof(Counters)));
  u64 chunk = kind.chunk;
  u32 W = MM_NARROW;
  if (const char* e = exp_env(kind.chunk_env)) chunk = std::max<u64>(1, std::strtoull(e, nullptr, 10));
  if (const char* e = exp_env("DICEY_MAP_NARROW")) W = (u32)std::min<u64>(std::strtoull(e, nullptr, 10), 0xFFFFFFFFull);
  ChunkTimer<2> tm;  // upload and bitmaps | the chunked search
  DG_TRY(tm.init());
  const u32 TB = 256;
  DG_HIP(hipMemsetAsync(b.ctr, 0, sizeof(Counters), st));
  DG_HIP(hipEventRecord(tm.ev[0], st));
  DG_TRY(b.upload(hq, kind.iupac));
  if (kind.nbm > 1) {
    DG_HIP(hipMemsetAsync(b.valid() + b.nw_data, 0, (b.nw - b.nw_data) * 8, st));
    hipLaunchKernelGGL(k_valid_bits, dim3(ceil_div(b.nw_data, TB)), dim3(TB), 0, st, (const u64*)b.acgt(), b.nw_data, k, b.valid());
  }
  DG_HIP(hipEventRecord(tm.ev[1], st));
  u64 launches = 0;
  for (u64 p0 = 0; p0 < qn; p0 += chunk, ++launches) {  // positions in chunks, one launch each: no single launch holds the device for long
    const u64 p1 = std::min(qn, p0 + chunk);
    DG_TRY(tm.launch(st));
    launch(b, W, p0, p1, dim3(ceil_div(p1 - p0, TB)), dim3(TB));
  }
  DG_HIP(hipEventRecord(tm.ev[2], st));
  DG_HIP(hipMemcpyAsync(hc, b.ctr, sizeof *hc, hipMemcpyDeviceToHost, st));
  DG_HIP(hipMemcpyAsync(vals.data(), b.out, qn * 4, hipMemcpyDeviceToHost, st));
  DG_HIP(hipStreamSynchronize(st));
  DG_HIP(hipGetLastError());
  float ms[2] = {0, 0}, longest = 0;
  DG_TRY(tm.read(ms, 1, &longest));
  stt->valid = hc->valid;
  stt->steps = hc->steps;
  stt->table_reads = hc->table_reads;
  stt->verified_rows = hc->verified_rows;
  stt->launches = launches;
  stt->ms_valid = ms[0];
  stt->ms_search = ms[1];
  stt->ms_total = (double)ms[0] + (double)ms[1];  // in double: exactly the sum of the reported parts
  if (tm.timing && launches)
    std::fprintf(stderr, "dicey timing: %s: %llu launches of the search, %.1f ms in all, longest %.1f ms\n", label, (unsigned long long)launches,
                 ms[1], longest);
  return DG_OK;
}

// "query map e=1" or, with an anchor, "query map e=1 anchor=5"
static std::string query_label(const char* what, u32 mismatches, const u32* anchor) {
  char s[96];
  if (anchor) std::snprintf(s, sizeof s, "%s e=%u anchor=%u", what, mismatches, *anchor);
  else std::snprintf(s, sizeof s, "%s e=%u", what, mismatches);
  return s;
}

// k_qmap per chunk of positions.  anchor: null for dg_query_map, else the number of last bases matched exactly (k_qmap_anch): the same
// buffers, chunks and W either way
static int query_map_impl(const char* who, dg_index* ix, const dg_qmap_params* prm, const u32* anchor, const std::vector<u8>& hq, std::vector<u32>& vals,
                          dg_qmap_stats_t* stt) {
  const FmView& f = ix->view;
  QmapCounters hc{};
  DG_TRY(query_run(who, ix, QUERY_MAP, prm->k, query_label("query map", prm->mismatches, anchor).c_str(), hq, vals, &hc, stt,
                   [&](const QueryDev& b, u32 W, u64 p0, u64 p1, dim3 grid, dim3 block) {
                     with_mismatches(prm->mismatches, [&](auto E) {
                       if (anchor)
                         hipLaunchKernelGGL(k_qmap_anch<E.value>, grid, block, 0, b.mem.st, f, (const u8*)b.q, (const u64*)b.valid(), prm->k, *anchor,
                                            prm->forward_only, W, prm->max_count, p0, p1, (u32*)b.out, (QmapCounters*)b.ctr);
                       else
                         hipLaunchKernelGGL(k_qmap<E.value>, grid, block, 0, b.mem.st, f, (const u8*)b.q, (const u64*)b.valid(), prm->k, prm->forward_only, W,
                                            prm->max_count, p0, p1, (u32*)b.out, (QmapCounters*)b.ctr);
                     });
                   }));
  stt->early_exits = hc.early_exits;
  return DG_OK;
}

// k_qmap_iupac per chunk of positions: the buffers and chunks of query_map_impl, the valid bitmap over the 15 letters.  max_degeneracy 0: 256
static int query_map_iupac_impl(const char* who, dg_index* ix, const dg_qmap_iupac_params* prm, const std::vector<u8>& hq, std::vector<u32>& vals,
                                dg_qmap_iupac_stats_t* stt) {
  const FmView& f = ix->view;
  const u32 maxdeg = prm->max_degeneracy ? prm->max_degeneracy : 256u;
  QiupacCounters hc{};
  DG_TRY(query_run(who, ix, QUERY_MAP_IUPAC, prm->k, query_label("query map iupac", prm->mismatches, &prm->anchor).c_str(), hq, vals, &hc, stt,
                   [&](const QueryDev& b, u32 W, u64 p0, u64 p1, dim3 grid, dim3 block) {
                     with_mismatches(prm->mismatches, [&](auto E) {
                       hipLaunchKernelGGL(k_qmap_iupac<E.value>, grid, block, 0, b.mem.st, f, (const u8*)b.q, (const u64*)b.valid(), prm->k, prm->anchor,
                                          maxdeg, prm->forward_only, W, prm->max_count, p0, p1, (u32*)b.out, (QiupacCounters*)b.ctr);
                     });
                   }));
  stt->early_exits = hc.early_exits;
  stt->too_degenerate = hc.too_degenerate;
  stt->degenerate = hc.degenerate;
  stt->expansions = hc.expansions;
  return DG_OK;
}

// the same buffer with the A/C/G/T bitmap alone (a lane finds its own limit), k_qminlen per chunk of positions.  anchor: null for
// dg_query_min_len, else the lengths are by END position with that many last bases exact (k_qminlen_end): the same buffers, chunks and W
static int query_min_len_impl(const char* who, dg_index* ix, const dg_qminlen_params* prm, const u32* anchor, const std::vector<u8>& hq,
                              std::vector<u32>& vals, dg_qminlen_stats_t* stt) {
  const FmView& f = ix->view;
  QminlenCounters hc{};
  DG_TRY(query_run(who, ix, QUERY_MIN_LEN, prm->max_k, query_label(anchor ? "query min length by end" : "query min length", prm->mismatches, anchor).c_str(),
                   hq, vals, &hc, stt, [&](const QueryDev& b, u32 W, u64 p0, u64 p1, dim3 grid, dim3 block) {
                     with_mismatches(prm->mismatches, [&](auto E) {
                       if (anchor)
                         hipLaunchKernelGGL(k_qminlen_end<E.value>, grid, block, 0, b.mem.st, f, (const u8*)b.q, (const u64*)b.acgt(), prm->min_k, prm->max_k,
                                            *anchor, prm->forward_only, W, prm->at_most, p0, p1, (u32*)b.out, (QminlenCounters*)b.ctr);
                       else
                         hipLaunchKernelGGL(k_qminlen<E.value>, grid, block, 0, b.mem.st, f, (const u8*)b.q, (const u64*)b.acgt(), b.nw, prm->min_k, prm->max_k,
                                            prm->forward_only, W, prm->at_most, p0, p1, (u32*)b.out, (QminlenCounters*)b.ctr);
                     });
                   }));
  u64 found = 0;
  for (u32 v : vals) found += v != 0 && v != QMAP_INVALID;
  stt->found = found;
  stt->probes = hc.probes;
  return DG_OK;
}

// What the dg_query_* entry points do once their parameter block is checked: totals, device, pack, search, unpack, stats.
// search(hq, vals, &st) is query_map_impl, query_map_iupac_impl or query_min_len_impl with the caller's name and parameters
template <class Stats, class Search>
static int query_call(dg_index* ix, const uint8_t* seqs, const uint64_t* off, size_t nseq, uint32_t* values, Stats* stats, Search search) {
  const u64 total = (off && nseq) ? off[nseq] : 0;
  Stats st{};
  st.positions = nseq ? total - off[0] : 0;
  if (total) {
    DG_HIP(hipSetDevice(ix->device));
    const std::vector<u8> hq = query_pack(seqs, off, nseq);
    std::vector<u32> vals(hq.size());
    DG_TRY(search(hq, vals, &st));
    query_unpack(vals, off, nseq, values);
  }
  if (stats) *stats = st;
  return DG_OK;
}

// default positions per k_min_cover workgroup tile (DICEY_COVER_TILE on the development build: a small genome then spans hundreds of tiles
// and a long halo several of them; results do not depend on it)
static constexpr u32 COVER_TILE = 2048;

// What dg_map_cover (min_cover false) and dg_map_min_cover do once their arguments are checked.  Everything runs on src's stream, which
// orders the transform behind whatever still reads or wrote src; the index contributes only its text, an immutable block.
static int cover_impl(const char* who, dg_index* ix, const dg_map* src, bool min_cover, u32 at_most, u32 max_count, dg_map* m) {
  const u64 n = src->n;
  const u32 k = src->st.k;
  hipStream_t st = src->stream;
  const u64 nw = (n + 63) / 64 + 1;
  size_t scan_bytes = 0;
  if (!min_cover)
    DG_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, rocprim::make_transform_iterator((const u64*)nullptr, PopcWord{}), (u32*)nullptr, 0u, (size_t)nw,
                                   rocprim::plus<u32>(), st));
  const u64 transient = min_cover ? sizeof(CoverCounters) : nw * 8 + nw * 4 + 512 + scan_bytes + sizeof(CoverCounters);
  const u64 need = n * 4 + 256 + transient + 64;
  size_t free_b = 0, total_b = 0;
  DG_HIP(hipMemGetInfo(&free_b, &total_b));
  if ((u64)free_b < need + (64ULL << 20))
    return fail(DG_ENOMEM, "%s: needs %llu MB of device memory, %llu MB free", who, (unsigned long long)(need >> 20), (unsigned long long)(free_b >> 20));
  StreamScratch b(st);
  void *b_words = nullptr, *b_dir = nullptr, *b_scan = nullptr, *b_ctr = nullptr;
  DG_HIP(big_alloc((void**)&m->out, n * 4 + 256, st));
  if (!min_cover) {
    DG_TRY(b.big(&b_words, nw * 8 + 256));
    DG_TRY(b.big(&b_dir, nw * 4 + 256));
    DG_TRY(b.small(&b_scan, scan_bytes + 256));
  }
  DG_TRY(b.small(&b_ctr, sizeof(CoverCounters)));
  u32 tile = COVER_TILE;
  if (const char* e = exp_env("DICEY_COVER_TILE")) tile = (u32)std::min<u64>(std::max<u64>(1, std::strtoull(e, nullptr, 10)), COVER_TILE_MAX);
  ChunkTimer<2> tm;  // the bitmap and its directory | the per-base kernel
  DG_TRY(tm.init());
  const u32 TB = 256;
  CoverCounters* ctr = (CoverCounters*)b_ctr;
  DG_HIP(hipMemsetAsync(b_ctr, 0, sizeof(CoverCounters), st));
  DG_HIP(hipEventRecord(tm.ev[0], st));
  if (min_cover) {
    DG_HIP(hipEventRecord(tm.ev[1], st));
    hipLaunchKernelGGL(k_min_cover, dim3(ceil_div(n, tile)), dim3(TB), 0, st, (const u32*)src->out, ix->view.text, n, k, tile, m->out, ctr);
  } else {
    u64* words = (u64*)b_words;
    u32* dir = (u32*)b_dir;
    hipLaunchKernelGGL(k_spec_bits, dim3(ceil_div(nw, 16)), dim3(TB), 0, st, (const u32*)src->out, n - 1, at_most, words, nw);
    DG_HIP(rocprim::exclusive_scan(b_scan, scan_bytes, rocprim::make_transform_iterator((const u64*)words, PopcWord{}), dir, 0u, (size_t)nw,
                                   rocprim::plus<u32>(), st));
    DG_HIP(hipEventRecord(tm.ev[1], st));
    hipLaunchKernelGGL(k_cover, dim3(ceil_div(n, COVER_PER_BLOCK)), dim3(TB), 0, st, (const u64*)words, (const u32*)dir, n, k, max_count, m->out, ctr);
  }
  DG_HIP(hipEventRecord(tm.ev[2], st));
  CoverCounters hc{};
  u32 total_bits = 0;  // the directory entry of the padding word behind the data: every set bit lies in front of it
  DG_HIP(hipMemcpyAsync(&hc, b_ctr, sizeof hc, hipMemcpyDeviceToHost, st));
  if (!min_cover) DG_HIP(hipMemcpyAsync(&total_bits, (const u32*)b_dir + (nw - 1), 4, hipMemcpyDeviceToHost, st));
  DG_HIP(hipStreamSynchronize(st));
  DG_HIP(hipGetLastError());
  float ms[2] = {0, 0}, longest = 0;
  DG_TRY(tm.read(ms, 1, &longest));
  m->cv.kind = m->kind;
  m->cv.k = k;
  m->cv.at_most = at_most;
  m->cv.max_count = max_count;
  u64 specific = total_bits, covered = 0;
  for (u32 j = 0; j < COVER_SLOTS * COVER_SLOT_STRIDE; j += COVER_SLOT_STRIDE) {
    specific += hc.specific[j];
    covered += hc.covered[j];
  }
  m->cv.specific = specific;
  m->cv.covered = covered;
  m->cv.ms_bits = min_cover ? 0.0 : (double)ms[0];
  m->cv.ms_cover = ms[1];
  m->cv.transient_bytes = transient;
  m->st.ms_total = m->cv.ms_bits + m->cv.ms_cover;
  return DG_OK;
}

}  // namespace dg

using namespace dg;

extern "C" {

// mode: 0 = dg_mappability / dg_mappability_mm (p->k is k), 1 = dg_min_unique, 2 = dg_min_unique_mm (p->k is max_k)
static int map_open(dg_index* ix, const dg_map_params* p, u32 mismatches, int mode, dg_map** out) {
  const char* who = mode == 2 ? "dg_min_unique_mm" : mode ? "dg_min_unique" : "dg_mappability";
  if (p->k < 10 || p->k > 1000) return fail(DG_ELIMIT, "%s: %s = %u outside 10..1000", who, mode ? "max_k" : "k", p->k);
  if (ix->view.n < 2 || ix->view.n > 0xFFFFFFFFull) return fail(DG_ELIMIT, "%s: index of %llu suffixes", who, (unsigned long long)ix->view.n);
  if (ix->any_lane_busy()) return fail(DG_EINVAL, "%s: a dg_hunt_submit batch is in flight on this handle (dg_hunt_wait first)", who);
  DG_HIP(hipSetDevice(ix->device));
  dg_map* m = new dg_map;
  m->device = ix->device;
  m->n = ix->view.n;
  m->st.n = ix->view.n;
  m->st.k = p->k;
  m->kind = mode ? DG_MAP_KIND_LENGTH : DG_MAP_KIND_COUNT;
  m->max_count = mode ? 0u : p->max_count;
  if (hipStreamCreate(&m->stream) != hipSuccess) {
    delete m;
    return fail(DG_EHIP, "%s: cannot create a stream", who);
  }
  const int rc = mode ? min_unique_impl(who, ix, p->k, p->forward_only, mismatches, m) : map_impl(ix, p, mismatches, m);
  if (rc != DG_OK) {
    delete m;
    return rc;
  }
  *out = m;
  return DG_OK;
}

int dg_mappability(dg_index* ix, const dg_map_params* p, dg_map** out) {
  if (out) *out = nullptr;
  if (!ix || !p || !out) return fail(DG_EINVAL, "dg_mappability: null argument");
  if (p->flags) return fail(DG_EINVAL, "dg_mappability: flags must be 0");
  return map_open(ix, p, 0, 0, out);
}

int dg_mappability_mm(dg_index* ix, const dg_map_mm_params* p, dg_map** out) {
  if (out) *out = nullptr;
  if (!p || !out) return fail(DG_EINVAL, "dg_mappability_mm: null argument");
  if (p->flags || p->reserved) return fail(DG_EINVAL, "dg_mappability_mm: flags and reserved must be 0");
  if (p->mismatches > 2) return fail(DG_ELIMIT, "dg_mappability_mm: %u mismatches outside 0..2", p->mismatches);
  if (!ix) return fail(DG_EINVAL, "dg_mappability_mm: null argument");
  const dg_map_params q = {p->k, p->forward_only, p->max_count, 0u};
  return map_open(ix, &q, p->mismatches, 0, out);
}

int dg_min_unique(dg_index* ix, const dg_min_unique_params* p, dg_map** out) {
  if (out) *out = nullptr;
  if (!p || !out) return fail(DG_EINVAL, "dg_min_unique: null argument");
  if (p->flags || p->reserved) return fail(DG_EINVAL, "dg_min_unique: flags and reserved must be 0");
  if (p->max_k < 10 || p->max_k > 1000) return fail(DG_ELIMIT, "dg_min_unique: max_k = %u outside 10..1000", p->max_k);
  if (!ix) return fail(DG_EINVAL, "dg_min_unique: null argument");
  const dg_map_params q = {p->max_k, p->forward_only, 0u, 0u};
  return map_open(ix, &q, 0, 1, out);
}

int dg_min_unique_mm(dg_index* ix, const dg_min_unique_mm_params* p, dg_map** out) {
  if (out) *out = nullptr;
  if (!p || !out) return fail(DG_EINVAL, "dg_min_unique_mm: null argument");
  if (p->flags || p->reserved) return fail(DG_EINVAL, "dg_min_unique_mm: flags and reserved must be 0");
  if (p->max_k < 10 || p->max_k > 1000) return fail(DG_ELIMIT, "dg_min_unique_mm: max_k = %u outside 10..1000", p->max_k);
  if (p->mismatches > 2) return fail(DG_ELIMIT, "dg_min_unique_mm: %u mismatches outside 0..2", p->mismatches);
  if (!ix) return fail(DG_EINVAL, "dg_min_unique_mm: null argument");
  const dg_map_params q = {p->max_k, p->forward_only, 0u, 0u};
  return map_open(ix, &q, p->mismatches, 2, out);
}

int dg_query_map(dg_index* ix, const dg_qmap_params* p, const uint8_t* seqs, const uint64_t* off, size_t nseq, uint32_t* values,
                 dg_qmap_stats_t* stats) {
  if (!p) return fail(DG_EINVAL, "dg_query_map: null argument");
  if (p->flags || p->reserved[0] || p->reserved[1] || p->reserved[2]) return fail(DG_EINVAL, "dg_query_map: flags and reserved must be 0");
  if (p->k < 10 || p->k > 1000) return fail(DG_ELIMIT, "dg_query_map: k = %u outside 10..1000", p->k);
  if (p->mismatches > 2) return fail(DG_ELIMIT, "dg_query_map: %u mismatches outside 0..2", p->mismatches);
  DG_TRY(query_args_check("dg_query_map", ix, seqs, off, nseq, values, false));
  return query_call(ix, seqs, off, nseq, values, stats, [&](const std::vector<u8>& hq, std::vector<u32>& vals, dg_qmap_stats_t* st) {
    return query_map_impl("dg_query_map", ix, p, nullptr, hq, vals, st);
  });
}

int dg_query_map_anchored(dg_index* ix, const dg_qmap_anchor_params* p, const uint8_t* seqs, const uint64_t* off, size_t nseq, uint32_t* values,
                          dg_qmap_stats_t* stats) {
  if (!p) return fail(DG_EINVAL, "dg_query_map_anchored: null argument");
  if (p->flags || p->reserved[0] || p->reserved[1]) return fail(DG_EINVAL, "dg_query_map_anchored: flags and reserved must be 0");
  if (p->k < 10 || p->k > 1000) return fail(DG_ELIMIT, "dg_query_map_anchored: k = %u outside 10..1000", p->k);
  if (p->mismatches > 2) return fail(DG_ELIMIT, "dg_query_map_anchored: %u mismatches outside 0..2", p->mismatches);
  if (p->anchor > p->k) return fail(DG_ELIMIT, "dg_query_map_anchored: anchor = %u above k = %u", p->anchor, p->k);
  DG_TRY(query_args_check("dg_query_map_anchored", ix, seqs, off, nseq, values, true));
  const dg_qmap_params q = {p->k, p->mismatches, p->forward_only, p->max_count, 0u, {0u, 0u, 0u}};
  return query_call(ix, seqs, off, nseq, values, stats, [&](const std::vector<u8>& hq, std::vector<u32>& vals, dg_qmap_stats_t* st) {
    return query_map_impl("dg_query_map_anchored", ix, &q, &p->anchor, hq, vals, st);
  });
}

int dg_query_map_iupac(dg_index* ix, const dg_qmap_iupac_params* p, const uint8_t* seqs, const uint64_t* off, size_t nseq, uint32_t* values,
                       dg_qmap_iupac_stats_t* stats) {
  if (!p) return fail(DG_EINVAL, "dg_query_map_iupac: null argument");
  if (p->flags || p->reserved[0] || p->reserved[1] || p->reserved[2]) return fail(DG_EINVAL, "dg_query_map_iupac: flags and reserved must be 0");
  if (p->k < 10 || p->k > 64) return fail(DG_ELIMIT, "dg_query_map_iupac: k = %u outside 10..64", p->k);
  if (p->mismatches > 2) return fail(DG_ELIMIT, "dg_query_map_iupac: %u mismatches outside 0..2", p->mismatches);
  if (p->anchor > p->k) return fail(DG_ELIMIT, "dg_query_map_iupac: anchor = %u above k = %u", p->anchor, p->k);
  if (p->max_degeneracy > 4096) return fail(DG_ELIMIT, "dg_query_map_iupac: max_degeneracy = %u above 4096", p->max_degeneracy);
  DG_TRY(query_args_check("dg_query_map_iupac", ix, seqs, off, nseq, values, true));
  return query_call(ix, seqs, off, nseq, values, stats, [&](const std::vector<u8>& hq, std::vector<u32>& vals, dg_qmap_iupac_stats_t* st) {
    return query_map_iupac_impl("dg_query_map_iupac", ix, p, hq, vals, st);
  });
}

int dg_query_min_len(dg_index* ix, const dg_qminlen_params* p, const uint8_t* seqs, const uint64_t* off, size_t nseq, uint32_t* values,
                     dg_qminlen_stats_t* stats) {
  if (!p) return fail(DG_EINVAL, "dg_query_min_len: null argument");
  if (p->flags || p->reserved[0] || p->reserved[1]) return fail(DG_EINVAL, "dg_query_min_len: flags and reserved must be 0");
  if (p->min_k < 10 || p->min_k > 1000) return fail(DG_ELIMIT, "dg_query_min_len: min_k = %u outside 10..1000", p->min_k);
  if (p->max_k < 10 || p->max_k > 1000) return fail(DG_ELIMIT, "dg_query_min_len: max_k = %u outside 10..1000", p->max_k);
  if (p->min_k > p->max_k) return fail(DG_ELIMIT, "dg_query_min_len: min_k = %u above max_k = %u", p->min_k, p->max_k);
  if (p->mismatches > 2) return fail(DG_ELIMIT, "dg_query_min_len: %u mismatches outside 0..2", p->mismatches);
  if (p->at_most > 0xFFFFFFFDu) return fail(DG_ELIMIT, "dg_query_min_len: at_most = %u above 4294967293", p->at_most);
  DG_TRY(query_args_check("dg_query_min_len", ix, seqs, off, nseq, values, true));
  return query_call(ix, seqs, off, nseq, values, stats, [&](const std::vector<u8>& hq, std::vector<u32>& vals, dg_qminlen_stats_t* st) {
    return query_min_len_impl("dg_query_min_len", ix, p, nullptr, hq, vals, st);
  });
}

int dg_query_min_len_end(dg_index* ix, const dg_qminlen_end_params* p, const uint8_t* seqs, const uint64_t* off, size_t nseq, uint32_t* values,
                         dg_qminlen_stats_t* stats) {
  if (!p) return fail(DG_EINVAL, "dg_query_min_len_end: null argument");
  if (p->flags || p->reserved[0] || p->reserved[1]) return fail(DG_EINVAL, "dg_query_min_len_end: flags and reserved must be 0");
  if (p->min_k < 10 || p->min_k > 1000) return fail(DG_ELIMIT, "dg_query_min_len_end: min_k = %u outside 10..1000", p->min_k);
  if (p->max_k < 10 || p->max_k > 1000) return fail(DG_ELIMIT, "dg_query_min_len_end: max_k = %u outside 10..1000", p->max_k);
  if (p->min_k > p->max_k) return fail(DG_ELIMIT, "dg_query_min_len_end: min_k = %u above max_k = %u", p->min_k, p->max_k);
  if (p->mismatches > 2) return fail(DG_ELIMIT, "dg_query_min_len_end: %u mismatches outside 0..2", p->mismatches);
  if (p->at_most > 0xFFFFFFFDu) return fail(DG_ELIMIT, "dg_query_min_len_end: at_most = %u above 4294967293", p->at_most);
  if (p->anchor > p->min_k) return fail(DG_ELIMIT, "dg_query_min_len_end: anchor = %u above min_k = %u", p->anchor, p->min_k);
  DG_TRY(query_args_check("dg_query_min_len_end", ix, seqs, off, nseq, values, true));
  const dg_qminlen_params q = {p->min_k, p->max_k, p->mismatches, p->forward_only, p->at_most, 0u, {0u, 0u}};
  return query_call(ix, seqs, off, nseq, values, stats, [&](const std::vector<u8>& hq, std::vector<u32>& vals, dg_qminlen_stats_t* st) {
    return query_min_len_impl("dg_query_min_len_end", ix, &q, &p->anchor, hq, vals, st);
  });
}


int dg_map_mm_stats(const dg_map* m, dg_map_mm_stats_t* out) {
  if (!m || !out) return fail(DG_EINVAL, "dg_map_mm_stats: null argument");
  *out = m->mm;
  return DG_OK;
}

int dg_map_mu_mm_stats(const dg_map* m, dg_mu_mm_stats_t* out) {
  if (!m || !out) return fail(DG_EINVAL, "dg_map_mu_mm_stats: null argument");
  *out = m->mu;
  return DG_OK;
}

// the checks behind the parameter block that dg_map_cover and dg_map_min_cover share, then the transform
static int cover_open(const char* who, dg_index* ix, const dg_map* src, bool min_cover, u32 at_most, u32 max_count, dg_map** out) {
  if (!ix) return fail(DG_EINVAL, "%s: null argument", who);
  if (min_cover ? src->kind != DG_MAP_KIND_LENGTH : src->kind != DG_MAP_KIND_COUNT)
    return fail(DG_EINVAL, "%s: the source map holds %s, not %s", who,
                src->kind == DG_MAP_KIND_COUNT ? "counts" : src->kind == DG_MAP_KIND_LENGTH ? "lengths" : "per-base values", min_cover ? "lengths" : "counts");
  if (src->n != ix->view.n || src->device != ix->device)
    return fail(DG_EINVAL, "%s: the source map is of an index of %llu suffixes on device %d, the handle's has %llu on device %d", who,
                (unsigned long long)src->n, src->device, (unsigned long long)ix->view.n, ix->device);
  if (!min_cover && src->max_count && at_most >= src->max_count)
    return fail(DG_EINVAL, "%s: the source map was made with max_count = %u and cannot tell counts up to at_most = %u apart", who, src->max_count, at_most);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(DG_ENODEV, "%s: no HIP device available", who);
  DG_HIP(hipSetDevice(src->device));
  dg_map* m = new dg_map;
  m->device = src->device;
  m->n = src->n;
  m->st.n = src->n;
  m->st.k = src->st.k;
  m->kind = min_cover ? DG_MAP_KIND_MIN_COVER : DG_MAP_KIND_COVER;
  m->max_count = max_count;
  if (hipStreamCreate(&m->stream) != hipSuccess) {
    delete m;
    return fail(DG_EHIP, "%s: cannot create a stream", who);
  }
  const int rc = cover_impl(who, ix, src, min_cover, at_most, max_count, m);
  if (rc != DG_OK) {
    delete m;
    return rc;
  }
  *out = m;
  return DG_OK;
}

int dg_map_cover(dg_index* ix, const dg_map* src, const dg_cover_params* p, dg_map** out) {
  if (out) *out = nullptr;
  if (!p || !out || !src) return fail(DG_EINVAL, "dg_map_cover: null argument");
  if (p->flags || p->reserved) return fail(DG_EINVAL, "dg_map_cover: flags and reserved must be 0");
  if (p->at_most < 1 || p->at_most > 0xFFFFFFFDu) return fail(DG_ELIMIT, "dg_map_cover: at_most = %u outside 1..4294967293", p->at_most);
  return cover_open("dg_map_cover", ix, src, false, p->at_most, p->max_count, out);
}

int dg_map_min_cover(dg_index* ix, const dg_map* src, const dg_min_cover_params* p, dg_map** out) {
  if (out) *out = nullptr;
  if (!p || !out || !src) return fail(DG_EINVAL, "dg_map_min_cover: null argument");
  if (p->flags || p->reserved) return fail(DG_EINVAL, "dg_map_min_cover: flags and reserved must be 0");
  return cover_open("dg_map_min_cover", ix, src, true, 0u, 0u, out);
}

int dg_map_cover_stats(const dg_map* m, dg_cover_stats_t* out) {
  if (!m || !out) return fail(DG_EINVAL, "dg_map_cover_stats: null argument");
  *out = m->cv;
  return DG_OK;
}

int dg_map_values(dg_map* m, uint64_t lo, uint64_t hi, uint32_t* out) {
  if (!m || (!out && hi > lo)) return fail(DG_EINVAL, "dg_map_values: null argument");
  if (lo > hi || hi > m->n - 1) return fail(DG_EINVAL, "dg_map_values: range [%llu, %llu) outside [0, %llu)", (unsigned long long)lo,
                                            (unsigned long long)hi, (unsigned long long)(m->n - 1));
  if (hi == lo) return DG_OK;
  DG_HIP(hipSetDevice(m->device));
  DG_HIP(hipMemcpyAsync(out, m->out + lo, (hi - lo) * 4, hipMemcpyDeviceToHost, m->stream));
  DG_HIP(hipStreamSynchronize(m->stream));
  return DG_OK;
}

int dg_map_runs(dg_map* m, uint64_t lo, uint64_t hi, uint64_t* nruns, uint64_t** start, uint32_t** len, uint32_t** value) {
  if (!m || !nruns || !start || !len || !value) return fail(DG_EINVAL, "dg_map_runs: null argument");
  *nruns = 0;
  *start = nullptr;
  *len = nullptr;
  *value = nullptr;
  if (lo > hi || hi > m->n - 1) return fail(DG_EINVAL, "dg_map_runs: range [%llu, %llu) outside [0, %llu)", (unsigned long long)lo,
                                            (unsigned long long)hi, (unsigned long long)(m->n - 1));
  DG_HIP(hipSetDevice(m->device));
  // the range goes through in chunks of positions; a run that crosses a chunk edge has its start in one chunk and its end in a later
  // one, and since starts and ends alternate along the range the two lists pair up in order
  u64 chunk = 1ULL << 24;
  if (const char* e = exp_env("DICEY_MAP_CHUNK")) chunk = std::max<u64>(1, std::strtoull(e, nullptr, 10));
  const u64 cmax = std::min<u64>(chunk, hi - lo);
  hipStream_t st = m->stream;
  rocprim::counting_iterator<u32> cnt0(0);
  size_t sel_bytes = 0;
  DG_HIP(rocprim::select(nullptr, sel_bytes, cnt0, (const u8*)nullptr, (u32*)nullptr, (unsigned long long*)nullptr, (size_t)std::max<u64>(cmax, 1), st));
  DG_TRY(m->run_flags.reserve(2 * cmax + 512 + sel_bytes));
  DG_TRY(m->run_pos.reserve(8 * cmax + 64));
  DG_TRY(m->run_val.reserve(4 * cmax + 64));
  DG_TRY(m->run_cnt.reserve(64));
  u8* fs = m->run_flags.as<u8>();
  u8* fe = fs + cmax;
  void* sel_tmp = (void*)(((uintptr_t)(fe + cmax) + 255) & ~(uintptr_t)255);
  u32* ps = m->run_pos.as<u32>();
  u32* pe = ps + cmax;
  u32* pv = m->run_val.as<u32>();
  unsigned long long* dc = m->run_cnt.as<unsigned long long>();
  std::vector<u64> S, E;
  std::vector<u32> V, hs, he;
  for (u64 a = lo; a < hi; a += chunk) {
    const u64 l = std::min<u64>(chunk, hi - a);
    hipLaunchKernelGGL(k_run_flags, dim3(ceil_div(l, 256)), dim3(256), 0, st, (const u32*)m->out, lo, hi, a, l, fs, fe);
    size_t b1 = sel_bytes;
    DG_HIP(rocprim::select(sel_tmp, b1, cnt0, (const u8*)fs, ps, dc, (size_t)l, st));
    DG_HIP(rocprim::select(sel_tmp, b1, cnt0, (const u8*)fe, pe, dc + 1, (size_t)l, st));
    hipLaunchKernelGGL(k_run_values, dim3(ceil_div(l, 256)), dim3(256), 0, st, (const u32*)m->out, a, (const u32*)ps, (const unsigned long long*)dc, pv);
    unsigned long long hc[2] = {0, 0};
    DG_HIP(hipMemcpyAsync(hc, dc, 16, hipMemcpyDeviceToHost, st));
    DG_HIP(hipStreamSynchronize(st));
    hs.resize(hc[0]);
    he.resize(hc[1]);
    const size_t v0 = V.size();
    V.resize(v0 + hc[0]);
    if (hc[0]) {
      DG_HIP(hipMemcpyAsync(hs.data(), ps, hc[0] * 4, hipMemcpyDeviceToHost, st));
      DG_HIP(hipMemcpyAsync(V.data() + v0, pv, hc[0] * 4, hipMemcpyDeviceToHost, st));
    }
    if (hc[1]) DG_HIP(hipMemcpyAsync(he.data(), pe, hc[1] * 4, hipMemcpyDeviceToHost, st));
    DG_HIP(hipStreamSynchronize(st));
    DG_HIP(hipGetLastError());
    for (u32 x : hs) S.push_back(a + x);
    for (u32 x : he) E.push_back(a + x);
  }
  if (S.size() != E.size() || S.size() != V.size())
    return fail(DG_EHIP, "dg_map_runs: %zu run starts but %zu ends", S.size(), E.size());
  const u64 nr = S.size();
  uint64_t* s = (uint64_t*)std::malloc(nr * 8 + 8);
  uint32_t* ln = (uint32_t*)std::malloc(nr * 4 + 4);
  uint32_t* vv = (uint32_t*)std::malloc(nr * 4 + 4);
  if (!s || !ln || !vv) {
    std::free(s);
    std::free(ln);
    std::free(vv);
    return fail(DG_ENOMEM, "dg_map_runs: %llu runs do not fit in host memory", (unsigned long long)nr);
  }
  for (u64 j = 0; j < nr; ++j) {
    s[j] = S[j];
    ln[j] = (uint32_t)(E[j] - S[j] + 1);
    vv[j] = V[j];
  }
  *nruns = nr;
  *start = s;
  *len = ln;
  *value = vv;
  return DG_OK;
}

const void* dg_map_device_values(const dg_map* m) { return m ? m->out : nullptr; }

int dg_map_stats(const dg_map* m, dg_map_stats_t* out) {
  if (!m || !out) return fail(DG_EINVAL, "dg_map_stats: null argument");
  *out = m->st;
  return DG_OK;
}

void dg_map_free(dg_map* m) { delete m; }

}  // extern "C"
