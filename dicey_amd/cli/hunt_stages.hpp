// The stages of `dicey hunt` (hunt.cpp) that need neither the GPU nor the library: the query reader, the open-flag rules, the chunk
// packer, the (rank, chunk, piece) plan of the one-process-per-GPU mode and the decoding of a gathered block.  Only the plain structs
// and constants of include/dicey_gpu.h are used, so a host program compiles this header on its own (tests/host/hunt_stages_main.cpp).
#pragma once
#include <sys/stat.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/dicey_gpu.h"

namespace hunt {

// one query of the input: name and sequence as views of the input file's bytes (r06: 10 M records as pairs of std::string were 20 M
// heap allocations, half a second of a 3 s run); a sequence that spans several lines is joined in `owned`
struct Query {
  std::string_view first, second;
};

// The queries of one input and the bytes their views point into.  Copying is deleted (the copy's views would point into the
// original); moving is the default and keeps every view valid: a moved std::vector or std::deque hands over its storage, no
// element changes its address, and no view points into a std::string that is itself moved (qfile is a vector for that reason: a
// short std::string carries its bytes inside the object).
struct QuerySet {
  std::vector<char> qfile;        // the input file's bytes: names and sequences are views of it
  std::deque<std::string> owned;  // sequences that span several lines, joined; the literal sequence of a non-regular input
  std::vector<Query> queries;
  bool bad_fasta = false;
  QuerySet() = default;
  QuerySet(const QuerySet&) = delete;
  QuerySet& operator=(const QuerySet&) = delete;
  QuerySet(QuerySet&&) = default;
  QuerySet& operator=(QuerySet&&) = default;
};

// hunter.h:272-283 over the whole file in memory (10 M records: std::getline per line was seconds).  A record = a name line and the
// non-empty lines up to the next '>' (std::getline keeps a '\r', so does this); the reference keeps a record when name and sequence
// are both non-empty (hunter.h:276-283).
inline void parse_records(QuerySet& qs) {
  qs.queries.reserve(qs.qfile.size() / 28 + 16);
  std::string_view name, seq;
  bool have = false, joined = false;
  auto flush = [&]() {
    if (have && !name.empty() && !seq.empty()) qs.queries.push_back(Query{name, seq});
    else if (joined) qs.owned.pop_back();
  };
  const char* p0 = qs.qfile.data();
  const char* const end = p0 + qs.qfile.size();
  while (p0 < end) {
    const char* nl = (const char*)std::memchr(p0, '\n', (size_t)(end - p0));
    const char* e = nl ? nl : end;
    if (e > p0) {  // (empty lines are skipped)
      if (*p0 == '>') {
        flush();
        name = std::string_view(p0 + 1, (size_t)(e - p0 - 1));
        seq = std::string_view();
        have = true;
        joined = false;
      } else if (seq.empty() && !joined) seq = std::string_view(p0, (size_t)(e - p0));
      else {  // a second sequence line: the record's sequence moves into a string of its own
        if (!joined) {
          qs.owned.emplace_back(seq);
          joined = true;
        }
        qs.owned.back().append(p0, e);
        seq = qs.owned.back();
      }
    }
    p0 = nl ? nl + 1 : end;
  }
  flush();
}

// hunter.h:262-287: a FASTA file of queries, or the literal sequence when `input` names no regular file.  `looks_fasta` is the
// reference's is_fasta (util.h:35-52: it reads through zlib, which this header does not ask for); a file it refuses sets bad_fasta.
inline QuerySet read_queries(const std::string& input, bool (*looks_fasta)(const std::string&)) {
  QuerySet qs;
  struct stat st;
  if (!(stat(input.c_str(), &st) == 0 && S_ISREG(st.st_mode))) {
    qs.owned.emplace_back(input);
    qs.queries.push_back(Query{std::string_view(), std::string_view(qs.owned.back())});
    return qs;
  }
  if (!looks_fasta(input)) {
    qs.bad_fasta = true;
    return qs;
  }
  if (FILE* f = std::fopen(input.c_str(), "rb")) {
    std::fseek(f, 0, SEEK_END);
    const long sz = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    qs.qfile.resize(sz > 0 ? (size_t)sz : 0);
    if (sz > 0 && std::fread(qs.qfile.data(), 1, (size_t)sz, f) != (size_t)sz) qs.qfile.clear();
    std::fclose(f);
  }
  parse_records(qs);
  return qs;
}

// What the environment says about the index open: DICEY_FULL_TABLE, DICEY_RESIDENT_LAYOUTS and DICEY_KMER_K are set or not.
struct OpenEnv {
  bool full_table = false, resident_layouts = false, kmer_k = false;
};
// The K-mer jump table (up to 137 GB, ~1.5 s to derive) only pays off for large batches: a literal sequence or a small FASTA is
// answered from the Occ blocks alone.  A process that opens the index for one input keeps the table compact (DG_OPEN_COMPACT): the
// 137 GB form saves microseconds per batch and costs seconds to allocate when the driver still has to wipe memory another process
// released (DG_OPEN_COMPACT since ABI 7: without the layouts that only pay for a resident index — the suffix array with context
// and its prefix levels are 40 GB, 0.36 s to derive and a second of driver wipe at exit, against 0.3 ms per 100 000 queries of a
// repeat-rich batch).  The preceding-characters array (0.19 s to derive) saves a fifth of the distance-1 search kernel and a
// twentieth of the distance-2 one: 0.3 ms per million queries at distance 1, 3 ms at distance 2 — left out unless the input is
// large enough to earn it back.
inline uint32_t hunt_open_flags(bool is_file, long long size, uint32_t distance, const OpenEnv& env) {
  uint32_t flags = (env.full_table ? DG_OPEN_BIG_TABLE : DG_OPEN_DEFAULT) | (env.resident_layouts ? 0u : DG_OPEN_COMPACT);
  if (!(is_file && size > (1 << 20)) && !env.kmer_k) flags |= DG_OPEN_NO_KMER_TABLE;
  if ((flags & DG_OPEN_COMPACT) && !(is_file && size > (distance >= 2 ? (1ll << 30) : (8ll << 30)))) flags |= DG_OPEN_NO_PRE5;
  return flags;
}

// Queries [q0, q1) as one batch of the library: the bytes in a row, their offsets, and the chunk's own parameters — the longest
// query as the bound (the library sizes the batch without another pass over the offsets) and compact results.
struct ChunkPack {
  std::string bytes;
  std::vector<uint64_t> off;
  dg_hunt_params params;
};
inline ChunkPack pack_chunk(const std::vector<Query>& queries, size_t q0, size_t q1, const dg_hunt_params& hp) {
  ChunkPack p{std::string(), std::vector<uint64_t>(q1 - q0 + 1, 0), hp};
  size_t longest = 0;
  for (size_t i = 0; i < q1 - q0; ++i) {
    p.bytes += queries[q0 + i].second;
    p.off[i + 1] = p.bytes.size();
    longest = std::max(longest, queries[q0 + i].second.size());
  }
  p.params.max_query_len = (uint32_t)std::min<size_t>(longest, 0xFFFFFFu);
  p.params.flags = DG_HUNT_COMPACT;
  return p;
}

// One process per GPU: rank r searches queries [r * per, (r + 1) * per) in chunks of CH; a chunk the library refuses is cut into
// `parts` equal pieces.  Everything here is a function of (nq, N) and (range, parts) alone, so rank 0 rebuilds every rank's ranges
// and pieces, and the number of chunks is the same on every rank: the collectives stay in step.
struct RankPlan {
  static constexpr size_t CH = 1u << 17;
  size_t nq, per, nchunks;
  RankPlan(size_t nq_, int N) : nq(nq_), per((nq_ + N - 1) / N), nchunks(std::max<size_t>(1, (per + CH - 1) / CH)) {}
  void range_of(int r, size_t k, size_t& q0, size_t& q1) const {
    const size_t s0 = std::min(nq, (size_t)r * per), s1 = std::min(nq, s0 + per);
    q0 = std::min(s1, s0 + k * CH);
    q1 = std::min(s1, q0 + CH);
  }
  static void piece_of(size_t q0, size_t q1, uint64_t parts, uint64_t pc, size_t& a, size_t& b) {
    const size_t n = q1 - q0;
    a = q0 + (size_t)((unsigned __int128)n * pc / parts);
    b = q0 + (size_t)((unsigned __int128)n * (pc + 1) / parts);
  }
};

// The block rank r sent for n queries as a compact result: [hit counts | query words | records].  S points into blk and hit_off;
// nseq and seq_start are the caller's.  false and the reason when the sizes do not fit.
inline bool block_as_result(const uint8_t* blk, size_t bytes, size_t n, int r, uint32_t nseq, uint64_t* seq_start, dg_hunt_result& S,
                            std::vector<uint64_t>& hit_off, std::string& why) {
  if (bytes < 8 * n) {
    why = "rank " + std::to_string(r) + " sent " + std::to_string(bytes) + " bytes for " + std::to_string(n) + " queries";
    return false;
  }
  S = dg_hunt_result{};
  hit_off.assign(n + 1, 0);
  const uint32_t* qh = (const uint32_t*)blk;
  for (size_t i = 0; i < n; ++i) hit_off[i + 1] = hit_off[i] + qh[i];
  S.nq = n;
  S.nhits = hit_off[n];
  const uint64_t rec_bytes = bytes - 8 * n;
  if (S.nhits && (rec_bytes % (4 * S.nhits) != 0 || rec_bytes / (4 * S.nhits) < 2)) {
    why = "rank " + std::to_string(r) + ": " + std::to_string(rec_bytes) + " record bytes for " + std::to_string(S.nhits) + " hits";
    return false;
  }
  S.ops_per_hit = S.nhits ? (uint32_t)(rec_bytes / (4 * S.nhits)) - 2 : 0;
  S.hit_off = hit_off.data();
  S.qinfo = const_cast<uint32_t*>(qh) + n;
  S.chits = const_cast<uint32_t*>(qh) + 2 * n;
  S.compact = 1;
  S.nseq = nseq;
  S.seq_start = seq_start;
  return true;
}

}  // namespace hunt
