// dicey_amd/cli/hunt_stages.hpp as a program of its own (tests/test_hunt_stages_host.py builds it plain and under the address and
// undefined-behaviour sanitizers): the query reader against a line-by-line model, the rank plan, the chunk packer, the decoding of
// a gathered block and the open-flag rules.  Exits non-zero with a message on the first mismatch.  argv[1]: a directory for the files.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <utility>
#include <vector>

#include "../../dicey_amd/cli/hunt_stages.hpp"
#include "../../include/dicey_gpu.h"

namespace {

[[noreturn]] void fail(const std::string& what) {
  std::fprintf(stderr, "FAILED: %s\n", what.c_str());
  std::exit(1);
}
void check(bool good, const std::string& what) {
  if (!good) fail(what);
}
std::string shown(const std::string& s) {
  std::string o;
  for (char c : s) o += c == '\n' ? "\\n" : c == '\r' ? "\\r" : std::string(1, c);
  return o;
}

// ------------------------------------------------------------------------------------------------ read_queries
using Records = std::vector<std::pair<std::string, std::string>>;

// hunter.h:272-283, line by line
Records model_records(const std::string& path) {
  Records queries;
  std::ifstream fafile(path.c_str());
  std::string line, fan, faseq;
  while (std::getline(fafile, line)) {  // hunter.h:275
    if (line.empty()) continue;         // hunter.h:276
    if (line[0] == '>') {               // hunter.h:277
      if (!fan.empty() && !faseq.empty()) queries.push_back(std::make_pair(fan, faseq));  // hunter.h:278
      faseq = "";                       // hunter.h:279
      fan = line.substr(1);             // hunter.h:280
    } else faseq += line;               // hunter.h:281
  }
  if (!fan.empty() && !faseq.empty()) queries.push_back(std::make_pair(fan, faseq));  // hunter.h:283
  return queries;
}

bool any_file(const std::string&) { return true; }
bool no_file(const std::string&) { return false; }

std::string g_dir;
size_t g_files = 0, g_records = 0, g_joined = 0;

void reader_case(const std::string& bytes) {
  const std::string path = g_dir + "/queries.fa";
  {
    std::ofstream f(path.c_str(), std::ios::binary | std::ios::trunc);
    f.write(bytes.data(), (std::streamsize)bytes.size());
  }
  const Records want = model_records(path);
  hunt::QuerySet qs;
  {
    hunt::QuerySet first = hunt::read_queries(path, any_file);
    g_joined += first.owned.size();
    qs = std::move(first);  // a move keeps the views (hunt.cpp moves the set out of its reader); the moved-from set is gone below
  }
  // compared as strings after all parsing (and the move) is done: a view of freed or moved bytes shows under the address sanitizer
  check(!qs.bad_fasta, "bad_fasta for \"" + shown(bytes) + "\"");
  check(qs.queries.size() == want.size(), std::to_string(qs.queries.size()) + " records, the model " + std::to_string(want.size()) + " for \"" + shown(bytes) + "\"");
  for (size_t i = 0; i < want.size(); ++i) {
    const std::string name(qs.queries[i].first), seq(qs.queries[i].second);
    check(name == want[i].first && seq == want[i].second,
          "record " + std::to_string(i) + " of \"" + shown(bytes) + "\": (" + shown(name) + ", " + shown(seq) + "), the model (" + shown(want[i].first) + ", " + shown(want[i].second) + ")");
  }
  // every joined sequence that was kept is a record's; the dropped ones are gone
  size_t joined = 0;
  for (const hunt::Query& q : qs.queries)
    for (const std::string& o : qs.owned) joined += q.second.data() == o.data();
  check(joined == qs.owned.size(), "a joined sequence without a record for \"" + shown(bytes) + "\"");
  ++g_files;
  g_records += want.size();
}

void test_read_queries() {
  const char* hand[] = {
      "",                                    // an empty file
      ">a\nACGT",                            // no trailing newline
      ">a\nACGT\n",
      ">",                                   // only '>'
      ">\n",
      ">name\n",                             // a name with no sequence
      ">name",
      "ACGT\n>a\nGGCC\n",                    // a sequence before any header
      "ACGT\nTTTT\n>a\nGGCC\n",              // ... of two lines (joined, then dropped)
      ">a\r\nACGT\r\n>b\r\nGG\r\nCC\r\n",    // CRLF: the '\r' stays in name and sequence
      "\n\n>a\n\nAC\n\n\nGT\n\n>b\n\nTT\n\n",  // blank lines between and inside records
      ">a\nAAAA\nCCCC\nGGGG\n>b\nT\n",       // a three-line sequence
      ">\nAC\nGT\n>good\nTTTT\n",            // a joined record with an empty name, then a good one (the joined string is dropped)
      ">a\nAC\nGT\n>b\nTT\nAA\n>c\nG\n",     // two joined records in a row
      ">\nAC\nGT\n>\nTT\nAA\n>c\nG\nC\n",    // two dropped joined records, then a kept one
      ">a name with blanks \t x\nACGT\n",    // a name with blanks
      ">a\n>b\nAC\n>c\n",                    // headers in a row
      ">a\nAC\n>",                           // ends on a bare '>'
      "\r\n>a\n\r\nAC\n",                    // a line of '\r' alone is a sequence line
  };
  for (const char* h : hand) reader_case(h);
  const char* pieces[] = {">", ">n", ">n x", "ACGT", "", "AC\r", "N"};
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto next = [&x]() {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return x >> 11;
  };
  for (int f = 0; f < 2000; ++f) {
    std::string bytes;
    const size_t lines = next() % 41;
    for (size_t l = 0; l < lines; ++l) {
      bytes += pieces[next() % 7];
      if (l + 1 < lines || (f & 1)) bytes.push_back('\n');
    }
    reader_case(bytes);
  }
  check(g_joined > 1000 && g_records > 5000, "the generated files hold too few joined sequences or records");
  // a regular file the FASTA check refuses: no record, bad_fasta
  const hunt::QuerySet bad = hunt::read_queries(g_dir + "/queries.fa", no_file);
  check(bad.bad_fasta && bad.queries.empty(), "a refused file must set bad_fasta and give no query");
  // not a regular file: the literal sequence, no name
  for (const std::string& literal : {std::string("CATTACTAACATCAGT"), g_dir, g_dir + "/no_such_file_ACGT", std::string()}) {
    hunt::QuerySet lit = hunt::read_queries(literal, no_file);
    hunt::QuerySet moved = std::move(lit);
    check(!moved.bad_fasta && moved.queries.size() == 1, "a non-regular path is one query");
    check(moved.queries[0].first.empty() && std::string(moved.queries[0].second) == literal, "a non-regular path is the literal sequence without a name");
  }
}

// ------------------------------------------------------------------------------------------------ RankPlan
void test_rank_plan() {
  const size_t CH = 1u << 17;
  check(hunt::RankPlan::CH == CH, "CH");
  for (size_t nq : {(size_t)0, (size_t)1, (size_t)2, (size_t)131071, (size_t)131072, (size_t)131073, (size_t)1000003})
    for (int N : {1, 2, 3, 8}) {
      const hunt::RankPlan plan(nq, N);
      const std::string at = "nq " + std::to_string(nq) + " N " + std::to_string(N);
      check(plan.per == (nq + N - 1) / N && plan.nchunks == std::max<size_t>(1, (plan.per + CH - 1) / CH), at + ": per / nchunks");
      size_t cursor = 0;
      for (int r = 0; r < N; ++r) {
        check(hunt::RankPlan(nq, N).nchunks == plan.nchunks, at + ": nchunks differs between ranks");
        for (size_t k = 0; k < plan.nchunks; ++k) {
          size_t q0 = ~(size_t)0, q1 = ~(size_t)0;
          plan.range_of(r, k, q0, q1);
          check(q0 <= q1 && q1 - q0 <= CH && q1 <= nq, at + ": a range out of shape");
          if (q1 > q0) check(q0 == cursor, at + ": gap or overlap at rank " + std::to_string(r) + " chunk " + std::to_string(k));
          if (q1 > q0) cursor = q1;
        }
      }
      check(cursor == nq, at + ": the ranges end at " + std::to_string(cursor));
    }
  for (size_t len = 0; len <= 70; ++len)
    for (uint64_t parts : {1, 2, 4, 8, 64, 128}) {
      const size_t q0 = 1000;
      size_t cursor = q0;
      for (uint64_t pc = 0; pc < parts; ++pc) {
        size_t a = 0, b = 0;
        hunt::RankPlan::piece_of(q0, q0 + len, parts, pc, a, b);
        check(a == cursor && b >= a, "pieces of " + std::to_string(len) + " in " + std::to_string(parts) + ": piece " + std::to_string(pc));
        check(b - a <= (len + parts - 1) / parts, "a piece larger than its share");
        cursor = b;
      }
      check(cursor == q0 + len, "pieces of " + std::to_string(len) + " in " + std::to_string(parts) + " end early");
    }
  // n * pc beyond 64 bits (the 128-bit product): floor(n * pc / parts) = (n / parts) * pc + floor((n % parts) * pc / parts)
  for (size_t n : {((size_t)1 << 56) + 3, ((size_t)1 << 62) + 77, ((size_t)1 << 63) / 128 - 1}) {
    const uint64_t parts = 128;
    for (uint64_t pc : {(uint64_t)0, (uint64_t)1, (uint64_t)126, (uint64_t)127}) {
      size_t a = 0, b = 0;
      hunt::RankPlan::piece_of(5, 5 + n, parts, pc, a, b);
      const size_t wa = 5 + (n / parts) * pc + (n % parts) * pc / parts, wb = 5 + (n / parts) * (pc + 1) + (n % parts) * (pc + 1) / parts;
      check(a == wa && b == wb, "piece " + std::to_string(pc) + " of a range of " + std::to_string(n));
    }
  }
}

// ------------------------------------------------------------------------------------------------ pack_chunk
void test_pack_chunk() {
  dg_hunt_params hp{};
  hp.distance = 2;
  hp.hamming = 1;
  hp.forward_only = 1;
  hp.max_locations = 77;
  hp.max_neighborhood = 999;
  hp.max_query_len = 5;                 // overwritten by the chunk's own
  hp.flags = DG_HUNT_PHASE_TIMES | 64;  // likewise
  const std::string big(0x1000000, 'A');
  const std::string seqs[] = {"ACGT", "", "GGGCCCTTTAAA", "N", big};
  std::vector<hunt::Query> queries;
  for (const std::string& s : seqs) queries.push_back(hunt::Query{"name", s});
  auto held = [&](size_t q0, size_t q1, uint32_t want_longest) {
    const hunt::ChunkPack p = hunt::pack_chunk(queries, q0, q1, hp);
    const std::string at = "pack_chunk [" + std::to_string(q0) + ", " + std::to_string(q1) + ")";
    std::string bytes;
    check(p.off.size() == q1 - q0 + 1 && p.off[0] == 0, at + ": offsets");
    for (size_t i = q0; i < q1; ++i) {
      bytes += seqs[i];
      check(p.off[i - q0 + 1] == bytes.size(), at + ": offset " + std::to_string(i - q0 + 1));
    }
    check(p.bytes == bytes, at + ": bytes");
    check(p.params.max_query_len == want_longest && p.params.flags == DG_HUNT_COMPACT, at + ": max_query_len / flags");
    check(p.params.distance == 2 && p.params.hamming == 1 && p.params.forward_only == 1 && p.params.max_locations == 77 && p.params.max_neighborhood == 999,
          at + ": the run's parameters are copied");
  };
  held(0, 0, 0);  // an empty range
  held(2, 2, 0);
  held(0, 1, 4);  // one query
  held(1, 2, 0);  // ... an empty one
  held(0, 4, 12);
  held(1, 4, 12);
  held(4, 5, 0xFFFFFF);  // 0x1000000 bytes: the bound saturates
  held(0, 5, 0xFFFFFF);
}

// ------------------------------------------------------------------------------------------------ block_as_result
void test_block_as_result() {
  const size_t n = 3;
  const uint32_t counts[n] = {2, 0, 1}, qinfo[n] = {0x101, 0x102, 0x30103};
  uint64_t seq_start[3] = {0, 100, 250};
  for (uint32_t ops : {0u, 3u}) {
    std::vector<uint32_t> words(counts, counts + n);
    words.insert(words.end(), qinfo, qinfo + n);
    for (uint32_t w = 0; w < 3 * (2 + ops); ++w) words.push_back(0xC0000000u + w);
    const uint8_t* blk = (const uint8_t*)words.data();
    const size_t bytes = 4 * words.size();
    dg_hunt_result S;
    std::vector<uint64_t> hit_off(7, 99);
    std::string why = "untouched";
    check(hunt::block_as_result(blk, bytes, n, 1, 2, seq_start, S, hit_off, why), "a well-formed block is refused: " + why);
    check(S.nq == n && S.nhits == 3 && S.ops_per_hit == ops && S.compact == 1 && S.nseq == 2 && S.seq_start == seq_start, "block: counts and sequences");
    check(hit_off == std::vector<uint64_t>({0, 2, 2, 3}) && S.hit_off == hit_off.data(), "block: hit_off");
    check(S.qinfo == words.data() + n && S.chits == words.data() + 2 * n && S.qinfo[2] == 0x30103 && S.chits[0] == 0xC0000000u, "block: pointers");
    check(S.hits == nullptr && S.ops == nullptr && S.qseq == nullptr && S.d_block == nullptr && S.owner_ == nullptr, "block: the rest is zero");
    // sizes that do not fit, with the messages as they are
    check(!hunt::block_as_result(blk, 8 * n - 1, n, 1, 2, seq_start, S, hit_off, why) && why == "rank 1 sent 23 bytes for 3 queries", "short block: " + why);
    check(!hunt::block_as_result(blk, 0, n, 0, 2, seq_start, S, hit_off, why) && why == "rank 0 sent 0 bytes for 3 queries", "empty block: " + why);
    check(!hunt::block_as_result(blk, 8 * n + 25, n, 7, 2, seq_start, S, hit_off, why) && why == "rank 7: 25 record bytes for 3 hits", "odd record bytes: " + why);
    check(!hunt::block_as_result(blk, 8 * n + 12, n, 2, 2, seq_start, S, hit_off, why) && why == "rank 2: 12 record bytes for 3 hits", "one word per hit: " + why);
    check(!hunt::block_as_result(blk, 8 * n, n, 2, 2, seq_start, S, hit_off, why) && why == "rank 2: 0 record bytes for 3 hits", "no record bytes: " + why);
  }
  const uint32_t none[6] = {0, 0, 0, 7, 8, 9};
  dg_hunt_result S;
  std::vector<uint64_t> hit_off;
  std::string why;
  check(hunt::block_as_result((const uint8_t*)none, sizeof none, n, 0, 2, seq_start, S, hit_off, why), "a block without hits is refused: " + why);
  check(S.nhits == 0 && S.ops_per_hit == 0 && S.nq == n && hit_off == std::vector<uint64_t>(4, 0) && S.qinfo[1] == 8, "block without hits");
}

// ------------------------------------------------------------------------------------------------ hunt_open_flags
// the rules as hunter() had them inline, evaluated once for: is_file 0, 1 x the six sizes x distance 1, 2 x (DICEY_FULL_TABLE,
// DICEY_RESIDENT_LAYOUTS, DICEY_KMER_K as bits 0, 1, 2), innermost last
const uint32_t kOpenFlags[192] = {
    22, 30, 2, 10, 20, 28, 0, 8, 22, 30, 2, 10, 20, 28, 0, 8,
    22, 30, 2, 10, 20, 28, 0, 8, 22, 30, 2, 10, 20, 28, 0, 8,
    22, 30, 2, 10, 20, 28, 0, 8, 22, 30, 2, 10, 20, 28, 0, 8,
    22, 30, 2, 10, 20, 28, 0, 8, 22, 30, 2, 10, 20, 28, 0, 8,
    22, 30, 2, 10, 20, 28, 0, 8, 22, 30, 2, 10, 20, 28, 0, 8,
    22, 30, 2, 10, 20, 28, 0, 8, 22, 30, 2, 10, 20, 28, 0, 8,
    22, 30, 2, 10, 20, 28, 0, 8, 22, 30, 2, 10, 20, 28, 0, 8,
    20, 28, 0, 8, 20, 28, 0, 8, 20, 28, 0, 8, 20, 28, 0, 8,
    20, 28, 0, 8, 20, 28, 0, 8, 20, 28, 0, 8, 20, 28, 0, 8,
    20, 28, 0, 8, 20, 28, 0, 8, 4, 12, 0, 8, 4, 12, 0, 8,
    20, 28, 0, 8, 20, 28, 0, 8, 4, 12, 0, 8, 4, 12, 0, 8,
    4, 12, 0, 8, 4, 12, 0, 8, 4, 12, 0, 8, 4, 12, 0, 8,
};
void test_open_flags() {
  static_assert(DG_OPEN_NO_KMER_TABLE == 2 && DG_OPEN_COMPACT == 4 && DG_OPEN_BIG_TABLE == 8 && DG_OPEN_NO_PRE5 == 16, "the table is in these bits");
  const long long sizes[6] = {1ll << 20, (1ll << 20) + 1, 1ll << 30, (1ll << 30) + 1, 8ll << 30, (8ll << 30) + 1};
  size_t at = 0;
  for (int is_file = 0; is_file < 2; ++is_file)
    for (long long size : sizes)
      for (uint32_t distance = 1; distance <= 2; ++distance)
        for (int e = 0; e < 8; ++e, ++at) {
          const uint32_t got = hunt::hunt_open_flags(is_file != 0, size, distance, hunt::OpenEnv{(e & 1) != 0, (e & 2) != 0, (e & 4) != 0});
          check(got == kOpenFlags[at], "open flags, entry " + std::to_string(at) + ": " + std::to_string(got) + ", the table " + std::to_string(kOpenFlags[at]));
        }
  check(at == 192, "table length");
}

}  // namespace

int main(int argc, char** argv) {
  g_dir = argc > 1 ? argv[1] : "/tmp";
  test_read_queries();
  test_rank_plan();
  test_pack_chunk();
  test_block_as_result();
  test_open_flags();
  std::printf("ok %zu files, %zu records, %zu joined sequences\n", g_files, g_records, g_joined);
  return 0;
}
