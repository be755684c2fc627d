// `dicey hunt` (reference src/hunter.h:177-447) over the C ABI of libdiceygpu.so: the command line and the JSON of the reference.
// hunter() at the bottom reads as the stages above it, top to bottom; the stages that need neither the GPU nor the library are in
// hunt_stages.hpp and are tested as a host program of their own.
//
// Host-side work that must stay on the host for bit-identical output: the hit vector arrives in the
// reference's push order and is sorted with libstdc++ std::sort under the reference's comparator (hunter.h:63-65,440).
#include <dlfcn.h>
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <functional>
#include <iostream>
#include <memory>
#include <mutex>
#include <thread>

#include "../../include/dicey_gather.h"
#include "cli_common.hpp"
#include "hunt_stages.hpp"

namespace {

using hunt::Query;

struct DnaHit {  // hunter.h:53-66
  int32_t score;
  uint32_t chr, start;
  char strand;
  std::string refalign, queryalign;
  bool operator<(const DnaHit& b) const {
    return ((score > b.score) || ((score == b.score) && (chr < b.chr)) || ((score == b.score) && (chr == b.chr) && (start < b.start)));
  }
};

struct Config {
  std::string genome, outfile, input;
  bool has_outfile = false, hamming = false, forward = false, help = false;
  uint64_t max_locations = 1000;
  uint32_t max_neighborhood = 10000, distance = 1;
};

// a finished JSON line of query i; a buffer of finished lines in query order (stdout only)
using LineSink = std::function<void(size_t, std::string&&)>;
using BulkSink = std::function<void(std::string&&)>;

struct ResultFree {
  void operator()(dg_hunt_result* r) const { dg_hunt_result_free(r); }
};
using ResultPtr = std::unique_ptr<dg_hunt_result, ResultFree>;

void timing_line(const char* what, double t0) {
  if (timing_on()) std::fprintf(stderr, "dicey timing: %-28s %8.1f ms\n", what, now_ms() - t0);
}

// hunter.h:99-160 (r04: appended in place — at 10 M queries per run the temporaries of the first form were the run time)
void hunt_json_append(std::string& o, const Config& c, uint32_t distance, std::string_view sequence, std::string_view qname,
                      const std::vector<std::string>& seqname, const std::vector<DnaHit>& ht, const std::vector<std::string>& msg) {
  o += "{\"errors\": [";
  bool errors = false;
  for (size_t i = 0; i < msg.size(); ++i) {
    bool err = msg[i].compare(0, 5, "Error") == 0;
    errors = errors || err;
    if (i) o.push_back(',');
    o += "{\"title\":";
    jstr_append(o, msg[i]);
    o += ",\"type\":";
    o += err ? "\"error\"" : "\"warning\"";
    o.push_back('}');
  }
  o.push_back(']');
  if (!errors) {
    o += ",\"meta\":{\"distance\":";
    uint_append(o, distance);
    o += ",\"forwardonly\":";
    o += c.forward ? "true" : "false";
    o += ",\"genome\":";
    jstr_append(o, c.genome);
    o += ",\"hamming\":";
    o += c.hamming ? "true" : "false";
    o += ",\"maxmatches\":";
    uint_append(o, c.max_locations);
    if (!qname.empty()) {
      o += ",\"name\":";
      jstr_append(o, qname.data(), qname.size());
    }
    o += ",\"outfile\":";
    jstr_append(o, c.outfile);
    o += ",\"sequence\":";
    jstr_append(o, sequence.data(), sequence.size());
    o += ",\"subcommand\":\"hunt\",\"version\":\"";
    o += kVersion;
    o += "\"},\"data\":[";
    uint32_t oldchr = 999999, oldstart = 0;
    bool first = true;
    for (const DnaHit& h : ht) {
      if (oldchr != h.chr || oldstart != h.start) {
        if (!first) o.push_back(',');
        first = false;
        uint32_t nuc = 0;
        for (char ch : h.refalign) nuc += ch != '-';
        o += "{\"chr\":";
        jstr_append(o, seqname[h.chr]);
        o += ",\"distance\":";
        uint_append(o, (uint64_t)std::abs(h.score));
        o += ",\"end\":";
        uint_append(o, (uint32_t)(h.start + nuc - 1));
        o += ",\"queryalign\":";
        jstr_append(o, h.queryalign);
        o += ",\"refalign\":";
        jstr_append(o, h.refalign);
        o += ",\"start\":";
        uint_append(o, h.start);
        o += ",\"strand\":\"";
        o.push_back(h.strand);
        o += "\"}";
      }
      oldchr = h.chr;
      oldstart = h.start;
    }
    o.push_back(']');
  }
  o += "}\n";
}
std::string hunt_json(const Config& c, uint32_t distance, std::string_view sequence, std::string_view qname,
                      const std::vector<std::string>& seqname, const std::vector<DnaHit>& ht, const std::vector<std::string>& msg) {
  std::string o;
  hunt_json_append(o, c, distance, sequence, qname, seqname, ht, msg);
  return o;
}

void emit(const Config& c, const std::string& json) {
  if (c.has_outfile) append_gzip_member(c.outfile, json);
  else {
    std::fwrite(json.data(), 1, json.size(), stdout);
    std::fflush(stdout);  // std::endl in the reference
  }
}

// a run that ends before any query is answered: the error JSON on the output, exit status 1
int fail_json(const Config& c, const std::vector<std::string>& seqname, const char* message) {
  emit(c, hunt_json(c, c.distance, c.input, "", seqname, {}, {message}));
  return 1;
}

// ------------------------------------------------------------------------------------------------ options
const OptSpec kHuntOpts[] = {{"help", '?', false}, {"genome", 'g', true}, {"outfile", 'o', true}, {"maxmatches", 'm', true},
                             {"maxNeighborhood", 'x', true}, {"distance", 'd', true}, {"hamming", 'n', false}, {"forward", 'f', false},
                             {"input-file", 0, true}};
void hunt_usage(const char* sub) {
  std::cout << "Usage: dicey " << sub << " [OPTIONS] -g Danio_rerio.fa.gz CATTACTAACATCAGT" << std::endl;
  std::cout << "       dicey " << sub << " [OPTIONS] -g Danio_rerio.fa.gz sequences.fasta" << std::endl;
  std::cout << "Generic options:\n"
               "  -? [ --help ]                      show help message\n"
               "  -g [ --genome ] arg                genome file\n"
               "  -o [ --outfile ] arg               gzipped output file\n"
               "  -m [ --maxmatches ] arg (=1000)    max. number of matches\n"
               "  -x [ --maxNeighborhood ] arg (=10000)\n"
               "                                     max. neighborhood size\n"
               "  -d [ --distance ] arg (=1)         neighborhood distance\n"
               "  -n [ --hamming ]                   use hamming neighborhood instead of edit \n"
               "                                     distance\n"
               "  -f [ --forward ]                   only forward matches\n"
               "\n";
}
// false: the usage text is due (help asked for, or no genome or no input)
bool parse_hunt_options(int argc, char** argv, Config& c) {
  Parsed p = parse_options(argc, argv, kHuntOpts, sizeof kHuntOpts / sizeof kHuntOpts[0]);
  if (!p.error.empty()) {  // program_options throws; the reference does not catch -> terminate
    std::cerr << "terminate called after throwing an instance of 'boost::program_options::error'\n  what():  " << p.error << std::endl;
    std::abort();
  }
  bool have_genome = false, have_input = false;
  for (auto& kv : p.kv) {
    const std::string& k = kv.first;
    if (k == "help") c.help = true;
    else if (k == "genome") { c.genome = kv.second; have_genome = true; }
    else if (k == "outfile") { c.outfile = kv.second; c.has_outfile = true; }
    else if (k == "maxmatches") c.max_locations = std::strtoull(kv.second.c_str(), nullptr, 10);
    else if (k == "maxNeighborhood") c.max_neighborhood = (uint32_t)std::strtoul(kv.second.c_str(), nullptr, 10);
    else if (k == "distance") c.distance = (uint32_t)std::strtoul(kv.second.c_str(), nullptr, 10);
    else if (k == "hamming") c.hamming = true;
    else if (k == "forward") c.forward = true;
    else if (k == "input-file") { c.input = kv.second; have_input = true; }
  }
  if (!p.positional.empty()) {
    c.input = p.positional.back();
    have_input = true;
  }
  return !c.help && have_input && have_genome;
}

// DICEY_DEVICES=0,1,2,...: the GPUs a batch is sharded over (a device may be listed more than once: one replica each)
std::vector<int> devices_from_env() {
  std::vector<int> out;
  if (const char* e = std::getenv("DICEY_DEVICES")) {
    std::string tok;
    for (const char* q = e;; ++q) {
      if (*q == ',' || *q == 0) {
        if (!tok.empty()) out.push_back(std::atoi(tok.c_str()));
        tok.clear();
        if (!*q) break;
      } else tok.push_back(*q);
    }
  }
  if (out.empty()) out.push_back(device_from_env());
  return out;
}

// stdout behind a writer thread (r06): the formatting threads of chunk k + 1 work while chunk k's buffers are written, in order.
// A 10 M-query run writes 5.2 GB of JSON; one write() stream into a file runs at ~2.8 GB/s (page allocation + copy), which was
// spent AFTER each chunk's formatting.  (Measured and dropped: the formatting threads copying their lines into a shared mapping of
// the file — page faults of a mapping are slower than write() and do not scale — and parallel pwrite(), which serialises on the
// inode: 1.7 / 3.1 against 2.8 GB/s on 8 cores.)  At most 512 MB wait in the queue.
class AsyncWriter {
 public:
  ~AsyncWriter() { finish(); }
  void push(std::string&& blob) {
    if (blob.empty()) return;
    std::unique_lock<std::mutex> lk(mu_);
    if (!th_.joinable()) th_ = std::thread([this] { run(); });
    cv_room_.wait(lk, [this] { return queued_ < kMax; });
    queued_ += blob.size();
    q_.push_back(std::move(blob));
    cv_work_.notify_one();
  }
  void finish() {  // everything handed over so far is on stdout when this returns
    {
      std::unique_lock<std::mutex> lk(mu_);
      done_ = true;
      cv_work_.notify_one();
    }
    if (th_.joinable()) th_.join();
    std::unique_lock<std::mutex> lk(mu_);
    done_ = false;
    std::fflush(stdout);
  }

 private:
  void run() {
    for (;;) {
      std::string blob;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_work_.wait(lk, [this] { return done_ || !q_.empty(); });
        if (q_.empty()) return;
        blob = std::move(q_.front());
        q_.pop_front();
      }
      std::fwrite(blob.data(), 1, blob.size(), stdout);
      {
        std::unique_lock<std::mutex> lk(mu_);
        queued_ -= blob.size();
        cv_room_.notify_all();
      }
    }
  }
  static constexpr size_t kMax = 512u << 20;
  std::mutex mu_;
  std::condition_variable cv_work_, cv_room_;
  std::deque<std::string> q_;
  size_t queued_ = 0;
  bool done_ = false;
  std::thread th_;
};

// ------------------------------------------------------------------------------------------------ a finished chunk as JSON lines
struct HuntFormatter {
  const Config& c;
  const std::vector<Query>& queries;
  const std::vector<std::string>& seqname;

  // the line of query q0 + i, query i of the result
  std::string line_of(const dg_hunt_result* R, size_t q0, size_t i) const {
    std::vector<std::string> m;
    std::vector<DnaHit> ht;
    const std::string_view qname = queries[q0 + i].first;
    // compact results (DG_HUNT_COMPACT): one word per query; the normalised sequence is formed here from the query's own bytes
    const uint32_t qw = R->qinfo[i], qfl = DG_QINFO_FLAGS(qw);
    if (qfl & DG_Q_TOO_SHORT) {
      m.push_back("Error: Input sequence is shorter than 10 nucleotides!");
      return hunt_json(c, c.distance, queries[q0 + i].second, qname, seqname, ht, m);
    }
    const std::string_view raw = queries[q0 + i].second;
    std::string seq(raw.size(), '\0');
    uint32_t nondna = 0;
    (void)dg_normalize_query((const uint8_t*)raw.data(), (uint32_t)raw.size(), (uint8_t*)seq.data(), &nondna);
    for (uint32_t k = 0; k < nondna; ++k) m.push_back("Warning: Non-DNA character in nucleotide sequence detected and replaced by 'N'!");
    if (qfl & DG_Q_DIST_ADJUSTED) m.push_back("Warning: Distance was adjusted to sequence length!");
    if (qfl & DG_Q_NBHD_EXCEEDED) {
      std::string x = std::to_string(c.max_neighborhood);
      m.push_back("Warning: Neighborhood size exceeds " + x + " candidates. Only first " + x + " neighbors are searched, results are likely incomplete!");
    }
    for (uint64_t h = R->hit_off[i]; h < R->hit_off[i + 1]; ++h) {
      // the hit from its compact record (dicey_gpu.h ABI 5: position, packed word, operation words) and its two rows from the
      // operation words — built here, on the formatting threads
      dg_hit H;
      const uint32_t* hops = nullptr;
      if (dg_chit_unpack(R, h, (uint32_t)i, &H, &hops) != DG_OK) {
        std::fprintf(stderr, "dicey hunt: %s\n", dg_last_error());
        std::abort();
      }
      std::string ra(H.aln_len, '\0'), qa(H.aln_len, '\0');
      if (dg_hit_rows(&H, hops, R->ops_per_hit, (const uint8_t*)seq.data(), (uint32_t)seq.size(), ra.data(), qa.data()) != DG_OK) {
        std::fprintf(stderr, "dicey hunt: %s\n", dg_last_error());
        std::abort();
      }
      ht.push_back(DnaHit{H.score, H.chr, H.start, (char)H.strand, std::move(ra), std::move(qa)});
    }
    if (qfl & DG_Q_MAX_MATCHES) {
      std::string x = std::to_string(c.max_locations);
      m.push_back("Warning: More than " + x + " matches found. Only first " + x + " matches are reported, results are likely incomplete!");
    }
    std::sort(ht.begin(), ht.end());  // hunter.h:440 — same comparator, same libstdc++ algorithm, same input order
    return hunt_json(c, DG_QINFO_DISTANCE(qw), seq, qname, seqname, ht, m);
  }

  static unsigned threads_for(size_t nq) {
    unsigned nthr = std::thread::hardware_concurrency();
    if (const char* e = std::getenv("DICEY_HOST_THREADS")) nthr = (unsigned)std::max(1, std::atoi(e));
    nthr = (unsigned)std::min<size_t>(std::min<unsigned>(nthr ? nthr : 1u, 64u), nq / 32);
    return nthr < 1 ? 1 : nthr;
  }

  // one JSON line per query of a finished chunk (queries q0 .. q0 + nq), handed to the sink in query order
  void format_chunk(const dg_hunt_result* R, size_t q0, size_t nq, const LineSink& sink, const BulkSink& bulk) const {
    const unsigned nthr = threads_for(nq);
    const size_t per_thr = (nq + nthr - 1) / nthr;
    if (bulk) {
      // stdout: every formatting thread appends its lines to one buffer, the buffers go out in order with one write each (the
      // reference flushes after every line; the bytes are the same)
      std::vector<std::string> blobs(nthr);
      auto work = [&](unsigned t) {
        std::string& o = blobs[t];
        const size_t i0 = t * per_thr, i1 = std::min(nq, i0 + per_thr);
        static std::atomic<size_t> per_line{700};  // bytes per line of the last buffer formatted (distance 2: ~8 KB): the next one is sized for it
        o.reserve((i1 > i0 ? i1 - i0 : 0) * per_line.load(std::memory_order_relaxed));
        for (size_t i = i0; i < i1; ++i) o += line_of(R, q0, i);
        if (i1 > i0 + 16) per_line.store(o.size() / (i1 - i0) + o.size() / (i1 - i0) / 8 + 64, std::memory_order_relaxed);
      };
      if (nthr > 1) {
        std::vector<std::thread> fmt;
        for (unsigned t = 0; t < nthr; ++t) fmt.emplace_back(work, t);
        for (auto& th : fmt) th.join();
      } else work(0);
      for (std::string& o : blobs) bulk(std::move(o));  // (the writer thread's queue: the next chunk is formatted while these go out)
      return;
    }
    if (nthr > 1) {
      std::vector<std::string> lines(nq);
      std::vector<std::thread> fmt;
      for (unsigned t = 0; t < nthr; ++t)
        fmt.emplace_back([&, t]() {
          for (size_t i = t * per_thr, e = std::min(nq, i + per_thr); i < e; ++i) lines[i] = line_of(R, q0, i);
        });
      for (auto& th : fmt) th.join();
      for (size_t i = 0; i < nq; ++i) sink(q0 + i, std::move(lines[i]));
    } else {
      for (size_t i = 0; i < nq; ++i) sink(q0 + i, line_of(R, q0, i));
    }
  }
};

// what every driver needs to search and format: the input, the genome's sequences, the run's parameters
struct HuntJob {
  const Config& c;
  const std::vector<Query>& queries;
  const std::vector<uint32_t>& seqlen;
  const dg_hunt_params& hp;
  const HuntFormatter& fmt;
};

// ------------------------------------------------------------------------------------------------ a range of queries on one handle
// queries [s0, s1) on one handle, chunk by chunk; sink(i, json line of query i) is called in query order
struct SliceRunner {
  const HuntJob& job;
  dg_index* ix;
  const LineSink& sink;
  const BulkSink& bulk;
  std::string err;
  using Chunk = std::pair<size_t, size_t>;

  void format(const dg_hunt_result* R, const Chunk& ch) const { job.fmt.format_chunk(R, ch.first, ch.second - ch.first, sink, bulk); }

  // a chunk through the blocking call; a chunk whose capped neighbourhoods would not fit the library's host budget (DG_ELIMIT,
  // hunt.hip cap_scan: long primers at distance 2) is answered in halves — the reference answers that input too, slowly
  bool run_sync(dg_index* hx, size_t q0, size_t q1) {
    const hunt::ChunkPack p = hunt::pack_chunk(job.queries, q0, q1, job.hp);
    dg_hunt_result* raw = nullptr;
    const int rc = dg_hunt(hx, &p.params, job.seqlen.data(), (uint32_t)job.seqlen.size(), (const uint8_t*)p.bytes.data(), p.off.data(), q1 - q0, &raw);
    const ResultPtr R(raw);
    if (rc == DG_ELIMIT && q1 - q0 > 1) {
      const size_t mid = q0 + (q1 - q0) / 2;
      return run_sync(hx, q0, mid) && run_sync(hx, mid, q1);
    }
    if (rc != DG_OK) {
      err = dg_last_error();  // outside the supported envelope: say so, never guess
      return false;
    }
    format(R.get(), Chunk(q0, q1));
    return true;
  }

  bool submit(dg_index* lane, const Chunk& ch, dg_hunt_ticket** ticket) {
    const hunt::ChunkPack p = hunt::pack_chunk(job.queries, ch.first, ch.second, job.hp);
    if (dg_hunt_submit(lane, &p.params, job.seqlen.data(), (uint32_t)job.seqlen.size(), (const uint8_t*)p.bytes.data(), p.off.data(),
                       ch.second - ch.first, ticket) != DG_OK) {
      err = dg_last_error();
      return false;
    }
    return true;
  }

  // Large inputs go chunk by chunk with TWO batches in flight (dg_hunt_submit / dg_hunt_wait on this handle and on a second
  // one that shares the resident index): while the host formats the lines of chunk k, chunk k+1 is on the GPU.
  bool run_pipelined(const std::vector<Chunk>& chunks) {
    dg_index* second = nullptr;
    if (dg_index_share(ix, &second) != DG_OK) second = nullptr;
    dg_index* lanes[2] = {ix, second ? second : ix};
    const size_t depth = second ? 2 : 1;
    std::vector<dg_hunt_ticket*> tickets(chunks.size(), nullptr);
    bool ok = true;
    // Invariant: chunk k runs on lane k % depth, and while everything is fine chunk k + depth is submitted as soon as chunk k's
    // lane is idle again — right after its wait() when the chunk was answered (the next one is on the GPU while this one is
    // formatted), or after the blocking halves when the library refused the chunk's size (DG_ELIMIT: the lane must be idle for
    // run_sync).  A missing ticket while `ok` holds is a bug of this loop and ends the run with an error, never with silence.
    size_t submitted = 0;
    auto top_up = [&]() {
      if (ok && submitted < chunks.size()) {
        ok = submit(lanes[submitted % depth], chunks[submitted], &tickets[submitted]);
        if (ok) ++submitted;
      }
    };
    for (; submitted < std::min(depth, chunks.size()) && ok;) top_up();
    for (size_t k = 0; k < chunks.size(); ++k) {
      if (!tickets[k]) {
        if (ok) {
          err = "internal error: chunk " + std::to_string(k) + " of " + std::to_string(chunks.size()) + " was never submitted";
          ok = false;
        }
        continue;
      }
      dg_hunt_result* raw = nullptr;
      const int rc = dg_hunt_wait(tickets[k], &raw);
      ResultPtr R(raw);
      tickets[k] = nullptr;
      if (!ok) continue;  // keep collecting what is in flight
      if (rc == DG_OK) {
        top_up();  // the lane is free again: the next chunk starts before this one is formatted
        format(R.get(), chunks[k]);
      } else if (rc == DG_ELIMIT) {
        R.reset();
        ok = run_sync(lanes[k % depth], chunks[k].first, chunks[k].second);  // that lane is idle: its wait() has returned and nothing new was submitted to it
        top_up();
      } else {
        err = dg_last_error();
        ok = false;
      }
    }
    if (second) dg_index_close(second);
    return ok;
  }

  // (distance >= 2: a query's line is ~8 KB on a 3 Gb genome — 131 072 of them are a gigabyte, twice what the writer's queue takes,
  //  and the formatting threads stood still while it drained; 16 384 keep both sides busy: 1 M queries 4.1 -> see DESIGN §9)
  bool run(size_t s0, size_t s1) {
    const size_t CHUNK = job.c.distance >= 2 ? (1u << 14) : (s1 - s0) > (1u << 18) ? (1u << 17) : (1u << 20);
    std::vector<Chunk> chunks;
    for (size_t q0 = s0; q0 < s1; q0 += CHUNK) chunks.emplace_back(q0, std::min(s1, q0 + CHUNK));
    if (chunks.size() >= 2 && !std::getenv("DICEY_NO_PIPELINE")) return run_pipelined(chunks);
    for (auto& ch : chunks)
      if (!run_sync(ix, ch.first, ch.second)) return false;
    return true;
  }
};

// ---------------------------------------------------------------------------- one process per GPU (DICEY_RANKS)
// libdiceygather.so is loaded only in this mode (it brings RCCL into the process): next to the binary, like libdiceygpu.so.
struct GatherApi {
  void* so = nullptr;
  int (*unique_id)(uint8_t*) = nullptr;
  int (*open)(const uint8_t*, int, int, int, uint64_t, int, dg_comm**) = nullptr;
  int (*open_tcp)(int, int, int, uint64_t, int, dg_comm**) = nullptr;
  int (*close)(dg_comm*) = nullptr;
  int (*submit)(dg_comm*, void*, const void*, uint64_t) = nullptr;
  int (*finish)(dg_comm*, uint64_t*, uint64_t*) = nullptr;
  int (*last_to_host)(dg_comm*, int, void*, uint64_t, uint64_t*) = nullptr;
  int (*max_u64)(dg_comm*, uint64_t, uint64_t*) = nullptr;
  const char* (*last_error)() = nullptr;
  bool load(std::string& err) {
    char exe[4096];
    const ssize_t n = readlink("/proc/self/exe", exe, sizeof exe - 1);
    std::string dir = n > 0 ? std::string(exe, (size_t)n) : std::string("./dicey");
    dir = dir.substr(0, dir.find_last_of('/') + 1);
    so = dlopen((dir + "libdiceygather.so").c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!so) {
      err = std::string("libdiceygather.so: ") + dlerror();
      return false;
    }
#define DG_SYM(field, name)                                     \
    field = reinterpret_cast<decltype(field)>(dlsym(so, name)); \
    if (!field) {                                               \
      err = std::string("libdiceygather.so lacks ") + name;     \
      return false;                                             \
    }
    DG_SYM(unique_id, "dg_comm_unique_id")
    DG_SYM(open, "dg_comm_open")
    DG_SYM(open_tcp, "dg_comm_open_tcp")
    DG_SYM(close, "dg_comm_close")
    DG_SYM(submit, "dg_gather_submit")
    DG_SYM(finish, "dg_gather_finish")
    DG_SYM(last_to_host, "dg_gather_last_to_host")
    DG_SYM(max_u64, "dg_comm_max_u64")
    DG_SYM(last_error, "dg_gather_last_error")
#undef DG_SYM
    return true;
  }
};

constexpr uint64_t kGatherCap = 64ull << 20;  // bytes per transfer; a chunk's block travels in as many pieces as the largest rank's needs

struct RankDie {  // a rank's message on stderr; the exit status of a rank that cannot go on
  int rank, N;
  int operator()(const std::string& m) const {
    std::cerr << "dicey (rank " << rank << " of " << N << "): " << m << std::endl;
    return 2;
  }
};

// The communicator id of this launch through DICEY_COMM_FILE.  The file holds the id followed by a 16-byte launch token
// (DICEY_COMM_TOKEN, zero-padded; empty = all zero): a file another launch left behind does not carry this launch's token and is not
// taken.  Rank 0 removes whatever lies at the path before it writes, and removes its own file once the communicator stands.
int exchange_comm_id(const GatherApi& G, const RankDie& die, const char* cf, uint8_t* id) {
  uint8_t token[16] = {0};
  if (const char* tk = std::getenv("DICEY_COMM_TOKEN")) std::memcpy(token, tk, std::min<size_t>(std::strlen(tk), sizeof token));
  if (die.N > 1 && !cf) return die("DICEY_COMM_FILE (where rank 0 leaves the communicator id) is not set");
  if (die.rank == 0) {
    if (cf) std::remove(cf);
    if (G.unique_id(id) != 0) return die(G.last_error());
    if (cf) {
      const std::string tmp = std::string(cf) + ".tmp";
      FILE* f = std::fopen(tmp.c_str(), "wb");
      if (!f || std::fwrite(id, 1, DG_COMM_ID_BYTES, f) != DG_COMM_ID_BYTES || std::fwrite(token, 1, sizeof token, f) != sizeof token)
        return die("cannot write " + tmp);
      std::fclose(f);
      if (std::rename(tmp.c_str(), cf) != 0) return die(std::string("cannot create ") + cf);
    }
    return 0;
  }
  bool got = false;
  for (int attempt = 0; attempt < 1200 && !got; ++attempt) {  // the ranks start together; rank 0 writes within milliseconds
    if (FILE* f = std::fopen(cf, "rb")) {
      uint8_t tk[sizeof token];
      got = std::fread(id, 1, DG_COMM_ID_BYTES, f) == DG_COMM_ID_BYTES && std::fread(tk, 1, sizeof tk, f) == sizeof tk &&
            std::memcmp(tk, token, sizeof tk) == 0;
      std::fclose(f);
    }
    if (!got) std::this_thread::sleep_for(std::chrono::milliseconds(50));
  }
  return got ? 0 : die(std::string("no communicator id of this launch in ") + cf);
}

// DICEY_COMM_TCP=<port>: the library's host-memory test transport (two ranks on the one GPU of a test box; RCCL does not
// take two ranks on one device).  The product form is RCCL: rank 0 writes the communicator id to DICEY_COMM_FILE.
int open_comm(const GatherApi& G, const RankDie& die, int device, dg_comm** comm) {
  if (const char* tcp = std::getenv("DICEY_COMM_TCP"))
    return G.open_tcp(std::atoi(tcp), die.N, die.rank, kGatherCap, 0, comm) != 0 ? die(G.last_error()) : 0;
  const char* cf = std::getenv("DICEY_COMM_FILE");
  uint8_t id[DG_COMM_ID_BYTES];
  if (const int rc = exchange_comm_id(G, die, cf, id)) return rc;
  // RCCL greets with a version banner on stdout (rank 0, communicator creation); stdout is the JSON stream (hunter.h:160-175), so
  // the banner goes to stderr: file descriptor 1 points there while the communicator is created
  std::fflush(stdout);
  const int saved_out = dup(1);
  if (saved_out >= 0) dup2(2, 1);
  const int orc = G.open(id, die.N, die.rank, device, kGatherCap, 0, comm);
  std::fflush(stdout);
  if (saved_out >= 0) {
    dup2(saved_out, 1);
    close(saved_out);
  }
  if (orc != 0) return die(G.last_error());
  if (die.rank == 0 && cf) std::remove(cf);  // the communicator stands: every rank has read the id
  return 0;
}

// Rank 0 keeps every (rank, chunk, piece) block on the host until everything has arrived, then formats in query order.
// A chunk normally is ONE piece.  When a rank's library refuses its chunk's size (DG_ELIMIT: capped neighbourhoods beyond the
// host budget — what SliceRunner::run_sync answers by halves) the ranks agree, through the collective that carries the byte counts,
// to cut the chunk into twice as many equal pieces ON EVERY RANK and start it again: the split is a function of (range, pieces)
// alone, so rank 0 can rebuild every rank's pieces and the collectives stay in step.  Any other failure travels the same way
// and ends every rank (one rank leaving alone left its peers blocked in the next collective).
struct RankGather {
  const HuntJob& job;
  const GatherApi& G;
  const RankDie& die;
  dg_comm* comm;
  dg_index* ix;
  const bool tcp;
  const hunt::RankPlan plan;
  std::vector<std::vector<std::vector<std::vector<uint8_t>>>> got;  // [rank][chunk][piece], on rank 0
  std::vector<uint64_t> parts_of;
  static constexpr uint64_t ST_SHIFT = 60, ST_SPLIT = 1, ST_FAIL = 2;
  enum Step { NEXT, SPLIT, LEAVE };

  RankGather(const HuntJob& job_, const GatherApi& G_, const RankDie& die_, dg_comm* comm_, dg_index* ix_)
      : job(job_), G(G_), die(die_), comm(comm_), ix(ix_), tcp(std::getenv("DICEY_COMM_TCP") != nullptr), plan(job_.queries.size(), die_.N),
        got(die_.rank == 0 ? die_.N : 0, std::vector<std::vector<std::vector<uint8_t>>>(plan.nchunks)), parts_of(plan.nchunks, 1) {}

  // this rank's block of `bytes` bytes and every peer's, in transfers of at most kGatherCap; rank 0 appends what arrived to got[r][k][piece]
  int transfer(const dg_hunt_result* R, size_t n, uint64_t bytes, uint64_t most, size_t k, uint64_t piece) {
    const uint64_t pieces = std::max<uint64_t>(1, (most + kGatherCap - 1) / kGatherCap);
    for (uint64_t pc = 0; pc < pieces; ++pc) {
      const uint64_t b0 = std::min(bytes, pc * kGatherCap), b1 = std::min(bytes, b0 + kGatherCap);
      // RCCL: out of HBM, staged on the stream the batch ran on; the TCP test transport takes the fetched copy of the same bytes
      const uint8_t* src = !R ? nullptr : tcp ? (const uint8_t*)R->qinfo - 4 * n : (const uint8_t*)R->d_block;
      if (G.submit(comm, (R && !tcp) ? R->stream : nullptr, src ? src + b0 : nullptr, b1 - b0) != 0) return die(G.last_error());
      if (G.finish(comm, nullptr, nullptr) != 0) return die(G.last_error());
      if (die.rank == 0)
        for (int r = 0; r < die.N; ++r) {
          uint64_t got_n = 0;
          if (G.last_to_host(comm, r, nullptr, 0, &got_n) != 0 && got_n == 0) return die(G.last_error());
          std::vector<uint8_t>& dst = got[r][k][piece];
          const size_t at = dst.size();
          dst.resize(at + got_n);
          if (got_n && G.last_to_host(comm, r, dst.data() + at, got_n, &got_n) != 0) return die(G.last_error());
        }
    }
    return 0;
  }

  // queries [a, b) of chunk k: search, agree with the peers on split / fail through max_u64, gather.  rc is the exit status on LEAVE.
  Step gather_piece(size_t k, uint64_t piece, size_t a, size_t b, int& rc) {
    ResultPtr R;
    uint64_t status = 0;
    if (b > a) {
      const hunt::ChunkPack p = hunt::pack_chunk(job.queries, a, b, job.hp);
      dg_hunt_result* raw = nullptr;
      const int hrc = dg_hunt(ix, &p.params, job.seqlen.data(), (uint32_t)job.seqlen.size(), (const uint8_t*)p.bytes.data(), p.off.data(), b - a, &raw);
      if (hrc == DG_ELIMIT && b - a > 1) status = ST_SPLIT;
      else if (hrc != DG_OK) {
        die(dg_last_error());  // outside the supported envelope: the whole job fails, never a partial answer
        status = ST_FAIL;
      }
      if (hrc == DG_OK) R.reset(raw);
    }
    const uint64_t bytes = R ? R->d_block_bytes : 0;
    uint64_t most = 0;
    rc = 0;
    if (G.max_u64(comm, (status << ST_SHIFT) | bytes, &most) != 0) rc = die(G.last_error());
    else if ((most >> ST_SHIFT) >= ST_FAIL) {  // some rank cannot answer: every rank leaves, none waits for a peer that is gone
      R.reset();
      G.close(comm);
      rc = status == ST_FAIL ? 2 : die("another rank failed; no output");
    } else if ((most >> ST_SHIFT) == ST_SPLIT) return SPLIT;
    else rc = transfer(R.get(), b - a, bytes, most, k, piece);
    return rc ? LEAVE : NEXT;
  }

  int gather_chunk(size_t k) {
    size_t q0, q1;
    plan.range_of(die.rank, k, q0, q1);
    for (uint64_t parts = 1;; parts *= 2) {
      Step s = NEXT;
      if (die.rank == 0)
        for (int r = 0; r < die.N; ++r) got[r][k].assign(parts, std::vector<uint8_t>());
      for (uint64_t piece = 0; piece < parts && s == NEXT; ++piece) {
        size_t a, b;
        int rc = 0;
        hunt::RankPlan::piece_of(q0, q1, parts, piece, a, b);
        s = gather_piece(k, piece, a, b, rc);
        if (s == LEAVE) return rc;
      }
      if (s == NEXT) {
        parts_of[k] = parts;
        return 0;
      }
    }
  }

  // rank 0, everything has arrived: every block as a result, formatted and written in query order
  int write_all(const LineSink& sink, const BulkSink& bulk) {
    std::vector<uint64_t> seq_start(job.seqlen.size() + 1, 0), hit_off;
    for (size_t i = 0; i < job.seqlen.size(); ++i) seq_start[i + 1] = seq_start[i] + job.seqlen[i];
    for (int r = 0; r < die.N; ++r)
      for (size_t k = 0; k < plan.nchunks; ++k)
        for (uint64_t piece = 0; piece < parts_of[k]; ++piece) {
          size_t c0, c1, q0, q1;
          plan.range_of(r, k, c0, c1);
          hunt::RankPlan::piece_of(c0, c1, parts_of[k], piece, q0, q1);
          const size_t n = q1 - q0;
          if (!n) continue;
          const std::vector<uint8_t>& blk = got[r][k][piece];
          dg_hunt_result S;
          std::string why;
          if (!hunt::block_as_result(blk.data(), blk.size(), n, r, (uint32_t)job.seqlen.size(), seq_start.data(), S, hit_off, why)) return die(why);
          job.fmt.format_chunk(&S, q0, n, sink, bulk);
        }
    return 0;
  }
};

// ------------------------------------------------------------------------------------------------ the three drivers
// DICEY_RANKS=N DICEY_RANK=r DICEY_COMM_FILE=<path>: ONE PROCESS PER GPU (BASELINE.json north_star: "the primer batch shards
// embarrassingly across the 8 GPUs of one node with RCCL over xGMI only to gather hit lists").  Every rank reads the same input,
// searches its contiguous range of the queries (ceil(nq/N) each, rank order = query order) on its own index replica, and the ranks'
// answers — per chunk the compact block [hit counts | query words | records], dg_hunt_result::d_block, straight out of HBM — are
// gathered to rank 0 by libdiceygather.so (include/dicey_gather.h: exact-size ncclSend / ncclRecv), which formats and writes
// every line in query order.  The reference is one process; what this replaces is the concatenation of the shards' results.
int run_ranks(const HuntJob& job, int N, int rank, dg_index* ix, int device) {
  const RankDie die{rank, N};
  if (rank < 0 || rank >= N) return die("DICEY_RANK outside [0, DICEY_RANKS)");
  GatherApi G;
  std::string err;
  if (!G.load(err)) return die(err);
  dg_comm* comm = nullptr;
  if (const int rc = open_comm(G, die, device, &comm)) return rc;
  RankGather gather(job, G, die, comm, ix);
  for (size_t k = 0; k < gather.plan.nchunks; ++k)
    if (const int rc = gather.gather_chunk(k)) return rc;
  G.close(comm);
  if (rank != 0) return 0;
  const Config& c = job.c;
  BulkSink bulk;
  if (!c.has_outfile)
    bulk = [](std::string&& blob) {
      std::fwrite(blob.data(), 1, blob.size(), stdout);
      std::fflush(stdout);
    };
  return gather.write_all([&c](size_t, std::string&& js) { emit(c, js); }, bulk);
}

// One device (DICEY_DEVICE, default 0): results stream out chunk by chunk.
int run_one_device(const HuntJob& job, dg_index* ix) {
  const Config& c = job.c;
  BulkSink bulk;
  AsyncWriter writer;
  if (!c.has_outfile)  // (the gzip outfile is one member per query, hunter.h:162-170: written line by line)
    bulk = [&](std::string&& blob) { writer.push(std::move(blob)); };
  const LineSink sink = [&c](size_t, std::string&& js) { emit(c, js); };
  const double t_run0 = now_ms();
  SliceRunner slice{job, ix, sink, bulk, {}};
  const bool ran = slice.run(0, job.queries.size());
  writer.finish();
  timing_line("search + format + write", t_run0);
  if (ran) return 0;
  std::cerr << "dicey: " << slice.err << std::endl;
  return 2;
}

// Queries are independent (hunter.h:291), so a batch shards over the GPUs of the node by contiguous ranges (ceil(nq/G) each,
// SURVEY.md 8(e)): DICEY_DEVICES=0,1,... gives one host thread and one full index replica per listed device; results are written
// in query order.
int run_devices(const HuntJob& job, const std::vector<dg_index*>& handles) {
  const size_t G = handles.size(), nq = job.queries.size(), per = (nq + G - 1) / G;
  std::vector<std::string> lines(nq);
  std::vector<std::string> errs(G);
  std::vector<char> ok(G, 1);
  std::vector<std::thread> pool;
  const BulkSink no_bulk;
  for (size_t g = 0; g < G; ++g)
    pool.emplace_back([&, g]() {
      const size_t s0 = std::min(nq, g * per), s1 = std::min(nq, s0 + per);
      const LineSink sink = [&lines](size_t i, std::string&& js) { lines[i] = std::move(js); };
      SliceRunner slice{job, handles[g], sink, no_bulk, {}};
      ok[g] = slice.run(s0, s1);
      errs[g] = std::move(slice.err);
    });
  for (auto& t : pool) t.join();
  for (size_t g = 0; g < G; ++g) {  // query order; stop at the first shard that failed
    const size_t s0 = std::min(nq, g * per), s1 = std::min(nq, s0 + per);
    for (size_t i = s0; i < s1 && !lines[i].empty(); ++i) emit(job.c, lines[i]);
    if (!ok[g]) {
      std::cerr << "dicey: " << errs[g] << std::endl;
      return 2;
    }
  }
  return 0;
}

// one index handle per listed device, opened side by side; every handle is closed by close()
struct Handles {
  std::vector<dg_index*> ix;
  std::vector<std::string> err;
  void open(const std::string& index_file, const std::vector<int>& devices, uint32_t flags) {
    ix.assign(devices.size(), nullptr);
    err.assign(devices.size(), std::string());
    std::vector<std::thread> pool;
    for (size_t g = 0; g < devices.size(); ++g)
      pool.emplace_back([&, g]() {
        if (dg_index_open(index_file.c_str(), devices[g], flags, &ix[g]) != DG_OK) err[g] = dg_last_error();
      });
    for (auto& t : pool) t.join();
  }
  void close() {
    const double t_close0 = now_ms();
    for (dg_index* h : ix)
      if (h) dg_index_close(h);
    timing_line("index close", t_close0);
  }
};

}  // namespace

// ------------------------------------------------------------------------------------------------ hunt (hunter.h:177-447)
int hunter(int argc, char** argv) {
  Config c;
  if (!parse_hunt_options(argc, argv, c)) {
    hunt_usage(argv[0]);
    return -1;
  }
  std::vector<uint32_t> seqlen;
  std::vector<std::string> seqname;
  if (c.has_outfile) {  // hunter.h:232-235
    std::ofstream trunc(c.outfile.c_str(), std::ios_base::out | std::ios_base::binary | std::ios_base::trunc);
  }
  if (!file_nonempty(c.genome)) return fail_json(c, seqname, "Error: Genome does not exist!");
  if (!seq_len_name(c.genome, seqlen, seqname)) return fail_json(c, seqname, "Error: Could not retrieve sequence lengths!");
  const std::string index_file = strip_last_extension(c.genome) + ".fm9";

  // hunter.h:262-287: the queries are read before the index is opened (the shard plan needs the count; a malformed input is still
  // reported after a failing index, as in the reference) — on a thread of its own beside the index open (r06: 0.3 s for a
  // 10 M-record file), joined before anything looks at them
  hunt::QuerySet qs;
  const double t_read0 = now_ms();
  std::thread reader([&]() {
    qs = hunt::read_queries(c.input, is_fasta);
    timing_line("input read + records", t_read0);
  });
  struct Joiner {
    std::thread& t;
    ~Joiner() { if (t.joinable()) t.join(); }
  } reader_joiner{reader};

  struct stat ist;
  const bool is_file = stat(c.input.c_str(), &ist) == 0 && S_ISREG(ist.st_mode);
  const uint32_t open_flags = hunt::hunt_open_flags(is_file, is_file ? (long long)ist.st_size : 0, c.distance,
                                                    {std::getenv("DICEY_FULL_TABLE") != nullptr, std::getenv("DICEY_RESIDENT_LAYOUTS") != nullptr,
                                                     std::getenv("DICEY_KMER_K") != nullptr});
  std::vector<int> devices = devices_from_env();
  const char* ranks = std::getenv("DICEY_RANKS");
  const int rank = std::getenv("DICEY_RANK") ? std::atoi(std::getenv("DICEY_RANK")) : 0;
  if (ranks) devices.assign(1, std::getenv("DICEY_DEVICE") ? device_from_env() : rank);  // one process per GPU: this process's device (DICEY_DEVICE, else its rank)
  if (devices.size() > 1) {  // the shard plan needs the count
    reader.join();
    if (devices.size() > qs.queries.size()) devices.resize(std::max<size_t>(1, qs.queries.size()));
  }
  Handles handles;
  handles.open(index_file, devices, open_flags);
  if (reader.joinable()) reader.join();
  for (size_t g = 0; g < devices.size(); ++g)
    if (!handles.ix[g]) {
      std::cerr << "dicey: " << handles.err[g] << std::endl;
      const int rc = fail_json(c, seqname, "Error: FM-Index cannot be loaded!");
      handles.close();
      return rc;
    }
  if (qs.bad_fasta) {
    const int rc = fail_json(c, seqname, "Error: Input file is not in FASTA format!");
    handles.close();
    return rc;
  }

  dg_hunt_params hp{};
  hp.distance = c.distance;
  hp.hamming = c.hamming;
  hp.forward_only = c.forward;
  hp.max_locations = c.max_locations;
  hp.max_neighborhood = c.max_neighborhood;
  const HuntFormatter fmt{c, qs.queries, seqname};
  const HuntJob job{c, qs.queries, seqlen, hp, fmt};
  if (ranks) {
    const int rc = run_ranks(job, std::max(1, std::atoi(ranks)), rank, handles.ix[0], devices[0]);
    handles.close();
    return rc;
  }
  const int rc = devices.size() == 1 ? run_one_device(job, handles.ix[0]) : run_devices(job, handles.ix);
  if (!quick_exit_on()) handles.close();  // (main leaves with _exit right behind this)
  return rc;
}
