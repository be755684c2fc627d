// `dicey` host binary for the MI355X search path: keeps the command line and the JSON of the reference (src/dicey.cpp:35-76
// dispatch) and calls the HIP kernels through the C ABI of libdiceygpu.so.  Here: the dispatch, `dicey search` and `dicey index`
// (src/index.h:34-141, so that a genome can be prepared without the reference binary); `hunt` (hunt.cpp), `padlock` (padlock.cpp)
// and `mappability` (mappability.cpp) ride on the same library; chop is out of scope.
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <iostream>

#include "../../include/dicey_gpu.h"
#include "cli_common.hpp"
#include "dtoa.hpp"

int hunter(int argc, char** argv);  // hunt.cpp
int padlock_main(int argc, char** argv);  // padlock.cpp
int mappability_main(int argc, char** argv);  // mappability.cpp

namespace {

// ------------------------------------------------------------------------------------------------ search (silica.h:208-651)
struct SearchConfig {
  std::string genome, outfile, infile, primer3Config = "./src/primer3_config/";
  bool has_outfile = false, hamming = false, pruneprimer = false, help = false;
  double cutTemp = 45.0, cutofPen = -1.0, penDiff = 0.6, penMis = 0.4, penLen = 0.001;
  double temp = 37.0, mv = 50.0, dv = 1.5, dna_conc = 50.0, dntp = 0.6;
  uint32_t maxProdSize = 15000, kmer = 15, distance = 1, maxNeighborhood = 10000, maxPruneCount = 0;
  uint64_t max_locations = 10000;
};
struct PrimerBind {  // silica.h:69-82
  uint32_t refIndex, pos, primerId;
  bool onFor;
  double temp, perfTemp;
  std::string genome;
  bool operator<(const PrimerBind& b) const { return (temp > b.temp); }
};
struct PcrProduct {  // silica.h:84-98
  uint32_t refIndex, leng, forPos, revPos, forId, revId;
  double forTemp, revTemp, penalty;
  bool operator<(const PcrProduct& b) const { return (penalty < b.penalty); }
};

// silica.h:100-187; amplicon sequences come from the index text (what faidx_fetch_seq + to_upper would return)
std::string search_json(const SearchConfig& c, dg_index* ix, const std::vector<uint32_t>& seqlen, const std::vector<std::string>& qn,
                        const std::vector<PrimerBind>& allp, const std::vector<PcrProduct>& pcr, const std::vector<std::string>& pName,
                        const std::vector<std::string>& pSeq, const std::vector<std::string>& msg) {
  std::string o = "{\"errors\": [";
  bool errors = false;
  for (size_t i = 0; i < msg.size(); ++i) {
    bool err = msg[i].compare(0, 5, "Error") == 0;
    errors = errors || err;
    if (i) o.push_back(',');
    o += "{\"title\":" + jstr(msg[i]) + ",\"type\":" + (err ? "\"error\"" : "\"warning\"") + "}";
  }
  o.push_back(']');
  if (!errors) {
    o += ",\"meta\":{\"distance\":" + std::to_string(c.distance) + ",\"genome\":" + jstr(c.genome);
    o += std::string(",\"hamming\":") + (c.hamming ? "true" : "false") + ",\"maxmatches\":" + std::to_string(c.max_locations);
    o += ",\"outfile\":" + jstr(c.outfile) + ",\"subcommand\":\"search\",\"version\":\"" + kVersion + "\"},";
    o += "\"data\":{\"primers\":[";
    for (size_t i = 0; i < allp.size(); ++i) {
      const PrimerBind& p = allp[i];
      if (i) o.push_back(',');
      o += "{\"Chrom\":" + jstr(qn[p.refIndex]) + ",\"End\":" + std::to_string((uint64_t)p.pos + pSeq[p.primerId].size());
      o += ",\"Genome\":" + jstr(p.genome) + ",\"Id\":" + std::to_string(i) + ",\"MatchTm\":" + dtoa::dump_double(p.perfTemp);
      o += ",\"Name\":" + jstr(pName[p.primerId]) + ",\"Ori\":" + (p.onFor ? "\"forward\"" : "\"reverse\"");
      o += ",\"Pos\":" + std::to_string(p.pos + 1) + ",\"Seq\":" + jstr(pSeq[p.primerId]) + ",\"Tm\":" + dtoa::dump_double(p.temp) + "}";
    }
    o += "],\"amplicons\":[";
    // amplicon sequences in one extract batch
    std::vector<uint64_t> lo, hi, off;
    uint64_t tot = 0;
    std::vector<char> has(pcr.size(), 0);
    for (size_t i = 0; i < pcr.size(); ++i) {
      const PcrProduct& a = pcr[i];
      uint64_t cstart = 0;
      for (uint32_t r = 0; r < a.refIndex; ++r) cstart += seqlen[r];
      uint64_t clen = seqlen[a.refIndex] - 1, b0 = a.forPos, e0 = (uint64_t)a.revPos + pSeq[a.revId].size() - 1;
      if (b0 < clen) {
        if (e0 >= clen) e0 = clen - 1;
        if (e0 >= b0) {
          has[i] = 1;
          lo.push_back(cstart + b0);
          hi.push_back(cstart + e0);
          off.push_back(tot);
          tot += e0 - b0 + 1;
        }
      }
    }
    std::string pool(tot, '\0');
    if (!lo.empty() && dg_extract(ix, lo.data(), hi.data(), lo.size(), (uint8_t*)&pool[0], off.data()) != DG_OK)
      std::cerr << "dicey: " << dg_last_error() << std::endl;
    size_t k = 0;
    for (size_t i = 0; i < pcr.size(); ++i) {
      const PcrProduct& a = pcr[i];
      std::string seqstr;
      if (has[i]) {
        seqstr = pool.substr(off[k], hi[k] - lo[k] + 1);
        ++k;
      }
      if (i) o.push_back(',');
      o += "{\"Chrom\":" + jstr(qn[a.refIndex]) + ",\"ForEnd\":" + std::to_string((uint64_t)a.forPos + pSeq[a.forId].size());
      o += ",\"ForName\":" + jstr(pName[a.forId]) + ",\"ForPos\":" + std::to_string(a.forPos + 1) + ",\"ForSeq\":" + jstr(pSeq[a.forId]);
      o += ",\"ForTm\":" + dtoa::dump_double(a.forTemp) + ",\"Id\":" + std::to_string(i) + ",\"Length\":" + std::to_string(a.leng);
      o += ",\"Penalty\":" + dtoa::dump_double(a.penalty) + ",\"RevEnd\":" + std::to_string((uint64_t)a.revPos + pSeq[a.revId].size());
      o += ",\"RevName\":" + jstr(pName[a.revId]) + ",\"RevPos\":" + std::to_string(a.revPos + 1) + ",\"RevSeq\":" + jstr(pSeq[a.revId]);
      o += ",\"RevTm\":" + dtoa::dump_double(a.revTemp) + ",\"Seq\":" + jstr(seqstr) + "}";
    }
    o += "]}";
  }
  o += "}\n";
  return o;
}

void emit_search(const SearchConfig& c, const std::string& json) {
  if (c.has_outfile) {  // silica.h:192-198: one gzip stream, file overwritten
    std::ofstream trunc(c.outfile.c_str(), std::ios_base::out | std::ios_base::binary | std::ios_base::trunc);
    trunc.close();
    append_gzip_member(c.outfile, json);
  } else {
    std::fwrite(json.data(), 1, json.size(), stdout);
    std::fflush(stdout);
  }
}

std::string revcomp_upper(std::string s) {  // util.h:110-114
  for (auto& ch : s) {
    char u = (char)std::toupper((unsigned char)ch);
    ch = u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : u == 'U' ? 'A' : u == 'R' ? 'Y' : u == 'Y' ? 'R' : u == 'S' ? 'S'
         : u == 'W' ? 'W' : u == 'K' ? 'M' : u == 'M' ? 'K' : u == 'B' ? 'V' : u == 'V' ? 'B' : u == 'D' ? 'H' : u == 'H' ? 'D' : 'N';
  }
  return std::string(s.rbegin(), s.rend());
}

int silica(int argc, char** argv) {
  SearchConfig c;
  const OptSpec specs[] = {{"help", '?', false}, {"genome", 'g', true}, {"config", 'i', true}, {"outfile", 'o', true}, {"kmer", 'k', true},
                           {"maxmatches", 'm', true}, {"maxNeighborhood", 'x', true}, {"distance", 'd', true}, {"pruneprimer", 'q', true},
                           {"hamming", 'n', false}, {"cutTemp", 'c', true}, {"maxProdSize", 'l', true}, {"cutoffPenalty", 0, true},
                           {"penaltyTmDiff", 0, true}, {"penaltyTmMismatch", 0, true}, {"penaltyLength", 0, true}, {"enttemp", 0, true},
                           {"monovalent", 0, true}, {"divalent", 0, true}, {"dna", 0, true}, {"dntp", 0, true}, {"input-file", 0, true}};
  Parsed p = parse_options(argc, argv, specs, sizeof specs / sizeof specs[0]);
  if (!p.error.empty()) {
    std::cerr << "terminate called after throwing an instance of 'boost::program_options::error'\n  what():  " << p.error << std::endl;
    std::abort();
  }
  bool have_genome = false, have_input = false;
  for (auto& kv : p.kv) {
    const std::string& k = kv.first;
    const char* v = kv.second.c_str();
    if (k == "help") c.help = true;
    else if (k == "genome") { c.genome = v; have_genome = true; }
    else if (k == "config") c.primer3Config = v;
    else if (k == "outfile") { c.outfile = v; c.has_outfile = true; }
    else if (k == "kmer") c.kmer = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "maxmatches") c.max_locations = std::strtoull(v, nullptr, 10);
    else if (k == "maxNeighborhood") c.maxNeighborhood = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "distance") c.distance = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "pruneprimer") { c.maxPruneCount = (uint32_t)std::strtoul(v, nullptr, 10); c.pruneprimer = true; }
    else if (k == "hamming") c.hamming = true;
    else if (k == "cutTemp") c.cutTemp = std::strtod(v, nullptr);
    else if (k == "maxProdSize") c.maxProdSize = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "cutoffPenalty") c.cutofPen = std::strtod(v, nullptr);
    else if (k == "penaltyTmDiff") c.penDiff = std::strtod(v, nullptr);
    else if (k == "penaltyTmMismatch") c.penMis = std::strtod(v, nullptr);
    else if (k == "penaltyLength") c.penLen = std::strtod(v, nullptr);
    else if (k == "enttemp") c.temp = std::strtod(v, nullptr);
    else if (k == "monovalent") c.mv = std::strtod(v, nullptr);
    else if (k == "divalent") c.dv = std::strtod(v, nullptr);
    else if (k == "dna") c.dna_conc = std::strtod(v, nullptr);
    else if (k == "dntp") c.dntp = std::strtod(v, nullptr);
    else if (k == "input-file") { c.infile = v; have_input = true; }
  }
  if (!p.positional.empty()) {
    c.infile = p.positional.back();
    have_input = true;
  }
  if (c.help || !have_input || !have_genome) {
    std::cout << "Usage: dicey " << argv[0] << " [OPTIONS] -g <ref.fa.gz> sequences.fasta" << std::endl;
    std::cout << "  -g genome  -i primer3 config dir  -o outfile  -k kmer(15)  -m maxmatches(10000)  -x maxNeighborhood(10000)\n"
                 "  -d distance(1)  -q pruneprimer  -n hamming  -c cutTemp(45)  -l maxProdSize(15000)  --cutoffPenalty(-1)\n"
                 "  --penaltyTmDiff(0.6)  --penaltyTmMismatch(0.4)  --penaltyLength(0.001)  --enttemp(37)  --monovalent(50)\n"
                 "  --divalent(1.5)  --dna(50)  --dntp(0.6)\n\n";
    return -1;
  }
  std::vector<PrimerBind> allp;
  std::vector<PcrProduct> pcrColl;
  std::vector<std::string> msg, seqname, pName, pSeq;
  std::vector<uint32_t> seqlen;
  dg_index* ix = nullptr;
  auto bail = [&](const char* m) {
    msg.push_back(m);
    emit_search(c, search_json(c, ix, seqlen, seqname, allp, pcrColl, pName, pSeq, msg));
    if (ix) dg_index_close(ix);
    return 1;
  };
  if (!file_nonempty(c.genome)) return bail("Error: Genome does not exist!");
  {  // silica.h:303-315
    struct stat st;
    if (stat(c.primer3Config.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return bail("Error: Cannot find primer3 config directory!");
    while (c.primer3Config.size() > 1 && c.primer3Config.back() == '/') c.primer3Config.pop_back();
    c.primer3Config.push_back('/');
    if (!is_regular(c.primer3Config + "tetraloop.dh")) return bail("Error: Config directory path appears to be incorrect!");
  }
  if (!seq_len_name(c.genome, seqlen, seqname)) return bail("Error: Could not retrieve sequence lengths!");
  const int dev = device_from_env();
  if (dg_index_open((strip_last_extension(c.genome) + ".fm9").c_str(), dev, (std::getenv("DICEY_FULL_TABLE") ? DG_OPEN_BIG_TABLE : DG_OPEN_DEFAULT) | DG_OPEN_COMPACT, &ix) != DG_OK) {
    std::cerr << "dicey: " << dg_last_error() << std::endl;
    ix = nullptr;
    return bail("Error: FM-Index cannot be loaded!");
  }
  dg_thal* th = nullptr;
  if (dg_thal_open(c.primer3Config.c_str(), c.mv, c.dv, c.dntp, c.dna_conc, dev, &th) != DG_OK) {
    std::cerr << "dicey: " << dg_last_error() << std::endl;
    return bail("Error: Config directory path appears to be incorrect!");
  }
  {  // silica.h:350-353
    struct stat st;
    if (stat(c.infile.c_str(), &st) != 0 || S_ISDIR(st.st_mode)) {
      dg_thal_close(th);
      return bail("Error: Input fasta file is missing!");
    }
  }
  // ---- primer FASTA (silica.h:355-410), quirks included: a record counts only if longer than k, and the sequence
  // buffer is cleared only when a record is taken
  auto count_le = [&](const std::string& s, uint32_t limit) {
    uint64_t off[2] = {0, s.size()}, cnt = 0;
    if (dg_count(ix, (const uint8_t*)s.data(), off, 1, &cnt) != DG_OK) std::cerr << "dicey: " << dg_last_error() << std::endl;
    return cnt <= limit;
  };
  bool fatal = false;
  auto take = [&](const std::string& fan, const std::string& tmpfasta) -> bool {
    std::string qr = tmpfasta.substr(tmpfasta.size() - c.kmer);
    if (!c.pruneprimer || count_le(qr, c.maxPruneCount)) {
      qr = revcomp_upper(qr);
      if (!c.pruneprimer || count_le(qr, c.maxPruneCount)) {
        std::string inseq;
        for (char ch : tmpfasta) {  // util.h:208-219
          if (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T') inseq.push_back(ch);
          else {
            msg.push_back("Warning: Non-DNA character in nucleotide sequence detected and replaced by 'N'!");
            inseq.push_back('N');
          }
        }
        if (inseq.size() < 10 || inseq.size() < c.kmer) {
          msg.push_back("Error: Input sequence is shorter than 10 nucleotides or shorter than the selected k-mer length!");
          return false;
        }
        if (c.distance >= inseq.size()) {
          c.distance = (uint32_t)inseq.size() - 1;
          msg.push_back("Warning: Distance was adjusted to sequence length!");
        }
        pName.push_back(fan);
        pSeq.push_back(inseq);
      }
    }
    return true;
  };
  {
    std::ifstream fa(c.infile.c_str());
    std::string fan, tmpfasta, line;
    while (!fatal && std::getline(fa, line)) {
      if (line.empty()) continue;
      if (line[0] == '>') {
        if (!fan.empty() && !tmpfasta.empty() && tmpfasta.size() > c.kmer) {
          if (!take(fan, tmpfasta)) fatal = true;
          tmpfasta = "";
        }
        fan = line.substr(1);
      } else {
        for (auto& ch : line) ch = (char)std::toupper((unsigned char)ch);
        tmpfasta += line;
      }
    }
    if (!fatal && !fan.empty() && !tmpfasta.empty() && tmpfasta.size() > c.kmer)
      if (!take(fan, tmpfasta)) fatal = true;
  }
  auto finish = [&](int rc) {
    emit_search(c, search_json(c, ix, seqlen, seqname, allp, pcrColl, pName, pSeq, msg));
    dg_thal_close(th);
    dg_index_close(ix);
    return rc;
  };
  if (fatal) return finish(1);
  const uint32_t nseq = (uint32_t)seqlen.size();
  std::vector<std::vector<PrimerBind>> forBind(nseq), revBind(nseq);
  // A primer over 64 nt is more than the library stores, and more than thal() takes (both oligos over 60 nt: silica.h:438-442 ends the
  // run there with the error JSON).  The primers before it are searched as usual, for the warnings they add ahead of the error.
  size_t nsearch = pSeq.size();
  for (size_t q = 0; q < pSeq.size(); ++q)
    if (pSeq[q].size() > 64) {
      nsearch = q;
      break;
    }
  const bool over_limit = nsearch < pSeq.size();
  if (nsearch) {
    std::string pb;
    std::vector<uint64_t> poff(1, 0);
    for (size_t q = 0; q < nsearch; ++q) {
      pb += pSeq[q];
      poff.push_back(pb.size());
    }
    dg_search_params sp;
    sp.distance = c.distance;
    sp.hamming = c.hamming;
    sp.max_locations = c.max_locations;
    sp.max_neighborhood = c.maxNeighborhood;
    sp.kmer = c.kmer;
    sp.cut_temp = c.cutTemp;
    dg_search_result* R = nullptr;
    if (dg_search_sites(ix, th, &sp, seqlen.data(), nseq, (const uint8_t*)pb.data(), poff.data(), nsearch, &R) != DG_OK) {
      std::cerr << "dicey: " << dg_last_error() << std::endl;
      dg_thal_close(th);
      dg_index_close(ix);
      return 2;
    }
    // per primer in order: a thal failure ends the run with the error JSON (silica.h:438-442, 512-516)
    uint64_t si = 0;
    for (size_t q = 0; q < nsearch; ++q) {
      if (R->pflags[q] & DG_P_THAL_FAILED) {
        msg.push_back("Error: Thermodynamical calculation failed!");
        dg_search_result_free(R);
        return finish(1);
      }
      if (R->pflags[q] & DG_Q_NBHD_EXCEEDED) {  // silica.h:457-460
        std::string x = std::to_string(c.maxNeighborhood);
        msg.push_back("Warning: Neighborhood size exceeds " + x + " candidates. Only first " + x + " neighbors are searched, results are likely incomplete!");
      }
      for (; si < R->nsites && R->sites[si].primer == q; ++si) {
        const dg_site& s = R->sites[si];
        PrimerBind b;
        b.refIndex = s.ref;
        b.pos = s.pos;
        b.primerId = s.primer;
        b.onFor = s.on_for != 0;
        b.temp = s.temp;
        b.perfTemp = s.perf_temp;
        b.genome.assign(R->genome_pool + s.genome_off, s.genome_len);
        (b.onFor ? forBind : revBind)[s.ref].push_back(b);
      }
      if (R->pflags[q] & DG_Q_MAX_MATCHES) {
        std::string x = std::to_string(c.max_locations);
        msg.push_back("Warning: More than " + x + " matches found. Only first " + x + " matches are reported, results are likely incomplete!");
      }
    }
    dg_search_result_free(R);
  }
  if (over_limit) {
    msg.push_back("Error: Thermodynamical calculation failed!");
    return finish(1);
  }
  for (uint32_t r = 0; r < nseq; ++r) {  // silica.h:581-584
    allp.insert(allp.end(), forBind[r].begin(), forBind[r].end());
    allp.insert(allp.end(), revBind[r].begin(), revBind[r].end());
  }
  std::sort(allp.begin(), allp.end());  // silica.h:587
  if (!c.pruneprimer) {
    // Amplicons (what silica.h:590-634 produces): per chromosome, every forward site in the order it was found, paired with
    // the reverse sites — taken in the order THEY were found — that start right of it and end within maxProdSize of it.
    // The reverse sites are looked up through a position-ordered view so that only the ones inside the window are touched;
    // the window's members are then put back into discovery order, which is the order the products must have before the
    // final (unstable) sort by penalty.
    struct Placed {
      uint32_t pos, found;  // position, discovery index within the chromosome's reverse sites
    };
    // the penalty of one primer pair: both Tm shortfalls against the perfect match, the Tm difference, the product length
    // (operands and order as in silica.h:623-629: the doubles are printed with 17 significant digits)
    auto pair_penalty = [&c](const PrimerBind& f, const PrimerBind& v, uint32_t span) {
      const double short_f = (f.perfTemp - f.temp) * c.penDiff, short_v = (v.perfTemp - v.temp) * c.penDiff;
      double total = short_f < 0 ? 0 : short_f;
      if (short_v > 0) total += short_v;
      total += std::abs(f.temp - v.temp) * c.penMis;
      total += span * c.penLen;
      return total;
    };
    std::vector<Placed> view;
    std::vector<uint32_t> window;
    for (uint32_t chrom = 0; chrom < nseq; ++chrom) {
      const std::vector<PrimerBind>& fwd = forBind[chrom];
      const std::vector<PrimerBind>& rev = revBind[chrom];
      view.resize(rev.size());
      for (uint32_t k = 0; k < rev.size(); ++k) view[k] = Placed{rev[k].pos, k};
      std::sort(view.begin(), view.end(), [](const Placed& x, const Placed& y) { return x.pos != y.pos ? x.pos < y.pos : x.found < y.found; });
      for (const PrimerBind& f : fwd) {
        const uint64_t reach = (uint64_t)f.pos + c.maxProdSize;  // a reverse site further right cannot end inside the limit
        const auto from = std::partition_point(view.begin(), view.end(), [&](const Placed& x) { return x.pos <= f.pos; });
        const auto upto = std::partition_point(from, view.end(), [&](const Placed& x) { return (uint64_t)x.pos <= reach; });
        window.clear();
        for (auto it = from; it != upto; ++it) window.push_back(it->found);
        std::sort(window.begin(), window.end());
        for (uint32_t k : window) {
          const PrimerBind& v = rev[k];
          const uint64_t span = (uint64_t)v.pos + pSeq[v.primerId].size() - f.pos;
          if (span > c.maxProdSize) continue;
          PcrProduct amp;
          amp.refIndex = chrom;
          amp.leng = (uint32_t)span;
          amp.forPos = f.pos;
          amp.revPos = v.pos;
          amp.forId = f.primerId;
          amp.revId = v.primerId;
          amp.forTemp = f.temp;
          amp.revTemp = v.temp;
          amp.penalty = pair_penalty(f, v, amp.leng);
          if (c.cutofPen < 0 || amp.penalty < c.cutofPen) pcrColl.push_back(amp);
        }
      }
    }
    std::sort(pcrColl.begin(), pcrColl.end());  // silica.h:637
  }
  return finish(0);
}

// ------------------------------------------------------------------------------------------------ index (index.h:34-141)
// `dicey index --verify genome.fa.gz`: the acceptance procedure for an index file this build did not write.  The
// reader's layout is restated from sdsl-lite: the first genuine file decides whether it is right, and this is
// what decides it in minutes — or names the section that is off.  1. dg_fm9_check, deep (host): byte accounting, rank words, tree,
// C[], samples.  2. dg_index_open: the device derives BWT / text / suffix array and checks them against the file (C[] against
// symbol totals, the file's SA samples, sampled suffix order).  3. the WHOLE text (dg_extract) against the text index.h:97-115
// builds from the FASTA.  4. 1 000 sampled 24-mers: dg_count, and every dg_locate position spells the pattern.
int verify_index(const std::string& fm9, const std::string& text) {
  std::vector<char> rep(1 << 16);
  std::cerr << "[1/4] sections of " << fm9 << " (host)" << std::endl;
  if (dg_fm9_check(fm9.c_str(), DG_FM9_CHECK_DEEP, rep.data(), rep.size()) != DG_OK) {
    std::cerr << "REFUSED: " << dg_last_error() << std::endl;
    std::cout << rep.data() << std::endl;
    return 1;
  }
  std::cerr << "[2/4] open on the device (derived layouts checked against the file)" << std::endl;
  dg_index* ix = nullptr;
  if (dg_index_open(fm9.c_str(), device_from_env(), 0, &ix) != DG_OK) {
    std::cerr << "REFUSED: " << dg_last_error() << std::endl;
    return 1;
  }
  dg_index_stats_t st;
  dg_index_stats(ix, &st);
  auto refuse = [&](const std::string& why) {
    std::cerr << "REFUSED: " << why << std::endl;
    dg_index_close(ix);
    return 1;
  };
  if (st.n != text.size() + 1) return refuse("the index holds " + std::to_string(st.n - 1) + " symbols, the FASTA gives " + std::to_string(text.size()));
  std::cerr << "[3/4] the whole text against the FASTA (" << text.size() << " symbols)" << std::endl;
  const uint64_t CH = 64ull << 20;
  std::vector<uint8_t> buf(std::min<uint64_t>(CH, text.size()));
  for (uint64_t at = 0; at < text.size(); at += CH) {
    const uint64_t lo = at, end = std::min<uint64_t>(text.size(), at + CH), hi = end - 1 /* inclusive */, off[1] = {0};
    if (dg_extract(ix, &lo, &hi, 1, buf.data(), off) != DG_OK) return refuse(dg_last_error());
    if (std::memcmp(buf.data(), text.data() + lo, end - lo) != 0) {
      uint64_t k = 0;
      while (buf[k] == (uint8_t)text[lo + k]) ++k;
      return refuse("text position " + std::to_string(lo + k) + ": the index spells byte " + std::to_string((unsigned)buf[k]) + ", the FASTA " +
                    std::to_string((unsigned)(uint8_t)text[lo + k]));
    }
  }
  std::cerr << "[4/4] 1000 sampled 24-mers: count and locate" << std::endl;
  const uint32_t m = 24;
  if (text.size() > m + 1) {
    std::string pat;
    std::vector<uint64_t> poff(1, 0), where;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    while (where.size() < 1000) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      const uint64_t p0 = x % (text.size() - m);
      pat.append(text, p0, m);
      poff.push_back(pat.size());
      where.push_back(p0);
    }
    std::vector<uint64_t> cnt(where.size());
    if (dg_count(ix, (const uint8_t*)pat.data(), poff.data(), where.size(), cnt.data()) != DG_OK) return refuse(dg_last_error());
    dg_locations* loc = nullptr;
    if (dg_locate(ix, (const uint8_t*)pat.data(), poff.data(), where.size(), &loc) != DG_OK) return refuse(dg_last_error());
    std::string why;
    for (size_t i = 0; i < where.size() && why.empty(); ++i) {
      const uint64_t a = loc->off[i], b = loc->off[i + 1];
      bool own = false;
      if (b - a != cnt[i]) why = "pattern " + std::to_string(i) + ": count says " + std::to_string(cnt[i]) + ", locate returns " + std::to_string(b - a);
      for (uint64_t k = a; k < b && why.empty(); ++k) {
        own = own || loc->pos[k] == where[i];
        if (loc->pos[k] + m > text.size() || text.compare(loc->pos[k], m, pat, poff[i], m) != 0)
          why = "pattern " + std::to_string(i) + ": located position " + std::to_string(loc->pos[k]) + " does not spell it";
      }
      if (why.empty() && !own) why = "pattern " + std::to_string(i) + " was cut from text position " + std::to_string(where[i]) + ", which locate does not return";
    }
    dg_locations_free(loc);
    if (!why.empty()) return refuse(why);
  }
  dg_index_close(ix);
  std::cout << "Verified: " << fm9 << " is the index of this FASTA (" << text.size() << " symbols)." << std::endl;
  return 0;
}

int indexer(int argc, char** argv) {
  std::string genome, outfile;
  bool out_given = false, help = false;
  bool verify = false;
  const OptSpec specs[] = {{"help", '?', false}, {"output", 'o', true}, {"input-file", 0, true}, {"verify", 'v', false}};
  Parsed p = parse_options(argc, argv, specs, 4);
  if (!p.error.empty()) {
    std::cerr << p.error << std::endl;
    std::abort();
  }
  for (auto& kv : p.kv) {
    if (kv.first == "help") help = true;
    else if (kv.first == "output") { outfile = kv.second; out_given = true; }
    else if (kv.first == "input-file") genome = kv.second;
    else if (kv.first == "verify") verify = true;
  }
  if (!p.positional.empty()) genome = p.positional.back();
  if (help || genome.empty()) {
    std::cout << "Usage: dicey " << argv[0] << " [OPTIONS] genome.fa.gz" << std::endl;
    std::cout << "Generic options:\n  -? [ --help ]                    show help message\n  -o [ --output ] arg (=genome.fm9) output file\n"
                 "  -v [ --verify ]                  do not build: accept or refuse the EXISTING index file against this FASTA\n"
                 "                                   (every section of the sdsl file, then the whole text and sampled\n"
                 "                                   count / locate answers on the GPU) - the check for the first\n"
                 "                                   index that `dicey index` of the reference wrote\n\n";
    return -1;
  }
  if (!out_given) outfile = strip_last_extension(genome) + ".fm9";  // index.h:67-69
  std::ifstream probe(genome.c_str(), std::ios::binary);
  if (!probe.is_open()) {
    std::cerr << "Error: " << genome << " cannot be opened!" << std::endl;
    return -1;
  }
  probe.close();
  if (!is_gz(genome)) {
    std::cerr << "Error: Please compress " << genome << " with bgzip." << std::endl;
    return -1;
  }
  // index.h:97-115: header lines become '\n' (except before the first sequence), sequence lines are upper-cased
  std::string text, line;
  LineReader r(genome);
  bool first = true;
  while (r.next(line)) {
    if (!line.empty() && line[0] == '>') {
      if (!first) text.push_back('\n');
      else first = false;
    } else {
      for (char ch : line) text.push_back((char)std::toupper((unsigned char)ch));
    }
  }
  text.push_back('\n');
  if (verify) return verify_index(outfile, text);
  if (dg_index_build((const uint8_t*)text.data(), text.size(), device_from_env(), outfile.c_str()) != DG_OK) {
    std::cerr << "dicey: " << dg_last_error() << std::endl;
    return 1;
  }
  std::cout << "Done." << std::endl;
  return 0;
}

void display_usage() {  // dicey.cpp:19-33 (only the subcommands this build carries)
  std::cout << "Usage: dicey <command> <arguments>" << std::endl;
  std::cout << std::endl;
  std::cout << "    index        index FASTA reference file (GPU builder)" << std::endl;
  std::cout << "    hunt         search DNA sequences (MI355X search path)" << std::endl;
  std::cout << "    search       in-silico PCR (MI355X search path)" << std::endl;
  std::cout << "    padlock      padlock probe design (MI355X search path)" << std::endl;
  std::cout << "    mappability  exact-match k-mer uniqueness track (MI355X search path)" << std::endl;
  std::cout << std::endl;
  std::cout << "chop is not part of this build." << std::endl;
  std::cout << std::endl;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    display_usage();
    return 0;
  }
  std::string cmd = argv[1];
  if (cmd == "version" || cmd == "--version" || cmd == "-v") {
    std::cout << "Dicey version: v" << kVersion << " (MI355X search path, libdiceygpu ABI " << dg_abi_version() << ")" << std::endl;
    return 0;
  }
  if (cmd == "help" || cmd == "--help" || cmd == "-h" || cmd == "-?") {
    display_usage();
    return 0;
  }
  if (cmd == "hunt") {
    const double t_main0 = now_ms();
    const int rc = hunter(argc - 1, argv + 1);
    if (timing_on()) std::fprintf(stderr, "dicey timing: %-28s %8.1f ms\n", "hunt, entry to return", now_ms() - t_main0);
    // every line is written and every file closed: leave without the runtime's teardown (unloading the code objects, releasing
    // 98 GB allocation by allocation — 0.1-0.2 s of a 10 M-query run; the driver releases the process's memory either way)
    if (quick_exit_on()) {
      std::cout.flush();
      std::fflush(stdout);
      std::fflush(stderr);
      _exit(rc);
    }
    return rc;
  }
  if (cmd == "index") return indexer(argc - 1, argv + 1);
  if (cmd == "search") return silica(argc - 1, argv + 1);
  if (cmd == "padlock") return padlock_main(argc - 1, argv + 1);
  if (cmd == "mappability") return mappability_main(argc - 1, argv + 1);
  std::cerr << "Unrecognized command " << cmd << std::endl;
  return 1;
}
