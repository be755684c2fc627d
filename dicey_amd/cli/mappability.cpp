// `dicey mappability`: a bedGraph of exact-match k-mer uniqueness over the indexed genome (include/dicey_gpu.h dg_mappability).
// Not upstream dicey's chop + aligner + mappability pipeline: the value of a position is the number of occurrences of the k-mer that
// starts there, on both strands, counted on the FM-index in HBM.  The device hands over runs of equal values per position chunk;
// the host formats the chunks on several threads, compresses them (-o) into concatenated gzip members and writes them in order.
// With -u the value is the minimum unique length instead (dg_min_unique): the shortest k-mer that starts at the position and is unique.
// With -u -w the length must be unique within -w mismatches, on both strands (dg_min_unique_mm).
// With -q the positions are those of the records of a second FASTA file, which need not be in the genome (dg_query_map): zero is a value there.
// With -q -l the value is the query minimum length (dg_query_min_len): the shortest k-mer from the position with at most -t places in the genome.
// With -q -a the last -a bases of every k-mer, the oligo's 3' end, must match exactly (dg_query_map_anchored).
// With -q -l -E the length is that of the shortest specific k-mer that ENDS at the position, its last -a bases exact (dg_query_min_len_end).
// With -q -I the records may hold IUPAC codes, each letter a set of bases (dg_query_map_iupac).
// With -p the value is per BASE: the number of k-mers over the base with at most -t places (dg_map_cover), or with -u -p the length of the
// shortest unique window that contains the base (dg_map_min_cover).  Both are device transforms of the map the command makes anyway.
#include <zlib.h>

#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <iostream>
#include <thread>

#include "../../include/dicey_gpu.h"
#include "cli_common.hpp"

int mappability_main(int argc, char** argv);

namespace {

const OptSpec kMapOpts[] = {{"help", '?', false},  {"genome", 'g', true},  {"kmer", 'k', true},
                            {"forward", 'f', false}, {"maxcount", 'c', true}, {"outfile", 'o', true},
                            {"mismatches", 'e', true}, {"minunique", 'u', false},
                            {"query", 'q', true}, {"minlength", 'l', false}, {"shortest", 's', true},
                            {"atmost", 't', true}, {"anchor", 'a', true},
                            {"byend", 'E', false}, {"iupac", 'I', false}, {"maxdegeneracy", 'D', true},
                            {"within", 'w', true}, {"perbase", 'p', false}};

void map_usage() {
  std::cout << "Usage: dicey mappability [OPTIONS] -g genome.fa.gz [-q targets.fa.gz]" << std::endl;
  std::cout << "       dicey mappability -g genome.fa.gz -p [-k 100] [-e 0] [-f] [-t 1] [-c 0] [-o out.bedgraph.gz]" << std::endl;
  std::cout << "       dicey mappability -g genome.fa.gz -u -p [-k 100] [-w 0] [-f] [-o out.bedgraph.gz]" << std::endl;
  std::cout << "Generic options:\n"
               "  -? [ --help ]                      show help message\n"
               "  -g [ --genome ] arg                genome file (indexed with dicey index: <genome stem>.fm9)\n"
               "  -k [ --kmer ] arg (=100)           k-mer length (10..1000)\n"
               "  -e [ --mismatches ] arg (=0)       count k-mers with up to this many mismatches (0..2)\n"
               "  -f [ --forward ]                   forward strand only\n"
               "  -c [ --maxcount ] arg (=0)         write min(value, maxcount); 0 = exact values\n"
               "  -u [ --minunique ]                 write the minimum unique length instead; -k is then the largest length tried\n"
               "  -w [ --within ] arg (=0)           with -u: a length is unique when no other k-mer of the genome, and no k-mer of its other\n"
               "                                     strand, is within arg mismatches (0..2)\n"
               "  -q [ --query ] arg                 FASTA file of sequences to rate against the genome instead of the genome itself\n"
               "  -l [ --minlength ]                 with -q: write the shortest specific length instead; -k is then the largest length tried\n"
               "  -s [ --shortest ] arg (=10)        with -l: the smallest length tried (10..1000, at most -k)\n"
               "  -t [ --atmost ] arg (=0)           with -l: a length is specific when its k-mer has at most this many places in the genome\n"
               "                                     with -p: a k-mer counts when its value is at most arg (=1, 1..4294967293)\n"
               "  -p [ --perbase ]                   write a value per base instead of per k-mer start: the number of k-mers over the base whose\n"
               "                                     value is at most -t; -c then clamps that number.  With -u: the shortest unique length over the base\n"
               "  -a [ --anchor ] arg                with -q: the last arg bases of every k-mer must match exactly (0..-k)\n"
               "  -E [ --byend ]                     with -l: the length of the shortest specific k-mer that ENDS at the position; -a then 0..-s\n"
               "  -I [ --iupac ]                     with -q: the records may hold IUPAC codes (R Y S W K M B D H V N), each a set of bases; -k 10..64\n"
               "  -D [ --maxdegeneracy ] arg (=256)  with -I: k-mers with more expansions than this have no line (1..4096)\n"
               "  -o [ --outfile ] arg               gzipped output file (default: plain text on stdout)\n"
               "\n"
               "Output: bedGraph lines name, start, end, value (0-based, end exclusive) of maximal runs of equal values, where the value\n"
               "of a k-mer start position is the number of occurrences of that k-mer plus those of its reverse complement in the\n"
               "genome (forward only: the k-mer alone; a reverse-complement palindrome counts twice).  Positions whose k-mer holds a\n"
               "character other than A/C/G/T or runs past the sequence end have no line.  With -e 1 or -e 2 the value counts the k-mers\n"
               "of the genome within that many mismatches (substitutions) of the k-mer and of its reverse complement, the k-mer\n"
               "itself included ((k,e)-mappability); k-mers with a character other than A/C/G/T are never counted.\n"
               "With -u the value of a position is the smallest length k (at most -k, and inside the run of A/C/G/T that starts there) at\n"
               "which the k-mer that starts there has value 1: it occurs once and its reverse complement nowhere (-f: once on the forward\n"
               "strand).  Positions without such a length, still repeated at -k or at the end of their run, have no line.\n"
               "With -u -w 1 or -w 2 a length counts as unique only when the k-mer that starts there is the one k-mer of the genome within that\n"
               "many mismatches (substitutions) of itself and of its reverse complement: the smallest k at which -e with the same number writes 1,\n"
               "for every k at once.  The lengths are never below those of -u alone, and a k-mer within -w mismatches of its own reverse\n"
               "complement is not unique at that length unless -f is given.  -w 0 writes what -u writes.\n"
               "With -q the lines are those of the records of the query file (upper-cased; the name is the header's first word), in file\n"
               "order: the value of a position is the number of k-mers of the GENOME within -e mismatches of the record's k-mer and of its\n"
               "reverse complement.  The sequences need not be in the genome, so 0 is a value (absent from the genome) and has lines of\n"
               "its own; positions without a k-mer of A/C/G/T and records shorter than -k have no line.  -u cannot be combined with -q.\n"
               "With -q -l the value of a position of a record is the smallest length k (from -s to -k, inside the run of A/C/G/T that starts\n"
               "there) at which the genome holds at most -t k-mers within -e mismatches of the record's k-mer and of its reverse complement\n"
               "(-f: of the k-mer alone): -t 0 asks how long an oligo must be to have no place in the genome, -t 1 for at most one place.\n"
               "Positions without such a length, and positions where not even a k-mer of length -s starts, have no line.\n"
               "With -q -a only the k-mers of the genome that match the LAST -a bases of the record's k-mer, the 3' end of the oligo, exactly\n"
               "are counted: the places a primer could extend from or a guide's seed could bind.  On the other strand the genome shows these\n"
               "bases, reverse-complemented, as the first -a of its k-mer.  -a 0 writes what -q alone writes, -a equal to -k what -e 0 writes.\n"
               "-a cannot be combined with -l unless -E is given: with an anchored 3' end a longer oligo can have more places than a shorter one.\n"
               "With -q -l -E the value of a position of a record is the smallest length k (from -s to -k, inside the run of A/C/G/T that ends\n"
               "there) at which the k-mer that ENDS at the position, the oligo whose 3' end it is, has at most -t places in the genome within\n"
               "-e mismatches: how far a primer with this 3' end must reach back.  With -a (0..-s) only places that match the oligo's last -a\n"
               "bases exactly are counted; the 3' end stays where it is while the oligo grows at its 5' end, so a longer oligo never has more\n"
               "places.  The lines are at the coordinates of the oligo's LAST base; positions without such a length, and positions where not\n"
               "even a k-mer of length -s ends, have no line.\n"
               "With -q -I a letter of a record may be an IUPAC code, which stands for a set of bases (R = A or G, ... N = any): a degenerate primer,\n"
               "or a probe with an N at a SNP site.  A k-mer of the genome mismatches where its base lies outside the record's set, the last -a\n"
               "letters must hold the genome's bases, and every k-mer of the genome counts once however many expansions of the record's k-mer it\n"
               "is close to.  Positions whose k-mer has more than -D expansions have no line; their number is reported on stderr.  -I cannot be\n"
               "combined with -l, -u or -E, and -k is at most 64 then.\n"
               "With -p the value of a base is the number of the up to -k k-mers that lie over it whose value, as written without -p, is between\n"
               "1 and -t: with the default -t 1 the unique k-mers over the base.  -c 1 writes the single-read mappability track (the base is\n"
               "covered by at least one uniquely mappable k-mer), the value divided by -k is the multi-read mappability.  Bases that no such\n"
               "k-mer covers have no line.  With -u -p the value of a base is the length of the shortest unique window (at most -k, within -w\n"
               "mismatches) that contains it: the minimum read length at which the base is uniquely mappable, in one track.  -p cannot be\n"
               "combined with -q, and -t has no meaning with -u.\n"
               "\n";
}

int bail(const std::string& m) {
  std::cerr << m << std::endl;
  return 1;
}

struct Piece {  // the runs of positions [a, b) of one sequence
  uint32_t seq = 0;
  uint64_t a = 0, b = 0;
  std::vector<uint64_t> start;
  std::vector<uint32_t> len, value;
};

// bedGraph of the query records: one line per maximal run of equal values over valid positions, zero included.  With lp (-l) the values
// are minimum lengths and zero, no length, has no line either, and with ep (-l -E) those by end position, at the coordinates of the
// k-mer's last base; with ap (-a) they are the anchored counts, with ip (-I) those of records with IUPAC codes
int write_query_map(dg_index* ix, const dg_qmap_params& qp, const dg_qminlen_params* lp, const dg_qminlen_end_params* ep,
                    const dg_qmap_anchor_params* ap, const dg_qmap_iupac_params* ip, const std::string& query, const std::string& outfile) {
  std::vector<std::string> names, seqs;
  if (!read_fasta(query, true, names, seqs)) return bail("Error: Could not read any sequence from " + query + "!");
  std::vector<uint64_t> off(seqs.size() + 1, 0);
  for (size_t i = 0; i < seqs.size(); ++i) off[i + 1] = off[i] + seqs[i].size();
  std::string all;
  all.reserve(off.back());
  for (const std::string& s : seqs) all += s;
  std::vector<uint32_t> val(off.back());
  dg_qmap_iupac_stats_t ist{};
  const int rc = ip   ? dg_query_map_iupac(ix, ip, (const uint8_t*)all.data(), off.data(), seqs.size(), val.data(), &ist)
                 : ep ? dg_query_min_len_end(ix, ep, (const uint8_t*)all.data(), off.data(), seqs.size(), val.data(), nullptr)
                 : lp ? dg_query_min_len(ix, lp, (const uint8_t*)all.data(), off.data(), seqs.size(), val.data(), nullptr)
                 : ap ? dg_query_map_anchored(ix, ap, (const uint8_t*)all.data(), off.data(), seqs.size(), val.data(), nullptr)
                      : dg_query_map(ix, &qp, (const uint8_t*)all.data(), off.data(), seqs.size(), val.data(), nullptr);
  if (rc != DG_OK) return bail(std::string("dicey: ") + dg_last_error());
  if (ist.too_degenerate)
    std::cerr << "Warning: " << ist.too_degenerate << " positions have a k-mer with more than " << (ip->max_degeneracy ? ip->max_degeneracy : 256u)
              << " expansions (-D) and no line!" << std::endl;
  FILE* fo = stdout;
  if (!outfile.empty()) {
    fo = std::fopen(outfile.c_str(), "wb");
    if (!fo) return bail("Error: cannot open " + outfile + " for writing!");
  }
  const std::string dest = outfile.empty() ? std::string("stdout") : outfile;
  bool ok = true, wrote = false;
  std::string text, packed, err;
  auto flush = [&]() {  // -o: one gzip member per flush, which gzip -dc reads in a row
    if (text.empty() || !ok) return;
    const std::string* w = &text;
    if (!outfile.empty()) {
      if (!gzip_member(text, packed)) {
        err = "Error: compression failed!";
        ok = false;
        return;
      }
      w = &packed;
    }
    if (std::fwrite(w->data(), 1, w->size(), fo) != w->size()) {
      err = "Error: short write to " + dest + "!";
      ok = false;
    }
    wrote = true;
    text.clear();
  };
  for (size_t i = 0; i < seqs.size() && ok; ++i) {
    const uint32_t* v = val.data() + off[i];
    const uint64_t len = seqs[i].size();
    for (uint64_t a = 0; a < len;) {
      uint64_t b = a + 1;
      while (b < len && v[b] == v[a]) ++b;
      if (v[a] != DG_QMAP_INVALID && !((lp || ep) && v[a] == 0)) {
        text += names[i];
        text.push_back('\t');
        uint_append(text, a);
        text.push_back('\t');
        uint_append(text, b);
        text.push_back('\t');
        uint_append(text, v[a]);
        text.push_back('\n');
        if (text.size() >= (16u << 20)) flush();
      }
      a = b;
    }
  }
  flush();
  if (ok && !wrote && !outfile.empty()) {  // no run at all: still a valid (empty) gzip file
    if (!gzip_member(std::string(), packed) || std::fwrite(packed.data(), 1, packed.size(), fo) != packed.size()) {
      err = "Error: short write to " + dest + "!";
      ok = false;
    }
  }
  if (fo != stdout) {
    if (std::fclose(fo) != 0 && ok) {
      err = "Error: cannot finish writing " + outfile + "!";
      ok = false;
    }
  } else if (std::fflush(stdout) != 0 && ok) {
    err = "Error: short write to stdout!";
    ok = false;
  }
  if (!ok) return bail(err);
  return 0;
}

}  // namespace

int mappability_main(int argc, char** argv) {
  Parsed p = parse_options(argc, argv, kMapOpts, sizeof kMapOpts / sizeof kMapOpts[0]);
  if (!p.error.empty()) {
    std::cerr << "Error: " << p.error << std::endl;
    map_usage();
    return -1;
  }
  std::string genome, outfile, query;
  bool help = false, have_genome = false, forward = false, minunique = false, have_query = false, minlength = false, have_shortest = false,
       have_atmost = false, have_anchor = false, byend = false, iupac = false, have_maxdeg = false, have_within = false, perbase = false;
  long long k = 100, maxcount = 0, mismatches = 0, shortest = 10, atmost = 0, anchor = 0, maxdeg = 256, within = 0;
  for (auto& kv : p.kv) {
    if (kv.first == "help") help = true;
    else if (kv.first == "genome") { genome = kv.second; have_genome = true; }
    else if (kv.first == "kmer") k = std::strtoll(kv.second.c_str(), nullptr, 10);
    else if (kv.first == "forward") forward = true;
    else if (kv.first == "maxcount") maxcount = std::strtoll(kv.second.c_str(), nullptr, 10);
    else if (kv.first == "outfile") outfile = kv.second;
    else if (kv.first == "mismatches") mismatches = std::strtoll(kv.second.c_str(), nullptr, 10);
    else if (kv.first == "minunique") minunique = true;
    else if (kv.first == "query") { query = kv.second; have_query = true; }
    else if (kv.first == "minlength") minlength = true;
    else if (kv.first == "shortest") { shortest = std::strtoll(kv.second.c_str(), nullptr, 10); have_shortest = true; }
    else if (kv.first == "atmost") { atmost = std::strtoll(kv.second.c_str(), nullptr, 10); have_atmost = true; }
    else if (kv.first == "anchor") { anchor = std::strtoll(kv.second.c_str(), nullptr, 10); have_anchor = true; }
    else if (kv.first == "byend") byend = true;
    else if (kv.first == "iupac") iupac = true;
    else if (kv.first == "maxdegeneracy") { maxdeg = std::strtoll(kv.second.c_str(), nullptr, 10); have_maxdeg = true; }
    else if (kv.first == "perbase") perbase = true;
    else if (kv.first == "within") { within = std::strtoll(kv.second.c_str(), nullptr, 10); have_within = true; }
  }
  if (help || !have_genome || !p.positional.empty()) {
    map_usage();
    return -1;
  }
  if (k < 10 || k > 1000) return bail("Error: k-mer length " + std::to_string(k) + " outside 10..1000!");
  if (mismatches < 0 || mismatches > 2) return bail("Error: number of mismatches " + std::to_string(mismatches) + " outside 0..2!");
  if (maxcount < 0 || maxcount > 0xFFFFFFFFll) return bail("Error: maxcount " + std::to_string(maxcount) + " outside 0..4294967295!");
  if (minunique && (mismatches != 0 || maxcount != 0)) return bail("Error: --minunique cannot be combined with --mismatches or --maxcount!");
  if (minunique && have_query) return bail("Error: --minunique cannot be combined with --query!");
  if (minlength && !have_query) return bail("Error: --minlength needs --query!");
  if (minlength && maxcount != 0) return bail("Error: --minlength cannot be combined with --maxcount!");
  if (perbase && have_query) return bail("Error: --perbase cannot be combined with --query!");
  if (perbase && minunique && have_atmost) return bail("Error: --perbase --minunique cannot be combined with --atmost!");
  if (perbase && !have_atmost) atmost = 1;
  if (perbase && (atmost < 1 || atmost > 0xFFFFFFFDll)) return bail("Error: atmost " + std::to_string(atmost) + " outside 1..4294967293!");
  if ((have_shortest || (have_atmost && !perbase)) && !minlength) return bail("Error: --shortest and --atmost need --minlength!");
  if (shortest < 10 || shortest > 1000) return bail("Error: shortest length " + std::to_string(shortest) + " outside 10..1000!");
  if (shortest > k) return bail("Error: shortest length " + std::to_string(shortest) + " above the largest length " + std::to_string(k) + " (-k)!");
  if (atmost < 0 || atmost > 0xFFFFFFFDll) return bail("Error: atmost " + std::to_string(atmost) + " outside 0..4294967293!");
  if (have_anchor && !have_query) return bail("Error: --anchor needs --query!");
  if (have_anchor && minlength && !byend) return bail("Error: --anchor cannot be combined with --minlength!");
  if (have_anchor && (anchor < 0 || anchor > k)) return bail("Error: anchor " + std::to_string(anchor) + " outside 0.." + std::to_string(k) + " (-k)!");
  if (iupac && !have_query) return bail("Error: --iupac needs --query!");
  if (iupac && minunique) return bail("Error: --iupac cannot be combined with --minunique!");
  if (iupac && minlength) return bail("Error: --iupac cannot be combined with --minlength!");
  if (iupac && byend) return bail("Error: --iupac cannot be combined with --byend!");
  if (have_maxdeg && !iupac) return bail("Error: --maxdegeneracy needs --iupac!");
  if (iupac && k > 64) return bail("Error: k-mer length " + std::to_string(k) + " outside 10..64 (--iupac)!");
  if (maxdeg < 1 || maxdeg > 4096) return bail("Error: maxdegeneracy " + std::to_string(maxdeg) + " outside 1..4096!");
  if (have_within && !minunique) return bail("Error: --within needs --minunique!");
  if (within < 0 || within > 2) return bail("Error: within " + std::to_string(within) + " outside 0..2!");
  if (!file_nonempty(genome)) return bail("Error: Genome does not exist!");
  if (have_query && !file_nonempty(query)) return bail("Error: Query file " + query + " does not exist or is empty!");
  if (byend && !minlength) return bail("Error: --byend needs --minlength!");
  if (byend && have_anchor && anchor > shortest)
    return bail("Error: anchor " + std::to_string(anchor) + " above the shortest length " + std::to_string(shortest) + " (-s)!");
  std::vector<uint32_t> seqlen;
  std::vector<std::string> seqname;
  if (!seq_len_name(genome, seqlen, seqname)) return bail("Error: Could not retrieve sequence lengths!");
  const std::string fm9 = strip_last_extension(genome) + ".fm9";
  if (!file_nonempty(fm9)) return bail("Error: Index " + fm9 + " does not exist (dicey index -o " + fm9 + " " + genome + ")!");
  const char* de = std::getenv("DICEY_DEVICE");
  const int device = de ? std::atoi(de) : 0;
  dg_index* ix = nullptr;
  if (dg_index_open(fm9.c_str(), device, DG_OPEN_COMPACT | DG_OPEN_NO_PRE5, &ix) != DG_OK) return bail(std::string("dicey: ") + dg_last_error());
  struct IxCloser {
    dg_index* ix;
    ~IxCloser() { dg_index_close(ix); }
  } ixc{ix};
  dg_index_stats_t ist;
  if (dg_index_stats(ix, &ist) != DG_OK) return bail(std::string("dicey: ") + dg_last_error());
  uint64_t total = 1;
  for (uint32_t l : seqlen) total += l;  // each length + its '\n', then the sentinel
  if (total != ist.n)
    return bail("Error: the sequence lengths of " + genome + " (" + std::to_string(total - 1) + " characters with separators) do not match the index " +
                fm9 + " (" + std::to_string(ist.n - 1) + ")!");
  if (have_query) {
    const dg_qmap_params qp = {(uint32_t)k, (uint32_t)mismatches, forward ? 1 : 0, (uint32_t)maxcount, 0u, {0u, 0u, 0u}};
    const dg_qminlen_params lp = {(uint32_t)shortest, (uint32_t)k, (uint32_t)mismatches, forward ? 1 : 0, (uint32_t)atmost, 0u, {0u, 0u}};
    const dg_qmap_anchor_params ap = {(uint32_t)k, (uint32_t)mismatches, (uint32_t)anchor, forward ? 1 : 0, (uint32_t)maxcount, 0u, {0u, 0u}};
    const dg_qminlen_end_params ep = {(uint32_t)shortest, (uint32_t)k, (uint32_t)mismatches, (uint32_t)anchor, forward ? 1 : 0, (uint32_t)atmost, 0u,
                                      {0u, 0u}};
    const dg_qmap_iupac_params ip = {(uint32_t)k, (uint32_t)mismatches, (uint32_t)anchor, forward ? 1 : 0, (uint32_t)maxcount, (uint32_t)maxdeg, 0u,
                                     {0u, 0u, 0u}};
    return write_query_map(ix, qp, minlength && !byend ? &lp : nullptr, byend ? &ep : nullptr, have_anchor && !byend && !iupac ? &ap : nullptr,
                           iupac ? &ip : nullptr, query, outfile);
  }
  // -p: the count map needs to tell 1..atmost from more, nothing else, so its search may stop at atmost + 1; -c clamps the cover count
  dg_map_mm_params mp = {(uint32_t)k, (uint32_t)mismatches, forward ? 1 : 0, perbase ? (uint32_t)atmost + 1u : (uint32_t)maxcount, 0u, 0u};
  dg_min_unique_params up = {(uint32_t)k, forward ? 1 : 0, 0u, 0u};
  dg_min_unique_mm_params wp = {(uint32_t)k, (uint32_t)within, forward ? 1 : 0, 0u, 0u};
  dg_map* m = nullptr;
  if ((minunique ? (within ? dg_min_unique_mm(ix, &wp, &m) : dg_min_unique(ix, &up, &m)) : dg_mappability_mm(ix, &mp, &m)) != DG_OK)
    return bail(std::string("dicey: ") + dg_last_error());
  if (perbase) {  // the per-base transform of the map just made, which is then dropped
    const dg_cover_params cp = {(uint32_t)atmost, (uint32_t)maxcount, 0u, 0u};
    const dg_min_cover_params np = {0u, 0u};
    dg_map* pb = nullptr;
    const int rc = minunique ? dg_map_min_cover(ix, m, &np, &pb) : dg_map_cover(ix, m, &cp, &pb);
    dg_map_free(m);
    m = pb;
    if (rc != DG_OK) return bail(std::string("dicey: ") + dg_last_error());
  }
  struct MapFreer {
    dg_map* m;
    ~MapFreer() { dg_map_free(m); }
  } mf{m};

  FILE* fo = stdout;
  if (!outfile.empty()) {
    fo = std::fopen(outfile.c_str(), "wb");
    if (!fo) return bail("Error: cannot open " + outfile + " for writing!");
  }
  // pieces of at most PIECE positions, in FASTA order; a run that crosses a piece edge is carried into the next piece of its sequence
  // (DICEY_MAP_PIECE: a smaller piece, so that tests put piece edges inside runs of a small genome)
  uint64_t PIECE = 1ull << 22;
  if (const char* e = std::getenv("DICEY_MAP_PIECE")) PIECE = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
  std::vector<Piece> jobs;
  {
    uint64_t off = 0;
    for (uint32_t s = 0; s < seqlen.size(); ++s) {
      const uint64_t len = seqlen[s] - 1;
      for (uint64_t a = 0; a < len; a += PIECE) {
        Piece pc;
        pc.seq = s;
        pc.a = off + a;
        pc.b = off + std::min(len, a + PIECE);
        jobs.push_back(std::move(pc));
      }
      off += seqlen[s];
    }
  }
  unsigned nthr = std::thread::hardware_concurrency();
  if (const char* e = std::getenv("OMP_NUM_THREADS")) nthr = (unsigned)std::max(1, std::atoi(e));
  nthr = std::max(1u, std::min(nthr, 16u));
  std::vector<uint64_t> seq_off(seqlen.size());
  for (size_t s = 0, o = 0; s < seqlen.size(); o += seqlen[s], ++s) seq_off[s] = o;
  bool have_carry = false;
  uint64_t carry_start = 0;
  uint32_t carry_len = 0, carry_val = 0;
  bool ok = true, wrote = false;
  std::string err;
  for (size_t j0 = 0; j0 < jobs.size() && ok; j0 += nthr) {
    const size_t j1 = std::min(jobs.size(), j0 + nthr);
    for (size_t j = j0; j < j1; ++j) {  // runs off the device (one call per piece), carries settled in order
      Piece& pc = jobs[j];
      uint64_t nr = 0;
      uint64_t* s = nullptr;
      uint32_t *l = nullptr, *v = nullptr;
      if (dg_map_runs(m, pc.a, pc.b, &nr, &s, &l, &v) != DG_OK) {
        err = std::string("dicey: ") + dg_last_error();
        ok = false;
        break;
      }
      pc.start.assign(s, s + nr);
      pc.len.assign(l, l + nr);
      pc.value.assign(v, v + nr);
      dg_buffer_free(s);
      dg_buffer_free(l);
      dg_buffer_free(v);
      if (have_carry) {
        if (!pc.start.empty() && pc.start[0] == pc.a && pc.value[0] == carry_val && carry_start + carry_len == pc.a) {
          pc.start[0] = carry_start;
          pc.len[0] += carry_len;
        } else {
          pc.start.insert(pc.start.begin(), carry_start);
          pc.len.insert(pc.len.begin(), carry_len);
          pc.value.insert(pc.value.begin(), carry_val);
        }
        have_carry = false;
      }
      const bool seq_goes_on = j + 1 < jobs.size() && jobs[j + 1].seq == pc.seq;
      if (seq_goes_on && !pc.start.empty() && pc.start.back() + pc.len.back() == pc.b) {
        have_carry = true;
        carry_start = pc.start.back();
        carry_len = pc.len.back();
        carry_val = pc.value.back();
        pc.start.pop_back();
        pc.len.pop_back();
        pc.value.pop_back();
      }
    }
    if (!ok) break;
    std::vector<std::string> text(j1 - j0), packed(j1 - j0);
    std::vector<char> good(j1 - j0, 1);
    auto work = [&](size_t t) {
      const Piece& pc = jobs[j0 + t];
      const std::string& name = seqname[pc.seq];
      const uint64_t so = seq_off[pc.seq];
      std::string& o = text[t];
      o.reserve(pc.start.size() * (name.size() + 24));
      for (size_t r = 0; r < pc.start.size(); ++r) {
        o += name;
        o.push_back('\t');
        uint_append(o, pc.start[r] - so);
        o.push_back('\t');
        uint_append(o, pc.start[r] - so + pc.len[r]);
        o.push_back('\t');
        uint_append(o, pc.value[r]);
        o.push_back('\n');
      }
      if (!outfile.empty() && !o.empty()) good[t] = gzip_member(o, packed[t]);
    };
    std::vector<std::thread> th;
    for (size_t t = 0; t < j1 - j0; ++t) th.emplace_back(work, t);
    for (auto& x : th) x.join();
    for (size_t t = 0; t < j1 - j0 && ok; ++t) {
      if (!good[t]) {
        err = "Error: compression failed!";
        ok = false;
        break;
      }
      const std::string& w = outfile.empty() ? text[t] : packed[t];
      wrote |= !w.empty();
      if (!w.empty() && std::fwrite(w.data(), 1, w.size(), fo) != w.size()) {
        err = "Error: short write to " + (outfile.empty() ? std::string("stdout") : outfile) + "!";
        ok = false;
      }
    }
    for (size_t j = j0; j < j1; ++j) {
      std::vector<uint64_t>().swap(jobs[j].start);
      std::vector<uint32_t>().swap(jobs[j].len);
      std::vector<uint32_t>().swap(jobs[j].value);
    }
  }
  if (ok && !wrote && !outfile.empty()) {  // no run at all: still a valid (empty) gzip file
    std::string empty;
    if (!gzip_member(std::string(), empty) || std::fwrite(empty.data(), 1, empty.size(), fo) != empty.size()) {
      err = "Error: short write to " + outfile + "!";
      ok = false;
    }
  }
  if (fo != stdout) {
    if (std::fclose(fo) != 0 && ok) {
      err = "Error: cannot finish writing " + outfile + "!";
      ok = false;
    }
  } else if (std::fflush(stdout) != 0 && ok) {
    err = "Error: short write to stdout!";
    ok = false;
  }
  if (!ok) return bail(err);
  return 0;
}
