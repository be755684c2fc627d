/* dicey_gpu.h — C ABI of libdiceygpu.so: the MI355X (gfx950) in-silico-PCR search path.
 *
 * gear-genomics/dicey has no plugin/FFI interface.  The seam this library replaces is the set of
 * calls `dicey hunt` makes into sdsl-lite and into its own helper headers:
 *
 *   reference call (file:line)                              entry point here
 *   ------------------------------------------------------  ---------------------------------
 *   load_from_checked_file(csa_wt<>&, path)  hunter.h:253-256, silica.h:340-343   dg_index_open
 *   fm_index.size()                          hunter.h:368-369                     dg_index_stats
 *   sdsl::count(fm_index, b, e)              hunter.h:353, silica.h:470           dg_count
 *   sdsl::locate(...) + std::sort            hunter.h:355-356, silica.h:472-473   dg_locate
 *   sdsl::extract(fm_index, lo, hi)          hunter.h:371, silica.h:490           dg_extract
 *   neighbors() -> count -> locate -> extract -> needle()/needleScore -> DnaHit push
 *                                            hunter.h:291-437 (whole per-query loop)  dg_hunt
 *   sdsl::construct + store_to_checked_file  index.h:121-122                      dg_index_build
 *   neighbors(q, alphabet, d, indel, maxsize, set)  neighbors.h:86-92 (hunter.h:334,339)  dg_neighbors
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative DG_E* code and
 * leaves a message retrievable with dg_last_error() (thread-local); objects returned through `out`
 * parameters are released with the paired *_free / *_close; no exceptions cross the boundary; one
 * HIP stream per dg_index; a dg_index may be used by one thread at a time (distinct handles are
 * independent — one handle per GPU for multi-GPU).  There is NO CPU fallback: without a HIP device
 * every compute entry point fails with DG_ENODEV.
 */
#ifndef DICEY_GPU_H
#define DICEY_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: hunt/count/locate/extract/index build; 2: + thal, search sites, neighbourhood counts, padlock scan, shared handles;
 * 3: + dg_neighbors, capped neighbourhoods answered instead of refused, max_locations 0
 * 4: hits carry their alignment in compact form (dg_hunt_result::ops; dg_hunt_rows / dg_hit_rows rebuild the two rows),
 *    result buffers come from a pinned pool, dg_hunt_submit / dg_hunt_wait
 * 5: dg_hunt_params grows by max_query_len and flags; DG_HUNT_COMPACT: 8 + 4 d bytes per hit and 8 bytes per query cross PCIe / xGMI
 *    (dg_chit_unpack, dg_hunt_expand, dg_normalize_query turn them back); dg_hunt_submit keeps up to three batches in flight on ONE handle
 * 6: dg_hunt_result grows by stream / d_block / d_block_bytes (the gather over RCCL lives in libdiceygather.so, include/dicey_gather.h)
 * 7 (additive exports, same version): dg_mappability, dg_map_values, dg_map_runs, dg_map_device_values, dg_map_stats, dg_map_free
 * 7 (additive exports, same version): dg_mappability_mm, dg_map_mm_stats ((k,e)-mappability, up to two mismatches)
 * 7 (additive exports, same version): dg_query_map (the same counts for the k-mers of sequences outside the index)
 * 7 (additive exports, same version): dg_min_unique (the shortest unique k-mer at each position)
 * 7 (additive exports, same version): dg_query_min_len (the shortest specific k-mer at each position of sequences outside the index)
 * 7 (additive exports, same version): dg_min_unique_mm, dg_map_mu_mm_stats (the shortest k-mer unique within up to two mismatches)
 * 7 (additive exports, same version): dg_map_cover, dg_map_min_cover, dg_map_cover_stats (per-base tracks: the unique k-mers over each base) */
#define DG_ABI_VERSION 7

enum {
  DG_OK = 0,
  DG_EINVAL = -1,   /* bad argument */
  DG_EIO = -2,      /* file cannot be read / written */
  DG_EFORMAT = -3,  /* not an sdsl csa_wt<> file (byte accounting failed) */
  DG_ENODEV = -4,   /* no usable HIP device */
  DG_EHIP = -5,     /* HIP runtime error */
  DG_ENOMEM = -6,
  DG_ELIMIT = -7    /* input outside the supported envelope (see DESIGN.md "limits") */
};

typedef struct dg_index dg_index;

/* flags for dg_index_open */
#define DG_OPEN_DEFAULT 0u
#define DG_OPEN_NO_SELFCHECK 1u /* skip the load-time self validation (C[] vs Occ totals, SA permutation spot checks) */
#define DG_OPEN_NO_KMER_TABLE 2u /* do not derive the K-mer jump table (saves up to 34 GB of HBM; search is slower) */
#define DG_OPEN_COMPACT 4u       /* ABI 7: a process that opens the index for ONE input — skip the layouts that only pay for a resident index: the suffix
                                  * array with context records and its prefix levels (40 GB of HBM on a 3.1 Gb genome, 0.36 s to derive, and as much again for
                                  * the driver to wipe at exit); hits of repeat-rich strings then read their context from the text and walk the block minima,
                                  * results are the same.  (ABI 4-6: accepted, no effect.)  `dicey hunt|search|padlock` pass it. */
#define DG_OPEN_NO_PRE5 16u      /* ABI 7: do not derive the preceding-characters array (6.2 GB, 0.19 s on a 3.1 Gb genome): narrow table intervals are then
                                  * extended character by character through the Occ blocks — the distance-1 search kernel takes a quarter longer per
                                  * batch (0.146 -> 0.183 ms per 100 000 20-mers; distance 2: + 5 %), which a process that answers a few million
                                  * queries and exits never earns back.  Same results.  `dicey hunt` passes it unless the input is very large. */
#define DG_OPEN_BIG_TABLE 8u     /* table of order ceil(log4 n) + 1 when the device has room (137 GB instead of 34 GB on a 3.1 Gb genome):
                                    the distance-1 search kernel gains ~5 % (0.175 -> 0.166 ms per 100 000 20-mers), the open takes longer
                                    and the process holds 199 GB instead of 90 GB — for resident servers with HBM to spare */

/* Parses the file written by `dicey index` (sdsl store_to_checked_file of csa_wt<>) unchanged, uploads it to
 * HBM on `device`, and derives the search layouts there (Occ blocks, full suffix array, text copy). */
int dg_index_open(const char* fm9_path, int device, uint32_t flags, dg_index** out);
void dg_index_close(dg_index* ix);
/* A second handle on the SAME device-resident index with its own HIP stream and batch workspaces, so that another host
 * thread can run batches concurrently (the small tail kernels of one batch overlap with the search kernel of the other).
 * No index data is copied.  Close every shared handle before the handle it was taken from. */
int dg_index_share(dg_index* src, dg_index** out);
/* The handle's HIP stream (a hipStream_t).  Work a caller enqueues on it is ordered with the handle's batches: a device-side copy
 * out of dg_hunt_result::d_hits issued on this stream is complete before the next batch overwrites the buffer, with no host
 * synchronisation (bench.py stages its RCCL gather this way). */
void* dg_index_stream(dg_index* ix);

typedef struct {
  uint64_t n;              /* fm_index.size(): text length + 1 (sentinel) */
  uint32_t sigma;          /* alphabet size incl. sentinel */
  uint32_t code_len[256];  /* Huffman code length of each byte in the loaded wavelet tree (0 = absent) */
  uint64_t file_bytes;     /* size of the .fm9 */
  uint64_t hbm_bytes;      /* device memory held by this index (raw sections + derived layouts) */
  double load_seconds;     /* file read + upload + derivation */
  double derive_seconds;   /* derivation kernels only */
} dg_index_stats_t;
int dg_index_stats(const dg_index* ix, dg_index_stats_t* out);

/* ---- sdsl seam, batched.  Patterns are raw bytes, concatenated; pattern i = pat[off[i] .. off[i+1]). ---- */
int dg_count(dg_index* ix, const uint8_t* pat, const uint64_t* off, size_t npat, uint64_t* counts /* [npat] */);

typedef struct {
  size_t npat;
  uint64_t* off; /* [npat+1] */
  uint64_t* pos; /* positions of pattern i, ascending: pos[off[i] .. off[i+1]) */
} dg_locations;
int dg_locate(dg_index* ix, const uint8_t* pat, const uint64_t* off, size_t npat, dg_locations** out);
void dg_locations_free(dg_locations* l);

/* text[lo[i] .. hi[i]] inclusive (hi < n), written to out + out_off[i] */
int dg_extract(dg_index* ix, const uint64_t* lo, const uint64_t* hi, size_t nrange, uint8_t* out, const uint64_t* out_off);

/* ---- hunt ---- */
typedef struct {
  uint32_t distance;         /* -d  (hunter.h:188, default 1) */
  int32_t hamming;           /* -n  (hunter.h:189): substitutions only, no context, no alignment */
  int32_t forward_only;      /* -f  (hunter.h:190) */
  uint64_t max_locations;    /* -m  (hunter.h:186, default 1000) */
  uint32_t max_neighborhood; /* -x  (hunter.h:187, default 10000) */
  uint32_t max_query_len;    /* ABI 5: an upper bound of the batch's query lengths when the caller knows one (a primer design tool does);
                              * 0 = the library finds out (the host entry points scan their offsets, dg_hunt_device reads its offsets
                              * back: a host round trip per new buffer).  The kernels count queries above the bound and the call fails
                              * with DG_EINVAL rather than answer them wrongly. */
  uint32_t flags;            /* ABI 5: DG_HUNT_* */
} dg_hunt_params;
#define DG_HUNT_COMPACT 1u   /* results in compact form (below): what the host needs to rebuild every DnaHit, nothing it already has */
#define DG_HUNT_PHASE_TIMES 2u /* measure ms_select / ms_locate / ms_verify too (HIP events between the stages: a few microseconds of
                                * stream markers per batch); ms_total and ms_search_flat are always measured */

/* per-query flag bits */
#define DG_Q_TOO_SHORT 1u     /* < 10 nt: "Error: Input sequence is shorter than 10 nucleotides!" (hunter.h:299-303) */
#define DG_Q_DIST_ADJUSTED 2u /* hunter.h:312-315 */
#define DG_Q_MAX_MATCHES 4u   /* hits >= max_locations (hunter.h:434-437) */
#define DG_Q_NBHD_EXCEEDED 8u /* hunter.h:342-345: a strand's neighbourhood reached max_neighborhood; the strings searched are
                               * the ones the reference's capped enumeration holds (see dg_neighbors) */

typedef struct {
  int32_t score;     /* DnaHit::score (0, -1, ...) */
  uint32_t chr;      /* refIndex */
  uint32_t start;    /* 1-based (chrpos+1, hunter.h:402) */
  uint32_t query;    /* index into the batch */
  uint16_t aln_len;  /* columns in refalign/queryalign */
  uint8_t strand;    /* '+' or '-' */
  uint8_t reserved;
} dg_hit;

/* Compact alignment (ABI 4).  The rows the reference pushes into DnaHit (hunter.h:391-405, 411-426) are the characters of the
 * query strand the hit was found on, with at most |score| <= distance columns that are not a match: leading and trailing
 * columns whose query row is a gap are stripped, and every other non-matching column costs one.  A hit therefore travels as
 * dg_hit + `ops_per_hit` 32-bit words, one per non-matching column in column order, DG_ALN_NONE behind the last:
 *   bits 0-15 column, bits 16-17 kind, bits 24-31 the reference byte of that column (kinds MISMATCH and QUERY_GAP)
 * 24 bytes per hit at distance 1 instead of 68 with two character rows — what crosses PCIe and xGMI.  dg_hit_rows() /
 * dg_hunt_rows() rebuild refalign / queryalign byte for byte. */
#define DG_ALN_MISMATCH 0u  /* reference byte over a different query character */
#define DG_ALN_REF_GAP 1u   /* '-' in refalign over a query character */
#define DG_ALN_QUERY_GAP 2u /* reference byte over '-' in queryalign */
#define DG_ALN_NONE 0xFFFFFFFFu
#define DG_ALN_COL(op) ((op) & 0xFFFFu)
#define DG_ALN_KIND(op) (((op) >> 16) & 3u)
#define DG_ALN_BYTE(op) ((op) >> 24)

/* Compact results (ABI 5, DG_HUNT_COMPACT).  Per hit 2 + ops_per_hit words, in push order, the hits of query i at
 * chits + hit_off[i] * (2 + ops_per_hit):
 *   word 0   text position of the neighbourhood string the hit stems from (what sdsl::locate returned, hunter.h:355): the
 *            sequence is the one that holds this position (hunter.h:358-362, seq_start[] below), chrpos = position - its start
 *   word 1   bits 0-3 -score, bit 4 strand (1 = '-'), bits 5-11 delta + 32 where DnaHit::start = chrpos + delta + 1 (the
 *            context characters in front of the string, hunter.h:382 with its strict '<', and the leading gap columns of
 *            hunter.h:391-401 are in delta), bits 16-31 aln_len
 *   words 2.. the alignment description of ABI 4 (DG_ALN_*)
 * Per query one word qinfo: bits 0-7 DG_Q_* flags, bits 8-15 effective distance, bits 16-31 characters replaced by 'N'.
 * The normalised queries are NOT returned: dg_normalize_query applies util.h:208-219 + to_upper to the caller's own bytes.
 * 12 bytes per hit at distance 1 (ABI 4: 24), 8 bytes per query (ABI 4: 12 + the sequence + 8 of offsets). */
#define DG_CHIT_WORDS(ops_per_hit) (2u + (ops_per_hit))
#define DG_CHIT_NEG_SCORE(meta) ((meta) & 15u)
#define DG_CHIT_STRAND(meta) ((((meta) >> 4) & 1u) ? '-' : '+')
#define DG_CHIT_DELTA(meta) ((int32_t)(((meta) >> 5) & 127u) - 32)
#define DG_CHIT_ALN_LEN(meta) ((meta) >> 16)
#define DG_QINFO_FLAGS(w) ((w) & 255u)
#define DG_QINFO_DISTANCE(w) (((w) >> 8) & 255u)
#define DG_QINFO_NONDNA(w) ((w) >> 16)

typedef struct {
  size_t nq;
  uint64_t nhits;
  uint64_t* hit_off;      /* [nq+1]: hits of query i = hits[hit_off[i] .. hit_off[i+1]) in REFERENCE PUSH ORDER (pre-sort) */
  dg_hit* hits;           /* [nhits] */
  uint32_t ops_per_hit;   /* words of alignment description per hit: the batch's largest effective distance (0: every row is the query) */
  uint32_t aln_stride;    /* bytes per row in refalign / queryalign (0 until dg_hunt_rows has run) */
  uint32_t* ops;          /* [nhits * ops_per_hit] */
  char* refalign;         /* NULL until dg_hunt_rows(): row of hit h = refalign + h*aln_stride, aln_len bytes */
  char* queryalign;       /* likewise */
  uint32_t* qflags;       /* [nq] DG_Q_* */
  uint32_t* qdistance;    /* [nq] effective (clamped) distance */
  uint32_t* qnondna;      /* [nq] number of characters replaced by 'N' (one warning each, util.h:214) */
  uint8_t* qseq;          /* normalised (upper-cased, non-ACGT -> N) queries, concatenated like the input */
  uint64_t* qoff;         /* [nq+1] */
  /* measurement: exact op counters of the executed device algorithm (DESIGN.md "algorithmic bytes") */
  uint64_t ctr_ext_steps; /* interval extensions (2 Occ-block reads each) */
  uint64_t ctr_leaves;    /* occurring neighbourhood strings emitted by the search kernel */
  uint64_t ctr_sa_reads;  /* suffix-array entries (and block minima) read by locate */
  uint64_t ctr_win_bytes; /* text window bytes the reference would extract (hunter.h:371), one window per hit */
  uint64_t ctr_tab_reads; /* K-mer jump-table entries read (8 B each) */
  double ms_total;        /* device time of the whole batch (HIP events on the index stream) */
  double ms_search;       /* of which: neighbourhood/backward-search kernel */
  double ms_select;       /* minimal-set + ordering kernel */
  double ms_locate;
  double ms_verify;       /* window fetch + Needleman-Wunsch */
  /* device-resident copies (HIP pointers on the index's device), valid until the next call on this index:
   * what a multi-GPU driver hands to RCCL to gather hit lists without a host round trip */
  const void* d_hits;     /* dg_hit[nhits] */
  const void* d_ops;      /* uint32_t[nhits * ops_per_hit] */
  uint64_t ctr_filter_probes; /* K-mer presence-filter bits tested (one 4-byte word each); ctr_tab_reads counts the table
                               * entries actually read, i.e. the probes that found their K-mer present */
  double ms_search_flat;      /* part of ms_search spent in the flat kernel (k_search1p at distance 1, k_search2p at edit distance 2); 0 when none ran */
  void* owner_;               /* library internal (pinned-pool bookkeeping) */
  /* ABI 5.  compact != 0: chits / qinfo / seq_start are set, hit_off as always; hits, ops, qflags, qdistance, qnondna, qseq, qoff are
   * NULL until dg_hunt_expand() builds them on the host; d_hits then points at the compact records in HBM and d_ops is NULL. */
  uint32_t compact;
  uint32_t nseq;
  uint32_t* chits;            /* [nhits * DG_CHIT_WORDS(ops_per_hit)] */
  uint32_t* qinfo;            /* [nq] */
  uint64_t* seq_start;        /* [nseq] text position of every sequence's first character (prefix sums of seqlen) */
  void* expanded_;            /* library internal (dg_hunt_expand's allocations) */
  /* measurement: the capped-neighbourhood stage in front of the batch (hunt_cap.hpp / nbhd_host.hpp), host wall clock, and what it did */
  double ms_cap;              /* 0 when no query of the batch could reach the cap */
  uint64_t cap_queries_device, cap_queries_host, cap_patterns; /* queries enumerated on the device / on the host, explicit patterns searched */
  /* Where the batch's flat search kernel ran on the handle's timeline (r04): begin / end in ms since a base event the handle's lanes
   * share.  With several batches in flight the launches of neighbouring batches overlap, and the time the kernel RAN is the union of these
   * intervals, not the sum of their lengths (bench.py's roofline).  t_base_gen: intervals of equal generation share a base (the
   * library takes a new base every few seconds to keep float precision); 0 = no timeline (one lane only so far, or no flat kernel). */
  double t_search_begin_ms, t_search_end_ms;
  uint32_t t_base_gen;
  uint32_t flat_kernel_form; /* measurement: the flat search kernel this batch ran — 0 none (general k_search only), 1 k_search1p, 2 k_search1s<.,
                              * false> (select stage inside), 3 k_search1s<., true> (select and take inside), 4 k_search2p<false, false>, 5 k_search2p<true, false>,
                              * 6 k_search2p<false, true>, 7 k_search2p<true, true> (second template argument: the r05 body for batches
                              * whose shortest strings still ask the long filter) */
  /* ABI 6: what a gather over RCCL needs (include/dicey_gather.h).  stream: the hipStream_t the batch ran on — the handle's own, or
   * the internal lane's for a dg_hunt_submit / dg_hunt_device_submit batch; a device-side copy out of the result's device buffers
   * queued on it is ordered before that lane's next batch, with no host synchronisation.  Compact results: d_block is the batch's
   * whole answer in HBM as ONE block [hit counts u32[nq] | qinfo u32[nq] | records (nhits * DG_CHIT_WORDS words)] = d_block_bytes
   * bytes (d_hits points at its records; hit_off is the prefix sum of the counts); after a fetch the host has the same bytes at
   * (uint8_t*)qinfo - 4 nq.  NULL / 0 for a classic result. */
  void* stream;
  const void* d_block;
  uint64_t d_block_bytes;
  /* ABI 7, measurement: which verify kernel served the batch — band width << 8 | hits per lane of k_verify_memo (7 << 8 | 4 is
   * k_verify_memo<7, 4>), 0 for the full-matrix / long-query kernels and for `search` (k_site); and how many of the batch's locate
   * jobs (strings with more than 16 occurrences) took a run of a prefix level's records instead of a walk down the block minima */
  uint32_t verify_kernel_form;
  uint32_t reserved7;
} dg_hunt_result;

/* One compact hit as a dg_hit (query = the query it belongs to, from hit_off) and a pointer to its ops words. */
int dg_chit_unpack(const dg_hunt_result* r, uint64_t h, uint32_t query, dg_hit* out, const uint32_t** ops);
/* hunter.h:306 + util.h:208-219: upper-case, every character outside A,C,G,T becomes 'N'; *nondna = how many were replaced
 * (a literal 'N' counts: the reference warns once per replaced character). */
int dg_normalize_query(const uint8_t* in, uint32_t len, uint8_t* out, uint32_t* nondna);
/* Builds the ABI-4 arrays (hits, ops, qflags, qdistance, qnondna, qseq, qoff) of a compact result on the host, from the caller's
 * own query bytes (the ones the batch was submitted with); several host threads.  Afterwards dg_hunt_rows / dg_hit_rows work as
 * on a classic result.  A no-op on a classic result. */
int dg_hunt_expand(dg_hunt_result* r, const uint8_t* qbytes, const uint64_t* qoff);

/* The two alignment rows of one hit from its compact description.  qseq / qlen: the NORMALISED query (dg_hunt_result::qseq:
 * A,C,G,T,N), forward strand — the reverse complement a '-' hit was aligned to is formed here (util.h:54-114).  ops: the hit's
 * ops_per_hit words (NULL when ops_per_hit == 0).  Writes hit->aln_len bytes to each row (no terminator).  DG_EINVAL when the
 * description does not fit the query (a corrupted record). */
int dg_hit_rows(const dg_hit* hit, const uint32_t* ops, uint32_t ops_per_hit, const uint8_t* qseq, uint32_t qlen, char* refalign,
                char* queryalign);
/* Fills r->refalign / r->queryalign / r->aln_stride for every hit of a fetched result (several host threads). */
int dg_hunt_rows(dg_hunt_result* r);

/* Host-buffer entry point: queries are raw bytes as read from the FASTA/argv (any case), concatenated.
 * seqlen[i] = faidx length of sequence i + 1 (util.h:201), nseq sequences. */
int dg_hunt(dg_index* ix, const dg_hunt_params* p, const uint32_t* seqlen, uint32_t nseq, const uint8_t* qbytes,
            const uint64_t* qoff, size_t nq, dg_hunt_result** out);
void dg_hunt_result_free(dg_hunt_result* r);

/* Asynchronous form: dg_hunt_submit returns as soon as the batch is handed to the library (the query buffers are copied, the
 * caller may reuse them at once); dg_hunt_wait blocks until the result is on the host (a pinned block, like dg_hunt's) and releases
 * the ticket.  ABI 5: up to THREE batches may be in flight on one handle (the library runs them on internal lanes — own stream,
 * own workspaces, own helper thread each, the same resident index — so uploads, kernels and downloads of neighbouring batches
 * overlap): submit A, submit B, wait A, submit C, wait B, ...  Tickets are waited for in the order they were submitted; a fourth
 * submit before the first wait fails with DG_EINVAL.  Every ticket must be waited for before its handle is closed. */
typedef struct dg_hunt_ticket dg_hunt_ticket;
int dg_hunt_submit(dg_index* ix, const dg_hunt_params* p, const uint32_t* seqlen, uint32_t nseq, const uint8_t* qbytes,
                   const uint64_t* qoff, size_t nq, dg_hunt_ticket** out);
int dg_hunt_wait(dg_hunt_ticket* t, dg_hunt_result** out);

/* Device-resident entry point used by bench.py: d_qbytes / d_qoff are HIP device pointers on the index's device.
 * The result stays in HBM; only the counters/timings and nhits are copied back.  `fetch` != 0 additionally
 * copies hits to host like dg_hunt.  The offsets are read back once to size the batch; a repeated call with the same
 * d_qoff, nq and total_qbytes reuses that bound, and the kernels report any query that exceeds it (the call then reads
 * the offsets again by itself), so the buffers may be refilled in place between calls. */
int dg_hunt_device(dg_index* ix, const dg_hunt_params* p, const uint32_t* seqlen, uint32_t nseq, const void* d_qbytes,
                   const void* d_qoff, size_t nq, uint64_t total_qbytes, int fetch, dg_hunt_result** out);
/* Asynchronous form of dg_hunt_device (r04), on the same lanes as dg_hunt_submit and collected with dg_hunt_wait: a caller whose
 * batches are resident in HBM keeps two or three in flight — submit A, submit B, wait A, submit C, wait B, ... — so that one batch's
 * launch-bound tail (locate, verify, the summary's read-back) runs beside another batch's search kernel.  The device buffers must
 * stay untouched until the ticket has been waited for; a result left in HBM (fetch = 0) is valid until the next submit after its
 * own wait (the lane that ran it is idle until then).  Replaces nothing in the reference: hunter.h:291 walks its queries one by one. */
int dg_hunt_device_submit(dg_index* ix, const dg_hunt_params* p, const uint32_t* seqlen, uint32_t nseq, const void* d_qbytes,
                          const void* d_qoff, size_t nq, uint64_t total_qbytes, int fetch, dg_hunt_ticket** out);

/* ---- `dicey padlock`: how often the neighbourhood of a probe arm occurs (reference src/padlock.h:392-421) ----
 * For sequence i (>= 10 nt; A/C/G/T sequences run on the search kernel, sequences with other letters are enumerated on
 * the host and counted with dg_count): fw_count[i] = sum over s in neighbors(seq_i, distance, indel, maxsize) of
 * sdsl::count(fm_index, s) and rv_count[i] the same for its reverse complement — the totals the reference accumulates in
 * hits[0] / hits[1] (its loops only stop early once the running total already exceeds the threshold it is compared with,
 * so every comparison it makes has the same outcome on the full totals).  The original sequence is part of its own
 * neighbourhood.  max_neighborhood is neighbors()' cap (10000 in padlock.h:396); when it can fire the reference's capped
 * enumeration is reproduced on the host and its strings are counted (DESIGN.md "the cap").  Sequences above 255 nt are
 * refused here with DG_ELIMIT (dg_hunt takes them). */
int dg_neighborhood_count(dg_index* ix, uint32_t distance, int hamming, uint32_t max_neighborhood, const uint8_t* qbytes,
                           const uint64_t* qoff, size_t nq, uint64_t* fw_count, uint64_t* rv_count);

/* ---- neighbors() with its size cap (reference src/neighbors.h:29-92), host side ----
 * The strings `dicey hunt` / `search` / `padlock` search for one sequence and one strand: seq is the normalised sequence
 * (A,C,G,T,N), alphabet {A,C,G,T}.  Edit mode keeps the substring-minimal strings; when the working set reaches
 * max_neighborhood the reference stops generating (neighbors.h:50) and what it holds then depends on its generation order,
 * which this function follows.  *out = the strings in std::set order, '\n'-terminated each, NUL at the end (release with
 * dg_buffer_free); *count their number; *cap_fired != 0 <=> count >= max_neighborhood (hunter.h:342-345 warns).
 * dg_hunt, dg_search_sites and dg_neighborhood_count call this for the sequences whose neighbourhood could reach the cap
 * and search exactly these strings; all other sequences are enumerated inside the search kernel.  Needs no device. */
int dg_neighbors(const uint8_t* seq, uint32_t len, uint32_t distance, int hamming, uint32_t max_neighborhood, char** out,
                 uint64_t* count, int* cap_fired);
void dg_buffer_free(void* p);

/* ---- index construction on the GPU (what `dicey index` does with sdsl::construct, index.h:97-123) ---- */
/* text = SEQ1 '\n' SEQ2 '\n' ... SEQk '\n' (upper-cased), no NUL inside.  Writes sdsl csa_wt<> layout. */
int dg_index_build(const uint8_t* text, uint64_t len, int device, const char* out_fm9_path);
/* same, text already in HBM (bench: synthetic genome generated on device) */
int dg_index_build_device(const void* d_text, uint64_t len, int device, const char* out_fm9_path);

/* ---- thermodynamic alignment for `dicey search` (primer3 thal(), type END1, temponly) ----
 * replaces primer3thal::get_thermodynamic_values + set_thal_default_args (silica.h:316-329) and primer3thal::thal()
 * (silica.h:437, 511; thal.h:2409-2655).  config_dir holds primer3's stack.ds ... tstack2.dh tables. */
typedef struct dg_thal dg_thal;
int dg_thal_open(const char* config_dir, double mv, double dv, double dntp, double dna_conc, int device, dg_thal** out);
void dg_thal_close(dg_thal* th);
/* pair k = (oligo1, oligo2) = seqs[off[2k]..off[2k+1]), seqs[off[2k+1]..off[2k+2]); temp[k] = o.temp (-999999 = THAL_ERROR_SCORE
 * when both sequences exceed 60 nt), end1/end2 = align_end_1/2 (may be NULL) */
int dg_thal_batch(dg_thal* th, const uint8_t* seqs, const uint64_t* off, size_t npairs, double* temp, int32_t* end1, int32_t* end2);

/* ---- `dicey padlock`: the per-position values of a batch of exons (reference src/padlock.h:321-428) ----
 * exons: strand-corrected, upper-case exon sequences (exonseq of padlock.h:313-315), concatenated; exon e =
 * exons[exon_off[e] .. exon_off[e+1]).  Exons shorter than 2*armlen carry no positions.  For exon e, arm window q
 * (0 <= q <= len-armlen) has slot pos_off[e] + q:
 *   arm_gc      gccontent(arm)                          (padlock.h:324, 342; -1 when the window holds an N)
 *   arm_tm      thal(arm, reverse complement).temp      (:331-336; DG_PADLOCK_NOT_COMPUTED when arm_gc fails the filter)
 *   probe_gc / probe_tm  the same for the 2*armlen probe starting at q (:356-371; q <= len-2*armlen; probe_tm is computed
 *                only when both arms pass GC, the Tm ceiling 93 + GC - 675/armlen and the Tm difference)
 *   arm_count   sdsl::count(arm) + sdsl::count(reverse complement)   (:381-385)
 *   arm_nbcount occurrences summed over neighbors(arm) and neighbors(reverse complement) (:396-405; see
 *                dg_neighborhood_count); both -1 unless the arm belongs to a probe inside the Tm window (:372-374)
 * The caller replays the reference's decisions (including `k += targetlen - 1` after an accepted probe) on these arrays;
 * a decision that would need a value not computed here cannot be reached.  thal refusing a pair (both oligos > 60 nt)
 * shows as -999999, the reference's error path (:337-340).
 * armlen < 10 with distance > 0 is refused with DG_EINVAL before any GPU work: the reference enumerates neighbors() of arms
 * of any length (:396-405, neighbors.h), dg_neighborhood_count takes 10 nt or more.  distance 0 takes every armlen >= 1. */
#define DG_PADLOCK_NOT_COMPUTED (-1e300)
typedef struct {
  uint32_t armlen;    /* -m */
  uint32_t distance;  /* -d */
  int32_t hamming;    /* -n */
  uint32_t tmdiff;    /* -z */
  double gc_min, gc_max; /* --gcmin / --gcmax */
} dg_padlock_params;
typedef struct {
  uint64_t nexons, npos;
  uint64_t* pos_off; /* nexons+1 */
  double *arm_gc, *arm_tm, *probe_gc, *probe_tm;
  int64_t *arm_count, *arm_nbcount;
  uint64_t n_arm_thal, n_probe_thal, n_arms_counted; /* work done, for measurements */
} dg_padlock_result;
int dg_padlock_scan(dg_index* ix, dg_thal* th, const dg_padlock_params* p, const uint8_t* exons, const uint64_t* exon_off, size_t nexons,
                    dg_padlock_result** out);
void dg_padlock_result_free(dg_padlock_result* r);

/* ---- `dicey search`: binding sites of a batch of primers (reference src/silica.h:429-573) ----
 * Per primer: thal(primer, revcomp) (silica.h:437); neighbourhood of its last k nucleotides on both strands through the
 * FM-index; per located hit the context window with the 5' overhang, thal(primer, window), the Tm cut, the alignment
 * position that de-duplicates hits, and the trimmed genomic site (silica.h:474-566). */
typedef struct {
  uint32_t distance;         /* -d */
  int32_t hamming;           /* -n */
  uint64_t max_locations;    /* -m (default 10000) */
  uint32_t max_neighborhood; /* -x */
  uint32_t kmer;             /* -k (default 15) */
  double cut_temp;           /* -c (default 45.0) */
} dg_search_params;
#define DG_P_THAL_FAILED 16u /* "Error: Thermodynamical calculation failed!" (silica.h:438-442, 512-516) */
typedef struct {
  uint32_t ref;      /* refIndex */
  uint32_t pos;      /* PrimerBind::pos (0-based) */
  uint32_t primer;   /* primerId */
  uint8_t on_for;    /* forward-strand site */
  uint8_t reserved[3];
  double temp;       /* Tm of primer vs site */
  double perf_temp;  /* Tm of primer vs its perfect complement */
  uint64_t genome_off;
  uint32_t genome_len;
  uint32_t pad;
} dg_site;
typedef struct {
  size_t nprimers;
  uint64_t nsites;
  dg_site* sites;     /* reference push order: primer-major, forward-strand hits then reverse-strand hits */
  char* genome_pool;  /* PrimerBind::genome strings */
  uint32_t* pflags;   /* [nprimers] DG_Q_MAX_MATCHES | DG_Q_NBHD_EXCEEDED | DG_P_THAL_FAILED */
  double* match_temp; /* [nprimers] */
  uint64_t nhits;     /* located hits, each of which went through thal() */
  double ms_device;   /* device time of the search + site kernels (HIP events) */
  /* measurement, as in dg_hunt_result: the FM-index part and the per-hit thal()/alignment part of ms_device */
  double ms_fm_search, ms_site_stage;
  uint64_t ctr_ext_steps, ctr_tab_reads, ctr_filter_probes, ctr_sa_reads;
} dg_search_result;
/* primers: already upper-cased / N-replaced sequences (silica.h:368), each at least `kmer` long */
int dg_search_sites(dg_index* ix, dg_thal* th, const dg_search_params* p, const uint32_t* seqlen, uint32_t nseq,
                    const uint8_t* pbytes, const uint64_t* poff, size_t nprimers, dg_search_result** out);
void dg_search_result_free(dg_search_result* r);

/* ABI 7.  Acceptance check of an index file WITHOUT a device (reference: the file sdsl::store_to_checked_file writes at
 * src/index.h:121-122 and load_from_checked_file reads at src/hunter.h:253-256).  The sections of csa_wt<wt_huff<>, 32, 64> are
 * walked byte by byte and held against each other; with DG_FM9_CHECK_DEEP the large sections are read through as well (rank words
 * against the bit vector's popcounts, node sizes / offsets of the Huffman tree, C[] against the leaf sizes, SA / ISA samples).
 * `report` (may be NULL) receives one JSON object: {"ok", "layout", "n", "sigma", "sections":[{"name","offset","bytes"}...],
 * "error"}.  Returns DG_OK, DG_EIO, or DG_EFORMAT with a message (also dg_last_error()) that NAMES the first section whose byte
 * count or invariant is off — what a maintainer needs when the first genuine `dicey index` file does not load. */
#define DG_FM9_CHECK_DEEP 1u
int dg_fm9_check(const char* fm9_path, uint32_t flags, char* report, size_t report_cap);

/* ABI 7, additive (the version stays 7: nothing that existed changed).  `dicey mappability`: exact-match k-mer uniqueness of every text
 * position, on the resident index.  For T = SEQ1 '\n' SEQ2 '\n' ... (the text `dicey index` wrote, sentinel at n-1), k in 10..1000
 * (else DG_ELIMIT) and a position p < n-1: value(p) = 0 when p + k > n-1 or T[p, p+k) holds a byte other than A/C/G/T (N, IUPAC
 * letters, the '\n' between sequences: a k-mer never crosses a sequence); otherwise count(w) + count(revcomp(w)) for w = T[p, p+k),
 * count = sdsl::count (overlapping occurrences included) — the both-strand total of `padlock` (hits[0] + hits[1]).  A reverse-complement
 * palindrome (w == revcomp(w), even k only) therefore counts TWICE per occurrence.  forward_only: count(w) alone.  Every valid position
 * has value >= 1; values saturate at 0xFFFFFFFF; max_count = C > 0 writes min(value, C) (C = 2: a unique / non-unique track).
 * This is NOT upstream dicey's chop + aligner + mappability pipeline.  The computation runs on the handle's stream and needs about
 * 8n + 3n/8 bytes of free HBM beside the index (DG_ENOMEM before any kernel otherwise); DG_EINVAL while a dg_hunt_submit batch is in
 * flight on the handle.  The map keeps u32[n-1] values in HBM and a stream of its own; free it before closing the index. */
typedef struct {
  uint32_t k;           /* k-mer length, 10..1000 */
  int32_t forward_only; /* count(w) only */
  uint32_t max_count;   /* 0 = exact values, else min(value, max_count) */
  uint32_t flags;       /* 0 */
} dg_map_params;
typedef struct dg_map dg_map;
typedef struct {
  uint64_t n;               /* the index's n: values cover positions [0, n-1) */
  uint32_t k, reserved;
  double ms_valid;          /* device time: valid-position bitmap */
  double ms_forward;        /* group boundaries in suffix-array order + the two scans (forward counts) */
  double ms_reverse;        /* backward search of revcomp(w) per group of equal k-mers (0-ish with forward_only) */
  double ms_scatter;        /* values to text positions */
  double ms_total;
  uint64_t rev_steps;       /* backward-search steps taken behind the K-mer table (measurement) */
  uint64_t transient_bytes; /* HBM held during the computation beside the result */
} dg_map_stats_t;
int dg_mappability(dg_index* ix, const dg_map_params* p, dg_map** out);
/* values of positions [lo, hi) (hi <= n-1) to the host */
int dg_map_values(dg_map* m, uint64_t lo, uint64_t hi, uint32_t* out);
/* maximal runs of equal non-zero values inside [lo, hi), in position order: run r covers start[r] .. start[r] + len[r] - 1 with
 * value[r].  A run is cut at lo and hi, never elsewhere.  The three arrays are library buffers (release each with dg_buffer_free);
 * only the runs cross PCIe. */
int dg_map_runs(dg_map* m, uint64_t lo, uint64_t hi, uint64_t* nruns, uint64_t** start, uint32_t** len, uint32_t** value);
/* u32[n-1] on the index's device, valid until dg_map_free */
const void* dg_map_device_values(const dg_map* m);
int dg_map_stats(const dg_map* m, dg_map_stats_t* out);
void dg_map_free(dg_map* m); /* NULL: no-op */

/* ABI 7, additive.  (k,e)-mappability, the definition of GEM and GenMap restricted to substitutions: a window q is VALID when T[q, q+k)
 * lies inside the text and holds only A/C/G/T (the rule above).  For a valid p with w = T[p, p+k) and e = mismatches in 0..2 (else
 * DG_ELIMIT):
 *   fwd_e(p) = #{valid q : Hamming(T[q, q+k), w) <= e}  (q = p included),   rev_e(p) = the same against revcomp(w),
 *   value_e(p) = fwd_e(p) + rev_e(p)   (forward_only: fwd_e(p)),
 * i.e. the sum of sdsl::count(u) over all u in {A,C,G,T}^k within Hamming distance e of w, and of revcomp(w).  A window that holds N,
 * an IUPAC letter or '\n' is never an occurrence; a reverse-complement (near-)palindrome is counted on both strands; invalid p has
 * value 0; sums saturate at 0xFFFFFFFF; max_count = C > 0 writes min(value, C), and the search of a k-mer stops once its total reaches
 * C.  mismatches = 0 is dg_mappability, bit for bit.  The result is an ordinary dg_map: dg_map_values / dg_map_runs /
 * dg_map_device_values / dg_map_stats (search time in ms_reverse, backward-search steps in rev_steps) / dg_map_free serve it.  Memory
 * and the refusal while a hunt batch is in flight are dg_mappability's.  The parameter block is checked before the handle: non-zero
 * flags or reserved DG_EINVAL, mismatches > 2 DG_ELIMIT, then a null handle DG_EINVAL; *out is cleared on every failure. */
typedef struct {
  uint32_t k;           /* k-mer length, 10..1000 */
  uint32_t mismatches;  /* e: 0, 1 or 2 substitutions */
  int32_t forward_only; /* fwd_e only */
  uint32_t max_count;   /* 0 = exact values, else min(value, max_count) */
  uint32_t flags;       /* 0 */
  uint32_t reserved;    /* 0 */
} dg_map_mm_params;
int dg_mappability_mm(dg_index* ix, const dg_map_mm_params* p, dg_map** out);
/* counters of the search per group head of equal k-mers (all zero for a map made with mismatches = 0 or by dg_mappability) */
typedef struct {
  uint64_t heads;         /* distinct valid k-mers searched */
  uint64_t steps;         /* backward-search steps (one pair of Occ lines each, all four characters) */
  uint64_t table_reads;   /* K-mer table entries read */
  uint64_t verified_rows; /* suffix-array rows finished on the text */
  uint64_t early_exits;   /* heads whose search stopped at max_count */
  uint64_t launches;      /* kernel launches of the search (head ranks go through in chunks) */
  double ms_search;       /* device time of the search */
} dg_map_mm_stats_t;
int dg_map_mm_stats(const dg_map* m, dg_map_mm_stats_t* out);

/* ABI 7, additive.  Minimum unique length: how long must an oligo that starts at p be before it is unique in the genome?  For the index
 * text T (sentinel at n-1), a position p in [0, n-1) and max_k in 10..1000 (else DG_ELIMIT):
 *   run(p)     = the number of consecutive A/C/G/T bytes from p; 0 when T[p] is anything else (N, IUPAC letters, the '\n' between
 *                sequences and the sentinel all end a run),
 *   limit(p)   = min(run(p), max_k),
 *   value_k(p) = dg_mappability's value at k: count(w) + count(revcomp(w)) for w = T[p, p+k), count = sdsl::count (forward_only:
 *                count(w) alone); a reverse-complement palindrome therefore never has value 1 at its own length,
 *   mul(p)     = the smallest k in 1..limit(p) with value_k(p) == 1, and 0 when there is none: the position is not A/C/G/T, or the
 *                k-mer is still repeated at limit(p).
 * So for every k in 10..max_k and every p whose k-mer is valid at k: mul(p) != 0 && mul(p) <= k  <=>  dg_mappability(k)[p] == 1; and
 * mul(p) = max(1 + maxlcp(p), first k with count(revcomp(w_k)) == 0) wherever both are <= limit(p), maxlcp(p) being the longer common
 * prefix (raw text bytes) of suffix p with its neighbours in suffix-array order.  Values below 10 are legal (small genomes).  One
 * pass over the suffix array instead of one dg_mappability pass per candidate k.  The result is an ordinary dg_map: dg_map_values /
 * dg_map_runs (a run is a stretch of equal non-zero lengths) / dg_map_device_values / dg_map_free serve it; dg_map_stats has k =
 * max_k, the neighbour-prefix pass in ms_forward, the backward search of the other strand in ms_reverse with its steps in rev_steps,
 * ms_valid = ms_scatter = 0 (the search writes the values); dg_map_mm_stats stays all zero.  Like dg_mappability the computation runs on
 * the index handle's stream (the map's own stream serves the reads afterwards).  Needs about 6n bytes of free HBM beside
 * the index (DG_ENOMEM before any kernel otherwise); DG_EINVAL while a dg_hunt_submit batch is in flight on the handle.  The parameter
 * block is checked before the handle: non-zero flags or reserved DG_EINVAL, max_k outside 10..1000 DG_ELIMIT, then a null handle
 * DG_EINVAL; *out is cleared on every failure. */
typedef struct {
  uint32_t max_k;       /* 10..1000 */
  int32_t forward_only; /* value_k = count(w) alone */
  uint32_t flags;       /* 0 */
  uint32_t reserved;    /* 0 */
} dg_min_unique_params;
int dg_min_unique(dg_index* ix, const dg_min_unique_params* p, dg_map** out);

/* ABI 7, additive.  Minimum unique length with mismatches, (k,e)-mappability over all k at once: how long must an oligo that starts at p
 * be before nothing else in the genome, on either strand, is within e substitutions of it?  T, run(p) and limit(p) as for dg_min_unique,
 * e = mismatches in 0..2:
 *   value_{e,k}(p) = what dg_mappability_mm writes at p for this k, e and forward_only with max_count = 0: the valid windows of the text
 *                    within e substitutions of w_k = T[p, p+k) and of its reverse complement; w_k itself is one of them, so the value is
 *                    >= 1 wherever k <= run(p),
 *   mul_e(p)       = the smallest k in 1..limit(p) with value_{e,k}(p) == 1, and 0 when there is none.
 * value_{e,k}(p) never rises with k on either strand (a window within e of the (k+1)-mer has its k-prefix within e of the k-mer; on the
 * other strand the window one further right; a valid (k+1)-window has a valid k-prefix and k-suffix), so "value == 1" is false up to some
 * k and true from there on.  Hence: mul_0 is dg_min_unique, bit for bit (mismatches = 0 IS that call); for every k in 10..max_k and every
 * p valid at k, mul_e(p) != 0 && mul_e(p) <= k  <=>  dg_mappability_mm(k, e)[p] == 1; mul_e(p) is 0 or >= mul_{e-1}(p), and 0 wherever
 * mul_{e-1}(p) is 0 (a window within e-1 is within e); and dg_query_min_len(min_k, max_k, at_most = 1, e) on a record equal to a whole
 * sequence returns DG_QMAP_INVALID where limit(p) < min_k, 0 where mul_e(p) == 0 and max(mul_e(p), min_k) elsewhere.  A k-mer within e
 * of its own reverse complement counts itself on the other strand and is never unique at that length unless forward_only is set.
 * The call runs dg_min_unique's two passes and then one search per position with mul_0(p) != 0 that probes lengths from mul_0(p)
 * upward (positions in chunks of launches); it needs dg_min_unique's memory, about 6n bytes of free HBM beside the index (DG_ENOMEM
 * before any kernel otherwise).  The result is an ordinary dg_map: dg_map_values / dg_map_runs / dg_map_device_values / dg_map_free
 * serve it; dg_map_stats has k = max_k, ms_forward and ms_reverse the two exact passes (rev_steps the steps of the second), ms_valid =
 * ms_scatter = 0 and ms_total = ms_forward + ms_reverse + dg_mu_mm_stats_t::ms_search, formed in double in that order;
 * dg_map_mm_stats stays all zero.  Checked in this order: a null parameter block or out pointer DG_EINVAL; non-zero flags or reserved
 * DG_EINVAL; max_k outside 10..1000 or mismatches > 2 DG_ELIMIT; a null handle DG_EINVAL; free HBM (DG_ENOMEM); then DG_EINVAL while a
 * dg_hunt_submit batch is in flight on the handle.  *out is cleared on every failure. */
typedef struct {
  uint32_t max_k;       /* 10..1000 */
  uint32_t mismatches;  /* e: 0, 1 or 2 substitutions */
  int32_t forward_only; /* the k-mer's own strand alone */
  uint32_t flags;       /* 0 */
  uint32_t reserved;    /* 0 */
} dg_min_unique_mm_params;
int dg_min_unique_mm(dg_index* ix, const dg_min_unique_mm_params* p, dg_map** out);
/* counters of the search with mismatches (all zero for a map made with mismatches = 0 or by any other call) */
typedef struct {
  uint64_t candidates;    /* positions with mul_0(p) != 0: the ones searched */
  uint64_t probes;        /* (position, k) pairs searched */
  uint64_t steps;         /* backward-search steps (one pair of Occ lines each, all four characters) */
  uint64_t table_reads;   /* K-mer table entries read */
  uint64_t verified_rows; /* suffix-array rows finished on the text */
  uint64_t launches;      /* kernel launches of the search (positions go through in chunks) */
  double ms_search;       /* device time of the search, behind the two exact passes */
} dg_mu_mm_stats_t;
int dg_map_mu_mm_stats(const dg_map* m, dg_mu_mm_stats_t* out);

/* ABI 7, additive.  Per-base tracks: device transforms of a dg_map that is already resident.  Every call above gives a value per k-mer
 * START position; these give a value per BASE, the form Umap and ENCODE publish.  T, "valid window", value_k, value_{e,k}, run, mul and
 * mul_e are those above; positions are p in [0, n-1).
 *
 * Cover count (dg_map_cover).  src is a count map made at length k by dg_mappability or dg_mappability_mm, t = at_most >= 1:
 *   spec(q)    = 1 iff 1 <= src(q) <= t   (t = 1: the k-mer that starts at q is unique),
 *   cover_t(p) = #{q : max(0, p-k+1) <= q <= p, spec(q) = 1}, the number of specific k-mers that lie over base p, in 0..k;
 * max_count = C > 0 writes min(cover, C).  C = 1 is the single-read mappability track (is this base covered by at least one uniquely
 * mappable k-mer?), cover / k the multi-read one.  A k-mer never crosses a sequence, an N or the text's end because src is 0 at those
 * starts; no boundary rule is needed beyond that.  The work per base does not grow with k (a bitmap of spec, a rank directory over it,
 * two ranks per base).
 *
 * Minimum covering length (dg_map_min_cover).  src is a length map made with max_k by dg_min_unique or dg_min_unique_mm (any mismatches,
 * any forward_only):
 *   mcl(p) = min{max(src(q), p-q+1) : p-max_k+1 <= q <= p, q >= 0, src(q) != 0, run(q) >= p-q+1}, and 0 when the set is empty:
 * the length of the shortest unique valid window, at most max_k, that contains base p, i.e. the minimum read length at which the base is
 * uniquely mappable.  (A window that starts at q with length m >= mul(q) inside q's run is unique, because value never rises with the
 * length.)
 *
 * The identity that ties the two together: for every k in 10..max_k and every p that lies in at least one VALID k-window,
 *   cover_1 at k is >= 1 at p   <=>   mcl(p) != 0 && mcl(p) <= k.
 * =>: a unique valid k-window at q over p has 0 != mul(q) <= k, run(q) >= k and p-q+1 <= k.  <=: mcl(p) = m <= k names a unique valid
 * window U of m bases over p; p lies in a valid k-window, so the A/C/G/T run around p holds at least k bases and U can be grown inside it
 * to a valid k-window W over p; W is unique, on both strands and with mismatches, because every place within e of W holds a place within
 * e of U at the matching offset, and U has one.  The restriction is needed: a base in an A/C/G/T run shorter than k can have
 * mcl(p) <= k while no k-window covers it.
 *
 * Both calls run on src's own stream and read only src and immutable blocks of the index, so a dg_hunt_submit batch in flight on the
 * handle does not refuse them.  src is left untouched and stays usable; it may be freed before the result.  The result is an ordinary
 * dg_map with a stream of its own, synchronised before return: dg_map_values / dg_map_runs / dg_map_device_values / dg_map_free serve
 * it; its dg_map_stats has n, k (src's k or max_k) and ms_total (the transform), everything else 0.  A call needs 4n bytes for the
 * result, plus n/8 + n/16 and the scan's scratch for the cover transform; the min-cover transform holds nothing beside its counters.
 * Checked in this order, *out cleared on every failure: a null parameter block, out or src DG_EINVAL; non-zero flags or reserved
 * DG_EINVAL; at_most outside 1..0xFFFFFFFD DG_ELIMIT; a null handle DG_EINVAL; src of the wrong kind (a length or per-base map given to
 * dg_map_cover, anything but a length map given to dg_map_min_cover) DG_EINVAL; src from an index with another n or device DG_EINVAL; src
 * made with max_count = C > 0 and at_most >= C, whose clamped values cannot answer the test, DG_EINVAL; no device DG_ENODEV; free HBM,
 * before any kernel and with every buffer allocated first, DG_ENOMEM. */
#define DG_MAP_KIND_COUNT 0u     /* dg_mappability, dg_mappability_mm */
#define DG_MAP_KIND_LENGTH 1u    /* dg_min_unique, dg_min_unique_mm */
#define DG_MAP_KIND_COVER 2u     /* dg_map_cover */
#define DG_MAP_KIND_MIN_COVER 3u /* dg_map_min_cover */
typedef struct {
  uint32_t at_most;   /* t: a start is specific when its count is in 1..t; 1..0xFFFFFFFD */
  uint32_t max_count; /* 0 = the cover count, else min(cover, max_count) */
  uint32_t flags;     /* 0 */
  uint32_t reserved;  /* 0 */
} dg_cover_params;
typedef struct {
  uint32_t flags;    /* 0 */
  uint32_t reserved; /* 0 */
} dg_min_cover_params;
int dg_map_cover(dg_index* ix, const dg_map* src, const dg_cover_params* p, dg_map** out);
int dg_map_min_cover(dg_index* ix, const dg_map* src, const dg_min_cover_params* p, dg_map** out);
/* all zero for a map that neither call made */
typedef struct {
  uint32_t kind;            /* DG_MAP_KIND_COVER or DG_MAP_KIND_MIN_COVER */
  uint32_t k;               /* src's k, or its max_k */
  uint32_t at_most;         /* 0 for a min-cover map */
  uint32_t max_count;       /* the clamp the map was made with */
  uint64_t specific;        /* cover: starts with spec = 1; min-cover: starts with a length */
  uint64_t covered;         /* positions with a non-zero result */
  double ms_bits;           /* device time: the bitmap of spec and its rank directory (0 for a min-cover map) */
  double ms_cover;          /* device time: the per-base kernel */
  uint64_t transient_bytes; /* HBM held during the transform beside the result */
} dg_cover_stats_t;
int dg_map_cover_stats(const dg_map* m, dg_cover_stats_t* out);

/* ABI 7, additive.  Query mappability: the (k,e) counts of dg_mappability_mm for the k-mers of sequences that are NOT in the index (a
 * transcript across an exon-exon junction, a transgene, a viral genome, another allele).  Record i is seqs[off[i] .. off[i+1]), bytes
 * as given; empty records are allowed; values[off[i] + p] answers position p of record i.  For a record Q, a position p and e =
 * mismatches in 0..2:
 *   p is VALID when p + k <= len(Q) and w = Q[p, p+k) holds only A/C/G/T (case-sensitive, the rule of the text),
 *   fwd_e(p) = #{valid windows q of the TEXT : Hamming(T[q, q+k), w) <= e},   rev_e(p) = the same against revcomp(w),
 *   value(p) = fwd_e(p) + rev_e(p)   (forward_only: fwd_e(p)).
 * The windows are those dg_mappability_mm counts: A/C/G/T only, inside one sequence, never across '\n', an N or an IUPAC letter, never
 * starting before position 0.  At e = 0 the value is sdsl::count(w) + sdsl::count(revcomp(w)).  Unlike the genome track w itself is
 * in the count only when the genome holds it, so 0 IS A VALUE (absent from the genome) and invalid positions carry DG_QMAP_INVALID
 * instead; sums saturate at 0xFFFFFFFE; max_count = C > 0 writes min(value, C) (invalid stays invalid) and the search of a k-mer
 * stops once its total reaches C.  The computation runs on the handle's stream, positions in chunks of launches, and needs the query
 * bytes, 4 bytes per position and two bitmaps of free HBM (DG_ENOMEM before any kernel otherwise).  nseq = 0 succeeds and writes
 * nothing.  Checked in this order, the parameter block before the handle: a null parameter block, non-zero flags or reserved
 * DG_EINVAL; k outside 10..1000 or mismatches > 2 DG_ELIMIT; off[nseq] + nseq >= 2^31 DG_ELIMIT; a null handle, null seqs / off /
 * values (where there is something to read or write) or decreasing offsets DG_EINVAL; then DG_EINVAL while a dg_hunt_submit batch is in
 * flight on the handle.  On every failure `values` is left untouched. */
#define DG_QMAP_INVALID 0xFFFFFFFFu
typedef struct {
  uint32_t k;           /* k-mer length, 10..1000 */
  uint32_t mismatches;  /* e: 0, 1 or 2 substitutions */
  int32_t forward_only; /* fwd_e only */
  uint32_t max_count;   /* 0 = exact values, else min(value, max_count) */
  uint32_t flags;       /* 0 */
  uint32_t reserved[3]; /* 0 */
} dg_qmap_params;
typedef struct {
  uint64_t positions;     /* off[nseq] - off[0]: values written */
  uint64_t valid;         /* positions with a k-mer of A/C/G/T (the others hold DG_QMAP_INVALID) */
  uint64_t steps;         /* backward-search steps (one pair of Occ lines each, all four characters) */
  uint64_t table_reads;   /* K-mer table entries read */
  uint64_t verified_rows; /* suffix-array rows finished on the text */
  uint64_t early_exits;   /* k-mers whose search stopped at max_count */
  uint64_t launches;      /* kernel launches of the search (positions go through in chunks) */
  double ms_valid;        /* device time: upload of the queries and the valid-position bitmap */
  double ms_search;       /* device time of the search */
  double ms_total;        /* ms_valid + ms_search */
} dg_qmap_stats_t;
int dg_query_map(dg_index* ix, const dg_qmap_params* p, const uint8_t* seqs, const uint64_t* off, size_t nseq, uint32_t* values,
                 dg_qmap_stats_t* stats /* may be NULL */);

/* ABI 7, additive.  Query minimum length: how long must an oligo that starts at p of a record be before at most `at_most` places of the
 * genome are within `mismatches` substitutions of it?  Records, bytes and the layout of `values` as for dg_query_map.  For a record Q and a
 * position p:
 *   run(p)     = the number of consecutive A/C/G/T bytes of Q from p (the record's end ends a run),   limit(p) = min(run(p), max_k),
 *   value_k(p) = what dg_query_map returns at p for this k, mismatches and forward_only with max_count = 0,
 *   len(p)     = DG_QMAP_INVALID when limit(p) < min_k (no k-mer of the smallest length starts there), otherwise
 *                the smallest k in [min_k, limit(p)] with value_k(p) <= at_most, and 0 when there is none (still not specific at limit(p)).
 * at_most = 0 asks for "absent from the genome" (off-target design), at_most = 1 for "at most one place" (for a cut of the genome: unique,
 * with mismatches; dg_min_unique_mm answers that for the whole index text in one call).  value_k(p) never rises with k (a window within e of the (k+1)-mer has its
 * k-prefix within e of the k-mer; on the other strand the window one further right), so the device searches per position instead of
 * scanning every k: one call where a scan of dg_query_map needs max_k - min_k + 1.  Runs on the handle's stream, positions in chunks of
 * launches; needs the query bytes, 4 bytes per position and one bitmap of free HBM (DG_ENOMEM before any kernel otherwise).  nseq = 0
 * succeeds and writes nothing.  Checked in this order, the parameter block before the handle: a null parameter block, non-zero flags or
 * reserved DG_EINVAL; min_k or max_k outside 10..1000, min_k > max_k, mismatches > 2 or at_most > 0xFFFFFFFD DG_ELIMIT; off[nseq] + nseq
 * >= 2^31 DG_ELIMIT; no usable HIP device DG_ENODEV; a null handle, null seqs / off / values (where there is something to read or write)
 * or decreasing offsets DG_EINVAL; then DG_EINVAL while a dg_hunt_submit batch is in flight on the handle.  On every failure `values` is
 * left untouched. */
typedef struct {
  uint32_t min_k;       /* smallest length tried, 10..1000 */
  uint32_t max_k;       /* largest length tried, min_k..1000 */
  uint32_t mismatches;  /* e: 0, 1 or 2 substitutions */
  int32_t forward_only; /* count the k-mer alone, not its reverse complement */
  uint32_t at_most;     /* t: a length is specific when its value is <= t; 0..0xFFFFFFFD */
  uint32_t flags;       /* 0 */
  uint32_t reserved[2]; /* 0 */
} dg_qminlen_params;
typedef struct {
  uint64_t positions;     /* off[nseq] - off[0]: values written */
  uint64_t valid;         /* positions with limit(p) >= min_k (the others hold DG_QMAP_INVALID) */
  uint64_t found;         /* positions with a length (neither 0 nor DG_QMAP_INVALID) */
  uint64_t probes;        /* (position, k) pairs searched */
  uint64_t steps;         /* backward-search steps (one pair of Occ lines each, all four characters) */
  uint64_t table_reads;   /* K-mer table entries read */
  uint64_t verified_rows; /* suffix-array rows finished on the text */
  uint64_t launches;      /* launches of the search (positions go through in chunks) */
  double ms_valid;        /* device time: upload of the queries and the A/C/G/T bitmap */
  double ms_search;       /* device time of the search */
  double ms_total;        /* ms_valid + ms_search */
} dg_qminlen_stats_t;
int dg_query_min_len(dg_index* ix, const dg_qminlen_params* p, const uint8_t* seqs, const uint64_t* off, size_t nseq, uint32_t* values,
                     dg_qminlen_stats_t* stats /* may be NULL */);

/* ABI 7, additive.  Anchored query mappability: dg_query_map with the LAST `anchor` bases of every k-mer, the oligo's 3' end, matched
 * exactly: the places within e mismatches that a primer could extend from or a guide's seed could bind.  Records, bytes, validity,
 * DG_QMAP_INVALID, saturation, max_count, forward_only, the layout of `values` and the statistics are dg_query_map's.  For w = Q[p, p+k):
 *   fwd(p) = #{valid windows u of the text : Hamming(u, w) <= e and u[k-a, k) == w[k-a, k)}
 *   rev(p) = #{valid windows u of the text : Hamming(u, revcomp(w)) <= e and u[0, a) == revcomp(w)[0, a)}
 *   value(p) = fwd(p) + rev(p)   (forward_only: fwd(p)).
 * The anchored bases are always the last a of the oligo w; on the other strand the text shows them as the FIRST a bases of the window.
 * anchor = 0 gives dg_query_map's values, anchor = k its e = 0 values, and the value never rises with the anchor.  It is NOT monotone
 * in k for an oligo that grows at its 3' end (a site whose only mismatch is at offset k-1 is rejected at length k and accepted at
 * k+1), so dg_query_min_len has no anchor.  By END position, the 3' end fixed and the oligo growing at its 5' end, it is monotone:
 * dg_query_min_len_end below.
 * Checks, in this order: a null block, non-zero flags or reserved DG_EINVAL; k outside 10..1000, mismatches > 2 or anchor > k DG_ELIMIT;
 * off[nseq] + nseq >= 2^31 DG_ELIMIT; no device DG_ENODEV; a null handle, null seqs / off / values (where there is something to read or
 * write) or decreasing offsets DG_EINVAL; then DG_EINVAL while a dg_hunt_submit batch is in flight on the handle.  On every failure
 * `values` is left untouched. */
typedef struct {
  uint32_t k;           /* k-mer length, 10..1000 */
  uint32_t mismatches;  /* e: 0, 1 or 2 substitutions */
  uint32_t anchor;      /* a: the last a bases of the k-mer match exactly, 0..k */
  int32_t forward_only; /* non-zero: fwd(p) alone */
  uint32_t max_count;   /* 0 = exact values, else min(value, max_count) */
  uint32_t flags;       /* 0 */
  uint32_t reserved[2]; /* 0 */
} dg_qmap_anchor_params;
int dg_query_map_anchored(dg_index* ix, const dg_qmap_anchor_params* p, const uint8_t* seqs, const uint64_t* off, size_t nseq, uint32_t* values,
                          dg_qmap_stats_t* stats /* may be NULL */);

/* ABI 7, additive.  Query minimum length by END position: how far must an oligo whose 3' end is position p of a record reach back before
 * at most `at_most` places of the genome are within `mismatches` substitutions of it with its last `anchor` bases exact?  The question of
 * a primer (its 3' end), a padlock arm (its ligation junction) or a guide (its PAM-proximal end) slid along a target.  Records, bytes,
 * DG_QMAP_INVALID, forward_only and the layout of `values` are dg_query_min_len's: one uint32 per byte of every record, here at the index
 * of the oligo's LAST base.  For a record Q and a position p:
 *   brun(p)    = the number of consecutive A/C/G/T bytes of Q that end at p, p included (0 when Q[p] is none; the record's start ends a
 *                run),   limit(p) = min(brun(p), max_k),
 *   w_k        = Q[p-k+1, p+1) for k <= limit(p),
 *   value_k(p) = what dg_query_map_anchored returns at position p-k+1 for this k, mismatches, anchor and forward_only with max_count = 0,
 *   len(p)     = DG_QMAP_INVALID when limit(p) < min_k, otherwise the smallest k in [min_k, limit(p)] with value_k(p) <= at_most, and 0
 *                when there is none.
 * anchor <= min_k, so the anchored bases are the same bases Q[p-a+1, p] at every length tried; anchor = 0 is the unanchored minimum
 * length by end position.  value_k(p) never rises with k (w_{k+1} = x w_k: a window within e of w_{k+1} whose last a bases are exact has
 * its k-suffix within e of w_k with the same exact bases, one position to the right; on the other strand its k-prefix, at the same
 * start), so the device searches per position: one call where a scan of dg_query_map_anchored needs max_k - min_k + 1.  A non-zero len
 * never grows with the anchor.  Stream, chunks and memory as dg_query_min_len.  nseq = 0 succeeds and writes nothing.  Checked in this
 * order: a null parameter block, non-zero flags or reserved DG_EINVAL; min_k or max_k outside 10..1000, min_k > max_k, mismatches > 2,
 * at_most > 0xFFFFFFFD or anchor > min_k DG_ELIMIT; off[nseq] + nseq >= 2^31 DG_ELIMIT; no usable HIP device DG_ENODEV; a null handle,
 * null seqs / off / values (where there is something to read or write) or decreasing offsets DG_EINVAL; then DG_EINVAL while a
 * dg_hunt_submit batch is in flight on the handle.  On every failure `values` is left untouched. */
typedef struct {
  uint32_t min_k;       /* smallest length tried, 10..1000 */
  uint32_t max_k;       /* largest length tried, min_k..1000 */
  uint32_t mismatches;  /* e: 0, 1 or 2 substitutions */
  uint32_t anchor;      /* a: the last a bases of the oligo match exactly, 0..min_k */
  int32_t forward_only; /* count the oligo alone, not its reverse complement */
  uint32_t at_most;     /* t: a length is specific when its value is <= t; 0..0xFFFFFFFD */
  uint32_t flags;       /* 0 */
  uint32_t reserved[2]; /* 0 */
} dg_qminlen_end_params;
int dg_query_min_len_end(dg_index* ix, const dg_qminlen_end_params* p, const uint8_t* seqs, const uint64_t* off, size_t nseq, uint32_t* values,
                         dg_qminlen_stats_t* stats /* may be NULL */);

/* ABI 7, additive.  Degenerate query mappability: dg_query_map_anchored for oligos with IUPAC codes, a degenerate primer or a probe with an
 * N at a SNP site.  The letters of a record are A, C, G, T and R Y S W K M B D H V N, upper case only; U, lower case and every other byte
 * are invalid exactly as for dg_query_map.  A letter c stands for a set S(c) of bases (R = {A,G}, ... N = all four).  For w = Q[p, p+k) of
 * these 15 letters:
 *   deg(w)     = the product of |S(w_j)|,
 *   dist(u, w) = #{ j : u_j not in S(w_j) } for a window u of the text (windows are dg_query_map's: A/C/G/T only, inside one sequence,
 *                never starting before position 0; an IUPAC letter IN THE GENOME is never part of an occurrence),
 *   fwd(p)     = #{valid windows u : dist(u, w) <= e and u_j in S(w_j) for the LAST a indices j},
 *   rev(p)     = the same against revcomp(w): the complemented sets (R<->Y, K<->M, B<->V, D<->H; S, W, N themselves) in reverse order,
 *                anchored at the FIRST a indices,
 *   value(p)   = fwd(p) + rev(p)   (forward_only: fwd(p)); 0 is a value, saturation and max_count as for dg_query_map.
 * Every window counts ONCE, however many expansions of w it is within e of; a sum of dg_query_map over the expansions counts a window
 * whose base at a degenerate index lies outside the set several times when e > 0.  value(p) = DG_QMAP_INVALID where no k-mer of the 15
 * letters starts at p and where deg(w) > max_degeneracy (counted in too_degenerate, not in valid).  On records of A/C/G/T only every
 * value and the counters valid, steps, table_reads and verified_rows are those of dg_query_map_anchored.  k is 10..64 here: an
 * expansion's state is a few 64-bit words of registers.  max_degeneracy is 1..4096, 0 = 256.
 * Checks, in this order: a null block, non-zero flags or reserved DG_EINVAL; k outside 10..64, mismatches > 2, anchor > k or
 * max_degeneracy > 4096 DG_ELIMIT; off[nseq] + nseq >= 2^31 DG_ELIMIT; no device DG_ENODEV; a null handle, null seqs / off / values
 * (where there is something to read or write) or decreasing offsets DG_EINVAL; then DG_EINVAL while a dg_hunt_submit batch is in flight
 * on the handle.  On every failure `values` is left untouched. */
typedef struct {
  uint32_t k;              /* k-mer length, 10..64 */
  uint32_t mismatches;     /* e: 0, 1 or 2 letters of the window outside the k-mer's sets */
  uint32_t anchor;         /* a: the last a letters of the k-mer take no mismatch, 0..k */
  int32_t forward_only;    /* non-zero: fwd(p) alone */
  uint32_t max_count;      /* 0 = exact values, else min(value, max_count) */
  uint32_t max_degeneracy; /* k-mers with more expansions are not searched; 1..4096, 0 = 256 */
  uint32_t flags;          /* 0 */
  uint32_t reserved[3];    /* 0 */
} dg_qmap_iupac_params;
typedef struct {
  uint64_t positions;      /* off[nseq] - off[0]: values written */
  uint64_t valid;          /* positions with a k-mer of the 15 letters and deg <= max_degeneracy (the others hold DG_QMAP_INVALID) */
  uint64_t steps;          /* as dg_qmap_stats_t, summed over the expansions */
  uint64_t table_reads;
  uint64_t verified_rows;
  uint64_t early_exits;    /* k-mers whose search stopped at max_count */
  uint64_t launches;
  uint64_t too_degenerate; /* positions with a k-mer of the 15 letters and deg > max_degeneracy */
  uint64_t degenerate;     /* valid positions with deg > 1 */
  uint64_t expansions;     /* searches started: one per expansion and strand */
  double ms_valid;
  double ms_search;
  double ms_total;         /* ms_valid + ms_search */
} dg_qmap_iupac_stats_t;
int dg_query_map_iupac(dg_index* ix, const dg_qmap_iupac_params* p, const uint8_t* seqs, const uint64_t* off, size_t nseq, uint32_t* values,
                       dg_qmap_iupac_stats_t* stats /* may be NULL */);

const char* dg_last_error(void);
int dg_abi_version(void);
int dg_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
