// Development and test switches of the library, in ONE place (r06).
//
// The product library (dicey_amd/libdiceygpu.so, `make`) has one behaviour: exp_env() is a constant nullptr there and every branch
// behind it is compiled out.  What it still reads from the environment is deployment, not behaviour: DICEY_TIMING (phase times on
// stderr), DICEY_HOST_THREADS, DICEY_CAP_BUDGET_MB, DICEY_KMER_K / DICEY_KMER_K2 (table and filter orders: tuning knobs, also how the
// tests give a 30 kb genome a table at all) and DICEY_FM9_HASH (the builder's stamp).
//
// A development build (`tools/build_variant.sh exp -DDG_EXPERIMENTS` -> dicey_amd/variants/libdiceygpu_exp.so; tests/conftest.py builds
// it when missing) reads the switches below.  They FORCE code paths the product takes by itself when the data asks for them — the
// search without the select stage inside (strings above 42 characters), the full-matrix verify (queries above 32 nt), the host
// enumerator of capped neighbourhoods (sequences with N), tiny buffer capacities (the retry path), an index without one of the
// derived layouts (a device short of memory) ... — so that the GPU suite can hold every path against the checker on the same
// small inputs (tests/test_gpu_parity.py SWITCHES), and a few measurement aids whose results are deliberately wrong (DICEY_EXP).
//   hunt.hip      DICEY_NO_BAND_VERIFY DICEY_CAP_HOST DICEY_NO_FUSED_SELECT DICEY_NO_FUSED_SELECT2 DICEY_NO_PREP_FUSION DICEY_NO_PRE5_D2
//                 DICEY_NO_FLAT_HAMMING2 DICEY_NO_N_WINDOW DICEY_NO_LONG2 DICEY_NO_DIRECT_CTX DICEY_DEBUG_CAPS DICEY_FUSED_LCAP DICEY_VERIFY_CH DICEY_DUMP_JOBS DICEY_EXP
//   index.hip     DICEY_NO_KMER_FILTER DICEY_NO_NRUN_PRUNE DICEY_NO_PRE5 DICEY_NO_SAX DICEY_NO_PLV DICEY_NO_SA_MINIMA DICEY_EXP_PRIO
//   mappability.hip   DICEY_MAP_CHUNK (positions per dg_map_runs pass) DICEY_MAP_HEAD_CHUNK (ranks per launch of the e >= 1 search, of dg_min_unique and of dg_min_unique_mm)
//                 DICEY_MAP_NARROW (W: intervals of at most W rows are verified on the text; 0 = never) DICEY_QMAP_CHUNK (positions per launch
//                 of dg_query_map) DICEY_QMINLEN_CHUNK (positions per launch of dg_query_min_len) DICEY_MU_MM_RANK_ORDER (dg_min_unique_mm: lanes by rank
//                 instead of by text position) DICEY_COVER_TILE (positions per k_min_cover workgroup tile, 1..2048) -- results do not depend on them
//   search.hip / thal_api.hip   DICEY_NO_LDS_TABLES DICEY_NO_WAVE_THAL DICEY_DEBUG_THAL_REDO DICEY_DEBUG_DUMP_RAW
//
// A development build also exports ONE function the header does not declare (index.hip, next to its struct dgx_layout_info):
//   int dgx_index_layout(dg_index*, uint32_t what, uint32_t level, void* host_out, uint64_t cap_bytes, dgx_layout_info* info)
// synchronises the handle's stream, copies at most cap_bytes of one derived layout to the host — what: 0 occ, 1 text, 2 sa, 3 ktab,
// 4 / 5 copy `level` of kf / kf2, 6 pre5, 7 sax, 8 / 9 directory / records of prefix level `level`, 10 block minima of level `level` >= 1
// — and fills info: the layout's bytes without allocation slack (0 = the handle does not have it: not an error), and FmView's scalars
// (n, C4, K, nrun_min, nlev, nplv, the level's x, each filter's k / nr / s / pick, whether pre5 / sax are null).  host_out == NULL: info
// only.  tests/test_gpu_index_layout.py holds every entry of every layout against tests/index_layout_ref.py through it.
#pragma once
#include <cstdlib>

namespace dg {
#ifdef DG_EXPERIMENTS
inline const char* exp_env(const char* name) { return std::getenv(name); }
#else
inline const char* exp_env(const char*) { return nullptr; }
#endif
}  // namespace dg
