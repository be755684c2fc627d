// Host build of the product's sequential thal formulation (dicey_amd/csrc/thal.hpp: end1_tm, as k_thal and k_site run it) with the
// product's table loader and environment arithmetic (thal_tables.hpp, as dg_thal_open runs them), for the CPU test suite.
#include <cstdint>
#include <string>
#include <vector>

static thread_local unsigned long long g_cutoff_wins = 0;
#define DG_THAL_CUTOFF_WIN() (++g_cutoff_wins)  // openings whose candidate wins with S < -2500 (thal.h:1322-1330)
#include "../../dicey_amd/csrc/thal_tables.hpp"

using namespace dg;

struct Handle {
  thal::Tables tables;
  thal::Env env;
  std::vector<uint8_t> a, b;
  std::vector<thal::Cell> cells;
};

extern "C" {

// config_dir as dg_thal_open takes it; nullptr when the tables cannot be read
void* thal_host_open(const char* config_dir, double mv, double dv, double dntp, double dna_conc) {
  std::string dir(config_dir);
  if (!dir.empty() && dir.back() != '/') dir.push_back('/');
  Handle* h = new Handle;
  std::string err;
  if (thal::load_tables(dir, h->tables, err) != thal::kLoadOk) {
    delete h;
    return nullptr;
  }
  h->env = thal::make_env(mv, dv, dntp, dna_conc);
  return h;
}
void thal_host_close(void* hv) { delete static_cast<Handle*>(hv); }

// pairs laid out as dg_thal_batch takes them: oligo 1 of pair k at seqs[off[2k] .. off[2k+1]), oligo 2 behind it.
// cutoff_wins (may be null): per pair, the number of entropy cut-off candidates that won.
void thal_host_batch(void* hv, const uint8_t* seqs, const uint64_t* off, uint64_t npairs, double* temp, int32_t* end1, int32_t* end2,
                     uint64_t* cutoff_wins) {
  Handle* h = static_cast<Handle*>(hv);
  for (uint64_t k = 0; k < npairs; ++k) {
    const uint8_t* s1 = seqs + off[2 * k];
    const uint8_t* s2 = seqs + off[2 * k + 1];
    const uint64_t l1 = off[2 * k + 1] - off[2 * k], l2 = off[2 * k + 2] - off[2 * k + 1];
    h->a.assign(l1 + 2, 4);
    h->b.assign(l2 + 2, 4);
    for (uint64_t i = 0; i < l1; ++i) h->a[1 + i] = thal::code_of((char)s1[i]);
    for (uint64_t j = 0; j < l2; ++j) h->b[1 + j] = thal::code_of((char)s2[l2 - 1 - j]);  // reversed
    const bool sym = thal::self_complementary(s1, l1) && thal::self_complementary(s2, l2);
    const bool both_long = l1 > (uint64_t)thal::kMaxAlign && l2 > (uint64_t)thal::kMaxAlign;
    h->cells.resize(both_long ? 1 : l1 * l2 + 1);
    const uint8_t* pa = h->a.data();
    const uint8_t* pb = h->b.data();
    g_cutoff_wins = 0;
    const thal::Result r = thal::end1_tm<const uint8_t*>(h->tables, h->env, pa, (int)l1, pb, (int)l2, sym, h->cells.data());
    temp[k] = r.temp;
    end1[k] = r.end1;
    end2[k] = r.end2;
    if (cutoff_wins) cutoff_wins[k] = g_cutoff_wins;
  }
}

}  // extern "C"
