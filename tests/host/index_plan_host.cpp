// Test harness (not part of the product): the rules an index open decides by (dicey_amd/csrc/index_plan.hpp) behind a C interface, so
// that `pytest -m "not gpu"` can hold them against a model (tests/test_index_plan_host.py).
#include "../../dicey_amd/csrc/index_plan.hpp"

using namespace dg::plan;
typedef unsigned long long W;

extern "C" {

unsigned ip_big_table_flag() { return DG_OPEN_BIG_TABLE; }
unsigned ip_max_levels() { return MAXPLV; }

void ip_table_orders(W n, int have_mem, W free_b, unsigned flags, int env_k, int env_k2_set, int env_k2, int no_filter, unsigned* K, unsigned* K2) {
  TableFacts t;
  t.n = n;
  t.have_mem = have_mem != 0;
  t.free_b = free_b;
  t.flags = flags;
  t.env_k = env_k;
  t.env_k2_set = env_k2_set != 0;
  t.env_k2 = env_k2;
  t.no_filter = no_filter != 0;
  const TableOrders o = table_orders(t);
  *K = o.K;
  *K2 = o.K2;
}
int ip_sax_fits(W n, int have_mem, W free_b) { return sax_fits(n, have_mem != 0, free_b) ? 1 : 0; }
int ip_plv_level_fits(W n, W x, int have_mem, W free_b) { return plv_level_fits(n, x, have_mem != 0, free_b) ? 1 : 0; }
int ip_plv_sizes(W n, W* out, int cap) {
  const std::vector<u64> xs = plv_sizes(n);
  for (int i = 0; i < (int)xs.size() && i < cap; ++i) out[i] = xs[i];
  return (int)xs.size();
}
// the byte sizes, in the order of SIZES in the test
W ip_bytes(int which, W v) {
  switch (which) {
    case 0: return occ_blocks(v) * 64;
    case 1: return text_bytes(v);
    case 2: return sa_bytes(v);
    case 3: return table_bytes((u32)v);
    case 4: return filter_copy_bytes((u32)v);
    case 5: return pre5_bytes(v);
    case 6: return sax_bytes(v);
    case 7: return plv_dir_bytes(v);
    case 8: return plv_rec_bytes(v);
  }
  return 0;
}

}  // extern "C"
