// dicey_amd/csrc/probe_schedule.hpp on the host, a program of its own (tests/test_min_unique_mm_host.py builds and runs it, once plainly and
// once with -fsanitize=address,undefined): for every bracket (lo, hi] of up to 200 lengths and every threshold in it, the schedule finds
// the smallest passing length exactly, asks only lengths inside the bracket, never the same one twice, and stays within the probe
// bound its own shape gives (the header has the derivation):
//   nothing passes            1 probe, the one at hi
//   the answer is lo + x      at most 2 ceil(log2(x + 1)) probes, and at most 1 + floor(log2(D)) + ceil(log2(D)) with D = hi - lo
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../dicey_amd/csrc/probe_schedule.hpp"

static uint32_t ceil_log2(uint32_t v) {  // v >= 1
  uint32_t r = 0;
  while ((1u << r) < v) ++r;
  return r;
}
static uint32_t floor_log2(uint32_t v) {  // v >= 1
  uint32_t r = 0;
  while ((2u << r) <= v) ++r;
  return r;
}

int main() {
  unsigned long long cases = 0, total_probes = 0;
  uint32_t worst = 0;
  for (uint32_t lo : {0u, 1u, 9u, 799u}) {
    for (uint32_t d = 1; d <= 200; ++d) {
      const uint32_t hi = lo + d;
      // threshold th: lengths >= th pass; th = hi + 1: nothing does
      for (uint32_t th = lo + 1; th <= hi + 1; ++th) {
        dg::ProbeSchedule s = dg::probe_begin(lo, hi);
        std::vector<char> asked(d + 1, 0);
        uint32_t probes = 0;
        do {
          const uint32_t k = dg::probe_next(s);
          if (k <= lo || k > hi || asked[k - lo]) {
            std::printf("FAIL lo=%u hi=%u th=%u: probe %u at k=%u outside the bracket or repeated\n", lo, hi, th, probes, k);
            return 1;
          }
          asked[k - lo] = 1;
          ++probes;
          if (probes > 64) {
            std::printf("FAIL lo=%u hi=%u th=%u: no end\n", lo, hi, th);
            return 1;
          }
          dg::probe_update(s, k, k >= th);
        } while (!dg::probe_done(s));
        const uint32_t want = th <= hi ? th : 0u, got = dg::probe_answer(s);
        uint32_t bound = 1;
        if (want) {
          const uint32_t by_answer = 2 * ceil_log2(want - lo + 1), by_bracket = 1 + floor_log2(d) + ceil_log2(d);
          bound = by_answer < by_bracket ? by_answer : by_bracket;
          if (bound < 1) bound = 1;
        }
        if (got != want || probes > bound) {
          std::printf("FAIL lo=%u hi=%u th=%u: answer %u (want %u) after %u probes (bound %u)\n", lo, hi, th, got, want, probes, bound);
          return 1;
        }
        ++cases;
        total_probes += probes;
        if (probes > worst) worst = probes;
      }
    }
  }
  std::printf("ok %llu cases, %llu probes, worst %u\n", cases, total_probes, worst);
  return 0;
}
