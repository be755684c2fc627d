// The order in which a lane probes lengths k for the smallest one that passes, as pure arithmetic: shared by the device kernel k_mu_mm
// (min_unique_mm.hpp) and by a host program (tests/host/probe_schedule_main.cpp) that runs it against every bracket and threshold.
//
// "k passes" is monotone: false up to some k, true from there on (query_min_len.hpp has the argument for the mismatch counts).  The
// caller knows a length `lo` that fails (or below which nothing is asked) and the largest length `hi` that may be asked at all:
//   first    hi itself.  A fail ends the search with no answer (0): nothing up to the limit passes.
//   gallop   then lo + 1, lo + 1 + 2, lo + 1 + 2 + 4, ... while the probe stays below hi: a fail moves lo there and doubles the step, a
//            pass moves hi there.  The answers sit a few characters above lo, far from hi.
//   bisect   once lo + step reaches hi, the middle of the bracket, until hi - lo == 1: hi is the answer.
// With the answer at lo + x (x >= 1) that is at most 2 ceil(log2(x + 1)) probes, the first one included: j = ceil(log2(x + 1)) is the
// first gallop probe (at lo + 2^j - 1) that passes; it leaves a bracket of 2^(j-1) lengths, j - 1 bisections.  Where hi comes before
// that probe the gallop is one probe shorter, the bracket no wider, and the probe at hi has been paid for either way.
// k_qminlen and k_qminlen_end (query_min_len.hpp, query_min_len_end.hpp) carry the same loop written out.
#pragma once
#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DG_PS __host__ __device__ __forceinline__
#else
#define DG_PS inline
#endif

namespace dg {

struct ProbeSchedule {
  uint32_t lo, hi;  // lo fails (or is below every length asked), hi passes once the first probe has
  uint32_t step;    // 0 marks the first probe, at hi
};

// lo < hi: lengths lo + 1 .. hi are candidates
DG_PS ProbeSchedule probe_begin(uint32_t lo, uint32_t hi) { return ProbeSchedule{lo, hi, 0u}; }

// the length to probe next (only while !probe_done)
DG_PS uint32_t probe_next(const ProbeSchedule& s) {
  if (s.step == 0) return s.hi;
  return s.lo + s.step < s.hi ? s.lo + s.step : s.lo + (s.hi - s.lo) / 2;  // the gallop while it stays below hi, then the bisection
}

// what the probe of k = probe_next(s) gave
DG_PS void probe_update(ProbeSchedule& s, uint32_t k, bool pass) {
  if (s.step == 0) {
    s.step = 1;
    if (!pass) s.lo = s.hi = 0;  // still failing at the limit: no answer
  } else if (pass) {
    s.hi = k;
  } else {
    s.lo = k;
    s.step <<= 1;
  }
}

DG_PS bool probe_done(const ProbeSchedule& s) { return s.step != 0 && s.hi - s.lo <= 1; }

// once done: the smallest length that passes, 0 when none does
DG_PS uint32_t probe_answer(const ProbeSchedule& s) { return s.hi; }

}  // namespace dg
