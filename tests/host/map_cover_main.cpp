// The arithmetic of dicey_amd/csrc/map_cover.hpp on the host: the window count over a bitmap with a rank directory and the backward walk
// over staged cells, fed from standard input by tests/test_cover_host.py, which holds the answers against tests/cover_ref.py.
//   count NBITS K      then a line of NBITS characters 0 / 1: prints cover_count of every position
//   walk NCELL MAX_K   then NCELL integers, -1 = not A/C/G/T, else the length of the source map (0 = none): prints cover_walk of every cell
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../../dicey_amd/csrc/map_cover.hpp"

int main() {
  std::string what;
  unsigned long long n = 0;
  unsigned k = 0;
  while (std::cin >> what >> n >> k) {
    std::string line;
    if (what == "count") {
      std::string bits;
      std::cin >> bits;
      if (bits.size() != n) return 2;
      const size_t nw = (n + 63) / 64 + 1;
      std::vector<uint64_t> words(nw, 0);
      for (size_t p = 0; p < n; ++p)
        if (bits[p] == '1') words[p >> 6] |= 1ULL << (p & 63);
      std::vector<uint32_t> dir(nw, 0);  // the exclusive scan of the words' popcounts
      for (size_t w = 1; w < nw; ++w) dir[w] = dir[w - 1] + (uint32_t)__builtin_popcountll(words[w - 1]);
      for (size_t p = 0; p < n; ++p) line += std::to_string(dg::cover_count(dir.data(), words.data(), p, k)) + ' ';
    } else if (what == "walk") {
      std::vector<uint16_t> cells(n);
      for (size_t p = 0; p < n; ++p) {
        long v = 0;
        if (!(std::cin >> v)) return 2;
        cells[p] = v < 0 ? dg::cover_cell(0, false) : dg::cover_cell((uint32_t)v, true);
      }
      for (size_t p = 0; p < n; ++p) line += std::to_string(dg::cover_walk(cells.data(), (uint32_t)p, k)) + ' ';
    } else {
      return 2;
    }
    std::puts(line.c_str());
  }
  return 0;
}
