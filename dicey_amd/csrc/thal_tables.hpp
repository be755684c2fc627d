// Host only: primer3's parameter files -> thal::Tables, the three constants that depend on the salt / DNA settings, and the
// per-oligo preparation of dg_thal_batch (base codes, the symmetry test).
// dg_thal_open (thal_api.hip) and the CPU test build of thal.hpp (tests/host/thal_host.cpp) both include this file, so the
// tests check the loader and the arithmetic the product runs, not a copy of them.
#pragma once
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "thal.hpp"

namespace dg {
namespace thal {

enum { kLoadOk = 0, kLoadIo = 1, kLoadFormat = 2 };  // load_tables: files missing / too short (`err` says which)

// one value per line, possibly "inf" (thal.h:403-414)
struct ValueFile {
  std::ifstream f;
  bool ok;
  explicit ValueFile(const std::string& p) : f(p.c_str()), ok(f.good()) {}
  bool line(std::string& s) { return (bool)std::getline(f, s); }
  double next() {
    std::string s;
    if (!line(s)) {
      ok = false;
      return 0;
    }
    size_t k = 0;
    while (k < s.size() && std::isspace((unsigned char)s[k])) ++k;
    if (s.compare(k, 3, "inf") == 0) return kInf;
    return std::strtod(s.c_str() + k, nullptr);
  }
};
inline double field(const std::string& tok) { return tok == "inf" ? kInf : std::strtod(tok.c_str(), nullptr); }

// dir ends with '/'
inline int load_tables(const std::string& dir, Tables& t, std::string& err) {
  auto quad = [&](const char* sname, const char* hname, double S[5][5][5][5], double H[5][5][5][5], bool terminal) -> int {
    ValueFile fs(dir + sname), fh(dir + hname);
    if (!fs.ok || !fh.ok) {
      err = "cannot read " + dir + sname + " / " + hname;
      return kLoadIo;
    }
    for (int i = 0; i < 5; ++i)
      for (int ii = 0; ii < 5; ++ii)
        for (int j = 0; j < 5; ++j)
          for (int jj = 0; jj < 5; ++jj) {
            if (!terminal) {  // getStack / getStackint2 (thal.h:497-555)
              if (i == 4 || j == 4 || ii == 4 || jj == 4) {
                S[i][ii][j][jj] = -1.0;
                H[i][ii][j][jj] = kInf;
                continue;
              }
            } else {  // getTstack / getTstack2 (thal.h:622-679)
              if (i == 4 || j == 4) {
                H[i][ii][j][jj] = kInf;
                S[i][ii][j][jj] = -1.0;
                continue;
              }
              if (ii == 4 || jj == 4) {
                S[i][ii][j][jj] = 0.00000000001;
                H[i][ii][j][jj] = 0.0;
                continue;
              }
            }
            S[i][ii][j][jj] = fs.next();
            H[i][ii][j][jj] = fh.next();
            if (!fin(S[i][ii][j][jj]) || !fin(H[i][ii][j][jj])) {
              S[i][ii][j][jj] = -1.0;
              H[i][ii][j][jj] = kInf;
            }
          }
    if (!fs.ok || !fh.ok) {
      err = dir + sname + " / " + hname + " are too short";
      return kLoadFormat;
    }
    return kLoadOk;
  };
  int rc;
  if ((rc = quad("stack.ds", "stack.dh", t.stackS, t.stackH, false)) != kLoadOk) return rc;
  if ((rc = quad("stackmm.ds", "stackmm.dh", t.stackmmS, t.stackmmH, false)) != kLoadOk) return rc;
  {  // getDangle (thal.h:558-604): 3' block then 5' block in the same files
    ValueFile fs(dir + "dangle.ds"), fh(dir + "dangle.dh");
    if (!fs.ok || !fh.ok) {
      err = "cannot read " + dir + "dangle.ds/.dh";
      return kLoadIo;
    }
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 5; ++j)
        for (int k = 0; k < 5; ++k) {
          if (i == 4 || j == 4 || k == 4) {
            t.dangle3S[i][k][j] = -1.0;
            t.dangle3H[i][k][j] = kInf;
          } else {
            t.dangle3S[i][k][j] = fs.next();
            t.dangle3H[i][k][j] = fh.next();
            if (!fin(t.dangle3S[i][k][j]) || !fin(t.dangle3H[i][k][j])) {
              t.dangle3S[i][k][j] = -1.0;
              t.dangle3H[i][k][j] = kInf;
            }
          }
        }
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 5; ++j)
        for (int k = 0; k < 5; ++k) {
          if (i == 4 || j == 4 || k == 4) {
            t.dangle5S[i][j][k] = -1.0;
            t.dangle5H[i][j][k] = kInf;
          } else {
            t.dangle5S[i][j][k] = fs.next();
            t.dangle5H[i][j][k] = fh.next();
            if (!fin(t.dangle5S[i][j][k]) || !fin(t.dangle5H[i][j][k])) {
              t.dangle5S[i][j][k] = -1.0;
              t.dangle5H[i][j][k] = kInf;
            }
          }
        }
    if (!fs.ok || !fh.ok) {
      err = dir + "dangle.ds/.dh are too short";
      return kLoadFormat;
    }
  }
  {  // getLoop (thal.h:606-620): "<size> <interior> <bulge> <hairpin>" per line, 30 lines
    ValueFile fs(dir + "loops.ds"), fh(dir + "loops.dh");
    if (!fs.ok || !fh.ok) {
      err = "cannot read " + dir + "loops.ds/.dh";
      return kLoadIo;
    }
    for (int k = 0; k < 30; ++k) {
      std::string ls, lh, a, b, c, d;
      if (!fs.line(ls) || !fh.line(lh)) {
        err = dir + "loops.ds/.dh are too short";
        return kLoadFormat;
      }
      std::istringstream ss(ls), sh(lh);
      ss >> a >> b >> c >> d;
      t.interiorS[k] = field(b);
      t.bulgeS[k] = field(c);
      sh >> a >> b >> c >> d;
      t.interiorH[k] = field(b);
      t.bulgeH[k] = field(c);
    }
  }
  if ((rc = quad("tstack_tm_inf.ds", "tstack.dh", t.tstackS, t.tstackH, true)) != kLoadOk) return rc;
  if ((rc = quad("tstack2.ds", "tstack2.dh", t.tstack2S, t.tstack2H, true)) != kLoadOk) return rc;
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j) {  // tableStartATS / tableStartATH (thal.h:767-783), AT_S = 6.9, AT_H = 2200
      t.atpS[i][j] = 0.00000000001;
      t.atpH[i][j] = 0.0;
    }
  t.atpS[0][3] = t.atpS[3][0] = 6.9;
  t.atpH[0][3] = t.atpH[3][0] = 2200.0;
  return kLoadOk;
}

// saltCorrectS (thal.h:354-359) and the two RC values (thal.h:2504-2508)
inline Env make_env(double mv, double dv, double dntp, double dna_conc) {
  Env env;
  double dn = dntp;
  if (dv <= 0) dn = dv;
  env.salt_correction = 0.368 * ((log((mv + 120 * (sqrt(fmax(0.0, dv - dn)))) / 1000)));
  env.rc_sym = 1.9872 * log(dna_conc / 1000000000.0);
  env.rc_asym = 1.9872 * log(dna_conc / 4000000000.0);
  return env;
}

inline uint8_t code_of(char c) {
  c = (char)std::toupper((unsigned char)c);
  return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;  // str2int, thal.h:260-275
}
// symmetry_thermo (thal.h:1976-2010): even length and self-complementary
inline bool self_complementary(const uint8_t* s, size_t n) {
  if (n % 2) return false;
  for (size_t i = 0; i < n / 2; ++i) {
    char a = (char)std::toupper(s[i]), b = (char)std::toupper(s[n - 1 - i]);
    if ((a == 'A' && b != 'T') || (a == 'T' && b != 'A') || (b == 'A' && a != 'T') || (b == 'T' && a != 'A')) return false;
    if ((a == 'C' && b != 'G') || (a == 'G' && b != 'C') || (b == 'C' && a != 'G') || (b == 'G' && a != 'C')) return false;
  }
  return true;
}

}  // namespace thal
}  // namespace dg
