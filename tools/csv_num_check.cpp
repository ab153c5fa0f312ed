// csv_num_check.cpp -- stand-alone CPU checker of csrc/knn_csv_num.h (the CSV
// reader's fast decimal conversion, shared with the device kernel).
//
// Every token is converted by csv_fast_atof / csv_fast_atoi on a buffer that
// holds exactly the token's bytes (no terminator: a read past the end is a
// heap overflow the sanitizers see) and by atof / atoi on a NUL-terminated
// copy.  Every `true` must carry atof's / atoi's bits.  Tokens: the tricky
// list of tests/test_csv_parse.py, boundary cases, and 3.2 million generated
// tokens from a fixed seed.  Prints the share of tokens per tier and per
// generator, "N mismatches", and exits non-zero on a mismatch or when a
// condition on the slow share fails:
//   integers 0..255 and k/256 grid values: no slow token (tier 1's rule);
//   %.17g of standard normals: at most 1 % slow (the Eisel-Lemire fallback is
//   rare by construction; a share near the cap means a wrong table).
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "knn_csv_num.h"

namespace {

knncsv::NumTable g_tab;
long long g_mismatch = 0;

struct Tally {
  const char* name;
  long long n = 0, tier[4] = {0, 0, 0, 0};
};

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double uniform01() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
double normal() {
  const double u = 1.0 - uniform01(), v = uniform01();
  return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v);
}

void check_atof(const std::string& s, Tally& t) {
  std::vector<char> exact(s.begin(), s.end());  // exactly the token's bytes
  const char* b = exact.data();
  double got = 0;
  int tier = 0;
  const bool ok = knncsv::csv_fast_atof(b, b + exact.size(), &g_tab, &got, &tier);
  ++t.n;
  ++t.tier[ok ? tier : 0];
  if (!ok) return;
  const double want = atof(s.c_str());
  if (memcmp(&got, &want, sizeof got) != 0) {
    uint64_t g, w;
    memcpy(&g, &got, 8);
    memcpy(&w, &want, 8);
    if (++g_mismatch <= 20)
      printf("MISMATCH atof \"%s\": tier %d gave %016" PRIx64 ", atof %016" PRIx64 "\n", s.c_str(),
             tier, g, w);
  }
}

void check_atoi(const std::string& s, Tally& t) {
  std::vector<char> exact(s.begin(), s.end());
  const char* b = exact.data();
  int32_t got = 0;
  const bool ok = knncsv::csv_fast_atoi(b, b + exact.size(), &got);
  ++t.n;
  ++t.tier[ok ? 1 : 0];
  if (ok && got != atoi(s.c_str())) {
    if (++g_mismatch <= 20) printf("MISMATCH atoi \"%s\": %d, atoi %d\n", s.c_str(), got, atoi(s.c_str()));
  }
}

void report(const Tally& t) {
  const double n = t.n ? (double)t.n : 1.0;
  printf("%-22s %9lld tokens: slow %8.4f %%  zero %8.4f %%  tier1 %8.4f %%  tier2 %8.4f %%\n", t.name,
         t.n, 100.0 * t.tier[0] / n, 100.0 * t.tier[1] / n, 100.0 * t.tier[2] / n,
         100.0 * t.tier[3] / n);
}

std::string fmt(const char* f, double v) {
  char buf[512];
  snprintf(buf, sizeof buf, f, v);
  return buf;
}

}  // namespace

int main() {
  knncsv::csv_build_num_table(&g_tab);
  int failed = 0;

  // the tricky list of tests/test_csv_parse.py
  const char* tricky[] = {"0.1", "-0.0", "1e-310", "  5.5", "+3", "0x1p-3", "inf", "-INF", "nan",
                          "1.5abc", "", ".5", "5.", "1e400", "4.9e-324", "-7",
                          "0.30000000000000004", "123456789012345678901", "  -2.5e+3", "1E5",
                          "abc", "0000.25"};
  const char* boundary[] = {"9007199254740992", "9007199254740993", "1.7976931348623157e308",
                            "2.2250738585072014e-308", "4.9e-324", "1e23", "8.5e-23",
                            "0.30000000000000004", "1e22", "1e-22", "9999999999999999999",
                            "99999999999999999999", "-0", "-0.0", "0e999", "5.", ".5", "-.5",
                            // the grammar's edges
                            ".", "-", "-.", "1e", "1e+", "1e-", "e5", "1.5\r", "1.5 ", "1,5", "--1",
                            "1e5.5", "0.0000000000000000000000000001", "1e-342", "1e-343", "1e308",
                            "1e309", "17976931348623158e292", "00000000000000000000001",
                            "1.00000000000000000000", "123456789", "1234567890", "-123456789",
                            "-1234567890", "2147483648", "007", "-", "3.0", " 7", "12345678901"};
  Tally tl{"tricky + boundary"}, ti{"atoi on the same"};
  for (const char* s : tricky) check_atof(s, tl), check_atoi(s, ti);
  for (const char* s : boundary) check_atof(s, tl), check_atoi(s, ti);
  report(tl);
  report(ti);
  // what the fixed cases must decide
  {
    double v;
    const auto fast = [&](const char* s) {
      return knncsv::csv_fast_atof(s, s + strlen(s), &g_tab, &v);
    };
    const char* must_slow[] = {"  5.5", "+3", "0x1p-3", "inf", "-INF", "nan", "1.5abc", "", ".",
                               "1e", "1.5\r", "99999999999999999999", "4.9e-324", "1e400"};
    for (const char* s : must_slow)
      if (fast(s)) printf("FAIL: \"%s\" must be slow\n", s), ++failed;
    const char* must_fast[] = {"0.1", "-0.0", ".5", "5.", "-.5", "1E5", "0000.25", "0e999", "-0",
                               "9007199254740993", "1e23", "8.5e-23", "9999999999999999999",
                               "1.7976931348623157e308"};
    for (const char* s : must_fast)
      if (!fast(s)) printf("FAIL: \"%s\" must be converted\n", s), ++failed;
  }

  const long long per = 400000;  // tokens per generator (8 generators: 3.2M)
  char buf[64];
  Tally g1{"integers 0..255"}, g2{"k/256 as %.8f"}, g3{"%.17g of normals"}, g4{"%.9g of normals"},
      g5{"%.6f of normals"}, g6{"%.17g of random bits"}, g7{"%de%d"}, g8{"atoi: labels"};
  for (long long i = 0; i < per; ++i) {
    snprintf(buf, sizeof buf, "%d", (int)(rnd() % 256));
    check_atof(buf, g1);
    check_atof(fmt("%.8f", (double)(rnd() % 256) / 256.0), g2);  // bench.write_grid_csv's form
    const double x = normal();
    check_atof(fmt("%.17g", x), g3);
    check_atof(fmt("%.9g", x), g4);
    check_atof(fmt("%.6f", x), g5);
    double r;
    do {
      const uint64_t bits = rnd();
      memcpy(&r, &bits, 8);
    } while (!std::isfinite(r));
    check_atof(fmt("%.17g", r), g6);
    {  // 1..19 digit significand, exponent in [-350, 320]
      const int nd = 1 + (int)(rnd() % 19);
      std::string s;
      for (int k = 0; k < nd; ++k) s += (char)('0' + (k == 0 ? 1 + rnd() % 9 : rnd() % 10));
      snprintf(buf, sizeof buf, "e%d", (int)(rnd() % 671) - 350);
      check_atof(s + buf, g7);
    }
    snprintf(buf, sizeof buf, "%lld", (long long)(rnd() % 4000000000ull) - 2000000000ll);
    check_atoi(buf, g8);
  }
  for (const Tally* t : {&g1, &g2, &g3, &g4, &g5, &g6, &g7, &g8}) report(*t);
  if (g1.tier[0] || g2.tier[0]) printf("FAIL: slow tokens among tier 1's generators\n"), ++failed;
  if (g3.tier[0] * 100 > g3.n) printf("FAIL: more than 1 %% slow among %%.17g normals\n"), ++failed;
  printf("%lld tokens checked\n%lld mismatches\n",
         tl.n + ti.n + g1.n + g2.n + g3.n + g4.n + g5.n + g6.n + g7.n + g8.n, g_mismatch);
  return (g_mismatch || failed) ? 1 : 0;
}
