// cert_rules_check.cpp — the certificate's rules (simgrid_amd/csrc/lmm_cert.hpp) against the comparisons
// System::check_certificate wrote out before the header existed, kept here literally (old_*), over inputs on both
// sides of every threshold: bounds that are not judged, usages one ulp either side of bound * (1 +- prec), values one
// ulp either side of bound +- max(prec, 1e-9 bound), levels one ulp either side of top * (1 - 1e-9).  Prints "ok N".
// (tests/test_cert_rules.py)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../simgrid_amd/csrc/lmm_cert.hpp"

static bool old_judged(double b, double prec) { return b > b * prec; }
static bool old_infeasible(double usage, double b, double prec) { return usage - b > b * prec; }
static bool old_sat(double usage, double b, double prec) { return !(b - usage > b * prec); }
static double old_excess(double usage, double b) { return (usage - b) / b; }
static bool old_at_bound(double rv, double bound, double prec) {
  return bound > 0 && std::fabs(rv - bound) <= std::max(prec, 1e-9 * bound);
}
static bool old_carries(double lvl, double top) { return lvl >= top * (1 - 1e-9); }

static long n_checked = 0, n_bad = 0;
static void same(bool a, bool b, const char* what, double p, double q, double r) {
  n_checked++;
  if (a != b) {
    n_bad++;
    std::printf("MISMATCH %s(%a, %a, %a): header %d, former %d\n", what, p, q, r, int(a), int(b));
  }
}
static void same_bits(double a, double b, const char* what, double p, double q) {
  n_checked++;
  if (std::memcmp(&a, &b, sizeof a) != 0) {
    n_bad++;
    std::printf("MISMATCH %s(%a, %a): header %a, former %a\n", what, p, q, a, b);
  }
}

// t, and one ulp either side of it
static void around(std::vector<double>& out, double t) {
  const double inf = std::numeric_limits<double>::infinity();
  out.push_back(std::nextafter(t, -inf));
  out.push_back(t);
  out.push_back(std::nextafter(t, inf));
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double denorm = std::numeric_limits<double>::denorm_min();
  const double bounds[] = {nan, -1.0, 0.0, denorm, 1.0, 1e300, 1e-300, 3.7, 1.25e8, inf};
  const double precs[] = {1e-5, 1e-9, 0.0};
  for (double prec : precs) {
    for (double b : bounds) {
      same(lmmcert::judged(b, prec), old_judged(b, prec), "judged", b, prec, 0);
      std::vector<double> us = {0.0, -0.0, nan, inf, b};
      around(us, b * (1 + prec));
      around(us, b * (1 - prec));
      around(us, b + b * prec);
      around(us, b - b * prec);
      for (double u : us) {
        same(lmmcert::infeasible(u, b, prec), old_infeasible(u, b, prec), "infeasible", u, b, prec);
        same(lmmcert::saturated(u, b, prec), old_sat(u, b, prec), "saturated", u, b, prec);
        same_bits(lmmcert::excess(u, b), old_excess(u, b), "excess", u, b);
      }
      // the variable's bound: the same set of magnitudes (-1 and 0 = unbounded)
      const double vb = b, tol = std::max(prec, 1e-9 * vb);
      std::vector<double> xs = {0.0, nan, inf, vb};
      around(xs, vb + tol);
      around(xs, vb - tol);
      around(xs, vb + prec);
      around(xs, vb - prec);
      around(xs, vb * (1 + 1e-9));
      around(xs, vb * (1 - 1e-9));
      for (double x : xs)
        same(lmmcert::at_bound(x, vb, prec), old_at_bound(x, vb, prec), "at_bound", x, vb, prec);
    }
  }
  const double tops[] = {0.0, denorm, 1e-300, 0.5, 1.0, 3.7, 1.25e8, 1e300, inf, nan};
  for (double top : tops) {
    std::vector<double> ls = {0.0, nan, inf, top};
    around(ls, top * (1 - 1e-9));
    around(ls, top - top * 1e-9);
    around(ls, top);
    for (double l : ls)
      same(lmmcert::carries(l, top), old_carries(l, top), "carries", l, top, 0);
  }
  if (lmmcert::kNoExcess != -1e300 || lmmcert::kWitAtBound != -1 || lmmcert::kWitNone != -2 ||
      lmmcert::kWitNotJudged != -3) {
    std::printf("MISMATCH constants\n");
    n_bad++;
  }
  if (n_bad) {
    std::printf("%ld of %ld comparisons differ\n", n_bad, n_checked);
    return 1;
  }
  std::printf("ok %ld\n", n_checked);
  return 0;
}
