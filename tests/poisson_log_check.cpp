// Host build of po_log (nautilus_amd/csrc/nb_poisson_log.h) against long
// double: prints the largest error in ulp of the exact result over arguments
// spread over 60 e-folds, over [1/2, 3/2], within 1e-8 .. 1/2 of 1, around
// the sqrt(1/2) 2^e seams of the range reduction, and a few fixed ones.
// Run by tests/test_poisson_log.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "nb_poisson_log.h"

int main(int argc, char** argv) {
  const long count = argc > 1 ? std::atol(argv[1]) : 500000;
  std::mt19937_64 g(1);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  double worst = 0.0, worst_x = 1.0;
  auto test = [&](double x) {
    const long double t = logl((long double)x);
    const double got = po_log(x);
    if (t == 0.0L) {
      if (got != 0.0) worst = INFINITY, worst_x = x;
      return;
    }
    const double ulp = std::ldexp(1.0, std::ilogb((double)t) - 52);
    const double err = std::fabs((double)(((long double)got - t) / ulp));
    if (!(err <= worst)) worst = err, worst_x = x;
  };
  for (long i = 0; i < count; ++i) {
    test(std::exp(60.0 * (u(g) - 0.5)));
    test(0.5 + u(g));
    test(1.0 + (u(g) - 0.5) * std::pow(10.0, -8.0 * u(g)));
    test(std::ldexp(0.70710678118654752 + 1e-3 * (u(g) - 0.5),
                    (int)(40 * u(g)) - 20));
  }
  const double fixed[] = {1.0, 0.5, 2.0, 5e-324, 1e-310, 2.3e-308, 1e308,
                          1e-12, 1e12, 0.70710678118654746,
                          0.70710678118654757, 1.4142135623730949,
                          1.4142135623730951};
  for (double x : fixed) test(x);
  std::printf("%.6f %.17g\n", worst, worst_x);
  return 0;
}
