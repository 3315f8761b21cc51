// qbeta_check.cpp -- a stand-alone host program around csrc/qbeta.hpp: reads lines "p a b" from standard input and prints
// qbeta(p; a, b) with 17 significant digits, one per line.  tests/test_mcse_device_cpu.py builds it (also under
// -fsanitize=address,undefined) and compares its output with mpmath at 40 digits.
//   g++ -O2 -ffp-contract=off -std=c++17 tools/qbeta_check.cpp -o qbeta_check
#include <cstdio>

#include "../rainier_amd/csrc/qbeta.hpp"

int main() {
  double p, a, b;
  while (std::scanf("%lf %lf %lf", &p, &a, &b) == 3) std::printf("%.17g\n", rh_qbeta::qbeta(p, a, b));
  return 0;
}
