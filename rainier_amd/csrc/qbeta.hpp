// qbeta.hpp -- the inverse of the regularised incomplete beta function for shapes a, b > 1, in plain C++ over <cmath>: what the
// quantiles' Monte Carlo standard errors need on the host (draws.cpp: rh_mcse_device; Vehtari et al. 2021, section 4.3: the 16 % and
// 84 % points of Beta(e p + 1, e (1 - p) + 1) with e an effective sample size up to millions).
//
// Deterministic: no tables that depend on the machine, no globals, no threads; the same arguments give the same bits wherever <cmath>'s
// log, exp, sqrt and lgamma do.
//
// With shapes in the millions the textbook prefactor exp(a log x + b log(1 - x) - log B(a, b)) loses as many digits as its terms
// have before the point, so the density is written in Loader's saddle-point form (C. Loader 2000, "Fast and accurate computation of
// binomial probabilities"): a beta density is a binomial probability with real arguments,
//     f(x; a, b) = (a + b - 1) binom_raw(a - 1, a + b - 2, x, 1 - x),
// whose exponent is a sum of small terms: the Stirling errors and the deviances bd0.  The distribution function is that density
// times Lentz's evaluation of the continued fraction (Numerical Recipes, betacf) on the side of the mean where it converges in
// O(sqrt(max(a, b))) terms; the quantile is a Newton iteration kept inside a bisection bracket, started at the normal approximation.
#ifndef RH_QBETA_HPP
#define RH_QBETA_HPP

#include <cmath>

namespace rh_qbeta {
// log(n!) - log(sqrt(2 pi n) (n / e)^n) for real n > 0
inline double stirlerr(const double n) {
  const double S0 = 1.0 / 12.0, S1 = 1.0 / 360.0, S2 = 1.0 / 1260.0, S3 = 1.0 / 1680.0, S4 = 1.0 / 1188.0;
  if (n <= 15.0) return std::lgamma(n + 1.0) - (n + 0.5) * std::log(n) + n - 0.918938533204672741780329736406;   // log(sqrt(2 pi))
  const double nn = n * n;
  if (n > 500.0) return (S0 - S1 / nn) / n;
  if (n > 80.0) return (S0 - (S1 - S2 / nn) / nn) / n;
  if (n > 35.0) return (S0 - (S1 - (S2 - S3 / nn) / nn) / nn) / n;
  return (S0 - (S1 - (S2 - (S3 - S4 / nn) / nn) / nn) / nn) / n;
}

// x log(x / np) + np - x for x, np > 0, without the cancellation when x is near np
inline double bd0(const double x, const double np) {
  if (std::fabs(x - np) < 0.1 * (x + np)) {
    double v = (x - np) / (x + np);
    double s = (x - np) * v, ej = 2.0 * x * v;
    v = v * v;
    for (int j = 1; j < 1000; j++) {
      ej *= v;
      const double s1 = s + ej / (double)(2 * j + 1);
      if (s1 == s) return s1;
      s = s1;
    }
    return s;
  }
  return x * std::log(x / np) + np - x;
}

// the binomial probability of x successes in n trials with real 0 < x < n and 0 < p < 1, q = 1 - p
inline double binom_raw(const double x, const double n, const double p, const double q) {
  const double lc = stirlerr(n) - stirlerr(x) - stirlerr(n - x) - bd0(x, n * p) - bd0(n - x, n * q);
  return std::exp(lc) * std::sqrt(n / (6.283185307179586476925286766559 * x * (n - x)));
}

// the density of Beta(a, b) at 0 < x < 1, a, b > 1; y = 1 - x
inline double density(const double x, const double y, const double a, const double b) { return (a + b - 1.0) * binom_raw(a - 1.0, a + b - 2.0, x, y); }

// the continued fraction of I_x(a, b) by the modified Lentz method; converges fast for x < (a + 1) / (a + b + 2)
inline double fraction(const double a, const double b, const double x) {
  const double tiny = 1e-300, eps = 3e-16;          // a factor within an ulp of 1 ends it
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (std::fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  const int limit = 200 + (int)(20.0 * std::sqrt(a > b ? a : b));
  for (int m = 1; m <= limit; m++) {
    const double dm = (double)m, m2 = 2.0 * dm;
    double aa = dm * (b - dm) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (std::fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (std::fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (std::fabs(del - 1.0) <= eps) break;
  }
  return h;
}

// I_x(a, b) for 0 < x < 1, y = 1 - x, a, b > 1; *f: the density there
inline double pbeta(const double x, const double y, const double a, const double b, double *f) {
  const double dens = density(x, y, a, b), bt = x * y * dens;
  *f = dens;
  if (x < (a + 1.0) / (a + b + 2.0)) return bt * fraction(a, b, x) / a;
  return 1.0 - bt * fraction(b, a, y) / b;
}

// the normal quantile of 0 < p < 1 to about 1e-9 (Acklam's rational approximation): the start of the iteration only
inline double start_z(const double p) {
  const double a[6] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
  const double b[5] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01, -1.328068155288572e+01};
  const double c[6] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
  const double d[4] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00};
  if (p < 0.02425 || p > 1.0 - 0.02425) {
    const double q = std::sqrt(-2.0 * std::log(p < 0.5 ? p : 1.0 - p));
    const double z = (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0);
    return p < 0.5 ? z : -z;
  }
  const double q = p - 0.5, r = q * q;
  return (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q / (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0);
}

// x with I_x(a, b) = p, for 0 < p < 1 and a, b > 1 (NaN otherwise)
inline double qbeta(const double p, const double a, const double b) {
  if (!(p > 0.0 && p < 1.0 && a > 1.0 && b > 1.0) || a > 1e300 || b > 1e300) return std::nan("");
  // the normal approximation around the mean, then Newton steps inside a bracket that every evaluation narrows
  const double mean = a / (a + b), sd = std::sqrt(a * b / ((a + b) * (a + b) * (a + b + 1.0)));
  double lo = 0.0, hi = 1.0;
  double x = mean + start_z(p) * sd;
  if (!(x > 0.0 && x < 1.0)) x = mean;
  for (int it = 0; it < 200; it++) {
    double f;
    const double F = pbeta(x, 1.0 - x, a, b, &f), r = F - p;
    if (r == 0.0) return x;
    if (r < 0.0) lo = x; else hi = x;
    double xn = x - r / f;
    if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);       // a step out of the bracket (or a density that underflowed): bisect
    if (xn == x || std::fabs(xn - x) <= 2.220446049250313e-16 * x) return xn;
    x = xn;
  }
  return x;
}
}  // namespace rh_qbeta
#endif
