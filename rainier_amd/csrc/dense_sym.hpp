// dense_sym.hpp -- the small dense symmetric routines behind the joint diagnostics' K x K finish (draws.cpp, K <= RJ_MAX_K): a
// Cholesky factor with its log-determinant, forward substitution, and the largest eigenvalue of a symmetric matrix by Householder
// tridiagonalisation and the implicit QL iteration (eigenvalues only; no power iteration: it stalls where two eigenvalues are
// close).  Plain C++ on row-major double [n][n]; no LAPACK, no allocation beyond the caller's vectors.  O(n^3) on one core.
#ifndef RH_DENSE_SYM_HPP
#define RH_DENSE_SYM_HPP

#include <cmath>
#include <limits>
#include <vector>

namespace rh_dense {
// A (its lower triangle is read) -> L in the lower triangle, A = L L^T.  false where a pivot is not finite and > 0 (not positive
// definite in double, or a NaN).  *logdet = log det A = 2 sum log L_ii.
inline bool cholesky(double *A, int n, double *logdet) {
  double ld = 0.0;
  for (int j = 0; j < n; j++) {
    double d = A[(size_t)j * n + j];
    for (int k = 0; k < j; k++) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    const double l = std::sqrt(d);
    A[(size_t)j * n + j] = l;
    ld += std::log(l);
    for (int i = j + 1; i < n; i++) {
      double v = A[(size_t)i * n + j];
      for (int k = 0; k < j; k++) v -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
      A[(size_t)i * n + j] = v / l;
    }
  }
  *logdet = 2.0 * ld;
  return true;
}

// x <- L^-1 x for the element stride `inc` of x (a column of a row-major matrix: inc = its row length)
inline void forward(const double *L, int n, double *x, size_t inc) {
  for (int i = 0; i < n; i++) {
    double v = x[i * inc];
    for (int k = 0; k < i; k++) v -= L[(size_t)i * n + k] * x[k * inc];
    x[i * inc] = v / L[(size_t)i * n + i];
  }
}

// The largest eigenvalue of symmetric A (its lower triangle is read; A is overwritten).  NaN where an entry is not finite or the
// iteration does not settle.
inline double lambda_max(double *A, int n) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++)
      if (!std::isfinite(A[(size_t)i * n + j])) return nan;
  if (n == 1) return A[0];
  std::vector<double> d(n), e(n);
  // Householder reduction to tridiagonal form, row i = n - 1 .. 1 against the leading i x i block
  for (int i = n - 1; i >= 1; i--) {
    double *ai = A + (size_t)i * n;
    const int l = i - 1;
    double h = 0.0, scale = 0.0;
    if (l > 0) {
      for (int k = 0; k <= l; k++) scale += std::fabs(ai[k]);
      if (scale == 0.0) e[i] = ai[l];
      else {
        for (int k = 0; k <= l; k++) { ai[k] /= scale; h += ai[k] * ai[k]; }
        double f = ai[l];
        double g = f >= 0.0 ? -std::sqrt(h) : std::sqrt(h);
        e[i] = scale * g;
        h -= f * g;
        ai[l] = f - g;
        f = 0.0;
        for (int j = 0; j <= l; j++) {
          g = 0.0;
          for (int k = 0; k <= j; k++) g += A[(size_t)j * n + k] * ai[k];
          for (int k = j + 1; k <= l; k++) g += A[(size_t)k * n + j] * ai[k];
          e[j] = g / h;
          f += e[j] * ai[j];
        }
        const double hh = f / (h + h);
        for (int j = 0; j <= l; j++) {
          f = ai[j];
          e[j] = g = e[j] - hh * f;
          for (int k = 0; k <= j; k++) A[(size_t)j * n + k] -= f * e[k] + g * ai[k];
        }
      }
    } else e[i] = ai[l];
  }
  for (int i = 0; i < n; i++) d[i] = A[(size_t)i * n + i];
  // implicit QL with Wilkinson's shift on (d, e)
  for (int i = 1; i < n; i++) e[i - 1] = e[i];
  e[n - 1] = 0.0;
  const double eps = std::numeric_limits<double>::epsilon();
  for (int l = 0; l < n; l++) {
    for (int iter = 0;; iter++) {
      int m = l;
      for (; m < n - 1; m++)
        if (std::fabs(e[m]) <= eps * (std::fabs(d[m]) + std::fabs(d[m + 1]))) break;
      if (m == l) break;
      if (iter == 60) return nan;
      double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
      double r = std::hypot(g, 1.0);
      g = d[m] - d[l] + e[l] / (g + std::copysign(r, g));
      double s = 1.0, c = 1.0, p = 0.0;
      int i = m - 1;
      for (; i >= l; i--) {
        double f = s * e[i];
        const double bb = c * e[i];
        e[i + 1] = r = std::hypot(f, g);
        if (r == 0.0) { d[i + 1] -= p; e[m] = 0.0; break; }
        s = f / r;
        c = g / r;
        g = d[i + 1] - p;
        r = (d[i] - g) * s + 2.0 * c * bb;
        d[i + 1] = g + (p = s * r);
        g = c * r - bb;
      }
      if (r == 0.0 && i >= l) continue;
      d[l] -= p;
      e[l] = g;
      e[m] = 0.0;
    }
  }
  double top = d[0];
  for (int i = 1; i < n; i++) top = d[i] > top ? d[i] : top;
  return top;
}

// The largest eigenvalue of W^-1 Bn = that of the symmetric L^-1 Bn L^-T, W = L L^T.  Where there are fewer chains than columns
// (C - 1 < K) Bn = D^T D / (C - 1) has rank below C, D [C][K] the chains' means less mu, and the C x C Gram Z Z^T / (C - 1),
// z_c = L^-1 d_c, has the same non-zero eigenvalues.  NaN where W has no Cholesky factor.
inline double lambda_max_within_between(const double *W, const double *Bn, const double *m, const double *mu, int C, int K) {
  std::vector<double> L(W, W + (size_t)K * K);
  double ld;
  if (!cholesky(L.data(), K, &ld)) return std::numeric_limits<double>::quiet_NaN();
  if (C - 1 < K) {
    std::vector<double> Z((size_t)C * K), G((size_t)C * C);
    for (int c = 0; c < C; c++) {
      for (int k = 0; k < K; k++) Z[(size_t)c * K + k] = m[(size_t)c * K + k] - mu[k];
      forward(L.data(), K, &Z[(size_t)c * K], 1);
    }
    for (int c = 0; c < C; c++)
      for (int e = 0; e <= c; e++) {
        double v = 0.0;
        for (int k = 0; k < K; k++) v += Z[(size_t)c * K + k] * Z[(size_t)e * K + k];
        G[(size_t)c * C + e] = v / (double)(C - 1);
      }
    return lambda_max(G.data(), C);
  }
  std::vector<double> X(Bn, Bn + (size_t)K * K), M((size_t)K * K);
  for (int j = 0; j < K; j++) forward(L.data(), K, &X[j], (size_t)K);                  // X = L^-1 Bn, column by column
  for (int i = 0; i < K; i++) forward(L.data(), K, &X[(size_t)i * K], 1);              // row i of X L^-T
  for (int i = 0; i < K; i++)
    for (int j = 0; j <= i; j++) M[(size_t)i * K + j] = 0.5 * (X[(size_t)i * K + j] + X[(size_t)j * K + i]);
  return lambda_max(M.data(), K);
}
}  // namespace rh_dense
#endif
