// rh_loo.hip.h -- pointwise WAIC and Pareto-smoothed importance-sampling leave-one-out (Vehtari, Gelman, Gabry 2017; Vehtari, Simpson,
// Gelman, Yao, Gabry: PSIS as the `loo` package computes it) over device-resident log-likelihood draws.
//
// Model-independent: a translation unit of its own (no RH_NVARS, no generated code), compiled once per toolchain through the
// engine's build_source() and inspected like every other code object before it is launched.  wave64, gfx950.  Its text follows
// rh_summary.hip.h's in the translation unit: the pooled sort (rs_tile_sort, rs_merge_tile), the key order (rs_to_key, rs_from_key)
// and rs_tree_sum are that header's, unchanged.
//
// ll [chains][iterations][nvars]; column i holds l_s = log p(y_i | theta_s).  The pooled column of a selected column: the kept
// iterations first + j * thin of every chain (rh_summary.hip.h's window), S = chains * kept values, S >= 2.
//
//   rh_loo_sort_kernel /      the summary's tile sort and merge pass over the selected columns, between two buffers of S keys per
//   rh_loo_merge_kernel       column: a [0 .. S) = the column's l in ascending key order.  The contract's r = -l in ascending order is
//                             a read backwards: r_(j) = -a [S - j], x_(j) = r_(j) - r_(S) = a [0] - a [S - j] (the same subtraction, so
//                             the same bits); the tail -- the largest ratios -- is the front of a.  No permutation is kept: a draw
//                             outside the tail has l_s + lw_s = a [0] exactly.
//   rh_loo_column_kernel      one workgroup per column over its sorted column, LL_BLOCK threads.
//                             The cutoff lc = max(a [0] - a [M], log DBL_MIN) and the tail's length n <= M (a binary search: x is
//                             monotone along a), then one pass for sum l, sum exp(l - max) and the weights outside the tail
//                             sum_{i >= n} exp(a [0] - a [i]) (thread t adds i = t, t + LL_BLOCK, .. ascending, then rs_tree_sum), a
//                             second for sum (l - mean)^2.  n > 4: the tail t_j = exp(x) - exp(lc) staged in LDS in ascending order;
//                             candidate j of Zhang & Stephens' m = 30 + floor(sqrt(n)) <= 119 is thread j - 1, walking the tail in
//                             ascending order with one accumulator; thread 0 adds the m weights in candidate order; khat and the two
//                             sums over the smoothed tail again by stride and tree.
//
// A column whose window holds a NaN or an infinity (read off the ends of the sorted column) gives NaN and tail_n = 0.  No
// floating-point atomics; every sum has a fixed order that depends on the shape (and, for where the tail begins, on the column's own
// values) alone: a second call, a window and its copy, any chunking of the columns and any order of the column list give the same bits.
// exp and log are fdlibm 5.3's e_exp.c and e_log.c written out; log1p and expm1 are the stated compositions of the two below, so that
// a host compiler (contraction off) and the device give the same bits.
// Workspace per column: the two key buffers, 16 S bytes; the host walks the columns in chunks below LL_WS_CAP_BYTES and refuses a
// single column beyond it, and one whose M is beyond LL_TAIL_MAX (S above about 7.2 million).
//
// The block routine is plain C++ over (thread id, LDS pointer): with RH_LOO_HOST (and RH_SUMMARY_HOST) defined it compiles with a
// host compiler, every "thread" of a phase run in turn (tests/test_loo_device_cpu.py): same text, same summation order.
#ifndef RH_LOO_HIP_H
#define RH_LOO_HIP_H
#ifndef RH_SUMMARY_HIP_H
#error "rh_loo.hip.h follows rh_summary.hip.h in its translation unit"
#endif

#define LL_BLOCK 256            // threads of every kernel here (== RS_BLOCK: the sort's routines run in the same workgroups)
#define LL_TAIL_MAX 8064        // the most tail values staged in LDS: 63 KiB (the trace kernel's budget)
#define LL_LDS_DOUBLES (LL_TAIL_MAX + 3 * LL_BLOCK)   // the tail and three rows of partial sums: 69 KiB of gfx950's 160
#define LL_MAX_CAND 119         // 30 + floor(sqrt(LL_TAIL_MAX)): candidate j is thread j - 1
#define LL_WS_CAP_BYTES (128ll << 20)
#define LL_KEY_NEG_INF 0x000fffffffffffffull
#define LL_KEY_POS_INF 0xfff0000000000000ull
#define LL_DBL_MIN 2.2250738585072014e-308

#ifndef RH_LOO_HOST
#define LL_FN static __device__ __forceinline__
#define LL_SYNC() __syncthreads()
#define LL_TID0 ((int)threadIdx.x)
#define LL_TID1 ((int)threadIdx.x + 1)
#else
#define LL_FN static inline
#define LL_SYNC() ((void)0)
#define LL_TID0 0
#define LL_TID1 ll_nthreads
#endif
#define LL_EACH_THREAD(tid) for (int tid = LL_TID0; tid < LL_TID1; tid++)

// ---- exp, log, log1p, expm1 ------------------------------------------------------------------------------------------------------------
LL_FN int ll_hi(const double x) { unsigned long long b; __builtin_memcpy(&b, &x, 8); return (int)(b >> 32); }
LL_FN unsigned ll_lo(const double x) { unsigned long long b; __builtin_memcpy(&b, &x, 8); return (unsigned)b; }
LL_FN double ll_with_hi(const double x, const int h) {
  unsigned long long b;
  __builtin_memcpy(&b, &x, 8);
  b = ((unsigned long long)(unsigned)h << 32) | (b & 0xffffffffull);
  double y;
  __builtin_memcpy(&y, &b, 8);
  return y;
}

// fdlibm 5.3 e_log.c
LL_FN double ll_log(double x) {
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, two54 = 1.80143985094819840000e+16,
               Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
               Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
               Lg7 = 1.479819860511658591e-01;
  int hx = ll_hi(x);
  const unsigned lx = ll_lo(x);
  int k = 0;
  if (hx < 0x00100000) {
    if (((hx & 0x7fffffff) | lx) == 0) return -__builtin_huge_val();
    if (hx < 0) return rs_from_key(RS_KEY_NAN);
    k -= 54;
    x *= two54;
    hx = ll_hi(x);
  }
  if (hx >= 0x7ff00000) return x + x;
  k += (hx >> 20) - 1023;
  hx &= 0x000fffff;
  int i = (hx + 0x95f64) & 0x100000;
  x = ll_with_hi(x, hx | (i ^ 0x3ff00000));
  k += (i >> 20);
  const double f = x - 1.0, dk = (double)k;
  if ((0x000fffff & (2 + hx)) < 3) {
    if (f == 0.0) return k == 0 ? 0.0 : dk * ln2_hi + dk * ln2_lo;
    const double R = f * f * (0.5 - 0.33333333333333333 * f);
    return k == 0 ? f - R : dk * ln2_hi - ((R - dk * ln2_lo) - f);
  }
  const double s = f / (2.0 + f), z = s * s, w = z * z;
  i = hx - 0x6147a;
  const int j = 0x6b851 - hx;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6)), t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  i |= j;
  const double R = t2 + t1;
  if (i > 0) {
    const double hfsq = 0.5 * f * f;
    return k == 0 ? f - (hfsq - s * (hfsq + R)) : dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
  }
  return k == 0 ? f - s * (f - R) : dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

// fdlibm 5.3 e_exp.c
LL_FN double ll_exp(double x) {
  const double huge = 1.0e+300, twom1000 = 9.33263618503218878990e-302, o_threshold = 7.09782712893383973096e+02,
               u_threshold = -7.45133219101941108420e+02, ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10,
               invln2 = 1.44269504088896338700e+00, P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03,
               P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
  double hi = 0.0, lo = 0.0;
  int k = 0;
  unsigned hx = (unsigned)ll_hi(x);
  const int xsb = (int)((hx >> 31) & 1);
  hx &= 0x7fffffff;
  if (hx >= 0x40862E42) {
    if (hx >= 0x7ff00000) {
      if (((hx & 0xfffff) | ll_lo(x)) != 0) return x + x;
      return xsb == 0 ? x : 0.0;
    }
    if (x > o_threshold) return huge * huge;
    if (x < u_threshold) return twom1000 * twom1000;
  }
  if (hx > 0x3fd62e42) {
    if (hx < 0x3FF0A2B2) {
      hi = x - (xsb ? -ln2HI : ln2HI);
      lo = xsb ? -ln2LO : ln2LO;
      k = 1 - xsb - xsb;
    } else {
      k = (int)(invln2 * x + (xsb ? -0.5 : 0.5));
      const double t = (double)k;
      hi = x - t * ln2HI;
      lo = t * ln2LO;
    }
    x = hi - lo;
  } else if (hx < 0x3e300000) {
    return 1.0 + x;
  }
  const double t = x * x;
  const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
  if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
  double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
  if (k >= -1021) return ll_with_hi(y, ll_hi(y) + (k << 20));
  y = ll_with_hi(y, ll_hi(y) + ((k + 1000) << 20));
  return y * twom1000;
}

// log(1 + x) = log(u) x / (u - 1), u = fl(1 + x): the factor undoes the rounding of u (x where u == 1); -inf at -1, NaN below
LL_FN double ll_log1p(const double x) {
  const double u = 1.0 + x;
  if (u == 1.0) return x;
  if (u - u != 0.0) return ll_log(u);            // +inf, NaN
  return ll_log(u) * (x / (u - 1.0));
}
// exp(x) - 1 = (u - 1) x / log(u), u = exp(x) (x where u == 1, -1 where u - 1 == -1, u where it is not finite)
LL_FN double ll_expm1(const double x) {
  const double u = ll_exp(x);
  if (u == 1.0) return x;
  if (u - u != 0.0) return u;
  const double um = u - 1.0;
  if (um == -1.0) return -1.0;
  return um * (x / ll_log(u));
}

LL_FN bool ll_finite(const double v) { return v - v == 0.0; }

// ---- the tail of one sorted column (steps 1 - 8 of the contract; rh_loo_expect.hip.h calls the same three routines) -------------------
// s: the column's keys in ascending order, finite; a0 = a [0].  The cutoff lc = max(a [0] - a [M], log DBL_MIN), exp(lc), and the tail's
// length n <= M: the values with x = a [0] - a [i] > lc (a binary search: x does not grow along a and x at M is not above lc)
LL_FN int ll_tail_cut(const rs_key *s, const long long M, const double a0, double *elc) {
  const double lc0 = a0 - rs_from_key(s[M]), lmin = ll_log(LL_DBL_MIN), lc = lc0 > lmin ? lc0 : lmin;
  *elc = ll_exp(lc);
  long long lo = 0, hi = M;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (a0 - rs_from_key(s[mid]) > lc) lo = mid + 1; else hi = mid;
  }
  return (int)lo;
}

// Zhang & Stephens' fit of the generalised Pareto distribution to the tail a [0 .. n), n > 4 (a block routine: every thread of the
// workgroup calls it).  lds: LL_LDS_DOUBLES doubles, all of them overwritten.  -> whether the tail is smoothed; *kk, *sigma: the shape
// (with the prior's weight) and the scale
LL_FN bool ll_tail_fit(const rs_key *s, const int n, const double a0, const double elc, double *lds, double *kk, double *sigma, const int ll_nthreads) {
  const int rs_nthreads = ll_nthreads;
  (void)rs_nthreads;
  double *tail = lds, *sa = lds + LL_TAIL_MAX, *sb = sa + LL_BLOCK, *sc = sb + LL_BLOCK;
  const double dn = (double)n;
  // t_j = exp(x_j) - exp(lc), j = 1 .. n ascending: tail [j - 1]
  LL_EACH_THREAD(tid) {
    for (int j = tid; j < n; j += LL_BLOCK) tail[j] = ll_exp(a0 - rs_from_key(s[n - 1 - j])) - elc;
  }
  LL_SYNC();
  int m = (int)__builtin_sqrt(dn);
  while (m * m > n) m--;
  while ((m + 1) * (m + 1) <= n) m++;
  m += 30;
  const double tq = tail[(n + 2) / 4 - 1], tn = tail[n - 1];
  LL_EACH_THREAD(tid) {
    if (tid < m) {
      const double b = (1.0 - __builtin_sqrt((double)m / ((double)(tid + 1) - 0.5))) / (3.0 * tq) + 1.0 / tn;
      double acc = 0.0;
      for (int i = 0; i < n; i++) acc += ll_log1p(-b * tail[i]);
      const double kj = acc / dn;
      sa[tid] = dn * (ll_log(-b / kj) - kj - 1.0);
      sb[tid] = b;
    }
  }
  LL_SYNC();
  LL_EACH_THREAD(tid) {
    if (tid == 0) {                             // the m weights in candidate order
      double top = sa[0], se = 0.0, bb = 0.0;
      for (int j = 1; j < m; j++) top = sa[j] > top ? sa[j] : top;
      for (int j = 0; j < m; j++) se += ll_exp(sa[j] - top);
      const double lse = top + ll_log(se);
      for (int j = 0; j < m; j++) bb += sb[j] * ll_exp(sa[j] - lse);
      sc[0] = bb;
    }
  }
  LL_SYNC();
  const double bbar = sc[0];
  LL_EACH_THREAD(tid) {
    double acc = 0.0;
    for (int i = tid; i < n; i += LL_BLOCK) acc += ll_log1p(-bbar * tail[i]);
    sa[tid] = acc;
  }
  rs_tree_sum(sa, rs_nthreads);
  const double khat = sa[0] / dn;
  *sigma = -khat / bbar;
  *kk = (dn * khat + 5.0) / (dn + 10.0);
  LL_SYNC();
  return ll_finite(*kk) && ll_finite(*sigma);
}

// the smoothed log weight lw_j of the tail's j-th smallest ratio, j = 1 .. n: the fitted distribution's quantile at (j - 0.5) / n, not above 0
LL_FN double ll_tail_lw(const int j, const int n, const double kk, const double sigma, const double elc) {
  const double l1 = ll_log1p(-((double)j - 0.5) / (double)n);
  const double q = kk == 0.0 ? -sigma * l1 : sigma * ll_expm1(-kk * l1) / kk;
  const double v = ll_log(q + elc);
  return v > 0.0 ? 0.0 : v;
}

// ---- one column -------------------------------------------------------------------------------------------------------------------------
// s: the column's S keys in ascending order (a [i] = rs_from_key(s [i])); M = ceil(min(S / 5, 3 sqrt(S))) <= LL_TAIL_MAX, M < S.
// lds: LL_LDS_DOUBLES doubles.  Evaluated as
//   lpd      = a [S-1] + log(sum_i exp(a [i] - a [S-1])) - log(S)
//   p_waic   = sum_i (a [i] - mean)^2 / (S - 1), mean = sum_i a [i] / S (a [0] itself where a [0] and a [S-1] have one key)
//   elpd_loo = a [0] + log((S - n) + sum_j exp(lw_j - x_j)) - log(sum_{i >= n} exp(a [0] - a [i]) + sum_j exp(lw_j)),  j = 1 .. n, x_j =
//              a [0] - a [n - j], lw_j the smoothed log weight -- or x_j itself where the tail is left as it is (then the first sum is n)
LL_FN void ll_column_block(const rs_key *s, const long long S, const long long M, double *lds, double *lpd, double *p_waic, double *elpd_loo,
                           double *pareto_k, int *tail_n, const int ll_nthreads) {
  const int rs_nthreads = ll_nthreads;
  (void)rs_nthreads;
  double *sa = lds + LL_TAIL_MAX, *sb = sa + LL_BLOCK, *sc = sb + LL_BLOCK;
  const double nan = rs_from_key(RS_KEY_NAN), inf = __builtin_huge_val();
  if (s[0] <= LL_KEY_NEG_INF || s[S - 1] >= LL_KEY_POS_INF) {       // a NaN or an infinity in the column
    LL_EACH_THREAD(tid) {
      if (tid == 0) { *lpd = nan; *p_waic = nan; *elpd_loo = nan; *pareto_k = nan; *tail_n = 0; }
    }
    return;
  }
  const double a0 = rs_from_key(s[0]), mx = rs_from_key(s[S - 1]), dS = (double)S;
  double elc;
  const int n = ll_tail_cut(s, M, a0, &elc);
  LL_EACH_THREAD(tid) {
    double as = 0.0, ae = 0.0, ad = 0.0;
    for (long long i = tid; i < S; i += LL_BLOCK) {
      const double v = rs_from_key(s[i]);
      as += v;
      ae += ll_exp(v - mx);
      if (i >= n) ad += ll_exp(a0 - v);
    }
    sa[tid] = as;
    sb[tid] = ae;
    sc[tid] = ad;
  }
  rs_tree_sum(sa, rs_nthreads);
  rs_tree_sum(sb, rs_nthreads);
  rs_tree_sum(sc, rs_nthreads);
  const double mean = s[0] == s[S - 1] ? a0 : sa[0] / dS, sumexp = sb[0], den_rest = sc[0];
  LL_SYNC();
  LL_EACH_THREAD(tid) {
    double acc = 0.0;
    for (long long i = tid; i < S; i += LL_BLOCK) {
      const double d = rs_from_key(s[i]) - mean;
      acc += d * d;
    }
    sa[tid] = acc;
  }
  rs_tree_sum(sa, rs_nthreads);
  LL_EACH_THREAD(tid) {
    if (tid == 0) {
      *lpd = mx + ll_log(sumexp) - ll_log(dS);
      *p_waic = sa[0] / (dS - 1.0);
    }
  }
  LL_SYNC();

  double k = inf, kk = 0.0, sigma = 0.0;
  bool smooth = false;
  if (n > 4) smooth = ll_tail_fit(s, n, a0, elc, lds, &kk, &sigma, ll_nthreads);
  // the tail's two sums: smoothed, or as it is
  LL_EACH_THREAD(tid) {
    double an = 0.0, ad = 0.0;
    for (int j = tid + 1; j <= n; j += LL_BLOCK) {
      const double x = a0 - rs_from_key(s[n - j]);
      if (smooth) {
        const double lw = ll_tail_lw(j, n, kk, sigma, elc);
        an += ll_exp(lw - x);
        ad += ll_exp(lw);
      } else {
        an += 1.0;
        ad += ll_exp(x);
      }
    }
    sa[tid] = an;
    sb[tid] = ad;
  }
  rs_tree_sum(sa, rs_nthreads);
  rs_tree_sum(sb, rs_nthreads);
  if (smooth) k = kk;
  LL_EACH_THREAD(tid) {
    if (tid == 0) {
      *elpd_loo = a0 + ll_log((double)(S - n) + sa[0]) - ll_log(den_rest + sb[0]);
      *pareto_k = k;
      *tail_n = n;
    }
  }
}

#ifndef RH_LOO_HOST
// The workspace holds, for the chunk's columns [k_lo, k_lo + p_cnt) of the selection, two buffers [p_cnt][S] of keys.
// grid: tiles x p_cnt, blockIdx.x = tile * p_cnt + column; cols: the chunk's entries of the column list
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_sort_kernel(const double *__restrict__ ll, const long long iterations, const long long nvars, const long long first, const long long thin,
                   const long long kept, const long long S, const int *__restrict__ cols, const int p_cnt, rs_key *__restrict__ ws) {
  __shared__ rs_key lds[RS_TILE_SLOTS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const int pl = (int)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt);
  const long long g0 = tile * RS_TILE;
  if (g0 >= S) return;
  rs_tile_sort(ll + first * nvars + cols[pl], iterations, nvars, thin, kept, S, g0, lds, ws + (long long)pl * S + g0, LL_BLOCK);
}

// one merge pass over runs of L keys, src -> dst ([p_cnt][S] each); grid: ceil(S / RS_MERGE_TILE) x p_cnt
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_merge_kernel(const rs_key *__restrict__ src, rs_key *__restrict__ dst, const long long S, const long long L, const int p_cnt) {
  __shared__ rs_key lds[RS_MERGE_LDS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const int pl = (int)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt);
  const long long o0 = tile * RS_MERGE_TILE;
  if (o0 >= S) return;
  rs_merge_tile(src + (long long)pl * S, dst + (long long)pl * S, S, L, o0, lds, LL_BLOCK);
}

// grid: the chunk's columns; the outputs are indexed by the column's place in the selection, k_lo + blockIdx.x
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_column_kernel(const rs_key *__restrict__ sorted, const long long S, const long long M, const int k_lo, double *__restrict__ lpd,
                     double *__restrict__ p_waic, double *__restrict__ elpd_loo, double *__restrict__ pareto_k, int *__restrict__ tail_n) {
  __shared__ double lds[LL_LDS_DOUBLES];
  const long long pl = (long long)blockIdx.x;
  const int k = k_lo + (int)pl;
  ll_column_block(sorted + pl * S, S, M, lds, lpd + k, p_waic + k, elpd_loo + k, pareto_k + k, tail_n + k, LL_BLOCK);
}
#endif
#endif
