// rh_loo_expect.hip.h -- PSIS leave-one-out expectations over device-resident draws: the mean and variance of the leave-one-out
// predictive distribution of an observation (the `loo` package's E_loo), the LOO probability integral transform P(y_rep <= y | y_-i)
// and the PSIS effective sample size, as weighted sums over the draws with the Pareto-smoothed weights of rh_loo.hip.h.
//
// Model-independent: a translation unit of its own, behind rh_summary.hip.h (the pooled sort, the key order, rs_tree_sum) and
// rh_loo.hip.h (exp and log, ll_tail_cut, ll_tail_fit, ll_tail_lw: the tail fit is that header's, called, so that pareto_k and tail_n
// are rh_loo_device's bit for bit).  wave64, gfx950.
//
// A pair k of the selection: the log-likelihood column ll_cols [k] of ll [chains][iterations][nll] and the value column val_cols [k] of
// val [chains][iterations][nval], over rh_summary.hip.h's window; draw s = c * kept + j, S = chains * kept >= 2.
//
//   rh_loo_expect_sort_kernel /   the summary's tile sort and merge pass over the pairs' log-likelihood columns, between two buffers of
//   rh_loo_expect_merge_kernel    S keys per pair: a [0 .. S) ascending; the tail -- the largest ratios -- is its front.
//   rh_loo_expect_fit_kernel      one workgroup per pair over its sorted column: the cutoff, the tail's length n and the fit (rh_loo.hip.h's
//                                 routines), pareto_k and tail_n; where the tail is smoothed, exp(lw_{n - p}) of every tail position p staged
//                                 in LDS, then the mean over each group of equal keys (the group's first thread adds it in ascending p with
//                                 one accumulator) written to all of the group's positions of tailw [M].
//   rh_loo_expect_reduce_kernel   one workgroup per pair over its draws in their own order.  The weight of draw s: a draw whose key is not
//                                 above a [n - 1] of a smoothed tail takes one lower-bound binary search in a [0 .. n) and reads tailw there;
//                                 every other draw has W = exp(a [0] - l_s).  W is kept in the sort's spare key buffer (the thread that wrote
//                                 it is the one that reads it).  Thread t adds s = t, t + LL_BLOCK, .. ascending, then rs_tree_sum:
//                                   den = sum W, sum W^2, sum W v, sum W [v <= y], sum W [v < y], the counts of values that are not
//                                   finite and of values that are not the first draw's;  mean = sum W v / den (the value itself where
//                                   all draws have the first one's, as rh_loo.hip.h takes a constant column's mean: the two sums round
//                                   apart);  a second pass: var = sum W (v - mean)^2 / den;
//                                   pit = sum W [v <= y] / den, pit_lt likewise with <;  ess = den^2 / sum W^2.
//
// A NaN or an infinity in the log-likelihood window gives NaN in every double and tail_n = 0; one in the value window gives NaN in mean,
// var, pit and pit_lt and leaves ess, pareto_k and tail_n as they are; a NaN y gives NaN in pit and pit_lt.  No floating-point atomics;
// every sum has an order fixed by the shape (and, for the tail's groups, by the column's own values): a second call, a window and its
// copy, any chunking and any order of the pair list give the same bits.  y = +inf sums what den sums in den's order: pit == 1 exactly.
// Workspace per pair: the two key buffers, 16 S bytes (the spare one holds W for the reduction), and 8 M for the tail's weights.
//
// The block routines are plain C++ over (thread id, LDS pointer): with RH_LOO_EXPECT_HOST (and RH_LOO_HOST, RH_SUMMARY_HOST) defined
// they compile with a host compiler, every "thread" of a phase run in turn (tests/test_loo_expect_device_cpu.py): same text, same
// summation order.
#ifndef RH_LOO_EXPECT_HIP_H
#define RH_LOO_EXPECT_HIP_H
#ifndef RH_LOO_HIP_H
#error "rh_loo_expect.hip.h follows rh_summary.hip.h and rh_loo.hip.h in its translation unit"
#endif
#if defined(RH_LOO_EXPECT_HOST) != defined(RH_LOO_HOST)
#error "rh_loo_expect.hip.h is compiled the way rh_loo.hip.h is: both for the host or both for the device"
#endif

#define LX_LDS_DOUBLES (7 * LL_BLOCK)        // the reduction's seven rows of partial sums; the fit kernel has rh_loo.hip.h's LL_LDS_DOUBLES
#define LX_WS_CAP_BYTES LL_WS_CAP_BYTES
#define LX_PAIR_BYTES(S, M) (16 * (S) + 8 * (M))

// ---- the tail's weights of one pair ----------------------------------------------------------------------------------------------------
// s: the log-likelihood column's S keys in ascending order; M as in ll_column_block; lds: LL_LDS_DOUBLES doubles; tailw [M]: written at
// [0 .. n) where the tail is smoothed (pareto_k finite), else left alone.
LL_FN void lx_fit_block(const rs_key *s, const long long S, const long long M, double *lds, double *tailw, double *pareto_k, int *tail_n,
                        const int ll_nthreads) {
  if (s[0] <= LL_KEY_NEG_INF || s[S - 1] >= LL_KEY_POS_INF) {       // a NaN or an infinity in the column
    LL_EACH_THREAD(tid) {
      if (tid == 0) { *pareto_k = rs_from_key(RS_KEY_NAN); *tail_n = 0; }
    }
    return;
  }
  const double a0 = rs_from_key(s[0]);
  double elc, kk = 0.0, sigma = 0.0;
  const int n = ll_tail_cut(s, M, a0, &elc);
  bool smooth = false;
  if (n > 4) smooth = ll_tail_fit(s, n, a0, elc, lds, &kk, &sigma, ll_nthreads);
  if (smooth) {
    double *e = lds;                                                // n <= M <= LL_TAIL_MAX
    LL_EACH_THREAD(tid) {
      for (int p = tid; p < n; p += LL_BLOCK) e[p] = ll_exp(ll_tail_lw(n - p, n, kk, sigma, elc));
    }
    LL_SYNC();
    LL_EACH_THREAD(tid) {
      for (int p = tid; p < n; p += LL_BLOCK) {
        if (p > 0 && s[p - 1] == s[p]) continue;                    // not the first of its group of equal keys
        int q = p;
        double acc = 0.0;
        while (q < n && s[q] == s[p]) acc += e[q++];
        const double w = acc / (double)(q - p);
        for (int r = p; r < q; r++) tailw[r] = w;
      }
    }
  }
  LL_EACH_THREAD(tid) {
    if (tid == 0) { *pareto_k = smooth ? kk : __builtin_huge_val(); *tail_n = n; }
  }
}

// ---- the weighted sums of one pair -------------------------------------------------------------------------------------------------------
// s, tailw, pk, n: the sorted column and what lx_fit_block left for it.  lcol, vcol: the draws at [chain 0][iteration `first`][the pair's
// column] of the two buffers of nll and nval columns; draw g is at ((g / kept) * iterations + (g % kept) * thin) columns' rows.  y: the
// observation (read where has_y).  w [S]: the draws' weights, written and read here.  lds: LX_LDS_DOUBLES doubles.  pit, pit_lt: written
// where has_y.
LL_FN void lx_reduce_block(const rs_key *s, const long long S, const double *tailw, const double pk, const int n, const double *lcol,
                           const long long nll, const double *vcol, const long long nval, const long long iterations, const long long thin,
                           const long long kept, const bool has_y, const double y, double *w, double *lds, double *mean_out, double *var_out,
                           double *pit, double *pit_lt, double *ess, const int ll_nthreads) {
  const int rs_nthreads = ll_nthreads;
  (void)rs_nthreads;
  double *r0 = lds, *r1 = r0 + LL_BLOCK, *r2 = r1 + LL_BLOCK, *r3 = r2 + LL_BLOCK, *r4 = r3 + LL_BLOCK, *r5 = r4 + LL_BLOCK, *r6 = r5 + LL_BLOCK;
  const double nan = rs_from_key(RS_KEY_NAN);
  if (s[0] <= LL_KEY_NEG_INF || s[S - 1] >= LL_KEY_POS_INF) {       // a NaN or an infinity in the log-likelihood column
    LL_EACH_THREAD(tid) {
      if (tid == 0) {
        *mean_out = nan; *var_out = nan; *ess = nan;
        if (has_y) { *pit = nan; *pit_lt = nan; }
      }
    }
    return;
  }
  const bool smooth = n > 4 && ll_finite(pk);
  const double a0 = rs_from_key(s[0]);
  const rs_key top = smooth ? s[n - 1] : 0;                         // the tail's last key
  const double v0 = vcol[0];                                        // the first draw's value
  LL_EACH_THREAD(tid) {
    double den = 0.0, sw2 = 0.0, swv = 0.0, sle = 0.0, slt = 0.0, nb = 0.0, nd = 0.0;
    for (long long g = tid; g < S; g += LL_BLOCK) {
      const long long c = g / kept, j = g - c * kept, row = c * iterations + j * thin;
      const double l = lcol[row * nll], v = vcol[row * nval];
      double W;
      const rs_key key = rs_to_key(l);
      if (smooth && key <= top) {                                   // in the tail: the first position of its key
        int lo = 0, hi = n - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s[mid] < key) lo = mid + 1; else hi = mid;
        }
        W = tailw[lo];
      } else {
        W = ll_exp(a0 - l);
      }
      w[g] = W;
      den += W;
      sw2 += W * W;
      swv += W * v;
      if (has_y) {
        sle += v <= y ? W : 0.0;
        slt += v < y ? W : 0.0;
      }
      if (!ll_finite(v)) nb += 1.0;
      if (v != v0) nd += 1.0;
    }
    r0[tid] = den; r1[tid] = sw2; r2[tid] = swv; r3[tid] = sle; r4[tid] = slt; r5[tid] = nb; r6[tid] = nd;
  }
  rs_tree_sum(r0, rs_nthreads);
  rs_tree_sum(r1, rs_nthreads);
  rs_tree_sum(r2, rs_nthreads);
  rs_tree_sum(r3, rs_nthreads);
  rs_tree_sum(r4, rs_nthreads);
  rs_tree_sum(r5, rs_nthreads);
  rs_tree_sum(r6, rs_nthreads);
  const double den = r0[0], sw2 = r1[0], mean = r6[0] == 0.0 ? v0 : r2[0] / den, sle = r3[0], slt = r4[0];
  const bool vbad = r5[0] != 0.0;
  LL_SYNC();
  LL_EACH_THREAD(tid) {
    double acc = 0.0;
    for (long long g = tid; g < S; g += LL_BLOCK) {
      const long long c = g / kept, j = g - c * kept, row = c * iterations + j * thin;
      const double d = vcol[row * nval] - mean;
      acc += w[g] * (d * d);
    }
    r0[tid] = acc;
  }
  rs_tree_sum(r0, rs_nthreads);
  LL_EACH_THREAD(tid) {
    if (tid == 0) {
      *mean_out = vbad ? nan : mean;
      *var_out = vbad ? nan : r0[0] / den;
      *ess = den * den / sw2;
      if (has_y) {
        const bool ybad = y != y;
        *pit = vbad || ybad ? nan : sle / den;
        *pit_lt = vbad || ybad ? nan : slt / den;
      }
    }
  }
}

#ifndef RH_LOO_EXPECT_HOST
// The workspace holds, for the chunk's pairs [k_lo, k_lo + p_cnt) of the selection, two buffers [p_cnt][S] of keys and tailw [p_cnt][M].
// grid: tiles x p_cnt, blockIdx.x = tile * p_cnt + pair; cols: the chunk's entries of the log-likelihood column list
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_expect_sort_kernel(const double *__restrict__ ll, const long long iterations, const long long nll, const long long first, const long long thin,
                          const long long kept, const long long S, const int *__restrict__ cols, const int p_cnt, rs_key *__restrict__ ws) {
  __shared__ rs_key lds[RS_TILE_SLOTS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const int pl = (int)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt);
  const long long g0 = tile * RS_TILE;
  if (g0 >= S) return;
  rs_tile_sort(ll + first * nll + cols[pl], iterations, nll, thin, kept, S, g0, lds, ws + (long long)pl * S + g0, LL_BLOCK);
}

// one merge pass over runs of L keys, src -> dst ([p_cnt][S] each); grid: ceil(S / RS_MERGE_TILE) x p_cnt
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_expect_merge_kernel(const rs_key *__restrict__ src, rs_key *__restrict__ dst, const long long S, const long long L, const int p_cnt) {
  __shared__ rs_key lds[RS_MERGE_LDS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const int pl = (int)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt);
  const long long o0 = tile * RS_MERGE_TILE;
  if (o0 >= S) return;
  rs_merge_tile(src + (long long)pl * S, dst + (long long)pl * S, S, L, o0, lds, LL_BLOCK);
}

// grid: the chunk's pairs; the outputs are indexed by the pair's place in the selection, k_lo + blockIdx.x
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_expect_fit_kernel(const rs_key *__restrict__ sorted, const long long S, const long long M, const int k_lo, double *__restrict__ tailw,
                         double *__restrict__ pareto_k, int *__restrict__ tail_n) {
  __shared__ double lds[LL_LDS_DOUBLES];
  const long long pl = (long long)blockIdx.x;
  const int k = k_lo + (int)pl;
  lx_fit_block(sorted + pl * S, S, M, lds, tailw + pl * M, pareto_k + k, tail_n + k, LL_BLOCK);
}

// grid: the chunk's pairs, behind the fit kernel.  lcols, vcols: the chunk's entries of the two column lists; y [K] or NULL; spare: the
// key buffer the last merge pass read, [p_cnt][S] words; pit, pit_lt: written where y is given
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_expect_reduce_kernel(const double *ll, const long long nll, const double *val, const long long nval, const long long iterations,
                            const long long first, const long long thin, const long long kept, const long long S, const long long M,
                            const int *__restrict__ lcols, const int *__restrict__ vcols, const double *__restrict__ y, const rs_key *__restrict__ sorted,
                            double *__restrict__ spare, const double *__restrict__ tailw, const int k_lo, const double *__restrict__ pareto_k,
                            const int *__restrict__ tail_n, double *__restrict__ mean, double *__restrict__ var, double *__restrict__ pit,
                            double *__restrict__ pit_lt, double *__restrict__ ess) {
  __shared__ double lds[LX_LDS_DOUBLES];
  const long long pl = (long long)blockIdx.x;
  const int k = k_lo + (int)pl;
  lx_reduce_block(sorted + pl * S, S, tailw + pl * M, pareto_k[k], tail_n[k], ll + first * nll + lcols[pl], nll, val + first * nval + vcols[pl], nval,
                  iterations, thin, kept, y != nullptr, y ? y[k] : 0.0, spare + pl * S, lds, mean + k, var + k, pit + k, pit_lt + k, ess + k, LL_BLOCK);
}
#endif
#endif
