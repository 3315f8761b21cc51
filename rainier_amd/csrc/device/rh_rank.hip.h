// rh_rank.hip.h -- rank-normalised split R-hat, bulk ESS and tail ESS (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021) over
// device-resident draws.
//
// Model-independent: a translation unit of its own (no RH_NVARS, no generated code), compiled once per toolchain through the
// engine's build_source() and inspected like every other code object before it is launched.  wave64, gfx950.  Its text follows
// rh_summary.hip.h's in the translation unit: the pooled sort (rs_tile_sort, rs_merge_tile), the key order (rs_to_key: Double.compare's,
// -0.0 before +0.0) and rs_tree_sum are that header's, unchanged.
//
// draws [chains][iterations][nvars]; analysed: the window [first, first + count) of every chain, count >= 4, the selected columns.
// Split: h = count / 2; sequence q = 2c is (c, first + i), q = 2c + 1 is (c, first + count - h + i), i = 0 .. h-1 (an odd count leaves
// the middle draw out); M = 2 chains sequences, S = M h values, flat index s = q h + i.
//
//   rh_rank_stage_kernel      the split window of a tile of <= RK_TP selected columns x RK_ROWS flat values, through LDS: read with the
//                             lanes along the columns (neighbouring doubles of a draw's row), written with the lanes along s into the
//                             dense y [column][S].
//   rh_rank_fold_kernel       u = |y - med|, med = 0.5 sorted[S/2 - 1] + 0.5 sorted[S/2] of the column's sorted keys.
//   rh_rank_sort_kernel /     the summary's tile sort and merge pass over a dense column (one flat chain: nvars = 1, thin = 1,
//   rh_rank_merge_kernel      kept = N = S), between two buffers of S keys per column.
//   rh_rank_normal_kernel     per value two binary searches in the sorted column -- L keys below, U keys at or below -- the average
//                             rank r = (L + U + 1) / 2 and z = rk_ndtri((r - 3/8) / (S + 1/4)) (Wichura's AS 241, PPND16, written out;
//                             its log is fdlibm's e_log.c written out too, so that host and device give the same bits).
//   rh_rank_indicator_kernel  u = I(key(y) <= sorted[idx]) as 1.0 / 0.0: an order statistic (precis'), not an interpolated quantile.
//   rh_rank_chain_kernel      one workgroup = one sequence x one column, RK_BLOCK threads.  The mean (thread t adds i = t, t + RK_BLOCK,
//                             .. ascending, then a fixed binary tree), the sequence centred into LDS -- whole when h <= RK_LDS_DOUBLES,
//                             else in time tiles with a halo of L values ahead -- and thread t <= L accumulates sum_i d_i d_{i+t},
//                             i ascending, in one accumulator: d_i is a broadcast read, d_{i+t} a unit-stride one (no bank conflict).
//                             L = min(h - 1, RK_MAXLAG) (lag t is thread t: the work is RK_BLOCK h whatever the chain does), or 0 for
//                             the folded series, of which only lag 0 is used.
//                             -> ws [column of the chunk][M][sl] = { m_q, g_q(0 .. L) }, g_q(t) = sum / h
//   rh_rank_finish_kernel     one workgroup per (column, series): the sums over q in sequence order, then W, B, V, rhat and Geyer's
//                             initial monotone sequence over pairs of lags on one thread.  fin [column][series][3] = rhat, ess, truncated.
//   rh_rank_combine_kernel    one thread per column: rhat_bulk, rhat_folded, ess_bulk, ess_tail = min of the two tails (NaN if either
//                             is), truncated = bit 0 bulk, bit 1 lower tail, bit 2 upper tail.
//
// A column whose window holds a NaN or an infinity (read off the ends of the sorted column) and a series with W == 0 (or no W > 0 at
// all) give NaN.  No floating-point atomics; every sum has a fixed order that depends on the shape alone: a second call, a window and
// its copy, and any chunking of the columns give the same bits.
// Workspace per column: y, two key buffers, one series buffer (reused by the four series) of S 8-byte words each, and ws; the host
// walks the columns in chunks below RK_WS_CAP_BYTES and refuses a single column beyond it.
//
// The block routines are plain C++ over (thread id, LDS pointer): with RH_RANK_HOST (and RH_SUMMARY_HOST) defined they compile with
// a host compiler, every "thread" of a phase run in turn (tests/test_rank_diagnostics_device_cpu.py): same text, same summation order.
#ifndef RH_RANK_HIP_H
#define RH_RANK_HIP_H
#ifndef RH_SUMMARY_HIP_H
#error "rh_rank.hip.h follows rh_summary.hip.h in its translation unit"
#endif

#define RK_BLOCK 256            // threads of every kernel here (== RS_BLOCK: the sort's routines run in the same workgroups)
#define RK_MAXLAG 255           // lag t is thread t of the chain kernel
#define RK_SL (RK_MAXLAG + 2)   // the most doubles per (column, sequence) in the workspace: the mean and g(0 .. 255)
#define RK_LDS_DOUBLES 8064     // the centred sequence: 63 KiB (the trace kernel's budget)
#define RK_TP 16                // columns of a stage tile
#define RK_ROWS 256             // flat values of a stage tile
#define RK_STAGE_STRIDE (RK_ROWS + 1)
#define RK_NSERIES 4            // 0 bulk z(y), 1 folded z(|y - med|), 2 lower-tail indicator, 3 upper-tail indicator
#define RK_NFIN 3               // rhat, ess, truncated per (column, series)
#define RK_WS_CAP_BYTES (128ll << 20)
#define RK_KEY_NEG_INF 0x000fffffffffffffull
#define RK_KEY_POS_INF 0xfff0000000000000ull

#ifndef RH_RANK_HOST
#define RK_FN static __device__ __forceinline__
#define RK_SYNC() __syncthreads()
#define RK_TID0 ((int)threadIdx.x)
#define RK_TID1 ((int)threadIdx.x + 1)
#define RK_ST(tid) 0
#define RK_NSTATE 1
#else
#define RK_FN static inline
#define RK_SYNC() ((void)0)
#define RK_TID0 0
#define RK_TID1 rk_nthreads
#define RK_ST(tid) (tid)
#define RK_NSTATE RK_BLOCK
#endif
#define RK_EACH_THREAD(tid) for (int tid = RK_TID0; tid < RK_TID1; tid++)

// ---- log and the normal quantile ---------------------------------------------------------------------------------------------------
// fdlibm 5.3 e_log.c for a finite, normal x > 0 (here 0 < x <= 1/2)
RK_FN double rk_log(double x) {
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, Lg1 = 6.666666666666735130e-01,
               Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
               Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01, Lg7 = 1.479819860511658591e-01;
  unsigned long long b;
  __builtin_memcpy(&b, &x, 8);
  int hx = (int)(b >> 32);
  int k = (hx >> 20) - 1023;
  hx &= 0x000fffff;
  int i = (hx + 0x95f64) & 0x100000;
  b = ((unsigned long long)(unsigned)(hx | (i ^ 0x3ff00000)) << 32) | (b & 0xffffffffull);
  __builtin_memcpy(&x, &b, 8);
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

// Wichura (1988), Algorithm AS 241, PPND16: the normal quantile of 0 < p < 1, about 1 part in 10^16
RK_FN double rk_ndtri(const double p) {
  const double q = p - 0.5;
  if (__builtin_fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                            4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                          1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
    const double den = ((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                           2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                         4.2313330701600911252e+1) * r + 1.0;
    return num / den;
  }
  double r = __builtin_sqrt(-rk_log(q <= 0.0 ? p : 1.0 - p));
  double num, den;
  if (r <= 5.0) {
    r = r - 1.6;
    num = ((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
              1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
            4.63033784615654529590e+0) * r + 1.42343711074968357734e+0;
    den = ((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
              1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
            2.05319162663775882187e+0) * r + 1.0;
  } else {
    r = r - 5.0;
    num = ((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
              2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
            5.46378491116411436990e+0) * r + 6.65790464350110377720e+0;
    den = ((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
              7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
            5.99832206555887937690e-1) * r + 1.0;
  }
  const double x = num / den;
  return q < 0.0 ? -x : x;
}

// ---- the split window, gathered --------------------------------------------------------------------------------------------------------
// where flat value s lies in draws: the row (in doubles / nvars) of sequence s / h, position s % h
RK_FN long long rk_row_of(const long long s, const long long h, const long long iterations, const long long first, const long long count) {
  const long long q = s / h, i = s - q * h;
  return (q >> 1) * iterations + first + ((q & 1) ? count - h : 0) + i;
}

// A tile of tpw columns (cols[0 .. tpw): their parameters) x the flat values [s0, min(s0 + RK_ROWS, S)) -> y[p * S + s].
// lds: RK_TP * RK_STAGE_STRIDE doubles.
RK_FN void rk_stage_tile(const double *draws, const long long iterations, const long long nvars, const long long first, const long long count,
                         const long long h, const long long S, const int *cols, const int tpw, const long long s0, double *lds, double *y,
                         const int rk_nthreads) {
  const int rows = (int)(S - s0 < RK_ROWS ? S - s0 : RK_ROWS), total = rows * tpw;
  RK_EACH_THREAD(tid) {
    for (int j = tid; j < total; j += RK_BLOCK) {
      const int r = j / tpw, p = j - r * tpw;
      lds[p * RK_STAGE_STRIDE + r] = draws[rk_row_of(s0 + r, h, iterations, first, count) * nvars + cols[p]];
    }
  }
  RK_SYNC();
  RK_EACH_THREAD(tid) {
    for (int j = tid; j < total; j += RK_BLOCK) {
      const int p = j / rows, r = j - p * rows;
      y[(long long)p * S + s0 + r] = lds[p * RK_STAGE_STRIDE + r];
    }
  }
}

// ---- per value: fold, rank -> z, indicator ---------------------------------------------------------------------------------------------
RK_FN double rk_median(const rs_key *sorted, const long long S) { return 0.5 * rs_from_key(sorted[S / 2 - 1]) + 0.5 * rs_from_key(sorted[S / 2]); }
RK_FN double rk_fold(const double y, const double med) { return __builtin_fabs(y - med); }

// how many of the n sorted keys lie below k (or_equal: at or below)
RK_FN long long rk_count(const rs_key *sorted, const long long n, const rs_key k, const bool or_equal) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (or_equal ? sorted[mid] <= k : sorted[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// twice the average rank of v among the column's S values: L + U + 1
RK_FN long long rk_rank2(const rs_key *sorted, const long long S, const double v) {
  const rs_key k = rs_to_key(v);
  return rk_count(sorted, S, k, false) + rk_count(sorted, S, k, true) + 1;
}
RK_FN double rk_rank_z(const rs_key *sorted, const long long S, const double v) {
  const double r = (double)rk_rank2(sorted, S, v) * 0.5;
  return rk_ndtri((r - 0.375) / ((double)S + 0.25));
}
RK_FN double rk_indicator(const rs_key threshold, const double v) { return rs_to_key(v) <= threshold ? 1.0 : 0.0; }

// ---- one sequence of one column ----------------------------------------------------------------------------------------------------------
// u: the sequence's h values; L <= min(h - 1, RK_MAXLAG).  lds: RK_LDS_DOUBLES doubles.  out: { mean, g(0) .. g(L) }
RK_FN void rk_chain_block(const double *u, const int h, const int L, double *lds, double *out, const int rk_nthreads) {
  const int rs_nthreads = rk_nthreads;
  (void)rs_nthreads;
  double acc[RK_NSTATE];
  RK_EACH_THREAD(tid) {
    double a = 0.0;
    for (int i = tid; i < h; i += RK_BLOCK) a += u[i];
    lds[tid] = a;
    acc[RK_ST(tid)] = 0.0;
  }
  rs_tree_sum(lds, rs_nthreads);
  const double mean = lds[0] / (double)h;
  const bool resident = h <= RK_LDS_DOUBLES;       // the whole sequence stays in LDS: staged once
  const int T = resident ? h : RK_LDS_DOUBLES - RK_MAXLAG;
  for (int t0 = 0; t0 < h; t0 += T) {
    const int t1 = t0 + T < h ? t0 + T : h;
    const int e1 = t1 + L < h ? t1 + L : h;         // the halo: the values the tile's lags reach ahead to
    RK_SYNC();
    RK_EACH_THREAD(tid) {
      for (int j = t0 + tid; j < e1; j += RK_BLOCK) lds[j - t0] = u[j] - mean;
    }
    RK_SYNC();
    RK_EACH_THREAD(tid) {
      if (tid <= L) {
        const int hi = t1 < h - tid ? t1 : h - tid;
        double a = acc[RK_ST(tid)];
        for (int i = t0; i < hi; i++) a += lds[i - t0] * lds[i - t0 + tid];
        acc[RK_ST(tid)] = a;
      }
    }
  }
  RK_EACH_THREAD(tid) {
    if (tid <= L) out[1 + tid] = acc[RK_ST(tid)] / (double)h;
    if (tid == 0) out[0] = mean;
  }
}

// ---- one series of one column ----------------------------------------------------------------------------------------------------------
// w [M][sl]: the chain kernel's output; sorted: the S keys the series was made from (its ends tell a NaN or an infinity); L: the
// lags the series carries (0: rhat only, ess NaN); tau_min = 1 / log10(S).  lds: RK_SL + RK_BLOCK doubles.  fin: rhat, ess, truncated
RK_FN void rk_series_finish(const double *w, const rs_key *sorted, const long long S, const int M, const int h, const int L, const int sl,
                            const double tau_min, double *lds, double *fin, const int rk_nthreads) {
  double *tmp = lds + RK_SL;
  RK_EACH_THREAD(tid) {
    for (int e = tid; e < L + 2; e += RK_BLOCK) {
      double s = 0.0;
#pragma unroll 8
      for (int q = 0; q < M; q++) s += w[(long long)q * sl + e];
      lds[e] = s;
    }
  }
  RK_SYNC();
  const double m = (double)M, hh = (double)h;
  const double mm = lds[0] / m;
  double bs = 0.0;                                  // sum over q of (m_q - mm)^2, in sequence order (thread 0)
  for (int q0 = 0; q0 < M; q0 += RK_BLOCK) {
    RK_EACH_THREAD(tid) {
      if (q0 + tid < M) { const double d = w[(long long)(q0 + tid) * sl] - mm; tmp[tid] = d * d; }
    }
    RK_SYNC();
    RK_EACH_THREAD(tid) {
      if (tid == 0) {
        const int cnt = M - q0 < RK_BLOCK ? M - q0 : RK_BLOCK;
        for (int j = 0; j < cnt; j++) bs += tmp[j];
      }
    }
    RK_SYNC();
  }
  RK_EACH_THREAD(tid) {
    if (tid == 0) {
      const double nan = rs_from_key(RS_KEY_NAN);
      const double W = lds[1] / m * hh / (hh - 1.0), B = bs / (m - 1.0), V = (hh - 1.0) / hh * W + B;
      double rhat = __builtin_sqrt(V / W), ess = nan, truncated = 0.0;
      if (L >= 1) {
        const int K = (L - 1) / 2;
        double tau = -1.0, prev = __builtin_huge_val();
        bool stopped = false;
        for (int k = 0; k <= K; k++) {
          const double r0 = k == 0 ? 1.0 : 1.0 - (W - lds[1 + 2 * k] / m) / V, r1 = 1.0 - (W - lds[2 + 2 * k] / m) / V;
          const double Pk = r0 + r1;
          if (!(Pk > 0.0)) { tau += r0 > 0.0 ? r0 : 0.0; stopped = true; break; }
          const double P = Pk < prev ? Pk : prev;
          prev = P;
          tau += 2.0 * P;
        }
        tau = tau > tau_min ? tau : tau_min;
        ess = (double)S / tau;
        truncated = stopped ? 0.0 : 1.0;
      }
      // a NaN or an infinity in the column; a series without a variance within its sequences
      if (sorted[0] <= RK_KEY_NEG_INF || sorted[S - 1] >= RK_KEY_POS_INF || !(W > 0.0)) { rhat = nan; ess = nan; truncated = 0.0; }
      fin[0] = rhat;
      fin[1] = ess;
      fin[2] = truncated;
    }
  }
}

// fin [RK_NSERIES][RK_NFIN] of one column -> its outputs
RK_FN void rk_combine(const double *fin, double *rhat_bulk, double *rhat_folded, double *ess_bulk, double *ess_tail, int *truncated) {
  const double lo = fin[2 * RK_NFIN + 1], hi = fin[3 * RK_NFIN + 1];
  *rhat_bulk = fin[0];
  *rhat_folded = fin[RK_NFIN];
  *ess_bulk = fin[1];
  *ess_tail = (lo != lo || hi != hi) ? rs_from_key(RS_KEY_NAN) : (lo < hi ? lo : hi);
  *truncated = (fin[2] != 0.0 ? 1 : 0) | (fin[2 * RK_NFIN + 2] != 0.0 ? 2 : 0) | (fin[3 * RK_NFIN + 2] != 0.0 ? 4 : 0);
}

#ifndef RH_RANK_HOST
// The workspace holds, for the chunk's columns [k_lo, k_lo + p_cnt) of the selection, y / u [p_cnt][S], two key buffers [p_cnt][S]
// and ws [p_cnt][M][sl].
// grid: tiles of RK_ROWS flat values x tiles of RK_TP columns, blockIdx.x = row tile * ctiles + column tile
extern "C" __global__ void __launch_bounds__(RK_BLOCK)
rh_rank_stage_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const long long first,
                     const long long count, const long long h, const long long S, const int *__restrict__ cols, const int p_cnt,
                     const int ctiles, double *__restrict__ y) {
  __shared__ double lds[RK_TP * RK_STAGE_STRIDE];
  const long long rt = (long long)(blockIdx.x / (unsigned)ctiles);
  const int pl = (int)(blockIdx.x - (unsigned)rt * (unsigned)ctiles) * RK_TP;
  const long long s0 = rt * RK_ROWS;
  if (s0 >= S || pl >= p_cnt) return;
  rk_stage_tile(draws, iterations, nvars, first, count, h, S, cols + pl, p_cnt - pl < RK_TP ? p_cnt - pl : RK_TP, s0, lds, y + (long long)pl * S, RK_BLOCK);
}

// grid: ceil(S / RK_BLOCK) x p_cnt, blockIdx.x = block * p_cnt + column
extern "C" __global__ void __launch_bounds__(RK_BLOCK)
rh_rank_fold_kernel(const rs_key *__restrict__ sorted, const double *__restrict__ y, const long long S, const int p_cnt, double *__restrict__ u) {
  const long long blk = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)blk * (unsigned)p_cnt), s = blk * RK_BLOCK + threadIdx.x;
  if (s < S) u[pl * S + s] = rk_fold(y[pl * S + s], rk_median(sorted + pl * S, S));
}

// grid: tiles x p_cnt, blockIdx.x = tile * p_cnt + column: a dense column is one flat chain
extern "C" __global__ void __launch_bounds__(RK_BLOCK)
rh_rank_sort_kernel(const double *__restrict__ y, const long long S, const int p_cnt, rs_key *__restrict__ keys) {
  __shared__ rs_key lds[RS_TILE_SLOTS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt), g0 = tile * RS_TILE;
  if (g0 >= S) return;
  rs_tile_sort(y + pl * S, S, 1, 1, S, S, g0, lds, keys + pl * S + g0, RK_BLOCK);
}

// one merge pass over runs of L keys, src -> dst ([p_cnt][S] each); grid: ceil(S / RS_MERGE_TILE) x p_cnt
extern "C" __global__ void __launch_bounds__(RK_BLOCK)
rh_rank_merge_kernel(const rs_key *__restrict__ src, rs_key *__restrict__ dst, const long long S, const long long L, const int p_cnt) {
  __shared__ rs_key lds[RS_MERGE_LDS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt), o0 = tile * RS_MERGE_TILE;
  if (o0 >= S) return;
  rs_merge_tile(src + pl * S, dst + pl * S, S, L, o0, lds, RK_BLOCK);
}

// grid as the fold kernel's; v and z may be one buffer (a thread reads its own value before it writes it)
extern "C" __global__ void __launch_bounds__(RK_BLOCK)
rh_rank_normal_kernel(const rs_key *__restrict__ sorted, const double *v, const long long S, const int p_cnt, double *z) {
  const long long blk = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)blk * (unsigned)p_cnt), s = blk * RK_BLOCK + threadIdx.x;
  if (s < S) z[pl * S + s] = rk_rank_z(sorted + pl * S, S, v[pl * S + s]);
}

// grid as the fold kernel's; idx: the order statistic that is the threshold
extern "C" __global__ void __launch_bounds__(RK_BLOCK)
rh_rank_indicator_kernel(const rs_key *__restrict__ sorted, const double *__restrict__ y, const long long S, const int p_cnt, const long long idx,
                         double *__restrict__ u) {
  const long long blk = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)blk * (unsigned)p_cnt), s = blk * RK_BLOCK + threadIdx.x;
  if (s < S) u[pl * S + s] = rk_indicator(sorted[pl * S + idx], y[pl * S + s]);
}

// grid: p_cnt x M, blockIdx.x = column * M + sequence
extern "C" __global__ void __launch_bounds__(RK_BLOCK)
rh_rank_chain_kernel(const double *__restrict__ u, const int h, const int L, const int sl, double *__restrict__ ws) {
  __shared__ double lds[RK_LDS_DOUBLES];
  rk_chain_block(u + (long long)blockIdx.x * h, h, L, lds, ws + (long long)blockIdx.x * sl, RK_BLOCK);
}

// grid: the chunk's columns; fin is indexed by the column's place in the selection, k_lo + blockIdx.x
extern "C" __global__ void __launch_bounds__(RK_BLOCK)
rh_rank_finish_kernel(const double *__restrict__ ws, const rs_key *__restrict__ sorted, const long long S, const int M, const int h, const int L,
                      const int sl, const double tau_min, const int k_lo, const int series, double *__restrict__ fin) {
  __shared__ double lds[RK_SL + RK_BLOCK];
  const long long pl = (long long)blockIdx.x;
  rk_series_finish(ws + pl * M * sl, sorted + pl * S, S, M, h, L, sl, tau_min, lds, fin + ((k_lo + pl) * RK_NSERIES + series) * RK_NFIN, RK_BLOCK);
}

// grid: ceil(K / RK_BLOCK)
extern "C" __global__ void __launch_bounds__(RK_BLOCK)
rh_rank_combine_kernel(const double *__restrict__ fin, const int K, double *__restrict__ rhat_bulk, double *__restrict__ rhat_folded,
                       double *__restrict__ ess_bulk, double *__restrict__ ess_tail, int *__restrict__ truncated) {
  const int k = (int)(blockIdx.x * RK_BLOCK + threadIdx.x);
  if (k < K) rk_combine(fin + (long long)k * RK_NSERIES * RK_NFIN, rhat_bulk + k, rhat_folded + k, ess_bulk + k, ess_tail + k, truncated + k);
}
#endif
#endif
