// rh_mcse.hip.h -- Monte Carlo standard errors and effective sample sizes of the reported figures (Vehtari, Gelman, Simpson,
// Carpenter, Buerkner 2021, section 4: ESS for the mean, the sd and any quantile, and the MCSEs derived from them) over
// device-resident draws.
//
// Model-independent: a translation unit of its own (no RH_NVARS, no generated code), compiled once per toolchain through the
// engine's build_source() and inspected like every other code object before it is launched.  wave64, gfx950.  Its text follows
// rh_summary.hip.h's and rh_rank.hip.h's in the translation unit: the pooled sort, the key order and rs_tree_sum are the summary's,
// the split layout (rk_stage_tile), rk_indicator and rk_series_finish are the rank diagnostics', all unchanged.
//
// Input: draws [chains][iterations][nvars], the window [first, first + count) of every chain, count >= 4, no thinning; the selected
// columns as in the rank diagnostics; probs [nprobs], 0 <= nprobs <= MK_MAXPROBS, 0 < p < 1; nlags, 0 <= nlags <= RK_MAXLAG.
// Split, M, h, S, the flat index s = q h + i, the key order and L = min(h - 1, RK_MAXLAG) are exactly rh_rank.hip.h's.
//
// Pooled figures per column, fixed-order sums whose order depends on S alone (thread t adds s = t, t + MK_BLOCK, .. ascending, then a
// fixed binary tree):   m = sum y / S,  E2 = sum (y - m)^2 / S,  E4 = sum ((y - m)^2)^2 / S,  sd = sqrt(S E2 / (S - 1)).
// Series per column, each [M][h], each through the rank diagnostics' estimator unchanged (m_q, g_q(t), W, B, V, Geyer's pairs,
// tau_min, truncated):   A: y   B: |y - m|   C: (y - m)^2   D_k: I(key(y) <= sorted[j_k]), j_k = min(S - 1, floor(S probs[k])) -- the
// summary's quantile index, computed on the host.
// Outputs:  mean = m, sd, ess_mean = ESS(A), ess_sd = ESS(B), mcse_mean = sd / sqrt(ess_mean),
//   mcse_sd = sqrt((E4 - E2^2) / ESS(C) / E2 / 4) (the delta method),  quantile[k] = sorted[j_k],  ess_quantile[k] = ESS(D_k),
//   mcse_quantile[k] = (sorted[i2] - sorted[i1]) / 2 with e = ess_quantile[k], a = qbeta(0.15865525393145707; e p + 1, e (1 - p) + 1),
//   b = qbeta(0.8413447460685429; the same shapes), i1 = max(floor(a S), 1) - 1, i2 = min(ceil(b S), S) - 1 (qbeta on the host:
//   csrc/qbeta.hpp),  acf [nlags + 1]: rho_t of series A, rho_0 = 1, rho_t = 1 - (W - g(t)) / V, NaN beyond L,
//   truncated: bit 0 A, bit 1 B, bit 2 C, bit 3 + k D_k.
// A NaN or an infinity in the window (read off the ends of the sorted column) turns every figure of the column into NaN; a series
// without W > 0 gives a NaN ESS and every figure derived from it is NaN (the acf with series A).
//
//   rh_mcse_stage_kernel /    the rank diagnostics' stage tile, tile sort and merge pass: y [column][S] and two key buffers.
//   rh_mcse_sort_kernel /
//   rh_mcse_merge_kernel
//   rh_mcse_moment_kernel     one workgroup per column: m, then E2 and E4 in one pass, through fixed trees.  mom [column][3].
//   rh_mcse_chain_kernel      one workgroup = one (column, series, sequence), MK_BLOCK threads.  The series' transform is applied while
//                             y is read -- for the mean and while the sequence is staged into LDS --, so no derived series is ever
//                             written to memory; from there rk_chain_block's arithmetic unchanged: the same mean tree, the same
//                             centring, one accumulator per lag with i ascending (d_i a broadcast read, d_{i+t} a unit-stride one: no
//                             bank conflict), the same time tiles with a halo of L values beyond RK_LDS_DOUBLES.  Its LDS is the
//                             launch's: max(h, MK_BLOCK) doubles up to RK_LDS_DOUBLES, not 63 KiB whatever h is.
//                             -> ws [column of the chunk][series][M][sl] = { m_q, g_q(0 .. L) }
//   rh_mcse_finish_kernel     one workgroup per (column, series): rk_series_finish; series A also writes its acf from the sums that
//                             routine leaves in LDS.  fin [column][3 + nprobs][3] = rhat, ess, truncated.
//   rh_mcse_pick_kernel       one thread per (column of the chunk, probability): sorted[j], (sorted[i2] - sorted[i1]) / 2 with the
//                             indices the host made from the chunk's ess_quantile.
//   rh_mcse_combine_kernel    one thread per column: the figures from mom and fin.
//
// No floating-point atomics; every sum has a fixed order that depends on the shape alone: a second call, a window and its copy, a
// duplicated column and any chunking of the columns give the same bits.
// Workspace per column: y and two key buffers of S 8-byte words each, and ws [3 + nprobs][M][L + 2]; there is no series buffer.  The
// host walks the columns in chunks below MK_WS_CAP_BYTES and refuses a single column beyond it.
//
// The block routines are plain C++ over (thread id, LDS pointer): with RH_MCSE_HOST (and RH_RANK_HOST, RH_SUMMARY_HOST) defined they
// compile with a host compiler, every "thread" of a phase run in turn (tests/test_mcse_device_cpu.py): same text, same summation order.
#ifndef RH_MCSE_HIP_H
#define RH_MCSE_HIP_H
#ifndef RH_RANK_HIP_H
#error "rh_mcse.hip.h follows rh_summary.hip.h and rh_rank.hip.h in its translation unit"
#endif

#define MK_BLOCK RK_BLOCK       // threads of every kernel here: the rank diagnostics' routines run in the same workgroups
#define MK_MAXPROBS 16
#define MK_NFIXED 3             // series 0 A: y, 1 B: |y - m|, 2 C: (y - m)^2; series 3 + k: the indicator of probs[k]
#define MK_NMOM 3               // m, E2, E4 per column
#define MK_NPICK 3              // j, i1, i2 per (column, probability); i1 < 0: no ess, mcse_quantile is NaN
#define MK_WS_CAP_BYTES (128ll << 20)
// doubles of LDS mk_chain_block touches for sequences of h values: the mean's tree (MK_BLOCK) and the centred sequence, whole when
// h <= RK_LDS_DOUBLES, else a time tile and its halo
#define MK_CHAIN_LDS(h) ((h) > RK_LDS_DOUBLES ? RK_LDS_DOUBLES : (h) > MK_BLOCK ? (h) : MK_BLOCK)
#define MK_FN RK_FN

// ---- the pooled moments of one column ------------------------------------------------------------------------------------------------
// y: the column's S values in flat order; sorted: its keys.  lds: MK_BLOCK doubles.  mom: m, E2, E4 (NaN with a NaN or an infinity)
MK_FN void mk_moment_block(const double *y, const rs_key *sorted, const long long S, double *lds, double *mom, const int rk_nthreads) {
  const int rs_nthreads = rk_nthreads;
  (void)rs_nthreads;
  RK_EACH_THREAD(tid) {
    double a = 0.0;
    for (long long s = tid; s < S; s += MK_BLOCK) a += y[s];
    lds[tid] = a;
  }
  rs_tree_sum(lds, rs_nthreads);
  const double m = lds[0] / (double)S;
  RK_SYNC();
  RK_EACH_THREAD(tid) {
    double a = 0.0;
    for (long long s = tid; s < S; s += MK_BLOCK) { const double d = y[s] - m; a += d * d; }
    lds[tid] = a;
  }
  rs_tree_sum(lds, rs_nthreads);
  const double e2 = lds[0] / (double)S;
  RK_SYNC();
  RK_EACH_THREAD(tid) {
    double a = 0.0;
    for (long long s = tid; s < S; s += MK_BLOCK) { const double d = y[s] - m, d2 = d * d; a += d2 * d2; }
    lds[tid] = a;
  }
  rs_tree_sum(lds, rs_nthreads);
  RK_EACH_THREAD(tid) {
    if (tid == 0) {
      const bool bad = sorted[0] <= RK_KEY_NEG_INF || sorted[S - 1] >= RK_KEY_POS_INF;
      const double nan = rs_from_key(RS_KEY_NAN);
      mom[0] = bad ? nan : m;
      mom[1] = bad ? nan : e2;
      mom[2] = bad ? nan : lds[0] / (double)S;
    }
  }
}

// ---- one sequence of one series of one column --------------------------------------------------------------------------------------------
// the value of series `kind` at y: m the column's pooled mean, thr the key of the series' order statistic
MK_FN double mk_value(const int kind, const double m, const rs_key thr, const double y) {
  if (kind == 0) return y;
  if (kind >= MK_NFIXED) return rk_indicator(thr, y);
  const double d = y - m;
  return kind == 1 ? __builtin_fabs(d) : d * d;
}

// rk_chain_block with u_i = mk_value(kind, m, thr, y_i) made where y_i is read.  y: the sequence's h values; L <= min(h - 1, RK_MAXLAG).
// lds: MK_CHAIN_LDS(h) doubles.  out: { mean, g(0) .. g(L) }
MK_FN void mk_chain_block(const double *y, const int kind, const double m, const rs_key thr, const int h, const int L, double *lds, double *out,
                          const int rk_nthreads) {
  const int rs_nthreads = rk_nthreads;
  (void)rs_nthreads;
  double acc[RK_NSTATE];
  RK_EACH_THREAD(tid) {
    double a = 0.0;
    for (int i = tid; i < h; i += RK_BLOCK) a += mk_value(kind, m, thr, y[i]);
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
      for (int j = t0 + tid; j < e1; j += RK_BLOCK) lds[j - t0] = mk_value(kind, m, thr, y[j]) - mean;
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

// ---- the autocorrelations of series A ----------------------------------------------------------------------------------------------------
// after rk_series_finish(w, ..., lds, fin): lds[e] still holds the sums over q of w[q][e].  W, B and V as that routine forms them (B's
// sum in sequence order); acf [nlags + 1]: rho_0 = 1, rho_t = 1 - (W - g(t)) / V, NaN beyond L and where the series has no ess
MK_FN void mk_acf(const double *w, const double *lds, const double *fin, const int M, const int h, const int L, const int sl, const int nlags,
                  double *acf, const int rk_nthreads) {
  const double m = (double)M, hh = (double)h, nan = rs_from_key(RS_KEY_NAN);
  const double mm = lds[0] / m;
  double bs = 0.0;
  for (int q = 0; q < M; q++) { const double d = w[(long long)q * sl] - mm; bs += d * d; }
  const double W = lds[1] / m * hh / (hh - 1.0), B = bs / (m - 1.0), V = (hh - 1.0) / hh * W + B;
  const bool none = fin[1] != fin[1];
  RK_EACH_THREAD(tid) {
    if (tid <= nlags) acf[tid] = (none || tid > L) ? nan : tid == 0 ? 1.0 : 1.0 - (W - lds[1 + tid] / m) / V;
  }
}

// ---- per (column, probability): the order statistics ---------------------------------------------------------------------------------------
// pick: j, i1, i2.  quantile = sorted[j]; mcse = (sorted[i2] - sorted[i1]) / 2, NaN where i1 < 0; both NaN with a NaN or an infinity
MK_FN void mk_pick(const rs_key *sorted, const long long S, const long long *pick, double *quantile, double *mcse) {
  const bool bad = sorted[0] <= RK_KEY_NEG_INF || sorted[S - 1] >= RK_KEY_POS_INF;
  const double nan = rs_from_key(RS_KEY_NAN);
  *quantile = bad ? nan : rs_from_key(sorted[pick[0]]);
  *mcse = (bad || pick[1] < 0) ? nan : (rs_from_key(sorted[pick[2]]) - rs_from_key(sorted[pick[1]])) / 2.0;
}

// ---- per column: the figures ---------------------------------------------------------------------------------------------------------------
// mom [MK_NMOM], fin [nseries][RK_NFIN] of one column
MK_FN void mk_combine(const double *mom, const double *fin, const long long S, const int nprobs, double *mean, double *sd, double *ess_mean,
                      double *ess_sd, double *mcse_mean, double *mcse_sd, double *ess_quantile, int *truncated) {
  const double m = mom[0], e2 = mom[1], e4 = mom[2];
  const double s = __builtin_sqrt((double)S * e2 / ((double)S - 1.0));
  const double ea = fin[1], eb = fin[RK_NFIN + 1], ec = fin[2 * RK_NFIN + 1];
  int tr = (fin[2] != 0.0 ? 1 : 0) | (fin[RK_NFIN + 2] != 0.0 ? 2 : 0) | (fin[2 * RK_NFIN + 2] != 0.0 ? 4 : 0);
  for (int k = 0; k < nprobs; k++) {
    ess_quantile[k] = fin[(MK_NFIXED + k) * RK_NFIN + 1];
    tr |= fin[(MK_NFIXED + k) * RK_NFIN + 2] != 0.0 ? 1 << (MK_NFIXED + k) : 0;
  }
  *mean = m;
  *sd = s;
  *ess_mean = ea;
  *ess_sd = eb;
  *mcse_mean = s / __builtin_sqrt(ea);
  *mcse_sd = __builtin_sqrt((e4 - e2 * e2) / ec / e2 / 4.0);
  *truncated = tr;
}

#ifndef RH_MCSE_HOST
// The workspace holds, for the chunk's columns [k_lo, k_lo + p_cnt) of the selection, y [p_cnt][S], two key buffers [p_cnt][S] and
// ws [p_cnt][nseries][M][sl].
// grid: tiles of RK_ROWS flat values x tiles of RK_TP columns, blockIdx.x = row tile * ctiles + column tile
extern "C" __global__ void __launch_bounds__(MK_BLOCK)
rh_mcse_stage_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const long long first,
                     const long long count, const long long h, const long long S, const int *__restrict__ cols, const int p_cnt,
                     const int ctiles, double *__restrict__ y) {
  __shared__ double lds[RK_TP * RK_STAGE_STRIDE];
  const long long rt = (long long)(blockIdx.x / (unsigned)ctiles);
  const int pl = (int)(blockIdx.x - (unsigned)rt * (unsigned)ctiles) * RK_TP;
  const long long s0 = rt * RK_ROWS;
  if (s0 >= S || pl >= p_cnt) return;
  rk_stage_tile(draws, iterations, nvars, first, count, h, S, cols + pl, p_cnt - pl < RK_TP ? p_cnt - pl : RK_TP, s0, lds, y + (long long)pl * S, MK_BLOCK);
}

// grid: tiles x p_cnt, blockIdx.x = tile * p_cnt + column: a dense column is one flat chain
extern "C" __global__ void __launch_bounds__(MK_BLOCK)
rh_mcse_sort_kernel(const double *__restrict__ y, const long long S, const int p_cnt, rs_key *__restrict__ keys) {
  __shared__ rs_key lds[RS_TILE_SLOTS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt), g0 = tile * RS_TILE;
  if (g0 >= S) return;
  rs_tile_sort(y + pl * S, S, 1, 1, S, S, g0, lds, keys + pl * S + g0, MK_BLOCK);
}

// one merge pass over runs of L keys, src -> dst ([p_cnt][S] each); grid: ceil(S / RS_MERGE_TILE) x p_cnt
extern "C" __global__ void __launch_bounds__(MK_BLOCK)
rh_mcse_merge_kernel(const rs_key *__restrict__ src, rs_key *__restrict__ dst, const long long S, const long long L, const int p_cnt) {
  __shared__ rs_key lds[RS_MERGE_LDS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt), o0 = tile * RS_MERGE_TILE;
  if (o0 >= S) return;
  rs_merge_tile(src + pl * S, dst + pl * S, S, L, o0, lds, MK_BLOCK);
}

// grid: the chunk's columns; mom is indexed by the column's place in the selection, k_lo + blockIdx.x
extern "C" __global__ void __launch_bounds__(MK_BLOCK)
rh_mcse_moment_kernel(const double *__restrict__ y, const rs_key *__restrict__ sorted, const long long S, const int k_lo, double *__restrict__ mom) {
  __shared__ double lds[MK_BLOCK];
  const long long pl = (long long)blockIdx.x;
  mk_moment_block(y + pl * S, sorted + pl * S, S, lds, mom + (k_lo + pl) * MK_NMOM, MK_BLOCK);
}

// grid: p_cnt x nseries x M, blockIdx.x = (column * nseries + series) * M + sequence; idx [nseries - MK_NFIXED]: the order statistics.
// The launch's dynamic LDS is MK_CHAIN_LDS(h) doubles: a short sequence does not hold the 63 KiB a long one needs, so that more
// than two workgroups share a CU's 160 KiB when h is small and there are many sequences.
extern __shared__ double mk_lds[];
extern "C" __global__ void __launch_bounds__(MK_BLOCK)
rh_mcse_chain_kernel(const double *__restrict__ y, const rs_key *__restrict__ sorted, const double *__restrict__ mom,
                     const long long *__restrict__ idx, const long long S, const int M, const int h, const int L, const int sl, const int nseries,
                     const int k_lo, double *__restrict__ ws) {
  double *lds = mk_lds;
  const unsigned cs = blockIdx.x / (unsigned)M;
  const int q = (int)(blockIdx.x - cs * (unsigned)M);
  const long long pl = (long long)(cs / (unsigned)nseries);
  const int kind = (int)(cs - (unsigned)pl * (unsigned)nseries);
  const double m = mom[(k_lo + pl) * MK_NMOM];
  const rs_key thr = kind >= MK_NFIXED ? sorted[pl * S + idx[kind - MK_NFIXED]] : 0ull;
  mk_chain_block(y + pl * S + (long long)q * h, kind, m, thr, h, L, lds, ws + (long long)blockIdx.x * sl, MK_BLOCK);
}

// grid: p_cnt x nseries, blockIdx.x = column * nseries + series; fin and acf are indexed by the column's place in the selection
extern "C" __global__ void __launch_bounds__(MK_BLOCK)
rh_mcse_finish_kernel(const double *__restrict__ ws, const rs_key *__restrict__ sorted, const long long S, const int M, const int h, const int L,
                      const int sl, const double tau_min, const int nseries, const int k_lo, const int nlags, double *__restrict__ fin,
                      double *__restrict__ acf) {
  __shared__ double lds[RK_SL + RK_BLOCK];
  const long long pl = (long long)(blockIdx.x / (unsigned)nseries);
  const int kind = (int)(blockIdx.x - (unsigned)pl * (unsigned)nseries);
  const double *w = ws + (long long)blockIdx.x * M * sl;
  double *f = fin + ((k_lo + pl) * nseries + kind) * RK_NFIN;
  rk_series_finish(w, sorted + pl * S, S, M, h, L, sl, tau_min, lds, f, MK_BLOCK);
  if (kind != 0) return;
  RK_SYNC();                                       // thread 0 wrote f; every thread reads it
  mk_acf(w, lds, f, M, h, L, sl, nlags, acf + (k_lo + pl) * (nlags + 1), MK_BLOCK);
}

// grid: ceil(p_cnt * nprobs / MK_BLOCK); pick [p_cnt][nprobs][MK_NPICK] of the chunk; quantile and mcse [K][nprobs]
extern "C" __global__ void __launch_bounds__(MK_BLOCK)
rh_mcse_pick_kernel(const rs_key *__restrict__ sorted, const long long S, const int p_cnt, const int nprobs, const int k_lo,
                    const long long *__restrict__ pick, double *__restrict__ quantile, double *__restrict__ mcse) {
  const int e = (int)(blockIdx.x * MK_BLOCK + threadIdx.x);
  if (e >= p_cnt * nprobs) return;
  const long long pl = e / nprobs;
  const long long o = (long long)k_lo * nprobs + e;
  mk_pick(sorted + pl * S, S, pick + (long long)e * MK_NPICK, quantile + o, mcse + o);
}

// grid: ceil(K / MK_BLOCK)
extern "C" __global__ void __launch_bounds__(MK_BLOCK)
rh_mcse_combine_kernel(const double *__restrict__ mom, const double *__restrict__ fin, const long long S, const int K, const int nprobs,
                       double *__restrict__ mean, double *__restrict__ sd, double *__restrict__ ess_mean, double *__restrict__ ess_sd,
                       double *__restrict__ mcse_mean, double *__restrict__ mcse_sd, double *__restrict__ ess_quantile, int *__restrict__ truncated) {
  const int k = (int)(blockIdx.x * MK_BLOCK + threadIdx.x);
  if (k < K)
    mk_combine(mom + (long long)k * MK_NMOM, fin + (long long)k * (MK_NFIXED + nprobs) * RK_NFIN, S, nprobs, mean + k, sd + k, ess_mean + k, ess_sd + k,
               mcse_mean + k, mcse_sd + k, ess_quantile + (long long)k * nprobs, truncated + k);
}
#endif
#endif
