// draws_plan.hpp -- the launch plans of the calls over device-resident draws (draws.cpp): how many parameters share a bounded
// workspace, how many tiles and merge passes, which order statistics, how many tile pairs of a covariance, how many column tiles and edges of a histogram, how many columns and lags of the rank diagnostics, how many series of the standard errors and which order statistics bracket a quantile, how long the tail of a PSIS column, how many pairs of a leave-one-out expectation or of its quantiles and scores, how many rows and lanes of a predictive check, which predict kernel, how many sampling tiles and slabs.  Arithmetic only: no HIP, no allocation,
// no globals.  draws.cpp launches what these functions say, and the CPU tests' drivers of the device text walk the same plan.
#ifndef RH_DRAWS_PLAN_HPP
#define RH_DRAWS_PLAN_HPP

#include <algorithm>
#include <cmath>

#include "qbeta.hpp"

// the constants are the device headers' own: their block routines compile as plain C++ in host mode
#define RH_TRACE_HOST 1
#define RH_SUMMARY_HOST 1
#define RH_COV_HOST 1
#define RH_HIST_HOST 1
#define RH_RANK_HOST 1
#define RH_MCSE_HOST 1
#define RH_LOO_HOST 1
#define RH_LOO_EXPECT_HOST 1
#define RH_LOO_QUANTILE_HOST 1
#define RH_PPC_HOST 1
#include "device/rh_trace.hip.h"
#include "device/rh_summary.hip.h"
#include "device/rh_cov.hip.h"
#include "device/rh_hist.hip.h"
#include "device/rh_rank.hip.h"
#include "device/rh_mcse.hip.h"
#include "device/rh_loo.hip.h"
#include "device/rh_loo_expect.hip.h"
#include "device/rh_loo_quantile.hip.h"
#include "device/rh_ppc.hip.h"
// rh_generate.hip.h's routine needs the prelude's rng around it: the CPU test's driver defines RH_GENERATE_HOST with one in place
#ifndef RH_GENERATE_HOST
#define RG_CONSTANTS_ONLY 1
#endif
#include "device/rh_generate.hip.h"
#include "device/rh_generate_ext.hip.h"
namespace rh_plan {
// ---- trace diagnostics (device/rh_trace.hip.h) ----
// parameters per chunk: the workspace [chunk][chains][RT_SL] stays under the cap; whole tiles where a tile fits
inline long long trace_chunk(int chains, int nvars) {
  long long pc = RT_WS_CAP_BYTES / ((long long)chains * RT_SL * (long long)sizeof(double));
  pc = std::max<long long>(1, std::min<long long>(pc, nvars));
  if (pc >= RT_TP) pc -= pc % RT_TP;
  return pc;
}
inline long long trace_tiles(long long p_cnt) { return (p_cnt + RT_TP - 1) / RT_TP; }
// ---- posterior summaries (device/rh_summary.hip.h) ----
struct Summary {
  long long kept, N;             // kept iterations per chain; values of one pooled column
  long long per_param, pc;       // workspace bytes of one parameter (the two ping-pong buffers of keys); parameters per chunk
  bool over_cap;                 // one column alone is beyond RS_WS_CAP_BYTES
  long long tiles, mtiles;       // tile sorts and merge workgroups per parameter
  int passes;                    // merge passes; pass k merges runs of run(k) keys
  long long idx[RS_MAX_PROBS];   // order statistics (precis: data(math.floor(data.size * q).toInt))
  long long hidx;                // hdpi's span (math.ceil(prob * sorted.size).toInt, in 1 .. N); 0: not asked for
  long long run(int k) const { return (long long)RS_TILE << k; }
};
inline Summary summary_plan(long long chains, long long count, long long thin, long long nvars, const double *probs, int nprobs, double hdpi_prob) {
  Summary P = {};
  P.kept = (count + thin - 1) / thin;
  P.N = chains * P.kept;
  P.per_param = 2 * P.N * (long long)sizeof(unsigned long long);
  P.over_cap = P.per_param > RS_WS_CAP_BYTES;
  P.pc = std::max<long long>(1, std::min<long long>(RS_WS_CAP_BYTES / P.per_param, nvars));
  P.tiles = (P.N + RS_TILE - 1) / RS_TILE;
  P.mtiles = (P.N + RS_MERGE_TILE - 1) / RS_MERGE_TILE;
  while (P.run(P.passes) < P.N) P.passes++;
  for (int k = 0; k < nprobs; k++) P.idx[k] = std::min<long long>(P.N - 1, (long long)std::floor((double)P.N * probs[k]));
  if (hdpi_prob > 0.0) P.hidx = std::max<long long>(1, std::min<long long>(P.N, (long long)std::ceil(hdpi_prob * (double)P.N)));
  return P;
}
// ---- covariance / correlation (device/rh_cov.hip.h) ----
struct Covariance {
  long long kept, N, S;          // kept iterations per chain; flat rows; splits of RC_SPLIT rows
  long long ctiles, pairs;       // column tiles of RC_TC; tile pairs bi <= bj, in rc_pair_of's order
  long long per_pair, pc;        // workspace bytes of one tile pair (its S partial tiles); tile pairs per chunk
  bool over_cap;                 // one tile pair alone is beyond the cap
};
// K: the selected columns; cap: RC_WS_CAP_BYTES (a parameter for the CPU tests' driver, where small shapes make several chunks)
inline Covariance covariance_plan(long long chains, long long count, long long thin, long long K, long long cap = RC_WS_CAP_BYTES) {
  Covariance P = {};
  P.kept = (count + thin - 1) / thin;
  P.N = chains * P.kept;
  P.S = (P.N + RC_SPLIT - 1) / RC_SPLIT;
  P.ctiles = (K + RC_TC - 1) / RC_TC;
  P.pairs = P.ctiles * (P.ctiles + 1) / 2;
  P.per_pair = RC_PAIR_BYTES(P.S);
  P.over_cap = P.per_pair > cap;
  P.pc = std::max<long long>(1, std::min<long long>(cap / P.per_pair, P.pairs));
  return P;
}
// ---- histograms and joint count grids (device/rh_hist.hip.h) ----
struct Histogram {
  long long kept, N, S;          // kept iterations per chain; flat rows; splits of RHH_SPLIT rows
  long long cpt, tiles, mtiles;  // columns of a tile at this nbins (rhh_tile_cols); tiles of the binning pass; tiles of RHH_TC of the min / max pass
  long long lds_bytes;           // the binning launch's dynamic LDS
  long long per_tile, tc;        // workspace bytes of one tile (its S partial histograms); tiles per chunk
  bool over_cap;                 // one tile alone is beyond the cap
};
// K: the selected columns; cap: RHH_WS_CAP_BYTES (a parameter for the CPU tests' driver, where small shapes make several chunks)
inline Histogram histogram_plan(long long chains, long long count, long long thin, long long K, int nbins, long long cap = RHH_WS_CAP_BYTES) {
  Histogram P = {};
  P.kept = (count + thin - 1) / thin;
  P.N = chains * P.kept;
  P.S = (P.N + RHH_SPLIT - 1) / RHH_SPLIT;
  P.cpt = rhh_tile_cols(nbins);
  P.tiles = (K + P.cpt - 1) / P.cpt;
  P.mtiles = (K + RHH_TC - 1) / RHH_TC;
  P.lds_bytes = P.cpt * RHH_COL_BYTES(nbins);
  P.per_tile = P.S * P.cpt * (nbins + RHH_TALLIES) * 4;
  P.over_cap = P.per_tile > cap;
  P.tc = std::max<long long>(1, std::min<long long>(cap / P.per_tile, P.tiles));
  return P;
}
struct Histogram2d {
  long long kept, N, S;          // as above
  long long words, lds_bytes;    // u32 words of one partial (nbx * nby cells and the rows outside); the pair launch's dynamic LDS
  long long per_pair, pc;        // workspace bytes of one pair; pairs per chunk
  bool over_cap;
};
inline Histogram2d histogram2d_plan(long long chains, long long count, long long thin, long long npairs, int nbx, int nby, long long cap = RHH_WS_CAP_BYTES) {
  Histogram2d P = {};
  P.kept = (count + thin - 1) / thin;
  P.N = chains * P.kept;
  P.S = (P.N + RHH_SPLIT - 1) / RHH_SPLIT;
  P.words = RHH_PAIR_WORDS(nbx, nby);
  P.lds_bytes = RHH_PAIR_LDS(nbx, nby);
  P.per_pair = P.S * P.words * 4;
  P.over_cap = P.per_pair > cap;
  P.pc = std::max<long long>(1, std::min<long long>(cap / P.per_pair, npairs));
  return P;
}
// given bounds (range != NULL and not both NaN) are used as they are, else the automatic ones; lo == hi: numpy's rule
inline bool histogram_auto(const double *range) { return !range || (std::isnan(range[0]) && std::isnan(range[1])); }
inline bool histogram_range_ok(const double *range) {
  return histogram_auto(range) || (std::isfinite(range[0]) && std::isfinite(range[1]) && range[0] <= range[1] && std::isfinite(range[1] - range[0]));
}
// e [nbins + 1] from the bounds, in double: non-decreasing by construction; NaN bounds (a column without a finite value): NaN edges
// (a constant of magnitude 2^53 or more: lo - 0.5 == lo, the width stays 0, all edges are equal and every row counts in the last,
// closed bin -- what the counts' definition against the edges gives; the density of a bin without width is NaN)
inline void histogram_edges(double lo, double hi, int nbins, double *e) {
  if (lo == hi) { lo -= 0.5; hi += 0.5; }
  if (std::isnan(lo) || std::isnan(hi)) { for (int i = 0; i <= nbins; i++) e[i] = std::nan(""); return; }
  const double w = hi - lo;
  e[0] = lo;
  for (int i = 1; i < nbins; i++) e[i] = std::min(hi, std::max(e[i - 1], lo + ((double)i * w) / (double)nbins));
  e[nbins] = hi;
}
// ---- rank-normalised split R-hat, bulk and tail ESS (device/rh_rank.hip.h) ----
struct Rank {
  long long h, M, S;             // values of a half; sequences (2 per chain); values of one column
  int L, sl;                     // lags 0 .. L of the bulk and tail series (min(h - 1, RK_MAXLAG)); doubles per (column, sequence) of ws: L + 2
  long long per_col, pc;         // workspace bytes of one column (y, two key buffers, one series buffer, ws); columns per chunk
  bool over_cap;                 // one column alone is beyond the cap
  long long tiles, mtiles;       // tile sorts and merge workgroups per column: the summary's plan of one flat chain of S values
  int passes;                    // merge passes; pass k merges runs of run(k) keys
  long long stiles, blocks;      // stage tiles of RK_ROWS flat values; blocks of RK_BLOCK values of the per-value kernels
  long long i05, i95;            // the tail thresholds' order statistics (precis: floor(S * q)), as summary_plan computes idx
  double tau_min;                // 1 / log10(S)
  long long run(int k) const { return (long long)RS_TILE << k; }
};
// K: the selected columns; cap: RK_WS_CAP_BYTES (a parameter for the CPU tests' driver, where small shapes make several chunks)
inline Rank rank_plan(long long chains, long long count, long long K, long long cap = RK_WS_CAP_BYTES) {
  Rank P = {};
  P.h = count / 2;
  P.M = 2 * chains;
  P.S = P.M * P.h;
  P.L = (int)std::min<long long>(P.h - 1, RK_MAXLAG);
  P.sl = P.L + 2;
  P.per_col = 4 * P.S * 8 + P.M * P.sl * 8;
  P.over_cap = P.per_col > cap;
  P.pc = std::max<long long>(1, std::min<long long>(cap / P.per_col, K));
  const double tails[2] = {0.05, 0.95};
  const Summary Q = summary_plan(1, P.S, 1, 1, tails, 2, 0.0);
  P.tiles = Q.tiles; P.mtiles = Q.mtiles; P.passes = Q.passes;
  P.i05 = Q.idx[0]; P.i95 = Q.idx[1];
  P.stiles = (P.S + RK_ROWS - 1) / RK_ROWS;
  P.blocks = (P.S + RK_BLOCK - 1) / RK_BLOCK;
  P.tau_min = 1.0 / std::log10((double)P.S);
  return P;
}
// ---- Monte Carlo standard errors and ESS of the reported figures (device/rh_mcse.hip.h) ----
struct Mcse {
  long long h, M, S;             // as Rank's
  int L, sl;                     // as Rank's
  int nprobs, nseries;           // probabilities; series per column: MK_NFIXED + nprobs
  long long per_col, pc;         // workspace bytes of one column (y, two key buffers, ws [nseries][M][sl]: no series buffer); columns per chunk
  bool over_cap;                 // one column alone is beyond the cap
  long long tiles, mtiles;       // as Rank's: the summary's plan of one flat chain of S values
  int passes;
  long long stiles;              // stage tiles of RK_ROWS flat values
  long long chain_lds;           // the chain launch's dynamic LDS in bytes: MK_CHAIN_LDS(h) doubles
  long long idx[MK_MAXPROBS];   // the quantiles' order statistics j_k (precis: floor(S * p)), as summary_plan computes idx
  double tau_min;                // 1 / log10(S)
  long long run(int k) const { return (long long)RS_TILE << k; }
};
// K: the selected columns; probs [nprobs], nprobs <= MK_MAXPROBS; cap: MK_WS_CAP_BYTES (a parameter for the CPU tests' driver, where small shapes make several chunks)
inline Mcse mcse_plan(long long chains, long long count, long long K, const double *probs, int nprobs, long long cap = MK_WS_CAP_BYTES) {
  Mcse P = {};
  const Rank R = rank_plan(chains, count, K, cap);
  P.h = R.h; P.M = R.M; P.S = R.S; P.L = R.L; P.sl = R.sl;
  P.tiles = R.tiles; P.mtiles = R.mtiles; P.passes = R.passes; P.stiles = R.stiles; P.tau_min = R.tau_min;
  P.nprobs = nprobs;
  P.nseries = MK_NFIXED + nprobs;
  P.chain_lds = 8 * (long long)MK_CHAIN_LDS(P.h);
  P.per_col = 3 * P.S * 8 + (long long)P.nseries * P.M * P.sl * 8;
  P.over_cap = P.per_col > cap;
  P.pc = std::max<long long>(1, std::min<long long>(cap / P.per_col, K));
  const Summary Q = summary_plan(1, P.S, 1, 1, probs, nprobs, 0.0);
  for (int k = 0; k < nprobs; k++) P.idx[k] = Q.idx[k];
  return P;
}
// the order statistics whose half distance is the standard error of the quantile at probability p with effective sample size e:
// the 16 % and 84 % points a, b of Beta(e p + 1, e (1 - p) + 1); i1 = max(floor(a S), 1) - 1, i2 = min(ceil(b S), S) - 1.
// pick: j, i1, i2 (MK_NPICK); no ess (NaN, or not above 0): i1 = i2 = -1
inline void mcse_pick(long long S, long long j, double p, double e, long long *pick) {
  pick[0] = j; pick[1] = -1; pick[2] = -1;
  if (!(e > 0.0) || !std::isfinite(e)) return;
  const double sa = e * p + 1.0, sb = e * (1.0 - p) + 1.0;
  const double a = rh_qbeta::qbeta(0.15865525393145707, sa, sb), b = rh_qbeta::qbeta(0.8413447460685429, sa, sb);
  if (!(a == a) || !(b == b)) return;
  pick[1] = std::max<long long>((long long)std::floor(a * (double)S), 1) - 1;
  pick[2] = std::min<long long>((long long)std::ceil(b * (double)S), S) - 1;
}
// ---- pointwise WAIC and PSIS-LOO (device/rh_loo.hip.h) ----
struct Loo {
  long long kept, S;             // kept iterations per chain; values of one pooled column
  long long M, cut;              // the most tail values, ceil(min(S / 5, 3 sqrt(S))); the cutoff's order statistic x_(cut) of the ascending ratios, cut = S - M (1-based)
  long long per_col, pc;         // workspace bytes of one column (the two key buffers); columns per chunk
  bool over_cap, over_lds;       // one column alone is beyond the cap; M is beyond the tail's LDS (LL_TAIL_MAX)
  long long tiles, mtiles;       // tile sorts and merge workgroups per column: the summary's plan
  int passes;                    // merge passes; pass k merges runs of run(k) keys
  long long run(int k) const { return (long long)RS_TILE << k; }
};
// K: the selected columns; cap: LL_WS_CAP_BYTES (a parameter for the CPU tests' driver, where small shapes make several chunks)
inline Loo loo_plan(long long chains, long long count, long long thin, long long K, long long cap = LL_WS_CAP_BYTES) {
  Loo P = {};
  const Summary Q = summary_plan(chains, count, thin, 1, nullptr, 0, 0.0);
  P.kept = Q.kept; P.S = Q.N;
  P.tiles = Q.tiles; P.mtiles = Q.mtiles; P.passes = Q.passes;
  P.M = (long long)std::ceil(std::min((double)P.S / 5.0, 3.0 * std::sqrt((double)P.S)));
  P.cut = P.S - P.M;
  P.per_col = 2 * P.S * (long long)sizeof(unsigned long long);
  P.over_cap = P.per_col > cap;
  P.over_lds = P.M > LL_TAIL_MAX;
  P.pc = std::max<long long>(1, std::min<long long>(cap / P.per_col, K));
  return P;
}
// ---- PSIS leave-one-out expectations (device/rh_loo_expect.hip.h) ----
struct LooExpect {
  long long kept, S, M;          // as Loo's
  long long per_pair, pc;        // workspace bytes of one pair (the two key buffers -- the spare one holds the draws' weights -- and the tail's weights [M]); pairs per chunk
  bool over_cap, over_lds;       // one pair alone is beyond the cap; M is beyond the tail's LDS (LL_TAIL_MAX)
  long long tiles, mtiles;       // tile sorts and merge workgroups per pair: the summary's plan
  int passes;                    // merge passes; pass k merges runs of run(k) keys
  long long run(int k) const { return (long long)RS_TILE << k; }
};
// K: the selected pairs; cap: LX_WS_CAP_BYTES (a parameter for the CPU tests' driver, where small shapes make several chunks)
inline LooExpect loo_expect_plan(long long chains, long long count, long long thin, long long K, long long cap = LX_WS_CAP_BYTES) {
  LooExpect P = {};
  const Loo Q = loo_plan(chains, count, thin, 1, cap);
  P.kept = Q.kept; P.S = Q.S; P.M = Q.M;
  P.tiles = Q.tiles; P.mtiles = Q.mtiles; P.passes = Q.passes;
  P.per_pair = LX_PAIR_BYTES(P.S, P.M);
  P.over_cap = P.per_pair > cap;
  P.over_lds = Q.over_lds;
  P.pc = std::max<long long>(1, std::min<long long>(cap / P.per_pair, K));
  return P;
}
// ---- leave-one-out predictive quantiles and CRPS (device/rh_loo_quantile.hip.h) ----
struct LooQuantile {
  long long kept, S, M;          // as Loo's
  long long per_pair, pc;        // workspace bytes of one pair (two buffers of keys and payloads, 32 S -- the log-likelihood side sorts inside the second -- and the tail's weights [M]); pairs per chunk
  bool over_cap, over_lds;       // one pair alone is beyond the cap; M is beyond the tail's LDS (LL_TAIL_MAX)
  long long tiles, mtiles;       // tile sorts and merge workgroups per pair, of either sort: the summary's plan (LQ_TILE == RS_TILE)
  int passes;                    // merge passes of either sort; pass k merges runs of run(k)
  long long seg;                 // draws of one thread's segment of the scan, ceil(S / LL_BLOCK)
  long long run(int k) const { return (long long)RS_TILE << k; }
};
// K: the selected pairs; cap: LQ_WS_CAP_BYTES (a parameter for the CPU tests' driver, where small shapes make several chunks)
inline LooQuantile loo_quantile_plan(long long chains, long long count, long long thin, long long K, long long cap = LQ_WS_CAP_BYTES) {
  LooQuantile P = {};
  const Loo Q = loo_plan(chains, count, thin, 1, cap);
  P.kept = Q.kept; P.S = Q.S; P.M = Q.M;
  P.tiles = Q.tiles; P.mtiles = Q.mtiles; P.passes = Q.passes;
  P.per_pair = LQ_PAIR_BYTES(P.S, P.M);
  P.over_cap = P.per_pair > cap;
  P.over_lds = Q.over_lds;
  P.pc = std::max<long long>(1, std::min<long long>(cap / P.per_pair, K));
  P.seg = (P.S + LL_BLOCK - 1) / LL_BLOCK;
  return P;
}
// ---- posterior predictive checks (device/rh_ppc.hip.h) ----
struct Ppc {
  long long kept, S;             // kept iterations per chain; flat rows (draws)
  int K, nseg, nstat, nout;      // selected columns; segments; statistics; nseg * nstat
  int nmax;                      // the longest segment
  int flags;                     // PP_F_*: what the table needs
  int team, team_log2, conc;     // lanes of an item's team, pp_width(nmax); items at once, PP_BLOCK / team
  int stride, rows;              // doubles between two staged rows; rows of a tile (rows * stride <= PP_STAGE, at most PP_BLOCK)
  long long tiles;               // workgroups of the stat launch
  int sortp, sort_stride;        // slots of the longest segment's network (0: no quantile); slots between two items' scratches
  long long lds_bytes;           // the stat launch's dynamic LDS
  long long count_rows, count_blocks, count_lds;   // rows per workgroup, workgroups and dynamic LDS of the count launch
  bool over_k, over_nstat, over_nout;              // beyond the caps: refused from the shape alone
};
// the order statistic of a QUANTILE(p) on a segment of n values: precis' rule, as summary_plan computes idx
inline int ppc_qidx(int n, double p) { return (int)std::min<long long>(n - 1, (long long)std::floor((double)n * p)); }
// seg_off [nseg + 1]: the runs of the K selected columns; kinds [nstat]
inline Ppc ppc_plan(long long chains, long long count, long long thin, int K, const int *seg_off, int nseg, const int *kinds, int nstat) {
  Ppc P = {};
  P.kept = (count + thin - 1) / thin;
  P.S = chains * P.kept;
  P.K = K; P.nseg = nseg; P.nstat = nstat;
  P.over_k = K > PP_MAX_K;
  P.over_nstat = nstat > PP_MAX_STATS;
  P.over_nout = (long long)nseg * nstat > PP_MAX_OUT;
  if (P.over_k || P.over_nstat || P.over_nout) return P;
  P.nout = nseg * nstat;
  for (int g = 0; g < nseg; g++) P.nmax = std::max(P.nmax, seg_off[g + 1] - seg_off[g]);
  for (int k = 0; k < nstat; k++)
    P.flags |= kinds[k] == PP_MEAN ? PP_F_MEAN : kinds[k] == PP_SD ? PP_F_MEAN | PP_F_SD : kinds[k] == PP_QUANTILE ? PP_F_SORT : 0;
  P.team = pp_width(P.nmax);
  while ((1 << P.team_log2) < P.team) P.team_log2++;
  P.conc = PP_BLOCK / P.team;
  P.stride = pp_stride(K);
  P.rows = std::max(1, std::min(PP_BLOCK, PP_STAGE / P.stride));
  for (int r = P.rows; r >= 1 && (long long)P.rows * nseg > P.conc; r--)   // whole passes where a smaller tile has them
    if ((long long)r * nseg % P.conc == 0) { P.rows = r; break; }
  P.tiles = (P.S + P.rows - 1) / P.rows;
  P.sortp = (P.flags & PP_F_SORT) ? pp_pow2(P.nmax) : 0;
  P.sort_stride = pp_sort_stride(P.conc, P.sortp);
  const long long scratch = std::max<long long>(2 * PP_BLOCK + 3 * P.conc, (long long)P.conc * P.sort_stride);
  P.lds_bytes = 8 * ((long long)P.rows * P.stride + scratch);
  P.count_rows = std::max<long long>(1, PP_COUNT_ELEMS / P.nout);
  P.count_blocks = (P.S + P.count_rows - 1) / P.count_rows;
  P.count_lds = 3ll * P.nout * 4;
  return P;
}
// ---- predict (device/rh_predict.hip.h) ----
// that header cannot be included without a generated program around it, so these four are mirrors: RP_WAVE, RP_MAX_TILE, RP_LDS_DOUBLES, RP_TILE_FOR
const int kPredWave = 64, kPredMaxTile = 256, kPredLdsDoubles = 8064;
inline int pred_tile_for(int stride) {
  const int rows = kPredLdsDoubles / stride;
  return rows >= kPredMaxTile ? kPredMaxTile : rows / kPredWave * kPredWave;
}
enum { PRED_FLAT = 0, PRED_GATHER = 1, PRED_DIRECT = 2 };   // RP_FLAT, RP_GATHER, RP_DIRECT
// which kernels a program's source holds (RP_HAVE_FLAT, RP_HAVE_GATHER; the direct kernel stands in for a missing gather kernel)
inline bool pred_has_flat(int nvars, int nref) { return pred_tile_for(nvars | 1) >= kPredWave && 2 * nref >= nvars; }
inline bool pred_has_gather(int nref) { return pred_tile_for(nref | 1) >= kPredWave; }
struct PredictLaunch { int form, tile; };
// flat when the program has that kernel and thin == 1, else gathered, else direct; the tile is the workgroup's size
inline PredictLaunch predict_launch(int nvars, int nref, int thin) {
  if (thin == 1 && pred_has_flat(nvars, nref)) return {PRED_FLAT, pred_tile_for(nvars | 1)};
  if (pred_has_gather(nref)) return {PRED_GATHER, pred_tile_for(nref | 1)};
  return {PRED_DIRECT, kPredWave};
}
// ---- posterior-predictive sampling (device/rh_generate.hip.h) ----
// one workgroup per RG_TILE flat rows; the results leave through LDS in slabs of at most RG_SLAB ops
inline long long generate_tiles(long long nrows) { return (nrows + RG_TILE - 1) / RG_TILE; }
inline int generate_slab(int nops) { return RG_SLAB_W(nops); }                       // ops per slab
inline int generate_slabs(int nops) { return (nops + generate_slab(nops) - 1) / generate_slab(nops); }
inline size_t generate_lds_bytes(int nops) { return sizeof(double) * (size_t)RG_TILE * (size_t)RG_STRIDE(nops); }   // the launch's dynamic LDS
// ---- its count families and composites (device/rh_generate_ext.hip.h): slabs are cut by VISIBLE outputs ----
inline bool generate_op_visible(const rg_op &op) { return (op.reserved & RGX_HIDDEN) == 0; }
inline int generate_visible(const rg_op *ops, int nops) { int n = 0; for (int o = 0; o < nops; o++) n += generate_op_visible(ops[o]) ? 1 : 0; return n; }   // nout
// does the table say anything rh_generate_kernel does not read: a family from 16, a guard, HIDDEN, PREV
inline bool generate_uses_ext(const rg_op *ops, int nops) {
  for (int o = 0; o < nops; o++)
    if (ops[o].family >= RGX_BINOMIAL || ops[o].reserved != 0 || ops[o].a.pad != 0 || ops[o].b.pad != 0) return true;
  return false;
}
// the ops of the slab that starts at op o0: up to and with its generate_slab(nout)-th visible op and the hidden ops that follow it
// (a slab starts at a visible op, or at op 0).  Returns the end of the slab's ops, *w: its visible ones.
inline int generate_ext_slab_end(const rg_op *ops, int nops, int nout, int o0, int *w) {
  int o1 = o0;
  *w = 0;
  while (o1 < nops && (*w < generate_slab(nout) || !generate_op_visible(ops[o1]))) { *w += generate_op_visible(ops[o1]) ? 1 : 0; o1++; }
  return o1;
}
inline int generate_ext_slabs(const rg_op *ops, int nops, int nout) {
  int n = 0, w = 0;
  for (int o0 = 0; o0 < nops; n++) o0 = generate_ext_slab_end(ops, nops, nout, o0, &w);
  return n;
}
inline size_t generate_ext_lds_bytes(int nout) { return generate_lds_bytes(nout); }   // the stride is the visible width's
}  // namespace rh_plan
#endif
