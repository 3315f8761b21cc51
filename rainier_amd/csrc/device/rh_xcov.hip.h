// rh_xcov.hip.h -- cross-covariance and cross-correlation of two device-resident draw sets: how the columns of one matrix (the
// parameters) move with the columns of another that was computed from the same draws (an observation's log-likelihood, a fitted
// value, a replicated observation).  A^T B of the centred rows on the fp64 matrix cores; Ka x Kb figures come back.  With B the
// pointwise log-likelihood, cross[k][i] is the influence of observation i on the posterior mean of parameter k, the raw material
// of the infinitesimal-jackknife covariance (Giordano and Broderick, "The Bayesian infinitesimal jackknife for variance").
//
// Model-independent: a translation unit of its own behind rh_cov.hip.h's text (its flat-row stepping, its mean routines, MFMA
// operand maps and host-mode macros), compiled once per toolchain through the engine's build_source() and inspected like every
// other code object before it is launched.  wave64, gfx950.
//
// A source is (base, extent, ncols, first, thin): a buffer [chains][extent][ncols] of which rows first, first + thin, .. of every
// chain are taken.  Source A and source B have the same chains and the same kept; flat row r = c * kept + j is row first + j * thin
// of chain c in either source, N = chains * kept >= 2 rows.  cols_a [Ka] and cols_b [Kb] select columns, duplicates allowed (the
// host turns "all columns" into the list 0, 1, ..).  A split is RC_SPLIT consecutive flat rows, S = ceil(N / RC_SPLIT).
//   mean_a[k], mean_b[k]  exactly rh_cov.hip.h's mean of that column (rc_mean_split, rc_mean_finish): same order, same bits;
//   d[r][k]     = x[r][k] - mean[k];
//   var_a[k], var_b[k]    per split one accumulator from +0.0 over r ascending, acc = fma(d, d, acc); the splits added in ascending
//               s from +0.0; the total divided by (double)(N - 1);
//   P_s[a][b]   = one accumulator from +0.0, r ascending in split s: acc = fma(dA[r][a], dB[r][b], acc); the rows past N of a ragged
//               group of four are staged as +0.0 and leave acc as it is;
//   cross[a][b] = (sum over s ascending of P_s[a][b]) / (double)(N - 1);
//   corr[a][b]  = cross[a][b] / (sqrt(var_a[a]) * sqrt(var_b[b])), not clamped; NaN where either variance is not finite and > 0.
// A NaN in a column makes that column's row (of A) or column (of B) of cross and corr NaN, together with its mean and variance, and
// touches nothing else.  No floating-point atomics; nothing depends on the tiling, the chunking of the tile pairs, the order of
// either column list or the launch.  With B the same buffer as A, entry (a, b) of cross has the bits of entry (cols_a[a], cols_b[b])
// of rh_cov.hip.h's cov over all columns, and var_a[a] those of its diagonal: the same fma chain over the same splits, the same sum
// of the splits, the same division.
//
//   rh_cov_mean_kernel, rh_cov_mean_finish_kernel   (rh_cov.hip.h's, in this code object too) the means of either side.
//   rh_xcov_var_kernel         the mean kernel's grid and staging, the subtraction on load: thread t < RC_TC runs the fma chain of
//                              its column's centred rows.  Writes part [S][K].
//   rh_xcov_var_finish_kernel  one thread per column: the S partial sums in ascending s, divided by N - 1.
//   rh_xcov_tile_kernel        one workgroup (4 wavefronts) = one A tile of RX_TA = 32 columns x one B tile of RX_TB = 128 columns x
//                              one split.  B is the wide matrix (observations: hundreds to thousands) and dominates the traffic, A
//                              the narrow one (parameters: 3 to 64): with Ka <= 32 every B value is read exactly once, and a square
//                              64 x 64 tile would spend half of its MFMAs on zero columns and read A again for every 64 B columns.
//                              Wavefront w owns B columns [32 w, 32 w + 32) against all 32 A columns: 2 x 2 accumulators of
//                              v_mfma_f64_16x16x4_f64 at rh_cov.hip.h's operand maps (D[i][j]: i an A column, j a B column).
//                              Slabs of RC_SLAB = 32 centred rows go through LDS as an A block 32 x 32 at row stride RX_SA = 48
//                              doubles and a B block 32 x 128 at row stride RX_SB = 144: both strides are 16 mod 32, so the 16
//                              lanes of one k read 16 consecutive doubles and the next k's start 16 mod 32 doubles on -- the 32
//                              lanes that a ds_read_b64 serves together cover all 64 banks once (the argument RC_STRIDE = 80
//                              rests on).  48 KiB: three workgroups per CU.  Staging: the lanes run along the columns (a B row is
//                              1 KiB of consecutive doubles where the list is contiguous), thread t owns A column t & 31 at rows
//                              t >> 5, + 8, .. and B column t & 127 at rows t >> 7, + 2, ..: its rows of the next slab follow those
//                              of this one at the same step, so the flat-row division happens once per split and a row's offset is the last one's plus a constant.  Ragged rows and
//                              columns are staged as +0.0: every loop around the MFMAs is wave-uniform.  An A tile of at most 16
//                              live columns (Ka <= 16, or the ragged last tile) skips the two MFMAs per k-group of its second
//                              sub-tile, a branch on launch arguments.
//                              Plain staging: a slab is loaded, centred and written to LDS, then multiplied.  Holding the next
//                              slab in registers while the MFMAs of this one run (20 doubles per thread) was measured on the
//                              MI355X and is not faster (profiles/cross_covariance_device/README.md): three resident workgroups
//                              per CU already put one's loads under another's MFMAs.
//                              Writes P_s to the workspace [pair][S][RX_TA][RX_TB], pair p = ta * TB + tb.
//   rh_xcov_finish_kernel      one workgroup per tile pair: the splits in ascending s, the division, into cross [Ka][Kb].
//   rh_xcov_corr_kernel        one thread per entry of corr [Ka][Kb], from the finished cross and variances.
// Workspace: S * 32 KiB per tile pair; the host walks the pairs in chunks that stay below RC_WS_CAP_BYTES and refuses a shape whose
// single pair is beyond it (S > 4096).
//
// As in rh_cov.hip.h the block routines are plain C++ over (thread id, LDS pointer): with RH_COV_HOST defined they compile with a
// host compiler, the MFMA a chain of fma over k = 0, 1, 2, 3 (tests/test_cross_covariance_device_cpu.py): same text, same order.
#ifndef RH_XCOV_HIP_H
#define RH_XCOV_HIP_H
#ifndef RH_COV_HIP_H
#error "rh_xcov.hip.h follows rh_cov.hip.h in its translation unit"
#endif

#define RX_TA 32                // A columns of a tile: 2 sub-tiles of 16
#define RX_TB 128               // B columns of a tile: 32 per wavefront
#define RX_SA 48                // doubles between two rows of the staged A block
#define RX_SB 144               // ... of the staged B block
#define RX_TILE_LDS (RC_SLAB * (RX_SA + RX_SB))   // 48 KiB: three workgroups per CU's 160 KiB, within the family's 63 KiB
#define RX_NA (RC_SLAB * RX_TA / RC_BLOCK)        // staged A values of a thread per slab: 4, at a step of RX_RA rows
#define RX_NB (RC_SLAB * RX_TB / RC_BLOCK)        // ... B values: 16, at a step of RX_RB rows
#define RX_RA (RC_BLOCK / RX_TA)
#define RX_RB (RC_BLOCK / RX_TB)
#define RX_PAIR_BYTES(S) ((long long)(S) * RX_TA * RX_TB * 8)   // workspace of one tile pair

// a source from its row `first` on: base = buffer + first * ncols
struct rx_src { const double *base; long long extent, ncols, thin; };

// ---- variance ---------------------------------------------------------------------------------------------------------------------
// rc_mean_split with the subtraction on load and the fma chain in place of the adds.  lds: RC_MROWS * RC_TC doubles.  part [S][K].
RC_FN void rx_var_split(const rx_src x, const long long kept, const long long N, const int *cols, const int K, const double *mean, const int k0,
                        const long long s, double *lds, double *part, const int rc_nthreads) {
  const long long r_lo = s * RC_SPLIT, r_hi = N - r_lo < RC_SPLIT ? N : r_lo + RC_SPLIT;
  const long long sq = (RC_BLOCK / RC_TC) / kept, sr = (RC_BLOCK / RC_TC) - sq * kept;
  double acc[RC_NSTATE];
  RC_EACH_THREAD(tid) acc[RC_ME(tid)] = 0.0;
  for (long long r0 = r_lo; r0 < r_hi; r0 += RC_MROWS) {
    const int nr = (int)(r_hi - r0 < RC_MROWS ? r_hi - r0 : RC_MROWS);
    RC_EACH_THREAD(tid) {
      const int k = k0 + (tid & (RC_TC - 1));
      if (k < K) {
        const int col = cols[k];
        const double mu = mean[k];
        rc_row w = rc_row_of(r0 + (tid >> 6), kept);
        for (int row = tid >> 6; row < nr; row += RC_BLOCK / RC_TC) {
          lds[row * RC_TC + (tid & (RC_TC - 1))] = x.base[(w.c * x.extent + w.j * x.thin) * x.ncols + col] - mu;
          rc_row_step(w, kept, sq, sr);
        }
      }
    }
    RC_SYNC();
    RC_EACH_THREAD(tid) {
      if (tid < RC_TC && k0 + tid < K) {
        double a = acc[RC_ME(tid)];
        for (int row = 0; row < nr; row++) {
          const double d = lds[row * RC_TC + tid];
          a = __builtin_fma(d, d, a);
        }
        acc[RC_ME(tid)] = a;
      }
    }
    RC_SYNC();
  }
  RC_EACH_THREAD(tid) {
    if (tid < RC_TC && k0 + tid < K) part[s * K + k0 + tid] = acc[RC_ME(tid)];
  }
}

RC_FN double rx_var_finish(const double *part, const long long S, const int K, const int k, const long long N) {
  double acc = 0.0;
  for (long long s = 0; s < S; s++) acc += part[s * K + k];
  return acc / (double)(N - 1);
}

// ---- tile pair x split -----------------------------------------------------------------------------------------------------------
// rc_operand at a block's own row stride
RC_FN double rx_operand(const double *blk, const int stride, const int r0, const int c0, const int lane) {
  return blk[(r0 + (lane >> 4)) * stride + c0 + (lane & 15)];
}
#ifndef RH_COV_HOST
#define RX_MFMA(acc, blkA, ca, blkB, cb, r0, lane) \
  (acc) = __builtin_amdgcn_mfma_f64_16x16x4f64(rx_operand(blkA, RX_SA, r0, ca, lane), rx_operand(blkB, RX_SB, r0, cb, lane), (acc), 0, 0, 0)
#else
// rc_mfma_host at the two strides
static inline void rx_mfma_host(rc_d4 &acc, const double *blkA, const int ca, const double *blkB, const int cb, const int r0, const int lane) {
  for (int reg = 0; reg < 4; reg++) {
    const int i = (lane >> 4) + 4 * reg, j = lane & 15;
    for (int k = 0; k < 4; k++)
      acc[reg] = __builtin_fma(rx_operand(blkA, RX_SA, r0, ca, i + 16 * k), rx_operand(blkB, RX_SB, r0, cb, j + 16 * k), acc[reg]);
  }
}
#define RX_MFMA(acc, blkA, ca, blkB, cb, r0, lane) rx_mfma_host(acc, blkA, ca, blkB, cb, r0, lane)
#endif

// A thread's walk down a source at a fixed step of rows: rc_row's kept iteration j of its row, and in place of the chain the row's
// offset in doubles from base, moved on by additions (rc_row_step's wrap; no multiplication per row).  step = sq * kept + sr rows,
// fwd = (sq * extent + sr * thin) * ncols, and a wrap into the next chain adds back = (extent - kept * thin) * ncols.
struct rx_walk { long long j, off, sr, fwd, back; };
RC_FN rx_walk rx_walk_of(const rx_src x, const long long r, const long long kept, const long long step) {
  const rc_row w = rc_row_of(r, kept);
  const long long sq = step / kept, sr = step - sq * kept;
  const rx_walk g = {w.j, (w.c * x.extent + w.j * x.thin) * x.ncols, sr, (sq * x.extent + sr * x.thin) * x.ncols, (x.extent - kept * x.thin) * x.ncols};
  return g;
}
// the thread's n values of the slab from flat row r0 on, at the walk's step of `step` rows, centred into the block (a dead row or
// column: the load is of base[0], unused, and +0.0 is staged); the walk ends on the thread's first row of the next slab
RC_FN void rx_stage(const rx_src x, double *blk, const int stride, const int c, const int col, const double mu, rx_walk &w, const long long kept,
                    const long long r0, const long long r_hi, const int row0, const int step, const int n) {
#pragma unroll
  for (int i = 0; i < n; i++) {
    const int row = row0 + i * step;
    const bool have = col >= 0 && r0 + row < r_hi;
    const double v = x.base[have ? w.off + col : 0];
    blk[row * stride + c] = have ? v - mu : 0.0;
    w.j += w.sr;
    const bool wrap = w.j >= kept;
    w.j -= wrap ? kept : 0;
    w.off += w.fwd + (wrap ? w.back : 0);
  }
}

// A tile ta x B tile tb over split s: P [RX_TA][RX_TB] = sum over the split's rows of dA[r][ta * RX_TA + a] * dB[r][tb * RX_TB + b].
// lds: RX_TILE_LDS doubles.
RC_FN void rx_tile_split(const rx_src A, const rx_src B, const long long kept, const long long N, const int *cols_a, const int Ka, const int *cols_b,
                         const int Kb, const double *mean_a, const double *mean_b, const int ta, const int tb, const long long s, double *lds,
                         double *P, const int rc_nthreads) {
  const long long r_lo = s * RC_SPLIT, r_hi = N - r_lo < RC_SPLIT ? N : r_lo + RC_SPLIT;
  const int subs = Ka - ta * RX_TA > 16 ? 2 : 1;   // live 16-column sub-tiles of this A tile
  double *blkA = lds, *blkB = lds + RC_SLAB * RX_SA;
  rc_d4 acc[RC_NSTATE][2][2];
  int col[RC_NSTATE][2];          // the staged column of this thread in the A and in the B block (-1: past K, staged as +0.0), its mean
  double mu[RC_NSTATE][2];
  rx_walk wa[RC_NSTATE], wb[RC_NSTATE];
  RC_EACH_THREAD(tid) {
    const int me = RC_ME(tid), ka = ta * RX_TA + (tid & (RX_TA - 1)), kb = tb * RX_TB + (tid & (RX_TB - 1));
    col[me][0] = ka < Ka ? cols_a[ka] : -1;
    mu[me][0] = ka < Ka ? mean_a[ka] : 0.0;
    col[me][1] = kb < Kb ? cols_b[kb] : -1;
    mu[me][1] = kb < Kb ? mean_b[kb] : 0.0;
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
      for (int mj = 0; mj < 2; mj++)
#pragma unroll
        for (int e = 0; e < 4; e++) acc[me][mi][mj][e] = 0.0;
    wa[me] = rx_walk_of(A, r_lo + tid / RX_TA, kept, RX_RA);
    wb[me] = rx_walk_of(B, r_lo + tid / RX_TB, kept, RX_RB);
  }
  for (long long r0 = r_lo; r0 < r_hi; r0 += RC_SLAB) {
    RC_EACH_THREAD(tid) {
      const int me = RC_ME(tid);
      rx_stage(A, blkA, RX_SA, tid & (RX_TA - 1), col[me][0], mu[me][0], wa[me], kept, r0, r_hi, tid / RX_TA, RX_RA, RX_NA);
      rx_stage(B, blkB, RX_SB, tid & (RX_TB - 1), col[me][1], mu[me][1], wb[me], kept, r0, r_hi, tid / RX_TB, RX_RB, RX_NB);
    }
    RC_SYNC();
    RC_EACH_THREAD(tid) {
      const int me = RC_ME(tid), lane = tid & 63, cb = (tid >> 6) * 32;   // wavefront w: B columns [32 w, 32 w + 32)
      if (subs > 1) {
#pragma unroll
        for (int kg = 0; kg < RC_SLAB / 4; kg++)
#pragma unroll
          for (int m = 0; m < 4; m++) RX_MFMA(acc[me][m >> 1][m & 1], blkA, 16 * (m >> 1), blkB, cb + 16 * (m & 1), 4 * kg, lane);
      } else {
#pragma unroll
        for (int kg = 0; kg < RC_SLAB / 4; kg++)
#pragma unroll
          for (int mj = 0; mj < 2; mj++) RX_MFMA(acc[me][0][mj], blkA, 0, blkB, cb + 16 * mj, 4 * kg, lane);
      }
    }
    RC_SYNC();
  }
  RC_EACH_THREAD(tid) {
    const int me = RC_ME(tid), lane = tid & 63, cb = (tid >> 6) * 32;
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
      for (int mj = 0; mj < 2; mj++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++)
          P[(16 * mi + (lane >> 4) + 4 * reg) * RX_TB + cb + 16 * mj + (lane & 15)] = acc[me][mi][mj][reg];
  }
}

// ---- finish ----------------------------------------------------------------------------------------------------------------------
// ws [S][RX_TA][RX_TB]: the partials of tile pair (ta, tb); cross [Ka][Kb]
RC_FN void rx_finish_pair(const double *ws, const long long S, const long long N, const int ta, const int tb, const int Ka, const int Kb,
                          double *cross, const int rc_nthreads) {
  RC_EACH_THREAD(tid) {
    for (int e = tid; e < RX_TA * RX_TB; e += RC_BLOCK) {
      const long long ga = (long long)ta * RX_TA + e / RX_TB, gb = (long long)tb * RX_TB + (e & (RX_TB - 1));
      if (ga >= Ka || gb >= Kb) continue;
      double acc = 0.0;
      for (long long s = 0; s < S; s++) acc += ws[s * RX_TA * RX_TB + e];
      cross[ga * Kb + gb] = acc / (double)(N - 1);
    }
  }
}

RC_FN double rx_corr_entry(const double *cross, const double *var_a, const double *var_b, const long long Kb, const long long a, const long long b) {
  const double va = var_a[a], vb = var_b[b];
  if (!(va > 0.0 && va < __builtin_inf() && vb > 0.0 && vb < __builtin_inf())) return __builtin_nan("");
  return cross[a * Kb + b] / (__builtin_sqrt(va) * __builtin_sqrt(vb));
}

#ifndef RH_COV_HOST
// grid: S x ceil(K / RC_TC), blockIdx.x = s * ctiles + column tile
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_xcov_var_kernel(const double *__restrict__ draws, const long long extent, const long long ncols, const long long first, const long long thin,
                   const long long kept, const long long N, const int *__restrict__ cols, const int K, const int ctiles,
                   const double *__restrict__ mean, double *__restrict__ part) {
  __shared__ double lds[RC_MROWS * RC_TC];
  const long long s = (long long)(blockIdx.x / (unsigned)ctiles);
  const int ct = (int)(blockIdx.x - (unsigned)s * (unsigned)ctiles);
  if (s * RC_SPLIT >= N) return;
  const rx_src x = {draws + first * ncols, extent, ncols, thin};
  rx_var_split(x, kept, N, cols, K, mean, ct * RC_TC, s, lds, part, RC_BLOCK);
}

// grid: ceil(K / RC_BLOCK)
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_xcov_var_finish_kernel(const double *__restrict__ part, const long long S, const int K, const long long N, double *__restrict__ var) {
  const int k = (int)(blockIdx.x * RC_BLOCK + threadIdx.x);
  if (k < K) var[k] = rx_var_finish(part, S, K, k, N);
}

// grid: the chunk's tile pairs [p_lo, p_lo + p_cnt) x S, blockIdx.x = (pair - p_lo) * S + s; TB: the B tiles; ws [p_cnt][S][RX_TA][RX_TB]
extern "C" __global__ void __launch_bounds__(RC_BLOCK, 3)   // three wavefronts per SIMD: the three workgroups per CU that the LDS allows
rh_xcov_tile_kernel(const double *__restrict__ a, const long long extent_a, const long long ncols_a, const long long first_a, const long long thin_a,
                    const double *__restrict__ b, const long long extent_b, const long long ncols_b, const long long first_b, const long long thin_b,
                    const long long kept, const long long N, const int *__restrict__ cols_a, const int Ka, const int *__restrict__ cols_b, const int Kb,
                    const double *__restrict__ mean_a, const double *__restrict__ mean_b, const int TB, const long long p_lo, const int p_cnt,
                    const long long S, double *__restrict__ ws) {
  __shared__ double lds[RX_TILE_LDS];
  const long long pl = (long long)blockIdx.x / S, s = (long long)blockIdx.x - pl * S;
  if (pl >= p_cnt) return;
  const long long p = p_lo + pl;
  const rx_src A = {a + first_a * ncols_a, extent_a, ncols_a, thin_a}, B = {b + first_b * ncols_b, extent_b, ncols_b, thin_b};
  rx_tile_split(A, B, kept, N, cols_a, Ka, cols_b, Kb, mean_a, mean_b, (int)(p / TB), (int)(p % TB), s, lds, ws + (pl * S + s) * RX_TA * RX_TB, RC_BLOCK);
}

// grid: the chunk's tile pairs
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_xcov_finish_kernel(const double *__restrict__ ws, const long long S, const long long N, const int TB, const long long p_lo, const int Ka,
                      const int Kb, double *__restrict__ cross) {
  const long long p = p_lo + blockIdx.x;
  rx_finish_pair(ws + (long long)blockIdx.x * S * RX_TA * RX_TB, S, N, (int)(p / TB), (int)(p % TB), Ka, Kb, cross, RC_BLOCK);
}

// grid: ceil(Ka * Kb / RC_BLOCK)
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_xcov_corr_kernel(const double *__restrict__ cross, const double *__restrict__ var_a, const double *__restrict__ var_b, const long long Ka,
                    const long long Kb, double *__restrict__ corr) {
  const long long e = (long long)blockIdx.x * RC_BLOCK + threadIdx.x;
  if (e < Ka * Kb) corr[e] = rx_corr_entry(cross, var_a, var_b, Kb, e / Kb, e - e / Kb * Kb);
}
#endif
#endif
