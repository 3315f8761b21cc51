// rh_linear.hip.h -- a linear map of device-resident draws: Y = (X[:, cols] - c) W + b on the fp64 matrix cores, the rows kept.  The
// one call over draws that makes new columns without a compiled program: whitened draws and their squared norms (Mahalanobis
// distances: W = L^-T of the covariance's Cholesky factor), principal-component scores (W the eigenvectors), contrasts (W of +-1), the
// linear predictor of a GLM at M new rows (W the transposed design matrix, b the intercept column).  The result is a draw set
// [chains][kept][M] that every other call here takes.
//
// Model-independent: a translation unit of its own behind rh_cov.hip.h's text (its flat-row stepping, the MFMA operand maps, the
// host-mode macros), compiled once per toolchain through the engine's build_source() and inspected like every other code object
// before it is launched.  wave64, gfx950.
//
// draws [chains][extent][nvars].  Flat row r = c * kept + j is row first + j * thin of chain c, N = chains * kept rows.  cols [K]
// selects columns, duplicates allowed (the host turns "all" into 0, 1, ..); W [K][M] row-major, center [K] (the host hands zeros for
// "none": x - (+0.0) has the bits of x), offset [M] or NULL.
//   d[r][k]   = x[r][cols[k]] - center[k], one rounding;
//   y[r][m]   = one accumulator from +0.0 over k ascending: acc = fma(d[r][k], W[k][m], acc); with offset, y = acc + offset[m];
//               the k past K of the last group of four are staged as +0.0 * +0.0 and leave acc as it is;
//   sqnorm[r] = one accumulator from +0.0 over m ascending: acc = fma(y[r][m], y[r][m], acc).
// A NaN in a selected value of row r makes row r of y and sqnorm[r] NaN and touches no other row (a row's accumulators see that
// row's values alone).  No floating-point atomics, no workspace, no partial sums: nothing depends on the tiling, the grid, the order
// of launch or a repeat.  With the MFMA taken as a chain of fma over its four k (the family's assumption, measured for this
// instruction), the host emulation and the device give the same bits.
//
//   rh_linear_tile_kernel   one workgroup (4 wavefronts) = one tile of RL_TR = 64 flat rows x a run of m tiles of RL_TM = 64 output
//                           columns, K walked in slabs of RC_SLAB = 32.  Wavefront w owns rows [16 w, 16 w + 16) against the 64
//                           output columns: four accumulators of v_mfma_f64_16x16x4_f64, D[i][j] with i a row and j an output
//                           column; the A operand of a k-group is loaded once and serves all four.  k-groups past K and 16-column
//                           sub-tiles past M are skipped, branches on launch arguments.
//                           Staging, per slab: the W block [k][m] at row stride RC_STRIDE = 80 doubles (16 mod 32), read with
//                           rc_operand and written with the lanes along m -- rh_cov.hip.h's argument as it stands.  The X block is
//                           NOT transposed: it lies [row][k] at row stride RL_SX = 34 doubles (2 mod 32) and the A operand is read
//                           through rl_operand_x, lane -> [row = lane & 15][k = lane >> 4].  The 32 lanes that a ds_read_b64 serves
//                           together are 16 rows x 2 consecutive k: 2 * row + k covers the 32 double-wide banks once.  The global
//                           loads run with the lanes along k first (a row's selected values are consecutive where the list is),
//                           then rows, and so do the LDS writes: 32 consecutive doubles of one staged row, every bank once.  A
//                           transposed block [k][row] at a stride of 16 mod 32 would read as well but take those writes 16 to a
//                           bank (k * stride is 0 or 16 mod 32); trading that for loads with the lanes along the rows would cut
//                           every 256 B row segment into 16 B pieces.  Centring happens on load; ragged rows, k and m are staged as
//                           +0.0, so every loop around the MFMAs is wave-uniform.  Thread t owns k = t & 31 at rows t >> 5, + 8, ..:
//                           the flat-row division happens once per tile, every later row is a step (rc_row_step).
//                           The finished tile always goes through LDS (over the staged blocks, [row][m] at row stride RL_ST = 65:
//                           odd, so the 32 rows that the chain's reads touch together lie in 32 different banks).  y is stored from
//                           there with the lanes along m, 512 B per wavefront and row.  For sqnorm thread t < 64 continues row t's
//                           fma chain over the tile's live m; the chain is carried across the m tiles in a register, which is why one
//                           workgroup walks all m tiles of its rows when sqnorm is asked for.  With sqnorm alone Y never reaches
//                           HBM.  Without sqnorm, and fewer than RL_FULL_GRID row tiles, every m tile gets a workgroup of its own
//                           (rh_plan::linear_plan); with M <= 64 every x is read once either way.
//                           LDS: 64 * 34 + 32 * 80 doubles = 37 KiB, four workgroups per CU, within the family's 63 KiB.
//
// As in rh_cov.hip.h the block routine is plain C++ over (thread id, LDS pointer): with RH_COV_HOST defined it compiles with a host
// compiler, the MFMA a chain of fma over k = 0, 1, 2, 3 (tests/test_linear_device_cpu.py): same text, same order.
#ifndef RH_LINEAR_HIP_H
#define RH_LINEAR_HIP_H
#ifndef RH_COV_HIP_H
#error "rh_linear.hip.h follows rh_cov.hip.h in its translation unit"
#endif

#define RL_TR 64                // flat rows of a tile: 16 per wavefront
#define RL_TM 64                // output columns of an m tile: 4 sub-tiles of 16
#define RL_SX 34                // doubles between two rows of the staged X block [row][k]
#define RL_ST 65                // ... of the finished tile [row][m]
#define RL_MAX_DIM 4096         // K and M at most: W then stays within RC_WS_CAP_BYTES
#define RL_FULL_GRID 1024       // row tiles from which the m tiles are no longer given workgroups of their own
#define RL_TILE_LDS (RL_TR * RL_SX + RC_SLAB * RC_STRIDE)   // 37 KiB; the finished tile (RL_TR * RL_ST doubles) fits over it
#define RL_NX (RL_TR * RC_SLAB / RC_BLOCK)                  // staged X values of a thread per slab: 8, at a step of RL_RX rows
#define RL_NW (RC_SLAB * RL_TM / RC_BLOCK)                  // ... W values: 8, at a step of RL_RW k
#define RL_RX (RC_BLOCK / RC_SLAB)
#define RL_RW (RC_BLOCK / RL_TM)

// what lane `lane` hands the MFMA as its A operand of the k k0 .. k0 + 3 of the staged X block, rows row0 .. row0 + 15
RC_FN double rl_operand_x(const double *blk, const int row0, const int k0, const int lane) {
  return blk[(row0 + (lane & 15)) * RL_SX + k0 + (lane >> 4)];
}
#ifndef RH_COV_HOST
#define RL_MFMA(acc, a, blkW, cb, k0, lane) (acc) = __builtin_amdgcn_mfma_f64_16x16x4f64((a), rc_operand(blkW, k0, cb, lane), (acc), 0, 0, 0)
#define RL_A_OF(blkX, row0, k0, lane) rl_operand_x(blkX, row0, k0, lane)
#else
// rc_mfma_host with the A operand from the untransposed X block; `a` is where that block's operand starts
struct rl_a_host { const double *blk; int row0, k0; };
static inline void rl_mfma_host(rc_d4 &acc, const rl_a_host a, const double *blkW, const int cb, const int k0, const int lane) {
  for (int reg = 0; reg < 4; reg++) {
    const int i = (lane >> 4) + 4 * reg, j = lane & 15;
    for (int k = 0; k < 4; k++) acc[reg] = __builtin_fma(rl_operand_x(a.blk, a.row0, a.k0, i + 16 * k), rc_operand(blkW, k0, cb, j + 16 * k), acc[reg]);
  }
}
#define RL_MFMA(acc, a, blkW, cb, k0, lane) rl_mfma_host(acc, a, blkW, cb, k0, lane)
#define RL_A_OF(blkX, row0, k0, lane) rl_a_host{blkX, row0, k0}
#endif

// Row tile rt against the m tiles [mt_lo, mt_hi).  base: draws[0][first][0]; lds: RL_TILE_LDS doubles; y [N][M] or NULL; sqnorm [N]
// or NULL (then mt_lo = 0 and mt_hi covers M: the chain of a row runs in this workgroup alone).
RC_FN void rl_tile(const double *base, const long long extent, const long long nvars, const long long thin, const long long kept, const long long N,
                   const int *cols, const int K, const double *center, const double *W, const int M, const double *offset, const long long rt,
                   const int mt_lo, const int mt_hi, double *lds, double *y, double *sqnorm, const int rc_nthreads) {
  const long long r0 = rt * RL_TR;
  const long long sq = RL_RX / kept, sr = RL_RX - sq * kept;
  double *blkX = lds, *blkW = lds + RL_TR * RL_SX;
  rc_d4 acc[RC_NSTATE][4];
  rc_row w0[RC_NSTATE];        // the thread's first staged row of the tile
  double norm[RC_NSTATE];      // thread t < RL_TR: the chain of row r0 + t so far
  RC_EACH_THREAD(tid) {
    w0[RC_ME(tid)] = rc_row_of(r0 + tid / RC_SLAB, kept);
    norm[RC_ME(tid)] = 0.0;
  }
  for (int mt = mt_lo; mt < mt_hi; mt++) {
    const int m0 = mt * RL_TM, live_m = M - m0 < RL_TM ? M - m0 : RL_TM, subs = (live_m + 15) / 16;
    RC_EACH_THREAD(tid) {
#pragma unroll
      for (int mj = 0; mj < 4; mj++)
#pragma unroll
        for (int e = 0; e < 4; e++) acc[RC_ME(tid)][mj][e] = 0.0;
    }
    for (int k0 = 0; k0 < K; k0 += RC_SLAB) {
      const int groups = K - k0 < RC_SLAB ? (K - k0 + 3) / 4 : RC_SLAB / 4;
      RC_EACH_THREAD(tid) {
        const int k = tid & (RC_SLAB - 1), m = tid & (RL_TM - 1);
        const bool have_k = k0 + k < K, have_m = m < live_m;
        const int col = have_k ? cols[k0 + k] : 0;
        const double mu = have_k ? center[k0 + k] : 0.0;
        rc_row w = w0[RC_ME(tid)];
#pragma unroll
        for (int i = 0; i < RL_NX; i++) {
          const int row = tid / RC_SLAB + i * RL_RX;
          const bool have = have_k && r0 + row < N;                          // else: staged as +0.0 (the load is of base[0], unused)
          const double x = base[have ? (w.c * extent + w.j * thin) * nvars + col : 0];
          blkX[row * RL_SX + k] = have ? x - mu : 0.0;
          rc_row_step(w, kept, sq, sr);
        }
#pragma unroll
        for (int i = 0; i < RL_NW; i++) {
          const int kw = tid / RL_TM + i * RL_RW;
          const bool have = have_m && k0 + kw < K;
          const double v = W[have ? (long long)(k0 + kw) * M + m0 + m : 0];
          blkW[kw * RC_STRIDE + m] = have ? v : 0.0;
        }
      }
      RC_SYNC();
      RC_EACH_THREAD(tid) {
        const int me = RC_ME(tid), lane = tid & 63, row0 = (tid >> 6) * 16;   // wavefront w: rows [16 w, 16 w + 16)
        for (int kg = 0; kg < groups; kg++) {
          const auto a = RL_A_OF(blkX, row0, 4 * kg, lane);
#pragma unroll
          for (int mj = 0; mj < 4; mj++)
            if (mj < subs) RL_MFMA(acc[me][mj], a, blkW, 16 * mj, 4 * kg, lane);
        }
      }
      RC_SYNC();
    }
    RC_EACH_THREAD(tid) {      // the finished tile over the staged blocks: [row][m]
      const int me = RC_ME(tid), lane = tid & 63, row0 = (tid >> 6) * 16;
#pragma unroll
      for (int mj = 0; mj < 4; mj++) {
        const int m = 16 * mj + (lane & 15);
        const bool add = offset && m < live_m;
        const double b = add ? offset[m0 + m] : 0.0;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) lds[(row0 + (lane >> 4) + 4 * reg) * RL_ST + m] = add ? acc[me][mj][reg] + b : acc[me][mj][reg];
      }
    }
    RC_SYNC();
    RC_EACH_THREAD(tid) {
      const int m = tid & (RL_TM - 1);
      if (y && m < live_m)
        for (int row = tid / RL_TM; row < RL_TR && r0 + row < N; row += RL_RW) y[(r0 + row) * M + m0 + m] = lds[row * RL_ST + m];
      if (sqnorm && tid < RL_TR && r0 + tid < N) {
        double a = norm[RC_ME(tid)];
        for (int mm = 0; mm < live_m; mm++) {
          const double v = lds[tid * RL_ST + mm];
          a = __builtin_fma(v, v, a);
        }
        norm[RC_ME(tid)] = a;
      }
    }
    RC_SYNC();
  }
  RC_EACH_THREAD(tid) {
    if (sqnorm && tid < RL_TR && r0 + tid < N) sqnorm[r0 + tid] = norm[RC_ME(tid)];
  }
}

#ifndef RH_COV_HOST
// grid: row tiles x mgroups, blockIdx.x = rt * mgroups + g; workgroup g takes the m tiles [g * mper, (g + 1) * mper) below ceil(M / RL_TM)
extern "C" __global__ void __launch_bounds__(RC_BLOCK, 4)   // four wavefronts per SIMD: the four workgroups per CU that the LDS allows
rh_linear_tile_kernel(const double *__restrict__ draws, const long long extent, const long long nvars, const long long first, const long long thin,
                      const long long kept, const long long N, const int *__restrict__ cols, const int K, const double *__restrict__ center,
                      const double *__restrict__ W, const int M, const double *__restrict__ offset, const int mgroups, const int mper,
                      double *__restrict__ y, double *__restrict__ sqnorm) {
  __shared__ double lds[RL_TILE_LDS];
  const long long rt = (long long)(blockIdx.x / (unsigned)mgroups);
  const int g = (int)(blockIdx.x - (unsigned)rt * (unsigned)mgroups), mtiles = (M + RL_TM - 1) / RL_TM;
  if (rt * RL_TR >= N) return;
  rl_tile(draws + first * nvars, extent, nvars, thin, kept, N, cols, K, center, W, M, offset, rt, g * mper, (g + 1) * mper < mtiles ? (g + 1) * mper : mtiles,
          lds, y, sqnorm, RC_BLOCK);
}
#endif
#endif
