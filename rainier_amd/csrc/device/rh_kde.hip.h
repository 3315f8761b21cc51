// rh_kde.hip.h -- Gaussian kernel density estimates over device-resident draws: the smooth density of a parameter on a grid of points,
// and of a pair of parameters on a grid of points x points (the reference's contour of pairs, rainier-notebook package.scala:93-98).
// The one posterior plot whose cost grows as draws x grid points; only the curve or the surface comes back.
//
// Model-independent: a translation unit of its own behind rh_cov.hip.h's text (its flat-row stepping, LDS row stride, MFMA operand
// maps and host-mode macros), compiled once per toolchain through the engine's build_source() and inspected like every other code
// object before it is launched.  wave64, gfx950.
//
// draws [chains][iterations][nvars].  Flat row r = c * kept + j is draw (c, first + j * thin), N = chains * kept rows; a split is
// RC_SPLIT consecutive flat rows, S = ceil(N / RC_SPLIT), the last one ragged.  The grids are the host's (draws_plan.hpp's kde_grid).
//   1-D    z = (g[i] - x[r]) / h; term = exp(-0.5 * z * z), IEEE operations in that order, exp being rkd_exp below;
//          P_s[i] = one accumulator from +0.0, r ascending in split s, plain adds;
//          density[k][i] = (sum over s ascending of P_s[i]) / ((double)N * h * sqrt(2 pi)).
//   pairs  phix[i][r] = exp(-0.5 * zx * zx), zx = (gx[i] - x[r]) / hx, phiy[j][r] likewise: (Gx + Gy) N exponentials, not Gx Gy N;
//          P_s[i][j] = one accumulator from +0.0, r ascending in split s: acc = fma(phix[i][r], phiy[j][r], acc) -- a Gx x N x Gy
//          matrix product on the fp64 matrix cores whose two operand blocks are generated on the fly; the rows past N of a ragged
//          group of four are staged as +0.0 and leave acc as it is;
//          density[p][i][j] = (sum over s ascending of P_s[i][j]) / ((double)N * 2 pi * hx * hy).
// No special cases: a +-inf draw contributes +0.0, a NaN draw makes its column's curve (its pair's surface: NaN * 0.0 is NaN) NaN
// and touches nothing else, a constant column is an ordinary input.  No floating-point atomics; nothing depends on the tiling, the
// chunking, the order of the column list or the launch.
//
//   rh_kde_point_kernel        one workgroup = one selected column x one split x one tile of RKD_GT grid points.  Slabs of RKD_ROWS of
//                              the split's rows are staged once into LDS (thread t loads rows t, t + 256, ..: cov's flat-row
//                              stepping); each thread owns RKD_PPT grid points in registers -- that many independent exp chains -- and
//                              walks the slab by LDS broadcast reads, r ascending.  Writes part [column][S][G].
//   rh_kde_finish_kernel       one thread per (column, grid point): the splits in ascending s, the scale.
//   rh_kde_tile_kernel         one workgroup (4 wavefronts) = one unit (pair x one 64 x 64 tile of the surface) x one split.  Per slab
//                              of RC_SLAB = 32 rows the 256 threads compute the two 64 x 32 operand blocks phix, phiy into LDS
//                              ([row][grid point], stride RC_STRIDE = 80 doubles; thread t owns grid point t & 63 of either axis in
//                              registers and rows t >> 6, + 4, ..: 16 exp per thread, the draws' loads wave-uniform); ragged grid
//                              points and rows are zero-filled.  Each wavefront then owns a 32 x 32 quadrant as 2 x 2 accumulators of
//                              v_mfma_f64_16x16x4_f64 at rh_cov.hip.h's operand maps; every loop around the MFMAs is wave-uniform.
//                              Writes P_s to the workspace [unit][S][64][64].
//   rh_kde_pairs_finish_kernel one workgroup per unit: the splits in ascending s, the scale, into density [P][npx][npy].
// Workspace: S * G * 8 bytes per column, S * 32 KiB per unit; the host walks columns resp. units in chunks that stay below
// RKD_WS_CAP_BYTES and refuses a shape whose single column or unit is beyond it.
//
// As in rh_cov.hip.h the block routines are plain C++ over (thread id, LDS pointer): with RH_KDE_HOST (and RH_COV_HOST) defined they
// compile with a host compiler, the MFMA a chain of fma over k = 0, 1, 2, 3 (tests/test_kde_device_cpu.py): same text, same order.
#ifndef RH_KDE_HIP_H
#define RH_KDE_HIP_H
#ifndef RH_COV_HIP_H
#error "rh_kde.hip.h follows rh_cov.hip.h in its translation unit"
#endif

#define RKD_PPT 2                       // grid points of a thread of the point kernel
#define RKD_GT (RC_BLOCK * RKD_PPT)     // grid points of a tile of the point kernel
#define RKD_ROWS 1024                   // rows of a staged slab of the point kernel: 8 KiB
#define RKD_MAX_POINTS 4096             // 2 .. this many points of a curve
#define RKD_MAX_SIDE 256                // 2 .. this many points per axis of a surface
#define RKD_WS_CAP_BYTES (128ll << 20)
#define RKD_UNIT_BYTES(S) ((long long)(S) * RC_TC * RC_TC * 8)   // workspace of one unit
#define RKD_SQRT_TWO_PI 2.5066282746310002
#define RKD_TWO_PI 6.283185307179586

// ---- exp: fdlibm 5.3 e_exp.c, the same text on the host and on the device -----------------------------------------------------------
RC_FN int rkd_hi(const double x) { unsigned long long b; __builtin_memcpy(&b, &x, 8); return (int)(b >> 32); }
RC_FN unsigned rkd_lo(const double x) { unsigned long long b; __builtin_memcpy(&b, &x, 8); return (unsigned)b; }
RC_FN double rkd_with_hi(const double x, const int h) {
  unsigned long long b;
  __builtin_memcpy(&b, &x, 8);
  b = ((unsigned long long)(unsigned)h << 32) | (b & 0xffffffffull);
  double y;
  __builtin_memcpy(&y, &b, 8);
  return y;
}
RC_FN double rkd_exp(double x) {
  const double huge = 1.0e+300, twom1000 = 9.33263618503218878990e-302, o_threshold = 7.09782712893383973096e+02,
               u_threshold = -7.45133219101941108420e+02, ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10,
               invln2 = 1.44269504088896338700e+00, P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03,
               P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
  double hi = 0.0, lo = 0.0;
  int k = 0;
  unsigned hx = (unsigned)rkd_hi(x);
  const int xsb = (int)((hx >> 31) & 1);
  hx &= 0x7fffffff;
  if (hx >= 0x40862E42) {
    if (hx >= 0x7ff00000) {
      if (((hx & 0xfffff) | rkd_lo(x)) != 0) return x + x;
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
  if (k >= -1021) return rkd_with_hi(y, rkd_hi(y) + (int)((unsigned)k << 20));   // (k < 0: the shift is the unsigned one)
  y = rkd_with_hi(y, rkd_hi(y) + (int)((unsigned)(k + 1000) << 20));
  return y * twom1000;
}
// the Gaussian kernel's term of grid point g and draw x at bandwidth h, unscaled
RC_FN double rkd_term(const double g, const double x, const double h) {
  const double z = (g - x) / h;
  return rkd_exp(-0.5 * z * z);
}

// ---- 1-D: column x split x tile of grid points ----------------------------------------------------------------------------------------
// Column `col` of the draws over split s, grid points [g0, g0 + RKD_GT) of grid [G] at bandwidth h.  base: draws[0][first][0].
// lds: RKD_ROWS doubles.  part [G]: this column's and split's partial sums.
RC_FN void rkd_point_split(const double *base, const long long iterations, const long long nvars, const long long thin, const long long kept,
                           const long long N, const int col, const double *grid, const int G, const double h, const int g0, const long long s,
                           double *lds, double *part, const int rc_nthreads) {
  const long long r_lo = s * RC_SPLIT, r_hi = N - r_lo < RC_SPLIT ? N : r_lo + RC_SPLIT;
  const long long sq = RC_BLOCK / kept, sr = RC_BLOCK - sq * kept;
  double acc[RC_NSTATE][RKD_PPT], g[RC_NSTATE][RKD_PPT];
  RC_EACH_THREAD(tid) {
#pragma unroll
    for (int p = 0; p < RKD_PPT; p++) {
      const int i = g0 + tid + p * RC_BLOCK;
      g[RC_ME(tid)][p] = i < G ? grid[i] : 0.0;   // (a point past G is computed and not written)
      acc[RC_ME(tid)][p] = 0.0;
    }
  }
  for (long long r0 = r_lo; r0 < r_hi; r0 += RKD_ROWS) {
    const int nr = (int)(r_hi - r0 < RKD_ROWS ? r_hi - r0 : RKD_ROWS);
    RC_EACH_THREAD(tid) {
      rc_row w = rc_row_of(r0 + tid, kept);
      for (int row = tid; row < nr; row += RC_BLOCK) {
        lds[row] = base[(w.c * iterations + w.j * thin) * nvars + col];
        rc_row_step(w, kept, sq, sr);
      }
    }
    RC_SYNC();
    RC_EACH_THREAD(tid) {
      const int me = RC_ME(tid);
      for (int row = 0; row < nr; row++) {
        const double x = lds[row];
#pragma unroll
        for (int p = 0; p < RKD_PPT; p++) acc[me][p] += rkd_term(g[me][p], x, h);
      }
    }
    RC_SYNC();
  }
  RC_EACH_THREAD(tid) {
#pragma unroll
    for (int p = 0; p < RKD_PPT; p++) {
      const int i = g0 + tid + p * RC_BLOCK;
      if (i < G) part[i] = acc[RC_ME(tid)][p];
    }
  }
}

// part [S][G] of one column
RC_FN double rkd_point_finish(const double *part, const long long S, const int G, const int i, const long long N, const double h) {
  double acc = 0.0;
  for (long long s = 0; s < S; s++) acc += part[s * G + i];
  return acc / ((double)N * h * RKD_SQRT_TWO_PI);
}

// ---- pairs: unit x split ---------------------------------------------------------------------------------------------------------------
// unit u of a call over tx x ty tiles per pair: pair u / (tx ty), tile (ti, tj) in row-major order
RC_FN void rkd_unit_of(const long long u, const int tx, const int ty, int *p, int *ti, int *tj) {
  const long long per = (long long)tx * ty, q = u / per;
  const int rest = (int)(u - q * per);
  *p = (int)q;
  *ti = rest / ty;
  *tj = rest - *ti * ty;
}

// Columns (colx, coly) over split s, tile (ti, tj) of the surface over xg [npx] x yg [npy]: P [RC_TC][RC_TC] = sum over the split's rows
// of phix[ti * RC_TC + a][r] * phiy[tj * RC_TC + b][r].  base: draws[0][first][0]; lds: RC_TILE_LDS doubles.
RC_FN void rkd_tile_split(const double *base, const long long iterations, const long long nvars, const long long thin, const long long kept,
                          const long long N, const int colx, const int coly, const double *xg, const double *yg, const int npx, const int npy,
                          const double hx, const double hy, const int ti, const int tj, const long long s, double *lds, double *P,
                          const int rc_nthreads) {
  const long long r_lo = s * RC_SPLIT, r_hi = N - r_lo < RC_SPLIT ? N : r_lo + RC_SPLIT;
  const long long sq = (RC_BLOCK / RC_TC) / kept, sr = (RC_BLOCK / RC_TC) - sq * kept;
  double *blkA = lds, *blkB = lds + RC_SLAB * RC_STRIDE;
  rc_d4 acc[RC_NSTATE][2][2];
  double gx[RC_NSTATE], gy[RC_NSTATE];   // this thread's grid point on either axis
  bool okx[RC_NSTATE], oky[RC_NSTATE];   // ... false: past the axis' points, staged as +0.0
  RC_EACH_THREAD(tid) {
    const int me = RC_ME(tid), i = ti * RC_TC + (tid & (RC_TC - 1)), j = tj * RC_TC + (tid & (RC_TC - 1));
    okx[me] = i < npx;
    oky[me] = j < npy;
    gx[me] = okx[me] ? xg[i] : 0.0;
    gy[me] = oky[me] ? yg[j] : 0.0;
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
      for (int mj = 0; mj < 2; mj++)
#pragma unroll
        for (int e = 0; e < 4; e++) acc[me][mi][mj][e] = 0.0;
  }
  for (long long r0 = r_lo; r0 < r_hi; r0 += RC_SLAB) {
    RC_EACH_THREAD(tid) {
      const int me = RC_ME(tid), c = tid & (RC_TC - 1);
      rc_row w = rc_row_of(r0 + (tid >> 6), kept);
#pragma unroll 2
      for (int row = tid >> 6; row < RC_SLAB; row += RC_BLOCK / RC_TC) {
        const bool live = r0 + row < r_hi;                               // wave-uniform, as are both loads
        const long long off = live ? (w.c * iterations + w.j * thin) * nvars : 0;   // (a dead row loads base[colx], base[coly]: row 0, unused)
        const double x = base[off + colx], y = base[off + coly];
        blkA[row * RC_STRIDE + c] = live && okx[me] ? rkd_term(gx[me], x, hx) : 0.0;
        blkB[row * RC_STRIDE + c] = live && oky[me] ? rkd_term(gy[me], y, hy) : 0.0;
        rc_row_step(w, kept, sq, sr);
      }
    }
    RC_SYNC();
    RC_EACH_THREAD(tid) {
      const int me = RC_ME(tid), lane = tid & 63, ca = (tid >> 7) * 32, cb = ((tid >> 6) & 1) * 32;   // wavefront w: quadrant (w >> 1, w & 1)
#pragma unroll
      for (int kg = 0; kg < RC_SLAB / 4; kg++) {
#pragma unroll
        for (int mi = 0; mi < 2; mi++)
#pragma unroll
          for (int mj = 0; mj < 2; mj++) RC_MFMA(acc[me][mi][mj], blkA, ca + 16 * mi, blkB, cb + 16 * mj, 4 * kg, lane);
      }
    }
    RC_SYNC();
  }
  RC_EACH_THREAD(tid) {
    const int me = RC_ME(tid), lane = tid & 63, ca = (tid >> 7) * 32, cb = ((tid >> 6) & 1) * 32;
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
      for (int mj = 0; mj < 2; mj++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++)
          P[(ca + 16 * mi + (lane >> 4) + 4 * reg) * RC_TC + cb + 16 * mj + (lane & 15)] = acc[me][mi][mj][reg];
  }
}

// ws [S][RC_TC][RC_TC]: the partials of tile (ti, tj) of one pair; dens [npx][npy]: that pair's surface
RC_FN void rkd_tile_finish(const double *ws, const long long S, const long long N, const int ti, const int tj, const int npx, const int npy,
                           const double hx, const double hy, double *dens, const int rc_nthreads) {
  RC_EACH_THREAD(tid) {
    for (int e = tid; e < RC_TC * RC_TC; e += RC_BLOCK) {
      const int i = ti * RC_TC + (e >> 6), j = tj * RC_TC + (e & (RC_TC - 1));
      if (i >= npx || j >= npy) continue;
      double acc = 0.0;
      for (long long s = 0; s < S; s++) acc += ws[s * RC_TC * RC_TC + e];
      dens[(long long)i * npy + j] = acc / ((double)N * RKD_TWO_PI * hx * hy);
    }
  }
}

#ifndef RH_KDE_HOST
// grid: the chunk's columns x S x gtiles, blockIdx.x = (column * S + s) * gtiles + tile; cols, grid [p_cnt][G], bw [p_cnt]: from the
// chunk's first column on; ws [p_cnt][S][G]
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_kde_point_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const long long first,
                    const long long thin, const long long kept, const long long N, const int *__restrict__ cols, const int p_cnt,
                    const double *__restrict__ grid, const double *__restrict__ bw, const int G, const int gtiles, const long long S,
                    double *__restrict__ ws) {
  __shared__ double lds[RKD_ROWS];
  const long long cs = (long long)blockIdx.x / gtiles, kl = cs / S, s = cs - kl * S;
  const int gt = (int)((long long)blockIdx.x - cs * gtiles);
  if (kl >= p_cnt) return;
  rkd_point_split(draws + first * nvars, iterations, nvars, thin, kept, N, cols[kl], grid + kl * G, G, bw[kl], gt * RKD_GT, s, lds,
                  ws + (kl * S + s) * G, RC_BLOCK);
}

// grid: ceil(p_cnt * G / RC_BLOCK); density [p_cnt][G] from the chunk's first column on
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_kde_finish_kernel(const double *__restrict__ ws, const long long S, const long long N, const int p_cnt, const int G,
                     const double *__restrict__ bw, double *__restrict__ density) {
  const long long e = (long long)blockIdx.x * RC_BLOCK + threadIdx.x;
  if (e >= (long long)p_cnt * G) return;
  const long long kl = e / G;
  density[e] = rkd_point_finish(ws + kl * S * G, S, G, (int)(e - kl * G), N, bw[kl]);
}

// grid: the chunk's units [u_lo, u_lo + u_cnt) x S, blockIdx.x = (unit - u_lo) * S + s; pairs [P][2], xgrid [P][npx], ygrid [P][npy],
// bw [P][2]; ws [u_cnt][S][RC_TC][RC_TC]
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_kde_tile_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const long long first,
                   const long long thin, const long long kept, const long long N, const int *__restrict__ pairs,
                   const double *__restrict__ xgrid, const double *__restrict__ ygrid, const double *__restrict__ bw, const int npx,
                   const int npy, const int tx, const int ty, const long long u_lo, const int u_cnt, const long long S,
                   double *__restrict__ ws) {
  __shared__ double lds[RC_TILE_LDS];
  const long long ul = (long long)blockIdx.x / S, s = (long long)blockIdx.x - ul * S;
  if (ul >= u_cnt) return;
  int p, ti, tj;
  rkd_unit_of(u_lo + ul, tx, ty, &p, &ti, &tj);
  rkd_tile_split(draws + first * nvars, iterations, nvars, thin, kept, N, pairs[2 * p], pairs[2 * p + 1], xgrid + (long long)p * npx,
                 ygrid + (long long)p * npy, npx, npy, bw[2 * p], bw[2 * p + 1], ti, tj, s, lds, ws + (ul * S + s) * RC_TC * RC_TC, RC_BLOCK);
}

// grid: the chunk's units; density [P][npx][npy]
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_kde_pairs_finish_kernel(const double *__restrict__ ws, const long long S, const long long N, const double *__restrict__ bw, const int npx,
                           const int npy, const int tx, const int ty, const long long u_lo, double *__restrict__ density) {
  int p, ti, tj;
  rkd_unit_of(u_lo + blockIdx.x, tx, ty, &p, &ti, &tj);
  rkd_tile_finish(ws + (long long)blockIdx.x * S * RC_TC * RC_TC, S, N, ti, tj, npx, npy, bw[2 * p], bw[2 * p + 1],
                  density + (long long)p * npx * npy, RC_BLOCK);
}
#endif
#endif
