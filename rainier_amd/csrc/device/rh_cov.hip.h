// rh_cov.hip.h -- pooled sample covariance and correlation of the kept draws over device-resident draws: how two parameters move
// together (the reference answers it with scatter / contour of pairs, rainier-notebook package.scala:79-98; the divisor N - 1 is
// CovarianceEstimator.covariance's, MassMatrixEstimator.scala:38-47).  X^T X of the centred draws on the fp64 matrix cores.
//
// Model-independent: a translation unit of its own (no RH_NVARS, no generated code), compiled once per toolchain through the
// engine's build_source() and inspected like every other code object before it is launched.  wave64, gfx950.
//
// draws [chains][iterations][nvars].  Flat row r = c * kept + j is draw (c, first + j * thin), N = chains * kept rows; column k of
// the result is parameter cols[k], K columns.  The sums run in a fixed order that depends on N alone:
//   a split is RC_SPLIT consecutive flat rows, S = ceil(N / RC_SPLIT), the last one ragged;
//   mean[k]   = (sum over s ascending of (sum over the rows r of split s ascending of x[r][k])) / (double)N, every sum one
//               accumulator from +0.0 with plain adds;
//   d[r][k]   = x[r][k] - mean[k] (two passes on purpose: a mean many standard deviations from zero costs no digits);
//   P_s[a][b] = one accumulator from +0.0, r ascending in split s: acc = fma(d[r][a], d[r][b], acc); the rows past N of a ragged
//               group of four are staged as +0.0 and leave acc as it is;
//   cov[a][b] = (sum over s ascending of P_s[a][b]) / (double)(N - 1), computed for tile pairs bi <= bj (on the diagonal tile for
//               a <= b) and mirrored: bitwise symmetric;
//   corr[a][b] = cov[a][b] / (sqrt(cov[a][a]) * sqrt(cov[b][b])), the diagonal exactly 1.0 where cov[a][a] is finite and > 0, else
//               NaN (so is the pair of a column that the list names twice: it is a diagonal entry of the whole matrix); not clamped.
// A NaN in a column makes that column's row and column of the result NaN and touches nothing else.  No floating-point atomics;
// nothing depends on the tiling, the chunking of the tile pairs, the order of the column list or the launch.
//
//   rh_cov_mean_kernel         one workgroup = RC_TC selected columns x one split: slabs of RC_MROWS rows go through LDS (the lanes
//                              along the columns on load, 512 B per row), thread t < RC_TC adds column t's rows in ascending order.
//                              Writes part [S][K].
//   rh_cov_mean_finish_kernel  one thread per column: the S partial sums in ascending s, divided by N.
//   rh_cov_tile_kernel         one workgroup (4 wavefronts) = one pair of column tiles (bi <= bj) x one split.  Slabs of RC_SLAB
//                              centred rows [row][col] in LDS (the subtraction happens on load; an A block and a B block, one
//                              block on the diagonal), row stride RC_STRIDE = 80 doubles: the 16 lanes of one k read 16 consecutive
//                              doubles and the next k's start 80 = 16 mod 32 doubles on, so the 32 lanes that a ds_read_b64 serves
//                              together cover all 64 banks once.  Every wavefront owns a 32 x 32 quadrant as 2 x 2 accumulators of
//                              v_mfma_f64_16x16x4_f64, four rows per instruction.  Operand maps: A and B hold one f64 per lane,
//                              i | j = lane & 15, k = lane >> 4; D is col = lane & 15, row = (lane >> 4) + 4 * reg.  Every loop
//                              around the MFMAs is wave-uniform: ragged rows and columns are zero-filled in staging.
//                              Writes P_s to the workspace [pair][S][RC_TC][RC_TC].
//   rh_cov_finish_kernel       one workgroup per tile pair: the splits in ascending s, the division, both mirrors into cov [K][K].
//   rh_cov_corr_kernel         one thread per entry of corr [K][K], from the finished cov.
// Workspace: S * 32 KiB per tile pair; the host walks the pairs in chunks that stay below RC_WS_CAP_BYTES (128 MiB, the trace
// kernels' figure) and refuses a shape whose single pair is beyond it.
//
// The block routines below are plain C++ over (thread id, LDS pointer): with RH_COV_HOST defined they compile with a host compiler,
// every "thread" of a phase run in turn, and the MFMA is a function that applies fma for k = 0, 1, 2, 3 in that order at the same
// lane maps (tests/test_covariance_device_cpu.py): same text, same order.
#ifndef RH_COV_HIP_H
#define RH_COV_HIP_H

#define RC_BLOCK 256            // threads of every kernel here
#define RC_SPLIT 4096           // flat rows of a split: one accumulator per entry runs over them
#define RC_TC 64                // columns of a tile
#define RC_SLAB 32              // rows of a staged slab of the tile kernel: 8 k-groups of 4
#define RC_STRIDE 80            // doubles between two rows of a staged block
#define RC_TILE_LDS (2 * RC_SLAB * RC_STRIDE)   // 40 KiB: four workgroups per CU's 160 KiB, within the family's 63 KiB
#define RC_MROWS 64             // rows of a slab of the mean kernel
#define RC_WS_CAP_BYTES (128ll << 20)
#define RC_PAIR_BYTES(S) ((long long)(S) * RC_TC * RC_TC * 8)   // workspace of one tile pair

#ifndef RH_COV_HOST
#define RC_FN static __device__ __forceinline__
#define RC_SYNC() __syncthreads()
#define RC_TID0 ((int)threadIdx.x)
#define RC_TID1 ((int)threadIdx.x + 1)
#define RC_NSTATE 1             // per-thread state that lives across barriers: registers
#define RC_ME(tid) 0
typedef double rc_d4 __attribute__((ext_vector_type(4)));
#else
#define RC_FN static inline
#define RC_SYNC() ((void)0)
#define RC_TID0 0
#define RC_TID1 rc_nthreads
#define RC_NSTATE RC_BLOCK      // ... on the host: one slot per thread
#define RC_ME(tid) (tid)
struct rc_d4 {
  double v[4];
  double &operator[](int i) { return v[i]; }
};
#endif
// every thread of the workgroup (device: this one; host: each in turn -- a phase ends where the device has its barrier)
#define RC_EACH_THREAD(tid) for (int tid = RC_TID0; tid < RC_TID1; tid++)

// tile pair p (0 <= p < T (T + 1) / 2) in the order (0,0) (0,1) .. (0,T-1) (1,1) ..: bi <= bj
RC_FN void rc_pair_of(long long p, const int T, int *bi, int *bj) {
  int i = 0;
  while (p >= T - i) { p -= T - i; i++; }
  *bi = i;
  *bj = i + (int)p;
}

// Flat row r is kept iteration j of chain c: one division where a thread starts, then steps of RC_BLOCK / RC_TC rows.  The draw's offset
// in doubles from draws[0][first][0] is (c * iterations + j * thin) * nvars.
struct rc_row { long long c, j; };
RC_FN rc_row rc_row_of(const long long r, const long long kept) {
  rc_row w;
  w.c = r / kept;
  w.j = r - w.c * kept;
  return w;
}
// step = sq * kept + sr, 0 <= sr < kept (the caller's, uniform): no loop and no branch for the lanes to diverge on
RC_FN void rc_row_step(rc_row &w, const long long kept, const long long sq, const long long sr) {
  w.j += sr;
  const bool wrap = w.j >= kept;
  w.j -= wrap ? kept : 0;
  w.c += sq + (wrap ? 1 : 0);
}

// ---- mean ------------------------------------------------------------------------------------------------------------------------
// Columns [k0, k0 + RC_TC) of the selection over split s.  base: draws[0][first][0].  lds: RC_MROWS * RC_TC doubles.  part [S][K].
RC_FN void rc_mean_split(const double *base, const long long iterations, const long long nvars, const long long thin, const long long kept,
                         const long long N, const int *cols, const int K, const int k0, const long long s, double *lds, double *part,
                         const int rc_nthreads) {
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
        rc_row w = rc_row_of(r0 + (tid >> 6), kept);
        for (int row = tid >> 6; row < nr; row += RC_BLOCK / RC_TC) {
          lds[row * RC_TC + (tid & (RC_TC - 1))] = base[(w.c * iterations + w.j * thin) * nvars + col];
          rc_row_step(w, kept, sq, sr);
        }
      }
    }
    RC_SYNC();
    RC_EACH_THREAD(tid) {
      if (tid < RC_TC && k0 + tid < K) {
        double a = acc[RC_ME(tid)];
        for (int row = 0; row < nr; row++) a += lds[row * RC_TC + tid];
        acc[RC_ME(tid)] = a;
      }
    }
    RC_SYNC();
  }
  RC_EACH_THREAD(tid) {
    if (tid < RC_TC && k0 + tid < K) part[s * K + k0 + tid] = acc[RC_ME(tid)];
  }
}

RC_FN double rc_mean_finish(const double *part, const long long S, const int K, const int k, const long long N) {
  double acc = 0.0;
  for (long long s = 0; s < S; s++) acc += part[s * K + k];
  return acc / (double)N;
}

// ---- tile pair x split -----------------------------------------------------------------------------------------------------------
// what lane `lane` hands the MFMA of the rows r0 .. r0 + 3 of a staged block, columns c0 .. c0 + 15: [k = lane >> 4][lane & 15]
RC_FN double rc_operand(const double *blk, const int r0, const int c0, const int lane) {
  return blk[(r0 + (lane >> 4)) * RC_STRIDE + c0 + (lane & 15)];
}
#ifndef RH_COV_HOST
#define RC_MFMA(acc, blkA, ca, blkB, cb, r0, lane) \
  (acc) = __builtin_amdgcn_mfma_f64_16x16x4f64(rc_operand(blkA, r0, ca, lane), rc_operand(blkB, r0, cb, lane), (acc), 0, 0, 0)
#else
// v_mfma_f64_16x16x4_f64 as this file takes it to work: lane's register `reg` is D[i = (lane >> 4) + 4 reg][j = lane & 15], A[i][k]
// comes from lane i + 16 k and B[k][j] from lane j + 16 k, and k runs 0, 1, 2, 3 as a chain of fma
static inline void rc_mfma_host(rc_d4 &acc, const double *blkA, const int ca, const double *blkB, const int cb, const int r0, const int lane) {
  for (int reg = 0; reg < 4; reg++) {
    const int i = (lane >> 4) + 4 * reg, j = lane & 15;
    for (int k = 0; k < 4; k++) acc[reg] = __builtin_fma(rc_operand(blkA, r0, ca, i + 16 * k), rc_operand(blkB, r0, cb, j + 16 * k), acc[reg]);
  }
}
#define RC_MFMA(acc, blkA, ca, blkB, cb, r0, lane) rc_mfma_host(acc, blkA, ca, blkB, cb, r0, lane)
#endif

// Tile pair (bi, bj), bi <= bj, over split s: P [RC_TC][RC_TC] = sum over the split's rows of d[r][bi * RC_TC + a] * d[r][bj * RC_TC + b].
// base: draws[0][first][0]; mean [K]; lds: RC_TILE_LDS doubles.
RC_FN void rc_tile_split(const double *base, const long long iterations, const long long nvars, const long long thin, const long long kept,
                         const long long N, const int *cols, const int K, const double *mean, const int bi, const int bj, const long long s,
                         double *lds, double *P, const int rc_nthreads) {
  const long long r_lo = s * RC_SPLIT, r_hi = N - r_lo < RC_SPLIT ? N : r_lo + RC_SPLIT;
  const long long sq = (RC_BLOCK / RC_TC) / kept, sr = (RC_BLOCK / RC_TC) - sq * kept;
  const bool diag = bi == bj;
  const int nblk = diag ? 1 : 2;
  double *blkA = lds, *blkB = diag ? lds : lds + RC_SLAB * RC_STRIDE;
  rc_d4 acc[RC_NSTATE][2][2];
  int col[RC_NSTATE][2];       // the staged column of this thread in either block (-1: past K, staged as +0.0) and its mean
  double mu[RC_NSTATE][2];
  RC_EACH_THREAD(tid) {
    const int me = RC_ME(tid);
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int k = (q ? bj : bi) * RC_TC + (tid & (RC_TC - 1));
      col[me][q] = k < K ? cols[k] : -1;
      mu[me][q] = k < K ? mean[k] : 0.0;
#pragma unroll
      for (int m = 0; m < 2; m++)
#pragma unroll
        for (int e = 0; e < 4; e++) acc[me][q][m][e] = 0.0;
    }
  }
  for (long long r0 = r_lo; r0 < r_hi; r0 += RC_SLAB) {
    RC_EACH_THREAD(tid) {
      const int me = RC_ME(tid), c = tid & (RC_TC - 1);
      rc_row w = rc_row_of(r0 + (tid >> 6), kept);
#pragma unroll 4
      for (int row = tid >> 6; row < RC_SLAB; row += RC_BLOCK / RC_TC) {
        const bool live = r0 + row < r_hi;
        const long long off = (w.c * iterations + w.j * thin) * nvars;
#pragma unroll
        for (int q = 0; q < 2; q++) {
          if (q < nblk) {
            const bool have = live && col[me][q] >= 0;                     // else: staged as +0.0 (the load is of base[0], unused)
            const double x = base[have ? off + col[me][q] : 0];
            lds[q * RC_SLAB * RC_STRIDE + row * RC_STRIDE + c] = have ? x - mu[me][q] : 0.0;
          }
        }
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

// ---- finish ----------------------------------------------------------------------------------------------------------------------
// ws [S][RC_TC][RC_TC]: the partials of tile pair (bi, bj); cov [K][K]
RC_FN void rc_finish_pair(const double *ws, const long long S, const long long N, const int bi, const int bj, const int K, double *cov,
                          const int rc_nthreads) {
  RC_EACH_THREAD(tid) {
    for (int e = tid; e < RC_TC * RC_TC; e += RC_BLOCK) {
      const int a = e >> 6, b = e & (RC_TC - 1);
      const long long ga = (long long)bi * RC_TC + a, gb = (long long)bj * RC_TC + b;
      if (ga >= K || gb >= K || (bi == bj && a > b)) continue;
      double acc = 0.0;
      for (long long s = 0; s < S; s++) acc += ws[s * RC_TC * RC_TC + e];
      const double v = acc / (double)(N - 1);
      cov[ga * K + gb] = v;
      cov[gb * K + ga] = v;
    }
  }
}

// (a pair of one parameter with itself -- the diagonal, and a column the list names twice -- is the diagonal of the whole matrix)
RC_FN double rc_corr_entry(const double *cov, const int *cols, const long long K, const long long a, const long long b) {
  const double va = cov[a * K + a], vb = cov[b * K + b];
  if (cols[a] == cols[b]) return va > 0.0 && va < __builtin_inf() ? 1.0 : __builtin_nan("");
  return cov[a * K + b] / (__builtin_sqrt(va) * __builtin_sqrt(vb));
}

#ifndef RH_COV_HOST
// grid: S x ceil(K / RC_TC), blockIdx.x = s * ctiles + column tile
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_cov_mean_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const long long first,
                   const long long thin, const long long kept, const long long N, const int *__restrict__ cols, const int K,
                   const int ctiles, double *__restrict__ part) {
  __shared__ double lds[RC_MROWS * RC_TC];
  const long long s = (long long)(blockIdx.x / (unsigned)ctiles);
  const int ct = (int)(blockIdx.x - (unsigned)s * (unsigned)ctiles);
  if (s * RC_SPLIT >= N) return;
  rc_mean_split(draws + first * nvars, iterations, nvars, thin, kept, N, cols, K, ct * RC_TC, s, lds, part, RC_BLOCK);
}

// grid: ceil(K / RC_BLOCK)
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_cov_mean_finish_kernel(const double *__restrict__ part, const long long S, const int K, const long long N, double *__restrict__ mean) {
  const int k = (int)(blockIdx.x * RC_BLOCK + threadIdx.x);
  if (k < K) mean[k] = rc_mean_finish(part, S, K, k, N);
}

// grid: the chunk's tile pairs [p_lo, p_lo + p_cnt) x S, blockIdx.x = (pair - p_lo) * S + s; ws [p_cnt][S][RC_TC][RC_TC]
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_cov_tile_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const long long first,
                   const long long thin, const long long kept, const long long N, const int *__restrict__ cols, const int K,
                   const double *__restrict__ mean, const long long p_lo, const int p_cnt, const long long S, double *__restrict__ ws) {
  __shared__ double lds[RC_TILE_LDS];
  const long long pl = (long long)blockIdx.x / S, s = (long long)blockIdx.x - pl * S;
  if (pl >= p_cnt) return;
  int bi, bj;
  rc_pair_of(p_lo + pl, (K + RC_TC - 1) / RC_TC, &bi, &bj);
  rc_tile_split(draws + first * nvars, iterations, nvars, thin, kept, N, cols, K, mean, bi, bj, s, lds, ws + (pl * S + s) * RC_TC * RC_TC, RC_BLOCK);
}

// grid: the chunk's tile pairs
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_cov_finish_kernel(const double *__restrict__ ws, const long long S, const long long N, const long long p_lo, const int K,
                     double *__restrict__ cov) {
  int bi, bj;
  rc_pair_of(p_lo + blockIdx.x, (K + RC_TC - 1) / RC_TC, &bi, &bj);
  rc_finish_pair(ws + (long long)blockIdx.x * S * RC_TC * RC_TC, S, N, bi, bj, K, cov, RC_BLOCK);
}

// grid: ceil(K * K / RC_BLOCK)
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_cov_corr_kernel(const double *__restrict__ cov, const int *__restrict__ cols, const long long K, double *__restrict__ corr) {
  const long long e = (long long)blockIdx.x * RC_BLOCK + threadIdx.x;
  if (e < K * K) corr[e] = rc_corr_entry(cov, cols, K, e / K, e - e / K * K);
}
#endif
#endif
