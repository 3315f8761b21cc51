// rh_joint.hip.h -- joint convergence of the parameters over device-resident draws: the multivariate effective sample size (Vats,
// Flegal, Jones 2019: batch means, replicated over the chains) and the multivariate potential scale reduction factor (Brooks and
// Gelman 1998).  Three Gram matrices of centred rows -- within the chains, between their means, of the batch means -- on the fp64
// matrix cores; the K x K finish (two log-determinants, one largest eigenvalue) is the host's (csrc/dense_sym.hpp).
//
// Model-independent: a translation unit of its own behind rh_cov.hip.h's text (its operand maps, its LDS layout of a staged slab,
// its stepping of a flat row through the groups, its order of the tile pairs), compiled once per toolchain through the engine's
// build_source() and inspected like every other code object before it is launched.  wave64, gfx950.
//
// draws [chains C][iterations][nvars]; the window first, count (no thinning: the estimators rest on consecutive draws); column k of
// every result is parameter cols[k], K columns.  b: the batch length, a = floor(count / b) batches per chain, n' = a b; the FIRST
// count - n' draws of every chain's window are dropped, N = C n'.  Every sum's order depends on (C, count, b) alone:
//   B[c][k][.]  = one accumulator from +0.0 over the b rows of batch k of chain c, ascending;  Ybar[c][k][.] = B / (double)b;
//   T[c][.]     = one accumulator from +0.0 over B[c][0], B[c][1], ..;                        m[c][.] = T / (double)n';
//   mu[.]       = (one accumulator from +0.0 over T[0], T[1], ..) / (double)N;
//   a Gram of R flat rows y[r][.] (the draws less their chain's m; the rows of Ybar less mu; the rows of m less mu): a split is
//   RC_SPLIT consecutive flat rows, P_s[i][j] = one accumulator from +0.0, r ascending in split s: acc = fma(y[r][i], y[r][j], acc),
//   G[i][j] = the P_s added in ascending s from +0.0 -- GW, GS, GB;
//   W      = GW / (double)(C (n' - 1));       Bn = GB / (double)(C - 1)  (one chain: 0 / 0, NaN);
//   Sigma  = (double)b * GS / (double)(C a - 1);
//   Lambda = ((double)(C (n' - 1)) * W + (double)(n' (C - 1)) * Bn) / (double)(N - 1), IEEE operations in that order (the ANOVA
//            identity: two positive semi-definite terms, no cancellation, no further pass); one chain: Lambda = W.
// Tile pairs bi <= bj (on the diagonal tile for i <= j) and mirrored: every matrix is bitwise symmetric.  A NaN in a column makes
// that column's row and column of every matrix NaN and touches nothing else.  No floating-point atomics; nothing depends on the
// tiling, the chunking of the tile pairs, the order of the column list or the launch.
//
//   rh_joint_batch_kernel   one workgroup = one chain x RC_TC selected columns, the lanes along the columns (512 B of a row per
//                           wavefront load where the list is contiguous).  Its four wavefronts take the batches round-robin; after
//                           every round the four batch sums meet in LDS and the first wavefront adds them to the chain's sum in
//                           ascending k.  Writes Ybar [C][a][K], m [C][K], T [C][K].
//   rh_joint_mean_kernel    one thread per column: T over the chains in ascending c, divided by N.
//   rh_joint_gram_kernel    rh_cov_tile_kernel's work split and MFMA loop (one pair of column tiles x one split per workgroup, slabs
//                           of RC_SLAB centred rows at stride RC_STRIDE in LDS, a 32 x 32 quadrant per wavefront as 2 x 2
//                           accumulators of v_mfma_f64_16x16x4_f64) over a row source that is a launch argument (rj_src): flat row
//                           r is row r % rpg of group r / rpg and is centred on load by its group's centre.  A slab whose live rows
//                           lie in one group (a uniform test on the slab's first row, stepped like rc_row_step's) takes the centre
//                           from registers, reloaded where the group changes; a slab that straddles groups reads it per row.
//                           Launched three times: the draws by chain about m, Ybar about mu, m about mu.
//   rh_joint_finish_kernel  one workgroup per tile pair: the three Grams' splits in ascending s, the divisors, Lambda, both mirrors.
// Workspace: (S_W + S_S + S_B) * 32 KiB per tile pair (the three Grams' splits); the host walks the pairs in chunks under
// RC_WS_CAP_BYTES and refuses a shape whose single pair is beyond it.
//
// As in rh_cov.hip.h the block routines are plain C++ over (thread id, LDS pointer): with RH_JOINT_HOST (and RH_COV_HOST) defined
// they compile with a host compiler, the MFMA a chain of fma over k = 0, 1, 2, 3 (tests/test_joint_device_cpu.py).
#ifndef RH_JOINT_HIP_H
#define RH_JOINT_HIP_H

#define RJ_MAX_K 256            // the host finish is O(K^3) on one core
#define RJ_WAVES (RC_BLOCK / 64)

// where a Gram's flat rows lie and what they are centred by
struct rj_src {
  const double *base;           // row 0 of group 0, column 0
  long long rpg;                // rows of a group
  long long gstride, rstride;   // doubles between two groups' first rows, between two rows of a group
  const int *cols;              // selected column k is column cols[k] of a row (NULL: column k)
  const double *centre;         // [groups][K], or [1][K] at cstride 0
  long long cstride;            // doubles between two groups' centres
};

// ---- batch means -----------------------------------------------------------------------------------------------------------------
// Chain c, columns [k0, k0 + RC_TC) of the selection.  base: draws[0][first + dropped][0].  lds: RJ_WAVES * RC_TC doubles.
RC_FN void rj_batch_chain(const double *base, const long long iterations, const long long nvars, const int *cols, const int K, const int k0,
                          const long long c, const long long b, const long long a, double *lds, double *ybar, double *m, double *tsum,
                          const int rc_nthreads) {
  double chain[RC_NSTATE];
  RC_EACH_THREAD(tid) chain[RC_ME(tid)] = 0.0;
  for (long long kb = 0; kb < a; kb += RJ_WAVES) {
    RC_EACH_THREAD(tid) {
      const int lane = tid & 63, k = k0 + lane;
      const long long batch = kb + (tid >> 6);                  // wave-uniform
      double acc = 0.0;
      if (batch < a && k < K) {
        const double *p = base + (c * iterations + batch * b) * nvars + cols[k];
#pragma unroll 8
        for (long long t = 0; t < b; t++) acc += p[t * nvars];
        ybar[(c * a + batch) * K + k] = acc / (double)b;
      }
      lds[(tid >> 6) * RC_TC + lane] = acc;
    }
    RC_SYNC();
    RC_EACH_THREAD(tid) {
      if (tid < RC_TC) {
        double s = chain[RC_ME(tid)];
        for (int w = 0; w < RJ_WAVES && kb + w < a; w++) s += lds[w * RC_TC + tid];
        chain[RC_ME(tid)] = s;
      }
    }
    RC_SYNC();
  }
  RC_EACH_THREAD(tid) {
    if (tid < RC_TC && k0 + tid < K) {
      tsum[c * K + k0 + tid] = chain[RC_ME(tid)];
      m[c * K + k0 + tid] = chain[RC_ME(tid)] / (double)(a * b);
    }
  }
}

RC_FN double rj_mean(const double *tsum, const long long C, const int K, const int k, const long long N) {
  double acc = 0.0;
  for (long long c = 0; c < C; c++) acc += tsum[c * K + k];
  return acc / (double)N;
}

// ---- tile pair x split of one Gram -------------------------------------------------------------------------------------------------
// Tile pair (bi, bj), bi <= bj, over split s of the R flat rows of src: P [RC_TC][RC_TC].  lds: RC_TILE_LDS doubles.
RC_FN void rj_gram_split(const rj_src src, const long long R, const int K, const int bi, const int bj, const long long s, double *lds,
                         double *P, const int rc_nthreads) {
  const long long r_lo = s * RC_SPLIT, r_hi = R - r_lo < RC_SPLIT ? R : r_lo + RC_SPLIT;
  const long long rpg = src.rpg;
  const long long sq = (RC_BLOCK / RC_TC) / rpg, sr = (RC_BLOCK / RC_TC) - sq * rpg;   // a thread's step from row to row
  const long long bq = RC_SLAB / rpg, br = RC_SLAB - bq * rpg;                         // the slab's step
  const bool diag = bi == bj;
  const int nblk = diag ? 1 : 2;
  double *blkA = lds, *blkB = diag ? lds : lds + RC_SLAB * RC_STRIDE;
  rc_d4 acc[RC_NSTATE][2][2];
  int sel[RC_NSTATE][2], col[RC_NSTATE][2];   // this thread's selected column in either block (-1: past K, staged as +0.0); where it lies in a row
  double mu[RC_NSTATE][2];                    // ... and its centre in group `cached`
  RC_EACH_THREAD(tid) {
    const int me = RC_ME(tid);
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int k = (q ? bj : bi) * RC_TC + (tid & (RC_TC - 1));
      sel[me][q] = k < K ? k : -1;
      col[me][q] = k < K ? (src.cols ? src.cols[k] : k) : -1;
      mu[me][q] = 0.0;
#pragma unroll
      for (int mm = 0; mm < 2; mm++)
#pragma unroll
        for (int e = 0; e < 4; e++) acc[me][q][mm][e] = 0.0;
    }
  }
  rc_row s0 = rc_row_of(r_lo, rpg);           // the slab's first row: the same in every thread
  long long cached = -1;
  for (long long r0 = r_lo; r0 < r_hi; r0 += RC_SLAB) {
    const int nlive = (int)(r_hi - r0 < RC_SLAB ? r_hi - r0 : RC_SLAB);
    if (s0.j + nlive <= rpg) {                // every live row in group s0.c: the centre from registers
      if (s0.c != cached) {
        RC_EACH_THREAD(tid) {
          const int me = RC_ME(tid);
#pragma unroll
          for (int q = 0; q < 2; q++) mu[me][q] = sel[me][q] >= 0 ? src.centre[s0.c * src.cstride + sel[me][q]] : 0.0;
        }
        cached = s0.c;
      }
      RC_EACH_THREAD(tid) {
        const int me = RC_ME(tid), c = tid & (RC_TC - 1);
#pragma unroll 4
        for (int row = tid >> 6; row < RC_SLAB; row += RC_BLOCK / RC_TC) {
          const bool live = row < nlive;
          const long long off = s0.c * src.gstride + (s0.j + row) * src.rstride;
#pragma unroll
          for (int q = 0; q < 2; q++) {
            if (q < nblk) {
              const bool have = live && col[me][q] >= 0;                  // else: staged as +0.0 (the load is of base[0], unused)
              const double x = src.base[have ? off + col[me][q] : 0];
              lds[q * RC_SLAB * RC_STRIDE + row * RC_STRIDE + c] = have ? x - mu[me][q] : 0.0;
            }
          }
        }
      }
    } else {                                  // the slab straddles groups: every row's own centre
      RC_EACH_THREAD(tid) {
        const int me = RC_ME(tid), c = tid & (RC_TC - 1);
        rc_row w = rc_row_of(r0 + (tid >> 6), rpg);
#pragma unroll 4
        for (int row = tid >> 6; row < RC_SLAB; row += RC_BLOCK / RC_TC) {
          const bool live = row < nlive;
          const long long off = w.c * src.gstride + w.j * src.rstride;
#pragma unroll
          for (int q = 0; q < 2; q++) {
            if (q < nblk) {
              const bool have = live && col[me][q] >= 0;                  // else: neither the row nor its group need exist
              const double x = src.base[have ? off + col[me][q] : 0];
              const double ctr = src.centre[have ? w.c * src.cstride + sel[me][q] : 0];
              lds[q * RC_SLAB * RC_STRIDE + row * RC_STRIDE + c] = have ? x - ctr : 0.0;
            }
          }
          rc_row_step(w, rpg, sq, sr);
        }
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
    rc_row_step(s0, rpg, bq, br);
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
// wsw [SW], wss [SS], wsb [SB] partial tiles of pair (bi, bj); W, Bn, Sigma, Lambda [K][K]
RC_FN void rj_finish_pair(const double *wsw, const double *wss, const double *wsb, const long long SW, const long long SS, const long long SB,
                          const long long C, const long long a, const long long b, const int bi, const int bj, const int K, double *W,
                          double *Bn, double *Sigma, double *Lambda, const int rc_nthreads) {
  const long long np = a * b, N = C * np;
  const double dw = (double)(C * (np - 1)), db = (double)(np * (C - 1));
  RC_EACH_THREAD(tid) {
    for (int e = tid; e < RC_TC * RC_TC; e += RC_BLOCK) {
      const int i = e >> 6, j = e & (RC_TC - 1);
      const long long gi = (long long)bi * RC_TC + i, gj = (long long)bj * RC_TC + j;
      if (gi >= K || gj >= K || (bi == bj && i > j)) continue;
      double gw = 0.0, gs = 0.0, gb = 0.0;
      for (long long s = 0; s < SW; s++) gw += wsw[s * RC_TC * RC_TC + e];
      for (long long s = 0; s < SS; s++) gs += wss[s * RC_TC * RC_TC + e];
      for (long long s = 0; s < SB; s++) gb += wsb[s * RC_TC * RC_TC + e];
      const double w = gw / dw, bn = gb / (double)(C - 1), sg = (double)b * gs / (double)(C * a - 1);
      const double lam = C == 1 ? w : (dw * w + db * bn) / (double)(N - 1);
      W[gi * K + gj] = w;           W[gj * K + gi] = w;
      Bn[gi * K + gj] = bn;         Bn[gj * K + gi] = bn;
      Sigma[gi * K + gj] = sg;      Sigma[gj * K + gi] = sg;
      Lambda[gi * K + gj] = lam;    Lambda[gj * K + gi] = lam;
    }
  }
}

#ifndef RH_JOINT_HOST
// grid: C x ceil(K / RC_TC), blockIdx.x = c * ctiles + column tile; start = first + dropped
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_joint_batch_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const long long start,
                      const int *__restrict__ cols, const int K, const int ctiles, const long long b, const long long a,
                      double *__restrict__ ybar, double *__restrict__ m, double *__restrict__ tsum) {
  __shared__ double lds[RJ_WAVES * RC_TC];
  const long long c = (long long)(blockIdx.x / (unsigned)ctiles);
  const int ct = (int)(blockIdx.x - (unsigned)c * (unsigned)ctiles);
  rj_batch_chain(draws + start * nvars, iterations, nvars, cols, K, ct * RC_TC, c, b, a, lds, ybar, m, tsum, RC_BLOCK);
}

// grid: ceil(K / RC_BLOCK)
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_joint_mean_kernel(const double *__restrict__ tsum, const long long C, const int K, const long long N, double *__restrict__ mu) {
  const int k = (int)(blockIdx.x * RC_BLOCK + threadIdx.x);
  if (k < K) mu[k] = rj_mean(tsum, C, K, k, N);
}

// grid: the chunk's tile pairs [p_lo, p_lo + p_cnt) x S, blockIdx.x = (pair - p_lo) * S + s; ws [p_cnt][S][RC_TC][RC_TC]
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_joint_gram_kernel(const rj_src src, const long long R, const int K, const long long p_lo, const int p_cnt, const long long S,
                     double *__restrict__ ws) {
  __shared__ double lds[RC_TILE_LDS];
  const long long pl = (long long)blockIdx.x / S, s = (long long)blockIdx.x - pl * S;
  if (pl >= p_cnt || s * RC_SPLIT >= R) return;
  int bi, bj;
  rc_pair_of(p_lo + pl, (K + RC_TC - 1) / RC_TC, &bi, &bj);
  rj_gram_split(src, R, K, bi, bj, s, lds, ws + (pl * S + s) * RC_TC * RC_TC, RC_BLOCK);
}

// grid: the chunk's tile pairs; wsw [p_cnt][SW], wss [p_cnt][SS], wsb [p_cnt][SB] tiles
extern "C" __global__ void __launch_bounds__(RC_BLOCK)
rh_joint_finish_kernel(const double *__restrict__ wsw, const double *__restrict__ wss, const double *__restrict__ wsb, const long long SW,
                       const long long SS, const long long SB, const long long C, const long long a, const long long b, const long long p_lo,
                       const int K, double *__restrict__ W, double *__restrict__ Bn, double *__restrict__ Sigma, double *__restrict__ Lambda) {
  int bi, bj;
  rc_pair_of(p_lo + blockIdx.x, (K + RC_TC - 1) / RC_TC, &bi, &bj);
  const long long tile = RC_TC * RC_TC, p = blockIdx.x;
  rj_finish_pair(wsw + p * SW * tile, wss + p * SS * tile, wsb + p * SB * tile, SW, SS, SB, C, a, b, bi, bj, K, W, Bn, Sigma, Lambda, RC_BLOCK);
}
#endif
#endif
