// rh_hist.hip.h -- histograms of single parameters and joint count grids of pairs of parameters over device-resident draws: the
// shape of a posterior (the reference's density(seq, bounds) and scatter / contour of pairs, rainier-notebook package.scala:63-98).
// One binning pass reads every draw once; only the counts come back.
//
// Model-independent: a translation unit of its own (no RH_NVARS, no generated code), compiled once per toolchain through the
// engine's build_source() and inspected like every other code object before it is launched.  wave64, gfx950.
//
// draws [chains][iterations][nvars].  Flat row r = c * kept + j is draw (c, first + j * thin), N = chains * kept rows; column k of
// the result is parameter cols[k], K columns.  The counts are integers and defined against the edge table e [nbins + 1] the host
// built (draws_plan.hpp: histogram_edges) and by nothing else:
//   bin b < nbins - 1 holds the rows with e[b] <= x < e[b + 1], the last bin is closed (e[nbins - 1] <= x <= e[nbins]);
//   under: x < e[0] (-inf too), over: x > e[nbins] (+inf too), nan: x != x;  sum(counts) + under + over + nan == N.
// A column without a finite value has NaN edges: its -inf rows are under, its +inf rows over.  The bin is guessed from
// (x - lo) * (nbins / (hi - lo)) and then walked down and up against the table until it is the defining one: edges may repeat (a
// width of a few ulps), so the walk is a loop; it is bounded by nbins.  All comparisons are IEEE.  Integer sums: nothing depends on
// the tiling, the chunking, the order of the column list or the launch.
//
//   rh_hist_minmax_kernel         one workgroup = up to RHH_TC selected columns x one split of RHH_SPLIT flat rows: the smallest and
//                                 largest finite value per column.  The lanes run along the columns (W = the power of two that
//                                 holds the tile's columns; a narrow selection wraps the wavefront over 64 / W rows), the
//                                 RHH_BLOCK / W row groups meet in LDS.  Writes part [2][S][K].
//   rh_hist_minmax_finish_kernel  one thread per column: min / max over the splits; NaN, NaN where nothing was finite; -0.0 -> +0.0.
//   rh_hist_bin_kernel            one workgroup = one tile of cpt columns (rhh_tile_cols(nbins): the power of two whose edge tables
//                                 and u32 histograms fit RHH_LDS_BYTES) x one split.  Edge tables [cpt][nbins + 1] f64 and histograms
//                                 [cpt][nbins + 3] u32 (bins, under, over, nan) in dynamic LDS; counting is an LDS integer add --
//                                 lanes on distinct columns never meet on an address, wrapped rows of one column and peaked
//                                 posteriors do, and the LDS atomic serves both.  Ragged rows and columns are masked, not
//                                 zero-filled: a zero would be counted.  Plain vector stores of the partial histogram to the
//                                 workspace [tile][S][cpt][nbins + 3].
//   rh_hist_pair_kernel           one workgroup = one pair x one split: both edge tables and the [nbx][nby] u32 grid (+ one word for
//                                 the rows outside) in LDS, thread t takes rows t, t + RHH_BLOCK, ..  Workspace [pair][S][nbx nby + 1].
//   rh_hist_finish_kernel         both forms: one thread per word of a unit (tile or pair), the S partials summed into 64 bits.
// No global atomics, no floating-point atomics.  The host walks tiles / pairs in chunks whose partials stay below RHH_WS_CAP_BYTES
// and refuses a shape whose single unit is beyond it.
//
// The block routines below are plain C++ over (thread id, LDS pointer): with RH_HIST_HOST defined they compile with a host
// compiler, every "thread" of a phase run in turn (the LDS add a plain add), a phase ending where the device has its barrier
// (tests/test_histogram_device_cpu.py): same text.
#ifndef RH_HIST_HIP_H
#define RH_HIST_HIP_H

#define RHH_BLOCK 256            // threads of every kernel here
#define RHH_SPLIT 4096           // flat rows of a split: a u32 partial count cannot overflow
#define RHH_TC 64                // most columns of a tile: one wavefront's lanes
#define RHH_MAX_BINS 1024
#define RHH_MAX_CELLS 4096       // nbx * nby of a pair
#define RHH_TALLIES 3            // under, over, nan: words nbins, nbins + 1, nbins + 2 of a column's histogram
#define RHH_LDS_BYTES (63 * 1024)   // the family's budget per workgroup
#define RHH_WS_CAP_BYTES (128ll << 20)
#define RHH_COL_BYTES(nbins) (8 * ((nbins) + 1) + 4 * ((nbins) + RHH_TALLIES))   // LDS of one column: edge table + histogram
#define RHH_PAIR_WORDS(nbx, nby) ((long long)(nbx) * (nby) + 1)                   // the grid and the rows outside it
#define RHH_PAIR_LDS(nbx, nby) (8 * ((nbx) + 1 + (nby) + 1) + 4 * RHH_PAIR_WORDS(nbx, nby))

#ifndef RH_HIST_HOST
#define RHH_FN static __device__ __forceinline__
#define RHH_SYNC() __syncthreads()
#define RHH_TID0 ((int)threadIdx.x)
#define RHH_TID1 ((int)threadIdx.x + 1)
#define RHH_LDS_ADD(p) ((void)atomicAdd((p), 1u))
#else
#define RHH_FN static inline
#define RHH_SYNC() ((void)0)
#define RHH_TID0 0
#define RHH_TID1 rhh_nthreads
#define RHH_LDS_ADD(p) ((void)(*(p) += 1u))
#endif
// every thread of the workgroup (device: this one; host: each in turn -- a phase ends where the device has its barrier)
#define RHH_EACH_THREAD(tid) for (int tid = RHH_TID0; tid < RHH_TID1; tid++)

// columns of a tile at nbins bins: the largest power of two, at most RHH_TC, whose LDS fits (64 up to 82 bins, 32 at 128, 16 at 257, 4 at 1024)
RHH_FN int rhh_tile_cols(const int nbins) {
  const int fit = RHH_LDS_BYTES / RHH_COL_BYTES(nbins);
  int c = 1;
  while (2 * c <= fit && 2 * c <= RHH_TC) c *= 2;
  return c;
}
RHH_FN int rhh_log2_up(const int n) {
  int l = 0;
  while ((1 << l) < n) l++;
  return l;
}
RHH_FN bool rhh_finite(const double x) { return __builtin_fabs(x) < __builtin_inf(); }

// Flat row r is kept iteration j of chain c: one division where a thread starts, then steps of a fixed number of rows.  The draw's
// offset in doubles from draws[0][first][0] is (c * iterations + j * thin) * nvars.
struct rhh_row { long long c, j; };
RHH_FN rhh_row rhh_row_of(const long long r, const long long kept) {
  rhh_row w;
  w.c = r / kept;
  w.j = r - w.c * kept;
  return w;
}
// step = sq * kept + sr, 0 <= sr < kept (the caller's, uniform): no loop and no branch for the lanes to diverge on
RHH_FN void rhh_row_step(rhh_row &w, const long long kept, const long long sq, const long long sr) {
  w.j += sr;
  const bool wrap = w.j >= kept;
  w.j -= wrap ? kept : 0;
  w.c += sq + (wrap ? 1 : 0);
}

// ---- automatic bounds ------------------------------------------------------------------------------------------------------------
// Columns [k0, k0 + RHH_TC) of the selection over split s.  base: draws[0][first][0].  lds: 2 * RHH_BLOCK doubles.  part [2][S][K].
RHH_FN void rhh_minmax_split(const double *base, const long long iterations, const long long nvars, const long long thin, const long long kept,
                             const long long N, const int *cols, const int K, const int k0, const long long s, const long long S, double *lds,
                             double *part, const int rhh_nthreads) {
  const long long r_lo = s * RHH_SPLIT, r_hi = N - r_lo < RHH_SPLIT ? N : r_lo + RHH_SPLIT;
  const int ncol = K - k0 < RHH_TC ? K - k0 : RHH_TC, lw = rhh_log2_up(ncol), step = RHH_BLOCK >> lw;
  const long long sq = step / kept, sr = step - sq * kept;
  RHH_EACH_THREAD(tid) {
    const int c = tid & ((1 << lw) - 1), g = tid >> lw;
    double mn = __builtin_inf(), mx = -__builtin_inf();
    if (c < ncol) {
      const int col = cols[k0 + c];
      rhh_row w = rhh_row_of(r_lo + g, kept);
      for (long long r = r_lo + g; r < r_hi; r += step) {
        const double x = base[(w.c * iterations + w.j * thin) * nvars + col];
        if (rhh_finite(x)) {
          mn = x < mn ? x : mn;
          mx = x > mx ? x : mx;
        }
        rhh_row_step(w, kept, sq, sr);
      }
    }
    lds[tid] = mn;
    lds[RHH_BLOCK + tid] = mx;
  }
  RHH_SYNC();
  RHH_EACH_THREAD(tid) {
    if (tid < ncol) {
      double mn = __builtin_inf(), mx = -__builtin_inf();
      for (int g = 0; g < step; g++) {
        const double a = lds[(g << lw) + tid], b = lds[RHH_BLOCK + (g << lw) + tid];
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
      }
      part[s * K + k0 + tid] = mn;
      part[(S + s) * K + k0 + tid] = mx;
    }
  }
}

// bounds [K][2]: (lo, hi) of column k over all splits; nothing finite: NaN, NaN; a -0.0 extreme leaves as +0.0
RHH_FN void rhh_minmax_finish(const double *part, const long long S, const int K, const int k, double *bounds) {
  double mn = __builtin_inf(), mx = -__builtin_inf();
  for (long long s = 0; s < S; s++) {
    const double a = part[s * K + k], b = part[(S + s) * K + k];
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  const bool none = mn > mx;
  bounds[2 * k] = none ? __builtin_nan("") : (mn == 0.0 ? 0.0 : mn);
  bounds[2 * k + 1] = none ? __builtin_nan("") : (mx == 0.0 ? 0.0 : mx);
}

// ---- binning ---------------------------------------------------------------------------------------------------------------------
// The word of a column's histogram that x counts in: its bin against e [nbins + 1], or nbins (under), nbins + 1 (over), nbins + 2
// (nan).  lo = e[0], hi = e[nbins], inv = nbins / (hi - lo) (0, inf or NaN at a width of inf or 0: the guess is then bin 0).
RHH_FN int rhh_word(const double x, const double *e, const int nbins, const double lo, const double hi, const double inv) {
  if (x != x) return nbins + 2;
  if (x < lo || (lo != lo && x < 0.0)) return nbins;
  if (x > hi || (hi != hi && x > 0.0)) return nbins + 1;
  const double t = (x - lo) * inv;
  int b = t >= 0.0 ? (t < (double)nbins ? (int)t : nbins - 1) : 0;
  while (b > 0 && x < e[b]) b--;
  while (b < nbins - 1 && x >= e[b + 1]) b++;
  return b;
}

// Columns [k0, k0 + cpt) of the selection over split s.  edges [K][nbins + 1] (global); ldsv: cpt * RHH_COL_BYTES(nbins) bytes;
// P [cpt][nbins + 3]: the split's partial histogram, zero for the columns past K.
RHH_FN void rhh_bin_split(const double *base, const long long iterations, const long long nvars, const long long thin, const long long kept,
                          const long long N, const int *cols, const int K, const int k0, const int cpt, const int nbins, const double *edges,
                          const long long s, void *ldsv, unsigned *P, const int rhh_nthreads) {
  const long long r_lo = s * RHH_SPLIT, r_hi = N - r_lo < RHH_SPLIT ? N : r_lo + RHH_SPLIT;
  const int ncol = K - k0 < cpt ? K - k0 : cpt, lw = rhh_log2_up(ncol), step = RHH_BLOCK >> lw, L = nbins + RHH_TALLIES;
  const long long sq = step / kept, sr = step - sq * kept;
  double *le = (double *)ldsv;
  unsigned *lh = (unsigned *)(le + cpt * (nbins + 1));
  RHH_EACH_THREAD(tid) {
    for (int i = tid; i < ncol * (nbins + 1); i += RHH_BLOCK) le[i] = edges[(long long)k0 * (nbins + 1) + i];
    for (int i = tid; i < cpt * L; i += RHH_BLOCK) lh[i] = 0u;
  }
  RHH_SYNC();
  RHH_EACH_THREAD(tid) {
    const int c = tid & ((1 << lw) - 1), g = tid >> lw;
    if (c < ncol) {
      const int col = cols[k0 + c];
      const double *e = le + c * (nbins + 1);
      const double lo = e[0], hi = e[nbins], inv = (double)nbins / (hi - lo);
      unsigned *h = lh + c * L;
      rhh_row w = rhh_row_of(r_lo + g, kept);
      for (long long r = r_lo + g; r < r_hi; r += step) {
        const double x = base[(w.c * iterations + w.j * thin) * nvars + col];
        RHH_LDS_ADD(h + rhh_word(x, e, nbins, lo, hi, inv));
        rhh_row_step(w, kept, sq, sr);
      }
    }
  }
  RHH_SYNC();
  RHH_EACH_THREAD(tid) {
    for (int i = tid; i < cpt * L; i += RHH_BLOCK) P[i] = lh[i];
  }
}

// Pair (ca, cb) over split s.  ex [nbx + 1], ey [nby + 1] (global); ldsv: RHH_PAIR_LDS(nbx, nby) bytes; P [nbx * nby + 1]: the
// grid [bx][by] and, last, the rows with a coordinate out of range or NaN.
RHH_FN void rhh_pair_split(const double *base, const long long iterations, const long long nvars, const long long thin, const long long kept,
                           const long long N, const int ca, const int cb, const int nbx, const int nby, const double *ex, const double *ey,
                           const long long s, void *ldsv, unsigned *P, const int rhh_nthreads) {
  const long long r_lo = s * RHH_SPLIT, r_hi = N - r_lo < RHH_SPLIT ? N : r_lo + RHH_SPLIT;
  const long long sq = RHH_BLOCK / kept, sr = RHH_BLOCK - sq * kept;
  const int cells = nbx * nby;
  double *lx = (double *)ldsv, *ly = lx + nbx + 1;
  unsigned *lh = (unsigned *)(ly + nby + 1);
  RHH_EACH_THREAD(tid) {
    for (int i = tid; i <= nbx; i += RHH_BLOCK) lx[i] = ex[i];
    for (int i = tid; i <= nby; i += RHH_BLOCK) ly[i] = ey[i];
    for (int i = tid; i <= cells; i += RHH_BLOCK) lh[i] = 0u;
  }
  RHH_SYNC();
  RHH_EACH_THREAD(tid) {
    const double xlo = lx[0], xhi = lx[nbx], xinv = (double)nbx / (xhi - xlo), ylo = ly[0], yhi = ly[nby], yinv = (double)nby / (yhi - ylo);
    rhh_row w = rhh_row_of(r_lo + tid, kept);
    for (long long r = r_lo + tid; r < r_hi; r += RHH_BLOCK) {
      const long long off = (w.c * iterations + w.j * thin) * nvars;
      const int bx = rhh_word(base[off + ca], lx, nbx, xlo, xhi, xinv), by = rhh_word(base[off + cb], ly, nby, ylo, yhi, yinv);
      RHH_LDS_ADD(lh + (bx < nbx && by < nby ? bx * nby + by : cells));
      rhh_row_step(w, kept, sq, sr);
    }
  }
  RHH_SYNC();
  RHH_EACH_THREAD(tid) {
    for (int i = tid; i <= cells; i += RHH_BLOCK) P[i] = lh[i];
  }
}

// word e of unit u (a tile's [cpt][nbins + 3], a pair's [nbx nby + 1]; L words) summed over its S partials: ws [unit][S][L]
RHH_FN unsigned long long rhh_finish_word(const unsigned *ws, const long long S, const long long L, const long long u, const long long e) {
  unsigned long long acc = 0;
  for (long long s = 0; s < S; s++) acc += ws[(u * S + s) * L + e];
  return acc;
}

#ifndef RH_HIST_HOST
// grid: S x ceil(K / RHH_TC), blockIdx.x = s * ctiles + column tile
extern "C" __global__ void __launch_bounds__(RHH_BLOCK)
rh_hist_minmax_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const long long first,
                      const long long thin, const long long kept, const long long N, const int *__restrict__ cols, const int K,
                      const int ctiles, const long long S, double *__restrict__ part) {
  __shared__ double lds[2 * RHH_BLOCK];
  const long long s = (long long)(blockIdx.x / (unsigned)ctiles);
  const int ct = (int)(blockIdx.x - (unsigned)s * (unsigned)ctiles);
  if (s >= S) return;
  rhh_minmax_split(draws + first * nvars, iterations, nvars, thin, kept, N, cols, K, ct * RHH_TC, s, S, lds, part, RHH_BLOCK);
}

// grid: ceil(K / RHH_BLOCK)
extern "C" __global__ void __launch_bounds__(RHH_BLOCK)
rh_hist_minmax_finish_kernel(const double *__restrict__ part, const long long S, const int K, double *__restrict__ bounds) {
  const int k = (int)(blockIdx.x * RHH_BLOCK + threadIdx.x);
  if (k < K) rhh_minmax_finish(part, S, K, k, bounds);
}

extern __shared__ double rhh_lds[];   // the launch's dynamic LDS: cpt * RHH_COL_BYTES(nbins), RHH_PAIR_LDS(nbx, nby)

// grid: the chunk's tiles [t_lo, t_lo + t_cnt) x S, blockIdx.x = (tile - t_lo) * S + s; ws [t_cnt][S][cpt][nbins + 3]
extern "C" __global__ void __launch_bounds__(RHH_BLOCK)
rh_hist_bin_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const long long first,
                   const long long thin, const long long kept, const long long N, const int *__restrict__ cols, const int K,
                   const int cpt, const int nbins, const double *__restrict__ edges, const long long t_lo, const int t_cnt,
                   const long long S, unsigned *__restrict__ ws) {
  const long long tl = (long long)blockIdx.x / S, s = (long long)blockIdx.x - tl * S;
  if (tl >= t_cnt) return;
  rhh_bin_split(draws + first * nvars, iterations, nvars, thin, kept, N, cols, K, (int)((t_lo + tl) * cpt), cpt, nbins, edges, s, rhh_lds,
                ws + (tl * S + s) * cpt * (nbins + RHH_TALLIES), RHH_BLOCK);
}

// grid: the chunk's pairs [p_lo, p_lo + p_cnt) x S, blockIdx.x = (pair - p_lo) * S + s; ws [p_cnt][S][nbx nby + 1]
extern "C" __global__ void __launch_bounds__(RHH_BLOCK)
rh_hist_pair_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const long long first,
                    const long long thin, const long long kept, const long long N, const int *__restrict__ pairs, const int nbx,
                    const int nby, const double *__restrict__ xedges, const double *__restrict__ yedges, const long long p_lo,
                    const int p_cnt, const long long S, unsigned *__restrict__ ws) {
  const long long pl = (long long)blockIdx.x / S, s = (long long)blockIdx.x - pl * S;
  if (pl >= p_cnt) return;
  const long long p = p_lo + pl;
  rhh_pair_split(draws + first * nvars, iterations, nvars, thin, kept, N, pairs[2 * p], pairs[2 * p + 1], nbx, nby, xedges + p * (nbx + 1),
                 yedges + p * (nby + 1), s, rhh_lds, ws + (pl * S + s) * RHH_PAIR_WORDS(nbx, nby), RHH_BLOCK);
}

// grid: ceil(u_cnt * L / RHH_BLOCK); out [units][L] of 64-bit counts, the chunk's units from u_lo
extern "C" __global__ void __launch_bounds__(RHH_BLOCK)
rh_hist_finish_kernel(const unsigned *__restrict__ ws, const long long S, const long long L, const long long u_lo, const long long u_cnt,
                      unsigned long long *__restrict__ out) {
  const long long i = (long long)blockIdx.x * RHH_BLOCK + threadIdx.x;
  if (i >= u_cnt * L) return;
  const long long u = i / L, e = i - u * L;
  out[(u_lo + u) * L + e] = rhh_finish_word(ws, S, L, u, e);
}
#endif
#endif
