// rh_ppc.hip.h -- posterior predictive checks over device-resident replicated draws: every row of rep [chains][iterations][nin], one
// replicated data set, is reduced ALONG the row to a few test statistics T(y_rep) per segment of its selected columns (Gelman, Meng
// and Stern 1996; bayesplot's ppc_stat and ppc_stat_grouped), and T is counted against T(y) over the draws.  Every other call over
// device draws reduces down a column; this is the one that reduces over the observations.
//
// Model-independent: a translation unit of its own, behind rh_summary.hip.h (rs_to_key's order, RS_CE, RS_KEY_FILL).  wave64, gfx950.
//
// A check is data: stats [nstat] (kind, arg), cols [K] (columns of the row, duplicates allowed), seg_off [nseg + 1] (the runs of the
// selection).  Segment g of a draw is row[cols[seg_off[g] .. seg_off[g + 1])], n_g values; output T[r][g * nstat + k] for flat row
// r = c * kept + j, which is draw (c, first + j * thin): the window of rh_summary.hip.h, the layout every other call here reads.
//
//   rh_ppc_stat_kernel    one workgroup = one tile of `rows` flat rows.  The K selected values of every row are staged once into LDS
//                         (element e of the tile is row e / K, selection e % K: consecutive lanes on consecutive doubles where the
//                         selection is the row in order), row r at r * stride, stride odd so that lanes on neighbouring rows hit
//                         different banks.  An item is one (row, segment) of the tile; a team of `team` = pp_width(longest segment)
//                         lanes takes an item, 256 / team items at once, in passes.  Of a team the first w = pp_width(n_g) lanes work
//                         on segment g: lane t takes the values i = t, t + w, .. in ascending i, then the w partials go through a
//                         fixed binary tree in LDS.  pp_width(n) = clamp(2^ceil(log2 n) / 16, 1, 256) depends on n alone, so every
//                         sum has an order fixed by n_g: not by K, the other segments, the tile or the call.
//                           min, max     as keys (rs_to_key: -0.0 before +0.0); a NaN's key is the largest, so max says "holds a NaN"
//                           mean         sum v / n; where min == max (all keys equal) the value itself
//                           sd           sqrt(sum (v - mean)^2 / (n - 1)), second pass; all keys equal: 0; n == 1: NaN
//                           frac_le(c)   #{v <= c} / n, the count exact
//                           quantile     keys copied to a scratch of 2^ceil(log2 n_g) slots (RS_KEY_FILL beyond n_g), a bitonic network
//                                        of that size run by the team, the key at the index the host computed
//                         A segment that holds a NaN gives the canonical NaN in all its statistics; every NaN result (inf - inf) is
//                         made the canonical one, so host and device agree in its bits.
//   rh_ppc_count_kernel   over T [S][nout] against t_obs [nout]: n_gt = #{T > t_obs}, n_eq = #{T == t_obs}, n_bad = #{T is NaN}, plain
//                         double comparisons, 32-bit integer adds in LDS per workgroup, then one 64-bit integer add per non-zero counter.
// t_obs is the stat kernel's output on y as a one-row buffer: both sides of every comparison went through the same arithmetic.
// No floating-point atomics; nothing depends on the launch order.
//
// LDS (dynamic, at most PP_LDS_DOUBLES * 8 = 64 KiB): the stage, rows * stride <= PP_STAGE doubles, then a scratch that first holds
// the trees' partials (2 x 256) and the items' min, max and mean (3 x 256 / team), and last -- all of those written out -- the sort's keys.
//
// The block routines are plain C++ over (thread id, LDS pointer): with RH_PPC_HOST (and RH_SUMMARY_HOST) defined they compile with a
// host compiler, every "thread" of a phase run in turn (tests/test_ppc_device_cpu.py): same text, same summation order.
#ifndef RH_PPC_HIP_H
#define RH_PPC_HIP_H
#ifndef RH_SUMMARY_HIP_H
#error "rh_ppc.hip.h follows rh_summary.hip.h in its translation unit"
#endif
#if defined(RH_PPC_HOST) != defined(RH_SUMMARY_HOST)
#error "rh_ppc.hip.h is compiled the way rh_summary.hip.h is: both for the host or both for the device"
#endif

#define PP_BLOCK 256                 // threads of every kernel here
#define PP_STAGE 4096                // doubles of the stage: one RS_TILE; the cap of K
#define PP_LDS_DOUBLES 8192          // the stage and the scratch together: 64 KiB
#define PP_MAX_K PP_STAGE
#define PP_MAX_STATS 16
#define PP_MAX_OUT 4096
#define PP_COUNT_ELEMS 8192          // values of T per workgroup of the count kernel (about: whole rows)

enum { PP_MEAN = 0, PP_SD = 1, PP_MIN = 2, PP_MAX = 3, PP_QUANTILE = 4, PP_FRAC_LE = 5, PP_NKINDS = 6 };
#define PP_F_MEAN 1                  // flags of a table: a mean is needed (MEAN or SD), a second pass, a sort
#define PP_F_SD 2
#define PP_F_SORT 4
typedef struct pp_stat { int kind; int reserved; double arg; } pp_stat;

#ifndef RH_PPC_HOST
#define PP_FN static __device__ __forceinline__
#define PP_SYNC() __syncthreads()
#define PP_TID0 ((int)threadIdx.x)
#define PP_TID1 ((int)threadIdx.x + 1)
#define PP_COUNT(p) atomicAdd((p), 1u)
#define PP_COUNT64(p, v) atomicAdd((p), (unsigned long long)(v))
#else
#define PP_FN static inline
#define PP_SYNC() ((void)0)
#define PP_TID0 0
#define PP_TID1 pp_nthreads
#define PP_COUNT(p) (*(p) += 1u)
#define PP_COUNT64(p, v) (*(p) += (unsigned long long)(v))
#endif
#define PP_EACH_THREAD(tid) for (int tid = PP_TID0; tid < PP_TID1; tid++)

// the smallest power of two that is not below n (n >= 1)
PP_FN int pp_pow2(const int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}
// lanes that work on a segment of n values
PP_FN int pp_width(const int n) {
  const int w = pp_pow2(n) / 16;
  return w < 1 ? 1 : w > PP_BLOCK ? PP_BLOCK : w;
}
// doubles between two staged rows of K values: odd, unless one row alone fills the stage
PP_FN int pp_stride(const int K) { return (K & 1) || K >= PP_STAGE ? K : K + 1; }
// slots between the sort scratches of two items: one pad where all of them still fit half the LDS
PP_FN int pp_sort_stride(const int conc, const int sortp) { return conc > 1 && conc * (sortp + 1) <= PP_LDS_DOUBLES - PP_STAGE ? sortp + 1 : sortp; }
// every NaN made the positive quiet one, on the bits (rs_to_key's test): a floating-point select "x != x ? nan : x" may be folded to x,
// and inf - inf has the sign bit set on some hardware and not on other
PP_FN double pp_canon(const double x) { return rs_from_key(rs_to_key(x)); }

// what thread tid does in pass `pass`: item = pass * conc + tid / team = row * nseg + segment
struct pp_item {
  bool on;              // the item exists in this tile
  int slot, t, w;       // the team's place among the conc at work; the lane in it; the lanes that work on this segment
  int r, g, n;          // row of the tile, segment, its length
  const double *v;      // the segment's staged values
};
PP_FN pp_item pp_item_of(const int tid, const int pass, const int team_log2, const int nitems, const int nseg, const int *seg_off, const double *stage,
                         const int stride) {
  pp_item it;
  it.slot = tid >> team_log2;
  it.t = tid - (it.slot << team_log2);
  const int item = pass * (PP_BLOCK >> team_log2) + it.slot;
  it.on = item < nitems;
  it.r = it.on ? item / nseg : 0;
  it.g = it.on ? item - it.r * nseg : 0;
  const int o0 = seg_off[it.g];
  it.n = seg_off[it.g + 1] - o0;
  it.w = pp_width(it.n);
  it.v = stage + it.r * stride + o0;
  return it;
}

// The partials p [tid] of every team's first w lanes into the team's first slot, as a fixed binary tree over w; KIND 0: doubles
// added, 1: the smaller key, 2: the larger key.  Ends behind a barrier.
#define PP_TREE(p, KIND)                                                                                             \
  for (int s_ = team >> 1; s_ >= 1; s_ >>= 1) {                                                                      \
    PP_SYNC();                                                                                                       \
    PP_EACH_THREAD(tid) {                                                                                            \
      const pp_item it = pp_item_of(tid, pass, team_log2, nitems, nseg, seg_off, stage, stride);                     \
      if (it.on && it.t < s_ && it.t + s_ < it.w) {                                                                  \
        if (KIND == 0) ((double *)(p))[tid] += ((double *)(p))[tid + s_];                                            \
        else if (KIND == 1) { if ((p)[tid + s_] < (p)[tid]) (p)[tid] = (p)[tid + s_]; }                              \
        else { if ((p)[tid + s_] > (p)[tid]) (p)[tid] = (p)[tid + s_]; }                                             \
      }                                                                                                              \
    }                                                                                                                \
  }                                                                                                                  \
  PP_SYNC();

// One tile: the flat rows [r0, r0 + nrows) of in [..][iterations][nin] (in: at [chain 0][iteration `first`][column 0]); flat row r is
// source row (r / kept) * iterations + (r % kept) * thin.  cols [K], seg_off [nseg + 1], stats [nstat], qidx [nseg * nstat] (the order
// statistic of every (segment, QUANTILE), anything elsewhere), flags PP_F_*, team = 1 << team_log2 = pp_width(the longest segment),
// sortp = pp_pow2(the longest segment) where a sort is asked for.  lds: nrows * stride + the scratch.  out [..][nseg * nstat].
PP_FN void pp_tile_block(const double *in, const long long iterations, const long long nin, const long long thin, const long long kept,
                         const long long r0, const int nrows, const int *cols, const int K, const int *seg_off, const int nseg, const pp_stat *stats,
                         const int nstat, const int *qidx, const int flags, const int stride, const int team_log2, const int sortp, rs_key *lds,
                         double *out, const int pp_nthreads) {
  const int team = 1 << team_log2, conc = PP_BLOCK >> team_log2, nitems = nrows * nseg, nout = nseg * nstat;
  double *stage = (double *)lds;
  rs_key *scr = lds + nrows * stride, *pa = scr, *pb = scr + PP_BLOCK, *rmin = scr + 2 * PP_BLOCK, *rmax = rmin + conc;
  double *rmean = (double *)(rmax + conc);
  const int sstride = pp_sort_stride(conc, sortp);
  const double nan = rs_from_key(RS_KEY_NAN);
  // the stage: every selected value once
  PP_EACH_THREAD(tid) {
    for (int e = tid; e < nrows * K; e += PP_BLOCK) {
      const int r = e / K, k = e - r * K;
      const long long fr = r0 + r, c = fr / kept, j = fr - c * kept;
      stage[r * stride + k] = in[(c * iterations + j * thin) * nin + cols[k]];
    }
  }
  PP_SYNC();
  for (int pass = 0; pass * conc < nitems; pass++) {
    // min and max, as keys
    PP_EACH_THREAD(tid) {
      const pp_item it = pp_item_of(tid, pass, team_log2, nitems, nseg, seg_off, stage, stride);
      if (it.on && it.t < it.w) {
        rs_key lo = RS_KEY_FILL, hi = 0;
        for (int i = it.t; i < it.n; i += it.w) {
          const rs_key key = rs_to_key(it.v[i]);
          lo = key < lo ? key : lo;
          hi = key > hi ? key : hi;
        }
        pa[tid] = lo;
        pb[tid] = hi;
      }
    }
    PP_TREE(pa, 1)
    PP_TREE(pb, 2)
    PP_EACH_THREAD(tid) {
      const pp_item it = pp_item_of(tid, pass, team_log2, nitems, nseg, seg_off, stage, stride);
      if (it.on && it.t == 0) {
        const rs_key lo = pa[tid], hi = pb[tid];
        rmin[it.slot] = lo;
        rmax[it.slot] = hi;
        double *o = out + (r0 + it.r) * nout + it.g * nstat;
        for (int k = 0; k < nstat; k++) {
          if (stats[k].kind == PP_MIN) o[k] = hi == RS_KEY_NAN ? nan : rs_from_key(lo);
          if (stats[k].kind == PP_MAX) o[k] = hi == RS_KEY_NAN ? nan : rs_from_key(hi);
        }
      }
    }
    if (flags & PP_F_MEAN) {
      PP_SYNC();
      PP_EACH_THREAD(tid) {
        const pp_item it = pp_item_of(tid, pass, team_log2, nitems, nseg, seg_off, stage, stride);
        if (it.on && it.t < it.w) {
          double acc = 0.0;
          for (int i = it.t; i < it.n; i += it.w) acc += it.v[i];
          ((double *)pa)[tid] = acc;
        }
      }
      PP_TREE(pa, 0)
      PP_EACH_THREAD(tid) {
        const pp_item it = pp_item_of(tid, pass, team_log2, nitems, nseg, seg_off, stage, stride);
        if (it.on && it.t == 0) {
          const rs_key lo = rmin[it.slot], hi = rmax[it.slot];
          const double mean = lo == hi ? rs_from_key(lo) : ((double *)pa)[tid] / (double)it.n;
          rmean[it.slot] = mean;
          double *o = out + (r0 + it.r) * nout + it.g * nstat;
          for (int k = 0; k < nstat; k++)
            if (stats[k].kind == PP_MEAN) o[k] = hi == RS_KEY_NAN ? nan : pp_canon(mean);
        }
      }
    }
    if (flags & PP_F_SD) {
      PP_SYNC();
      PP_EACH_THREAD(tid) {
        const pp_item it = pp_item_of(tid, pass, team_log2, nitems, nseg, seg_off, stage, stride);
        if (it.on && it.t < it.w) {
          const double mean = rmean[it.slot];
          double acc = 0.0;
          for (int i = it.t; i < it.n; i += it.w) {
            const double d = it.v[i] - mean;
            acc += d * d;
          }
          ((double *)pa)[tid] = acc;
        }
      }
      PP_TREE(pa, 0)
      PP_EACH_THREAD(tid) {
        const pp_item it = pp_item_of(tid, pass, team_log2, nitems, nseg, seg_off, stage, stride);
        if (it.on && it.t == 0) {
          const rs_key lo = rmin[it.slot], hi = rmax[it.slot];
          const double sd = hi == RS_KEY_NAN || it.n == 1 ? nan : lo == hi ? 0.0 : pp_canon(__builtin_sqrt(((double *)pa)[tid] / (double)(it.n - 1)));
          double *o = out + (r0 + it.r) * nout + it.g * nstat;
          for (int k = 0; k < nstat; k++)
            if (stats[k].kind == PP_SD) o[k] = sd;
        }
      }
    }
    for (int k = 0; k < nstat; k++) {
      if (stats[k].kind != PP_FRAC_LE) continue;
      const double c = stats[k].arg;
      PP_SYNC();
      PP_EACH_THREAD(tid) {
        const pp_item it = pp_item_of(tid, pass, team_log2, nitems, nseg, seg_off, stage, stride);
        if (it.on && it.t < it.w) {
          double acc = 0.0;                                         // a count: exact in any order
          for (int i = it.t; i < it.n; i += it.w) acc += it.v[i] <= c ? 1.0 : 0.0;
          ((double *)pa)[tid] = acc;
        }
      }
      PP_TREE(pa, 0)
      PP_EACH_THREAD(tid) {
        const pp_item it = pp_item_of(tid, pass, team_log2, nitems, nseg, seg_off, stage, stride);
        if (it.on && it.t == 0) out[(r0 + it.r) * nout + it.g * nstat + k] = rmax[it.slot] == RS_KEY_NAN ? nan : ((double *)pa)[tid] / (double)it.n;
      }
    }
    if (flags & PP_F_SORT) {
      PP_SYNC();                                                    // the scratch changes hands: partials, min, max and mean are all written out
      PP_EACH_THREAD(tid) {
        const pp_item it = pp_item_of(tid, pass, team_log2, nitems, nseg, seg_off, stage, stride);
        if (it.on) {
          rs_key *s = scr + it.slot * sstride;
          const int P = pp_pow2(it.n);
          for (int i = it.t; i < P; i += team) s[i] = i < it.n ? rs_to_key(it.v[i]) : RS_KEY_FILL;
        }
      }
      PP_SYNC();
      for (int kk = 2; kk <= sortp; kk <<= 1) {
        for (int j = kk >> 1; j >= 1; j >>= 1) {
          PP_EACH_THREAD(tid) {
            const pp_item it = pp_item_of(tid, pass, team_log2, nitems, nseg, seg_off, stage, stride);
            const int P = pp_pow2(it.n);
            if (it.on && kk <= P) {
              rs_key *s = scr + it.slot * sstride;
              for (int i = it.t; i < P / 2; i += team) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
                const bool up = (lo & kk) == 0;
                rs_key a = s[lo], b = s[hi];
                RS_CE(a, b, up);
                s[lo] = a;
                s[hi] = b;
              }
            }
          }
          PP_SYNC();
        }
      }
      PP_EACH_THREAD(tid) {
        const pp_item it = pp_item_of(tid, pass, team_log2, nitems, nseg, seg_off, stage, stride);
        if (it.on && it.t == 0) {
          const rs_key *s = scr + it.slot * sstride;
          const bool has_nan = s[it.n - 1] == RS_KEY_NAN;           // a NaN sorts last of the values
          double *o = out + (r0 + it.r) * nout + it.g * nstat;
          for (int k = 0; k < nstat; k++)
            if (stats[k].kind == PP_QUANTILE) o[k] = has_nan ? nan : rs_from_key(s[qidx[it.g * nstat + k]]);
        }
      }
    }
    PP_SYNC();                                                      // the next pass writes the scratch again
  }
}

// T [..][nout]: the rows [r0, r1) counted against tobs [nout] into counts [3][nout] (n_gt, n_eq, n_bad).  lds: 3 * nout 32-bit counters.
PP_FN void pp_count_block(const double *T, const long long r0, const long long r1, const int nout, const double *tobs, unsigned int *lds,
                          unsigned long long *counts, const int pp_nthreads) {
  PP_EACH_THREAD(tid) {
    for (int o = tid; o < 3 * nout; o += PP_BLOCK) lds[o] = 0u;
  }
  PP_SYNC();
  const long long ne = (r1 - r0) * nout;
  PP_EACH_THREAD(tid) {
    for (long long e = tid; e < ne; e += PP_BLOCK) {
      const int o = (int)(e % nout);
      const double x = T[r0 * nout + e], y = tobs[o];
      if (x != x) PP_COUNT(&lds[2 * nout + o]);
      else if (x > y) PP_COUNT(&lds[o]);
      else if (x == y) PP_COUNT(&lds[nout + o]);
    }
  }
  PP_SYNC();
  PP_EACH_THREAD(tid) {
    for (int o = tid; o < 3 * nout; o += PP_BLOCK)
      if (lds[o]) PP_COUNT64(&counts[o], lds[o]);
  }
}

#ifndef RH_PPC_HOST
// grid: the tiles of `rows` flat rows; dynamic LDS: the plan's (rows * stride doubles and the scratch)
extern "C" __global__ void __launch_bounds__(PP_BLOCK)
rh_ppc_stat_kernel(const double *__restrict__ in, const long long iterations, const long long nin, const long long first, const long long thin,
                   const long long kept, const long long S, const int *__restrict__ cols, const int K, const int *__restrict__ seg_off, const int nseg,
                   const pp_stat *__restrict__ stats, const int nstat, const int *__restrict__ qidx, const int flags, const int rows, const int stride,
                   const int team_log2, const int sortp, double *__restrict__ out) {
  extern __shared__ rs_key pp_lds[];
  const long long r0 = (long long)blockIdx.x * rows;
  if (r0 >= S) return;
  const int nrows = (int)(S - r0 < rows ? S - r0 : rows);
  pp_tile_block(in + first * nin, iterations, nin, thin, kept, r0, nrows, cols, K, seg_off, nseg, stats, nstat, qidx, flags, stride, team_log2, sortp, pp_lds,
                out, PP_BLOCK);
}

// grid: ceil(S / rpb) workgroups of rpb rows; dynamic LDS: 3 * nout * 4 bytes; counts zeroed before the launch
extern "C" __global__ void __launch_bounds__(PP_BLOCK)
rh_ppc_count_kernel(const double *__restrict__ T, const long long S, const int nout, const double *__restrict__ tobs, const long long rpb,
                    unsigned long long *__restrict__ counts) {
  extern __shared__ rs_key pp_lds[];
  const long long r0 = (long long)blockIdx.x * rpb;
  if (r0 >= S) return;
  pp_count_block(T, r0, S - r0 < rpb ? S : r0 + rpb, nout, tobs, (unsigned int *)pp_lds, counts, PP_BLOCK);
}
#endif
#endif
