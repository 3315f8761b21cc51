// rh_rank_plot.hip.h -- rank plots (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021, section 4.1) over device-resident draws: per
// chain, the histogram of the ranks its draws take among the pooled draws of all chains.  Which chain is off, and how: a slope, a cup,
// a cap.
//
// Model-independent: a translation unit of its own (no RH_NVARS, no generated code), compiled once per toolchain through the
// engine's build_source() and inspected like every other code object before it is launched.  wave64, gfx950.  Its text follows
// rh_summary.hip.h's in the translation unit: the pooled sort (rs_tile_sort, rs_merge_tile), the key order (rs_to_key: Double.compare's,
// -0.0 before +0.0) and the key type are that header's, unchanged.
//
// draws [chains][iterations][nvars]; analysed: the window [first, first + count) of every chain, unsplit, the selected columns.
// C = chains, n = count, S = C n values per column, flat index s = c n + i; B bins, 2 <= B <= RU_MAXBINS.
// For the value v of (c, i): L keys of the column below key(v), U at or below it, r2 = L + U + 1 (twice the average rank; ties share
// it), bin = ((r2 - 1) B) / (2 S) in 64-bit integers -- floor(u B) with u = (r - 1/2) / S, so 0 <= bin < B.  counts [column][c][bin].
//
//   rh_rank_plot_stage_kernel   the unsplit window of a tile of <= RU_TP selected columns x RU_ROWS flat values, through LDS: read with
//                               the lanes along the columns (neighbouring doubles of a draw's row), written with the lanes along s into
//                               the dense y [column][S].
//   rh_rank_plot_sort_kernel /  the summary's tile sort and merge pass over a dense column (one flat chain: nvars = 1, thin = 1,
//   rh_rank_plot_merge_kernel   kept = N = S), between two buffers of S keys per column.
//   rh_rank_plot_split_kernel   every stride-th key of the sorted column, stride = 1 << shift, packed into the spare key buffer: the
//                               count kernel's splitters, nsplit = ceil(S / stride) <= RU_MAXSPLIT of them, read from there in whole lines.
//   rh_rank_plot_count_kernel   one workgroup = one column x one chain x one segment of the chain's iterations, RU_BLOCK threads.  LDS,
//                               sized by the launch: the column's nsplit splitters (8 bytes each), then B count words.  A value's two
//                               searches run over the splitters in LDS first: sp splitters lie below the key, so L lies in
//                               ((sp - 1) stride, sp stride] -- one contiguous run of the sorted column, finished there in at most `shift`
//                               steps (none at stride 1).  The search for U starts from the first's answers: the splitters from sp on, and,
//                               where it ends in the same run, the run from L on.  The bin is one integer LDS add; after a barrier the
//                               table is added to the result, zeroed by the host, with integer atomics (segments of one chain meet
//                               there).  The workgroups of a column whose top key is the NaN's leave its counts zero; the first of them
//                               writes nan[column], the number of NaN keys, from one binary search of the column's top.
//
// Integers only: whatever the segments per chain, the chunking of the columns or the order of the workgroups, the same counts.
// Workspace per column: y and two key buffers of S 8-byte words each; the host walks the columns in chunks below RU_WS_CAP_BYTES and
// refuses a single column beyond it.
//
// The block routines are plain C++ over (thread id, LDS pointer): with RH_RANK_PLOT_HOST (and RH_SUMMARY_HOST) defined they compile
// with a host compiler, every "thread" of a phase run in turn (tests/test_rank_plot_device_cpu.py): same text, same integers.
#ifndef RH_RANK_PLOT_HIP_H
#define RH_RANK_PLOT_HIP_H
#ifndef RH_SUMMARY_HIP_H
#error "rh_rank_plot.hip.h follows rh_summary.hip.h in its translation unit"
#endif

#define RU_BLOCK 256            // threads of every kernel here (== RS_BLOCK: the sort's routines run in the same workgroups)
#define RU_MAXBINS 1024         // 4 KiB of count words
#define RU_MAXSPLIT 2048        // 16 KiB of splitters: with the counts at most 20 KiB, eight workgroups to a CU's 160 KiB
#define RU_TP 16                // columns of a stage tile
#define RU_ROWS 256             // flat values of a stage tile
#define RU_STAGE_STRIDE (RU_ROWS + 1)
#define RU_SEG_MIN 1024         // the fewest iterations of a segment where a chain is cut: four per thread against the splitters' load
#define RU_TARGET_WGS 2048      // workgroups the count launch aims at: eight to each of 256 CUs
#define RU_WS_CAP_BYTES (128ll << 20)
#define RU_LDS_BYTES(nsplit, bins) (8ll * (nsplit) + 4ll * (bins))

#ifndef RH_RANK_PLOT_HOST
#define RU_FN static __device__ __forceinline__
#define RU_SYNC() __syncthreads()
#define RU_TID0 ((int)threadIdx.x)
#define RU_TID1 ((int)threadIdx.x + 1)
#define RU_LDS_ADD(p) ((void)atomicAdd((p), 1u))
#define RU_OUT_ADD(p, v) ((void)atomicAdd((p), (v)))
#else
#define RU_FN static inline
#define RU_SYNC() ((void)0)
#define RU_TID0 0
#define RU_TID1 ru_nthreads
#define RU_LDS_ADD(p) ((void)(*(p) += 1u))
#define RU_OUT_ADD(p, v) ((void)(*(p) += (v)))
#endif
#define RU_EACH_THREAD(tid) for (int tid = RU_TID0; tid < RU_TID1; tid++)

// ---- the unsplit window, gathered --------------------------------------------------------------------------------------------------------
// A tile of tpw columns (cols[0 .. tpw): their parameters) x the flat values [s0, min(s0 + RU_ROWS, S)) -> y[p * S + s]; flat value s
// is draw first + s % n of chain s / n.  lds: RU_TP * RU_STAGE_STRIDE doubles.
RU_FN void ru_stage_tile(const double *draws, const long long iterations, const long long nvars, const long long first, const long long n,
                         const long long S, const int *cols, const int tpw, const long long s0, double *lds, double *y, const int ru_nthreads) {
  const int rows = (int)(S - s0 < RU_ROWS ? S - s0 : RU_ROWS), total = rows * tpw;
  RU_EACH_THREAD(tid) {
    for (int j = tid; j < total; j += RU_BLOCK) {
      const int r = j / tpw, p = j - r * tpw;
      const long long s = s0 + r, c = s / n, i = s - c * n;
      lds[p * RU_STAGE_STRIDE + r] = draws[(c * iterations + first + i) * nvars + cols[p]];
    }
  }
  RU_SYNC();
  RU_EACH_THREAD(tid) {
    for (int j = tid; j < total; j += RU_BLOCK) {
      const int p = j / rows, r = j - p * rows;
      y[(long long)p * S + s0 + r] = lds[p * RU_STAGE_STRIDE + r];
    }
  }
}

// ---- the two-level search ----------------------------------------------------------------------------------------------------------------
// how many of a[lo, hi) lie below k (or_equal: at or below), given that all of a[0, lo) do and none of a[hi, ..) does: lo + that count
RU_FN long long ru_bound(const rs_key *a, long long lo, long long hi, const rs_key k, const bool or_equal) {
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (or_equal ? a[mid] <= k : a[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// split [nsplit]: sorted[j << shift], j = 0 .. nsplit-1 (in LDS).  *L: the keys of sorted [S] below k, *U: those at or below it.
RU_FN void ru_rank(const rs_key *split, const int nsplit, const rs_key *sorted, const long long S, const int shift, const rs_key k,
                   long long *L, long long *U) {
  // sp splitters lie below k: sorted[(sp - 1) << shift] < k <= sorted[sp << shift] (where that one exists) -- the answer's run
  const long long sp = ru_bound(split, 0, nsplit, k, false);
  long long lo = 0;
  if (sp > 0) {
    const long long end = sp << shift;
    lo = ru_bound(sorted, ((sp - 1) << shift) + 1, end < S ? end : S, k, false);
  }
  *L = lo;
  // the splitters at or below k are those and the equal ones that follow; in the same run the search goes on from L
  const long long sq = ru_bound(split, sp, nsplit, k, true);
  long long up = 0;
  if (sq > 0) {
    const long long begin = ((sq - 1) << shift) + 1, end = sq << shift;
    up = ru_bound(sorted, begin > lo ? begin : lo, end < S ? end : S, k, true);
  }
  *U = up;
}
RU_FN int ru_bin(const long long L, const long long U, const long long S, const int bins) {
  return (int)((unsigned long long)(L + U) * (unsigned long long)bins / (unsigned long long)(2 * S));   // r2 - 1 = L + U
}

// ---- one column x one chain x one segment ------------------------------------------------------------------------------------------------
// sorted [S]: the column's keys; packed [nsplit]: its splitters; v [len]: the segment's values.  lds: RU_LDS_BYTES(nsplit, bins) bytes.
// out [bins]: the chain's counts, added to.  nan_out: NULL, or where the column's first workgroup leaves the number of NaN keys.
RU_FN void ru_count_block(const rs_key *sorted, const rs_key *packed, const long long S, const int nsplit, const int shift, const double *v,
                          const int len, const int bins, rs_key *lds, unsigned *out, unsigned *nan_out, const int ru_nthreads) {
  const bool has_nan = sorted[S - 1] == RS_KEY_NAN;   // a NaN sorts last
  if (nan_out) {
    RU_EACH_THREAD(tid) {
      if (tid == 0) *nan_out = has_nan ? (unsigned)(S - ru_bound(sorted, 0, S, RS_KEY_NAN, false)) : 0u;
    }
  }
  if (has_nan) return;
  rs_key *split = lds;
  unsigned *cnt = (unsigned *)(lds + nsplit);
  RU_EACH_THREAD(tid) {
    for (int j = tid; j < nsplit; j += RU_BLOCK) split[j] = packed[j];
    for (int b = tid; b < bins; b += RU_BLOCK) cnt[b] = 0u;
  }
  RU_SYNC();
  RU_EACH_THREAD(tid) {
    for (int i = tid; i < len; i += RU_BLOCK) {
      long long L, U;
      ru_rank(split, nsplit, sorted, S, shift, rs_to_key(v[i]), &L, &U);
      RU_LDS_ADD(cnt + ru_bin(L, U, S, bins));
    }
  }
  RU_SYNC();
  RU_EACH_THREAD(tid) {
    for (int b = tid; b < bins; b += RU_BLOCK)
      if (cnt[b]) RU_OUT_ADD(out + b, cnt[b]);
  }
}

#ifndef RH_RANK_PLOT_HOST
// The workspace holds, for the chunk's columns [k_lo, k_lo + p_cnt) of the selection, y [p_cnt][S] and two key buffers [p_cnt][S].
// grid: tiles of RU_ROWS flat values x tiles of RU_TP columns, blockIdx.x = row tile * ctiles + column tile
extern "C" __global__ void __launch_bounds__(RU_BLOCK)
rh_rank_plot_stage_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const long long first,
                          const long long n, const long long S, const int *__restrict__ cols, const int p_cnt, const int ctiles,
                          double *__restrict__ y) {
  __shared__ double lds[RU_TP * RU_STAGE_STRIDE];
  const long long rt = (long long)(blockIdx.x / (unsigned)ctiles);
  const int pl = (int)(blockIdx.x - (unsigned)rt * (unsigned)ctiles) * RU_TP;
  const long long s0 = rt * RU_ROWS;
  if (s0 >= S || pl >= p_cnt) return;
  ru_stage_tile(draws, iterations, nvars, first, n, S, cols + pl, p_cnt - pl < RU_TP ? p_cnt - pl : RU_TP, s0, lds, y + (long long)pl * S, RU_BLOCK);
}

// grid: tiles x p_cnt, blockIdx.x = tile * p_cnt + column: a dense column is one flat chain
extern "C" __global__ void __launch_bounds__(RU_BLOCK)
rh_rank_plot_sort_kernel(const double *__restrict__ y, const long long S, const int p_cnt, rs_key *__restrict__ keys) {
  __shared__ rs_key lds[RS_TILE_SLOTS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt), g0 = tile * RS_TILE;
  if (g0 >= S) return;
  rs_tile_sort(y + pl * S, S, 1, 1, S, S, g0, lds, keys + pl * S + g0, RU_BLOCK);
}

// one merge pass over runs of L keys, src -> dst ([p_cnt][S] each); grid: ceil(S / RS_MERGE_TILE) x p_cnt
extern "C" __global__ void __launch_bounds__(RU_BLOCK)
rh_rank_plot_merge_kernel(const rs_key *__restrict__ src, rs_key *__restrict__ dst, const long long S, const long long L, const int p_cnt) {
  __shared__ rs_key lds[RS_MERGE_LDS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt), o0 = tile * RS_MERGE_TILE;
  if (o0 >= S) return;
  rs_merge_tile(src + pl * S, dst + pl * S, S, L, o0, lds, RU_BLOCK);
}

// packed[column * S + j] = sorted[column * S + (j << shift)], j < nsplit; grid: ceil(nsplit / RU_BLOCK) x p_cnt, blockIdx.x = block * p_cnt + column
extern "C" __global__ void __launch_bounds__(RU_BLOCK)
rh_rank_plot_split_kernel(const rs_key *__restrict__ sorted, const long long S, const int nsplit, const int shift, const int p_cnt,
                          rs_key *__restrict__ packed) {
  const long long blk = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)blk * (unsigned)p_cnt), j = blk * RU_BLOCK + threadIdx.x;
  if (j < nsplit) packed[pl * S + j] = sorted[pl * S + (j << shift)];
}

extern __shared__ rs_key ru_lds[];   // the launch's dynamic LDS: RU_LDS_BYTES(nsplit, bins)
// grid: p_cnt x chains x segs, blockIdx.x = (column * chains + chain) * segs + segment; a segment is seg_len iterations (the last one
// of a chain the rest).  counts [K][chains][bins] and nan [K] are indexed by the column's place in the selection, k_lo + column.
extern "C" __global__ void __launch_bounds__(RU_BLOCK)
rh_rank_plot_count_kernel(const rs_key *__restrict__ sorted, const rs_key *__restrict__ packed, const double *__restrict__ y, const long long S,
                          const long long n, const int chains, const int segs, const long long seg_len, const int nsplit, const int shift,
                          const int bins, const int k_lo, unsigned *__restrict__ counts, unsigned *__restrict__ nan) {
  const unsigned per_col = (unsigned)chains * (unsigned)segs;
  const long long pl = (long long)(blockIdx.x / per_col);
  const unsigned rest = blockIdx.x - (unsigned)pl * per_col;
  const long long c = (long long)(rest / (unsigned)segs), g = (long long)(rest - (unsigned)c * (unsigned)segs);
  const long long i0 = g * seg_len;
  if (i0 >= n) return;
  const int len = (int)(n - i0 < seg_len ? n - i0 : seg_len);
  ru_count_block(sorted + pl * S, packed + pl * S, S, nsplit, shift, y + pl * S + c * n + i0, len, bins, ru_lds,
                 counts + ((k_lo + pl) * chains + c) * bins, rest == 0 ? nan + k_lo + pl : nullptr, RU_BLOCK);
}
#endif
#endif
