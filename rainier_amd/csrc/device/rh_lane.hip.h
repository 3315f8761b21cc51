// rh_lane.hip.h -- hand-written gfx950 device library, part 3: the lane walk of the gradient row loop.
//
// ---- the lane walk: chains in the lanes, row values in scalar registers ------------------------------------------------------------
// rh_grad_kernel with the parallelisation turned round.  This file follows rh_engine.hip.h in the translation unit of the lane walk's
// code object only (engine.cpp build_lane_code: the model's own source + this), for models whose row code fits it; the engine
// decides per sampler which walk runs (lanes_plan.hpp walk_is_lane).
//   A lane holds the parameter vectors, invariants() and sums of RH_LANE_C chains -- lane l of chain group g serves the slots
// g * 64 C + k * 64 + l, k < C -- and the row values are wave-uniform: they come in through constant-address-space pointers (scalar
// loads, RH_LANE_R rows of every column per request) and enter row() as scalar operands.  No tile in vector registers, no lane masks (the ragged end is a scalar loop over single rows), no wave reduction.
// One scalar request feeds 9 C vector instructions of cfg 2's row: with C = 1 the scalar data cache is what binds (2.7 B/cycle/CU
// delivered, whether the lines hit or miss), with C = 2 the fp64 pipe is again (profiles/lane_walk_cfg2).
//   A workgroup is RH_LANE_W wavefronts that share one chain group and one row split: the split -- whole blocks of R rows,
// ceil(blocks / nsplit) blocks per split -- is cut into W contiguous pieces of ceil(blocks_per_split / W) blocks, wavefront w walks
// piece w.  SUMMATION ORDER of a chain's sum over a split: every wavefront adds its piece's rows in ascending row order into one
// accumulator set; the W wavefronts' sums go through LDS and are added in ascending w; one store per (split, chain, sum) into the
// partial-sum layout of rh_grad_kernel.  A chain's bits depend on nsplit, W and R only -- not on the live count, the slot, the lane,
// the other chains or the shards.  Only loads are scalar; every store is a vector store.
//
// ---- the two feeds -----------------------------------------------------------------------------------------------------------------
// The COLUMN feed (rh_grad_lane_kernel) reads the model's columns as they are: a request is R rows of ONE column, so every column's
// request must have arrived before the first row can start, and the R x NC values fill the 64 scalar registers there are for them --
// a wavefront has nothing in flight while it computes, and only its SIMD's other wavefronts hide its requests' latency.
// The ROW feed (this file compiled with RH_LANE_FEED_ROWS 1: rh_grad_lane_kernel of a code object of its own, engine.cpp
// build_lane_rows_code) reads an interleaved copy of a target's columns -- element (r, j) at r NC + j, zeros up to a whole block of 8
// rows, made once per model and device by the engine (ensure_lane_rows; lanes_plan.hpp lane_rows_*), its address a launch argument
// (struct rh_lane_rows), rh_model_data untouched.  A 64-byte request is then whole rows; a SET is min(R, 16 / NC) rows = at most two
// requests = 32 scalar registers, and there are two sets: while the pipe works on one, the other is on its way (wait for this set,
// request the next, the rows of this set, swap).  For targets of 1, 2, 4 or 8 columns; any other target of the model walks its columns
// as above.  Same grid, same split / piece arithmetic in blocks of R rows, same LDS reduction and stores, and the same rows in the same
// order through the same rh_row into one accumulator set per chain: a chain's sums are the column feed's BIT FOR BIT
// (tests/test_gpu_lane_feed.py), and SUMMATION ORDER above holds for both.  Measured on cfg 2: profiles/lane_feed_cfg2.
#if RH_NROWTARGETS > 0 && !RH_HAS_GATHER && !RH_BIGTH && !RH_BIGN && !RH_LK_LDS
#ifndef RH_LANE_W
#define RH_LANE_W 8
#endif
#ifndef RH_LANE_R
#define RH_LANE_R 8
#endif
#ifndef RH_LANE_C
#define RH_LANE_C 2
#endif
#ifndef RH_LANE_FEED_ROWS
#define RH_LANE_FEED_ROWS 0
#endif
typedef const double __attribute__((address_space(4))) *rh_ccol_t;
struct rh_lane_rows { const double *p[RH_NROWTARGETS]; };   // the interleaved copy of every row target (ROWT order; nullptr: none)
// does a target of NC columns take its rows from the interleaved copy (lanes_plan.hpp lane_rows_eligible), and in sets of how many
constexpr bool rh_lane_rowfed(int nc) { return RH_LANE_FEED_ROWS && (nc == 1 || nc == 2 || nc == 4 || nc == 8); }
constexpr int rh_lane_set(int nc) { return 16 / nc < RH_LANE_R ? 16 / nc : RH_LANE_R; }
// one set of S rows x NC columns, 64 or 128 bytes in whole aligned lines, from the interleaved copy into scalar registers
template <int S, int NC> RH_DEV void rh_lane_request(double (&c)[S][NC], rh_ccol_t rp, const long long row) {
#pragma unroll
  for (int u = 0; u < S; u++)
#pragma unroll
    for (int j = 0; j < NC; j++) c[u][j] = rp[(row + u) * NC + j];
}
// "wait for this set": an empty statement that reads the set's registers, so that the wait for its requests stands HERE -- ahead of the
// next set's requests (scalar loads return out of order: a wait further down would be for both sets)
template <int S, int NC> RH_DEV void rh_lane_arrived(const double (&c)[S][NC]) {
#pragma unroll
  for (int u = 0; u < S; u++)
#pragma unroll
    for (int j = 0; j < NC; j++) asm volatile("" ::"s"(c[u][j]));
}
template <int T, bool NV>   // NV: the log-density is needed (row()); otherwise row_g()
RH_DEV void rh_lane_targets(const double (&th)[RH_LANE_C][RH_NTH], const rh_model_data &d, const rh_lane_rows *rows, const int w, const int split, const int nsplit,
                            const int *__restrict__ lp, const int nvalid, const int chains, double *__restrict__ partial,
                            double *red, int &err) {
  if constexpr (T < RH_NTARGETS) {
    typedef rh_target<T> TG;
    if constexpr (TG::HAS_ROWS) {
      constexpr int NC = TG::NCOLS, R = RH_LANE_R, C = RH_LANE_C, W = RH_LANE_W;
      constexpr int NA = TG::NACC > 0 ? TG::NACC : 1;
      const int lane = threadIdx.x & 63;
      double inv[C][TG::NINV > 0 ? TG::NINV : 1];
#pragma unroll
      for (int k = 0; k < C; k++) TG::invariants(th[k], inv[k], err);
      const long long n = d.nrows[T];
      const long long blocks = (n + R - 1) / R, per = (blocks + nsplit - 1) / nsplit, perw = (per + W - 1) / W;
      long long s0 = (long long)split * per * R, s1 = s0 + per * R;
      if (s0 > n) s0 = n;
      if (s1 > n) s1 = n;
      long long r0 = s0 + (long long)w * perw * R, r1 = r0 + perw * R;   // wavefront w's piece (empty where the split ran out)
      if (r0 > s1) r0 = s1;
      if (r1 > s1) r1 = s1;
      rh_ccol_t cp[NC];
#pragma unroll
      for (int j = 0; j < NC; j++) cp[j] = (rh_ccol_t)d.cols[TG::COL0 + j];
      double acc[C][NA];
#pragma unroll
      for (int k = 0; k < C; k++)
#pragma unroll
        for (int o = 0; o < NA; o++) acc[k][o] = 0.0;
      long long kb = r0;   // wave-uniform: the loops branch on scalars, the row code runs with all lanes active
      if constexpr (rh_lane_rowfed(NC)) {
        // THE ROW FEED: sets of S whole rows from the interleaved copy, two register sets; a set is requested one compute phase ahead
        // (wait for A, request B, rows of A; wait for B, request A, rows of B).  The sets go in pairs, so that every request is used
        // further down the same path and stays where it is written; an odd last set has been requested by the pair before it, and a
        // request with no set behind it asks for the piece's last set again (a hit, never past the copy) and is dropped.  Same rows,
        // same order, same rh_row as the column feed.
        constexpr int S = rh_lane_set(NC);
        static_assert(R % S == 0 && S * NC * 2 * 2 <= 64, "two sets of whole rows in 64 scalar registers, a block of R rows in whole sets");
        const rh_ccol_t rp = (rh_ccol_t)rows->p[TG::ROWT];
        const int nsets = (int)((r1 - kb) / S);
        const long long last = kb + (long long)(nsets > 0 ? nsets - 1 : 0) * S;
        auto rows_of = [&](const double (&cur)[S][NC]) {
#pragma unroll
          for (int u = 0; u < S; u++)
#pragma unroll
            for (int k = 0; k < C; k++) rh_row<TG, NV>(th[k], inv[k], cur[u], acc[k], err);
        };
        double ca[S][NC], cb[S][NC];
        if (nsets > 0) rh_lane_request<S, NC>(ca, rp, kb);
        for (int i = 0; i + 2 <= nsets; i += 2) {
          rh_lane_arrived<S, NC>(ca);
          rh_lane_request<S, NC>(cb, rp, kb + S);
          __builtin_amdgcn_sched_barrier(0);   // (the requests stay ahead of the arithmetic)
          rows_of(ca);
          rh_lane_arrived<S, NC>(cb);
          rh_lane_request<S, NC>(ca, rp, kb + 2 * S <= last ? kb + 2 * S : last);
          __builtin_amdgcn_sched_barrier(0);
          rows_of(cb);
          kb += 2 * S;
        }
        if (nsets & 1) { rows_of(ca); kb += S; }
        for (; kb < r1; kb++) {   // the ragged end of the last split: single rows, one request each
          double c[1][NC];
          rh_lane_request<1, NC>(c, rp, kb);
#pragma unroll
          for (int k = 0; k < C; k++) rh_row<TG, NV>(th[k], inv[k], c[0], acc[k], err);
        }
      } else {
      for (; kb + R <= r1; kb += R) {
        double c[R][NC];
#pragma unroll
        for (int u = 0; u < R; u++)
#pragma unroll
          for (int j = 0; j < NC; j++) c[u][j] = cp[j][kb + u];
#pragma unroll
        for (int u = 0; u < R; u++)
#pragma unroll
          for (int k = 0; k < C; k++) rh_row<TG, NV>(th[k], inv[k], c[u], acc[k], err);
      }
      for (; kb < r1; kb++) {   // the ragged end of the last split: single rows, still scalar
        double c[NC];
#pragma unroll
        for (int j = 0; j < NC; j++) c[j] = cp[j][kb];
#pragma unroll
        for (int k = 0; k < C; k++) rh_row<TG, NV>(th[k], inv[k], c, acc[k], err);
      }
      }
#pragma unroll
      for (int k = 0; k < C; k++)
#pragma unroll
        for (int o = 0; o < NA; o++) red[((w * C + k) * NA + o) * 64 + lane] = acc[k][o];
      __syncthreads();
      // the (chain, sum) pairs of the group spread over the workgroup's threads; a pair's W values are added in ascending w
      for (int t = threadIdx.x; t < C * NA * 64; t += 64 * W) {
        const int ko = t >> 6, l = t & 63, k = ko / NA, o = ko - k * NA;
        double s = red[ko * 64 + l];
#pragma unroll
        for (int ww = 1; ww < W; ww++) s += red[(ww * C * NA + ko) * 64 + l];
        const int slot = k * 64 + l;
        if (slot < nvalid) partial[(((size_t)TG::ROWT * nsplit + split) * chains + lp[slot]) * RH_NACC_MAX + o] = s;
      }
      __syncthreads();   // (the next row target's sums go through the same buffer)
    }
    rh_lane_targets<T + 1, NV>(th, d, rows, w, split, nsplit, lp, nvalid, chains, partial, red, err);
  }
}
// grid: ngroups * nsplit workgroups of W wavefronts, ngroups = ceil(chains / (64 C)); the XCD mapping of rh_grad_kernel
RH_DEV void rh_grad_lane_body(const rh_model_data &d, const rh_lane_rows *rows, const double *__restrict__ q, const int *__restrict__ list,
                              const int *__restrict__ nlive, const int *__restrict__ vflag, double *__restrict__ partial, int *__restrict__ err_out,
                              int *__restrict__ n_running, const int chains, const int nsplit, const int xcd_aware, double *red) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int b = blockIdx.x;
  if (b == 0 && threadIdx.x == 0) *n_running = 0; // re-armed for the tick kernel that follows in stream order
  const int nl = rh_live_count(nlive, chains);
  int split, group;
  rh_grad_map(b, nsplit, xcd_aware, split, group);
  const int slot0 = group * (64 * RH_LANE_C);
  if (slot0 >= nl) return;   // (no live chain for this workgroup: all of its wavefronts leave)
  double th[RH_LANE_C][RH_NTH];
  bool gonly = rh_any_value_only<0>::v && vflag != nullptr;   // every chain of the group asked for the gradient only
#pragma unroll
  for (int k = 0; k < RH_LANE_C; k++) {
    const int c = rh_live_chain(list, slot0 + k * 64 + lane, nl);   // (a slot past the live count: the last live chain, its sums are dropped)
    if constexpr (rh_any_value_only<0>::v) gonly = gonly && vflag[c] == 2;
#pragma unroll
    for (int i = 0; i < RH_NVARS; i++) th[k][i] = q[(size_t)c * RH_NVARS + i];
  }
  int err = 0;
  if constexpr (rh_any_value_only<0>::v) {
    if (__all(gonly)) rh_lane_targets<0, false>(th, d, rows, w, split, nsplit, list + slot0, nl - slot0, chains, partial, red, err);
    else rh_lane_targets<0, true>(th, d, rows, w, split, nsplit, list + slot0, nl - slot0, chains, partial, red, err);
  } else
  rh_lane_targets<0, true>(th, d, rows, w, split, nsplit, list + slot0, nl - slot0, chains, partial, red, err);
  if (__any(err != 0) && lane == 0) atomicOr(err_out, 1);
}
#if !RH_LANE_FEED_ROWS
extern "C" __global__ void __launch_bounds__(64 * RH_LANE_W)
rh_grad_lane_kernel(const rh_model_data d, const double *__restrict__ q, const int *__restrict__ list, const int *__restrict__ nlive,
                    const int *__restrict__ vflag, double *__restrict__ partial, int *__restrict__ err_out, int *__restrict__ n_running,
                    const int chains, const int nsplit, const int xcd_aware) {
  __shared__ double red[RH_LANE_W * RH_LANE_C * RH_NACC_MAX * 64];
  rh_grad_lane_body(d, nullptr, q, list, nlive, vflag, partial, err_out, n_running, chains, nsplit, xcd_aware, red);
}
#else
// the same launch with the rows fed from the interleaved copies: a code object of its own (engine.cpp build_lane_rows_code) and the
// same name in it -- a sampler's timing names rh_grad_lane_kernel whichever feed its launches take (rh_sampler_lane_feed says which)
extern "C" __global__ void __launch_bounds__(64 * RH_LANE_W)
rh_grad_lane_kernel(const rh_model_data d, const rh_lane_rows rows, const double *__restrict__ q, const int *__restrict__ list,
                    const int *__restrict__ nlive, const int *__restrict__ vflag, double *__restrict__ partial, int *__restrict__ err_out,
                    int *__restrict__ n_running, const int chains, const int nsplit, const int xcd_aware) {
  __shared__ double red[RH_LANE_W * RH_LANE_C * RH_NACC_MAX * 64];
  rh_grad_lane_body(d, &rows, q, list, nlive, vflag, partial, err_out, n_running, chains, nsplit, xcd_aware, red);
}
#endif
#endif
