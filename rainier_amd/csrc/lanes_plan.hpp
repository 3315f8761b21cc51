// lanes_plan.hpp -- the tick engine's lanes (engine.cpp, advance_to_ticks): where a sampler's chains are cut into two halves that
// advance on two streams, and how the time of gradient launches that overlap is shared out among them.  Arithmetic only: no HIP, no
// allocation beyond the sweep's own scratch, no globals.
#ifndef RH_LANES_PLAN_HPP
#define RH_LANES_PLAN_HPP

#include <algorithm>
#include <vector>

namespace rh_plan {
// ---- the cut ----
// chains: the sampler's; group: chains per wavefront of the gradient kernel (RH_GRAD_K, or the 16-chain tile of the MFMA GLM kernel);
// nsplit: row splits per chain group, computed from the TOTAL chain count (a chain's sums keep their order whatever the cut);
// waves_per_wg: wavefronts of one gradient workgroup; cus: the device's compute units (4 SIMDs each); forced: 0 = the rule below,
// 1 = one lane, 2 = two lanes wherever there are two chain groups to part.
struct LaneCut { int lanes, first[2], count[2]; };
inline LaneCut lanes_cut(int chains, int group, int nsplit, int waves_per_wg, int cus, int forced) {
  LaneCut one = {1, {0, 0}, {chains, 0}};
  const int ngroups = (chains + group - 1) / group;
  if (forced == 1 || ngroups < 2) return one;
  // on a group boundary, as near the middle as that allows (a tie goes to the upper boundary); both lanes keep a group
  const int cg = std::max(1, std::min(ngroups - 1, (chains + group) / (2 * group)));
  const int cut = cg * group;
  // two lanes only where each one alone still offers a wavefront to every SIMD: the other lane's launch must be able to keep the
  // fp64 pipe busy alone while this one sits in a gap, a tick or a prologue (profiles/r3_a_cfg2/sweep.txt: p2_u8_s8 against p2_u8_s16)
  const long long smaller = std::min(cg, ngroups - cg);
  if (forced != 2 && smaller * nsplit * waves_per_wg < 4LL * cus) return one;
  return {2, {0, cut}, {cut, chains - cut}};
}

// ---- the lane walk (rh_grad_lane_kernel) ----
// Its shape: W wavefronts per workgroup, R rows per scalar request, C chains per lane (RH_LANE_W / _R / _C of rh_lane.hip.h), a
// chain group of 64 C chains; measured on cfg 2, profiles/lane_walk_cfg2.
constexpr int kLaneW = 8, kLaneR = 8, kLaneC = 2, kLaneGroup = 64 * kLaneC;
// Where the lane walk is chosen (profiles/lane_walk_cfg2/threshold_sweep.jsonl: tile against lane walk, same machine, static HMC
// L = 32): at 1e6 rows it wins by 14-18 % from 512 to 2048 chains and by 5 % at 256; at 70 000 rows it LOSES 17-20 % at 1024 and
// 2048 chains, where a launch takes 20-30 us and the tick behind every launch (the walk has no fused form) costs more than the
// kernel gains.  So: at least 512 chains and 5.12e8 row-chain evaluations per gradient, the smallest point measured with a clear gain.
constexpr int kLaneMinChains = 512;
constexpr long long kLaneMinEvals = 512LL * 1000000LL;
// does a model's row code fit the walk at R rows per request: R rows of every column in scalar registers (2 each, 64 of the ~100
// there are), and the W wavefronts' sums of a chain group in 64 KB of LDS
inline bool lane_walk_fits_r(int ncols_max, int nacc_max, int r) {
  return ncols_max >= 1 && ncols_max * r * 2 <= 64 && nacc_max >= 1 && (long long)kLaneW * kLaneC * nacc_max * 64 * 8 <= 64 * 1024;
}
inline bool lane_walk_fits(int ncols_max, int nacc_max) { return lane_walk_fits_r(ncols_max, nacc_max, kLaneR); }
// Which walk a sampler's gradient launches take -- decided once, at its creation, from the model, the sampler's configuration and
// the TOTAL chain count only (like nsplit; rh_sample_multi hands its decision to its shards).  model_has_lane: the lane kernel was
// built and is fit to run; grad_chains: the caller's rh_compile_opts.grad_chains (an explicit K asks for K chains per wavefront,
// which is the tile kernel); max_rows: the rows of the model's longest row target; forced: 0 = this rule, 1 = tile, 2 = lane
// wherever the model has it (RH_GRAD_WALK).
inline bool walk_is_lane(bool model_has_lane, bool static_hmc, int grad_chains, int total_chains, long long max_rows, int forced) {
  if (!model_has_lane || forced == 1) return false;
  if (forced == 2) return true;
  return static_hmc && grad_chains == 0 && total_chains >= kLaneMinChains && (long long)total_chains * max_rows >= kLaneMinEvals;
}
// The lane walk's row splits per chain group: eight wavefronts per SIMD of a 256-CU device (8192) over groups x splits x W, a
// multiple of 8 for the XCD mapping, and no more than leave a split 512 rows (a block of R rows for each of the W wavefronts,
// eight times over).  cfg 2: 8 groups -> 128 splits.
inline int lane_nsplit(int total_chains, long long max_rows) {
  const long long ngroups = std::max(1, (total_chains + kLaneGroup - 1) / kLaneGroup);
  long long nsplit = std::max<long long>(1, (8192 + ngroups * kLaneW - 1) / (ngroups * kLaneW));
  nsplit = ((nsplit + 7) / 8) * 8;
  const long long cap = std::max<long long>(8, (max_rows / 512) / 8 * 8);
  return (int)std::min(nsplit, cap);
}

// ---- the lane walk's row feed (rh_grad_lane_kernel of the *.lanerows.co) ----
// The same walk with the rows of a target taken from an interleaved copy of its columns -- element (r, j) of rows x NC at r NC + j,
// zeros up to a whole block of 8 rows, base aligned to a 64-byte line -- so that one 64-byte request is whole rows and a SET of rows
// can be asked for while the set before it is worked on.  A target takes the feed when its rows are 8, 16, 32 or 64 bytes:
//   rows per set = min(rows per block, 16 / NC), at most 128 bytes = two requests = 32 scalar registers; two sets are the 64 the
//   column feed holds; the set divides the block, so a piece of whole blocks is whole sets.
inline int lane_rows_set(int nc, int r = kLaneR) { return nc >= 1 && nc <= 16 ? std::min(r, 16 / nc) : 0; }
inline bool lane_rows_eligible(int nc, int r = kLaneR) {
  if (!(nc == 1 || nc == 2 || nc == 4 || nc == 8)) return false;
  const int set = lane_rows_set(nc, r);
  return set >= 1 && 2 * set * nc * 2 <= 64 && r % set == 0 && 8 % set == 0;
}
inline long long lane_rows_padded(long long rows) { return (rows + 7) / 8 * 8; }              // rows of the copy, padding included
inline long long lane_rows_doubles(long long rows, int nc) { return lane_rows_padded(rows) * nc; }
inline long long lane_rows_index(long long r, int nc, int j) { return r * nc + j; }
// out: lane_rows_doubles(rows, nc) doubles; cols: the target's nc columns of `rows` values
inline void lane_rows_place_column(const double *col, long long rows, int nc, int j, double *out) {   // (the padding is the caller's)
  for (long long r = 0; r < rows; r++) out[lane_rows_index(r, nc, j)] = col[r];
}
inline void lane_rows_interleave(const double *const *cols, long long rows, int nc, double *out) {
  for (int j = 0; j < nc; j++) lane_rows_place_column(cols[j], rows, nc, j, out);
  for (long long i = rows * nc, e = lane_rows_doubles(rows, nc); i < e; i++) out[i] = 0.0;
}
// May a launch whose row targets have want[i] rows read the copies -- have[i] rows each, copy[i] == nullptr where target i walks its
// columns --?  Only if every copy holds at least the rows the launch walks (the kernel reads rows below want[i] and nothing else).
inline bool lane_rows_cover(int n_want, const long long *want, int n_have, const long long *have, const void *const *copy) {
  if (n_want != n_have) return false;
  for (int i = 0; i < n_want; i++) if (copy[i] && want[i] > have[i]) return false;
  return true;
}
// Which feed a sampler's lane-walk launches take: the row feed wherever the model has the kernel -- measured on cfg 2,
// profiles/lane_feed_cfg2 --; forced: 0 = this rule, 1 = columns, 2 = rows wherever the kernel exists (RH_LANE_FEED).
constexpr bool kLaneFeedRowsDefault = true;
inline bool feed_is_rows(bool model_has_rows_kernel, int forced) {
  if (!model_has_rows_kernel || forced == 1) return false;
  return forced == 2 || kLaneFeedRowsDefault;
}

// ---- the rounds of a run ----
// advance_to_ticks enqueues a ROUND of gradient launches (each with its tick and compaction) on every live lane, then synchronises and
// reads how many chains still run.  A lock-step run -- static HMC in the sampling phase: every chain asks for the same launches, and
// `remaining`, the gradient launches the call still has to do, is exact -- takes the whole remainder in one round, up to the cap: the
// host has nothing to decide in between, and every round boundary is a stretch in which the device waits for the host.  Everything
// else does not know how far its chains are, and asks after kRoundHint launches (never more than kRoundMaxDynamic in a round).  A
// lock-step count that has run out while a chain still runs (a chain out of step) is no longer exact: one trajectory of `ltraj`
// launches at a time.
constexpr int kRoundCapDefault = 4096, kRoundMaxDynamic = 256, kRoundHint = 32;
// the cap of a sampler's rounds, which sizes its per-lane live log and event pools: RH_ROUND_MAX=n lowers it, to 1 at the least
inline int round_cap(int requested) { return std::max(1, std::min(requested, kRoundCapDefault)); }
// launches of the next round; a cap below 1 reads as 1
inline int round_launches(bool lock_step, long long remaining, int ltraj, int cap) {
  const long long c = std::max(1, cap);
  if (!lock_step) return (int)std::min<long long>(c, std::min<long long>(kRoundMaxDynamic, std::max<long long>(1, remaining)));
  return (int)std::min<long long>(c, remaining > 0 ? remaining : std::max(1, ltraj));
}

// ---- the busy share of overlapping spans ----
// n spans [t0[i], t1[i]] on one time base (t1 < t0 is read as an empty span at t0).  share[i] = the integral over span i of
// 1 / (spans open at that instant); the shares add up to the length of the union of the spans, which is the value returned.
inline double busy_shares(int n, const double *t0, const double *t1, double *share) {
  struct End { double t; int kind, i; };   // kind 0 opens span i, 1 closes it: at one instant the openings come first
  std::vector<End> ends;
  ends.reserve((size_t)2 * n);
  for (int i = 0; i < n; i++) {
    share[i] = 0.0;
    ends.push_back({t0[i], 0, i});
    ends.push_back({std::max(t0[i], t1[i]), 1, i});
  }
  std::sort(ends.begin(), ends.end(), [](const End &a, const End &b) { return a.t != b.t ? a.t < b.t : (a.kind != b.kind ? a.kind < b.kind : a.i < b.i); });
  std::vector<int> open;
  double uni = 0.0, prev = 0.0;
  for (const End &e : ends) {
    if (!open.empty() && e.t > prev) {
      const double part = (e.t - prev) / (double)open.size();
      for (int i : open) share[i] += part;
      uni += e.t - prev;
    }
    prev = e.t;
    if (e.kind == 0) open.push_back(e.i);
    else open.erase(std::find(open.begin(), open.end(), e.i));
  }
  return uni;
}
}  // namespace rh_plan
#endif
