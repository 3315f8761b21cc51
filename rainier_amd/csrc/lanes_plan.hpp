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
