"""The tick engine's lanes as arithmetic (csrc/lanes_plan.hpp: where csrc/engine.cpp cuts a sampler's chains into two halves, and how
it shares the time of overlapping gradient launches out among them), called through a tiny host library and compared with literals
worked by hand.  The rule: two lanes when the smaller lane alone still offers a wavefront to every SIMD,
groups_in_lane x splits x waves_per_workgroup >= 4 x compute units (256 on the MI355X: 1024), the cut on a chain-group boundary as
near the middle as that allows."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rainier_amd", "csrc")
CUS = 256

_WRAP = r'''
// out: lanes, first[0], count[0], first[1], count[1]
extern "C" void lp_cut(int chains, int group, int nsplit, int waves_per_wg, int cus, int forced, int *out) {
  const rh_plan::LaneCut c = rh_plan::lanes_cut(chains, group, nsplit, waves_per_wg, cus, forced);
  out[0] = c.lanes; out[1] = c.first[0]; out[2] = c.count[0]; out[3] = c.first[1]; out[4] = c.count[1];
}
extern "C" double lp_shares(int n, const double *t0, const double *t1, double *share) { return rh_plan::busy_shares(n, t0, t1, share); }
'''
_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="rh_lanes_plan")
        src, so = os.path.join(d, "plan.cpp"), os.path.join(d, "plan.so")
        open(src, "w").write('#include "%s"\n%s' % (os.path.join(CSRC, "lanes_plan.hpp"), _WRAP))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        L.lp_shares.restype = C.c_double
        L.lp_shares.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _lib = L
    return _lib


def cut(chains, group, nsplit, waves_per_wg=1, forced=0, cus=CUS):
    """[(first, count)] of every lane"""
    out = (C.c_int * 5)()
    lib().lp_cut(chains, group, nsplit, waves_per_wg, cus, forced, out)
    return [(out[1 + 2 * k], out[2 + 2 * k]) for k in range(out[0])]


def shares(spans):
    t0 = np.array([a for a, _ in spans], dtype=np.float64)
    t1 = np.array([b for _, b in spans], dtype=np.float64)
    sh = np.full(len(spans), -1.0)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    uni = lib().lp_shares(len(spans), dp(t0), dp(t1), dp(sh))
    return uni, list(sh)


def test_the_automatic_cut():
    assert cut(1024, 8, 16) == [(0, 512), (512, 512)]           # 64 groups x 16 splits = 1024 wavefronts per lane = 4 x 256
    assert cut(1024, 8, 8) == [(0, 1024)]                       # 64 x 8 = 512 < 1024
    assert cut(256, 16, 128, waves_per_wg=1) == [(0, 128), (128, 128)]   # the 16-chain tile: 8 tiles x 128 splits = 1024
    assert cut(256, 16, 64) == [(0, 256)]
    assert cut(1024, 8, 15) == [(0, 1024)] and cut(1016, 8, 16) == [(0, 1016)]   # 960 and 63 x 16 = 1008: one short of the rule
    assert cut(1024, 8, 16, cus=304) == [(0, 1024)]             # the rule follows the device's compute units


def test_37_chains_stay_in_one_lane():
    """5 groups of 8: the smaller lane would have 2, and 2 x splits x 1 reaches 1024 from 512 splits on -- which is the rule itself
    and no property of 37; every count below stays in one lane"""
    for nsplit in range(1, 512):
        assert cut(37, 8, nsplit) == [(0, 37)], nsplit
    assert cut(37, 8, 512) == [(0, 16), (16, 21)]


def test_forced_counts():
    assert cut(1024, 8, 16, forced=1) == [(0, 1024)]
    assert cut(1024, 8, 8, forced=2) == [(0, 512), (512, 512)]
    # 37 chains: the middle is 18.5; boundaries of 8: 16 (2.5 away) or 24 (5.5); of 4: 16 (2.5) or 20 (1.5); of 16: 16 or 32
    assert cut(37, 8, 8, forced=2) == [(0, 16), (16, 21)]
    assert cut(37, 4, 8, forced=2) == [(0, 20), (20, 17)]
    assert cut(37, 16, 8, forced=2) == [(0, 16), (16, 21)]
    assert cut(64, 8, 8, forced=2) == [(0, 32), (32, 32)]
    assert cut(24, 8, 8, forced=2) == [(0, 16), (16, 8)]        # 3 groups, middle 12: a tie between 8 and 16 -> (24 + 8) // 16 = 2 groups
    # fewer than two chain groups: nothing to part
    assert cut(8, 8, 8, forced=2) == [(0, 8)] and cut(5, 8, 8, forced=2) == [(0, 5)] and cut(16, 16, 999, forced=2) == [(0, 16)]
    assert cut(9, 8, 8, forced=2) == [(0, 8), (8, 1)]


@pytest.mark.parametrize("group", [4, 8, 16])
def test_a_forced_cut_never_falls_inside_a_group(group):
    for chains in range(2, 200):
        lanes = cut(chains, group, 8, forced=2)
        if chains <= group:
            assert lanes == [(0, chains)]
            continue
        (f0, c0), (f1, c1) = lanes
        assert f0 == 0 and f1 == c0 and c0 + c1 == chains and c0 % group == 0 and c0 >= group and c1 >= 1, chains
        # no other boundary is nearer the middle
        assert all(abs(2 * c0 - chains) <= abs(2 * b - chains) for b in range(group, chains, group)), chains


@pytest.mark.parametrize("spans,want", [
    ([(0.0, 1.0), (2.0, 4.0), (4.0, 4.5)], [1.0, 2.0, 0.5]),                 # disjoint: shares = spans
    ([(1.0, 3.0), (1.0, 3.0)], [1.0, 1.0]),                                  # identical: half each
    ([(0.0, 8.0), (2.0, 4.0)], [7.0, 1.0]),                                  # nested: 2 + 1 + 4 and 1
    ([(0.0, 6.0), (2.0, 8.0), (4.0, 5.0)], [2.0 + 1.0 + 1.0 / 3 + 0.5, 1.0 + 1.0 / 3 + 0.5 + 2.0, 1.0 / 3]),   # three-way in [4, 5]
    ([(1.0, 1.0), (0.0, 2.0), (5.0, 5.0)], [0.0, 2.0, 0.0]),                 # zero-length spans, inside another and alone
    ([(3.0, 2.0)], [0.0]),                                                   # an end before its start reads as empty
    ([], []),
])
def test_busy_shares(spans, want):
    uni, sh = shares(spans)
    assert sh == pytest.approx(want, rel=0, abs=1e-14)
    # the union worked by hand: merge the sorted spans
    merged = 0.0
    end = -np.inf
    for a, b in sorted((a, max(a, b)) for a, b in spans):
        merged += max(0.0, b - max(a, end))
        end = max(end, b)
    assert uni == merged and sum(sh) == pytest.approx(merged, rel=0, abs=1e-14)


def test_busy_shares_of_two_interleaved_lanes():
    """the engine's case: two lanes of back-to-back launches, the second lane late by 0.25 of a launch and with gaps of its own"""
    a = [(float(i), i + 0.875) for i in range(8)]                 # lane 0: gaps of 0.125
    b = [(i + 0.25, i + 1.125) for i in range(8)]                 # lane 1
    uni, sh = shares(a + b)
    assert uni == 8.125 and sum(sh) == pytest.approx(8.125, rel=0, abs=1e-14)
    # lane 0's first launch runs alone for 0.25, beside lane 1's for 0.625; its later ones alone for 0.125 (lane 1's gap) + 0.75 shared
    assert sh[0] == 0.25 + 0.625 / 2 and sh[1] == 0.125 + 0.75 / 2
    # lane 1's launches: 0.75 shared + 0.125 alone (lane 0's gap); its last one is alone from 7.875 to 8.125
    assert sh[8] == 0.625 / 2 + 0.125 + 0.125 / 2 and sh[15] == 0.625 / 2 + 0.25
