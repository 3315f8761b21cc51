"""The lane walk without a device: what the cross-compiled kernel looks like (rh_grad_lane_kernel, a code object of its own next
to the model's), which models get one, and the rule that picks the walk for a sampler (csrc/lanes_plan.hpp: walk_is_lane,
lane_nsplit), called through a tiny host library like tests/test_lanes_plan_cpu.py does."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from rainier_amd import _capi, models
from tests import lane_walk_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rainier_amd", "csrc")
FAST = dict(fp_contract=True, factor_outputs=True)

_WRAP = r'''
extern "C" int lw_is_lane(int has_lane, int static_hmc, int grad_chains, int total_chains, long long max_rows, int forced) {
  return rh_plan::walk_is_lane(has_lane != 0, static_hmc != 0, grad_chains, total_chains, max_rows, forced) ? 1 : 0;
}
extern "C" int lw_nsplit(int total_chains, long long max_rows) { return rh_plan::lane_nsplit(total_chains, max_rows); }
extern "C" int lw_fits(int ncols_max, int nacc_max) { return rh_plan::lane_walk_fits(ncols_max, nacc_max) ? 1 : 0; }
extern "C" int lw_fits_r(int ncols_max, int nacc_max, int r) { return rh_plan::lane_walk_fits_r(ncols_max, nacc_max, r) ? 1 : 0; }
extern "C" int lw_shape(int i) { const int v[] = {rh_plan::kLaneW, rh_plan::kLaneR, rh_plan::kLaneC, rh_plan::kLaneGroup, rh_plan::kLaneMinChains, (int)(rh_plan::kLaneMinEvals / 1000000)}; return v[i]; }
'''
_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="rh_lane_walk")
        src, so = os.path.join(d, "plan.cpp"), os.path.join(d, "plan.so")
        open(src, "w").write('#include "%s"\n%s' % (os.path.join(CSRC, "lanes_plan.hpp"), _WRAP))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", so])
        _lib = C.CDLL(so)
        _lib.lw_nsplit.argtypes = [C.c_int, C.c_longlong]
        _lib.lw_is_lane.argtypes = [C.c_int] * 4 + [C.c_longlong, C.c_int]
    return _lib


def _lane(rep):
    return {k: v for (tag, k), v in rep["kernels"].items() if tag == "lane"}


def test_the_flagship_build_carries_a_lane_kernel_that_fits_eight_wavefronts_per_simd():
    spec = models.linreg(n=8, k=3)
    src, rep = _capi.lower_report(spec.rir, _capi.compile_opts(**FAST))
    lane = _lane(rep)
    assert list(lane) == ["rh_grad_lane_kernel"]
    k = lane["rh_grad_lane_kernel"]
    assert k["fit"] and k["vgpr_spills"] == 0 and k["sgpr_spills"] == 0 and k["scratch"] == 0 and k["unproven"] == 0
    assert 0 < k["vgprs"] <= 64          # 512 registers per SIMD lane: eight wavefronts
    # the model's own code object is what it was: no kernel of the lane walk in it, the tile kernels in their shape
    base = {k for (tag, k) in rep["kernels"] if tag == "base"}
    assert "rh_grad_lane_kernel" not in base and {"rh_grad_kernel", "rh_grad_fused_kernel", "rh_tick_kernel"} <= base
    assert "rh_grad_lane_kernel" not in src      # ... and its source: csrc/device/rh_lane.hip.h follows it in the lane build only


def test_an_explicit_chain_group_size_or_a_sampler_variant_builds_no_lane_kernel():
    spec = models.linreg(n=8, k=3)
    _, rep8 = _capi.lower_report(spec.rir, _capi.compile_opts(grad_chains=8, **FAST))
    assert not _lane(rep8)
    tile = {k: v for (tag, k), v in rep8["kernels"].items() if tag == "base" and k in ("rh_grad_kernel", "rh_grad_fused_kernel")}
    assert len(tile) == 2 and all(v["fit"] and 128 < v["vgprs"] <= 200 and v["vgpr_spills"] == 0 for v in tile.values())
    _, repn = _capi.lower_report(spec.rir, _capi.compile_opts(with_nuts=True, **FAST))
    assert not _lane(repn)


def test_a_strict_build_takes_four_rows_per_request_and_a_row_that_fits_neither_has_no_lane_kernel():
    # strict arithmetic (no contraction, the log-density's own terms): with 8 rows the kernel spills scalar registers and is dropped
    # (a marker takes its place in the cache); with 4 it fits
    _, rep = _capi.lower_report(models.linreg(n=8, k=3).rir, _capi.compile_opts(math_mode=_capi.MATH_STRICT))
    k = _lane(rep)["rh_grad_lane_kernel"]
    assert k["fit"] and k["vgpr_spills"] == 0 and k["sgpr_spills"] == 0 and k["scratch"] == 0 and k["sgprs"] < 96
    _, rep = _capi.lower_report(models.logistic(n=8, k=2).rir, _capi.compile_opts(math_mode=_capi.MATH_STRICT))
    assert not _lane(rep)


def test_which_models_the_walk_fits():
    L = lib()
    assert [L.lw_shape(i) for i in range(6)] == [8, 8, 2, 128, 512, 512]
    assert L.lw_fits(4, 5) == 1 and L.lw_fits(1, 1) == 1 and L.lw_fits(4, 8) == 1
    assert L.lw_fits(5, 5) == 0        # 5 columns x 8 rows x 2 = 80 scalar registers
    assert L.lw_fits(4, 9) == 0        # 8 x 2 x 9 x 64 doubles = 72 KB of LDS
    assert L.lw_fits(0, 5) == 0
    assert L.lw_fits_r(8, 5, 4) == 1 and L.lw_fits_r(9, 5, 4) == 0


def test_the_rule_that_picks_the_walk():
    L = lib()
    M = 1_000_000
    is_lane = lambda has, static, k, chains, rows=M, forced=0: bool(L.lw_is_lane(int(has), int(static), k, chains, rows, forced))
    assert is_lane(True, True, 0, 1024) and is_lane(True, True, 0, 4096)      # the flagship: static HMC, automatic K, 1024 chains x 1e6 rows
    # the measured points (profiles/lane_walk_cfg2/threshold_sweep.jsonl): a gain from 512 chains x 1e6 rows on, a loss on short rows
    assert is_lane(True, True, 0, 512) and is_lane(True, True, 0, 768) and is_lane(True, True, 0, 2048)
    assert not is_lane(True, True, 0, 511) and not is_lane(True, True, 0, 256)
    assert not is_lane(True, True, 0, 1024, rows=70_000) and not is_lane(True, True, 0, 2048, rows=70_000)
    assert not is_lane(True, True, 0, 1024, rows=499_999) and is_lane(True, True, 0, 1024, rows=500_000)
    assert not is_lane(True, False, 0, 1024)         # EHMC / NUTS (cfg 2 under DefaultConfig, cfg 4, cfg 5)
    assert not is_lane(True, True, 8, 1024)          # an explicit K is a request for the tile kernel
    assert not is_lane(False, True, 0, 1024) and not is_lane(False, True, 0, 1024, forced=2)
    assert is_lane(True, False, 8, 1, rows=10, forced=2) and not is_lane(True, True, 0, 1024, forced=1)
    # every sampler the GPU tests create has fewer than 512 chains in all, or an explicit K, or a dynamic sampler: the tile walk --
    # but for the benched configuration's own test (tests/test_gpu_baseline_sizes.py), where the rule picks the walk on the device
    for chains in (1, 3, 9, 11, 21, 37, 64, 165, 256, 511):
        for k in (0, 2, 4, 8):
            for static in (False, True):
                for rows in (3000, 70_001, 600_000, M, 10 * M):
                    assert not is_lane(True, static, k, chains, rows)


def test_row_splits_of_the_lane_walk():
    L = lib()
    assert L.lw_nsplit(1024, 1_000_000) == 128      # 8 groups x 128 splits x 8 wavefronts = 8192 = eight per SIMD
    assert L.lw_nsplit(2048, 1_000_000) == 64 and L.lw_nsplit(4096, 10_000_000) == 32
    assert L.lw_nsplit(1, 65_573) == 128 and L.lw_nsplit(165, 65_573) == 128      # capped: a split keeps 512 rows
    assert L.lw_nsplit(1024, 100) == 8
    for chains in (1, 100, 1000, 1024, 1500, 5000, 100_000):
        for rows in (1, 4096, 65_573, 1_000_000, 10_000_000):
            n = L.lw_nsplit(chains, rows)
            assert n >= 8 and n % 8 == 0


# ---- which models get the walk (tests/lane_walk_cases.py): the cross-compile report of every case, with the case's data ----
LANE = "rh_grad_lane_kernel"
_reports = {}


def _report(name, spec, opts):
    if name not in _reports:
        _reports[name] = _capi.lower_report(spec.rir, _capi.compile_opts(**opts), columns=spec.columns, nrows=spec.nrows)
    return _reports[name]


def _check_lane_entry(k, src):
    """a lane kernel the engine keeps: fit, no spill, no scratch, and the static LDS of the workgroup's sums -- W wavefronts x C chains
    per lane x RH_NACC_MAX sums x 64 lanes of doubles; -> (rows per scalar request, RH_NACC_MAX)"""
    assert k["fit"] and k["vgpr_spills"] == 0 and k["sgpr_spills"] == 0 and k["scratch"] == 0 and k["unproven"] == 0
    assert 0 < k["vgprs"] <= 256          # (__launch_bounds__(512): eight wavefronts on four SIMDs)
    nacc_max = int(re.search(r"#define RH_NACC_MAX (\d+)", src).group(1))
    assert k["lds"] == 8 * 2 * nacc_max * 64 * 8 <= 65536
    return k["lane_r"], nacc_max


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_which_models_get_a_lane_kernel_and_with_how_many_rows_per_request(case):
    """lane_eligible() / build_lane_code() decide silently, and RH_GRAD_WALK=lane falls back to the tile walk for a model without the
    kernel: this is the test that notices a model losing, or gaining, the walk"""
    spec = case.make(case.n_build)[0]
    src, rep = _report(case.name, spec, case.opts)
    lane = _lane(rep)
    if not case.lane:
        assert not lane, (case, lane)
        return
    assert list(lane) == [LANE], (case, "no lane kernel")
    r, nacc_max = _check_lane_entry(lane[LANE], src)
    assert r == case.r
    assert nacc_max == {"linreg5-strict": 8, "linreg6-fast": 8}.get(case.name, nacc_max)      # the 64 KB of static LDS ...
    if nacc_max == 8:
        assert lane[LANE]["lds"] == 65536                                                     # ... exactly
    assert ("HAS_VALUE_ONLY = true" in src) == case.value_only
    assert int(re.search(r"#define RH_NROWTARGETS (\d+)", src).group(1)) == case.targets
    if case.targets == 2:     # a target that adds fewer sums than the other: its own NA under the stride RH_NACC_MAX (in three of the four)
        nacc = tuple(int(x) for x in re.findall(r"NACC = (\d+), ROWT = [01];", src))
        assert nacc == {"two_targets-fast": (3, 2), "two_targets-strict": (4, 2), "two_targets_log-fast": (2, 2), "two_targets_log-strict": (2, 3)}[case.name]
        assert max(nacc) == nacc_max


def _source(spec, opts):
    src = _capi.lower_only(spec.rir, _capi.compile_opts(**opts), columns=spec.columns, nrows=spec.nrows, compile=False)[0]
    return src.split("\n// rh_kpool")[0]      # (the constant pool's values travel behind the source as a comment: not hashed)


@pytest.mark.parametrize("case", LC.POSITIVE, ids=repr)
def test_the_cases_source_does_not_depend_on_the_row_count(case):
    # ... so that every row count tests/test_gpu_lane_walk_models.py runs loads the code objects build() left in the kernel cache
    base = _source(case.make(case.n_build)[0], case.opts)
    for n in tuple(case.row_counts) + (case.n_main,):
        assert _source(case.make(n)[0], case.opts) == base, (case, n)


def test_which_random_models_get_a_lane_kernel():
    """tests/fuzz_models.GPU_FUZZ_CASES' eight-slot models, lowered with their data like build() does: LC.FUZZ_LANE lists exactly the
    (seed, build) pairs with a lane kernel, so tests/test_gpu_lane_walk_models.py leaves out none that has one"""
    have = []
    for seed, kw in LC.FUZZ_SLOTS:
        spec = LC.fuzz_spec(seed, kw)[0]
        for build in ("fast", "strict"):
            src, rep = _report("fuzz_slots_%d-%s" % (seed, build), spec, LC.BUILDS[build])
            lane = _lane(rep)
            if lane:
                _check_lane_entry(lane[LANE], src)
                have.append((seed, build))
    assert sorted(have) == sorted(LC.FUZZ_LANE)
    # (seed 1 has none in either build: its fast row code spills vector registers at 8 rows per request and scalar ones at 4)
    assert {(0, "fast"), (2, "fast"), (3, "fast"), (2, "strict")} <= set(have) and not {(1, "fast"), (1, "strict")} & set(have)
