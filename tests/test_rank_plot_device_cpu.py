"""Rank plots on the device (csrc/device/rh_rank_plot.hip.h) without a GPU: the text of its block routines, compiled with the host g++
and driven as rank_plot_run's launches walk them (the workspace cap a parameter), against plain numpy -- searchsorted left / right on
the keys in Double.compare's order, then the bin in Python integers.  Counts and nan are equal or the test fails."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rainier_amd import _capi
from tests.test_rank_diagnostics_device_cpu import ROOT, to_keys

_DRIVER = r'''
#include <vector>
// rank_plot_run's launches (csrc/draws.cpp) by its own plan, one workgroup after the other.  Returns the number of chunks, -1 beyond the cap.
extern "C" int ru_emulate(const double *draws, int chains, long long iterations, long long nvars, long long first, long long n, const int *cols, int K,
                          int bins, long long cap, long long *counts, long long *nan) {
  const rh_plan::RankPlot P = rh_plan::rank_plot_plan(chains, n, K, bins, cap);
  if (P.over_cap) return -1;
  const long long S = P.S, ncounts = (long long)K * chains * bins;
  std::vector<double> y((size_t)(P.pc * S)), slds(RU_TP * RU_STAGE_STRIDE);
  std::vector<rs_key> ka((size_t)(P.pc * S)), kb((size_t)(P.pc * S)), klds(RS_TILE_SLOTS + RS_MERGE_LDS + (size_t)P.lds_bytes / 8 + 1);
  std::vector<unsigned> out((size_t)(ncounts + K), 0u);
  int chunks = 0;
  for (long long k0 = 0; k0 < K; k0 += P.pc, chunks++) {
    const long long p_cnt = P.pc < K - k0 ? P.pc : K - k0;
    rs_key *src = ka.data(), *dst = kb.data();
    for (long long rt = 0; rt < P.stiles; rt++)
      for (long long pl = 0; pl < p_cnt; pl += RU_TP)
        ru_stage_tile(draws, iterations, nvars, first, n, S, cols + k0 + pl, (int)(p_cnt - pl < RU_TP ? p_cnt - pl : RU_TP), rt * RU_ROWS, slds.data(), y.data() + pl * S, RU_BLOCK);
    for (long long bid = 0; bid < P.tiles * p_cnt; bid++)
      rs_tile_sort(y.data() + bid % p_cnt * S, S, 1, 1, S, S, bid / p_cnt * RS_TILE, klds.data(), src + bid % p_cnt * S + bid / p_cnt * RS_TILE, RU_BLOCK);
    for (int k = 0; k < P.passes; k++, std::swap(src, dst))
      for (long long bid = 0; bid < P.mtiles * p_cnt; bid++)
        rs_merge_tile(src + bid % p_cnt * S, dst + bid % p_cnt * S, S, P.run(k), bid / p_cnt * RS_MERGE_TILE, klds.data(), RU_BLOCK);
    for (long long pl = 0; pl < p_cnt; pl++)
      for (long long j = 0; j < P.nsplit; j++) dst[pl * S + j] = src[pl * S + (j << P.shift)];
    for (long long bid = 0; bid < p_cnt * chains * P.segs; bid++) {
      const long long pl = bid / (chains * P.segs), rest = bid - pl * chains * P.segs, c = rest / P.segs, i0 = (rest - c * P.segs) * P.seg_len;
      if (i0 >= n) continue;
      ru_count_block(src + pl * S, dst + pl * S, S, (int)P.nsplit, P.shift, y.data() + pl * S + c * n + i0, (int)(n - i0 < P.seg_len ? n - i0 : P.seg_len), bins,
                     klds.data(), out.data() + ((k0 + pl) * chains + c) * bins, rest == 0 ? out.data() + ncounts + k0 + pl : nullptr, RU_BLOCK);
    }
  }
  for (long long i = 0; i < ncounts; i++) counts[i] = out[i];
  for (int k = 0; k < K; k++) nan[k] = out[ncounts + k];
  return chunks;
}
extern "C" void ru_plan(long long chains, long long n, long long K, int bins, long long cap, long long *o) {
  const rh_plan::RankPlot P = cap ? rh_plan::rank_plot_plan(chains, n, K, bins, cap) : rh_plan::rank_plot_plan(chains, n, K, bins);
  const long long v[11] = {P.tiles, P.passes, P.segs, P.stride, P.nsplit, RS_TILE, RS_MERGE_TILE, RU_MAXBINS, RU_MAXSPLIT, RU_SEG_MIN, RU_WS_CAP_BYTES};
  for (int i = 0; i < 11; i++) o[i] = v[i];
}
'''
PLAN_FIELDS = ("tiles", "passes", "segs", "stride", "nsplit", "TILE", "MERGE_TILE", "MAXBINS", "MAXSPLIT", "SEG_MIN", "CAP")
_emu, _cases = None, {}


def emulation():
    """draws_plan.hpp (which brings rh_summary.hip.h and rh_rank_plot.hip.h in host mode) + the driver above as a host shared library"""
    global _emu
    if _emu is None:
        d = tempfile.mkdtemp(prefix="rh_rank_plot_emu")
        src, so = os.path.join(d, "emu.cpp"), os.path.join(d, "emu.so")
        open(src, "w").write('#include "%s"\n%s' % (os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp"), _DRIVER))
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-shared", "-fPIC", src, "-o", so])
        _emu = C.CDLL(so)
        ll, lp = C.c_longlong, C.POINTER(C.c_longlong)
        _emu.ru_emulate.argtypes = [C.POINTER(C.c_double), C.c_int, ll, ll, ll, ll, C.POINTER(C.c_int), C.c_int, C.c_int, ll, lp, lp]
        _emu.ru_plan.argtypes = [ll, ll, ll, C.c_int, ll, lp]
    return _emu


def plan(chains, n, k, bins, cap=0):
    out = (C.c_longlong * len(PLAN_FIELDS))()
    emulation().ru_plan(chains, n, k, bins, cap, out)
    return dict(zip(PLAN_FIELDS, list(out)))


def emulate(x, first, n, cols, bins, cap=0):
    """the host emulation over x [chains][iterations][nvars] -> (counts [K][chains][bins], nan [K], chunks)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    sel = np.ascontiguousarray(range(x.shape[2]) if cols is None else cols, dtype=np.int32)
    counts, nan = np.full((len(sel), x.shape[0], bins), -1, dtype=np.int64), np.full(len(sel), -1, dtype=np.int64)
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
    chunks = emulation().ru_emulate(_capi.dptr(x), x.shape[0], x.shape[1], x.shape[2], first, n, sel.ctypes.data_as(C.POINTER(C.c_int)), len(sel), bins,
                                    cap or plan(1, 1, 1, 2)["CAP"], lp(counts), lp(nan))
    return counts, nan, chunks


def reference(x, first, n, cols, bins):
    """numpy on the same window: ranks by searchsorted on the sorted keys, the bin in Python integers"""
    w = x[:, first:first + n, :]
    sel = range(x.shape[2]) if cols is None else cols
    S = w.shape[0] * n
    counts, nan = np.zeros((len(sel), w.shape[0], bins), dtype=np.int64), np.array([int(np.isnan(w[:, :, c]).sum()) for c in sel], dtype=np.int64)
    for k, c in enumerate(sel):
        keys = to_keys(w[:, :, c].ravel())
        s = np.sort(keys)
        b = [(int(lo) + int(up)) * bins // (2 * S) for lo, up in zip(np.searchsorted(s, keys, "left"), np.searchsorted(s, keys, "right"))]
        if nan[k] == 0:
            np.add.at(counts[k], (np.repeat(np.arange(w.shape[0]), n), np.array(b)), 1)
    return counts, nan


def derived(counts, nan, n, dtype=np.float64):
    """ecdf_gap, ks, chi2 from the counts by the contract's formulas in `dtype`; NaN where the column holds one"""
    b = counts.shape[2]
    gap = np.cumsum(counts, axis=2).astype(dtype) / dtype(n) - np.arange(1, b + 1).astype(dtype) / dtype(b)
    chi2 = ((counts.astype(dtype) - dtype(n) / dtype(b)) ** 2 / (dtype(n) / dtype(b))).sum(axis=2)
    gap[nan > 0], chi2[nan > 0] = np.nan, np.nan
    return gap, np.abs(gap).max(axis=2), chi2


# the columns of the seven-column buffer: 0 normal, 1 constant, 2 only -0.0 / +0.0, 3 with -inf and two +inf, 4 with one NaN, 5 chain 0 up by 10 sd, 6 ties
CASES = ("one", "four", "ragged", "values", "tiles", "segments", "maxbins", "identity")


def case(name):
    """name -> dict(x, first, n, cols, bins, cap (0: the header's), ref = the reference's (counts, nan)), built once and shared"""
    if name not in _cases:
        k = plan(1, 1, 1, 2)
        chains, n, nvars, cols, bins, first, cap = {
            "one": (1, 1, 1, None, 2, 0, 0), "four": (1, 4, 1, None, 2, 0, 0),
            "ragged": (3, 257, 7, [5, 0, 5, 2], 20, 2, 0), "values": (3, 257, 7, None, 20, 2, 0),
            "tiles": (8, k["TILE"] + 3, 2, None, 64, 1, 0),                                 # several sort tiles and merge passes, stride > 1
            "segments": (2, 2 * k["SEG_MIN"] + 5, 3, None, 20, 0, 2 * 24 * 2 * (2 * k["SEG_MIN"] + 5)),   # two columns to a chunk on the CPU
            "maxbins": (2, 37, 1, None, k["MAXBINS"], 0, 0), "identity": (4, 250, 1, None, 20, 0, 0)}[name]
        x = np.random.default_rng(len(name) + 7 * chains).standard_normal((chains, first + n + 3, nvars))
        if nvars == 7:
            x[:, :, 1] = 2.0
            x[:, :, 2] = np.where(x[:, :, 2] < 0.0, -0.0, 0.0)
            x[1, first + 5, 3], x[2, first, 3], x[0, first + n - 1, 3] = np.inf, -np.inf, np.inf
            x[1, first + 100, 4], x[0, first - 1, 4] = np.nan, np.nan                        # the second one lies outside the window
            x[0, :, 5] += 10.0
            x[:, :, 6] = np.round(2.0 * x[:, :, 6])
        _cases[name] = dict(x=x, first=first, n=n, cols=cols, bins=bins, cap=cap, ref=reference(x, first, n, cols, bins))
    return _cases[name]


@pytest.mark.parametrize("name", CASES)
def test_emulation_equals_the_numpy_reference(name):
    c = case(name)
    x, first, n, cols, B = c["x"], c["first"], c["n"], c["cols"], c["bins"]
    chains, k = x.shape[0], len(cols) if cols else x.shape[2]
    counts, nan, chunks = emulate(x, first, n, cols, B, c["cap"])
    assert np.array_equal(counts, c["ref"][0]) and np.array_equal(nan, c["ref"][1]), name
    assert np.array_equal(counts.sum(axis=2)[nan == 0], np.full(((nan == 0).sum(), chains), n))
    p, S = plan(chains, n, k, B, c["cap"]), chains * n
    if name == "tiles":
        assert p["tiles"] > 1 and p["passes"] >= 2 and p["stride"] > 1 and p["nsplit"] <= p["MAXSPLIT"] and S % p["MERGE_TILE"] != 0
    if name == "segments":
        assert p["segs"] > 1 and chunks == 2 and plan(chains, n, k, B)["segs"] > 1                   # ... and with the header's cap, as the GPU runs it
        assert plan(4, 100000, 1, B)["segs"] * 4 >= 256 and plan(1024, 1000, 5, B)["segs"] == 1      # few long chains fill the device; many short ones are not cut
        assert np.array_equal(emulate(x, first, n, cols, B)[0], counts)                              # one chunk: the same integers
    if name == "identity":                                                                           # no ties, bins divides S
        assert np.array_equal(counts.sum(axis=1), np.full((1, B), S // B))
    if name == "ragged":                                                                             # a window gives what its copy gives
        assert np.array_equal(emulate(x[:, first:first + n, :], 0, n, cols, B)[0], counts) and np.array_equal(counts[0], counts[2])
    if name == "values":
        neg = int(np.signbit(x[:, first:first + n, 2]).sum())                                        # -0.0 ranks first: they share r2 = neg + 1
        assert np.all(counts[1, :, (S * B) // (2 * S)] == n) and counts[2][:, (neg * B) // (2 * S)].sum() >= neg        # the constant: r2 = S + 1
        assert counts[3][:, 0].sum() >= 1 and counts[3][:, B - 1].sum() >= 2 and list(nan) == [0, 0, 0, 0, 1, 0, 0] and not counts[4].any()
        ks = derived(counts, nan, n)[1]
        assert counts[5, 0, :B - B // 3 - 1].sum() == 0 and ks[5, 0] == np.nanmax(ks) and np.all(np.isnan(ks[4]))


def test_exports_code_object_and_refusals():
    import rainier_amd as R
    L = _capi.lib()
    assert all(name in _capi.EXPORTS and hasattr(L, name) for name in ("rh_sampler_rank_plot", "rh_rank_plot_device", "rh_rank_plot_lower_only"))
    assert L.rh_abi_version() == 6 and R.RankPlot._fields == ("counts", "ecdf_gap", "ks", "chi2", "nan", "cols", "bins")
    assert b"rh_rank_plot_count_kernel" in _capi.rank_plot_lower_only("gfx950")                     # built, and judged as before a launch
    counts, nan = np.zeros((2, 4, 1024), dtype=np.int64), np.zeros(2, dtype=np.int64)
    lp, ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)), C.POINTER(C.c_int32)

    def call(ptr=C.c_void_p(4096), chains=4, iters=10, first=0, count=10, cols=None, bins=20, out=(counts, nan)):   # the pointer is never dereferenced
        sel = np.array(cols, dtype=np.int32) if cols is not None else None
        return L.rh_rank_plot_device(ptr, 0, chains, iters, 2, first, count, sel.ctypes.data_as(ip) if cols is not None else None, len(cols or ()),
                                     bins, *[lp(a) if a is not None else None for a in out])
    for kw in (dict(ptr=None), dict(out=(None, nan)), dict(out=(counts, None)), dict(bins=1), dict(bins=1025), dict(count=0), dict(first=-1), dict(first=5, count=6),
               dict(count=11), dict(cols=[2]), dict(cols=[0, -1]), dict(chains=0)):
        assert call(**kw) == _capi.RH_E_INVALID, kw
    assert L.rh_sampler_rank_plot(None, 0, 10, None, 0, 20, lp(counts), lp(nan)) == _capi.RH_E_INVALID
    assert call(chains=4096, iters=2048, count=2048) == _capi.RH_E_UNSUPPORTED and "workspace" in L.rh_last_error(None).decode()
    with pytest.raises(R.RainierHipError, match="bins must be"):                                    # ... before anything of that size is allocated
        R.rank_plot_device(4096, 4, 10, 2, bins=10 ** 12)
    if L.rh_device_count() == 0:
        assert call() == _capi.RH_E_DEVICE and call(count=1, bins=2) == _capi.RH_E_DEVICE
        with pytest.raises(R.RainierHipError, match="no CPU fallback"):
            R.rank_plot_device(4096, 4, 10, 2)
