"""The launch plan of the calls over device-resident draws (csrc/draws_plan.hpp: the arithmetic csrc/draws.cpp launches from and the
CPU tests' drivers of the device text walk), called through a tiny host library and compared with literals worked by hand from the
rules: cap = 134217728 bytes for both workspaces, RT_SL = 101 doubles per (parameter, chain), RT_TP = 16 parameters per tile,
RS_TILE = 4096 keys per tile sort, RS_MERGE_TILE = 2048 outputs per merge workgroup, 16 bytes of sort workspace per pooled value,
RP_TILE_FOR over 8064 staged doubles.  Nothing of the sizes named here is allocated: the plan is arithmetic."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rainier_amd", "csrc")
FLAT, GATHER, DIRECT = 0, 1, 2

_WRAP = r'''
extern "C" long long tp_trace_chunk(int chains, int nvars) { return rh_plan::trace_chunk(chains, nvars); }
extern "C" long long tp_trace_tiles(long long p_cnt) { return rh_plan::trace_tiles(p_cnt); }
// out: kept, N, per_param, over_cap, pc, tiles, mtiles, passes, hidx, the run lengths [8], the indices [RS_MAX_PROBS]
extern "C" void tp_summary(long long chains, long long count, long long thin, long long nvars, const double *probs, int nprobs, double hdpi_prob,
                           long long *out) {
  const rh_plan::Summary P = rh_plan::summary_plan(chains, count, thin, nvars, probs, nprobs, hdpi_prob);
  const long long head[9] = {P.kept, P.N, P.per_param, P.over_cap, P.pc, P.tiles, P.mtiles, P.passes, P.hidx};
  for (int i = 0; i < 9; i++) out[i] = head[i];
  for (int k = 0; k < 8; k++) out[9 + k] = k < P.passes ? P.run(k) : 0;
  for (int k = 0; k < RS_MAX_PROBS; k++) out[17 + k] = P.idx[k];
}
extern "C" void tp_predict(int nvars, int nref, int thin, int *form_tile) {
  const rh_plan::PredictLaunch pl = rh_plan::predict_launch(nvars, nref, thin);
  form_tile[0] = pl.form; form_tile[1] = pl.tile;
}
extern "C" int tp_pred_tile_mirror(int stride) { return rh_plan::pred_tile_for(stride); }
extern "C" int tp_pred_tile_macro(int stride) { return RP_TILE_FOR(stride); }
'''
_lib = None


def lib():
    """draws_plan.hpp + the wrappers above, and -- for the predict mirrors -- the four defines of rh_predict.hip.h they mirror, taken
    from that header's text"""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="rh_draws_plan")
        hdr = open(os.path.join(CSRC, "device", "rh_predict.hip.h")).read()
        defines = [re.search(r"^#define %s\b.*$" % n, hdr, re.M).group(0) for n in ("RP_WAVE", "RP_MAX_TILE", "RP_LDS_DOUBLES", "RP_TILE_FOR")]
        src, so = os.path.join(d, "plan.cpp"), os.path.join(d, "plan.so")
        open(src, "w").write('#include "%s"\n%s\n%s' % (os.path.join(CSRC, "draws_plan.hpp"), "\n".join(defines), _WRAP))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        ll = C.c_longlong
        L.tp_trace_chunk.restype = L.tp_trace_tiles.restype = ll
        L.tp_trace_tiles.argtypes = [ll]
        L.tp_summary.argtypes = [ll, ll, ll, ll, C.POINTER(C.c_double), C.c_int, C.c_double, C.POINTER(ll)]
        _lib = L
    return _lib


def summary(n, nvars=1, probs=(0.5,), hdpi=0.0, chains=1, thin=1, count=None):
    out = (C.c_longlong * 33)()
    pr = np.array(probs, dtype=np.float64)
    lib().tp_summary(chains, n if count is None else count, thin, nvars, pr.ctypes.data_as(C.POINTER(C.c_double)), len(pr), hdpi, out)
    keys = ("kept", "N", "per_param", "over_cap", "pc", "tiles", "mtiles", "passes", "hidx")
    r = dict(zip(keys, out[:9]))
    r["runs"], r["idx"] = [v for v in out[9:17] if v], list(out[17:17 + len(pr)])
    return r


@pytest.mark.parametrize("chains,nvars,chunk", [
    (2, 5, 5), (4, 65, 64), (4, 16, 16), (4, 15, 15),
    (10381, 65, 16),      # 16 * 10381 * 808 B = 134205568: under the cap by 12160 B
    (10382, 65, 15),      # 16 * 10382 * 808 B = 134218496: over it by 768 B
    (20000, 65, 8), (200000, 3, 1)])
def test_trace_chunk(chains, nvars, chunk):
    assert lib().tp_trace_chunk(chains, nvars) == chunk
    assert 134217728 - 16 * 10381 * 808 == 12160 and 16 * 10382 * 808 - 134217728 == 768


def test_trace_tiles():
    assert [lib().tp_trace_tiles(p) for p in (1, 15, 16, 17, 64, 65)] == [1, 1, 1, 2, 4, 5]


@pytest.mark.parametrize("n,tiles,mtiles,runs", [(4096, 1, 2, []), (4097, 2, 3, [4096]), (8193, 3, 5, [4096, 8192]),
                                                 (20484, 6, 11, [4096, 8192, 16384])])
def test_summary_tiles_and_merge_passes(n, tiles, mtiles, runs):
    p = summary(n)
    assert (p["N"], p["tiles"], p["mtiles"], p["passes"], p["runs"]) == (n, tiles, mtiles, len(runs), runs)


def test_summary_chunk_and_workspace_cap():
    p = summary(12288, nvars=1000)
    assert (p["per_param"], p["pc"], p["over_cap"]) == (196608, 682, 0)          # 134217728 // 196608 = 682
    assert summary(12288, nvars=5)["pc"] == 5
    for nvars in (1, 7, 1000):
        p = summary(1 << 23, nvars=nvars)
        assert (p["per_param"], p["pc"], p["over_cap"]) == (134217728, 1, 0)
    assert summary((1 << 23) + 1)["over_cap"] == 1
    # the pooled column: chains x the kept iterations of a thinned window
    p = summary(None, chains=3, count=10, thin=3)
    assert (p["kept"], p["N"]) == (4, 12)


def test_summary_indices():
    assert summary(10, probs=(0.0, 0.055, 0.5, 0.945, 1.0))["idx"] == [0, 0, 5, 9, 9]
    assert [summary(10, hdpi=h)["hidx"] for h in (0.89, 1.0, 1e-9, 0.0, -1.0)] == [9, 10, 1, 0, 0]


@pytest.mark.parametrize("nvars,nref,thin,form,tile", [
    (10, 10, 1, FLAT, 256), (10, 10, 3, GATHER, 256),
    (704, 704, 1, DIRECT, 64),       # stride 705: 8064 // 705 = 11 staged rows, fewer than a wavefront: neither flat nor gather
    (704, 3, 1, GATHER, 256),        # flat is excluded by 2 * nref < nvars
    (704, 125, 1, GATHER, 64),       # stride 125: 8064 // 125 = 64 rows, one wavefront
    (704, 126, 1, DIRECT, 64),       # stride 127: 8064 // 127 = 63 rows -> 0: no gather kernel
    (704, 127, 1, DIRECT, 64)])
def test_predict_form_and_tile(nvars, nref, thin, form, tile):
    ft = (C.c_int * 2)()
    lib().tp_predict(nvars, nref, thin, ft)
    assert tuple(ft) == (form, tile)


def test_predict_mirrors_are_the_device_header_s_macros():
    L = lib()
    assert all(L.tp_pred_tile_mirror(s) == L.tp_pred_tile_macro(s) for s in range(1, 8200))
    assert [L.tp_pred_tile_macro(s) for s in (11, 31, 33, 125, 127, 705)] == [256, 256, 192, 64, 0, 0]
