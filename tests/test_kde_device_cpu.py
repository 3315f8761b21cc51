"""Kernel density estimates on the device (csrc/device/rh_kde.hip.h) without a GPU: the text of its block routines, compiled with the
host g++ (the MFMA a chain of fma at the same lane maps) and driven as kde_run's and kde_pairs_run's launches walk them (the workspace
cap a parameter), against the contract evaluated in np.longdouble.  Tolerance, derived: every term is >= 0, so a 4096-long add chain
plus S split adds err by at most (4096 + S) 2^-53 relative; a term's own error is about (t + 4) 2^-52 with t = z^2 / 2 <= 745 per axis
(the argument's error amplified by t, exp within 1 ulp); two axes stay below 8e-13: |got - ref| <= 1e-12 ref + 1e-300."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rainier_amd import _capi

ROOT, LD = os.path.dirname(os.path.dirname(os.path.abspath(__file__))), np.longdouble
_DRIVER = r'''
#include <vector>
// kde_run's and kde_pairs_run's launches (csrc/draws.cpp) by their own plans, blockIdx.x decoded as the kernels decode it -> chunks, -1 beyond the cap
extern "C" int kd_curves(const double *draws, int chains, long long iterations, long long nvars, long long first, long long count, long long thin,
                         const int *cols, int K, int G, const double *range, const double *bw, long long cap, double *grid, double *density) {
  const rh_plan::Kde P = rh_plan::kde_plan(chains, count, thin, K, G, cap);
  if (P.over_cap) return -1;
  std::vector<double> ws((size_t)(P.pc * P.S * G), std::nan("")), lds(RKD_ROWS);
  for (int k = 0; k < K; k++) rh_plan::kde_grid(range[2 * k], range[2 * k + 1], G, grid + (long long)k * G);
  int chunks = 0;
  for (long long k0 = 0; k0 < K; k0 += P.pc, chunks++) {
    const long long p_cnt = P.pc < K - k0 ? P.pc : K - k0;
    for (long long bid = 0; bid < p_cnt * P.S * P.gtiles; bid++) {
      const long long cs = bid / P.gtiles, kl = cs / P.S, s = cs - kl * P.S;
      rkd_point_split(draws + first * nvars, iterations, nvars, thin, P.kept, P.N, cols[k0 + kl], grid + (k0 + kl) * G, G, bw[k0 + kl],
                      (int)(bid - cs * P.gtiles) * RKD_GT, s, lds.data(), ws.data() + (kl * P.S + s) * G, RC_BLOCK);
    }
    for (long long e = 0; e < p_cnt * G; e++) density[k0 * G + e] = rkd_point_finish(ws.data() + e / G * P.S * G, P.S, G, (int)(e % G), P.N, bw[k0 + e / G]);
  }
  return chunks;
}
extern "C" int kd_surfaces(const double *draws, int chains, long long iterations, long long nvars, long long first, long long count, long long thin,
                           const int *pairs, int np, int npx, int npy, const double *range, const double *bw, long long cap, double *xg, double *yg,
                           double *density) {
  const rh_plan::KdePairs P = rh_plan::kde_pairs_plan(chains, count, thin, np, npx, npy, cap);
  if (P.over_cap) return -1;
  std::vector<double> ws((size_t)(P.uc * P.S * RC_TC * RC_TC), std::nan("")), lds(RC_TILE_LDS);
  for (int p = 0; p < np; p++) {
    rh_plan::kde_grid(range[4 * p], range[4 * p + 1], npx, xg + (long long)p * npx);
    rh_plan::kde_grid(range[4 * p + 2], range[4 * p + 3], npy, yg + (long long)p * npy);
  }
  int chunks = 0, p, ti, tj;
  for (long long u0 = 0; u0 < P.units; u0 += P.uc, chunks++) {
    const long long u_cnt = P.uc < P.units - u0 ? P.uc : P.units - u0;
    for (long long bid = 0; bid < u_cnt * P.S; bid++) {
      rkd_unit_of(u0 + bid / P.S, (int)P.tx, (int)P.ty, &p, &ti, &tj);
      rkd_tile_split(draws + first * nvars, iterations, nvars, thin, P.kept, P.N, pairs[2 * p], pairs[2 * p + 1], xg + (long long)p * npx,
                     yg + (long long)p * npy, npx, npy, bw[2 * p], bw[2 * p + 1], ti, tj, bid % P.S, lds.data(), ws.data() + bid * RC_TC * RC_TC, RC_BLOCK);
    }
    for (long long ul = 0; ul < u_cnt; ul++) {
      rkd_unit_of(u0 + ul, (int)P.tx, (int)P.ty, &p, &ti, &tj);
      rkd_tile_finish(ws.data() + ul * P.S * RC_TC * RC_TC, P.S, P.N, ti, tj, npx, npy, bw[2 * p], bw[2 * p + 1], density + (long long)p * npx * npy, RC_BLOCK);
    }
  }
  return chunks;
}
extern "C" long long kd_grid_tile() { return RKD_GT; }
'''
_emu, _cases = None, {}


def emulation():
    """draws_plan.hpp (which brings rh_cov.hip.h and rh_kde.hip.h in host mode) + the driver above as a host shared library"""
    global _emu
    if _emu is None:
        d = tempfile.mkdtemp(prefix="rh_kde_emu")
        src, so = os.path.join(d, "emu.cpp"), os.path.join(d, "emu.so")
        open(src, "w").write('#include "%s"\n%s' % (os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp"), _DRIVER))
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-shared", "-fPIC", src, "-o", so])
        _emu = C.CDLL(so)
        ll, dp, ip = C.c_longlong, C.POINTER(C.c_double), C.POINTER(C.c_int)
        _emu.kd_curves.argtypes = [dp, C.c_int, ll, ll, ll, ll, ll, ip, C.c_int, C.c_int, dp, dp, ll, dp, dp]
        _emu.kd_surfaces.argtypes = [dp, C.c_int, ll, ll, ll, ll, ll, ip, C.c_int, C.c_int, C.c_int, dp, dp, ll, dp, dp, dp]
        _emu.kd_grid_tile.restype = ll
    return _emu


def emulate(c, sel, rng, bw, cap=0):
    """the host emulation of case c over the columns resp. pairs `sel` -> (grids.., density, chunks)"""
    x, sel = c["x"], np.ascontiguousarray(sel, dtype=np.int32)
    rng, bw = np.ascontiguousarray(rng, dtype=np.float64), np.ascontiguousarray(bw, dtype=np.float64)
    at = (_capi.dptr(x), x.shape[0], x.shape[1], x.shape[2], c["first"], c["count"], c["thin"], sel.ctypes.data_as(C.POINTER(C.c_int)), len(sel))
    if c["form"] == "curves":
        grid, dens = np.zeros((len(sel), c["points"])), np.full((len(sel), c["points"]), -1.0)
        return grid, dens, emulation().kd_curves(*at, c["points"], _capi.dptr(rng), _capi.dptr(bw), cap or 128 << 20, _capi.dptr(grid), _capi.dptr(dens))
    (npx, npy) = c["points"]
    xg, yg, dens = np.zeros((len(sel), npx)), np.zeros((len(sel), npy)), np.full((len(sel), npx, npy), -1.0)
    return xg, yg, dens, emulation().kd_surfaces(*at, npx, npy, _capi.dptr(rng), _capi.dptr(bw), cap or 128 << 20, _capi.dptr(xg), _capi.dptr(yg), _capi.dptr(dens))


def grid_of(lo, hi, g):
    e = lo + (np.arange(g, dtype=np.float64) * (hi - lo)) / np.float64(g - 1)
    e[0], e[-1] = lo, hi
    return e


def phi(x, lo, hi, g, h):
    with np.errstate(all="ignore"):
        z = (grid_of(lo, hi, g).astype(LD)[:, None] - x.astype(LD)[None, :]) / LD(h)
        return np.exp(-0.5 * z * z)


def reference(c):
    """the contract in np.longdouble: one curve per column of c["ref"], resp. one surface per pair"""
    w = c["x"][:, c["first"]:c["first"] + c["count"]:c["thin"], :].reshape(-1, c["x"].shape[2])
    n, pi = LD(len(w)), 4 * np.arctan(LD(1))
    with np.errstate(all="ignore"):
        if c["form"] == "curves":
            return {k: phi(w[:, k], *c["range"][k], c["points"], c["bw"][k]).sum(axis=1) / (n * LD(c["bw"][k]) * np.sqrt(2 * pi)) for k in c["ref"]}
        return [phi(w[:, a], *r[0], c["points"][0], h[0]).dot(phi(w[:, b], *r[1], c["points"][1], h[1]).T) / (n * 2 * pi * LD(h[0]) * LD(h[1]))
                for (a, b), r, h in zip(c["sel"], c["range"], c["bw"])]


def close(got, ref):
    nan = np.isnan(ref)
    return np.array_equal(np.isnan(got), nan) and bool(np.all(np.abs(got[~nan].astype(LD) - ref[~nan]) <= LD(1e-12) * ref[~nan] + LD(1e-300)))


# the seven columns: 0 normal, 1 normal about 1000, 2 ties, 3 constant, 4 one +inf and one -inf, 5 a NaN inside the window, 6 NaN only outside it
COL_RANGE = [(-4.5, 4.5), (990.0, 1010.0), (-7.0, 7.5), (1.0, 3.0), (-3.0, 3.0), (-4.0, 4.0), (-5.0, 3.0)]
COL_BW = [0.3, 0.05, 0.4, 0.25, 0.2, 0.3, 0.01]
CURVES, SURFACES = ("one", "ragged", "tile", "thin", "maxpoints", "chunks"), ("pone", "pragged", "pmax")


def case(name):
    """name -> dict(form, x, first, count, thin, points, sel (the column list resp. the pairs), range, bw (curves: per column of x; surfaces:
    per pair), ref (curves: the columns held to the reference), cap (CPU tier, 0: the header's), want = the reference), built once"""
    if name not in _cases:
        gt = int(emulation().kd_grid_tile())
        chains, count, thin, nvars, first, points, sel, cap = {
            "one": (1, 1, 1, 1, 0, 2, [0], 0), "ragged": (3, 1367, 1, 7, 2, 67, [5, 0, 5, 2], 0), "tile": (3, 1367, 1, 7, 2, gt + 1, [5, 0, 5, 2], 0),
            "thin": (2, 50, 3, 2, 1, 16, [1], 0), "maxpoints": (2, 20, 1, 1, 0, 4096, [0], 0), "chunks": (2, 30, 1, 3, 0, 8, [2, 1], 2 * 8 * 8),
            "pone": (1, 1, 1, 1, 0, (2, 2), [(0, 0)], 0), "pragged": (3, 1367, 1, 7, 2, (65, 17), [(0, 1), (1, 0), (2, 2), (0, 5)], 3 * 2 * 32768),
            "pmax": (2, 3, 1, 2, 0, (256, 256), [(0, 1)], 0)}[name]
        x = np.random.default_rng(len(name) + 11 * chains).standard_normal((chains, first + count + 3, nvars))
        rng, bw = [(-4.0, 4.0 + k) for k in range(nvars)], [0.3 + 0.1 * k for k in range(nvars)]
        if nvars == 7:
            rng, bw = COL_RANGE, COL_BW
            x[:, :, 1] = 1000.0 + 0.8 * x[:, :, 0] + 0.6 * x[:, :, 1]
            x[:, :, 2] = np.round(2.0 * x[:, :, 2])
            x[:, :, 3] = 2.0
            x[1, first + 5, 4], x[2, first, 4] = np.inf, -np.inf
            x[1, first + 100, 5], x[0, first - 1, 6], x[2, first + count, 6] = np.nan, np.nan, np.nan
        c = dict(form="surfaces" if name[0] == "p" else "curves", x=x, first=first, count=count, thin=thin, points=points, sel=sel, cap=cap)
        if c["form"] == "curves":
            c.update(range=rng, bw=bw, ref=sorted(set(sel)) if name == "tile" else list(range(nvars)))
        else:
            c.update(range=[(rng[a], rng[b]) for a, b in sel], bw=[(bw[a], bw[b]) for a, b in sel])
        c["want"] = reference(c)
        _cases[name] = c
    return _cases[name]


@pytest.mark.parametrize("name", CURVES)
def test_curves_emulation_equals_the_longdouble_reference(name):
    c = case(name)
    nvars, g = c["x"].shape[2], c["points"]
    grid, dens, chunks = emulate(c, range(nvars), c["range"], c["bw"], c["cap"])
    for k in c["ref"]:
        assert np.array_equal(grid[k], grid_of(*c["range"][k], g)) and close(dens[k], c["want"][k]), (name, k)
    sub = emulate(c, c["sel"], [c["range"][k] for k in c["sel"]], [c["bw"][k] for k in c["sel"]], c["cap"])
    assert np.array_equal(sub[1], dens[c["sel"]], equal_nan=True) and np.array_equal(sub[0], grid[c["sel"]])       # the bits of the all-columns call
    assert np.array_equal(emulate(c, range(nvars), c["range"], c["bw"])[1], dens, equal_nan=True)                  # ... and of one chunk
    assert name != "chunks" or (chunks == 2 and sub[2] == 1)


@pytest.mark.parametrize("name", SURFACES)
def test_surfaces_emulation_equals_the_longdouble_reference(name):
    c = case(name)
    npx, npy = c["points"]
    xg, yg, dens, chunks = emulate(c, c["sel"], c["range"], c["bw"], c["cap"])
    for p, (r, want) in enumerate(zip(c["range"], c["want"])):
        assert np.array_equal(xg[p], grid_of(*r[0], npx)) and np.array_equal(yg[p], grid_of(*r[1], npy)) and close(dens[p], want), (name, p)
    assert np.array_equal(emulate(c, c["sel"], c["range"], c["bw"])[2], dens, equal_nan=True)                      # one chunk: the same bits
    if name == "pragged":
        assert chunks == 3 and np.all(np.isnan(dens[3])) and not np.isnan(dens[:3]).any()
        turned = emulate(dict(c, points=(npy, npx)), [(1, 0)], [c["range"][0][::-1]], [c["bw"][0][::-1]])[2]       # (1, 0) on the turned grid: the transpose
        assert close(turned[0], c["want"][0].T)


def test_exports_code_object_and_refusals():
    import rainier_amd as R
    L = _capi.lib()
    names = ("rh_sampler_kde", "rh_kde_device", "rh_sampler_kde_pairs", "rh_kde_pairs_device", "rh_kde_lower_only")
    assert all(name in _capi.EXPORTS and hasattr(L, name) for name in names) and L.rh_abi_version() == 6
    assert R.Kde._fields == ("cols", "grid", "density", "bw") and R.KdePairs._fields == ("pairs", "xgrid", "ygrid", "density", "bw")
    assert b"rh_kde_tile_kernel" in _capi.kde_lower_only("gfx950")                                  # built, and judged as before a launch
    out, ip, nan, inf = np.zeros(2 * 4097), C.POINTER(C.c_int32), float("nan"), float("inf")
    d = lambda a: _capi.dptr(np.ascontiguousarray(a, dtype=np.float64)) if a is not None else None

    def curves(ptr=C.c_void_p(4096), chains=4, iters=10, first=0, count=10, thin=1, cols=None, g=16, rng=((0, 1), (0, 1)), bw=(1, 1), grid=out, dens=out):
        sel = np.array(cols, dtype=np.int32) if cols is not None else None                           # the pointer is never dereferenced
        return L.rh_kde_device(ptr, 0, chains, iters, 2, first, count, thin, sel.ctypes.data_as(ip) if cols is not None else None, len(cols or ()), g,
                               d(rng), d(bw), d(grid), d(dens))

    def surfaces(ptr=C.c_void_p(4096), chains=4, iters=10, first=0, count=10, pairs=((0, 1),), npx=8, npy=8, rng=((0, 1), (0, 1)), bw=(1, 1), xg=out, dens=out):
        pr = np.array(pairs, dtype=np.int32) if pairs is not None else None
        return L.rh_kde_pairs_device(ptr, 0, chains, iters, 2, first, count, 1, pr.ctypes.data_as(ip) if pairs is not None else None, len(pairs or ()), npx, npy,
                                     d(rng), d(bw), d(xg), d(out), d(dens))
    for kw in (dict(ptr=None), dict(rng=None), dict(bw=None), dict(grid=None), dict(dens=None), dict(g=1), dict(g=4097), dict(bw=(1, 0)), dict(bw=(-1, 1)),
               dict(bw=(nan, 1)), dict(bw=(1, inf)), dict(rng=((1, 0), (0, 1))), dict(rng=((0, 1), (0, inf))), dict(rng=((nan, 1), (0, 1))), dict(count=0),
               dict(first=-1), dict(first=5, count=6), dict(thin=0), dict(cols=[2]), dict(cols=[0, -1]), dict(chains=0)):
        assert curves(**kw) == _capi.RH_E_INVALID, kw
        assert {"rng": "range", "bw": "bw", "grid": "grid", "dens": "density", "g": "npoints"}.get(next(iter(kw)), "") in L.rh_last_error(None).decode()   # the message names the argument
    for kw in (dict(ptr=None), dict(pairs=None), dict(rng=None), dict(bw=None), dict(xg=None), dict(dens=None), dict(npx=1), dict(npx=257), dict(npy=257),
               dict(bw=(1, 0)), dict(bw=(nan, 1)), dict(rng=((0, 1), (1, 0))), dict(rng=((0, 1), (-inf, 1))), dict(count=11), dict(pairs=((0, 2),)), dict(chains=0)):
        assert surfaces(**kw) == _capi.RH_E_INVALID, kw
    assert L.rh_sampler_kde(None, 0, 10, 1, None, 0, 16, *[d(out)] * 4) == L.rh_sampler_kde_pairs(None, 0, 10, 1, None, 0, 8, 8, *[d(out)] * 5) == _capi.RH_E_INVALID
    assert curves(chains=4096, iters=8192, count=8192, g=4096) == _capi.RH_E_UNSUPPORTED and "workspace" in L.rh_last_error(None).decode()
    assert curves(chains=(1 << 31) - 1, iters=(1 << 31) - 1, count=(1 << 31) - 1, g=4096) == _capi.RH_E_UNSUPPORTED   # the plan's products saturate
    if L.rh_device_count() == 0:
        assert curves() == _capi.RH_E_DEVICE and surfaces() == _capi.RH_E_DEVICE and "no CPU fallback" in L.rh_last_error(None).decode()


def test_bandwidth_rules_and_default_ranges():
    from rainier_amd.sampler import _kde_rules
    sd, q = np.array([2.0, 3.0, 0.5, 0.0]), np.array([[-5.0, -1.0, 1.0, 6.0], [0.0, 1.0, 9.0, 10.0], [1.0, 2.0, 2.0, 3.0], [7.0, 7.0, 7.0, 7.0]])
    fig, n = lambda: (sd, q), 1000
    h, r = _kde_rules("silverman", None, 3.0, n, 1, [1, 0, 2], fig, "kde")
    want = 0.9 * np.array([3.0, 2.0 / 1.349, 0.5]) * n ** -0.2                                       # sd < IQR / 1.349; IQR / 1.349 < sd; IQR == 0: sd alone
    assert np.allclose(h, want, rtol=1e-15) and np.allclose(r, np.stack([q[[1, 0, 2], 0] - 3.0 * want, q[[1, 0, 2], 3] + 3.0 * want], axis=1), rtol=1e-15)
    h, r = _kde_rules("scott", np.array([[np.nan, 4.0], [-1.0, 1.0]]), 2.0, n, 2, [0, 1], fig, "kde_pairs")
    assert np.allclose(h, sd[:2] * n ** (-1.0 / 6.0), rtol=1e-15) and np.array_equal(r, [[-5.0 - 2.0 * h[0], 4.0], [-1.0, 1.0]])
    for rule in ("silverman", "scott"):
        with pytest.raises(ValueError, match="column 3.*bw explicitly"):                              # a constant column
            _kde_rules(rule, None, 3.0, n, 1, [0, 3], fig, "kde")
