"""A linear map of the draws on the device (csrc/device/rh_linear.hip.h: (X[:, cols] - c) W + b on the fp64 matrix cores, the rows
kept) without a GPU: the text of its block routine, compiled with the host g++ (the MFMA a chain of fma at the same lane maps) and
driven as linear_run's launch walks it (draws_plan.hpp's linear_plan), against the contract in np.longdouble.  Shapes: the kernel's
tiles are the suggested ones (64 flat rows, 64 output columns, slabs of 32 k), so n, K and M sit below, at and above those edges.

The bounds, derived (u = 2^-53, d the exact centred values, T[r][m] = sum_k |d[r][k] W[k][m]| + |offset[m]|): each staged fl(x - c) has one
rounding, which moves its term by at most u |d W|; a chain of K fused multiply-adds from +0.0 errs by at most K u sum|d W| to first
order (each step rounds a partial sum that is at most the sum of the absolute terms); the final add of offset rounds once more, by at
most u T; the second-order cross terms and the reference's own longdouble error (2^-64 per operation) stay below one further u T:
    |y - ref| <= (K + 3) u T.   A dropped or doubled k term is off by about T / K: orders above it.
sqnorm is a chain of M fused multiply-adds over the returned y, exact products: |sqnorm - sum_m y^2| <= (M + 2) u sum_m y^2 (M
roundings of partial sums, the reference's error and the second order under the other two)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rainier_amd import _capi
from tests.test_covariance_device_cpu import fixture, pooled, same_bits, shape_for, shuffled_with_duplicate, window

ROOT, LD, U53 = os.path.dirname(os.path.dirname(os.path.abspath(__file__))), np.longdouble, 2.0 ** -53
NS, KS, MS = (9, 64, 65), (1, 32, 33), (1, 65)   # a ragged row tile, a full one, a second of one row; the same of the k slabs; one ragged m tile, a second of one column
_DRIVER = r'''
#include <vector>
// linear_run's launch (csrc/draws.cpp) by its own plan, blockIdx.x decoded as rh_linear_tile_kernel decodes it; y, sqnorm: NULL where not asked for
extern "C" void rl_emulate(const double *draws, int chains, long long iterations, long long nvars, long long first, long long count, long long thin,
                           const int *cols, int K, const double *center, const double *W, int M, const double *offset, double *y, double *sqnorm) {
  const rh_plan::Linear P = rh_plan::linear_plan(chains, count, thin, K, M, y != nullptr, sqnorm != nullptr);
  std::vector<double> lds(RL_TILE_LDS);
  for (long long bid = 0; bid < P.grid; bid++) {
    const long long rt = bid / P.mgroups, g = bid - rt * P.mgroups, hi = (g + 1) * P.mper < P.mt ? (g + 1) * P.mper : P.mt;
    rl_tile(draws + first * nvars, iterations, nvars, thin, P.kept, P.N, cols, K, center, W, M, offset, rt, (int)(g * P.mper), (int)hi, lds.data(), y, sqnorm, RC_BLOCK);
  }
}
// kept, N, rt, mt, slabs, mgroups, mper, grid, y_bytes, sq_bytes
extern "C" void rl_plan(long long chains, long long count, long long thin, long long K, long long M, int want_y, int want_sq, long long *out) {
  const rh_plan::Linear P = rh_plan::linear_plan(chains, count, thin, K, M, want_y != 0, want_sq != 0);
  const long long v[10] = {P.kept, P.N, P.rt, P.mt, P.slabs, P.mgroups, P.mper, P.grid, P.y_bytes, P.sq_bytes};
  for (int i = 0; i < 10; i++) out[i] = v[i];
}
'''
_emu = None


def emulation():
    """draws_plan.hpp (which brings rh_cov.hip.h and rh_linear.hip.h in host mode) + the driver above as a host shared library"""
    global _emu
    if _emu is None:
        d = tempfile.mkdtemp(prefix="rh_linear_emu")
        src, so = os.path.join(d, "emu.cpp"), os.path.join(d, "emu.so")
        open(src, "w").write('#include "%s"\n%s' % (os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp"), _DRIVER))
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-shared", "-fPIC", src, "-o", so])
        _emu = C.CDLL(so)
        ll, dp, ip = C.c_longlong, C.POINTER(C.c_double), C.POINTER(C.c_int)
        _emu.rl_emulate.argtypes = [dp, C.c_int, ll, ll, ll, ll, ll, ip, C.c_int, dp, dp, C.c_int, dp, dp, dp]
        _emu.rl_plan.argtypes = [ll] * 5 + [C.c_int, C.c_int, C.POINTER(ll)]
    return _emu


def emulate(x, W, center=None, offset=None, cols=None, first=0, count=None, thin=1, y=True, sqnorm=True):
    """the host emulation over x [chains][iterations][nvars] -> (y [chains][kept][M] or None, sqnorm [chains][kept] or None)"""
    x, W = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(W, dtype=np.float64)
    count = x.shape[1] - first if count is None else count
    kept, (k, m) = -(-count // thin), W.shape
    sel = np.ascontiguousarray(range(k) if cols is None else cols, dtype=np.int32)
    ctr = np.zeros(k) if center is None else np.ascontiguousarray(center, dtype=np.float64)   # as rh_linear_create hands "none" to the device
    off = None if offset is None else np.ascontiguousarray(offset, dtype=np.float64)
    oy, osq = np.full((x.shape[0], kept, m), -1.0) if y else None, np.full((x.shape[0], kept), -1.0) if sqnorm else None
    ptr = lambda a: None if a is None else _capi.dptr(a)
    emulation().rl_emulate(_capi.dptr(x), x.shape[0], x.shape[1], x.shape[2], first, count, thin, sel.ctypes.data_as(C.POINTER(C.c_int)), k, _capi.dptr(ctr),
                           _capi.dptr(W), m, ptr(off), ptr(oy), ptr(osq))
    return oy, osq


def case(n, k, m, thin):
    """draws of the covariance tests' kinds [chains][iters][k + 2], a map over k of its columns in an order of its own, the window"""
    chains, kept = shape_for(n)
    first, count, iters = window(kept, thin)
    rng = np.random.default_rng(1000 * n + 10 * k + m + thin)
    x = fixture(chains, iters, k + 2, 7 * n + 31 * k + m + thin)
    cols = [int(c) for c in rng.permutation(k + 2)[:k]]
    center = x[:, first:first + count:thin, cols].mean(axis=(0, 1)) + 0.01 * rng.standard_normal(k)
    lmap = dict(W=rng.standard_normal((k, m)), center=center, offset=None if k == 1 else rng.standard_normal(m), cols=cols)   # K = 1: no offset
    return x, lmap, dict(first=first, count=count, thin=thin)


def check_bounds(rows, lmap, y, sq, what):
    """rows [N][K]: the pooled, selected draws; y [N][M], sq [N]: the module's two bounds"""
    k, m = lmap["W"].shape
    d, w = rows.astype(LD) - lmap["center"].astype(LD), lmap["W"].astype(LD)
    b = np.zeros(m, dtype=LD) if lmap["offset"] is None else lmap["offset"].astype(LD)
    err, bound = np.abs(y.astype(LD) - (d @ w + b)), LD((k + 3) * U53) * (np.abs(d) @ np.abs(w) + np.abs(b))
    assert np.all(err <= bound), (what, "y", np.argwhere(~(err <= bound))[:4].ravel(), float(np.max(err - bound)))
    t = (y.astype(LD) ** 2).sum(axis=1)
    assert np.all(np.abs(sq.astype(LD) - t) <= LD((m + 2) * U53) * t), (what, "sqnorm")


def check_properties(run, x, lmap, at, what):
    """run(x, **map, **window, y=, sqnorm=) -> (y, sqnorm), the emulation or the device: the bounds, then what must not change a bit"""
    k, m = lmap["W"].shape
    y, sq = run(x, **lmap, **at)
    n = y.shape[0] * y.shape[1]
    check_bounds(pooled(x, cols=lmap["cols"], **at), lmap, y.reshape(n, m), sq.reshape(n), what)                     # 1, 2: against np.longdouble
    assert same_bits(run(x, y=False, **lmap, **at)[1], sq), (what, "sqnorm alone")                                   # 3. sqnorm alone (Y stays on chip), y alone
    assert same_bits(run(x, sqnorm=False, **lmap, **at)[0], y), (what, "y alone: the m tiles in workgroups of their own")
    again = run(x, **lmap, **at)
    assert same_bits(again[0], y) and same_bits(again[1], sq), (what, "a repeat")
    pick = shuffled_with_duplicate(k, sum(what[:3]))                                                                  # rows of the map, shuffled, one twice ...
    sub = dict(W=lmap["W"][pick], center=lmap["center"][pick], offset=lmap["offset"], cols=[lmap["cols"][i] for i in pick])
    gathered = np.ascontiguousarray(x[:, :, sub["cols"]])                                                             # ... against a buffer that holds those columns in that order
    for u, v in zip(run(x, **sub, **at), run(gathered, **dict(sub, cols=None), **at)):
        assert same_bits(u, v), (what, "a shuffled column list with a duplicate")
    zero = dict(lmap, center=np.zeros(k))
    for u, v in zip(run(x, **dict(lmap, center=None), **at), run(x, **zero, **at)):
        assert same_bits(u, v), (what, "center None")
    c, j = x.shape[0] // 2, y.shape[1] // 2                                                                           # 4. a NaN in one selected value: that flat row alone
    xn = x.copy()
    xn[c, at["first"] + j * at["thin"], lmap["cols"][k // 2]] = np.nan
    yn, sqn = run(xn, **lmap, **at)
    assert np.isnan(yn[c, j]).all() and np.isnan(sqn[c, j]), (what, "the NaN row")
    yn[c, j], sqn[c, j] = y[c, j], sq[c, j]
    assert same_bits(yn, y) and same_bits(sqn, sq), (what, "every other row")
    return y, sq


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_emulation_within_the_derived_bounds_and_invariant(n, k, m):
    for thin in (1, 3):
        check_properties(emulate, *case(n, k, m, thin), (n, k, m, thin))


def test_plan_exports_and_refusals():
    import rainier_amd as R
    L, out, big, top = _capi.lib(), (C.c_longlong * 10)(), (1 << 31) - 1, (1 << 63) - 1
    plan = lambda *a: (emulation().rl_plan(*a, out), list(out))[1]
    assert plan(4, 5000, 3, 33, 129, 1, 0) == [1667, 6668, 105, 3, 2, 3, 1, 315, 6668 * 129 * 8, 0]      # few row tiles, no sqnorm: a workgroup per m tile
    assert plan(4, 5000, 3, 33, 129, 0, 1) == [1667, 6668, 105, 3, 2, 1, 3, 105, 0, 6668 * 8]            # sqnorm: one workgroup walks a row tile's m tiles
    assert plan(1024, 1000, 1, 64, 1024, 1, 0) == [1000, 1024000, 16000, 16, 2, 1, 16, 16000, 1024000 * 1024 * 8, 0]
    assert plan(big, big, 1, 4096, 4096, 1, 1)[-2:] == [top, top]                                        # the bytes saturate
    names = ("rh_linear_create", "rh_linear_destroy", "rh_linear_nout", "rh_linear_device", "rh_sampler_linear", "rh_linear_lower_only")
    assert all(name in _capi.EXPORTS and hasattr(L, name) for name in names) and L.rh_abi_version() == 6
    assert b"rh_linear_tile_kernel" in _capi.linear_lower_only("gfx950")                                 # built, and judged as before a launch
    assert R.Mahalanobis._fields == ("d2", "mean", "cov", "cols")
    w, buf, h, ip = np.ones(4097), np.zeros(64), C.c_void_p(), C.POINTER(C.c_int32)
    said = lambda word: word in L.rh_last_error(None).decode()
    for kw, word in ((dict(W=None), "NULL"), (dict(K=0), "K and M"), (dict(K=4097), "K and M"), (dict(M=0), "K and M"), (dict(M=4097), "K and M"), (dict(cols=[0, -1]), "cols[1]")):
        a = dict(dict(W=_capi.dptr(w), K=2, M=1, cols=None), **kw)
        cols = None if a["cols"] is None else np.array(a["cols"], dtype=np.int32).ctypes.data_as(ip)
        assert L.rh_linear_create(a["W"], a["K"], a["M"], None, None, cols, -1, C.byref(h)) == _capi.RH_E_INVALID and said(word) and not h, kw
    lmap = R.LinearMap(np.ones((2, 3)), cols=[0, 4])
    assert lmap.nout == 3 and L.rh_linear_nout(None) == -1

    def call(h=lmap._h, ptr=C.c_void_p(4096), nvars=5, first=0, count=10, thin=1, outs=(1, 0, 1, 0)):   # (the pointer is never dereferenced)
        hy, dy, hs, ds = [o or None for o in (outs[0] and _capi.dptr(buf), outs[1] and C.byref(C.c_void_p()), outs[2] and _capi.dptr(buf), outs[3] and C.byref(C.c_void_p()))]
        return L.rh_linear_device(h, ptr, 0, 4, 10, nvars, first, count, thin, hy, dy, hs, ds)
    for kw, word in ((dict(h=None), "NULL"), (dict(ptr=None), "NULL"), (dict(nvars=4), "cols[1]"), (dict(count=11), "window"), (dict(first=-1), "window"),
                     (dict(thin=0), "window"), (dict(count=0), "window"), (dict(outs=(0,) * 4), "all NULL")):
        assert call(**kw) == _capi.RH_E_INVALID and said(word), kw                                       # the message names the argument
    assert L.rh_sampler_linear(None, lmap._h, 0, 10, 1, _capi.dptr(buf), None, None, None) == _capi.RH_E_INVALID
    if L.rh_device_count() == 0:
        assert call() == call(outs=(0, 1, 0, 0)) == _capi.RH_E_DEVICE and said("no CPU fallback")
    lmap.close()
