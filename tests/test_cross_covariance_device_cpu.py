"""Cross-covariance of two draw sets on the device (csrc/device/rh_xcov.hip.h: A^T B of the centred rows on the fp64 matrix cores)
without a GPU: the text of its block routines, compiled with the host g++ (the MFMA a chain of fma at the same lane maps) and driven
as cross_covariance_run's launches walk them (the workspace cap a parameter), against the contract in np.longdouble.

The bound, derived (u = 2^-53, d the exact centred values, T = sum_r |dA dB|, n = min(N, 4096) rows of a split): the returned mean is
m + e, |e| <= E = (N + 2) u sum|x| / N (the covariance test's mean term: N - 1 adds in any order, the division); sum_r (dA - eA)(dB - eB)
= sum_r dA dB + N eA eB exactly (exact deviations sum to zero), so the means' rounding enters in second order, by at most N EA EB; each
staged fl(x - m^) has one rounding (2 u T), a chain of n fused multiply-adds errs by at most n u T, the S - 1 adds of the splits by
S u T, the division by u T; their cross terms and the reference's own error (longdouble products, pairwise sums) stay below the last u T:
    |cross - ref| <= ((n + S + 4) u T + N EA EB) / (N - 1).   A dropped or doubled row is off by about T / N: eight orders above it."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rainier_amd import _capi
from tests.test_covariance_device_cpu import emulate as cov_emulate, fixture, pooled, same_bits, shape_for, shuffled_with_duplicate, window

ROOT, LD, U53, CAP = os.path.dirname(os.path.dirname(os.path.abspath(__file__))), np.longdouble, 2.0 ** -53, 128 << 20
same_results = lambda x, y: all(same_bits(u, v) for u, v in zip(x, y))
NS, KAS, KBS = (9, 4096, 4097), (1, 17, 33), (1, 129)   # a ragged slab, a full split, a second split of one row; one sub-tile, two, two A tiles; one and two B tiles
_DRIVER = r'''
#include <vector>
// cross_covariance_run's launches (csrc/draws.cpp) by its own plan, blockIdx.x decoded as the kernels decode it -> chunks, -1 beyond the cap
// out: mean_a [Ka], mean_b [Kb], var_a [Ka], var_b [Kb], cross [Ka][Kb], corr [Ka][Kb]
extern "C" int rx_emulate(const double *a, long long na, const double *b, long long nb, int chains, long long iterations, long long first, long long count,
                          long long thin, const int *cols_a, int Ka, const int *cols_b, int Kb, long long cap, double *out) {
  const rh_plan::CrossCovariance P = rh_plan::cross_covariance_plan(chains, count, thin, Ka, Kb, cap);
  if (P.over_cap) return -1;
  const long long tile = RX_TA * RX_TB;
  std::vector<double> part((size_t)(P.S * (Ka > Kb ? Ka : Kb))), ws((size_t)(P.pc * P.S * tile), std::nan("")), lds(RX_TILE_LDS);
  double *mean[2] = {out, out + Ka}, *var[2] = {out + Ka + Kb, out + 2 * Ka + Kb}, *cross = out + 2 * (Ka + Kb), *corr = cross + (long long)Ka * Kb;
  const rx_src src[2] = {{a + first * na, iterations, na, thin}, {b + first * nb, iterations, nb, thin}};
  for (int q = 0; q < 2; q++) {
    const int *cols = q ? cols_b : cols_a;
    const int K = q ? Kb : Ka, ctiles = (K + RC_TC - 1) / RC_TC;
    for (long long bid = 0; bid < P.S * ctiles; bid++)
      rc_mean_split(src[q].base, iterations, src[q].ncols, thin, P.kept, P.N, cols, K, (int)(bid % ctiles) * RC_TC, bid / ctiles, lds.data(), part.data(), RC_BLOCK);
    for (int k = 0; k < K; k++) mean[q][k] = rc_mean_finish(part.data(), P.S, K, k, P.N);
    for (long long bid = 0; bid < P.S * ctiles; bid++)
      rx_var_split(src[q], P.kept, P.N, cols, K, mean[q], (int)(bid % ctiles) * RC_TC, bid / ctiles, lds.data(), part.data(), RC_BLOCK);
    for (int k = 0; k < K; k++) var[q][k] = rx_var_finish(part.data(), P.S, K, k, P.N);
  }
  int chunks = 0;
  for (long long p0 = 0; p0 < P.pairs; p0 += P.pc, chunks++) {
    const long long p_cnt = P.pc < P.pairs - p0 ? P.pc : P.pairs - p0;
    for (long long bid = 0; bid < p_cnt * P.S; bid++) {
      const long long p = p0 + bid / P.S;
      rx_tile_split(src[0], src[1], P.kept, P.N, cols_a, Ka, cols_b, Kb, mean[0], mean[1], (int)(p / P.tb), (int)(p % P.tb), bid % P.S, lds.data(),
                    ws.data() + bid * tile, RC_BLOCK);
    }
    for (long long pl = 0; pl < p_cnt; pl++)
      rx_finish_pair(ws.data() + pl * P.S * tile, P.S, P.N, (int)((p0 + pl) / P.tb), (int)((p0 + pl) % P.tb), Ka, Kb, cross, RC_BLOCK);
  }
  for (long long e = 0; e < (long long)Ka * Kb; e++) corr[e] = rx_corr_entry(cross, var[0], var[1], Kb, e / Kb, e % Kb);
  return chunks;
}
// kept, N, S, ta, tb, pairs, per_pair, pc, over_cap
extern "C" void rx_plan(long long chains, long long count, long long thin, long long Ka, long long Kb, long long *out) {
  const rh_plan::CrossCovariance P = rh_plan::cross_covariance_plan(chains, count, thin, Ka, Kb);
  const long long v[9] = {P.kept, P.N, P.S, P.ta, P.tb, P.pairs, P.per_pair, P.pc, P.over_cap ? 1 : 0};
  for (int i = 0; i < 9; i++) out[i] = v[i];
}
'''
_emu = None


def emulation():
    """draws_plan.hpp (which brings rh_cov.hip.h and rh_xcov.hip.h in host mode) + the driver above as a host shared library"""
    global _emu
    if _emu is None:
        d = tempfile.mkdtemp(prefix="rh_xcov_emu")
        src, so = os.path.join(d, "emu.cpp"), os.path.join(d, "emu.so")
        open(src, "w").write('#include "%s"\n%s' % (os.path.join(ROOT, "rainier_amd", "csrc", "draws_plan.hpp"), _DRIVER))
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-shared", "-fPIC", src, "-o", so])
        _emu = C.CDLL(so)
        ll, dp, ip = C.c_longlong, C.POINTER(C.c_double), C.POINTER(C.c_int)
        _emu.rx_emulate.argtypes = [dp, ll, dp, ll, C.c_int, ll, ll, ll, ll, ip, C.c_int, ip, C.c_int, ll, dp]
        _emu.rx_plan.argtypes = [ll] * 5 + [C.POINTER(ll)]
    return _emu


def emulate(a, b, first=0, count=None, thin=1, cols_a=None, cols_b=None, cap=CAP):
    """the host emulation over a [chains][iterations][na], b [chains][iterations][nb] -> (mean_a, mean_b, var_a, var_b, cross, corr), chunks"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    sa = np.ascontiguousarray(range(a.shape[2]) if cols_a is None else cols_a, dtype=np.int32)
    sb = np.ascontiguousarray(range(b.shape[2]) if cols_b is None else cols_b, dtype=np.int32)
    ka, kb, ip = len(sa), len(sb), C.POINTER(C.c_int)
    out = np.full(2 * (ka + kb) + 2 * ka * kb, -1.0)
    chunks = emulation().rx_emulate(_capi.dptr(a), a.shape[2], _capi.dptr(b), b.shape[2], a.shape[0], a.shape[1], first, a.shape[1] - first if count is None else count,
                                    thin, sa.ctypes.data_as(ip), ka, sb.ctypes.data_as(ip), kb, cap, _capi.dptr(out))
    parts = np.split(out, np.cumsum([ka, kb, ka, kb, ka * kb]))
    return tuple(parts[:4]) + (parts[4].reshape(ka, kb), parts[5].reshape(ka, kb)), chunks


def two_fixtures(n, ka, kb, thin):
    """a [chains][iters][ka] and b [chains][iters][kb] of the covariance tests' kinds, every fourth column of b moving with a's first; the window"""
    chains, kept = shape_for(n)
    first, count, iters = window(kept, thin)
    a, b = fixture(chains, iters, ka, 7 * n + 31 * ka + thin), fixture(chains, iters, kb, 11 * n + 13 * kb + thin)
    b[:, :, ::4] += 0.7 * a[:, :, :1]
    return a, b, first, count


def check_bounds(ra, rb, got, what):
    """ra [N][Ka], rb [N][Kb]: the pooled rows; got: the six figures.  The module's bound on cross and (B = A) the variances; corr from them"""
    n, s = len(ra), -(-len(ra) // 4096)
    chain = LD((min(n, 4096) + s + 4) * U53)
    da, db = ra.astype(LD) - ra.astype(LD).mean(axis=0), rb.astype(LD) - rb.astype(LD).mean(axis=0)
    ea, eb = [np.array([(n + 2) * U53 * math.fsum(map(abs, col)) / n for col in r.T.tolist()], dtype=LD) for r in (ra, rb)]
    dbt = np.ascontiguousarray(db.T)
    for k in range(ra.shape[1]):
        prod = da[:, k][None, :] * dbt                                     # [Kb][N]: the sums run pairwise along the rows
        err = np.abs(got[4][k].astype(LD) - prod.sum(axis=1) / LD(n - 1))
        bound = (chain * np.abs(prod).sum(axis=1) + LD(n) * ea[k] * eb) / LD(n - 1)
        assert np.all(err <= bound), (what, "cross", k, np.argwhere(~(err <= bound))[:4].ravel(), float(np.max(err - bound)))
    for d, e, var, side in ((da, ea, got[2], "var_a"), (db, eb, got[3], "var_b")):
        t = (d * d).sum(axis=0)
        assert np.all(np.abs(var.astype(LD) - t / LD(n - 1)) <= (chain * t + LD(n) * e * e) / LD(n - 1)), (what, side)
    with np.errstate(all="ignore"):
        ok = (np.isfinite(got[2]) & (got[2] > 0))[:, None] & (np.isfinite(got[3]) & (got[3] > 0))[None, :]
        assert same_bits(got[5], np.where(ok, got[4] / (np.sqrt(got[2])[:, None] * np.sqrt(got[3])[None, :]), np.nan)), (what, "corr")


def submatrix(full, ca, cb):   # what a call over the lists ca, cb must return, from the call over all columns
    ca, cb = np.asarray(ca, dtype=int), np.asarray(cb, dtype=int)
    return full[0][ca], full[1][cb], full[2][ca], full[3][cb], full[4][np.ix_(ca, cb)], full[5][np.ix_(ca, cb)]


@pytest.mark.parametrize("kb", KBS)
@pytest.mark.parametrize("ka", KAS)
@pytest.mark.parametrize("n", NS)
def test_emulation_within_the_derived_bound_equals_the_square_kernel_and_is_invariant(n, ka, kb):
    for thin in (1, 3):
        a, b, first, count = two_fixtures(n, ka, kb, thin)
        what, at = (n, ka, kb, thin), dict(first=first, count=count, thin=thin)
        got, chunks = emulate(a, b, cap=-(-n // 4096) * 32768, **at)                                 # one tile pair to a chunk
        assert chunks == -(-ka // 32) * -(-kb // 128)
        check_bounds(pooled(a, first, count, thin), pooled(b, first, count, thin), got, what)        # 1. against np.longdouble
        ca, cb = shuffled_with_duplicate(ka, n + ka), shuffled_with_duplicate(ka, n + kb)
        square = cov_emulate(a, **at)
        own, _ = emulate(a, a, cols_a=ca, cols_b=cb, **at)                                           # 2. B = A: the square kernel's bits
        assert same_bits(own[4], square[1][np.ix_(ca, cb)]) and same_bits(own[2], np.diag(square[1])[ca]) and same_bits(own[0], square[0][ca]), what
        cb = shuffled_with_duplicate(kb, n + kb)                                                      # 3. sub-matrix, column order, chunking
        assert same_results(emulate(a, b, cols_a=ca, cols_b=cb, **at)[0], submatrix(got, ca, cb)), what
        whole, chunks = emulate(a, b, **at)
        assert chunks == 1 and same_results(whole, got), what
        an, bn = a.copy(), b.copy()                                                                   # 4. a NaN column on either side
        an[a.shape[0] // 2, first + thin, ka - 1], bn[0, first, kb // 2] = np.nan, np.nan
        nan, _ = emulate(an, bn, **at)
        keep_a, keep_b = [k for k in range(ka) if k != ka - 1], [k for k in range(kb) if k != kb // 2]
        assert same_results(submatrix(nan, keep_a, keep_b), submatrix(got, keep_a, keep_b)), what
        assert all(np.isnan(nan[q][ka - 1]).all() for q in (0, 2, 4, 5)) and all(np.isnan(nan[q][..., kb // 2]).all() for q in (1, 3, 4, 5)), what


def test_plan_exports_and_refusals():
    import rainier_amd as R
    L, out, big = _capi.lib(), (C.c_longlong * 9)(), (1 << 31) - 1
    plan = lambda *a: (emulation().rx_plan(*a, out), list(out))[1]
    assert plan(4, 5000, 3, 33, 129) == [1667, 6668, 2, 2, 2, 4, 2 << 15, 4, 0]
    assert plan(4096, 4096, 1, 4, 512)[-3:] == [CAP, 1, 0] and plan(4097, 4096, 1, 4, 512)[-2:] == [1, 1]     # S = 4096 fits, S = 4097 does not
    assert plan(big, big, 1, big, big)[-3:] == [(1 << 63) - 1, 1, 1]                                            # the product saturates
    assert all(name in _capi.EXPORTS and hasattr(L, name) for name in ("rh_cross_covariance_device", "rh_sampler_cross_covariance", "rh_cross_covariance_lower_only")) and L.rh_abi_version() == 6
    assert R.CrossCovariance._fields == ("mean_a", "mean_b", "var_a", "var_b", "cross", "corr", "cols_a", "cols_b")
    assert R.Influence._fields == ("influence", "ij_cov", "ij_se", "post_sd", "cols", "ll_cols")
    assert b"rh_xcov_tile_kernel" in _capi.cross_covariance_lower_only("gfx950")                   # built, and judged as before a launch
    buf, ip = np.zeros(64), C.POINTER(C.c_int32)

    def call(pa=C.c_void_p(4096), pb=C.c_void_p(8192), chains=4, iters=10, first=0, count=10, thin=1, cols_a=None, cols_b=None, outs=(1,) * 6):
        sa, sb = [None if c is None else np.array(c + [0], dtype=np.int32) for c in (cols_a, cols_b)]   # (the pointers are never dereferenced)
        return L.rh_cross_covariance_device(pa, 2, pb, 3, 0, chains, iters, first, count, thin, None if sa is None else sa.ctypes.data_as(ip), len(cols_a or ()),
                                            None if sb is None else sb.ctypes.data_as(ip), len(cols_b or ()), *[_capi.dptr(buf) if o else None for o in outs])
    for kw, word in ((dict(pa=None), "NULL"), (dict(pb=None), "NULL"), (dict(count=11), "window"), (dict(first=-1), "window"), (dict(thin=0), "window"),
                     (dict(count=0), "window"), (dict(chains=1, count=1), "at least 2"), (dict(chains=1, thin=10), "at least 2"), (dict(cols_a=[2]), "cols_a"),
                     (dict(cols_a=[0, -1]), "cols_a"), (dict(cols_b=[3]), "cols_b"), (dict(cols_a=[]), "ncols_a"), (dict(cols_b=[]), "ncols_b"),
                     (dict(outs=(0,) * 6), "all NULL")):
        assert call(**kw) == _capi.RH_E_INVALID and word in L.rh_last_error(None).decode(), kw       # the message names the argument
    assert L.rh_sampler_cross_covariance(None, None, 0, 10, 1, None, 0, None, 0, *[_capi.dptr(buf)] * 6) == _capi.RH_E_INVALID
    assert call(chains=4097, iters=4096, count=4096) == _capi.RH_E_UNSUPPORTED and "workspace" in L.rh_last_error(None).decode()   # S > 4096, before any device call
    if L.rh_device_count() == 0:
        assert call() == call(cols_a=[1, 1], cols_b=[2, 0], outs=(0, 0, 0, 0, 0, 1)) == _capi.RH_E_DEVICE and "no CPU fallback" in L.rh_last_error(None).decode()
