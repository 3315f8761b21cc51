"""Times the rank-normalised split R-hat, bulk ESS and tail ESS on the device (rh_rank_diagnostics_device: the gather of the split
window, two pooled sorts, the ranks and z-scores, the autocovariances up to lag 255 of four series, the scans) against what there
was before it for the same answer: the draws copied to the host and the contract restated in numpy and scipy, column by column (the
same 256 lags, summed directly).  Shapes: cfg 2's (1024 chains x 1000 iterations x 5 parameters) and a wide one (64 x 2000 x 512).
One process; every figure -- device call, copy, numpy -- is one warm call, then the median of 5.  The numpy route of the wide shape
is timed over its first 8 columns and scaled to 512 (it is a loop over the columns); the figure says so.  The buffers are synthetic
AR(1) draws: 16 distinct chains generated on the host and uploaded chains / 16 times.  Prints one JSON line.

    python tools/rank_diagnostics_device_timing.py
"""
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
from scipy.special import ndtri

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rainier_amd as R  # noqa: E402

hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
MAXLAG = 255                             # RK_MAXLAG (csrc/device/rh_rank.hip.h)


def median5(fn):
    fn()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def block(chains, n, k, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((chains, n, k))
    for i in range(1, n):
        x[:, i, :] += 0.5 * x[:, i - 1, :]
    return x


def upload(m, n, k):
    blk = block(16, n, k, 1)
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), m * n * k * 8) == 0
    for r in range(m // 16):
        assert hip.hipMemcpy(C.c_void_p(ptr.value + r * blk.nbytes), blk.ctypes.data_as(C.c_void_p), blk.nbytes, 1) == 0
    return ptr


def zscores(v):
    """the average ranks of v (finite values: the usual order is the key order but for signed zeros) through (r - 3/8) / (S + 1/4)"""
    flat = v.ravel()
    s = np.sort(flat)
    r = (np.searchsorted(s, flat, "left") + np.searchsorted(s, flat, "right") + 1) * 0.5
    return ndtri((r - 0.375) / (flat.size + 0.25)).reshape(v.shape)


def estimator(u, lags=True):
    """(rhat, ess) of a series u [M][h] by the contract's formulas"""
    M, h = u.shape
    S, L = M * h, (min(h - 1, MAXLAG) if lags else 0)
    m = u.mean(axis=1)
    d = u - m[:, None]
    g = np.array([np.mean(np.sum(d[:, :h - t] * d[:, t:], axis=1) / h) for t in range(L + 1)])
    W = g[0] * h / (h - 1)
    V = (h - 1) / h * W + np.sum((m - m.mean()) ** 2) / (M - 1)
    if not W > 0:
        return math.nan, math.nan
    rhat = math.sqrt(V / W)
    if L == 0:
        return rhat, math.nan
    rho = 1.0 - (W - g) / V
    rho[0] = 1.0
    tau, prev = -1.0, math.inf
    for k in range((L - 1) // 2 + 1):
        P = rho[2 * k] + rho[2 * k + 1]
        if not P > 0:
            tau += max(rho[2 * k], 0.0)
            break
        prev = min(P, prev)
        tau += 2 * prev
    return rhat, S / max(tau, 1.0 / math.log10(S))


def host_route(x, cols):
    """x [chains][n][nvars] on the host -> (rhat_bulk, rhat_folded, ess_bulk, ess_tail) per column of cols"""
    m, n, _ = x.shape
    h = n // 2
    out = []
    for p in cols:
        y = np.stack([x[:, :h, p], x[:, n - h:, p]], axis=1).reshape(2 * m, h)
        S = y.size
        s = np.sort(y.ravel())
        med = 0.5 * s[S // 2 - 1] + 0.5 * s[S // 2]
        rb, eb = estimator(zscores(y))
        rf, _ = estimator(zscores(np.abs(y - med)), lags=False)
        tails = [estimator((y <= s[min(S - 1, int(math.floor(S * q)))]).astype(np.float64))[1] for q in (0.05, 0.95)]
        out.append((rb, rf, eb, min(tails)))
    return np.array(out).T


def shape(name, m, n, k, host_cols):
    ptr = upload(m, n, k)
    back = np.empty((m, n, k))
    copy, _ = median5(lambda: hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), ptr, back.nbytes, 2))
    dev, dev_all = median5(lambda: R.rank_diagnostics_device(ptr.value, m, n, k, device=0))
    one, _ = median5(lambda: R.rank_diagnostics_device(ptr.value, m, n, k, device=0, cols=[0]))
    got = R.rank_diagnostics_device(ptr.value, m, n, k, device=0)
    cols = list(range(host_cols))
    res = []
    host, host_all = median5(lambda: res.append(host_route(back, cols)))
    want = res[-1]
    for a, b in zip((got.rhat_bulk, got.rhat_folded, got.ess_bulk, got.ess_tail), want):
        assert np.allclose(a[:host_cols], b, rtol=1e-9, atol=0.0), (name, a[:host_cols], b)
    h = n // 2
    S = 2 * m * h
    out = {"shape": name, "chains": m, "iterations": n, "nvars": k, "S": S, "sequences": 2 * m, "h": h, "draws_bytes": m * n * k * 8,
           "workspace_bytes_per_column": 32 * S + 8 * 2 * m * (min(h - 1, MAXLAG) + 2), "host_copy_s_median5": copy, "device_s_median5": dev,
           "device_s_all": dev_all, "device_one_column_s_median5": one, "host_numpy_columns_timed": host_cols, "host_numpy_s_median5": host,
           "host_numpy_s_all": host_all, "host_numpy_s_scaled_to_all_columns": host * k / host_cols,
           "rhat_max": float(np.nanmax(got.rhat)), "ess_bulk_min": float(np.nanmin(got.ess_bulk)), "truncated_any": int(np.any(got.truncated != 0))}
    out["host_route_s"] = copy + out["host_numpy_s_scaled_to_all_columns"]
    out["speedup_over_the_host_route"] = out["host_route_s"] / dev
    hip.hipFree(ptr)
    return out


if __name__ == "__main__":
    shapes = [dict(name="cfg2", m=1024, n=1000, k=5, host_cols=5), dict(name="64x2000x512", m=64, n=2000, k=512, host_cols=8)]
    print(json.dumps([shape(**s) for s in shapes]))
