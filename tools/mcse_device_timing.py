"""Times the Monte Carlo standard errors on the device (rh_mcse_device: the gather of the split window, one pooled sort, the pooled
moments, the autocovariances up to lag 255 of 3 + nprobs series made where y is read, the scans, the host's beta quantiles, the
order statistics) against two yardsticks on the same buffer: rh_rank_diagnostics_device (merged code: two sorts, four series of which
three carry lags, each written to memory before its chain kernel reads it) and the host route (the draws copied to the host and the
contract restated in numpy and scipy, column by column).  Shape: [1024][200][k], k = 5 and 64.  One process; every figure is one
warm call, then the median of 5 whole-call wall times.  Wall clock only: no counters were collected.  The numpy route of k = 64 is
timed over its first 8 columns and scaled (it is a loop over the columns); the figure says so.  The buffers are synthetic AR(1)
draws: 16 distinct chains generated on the host and uploaded chains / 16 times.  Prints one JSON line.

    python tools/mcse_device_timing.py
"""
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
from scipy.special import betaincinv

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rainier_amd as R  # noqa: E402
from tools.rank_diagnostics_device_timing import MAXLAG, hip, median5, upload  # noqa: E402

PROBS = (0.05, 0.5, 0.95)
MANY = tuple(np.linspace(0.03, 0.97, 16))
P16, P84 = 0.15865525393145707, 0.8413447460685429


def ess_of(u):
    """the contract's ESS of a series u [M][h]"""
    M, h = u.shape
    S, L = M * h, min(h - 1, MAXLAG)
    m = u.mean(axis=1)
    d = u - m[:, None]
    g = np.array([np.mean(np.sum(d[:, :h - t] * d[:, t:], axis=1) / h) for t in range(L + 1)])
    W = g[0] * h / (h - 1)
    V = (h - 1) / h * W + np.sum((m - m.mean()) ** 2) / (M - 1)
    if not W > 0:
        return math.nan
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
    return S / max(tau, 1.0 / math.log10(S))


def host_route(x, cols, probs):
    """x [chains][n][nvars] on the host -> (mean, sd, ess_mean, ess_sd, mcse_mean, mcse_sd) [6][K] and mcse_quantile [K][nprobs]"""
    m, n, _ = x.shape
    h = n // 2
    out, mq = [], []
    for p in cols:
        y = np.stack([x[:, :h, p], x[:, n - h:, p]], axis=1).reshape(2 * m, h)
        S = y.size
        s = np.sort(y.ravel())
        mean = y.mean()
        d = y - mean
        e2, e4 = np.mean(d * d), np.mean((d * d) * (d * d))
        sd = math.sqrt(S * e2 / (S - 1))
        ea, eb, ec = ess_of(y), ess_of(np.abs(d)), ess_of(d * d)
        out.append((mean, sd, ea, eb, sd / math.sqrt(ea), math.sqrt((e4 - e2 * e2) / ec / e2 / 4)))
        row = []
        for q in probs:
            e = ess_of((y <= s[min(S - 1, int(math.floor(S * q)))]).astype(np.float64))
            a, b = betaincinv(e * q + 1, e * (1 - q) + 1, [P16, P84])
            row.append((s[min(int(math.ceil(b * S)), S) - 1] - s[max(int(math.floor(a * S)), 1) - 1]) / 2)
        mq.append(row)
    return np.array(out).T, np.array(mq)


def shape(name, m, n, k, host_cols):
    ptr = upload(m, n, k)
    back = np.empty((m, n, k))
    copy, _ = median5(lambda: hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), ptr, back.nbytes, 2))
    call = lambda probs, **kw: R.mcse_device(ptr.value, m, n, k, device=0, probs=probs, **kw)
    dev, dev_all = median5(lambda: call(PROBS))
    dev0, _ = median5(lambda: call(()))
    dev16, _ = median5(lambda: call(MANY))
    one, _ = median5(lambda: call(PROBS, cols=[0]))
    rank, rank_all = median5(lambda: R.rank_diagnostics_device(ptr.value, m, n, k, device=0))
    got = call(PROBS)
    cols = list(range(host_cols))
    res = []
    host, host_all = median5(lambda: res.append(host_route(back, cols, PROBS)))
    want, want_mq = res[-1]
    for a, b in zip((got.mean, got.sd, got.ess_mean, got.ess_sd, got.mcse_mean, got.mcse_sd), want):
        assert np.allclose(a[:host_cols], b, rtol=1e-8, atol=1e-12), (name, a[:host_cols], b)
    assert np.allclose(got.mcse_quantile[:host_cols], want_mq, rtol=1e-9, atol=0.0)
    h = n // 2
    S, L = 2 * m * h, min(h - 1, MAXLAG)
    out = {"shape": name, "chains": m, "iterations": n, "nvars": k, "S": S, "sequences": 2 * m, "h": h, "lags": L, "draws_bytes": m * n * k * 8,
           "workspace_bytes_per_column_3_probs": 24 * S + 8 * 6 * 2 * m * (L + 2), "host_copy_s_median5": copy,
           "device_s_median5": dev, "device_s_all": dev_all, "device_series": 6, "device_no_probs_s_median5": dev0, "device_16_probs_s_median5": dev16,
           "device_s_per_added_series": (dev16 - dev0) / 16.0, "device_one_column_s_median5": one,
           "rank_diagnostics_device_s_median5": rank, "rank_diagnostics_device_s_all": rank_all, "rank_series_with_lags": 3,
           "host_numpy_columns_timed": host_cols, "host_numpy_s_median5": host, "host_numpy_s_all": host_all,
           "host_numpy_s_scaled_to_all_columns": host * k / host_cols,
           "ess_mean_min": float(np.nanmin(got.ess_mean)), "mcse_mean_max": float(np.nanmax(got.mcse_mean)), "truncated_any": int(np.any(got.truncated != 0))}
    out["host_route_s"] = copy + out["host_numpy_s_scaled_to_all_columns"]
    out["speedup_over_the_host_route"] = out["host_route_s"] / dev
    hip.hipFree(ptr)
    return out


if __name__ == "__main__":
    shapes = [dict(name="1024x200x5", m=1024, n=200, k=5, host_cols=5), dict(name="1024x200x64", m=1024, n=200, k=64, host_cols=8)]
    print(json.dumps({"clock": "wall (time.perf_counter around whole calls); no counters collected", "shapes": [shape(**s) for s in shapes]}))
