"""Times pointwise WAIC and PSIS-LOO on the device (rh_loo_device: the pooled sort of every column, the moments, the Pareto fit of
the tail, the smoothed weights) against what there was before it for the same answer: the log-likelihood matrix copied to the host
and the contract restated in numpy, column by column (tests/test_loo_device_cpu.py's restate_column, in longdouble).  Shape: KidIQ's
at the bench's chain count, 1024 chains x 200 draws x 434 observations (711 MB), made on the host in blocks of 64 chains with seeds of
their own (no value is tied with a copy) and uploaded once.  One process; every figure -- device call, copy, numpy -- is one warm call,
then 5 repetitions: the median and all five.  The numpy route is timed over the first 8 columns and scaled to 434 (it is a loop over the
columns); the figure says so.  Prints one JSON line.

    python tools/loo_device_timing.py
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rainier_amd as R  # noqa: E402
from tests.test_loo_device_cpu import restate_column  # noqa: E402

hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
BLOCK = 64


def median5(fn):
    fn()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def block(n, k, seed):
    """BLOCK chains x n x k log-likelihoods: observation i is -(theta - c_i)^2 / (2 s_i^2) over theta ~ N(0, 1), the c_i spread over
    (-1.5, 1.5) and the s_i over (1, 3): Pareto k from about 0.1 to beyond 0.7, as a real data set has"""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((BLOCK, n, k))
    c, s = np.linspace(-1.5, 1.5, k), 1.0 + 2.0 * ((np.arange(k) * 7) % k) / k
    return np.ascontiguousarray(-0.5 * ((t - c) / s) ** 2 - np.log(s))


def shape(name, m, n, k, host_cols):
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), m * n * k * 8) == 0
    for r in range(m // BLOCK):
        blk = block(n, k, 100 + r)
        assert hip.hipMemcpy(C.c_void_p(ptr.value + r * blk.nbytes), blk.ctypes.data_as(C.c_void_p), blk.nbytes, 1) == 0
    back = np.empty((m, n, k))
    copy, copy_all = median5(lambda: hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), ptr, back.nbytes, 2))
    dev, dev_all = median5(lambda: R.loo_device(ptr.value, m, n, k, device=0))
    one, _ = median5(lambda: R.loo_device(ptr.value, m, n, k, device=0, cols=[0]))
    got = R.loo_device(ptr.value, m, n, k, device=0)
    res = []
    host, host_all = median5(lambda: res.append([restate_column(back[:, :, p].reshape(-1)) for p in range(host_cols)]))
    for p, want in enumerate(res[-1]):
        have = (got.lpd[p], got.p_waic[p], got.elpd_loo[p], got.pareto_k[p], got.tail_n[p])
        assert np.allclose(have, want, rtol=1e-9, atol=0.0), (name, p, have, want)
    S = m * n
    out = {"shape": name, "chains": m, "iterations": n, "nvars": k, "S": S, "ll_bytes": m * n * k * 8, "workspace_bytes_per_column": 16 * S,
           "tail_n": int(got.tail_n[0]), "host_copy_s_median5": copy, "host_copy_s_all": copy_all, "device_s_median5": dev, "device_s_all": dev_all,
           "device_one_column_s_median5": one, "host_numpy_columns_timed": host_cols, "host_numpy_s_median5": host, "host_numpy_s_all": host_all,
           "host_numpy_s_scaled_to_all_columns": host * k / host_cols, "elpd_loo_total": got.loo()[0], "elpd_loo_se": got.loo()[1],
           "elpd_waic_total": got.waic()[0], "pareto_k_min": float(np.min(got.pareto_k)), "pareto_k_max": float(np.max(got.pareto_k)),
           "pareto_k_above_0.7": int(np.sum(got.pareto_k > 0.7))}
    out["host_route_s"] = copy + out["host_numpy_s_scaled_to_all_columns"]
    out["speedup_over_the_host_route"] = out["host_route_s"] / dev
    hip.hipFree(ptr)
    return out


if __name__ == "__main__":
    print(json.dumps([shape("kidiq_1024x200x434", 1024, 200, 434, 8)]))
