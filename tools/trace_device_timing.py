"""Times Trace.diagnostics on the device against the host route (device -> host copy + rh_diagnostics) at the shapes of cfg 2
(1024 chains x 1000 iterations x 5 parameters) and cfg 5 (1024 x 400 x 10 004).  One process; per figure one warm call, then the
median of 5.  The buffers are synthetic AR(1) draws: 16 distinct chains generated on the host and uploaded 64 times (the kernels'
time does not depend on the values; only the finish kernel's scan length does).  Prints one JSON line.

    python tools/trace_device_timing.py [--small]        (--small: a tenth of cfg 5's parameters)
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rainier_amd as R  # noqa: E402

hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
HBM_PEAK = 8.0e12        # bytes / s, MI355X


def median5(fn):
    fn()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def block(chains, n, k, seed):
    rng = np.random.default_rng(seed)
    x = np.empty((chains, n, k))
    x[:, 0, :] = rng.standard_normal((chains, k))
    for i in range(1, n):
        x[:, i, :] = 0.5 * x[:, i - 1, :] + rng.standard_normal((chains, k))
    return x


def shape(name, m, n, k, host_cols):
    blk = block(16, n, k, 1)
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), m * n * k * 8) == 0
    for r in range(m // 16):
        assert hip.hipMemcpy(C.c_void_p(ptr.value + r * blk.nbytes), blk.ctypes.data_as(C.c_void_p), blk.nbytes, 1) == 0
    dev, dev_all = median5(lambda: R.diagnostics_device(ptr.value, m, n, k, device=0, moments=True))
    # the host route on `host_cols` parameters: copy the chains' blocks back (as rh_sampler_draws does), then one host thread
    back = np.empty_like(blk)
    copy, _ = median5(lambda: [hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(ptr.value + r * blk.nbytes), blk.nbytes, 2) for r in range(min(4, m // 16))])
    copy_bw = min(4, m // 16) * blk.nbytes / copy
    hx = np.ascontiguousarray(np.tile(blk[:, :, :host_cols], (m // 16, 1, 1)))
    t0 = time.perf_counter(); R.diagnostics(hx); host = time.perf_counter() - t0
    hip.hipFree(ptr)
    gb = m * n * k * 8 / 1e9
    return {"shape": name, "chains": m, "iterations": n, "nvars": k, "draws_gb": gb, "device_s_median5": dev, "device_s_all": dev_all,
            "hbm_frac_one_pass": gb * 1e9 / dev / HBM_PEAK, "d2h_gb_per_s": copy_bw / 1e9, "host_cols": host_cols, "host_s_on_host_cols": host,
            "host_route_s_all_params_extrapolated": gb * 1e9 / copy_bw + host * k / host_cols}


if __name__ == "__main__":
    small = "--small" in sys.argv
    out = [shape("cfg2", 1024, 1000, 5, 5), shape("cfg5/10" if small else "cfg5", 1024, 400, 1000 if small else 10004, 64)]
    print(json.dumps(out))
