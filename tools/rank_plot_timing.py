"""Times the rank plots on the device (rh_rank_plot_device: the gather, one pooled sort per column, the splitters, the count kernel's
two-level search, chains x bins integers per column back) against (a) what there was before it for the same answer -- the draws copied
to the host and the numpy reference (sort, searchsorted left / right, the integer bin, bincount) -- and (b) rank_diagnostics_device on
the same buffer, which does two of these pooled sorts and the autocorrelation work on top.  Shapes: cfg 2's (1024 chains x 1000
iterations x 5 parameters) and 64 x 2000 x 512, 20 bins.  One process; whole-call wall times that end in the call's own synchronise;
per shape two warm calls of each, then the two device calls alternating, 9 samples each, a sample the mean of a batch of calls (50 at
the first shape, 10 at the second: a quarter of a second or so of work): median, smallest and largest.  The host route: one warm run,
then the median of 3 single runs.  The device counts are compared with the host route's at the timed size.  The buffers are
synthetic AR(1) draws: 16 distinct chains generated on the host and uploaded chains / 16 times, each copy with an offset of its own.
Prints one JSON line.

    python tools/rank_plot_timing.py
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
BINS = 20


def timed(fn, batch=1):
    t0 = time.perf_counter()
    for _ in range(batch):
        fn()
    return (time.perf_counter() - t0) / batch


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "n": len(ts)}


def host_route(x):
    """the rank counts [K][chains][BINS] in numpy from the draws on the host (finite draws: the float order is the key order)"""
    c, n, k = x.shape
    s_total = c * n
    counts = np.empty((k, c, BINS), dtype=np.int64)
    chain = np.repeat(np.arange(c, dtype=np.int64), n)
    for p in range(k):
        v = np.ascontiguousarray(x[:, :, p]).ravel()
        s = np.sort(v)
        b = (np.searchsorted(s, v, "left") + np.searchsorted(s, v, "right")).astype(np.int64) * BINS // (2 * s_total)
        counts[p] = np.bincount(chain * BINS + b, minlength=c * BINS).reshape(c, BINS)
    return counts


def shape(name, m, n, k, batch):
    rng = np.random.default_rng(1)
    blk = rng.standard_normal((16, n, k))
    for i in range(1, n):
        blk[:, i, :] += 0.5 * blk[:, i - 1, :]
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), m * n * k * 8) == 0
    for r in range(m // 16):
        part = blk + 0.05 * rng.standard_normal((16, 1, k))
        assert hip.hipMemcpy(C.c_void_p(ptr.value + r * part.nbytes), part.ctypes.data_as(C.c_void_p), part.nbytes, 1) == 0
    res = {}
    plot = lambda: res.__setitem__("plot", R.rank_plot_device(ptr.value, m, n, k, device=0, bins=BINS))
    diag = lambda: res.__setitem__("diag", R.rank_diagnostics_device(ptr.value, m, n, k, device=0))
    for fn in (plot, diag, plot, diag):
        fn()
    t_plot, t_diag = [], []
    for _ in range(9):
        t_plot.append(timed(plot, batch)); t_diag.append(timed(diag, batch))
    back = np.empty((m, n, k))
    copy = lambda: hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), ptr, back.nbytes, 2)
    host = lambda: res.__setitem__("host", host_route(back))
    copy(); host()
    t_copy, t_host = [timed(copy) for _ in range(3)], [timed(host) for _ in range(3)]
    hip.hipFree(ptr)
    same = bool(np.array_equal(res["plot"].counts, res["host"])) and not res["plot"].nan.any()
    p, d, hc, hn = stats(t_plot), stats(t_diag), stats(t_copy), stats(t_host)
    return {"shape": name, "chains": m, "iterations": n, "nvars": k, "bins": BINS, "calls_per_sample": batch, "S": m * n, "draws_bytes": m * n * k * 8, "result_bytes": k * m * BINS * 4 + k * 4,
            "counts_equal_the_host_routes": same, "largest_ks": float(res["plot"].ks.max()), "largest_rhat": float(np.nanmax(res["diag"].rhat)),
            "rank_plot_device": p, "rank_diagnostics_device": d, "host_copy": hc, "host_numpy": hn,
            "host_route_s": hc["median_s"] + hn["median_s"], "host_route_over_rank_plot": (hc["median_s"] + hn["median_s"]) / p["median_s"],
            "rank_plot_over_rank_diagnostics": p["median_s"] / d["median_s"]}


if __name__ == "__main__":
    print(json.dumps([shape(*s) for s in [("cfg2", 1024, 1000, 5, 50), ("64x2000x512", 64, 2000, 512, 10)]]))
