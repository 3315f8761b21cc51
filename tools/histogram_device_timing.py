"""Times the posterior histograms and joint count grids on the device (rh_histogram_device / rh_histogram2d_device: the min / max
pass, the binning pass with LDS integer adds, the finish) against what there was before them for the same answer: the draws copied
to the host and np.histogram / np.histogram2d per column or pair.  Shapes: cfg 2's (1024 chains x 1000 iterations x 5 parameters),
1024 x 400 x 160, 256 x 40 x 10 004 (all columns, 20 bins) and 10 pairs of the second shape at 64 x 64.  One process; every figure --
device call, copy, numpy -- is one warm call, then the median of 5.  The buffers are synthetic AR(1) draws: 16 distinct chains
generated on the host and uploaded chains / 16 times.  Beside the times: the bytes each pass moves (by the kernels' own arithmetic,
not counters) and the rate of the call with given bounds (it has no min / max pass: one read of the draws) against the 8 TB/s of
HBM -- a lower bound of the binning pass's own rate, since the call's fixed costs (allocations, two copies, the waits) are in it.
Prints one JSON line.

    python tools/histogram_device_timing.py [--small]        (--small: the first two shapes only)
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
SPLIT, HBM_TBS = 4096, 8.0              # RHH_SPLIT (csrc/device/rh_hist.hip.h); the MI355X's HBM figure


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


def shape(name, m, n, k, nbins=20, pairs=None, bins2=(64, 64)):
    ptr = upload(m, n, k)
    back = np.empty((m, n, k))
    copy, _ = median5(lambda: hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), ptr, back.nbytes, 2))
    rows = back.reshape(m * n, k)
    N, draws = m * n, m * n * k * 8
    S = -(-N // SPLIT)
    out = {"shape": name, "chains": m, "iterations": n, "nvars": k, "N": N, "draws_bytes": draws, "splits": S, "host_copy_s_median5": copy,
           "host_route_bytes_over_the_link": draws}
    if pairs is None:
        auto = R.histogram_device(ptr.value, m, n, k, device=0, bins=nbins)
        given = np.stack([auto.edges[:, 0], auto.edges[:, -1]], axis=1)
        dev, dev_all = median5(lambda: R.histogram_device(ptr.value, m, n, k, device=0, bins=nbins))
        dev_given, _ = median5(lambda: R.histogram_device(ptr.value, m, n, k, device=0, bins=nbins, range=given))
        one, _ = median5(lambda: R.histogram_device(ptr.value, m, n, k, device=0, bins=nbins, cols=[0], range=given[:1]))
        host, host_all = median5(lambda: [np.histogram(rows[:, p], bins=nbins) for p in range(k)])
        want = np.stack([np.histogram(rows[:, p], bins=auto.edges[p])[0] for p in range(min(k, 64))])
        assert np.array_equal(auto.counts[:min(k, 64)], want)
        partials = S * k * (nbins + 3) * 4
        out.update({"nbins": nbins, "columns": k, "device_s_median5": dev, "device_s_all": dev_all, "device_given_bounds_s_median5": dev_given,
                    "device_one_column_given_bounds_s_median5": one, "host_numpy_s_median5": host, "host_numpy_s_all": host_all,
                    "bytes": {"minmax_pass_reads": draws, "binning_pass_reads": draws, "partials_written_and_read": 2 * partials,
                              "counts_and_edges_copied": k * (nbins + 3) * 8 + 2 * k * (nbins + 1) * 8},
                    "given_bounds_call_TBs": draws / dev_given / 1e12, "given_bounds_call_share_of_hbm": draws / dev_given / 1e12 / HBM_TBS})
    else:
        auto = R.histogram2d_device(ptr.value, m, n, k, pairs, device=0, bins=bins2)
        dev, dev_all = median5(lambda: R.histogram2d_device(ptr.value, m, n, k, pairs, device=0, bins=bins2))
        host, host_all = median5(lambda: [np.histogram2d(rows[:, a], rows[:, b], bins=bins2) for a, b in pairs])
        a, b = pairs[0]
        assert np.array_equal(auto.grid[0], np.histogram2d(rows[:, a], rows[:, b], bins=[auto.xedges[0], auto.yedges[0]])[0].astype(np.int64))
        touched = N * 64 * 2 * len(pairs)            # a pair's two columns of a row are two 64-byte sectors of it
        out.update({"pairs": len(pairs), "bins": list(bins2), "device_s_median5": dev, "device_s_all": dev_all, "host_numpy_s_median5": host,
                    "host_numpy_s_all": host_all,
                    "bytes": {"minmax_pass_reads_at_least": N * 64 * min(2 * len(pairs), -(-k * 8 // 64)), "pair_pass_sectors_touched": touched,
                              "partials_written_and_read": 2 * S * len(pairs) * (bins2[0] * bins2[1] + 1) * 4}})
    out["host_route_s"] = copy + out["host_numpy_s_median5"]
    out["speedup_over_the_host_route"] = out["host_route_s"] / out["device_s_median5"]
    hip.hipFree(ptr)
    return out


if __name__ == "__main__":
    shapes = [dict(name="cfg2", m=1024, n=1000, k=5), dict(name="1024x400x160", m=1024, n=400, k=160),
              dict(name="256x40x10004", m=256, n=40, k=10004),
              dict(name="1024x400x160, 10 pairs at 64x64", m=1024, n=400, k=160, pairs=[(i, 159 - 7 * i) for i in range(10)])]
    if "--small" in sys.argv:
        shapes = shapes[:2]
    print(json.dumps([shape(**s) for s in shapes]))
