"""Times the posterior summary on the device (rh_summary_device: sort of every pooled column, order statistics, hdpi, mean, sd)
against what there was before it for the same answer: the draws copied to the host and np.sort per column.  Shapes: cfg 2's
(1024 chains x 1000 iterations x 5 parameters), 256 x 40 x 704 and 1024 x 400 x 160.  One process; every figure -- device call, copy, np.sort -- is
one warm call, then the median of 5.  The buffers are synthetic AR(1) draws: 16 distinct chains generated on the host and uploaded chains / 16 times.
Beside the times, the HBM bytes each pass moves (by the kernels' own arithmetic, not counters).  Prints one JSON line.

    python tools/summary_device_timing.py [--small]        (--small: the first two shapes only)
"""
import ctypes as C
import json
import math
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
TILE = 4096              # RS_TILE (csrc/device/rh_summary.hip.h)


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


def shape(name, m, n, k):
    blk = block(16, n, k, 1)
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), m * n * k * 8) == 0
    for r in range(m // 16):
        assert hip.hipMemcpy(C.c_void_p(ptr.value + r * blk.nbytes), blk.ctypes.data_as(C.c_void_p), blk.nbytes, 1) == 0
    dev, dev_all = median5(lambda: R.summary_device(ptr.value, m, n, k, device=0))
    # the host route: the whole buffer back to the host (as rh_sampler_draws does), then np.sort of every pooled column
    back = np.empty((m, n, k))
    copy, _ = median5(lambda: hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), ptr, back.nbytes, 2))
    cols = np.ascontiguousarray(back.reshape(m * n, k).T)
    host_sort, host_sort_all = median5(lambda: np.sort(cols, axis=1))
    hip.hipFree(ptr)
    N, draws = m * n, m * n * k * 8
    passes = 0 if N <= TILE else math.ceil(math.log2(math.ceil(N / TILE)))
    return {"shape": name, "chains": m, "iterations": n, "nvars": k, "N": N, "draws_bytes": draws, "merge_passes": passes,
            "device_s_median5": dev, "device_s_all": dev_all,
            "hbm_bytes": {"tile_sort_read_plus_write": 2 * draws, "each_merge_pass_read_plus_write": 2 * draws,
                          "finish_reads_4_sweeps": 4 * draws, "total": (2 + 2 * passes + 4) * draws},
            "host_copy_s_median5": copy, "host_np_sort_s_median5": host_sort, "host_np_sort_s_all": host_sort_all, "host_route_s": copy + host_sort, "host_route_bytes_over_the_link": draws}


if __name__ == "__main__":
    shapes = [("cfg2", 1024, 1000, 5), ("256x40x704", 256, 40, 704), ("1024x400x160", 1024, 400, 160)]
    if "--small" in sys.argv:
        shapes = shapes[:2]
    print(json.dumps([shape(*s) for s in shapes]))
