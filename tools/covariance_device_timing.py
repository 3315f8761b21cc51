"""Times the posterior covariance and correlation on the device (rh_covariance_device: the pooled mean, X^T X of the centred draws
on the fp64 matrix cores, the correlation) against what there was before it for the same answer: the draws copied to the host and
np.cov.  Shapes: cfg 2's (1024 chains x 1000 iterations x 5 parameters), 256 x 40 x 704 and 1024 x 400 x 160.  One process; every
figure -- device call, copy, np.cov -- is one warm call, then the median of 5.  The buffers are synthetic AR(1) draws: 16 distinct
chains generated on the host and uploaded chains / 16 times.  Beside the times: the flop the tile kernel issues and the flop of the
answer (2 N K^2 / 2 for the triangle), the rate against the 47 TFLOP/s that profiles/r3_d_fp64_mfma measured for
v_mfma_f64_16x16x4_f64 at this shape of use, and the bytes each pass moves (by the kernels' own arithmetic, not counters).
Prints one JSON line.

    python tools/covariance_device_timing.py [--small]        (--small: the first two shapes only)
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
SPLIT, TC, SLAB = 4096, 64, 32          # RC_SPLIT, RC_TC, RC_SLAB (csrc/device/rh_cov.hip.h)
MFMA_F64_TFLOPS = 47.0                  # profiles/r3_d_fp64_mfma: one 16x16x4 issue per 105 cycles


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
    dev, dev_all = median5(lambda: R.covariance_device(ptr.value, m, n, k, device=0, corr=True))
    mean_only, _ = median5(lambda: R.covariance_device(ptr.value, m, n, k, device=0, cols=[0]))      # one column: the call's fixed costs
    # the host route: the whole buffer back to the host (as rh_sampler_draws does), then np.cov and np.corrcoef's division
    back = np.empty((m, n, k))
    copy, _ = median5(lambda: hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), ptr, back.nbytes, 2))
    rows = back.reshape(m * n, k)

    def host():
        c = np.cov(rows, rowvar=False, ddof=1).reshape(k, k)
        sd = np.sqrt(np.diag(c))
        return c / (sd[:, None] * sd[None, :])
    host_cov, host_all = median5(host)
    hip.hipFree(ptr)
    N, draws = m * n, m * n * k * 8
    S, T = -(-N // SPLIT), -(-k // TC)
    pairs = T * (T + 1) // 2
    rows_issued = (S - 1) * SPLIT + -(-(N - (S - 1) * SPLIT) // SLAB) * SLAB
    issued = 2.0 * pairs * rows_issued * TC * TC
    useful = 1.0 * N * k * (k + 1)
    ws = pairs * S * TC * TC * 8
    return {"shape": name, "chains": m, "iterations": n, "nvars": k, "N": N, "draws_bytes": draws, "splits": S, "tile_pairs": pairs,
            "device_s_median5": dev, "device_s_all": dev_all, "device_one_column_s_median5": mean_only,
            "flop_issued_by_the_tile_kernel": issued, "flop_of_the_answer": useful,
            "tflops_issued_over_the_whole_call": issued / dev / 1e12, "tflops_of_the_answer_over_the_whole_call": useful / dev / 1e12,
            "share_of_the_measured_mfma_f64_rate": issued / dev / 1e12 / MFMA_F64_TFLOPS,
            "bytes": {"mean_pass_reads": draws, "tile_pass_reads": N * TC * 8 * T * T, "partials_written_and_read": 2 * ws,
                      "cov_and_corr_written_and_copied": 3 * 8 * k * k + 8 * k * k,
                      "total": draws + N * TC * 8 * T * T + 2 * ws + 4 * 8 * k * k},
            "host_copy_s_median5": copy, "host_np_cov_s_median5": host_cov, "host_np_cov_s_all": host_all, "host_route_s": copy + host_cov,
            "host_route_bytes_over_the_link": draws}


if __name__ == "__main__":
    shapes = [("cfg2", 1024, 1000, 5), ("256x40x704", 256, 40, 704), ("1024x400x160", 1024, 400, 160)]
    if "--small" in sys.argv:
        shapes = shapes[:2]
    print(json.dumps([shape(*s) for s in shapes]))
