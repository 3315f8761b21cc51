"""Times a linear map of device-resident draws (rh_linear_device: Y = (X - c) W + b on the fp64 matrix cores in tiles of 64 rows x 64
output columns, the rows kept) against what there was before for the same columns: the draws copied to the host, then one numpy
product.  1024 chains x 1000 iterations, the buffer exactly K columns wide.  Cases: K x M = 5 x 5 (whitening cfg 2) and 64 x 64 with y
copied to the host and with y kept on the device, 64 x 1024 with y kept on the device, 64 x 64 with sqnorm alone (Y is never written),
copied to the host and kept on the device.  One process; whole-call wall times that end in the call's own synchronise; two warm calls
of each case, then the cases alternating, 9 samples each, a sample the mean of a batch of calls (3 to 200, the short calls in the
longer batches): median, smallest and largest.  Beside each: the bytes the
call must move (x read once, what is asked for written once, and what goes to the host copied) over the call's time, as a share of
8 TB/s -- a whole-call figure, not the kernel's.  The host route: one copy of the buffer, then one run of (x - c) @ W + b in numpy
(BLAS); its figures are compared with the device's at the timed size.  Synthetic draws: 16 distinct chains generated on the host and
uploaded chains / 16 times, each copy with an offset of its own.  Prints one JSON line.

    python tools/linear_timing.py
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
M, N, PEAK = 1024, 1000, 8e12
# name: K, M, to_host, sqnorm, calls per sample (the short calls in longer batches: a sample is tens of milliseconds at the least)
CASES = {"k5_m5_host": (5, 5, True, False, 10), "k5_m5_device": (5, 5, False, False, 200), "k64_m64_host": (64, 64, True, False, 3),
         "k64_m64_device": (64, 64, False, False, 100), "k64_m1024_device": (64, 1024, False, False, 10),
         "k64_m64_sqnorm_only": (64, 64, True, "only", 30), "k64_m64_sqnorm_only_device": (64, 64, False, "only", 100)}


def timed(fn, batch=1):
    t0 = time.perf_counter()
    for _ in range(batch):
        fn()
    return (time.perf_counter() - t0) / batch


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "n": len(ts)}


def upload(rng, k):
    """[M][N][k] on the device: 16 distinct chains, M / 16 copies, each with an offset of its own"""
    blk, ptr = rng.standard_normal((16, N, k)), C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), M * N * k * 8) == 0
    for r in range(M // 16):
        part = blk + 0.05 * rng.standard_normal((16, 1, k))
        assert hip.hipMemcpy(C.c_void_p(ptr.value + r * part.nbytes), part.ctypes.data_as(C.c_void_p), part.nbytes, 1) == 0
    return ptr


def host_route(ptr, lmap):
    """(seconds of the copy, seconds of numpy, y [M N][m])"""
    w, c, b = lmap
    x, out = np.empty((M * N, len(c))), {}
    t_copy = timed(lambda: hip.hipMemcpy(x.ctypes.data_as(C.c_void_p), ptr, x.nbytes, 2))
    t_np = timed(lambda: out.__setitem__("y", (x - c) @ w + b))
    return t_copy, t_np, out["y"]


def main():
    rng = np.random.default_rng(1)
    bufs = {k: upload(rng, k) for k in (5, 64)}
    parts = {(k, m): (rng.standard_normal((k, m)) / np.sqrt(k), 0.1 * rng.standard_normal(k), rng.standard_normal(m)) for k, m, *_ in CASES.values()}
    maps = {km: R.LinearMap(w, center=c, offset=b, device=0) for km, (w, c, b) in parts.items()}
    res = {}

    def call(name):
        k, m, to_host, sqnorm, _ = CASES[name]
        res[name] = R.linear_device(maps[(k, m)], bufs[k].value, M, N, k, device=0, to_host=to_host, sqnorm=sqnorm)
    for name in list(CASES) * 2:
        call(name)
    t = {name: [] for name in CASES}
    for _ in range(9):
        for name in CASES:
            t[name].append(timed(lambda: call(name), CASES[name][4]))
    out = {"chains": M, "iterations": N, "N": M * N, "peak_bytes_per_s": PEAK}
    hosts = {}
    for name, (k, m, to_host, sqnorm, batch) in CASES.items():
        st, rows = stats(t[name]), M * N
        made = rows * 8 if sqnorm == "only" else rows * m * 8
        moved = rows * k * 8 + made + (made if to_host else 0)
        if (k, m) not in hosts:
            compared = any(c[:2] == (k, m) and c[2] for c in CASES.values())     # (64 x 1024: 8 GB of y that nothing is held against)
            hosts[(k, m)] = host_route(bufs[k], parts[(k, m)])[:3 if compared else 2] + (() if compared else (None,))
        t_copy, t_np, want = hosts[(k, m)]
        entry = dict(st, calls_per_sample=batch, x_bytes=rows * k * 8, result_bytes=made, bytes_moved=moved, bytes_per_s=moved / st["median_s"], share_of_peak=moved / st["median_s"] / PEAK,
                     host_copy_s=t_copy, host_numpy_s=t_np, host_over_device=(t_copy + t_np) / st["median_s"])
        if to_host:
            want = (want * want).sum(axis=1) if sqnorm == "only" else want
            entry["largest_difference_over_largest_entry"] = float(np.max(np.abs(res[name].reshape(want.shape) - want)) / np.max(np.abs(want)))
        out[name] = entry
    for lm in maps.values():
        lm.close()
    for p in bufs.values():
        hip.hipFree(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
