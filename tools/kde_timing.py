"""Times the kernel density estimates on the device (rh_kde_device: one pass of exponentials per split, G doubles per column back;
rh_kde_pairs_device: the two operand blocks generated into LDS, the surface as a matrix product on the fp64 matrix cores) against
what there was before for the same figures: the draws copied to the host, then numpy.  Shape: cfg 2's (1024 chains x 1000 iterations
x 5 parameters); curves of all 5 columns at 512 points, surfaces of the pairs (0, 1) and (2, 3) at 64 x 64 and 128 x 128.  Bandwidths
and bounds are given, so that the calls timed are the kernels' (a rule would add one summary call).  One process; whole-call wall
times that end in the call's own synchronise; two warm calls of each, then the three device calls alternating, 9 samples each, a
sample the mean of a batch of 5 calls: median, smallest and largest.  The host route: one copy, then one run each of the curve of ONE
column (in blocks of 16 grid points) and of ONE 64 x 64 surface (exponentials per axis, then a BLAS product).  The device figures are
compared with the host route's at the timed size.  Synthetic draws: 16 distinct chains generated on the host and uploaded chains / 16
times, each copy with an offset of its own.  Prints one JSON line.

    python tools/kde_timing.py
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
M, N, K, G, BATCH, H, LO, HI = 1024, 1000, 5, 512, 5, 0.07, -4.5, 4.5
PAIRS = [(0, 1), (2, 3)]


def timed(fn, batch=1):
    t0 = time.perf_counter()
    for _ in range(batch):
        fn()
    return (time.perf_counter() - t0) / batch


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "n": len(ts)}


def phi(v, grid):
    z = (grid[:, None] - v[None, :]) / H
    return np.exp(-0.5 * z * z)


def host_curve(v, grid):
    return np.concatenate([phi(v, g).sum(axis=1) for g in np.split(grid, len(grid) // 16)]) / (len(v) * H * np.sqrt(2 * np.pi))


def host_surface(a, b, xgrid, ygrid):
    return phi(a, xgrid) @ phi(b, ygrid).T / (len(a) * 2 * np.pi * H * H)


def main():
    rng = np.random.default_rng(1)
    blk = rng.standard_normal((16, N, K))
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), M * N * K * 8) == 0
    for r in range(M // 16):
        part = blk + 0.05 * rng.standard_normal((16, 1, K))
        assert hip.hipMemcpy(C.c_void_p(ptr.value + r * part.nbytes), part.ctypes.data_as(C.c_void_p), part.nbytes, 1) == 0
    res = {}
    box = ((LO, HI), (LO, HI))
    curve = lambda: res.__setitem__("curve", R.kde_device(ptr.value, M, N, K, device=0, points=G, bw=H, range=(LO, HI)))
    small = lambda: res.__setitem__("small", R.kde_pairs_device(ptr.value, M, N, K, PAIRS, device=0, points=(64, 64), bw=H, range=box))
    large = lambda: res.__setitem__("large", R.kde_pairs_device(ptr.value, M, N, K, PAIRS, device=0, points=(128, 128), bw=H, range=box))
    for fn in (curve, small, large) * 2:
        fn()
    t = {"curve": [], "small": [], "large": []}
    for _ in range(9):
        for name, fn in (("curve", curve), ("small", small), ("large", large)):
            t[name].append(timed(fn, BATCH))
    back = np.empty((M, N, K))
    t_copy = timed(lambda: hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), ptr, back.nbytes, 2))
    hip.hipFree(ptr)
    flat = back.reshape(-1, K)
    t_hc = timed(lambda: res.__setitem__("hcurve", host_curve(np.ascontiguousarray(flat[:, 0]), res["curve"].grid[0])))
    t_hs = timed(lambda: res.__setitem__("hsurf", host_surface(np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1]), res["small"].xgrid[0],
                                                                res["small"].ygrid[0])))
    rel = lambda got, want: float(np.max(np.abs(got - want) / want))
    c, s, l = stats(t["curve"]), stats(t["small"]), stats(t["large"])
    draws = M * N
    print(json.dumps({"chains": M, "iterations": N, "nvars": K, "N": draws, "bw": H, "calls_per_sample": BATCH, "draws_bytes": draws * K * 8,
                      "kde_device_5_columns_512_points": c, "kde_pairs_device_2_pairs_64x64": s, "kde_pairs_device_2_pairs_128x128": l,
                      "exponentials": {"curves": K * G * draws, "pairs_64": 2 * 128 * draws, "pairs_128": 2 * 4 * 128 * draws,   # 128 N per 64 x 64 tile
                                       "pairs_64_naive": 2 * 64 * 64 * draws, "pairs_128_naive": 2 * 128 * 128 * draws},
                      "pairs_128_over_64": l["median_s"] / s["median_s"], "host_copy_s": t_copy, "host_numpy_one_column_512_points_s": t_hc,
                      "host_numpy_one_pair_64x64_s": t_hs, "host_one_column_over_device_per_column": (t_copy + t_hc) / (c["median_s"] / K),
                      "host_one_pair_over_device_per_pair": (t_copy + t_hs) / (s["median_s"] / len(PAIRS)),
                      "largest_relative_difference_curve": rel(res["curve"].density[0], res["hcurve"]),
                      "largest_relative_difference_surface": rel(res["small"].density[0], res["hsurf"])}))


if __name__ == "__main__":
    main()
