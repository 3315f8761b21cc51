"""Times the cross-covariance of two device-resident draw sets (rh_cross_covariance_device: the means and variances of both sides, then
A^T B of the centred rows on the fp64 matrix cores in 32 x 128 tiles, Ka x Kb figures back) against what there was before for the same figures:
both buffers copied to the host, then numpy.  Shapes: 1024 chains x 1000 iterations; Ka = 4 against Kb = 64 and 512, Ka = 64 against
Kb = 512, each side a buffer of exactly that width (a B row is Kb consecutive doubles).  One process; whole-call wall times that end
in the call's own synchronise; two warm calls of each shape, then the shapes alternating, 9 samples each, a sample the mean of a batch
of 5 calls: median, smallest and largest.  Beside each: the bytes of B the tile kernel reads (N Kb 8 per A tile of 32 columns) over
the call's time, as a share of 8 TB/s -- a whole-call figure, not the kernel's.  The host route: one copy of each buffer, then one
run of the centred product in numpy (BLAS); its figures are compared with the device's at the timed size.  Synthetic draws: 16
distinct chains generated on the host and uploaded chains / 16 times, each copy with an offset of its own.  Prints one JSON line.

    python tools/cross_covariance_timing.py
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
M, N, BATCH, PEAK = 1024, 1000, 5, 8e12
SHAPES = ((4, 64), (4, 512), (64, 512))


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


def host_route(pa, ka, pb, kb):
    """(seconds of the two copies, seconds of numpy, cross [ka][kb])"""
    a, b = np.empty((M * N, ka)), np.empty((M * N, kb))
    t_copy = timed(lambda: [hip.hipMemcpy(x.ctypes.data_as(C.c_void_p), p, x.nbytes, 2) for x, p in ((a, pa), (b, pb))])
    out = {}
    t_np = timed(lambda: out.__setitem__("cross", (a - a.mean(axis=0)).T @ (b - b.mean(axis=0)) / (M * N - 1)))
    return t_copy, t_np, out["cross"]


def main():
    rng = np.random.default_rng(1)
    bufs = {k: upload(rng, k) for k in (4, 64, 512)}
    res = {}
    call = lambda ka, kb: res.__setitem__((ka, kb), R.cross_covariance_device(bufs[ka].value, bufs[kb].value, M, N, ka, kb, device=0))
    for shape in SHAPES * 2:
        call(*shape)
    t = {shape: [] for shape in SHAPES}
    for _ in range(9):
        for shape in SHAPES:
            t[shape].append(timed(lambda: call(*shape), BATCH))
    out = {"chains": M, "iterations": N, "N": M * N, "calls_per_sample": BATCH, "peak_bytes_per_s": PEAK}
    for ka, kb in SHAPES:
        st = stats(t[(ka, kb)])
        b_bytes = M * N * kb * 8 * ((ka + 31) // 32)
        t_copy, t_np, want = host_route(bufs[ka], ka, bufs[kb], kb)
        out["ka_%d_kb_%d" % (ka, kb)] = dict(st, a_bytes=M * N * ka * 8, b_bytes_read=b_bytes, b_bytes_per_s=b_bytes / st["median_s"],
                                             share_of_peak=b_bytes / st["median_s"] / PEAK, host_copy_s=t_copy, host_numpy_s=t_np,
                                             host_over_device=(t_copy + t_np) / st["median_s"],
                                             largest_difference_over_largest_entry=float(np.max(np.abs(res[(ka, kb)].cross - want)) / np.max(np.abs(want))))
    for p in bufs.values():
        hip.hipFree(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
