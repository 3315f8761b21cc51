"""Times a posterior predictive check on the device (rh_ppc_device: every replicated data set staged once through LDS and reduced
along its row to the check's statistics, T(y) by the same routine, the counts of the p-values) against the only route there was for
the same answer: the replicated-observations buffer copied to the host and the statistics restated in numpy (mean, std with ddof = 1,
min, max, a sort for the order statistic, a comparison for the share).  Three shapes:

  kidiq             1024 chains x 200 draws x 434 observations (711 MB), one segment, six statistics of which one is a quantile
  kidiq_10_segments the same columns in 10 uneven segments
  narrow            1024 x 1000 x 8

The buffers are made on the host in blocks of 64 chains with seeds of their own and uploaded once.  One process; every figure --
device call, copy, numpy -- is one warm call, then 5 repetitions: the median and all five.  The device call is the whole call: the
upload of y, T(y), the statistics, the counts, their way back and the waits; once with T [S][nout] left on the device and once
copied back.  bytes_read is what the algorithm needs, S * K * 8 (each selected value once), over the whole call's time.
Writes timing.json and README.md into --out (default profiles/ppc_device) and prints the JSON line.  The README ends with
profiles/ppc_device/bench.md as it stands: the record of bench.py on the parent commit and on this tree, which is kept by hand (this
tool does not run the benchmark), so a new timing run keeps it.

    python tools/ppc_device_timing.py [--out DIR]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rainier_amd as R  # noqa: E402

hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
BLOCK = 64
KIDIQ_SEGS = (60, 50, 44, 43, 43, 42, 41, 40, 40, 31)
STREAM_READ_TBS = (6.0, 6.1)      # what an in-order sweep of a large table reads from this part's HBM (8 TB/s peak)


def median5(fn):
    fn()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def host_stats(rows, segments):
    """the check in numpy over rows [S][nin] -> T [S][nseg * 6]"""
    out = np.empty((rows.shape[0], 6 * len(segments)))
    for g, seg in enumerate(segments):
        v = rows[:, seg[0]:seg[-1] + 1]
        n = v.shape[1]
        out[:, 6 * g + 0] = v.mean(axis=1)
        out[:, 6 * g + 1] = v.std(axis=1, ddof=1)
        out[:, 6 * g + 2] = v.min(axis=1)
        out[:, 6 * g + 3] = v.max(axis=1)
        out[:, 6 * g + 4] = np.sort(v, axis=1)[:, min(n - 1, int(np.floor(n * 0.5)))]
        out[:, 6 * g + 5] = (v <= 0.0).mean(axis=1)
    return out


def shape(name, m, n, k, seg_sizes):
    ptr = C.c_void_p()
    nbytes = m * n * k * 8
    assert hip.hipMalloc(C.byref(ptr), nbytes) == 0
    for r in range(m // BLOCK):
        blk = np.random.default_rng(100 + r).standard_normal((BLOCK, n, k))
        assert hip.hipMemcpy(C.c_void_p(ptr.value + r * blk.nbytes), blk.ctypes.data_as(C.c_void_p), blk.nbytes, 1) == 0
    off = np.concatenate([[0], np.cumsum(seg_sizes)])
    segments = [list(range(off[g], off[g + 1])) for g in range(len(seg_sizes))]
    chk = R.Check([R.ppc.mean(), R.ppc.sd(), R.ppc.min(), R.ppc.max(), R.ppc.quantile(0.5), R.ppc.frac_le(0.0)], k, segments=segments, device=0)
    y = np.random.default_rng(7).standard_normal(k)
    S = m * n
    dev, dev_all = median5(lambda: R.ppc_device(chk, ptr.value, m, n, k, y=y, device=0, to_host=False))
    devh, devh_all = median5(lambda: R.ppc_device(chk, ptr.value, m, n, k, y=y, device=0, to_host=True))
    got = R.ppc_device(chk, ptr.value, m, n, k, y=y, device=0)
    back = np.empty((m, n, k))
    copy, copy_all = median5(lambda: hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), ptr, nbytes, 2))
    res = []
    host, host_all = median5(lambda: res.append(host_stats(back.reshape(S, k), segments)))
    want = res[-1]
    have = got.t_rep.reshape(S, chk.nout)
    exact = [o for o in range(chk.nout) if o % 6 >= 2]
    assert np.array_equal(have[:, exact], want[:, exact]) and np.allclose(have, want, rtol=1e-11, atol=1e-13), name
    t_obs = host_stats(y[None, :], segments)[0]
    assert np.array_equal(got.n_gt.reshape(-1)[exact], (want[:, exact] > t_obs[exact]).sum(axis=0)), name
    hip.hipFree(ptr)
    chk.close()
    read = S * k * 8
    out = {"shape": name, "chains": m, "iterations": n, "nin": k, "segments": len(seg_sizes), "statistics": 6, "nout": chk.nout, "S": S, "rep_bytes": nbytes,
           "bytes_read": read, "t_rep_bytes": S * chk.nout * 8, "device_s_median5": dev, "device_s_all": dev_all, "device_with_t_rep_on_host_s_median5": devh,
           "device_with_t_rep_on_host_s_all": devh_all, "achieved_read_TBps_whole_call": read / dev / 1e12, "host_copy_s_median5": copy, "host_copy_s_all": copy_all,
           "host_numpy_s_median5": host, "host_numpy_s_all": host_all, "host_route_s": copy + host, "speedup_over_the_host_route": (copy + host) / dev,
           "p_ge_min": float(np.min(got.p_ge)), "p_ge_max": float(np.max(got.p_ge)), "n_bad": int(got.n_bad.sum())}
    return out


README = """# Posterior predictive checks on the device: timing

`python tools/ppc_device_timing.py` on one MI355X, one process.  Every figure is one warm call, then the median of 5 (all five are in
`timing.json`).  The device figure is the whole call -- the upload of y, T(y), the statistics of every draw, the counts, their way back
and the waits -- with T [S][nout] left on the device; the second device column copies T back as well.  The host route is the copy of
the replicated-observations buffer to the host plus the same statistics in numpy.  There was no device route before, so no ratio was
fixed in advance and none is asserted.

| shape | S | K | segments | nout | device (ms) | device, T on the host (ms) | copy back (s) | numpy (s) | host route / device | bytes read / whole call (TB/s) |
|---|---|---|---|---|---|---|---|---|---|---|
%(rows)s

Bytes read is what the algorithm needs, S x K x 8: each selected value once.  The part's streaming-read rate is %(lo).1f-%(hi).1f TB/s
(a large table swept in order from HBM, whose peak is 8 TB/s).  The figure above is over the whole call's host-clock time, not a kernel time:
it holds the launches of three kernels, one upload, the copies back and one wait.  No kernel trace and no counters were collected,
so how the gap to the streaming rate divides between those fixed costs, the stat kernel's passes over the staged rows (barriers of a
256-thread workgroup per tree level and per sort step, two workgroups of KidIQ's shape per CU) and the memory system is not known.

The exact kinds (min, max, quantile, share) of every draw equal numpy's bit for bit in this run, mean and sd agree to 1e-11, and n_gt of
the exact kinds equals numpy's count.
"""
BENCH = os.path.join(ROOT, "profiles", "ppc_device", "bench.md")     # the benchmark's record, kept by hand, appended as it is


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppc_device"))
    a = ap.parse_args()
    res = [shape("kidiq_1024x200x434", 1024, 200, 434, (434,)), shape("kidiq_1024x200x434_10_segments", 1024, 200, 434, KIDIQ_SEGS),
           shape("narrow_1024x1000x8", 1024, 1000, 8, (8,))]
    os.makedirs(a.out, exist_ok=True)
    line = json.dumps(res)
    open(os.path.join(a.out, "timing.json"), "w").write(line + "\n")
    rows = "\n".join("| %s | %d | %d | %d | %d | %.2f | %.2f | %.3f | %.3f | %.0f | %.3f |" % (
        r["shape"], r["S"], r["nin"], r["segments"], r["nout"], 1e3 * r["device_s_median5"], 1e3 * r["device_with_t_rep_on_host_s_median5"], r["host_copy_s_median5"],
        r["host_numpy_s_median5"], r["speedup_over_the_host_route"], r["achieved_read_TBps_whole_call"]) for r in res)
    bench = "\n" + open(BENCH).read() if os.path.exists(BENCH) else ""
    open(os.path.join(a.out, "README.md"), "w").write(README % dict(rows=rows, lo=STREAM_READ_TBS[0], hi=STREAM_READ_TBS[1]) + bench)
    print(line)
