// rh_trace.hip.h -- Trace.diagnostics (core/Trace.scala:52-120) and the pooled moments over device-resident draws.
//
// Model-independent: a translation unit of its own (no RH_NVARS, no generated code), compiled once per toolchain through the
// engine's build_source() and inspected like every other code object before it is launched.  wave64, gfx950.
//
// draws [chains][iterations][nvars]; analysed: the window [first, first + n) of every chain, all parameters.
//
//   rh_trace_chain_kernel   one workgroup = one chain x a tile of <= RT_TP parameters.  The window is staged in LDS -- whole when
//                           n * tile fits (RT_LDS_DOUBLES), else in time tiles that carry a halo of RT_MAXLAG rows -- and thread
//                           (p, g) of the tile owns the "lag slots" g, g + lpp, g + 2 lpp, ... of parameter p (lpp = RT_BLOCK / tile
//                           width): slot 0 accumulates sum (x_i - mean)^2, slot l >= 1 the variogram sum (x_i - x_{i-l})^2.  The
//                           thread reads x_i once per row and serves up to RT_NACC slots from it.  A narrow tile (nvars small:
//                           the chain's [n][nvars] slab is contiguous and is copied flat) spreads more lags over the lanes; a
//                           full tile runs its lanes along p.  Every sum runs over i in ascending order, in one accumulator:
//                           the order does not depend on the tiling, on `first`, or on the launch.
//                           -> ws [param of the chunk][chain][RT_SL] = { mean, s2, variogram(1) .. variogram(L) }, L = min(99, n-1)
//   rh_trace_finish_kernel  one workgroup per parameter: the sums over chains, in chain order (thread j owns column j of ws), then
//                           B, W, v, rHat and the sequential scan over lags exactly as Trace.scala:100-117.
//
// No floating-point atomics; results are bit-identical from run to run and a window gives the bits of a copy of its rows.
// Workspace: the host walks the parameters in chunks so that ws stays below RT_WS_CAP_BYTES (128 MiB) whatever
// chains x lags x nvars is -- at 1024 chains a chunk is 160 parameters.
//
// The two block routines below are plain C++ over (thread id, LDS pointer): with RH_TRACE_HOST defined they compile with a host
// compiler, every "thread" of a phase run in turn (tests/test_trace_device_cpu.py), same text, same summation order.
#ifndef RH_TRACE_HIP_H
#define RH_TRACE_HIP_H

#define RT_BLOCK 256         // threads of rh_trace_chain_kernel
#define RT_TP 16             // parameters per tile
#define RT_MAXLAG 99         // Trace.scala:112: lags 1 .. 99 enter the sum
#define RT_SL 101            // doubles per (parameter, chain) in the workspace: mean, s2, 99 variograms
#define RT_NACC 7            // lag slots per thread: ceil((RT_MAXLAG + 1) / (RT_BLOCK / RT_TP))
#define RT_LDS_DOUBLES 8064  // staged rows: 63 KiB of the workgroup's 64 KiB (two workgroups per CU's 160 KiB)
#define RT_FIN_BLOCK 128     // threads of rh_trace_finish_kernel (>= RT_SL)
#define RT_WS_CAP_BYTES (128ll << 20)

#ifndef RH_TRACE_HOST
#define RT_FN static __device__ __forceinline__
#define RT_SYNC() __syncthreads()
#define RT_TID0 ((int)threadIdx.x)
#define RT_TID1 ((int)threadIdx.x + 1)
#define RT_ST(tid) 0
#define RT_NSTATE 1
#else
#define RT_FN static inline
#define RT_SYNC() ((void)0)
#define RT_TID0 0
#define RT_TID1 rt_nthreads
#define RT_ST(tid) (tid)
#define RT_NSTATE RT_BLOCK
#endif
// every thread of the workgroup (device: this one; host: each in turn -- a phase ends where the device has its barrier)
#define RT_EACH_THREAD(tid) for (int tid = RT_TID0; tid < RT_TID1; tid++)

// rows [r0, r1) of the tile -> lds[(r - r0) * tpw + p]; x = the chain's window at the tile's first parameter, row stride nvars
RT_FN void rt_stage(const double *x, const long long nvars, const int tpw, const int r0, const int r1, double *lds, const int rt_nthreads) {
  const int total = (r1 - r0) * tpw;
  RT_EACH_THREAD(tid) {
    for (int j = tid; j < total; j += RT_BLOCK) {
      const int r = j / tpw, p = j - r * tpw;
      lds[j] = x[(long long)(r0 + r) * nvars + p];
    }
  }
}

// One chain x one tile of tpw parameters over the window of n rows.  lds: RT_LDS_DOUBLES doubles of rows + RT_TP means.
// out: the workspace entry of (tile's first parameter, this chain); the next parameter's is out_pstride doubles further.
RT_FN void rt_chain_block(const double *x, const long long nvars, const int n, const int tpw, double *lds, double *out,
                          const long long out_pstride, const int rt_nthreads) {
  double *lds_mean = lds + RT_LDS_DOUBLES;
  const int L = n - 1 < RT_MAXLAG ? n - 1 : RT_MAXLAG;
  const int lpp = RT_BLOCK / tpw;                  // lag slots served per pass over the threads
  const int cap_rows = RT_LDS_DOUBLES / tpw;
  const bool resident = n <= cap_rows;             // the whole window stays in LDS: the draws are read once
  const int T = resident ? n : cap_rows - RT_MAXLAG;
  double sum[RT_NSTATE], acc[RT_NSTATE][RT_NACC];
  RT_EACH_THREAD(tid) {
    sum[RT_ST(tid)] = 0.0;
#pragma unroll
    for (int k = 0; k < RT_NACC; k++) acc[RT_ST(tid)][k] = 0.0;
  }
  // pass 0: the chain's means (thread p < tpw sums parameter p over the rows, in order)
  for (int t0 = 0; t0 < n; t0 += T) {
    const int t1 = t0 + T < n ? t0 + T : n;
    RT_SYNC();
    rt_stage(x, nvars, tpw, t0, t1, lds, rt_nthreads);
    RT_SYNC();
    RT_EACH_THREAD(tid) {
      if (tid < tpw) {
        double s = sum[RT_ST(tid)];
        for (int i = 0; i < t1 - t0; i++) s += lds[i * tpw + tid];
        sum[RT_ST(tid)] = s;
      }
    }
  }
  RT_EACH_THREAD(tid) {
    if (tid < tpw) lds_mean[tid] = sum[RT_ST(tid)] / (double)n;
  }
  RT_SYNC();
  // pass 1: sum (x_i - mean)^2 (slot 0) and the variogram sums (slot = lag), every one over i ascending
  for (int t0 = 0; t0 < n; t0 += T) {
    const int t1 = t0 + T < n ? t0 + T : n;
    const int h0 = t0 - RT_MAXLAG > 0 ? t0 - RT_MAXLAG : 0;   // the halo: the rows the tile's lags reach back to
    if (!resident) {
      RT_SYNC();
      rt_stage(x, nvars, tpw, h0, t1, lds, rt_nthreads);
      RT_SYNC();
    }
    RT_EACH_THREAD(tid) {
      const int g = tid / tpw, p = tid - g * tpw;
      if (g < lpp) {
        const double mean = lds_mean[p];
        for (int i = t0; i < t1; i++) {
          const double xi = lds[(i - h0) * tpw + p];
#pragma unroll
          for (int k = 0; k < RT_NACC; k++) {
            const int slot = g + k * lpp;
            if (slot <= L && i >= slot) {
              const double prev = slot == 0 ? mean : lds[(i - slot - h0) * tpw + p];
              const double d = xi - prev;
              acc[RT_ST(tid)][k] += d * d;
            }
          }
        }
      }
    }
  }
  RT_EACH_THREAD(tid) {
    const int g = tid / tpw, p = tid - g * tpw;
    if (g < lpp) {
      double *o = out + (long long)p * out_pstride;
#pragma unroll
      for (int k = 0; k < RT_NACC; k++) {
        const int slot = g + k * lpp;
        if (slot <= L) o[1 + slot] = acc[RT_ST(tid)][k] / (double)(slot == 0 ? n - 1 : n - slot);   // s2 = sum / (n - 1); variogram(l) = sum / (n - l)
      }
      if (g == 0) o[0] = lds_mean[p];
    }
  }
}

// One parameter: w [chains][RT_SL] -> rHat, ess, meanMean, v.  lds: RT_SL + RT_FIN_BLOCK doubles.
RT_FN void rt_param_finish(const double *w, const int chains, const int n, double *lds, double *rhat, double *ess, double *mean_out,
                           double *var_out, const int rt_nthreads) {
  double *tmp = lds + RT_SL;
  const int L = n - 1 < RT_MAXLAG ? n - 1 : RT_MAXLAG;
  const double m = (double)chains, nn = (double)n;
  RT_EACH_THREAD(tid) {
    if (tid < L + 2) {
      double s = 0.0;
#pragma unroll 8
      for (int c = 0; c < chains; c++) s += w[(long long)c * RT_SL + tid];
      lds[tid] = s;
    }
  }
  RT_SYNC();
  const double mm = lds[0] / m;          // meanMean (Trace.scala:69)
  double bs = 0.0;                        // sum over chains of (mean_c - meanMean)^2, in chain order (thread 0)
  for (int c0 = 0; c0 < chains; c0 += RT_FIN_BLOCK) {
    RT_EACH_THREAD(tid) {
      if (c0 + tid < chains) { const double d = w[(long long)(c0 + tid) * RT_SL] - mm; tmp[tid] = d * d; }
    }
    RT_SYNC();
    RT_EACH_THREAD(tid) {
      if (tid == 0) {
        const int cnt = chains - c0 < RT_FIN_BLOCK ? chains - c0 : RT_FIN_BLOCK;
        for (int j = 0; j < cnt; j++) bs += tmp[j];
      }
    }
    RT_SYNC();
  }
  RT_EACH_THREAD(tid) {
    if (tid == 0) {
      const double b = (nn / (m - 1.0)) * bs;
      const double W = lds[1] / m;
      const double v = (nn - 1.0) / nn * W + b / nn;
      *rhat = __builtin_sqrt(v / W);
      double acc = 0.0;
      // Trace.scala:100-117: acc += pt while pt > 0 and lag < 100; at lag == n the variogram is 0/0 = NaN and the scan stops
      for (int lag = 1; lag <= L; lag++) {
        const double vt = lds[1 + lag] / m;
        const double pt = 1.0 - (vt / (2.0 * v));
        if (!(pt > 0.0)) break;
        acc += pt;
      }
      *ess = nn * m / (1.0 + (2.0 * acc));
      if (mean_out) *mean_out = mm;
      if (var_out) *var_out = v;
    }
  }
}

#ifndef RH_TRACE_HOST
// grid: chains x tiles of the chunk [p_lo, p_lo + p_cnt), blockIdx.x = tile * chains + chain
extern "C" __global__ void __launch_bounds__(RT_BLOCK)
rh_trace_chain_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const int first, const int n,
                      const int chains, const int p_lo, const int p_cnt, double *__restrict__ ws) {
  __shared__ double lds[RT_LDS_DOUBLES + RT_TP];
  const int tile = (int)(blockIdx.x / (unsigned)chains), c = (int)(blockIdx.x - (unsigned)tile * (unsigned)chains);
  const int pl = tile * RT_TP;
  if (pl >= p_cnt) return;
  const int tpw = p_cnt - pl < RT_TP ? p_cnt - pl : RT_TP;
  const double *x = draws + ((long long)c * iterations + first) * nvars + p_lo + pl;
  rt_chain_block(x, nvars, n, tpw, lds, ws + ((long long)pl * chains + c) * RT_SL, (long long)chains * RT_SL, RT_BLOCK);
}

// grid: the chunk's parameters; rhat / ess / mean / var are indexed by the global parameter
extern "C" __global__ void __launch_bounds__(RT_FIN_BLOCK)
rh_trace_finish_kernel(const double *__restrict__ ws, const int chains, const int n, const int p_lo, double *__restrict__ rhat,
                       double *__restrict__ ess, double *__restrict__ mean, double *__restrict__ var) {
  __shared__ double lds[RT_SL + RT_FIN_BLOCK];
  const int pl = (int)blockIdx.x, p = p_lo + pl;
  rt_param_finish(ws + (long long)pl * chains * RT_SL, chains, n, lds, rhat + p, ess + p, mean + p, var + p, RT_FIN_BLOCK);
}
#endif
#endif
