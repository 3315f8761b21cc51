// rh_summary.hip.h -- posterior summaries over device-resident draws: order statistics (precis' credible interval), the
// highest-density interval (hdpi) and the pooled mean / standard deviation (rainier-notebook package.scala:327-342, 367-418,
// 456-469).  All of them read the SORTED pooled column of a parameter, so this is a segmented sort of strided fp64 columns.
//
// Model-independent: a translation unit of its own (no RH_NVARS, no generated code), compiled once per toolchain through the
// engine's build_source() and inspected like every other code object before it is launched.  wave64, gfx950.
//
// draws [chains][iterations][nvars].  The pooled column of parameter p: x[c][first + j * thin][p], c = 0 .. chains-1 (outer),
// j = 0 .. kept-1 (inner), N = chains * kept values.  Order: java.lang.Double.compare's (-0.0 < +0.0, every NaN -- made the
// positive quiet NaN on load -- after +inf), through the usual 64-bit key: negatives have all bits flipped, the others the sign
// bit, and keys compare unsigned.  A key carries no payload, so the sorted column is unique: any correct sort gives these bits.
//
//   rh_summary_sort_kernel    one workgroup = one parameter x one tile of RS_TILE pooled values: gathered from the strided draws,
//                             made keys, sorted in LDS by a bitonic network (a ragged tile is filled up with the all-ones key, which
//                             no value has), written as a sorted run.  Thread t keeps elements 16t .. 16t+15 in registers for
//                             the steps of stride <= 8; the steps of stride >= 16 go pairwise through LDS.  LDS image: element e
//                             at slot e + (e >> 4) (one pad per 16), which makes the register phase's ds_read_b64 / ds_write_b64
//                             (lane stride 17 slots) conflict-free; in the pairwise steps lanes 16..31 of a half wave take the
//                             run 256 elements on from lanes 0..15 (slot distance 272 = 16 mod 32: the other half of the 64
//                             banks) -- conflict-free but for stride 256, where that element bit is the stride itself and one
//                             bank pair is hit twice (3 LDS cycles instead of 2, in 4 of the 36 pairwise steps; 42 steps run in registers).
//   rh_summary_merge_kernel   one pass of merge-path merges of pairs of runs, from one workspace buffer to the other: a workgroup
//                             produces RS_MERGE_TILE outputs of one parameter after a binary search of its two diagonals, stages
//                             its two input segments in LDS, and every thread merges RS_MERGE_E outputs from its own diagonal.
//                             ceil(log2(ceil(N / RS_TILE))) passes; none when N <= RS_TILE.
//   rh_summary_finish_kernel  one workgroup per parameter over its sorted column: the order statistics at the indices the host
//                             computed, mean and sd in two passes, and the hdpi scan as a minimum over (width, i) compared
//                             lexicographically (width in Double.compare's order, so a NaN width -- inf - inf -- loses).
//
// Sums: thread t adds the sorted values i = t, t + RS_BLOCK, ... in ascending i, then the RS_BLOCK partial sums are added as a
// fixed binary tree.  The order depends on N alone -- not on the chunking of the parameters, on the tiling or on the call.  No
// floating-point atomics; no result depends on the launch order.
// Workspace: two ping-pong buffers of N keys per parameter (2 * N * 8 bytes); the host walks the parameters in chunks so that
// they stay below RS_WS_CAP_BYTES (128 MiB, the trace kernels' figure) and refuses a single column beyond it.
//
// The block routines below are plain C++ over (thread id, LDS pointer): with RH_SUMMARY_HOST defined they compile with a host
// compiler, every "thread" of a phase run in turn (tests/test_summary_device_cpu.py): same text, same summation order.
#ifndef RH_SUMMARY_HIP_H
#define RH_SUMMARY_HIP_H

#define RS_BLOCK 256            // threads of every kernel here
#define RS_TILE 4096            // keys of a tile sort: 16 per thread, 34 KiB of LDS with the pads (four workgroups per CU's 160 KiB)
#define RS_TILE_SLOTS (RS_TILE + RS_TILE / 16)
#define RS_MERGE_TILE 2048      // outputs of a merge workgroup (divides RS_TILE: an output tile never straddles two pairs of runs)
#define RS_MERGE_E 8            // outputs per thread: RS_MERGE_TILE / RS_BLOCK
#define RS_MERGE_OUT_SLOTS (RS_MERGE_TILE + RS_MERGE_TILE / 8)
#define RS_MERGE_LDS (RS_MERGE_TILE + RS_MERGE_OUT_SLOTS + 2)
#define RS_MAX_PROBS 16
#define RS_WS_CAP_BYTES (128ll << 20)

typedef unsigned long long rs_key;
#define RS_KEY_FILL 0xffffffffffffffffull   // above every key (the canonical NaN's is 0xfff8000000000000)
#define RS_KEY_NAN 0xfff8000000000000ull

#ifndef RH_SUMMARY_HOST
#define RS_FN static __device__ __forceinline__
#define RS_SYNC() __syncthreads()
#define RS_TID0 ((int)threadIdx.x)
#define RS_TID1 ((int)threadIdx.x + 1)
#else
#define RS_FN static inline
#define RS_SYNC() ((void)0)
#define RS_TID0 0
#define RS_TID1 rs_nthreads
#endif
// every thread of the workgroup (device: this one; host: each in turn -- a phase ends where the device has its barrier)
#define RS_EACH_THREAD(tid) for (int tid = RS_TID0; tid < RS_TID1; tid++)

RS_FN rs_key rs_to_key(const double x) {
  rs_key b;
  __builtin_memcpy(&b, &x, 8);
  if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;   // every NaN: the positive quiet NaN
  return b ^ ((b >> 63) ? 0xffffffffffffffffull : 0x8000000000000000ull);
}
RS_FN double rs_from_key(const rs_key k) {
  const rs_key b = k ^ ((k >> 63) ? 0x8000000000000000ull : 0xffffffffffffffffull);
  double x;
  __builtin_memcpy(&x, &b, 8);
  return x;
}

// ---- tile sort -------------------------------------------------------------------------------------------------------------------
#define RS_SLOT(e) ((e) + ((e) >> 4))
#define RS_CE(a, b, up)                                        \
  {                                                            \
    const rs_key x_ = (a), y_ = (b);                           \
    const bool sw_ = (x_ > y_) == (up);                        \
    (a) = sw_ ? y_ : x_;                                       \
    (b) = sw_ ? x_ : y_;                                       \
  }

// the steps of stride jmax, jmax / 2, ... 1 of stage k on the 16 keys r[] of elements base .. base + 15 (all indices static)
RS_FN void rs_local_steps(rs_key *r, const int base, const int k, const int jmax) {
#pragma unroll
  for (int j = 8; j >= 1; j >>= 1) {
    if (j <= jmax) {
#pragma unroll
      for (int i = 0; i < 16; i++) {
        if ((i & j) == 0) {
          const bool up = ((base + i) & k) == 0;
          RS_CE(r[i], r[i + j], up);
        }
      }
    }
  }
}

// The lower element of pair i (0 <= i < RS_TILE / 2) of a pairwise step of stride j >= 16; the upper one is j further.  Bit 4 of the
// pair index (lanes 16..31 of a half wave) trades places with the bit that becomes element bit 8, except at j == 256 where that bit
// is the stride.  (tests/test_summary_device_cpu.py enumerates the banks of every step from this function and RS_SLOT.)
RS_FN int rs_pair_lo(int i, const int j) {
  if (j != 256) {
    const int sb = j > 256 ? 8 : 7;
    const int d = ((i >> 4) ^ (i >> sb)) & 1;
    i ^= (d << 4) | (d << sb);
  }
  return ((i & ~(j - 1)) << 1) | (i & (j - 1));
}

// One parameter x one tile.  col: the draws at [chain 0][iteration `first`][this parameter]; pooled value g is
// col[((g / kept) * iterations + (g % kept) * thin) * nvars].  The tile holds the pooled values g0 .. min(g0 + RS_TILE, N) - 1 and
// is written, sorted, to run[0 .. that many).  lds: RS_TILE_SLOTS keys.
RS_FN void rs_tile_sort(const double *col, const long long iterations, const long long nvars, const long long thin, const long long kept,
                        const long long N, const long long g0, rs_key *lds, rs_key *run, const int rs_nthreads) {
  const int nv = (int)(N - g0 < RS_TILE ? N - g0 : RS_TILE);
  RS_EACH_THREAD(tid) {
#pragma unroll 4
    for (int q = 0; q < RS_TILE / RS_BLOCK; q++) {
      const int e = tid + q * RS_BLOCK;
      rs_key key = RS_KEY_FILL;
      if (e < nv) {
        const long long g = g0 + e, c = g / kept, j = g - c * kept;
        key = rs_to_key(col[(c * iterations + j * thin) * nvars]);
      }
      lds[RS_SLOT(e)] = key;
    }
  }
  RS_SYNC();
  // stages 2 .. 16 never leave a thread's 16 elements
  RS_EACH_THREAD(tid) {
    rs_key r[16];
#pragma unroll
    for (int i = 0; i < 16; i++) r[i] = lds[17 * tid + i];
    rs_local_steps(r, 16 * tid, 2, 1);
    rs_local_steps(r, 16 * tid, 4, 2);
    rs_local_steps(r, 16 * tid, 8, 4);
    rs_local_steps(r, 16 * tid, 16, 8);
#pragma unroll
    for (int i = 0; i < 16; i++) lds[17 * tid + i] = r[i];
  }
  RS_SYNC();
  for (int k = 32; k <= RS_TILE; k <<= 1) {
    for (int j = k >> 1; j >= 16; j >>= 1) {
      RS_EACH_THREAD(tid) {
#pragma unroll 4
        for (int q = 0; q < RS_TILE / 2 / RS_BLOCK; q++) {
          const int lo = rs_pair_lo(tid + q * RS_BLOCK, j), hi = lo + j;
          const bool up = (lo & k) == 0;
          rs_key a = lds[RS_SLOT(lo)], b = lds[RS_SLOT(hi)];
          RS_CE(a, b, up);
          lds[RS_SLOT(lo)] = a;
          lds[RS_SLOT(hi)] = b;
        }
      }
      RS_SYNC();
    }
    RS_EACH_THREAD(tid) {
      rs_key r[16];
#pragma unroll
      for (int i = 0; i < 16; i++) r[i] = lds[17 * tid + i];
      rs_local_steps(r, 16 * tid, k, 8);
#pragma unroll
      for (int i = 0; i < 16; i++) lds[17 * tid + i] = r[i];
    }
    RS_SYNC();
  }
  RS_EACH_THREAD(tid) {
#pragma unroll 4
    for (int q = 0; q < RS_TILE / RS_BLOCK; q++) {
      const int e = tid + q * RS_BLOCK;
      if (e < nv) run[e] = lds[RS_SLOT(e)];
    }
  }
}

// ---- merge pass ------------------------------------------------------------------------------------------------------------------
// how many of the first d outputs of merge(A[0, na), B[0, nb)) come from A (on a tie A goes first); 0 <= d <= na + nb
RS_FN long long rs_merge_split(const rs_key *A, const long long na, const rs_key *B, const long long nb, const long long d) {
  long long lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (A[mid] <= B[d - 1 - mid]) lo = mid + 1; else hi = mid;
  }
  return lo;
}

#define RS_OSLOT(i) ((i) + ((i) >> 3))
// One parameter's column of N keys in sorted runs of L (the last one ragged): outputs [o0, min(o0 + RS_MERGE_TILE, N)) of the
// pass that merges runs 2m and 2m + 1 (a last run without a partner is copied).  lds: RS_MERGE_LDS keys.
RS_FN void rs_merge_tile(const rs_key *src, rs_key *dst, const long long N, const long long L, const long long o0, rs_key *lds,
                         const int rs_nthreads) {
  rs_key *lds_in = lds, *lds_out = lds + RS_MERGE_TILE, *lds_sp = lds_out + RS_MERGE_OUT_SLOTS;
  const long long ps = o0 / (2 * L) * (2 * L);                 // the pair's first key
  const long long na = N - ps < L ? N - ps : L, nb = N - ps - na < L ? N - ps - na : L;
  const rs_key *A = src + ps, *B = A + na;
  const long long d0 = o0 - ps, d1 = d0 + RS_MERGE_TILE < na + nb ? d0 + RS_MERGE_TILE : na + nb;
  RS_EACH_THREAD(tid) {
    if (tid < 2) lds_sp[tid] = (rs_key)rs_merge_split(A, na, B, nb, tid ? d1 : d0);
  }
  RS_SYNC();
  const long long a0 = (long long)lds_sp[0], a1 = (long long)lds_sp[1], b0 = d0 - a0;
  const int sna = (int)(a1 - a0), n_out = (int)(d1 - d0), snb = n_out - sna;
  RS_EACH_THREAD(tid) {
#pragma unroll 4
    for (int q = 0; q < RS_MERGE_E; q++) {
      const int i = tid + q * RS_BLOCK;
      if (i < n_out) lds_in[i] = i < sna ? A[a0 + i] : B[b0 + (i - sna)];
    }
  }
  RS_SYNC();
  RS_EACH_THREAD(tid) {
    const int d = tid * RS_MERGE_E < n_out ? tid * RS_MERGE_E : n_out;
    int ai = (int)rs_merge_split(lds_in, sna, lds_in + sna, snb, d), bi = d - ai;
    for (int k = 0; k < RS_MERGE_E; k++) {
      if (d + k < n_out) {
        const bool take_a = bi >= snb || (ai < sna && lds_in[ai] <= lds_in[sna + bi]);
        lds_out[RS_OSLOT(d + k)] = take_a ? lds_in[ai] : lds_in[sna + bi];
        ai += take_a ? 1 : 0;
        bi += take_a ? 0 : 1;
      }
    }
  }
  RS_SYNC();
  RS_EACH_THREAD(tid) {
#pragma unroll 4
    for (int q = 0; q < RS_MERGE_E; q++) {
      const int i = tid + q * RS_BLOCK;
      if (i < n_out) dst[o0 + i] = lds_out[RS_OSLOT(i)];
    }
  }
}

// ---- finish ----------------------------------------------------------------------------------------------------------------------
// lds_d[0 .. RS_BLOCK) summed into lds_d[0] as a fixed binary tree
RS_FN void rs_tree_sum(double *lds_d, const int rs_nthreads) {
  for (int w = RS_BLOCK / 2; w >= 1; w >>= 1) {
    RS_SYNC();
    RS_EACH_THREAD(tid) {
      if (tid < w) lds_d[tid] += lds_d[tid + w];
    }
  }
  RS_SYNC();
}

// One parameter: s = its sorted column of N keys.  idx [nprobs]: the order statistics asked for (0 <= idx < N); hidx: the hdpi's
// ceil(prob * N) in 1 .. N, or 0 for "not asked for".  lds: 3 * RS_BLOCK 8-byte words.  quant [nprobs], hdpi [2].
RS_FN void rs_param_finish(const rs_key *s, const long long N, const long long *idx, const int nprobs, const long long hidx, rs_key *lds,
                           double *mean_out, double *sd_out, double *quant, double *hdpi, const int rs_nthreads) {
  double *lds_d = (double *)lds;
  rs_key *lds_k = lds + RS_BLOCK;
  long long *lds_i = (long long *)(lds + 2 * RS_BLOCK);
  RS_EACH_THREAD(tid) {
    if (tid < nprobs) quant[tid] = rs_from_key(s[idx[tid]]);
  }
  // mean = sum x / N, then sd = sqrt(sum (x - mean)^2 / N): two passes, so that a mean far from zero costs no digits
  RS_EACH_THREAD(tid) {
    double acc = 0.0;
    for (long long i = tid; i < N; i += RS_BLOCK) acc += rs_from_key(s[i]);
    lds_d[tid] = acc;
  }
  rs_tree_sum(lds_d, rs_nthreads);
  const double mean = lds_d[0] / (double)N;
  RS_SYNC();
  RS_EACH_THREAD(tid) {
    double acc = 0.0;
    for (long long i = tid; i < N; i += RS_BLOCK) {
      const double d = rs_from_key(s[i]) - mean;
      acc += d * d;
    }
    lds_d[tid] = acc;
  }
  rs_tree_sum(lds_d, rs_nthreads);
  RS_EACH_THREAD(tid) {
    if (tid == 0) {
      *mean_out = mean;
      *sd_out = __builtin_sqrt(lds_d[0] / (double)N);
    }
  }
  if (hidx <= 0) return;
  const double nan = rs_from_key(RS_KEY_NAN);
  if (s[N - 1] == RS_KEY_NAN || hidx >= N) {      // a NaN sorts last: the column holds one
    const bool has_nan = s[N - 1] == RS_KEY_NAN;
    RS_EACH_THREAD(tid) {
      if (tid == 0) {
        hdpi[0] = has_nan ? nan : rs_from_key(s[0]);
        hdpi[1] = has_nan ? nan : rs_from_key(s[N - 1]);
      }
    }
    return;
  }
  // min over i in [0, N - hidx) of (width_i, i), width_i = sorted[i + hidx] - sorted[i]: minBy's first minimum
  RS_EACH_THREAD(tid) {
    rs_key best = RS_KEY_FILL;
    long long bi = 0x7fffffffffffffffll;
    for (long long i = tid; i < N - hidx; i += RS_BLOCK) {
      const rs_key w = rs_to_key(rs_from_key(s[i + hidx]) - rs_from_key(s[i]));
      if (w < best) { best = w; bi = i; }
    }
    lds_k[tid] = best;
    lds_i[tid] = bi;
  }
  for (int w = RS_BLOCK / 2; w >= 1; w >>= 1) {
    RS_SYNC();
    RS_EACH_THREAD(tid) {
      if (tid < w) {
        const rs_key ok = lds_k[tid + w];
        const long long oi = lds_i[tid + w];
        if (ok < lds_k[tid] || (ok == lds_k[tid] && oi < lds_i[tid])) { lds_k[tid] = ok; lds_i[tid] = oi; }
      }
    }
  }
  RS_SYNC();
  RS_EACH_THREAD(tid) {
    if (tid == 0) {
      const long long i = lds_i[0];
      hdpi[0] = rs_from_key(s[i]);
      hdpi[1] = rs_from_key(s[i + hidx]);
    }
  }
}

#ifndef RH_SUMMARY_HOST
// The workspace holds, for the chunk's parameters [p_lo, p_lo + p_cnt), two buffers [p_cnt][N] of keys.
// grid: tiles x p_cnt, blockIdx.x = tile * p_cnt + (parameter - p_lo).  A lane reads 8 bytes of its own row (one cache line per lane
// once nvars * thin >= 16); the parameter runs fastest over the workgroups so that those in flight together want neighbouring doubles
// of the same lines.  How often a line is then fetched -- the workgroups are spread over 8 XCDs with an L2 each -- has NOT been
// measured: the intent is one fetch from HBM behind the shared last-level cache, several L2 fills.  Staging rows through LDS with
// the lanes along the parameters (as rh_trace.hip.h does) would need a workgroup to own several parameters' tiles; not done here.
extern "C" __global__ void __launch_bounds__(RS_BLOCK)
rh_summary_sort_kernel(const double *__restrict__ draws, const long long iterations, const long long nvars, const long long first,
                       const long long thin, const long long kept, const long long N, const int p_lo, const int p_cnt,
                       rs_key *__restrict__ ws) {
  __shared__ rs_key lds[RS_TILE_SLOTS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const int pl = (int)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt);
  const long long g0 = tile * RS_TILE;
  if (g0 >= N) return;
  rs_tile_sort(draws + first * nvars + p_lo + pl, iterations, nvars, thin, kept, N, g0, lds, ws + (long long)pl * N + g0, RS_BLOCK);
}

// one merge pass over runs of L keys, src -> dst ([p_cnt][N] each); grid: ceil(N / RS_MERGE_TILE) x p_cnt
extern "C" __global__ void __launch_bounds__(RS_BLOCK)
rh_summary_merge_kernel(const rs_key *__restrict__ src, rs_key *__restrict__ dst, const long long N, const long long L, const int p_cnt) {
  __shared__ rs_key lds[RS_MERGE_LDS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const int pl = (int)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt);
  const long long o0 = tile * RS_MERGE_TILE;
  if (o0 >= N) return;
  rs_merge_tile(src + (long long)pl * N, dst + (long long)pl * N, N, L, o0, lds, RS_BLOCK);
}

// grid: the chunk's parameters; sorted [p_cnt][N]; the outputs are indexed by the global parameter
extern "C" __global__ void __launch_bounds__(RS_BLOCK)
rh_summary_finish_kernel(const rs_key *__restrict__ sorted, const long long N, const long long *__restrict__ idx, const int nprobs,
                         const long long hidx, const int p_lo, double *__restrict__ mean, double *__restrict__ sd,
                         double *__restrict__ quant, double *__restrict__ hdpi) {
  __shared__ rs_key lds[3 * RS_BLOCK];
  const int pl = (int)blockIdx.x, p = p_lo + pl;
  rs_param_finish(sorted + (long long)pl * N, N, idx, nprobs, hidx, lds, mean + p, sd + p, quant + (long long)p * nprobs, hdpi + 2 * (long long)p,
                  RS_BLOCK);
}
#endif
#endif
