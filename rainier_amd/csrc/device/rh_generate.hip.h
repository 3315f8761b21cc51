// rh_generate.hip.h -- posterior-predictive sampling over device-resident draws: the sampling half of Trace.predict
// (core/Trace.scala:34-41, core/Generator.scala:171-174: predict takes any ToGenerator, a Distribution among them).
//
// Model-independent, like rh_trace.hip.h and rh_summary.hip.h: a generator is a TABLE of ops given as data, no per-model code
// object.  Follows the prelude in its translation unit (rh_rng_*, rh_strict_log / rh_strict_exp / rh_strict_sqrt).  wave64, gfx950.
//
// in [nrows][nin]: per-draw distribution parameters, flat rows r = chain * kept + j (a predictor's [chains][kept][nreq]);
// out [nrows][nops]: output o of draw r is out[r * nops + o] -- the layout rh_trace.hip.h and rh_summary.hip.h read.
//
// One RNG stream per draw.  The reference threads one RNG through chains.flatMap(_.map(fn)), an order that is serial by construction
// (how many numbers a draw consumes depends on its parameters).  Here draw d (global index: row0_global + r, unsigned 64-bit) runs
// Generator.get on  new java.util.Random(seed_d),  seed_d = splitmix64's finaliser of  seed + (d + 1) * 0x9E3779B97F4A7C15  (rg_seed
// below; not seed + d: java.util.Random only XORs its seed and adjacent seeds give strongly correlated first numbers).  The ops of a
// draw run left to right on that one stream, as Generator.zip / traverse evaluate lf(r, n), then rf(r, n) (Generator.scala:38-47,
// 145-150); the pending nextNextGaussian is carried from one op to the next.  Nothing depends on tiling, launch shape or sharding.
//
// The families (u = standardUniform, g = standardNormal; separate * and +: contraction is off):
//   REAL       a                 a                                                         Generator.scala:119-122
//   NORMAL     loc, scale        g * scale + loc                                           Continuous.scala:54-57, 63-67, Injection.scala:50-52, 70-72
//   CAUCHY     loc, scale        (g1 / g2) * scale + loc, g1 drawn first                   Continuous.scala:72-77
//   LAPLACE    loc, scale        x * scale + loc, u' = u - 0.5, x = (signum(u') * -1) * log(1 - 2 * abs(u'))    :82-89
//   UNIFORM    loc, scale        u * scale + loc (the caller passes scale = to - from)     :202-215
//   LOGNORMAL  loc, scale        exp(g * scale + loc)                                      :194-197, Injection.scala:89-91
//   GAMMA      shape, scale      Marsaglia-Tsang with the a < 1 boost, then * scale        :94-147
//   BETA       a, b              z1 / (z1 + z2), z1 = gamma(a) * 1.0, then z2 = gamma(b) * 1.0                  :163-176
//   BERNOULLI  p                 u <= p ? 1 : 0                                            Discrete.scala:38-48
//   GEOMETRIC  p                 (double)(long)floor(log(u) / log(1 - p))                  :59-69
//   POISSON    lambda            `small` below 30, else `large` with logFactorial          :122-186
// .toLong is Java's d2l (saturating, NaN -> 0); every output is a double.
//
// java.lang.Math policy: the project's JM_DET (oracle/jmath.h).  log and exp are rh_strict_log / rh_strict_exp (fdlibm), sqrt is the
// IEEE square root, math.pow(t, 2) of Poisson.large is t * t, and Math.pow(u, 1.0 / a) of Gamma's a < 1 branch is
// rh_strict_exp((1.0 / a) * rh_strict_log(u)) -- a bit-reproducible composition in the manner of jm_pow_neg075 that differs from
// Math.pow by rounding only; no accept / reject test depends on it.  With this policy every family compares bit for bit.
//
// No loop a parameter can make endless (the reference's Poisson.large is while (true), and Marsaglia-Tsang with a bad shape need not
// end either):
//   domain guards  in straight-line code before any loop: GAMMA and BETA need every shape finite and > 0, POISSON needs lambda
//                  finite and >= 0; otherwise the output is NaN and the draw raises RG_F_DOMAIN.  A guarded op leaves the stream
//                  UNTOUCHED, so the draw's later ops are well defined: they see what they would see without that op.  The families
//                  without a parameter-dependent loop take whatever IEEE arithmetic and d2l give.
//   iteration cap  every loop of this file -- the Marsaglia-Tsang outer retry, its inner v <= 0 retry, Poisson.small's product,
//                  Poisson.large's retry -- stops after RG_MAX_ATTEMPTS passes; a capped op writes NaN and raises RG_F_CAP (the
//                  stream has then advanced by what the passes drew).  A safety condition, not a measurement: the reference's own
//                  loops needed at most 5 / 2 / 53 / 10 passes over 20 000 draws at shapes 1 .. 50 and lambda 0.5 .. 1e6.
//   rh_rng_normal's polar loop is the sampler's own and is used as it is.
//
// rh_generate_kernel: one thread per flat row, a workgroup = RG_TILE consecutive rows (flat, so many chains x few kept iterations
// still fill the tiles).  The tail lanes of the last tile compute the last valid row and store nothing, so every lane reaches every
// barrier.  A lane keeps its rh_rng in registers and walks the op table in order: the op index is wave-uniform (the family switch is
// a scalar branch, the table is read with scalar loads), only the rejection loops diverge, and no barrier, ballot or other cross-lane
// operation sits inside one.  Inputs are read by the lane where an op needs them, in[r * nin + col]: the wavefront's 64 rows are
// walked together and served from L2 (rh_predict_direct_kernel's argument).  Outputs leave through LDS in slabs of at most RG_SLAB
// ops, [row][op of the slab] with an odd row stride, then consecutive lanes store consecutive doubles; when nops fits one slab the
// tile's results are one contiguous block of out.  The LDS is sized by the launch (dynamic: RG_TILE x stride doubles, at most 62 KiB),
// so a narrow table does not pay a wide one's occupancy: the kernel is bound by what it issues (a NORMAL sample is about 5 LCG steps
// of a 64-bit multiply each, half an fdlibm log, a square root and a divide against 24 bytes moved), and more resident wavefronts
// hide the latency of those dependent chains.  The flags are raised with one atomicOr per wavefront after reconvergence.
//
// The block routine is plain C++ over (thread id, LDS pointer): with RH_GENERATE_HOST defined it compiles with a host compiler,
// every "thread" of a phase run in turn (tests/test_generate_device_cpu.py), same text.  RG_CONSTANTS_ONLY leaves the constants and
// the op table's types alone (draws_plan.hpp outside the tests).
#ifndef RH_GENERATE_HIP_H
#define RH_GENERATE_HIP_H

#define RG_TILE 256          // rows per workgroup = threads
#define RG_WAVE 64
#define RG_LDS_DOUBLES 8064  // 63 KiB, as in rh_trace.hip.h / rh_predict.hip.h
#define RG_SLAB 31           // ops per slab: RG_TILE rows x the odd stride 31 = 7936 doubles <= RG_LDS_DOUBLES
#define RG_MAX_OPS 4096
#ifndef RG_MAX_ATTEMPTS
#define RG_MAX_ATTEMPTS 4096
#endif
#define RG_F_DOMAIN 1
#define RG_F_CAP 2
// slab arithmetic: ops per slab and the LDS row stride (odd: lane d's ds_write_b64 at d * stride + k meets no bank twice)
#define RG_SLAB_W(nops) ((nops) < RG_SLAB ? (nops) : RG_SLAB)
#define RG_STRIDE(nops) (RG_SLAB_W(nops) | 1)

enum { RG_REAL = 0, RG_NORMAL, RG_CAUCHY, RG_LAPLACE, RG_UNIFORM, RG_LOGNORMAL, RG_GAMMA, RG_BETA, RG_BERNOULLI, RG_GEOMETRIC, RG_POISSON, RG_NFAMILIES };

// the op table, as include/rainier_hip.h declares it (rh_gen_arg / rh_gen_op): col >= 0: column of `in`; col == -1: `value`
typedef struct rg_arg { int col, pad; double value; } rg_arg;
typedef struct rg_op { int family, reserved; rg_arg a, b; } rg_op;

#ifndef RG_CONSTANTS_ONLY
#ifndef RH_GENERATE_HOST
#pragma clang fp contract(off)
#define RG_FN static __device__ __forceinline__
#define RG_SYNC() __syncthreads()
#define RG_TID0 ((int)threadIdx.x)
#define RG_TID1 ((int)threadIdx.x + 1)
#define RG_ST(tid) 0
#define RG_NSTATE 1
// one atomic per wavefront that raised a flag (whole wavefronts: blockDim.x = RG_TILE), after the lanes have reconverged
#define RG_RAISE(fl, flags_out)                                                                                                   \
  do {                                                                                                                              \
    const int rg_bits_ = (__ballot(((fl) & RG_F_DOMAIN) != 0) != 0ull ? RG_F_DOMAIN : 0) | (__ballot(((fl) & RG_F_CAP) != 0) != 0ull ? RG_F_CAP : 0); \
    if (rg_bits_ != 0 && (threadIdx.x & (RG_WAVE - 1)) == 0) atomicOr((flags_out), rg_bits_);                                       \
  } while (0)
#else
#define RG_FN static inline
#define RG_SYNC() ((void)0)
#define RG_TID0 0
#define RG_TID1 rg_nthreads
#define RG_ST(tid) (tid)
#define RG_NSTATE RG_TILE
#define RG_RAISE(fl, flags_out) do { *(flags_out) |= (fl); } while (0)
#endif
// every thread of the workgroup (device: this one; host: each in turn -- a phase ends where the device has its barrier)
#define RG_EACH_THREAD(tid) for (int tid = RG_TID0; tid < RG_TID1; tid++)

// the seed of draw d: splitmix64's finaliser, all arithmetic mod 2^64
RG_FN rh_i64 rg_seed(const rh_i64 seed, const rh_u64 d) {
  rh_u64 z = (rh_u64)seed + (d + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (rh_i64)(z ^ (z >> 31));
}
RG_FN bool rg_finite(const double x) { return __builtin_fabs(x) < __builtin_huge_val(); }   // false for NaN
RG_FN rh_i64 rg_d2l(const double x) {   // D2L: NaN -> 0, saturating
  if (x != x) return 0;
  if (x >= 9223372036854775807.0) return 0x7fffffffffffffffll;
  if (x <= -9223372036854775808.0) return -0x7fffffffffffffffll - 1;
  return (rh_i64)x;
}
RG_FN double rg_arg_value(const rg_arg &a, const double *row) { return a.col >= 0 ? row[a.col] : a.value; }

// Gamma.standard(a).generator (Continuous.scala:114-144), a finite and > 0: the a < 1 boost, then Marsaglia-Tsang
RG_FN double rg_gamma(rh_rng &r, const double a, int &fl) {
  double boost = 1.0, aa = a;
  if (a < 1) {
    const double u = rh_rng_uniform(r);
    boost = rh_strict_exp((1.0 / a) * rh_strict_log(u));   // Math.pow(u, 1.0 / a), see the policy above
    aa = a + 1;
  }
  const double d = aa - 1.0 / 3.0;
  const double c = (1.0 / 3.0) / rh_strict_sqrt(d);
  double res = __builtin_nan("");
  bool done = false, open = true;
  for (int pass = 0; pass < RG_MAX_ATTEMPTS && open; pass++) {
    double x = 0.0, v = 0.0;
    bool positive = false;
    for (int inner = 0; inner < RG_MAX_ATTEMPTS && !positive; inner++) {
      x = rh_rng_normal(r);
      v = 1.0 + c * x;
      positive = !(v <= 0);
    }
    if (!positive) { open = false; continue; }   // the inner retry hit the cap
    const double v3 = v * v * v;
    const double u = rh_rng_uniform(r);
    if ((u < 1 - 0.0331 * x * x * x * x) || (rh_strict_log(u) < 0.5 * x * x + d * (1 - v3 + rh_strict_log(v3)))) {
      res = d * v3;
      done = true; open = false;
    }
  }
  if (!done) { fl |= RG_F_CAP; return res; }
  return a < 1 ? res * boost : res;
}

// Poisson.generator (Discrete.scala:128-186), lambda finite and >= 0
RG_FN double rg_poisson(rh_rng &r, const double lambda, int &fl) {
  double res = __builtin_nan("");
  bool done = false;
  if (lambda < 30.0) {   // Poisson.small
    const double l = rh_strict_exp(-lambda);
    if (l >= 1.0) return 0.0;
    int k = 0;
    double p = 1.0;
    while (p > l && k < RG_MAX_ATTEMPTS) {
      k += 1;
      p *= rh_rng_uniform(r);
    }
    if (!(p > l)) { res = (double)(k - 1); done = true; }
  } else {               // Poisson.large
    const double c = 0.767 - 3.36 / lambda;
    const double beta = 3.141592653589793 / rh_strict_sqrt(3.0 * lambda);
    const double alpha = beta * lambda;
    const double k = rh_strict_log(c) - lambda - rh_strict_log(beta);
    const double loglam = rh_strict_log(lambda), half_log_2pi = 0.5 * rh_strict_log(2 * 3.141592653589793);
    for (int pass = 0; pass < RG_MAX_ATTEMPTS && !done; pass++) {
      const double u = rh_rng_uniform(r);
      const double x = (alpha - rh_strict_log((1.0 - u) / u)) / beta;
      const rh_i64 n = rg_d2l(__builtin_floor(x + 0.5));
      if (n >= 0) {
        const double v = rh_rng_uniform(r);
        const double y = alpha - beta * x;
        const double t = 1.0 + rh_strict_exp(y);
        const double lhs = y + rh_strict_log(v / (t * t));
        const double xf = (double)(rh_i64)((rh_u64)n + 1ull);   // logFactorial: (n + 1).toDouble, the long sum wrapping as the JVM's
        const double logfact = ((xf - 0.5) * rh_strict_log(xf)) - xf + half_log_2pi;
        const double rhs = k + (double)n * loglam - logfact;
        if (lhs <= rhs) { res = (double)n; done = true; }
      }
    }
  }
  if (!done) fl |= RG_F_CAP;
  return res;
}

// one op of one draw: Generator.get(rng, evaluator) of the family on the draw's stream
RG_FN double rg_sample(const rg_op &op, const double *row, rh_rng &r, int &fl) {
  const double a = rg_arg_value(op.a, row), b = rg_arg_value(op.b, row);
  const int f = op.family;
  switch (f) {
    case RG_NORMAL:
    case RG_LOGNORMAL:
    case RG_CAUCHY: {
      double g = rh_rng_normal(r);
      if (f == RG_CAUCHY) g = g / rh_rng_normal(r);   // g1 drawn first
      const double x = g * b + a;
      return f == RG_LOGNORMAL ? rh_strict_exp(x) : x;
    }
    case RG_LAPLACE:
    case RG_UNIFORM:
    case RG_BERNOULLI:
    case RG_GEOMETRIC: {
      const double u = rh_rng_uniform(r);
      if (f == RG_UNIFORM) return u * b + a;
      if (f == RG_BERNOULLI) return u <= a ? 1.0 : 0.0;
      if (f == RG_GEOMETRIC) return (double)rg_d2l(__builtin_floor(rh_strict_log(u) / rh_strict_log(1 - a)));
      const double uc = u - 0.5;
      const double sg = uc > 0 ? 1.0 : (uc < 0 ? -1.0 : uc);   // Math.signum
      const double x = sg * -1.0 * rh_strict_log(1 - (2 * __builtin_fabs(uc)));
      return x * b + a;
    }
    case RG_GAMMA:
    case RG_BETA: {
      const bool beta = f == RG_BETA;
      if (!(rg_finite(a) && a > 0) || (beta && !(rg_finite(b) && b > 0))) { fl |= RG_F_DOMAIN; return __builtin_nan(""); }
      double z1 = 0.0, z2 = 0.0;   // (one copy of the sampler's text for both of BETA's draws; no indexed array: nothing for scratch)
      for (int i = 0; i < (beta ? 2 : 1); i++) {
        const double zi = rg_gamma(r, i == 0 ? a : b, fl);
        if (i == 0) z1 = zi; else z2 = zi;
      }
      return beta ? (z1 * 1.0) / ((z1 * 1.0) + (z2 * 1.0)) : z1 * b;
    }
    case RG_POISSON:
      if (!(rg_finite(a) && a >= 0)) { fl |= RG_F_DOMAIN; return __builtin_nan(""); }
      return rg_poisson(r, a, fl);
    default:   // RG_REAL (rh_generate_create admits no other family)
      return a;
  }
}

// One tile: rows 0 .. valid - 1 (1 <= valid <= RG_TILE) of `in` (the tile's first row), draw d0 + r on row r; out: the tile's first
// row of results; lds: RG_TILE * RG_STRIDE(nops) doubles.
RG_FN void rg_block(const double *in, const int nin, const rg_op *ops, const int nops, const int valid, const rh_i64 seed, const rh_u64 d0,
                    double *lds, double *out, int *flags_out, const int rg_nthreads) {
  const int W = RG_SLAB_W(nops), stride = RG_STRIDE(nops);
  rh_rng rng[RG_NSTATE];
  int fl[RG_NSTATE];
  RG_EACH_THREAD(tid) {
    const int r = tid < valid ? tid : valid - 1;   // the tail lanes of a ragged tile take the last valid row
    rh_rng_init(rng[RG_ST(tid)], rg_seed(seed, d0 + (rh_u64)r));
    fl[RG_ST(tid)] = 0;
  }
  for (int o0 = 0; o0 < nops; o0 += W) {
    const int w = nops - o0 < W ? nops - o0 : W;
    RG_EACH_THREAD(tid) {
      const int r = tid < valid ? tid : valid - 1;
      const double *row = in + (long long)r * nin;
      for (int k = 0; k < w; k++) lds[tid * stride + k] = rg_sample(ops[o0 + k], row, rng[RG_ST(tid)], fl[RG_ST(tid)]);
    }
    RG_SYNC();
    const int total = valid * w;
    RG_EACH_THREAD(tid) {
      for (int j = tid; j < total; j += RG_TILE) {
        const int rr = j / w, k = j - rr * w;
        out[(long long)rr * nops + o0 + k] = lds[rr * stride + k];
      }
    }
    RG_SYNC();                    // the slab is no longer read
  }
  RG_EACH_THREAD(tid) { RG_RAISE(fl[RG_ST(tid)], flags_out); }
}

#if !defined(RH_GENERATE_HOST) && !defined(RH_GENERATE_EXT)   // (rh_generate_ext.hip.h's code object holds its own kernel only)
// grid: rh_plan::generate_tiles(nrows) workgroups of RG_TILE threads; dynamic LDS: RG_TILE * RG_STRIDE(nops) doubles
extern "C" __global__ void __launch_bounds__(RG_TILE)
rh_generate_kernel(const double *__restrict__ in, const int nin, const rg_op *__restrict__ ops, const int nops, const long long nrows,
                   const long long seed, const long long row0_global, double *__restrict__ out, int *__restrict__ flags_out) {
  extern __shared__ double rg_lds[];
  const long long r0 = (long long)blockIdx.x * RG_TILE;
  const int valid = nrows - r0 < RG_TILE ? (int)(nrows - r0) : RG_TILE;
  rg_block(in + r0 * nin, nin, ops, nops, valid, seed, (rh_u64)row0_global + (rh_u64)r0, rg_lds, out + r0 * nops, flags_out, RG_TILE);
}
#endif
#endif
#endif
