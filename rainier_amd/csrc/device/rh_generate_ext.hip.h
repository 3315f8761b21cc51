// rh_generate_ext.hip.h -- the count families and the composites of posterior-predictive sampling: Binomial, NegativeBinomial,
// Categorical, and -- as TABLES of ops, not families -- BetaBinomial, mixtures and zero inflation (core/Discrete.scala:81-109,
// 194-273, core/Multinomial.scala:26-29, core/Generator.scala:129-141, core/Continuous.scala's Mixture).
//
// Follows rh_generate.hip.h in its translation unit and reuses its text: rg_seed, rg_d2l, rg_gamma, rg_poisson, rg_sample, the tile /
// slab macros, the flags, one java.util.Random stream per draw with the ops of a draw run left to right on it.  A code object of its
// own (rh_generate_ext_kernel); rh_generate_create sends a table here only when it uses what is below, so every other table runs
// rh_generate_kernel as before.
//
// What a table may say beyond rh_generate.hip.h's (include/rainier_hip.h: rh_gen_op.reserved is a flags word, rh_gen_arg.pad a source):
//   guard    reserved bits 0-7: 0 = the op always runs; j + 1 = it runs only in the draws whose SELECTOR is j.  The selector is the
//            sample of the nearest earlier CATEGORICAL op that ran in this draw (none yet, or a NaN sample: no guard matches).  A
//            skipped op draws nothing, raises nothing, and its value is the carry.
//   hidden   reserved bit 8: the op's value is not stored; output column c is the c-th visible op, the row stride is nout.
//   PREV     arg.pad == 1: the argument is the draw's CARRY, the value of op o - 1 (a skipped op's value is the carry before it).
//
// The families, numbered from 16 (u = standardUniform, g = standardNormal; every argument the reference builds out of Reals is the
// plain left-to-right double expression: it differs from the reference's evaluation by rounding only, but unlike Gamma's pow it feeds
// a .toLong):
//   BINOMIAL (p, k)      Discrete.scala:194-230
//       k >= 100 && k * p <= 10                          min(Poisson(p * k), (long)k)                      :205-208, 223-224
//       else k >= 100 && k * p >= 9 && k * (1 - p) >= 9  min(max((long)(g * sqrt(k * p * (1 - p)) + k * p), 0), (long)k)     :209-214, 225-226
//       else                                             (int)k trials (Java's d2i), each one u, counting p + 0.0 >= u       :215-217,
//                                                        Multinomial.scala:26-29, Generator.scala:49-57, 129-141 (cdf(true) = p + 0)
//   NEGBINOMIAL (p, n)   Discrete.scala:81-109
//       p < -100 / n + 1 && p > 100 / n - .25            max((long)(g * (sqrt(n * p) / (1 - p)) + n * p / (1 - p)), 0)        :95-97, 103-104
//       else                                             the sum of (long)n draws of (long)floor(log(u) / log(1 - (1 - p))),
//                                                        a 64-bit sum that wraps as the JVM's                                :88-94, 59-69
//   CATEGORICAL (a = the first of m consecutive weight columns, b = the immediate m)                      Generator.scala:129-141
//       one u; cdf_i = w_i + cdf_(i-1), cdf_(-1) = 0.0; the first i (from 0) with cdf_i >= u, else m - 1
// pow(x, 0.5) is the IEEE square root (JM_DET, as rh_generate.hip.h's policy says).
//
// No parameter can make a loop endless, and nothing is drawn where a guard refuses -- in straight-line code before any loop:
//   domain   BINOMIAL / NEGBINOMIAL need p finite in [0, 1] and k / n finite and >= 0, CATEGORICAL every weight finite and >= 0;
//            otherwise NaN, RG_F_DOMAIN, the stream untouched.  A NaN selector matches no guard: the NaN is carried to the mixture's column.
//   cap      an exact path of more than RG_MAX_ATTEMPTS trials gives NaN and RG_F_CAP and draws nothing; the Poisson and normal draws
//            inside keep their own caps.
//
// rh_generate_ext_kernel keeps rh_generate_kernel's shape: one lane per flat row, RG_TILE per workgroup, the op index wave-uniform;
// a lane's state is its rh_rng, the carry, the selector and the flags, in registers (no indexed per-lane array: nothing for scratch).
// A guard is a per-lane predicate around straight calls; every family funnels into ONE call of rg_sample (BINOMIAL's Poisson branch as
// a POISSON op, the normal branches as a NORMAL op, CATEGORICAL's u as UNIFORM(0, 1): u * 1.0 + 0.0 is u), so the samplers' text is
// there once; the exact paths are one loop behind it.  Slabs are cut by VISIBLE outputs: the ops of a slab are those up to and with
// its RG_SLAB_W(nout)-th visible one and the hidden ops that follow it (a slab starts at a visible op or at op 0), counted from the
// table with scalar loads, so every lane reaches every RG_SYNC; carry and selector live across slabs.  The transpose through LDS and the store are
// rh_generate.hip.h's, with the row stride nout.
#ifndef RH_GENERATE_EXT_HIP_H
#define RH_GENERATE_EXT_HIP_H

enum { RGX_BINOMIAL = 16, RGX_NEGBINOMIAL = 17, RGX_CATEGORICAL = 18, RGX_END_FAMILIES = 19 };
#define RGX_GUARD(reserved) ((reserved) & 0xff)
#define RGX_HIDDEN 0x100
#define RGX_FLAG_BITS 0x1ff
#define RGX_PREV 1            // rg_arg.pad
#define RGX_MAX_WEIGHTS 255

#ifndef RG_CONSTANTS_ONLY
// what follows the one rg_sample call of an op
#define RGX_P_LONG 1          // (long)x max 0
#define RGX_P_MIN 2           // min (long)k
#define RGX_P_BIN 4           // the exact binomial trials
#define RGX_P_NB 8            // the exact negative binomial sum
#define RGX_P_CAT 16          // the walk along the cdf

RG_FN double rgx_arg(const rg_arg &a, const double *row, const double carry) { return a.pad == RGX_PREV ? carry : rg_arg_value(a, row); }

// one op of one draw -> its value (the carry where the guard refuses); sel: the draw's selector, -1 = none
RG_FN double rgx_op(const rg_op &op, const double *row, rh_rng &r, int &fl, const double carry, int &sel) {
  const int f = op.family, guard = RGX_GUARD(op.reserved);
  if (guard != 0 && sel != guard - 1) return carry;
  const double a = rgx_arg(op.a, row, carry), b = rgx_arg(op.b, row, carry);
  rg_op t;   // what rg_sample is asked for, its arguments as immediates
  t.family = f; t.reserved = 0;
  t.a.col = -1; t.a.pad = 0; t.a.value = a;
  t.b.col = -1; t.b.pad = 0; t.b.value = b;
  int post = 0, trials = 0;
  rh_i64 kl = 0;
  double pp = 0.0, lq = 0.0;
  if (f == RGX_BINOMIAL || f == RGX_NEGBINOMIAL) {
    t.family = RG_REAL; t.a.value = __builtin_nan(""); t.b.value = 0.0;
    if (!(rg_finite(a) && a >= 0 && a <= 1 && rg_finite(b) && b >= 0)) {
      fl |= RG_F_DOMAIN;
    } else if (f == RGX_BINOMIAL) {
      kl = rg_d2l(b);
      if (b >= 100 && b * a <= 10) {
        t.family = RG_POISSON; t.a.value = a * b; post = RGX_P_MIN;
      } else if (b >= 100 && b * a >= 9 && b * (1.0 - a) >= 9) {
        t.family = RG_NORMAL; t.a.value = b * a; t.b.value = rh_strict_sqrt(b * a * (1 - a)); post = RGX_P_LONG | RGX_P_MIN;
      } else {
        const int n = b >= 2147483647.0 ? 0x7fffffff : (int)b;   // D2I
        if (n > RG_MAX_ATTEMPTS) fl |= RG_F_CAP;
        else { trials = n; pp = a + 0.0; post = RGX_P_BIN; }
      }
    } else {
      if (a < -100 / b + 1 && a > 100 / b - .25) {
        t.family = RG_NORMAL; t.a.value = b * a / (1 - a); t.b.value = rh_strict_sqrt(b * a) / (1 - a); post = RGX_P_LONG;
      } else {
        const rh_i64 n = rg_d2l(b);
        if (n > RG_MAX_ATTEMPTS) fl |= RG_F_CAP;
        else { trials = (int)n; lq = rh_strict_log(1 - (1 - a)); post = RGX_P_NB; }
      }
    }
  }
  const int m = f == RGX_CATEGORICAL ? (int)op.b.value : 0;   // wave-uniform: an immediate of the table
  if (f == RGX_CATEGORICAL) {
    bool ok = true;
    for (int i = 0; i < m; i++) { const double w = row[op.a.col + i]; ok = ok && rg_finite(w) && w >= 0; }
    sel = -1;
    if (ok) { t.family = RG_UNIFORM; t.a.value = 0.0; t.b.value = 1.0; post = RGX_P_CAT; }
    else { fl |= RG_F_DOMAIN; t.family = RG_REAL; t.a.value = __builtin_nan(""); t.b.value = 0.0; }
  }
  double v = rg_sample(t, row, r, fl);
  if (post & RGX_P_LONG) {
    const rh_i64 x = rg_d2l(v);
    v = (double)(x < 0 ? 0 : x);
  }
  if ((post & RGX_P_MIN) && v == v) {   // (a capped Poisson stays NaN)
    const rh_i64 x = rg_d2l(v);
    v = (double)(x < kl ? x : kl);
  }
  if (post & (RGX_P_BIN | RGX_P_NB)) {
    rh_u64 acc = 0;
    for (int i = 0; i < trials; i++) {
      const double u = rh_rng_uniform(r);
      if (post & RGX_P_BIN) acc += pp >= u ? 1ull : 0ull;
      else acc += (rh_u64)rg_d2l(__builtin_floor(rh_strict_log(u) / lq));
    }
    v = (double)(rh_i64)acc;
  }
  if (post & RGX_P_CAT) {
    double cdf = 0.0;
    int idx = m - 1;
    bool found = false;
    for (int i = 0; i < m; i++) {
      cdf = row[op.a.col + i] + cdf;
      if (!found && cdf >= v) { idx = i; found = true; }
    }
    sel = idx;
    v = (double)idx;
  }
  return v;
}

// One tile, as rg_block: rows 0 .. valid - 1 of `in`, draw d0 + r on row r; out: the tile's first row of results, row stride nout (the
// table's visible ops, >= 1); lds: RG_TILE * RG_STRIDE(nout) doubles.
RG_FN void rgx_block(const double *in, const int nin, const rg_op *ops, const int nops, const int nout, const int valid, const rh_i64 seed,
                     const rh_u64 d0, double *lds, double *out, int *flags_out, const int rg_nthreads) {
  const int W = RG_SLAB_W(nout), stride = RG_STRIDE(nout);
  rh_rng rng[RG_NSTATE];
  int fl[RG_NSTATE], sel[RG_NSTATE];
  double carry[RG_NSTATE];
  RG_EACH_THREAD(tid) {
    const int r = tid < valid ? tid : valid - 1;   // the tail lanes of a ragged tile take the last valid row
    rh_rng_init(rng[RG_ST(tid)], rg_seed(seed, d0 + (rh_u64)r));
    fl[RG_ST(tid)] = 0; sel[RG_ST(tid)] = -1; carry[RG_ST(tid)] = 0.0;
  }
  int c0 = 0;   // the slab's first output column
  for (int o0 = 0; o0 < nops;) {
    int o1 = o0, w = 0;   // the slab's ops [o0, o1) and its visible ones, from the table
    while (o1 < nops && (w < W || (ops[o1].reserved & RGX_HIDDEN))) { w += (ops[o1].reserved & RGX_HIDDEN) ? 0 : 1; o1++; }
    RG_EACH_THREAD(tid) {
      const int r = tid < valid ? tid : valid - 1;
      const double *row = in + (long long)r * nin;
      double cr = carry[RG_ST(tid)];
      int sl = sel[RG_ST(tid)], k = 0;
      for (int o = o0; o < o1; o++) {
        cr = rgx_op(ops[o], row, rng[RG_ST(tid)], fl[RG_ST(tid)], cr, sl);
        if (!(ops[o].reserved & RGX_HIDDEN)) { lds[tid * stride + k] = cr; k++; }
      }
      carry[RG_ST(tid)] = cr; sel[RG_ST(tid)] = sl;
    }
    RG_SYNC();
    const int total = valid * w;
    RG_EACH_THREAD(tid) {
      for (int j = tid; j < total; j += RG_TILE) {
        const int rr = j / w, k = j - rr * w;
        out[(long long)rr * nout + c0 + k] = lds[rr * stride + k];
      }
    }
    RG_SYNC();                    // the slab is no longer read
    c0 += w; o0 = o1;
  }
  RG_EACH_THREAD(tid) { RG_RAISE(fl[RG_ST(tid)], flags_out); }
}

#ifndef RH_GENERATE_HOST
// grid: rh_plan::generate_tiles(nrows) workgroups of RG_TILE threads; dynamic LDS: RG_TILE * RG_STRIDE(nout) doubles
extern "C" __global__ void __launch_bounds__(RG_TILE)
rh_generate_ext_kernel(const double *__restrict__ in, const int nin, const rg_op *__restrict__ ops, const int nops, const int nout,
                       const long long nrows, const long long seed, const long long row0_global, double *__restrict__ out,
                       int *__restrict__ flags_out) {
  extern __shared__ double rg_lds[];
  const long long r0 = (long long)blockIdx.x * RG_TILE;
  const int valid = nrows - r0 < RG_TILE ? (int)(nrows - r0) : RG_TILE;
  rgx_block(in + r0 * nin, nin, ops, nops, nout, valid, seed, (rh_u64)row0_global + (rh_u64)r0, rg_lds, out + r0 * nout, flags_out, RG_TILE);
}
#endif
#endif
#endif
