// rh_loo_quantile.hip.h -- leave-one-out predictive quantiles and the continuous ranked probability score over device-resident draws: the
// quantiles of the PSIS-weighted predictive distribution of an observation (the `loo` package's E_loo(type = "quantile"), the input of
// ppc_loo_intervals), its CRPS against y and its spread E|X - X'|.  All of them are functionals of the weighted empirical distribution
// function of a value column: a sort that carries a payload, and a scan behind it.
//
// Model-independent: a translation unit of its own, behind rh_summary.hip.h (the key order, the tile sort's slots and pair order,
// rs_tree_sum), rh_loo.hip.h (exp and log, the tail's three routines) and rh_loo_expect.hip.h (lx_fit_block, called as it is, so that
// pareto_k, tail_n and the tail's group-mean weights are that family's bit for bit).  wave64, gfx950.
//
// A pair k of the selection: the log-likelihood column ll_cols [k] of ll [chains][iterations][nll] and the value column val_cols [k] of
// val [chains][iterations][nval], over rh_summary.hip.h's window; draw s = c * kept + j, S = chains * kept >= 2.  Plain mode: no
// log-likelihood buffer, every weight is 1, and the first four kernels are not launched.
//
//   rh_loo_quantile_sort_kernel /    the log-likelihood side, as rh_loo_expect's: the summary's tile sort and merge pass over the pairs'
//   rh_loo_quantile_merge_kernel /   log-likelihood columns, then lx_fit_block: pareto_k, tail_n, tailw [M].
//   rh_loo_quantile_fit_kernel
//   rh_loo_quantile_weight_kernel    one workgroup per pair x tile of RS_TILE draws: W_s of every draw, rh_loo_expect's expressions restated
//                                    (a tail draw takes one lower-bound search in a [0 .. n) and reads tailw; every other draw has
//                                    exp(a [0] - l_s)), into a contiguous w [S] in draw order.
//   rh_loo_quantile_kvsort_kernel    one workgroup = one pair x one tile of LQ_TILE draws: the pairs (rs_to_key(v_s), bits of W_s) gathered
//                                    from the strided value column and w, sorted in LDS by rs_tile_sort's network over two parallel
//                                    arrays of slots (keys, payloads; the same pads, so the bank pattern of each array is the summary's),
//                                    ascending lexicographically: the key, then the payload's bits (W >= 0: the bits' order is the
//                                    numeric one).  No two distinct pairs compare equal, so the sorted sequence is a function of the
//                                    multiset alone: any correct network gives these bits, whatever the draws' order.  A ragged tile is
//                                    filled up with (all-ones, all-ones), above every pair.
//   rh_loo_quantile_kvmerge_kernel   rs_merge_tile over pairs: one merge-path pass between two workspace buffers of two parallel arrays.
//   rh_loo_quantile_scan_kernel      one workgroup per pair over its sorted pairs x_(1..S), W_(1..S).  Thread t owns the contiguous
//                                    segment [t L, (t + 1) L), L = ceil(S / LL_BLOCK).  Pass 1: r = the segment's weights added in ascending
//                                    order; thread 0 adds the LL_BLOCK segment sums in thread order: off [t], the exclusive offset, and
//                                    C_S = off [LL_BLOCK].  Pass 2: C_j = off [t] + r_j with r_j the thread's running sum -- non-decreasing
//                                    in j as computed (r_j is, an addition is monotone, and off [t + 1] == off [t] + the segment's last r)
//                                    -- written to cum [S].  Pass 3, backwards: R_j = offr [t] + the thread's running sum of the weights
//                                    behind j (offr: the later threads' segment sums, added in descending thread order), the weight
//                                    above x_(j); with F_j = C_j / C_S and 1 - F_j taken as R_j / C_S (the subtraction cancels where a
//                                    few draws carry the weight: every factor is a quotient of sums of non-negative terms instead) the two
//                                    scores' terms of the gap [x_(j), x_(j+1)), added in descending j, then rs_tree_sum over the threads.
//                                    Then thread i < nprobs: t = p_i C_S, the smallest j with C_j >= t by a binary search along cum, and
//                                    the interpolation between the knots j - 1 and j.
//
// Tile: LQ_TILE = RS_TILE = 4096 pairs, 68 KiB of LDS with the pads: two workgroups per CU's 160 KiB, against four at 2048 pairs.  The
// larger one was taken because it keeps the summary's plan (tiles, merge passes, the network's pair order with its checked bank pattern)
// as it is and saves a merge pass over 16 bytes per draw; the two have not been measured against each other.
//
// A NaN or an infinity in the log-likelihood window gives NaN in every double of the pair and tail_n = 0; one in the value window (read
// off the two ends of the sorted values) gives NaN in the pair's quantiles, crps and spread and leaves pareto_k and tail_n alone; a NaN y
// gives NaN in crps only.  Every NaN that leaves is the positive quiet one, made on the bits.  No floating-point atomics; every sum has
// an order fixed by S alone over a sequence fixed by the multiset: a second call, a window and its copy, any chunking, any order of the
// pair list and any order of the draws give the same bits.
// Workspace per pair, LQ_PAIR_BYTES: two buffers of two parallel arrays of S words, 32 S bytes, and 8 M for the tail's weights.  The
// log-likelihood side sorts between the two arrays of the second buffer and leaves w in the spare one; the first merge pass over pairs
// overwrites them, after the tile sort has read w.  cum lies in the key array of the buffer the last merge pass read.
//
// The block routines are plain C++ over (thread id, LDS pointer): with RH_LOO_QUANTILE_HOST (and RH_LOO_EXPECT_HOST, RH_LOO_HOST,
// RH_SUMMARY_HOST) defined they compile with a host compiler, every "thread" of a phase run in turn
// (tests/test_loo_quantile_device_cpu.py): same text, same summation order.
#ifndef RH_LOO_QUANTILE_HIP_H
#define RH_LOO_QUANTILE_HIP_H
#ifndef RH_LOO_EXPECT_HIP_H
#error "rh_loo_quantile.hip.h follows rh_summary.hip.h, rh_loo.hip.h and rh_loo_expect.hip.h in its translation unit"
#endif
#if defined(RH_LOO_QUANTILE_HOST) != defined(RH_LOO_HOST)
#error "rh_loo_quantile.hip.h is compiled the way rh_loo.hip.h is: both for the host or both for the device"
#endif

#define LQ_TILE RS_TILE                                           // pairs of a tile sort (the plan is the summary's)
#define LQ_SORT_LDS (2 * RS_TILE_SLOTS)                           // keys, then payloads: 68 KiB
#define LQ_MERGE_HALF (RS_MERGE_TILE + RS_MERGE_OUT_SLOTS)        // one array's staged inputs and outputs
#define LQ_MERGE_LDS (2 * LQ_MERGE_HALF + 2)                      // keys, payloads, the two splits: 68 KiB
#define LQ_SCAN_LDS_DOUBLES (5 * LL_BLOCK + 2)                    // the segment sums, the offsets and C_S, the offsets from behind, two rows of partial sums
#define LQ_WS_CAP_BYTES LL_WS_CAP_BYTES
#define LQ_PAIR_BYTES(S, M) (32 * (S) + 8 * (M))
#define LQ_ONE_BITS 0x3ff0000000000000ull                         // the bits of the weight 1.0

// (ka, wa) <= (kb, wb), lexicographically
LL_FN bool lq_le(const rs_key ka, const rs_key wa, const rs_key kb, const rs_key wb) { return ka < kb || (ka == kb && wa <= wb); }
LL_FN double lq_weight_of(const rs_key bits) { double w; __builtin_memcpy(&w, &bits, 8); return w; }
// every NaN made the positive quiet one, on the bits (a floating-point select "x != x ? nan : x" may be folded to x)
LL_FN double lq_canon(const double x) { return rs_from_key(rs_to_key(x)); }

#define LQ_CE(ka, wa, kb, wb, up)                                               \
  {                                                                             \
    const rs_key xk_ = (ka), yk_ = (kb), xw_ = (wa), yw_ = (wb);                \
    const bool gt_ = xk_ > yk_ || (xk_ == yk_ && xw_ > yw_);                    \
    const bool sw_ = gt_ == (up);                                               \
    (ka) = sw_ ? yk_ : xk_;                                                     \
    (wa) = sw_ ? yw_ : xw_;                                                     \
    (kb) = sw_ ? xk_ : yk_;                                                     \
    (wb) = sw_ ? xw_ : yw_;                                                     \
  }

// rs_local_steps over pairs
LL_FN void lq_local_steps(rs_key *r, rs_key *p, const int base, const int k, const int jmax) {
#pragma unroll
  for (int j = 8; j >= 1; j >>= 1) {
    if (j <= jmax) {
#pragma unroll
      for (int i = 0; i < 16; i++) {
        if ((i & j) == 0) {
          const bool up = ((base + i) & k) == 0;
          LQ_CE(r[i], p[i], r[i + j], p[i + j], up);
        }
      }
    }
  }
}

// ---- the weights of one pair's draws [g0, g0 + RS_TILE) ------------------------------------------------------------------------------
// s, tailw, pk, n: the sorted log-likelihood column and what lx_fit_block left for it.  lcol: the draws at [chain 0][iteration `first`]
// [the pair's column]; draw g is at ((g / kept) * iterations + (g % kept) * thin) rows of nll columns.  w [S]: written at the tile's
// draws.  The expressions are lx_reduce_block's.
LL_FN void lq_weight_block(const rs_key *s, const long long S, const double *tailw, const double pk, const int n, const double *lcol, const long long nll,
                           const long long iterations, const long long thin, const long long kept, const long long g0, double *w, const int ll_nthreads) {
  const bool bad = s[0] <= LL_KEY_NEG_INF || s[S - 1] >= LL_KEY_POS_INF;   // a NaN or an infinity in the column: the scan writes NaN, w is not used
  const bool smooth = !bad && n > 4 && ll_finite(pk);
  const double a0 = rs_from_key(s[0]);
  const rs_key top = smooth ? s[n - 1] : 0;                         // the tail's last key
  LL_EACH_THREAD(tid) {
    for (int q = 0; q < RS_TILE / LL_BLOCK; q++) {
      const long long g = g0 + tid + q * LL_BLOCK;
      if (g >= S) break;
      const long long c = g / kept, j = g - c * kept, row = c * iterations + j * thin;
      const double l = lcol[row * nll];
      double W;
      const rs_key key = rs_to_key(l);
      if (bad) {
        W = 1.0;
      } else if (smooth && key <= top) {                            // in the tail: the first position of its key
        int lo = 0, hi = n - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s[mid] < key) lo = mid + 1; else hi = mid;
        }
        W = tailw[lo];
      } else {
        W = ll_exp(a0 - l);
      }
      w[g] = W;
    }
  }
}

// ---- tile sort over pairs -------------------------------------------------------------------------------------------------------------
// One pair x one tile, as rs_tile_sort.  vcol: the draws at [chain 0][iteration `first`][the pair's value column] of nval columns;
// w [S]: the draws' weights, or NULL (every weight 1).  The tile holds the draws g0 .. min(g0 + LQ_TILE, S) - 1 and is written, sorted, to
// run_k / run_w [0 .. that many).  lds: LQ_SORT_LDS words.
LL_FN void lq_tile_sort(const double *vcol, const long long iterations, const long long nval, const long long thin, const long long kept, const long long S,
                        const long long g0, const double *w, rs_key *lds, rs_key *run_k, rs_key *run_w, const int ll_nthreads) {
  rs_key *lk = lds, *lw = lds + RS_TILE_SLOTS;
  const int nv = (int)(S - g0 < LQ_TILE ? S - g0 : LQ_TILE);
  LL_EACH_THREAD(tid) {
#pragma unroll 4
    for (int q = 0; q < LQ_TILE / LL_BLOCK; q++) {
      const int e = tid + q * LL_BLOCK;
      rs_key key = RS_KEY_FILL, pay = RS_KEY_FILL;
      if (e < nv) {
        const long long g = g0 + e, c = g / kept, j = g - c * kept;
        key = rs_to_key(vcol[(c * iterations + j * thin) * nval]);
        pay = LQ_ONE_BITS;
        if (w) __builtin_memcpy(&pay, w + g, 8);
      }
      lk[RS_SLOT(e)] = key;
      lw[RS_SLOT(e)] = pay;
    }
  }
  LL_SYNC();
  // stages 2 .. 16 never leave a thread's 16 elements
  LL_EACH_THREAD(tid) {
    rs_key r[16], p[16];
#pragma unroll
    for (int i = 0; i < 16; i++) { r[i] = lk[17 * tid + i]; p[i] = lw[17 * tid + i]; }
    lq_local_steps(r, p, 16 * tid, 2, 1);
    lq_local_steps(r, p, 16 * tid, 4, 2);
    lq_local_steps(r, p, 16 * tid, 8, 4);
    lq_local_steps(r, p, 16 * tid, 16, 8);
#pragma unroll
    for (int i = 0; i < 16; i++) { lk[17 * tid + i] = r[i]; lw[17 * tid + i] = p[i]; }
  }
  LL_SYNC();
  for (int k = 32; k <= LQ_TILE; k <<= 1) {
    for (int j = k >> 1; j >= 16; j >>= 1) {
      LL_EACH_THREAD(tid) {
#pragma unroll 4
        for (int q = 0; q < LQ_TILE / 2 / LL_BLOCK; q++) {
          const int lo = rs_pair_lo(tid + q * LL_BLOCK, j), hi = lo + j;
          const bool up = (lo & k) == 0;
          rs_key a = lk[RS_SLOT(lo)], b = lk[RS_SLOT(hi)], pa = lw[RS_SLOT(lo)], pb = lw[RS_SLOT(hi)];
          LQ_CE(a, pa, b, pb, up);
          lk[RS_SLOT(lo)] = a;
          lk[RS_SLOT(hi)] = b;
          lw[RS_SLOT(lo)] = pa;
          lw[RS_SLOT(hi)] = pb;
        }
      }
      LL_SYNC();
    }
    LL_EACH_THREAD(tid) {
      rs_key r[16], p[16];
#pragma unroll
      for (int i = 0; i < 16; i++) { r[i] = lk[17 * tid + i]; p[i] = lw[17 * tid + i]; }
      lq_local_steps(r, p, 16 * tid, k, 8);
#pragma unroll
      for (int i = 0; i < 16; i++) { lk[17 * tid + i] = r[i]; lw[17 * tid + i] = p[i]; }
    }
    LL_SYNC();
  }
  LL_EACH_THREAD(tid) {
#pragma unroll 4
    for (int q = 0; q < LQ_TILE / LL_BLOCK; q++) {
      const int e = tid + q * LL_BLOCK;
      if (e < nv) { run_k[e] = lk[RS_SLOT(e)]; run_w[e] = lw[RS_SLOT(e)]; }
    }
  }
}

// ---- merge pass over pairs ------------------------------------------------------------------------------------------------------------
// rs_merge_split over pairs: how many of the first d outputs of merge(A [0, na), B [0, nb)) come from A (on a tie -- identical pairs -- A
// goes first)
LL_FN long long lq_merge_split(const rs_key *Ak, const rs_key *Aw, const long long na, const rs_key *Bk, const rs_key *Bw, const long long nb, const long long d) {
  long long lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (lq_le(Ak[mid], Aw[mid], Bk[d - 1 - mid], Bw[d - 1 - mid])) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// rs_merge_tile over pairs: one pair's S sorted pairs in runs of L, outputs [o0, min(o0 + RS_MERGE_TILE, S)).  lds: LQ_MERGE_LDS words.
LL_FN void lq_merge_tile(const rs_key *src_k, const rs_key *src_w, rs_key *dst_k, rs_key *dst_w, const long long S, const long long L, const long long o0,
                         rs_key *lds, const int ll_nthreads) {
  rs_key *in_k = lds, *out_k = in_k + RS_MERGE_TILE, *in_w = lds + LQ_MERGE_HALF, *out_w = in_w + RS_MERGE_TILE, *lds_sp = lds + 2 * LQ_MERGE_HALF;
  const long long ps = o0 / (2 * L) * (2 * L);                 // the pair of runs' first element
  const long long na = S - ps < L ? S - ps : L, nb = S - ps - na < L ? S - ps - na : L;
  const rs_key *Ak = src_k + ps, *Aw = src_w + ps, *Bk = Ak + na, *Bw = Aw + na;
  const long long d0 = o0 - ps, d1 = d0 + RS_MERGE_TILE < na + nb ? d0 + RS_MERGE_TILE : na + nb;
  LL_EACH_THREAD(tid) {
    if (tid < 2) lds_sp[tid] = (rs_key)lq_merge_split(Ak, Aw, na, Bk, Bw, nb, tid ? d1 : d0);
  }
  LL_SYNC();
  const long long a0 = (long long)lds_sp[0], a1 = (long long)lds_sp[1], b0 = d0 - a0;
  const int sna = (int)(a1 - a0), n_out = (int)(d1 - d0), snb = n_out - sna;
  LL_EACH_THREAD(tid) {
#pragma unroll 4
    for (int q = 0; q < RS_MERGE_E; q++) {
      const int i = tid + q * LL_BLOCK;
      if (i < n_out) {
        in_k[i] = i < sna ? Ak[a0 + i] : Bk[b0 + (i - sna)];
        in_w[i] = i < sna ? Aw[a0 + i] : Bw[b0 + (i - sna)];
      }
    }
  }
  LL_SYNC();
  LL_EACH_THREAD(tid) {
    const int d = tid * RS_MERGE_E < n_out ? tid * RS_MERGE_E : n_out;
    int ai = (int)lq_merge_split(in_k, in_w, sna, in_k + sna, in_w + sna, snb, d), bi = d - ai;
    for (int k = 0; k < RS_MERGE_E; k++) {
      if (d + k < n_out) {
        const bool take_a = bi >= snb || (ai < sna && lq_le(in_k[ai], in_w[ai], in_k[sna + bi], in_w[sna + bi]));
        out_k[RS_OSLOT(d + k)] = take_a ? in_k[ai] : in_k[sna + bi];
        out_w[RS_OSLOT(d + k)] = take_a ? in_w[ai] : in_w[sna + bi];
        ai += take_a ? 1 : 0;
        bi += take_a ? 0 : 1;
      }
    }
  }
  LL_SYNC();
  LL_EACH_THREAD(tid) {
#pragma unroll 4
    for (int q = 0; q < RS_MERGE_E; q++) {
      const int i = tid + q * LL_BLOCK;
      if (i < n_out) { dst_k[o0 + i] = out_k[RS_OSLOT(i)]; dst_w[o0 + i] = out_w[RS_OSLOT(i)]; }
    }
  }
}

// ---- the scan of one pair -------------------------------------------------------------------------------------------------------------
// xs, ws: the pair's S sorted pairs.  ll_bad: its log-likelihood column holds a NaN or an infinity.  y: read where has_y.  probs [nprobs]
// in [0, 1].  cum [S]: the cumulative weights, written and read here.  lds: LQ_SCAN_LDS_DOUBLES doubles.  quant [nprobs]; crps (asked for
// with y only), spread: written where not NULL.
LL_FN void lq_scan_block(const rs_key *xs, const rs_key *ws, const long long S, const bool ll_bad, const bool has_y, const double y, const double *probs,
                         const int nprobs, double *cum, double *lds, double *quant, double *crps, double *spread, const int ll_nthreads) {
  const int rs_nthreads = ll_nthreads;
  (void)rs_nthreads;
  double *part = lds, *off = part + LL_BLOCK, *offr = off + LL_BLOCK + 2, *r0 = offr + LL_BLOCK, *r1 = r0 + LL_BLOCK;
  const double nan = rs_from_key(RS_KEY_NAN);
  if (ll_bad || xs[0] <= LL_KEY_NEG_INF || xs[S - 1] >= LL_KEY_POS_INF) {     // a NaN or an infinity in either window
    LL_EACH_THREAD(tid) {
      if (tid < nprobs) quant[tid] = nan;
      if (tid == 0) {
        if (crps) *crps = nan;
        if (spread) *spread = nan;
      }
    }
    return;
  }
  const long long L = (S + LL_BLOCK - 1) / LL_BLOCK;
  LL_EACH_THREAD(tid) {
    const long long lo = tid * L < S ? tid * L : S, hi = lo + L < S ? lo + L : S;
    double r = 0.0;
    for (long long j = lo; j < hi; j++) r += lq_weight_of(ws[j]);
    part[tid] = r;
  }
  LL_SYNC();
  LL_EACH_THREAD(tid) {
    if (tid == 0) {                                                 // the exclusive offsets, in thread order
      double c = 0.0;
      for (int t = 0; t < LL_BLOCK; t++) { off[t] = c; c += part[t]; }
      off[LL_BLOCK] = c;
      c = 0.0;
      for (int t = LL_BLOCK - 1; t >= 0; t--) { offr[t] = c; c += part[t]; }   // and from behind
    }
  }
  LL_SYNC();
  const double total = off[LL_BLOCK];                               // C_S: > 0, the draw of a [0] has weight 1 or the tail's largest
  const double x1 = rs_from_key(xs[0]), xS = rs_from_key(xs[S - 1]);
  LL_EACH_THREAD(tid) {
    const long long lo = tid * L < S ? tid * L : S, hi = lo + L < S ? lo + L : S;
    const double base = off[tid];
    double r = 0.0, ac = 0.0, as = 0.0;
    for (long long j = lo; j < hi; j++) {
      r += lq_weight_of(ws[j]);
      cum[j] = base + r;
    }
    const double baser = offr[tid];
    r = 0.0;                                                        // the segment's weights behind j
    for (long long j = hi - 1; j >= lo; j--) {
      if (j + 1 < S) {                                              // the gap [x_(j), x_(j+1)) in the contract's 1-based j
        const double a = rs_from_key(xs[j]), b = rs_from_key(xs[j + 1]), F = cum[j] / total, G = (baser + r) / total;
        as += (b - a) * F * G;
        if (has_y) {
          double m = y > a ? y : a;
          m = m < b ? m : b;
          ac += (m - a) * (F * F) + (b - m) * (G * G);
        }
      }
      r += lq_weight_of(ws[j]);
    }
    r0[tid] = ac;
    r1[tid] = as;
  }
  rs_tree_sum(r0, rs_nthreads);
  rs_tree_sum(r1, rs_nthreads);
  // The searches read cum [] as other threads of the workgroup wrote it, through global memory: this barrier (on the device
  // __syncthreads, a workgroup-scope release and acquire that covers global stores) is what makes them visible.  It is the searches'
  // own: the tree sums above may be reordered or dropped without touching it.
  LL_SYNC();
  LL_EACH_THREAD(tid) {
    if (tid < nprobs) {
      const double t = probs[tid] * total;
      long long lo = 0, hi = S - 1;                                 // cum [S - 1] == total >= t
      while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (cum[mid] < t) lo = mid + 1; else hi = mid;
      }
      const double xj = rs_from_key(xs[lo]), cj = cum[lo];
      double q = xj;                                                // j = 1, or t == C_j: the knot itself
      if (lo > 0 && cj != t) {
        const double xp = rs_from_key(xs[lo - 1]), cp = cum[lo - 1];
        q = xp + (xj - xp) * ((t - cp) / (cj - cp));
      }
      quant[tid] = lq_canon(q);
    }
    if (tid == 0) {
      if (crps) {
        const double e_lo = x1 - y > 0.0 ? x1 - y : 0.0, e_hi = y - xS > 0.0 ? y - xS : 0.0;
        *crps = rs_to_key(y) == RS_KEY_NAN ? nan : lq_canon(r0[0] + e_lo + e_hi);
      }
      if (spread) *spread = lq_canon(2.0 * r1[0]);
    }
  }
}

#ifndef RH_LOO_QUANTILE_HOST
// The workspace holds, for the chunk's pairs [k_lo, k_lo + p_cnt) of the selection, two buffers of two arrays [p_cnt][S] of words and
// tailw [p_cnt][M].  The first three kernels are rh_loo_expect's over the second buffer's two arrays.
// grid: tiles x p_cnt, blockIdx.x = tile * p_cnt + pair; cols: the chunk's entries of the log-likelihood column list
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_quantile_sort_kernel(const double *__restrict__ ll, const long long iterations, const long long nll, const long long first, const long long thin,
                            const long long kept, const long long S, const int *__restrict__ cols, const int p_cnt, rs_key *__restrict__ ws) {
  __shared__ rs_key lds[RS_TILE_SLOTS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const int pl = (int)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt);
  const long long g0 = tile * RS_TILE;
  if (g0 >= S) return;
  rs_tile_sort(ll + first * nll + cols[pl], iterations, nll, thin, kept, S, g0, lds, ws + (long long)pl * S + g0, LL_BLOCK);
}

// one merge pass over runs of L keys, src -> dst ([p_cnt][S] each); grid: ceil(S / RS_MERGE_TILE) x p_cnt
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_quantile_merge_kernel(const rs_key *__restrict__ src, rs_key *__restrict__ dst, const long long S, const long long L, const int p_cnt) {
  __shared__ rs_key lds[RS_MERGE_LDS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const int pl = (int)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt);
  const long long o0 = tile * RS_MERGE_TILE;
  if (o0 >= S) return;
  rs_merge_tile(src + (long long)pl * S, dst + (long long)pl * S, S, L, o0, lds, LL_BLOCK);
}

// grid: the chunk's pairs; the outputs are indexed by the pair's place in the selection, k_lo + blockIdx.x
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_quantile_fit_kernel(const rs_key *__restrict__ sorted, const long long S, const long long M, const int k_lo, double *__restrict__ tailw,
                           double *__restrict__ pareto_k, int *__restrict__ tail_n) {
  __shared__ double lds[LL_LDS_DOUBLES];
  const long long pl = (long long)blockIdx.x;
  const int k = k_lo + (int)pl;
  lx_fit_block(sorted + pl * S, S, M, lds, tailw + pl * M, pareto_k + k, tail_n + k, LL_BLOCK);
}

// grid: tiles x p_cnt, behind the fit kernel.  lcols: the chunk's entries of the log-likelihood column list; w [p_cnt][S]
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_quantile_weight_kernel(const double *__restrict__ ll, const long long nll, const long long iterations, const long long first, const long long thin,
                              const long long kept, const long long S, const long long M, const int *__restrict__ lcols, const rs_key *__restrict__ sorted,
                              double *__restrict__ w, const double *__restrict__ tailw, const int k_lo, const double *__restrict__ pareto_k,
                              const int *__restrict__ tail_n, const int p_cnt) {
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt);
  const int k = k_lo + (int)pl;
  const long long g0 = tile * RS_TILE;
  if (g0 >= S) return;
  lq_weight_block(sorted + pl * S, S, tailw + pl * M, pareto_k[k], tail_n[k], ll + first * nll + lcols[pl], nll, iterations, thin, kept, g0, w + pl * S, LL_BLOCK);
}

// grid: tiles x p_cnt.  vcols: the chunk's entries of the value column list; w [p_cnt][S] or NULL (plain mode); out_k, out_w [p_cnt][S]
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_quantile_kvsort_kernel(const double *__restrict__ val, const long long iterations, const long long nval, const long long first, const long long thin,
                              const long long kept, const long long S, const int *__restrict__ vcols, const int p_cnt, const double *__restrict__ w,
                              rs_key *__restrict__ out_k, rs_key *__restrict__ out_w) {
  __shared__ rs_key lds[LQ_SORT_LDS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt);
  const long long g0 = tile * LQ_TILE;
  if (g0 >= S) return;
  lq_tile_sort(val + first * nval + vcols[pl], iterations, nval, thin, kept, S, g0, w ? w + pl * S : nullptr, lds, out_k + pl * S + g0, out_w + pl * S + g0, LL_BLOCK);
}

// one merge pass over runs of L pairs, src -> dst; grid: ceil(S / RS_MERGE_TILE) x p_cnt
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_quantile_kvmerge_kernel(const rs_key *__restrict__ src_k, const rs_key *__restrict__ src_w, rs_key *__restrict__ dst_k, rs_key *__restrict__ dst_w,
                               const long long S, const long long L, const int p_cnt) {
  __shared__ rs_key lds[LQ_MERGE_LDS];
  const long long tile = (long long)(blockIdx.x / (unsigned)p_cnt);
  const long long pl = (long long)(blockIdx.x - (unsigned)tile * (unsigned)p_cnt);
  const long long o0 = tile * RS_MERGE_TILE;
  if (o0 >= S) return;
  lq_merge_tile(src_k + pl * S, src_w + pl * S, dst_k + pl * S, dst_w + pl * S, S, L, o0, lds, LL_BLOCK);
}

// grid: the chunk's pairs.  pareto_k [K] or NULL (plain mode): a NaN there says the pair's log-likelihood column is not finite; y [K] or
// NULL; probs [nprobs]; cum [p_cnt][S] (not restrict: written and read across the workgroup's threads); quant [K][nprobs]; crps, spread
// [K] or NULL
extern "C" __global__ void __launch_bounds__(LL_BLOCK)
rh_loo_quantile_scan_kernel(const rs_key *__restrict__ sk, const rs_key *__restrict__ sw, const long long S, const int k_lo, const double *__restrict__ pareto_k,
                            const double *__restrict__ y, const double *__restrict__ probs, const int nprobs, double *cum, double *__restrict__ quant,
                            double *__restrict__ crps, double *__restrict__ spread) {
  __shared__ double lds[LQ_SCAN_LDS_DOUBLES];
  const long long pl = (long long)blockIdx.x;
  const int k = k_lo + (int)pl;
  const bool ll_bad = pareto_k != nullptr && rs_to_key(pareto_k[k]) == RS_KEY_NAN;
  lq_scan_block(sk + pl * S, sw + pl * S, S, ll_bad, y != nullptr, y ? y[k] : 0.0, probs, nprobs, cum + pl * S, lds, quant + (long long)k * nprobs,
                crps ? crps + k : nullptr, spread ? spread + k : nullptr, LL_BLOCK);
}
#endif
#endif
