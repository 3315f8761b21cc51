// rh_predict.hip.h -- Trace.predict / Trace.thin (core/Trace.scala:23-41, core/Generator.scala:59-94) over device-resident draws.
//
// Follows, in one translation unit per requirements program: the defines of emit_predict (RH_NVARS, RH_NREQ, RH_NREF,
// RH_REQ_REF_INIT, RH_EXP / RH_LOG), rh_shared.h, the prelude, and the generated  rh_pred_eval(th, out, err)  whose parameter reads
// are th(slot): slot s stands for parameter rh_req_ref[s], the sorted list of the parameters the program reads.  wave64, gfx950.
//
// draws [chains][iterations][RH_NVARS]; kept iteration j of a chain is row first + j * thin (Trace.thin: i % n == 0 applied to the
// window), j = 0 .. kept - 1; out [chains][kept][RH_NREQ] -- the layout rh_trace.hip.h reads, so the diagnostics of a prediction
// run over this buffer as it is.
//
// One workgroup = one chain x a tile of consecutive kept iterations, one thread per draw of the tile (blockDim.x = tile), in three
// phases separated by barriers:
//   stage     the tile's parameters -> LDS rows [draw][slot] with an ODD row stride, so that lane d's ds_read_b64 of slot s
//             (address d * stride + s) meets no bank twice;
//   evaluate  lane d runs rh_pred_eval on row d.  Register use follows the program's live temporaries, never RH_NREF: no thread
//             holds a parameter vector.  A ragged last tile evaluates its last valid row in the tail lanes -- all lanes run the
//             generated code together, nothing generated sits in a divergent region -- and the tail lanes store nothing;
//   store     the RH_NREQ results of the tile -> LDS [draw][requirement] (odd stride again) -> out with consecutive lanes on
//             consecutive doubles (the tile's results are contiguous in out).  When tile x RH_NREQ does not fit the LDS the lanes
//             store their own rows directly.
// Three kernels, of which a program gets the ones it can use (the choice needs RH_NREF and RH_NVARS -- fixed when the handle is
// created -- and `thin`, an argument of the call):
//   rh_predict_flat_kernel     the program reads at least half of a SHORT parameter vector and thin == 1: the tile's rows are one
//                              contiguous slab of the draws, copied with consecutive lanes on consecutive doubles; LDS rows hold
//                              the whole vector and the accessor reads row[rh_req_ref[s]] (a constant offset after inlining).
//   rh_predict_gather_kernel   otherwise: for each draw of the tile the lanes run along the referenced slots, so runs of adjacent
//                              parameters are contiguous requests and a program that reads 4 of 10 004 parameters fetches 4 cache
//                              lines per draw, not the row.  LDS rows hold the RH_NREF referenced values, the accessor reads row[s].
//   rh_predict_direct_kernel   RH_NREF too large for a wavefront of staged draws (below): nothing is staged, lane d reads its own
//                              row of the draws where the expression needs a value (row[rh_req_ref[s]] in global memory; the
//                              wavefront's 64 rows are walked front to back together and every line fetched is used in full, out
//                              of L2).  Uncoalesced, but still one pass over the referenced doubles and no per-thread vector.
// The tile is as many draws as RP_LDS_DOUBLES (63 KiB: two workgroups share a CU's 160 KiB, as in rh_trace.hip.h) holds, a multiple
// of the wavefront, at most 256.  Bound: the staged forms need one wavefront of draws, 64 x (RH_NREF | 1) <= 8064, i.e.
// RH_NREF <= 125 (flat: RH_NVARS <= 125); at RH_NREF <= 31 the tile is 256 draws.  Beyond the bound the direct kernel is the only one.
//
// Evaluation is per draw: no sum runs across draws, so nothing depends on the tiling, on `first` / `thin` or on the form, and with
// contraction off every value has the bits rh_req_eval gives for the same row.  The lookup-error flag is one atomicOr per wavefront
// that saw one.  The block routine is plain C++ over (thread id, LDS pointer): with RH_PREDICT_HOST defined it compiles with a host
// compiler, every "thread" of a phase run in turn (tests/test_predict_device_cpu.py), same text.
#ifndef RH_PREDICT_HIP_H
#define RH_PREDICT_HIP_H

#define RP_WAVE 64
#define RP_MAX_TILE 256
#define RP_LDS_DOUBLES 8064   // 63 KiB of staged rows per workgroup
// draws per tile for LDS rows of `stride` doubles: whole wavefronts, at most RP_MAX_TILE; 0 = not even one wavefront fits
#define RP_TILE_FOR(stride) ((RP_LDS_DOUBLES / (stride)) >= RP_MAX_TILE ? RP_MAX_TILE : ((RP_LDS_DOUBLES / (stride)) / RP_WAVE) * RP_WAVE)
#define RP_GSTRIDE (RH_NREF | 1)
#define RP_FSTRIDE (RH_NVARS | 1)
#define RP_OSTRIDE (RH_NREQ | 1)
#define RP_GTILE RP_TILE_FOR(RP_GSTRIDE)
#define RP_FTILE RP_TILE_FOR(RP_FSTRIDE)
#define RP_DTILE RP_WAVE
#define RP_HAVE_GATHER (RP_GTILE >= RP_WAVE)
#define RP_HAVE_FLAT (RP_FTILE >= RP_WAVE && 2 * RH_NREF >= RH_NVARS)
#define RP_HAVE_DIRECT (!RP_HAVE_GATHER)
#define RP_FLAT 0
#define RP_GATHER 1
#define RP_DIRECT 2

#ifndef RH_PREDICT_HOST
#define RP_FN static __device__ __forceinline__
#define RP_MEMBER __device__ __forceinline__
#define RP_TABLE static __device__ const
#define RP_SYNC() __syncthreads()
#define RP_TID0 ((int)threadIdx.x)
#define RP_TID1 ((int)threadIdx.x + 1)
#define RP_ST(tid) 0
#define RP_NSTATE 1
// one atomic per wavefront that saw a lookup error (the wavefronts of a tile are whole: blockDim.x is a multiple of 64)
#define RP_FLAG_ERR(err, err_out) do { if (__ballot((err) != 0) != 0ull && (threadIdx.x & (RP_WAVE - 1)) == 0) atomicOr((err_out), 1); } while (0)
#else
#define RP_FN static inline
#define RP_MEMBER inline
#define RP_TABLE static const
#define RP_SYNC() ((void)0)
#define RP_TID0 0
#define RP_TID1 rp_nthreads
#define RP_ST(tid) (tid)
#define RP_NSTATE RP_MAX_TILE
#define RP_FLAG_ERR(err, err_out) do { if ((err) != 0) *(err_out) |= 1; } while (0)
#endif
// every thread of the workgroup (device: this one; host: each in turn -- a phase ends where the device has its barrier)
#define RP_EACH_THREAD(tid) for (int tid = RP_TID0; tid < RP_TID1; tid++)

// slot s of the compact list <-> parameter rh_req_ref[s] (ascending)
RP_TABLE int rh_req_ref[RH_NREF > 0 ? RH_NREF : 1] = RH_REQ_REF_INIT;

// what the generated code reads its parameters through: a row of referenced values (gather), a row of all parameters (flat: LDS,
// direct: the draws themselves)
struct rp_th_slots {
  const double *row;
  RP_MEMBER double operator()(const int s) const { return row[s]; }
};
struct rp_th_params {
  const double *row;
  RP_MEMBER double operator()(const int s) const { return row[rh_req_ref[s]]; }
};

template <int FORM> struct rp_cfg;
template <> struct rp_cfg<RP_FLAT> { static constexpr int TILE = RP_FTILE > 0 ? RP_FTILE : RP_WAVE, STRIDE = RP_FSTRIDE; typedef rp_th_params TH; };
template <> struct rp_cfg<RP_GATHER> { static constexpr int TILE = RP_GTILE > 0 ? RP_GTILE : RP_WAVE, STRIDE = RP_GSTRIDE; typedef rp_th_slots TH; };
template <> struct rp_cfg<RP_DIRECT> { static constexpr int TILE = RP_DTILE, STRIDE = 0; typedef rp_th_params TH; };
// the results travel through LDS when the tile's fit; the workgroup's LDS holds the larger of the two uses
template <int FORM> struct rp_lds {
  static constexpr bool OUT = rp_cfg<FORM>::TILE * RP_OSTRIDE <= RP_LDS_DOUBLES;
  static constexpr int STAGE = rp_cfg<FORM>::TILE * rp_cfg<FORM>::STRIDE, OUTD = OUT ? rp_cfg<FORM>::TILE * RP_OSTRIDE : 0;
  static constexpr int DOUBLES = STAGE > OUTD ? (STAGE > 0 ? STAGE : 1) : (OUTD > 0 ? OUTD : 1);
};

// One chain x one tile.  x: the chain's row `first`; the tile's draws are the kept iterations k0 .. k0 + valid - 1 (1 <= valid <=
// TILE), row (k0 + r) * thin of x.  out: the chain's results at kept iteration k0 (valid * RH_NREQ contiguous doubles).
template <int FORM>
RP_FN void rp_block(const double *x, const int thin, const int k0, const int valid, double *lds, double *out, int *err_out,
                    const int rp_nthreads) {
  typedef rp_cfg<FORM> CF;
  const double *xt = x + (long long)k0 * thin * RH_NVARS;
  const long long rstride = (long long)thin * RH_NVARS;
  // ---- stage
  if constexpr (FORM == RP_FLAT) {          // thin == 1: valid * RH_NVARS contiguous doubles
    const int total = valid * RH_NVARS;
    RP_EACH_THREAD(tid) {
      for (int j = tid; j < total; j += CF::TILE) {
        const int r = j / RH_NVARS, p = j - r * RH_NVARS;
        lds[r * CF::STRIDE + p] = xt[j];
      }
    }
  } else if constexpr (FORM == RP_GATHER) { // lanes along the referenced slots of a draw, then the next draw
    const int total = valid * RH_NREF;
    RP_EACH_THREAD(tid) {
      for (int j = tid; j < total; j += CF::TILE) {
        const int r = RH_NREF > 0 ? j / (RH_NREF > 0 ? RH_NREF : 1) : 0, s = j - r * RH_NREF;
        lds[r * CF::STRIDE + s] = xt[r * rstride + rh_req_ref[s]];
      }
    }
  }
  RP_SYNC();
  // ---- evaluate: every lane, a valid row (the tail lanes of a ragged tile take the last one)
  double o[RP_NSTATE][RH_NREQ];
  RP_EACH_THREAD(tid) {
    const int d = tid < valid ? tid : valid - 1;
    typename CF::TH th;
    th.row = FORM == RP_DIRECT ? xt + d * rstride : lds + d * CF::STRIDE;
    int err = 0;
    rh_pred_eval(th, o[RP_ST(tid)], err);
    RP_FLAG_ERR(err, err_out);
  }
  // ---- store
  if constexpr (rp_lds<FORM>::OUT) {
    RP_SYNC();                    // the staged rows are no longer read
    RP_EACH_THREAD(tid) {
#pragma unroll
      for (int m = 0; m < RH_NREQ; m++) lds[tid * RP_OSTRIDE + m] = o[RP_ST(tid)][m];
    }
    RP_SYNC();
    const int total = valid * RH_NREQ;
    RP_EACH_THREAD(tid) {
      for (int j = tid; j < total; j += CF::TILE) {
        const int r = j / RH_NREQ, m = j - r * RH_NREQ;
        out[j] = lds[r * RP_OSTRIDE + m];
      }
    }
  } else {
    RP_EACH_THREAD(tid) {
      if (tid < valid) {
#pragma unroll
        for (int m = 0; m < RH_NREQ; m++) out[(long long)tid * RH_NREQ + m] = o[RP_ST(tid)][m];
      }
    }
  }
}

#ifndef RH_PREDICT_HOST
// grid: chains x tiles, blockIdx.x = chain * ntiles + tile; blockDim.x = the form's tile
#define RP_KERNEL(name, FORM)                                                                                                       \
  extern "C" __global__ void __launch_bounds__(rp_cfg<FORM>::TILE)                                                                  \
  name(const double *__restrict__ draws, const long long iterations, const int first, const int thin, const int kept,              \
       const int ntiles, double *__restrict__ out, int *__restrict__ err_out) {                                                    \
    __shared__ double lds[rp_lds<FORM>::DOUBLES];                                                                                   \
    const int chain = (int)(blockIdx.x / (unsigned)ntiles), tile = (int)(blockIdx.x - (unsigned)chain * (unsigned)ntiles);         \
    const int k0 = tile * rp_cfg<FORM>::TILE;                                                                                       \
    const int valid = kept - k0 < rp_cfg<FORM>::TILE ? kept - k0 : rp_cfg<FORM>::TILE;                                              \
    rp_block<FORM>(draws + ((long long)chain * iterations + first) * RH_NVARS, thin, k0, valid, lds,                                \
                   out + ((long long)chain * kept + k0) * RH_NREQ, err_out, rp_cfg<FORM>::TILE);                                    \
  }
#if RP_HAVE_FLAT
RP_KERNEL(rh_predict_flat_kernel, RP_FLAT)
#endif
#if RP_HAVE_GATHER
RP_KERNEL(rh_predict_gather_kernel, RP_GATHER)
#endif
#if RP_HAVE_DIRECT
RP_KERNEL(rh_predict_direct_kernel, RP_DIRECT)
#endif
#endif
#endif
