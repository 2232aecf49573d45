/* floxhip — MI355X (gfx950, CDNA4) grouped-reduction kernels.
 *
 * Re-implements, from scratch and HBM-first, the hot path of
 * xarray-contrib/flox: factorize + per-group sum/count/min/max/var
 * (reference flox/core.py:214-394 chunk_reduce, flox/aggregate_flox.py,
 * flox/aggregate_npg.py). Design notes in /root/repo/DESIGN.md.
 *
 * Two paths, selected by group cardinality (the GPU analogue of the
 * reference's _choose_engine, flox/core.py:712-736):
 *
 *  1. LDS-binned scatter (ngroups small enough that the per-group partial
 *     bins fit in the CU's 160 KiB LDS): each 1024-thread workgroup keeps
 *     private bins in LDS, streams its grid-stride share of the rows with
 *     16-byte vector loads (values) + int64 label loads, updates bins with
 *     native LDS atomics (ds_add_f64 / ds_add_u32 / ds_min_u32|u64), then
 *     writes its bins to a per-block slab in HBM with plain coalesced
 *     stores. A combine kernel folds the slab over blocks (fixed order).
 *     Nothing in this path uses inter-workgroup communication.
 *
 *  2. Global-atomic scatter (large ngroups, e.g. the 1e7-group config):
 *     bins live in HBM (LLC-cached), rows update them with device-scope
 *     atomics (global_atomic_add_f64 / _umin / _umax ...). min/max bins are
 *     kept in an order-preserving unsigned encoding so init is a memset and
 *     the atomic is an integer min/max; a decode kernel maps back.
 *
 * Numerics: float32 sums/counts/means/var accumulate in float64 (the
 * numpy_groupies contract, reference tests/test_properties.py:146-151).
 * count/min/max are bit-exact. fp sums use atomics, so the reduction order
 * is not fixed: results are reproducible only to fp-roundoff tolerance
 * (stated in DESIGN.md and the parity tests).
 */

#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include <limits>
#include <cstdio>
#include <cstdlib>

#include "../../include/floxhip.h"
#include "../../include/floxhip_codes.h"

#define FH_CHECK(x)                       \
  do {                                    \
    hipError_t _e = (x);                  \
    if (_e != hipSuccess) return (int)_e + 1000; \
  } while (0)

/* propagate a nonzero return code of a host stage */
#define FH_TRY(x)           \
  do {                      \
    int _rc = (x);          \
    if (_rc) return _rc;    \
  } while (0)

namespace {

constexpr int BLOCK_LDS = 1024;   /* 16 waves/CU at 1 block/CU */
constexpr int BLOCK_ATOMIC = 256;
constexpr int NUM_CU = 256;
constexpr int64_t LDS_MAX = 160 * 1024 - 512; /* gfx950 LDS per workgroup */

/* ---- op-set membership ------------------------------------------------- */
enum {
  B_SUM = 1,
  B_CNT = 2,
  B_PRESENT = 4,
  B_MIN = 8,
  B_MAX = 16,
  B_NANFLAG = 32,
  B_SSD = 64,
  B_PROD = 128,
  B_IDXMIN = 256,
  B_IDXMAX = 512,
  B_WELFORD = 1024,
  B_ARGROW = 2048, /* pair-payload arg-reductions: second bucket pass takes
                      the min row among rows matching the group extremum */
  B_MOM2 = 4096,   /* pivoted single-pass second moment (FH_SET_SUMMARY); with
                      it B_MIN and B_MAX may both be set: min keeps
                      minmax_off, max takes max_off */
  /* single-pass arg-reductions of the column path (FH_SET_ARG*_COLS): the
   * running extremum, its row and the first NaN row per (group, column) */
  B_ARGMINC = 8192,
  B_ARGMAXC = 16384,
};
constexpr int B_ARGC = B_ARGMINC | B_ARGMAXC;
/* the sets k_order_cols serves */
constexpr int B_ORDERC = B_IDXMIN | B_IDXMAX | B_ARGC;
constexpr int OPS_SUMMARY = B_SUM | B_CNT | B_MIN | B_MAX | B_NANFLAG | B_MOM2;

__host__ __device__ constexpr int set_bits(int op_set) {
  switch (op_set) {
    case FH_SET_SUM_COUNT: return B_SUM | B_CNT;
    case FH_SET_SUM_COUNT_PRESENT: return B_SUM | B_CNT | B_PRESENT;
    case FH_SET_COUNT: return B_CNT;
    case FH_SET_MIN_FULL: return B_MIN | B_CNT | B_PRESENT | B_NANFLAG;
    case FH_SET_MIN_COUNT: return B_MIN | B_CNT;
    case FH_SET_MAX_FULL: return B_MAX | B_CNT | B_PRESENT | B_NANFLAG;
    case FH_SET_MAX_COUNT: return B_MAX | B_CNT;
    case FH_SET_SSD: return B_SSD;
    case FH_SET_PROD: return B_PROD | B_CNT | B_PRESENT;
    case FH_SET_IDXMIN: return B_IDXMIN | B_CNT | B_PRESENT;
    case FH_SET_IDXMAX: return B_IDXMAX | B_CNT | B_PRESENT;
    case FH_SET_WELFORD: return B_WELFORD | B_CNT;
    case FH_SET_ARGMIN_PAIR: return B_MIN | B_CNT | B_PRESENT | B_NANFLAG | B_ARGROW;
    case FH_SET_ARGMAX_PAIR: return B_MAX | B_CNT | B_PRESENT | B_NANFLAG | B_ARGROW;
    case FH_SET_SUMMARY: return B_SUM | B_CNT | B_MIN | B_MAX | B_NANFLAG | B_MOM2;
    case FH_SET_ARGMIN_COLS: return B_ARGMINC | B_CNT | B_PRESENT | B_NANFLAG;
    case FH_SET_ARGMAX_COLS: return B_ARGMAXC | B_CNT | B_PRESENT | B_NANFLAG;
    default: return 0;
  }
}

/* ---- per-dtype traits --------------------------------------------------- */
template <typename V> struct Traits;

template <> struct Traits<float> {
  using Acc = double;          /* f64 accumulation (npg contract) */
  using Enc = uint32_t;        /* order-preserving encoding for min/max */
  static constexpr int VEC = 4;
  static __device__ __forceinline__ bool isnan_(float v) { return v != v; }
  static __device__ __forceinline__ Enc enc(float v) {
    uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  static __device__ __forceinline__ float dec(Enc u) {
    uint32_t r = (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u;
    return __uint_as_float(r);
  }
  static __device__ __forceinline__ float pos_inf() { return __builtin_inff(); }
  /* pivot slot of the summary set: never 0 (0 decodes to a NaN), so 0 = EMPTY */
  static __device__ __forceinline__ Enc piv_enc(float v) { return enc(v); }
  static __device__ __forceinline__ double piv_dec(Enc e) { return (double)dec(e); }
};

template <> struct Traits<double> {
  using Acc = double;
  using Enc = uint64_t;
  static constexpr int VEC = 2;
  static __device__ __forceinline__ bool isnan_(double v) { return v != v; }
  static __device__ __forceinline__ Enc enc(double v) {
    uint64_t u = __double_as_longlong(v);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
  }
  static __device__ __forceinline__ double dec(Enc u) {
    uint64_t r = (u & 0x8000000000000000ull) ? (u ^ 0x8000000000000000ull) : ~u;
    return __longlong_as_double((long long)r);
  }
  static __device__ __forceinline__ double pos_inf() { return __builtin_inf(); }
  static __device__ __forceinline__ Enc piv_enc(double v) { return enc(v); }
  static __device__ __forceinline__ double piv_dec(Enc e) { return dec(e); }
};

template <> struct Traits<int32_t> {
  using Acc = int64_t;         /* numpy promotes i32 sums to platform int */
  using Enc = uint32_t;
  static constexpr int VEC = 4;
  static __device__ __forceinline__ bool isnan_(int32_t) { return false; }
  static __device__ __forceinline__ Enc enc(int32_t v) {
    return (uint32_t)v ^ 0x80000000u;   /* order-preserving signed->unsigned */
  }
  static __device__ __forceinline__ int32_t dec(Enc u) { return (int32_t)(u ^ 0x80000000u); }
  static __device__ __forceinline__ int32_t pos_inf() { return INT32_MAX; }
  /* every integer is a legal value, so the pivot is the value with bit 0 set:
   * within 1 of a row of the group (all a pivot has to be) and never 0 = EMPTY */
  static __device__ __forceinline__ Enc piv_enc(int32_t v) { return (uint32_t)v | 1u; }
  static __device__ __forceinline__ double piv_dec(Enc e) { return (double)(int32_t)e; }
};

template <> struct Traits<int64_t> {
  using Acc = int64_t;
  using Enc = uint64_t;
  static constexpr int VEC = 2;
  static __device__ __forceinline__ bool isnan_(int64_t) { return false; }
  static __device__ __forceinline__ Enc enc(int64_t v) {
    return (uint64_t)v ^ 0x8000000000000000ull;
  }
  static __device__ __forceinline__ int64_t dec(Enc u) {
    return (int64_t)(u ^ 0x8000000000000000ull);
  }
  static __device__ __forceinline__ int64_t pos_inf() { return INT64_MAX; }
  static __device__ __forceinline__ Enc piv_enc(int64_t v) { return (uint64_t)v | 1ull; }
  static __device__ __forceinline__ double piv_dec(Enc e) { return (double)(int64_t)e; }
};

/* atomic add on the accumulator type (LDS or global pointer) */
__device__ __forceinline__ void acc_add(double* p, double v) { atomicAdd(p, v); }
__device__ __forceinline__ void acc_add(int64_t* p, int64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}
__device__ __forceinline__ void enc_min(uint32_t* p, uint32_t v) { atomicMin(p, v); }
__device__ __forceinline__ void enc_min(uint64_t* p, uint64_t v) {
  atomicMin(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}
__device__ __forceinline__ void enc_max(uint32_t* p, uint32_t v) { atomicMax(p, v); }
__device__ __forceinline__ void enc_max(uint64_t* p, uint64_t v) {
  atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}
/* claim an EMPTY (0) slot; returns what the slot held before */
__device__ __forceinline__ uint32_t enc_claim(uint32_t* p, uint32_t v) {
  return atomicCAS(p, 0u, v);
}
__device__ __forceinline__ uint64_t enc_claim(uint64_t* p, uint64_t v) {
  return (uint64_t)atomicCAS(reinterpret_cast<unsigned long long*>(p), 0ull,
                             (unsigned long long)v);
}
__device__ __forceinline__ void idx_min(int64_t* p, int64_t v) {
  atomicMin(reinterpret_cast<long long*>(p), (long long)v);
}
__device__ __forceinline__ void idx_max(int64_t* p, int64_t v) {
  atomicMax(reinterpret_cast<long long*>(p), (long long)v);
}

/* CAS product (prod is rare; contention-tolerant CAS loop) */
__device__ __forceinline__ void acc_mul(double* p, double v) {
  unsigned long long* u = reinterpret_cast<unsigned long long*>(p);
  unsigned long long old = *u, assumed;
  do {
    assumed = old;
    double cur = __longlong_as_double((long long)assumed);
    old = atomicCAS(u, assumed, (unsigned long long)__double_as_longlong(cur * v));
  } while (old != assumed);
}
__device__ __forceinline__ void acc_mul(int64_t* p, int64_t v) {
  unsigned long long* u = reinterpret_cast<unsigned long long*>(p);
  unsigned long long old = *u, assumed;
  do {
    assumed = old;
    old = atomicCAS(u, assumed, (unsigned long long)((int64_t)assumed * v));
  } while (old != assumed);
}

/* 16-byte-aligned vector type for coalesced loads */
template <typename T, int N> struct alignas(sizeof(T) * N) Vec { T v[N]; };

/* ---- bin layout (shared between LDS carve, slab and combine) ------------ */
struct BinLayout {
  int64_t sum_off, cnt_off, present_off, minmax_off, nanflag_off, sumx_off;
  int64_t bytes;  /* per block-copy of the bins */
  /* B_MOM2 only, carved after every older section: max (minmax_off is then
   * the min), the pivot x0, s1 and s2 (in the slab: the block's mean as
   * x0 + s1/n, and its M2) */
  int64_t max_off, s1_off, s2_off, pivot_off;
  /* B_ARGC only (the column path's slab), carved last: the chunk's extremum
   * as the value's own bits, and its first NaN row (int64); the extremum's
   * row has sum_off */
  int64_t argval_off, nanrow_off;
};

template <typename V>
__host__ __device__ BinLayout bin_layout(int bits, int64_t ngroups, int64_t cnt_elem_size) {
  BinLayout L{};
  int64_t off = 0;
  auto carve = [&](int64_t elem) {
    int64_t o = off;
    off += ((ngroups * elem + 255) / 256) * 256; /* 256-B aligned sections */
    return o;
  };
  L.sum_off = (bits & (B_SUM | B_SSD | B_PROD | B_IDXMIN | B_IDXMAX | B_WELFORD | B_ARGC)) ? carve(8) : -1;
  L.cnt_off = (bits & B_CNT) ? carve(cnt_elem_size) : -1;
  L.present_off = (bits & B_PRESENT) ? carve(4) : -1;
  L.minmax_off = (bits & (B_MIN | B_MAX)) ? carve(sizeof(typename Traits<V>::Enc)) : -1;
  L.nanflag_off = (bits & B_NANFLAG) ? carve(4) : -1;
  L.sumx_off = (bits & B_WELFORD) ? carve(8) : -1;
  L.max_off = L.s1_off = L.s2_off = L.pivot_off = -1;
  if (bits & B_MOM2) {
    L.max_off = carve(sizeof(typename Traits<V>::Enc));
    L.s1_off = carve(8);
    L.s2_off = carve(8);
    L.pivot_off = carve(sizeof(typename Traits<V>::Enc));
  }
  L.argval_off = L.nanrow_off = -1;
  if (bits & B_ARGC) {
    L.argval_off = carve(sizeof(V));
    L.nanrow_off = carve(8);
  }
  L.bytes = off;
  return L;
}

/* streaming vector load of one Vec. Every input byte of the LDS kernel is
 * read once. NT = nontemporal 16-byte loads: 4.4-5.5 % faster for the
 * int64/int32-label forms (12 B/row), no difference for the u16-code form,
 * which keeps plain loads (profiles/r03_label_cache.md), 3 % faster for the
 * packed-code form (profiles/r06_packed_codes.md). Vecs narrower
 * than 16 B are loaded plainly either way. */
template <typename VT, bool NT>
__device__ __forceinline__ VT ld_vec(const void* p) {
  if constexpr (NT && sizeof(VT) % 16 == 0) {
    using u32x4 = uint32_t __attribute__((ext_vector_type(4)));
    VT t;
#pragma unroll
    for (int j = 0; j < (int)(sizeof(VT) / 16); ++j) {
      u32x4 r = __builtin_nontemporal_load((const u32x4*)p + j);
      __builtin_memcpy((char*)&t + 16 * j, &r, 16);
    }
    return t;
  } else {
    return *reinterpret_cast<const VT*>(p);
  }
}

constexpr uint32_t CODE_NONE = 0xFFFFu; /* u16 code of a row in no group */
constexpr int U16_ROWS = 8;  /* rows per lane per iteration, u16-code form */
constexpr int EMIT_ROWS = 4; /* rows per lane per iteration when emitting */

/* label tags of the packed code forms (include/floxhip_codes.h): `labels`
 * then points at whole tiles of W-bit codes, 16 rows per lane per tile */
template <int W> struct PackedCodes { static constexpr int width = W; };
/* bits per cached code of a label type; 0 = the caller's own labels */
template <typename L> struct CodeWidth { static constexpr int value = 0; };
template <> struct CodeWidth<uint16_t> { static constexpr int value = 16; };
template <int W> struct CodeWidth<PackedCodes<W>> { static constexpr int value = W; };

/* a lane's W/2 dwords of one tile: one load per plane. Nontemporal, like
 * the values of the packed form: 3 % faster there than plain loads
 * (profiles/r06_packed_codes.md), unlike in the u16 form. */
template <int W>
__device__ __forceinline__ void ld_packed(const char* tile, int lane, uint32_t* cw) {
  using u32x4 = uint32_t __attribute__((ext_vector_type(4)));
  using u32x2 = uint32_t __attribute__((ext_vector_type(2)));
  const u32x4 a = __builtin_nontemporal_load((const u32x4*)(tile + lane * 16));
  const u32x2 b =
      __builtin_nontemporal_load((const u32x2*)(tile + FH_PLANE8_OFF + lane * 8));
  cw[0] = a.x, cw[1] = a.y, cw[2] = a.z, cw[3] = a.w;
  cw[4] = b.x, cw[5] = b.y;
  if constexpr (W == 14)
    cw[6] = __builtin_nontemporal_load(
        (const uint32_t*)(tile + FH_PLANE4_OFF + lane * 4));
}

/* ---- kernel 1: LDS-binned grouped reduce --------------------------------
 * L = uint16_t: labels are precomputed final codes (CODE_NONE = no group,
 * labels2 unused); each lane takes U16_ROWS rows per iteration so that every
 * stream is still read with 16-byte loads (one for the codes, 32 or 64 B of
 * values). L = PackedCodes<W>: the same codes at W = 12 or 14 bits; a wave
 * takes one 1024-row tile per iteration, each lane W/2 dwords of codes (two
 * or three coalesced loads) and 16 values in 16-byte loads. EMIT: the
 * int64/int32-label run also writes each row's final code to `emit`
 * (EMIT_ROWS rows per lane, one 8-byte store). */
template <typename V, typename L, int OPS, bool EMIT = false>
__launch_bounds__(BLOCK_LDS) __global__ void k_reduce_lds(
    const V* __restrict__ values, const L* __restrict__ labels,
    const L* __restrict__ labels2, int64_t n, int64_t ngroups, int64_t g0,
    int64_t g1, const double* __restrict__ means,
    const V* __restrict__ target, int64_t row_offset, int skipnan,
    char* __restrict__ slab, BinLayout lay, uint16_t* __restrict__ emit) {
  using TR = Traits<V>;
  using Acc = typename TR::Acc;
  using SumT = typename std::conditional<
      (OPS & (B_SSD | B_WELFORD)) != 0, double,
      typename std::conditional<(OPS & (B_IDXMIN | B_IDXMAX)) != 0, int64_t, Acc>::type>::type;
  using Enc = typename TR::Enc;
  constexpr int VEC = TR::VEC;
  constexpr bool IS_PROD = (OPS & B_PROD) != 0;
  constexpr bool MOM2 = (OPS & B_MOM2) != 0;
  static_assert(!MOM2 || OPS == OPS_SUMMARY, "B_MOM2 exists in the summary set only");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  SumT* s_sum = (OPS & (B_SUM | B_SSD | B_PROD | B_IDXMIN | B_IDXMAX)) ? (SumT*)(smem + lay.sum_off) : nullptr;
  uint32_t* s_cnt = (OPS & B_CNT) ? (uint32_t*)(smem + lay.cnt_off) : nullptr;
  uint32_t* s_present = (OPS & B_PRESENT) ? (uint32_t*)(smem + lay.present_off) : nullptr;
  Enc* s_mm = (OPS & (B_MIN | B_MAX)) ? (Enc*)(smem + lay.minmax_off) : nullptr;
  uint32_t* s_nanflag = (OPS & B_NANFLAG) ? (uint32_t*)(smem + lay.nanflag_off) : nullptr;
  /* summary set: s_mm is the min, the max has its own section */
  Enc* s_mx = MOM2 ? (Enc*)(smem + lay.max_off) : s_mm;
  double* s_s1 = MOM2 ? (double*)(smem + lay.s1_off) : nullptr;
  double* s_s2 = MOM2 ? (double*)(smem + lay.s2_off) : nullptr;
  Enc* s_piv = MOM2 ? (Enc*)(smem + lay.pivot_off) : nullptr;

  const int tid = threadIdx.x;
  for (int64_t g = tid; g < ngroups; g += blockDim.x) {
    if (OPS & (B_SUM | B_SSD)) s_sum[g] = (SumT)0;
    if (IS_PROD) s_sum[g] = (SumT)1;
    if (OPS & B_IDXMIN) s_sum[g] = (SumT)INT64_MAX;
    if (OPS & B_IDXMAX) s_sum[g] = (SumT)(-1);
    if (OPS & B_CNT) s_cnt[g] = 0u;
    if (OPS & B_PRESENT) s_present[g] = 0u;
    if (OPS & B_MIN) s_mm[g] = (Enc)~(Enc)0;
    if (OPS & B_MAX) s_mx[g] = (Enc)0;
    if (OPS & B_NANFLAG) s_nanflag[g] = 0u;
    if constexpr (MOM2) {
      s_s1[g] = 0.0;
      s_s2[g] = 0.0;
      s_piv[g] = (Enc)0; /* EMPTY */
    }
  }
  __syncthreads();

  const bool twolab = labels2 != nullptr;

  /* returns the row's final code (CODE_NONE when it is in no group) */
  auto process = [&](V v, int64_t l0raw, int64_t l1raw, int64_t row) -> uint32_t {
    uint64_t code;
    if (twolab) {
      if ((uint64_t)l0raw >= (uint64_t)g0 || (uint64_t)l1raw >= (uint64_t)g1) return CODE_NONE;
      code = (uint64_t)l0raw * (uint64_t)g1 + (uint64_t)l1raw;
    } else {
      if ((uint64_t)l0raw >= (uint64_t)ngroups) return CODE_NONE;
      code = (uint64_t)l0raw;
    }
    const uint32_t rcode = (uint32_t)code;
    const bool vnan = TR::isnan_(v);
    if (OPS & B_PRESENT) s_present[code] = 1u;  /* benign write race: all store 1 */
    if constexpr (MOM2) {
      /* a NaN row leaves its mark and nothing else, whatever skipnan says */
      if (vnan) {
        s_nanflag[code] = 1u;
        return rcode;
      }
    }
    if (vnan && skipnan) return rcode;
    if (OPS & B_SUM) acc_add(&s_sum[code], (Acc)v);
    if (IS_PROD) acc_mul(&s_sum[code], (Acc)v);
    if (OPS & B_SSD) {
      double d = (double)v - means[code];
      atomicAdd((double*)s_sum + code, d * d);
    }
    if (OPS & (B_IDXMIN | B_IDXMAX)) {
      /* candidate: every surviving row, or rows matching the per-group
       * target value (NaN target matches NaN rows: argmax over data with
       * NaNs lands on the first NaN, as np.argmax does) */
      bool match = true;
      if (target) {
        const V t = target[code];
        match = vnan ? TR::isnan_(t) : (!TR::isnan_(t) && v == t);
      }
      if (match) {
        if (OPS & B_IDXMIN) idx_min((int64_t*)s_sum + code, row + row_offset);
        if (OPS & B_IDXMAX) idx_max((int64_t*)s_sum + code, row + row_offset);
      }
    }
    if (OPS & B_CNT) {
      if (!vnan) atomicAdd(&s_cnt[code], 1u);
    }
    if (OPS & (B_MIN | B_MAX)) {
      if (vnan) {
        if (OPS & B_NANFLAG) s_nanflag[code] = 1u;
      } else {
        if (OPS & B_MIN) enc_min(&s_mm[code], TR::enc(v));
        if (OPS & B_MAX) enc_max(&s_mx[code], TR::enc(v));
      }
    }
    if constexpr (MOM2) {
      /* deviations about the block's pivot for this group: the first value
       * to claim the slot. Steady state is one plain LDS read; a stale EMPTY
       * only costs a CAS that returns the pivot already there. */
      Enc pe = s_piv[code];
      if (pe == (Enc)0) {
        const Enc mine = TR::piv_enc(v);
        const Enc old = enc_claim(&s_piv[code], mine);
        pe = old != (Enc)0 ? old : mine;
      }
      const double d = (double)v - TR::piv_dec(pe);
      atomicAdd(&s_s1[code], d);
      atomicAdd(&s_s2[code], d * d);
    }
    return rcode;
  };

  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + tid;
  if constexpr (std::is_same<L, uint16_t>::value) {
    /* compact codes: one 16-B code load + U16_ROWS values per lane. The
     * sentinel fails the bounds check in process() like any other
     * out-of-range label. */
    static_assert(!EMIT, "u16 codes are never re-emitted");
    const int64_t nvec = n / U16_ROWS;
    for (int64_t i = gtid; i < nvec; i += stride) {
      const int64_t r0 = i * U16_ROWS;
      Vec<uint16_t, U16_ROWS> cv = ld_vec<Vec<uint16_t, U16_ROWS>, false>(labels + r0);
      Vec<V, VEC> vv[U16_ROWS / VEC];
#pragma unroll
      for (int j = 0; j < U16_ROWS / VEC; ++j)
        vv[j] = ld_vec<Vec<V, VEC>, false>(values + r0 + j * VEC);
#pragma unroll
      for (int k = 0; k < U16_ROWS; ++k)
        process(vv[k / VEC].v[k % VEC], (int64_t)cv.v[k], 0, r0 + k);
    }
    for (int64_t i = nvec * U16_ROWS + gtid; i < n; i += stride)
      process(values[i], (int64_t)labels[i], 0, i);
  } else if constexpr (CodeWidth<L>::value != 0) {
    /* packed codes: whole tiles, one per wave per iteration. The buffer is
     * padded to whole tiles, so the code loads need no guard; the values
     * are read past a full tile only row by row, never past n. */
    constexpr int W = CodeWidth<L>::value;
    static_assert(!EMIT, "packed codes are never re-emitted");
    const int lane = tid & (FH_TILE_LANES - 1);
    const int64_t nwaves = stride / FH_TILE_LANES;
    const int64_t nfull = n / FH_TILE_ROWS;
    const char* codes = reinterpret_cast<const char*>(labels);
    int64_t tile = gtid / FH_TILE_LANES;
    for (; tile < nfull; tile += nwaves) {
      uint32_t cw[W / 2];
      ld_packed<W>(codes + tile * (FH_TILE_ROWS / 8 * W), lane, cw);
      Vec<V, VEC> vv[FH_LANE_SLOTS / VEC];
      const int64_t r0 = tile * FH_TILE_ROWS + lane * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < 4 / VEC; ++h)
          vv[j * (4 / VEC) + h] =
              ld_vec<Vec<V, VEC>, true>(values + r0 + j * 256 + h * VEC);
#pragma unroll
      for (int s = 0; s < FH_LANE_SLOTS; ++s)
        process(vv[s / VEC].v[s % VEC], (int64_t)fh_unpack1<W>(cw, s), 0,
                r0 + (s >> 2) * 256 + (s & 3));
    }
    if (tile == nfull && nfull * FH_TILE_ROWS < n) {
      /* the last, partial tile: the one wave whose turn it is */
      uint32_t cw[W / 2];
      ld_packed<W>(codes + tile * (FH_TILE_ROWS / 8 * W), lane, cw);
#pragma unroll
      for (int s = 0; s < FH_LANE_SLOTS; ++s) {
        const int64_t row = fh_tile_row(tile, lane, s);
        if (row < n) process(values[row], (int64_t)fh_unpack1<W>(cw, s), 0, row);
      }
    }
  } else if constexpr (EMIT) {
    const int64_t nvec = n / EMIT_ROWS;
    for (int64_t i = gtid; i < nvec; i += stride) {
      const int64_t r0 = i * EMIT_ROWS;
      Vec<V, VEC> vv[EMIT_ROWS / VEC];
#pragma unroll
      for (int j = 0; j < EMIT_ROWS / VEC; ++j)
        vv[j] = ld_vec<Vec<V, VEC>, true>(values + r0 + j * VEC);
      Vec<L, EMIT_ROWS> lv = ld_vec<Vec<L, EMIT_ROWS>, true>(labels + r0);
      Vec<L, EMIT_ROWS> lv2 = lv;
      if (twolab) lv2 = ld_vec<Vec<L, EMIT_ROWS>, true>(labels2 + r0);
      Vec<uint16_t, EMIT_ROWS> cv;
#pragma unroll
      for (int k = 0; k < EMIT_ROWS; ++k)
        cv.v[k] = (uint16_t)process(vv[k / VEC].v[k % VEC], (int64_t)lv.v[k],
                                    (int64_t)lv2.v[k], r0 + k);
      *reinterpret_cast<Vec<uint16_t, EMIT_ROWS>*>(emit + r0) = cv;
    }
    for (int64_t i = nvec * EMIT_ROWS + gtid; i < n; i += stride)
      emit[i] = (uint16_t)process(values[i], (int64_t)labels[i],
                                  twolab ? (int64_t)labels2[i] : 0, i);
  } else {
    const int64_t nvec = n / VEC;
    for (int64_t i = gtid; i < nvec; i += stride) {
      Vec<V, VEC> vv = ld_vec<Vec<V, VEC>, true>(values + i * VEC);
      Vec<L, VEC> lv = ld_vec<Vec<L, VEC>, true>(labels + i * VEC);
      if (twolab) {
        Vec<L, VEC> lv2 = ld_vec<Vec<L, VEC>, true>(labels2 + i * VEC);
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          process(vv.v[k], (int64_t)lv.v[k], (int64_t)lv2.v[k], i * VEC + k);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) process(vv.v[k], (int64_t)lv.v[k], 0, i * VEC + k);
      }
    }
    /* tail */
    for (int64_t i = nvec * VEC + gtid; i < n; i += stride) {
      process(values[i], (int64_t)labels[i], twolab ? (int64_t)labels2[i] : 0, i);
    }
  }

  __syncthreads();
  /* flush bins to this block's slab section with plain coalesced stores */
  char* my = slab + (int64_t)blockIdx.x * lay.bytes;
  for (int64_t g = tid; g < ngroups; g += blockDim.x) {
    if (OPS & (B_SUM | B_SSD | B_PROD | B_IDXMIN | B_IDXMAX)) ((SumT*)(my + lay.sum_off))[g] = s_sum[g];
    if (OPS & B_CNT) ((uint32_t*)(my + lay.cnt_off))[g] = s_cnt[g];
    if (OPS & B_PRESENT) ((uint32_t*)(my + lay.present_off))[g] = s_present[g];
    if (OPS & (B_MIN | B_MAX)) ((Enc*)(my + lay.minmax_off))[g] = s_mm[g];
    if (OPS & B_NANFLAG) ((uint32_t*)(my + lay.nanflag_off))[g] = s_nanflag[g];
    if constexpr (MOM2) {
      ((Enc*)(my + lay.max_off))[g] = s_mx[g];
      /* the block's (n, mean, M2) triple; n travels in the count section and
       * the mean in two parts, pivot x0 and offset s1/n: summed into one
       * double it would round at ulp(x0), and the merge is first-order in
       * the difference of two means */
      const uint32_t nb = s_cnt[g];
      double off_b = 0.0, m2_b = 0.0;
      if (nb) {
        const double s1 = s_s1[g], s2 = s_s2[g], dn = (double)nb;
        off_b = s1 / dn;
        m2_b = s2 - s1 * s1 / dn;
        if (m2_b < 0.0) m2_b = 0.0; /* rounding only: M2 >= 0 by Cauchy-Schwarz */
      }
      ((Enc*)(my + lay.pivot_off))[g] = s_piv[g];
      ((double*)(my + lay.s1_off))[g] = off_b;
      ((double*)(my + lay.s2_off))[g] = m2_b;
    }
  }
}

/* Chan's pairwise merge of two (n, mean, M2) partials into a; an empty side
 * is skipped, so no 0/0 enters. Unlike the closed form of k_combine's
 * B_WELFORD branch it never subtracts squared sums, so it stays accurate when
 * mean^2 >> var. A mean is piv + off, piv a value of the group: the pivots
 * subtract exactly where the data is clustered (the hard case) and the
 * offsets are small, so d keeps the precision a single rounded mean loses.
 * The merged mean stays relative to a's pivot. */
__device__ __forceinline__ void chan_merge(double na, double& piv_a, double& off_a,
                                           double& m2_a, double nb, double piv_b,
                                           double off_b, double m2_b) {
  if (nb == 0.0) return;
  if (na == 0.0) {
    piv_a = piv_b;
    off_a = off_b;
    m2_a = m2_b;
    return;
  }
  const double nt = na + nb, d = (piv_b - piv_a) + (off_b - off_a);
  off_a += d * (nb / nt);
  m2_a += m2_b + d * d * (na * nb / nt);
}

/* the column kernel's pivot in the slab's pivot section (one Enc per bin):
 * x0 is a double in registers, (double)v of a row. 8-byte dtypes store its
 * bits; 4-byte dtypes store v itself, which (double) restores exactly. */
template <typename V>
__device__ __forceinline__ typename Traits<V>::Enc cols_piv_pack(double x0) {
  if constexpr (sizeof(V) == 8) {
    return (uint64_t)__double_as_longlong(x0);
  } else if constexpr (std::is_same<V, float>::value) {
    return __float_as_uint((float)x0);
  } else {
    return (uint32_t)(int32_t)x0;
  }
}
template <typename V>
__device__ __forceinline__ double cols_piv_unpack(typename Traits<V>::Enc e) {
  if constexpr (sizeof(V) == 8) {
    return __longlong_as_double((long long)e);
  } else if constexpr (std::is_same<V, float>::value) {
    return (double)__uint_as_float(e);
  } else {
    return (double)(int32_t)e;
  }
}

/* ---- kernel 2: combine per-chunk slabs (column path) ---------------------
 * one thread per bin folds every chunk's partial and writes the final bin
 * (min/max decoded inline). The LDS-binned path folds its per-block slab
 * with k_combine_tree below. The summary set folds the chunks' (n, x0 + off,
 * M2) triples in chunk order with chan_merge, as k_combine_tree does. */
template <typename V, int OPS>
__global__ void k_combine(const char* __restrict__ slab, int nblocks,
                          int64_t ngroups, BinLayout lay, void* out_sum,
                          int64_t* out_count, uint32_t* out_present,
                          void* out_min, void* out_max, uint32_t* out_nanflag,
                          double* out_ssd) {
  using TR = Traits<V>;
  using Acc = typename TR::Acc;
  using SumT = typename std::conditional<
      (OPS & (B_SSD | B_WELFORD)) != 0, double,
      typename std::conditional<(OPS & (B_IDXMIN | B_IDXMAX)) != 0, int64_t, Acc>::type>::type;
  using Enc = typename TR::Enc;
  constexpr bool IS_PROD = (OPS & B_PROD) != 0;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngroups) return;
  if constexpr ((OPS & B_MOM2) != 0) {
    Acc s = 0;
    int64_t c = 0;
    uint32_t nf = 0;
    Enc mn = (Enc)~(Enc)0, mx = (Enc)0;
    double piv = 0.0, off = 0.0, m2 = 0.0;
    for (int b = 0; b < nblocks; ++b) {
      const char* blk = slab + (int64_t)b * lay.bytes;
      const uint32_t nb = ((const uint32_t*)(blk + lay.cnt_off))[g];
      chan_merge((double)c, piv, off, m2, (double)nb,
                 cols_piv_unpack<V>(((const Enc*)(blk + lay.pivot_off))[g]),
                 ((const double*)(blk + lay.s1_off))[g],
                 ((const double*)(blk + lay.s2_off))[g]);
      s += ((const Acc*)(blk + lay.sum_off))[g];
      c += (int64_t)nb;
      const Enc lo = ((const Enc*)(blk + lay.minmax_off))[g];
      const Enc hi = ((const Enc*)(blk + lay.max_off))[g];
      mn = lo < mn ? lo : mn;
      mx = hi > mx ? hi : mx;
      nf |= ((const uint32_t*)(blk + lay.nanflag_off))[g];
    }
    ((Acc*)out_sum)[g] = s;
    out_count[g] = c;
    out_nanflag[g] = nf;
    out_present[g] = (c != 0 || nf != 0) ? 1u : 0u; /* any row seen */
    ((V*)out_min)[g] = c != 0 ? TR::dec(mn) : TR::pos_inf();
    ((V*)out_max)[g] = c != 0 ? TR::dec(mx) : (V)-TR::pos_inf();
    out_ssd[g] = m2 > 0.0 ? m2 : 0.0;
    return;
  }
  if constexpr ((OPS & B_ARGC) != 0) {
    /* (value, row, NaN row) per chunk: the better value wins, equal values
     * (==, so -0.0 ties +0.0) the smaller row; the smallest NaN row beats
     * every value. A skipping chunk never writes a NaN row. */
    constexpr bool ISMAX = (OPS & B_ARGMAXC) != 0;
    int64_t c = 0, row = INT64_MAX, nanrow = INT64_MAX;
    uint32_t p = 0, nf = 0;
    V best = (V)0;
    for (int b = 0; b < nblocks; ++b) {
      const char* blk = slab + (int64_t)b * lay.bytes;
      c += (int64_t)((const uint32_t*)(blk + lay.cnt_off))[g];
      p |= ((const uint32_t*)(blk + lay.present_off))[g];
      nf |= ((const uint32_t*)(blk + lay.nanflag_off))[g];
      const int64_t nr = ((const int64_t*)(blk + lay.nanrow_off))[g];
      nanrow = nr < nanrow ? nr : nanrow;
      const int64_t r = ((const int64_t*)(blk + lay.sum_off))[g];
      if (r == INT64_MAX) continue;
      const V x = ((const V*)(blk + lay.argval_off))[g];
      const bool better = ISMAX ? x > best : x < best;
      if (row == INT64_MAX || better || (x == best && r < row)) {
        best = x;
        row = r;
      }
    }
    ((int64_t*)out_sum)[g] = nanrow != INT64_MAX ? nanrow : row;
    out_count[g] = c;
    out_present[g] = p;
    out_nanflag[g] = nf;
    return;
  }
  SumT s = IS_PROD ? (SumT)1 : (SumT)0;
  if (OPS & B_IDXMIN) s = (SumT)INT64_MAX;
  if (OPS & B_IDXMAX) s = (SumT)(-1);
  int64_t c = 0;
  uint32_t p = 0, nf = 0;
  double w_sum = 0.0;
  Enc mn = (Enc)~(Enc)0, mx = (Enc)0;
  for (int b = 0; b < nblocks; ++b) {
    const char* blk = slab + (int64_t)b * lay.bytes;
    if (OPS & (B_SUM | B_SSD)) s += ((const SumT*)(blk + lay.sum_off))[g];
    if (OPS & B_WELFORD) {
      /* pairwise var merge: fold ssd_i + sum_i^2/n_i, subtract the global
       * term after the loop (the reference's _var_combine adjustment,
       * aggregations.py:392-451, in closed form) */
      const double ssd_i = ((const double*)(blk + lay.sum_off))[g];
      const double sum_i = ((const double*)(blk + lay.sumx_off))[g];
      const double n_i = (double)((const uint32_t*)(blk + lay.cnt_off))[g];
      s += (SumT)(ssd_i + (n_i > 0.0 ? (sum_i * sum_i) / n_i : 0.0));
      w_sum += sum_i;
    }
    if (IS_PROD) s *= ((const SumT*)(blk + lay.sum_off))[g];
    if (OPS & B_IDXMIN) {
      const SumT x = ((const SumT*)(blk + lay.sum_off))[g];
      s = x < s ? x : s;
    }
    if (OPS & B_IDXMAX) {
      const SumT x = ((const SumT*)(blk + lay.sum_off))[g];
      s = x > s ? x : s;
    }
    if (OPS & B_CNT) c += (int64_t)((const uint32_t*)(blk + lay.cnt_off))[g];
    if (OPS & B_PRESENT) p |= ((const uint32_t*)(blk + lay.present_off))[g];
    if (OPS & B_MIN) {
      Enc e = ((const Enc*)(blk + lay.minmax_off))[g];
      mn = e < mn ? e : mn;
    }
    if (OPS & B_MAX) {
      Enc e = ((const Enc*)(blk + lay.minmax_off))[g];
      mx = e > mx ? e : mx;
    }
    if (OPS & B_NANFLAG) nf |= ((const uint32_t*)(blk + lay.nanflag_off))[g];
  }
  const bool present = (OPS & B_PRESENT) ? (p != 0) : (c != 0);
  if (OPS & B_WELFORD) {
    const double total = (double)s - (c > 0 ? (w_sum * w_sum) / (double)c : 0.0);
    ((double*)out_sum)[g] = c > 0 ? total : 0.0;
    ((double*)out_min)[g] = w_sum;
    out_count[g] = c;
    return;
  }
  if (OPS & (B_SUM | B_SSD | B_PROD | B_IDXMIN | B_IDXMAX)) ((SumT*)out_sum)[g] = s;
  if (OPS & B_CNT) out_count[g] = c;
  if (OPS & B_PRESENT) out_present[g] = p;
  if (OPS & B_MIN) ((V*)out_min)[g] = present ? TR::dec(mn) : TR::pos_inf();
  if (OPS & B_MAX) ((V*)out_max)[g] = present ? TR::dec(mx) : (V)-TR::pos_inf();
  if (OPS & B_NANFLAG) out_nanflag[g] = nf;
}

/* ---- kernel 2b: tree combine of the LDS path's per-block slab -------------
 * Thread block = CT_X consecutive groups (x) by CT_Y slab-block lanes (y).
 * Thread (x, y) folds slab blocks y, y + CT_Y, ... of its group in registers
 * (a wave reads two rows of CT_X consecutive bins: 256 B per f64 row), the
 * CT_Y partials are folded through LDS in a fixed halving order, and the
 * y == 0 threads write the final bins: no pre-zeroed outputs, no atomics, no
 * decode pass, and a fold order that depends only on nblocks. CT_X = 32 keeps
 * 1e4 groups at 313 blocks; a handful of groups is a single block.
 *
 * FIN != FIN_NONE finishes the aggregation in the same threads instead of
 * writing partials: one result value per group, in fa.rdtype, with the fill
 * where the group is masked (FinishArgs below). */
constexpr int CT_X = 32;
constexpr int CT_Y = 32;

enum { FIN_NONE = 0, FIN_MEAN = FH_FINISH_MEAN, FIN_SUM = FH_FINISH_SUM,
       FIN_COUNT = FH_FINISH_COUNT };

__host__ __device__ constexpr int finish_of(int ops) {
  return ops == (B_SUM | B_CNT)               ? FIN_MEAN
         : ops == (B_SUM | B_CNT | B_PRESENT) ? FIN_SUM
         : ops == B_CNT                       ? FIN_COUNT
                                              : FIN_NONE;
}

struct FinishArgs {
  void* result;
  int rdtype;        /* fh_dtype of result: F32, F64 or I64 */
  int has_fill;
  int64_t min_count; /* masked = count < min_count, or empty when 0 */
  double fill;
};

template <typename T>
__device__ __forceinline__ void store_finished(const FinishArgs& fa, int64_t g,
                                               T val, bool masked) {
  switch (fa.rdtype) {
    case FH_F32: ((float*)fa.result)[g] = masked ? (float)fa.fill : (float)val; break;
    case FH_F64: ((double*)fa.result)[g] = masked ? fa.fill : (double)val; break;
    default: ((int64_t*)fa.result)[g] = masked ? (int64_t)fa.fill : (int64_t)val; break;
  }
}

template <typename V, int OPS, int FIN>
__launch_bounds__(CT_X * CT_Y) __global__ void k_combine_tree(
    const char* __restrict__ slab, int nblocks, int64_t ngroups, BinLayout lay,
    void* out_sum, int64_t* out_count, uint32_t* out_present, void* out_min,
    void* out_max, uint32_t* out_nanflag, double* out_ssd, FinishArgs fa) {
  using TR = Traits<V>;
  using Acc = typename TR::Acc;
  using SumT = typename std::conditional<
      (OPS & B_SSD) != 0, double,
      typename std::conditional<(OPS & (B_IDXMIN | B_IDXMAX)) != 0, int64_t, Acc>::type>::type;
  using Enc = typename TR::Enc;
  constexpr bool IS_PROD = (OPS & B_PROD) != 0;
  constexpr bool HAS_S = (OPS & (B_SUM | B_SSD | B_PROD | B_IDXMIN | B_IDXMAX)) != 0;
  constexpr bool HAS_MM = (OPS & (B_MIN | B_MAX)) != 0;
  constexpr bool HAS_FLAGS = (OPS & (B_PRESENT | B_NANFLAG)) != 0;
  constexpr bool MOM2 = (OPS & B_MOM2) != 0;
  static_assert(FIN == FIN_NONE || FIN == finish_of(OPS), "finish mode/op set mismatch");
  constexpr int NT = CT_X * CT_Y;

  __shared__ SumT sh_s[HAS_S ? NT : 1];
  __shared__ int64_t sh_c[(OPS & B_CNT) ? NT : 1];
  __shared__ Enc sh_mm[HAS_MM ? NT : 1];
  __shared__ uint32_t sh_f[HAS_FLAGS ? NT : 1]; /* bit 0 present, bit 1 nanflag */
  /* summary set: mm is the min and mx the max; (c, piv + off, m2) is the
   * triple */
  __shared__ Enc sh_mx[MOM2 ? NT : 1];
  __shared__ double sh_piv[MOM2 ? NT : 1];
  __shared__ double sh_off[MOM2 ? NT : 1];
  __shared__ double sh_m2[MOM2 ? NT : 1];

  const int tx = threadIdx.x, ty = threadIdx.y;
  const int t = ty * CT_X + tx;
  const int64_t g = (int64_t)blockIdx.x * CT_X + tx;
  const bool live = g < ngroups;

  SumT s = IS_PROD ? (SumT)1 : (SumT)0;
  if (OPS & B_IDXMIN) s = (SumT)INT64_MAX;
  if (OPS & B_IDXMAX) s = (SumT)(-1);
  int64_t c = 0;
  uint32_t f = 0;
  Enc mm = (OPS & B_MIN) ? (Enc)~(Enc)0 : (Enc)0;
  Enc mx = (Enc)0;
  double piv = 0.0, off = 0.0, m2 = 0.0;
  if (live) {
#pragma unroll 4
    for (int b = ty; b < nblocks; b += CT_Y) {
      const char* blk = slab + (int64_t)b * lay.bytes;
      if constexpr (MOM2) { /* before c takes this block's count */
        chan_merge((double)c, piv, off, m2,
                   (double)((const uint32_t*)(blk + lay.cnt_off))[g],
                   TR::piv_dec(((const Enc*)(blk + lay.pivot_off))[g]),
                   ((const double*)(blk + lay.s1_off))[g],
                   ((const double*)(blk + lay.s2_off))[g]);
        const Enc e = ((const Enc*)(blk + lay.max_off))[g];
        mx = e > mx ? e : mx;
      }
      if (HAS_S) {
        const SumT x = ((const SumT*)(blk + lay.sum_off))[g];
        if (OPS & (B_SUM | B_SSD)) s += x;
        if (IS_PROD) s *= x;
        if (OPS & B_IDXMIN) s = x < s ? x : s;
        if (OPS & B_IDXMAX) s = x > s ? x : s;
      }
      if (OPS & B_CNT) c += (int64_t)((const uint32_t*)(blk + lay.cnt_off))[g];
      if (OPS & B_PRESENT) f |= ((const uint32_t*)(blk + lay.present_off))[g] ? 1u : 0u;
      if (OPS & B_NANFLAG) f |= ((const uint32_t*)(blk + lay.nanflag_off))[g] ? 2u : 0u;
      if (HAS_MM) {
        const Enc e = ((const Enc*)(blk + lay.minmax_off))[g];
        if (OPS & B_MIN) mm = e < mm ? e : mm;
        if ((OPS & B_MAX) && !MOM2) mm = e > mm ? e : mm;
      }
    }
  }
  if constexpr (MOM2) {
    sh_mx[t] = mx;
    sh_piv[t] = piv;
    sh_off[t] = off;
    sh_m2[t] = m2;
  }
  if (HAS_S) sh_s[t] = s;
  if (OPS & B_CNT) sh_c[t] = c;
  if (HAS_MM) sh_mm[t] = mm;
  if (HAS_FLAGS) sh_f[t] = f;
  __syncthreads();
  /* fixed-order fold over y: row y takes row y + h, h = CT_Y/2 .. 1 */
#pragma unroll
  for (int h = CT_Y / 2; h > 0; h >>= 1) {
    if (ty < h) {
      const int o = t + h * CT_X;
      if constexpr (MOM2) { /* before c takes row o's count */
        chan_merge((double)c, piv, off, m2, (double)sh_c[o], sh_piv[o], sh_off[o], sh_m2[o]);
        sh_piv[t] = piv;
        sh_off[t] = off;
        sh_m2[t] = m2;
        const Enc e = sh_mx[o];
        mx = e > mx ? e : mx;
        sh_mx[t] = mx;
      }
      if (HAS_S) {
        const SumT x = sh_s[o];
        if (OPS & (B_SUM | B_SSD)) s += x;
        if (IS_PROD) s *= x;
        if (OPS & B_IDXMIN) s = x < s ? x : s;
        if (OPS & B_IDXMAX) s = x > s ? x : s;
        sh_s[t] = s;
      }
      if (OPS & B_CNT) { c += sh_c[o]; sh_c[t] = c; }
      if (HAS_FLAGS) { f |= sh_f[o]; sh_f[t] = f; }
      if (HAS_MM) {
        const Enc e = sh_mm[o];
        if (OPS & B_MIN) mm = e < mm ? e : mm;
        if ((OPS & B_MAX) && !MOM2) mm = e > mm ? e : mm;
        sh_mm[t] = mm;
      }
    }
    __syncthreads();
  }
  if (ty != 0 || !live) return;

  const uint32_t p = f & 1u, nf = (f >> 1) & 1u;
  const bool present = (OPS & B_PRESENT) ? (p != 0) : (c != 0);
  if constexpr (FIN != FIN_NONE) {
    const bool masked = fa.has_fill && (fa.min_count > 0 ? c < fa.min_count : !present);
    if constexpr (FIN == FIN_MEAN) store_finished(fa, g, (double)s / (double)c, masked);
    if constexpr (FIN == FIN_SUM) store_finished(fa, g, s, masked);
    if constexpr (FIN == FIN_COUNT) store_finished(fa, g, c, masked);
  } else {
    if (HAS_S) ((SumT*)out_sum)[g] = s;
    if (OPS & B_CNT) out_count[g] = c;
    if (OPS & B_PRESENT) out_present[g] = p;
    if (OPS & B_MIN) ((V*)out_min)[g] = present ? TR::dec(mm) : TR::pos_inf();
    if (OPS & B_MAX) ((V*)out_max)[g] = present ? TR::dec(MOM2 ? mx : mm) : (V)-TR::pos_inf();
    if (OPS & B_NANFLAG) out_nanflag[g] = nf;
    if constexpr (MOM2) {
      out_present[g] = (c != 0 || nf != 0) ? 1u : 0u; /* any row seen */
      out_ssd[g] = m2;
    }
  }
}

/* ---- global-atomic path -------------------------------------------------- */
/* bins live in HBM/LLC; min/max bins are ENCODED in out_min/out_max during
 * accumulation (memset-friendly init) and decoded by k_decode afterwards. */
template <typename V, typename L, int OPS>
__launch_bounds__(BLOCK_ATOMIC) __global__ void k_reduce_atomic(
    const V* __restrict__ values, const L* __restrict__ labels,
    const L* __restrict__ labels2, int64_t n, int64_t ngroups, int64_t g0,
    int64_t g1, const double* __restrict__ means,
    const V* __restrict__ target, int64_t row_offset, int skipnan,
    void* out_sum, int64_t* out_count, uint32_t* out_present, void* out_min,
    void* out_max, uint32_t* out_nanflag) {
  using TR = Traits<V>;
  using Acc = typename TR::Acc;
  using Enc = typename TR::Enc;
  constexpr int VEC = TR::VEC;
  constexpr bool IS_PROD = (OPS & B_PROD) != 0;
  const bool twolab = labels2 != nullptr;

  auto process = [&](V v, int64_t l0raw, int64_t l1raw, int64_t row) {
    uint64_t code;
    if (twolab) {
      if ((uint64_t)l0raw >= (uint64_t)g0 || (uint64_t)l1raw >= (uint64_t)g1) return;
      code = (uint64_t)l0raw * (uint64_t)g1 + (uint64_t)l1raw;
    } else {
      if ((uint64_t)l0raw >= (uint64_t)ngroups) return;
      code = (uint64_t)l0raw;
    }
    const bool vnan = TR::isnan_(v);
    if (OPS & B_PRESENT) out_present[code] = 1u;
    if (vnan && skipnan) return;
    if (OPS & B_SUM) acc_add(&((Acc*)out_sum)[code], (Acc)v);
    if (IS_PROD) acc_mul(&((Acc*)out_sum)[code], (Acc)v);
    if (OPS & B_SSD) {
      double d = (double)v - means[code];
      atomicAdd(&((double*)out_sum)[code], d * d);
    }
    if (OPS & (B_IDXMIN | B_IDXMAX)) {
      bool match = true;
      if (target) {
        const V t = target[code];
        match = vnan ? TR::isnan_(t) : (!TR::isnan_(t) && v == t);
      }
      if (match) {
        if (OPS & B_IDXMIN) idx_min((int64_t*)out_sum + code, row + row_offset);
        if (OPS & B_IDXMAX) idx_max((int64_t*)out_sum + code, row + row_offset);
      }
    }
    if (OPS & B_CNT) {
      if (!vnan)
        atomicAdd(reinterpret_cast<unsigned long long*>(&out_count[code]), 1ull);
    }
    if (OPS & (B_MIN | B_MAX)) {
      if (vnan) {
        if (OPS & B_NANFLAG) out_nanflag[code] = 1u;
      } else {
        if (OPS & B_MIN) enc_min(&((Enc*)out_min)[code], TR::enc(v));
        if (OPS & B_MAX) enc_max(&((Enc*)out_max)[code], TR::enc(v));
      }
    }
  };

  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nvec = n / VEC;
  for (int64_t i = gtid; i < nvec; i += stride) {
    Vec<V, VEC> vv = *reinterpret_cast<const Vec<V, VEC>*>(values + i * VEC);
    Vec<L, VEC> lv = *reinterpret_cast<const Vec<L, VEC>*>(labels + i * VEC);
    if (twolab) {
      Vec<L, VEC> lv2 = *reinterpret_cast<const Vec<L, VEC>*>(labels2 + i * VEC);
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        process(vv.v[k], (int64_t)lv.v[k], (int64_t)lv2.v[k], i * VEC + k);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) process(vv.v[k], (int64_t)lv.v[k], 0, i * VEC + k);
    }
  }
  for (int64_t i = nvec * VEC + gtid; i < n; i += stride) {
    process(values[i], (int64_t)labels[i], twolab ? (int64_t)labels2[i] : 0, i);
  }
}


/* ---- column path: grouped reduce over a strided/leading axis ------------- */
/* For array (..., reduced axis) with leading dims — e.g. the hour-of-day
 * climatology (reference asv ERA5 shapes, BASELINE config 4). The label
 * vector lives on the (small) reduced axis only, so the host argsorts it
 * once (the GPU analogue of the reference's _prepare_for_flox sort,
 * aggregate_flox.py:9-23 — but over N_t labels, not N_t*M rows) and the
 * kernel walks rows in GROUP ORDER: each thread owns one column, keeps ONE
 * running accumulator in registers, and writes it out at each (wave-uniform)
 * segment boundary. No atomics, no LDS bins, any ngroups.
 * Element (t, c) is at values[t*ldm + c] (column stride 1 — the natural
 * layout for time-major climate data; a torch permute view, no transpose).
 * Outputs are (ngroups, m) group-major so flush stores coalesce. */
constexpr int COLS_BLOCK = 256;
constexpr int COLS_TTILE = 2048;

/* VC columns per thread (16-B vector loads per G13); blockIdx.y = row chunk.
 * With several row chunks each chunk writes PARTIAL bins (cnt as u32) into
 * its section of the scratch slab, identical in layout to the 1-D path's
 * per-block slab, and k_combine folds the chunks; with one chunk the final
 * bins are written directly (cnt as i64). */
template <typename V, int OPS, int VC, bool SLAB, bool SKIP>
__launch_bounds__(COLS_BLOCK) __global__ void k_reduce_cols(
    const V* __restrict__ values, const int* __restrict__ codes_sorted,
    const int* __restrict__ perm, int64_t n_t, int64_t m, int64_t ldm,
    int64_t ngroups, const double* __restrict__ means, int skipnan,
    int64_t chunk_rows, const int64_t* __restrict__ chunk_offs,
    char* __restrict__ slab, BinLayout lay,
    void* out_sum, int64_t* out_count, uint32_t* out_present, void* out_min,
    void* out_max, uint32_t* out_nanflag, double* out_ssd) {
  using TR = Traits<V>;
  using Acc = typename TR::Acc;
  using SumT = typename std::conditional<
      (OPS & (B_SSD | B_WELFORD)) != 0, double,
      typename std::conditional<(OPS & (B_IDXMIN | B_IDXMAX)) != 0, int64_t, Acc>::type>::type;
  using Enc = typename TR::Enc;
  constexpr bool IS_PROD = (OPS & B_PROD) != 0;
  /* the summary set: acc is the direct sum, and per column the pivoted
   * moments ride along: x0 = the segment's first non-NaN value (cnt == 0
   * until it arrives), s1 = sum(x - x0), s2 = sum((x - x0)^2). A NaN row sets
   * nanflag and nothing else, so SKIP is always true here. */
  constexpr bool MOM2 = (OPS & B_MOM2) != 0;
  static_assert(!MOM2 || (OPS == OPS_SUMMARY && SKIP), "summary set: skipping form only");

  __shared__ int s_code[COLS_TTILE];
  __shared__ int s_perm[COLS_TTILE];

  const int64_t c0 = ((int64_t)blockIdx.x * COLS_BLOCK + threadIdx.x) * VC;
  const bool full = c0 + VC <= m;
  int64_t t_begin, t_end;
  if (chunk_offs) {
    t_begin = chunk_offs[blockIdx.y];
    t_end = chunk_offs[blockIdx.y + 1];
  } else {
    t_begin = (int64_t)blockIdx.y * chunk_rows;
    t_end = (t_begin + chunk_rows < n_t) ? t_begin + chunk_rows : n_t;
  }

  char* my_slab = SLAB ? slab + (int64_t)blockIdx.y * lay.bytes : nullptr;

  constexpr bool IS_WEL = (OPS & B_WELFORD) != 0;
  SumT acc[VC];
  uint32_t cnt[VC];
  Enc mn[VC], mx[VC];
  uint32_t nanflag[VC];
  double mean_g[VC];
  /* shifted-variance state: s1 = sum(x - x0), acc holds s2 = sum((x-x0)^2) */
  double w_s1[VC], w_x0[VC];
  uint32_t w_have[VC];
  double q_x0[MOM2 ? VC : 1], q_s1[MOM2 ? VC : 1], q_s2[MOM2 ? VC : 1];
  int cur_g = -1;

  auto reset = [&]() {
#pragma unroll
    for (int k = 0; k < VC; ++k) {
      acc[k] = IS_PROD ? (SumT)1 : (SumT)0;
      cnt[k] = 0;
      mn[k] = (Enc)~(Enc)0;
      mx[k] = (Enc)0;
      nanflag[k] = 0;
      if (IS_WEL) {
        w_s1[k] = 0.0;
        w_x0[k] = 0.0;
        w_have[k] = 0;
      }
      if constexpr (MOM2) {
        q_x0[k] = 0.0;
        q_s1[k] = 0.0;
        q_s2[k] = 0.0;
      }
    }
  };
  reset();

  auto flush = [&](int g) {
    if (g < 0) return;
#pragma unroll
    for (int k = 0; k < VC; ++k) {
      if (c0 + k >= m) break;
      const int64_t o = (int64_t)g * m + c0 + k;
      if constexpr (MOM2) {
        /* M2 about the segment mean; the slab keeps the mean in its two
         * parts, x0 and s1/n, so that the merge subtracts pivots exactly */
        double off = 0.0, m2 = 0.0;
        if (cnt[k]) {
          const double dn = (double)cnt[k];
          off = q_s1[k] / dn;
          m2 = q_s2[k] - q_s1[k] * q_s1[k] / dn;
          if (m2 < 0.0) m2 = 0.0; /* rounding only: M2 >= 0 by Cauchy-Schwarz */
        }
        if (SLAB) {
          ((Acc*)(my_slab + lay.sum_off))[o] = acc[k];
          ((uint32_t*)(my_slab + lay.cnt_off))[o] = cnt[k];
          ((Enc*)(my_slab + lay.minmax_off))[o] = mn[k];
          ((Enc*)(my_slab + lay.max_off))[o] = mx[k];
          ((uint32_t*)(my_slab + lay.nanflag_off))[o] = nanflag[k];
          ((Enc*)(my_slab + lay.pivot_off))[o] = cols_piv_pack<V>(q_x0[k]);
          ((double*)(my_slab + lay.s1_off))[o] = off;
          ((double*)(my_slab + lay.s2_off))[o] = m2;
        } else {
          ((Acc*)out_sum)[o] = acc[k];
          out_count[o] = (int64_t)cnt[k];
          ((Enc*)out_min)[o] = mn[k]; /* decoded by k_decode */
          ((Enc*)out_max)[o] = mx[k];
          out_nanflag[o] = nanflag[k];
          out_present[o] = (cnt[k] != 0 || nanflag[k] != 0) ? 1u : 0u;
          out_ssd[o] = m2;
        }
        continue;
      }
      if (IS_WEL) {
        /* convert shifted sums to the var_chunk triple: sum = s1 + n*x0,
         * ssd = s2 - s1^2/n (the mean-shifted form) */
        const double nn = (double)cnt[k];
        const double sum = w_s1[k] + nn * w_x0[k];
        const double ssd = cnt[k] ? (double)acc[k] - (w_s1[k] * w_s1[k]) / nn : 0.0;
        if (SLAB) {
          ((double*)(my_slab + lay.sum_off))[o] = ssd;
          ((double*)(my_slab + lay.sumx_off))[o] = sum;
          ((uint32_t*)(my_slab + lay.cnt_off))[o] = cnt[k];
        } else {
          ((double*)out_sum)[o] = ssd;
          ((double*)out_min)[o] = sum; /* sum-of-x rides the out_min slot */
          out_count[o] = (int64_t)cnt[k];
        }
        continue;
      }
      if (SLAB) {
        if (OPS & (B_SUM | B_SSD | B_PROD)) ((SumT*)(my_slab + lay.sum_off))[o] = acc[k];
        if (OPS & B_CNT) ((uint32_t*)(my_slab + lay.cnt_off))[o] = cnt[k];
        if (OPS & B_PRESENT) ((uint32_t*)(my_slab + lay.present_off))[o] = 1u;
        if (OPS & B_MIN) ((Enc*)(my_slab + lay.minmax_off))[o] = mn[k];
        if (OPS & B_MAX) ((Enc*)(my_slab + lay.minmax_off))[o] = mx[k];
        if (OPS & B_NANFLAG) ((uint32_t*)(my_slab + lay.nanflag_off))[o] = nanflag[k];
      } else {
        if (OPS & (B_SUM | B_SSD | B_PROD)) ((SumT*)out_sum)[o] = acc[k];
        if (OPS & B_CNT) out_count[o] = (int64_t)cnt[k];
        if (OPS & B_PRESENT) out_present[o] = 1u;
        if (OPS & B_MIN) ((Enc*)out_min)[o] = mn[k];
        if (OPS & B_MAX) ((Enc*)out_max)[o] = mx[k];
        if (OPS & B_NANFLAG) out_nanflag[o] = nanflag[k];
      }
    }
  };

  auto consume = [&](V v, int k, bool lanes_ok) {
    if (!lanes_ok) return;
    /* SKIP is compile-time (skipnan-templated variants): the skip branch
     * and the count select drop out of the per-element stream */
    const bool vnan = TR::isnan_(v);
    if constexpr (MOM2) {
      if (vnan) {
        nanflag[k] = 1u;
        return;
      }
      const double x = (double)v;
      if (cnt[k] == 0) q_x0[k] = x;
      const double d = x - q_x0[k];
      q_s1[k] += d;
      q_s2[k] += d * d;
      acc[k] += (Acc)v;
      cnt[k] += 1u;
      const Enc e = TR::enc(v);
      mn[k] = e < mn[k] ? e : mn[k];
      mx[k] = e > mx[k] ? e : mx[k];
      return;
    }
    if constexpr (SKIP) {
      if (vnan) return;
    }
    if (IS_WEL) {
      if (!w_have[k]) {
        w_x0[k] = (double)v; /* non-skip: a NaN first value poisons the group */
        w_have[k] = 1;
      }
      const double d = (double)v - w_x0[k];
      w_s1[k] += d;
      acc[k] += (SumT)(d * d);
      if constexpr (SKIP) cnt[k] += 1u; else cnt[k] += vnan ? 0u : 1u;
      return;
    }
    if (OPS & B_SUM) acc[k] += (SumT)v;
    if (IS_PROD) acc[k] *= (SumT)v;
    if (OPS & B_SSD) {
      const double d = (double)v - mean_g[k];
      acc[k] += d * d;
    }
    if (OPS & B_CNT) {
      if constexpr (SKIP) cnt[k] += 1u; else cnt[k] += vnan ? 0u : 1u;
    }
    if (OPS & (B_MIN | B_MAX)) {
      if (vnan) {
        if (OPS & B_NANFLAG) nanflag[k] = 1u;
      } else {
        const Enc e = TR::enc(v);
        if (OPS & B_MIN) mn[k] = e < mn[k] ? e : mn[k];
        if (OPS & B_MAX) mx[k] = e > mx[k] ? e : mx[k];
      }
    }
  };

  for (int64_t t0 = t_begin; t0 < t_end; t0 += COLS_TTILE) {
    const int nt = (int)((t_end - t0 < COLS_TTILE) ? (t_end - t0) : COLS_TTILE);
    __syncthreads();
    for (int i = threadIdx.x; i < nt; i += COLS_BLOCK) {
      s_code[i] = codes_sorted[t0 + i];
      s_perm[i] = perm[t0 + i];
    }
    __syncthreads();
    const bool col_act = c0 < m;
    int i = 0;
    while (i < nt) {
      const int g = s_code[i];
      if (g != cur_g) {
        flush(cur_g);
        reset();
        cur_g = g;
        if ((OPS & B_SSD) && g >= 0 && col_act) {
#pragma unroll
          for (int k = 0; k < VC; ++k)
            if (c0 + k < m) mean_g[k] = means[(int64_t)g * m + c0 + k];
        }
      }
      if (g < 0 || !col_act) {
        ++i;
        continue;
      }
      /* two rows of the same segment per iteration: halves the LDS reads,
       * compares and loop control per element (segment boundaries are rare
       * relative to rows) */
      if (VC > 1 && full) {
        if (i + 1 < nt && s_code[i + 1] == g) {
          const int64_t rowa = (int64_t)s_perm[i] * ldm;
          const int64_t rowb = (int64_t)s_perm[i + 1] * ldm;
          Vec<V, VC> va = *reinterpret_cast<const Vec<V, VC>*>(values + rowa + c0);
          Vec<V, VC> vb = *reinterpret_cast<const Vec<V, VC>*>(values + rowb + c0);
#pragma unroll
          for (int k = 0; k < VC; ++k) consume(va.v[k], k, true);
#pragma unroll
          for (int k = 0; k < VC; ++k) consume(vb.v[k], k, true);
          i += 2;
          continue;
        }
        Vec<V, VC> vv = *reinterpret_cast<const Vec<V, VC>*>(values + (int64_t)s_perm[i] * ldm + c0);
#pragma unroll
        for (int k = 0; k < VC; ++k) consume(vv.v[k], k, true);
        ++i;
      } else {
        const int64_t row = (int64_t)s_perm[i] * ldm;
#pragma unroll
        for (int k = 0; k < VC; ++k)
          consume((c0 + k < m) ? values[row + c0 + k] : (V)0, k, c0 + k < m);
        ++i;
      }
    }
  }
  flush(cur_g);
}

/* identities of a running max / min over V: no value is below / above them */
template <typename V>
__host__ __device__ constexpr V cols_lowest() {
  return std::numeric_limits<V>::has_infinity ? -std::numeric_limits<V>::infinity()
                                              : std::numeric_limits<V>::lowest();
}
template <typename V>
__host__ __device__ constexpr V cols_highest() {
  return std::numeric_limits<V>::has_infinity ? std::numeric_limits<V>::infinity()
                                              : std::numeric_limits<V>::max();
}

/* ---- column path, order-dependent sets ------------------------------------
 * k_reduce_cols' walk (rows in group order, staged code/perm tiles, VC columns
 * per thread, the three flush modes) for the sets whose state is a ROW:
 *   B_IDXMIN / B_IDXMAX  the smallest / largest original row perm[i] of the
 *                        segment (non-NaN rows only when SKIP): first / last;
 *   B_ARGMINC / B_ARGMAXC  the running extremum bv, its row brow and the
 *                        first NaN row nrow, one pass: arg-reductions.
 * Rows are kept as int32 (n_t < 2^31) and widened, + row_offset, at the
 * flush; NONE (INT32_MAX, or -1 for IDXMAX) becomes the 1-D sentinel. The
 * extremum starts at its identity with row NONE, so "better, or equal and an
 * earlier row" also admits the first candidate; the row compare makes ties go
 * to the smallest row under any perm that sorts the codes, and == makes
 * -0.0 tie +0.0. Address arithmetic is row * ldm + c0 in 64 bits. */
template <typename V, int OPS, int VC, bool SLAB, bool SKIP>
__launch_bounds__(COLS_BLOCK) __global__ void k_order_cols(
    const V* __restrict__ values, const int* __restrict__ codes_sorted,
    const int* __restrict__ perm, int64_t n_t, int64_t m, int64_t ldm,
    int64_t row_offset, int64_t chunk_rows,
    const int64_t* __restrict__ chunk_offs, char* __restrict__ slab,
    BinLayout lay, int64_t* out_idx, int64_t* out_count, uint32_t* out_present,
    uint32_t* out_nanflag) {
  using TR = Traits<V>;
  constexpr bool ARG = (OPS & B_ARGC) != 0;
  constexpr bool ISMAX = (OPS & (B_ARGMAXC | B_IDXMAX)) != 0;
  static_assert((OPS & B_ORDERC) != 0 && (OPS & B_CNT) && (OPS & B_PRESENT),
                "row-valued sets only");
  /* "no row": IDXMAX folds with max, everything else with min */
  constexpr int NONE = (OPS & B_IDXMAX) ? -1 : INT32_MAX;
  constexpr V START = ISMAX ? cols_lowest<V>() : cols_highest<V>();

  __shared__ int s_code[COLS_TTILE];
  __shared__ int s_perm[COLS_TTILE];

  const int64_t c0 = ((int64_t)blockIdx.x * COLS_BLOCK + threadIdx.x) * VC;
  const bool full = c0 + VC <= m;
  int64_t t_begin, t_end;
  if (chunk_offs) {
    t_begin = chunk_offs[blockIdx.y];
    t_end = chunk_offs[blockIdx.y + 1];
  } else {
    t_begin = (int64_t)blockIdx.y * chunk_rows;
    t_end = (t_begin + chunk_rows < n_t) ? t_begin + chunk_rows : n_t;
  }
  char* my_slab = SLAB ? slab + (int64_t)blockIdx.y * lay.bytes : nullptr;

  int brow[VC];
  uint32_t cnt[VC];
  V bv[ARG ? VC : 1];
  int nrow[ARG ? VC : 1];
  int cur_g = -1;

  auto reset = [&]() {
#pragma unroll
    for (int k = 0; k < VC; ++k) {
      brow[k] = NONE;
      cnt[k] = 0;
      if constexpr (ARG) {
        bv[k] = START;
        nrow[k] = INT32_MAX;
      }
    }
  };
  reset();

  auto widen = [&](int r) -> int64_t {
    if (r == NONE) return (OPS & B_IDXMAX) ? (int64_t)-1 : INT64_MAX;
    return (int64_t)r + row_offset;
  };

  auto flush = [&](int g) {
    if (g < 0) return;
#pragma unroll
    for (int k = 0; k < VC; ++k) {
      if (c0 + k >= m) break;
      const int64_t o = (int64_t)g * m + c0 + k;
      if (SLAB) {
        ((int64_t*)(my_slab + lay.sum_off))[o] = widen(brow[k]);
        ((uint32_t*)(my_slab + lay.cnt_off))[o] = cnt[k];
        ((uint32_t*)(my_slab + lay.present_off))[o] = 1u;
        if constexpr (ARG) {
          ((V*)(my_slab + lay.argval_off))[o] = bv[k];
          ((int64_t*)(my_slab + lay.nanrow_off))[o] =
              (SKIP || nrow[k] == INT32_MAX) ? INT64_MAX : (int64_t)nrow[k] + row_offset;
          ((uint32_t*)(my_slab + lay.nanflag_off))[o] = nrow[k] != INT32_MAX ? 1u : 0u;
        }
      } else {
        int r = brow[k];
        if constexpr (ARG) {
          if (!SKIP && nrow[k] != INT32_MAX) r = nrow[k]; /* the first NaN wins */
          out_nanflag[o] = nrow[k] != INT32_MAX ? 1u : 0u;
        }
        out_idx[o] = widen(r);
        out_count[o] = (int64_t)cnt[k];
        out_present[o] = 1u;
      }
    }
  };

  auto consume = [&](V v, int k, int row) {
    const bool vnan = TR::isnan_(v);
    if constexpr (ARG) {
      if (vnan) {
        nrow[k] = row < nrow[k] ? row : nrow[k];
        return;
      }
      cnt[k] += 1u;
      const bool better = ISMAX ? v > bv[k] : v < bv[k];
      const bool take = better || (v == bv[k] && row < brow[k]);
      bv[k] = take ? v : bv[k];
      brow[k] = take ? row : brow[k];
    } else {
      if constexpr (SKIP) {
        if (vnan) return;
      }
      cnt[k] += vnan ? 0u : 1u;
      if (OPS & B_IDXMIN) brow[k] = row < brow[k] ? row : brow[k];
      if (OPS & B_IDXMAX) brow[k] = row > brow[k] ? row : brow[k];
    }
  };

  for (int64_t t0 = t_begin; t0 < t_end; t0 += COLS_TTILE) {
    const int nt = (int)((t_end - t0 < COLS_TTILE) ? (t_end - t0) : COLS_TTILE);
    __syncthreads();
    for (int i = threadIdx.x; i < nt; i += COLS_BLOCK) {
      s_code[i] = codes_sorted[t0 + i];
      s_perm[i] = perm[t0 + i];
    }
    __syncthreads();
    const bool col_act = c0 < m;
    int i = 0;
    while (i < nt) {
      const int g = s_code[i];
      if (g != cur_g) {
        flush(cur_g);
        reset();
        cur_g = g;
      }
      if (g < 0 || !col_act) {
        ++i;
        continue;
      }
      const int pa = s_perm[i];
      if (VC > 1 && full) {
        /* two rows of the same segment per iteration, as k_reduce_cols */
        if (i + 1 < nt && s_code[i + 1] == g) {
          const int pb = s_perm[i + 1];
          Vec<V, VC> va = *reinterpret_cast<const Vec<V, VC>*>(values + (int64_t)pa * ldm + c0);
          Vec<V, VC> vb = *reinterpret_cast<const Vec<V, VC>*>(values + (int64_t)pb * ldm + c0);
#pragma unroll
          for (int k = 0; k < VC; ++k) consume(va.v[k], k, pa);
#pragma unroll
          for (int k = 0; k < VC; ++k) consume(vb.v[k], k, pb);
          i += 2;
          continue;
        }
        Vec<V, VC> vv = *reinterpret_cast<const Vec<V, VC>*>(values + (int64_t)pa * ldm + c0);
#pragma unroll
        for (int k = 0; k < VC; ++k) consume(vv.v[k], k, pa);
        ++i;
      } else {
        const int64_t row = (int64_t)pa * ldm;
#pragma unroll
        for (int k = 0; k < VC; ++k)
          if (c0 + k < m) consume(values[row + c0 + k], k, pa);
        ++i;
      }
    }
  }
  flush(cur_g);
}

__global__ void k_init_cursors(uint32_t* cur, int n, uint32_t cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) cur[i] = (uint32_t)i * cap;
}

/* init product bins to 1 (memset cannot) */
__global__ void k_fill_f64(double* p, int64_t n, double v) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
__global__ void k_fill_i64(int64_t* p, int64_t n, int64_t v) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

/* decode min/max bins in place (global-atomic path) */
template <typename V, int OPS>
__global__ void k_decode(int64_t ngroups, void* out_min, void* out_max,
                         const int64_t* out_count, const uint32_t* out_present) {
  using TR = Traits<V>;
  using Enc = typename TR::Enc;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngroups) return;
  const bool present =
      (OPS & B_PRESENT) ? (out_present[g] != 0) : (out_count && out_count[g] != 0);
  if (OPS & B_MIN) {
    Enc e = ((Enc*)out_min)[g];
    ((V*)out_min)[g] = present ? TR::dec(e) : TR::pos_inf();
  }
  if (OPS & B_MAX) {
    Enc e = ((Enc*)out_max)[g];
    ((V*)out_max)[g] = present ? TR::dec(e) : (V)-TR::pos_inf();
  }
}


/* ---- partition path (huge ngroups, e.g. 1e7): bucket scatter + per-bucket
 * LDS reduce — the GPU analogue of the reference's sort-by-key + reduceat
 * engine (aggregate_flox.py:9-23 _prepare_for_flox + :133-192
 * _np_grouped_op), except only ONE radix digit is needed: rows are
 * partitioned by the high bits of their group code into buckets whose bins
 * fit in LDS, then each bucket is reduced like the LDS path. Traffic:
 * labels (count) + values+labels (scatter read) + pairs (write+read) ~=
 * 3.7x the algorithmic bytes, vs ~45x slower raw global atomics. */

template <typename V> struct PairT;
template <> struct PairT<float> { float v; uint32_t lc; };
template <> struct PairT<int32_t> { int32_t v; uint32_t lc; };
template <> struct PairT<double> { double v; uint32_t lc; uint32_t pad; };
template <> struct PairT<int64_t> { int64_t v; uint32_t lc; uint32_t pad; };

__device__ __forceinline__ int64_t code_of(int64_t l0, int64_t l1, bool twolab,
                                           int64_t g0, int64_t g1, int64_t ngroups) {
  if (twolab) {
    if ((uint64_t)l0 >= (uint64_t)g0 || (uint64_t)l1 >= (uint64_t)g1) return -1;
    return l0 * g1 + l1;
  }
  return ((uint64_t)l0 >= (uint64_t)ngroups) ? -1 : l0;
}

template <typename L>
__launch_bounds__(256) __global__ void k_part_count(
    const L* __restrict__ labels, const L* __restrict__ labels2, int64_t n,
    int64_t ngroups, int64_t g0, int64_t g1, int shift, int B,
    uint32_t* __restrict__ bucket_counts) {
  extern __shared__ __attribute__((aligned(16))) char smem_pc[];
  uint32_t* s_hist = (uint32_t*)smem_pc;
  for (int i = threadIdx.x; i < B; i += blockDim.x) s_hist[i] = 0;
  __syncthreads();
  const bool twolab = labels2 != nullptr;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int64_t code = code_of((int64_t)labels[i], twolab ? (int64_t)labels2[i] : 0,
                           twolab, g0, g1, ngroups);
    if (code >= 0) atomicAdd(&s_hist[(int)(code >> shift)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < B; i += blockDim.x)
    if (s_hist[i]) atomicAdd(&bucket_counts[i], s_hist[i]);
}

/* tile-staged scatter: per tile, histogram -> tiny scan -> global
 * reservation (one returning atomic per nonempty bucket) -> bucket-ordered
 * staging in LDS with per-slot destinations -> coalesced dump.
 * With the two-level scheme this pass NEVER sees more than PART_SUB=64
 * buckets (pass A uses the <= 64 super-buckets; single-level runs only when
 * the fine bucket count is <= 64), so the histogram/scan state is tiny and
 * three blocks fit per CU. */
constexpr int PART_BLOCK = 512;

/* per-wave-histogram tile scatter machinery, shared by both scatter passes:
 * each of the NW waves owns its own 64-entry histogram slice (layout
 * [bucket][wave]) so LDS atomic contention is divided by NW, the exclusive
 * scan over the 512 (bucket, wave) slots runs as wave shuffle scans plus
 * one tiny cross-wave combine (2 barriers instead of 18), and the scanned
 * slots double as the staging cursors. */
constexpr int PART_NW = PART_BLOCK / 64;

/* staging tile of both scatter passes, in pairs: ~76 KB of LDS, 2 blocks/CU */
template <typename V>
constexpr int PART_TILE = sizeof(V) == 4 ? 6144 : 3072;

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up((int)v, d);
    if ((threadIdx.x & 63) >= d) v += o;
  }
  return v;
}

template <typename V, typename L, bool CROW = false, int T = PART_TILE<V>>
__launch_bounds__(PART_BLOCK) __global__ void k_part_scatter(
    const V* __restrict__ values, const L* __restrict__ labels,
    const L* __restrict__ labels2, int64_t n, int64_t ngroups, int64_t g0,
    int64_t g1, int shift, int B, int Bpad /* unused, <= 64 buckets */,
    uint32_t* __restrict__ cursors, uint32_t cap /* 0 = exact bases */,
    uint32_t* __restrict__ overflow, PairT<V>* __restrict__ pairs,
    int64_t row_base = 0 /* CROW: global row = row_base + i in .pad */) {
  constexpr int RPT = T / PART_BLOCK;
  constexpr int NB = 64;
  constexpr int NE = NB * PART_NW; /* = PART_BLOCK slots */
  extern __shared__ __attribute__((aligned(16))) char smem_ps[];
  uint32_t* s_slot = (uint32_t*)smem_ps;              /* [NE] hist -> excl -> cursor */
  uint32_t* s_wtot = s_slot + NE;                     /* [PART_NW + 1] wave totals */
  uint32_t* s_gbase = s_wtot + PART_NW + 1;           /* [NB] gbase - bucket excl */
  uint32_t* s_dest = s_gbase + NB + 3;                /* [T]; pads stage to 16 B */
  PairT<V>* s_stage = (PairT<V>*)(s_dest + T);        /* [T] */

  const bool twolab = labels2 != nullptr;
  const int tid = threadIdx.x;
  const int wid = tid >> 6;

  for (int64_t tile = (int64_t)blockIdx.x * T; tile < n; tile += (int64_t)gridDim.x * T) {
    const int nt = (int)((n - tile < T) ? (n - tile) : T);
    s_slot[tid] = 0;
    __syncthreads();

    V rv[RPT];
    uint32_t rlc[RPT];
    int rbk[RPT];
    /* per-thread CONTIGUOUS rows -> 16-B vector loads (G13) */
    const int base = tid * RPT;
    if (base + RPT <= nt) {
      constexpr int VW = 16 / (int)sizeof(V);
#pragma unroll
      for (int k = 0; k < RPT; k += VW) {
        const Vec<V, VW> vv =
            *reinterpret_cast<const Vec<V, VW>*>(values + tile + base + k);
#pragma unroll
        for (int j = 0; j < VW; ++j) rv[k + j] = vv.v[j];
      }
      Vec<L, 2> lv[RPT / 2 > 0 ? RPT / 2 : 1];
      if (sizeof(L) == 8) {
#pragma unroll
        for (int k = 0; k < RPT; k += 2)
          lv[k / 2] = *reinterpret_cast<const Vec<L, 2>*>(labels + tile + base + k);
      }
#pragma unroll
      for (int k = 0; k < RPT; ++k) {
        const int64_t i = tile + base + k;
        const int64_t l0 = sizeof(L) == 8 ? (int64_t)lv[k / 2].v[k & 1] : (int64_t)labels[i];
        const int64_t code = code_of(l0, twolab ? (int64_t)labels2[i] : 0, twolab,
                                     g0, g1, ngroups);
        rbk[k] = -1;
        if (code >= 0) {
          rbk[k] = (int)(code >> shift);
          rlc[k] = (uint32_t)(code - ((int64_t)rbk[k] << shift));
          atomicAdd(&s_slot[wid * NB + rbk[k]], 1u);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < RPT; ++k) {
        const int idx = base + k;
        rbk[k] = -1;
        if (idx < nt) {
          const int64_t i = tile + idx;
          const int64_t code = code_of((int64_t)labels[i],
                                       twolab ? (int64_t)labels2[i] : 0, twolab,
                                       g0, g1, ngroups);
          if (code >= 0) {
            rv[k] = values[i];
            rbk[k] = (int)(code >> shift);
            rlc[k] = (uint32_t)(code - ((int64_t)rbk[k] << shift));
            atomicAdd(&s_slot[wid * NB + rbk[k]], 1u);
          }
        }
      }
    }
    __syncthreads();
    /* exclusive scan over the NE slots: wave shuffle scans + wave totals */
    {
      /* s_slot layout is [wave][bucket] (addr = w*NB + b): the per-row
       * histogram/cursor atomics touch all 32 LDS banks (the previous
       * [bucket][wave] stride-NW layout mapped random buckets onto only 4
       * banks). Measured NEUTRAL on the 1e9/1e7 sum (10.60 vs 10.62 ms) —
       * the wave parking is memory-latency-bound, not LDS-bound — kept for
       * the clean banking. The scan is still over the semantic
       * (bucket, wave) order = tid; only this once-per-tile gather reads
       * transposed. */
      const int tb = tid / PART_NW, tw = tid % PART_NW;
      const uint32_t mine = s_slot[tw * NB + tb];
      const uint32_t incl = wave_incl_scan(mine);
      if ((tid & 63) == 63) s_wtot[wid] = incl;
      __syncthreads();
      if (tid == 0) {
        uint32_t run = 0;
        for (int w = 0; w < PART_NW; ++w) {
          const uint32_t x = s_wtot[w];
          s_wtot[w] = run;
          run += x;
        }
        s_wtot[PART_NW] = run;
      }
      __syncthreads();
      s_slot[tw * NB + tb] = incl - mine + s_wtot[wid];
    }
    __syncthreads();
    const uint32_t total = s_wtot[PART_NW];
    for (int b = tid; b < B; b += PART_BLOCK) {
      const uint32_t excl = s_slot[b]; /* (b, w=0) in [w][b] layout */
      const uint32_t nxt = (b + 1 < NB) ? s_slot[b + 1] : total;
      const uint32_t cnt = nxt - excl;
      if (cnt) {
        uint32_t gb = atomicAdd(&cursors[b], cnt);
        if (cap && gb + cnt > (uint32_t)(b + 1) * cap) {
          /* optimistic region overflow: flag it and keep writes in-bounds
           * (results are discarded and recomputed by the exact path) */
          *overflow = 1u;
          gb = (uint32_t)b * cap;
        }
        s_gbase[b] = gb - excl;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      if (rbk[k] >= 0) {
        const uint32_t pos = atomicAdd(&s_slot[wid * NB + rbk[k]], 1u);
        s_stage[pos].v = rv[k];
        s_stage[pos].lc = rlc[k];
        if constexpr (CROW && sizeof(PairT<V>) == 16)
          s_stage[pos].pad = (uint32_t)(tile + base + k + row_base);
        s_dest[pos] = s_gbase[rbk[k]] + pos;
      }
    }
    __syncthreads();
    for (int i = tid; i < (int)total; i += PART_BLOCK) pairs[s_dest[i]] = s_stage[i];
    __syncthreads();
  }
}

/* second-level scatter: rows of one super-bucket (already contiguous in
 * `in`) are partitioned into their <= 64 fine buckets. Same tile machinery
 * as k_part_scatter, with a fixed 64-entry histogram. */
constexpr int PART_SUB = 64;

template <typename V, bool CROW = false, int T = PART_TILE<V>>
__launch_bounds__(PART_BLOCK) __global__ void k_part_scatter2(
    const PairT<V>* __restrict__ in, const uint32_t* __restrict__ baseA,
    uint32_t capA /* 0: baseA[sb]..baseA[sb+1]; else sb*capA..baseA[sb] */,
    int shift /* fine-bucket shift */, int bfine /* total fine buckets */,
    uint32_t* __restrict__ cursors,
    uint32_t cap2 /* 0 = exact fine bases */, uint32_t* __restrict__ overflow,
    PairT<V>* __restrict__ out) {
  constexpr int RPT = T / PART_BLOCK;
  constexpr int NB = PART_SUB;
  constexpr int NE = NB * PART_NW;
  extern __shared__ __attribute__((aligned(16))) char smem_p2[];
  uint32_t* s_slot = (uint32_t*)smem_p2;
  uint32_t* s_wtot = s_slot + NE;
  uint32_t* s_gbase = s_wtot + PART_NW + 1;
  uint32_t* s_dest = s_gbase + NB + 3;
  PairT<V>* s_stage = (PairT<V>*)(s_dest + T);

  const int sb = blockIdx.y;
  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int64_t r0 = capA ? (int64_t)(uint32_t)sb * capA : (int64_t)baseA[sb];
  int64_t r1 = capA ? (int64_t)baseA[sb] : (int64_t)baseA[sb + 1];
  /* pass-A overflow leaves its cursor beyond the capacity region; clamp so
   * we never read the neighbouring region's (or uninitialized) pairs — the
   * results are discarded and recomputed by the exact path anyway */
  if (capA && r1 > r0 + (int64_t)capA) r1 = r0 + (int64_t)capA;
  const uint32_t lmask = (1u << shift) - 1u;

  for (int64_t tile = r0 + (int64_t)blockIdx.x * T; tile < r1;
       tile += (int64_t)gridDim.x * T) {
    const int nt = (int)((r1 - tile < T) ? (r1 - tile) : T);
    s_slot[tid] = 0;
    __syncthreads();
    V rv[RPT];
    uint32_t rlc[RPT];
    uint32_t rpd[CROW ? RPT : 1];
    int rbk[RPT];
    const int base = tid * RPT;
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const int idx = base + k;
      rbk[k] = -1;
      if (idx < nt) {
        const PairT<V> pr = in[tile + idx];
        rv[k] = pr.v;
        if constexpr (CROW && sizeof(PairT<V>) == 16) rpd[k] = pr.pad;
        /* mask: stale pairs after a pass-A overflow can carry garbage lc */
        rbk[k] = (int)((pr.lc >> shift) & (PART_SUB - 1));
        rlc[k] = pr.lc & lmask;
        atomicAdd(&s_slot[wid * NB + rbk[k]], 1u);
      }
    }
    __syncthreads();
    {
      /* s_slot layout is [wave][bucket] (addr = w*NB + b): the per-row
       * histogram/cursor atomics touch all 32 LDS banks (the previous
       * [bucket][wave] stride-NW layout mapped random buckets onto only 4
       * banks). Measured NEUTRAL on the 1e9/1e7 sum (10.60 vs 10.62 ms) —
       * the wave parking is memory-latency-bound, not LDS-bound — kept for
       * the clean banking. The scan is still over the semantic
       * (bucket, wave) order = tid; only this once-per-tile gather reads
       * transposed. */
      const int tb = tid / PART_NW, tw = tid % PART_NW;
      const uint32_t mine = s_slot[tw * NB + tb];
      const uint32_t incl = wave_incl_scan(mine);
      if ((tid & 63) == 63) s_wtot[wid] = incl;
      __syncthreads();
      if (tid == 0) {
        uint32_t run = 0;
        for (int w = 0; w < PART_NW; ++w) {
          const uint32_t x = s_wtot[w];
          s_wtot[w] = run;
          run += x;
        }
        s_wtot[PART_NW] = run;
      }
      __syncthreads();
      s_slot[tw * NB + tb] = incl - mine + s_wtot[wid];
    }
    __syncthreads();
    const uint32_t total = s_wtot[PART_NW];
    for (int b = tid; b < NB; b += PART_BLOCK) {
      const uint32_t excl = s_slot[b]; /* (b, w=0) in [w][b] layout */
      const uint32_t nxt = (b + 1 < NB) ? s_slot[b + 1] : total;
      const uint32_t cnt = nxt - excl;
      if (cnt) {
        const uint32_t fb = (uint32_t)sb * PART_SUB + (uint32_t)b;
        if (fb >= (uint32_t)bfine) {
          /* only reachable via pass-A overflow garbage: flag, park the
           * rows at the buffer start (results are discarded) */
          *overflow = 1u;
          s_gbase[b] = 0u - excl;
        } else {
          uint32_t gb = atomicAdd(&cursors[fb], cnt);
          if (cap2 && gb + cnt > (fb + 1u) * cap2) {
            *overflow = 1u;
            gb = fb * cap2;
          }
          s_gbase[b] = gb - excl;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      if (rbk[k] >= 0) {
        const uint32_t pos = atomicAdd(&s_slot[wid * NB + rbk[k]], 1u);
        s_stage[pos].v = rv[k];
        s_stage[pos].lc = rlc[k];
        if constexpr (CROW && sizeof(PairT<V>) == 16) s_stage[pos].pad = rpd[k];
        s_dest[pos] = s_gbase[rbk[k]] + pos;
      }
    }
    __syncthreads();
    for (int i = tid; i < (int)total; i += PART_BLOCK) out[s_dest[i]] = s_stage[i];
    __syncthreads();
  }
}

/* sorted-labels direct path: bucket b's rows are the contiguous range
 * [base[b], base[b+1]) of the ORIGINAL arrays (no scatter passes at all —
 * 12 B/row instead of the partition's ~44 B/row). base comes from
 * k_bucket_bounds; the FH_SORTED_LABELS contract guarantees nondecreasing
 * in-range labels. */
template <typename L>
__global__ void k_bucket_bounds(const L* __restrict__ labels, int64_t n,
                                int nb, int shift,
                                uint32_t* __restrict__ base) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > nb) return;
  if (b == nb) {
    base[nb] = (uint32_t)n;
    return;
  }
  const int64_t target = (int64_t)b << shift;
  int64_t lo = 0, hi = n; /* lower_bound */
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)labels[mid] < target) lo = mid + 1; else hi = mid;
  }
  base[b] = (uint32_t)lo;
}

template <typename V, typename L, int OPS>
__launch_bounds__(BLOCK_LDS) __global__ void k_reduce_bucket_direct(
    const V* __restrict__ values, const L* __restrict__ labels,
    const uint32_t* __restrict__ base, int64_t chunk, int gpb, int shift,
    int64_t ngroups, const double* __restrict__ means, int skipnan,
    BinLayout lay, void* out_sum, int64_t* out_count, uint32_t* out_present,
    void* out_min, void* out_max, uint32_t* out_nanflag) {
  using TR = Traits<V>;
  using Acc = typename TR::Acc;
  using SumT = typename std::conditional<
      (OPS & (B_SSD | B_WELFORD)) != 0, double,
      typename std::conditional<(OPS & (B_IDXMIN | B_IDXMAX)) != 0, int64_t, Acc>::type>::type;
  using Enc = typename TR::Enc;
  constexpr bool IS_PROD = (OPS & B_PROD) != 0;

  const int b = blockIdx.y;
  const int64_t bkt_begin = base[b];
  const int64_t bkt_end = base[b + 1];
  if (bkt_begin >= bkt_end) return;
  const int64_t gbase = (int64_t)b << shift;
  const int ng_here = (int)(((gbase + gpb) <= ngroups) ? gpb : (ngroups - gbase));

  extern __shared__ __attribute__((aligned(16))) char smem_rd[];
  SumT* s_sum = (OPS & (B_SUM | B_SSD | B_PROD | B_IDXMIN | B_IDXMAX))
                    ? (SumT*)(smem_rd + lay.sum_off) : nullptr;
  uint32_t* s_cnt = (OPS & B_CNT) ? (uint32_t*)(smem_rd + lay.cnt_off) : nullptr;
  uint32_t* s_present = (OPS & B_PRESENT) ? (uint32_t*)(smem_rd + lay.present_off) : nullptr;
  Enc* s_mm = (OPS & (B_MIN | B_MAX)) ? (Enc*)(smem_rd + lay.minmax_off) : nullptr;
  uint32_t* s_nanflag = (OPS & B_NANFLAG) ? (uint32_t*)(smem_rd + lay.nanflag_off) : nullptr;

  const int tid = threadIdx.x;
  for (int g = tid; g < ng_here; g += blockDim.x) {
    if (OPS & (B_SUM | B_SSD)) s_sum[g] = (SumT)0;
    if (IS_PROD) s_sum[g] = (SumT)1;
    if (OPS & B_CNT) s_cnt[g] = 0u;
    if (OPS & B_PRESENT) s_present[g] = 0u;
    if (OPS & B_MIN) s_mm[g] = (Enc)~(Enc)0;
    if (OPS & B_MAX) s_mm[g] = (Enc)0;
    if (OPS & B_NANFLAG) s_nanflag[g] = 0u;
  }
  __syncthreads();

  /* grid-stride over the bucket's row chunks (handles any skew). Sorted
   * labels put a wave's 64 lanes in at most a couple of groups, so naive
   * per-lane LDS atomics serialize 64-way; instead each wave combines its
   * run segments with a shuffle scan and only the last lane of each run
   * touches LDS (one atomic per run per wave). */
  const int lane = tid & 63;
  constexpr uint32_t LC_INVALID = 0xFFFFFFFFu;
  for (int64_t start = bkt_begin + (int64_t)blockIdx.x * chunk; start < bkt_end;
       start += (int64_t)gridDim.x * chunk) {
    const int64_t end = (start + chunk < bkt_end) ? start + chunk : bkt_end;
    for (int64_t i0 = start + (int64_t)(tid & ~63); i0 < end; i0 += blockDim.x) {
      const int64_t i = i0 + lane;
      uint32_t lc = LC_INVALID;
      V v = (V)0;
      bool vnan = false;
      if (i < end) {
        lc = (uint32_t)((int64_t)labels[i] - gbase);
        if (lc >= (uint32_t)ng_here) {
          lc = LC_INVALID; /* defensive: contract says in-range */
        } else {
          v = values[i];
          vnan = TR::isnan_(v);
        }
      }
      const bool skiprow = vnan && skipnan;
      SumT s = (SumT)0;
      uint32_t cn = 0;
      Enc mm = (OPS & B_MIN) ? (Enc)~(Enc)0 : (Enc)0; /* combine identity */
      uint32_t nf = 0;
      if (lc != LC_INVALID) {
        if (OPS & B_SUM) s = skiprow ? (SumT)0 : (SumT)(Acc)v;
        if (IS_PROD) s = skiprow ? (SumT)1 : (SumT)(Acc)v;
        if (OPS & B_SSD) {
          if (!skiprow) {
            const double d = (double)v - means[gbase + lc];
            s = (SumT)(d * d);
          }
        }
        cn = vnan ? 0u : 1u;
        if ((OPS & (B_MIN | B_MAX)) && !vnan) mm = TR::enc(v);
        nf = vnan ? 1u : 0u;
      } else if (IS_PROD) {
        s = (SumT)1;
      }
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t olc = __shfl_up(lc, d, 64);
        const SumT os = __shfl_up(s, d, 64);
        const uint32_t ocn = __shfl_up(cn, d, 64);
        const Enc omm = __shfl_up(mm, d, 64);
        const uint32_t onf = __shfl_up(nf, d, 64);
        if (lane >= d && lc != LC_INVALID && olc == lc) {
          if (OPS & (B_SUM | B_SSD)) s += os;
          if (IS_PROD) s *= os;
          cn += ocn;
          if (OPS & B_MIN) mm = omm < mm ? omm : mm;
          if (OPS & B_MAX) mm = omm > mm ? omm : mm;
          nf |= onf;
        }
      }
      const uint32_t nlc = __shfl_down(lc, 1, 64);
      const bool boundary = (lane == 63) || (nlc != lc);
      if (boundary && lc != LC_INVALID) {
        /* s is already SumT: never narrow through Acc here — for SSD with
         * integer V, Acc is int64 and the cast would truncate the run's
         * double d^2 partial (found by the huge fuzz, seed 246810 case 21) */
        if (OPS & (B_SUM | B_SSD)) acc_add(&s_sum[lc], s);
        if (IS_PROD) acc_mul(&s_sum[lc], s);
        if ((OPS & B_CNT) && cn) atomicAdd(&s_cnt[lc], cn);
        if (OPS & B_PRESENT) s_present[lc] = 1u;
        /* gate on cn (count of non-NaN rows in the run): a real extreme can
         * encode to the combine identity (e.g. INT_MAX under min) */
        if ((OPS & B_MIN) && cn) enc_min(&s_mm[lc], mm);
        if ((OPS & B_MAX) && cn) enc_max(&s_mm[lc], mm);
        if ((OPS & B_NANFLAG) && nf) s_nanflag[lc] = 1u;
      }
    }
  }
  __syncthreads();
  for (int g = tid; g < ng_here; g += blockDim.x) {
    const int64_t o = gbase + g;
    if ((OPS & (B_SUM | B_SSD)) && s_sum[g] != (SumT)0) acc_add(&((SumT*)out_sum)[o], s_sum[g]);
    if (IS_PROD && s_sum[g] != (SumT)1) acc_mul(&((SumT*)out_sum)[o], s_sum[g]);
    if ((OPS & B_CNT) && s_cnt[g])
      atomicAdd(reinterpret_cast<unsigned long long*>(&out_count[o]), (unsigned long long)s_cnt[g]);
    if ((OPS & B_PRESENT) && s_present[g]) out_present[o] = 1u;
    if (OPS & B_MIN) enc_min(&((Enc*)out_min)[o], s_mm[g]);
    if (OPS & B_MAX) enc_max(&((Enc*)out_max)[o], s_mm[g]);
    if ((OPS & B_NANFLAG) && s_nanflag[g]) out_nanflag[o] = 1u;
  }
}

/* per-bucket LDS-binned reduce of the scattered pairs; flush with global
 * atomics (a few chunks per bucket at most) into the FINAL bins */
template <typename V, int OPS>
__launch_bounds__(BLOCK_LDS) __global__ void k_reduce_bucket(
    const PairT<V>* __restrict__ pairs, const uint32_t* __restrict__ base,
    uint32_t cap2 /* 0: base[b]..base[b+1]; else b*cap2..min(base[b],(b+1)*cap2) */,
    int64_t chunk, int gpb, int shift, int64_t ngroups,
    const double* __restrict__ means, int skipnan, BinLayout lay,
    void* out_sum, int64_t* out_count, uint32_t* out_present, void* out_min,
    void* out_max, uint32_t* out_nanflag) {
  using TR = Traits<V>;
  using Acc = typename TR::Acc;
  using SumT = typename std::conditional<
      (OPS & (B_SSD | B_WELFORD)) != 0, double,
      typename std::conditional<(OPS & (B_IDXMIN | B_IDXMAX)) != 0, int64_t, Acc>::type>::type;
  using Enc = typename TR::Enc;
  constexpr bool IS_PROD = (OPS & B_PROD) != 0;

  const int b = blockIdx.y;
  int64_t bkt_begin, bkt_end;
  if (cap2) {
    bkt_begin = (int64_t)(uint32_t)b * cap2;
    bkt_end = base[b];
    const int64_t lim = bkt_begin + cap2;
    if (bkt_end > lim) bkt_end = lim;
  } else {
    bkt_begin = base[b];
    bkt_end = base[b + 1];
  }
  const int64_t start = bkt_begin + (int64_t)blockIdx.x * chunk;
  if (start >= bkt_end) return;
  const int64_t end = (start + chunk < bkt_end) ? start + chunk : bkt_end;
  const int64_t gbase = (int64_t)b << shift;
  const int ng_here = (int)(((gbase + gpb) <= ngroups) ? gpb : (ngroups - gbase));

  extern __shared__ __attribute__((aligned(16))) char smem_rb[];
  SumT* s_sum = (OPS & (B_SUM | B_SSD | B_PROD | B_IDXMIN | B_IDXMAX))
                    ? (SumT*)(smem_rb + lay.sum_off) : nullptr;
  uint32_t* s_cnt = (OPS & B_CNT) ? (uint32_t*)(smem_rb + lay.cnt_off) : nullptr;
  uint32_t* s_present = (OPS & B_PRESENT) ? (uint32_t*)(smem_rb + lay.present_off) : nullptr;
  Enc* s_mm = (OPS & (B_MIN | B_MAX)) ? (Enc*)(smem_rb + lay.minmax_off) : nullptr;
  uint32_t* s_nanflag = (OPS & B_NANFLAG) ? (uint32_t*)(smem_rb + lay.nanflag_off) : nullptr;

  const int tid = threadIdx.x;
  for (int g = tid; g < ng_here; g += blockDim.x) {
    if (OPS & (B_SUM | B_SSD)) s_sum[g] = (SumT)0;
    if (IS_PROD) s_sum[g] = (SumT)1;
    if (OPS & B_IDXMIN) s_sum[g] = (SumT)INT64_MAX;
    if (OPS & B_IDXMAX) s_sum[g] = (SumT)(-1);
    if (OPS & B_CNT) s_cnt[g] = 0u;
    if (OPS & B_PRESENT) s_present[g] = 0u;
    if (OPS & B_MIN) s_mm[g] = (Enc)~(Enc)0;
    if (OPS & B_MAX) s_mm[g] = (Enc)0;
    if (OPS & B_NANFLAG) s_nanflag[g] = 0u;
  }
  __syncthreads();

  auto body = [&](const PairT<V> p) {
    const uint32_t lc = p.lc;
    const V v = p.v;
    const bool vnan = TR::isnan_(v);
    if (OPS & B_PRESENT) s_present[lc] = 1u;
    if (vnan && skipnan) return;
    if (OPS & B_SUM) acc_add(&s_sum[lc], (Acc)v);
    if (IS_PROD) acc_mul(&s_sum[lc], (Acc)v);
    if (OPS & B_SSD) {
      const double d = (double)v - means[gbase + lc];
      atomicAdd((double*)s_sum + lc, d * d);
    }
    if (OPS & B_CNT) {
      if (!vnan) atomicAdd(&s_cnt[lc], 1u);
    }
    if (OPS & (B_MIN | B_MAX)) {
      if (vnan) {
        if (OPS & B_NANFLAG) s_nanflag[lc] = 1u;
      } else {
        if (OPS & B_MIN) enc_min(&s_mm[lc], TR::enc(v));
        if (OPS & B_MAX) enc_max(&s_mm[lc], TR::enc(v));
      }
    }
  };
  if constexpr (sizeof(PairT<V>) == 8) {
    /* two pairs per thread per trip (one 16-B load): doubles the per-wave
     * outstanding-load count — this kernel is latency-parked, not
     * bandwidth-bound (SQ_WAIT_ANY ~88% of WAVE_CYCLES before this) */
    struct Pair2 { PairT<V> a, b; };
    const int64_t s2 = (start + 1) & ~1LL;
    if (start < s2 && start < end && tid == 0) body(pairs[start]);
    const int64_t nv = (end - s2) / 2;
    const Pair2* __restrict__ vp = (const Pair2*)(pairs + s2);
    for (int64_t j = tid; j < nv; j += blockDim.x) {
      const Pair2 q = vp[j];
      body(q.a);
      body(q.b);
    }
    const int64_t rem = s2 + nv * 2;
    if (rem < end && tid == 0) body(pairs[rem]);
  } else {
    for (int64_t i = start + tid; i < end; i += blockDim.x) body(pairs[i]);
  }
  __syncthreads();
  /* flush into the final bins (out_min/out_max hold ENCODED values until
   * k_decode, exactly like the global-atomic path) */
  for (int g = tid; g < ng_here; g += blockDim.x) {
    const int64_t o = gbase + g;
    if ((OPS & (B_SUM | B_SSD)) && s_sum[g] != (SumT)0) acc_add(&((SumT*)out_sum)[o], s_sum[g]);
    if (IS_PROD && s_sum[g] != (SumT)1) acc_mul(&((SumT*)out_sum)[o], s_sum[g]);
    if ((OPS & B_CNT) && s_cnt[g])
      atomicAdd(reinterpret_cast<unsigned long long*>(&out_count[o]), (unsigned long long)s_cnt[g]);
    if ((OPS & B_PRESENT) && s_present[g]) out_present[o] = 1u;
    if (OPS & B_MIN) enc_min(&((Enc*)out_min)[o], s_mm[g]);
    if (OPS & B_MAX) enc_max(&((Enc*)out_max)[o], s_mm[g]);
    if ((OPS & B_NANFLAG) && s_nanflag[g]) out_nanflag[o] = 1u;
  }
}


/* second bucket pass for the pair-payload arg-reductions (FH_SET_ARG*_PAIR):
 * re-reads the scattered pairs and keeps, per group, the SMALLEST row index
 * among rows matching the group's extremum (first occurrence = np.argmin /
 * np.argmax tie rule; numeric == so +-0.0 match each other exactly as the
 * reference's target-match pass does). Targets and nanflags are staged into
 * LDS once per bucket — after the partition they are bucket-local, unlike
 * the two-pass atomic form's random gathers over the full 80 MB bins. */
template <typename V>
__launch_bounds__(BLOCK_LDS) __global__ void k_reduce_bucket_argrow(
    const PairT<V>* __restrict__ pairs, const uint32_t* __restrict__ base,
    uint32_t cap2, int64_t chunk, int gpb, int shift, int64_t ngroups,
    int skipnan, const V* __restrict__ target,
    const uint32_t* __restrict__ nanflag, int64_t* __restrict__ out_idx) {
  using TR = Traits<V>;
  const int b = blockIdx.y;
  int64_t bkt_begin, bkt_end;
  if (cap2) {
    bkt_begin = (int64_t)(uint32_t)b * cap2;
    bkt_end = base[b];
    const int64_t lim = bkt_begin + cap2;
    if (bkt_end > lim) bkt_end = lim;
  } else {
    bkt_begin = base[b];
    bkt_end = base[b + 1];
  }
  const int64_t start = bkt_begin + (int64_t)blockIdx.x * chunk;
  if (start >= bkt_end) return;
  const int64_t end = (start + chunk < bkt_end) ? start + chunk : bkt_end;
  const int64_t gbase = (int64_t)b << shift;
  const int ng_here = (int)(((gbase + gpb) <= ngroups) ? gpb : (ngroups - gbase));

  extern __shared__ __attribute__((aligned(16))) char smem_ar[];
  V* s_target = (V*)smem_ar;
  uint32_t* s_row = (uint32_t*)(smem_ar + (int64_t)gpb * sizeof(V));
  uint32_t* s_nan = nanflag ? s_row + gpb : nullptr;
  const int tid = threadIdx.x;
  for (int g = tid; g < ng_here; g += blockDim.x) {
    s_target[g] = target[gbase + g];
    s_row[g] = 0xFFFFFFFFu;
    if (s_nan) s_nan[g] = nanflag[gbase + g];
  }
  __syncthreads();
  for (int64_t i = start + tid; i < end; i += blockDim.x) {
    const PairT<V> p = pairs[i];
    const uint32_t lc = p.lc;
    const V v = p.v;
    const bool vnan = TR::isnan_(v);
    bool match;
    if (skipnan)
      match = !vnan && v == s_target[lc];
    else if (s_nan && s_nan[lc])
      match = vnan; /* non-skip arg* land on the first NaN, as numpy does */
    else
      match = !vnan && v == s_target[lc];
    if (match) atomicMin(&s_row[lc], p.pad);
  }
  __syncthreads();
  for (int g = tid; g < ng_here; g += blockDim.x) {
    const uint32_t r = s_row[g];
    if (r != 0xFFFFFFFFu)
      idx_min(&out_idx[gbase + g], (int64_t)r);
  }
}

/* ---- host launch helpers ------------------------------------------------- */

/* blocks of `per` items covering n */
inline int grid_for(int64_t n, int64_t per = 256) { return (int)((n + per - 1) / per); }

/* the same, but at least one block and at most `cap` (grid-stride kernels) */
inline int capped_grid(int64_t n, int64_t per, int cap) {
  const int64_t wb = (n + per - 1) / per;
  return (int)(wb < cap ? (wb > 0 ? wb : 1) : cap);
}

/* p[0..n) = v, for identities memset cannot write */
inline hipError_t fill_bins(void* p, int64_t n, int64_t v, hipStream_t stream) {
  hipLaunchKernelGGL(k_fill_i64, dim3(grid_for(n)), dim3(256), 0, stream,
                     (int64_t*)p, n, v);
  return hipGetLastError();
}
inline hipError_t fill_bins(void* p, int64_t n, double v, hipStream_t stream) {
  hipLaunchKernelGGL(k_fill_f64, dim3(grid_for(n)), dim3(256), 0, stream,
                     (double*)p, n, v);
  return hipGetLastError();
}

/* where one copy of the bins lives: the call's output arrays (8-byte counts)
 * or one row chunk's slab sections (4-byte counts) */
struct BinPtrs {
  void *sum, *cnt, *present, *min, *max, *nanflag, *sumx;
  int cnt_bytes;
  /* B_MOM2: the M2 bins (out_ssd, or a chunk's s2 section). `present` is
   * then null in a slab, which has no such section for the set. */
  void* ssd;
  /* B_ARGC: a chunk's first-NaN-row section; null for the output arrays */
  void* nanrow;
};

inline BinPtrs out_bins(const fh_call* c) {
  /* B_WELFORD's sum-of-x rides the out_min slot */
  return {c->out_sum, c->out_count, c->out_present, c->out_min,
          c->out_max, c->out_nanflag, c->out_min, 8, c->out_ssd};
}

inline BinPtrs slab_bins(char* s, const BinLayout& lay) {
  /* sections a set lacks (offset -1) are never touched; min and max share
   * minmax_off except in the summary set, whose max has max_off */
  const bool mom2 = lay.max_off >= 0;
  return {s + lay.sum_off, s + lay.cnt_off,
          mom2 ? nullptr : s + lay.present_off, s + lay.minmax_off,
          s + (mom2 ? lay.max_off : lay.minmax_off), s + lay.nanflag_off,
          s + lay.sumx_off, 4, mom2 ? s + lay.s2_off : nullptr,
          lay.nanrow_off >= 0 ? s + lay.nanrow_off : nullptr};
}

/* identity-fill every section of OPS: min bins 0xFF.., max bins 0x00.. (the
 * order-preserving encoding), products 1, row-index bins INT64_MAX (IDXMIN,
 * and ARGROW: min-row on both argmin and argmax, first occurrence) or -1
 * (IDXMAX), everything else 0 */
template <typename V, int OPS>
int init_bins(const BinPtrs& b, int64_t nbins, hipStream_t stream) {
  using TR = Traits<V>;
  if (OPS & (B_SUM | B_SSD | B_WELFORD)) FH_CHECK(hipMemsetAsync(b.sum, 0, nbins * 8, stream));
  if (OPS & B_WELFORD) FH_CHECK(hipMemsetAsync(b.sumx, 0, nbins * 8, stream));
  if (OPS & (B_IDXMIN | B_ARGROW | B_ARGC)) FH_CHECK(fill_bins(b.sum, nbins, (int64_t)INT64_MAX, stream));
  /* a chunk's extremum section stays unwritten: the merge skips a side
   * whose row is the sentinel */
  if ((OPS & B_ARGC) && b.nanrow) FH_CHECK(fill_bins(b.nanrow, nbins, (int64_t)INT64_MAX, stream));
  if (OPS & B_IDXMAX) FH_CHECK(fill_bins(b.sum, nbins, (int64_t)-1, stream));
  if (OPS & B_PROD) FH_CHECK(fill_bins(b.sum, nbins, (typename TR::Acc)1, stream));
  if (OPS & B_CNT) FH_CHECK(hipMemsetAsync(b.cnt, 0, nbins * b.cnt_bytes, stream));
  if (OPS & B_PRESENT) FH_CHECK(hipMemsetAsync(b.present, 0, nbins * 4, stream));
  if (OPS & B_MIN)
    FH_CHECK(hipMemsetAsync(b.min, 0xFF, nbins * sizeof(typename TR::Enc), stream));
  if (OPS & B_MAX)
    FH_CHECK(hipMemsetAsync(b.max, 0x00, nbins * sizeof(typename TR::Enc), stream));
  if (OPS & B_NANFLAG) FH_CHECK(hipMemsetAsync(b.nanflag, 0, nbins * 4, stream));
  if constexpr ((OPS & B_MOM2) != 0) {
    /* bins no segment touches: M2 0, and "no row seen". A slab's pivot and
     * offset sections stay unwritten: the merge skips a side with count 0. */
    FH_CHECK(hipMemsetAsync(b.ssd, 0, nbins * 8, stream));
    if (b.present) FH_CHECK(hipMemsetAsync(b.present, 0, nbins * 4, stream));
  }
  return 0;
}

/* decode the output min/max bins in place */
template <typename V, int OPS>
int launch_decode(fh_call* c, int64_t nbins, hipStream_t stream) {
  if (OPS & (B_MIN | B_MAX)) {
    hipLaunchKernelGGL((k_decode<V, OPS>), dim3(grid_for(nbins)), dim3(256), 0,
                       stream, nbins, c->out_min, c->out_max, c->out_count,
                       c->out_present);
    FH_CHECK(hipGetLastError());
  }
  return 0;
}

/* ---- partition-path host plumbing ---------------------------------------- */
struct PartPlan {
  int shift, gpb, B, Bpad;
  bool two_level;      /* B > 64: scatter via <= 64 super-buckets first */
  int B1;              /* super-bucket count (two_level) */
  BinLayout lay;       /* per-bucket bins (gpb entries) */
  int64_t pairs_off, pairs2_off, counts_off, base_off, baseA_off, cursors_off, bytes;
  int64_t overflow_off;
  uint32_t cap1, cap2; /* optimistic region strides (super / fine) */
  bool optimistic;     /* capacity regions fit u32 cursors */
  int64_t tile_lds;    /* dynamic LDS of either scatter pass */
  bool feasible;
};

constexpr int64_t part_tile_lds(int T, int pairsz) {
  return (int64_t)(PART_SUB * PART_NW + PART_NW + 1 + PART_SUB + 3) * 4 +
         (int64_t)T * 4 + (int64_t)T * pairsz;
}

/* FH_PART_BINKB: pass-C LDS bin budget in KiB (larger bins -> fewer, bigger
 * buckets -> fewer reservation atomics) */
inline int64_t fh_part_bin_bytes() {
  static int64_t v = -1;
  if (v < 0) {
    /* default 120 measured best: for 16 B/group sets it keeps shift 12
     * (4096 groups/bucket, 2 reduce WGs/CU) — 10.6 ms vs 11.4 at 150 KiB
     * (shift 13, 1 WG/CU) on the 1e9-row/1e7-group sum (r02 A/B) */
    const char* e = getenv("FH_PART_BINKB");
    int kb = e ? atoi(e) : 120;
    if (kb < 16) kb = 16;
    v = (int64_t)kb * 1024;
    if (v > LDS_MAX) v = LDS_MAX;
  }
  return v;
}

template <typename V>
PartPlan part_plan(const fh_call* c) {
  PartPlan p{};
  p.feasible = false;
  if (c->n >= ((int64_t)1 << 31) || c->ngroups <= 0) return p;
  const int bits = set_bits(c->op_set);
  if (bits & (B_IDXMIN | B_IDXMAX)) return p; /* pairs carry no row index */
  if ((bits & B_ARGROW) &&
      (sizeof(PairT<V>) != 16 || c->n + c->row_offset >= ((int64_t)1 << 32)))
    return p; /* pad word (8-byte dtypes) carries the 32-bit row */
  int shift = 13;
  while (shift > 8 && bin_layout<V>(bits, (int64_t)1 << shift, 4).bytes > fh_part_bin_bytes())
    shift--;
  BinLayout lay = bin_layout<V>(bits, (int64_t)1 << shift, 4);
  if (lay.bytes > fh_part_bin_bytes()) return p;
  int64_t B64 = (c->ngroups + ((int64_t)1 << shift) - 1) >> shift;
  if (B64 > 4096) return p;
  p.B = (int)B64;
  p.shift = shift;
  p.gpb = 1 << shift;
  p.lay = lay;
  p.two_level = p.B > PART_SUB;
  p.B1 = p.two_level ? (p.B + PART_SUB - 1) / PART_SUB : 0;
  /* pass-A bucket count: B1 when two-level, else the fine B */
  const int bA = p.two_level ? p.B1 : p.B;
  if (bA > PART_SUB) return p; /* scatter passes handle <= 64 buckets */
  p.Bpad = PART_SUB;
  p.tile_lds = part_tile_lds(PART_TILE<V>, (int)sizeof(PairT<V>));
  if (p.tile_lds > LDS_MAX) return p;
  /* optimistic capacity regions: uniform 25% + 8K rows of slack per bucket;
   * overflow (extreme skew) falls back to the exact counted path */
  auto cap_of = [&](int nb) {
    const int64_t mean = (c->n + nb - 1) / nb;
    return (uint32_t)(((mean + (mean >> 2) + 8192) + 63) / 64 * 64);
  };
  p.cap2 = cap_of(p.B);
  p.cap1 = p.two_level ? cap_of(p.B1) : 0;
  const int64_t reg2 = (int64_t)p.B * p.cap2;
  const int64_t reg1 = p.two_level ? (int64_t)p.B1 * p.cap1 : reg2;
  p.optimistic = reg1 < ((int64_t)1 << 31) && reg2 < ((int64_t)1 << 31);
  int64_t off = 0;
  auto carve = [&](int64_t b) {
    int64_t o = off;
    off += ((b + 255) / 256) * 256;
    return o;
  };
  const int64_t p1elems = p.optimistic ? std::max(c->n, reg1) : c->n;
  const int64_t p2elems = p.optimistic ? std::max(c->n, reg2) : c->n;
  p.pairs_off = carve(p1elems * (int64_t)sizeof(PairT<V>));
  p.pairs2_off = p.two_level ? carve(p2elems * (int64_t)sizeof(PairT<V>)) : p.pairs_off;
  p.counts_off = carve((int64_t)p.B * 4);
  p.base_off = carve(((int64_t)p.B + 1) * 4);
  p.baseA_off = carve(((int64_t)p.B1 + 1) * 4);
  p.cursors_off = carve((int64_t)p.B * 4);
  p.overflow_off = carve(256);
  p.bytes = off;
  p.feasible = true;
  return p;
}

/* the plan's carve of the caller's scratch */
template <typename V>
struct PartScratch {
  PairT<V> *pairs, *pairs2;
  uint32_t *counts, *base, *baseA, *cursors, *overflow;
};

template <typename V>
PartScratch<V> part_scratch(const fh_call* c, const PartPlan& pp) {
  char* scr = (char*)c->scratch;
  return {(PairT<V>*)(scr + pp.pairs_off),     (PairT<V>*)(scr + pp.pairs2_off),
          (uint32_t*)(scr + pp.counts_off),    (uint32_t*)(scr + pp.base_off),
          (uint32_t*)(scr + pp.baseA_off),     (uint32_t*)(scr + pp.cursors_off),
          (uint32_t*)(scr + pp.overflow_off)};
}

/* one level of scattered buckets as the next stage reads it. cap == 0: the
 * counted directory, bucket b is [ends[b], ends[b+1]). cap != 0: optimistic
 * capacity regions, bucket b is [b*cap, ends[b]) with `ends` the cursors the
 * scatter left behind. maxspan bounds any bucket's rows (it sizes the grid). */
struct BucketDir {
  const uint32_t* ends;
  uint32_t cap;
  int64_t maxspan;
};

/* pass 1: rows -> pairs, into the super-buckets when two-level, else the
 * fine buckets. cursors[b] is bucket b's next free slot: a counted base
 * (cap 0), or b*cap with writes past (b+1)*cap flagged in *overflow */
template <typename V, typename L, bool CROW>
int scatter_pass1(fh_call* c, const PartPlan& pp, uint32_t* cursors, uint32_t cap,
                  uint32_t* overflow, PairT<V>* pairs, hipStream_t stream) {
  auto kern = k_part_scatter<V, L, CROW>;
  FH_CHECK(hipFuncSetAttribute((const void*)kern,
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)pp.tile_lds));
  const int shA = pp.two_level ? pp.shift + 6 : pp.shift;
  const int bA = pp.two_level ? pp.B1 : pp.B;
  hipLaunchKernelGGL(kern, dim3(capped_grid(c->n, PART_TILE<V>, 1024)),
                     dim3(PART_BLOCK), pp.tile_lds, stream, (const V*)c->values,
                     (const L*)c->labels, (const L*)c->labels2, c->n, c->ngroups,
                     c->g0, c->g1, shA, bA, pp.Bpad, cursors, cap, overflow,
                     pairs, c->row_offset);
  FH_CHECK(hipGetLastError());
  return 0;
}

/* pass 2 (two-level only): each super-bucket of `in` -> its <= 64 fine
 * buckets in `out`; cursors/cap2 as in pass 1 */
template <typename V, bool CROW>
int scatter_pass2(const PartPlan& pp, const PairT<V>* in, const BucketDir& super,
                  uint32_t* cursors, uint32_t cap2, uint32_t* overflow,
                  PairT<V>* out, hipStream_t stream) {
  auto kern = k_part_scatter2<V, CROW>;
  FH_CHECK(hipFuncSetAttribute((const void*)kern,
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)pp.tile_lds));
  const int tiles_x = capped_grid(super.maxspan, PART_TILE<V>, 64);
  hipLaunchKernelGGL(kern, dim3(tiles_x, pp.B1), dim3(PART_BLOCK), pp.tile_lds,
                     stream, in, super.ends, super.cap, pp.shift, pp.B, cursors,
                     cap2, overflow, out);
  FH_CHECK(hipGetLastError());
  return 0;
}

/* pass C: identity-fill the outputs, reduce every fine bucket in LDS, decode
 * min/max, then the arg-pair sets' matching-row phase */
template <typename V, int OPS>
int reduce_buckets(fh_call* c, const PartPlan& pp, const PairT<V>* pairs,
                   const BucketDir& fine, hipStream_t stream) {
  const int skipnan = (c->flags & FH_SKIPNAN) ? 1 : 0;
  const int64_t chunk = 1 << 19;
  const int maxchunks = capped_grid(fine.maxspan, chunk, INT32_MAX);
  FH_TRY((init_bins<V, OPS>(out_bins(c), c->ngroups, stream)));
  auto kern = k_reduce_bucket<V, OPS>;
  FH_CHECK(hipFuncSetAttribute((const void*)kern,
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)pp.lay.bytes));
  hipLaunchKernelGGL(kern, dim3(maxchunks, pp.B), dim3(BLOCK_LDS), pp.lay.bytes,
                     stream, pairs, fine.ends, fine.cap, chunk, pp.gpb, pp.shift,
                     c->ngroups, c->means, skipnan, pp.lay, c->out_sum,
                     c->out_count, c->out_present, c->out_min, c->out_max,
                     c->out_nanflag);
  FH_CHECK(hipGetLastError());
  FH_TRY((launch_decode<V, OPS>(c, c->ngroups, stream)));
  if constexpr ((OPS & B_ARGROW) != 0 && sizeof(PairT<V>) == 16) {
    const V* target = (const V*)((OPS & B_MIN) ? c->out_min : c->out_max);
    const uint32_t* nan = skipnan ? nullptr : (const uint32_t*)c->out_nanflag;
    const int64_t lds = ((int64_t)pp.gpb * (sizeof(V) + 8) + 255) / 256 * 256;
    auto arg = k_reduce_bucket_argrow<V>;
    FH_CHECK(hipFuncSetAttribute((const void*)arg,
                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds));
    hipLaunchKernelGGL(arg, dim3(maxchunks, pp.B), dim3(BLOCK_LDS), lds, stream,
                       pairs, fine.ends, fine.cap, chunk, pp.gpb, pp.shift,
                       c->ngroups, skipnan, target, nan, (int64_t*)c->out_sum);
    FH_CHECK(hipGetLastError());
  }
  return 0;
}

/* exact partition: a counting pre-pass and a host-built bucket directory
 * give every bucket its true extent (cap 0 throughout) */
template <typename V, typename L, int OPS>
int launch_partition_exact(fh_call* c, const PartPlan& pp) {
  hipStream_t stream = (hipStream_t)c->stream;
  constexpr bool CROW = (OPS & B_ARGROW) != 0 && sizeof(PairT<V>) == 16;
  const PartScratch<V> s = part_scratch<V>(c, pp);

  FH_CHECK(hipMemsetAsync(s.counts, 0, (int64_t)pp.B * 4, stream));
  {
    /* the count pass histograms the FINE buckets (up to 4096) */
    const int64_t hist_lds = ((int64_t)pp.B + 63) / 64 * 64 * 4;
    hipLaunchKernelGGL((k_part_count<L>), dim3(capped_grid(c->n, 256, 2048)),
                       dim3(256), hist_lds, stream, (const L*)c->labels,
                       (const L*)c->labels2, c->n, c->ngroups, c->g0, c->g1,
                       pp.shift, pp.B, s.counts);
    FH_CHECK(hipGetLastError());
  }
  /* bucket directory on the host (one sync; B <= 4096 words) */
  static thread_local uint32_t h_counts[4096], h_base[4097];
  FH_CHECK(hipMemcpyAsync(h_counts, s.counts, (int64_t)pp.B * 4,
                          hipMemcpyDeviceToHost, stream));
  FH_CHECK(hipStreamSynchronize(stream));
  uint32_t acc = 0, maxc = 0;
  for (int i = 0; i < pp.B; ++i) {
    h_base[i] = acc;
    acc += h_counts[i];
    if (h_counts[i] > maxc) maxc = h_counts[i];
  }
  h_base[pp.B] = acc;
  FH_CHECK(hipMemcpyAsync(s.base, h_base, ((int64_t)pp.B + 1) * 4,
                          hipMemcpyHostToDevice, stream));
  /* super-bucket directory: sums of PART_SUB fine buckets */
  static thread_local uint32_t h_baseA[4097];
  uint32_t maxA = 0;
  if (pp.two_level) {
    for (int sbi = 0; sbi <= pp.B1; ++sbi) {
      const int fb = sbi * PART_SUB;
      h_baseA[sbi] = h_base[fb < pp.B ? fb : pp.B];
    }
    for (int sbi = 0; sbi < pp.B1; ++sbi) {
      const uint32_t cnt = h_baseA[sbi + 1] - h_baseA[sbi];
      if (cnt > maxA) maxA = cnt;
    }
    FH_CHECK(hipMemcpyAsync(s.baseA, h_baseA, ((int64_t)pp.B1 + 1) * 4,
                            hipMemcpyHostToDevice, stream));
  }
  /* pass-1 cursors: the bases of the buckets it scatters into */
  FH_CHECK(hipMemcpyAsync(s.cursors, pp.two_level ? h_baseA : h_base,
                          (int64_t)(pp.two_level ? pp.B1 : pp.B) * 4,
                          hipMemcpyHostToDevice, stream));
  FH_TRY((scatter_pass1<V, L, CROW>(c, pp, s.cursors, 0u, s.overflow, s.pairs, stream)));
  if (pp.two_level) {
    /* fine-bucket cursors, then the in-super-bucket scatter */
    FH_CHECK(hipMemcpyAsync(s.cursors, h_base, (int64_t)pp.B * 4,
                            hipMemcpyHostToDevice, stream));
    FH_TRY((scatter_pass2<V, CROW>(pp, s.pairs, BucketDir{s.baseA, 0u, (int64_t)maxA},
                                   s.cursors, 0u, s.overflow, s.pairs2, stream)));
  }
  FH_TRY((reduce_buckets<V, OPS>(c, pp, pp.two_level ? s.pairs2 : s.pairs,
                                 BucketDir{s.base, 0u, (int64_t)maxc}, stream)));
  c->path_used = 4;
  return 0;
}

/* optimistic partition: capacity regions replace the counting pre-pass and
 * every host round trip except the final 4-byte overflow check. (A one-level
 * direct scatter into all fine buckets was measured and rejected:
 * profiles/r02_direct_pmc.md, 3.5x write amplification.) */
template <typename V, typename L, int OPS>
int launch_partition(fh_call* c, const PartPlan& pp) {
  if (!pp.optimistic) return launch_partition_exact<V, L, OPS>(c, pp);
  hipStream_t stream = (hipStream_t)c->stream;
  constexpr bool CROW = (OPS & B_ARGROW) != 0 && sizeof(PairT<V>) == 16;
  const PartScratch<V> s = part_scratch<V>(c, pp);

  FH_CHECK(hipMemsetAsync(s.overflow, 0, 4, stream));
  uint32_t* cursorsA = s.counts; /* reused slot */
  const int bA = pp.two_level ? pp.B1 : pp.B;
  const uint32_t capA = pp.two_level ? pp.cap1 : pp.cap2;
  hipLaunchKernelGGL(k_init_cursors, dim3(1), dim3(PART_SUB), 0, stream,
                     cursorsA, bA, capA);
  FH_CHECK(hipGetLastError());
  FH_TRY((scatter_pass1<V, L, CROW>(c, pp, cursorsA, capA, s.overflow, s.pairs, stream)));
  BucketDir fine{cursorsA, capA, (int64_t)capA};
  if (pp.two_level) {
    hipLaunchKernelGGL(k_init_cursors, dim3(grid_for(pp.B)), dim3(256), 0,
                       stream, s.cursors, pp.B, pp.cap2);
    FH_CHECK(hipGetLastError());
    FH_TRY((scatter_pass2<V, CROW>(pp, s.pairs, fine, s.cursors, pp.cap2,
                                   s.overflow, s.pairs2, stream)));
    fine = BucketDir{s.cursors, pp.cap2, (int64_t)pp.cap2};
  }
  FH_TRY((reduce_buckets<V, OPS>(c, pp, pp.two_level ? s.pairs2 : s.pairs, fine, stream)));
  uint32_t h_ov = 0;
  FH_CHECK(hipMemcpyAsync(&h_ov, s.overflow, 4, hipMemcpyDeviceToHost, stream));
  FH_CHECK(hipStreamSynchronize(stream));
  if (h_ov) return launch_partition_exact<V, L, OPS>(c, pp);
  c->path_used = 4;
  return 0;
}

/* sorted-labels direct path: skip every scatter pass — each bucket's rows
 * are already a contiguous range of the original arrays. Returns -1 when the
 * path does not apply to this call. */
template <typename V, typename L, int OPS>
int launch_sorted_direct(fh_call* c) {
  if (!(c->flags & FH_SORTED_LABELS) || c->labels2 ||
      (c->flags & FH_FORCE_ATOMIC) || (OPS & (B_IDXMIN | B_IDXMAX)))
    return -1;
  const PartPlan pp = part_plan<V>(c);
  if (!pp.feasible || c->scratch_bytes < (int64_t)(pp.B + 1) * 4) return -1;
  hipStream_t stream = (hipStream_t)c->stream;
  const bool skipnan = (c->flags & FH_SKIPNAN) != 0;
  uint32_t* base = (uint32_t*)c->scratch;
  hipLaunchKernelGGL((k_bucket_bounds<L>), dim3(grid_for(pp.B + 1)), dim3(256),
                     0, stream, (const L*)c->labels, c->n, pp.B, pp.shift, base);
  FH_CHECK(hipGetLastError());
  FH_TRY((init_bins<V, OPS>(out_bins(c), c->ngroups, stream)));
  auto kern = k_reduce_bucket_direct<V, L, OPS>;
  FH_CHECK(hipFuncSetAttribute((const void*)kern,
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)pp.lay.bytes));
  const int64_t chunk = 1 << 19;
  int nchunks = (int)((c->n / pp.B + chunk) / chunk) + 1;
  if (nchunks > 16) nchunks = 16;
  hipLaunchKernelGGL(kern, dim3(nchunks, pp.B), dim3(BLOCK_LDS), pp.lay.bytes,
                     stream, (const V*)c->values, (const L*)c->labels, base,
                     chunk, pp.gpb, pp.shift, c->ngroups, c->means, skipnan,
                     pp.lay, c->out_sum, c->out_count, c->out_present,
                     c->out_min, c->out_max, c->out_nanflag);
  FH_CHECK(hipGetLastError());
  FH_TRY((launch_decode<V, OPS>(c, c->ngroups, stream)));
  c->path_used = 5;
  return 0;
}

/* ---- host-side dispatch -------------------------------------------------- */

/* do the per-block bins of an op set fit LDS, and how many blocks per CU */
struct LdsPlan {
  BinLayout lay;
  bool fits;
  int blocks_per_cu;
};

template <typename V>
LdsPlan lds_plan(int bits, int64_t ngroups) {
  LdsPlan p{};
  p.lay = bin_layout<V>(bits, ngroups, 4);
  p.fits = p.lay.bytes <= LDS_MAX;
  p.blocks_per_cu = p.lay.bytes * 2 <= LDS_MAX ? 2 : 1;
  return p;
}

/* everything past the LDS-binned path: sorted-direct, bucket partition,
 * global atomics (never instantiated for cached code labels) */
template <typename V, typename L, int OPS>
int launch_beyond_lds(fh_call* c) {
  using TR = Traits<V>;
  hipStream_t stream = (hipStream_t)c->stream;
  const bool skipnan = (c->flags & FH_SKIPNAN) != 0;
  if (c->emit_codes) return 13; /* codes are emitted by the LDS kernel only */

  {
    const int rc = launch_sorted_direct<V, L, OPS>(c);
    if (rc >= 0) return rc;
  }

  /* huge group counts: bucket-partition path when scratch allows. Not
   * during hipGraph capture (FH_NO_HOST_SYNC): the optimistic overflow
   * check and the exact path's counting pre-pass read back to the host
   * and synchronize the stream, which invalidates a capture. */
  if (!(c->flags & (FH_FORCE_ATOMIC | FH_NO_HOST_SYNC))) {
    PartPlan pp = part_plan<V>(c);
    if (pp.feasible && c->scratch_bytes >= pp.bytes)
      return launch_partition<V, L, OPS>(c, pp);
  }

  /* global-atomic path */
  FH_TRY((init_bins<V, OPS>(out_bins(c), c->ngroups, stream)));
  hipLaunchKernelGGL((k_reduce_atomic<V, L, OPS>),
                     dim3(capped_grid(c->n / TR::VEC, BLOCK_ATOMIC, 2048)),
                     dim3(BLOCK_ATOMIC), 0, stream, (const V*)c->values,
                     (const L*)c->labels, (const L*)c->labels2, c->n, c->ngroups,
                     c->g0, c->g1, c->means, (const V*)c->target, c->row_offset,
                     (int)skipnan, c->out_sum,
                     c->out_count, c->out_present, c->out_min, c->out_max,
                     c->out_nanflag);
  FH_CHECK(hipGetLastError());
  FH_TRY((launch_decode<V, OPS>(c, c->ngroups, stream)));
  c->path_used = 2;
  return 0;
}

template <typename V, typename L, int OPS>
int launch_typed(fh_call* c) {
  hipStream_t stream = (hipStream_t)c->stream;
  const bool skipnan = (c->flags & FH_SKIPNAN) != 0;
  const LdsPlan lp = lds_plan<V>(OPS, c->ngroups);
  const BinLayout& lay = lp.lay;
  constexpr int CW = CodeWidth<L>::value; /* cached codes: 16, 14 or 12 bits */
  constexpr bool CODES = CW != 0;

  if (c->finish) {
    /* a finish mode is served by the LDS path's combine only: refuse rather
     * than hand back partials the caller did not allocate */
    if (c->finish != finish_of(OPS) || !lp.fits ||
        (c->flags & FH_FORCE_ATOMIC) || !c->result ||
        (c->result_dtype != FH_F32 && c->result_dtype != FH_F64 &&
         c->result_dtype != FH_I64) ||
        (c->finish == FH_FINISH_MEAN && c->result_dtype == FH_I64))
      return 14;
  }

  if constexpr ((OPS & B_MOM2) != 0) {
    /* the summary set exists on the LDS-binned path only */
    if (!lp.fits || (c->flags & FH_FORCE_ATOMIC)) return 15;
    if (!c->out_ssd) return 16;
  }

  if constexpr (CODES) {
    /* compact codes exist for the LDS-binned kernel only, and the all-ones
     * code of the width stays out of range */
    if ((OPS & B_ARGROW) || c->labels2 || c->emit_codes ||
        c->ngroups >= (int64_t)((1u << CW) - 1u) || !lp.fits ||
        (c->flags & FH_FORCE_ATOMIC))
      return 12;
  } else if (OPS & B_ARGROW) {
    /* pair-payload arg-reductions exist only on the partition path (which
     * host-syncs, so also refused during capture — callers use the
     * two-pass form there) */
    if (c->flags & (FH_FORCE_LDS | FH_FORCE_ATOMIC | FH_NO_HOST_SYNC))
      return 11;
    PartPlan pp = part_plan<V>(c);
    if (!pp.feasible || c->scratch_bytes < pp.bytes) return 11;
    return launch_partition<V, L, OPS>(c, pp);
  }

  bool use_lds = lp.fits;
  if (c->flags & FH_FORCE_ATOMIC) use_lds = false;
  if (c->flags & FH_FORCE_LDS) {
    if (!lp.fits) return 2; /* cannot honor */
    use_lds = true;
  }

  if (use_lds) {
    int nblocks = NUM_CU * lp.blocks_per_cu;
    /* do not launch more blocks than there is work or scratch for */
    const int64_t block_rows =
        (int64_t)BLOCK_LDS * (CW == 16 ? U16_ROWS : CODES ? FH_LANE_SLOTS : 1);
    int64_t work_blocks = (c->n + block_rows - 1) / block_rows;
    if (work_blocks < nblocks) nblocks = (int)(work_blocks > 0 ? work_blocks : 1);
    if ((int64_t)nblocks * lay.bytes > c->scratch_bytes) return 3;

    auto kern = k_reduce_lds<V, L, OPS>;
    if constexpr (!CODES) {
      if (c->emit_codes) {
        if (c->ngroups >= (int64_t)CODE_NONE) return 13;
        kern = k_reduce_lds<V, L, OPS, true>;
      }
    }
    FH_CHECK(hipFuncSetAttribute((const void*)kern,
                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lay.bytes));
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(BLOCK_LDS), lay.bytes, stream,
                       (const V*)c->values, (const L*)c->labels,
                       (const L*)c->labels2, c->n, c->ngroups, c->g0, c->g1,
                       c->means, (const V*)c->target, c->row_offset,
                       (int)skipnan, (char*)c->scratch, lay,
                       (uint16_t*)c->emit_codes);
    FH_CHECK(hipGetLastError());
    /* fold the slab; with a finish mode the same kernel writes the result */
    const int cb = (int)((c->ngroups + CT_X - 1) / CT_X);
    FinishArgs fa{c->result, c->result_dtype, c->has_fill, c->min_count, c->fill};
    auto comb = k_combine_tree<V, OPS, FIN_NONE>;
    if constexpr (finish_of(OPS) != FIN_NONE) {
      if (c->finish) comb = k_combine_tree<V, OPS, finish_of(OPS)>;
    }
    hipLaunchKernelGGL(comb, dim3(cb), dim3(CT_X, CT_Y), 0, stream,
                       (const char*)c->scratch, nblocks, c->ngroups, lay,
                       c->out_sum, c->out_count, c->out_present, c->out_min,
                       c->out_max, c->out_nanflag, (double*)c->out_ssd, fa);
    FH_CHECK(hipGetLastError());
    c->path_used = 1;
    return 0;
  }
  if constexpr ((OPS & B_MOM2) != 0)
    return 15; /* not reached: refused above */
  else if constexpr (CODES)
    return 12; /* not reached: the guard above admits LDS-sized bins only */
  else
    return launch_beyond_lds<V, L, OPS>(c);
}

/* run-time value -> compile-time tag visitors. f is a generic lambda; it
 * reads the type as `typename decltype(tag)::type` and a constant as
 * `decltype(tag)::value`. */
template <typename V> struct TypeTag { using type = V; };

/* value dtype; `bad` is returned for an unknown one */
template <typename F, typename R>
R with_vdtype(int vdtype, R bad, F&& f) {
  switch (vdtype) {
    case FH_F32: return f(TypeTag<float>{});
    case FH_F64: return f(TypeTag<double>{});
    case FH_I64: return f(TypeTag<int64_t>{});
    case FH_I32: return f(TypeTag<int32_t>{});
    default: return bad;
  }
}

/* op bits of the set; an unknown set is error 4. A launcher refuses the sets
 * it does not serve with `if constexpr` on the tag, so that no kernel is
 * instantiated for them. */
template <typename F>
int with_ops(int op_set, F&& f) {
  switch (op_set) {
#define FH_OPS_CASE(s) \
  case s: return f(std::integral_constant<int, set_bits(s)>{});
    FH_OPS_CASE(FH_SET_SUM_COUNT)
    FH_OPS_CASE(FH_SET_SUM_COUNT_PRESENT)
    FH_OPS_CASE(FH_SET_COUNT)
    FH_OPS_CASE(FH_SET_MIN_FULL)
    FH_OPS_CASE(FH_SET_MIN_COUNT)
    FH_OPS_CASE(FH_SET_MAX_FULL)
    FH_OPS_CASE(FH_SET_MAX_COUNT)
    FH_OPS_CASE(FH_SET_SSD)
    FH_OPS_CASE(FH_SET_PROD)
    FH_OPS_CASE(FH_SET_IDXMIN)
    FH_OPS_CASE(FH_SET_IDXMAX)
    FH_OPS_CASE(FH_SET_WELFORD)
    FH_OPS_CASE(FH_SET_ARGMIN_PAIR)
    FH_OPS_CASE(FH_SET_ARGMAX_PAIR)
    FH_OPS_CASE(FH_SET_SUMMARY)
    FH_OPS_CASE(FH_SET_ARGMIN_COLS)
    FH_OPS_CASE(FH_SET_ARGMAX_COLS)
#undef FH_OPS_CASE
    default: return 4;
  }
}

template <typename F>
int with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

template <typename V, typename L>
int dispatch_ops(fh_call* c) {
  return with_ops(c->op_set, [&](auto ops) -> int {
    constexpr int OPS = decltype(ops)::value;
    if constexpr ((OPS & B_WELFORD) != 0) {
      return 4; /* column path only */
    } else if constexpr ((OPS & B_ARGC) != 0) {
      return 18; /* column path only */
    } else if constexpr ((OPS & B_ARGROW) != 0) {
      if constexpr (CodeWidth<L>::value != 0)
        return 12; /* partition path only: no compact-code form */
      else if constexpr (sizeof(V) == 8)
        return launch_typed<V, L, OPS>(c);
      else
        return 11; /* 4-byte dtypes pack (enc32,row32) keys instead */
    } else {
      return launch_typed<V, L, OPS>(c);
    }
  });
}

template <typename V>
int dispatch_label(fh_call* c) {
  switch (c->ldtype) {
    case FH_L_I64: return dispatch_ops<V, int64_t>(c);
    case FH_L_I32: return dispatch_ops<V, int32_t>(c);
    case FH_L_U16: return dispatch_ops<V, uint16_t>(c);
    case FH_L_P12: return dispatch_ops<V, PackedCodes<12>>(c);
    case FH_L_P14: return dispatch_ops<V, PackedCodes<14>>(c);
    default: return 5;
  }
}


/* launch geometry for the column path: vector width per thread, column
 * blocks, and how many row chunks to split into so the chip is filled
 * (~2048 workgroups) when the column count alone is too small */
/* columns per thread of the summary set, by value size. Its per-column state
 * is 12-14 VGPRs against the 3-5 of every other set, so it does not simply
 * take their widths (profiles/r07_cols_summary.md has the resource report and
 * the measured A/B between the candidates). */
#ifndef FH_COLS_SUMMARY_VC4B
#define FH_COLS_SUMMARY_VC4B 4
#endif
#ifndef FH_COLS_SUMMARY_VC8B
#define FH_COLS_SUMMARY_VC8B 2
#endif
template <typename V>
constexpr int COLS_SUMMARY_VC = sizeof(V) == 4 ? FH_COLS_SUMMARY_VC4B : FH_COLS_SUMMARY_VC8B;
/* columns per thread of the row-valued sets (k_order_cols), by value size:
 * the arg sets keep 4 (4-byte) or 5 (8-byte) VGPRs per column, the index
 * sets 2. 4-byte dtypes take one 16-B vector, not k_reduce_cols' two: 8
 * columns measured 12 % slower for the arg sets (85 against 65 VGPRs) and
 * 5 % slower for the index sets (profiles/r08_cols_order.md has the resource
 * report and the measurement) */
#ifndef FH_COLS_ORDER_VC4B
#define FH_COLS_ORDER_VC4B 4
#endif
#ifndef FH_COLS_ORDER_VC8B
#define FH_COLS_ORDER_VC8B 2
#endif
template <typename V>
constexpr int COLS_ORDER_VC = sizeof(V) == 4 ? FH_COLS_ORDER_VC4B : FH_COLS_ORDER_VC8B;

struct ColsPlan {
  int vc;
  int64_t ncolblk;
  int nchunks;
  int64_t chunk_rows;
  BinLayout lay;  /* per-chunk slab layout over ngroups*m bins */
};

template <typename V>
ColsPlan cols_plan(const fh_call* c) {
  ColsPlan p{};
  p.vc = Traits<V>::VEC;
  /* 4-byte dtypes: 8 columns per thread (two 16-B vectors) amortizes the
   * per-row LDS reads, segment compare and address arithmetic further */
  if (sizeof(V) == 4 && c->ldm % 8 == 0 && c->m >= 8 &&
      ((uintptr_t)c->values % 32) == 0)
    p.vc = 8;
  if (c->ldm % p.vc != 0 || ((uintptr_t)c->values % 16) != 0) p.vc = 1;
  if (set_bits(c->op_set) & B_MOM2) {
    /* narrower loads are aligned wherever wider ones are */
    p.vc = p.vc >= COLS_SUMMARY_VC<V> ? COLS_SUMMARY_VC<V> : 1;
  }
  if ((set_bits(c->op_set) & B_ORDERC) && p.vc > COLS_ORDER_VC<V>) p.vc = COLS_ORDER_VC<V>;
  p.ncolblk = (c->m + (int64_t)COLS_BLOCK * p.vc - 1) / ((int64_t)COLS_BLOCK * p.vc);
  if (p.ncolblk == 0) p.ncolblk = 1;
  int want = (int)((2048 + p.ncolblk - 1) / p.ncolblk);
  if (want < 1) want = 1;
  if (want > 64) want = 64;
  p.lay = bin_layout<V>(set_bits(c->op_set), c->ngroups * c->m, 4);
  /* cap slab at 2 GiB */
  while (want > 1 && (int64_t)want * p.lay.bytes > (int64_t)2 << 30) want--;
  if ((int64_t)want * COLS_TTILE > c->n) want = (int)((c->n + COLS_TTILE - 1) / COLS_TTILE);
  if (want < 1) want = 1;
  p.nchunks = want;
  p.chunk_rows = (c->n + p.nchunks - 1) / p.nchunks;
  return p;
}

/* init + decode shared with the atomic path, bins sized ngroups*m */
template <typename V, int OPS>
int launch_cols(fh_call* c) {
  hipStream_t stream = (hipStream_t)c->stream;
  const int64_t nbins = c->ngroups * c->m;
  ColsPlan plan = cols_plan<V>(c);
  const bool aligned_chunks = c->chunk_offsets != nullptr && c->nchunks > 0;
  if (aligned_chunks) plan.nchunks = (int)c->nchunks;
  const bool slab_mode = !aligned_chunks && plan.nchunks > 1;
  const int skipnan = (c->flags & FH_SKIPNAN) ? 1 : 0;

  if (slab_mode) {
    if ((int64_t)plan.nchunks * plan.lay.bytes > c->scratch_bytes) return 3;
    /* identity-fill every chunk's slab sections (bins no segment touches) */
    for (int ch = 0; ch < plan.nchunks; ++ch) {
      char* s = (char*)c->scratch + (int64_t)ch * plan.lay.bytes;
      FH_TRY((init_bins<V, OPS>(slab_bins(s, plan.lay), nbins, stream)));
    }
  } else {
    FH_TRY((init_bins<V, OPS>(out_bins(c), nbins, stream)));
  }

  dim3 grid((uint32_t)plan.ncolblk, (uint32_t)plan.nchunks);
  const int64_t* offs = aligned_chunks ? (const int64_t*)c->chunk_offsets : nullptr;
  auto launch = [&](auto vc, auto slab, auto skip) -> int {
    auto kern = k_reduce_cols<V, OPS, decltype(vc)::value, decltype(slab)::value,
                              decltype(skip)::value>;
    hipLaunchKernelGGL(kern, grid, dim3(COLS_BLOCK), 0, stream,
                       (const V*)c->values, (const int*)c->labels,
                       (const int*)c->perm, c->n, c->m, c->ldm, c->ngroups,
                       c->means, skipnan, plan.chunk_rows, offs,
                       (char*)c->scratch, plan.lay, c->out_sum, c->out_count,
                       c->out_present, c->out_min, c->out_max, c->out_nanflag,
                       (double*)c->out_ssd);
    FH_CHECK(hipGetLastError());
    return 0;
  };
  /* columns per thread: 8 (4-byte dtypes only), the dtype's 16-B vector, 1 */
  auto with_vc = [&](auto f) -> int {
    if constexpr ((OPS & B_MOM2) != 0) {
      return plan.vc > 1 ? f(std::integral_constant<int, COLS_SUMMARY_VC<V>>{})
                         : f(std::integral_constant<int, 1>{});
    } else {
      if constexpr (sizeof(V) == 4) {
        if (plan.vc == 8) return f(std::integral_constant<int, 8>{});
      }
      return plan.vc > 1 ? f(std::integral_constant<int, Traits<V>::VEC>{})
                         : f(std::integral_constant<int, 1>{});
    }
  };
  FH_TRY(with_vc([&](auto vc) {
    return with_bool(slab_mode, [&](auto slab) {
      /* the summary set has the skipping form only: NaN rows mark nanflag */
      if constexpr ((OPS & B_MOM2) != 0)
        return launch(vc, slab, std::true_type{});
      else
        return with_bool(skipnan != 0, [&](auto skip) { return launch(vc, slab, skip); });
    });
  }));

  if (slab_mode) {
    /* fold the chunk partials; k_combine decodes min/max (gridDim.y==1) */
    hipLaunchKernelGGL((k_combine<V, OPS>), dim3(grid_for(nbins), 1), dim3(256),
                       0, stream, (const char*)c->scratch, plan.nchunks, nbins,
                       plan.lay, c->out_sum, c->out_count, c->out_present,
                       c->out_min, c->out_max, c->out_nanflag,
                       (double*)c->out_ssd);
    FH_CHECK(hipGetLastError());
  } else {
    FH_TRY((launch_decode<V, OPS>(c, nbins, stream)));
  }
  c->path_used = 3;
  return 0;
}

/* the row-valued sets: same plan, init, chunking and combine as launch_cols,
 * k_order_cols in place of k_reduce_cols */
template <typename V, int OPS>
int launch_order_cols(fh_call* c) {
  hipStream_t stream = (hipStream_t)c->stream;
  const int64_t nbins = c->ngroups * c->m;
  ColsPlan plan = cols_plan<V>(c);
  const bool aligned_chunks = c->chunk_offsets != nullptr && c->nchunks > 0;
  if (aligned_chunks) plan.nchunks = (int)c->nchunks;
  const bool slab_mode = !aligned_chunks && plan.nchunks > 1;
  const bool skipnan = (c->flags & FH_SKIPNAN) != 0;

  if (slab_mode) {
    if ((int64_t)plan.nchunks * plan.lay.bytes > c->scratch_bytes) return 3;
    for (int ch = 0; ch < plan.nchunks; ++ch) {
      char* s = (char*)c->scratch + (int64_t)ch * plan.lay.bytes;
      FH_TRY((init_bins<V, OPS>(slab_bins(s, plan.lay), nbins, stream)));
    }
  } else {
    FH_TRY((init_bins<V, OPS>(out_bins(c), nbins, stream)));
  }

  dim3 grid((uint32_t)plan.ncolblk, (uint32_t)plan.nchunks);
  const int64_t* offs = aligned_chunks ? (const int64_t*)c->chunk_offsets : nullptr;
  auto launch = [&](auto vc, auto slab, auto skip) -> int {
    auto kern = k_order_cols<V, OPS, decltype(vc)::value, decltype(slab)::value,
                             decltype(skip)::value>;
    hipLaunchKernelGGL(kern, grid, dim3(COLS_BLOCK), 0, stream,
                       (const V*)c->values, (const int*)c->labels,
                       (const int*)c->perm, c->n, c->m, c->ldm, c->row_offset,
                       plan.chunk_rows, offs, (char*)c->scratch, plan.lay,
                       (int64_t*)c->out_sum, c->out_count, c->out_present,
                       c->out_nanflag);
    FH_CHECK(hipGetLastError());
    return 0;
  };
  /* columns per thread: COLS_ORDER_VC, the dtype's 16-B vector below it, 1 */
  auto with_vc = [&](auto f) -> int {
    if (plan.vc == COLS_ORDER_VC<V>) return f(std::integral_constant<int, COLS_ORDER_VC<V>>{});
    if constexpr (COLS_ORDER_VC<V> != Traits<V>::VEC) {
      if (plan.vc == Traits<V>::VEC) return f(std::integral_constant<int, Traits<V>::VEC>{});
    }
    return f(std::integral_constant<int, 1>{});
  };
  FH_TRY(with_vc([&](auto vc) {
    return with_bool(slab_mode, [&](auto slab) {
      return with_bool(skipnan, [&](auto skip) { return launch(vc, slab, skip); });
    });
  }));

  if (slab_mode) {
    hipLaunchKernelGGL((k_combine<V, OPS>), dim3(grid_for(nbins), 1), dim3(256),
                       0, stream, (const char*)c->scratch, plan.nchunks, nbins,
                       plan.lay, c->out_sum, c->out_count, c->out_present,
                       c->out_min, c->out_max, c->out_nanflag,
                       (double*)c->out_ssd);
    FH_CHECK(hipGetLastError());
  }
  c->path_used = 3;
  return 0;
}

/* whether fh_grouped_reduce_cols has a form of the set */
constexpr bool cols_serves(int bits) { return bits != 0 && !(bits & B_ARGROW); }

template <typename V>
int dispatch_cols_ops(fh_call* c) {
  return with_ops(c->op_set, [&](auto ops) -> int {
    constexpr int OPS = decltype(ops)::value;
    if constexpr (!cols_serves(OPS)) {
      return 4; /* no column form */
    } else if constexpr ((OPS & B_ORDERC) != 0) {
      if (c->target) return 19;
      if (!c->out_sum || !c->out_count || !c->out_present ||
          ((OPS & B_NANFLAG) && !c->out_nanflag))
        return 6;
      return launch_order_cols<V, OPS>(c);
    } else if constexpr ((OPS & B_MOM2) != 0) {
      if (!c->out_ssd) return 16;
      if (!c->out_sum || !c->out_count || !c->out_present || !c->out_min ||
          !c->out_max || !c->out_nanflag)
        return 6;
      return launch_cols<V, OPS>(c);
    } else {
      return launch_cols<V, OPS>(c);
    }
  });
}

}  // namespace

/* pack (order-preserving 32-bit value encoding, global row) into one int64
 * key whose grouped MIN is argmin/argmax with np.argmin's first-occurrence
 * tie-break — one 12 GB/1e9-row pass replacing ~10 torch elementwise passes.
 * ismax inverts the encoding; NaN rows take the smallest key (propagate: a
 * NaN wins, as np.argmax) or all-ones (skipnan: all-NaN groups land on the
 * empty-group sentinel INT64_MAX after the sign-flip). */
template <typename V>
__global__ void k_pack_argkeys(const V* __restrict__ v, int64_t n,
                               int64_t row_offset, int ismax, int skipnan,
                               int64_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    uint64_t row = (uint64_t)(i + row_offset);
    uint64_t key;
    if constexpr (std::is_same<V, float>::value) {
      const float x = v[i];
      if (x != x) {
        key = skipnan ? ~0ULL : row;
      } else {
        uint32_t u = __float_as_uint(x);
        uint32_t enc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        if (ismax) enc = ~enc;
        key = ((uint64_t)enc << 32) | row;
      }
    } else {
      uint32_t enc = (uint32_t)v[i] ^ 0x80000000u;
      if (ismax) enc = ~enc;
      key = ((uint64_t)enc << 32) | row;
    }
    out[i] = (int64_t)(key ^ (1ULL << 63));  /* i64 compare == u64 compare */
  }
}

/* rewrite uint16 codes (0xFFFF = no group) into W-bit tiles
 * (include/floxhip_codes.h): one wave per tile, grid-stride over tiles. Rows
 * past n take the sentinel, so every slot of the last tile is defined. */
template <int W>
__launch_bounds__(256) __global__ void k_pack_codes(
    const uint16_t* __restrict__ u16, int64_t n, char* __restrict__ out) {
  constexpr uint32_t NONE = (1u << W) - 1u;
  const int lane = threadIdx.x & (FH_TILE_LANES - 1);
  const int64_t nwaves = (int64_t)gridDim.x * blockDim.x / FH_TILE_LANES;
  const int64_t ntiles = (n + FH_TILE_ROWS - 1) / FH_TILE_ROWS;
  for (int64_t tile = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / FH_TILE_LANES;
       tile < ntiles; tile += nwaves) {
    uint32_t code[FH_LANE_SLOTS];
    if ((tile + 1) * FH_TILE_ROWS <= n) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const Vec<uint16_t, 4> cv = *reinterpret_cast<const Vec<uint16_t, 4>*>(
            u16 + fh_tile_row(tile, lane, 4 * j));
#pragma unroll
        for (int k = 0; k < 4; ++k) code[4 * j + k] = cv.v[k];
      }
    } else {
#pragma unroll
      for (int s = 0; s < FH_LANE_SLOTS; ++s) {
        const int64_t row = fh_tile_row(tile, lane, s);
        code[s] = row < n ? (uint32_t)u16[row] : NONE;
      }
    }
#pragma unroll
    for (int s = 0; s < FH_LANE_SLOTS; ++s)
      if (code[s] >= NONE) code[s] = NONE;
    uint32_t cw[W / 2];
    fh_pack16<W>(code, cw);
    char* t = out + tile * (FH_TILE_ROWS / 8 * W);
    *reinterpret_cast<Vec<uint32_t, 4>*>(t + lane * 16) =
        Vec<uint32_t, 4>{{cw[0], cw[1], cw[2], cw[3]}};
    *reinterpret_cast<Vec<uint32_t, 2>*>(t + FH_PLANE8_OFF + lane * 8) =
        Vec<uint32_t, 2>{{cw[4], cw[5]}};
    if constexpr (W == 14)
      *reinterpret_cast<uint32_t*>(t + FH_PLANE4_OFF + lane * 4) = cw[6];
  }
}

extern "C" {

int64_t fh_scratch_bytes(const fh_call* c) {
  return with_vdtype(c->vdtype, (int64_t)-1, [&](auto t) -> int64_t {
    using V = typename decltype(t)::type;
    const int bits = set_bits(c->op_set);
    const LdsPlan lp = lds_plan<V>(bits, c->ngroups);
    if (bits & B_MOM2) {
      /* a call that would be refused needs no scratch. 1-D: LDS-binned
       * path or nothing (error 15), never a partition plan. Column form
       * (m > 0): error 16 without out_ssd; otherwise its slab is sized
       * below like any other set's */
      if (c->m > 0 ? !c->out_ssd : !lp.fits) return 0;
    }
    if (c->m > 0) {
      if (c->chunk_offsets) return 0; /* group-aligned chunks write directly */
      /* column path: per-chunk slab when the row range is split */
      const ColsPlan p = cols_plan<V>(c);
      return p.nchunks > 1 ? (int64_t)p.nchunks * p.lay.bytes : 0;
    }
    if (!lp.fits && !(c->flags & FH_FORCE_LDS)) {
      if (c->flags & FH_FORCE_ATOMIC) return 0;
      /* partition path wants the pairs buffer + bucket directory */
      const PartPlan p = part_plan<V>(c);
      return p.feasible ? p.bytes : 0;
    }
    return (int64_t)NUM_CU * lp.blocks_per_cu * lp.lay.bytes;
  });
}

int fh_query_path(const fh_call* c) {
  if (!c) return -1;
  const int bits = set_bits(c->op_set);
  if (!bits) return -1;
  return with_vdtype(c->vdtype, -1, [&](auto t) -> int {
    using V = typename decltype(t)::type;
    /* arg-pair sets never bin in LDS, FORCE_ATOMIC wins over size,
     * everything else is decided by the bins fitting */
    if ((bits & B_ARGROW) || (c->flags & FH_FORCE_ATOMIC)) return 0;
    return lds_plan<V>(bits, c->ngroups).fits ? 1 : 0;
  });
}

int fh_grouped_reduce(fh_call* c) {
  if (!c || !c->values || !c->labels) return 6;
  if (c->labels2 && c->g0 * c->g1 != c->ngroups) return 7;
  if (c->op_set == FH_SET_SSD && !c->means) return 8;
  if (set_bits(c->op_set) & B_ARGC) return 18;
  return with_vdtype(c->vdtype, 9, [&](auto t) {
    return dispatch_label<typename decltype(t)::type>(c);
  });
}

int fh_cols_supports(int op_set) { return cols_serves(set_bits(op_set)) ? 1 : 0; }


int fh_grouped_reduce_cols(fh_call* c) {
  /* column path: values (n_t rows x m columns, column stride 1, row stride
   * ldm); labels = group codes pre-sorted ascending (int32), perm = the
   * argsort permutation (int32) such that codes_sorted[i] = codes[perm[i]].
   * Outputs are (ngroups, m) group-major. */
  if (!c || !c->values || !c->labels || !c->perm) return 6;
  if (c->finish) return 14;
  if (c->op_set == FH_SET_SSD && !c->means) return 8;
  return with_vdtype(c->vdtype, 9, [&](auto t) {
    return dispatch_cols_ops<typename decltype(t)::type>(c);
  });
}

int fh_pack_argkeys(const void* values, int vdtype, int64_t n,
                    int64_t row_offset, int ismax, int skipnan, void* out,
                    void* stream) {
  if (!values || !out || n < 0) return 6;
  if (n + row_offset >= (1LL << 32)) return 10; /* row must fit 32 bits */
  return with_vdtype(vdtype, 9, [&](auto t) -> int {
    using V = typename decltype(t)::type;
    if constexpr (sizeof(V) == 4) {
      hipLaunchKernelGGL(k_pack_argkeys<V>, dim3(capped_grid(n, 256, 8192)),
                         dim3(256), 0, (hipStream_t)stream, (const V*)values, n,
                         row_offset, ismax, skipnan, (int64_t*)out);
      FH_CHECK(hipGetLastError());
      return 0;
    } else {
      return 9; /* 8-byte dtypes take the pair-payload sets instead */
    }
  });
}

int64_t fh_packed_code_bytes(int64_t n, int width) {
  return fh_packed_bytes(n, width);
}

int fh_pack_codes(const void* u16, int64_t n, int width, void* out,
                  void* stream) {
  if (!u16 || !out || n < 0) return 6;
  if (width != 12 && width != 14) return 17;
  if (n == 0) return 0;
  const int64_t ntiles = (n + FH_TILE_ROWS - 1) / FH_TILE_ROWS;
  /* 4 waves (tiles) per block */
  const dim3 grid(capped_grid(ntiles * FH_TILE_LANES, 256, 8192));
  if (width == 12)
    hipLaunchKernelGGL(k_pack_codes<12>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)u16, n, (char*)out);
  else
    hipLaunchKernelGGL(k_pack_codes<14>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)u16, n, (char*)out);
  FH_CHECK(hipGetLastError());
  return 0;
}

const char* fh_error_string(int code) {
  switch (code) {
    case 0: return "ok";
    case 2: return "FH_FORCE_LDS but bins exceed LDS capacity";
    case 3: return "scratch buffer too small (call fh_scratch_bytes)";
    case 4: return "unknown op_set";
    case 5: return "unknown label dtype";
    case 6: return "null values/labels pointer, or a missing output buffer of FH_SET_SUMMARY or of a row-valued set on the column path";
    case 7: return "labels2 given but g0*g1 != ngroups";
    case 8: return "FH_SET_SSD requires means";
    case 9: return "unknown value dtype";
    case 11: return "arg-pair reduction needs the bucket-partition path (8-byte dtype, n < 2^31, ngroups <= 2^24)";
    case 12: return "code labels (uint16 or packed) are valid on the LDS-binned path only (single code stream, bins within LDS, ngroups below the all-ones code of the width; see fh_query_path)";
    case 13: return "emit_codes needs the LDS-binned path and ngroups < 65535";
    case 14: return "finish mode needs the LDS-binned path, the op set it finishes (mean: SUM_COUNT, sum: SUM_COUNT_PRESENT, count: COUNT) and an f32/f64/i64 result buffer (see fh_query_path)";
    case 15: return "fh_grouped_reduce serves FH_SET_SUMMARY on the LDS-binned path only (bins within LDS, no FH_FORCE_ATOMIC; see fh_query_path)";
    case 16: return "FH_SET_SUMMARY requires out_ssd";
    case 17: return "packed code width must be 12 or 14";
    case 18: return "FH_SET_ARGMIN_COLS/FH_SET_ARGMAX_COLS exist on the column path only (fh_grouped_reduce_cols; see fh_cols_supports)";
    case 19: return "fh_grouped_reduce_cols takes no target: FH_SET_IDXMIN/IDXMAX there keep every (non-NaN under FH_SKIPNAN) row as a candidate";
    default: return code >= 1000 ? hipGetErrorString((hipError_t)(code - 1000)) : "unknown error";
  }
}

int fh_version(void) { return 1; }
int fh_abi_revision(void) { return 6; }

}  /* extern "C" */
