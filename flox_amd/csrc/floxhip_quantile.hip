/* floxhip — sorted-quantile family (quantile/nanquantile/median/nanmedian).
 *
 * The GPU analogue of the reference's group-aware quantile
 * (flox/aggregate_flox.py:50-130): instead of the complex-number partition
 * trick, rows are radix-sorted by the packed key (group code, encoded
 * value) so every group's values lie ascending in one contiguous run, with
 * NaNs (canonicalized) at the run's tail; a segmented kernel then
 * binary-searches each group's run boundaries + NaN boundary and computes
 * numpy's method="linear" interpolation (reference _lerp,
 * aggregate_flox.py:26-47).
 *
 * f32/i32 values: ONE keys-only 64-bit radix sort (code<<32 | enc32(v)).
 * f64/i64 values: sort by enc64(v) carrying the code, then a stable 32-bit
 * sort by code carrying enc64(v).
 * Sorts are rocprim::radix_sort_{keys,pairs} (device-wide LSD radix).
 */

#include <hip/hip_runtime.h>
#include <cstring>
#include <cstdint>
#include <rocprim/rocprim.hpp>

#include "../../include/floxhip.h"
#include "../../include/floxhip_qcols.h"
#include "../../include/floxhip_selcols.h"

#define FHQ_CHECK(x)                                \
  do {                                              \
    hipError_t _e = (x);                            \
    if (_e != hipSuccess) return (int)_e + 1000;    \
  } while (0)

namespace {

constexpr uint32_t INVALID_CODE = 0xFFFFFFFFu;

/* order-preserving encodings with a single canonical NaN that sorts last */
__device__ __forceinline__ uint32_t enc32f(float v) {
  if (v != v) return 0xFFFFFFFFu; /* canonical NaN: after every real/inf */
  uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec32f(uint32_t u) {
  if (u == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  uint32_t r = (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u;
  return __uint_as_float(r);
}
__device__ __forceinline__ uint32_t enc32i(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
__device__ __forceinline__ int32_t dec32i(uint32_t u) { return (int32_t)(u ^ 0x80000000u); }

__device__ __forceinline__ uint64_t enc64f(double v) {
  if (v != v) return ~0ull;
  uint64_t u = __double_as_longlong(v);
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dec64f(uint64_t u) {
  if (u == ~0ull) return __longlong_as_double(0x7FF8000000000000ll);
  uint64_t r = (u & 0x8000000000000000ull) ? (u ^ 0x8000000000000000ull) : ~u;
  return __longlong_as_double((long long)r);
}
__device__ __forceinline__ uint64_t enc64i(int64_t v) {
  return (uint64_t)v ^ 0x8000000000000000ull;
}
__device__ __forceinline__ int64_t dec64i(uint64_t u) {
  return (int64_t)(u ^ 0x8000000000000000ull);
}

__device__ __forceinline__ int64_t qcode_of(int64_t l0, int64_t l1, bool twolab,
                                            int64_t g0, int64_t g1, int64_t ngroups) {
  if (twolab) {
    if ((uint64_t)l0 >= (uint64_t)g0 || (uint64_t)l1 >= (uint64_t)g1) return -1;
    return l0 * g1 + l1;
  }
  return ((uint64_t)l0 >= (uint64_t)ngroups) ? -1 : l0;
}

/* pack (code, value) into one u64 key (4-byte value dtypes) */
template <typename V, typename L>
__global__ void k_qpack32(const V* __restrict__ values, const L* __restrict__ labels,
                          const L* __restrict__ labels2, int64_t n, int64_t ngroups,
                          int64_t g0, int64_t g1, uint64_t* __restrict__ keys) {
  const bool twolab = labels2 != nullptr;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t code = qcode_of((int64_t)labels[i], twolab ? (int64_t)labels2[i] : 0,
                                  twolab, g0, g1, ngroups);
    uint32_t e;
    if (std::is_same<V, float>::value)
      e = enc32f((float)values[i]);
    else
      e = enc32i((int32_t)values[i]);
    keys[i] = (code < 0) ? ~0ull : (((uint64_t)(uint32_t)code) << 32) | e;
  }
}

/* 8-byte value dtypes: encoded value + separate code array */
template <typename V, typename L>
__global__ void k_qpack64(const V* __restrict__ values, const L* __restrict__ labels,
                          const L* __restrict__ labels2, int64_t n, int64_t ngroups,
                          int64_t g0, int64_t g1, uint64_t* __restrict__ enc,
                          uint32_t* __restrict__ codes) {
  const bool twolab = labels2 != nullptr;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t code = qcode_of((int64_t)labels[i], twolab ? (int64_t)labels2[i] : 0,
                                  twolab, g0, g1, ngroups);
    if (std::is_same<V, double>::value)
      enc[i] = enc64f((double)values[i]);
    else
      enc[i] = enc64i((int64_t)values[i]);
    codes[i] = (code < 0) ? INVALID_CODE : (uint32_t)code;
  }
}

/* per-group run boundaries by binary search over the sorted codes */
template <bool PACKED>
__global__ void k_qoffsets(const uint64_t* __restrict__ keys,
                           const uint32_t* __restrict__ codes, int64_t n,
                           int64_t ngroups, int64_t* __restrict__ off) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g > ngroups) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const uint32_t c = PACKED ? (uint32_t)(keys[mid] >> 32) : codes[mid];
    if ((int64_t)c < g)
      lo = mid + 1;
    else
      hi = mid;
  }
  off[g] = lo;
}

/* ---- selection rules over one group's ascending keys ---------------------
 * Shared by the 1-D kernels (keys in global memory after the radix sort) and
 * the column kernel (keys in LDS after the bitonic sort). `key_at(k)` returns
 * the encoded value at position k of the group's run, 0 <= k < full: the
 * enc32 / enc64 form of the value alone, without the group code. */
template <typename V>
using qkey_t = typename std::conditional<sizeof(V) == 4, uint32_t, uint64_t>::type;

template <typename V>
constexpr bool is_float_v = std::is_same<V, float>::value || std::is_same<V, double>::value;

template <typename V>
__device__ __forceinline__ qkey_t<V> enc_key(V v) {
  if constexpr (std::is_same<V, float>::value) return enc32f(v);
  else if constexpr (std::is_same<V, int32_t>::value) return enc32i(v);
  else if constexpr (std::is_same<V, double>::value) return enc64f(v);
  else return enc64i(v);
}
template <typename V>
__device__ __forceinline__ V dec_key(qkey_t<V> e) {
  if constexpr (std::is_same<V, float>::value) return dec32f(e);
  else if constexpr (std::is_same<V, int32_t>::value) return dec32i(e);
  else if constexpr (std::is_same<V, double>::value) return dec64f(e);
  else return dec64i(e);
}

/* rows before the first canonical NaN (they sort last within the run) */
template <typename V, typename KeyAt>
__device__ __forceinline__ int64_t sorted_nonnan(KeyAt key_at, int64_t full) {
  if (!is_float_v<V>) return full;
  const qkey_t<V> nan_key = ~(qkey_t<V>)0;
  int64_t lo = 0, hi = full;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (key_at(mid) < nan_key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

/* numpy method="linear" quantile; reference _lerp (aggregate_flox.py:26-47)
 * including the t>=0.5 form. NaN for an empty group, an all-NaN group, and a
 * NaN-containing group without skipna. actual = sorted_nonnan(key_at, full). */
/* the two positions quantile_of_sorted reads for `actual` > 0 non-NaN rows;
 * returns the virtual index q * (actual - 1) */
__device__ __forceinline__ double quantile_ranks(int64_t actual, double q, int64_t& lo_i,
                                                 int64_t& hi_i) {
  const double vi = q * (double)(actual - 1);
  lo_i = (int64_t)floor(vi);
  hi_i = (int64_t)ceil(vi);
  /* q in [0, 1] needs only the first and the last clamp; the other two
   * keep a q outside it inside the run */
  if (lo_i < 0) lo_i = 0;
  if (lo_i > actual - 1) lo_i = actual - 1;
  if (hi_i < 0) hi_i = 0;
  if (hi_i > actual - 1) hi_i = actual - 1;
  return vi;
}

template <typename V, typename KeyAt>
__device__ __forceinline__ double quantile_of_sorted(KeyAt key_at, int64_t full,
                                                     int64_t actual, double q, int skipna) {
  double res = __longlong_as_double(0x7FF8000000000000ll);
  if (full > 0) {
    const bool nanmask = actual != full;
    if (actual > 0 && (skipna || !nanmask)) {
      int64_t lo_i, hi_i;
      const double vi = quantile_ranks(actual, q, lo_i, hi_i);
      const double a = (double)dec_key<V>(key_at(lo_i));
      const double b = (double)dec_key<V>(key_at(hi_i));
      const double tq = vi - (double)lo_i;
      const double diff = b - a;
      res = (tq >= 0.5) ? (b - diff * (1.0 - tq)) : (a + diff * tq);
    }
  }
  return res;
}

/* mode: longest equal-value run in the sorted span; sorted order makes
 * scipy's tie rule (smallest of the modes) the first-found run.
 * nan_policy: "propagate" (mode) -> NaN result when NaNs are strictly the
 * most frequent value; "omit" (nanmode) -> NaN tail ignored (reference
 * aggregate_npg.py:185-215). Empty and all-NaN groups give NaN (0 for
 * integer dtypes): scipy omit warns and returns NaN; propagate's most-common
 * value IS NaN. */
template <typename V, typename KeyAt>
__device__ __forceinline__ V mode_of_sorted(KeyAt key_at, int64_t full, int64_t actual,
                                            int skipna) {
  const V nan_or_zero =
      is_float_v<V> ? (V)__longlong_as_double(0x7FF8000000000000ll) : (V)0;
  if (full <= 0 || actual == 0) return nan_or_zero;
  qkey_t<V> best = key_at(0), cur = best;
  int64_t best_n = 1, cur_n = 1;
  for (int64_t i = 1; i < actual; ++i) {
    const qkey_t<V> k = key_at(i);
    if (k == cur) {
      ++cur_n;
    } else {
      if (cur_n > best_n) {
        best = cur;
        best_n = cur_n;
      }
      cur = k;
      cur_n = 1;
    }
  }
  if (cur_n > best_n) {
    best = cur;
    best_n = cur_n;
  }
  /* scipy propagate counts NaNs as a value: a strictly-most-frequent NaN run
   * wins (ties resolve to the smallest, i.e. any non-NaN) */
  if (!skipna && (full - actual) > best_n) return nan_or_zero;
  return dec_key<V>(best);
}

template <typename V, bool PACKED>
__global__ void k_quantile(const uint64_t* __restrict__ keys, int64_t n,
                           const int64_t* __restrict__ off, int64_t ngroups,
                           const double* __restrict__ q, int nq, int skipna,
                           double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ngroups * nq) return;
  const int64_t g = t % ngroups;
  const int qi = (int)(t / ngroups);
  const int64_t start = off[g], full = off[g + 1] - start;
  /* a packed key carries the group code above the value: drop it */
  auto key_at = [&](int64_t k) { return (qkey_t<V>)keys[start + k]; };
  const int64_t actual = full > 0 ? sorted_nonnan<V>(key_at, full) : 0;
  out[(int64_t)qi * ngroups + g] = quantile_of_sorted<V>(key_at, full, actual, q[qi], skipna);
}

template <typename V, bool PACKED>
__global__ void k_mode(const uint64_t* __restrict__ keys, int64_t n,
                       const int64_t* __restrict__ off, int64_t ngroups,
                       int skipna, V* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngroups) return;
  const int64_t start = off[g], full = off[g + 1] - start;
  auto key_at = [&](int64_t k) { return (qkey_t<V>)keys[start + k]; };
  const int64_t actual = full > 0 ? sorted_nonnan<V>(key_at, full) : 0;
  out[g] = mode_of_sorted<V>(key_at, full, actual, skipna);
}

/* ---- column form: sort each group's segment in LDS ----------------------
 * One workgroup per (column tile, group); the tile index runs fastest, so
 * neighbouring workgroups read neighbouring pieces of the same rows. The
 * workgroup finds its segment of the sorted codes by binary search, stages
 * the segment's rows for C = 1 << logC columns as keys [row][column] in
 * dynamic LDS (lanes along columns: one row of the tile per request), sorts
 * every column with a bitonic network whose compare-exchange steps take
 * (pair, column) with the column fastest, and evaluates the rules above on
 * the sorted keys. The network is as wide as the next power of two above the
 * segment found, never wider than P; slots past the segment hold the
 * all-ones key, which sorts last (for floats it is the canonical NaN, for
 * integers the dtype's maximum: either way positions below the segment's
 * length hold the segment's own values). A segment longer than P rows is cut
 * at P: memory-safe, that group's result is unspecified.
 * MODE folds -0.0 into +0.0 while staging (scipy counts by numeric
 * equality; the two encodings differ). */
template <typename V, bool MODE>
__global__ __launch_bounds__(1024) void k_sortsel_cols(
    const V* __restrict__ values, const int32_t* __restrict__ codes,
    const int32_t* __restrict__ perm, int64_t n, int64_t m, int64_t ldm,
    int64_t ngroups, int64_t g_base, int64_t ntiles, int P, int logC,
    const double* __restrict__ q, int nq, int skipna, void* __restrict__ out,
    int64_t* __restrict__ out_count) {
  using K = qkey_t<V>;
  extern __shared__ __align__(16) unsigned char qcols_lds[];
  K* s = reinterpret_cast<K*>(qcols_lds);
  const int C = 1 << logC;
  const int64_t g = g_base + (int64_t)blockIdx.x / ntiles;
  const int64_t c0 = ((int64_t)blockIdx.x % ntiles) << logC;
  if (g >= ngroups) return;
  const int tid = threadIdx.x, nthr = blockDim.x;

  /* segment [start, start + len) of code g; rows of code -1 sort first */
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)codes[mid] < g)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int64_t start = lo;
  hi = start + P < n ? start + P : n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)codes[mid] <= g)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int len = (int)(lo - start); /* <= P */
  int W = 1;
  while (W < len) W <<= 1; /* <= P: P is a power of two >= len */

  if (len > 0) {
    const int c = tid & (C - 1);
    const bool col_ok = c0 + c < m;
    const int rstep = nthr >> logC;
#pragma unroll 4
    for (int r = tid >> logC; r < W; r += rstep) {
      K key = ~(K)0;
      if (r < len && col_ok) {
        V v = values[(int64_t)perm[start + r] * ldm + c0 + c];
        if (MODE && is_float_v<V>) {
          if (v == (V)0) v = (V)0;
        }
        key = enc_key<V>(v);
      }
      s[(r << logC) + c] = key;
    }
    __syncthreads();
    const int npairs = (W >> 1) << logC;
    for (int k = 2; k <= W; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < npairs; t += nthr) {
          const int cc = t & (C - 1), pi = t >> logC;
          const int i = ((pi & ~(j - 1)) << 1) | (pi & (j - 1));
          const int ia = (i << logC) + cc, ib = ((i | j) << logC) + cc;
          const K a = s[ia], b = s[ib];
          if ((i & k) == 0 ? a > b : a < b) {
            s[ia] = b;
            s[ib] = a;
          }
        }
        __syncthreads();
      }
    }
  }

  const int nsel = MODE ? C : (nq << logC);
  for (int t = tid; t < nsel; t += nthr) {
    const int cc = t & (C - 1), qi = t >> logC;
    const int64_t col = c0 + cc;
    if (col >= m) continue;
    auto key_at = [&](int64_t k) { return s[((int)k << logC) + cc]; };
    const int64_t actual = len > 0 ? sorted_nonnan<V>(key_at, len) : 0;
    if (MODE)
      ((V*)out)[g * m + col] = mode_of_sorted<V>(key_at, len, actual, skipna);
    else
      ((double*)out)[((int64_t)qi * ngroups + g) * m + col] =
          quantile_of_sorted<V>(key_at, len, actual, q[qi], skipna);
    if (out_count && qi == 0) out_count[g * m + col] = actual;
  }
}

template <typename V, bool MODE>
int launch_sortsel_cols(fh_call* c, int nq, const fh_qcols_plan& pl) {
  auto kern = k_sortsel_cols<V, MODE>;
  if (pl.lds_bytes > 64 * 1024)
    FHQ_CHECK(hipFuncSetAttribute((const void*)kern,
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)pl.lds_bytes));
  const int64_t ntiles = (c->m + pl.C - 1) / pl.C;
  /* the grid is one-dimensional (no 65535 cap on groups): launch in slices
   * of groups where tiles x groups passes 2^31 - 1 */
  const int64_t gstep = std::max<int64_t>(1, (int64_t)0x7FFFFFFF / ntiles);
  for (int64_t g0 = 0; g0 < c->ngroups; g0 += gstep) {
    const int64_t ng = std::min<int64_t>(gstep, c->ngroups - g0);
    hipLaunchKernelGGL(kern, dim3((unsigned)(ng * ntiles)), dim3(pl.block),
                       (size_t)pl.lds_bytes, (hipStream_t)c->stream,
                       (const V*)c->values, (const int32_t*)c->labels,
                       (const int32_t*)c->perm, c->n, c->m, c->ldm, c->ngroups, g0,
                       ntiles, (int)pl.P, pl.logC, c->means, nq,
                       (c->flags & FH_SKIPNAN) ? 1 : 0, c->out_sum, c->out_count);
    FHQ_CHECK(hipGetLastError());
  }
  return 0;
}

template <typename V>
int run_quantile_cols(fh_call* c, int nq, int64_t max_seg_rows) {
  fh_qcols_plan pl;
  if (!fh_qcols_plan_for(max_seg_rows < 1 ? 1 : max_seg_rows, (int)sizeof(V), &pl)) return 20;
  c->path_used = 3;
  if (c->ngroups == 0 || c->m == 0) return 0;
  return nq == 0 ? launch_sortsel_cols<V, true>(c, nq, pl)
                 : launch_sortsel_cols<V, false>(c, nq, pl);
}

/* ---- column form for groups of any length: radix selection ---------------
 * Grid, segment search and row addressing as k_sortsel_cols (lanes along
 * columns, the workgroup's other threads stride the rows), but no row is
 * kept: every pass reads the segment again and counts one DB-bit digit of the
 * keys, most significant first, into LDS histograms [slot][bin][column]
 * (column fastest: the lanes of a wave hit distinct addresses). A slot is one
 * q: its key prefix so far and the rank that remains inside that prefix.
 * After a pass one thread per (slot, column) walks the slot's bins and
 * appends the bin its rank falls in. Pass 0 has the same (empty) prefix in
 * every slot, so one histogram serves them all; it also counts the canonical
 * NaN keys per column, so `actual` and with it the ranks floor(vi) / ceil(vi)
 * (quantile_ranks) are known before the first bin is chosen. The passes give
 * the key at floor(vi). Where some (slot, column) has ceil(vi) != floor(vi),
 * one more read counts the keys <= that key and finds the smallest key above
 * it: the key at floor(vi) + 1 is the same key when the count reaches
 * floor(vi) + 2, else that successor. quantile_of_sorted then runs on the
 * two keys. NaN keys are all ones, sort last and are never selected while a
 * rank is below `actual`. Counters are 32-bit: len <= n < 2^31. */
__device__ __forceinline__ void lds_min(uint32_t* p, uint32_t v) { atomicMin(p, v); }
__device__ __forceinline__ void lds_min(uint64_t* p, uint64_t v) {
  atomicMin(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

template <typename V>
__global__ __launch_bounds__(1024) void k_radixsel_cols(
    const V* __restrict__ values, const int32_t* __restrict__ codes,
    const int32_t* __restrict__ perm, int64_t n, int64_t m, int64_t ldm,
    int64_t ngroups, int64_t g_base, int64_t ntiles, int logC,
    const double* __restrict__ q, int nq, int skipna, double* __restrict__ out,
    int64_t* __restrict__ out_count) {
  using K = qkey_t<V>;
  constexpr int KB = (int)sizeof(K) * 8, DB = FH_SELCOLS_DIGIT_BITS, NB = 1 << DB;
  constexpr int NPASS = KB / DB, MAXS = FH_SELCOLS_MAX_SLOTS;
  constexpr K NAN_KEY = ~(K)0;
  extern __shared__ __align__(16) unsigned char selcols_lds[];
  const int C = 1 << logC;
  const int nsc = nq << logC; /* (slot, column) pairs: <= blockDim.x */
  uint32_t* hist = reinterpret_cast<uint32_t*>(selcols_lds); /* [nq][NB][C] */
  K* pref = reinterpret_cast<K*>(hist + (size_t)nsc * NB);   /* [nq][C] */
  K* succ = pref + nsc;                                       /* [nq][C] */
  uint32_t* rank = reinterpret_cast<uint32_t*>(succ + nsc);  /* [nq][C] */
  uint32_t* cle = rank + nsc;                                 /* [nq][C] */
  uint32_t* nanc = cle + nsc;                                 /* [C] */
  const int64_t g = g_base + (int64_t)blockIdx.x / ntiles;
  const int64_t c0 = ((int64_t)blockIdx.x % ntiles) << logC;
  if (g >= ngroups) return;
  const int tid = threadIdx.x, nthr = blockDim.x;

  /* segment [start, start + len) of code g; rows of code -1 sort first */
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)codes[mid] < g)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int64_t start = lo;
  hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)codes[mid] <= g)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int len = (int)(lo - start); /* < 2^31 */

  const int c = tid & (C - 1);
  const int64_t col = c0 + c;
  const bool col_ok = col < m;
  const int r0 = tid >> logC, rstep = nthr >> logC;
  /* this thread's (slot, column) where tid < nsc */
  const int my_s = tid >> logC;
  const bool owner = tid < nsc;
  const double my_q = owner ? q[my_s] : 0.0;
  int need = 0;

  if (len > 0) {
    if (owner) {
      pref[tid] = 0;
      succ[tid] = NAN_KEY;
      cle[tid] = 0;
    }
    if (tid < C) nanc[tid] = 0;
    for (int pass = 0; pass < NPASS; ++pass) {
      const int shift = KB - DB * (pass + 1);
      const int nh = (pass == 0 ? C : nsc) * NB;
      for (int t = tid; t < nh; t += nthr) hist[t] = 0;
      __syncthreads();
      if (col_ok) {
        if (pass == 0) {
          uint32_t my_nan = 0;
#pragma unroll 4
          for (int r = r0; r < len; r += rstep) {
            const K key = enc_key<V>(values[(int64_t)perm[start + r] * ldm + col]);
            if (is_float_v<V>) my_nan += key == NAN_KEY;
            atomicAdd(&hist[((int)(key >> shift) << logC) + c], 1u);
          }
          if (is_float_v<V> && my_nan) atomicAdd(&nanc[c], my_nan);
        } else {
          K top[MAXS];
#pragma unroll
          for (int s = 0; s < MAXS; ++s)
            top[s] = s < nq ? (K)(pref[(s << logC) + c] >> (shift + DB)) : (K)0;
#pragma unroll 4
          for (int r = r0; r < len; r += rstep) {
            const K key = enc_key<V>(values[(int64_t)perm[start + r] * ldm + col]);
            const int d = (int)((key >> shift) & (K)(NB - 1));
            const K ktop = key >> (shift + DB);
#pragma unroll
            for (int s = 0; s < MAXS; ++s)
              if (s < nq && ktop == top[s]) atomicAdd(&hist[((s * NB + d) << logC) + c], 1u);
          }
        }
      }
      __syncthreads();
      if (owner) {
        uint32_t rem;
        if (pass == 0) {
          const int64_t actual = (int64_t)len - (int64_t)nanc[c];
          int64_t lo_i = 0, hi_i = 0;
          if (actual > 0) quantile_ranks(actual, my_q, lo_i, hi_i);
          need = hi_i != lo_i;
          rem = (uint32_t)lo_i;
        } else {
          rem = rank[tid];
        }
        const uint32_t* h = hist + (((pass == 0 ? 0 : my_s) * NB) << logC) + c;
        uint32_t cum = 0, below = 0;
        int bin = 0;
#pragma unroll 8
        for (int b = 0; b < NB; ++b) {
          cum += h[b << logC];
          if (cum <= rem) {
            bin = b + 1;
            below = cum;
          }
        }
        /* a column past m has an empty histogram: keep the digit in range */
        if (bin > NB - 1) bin = NB - 1;
        pref[tid] |= (K)bin << shift;
        rank[tid] = rem - below;
      }
      __syncthreads();
    }
    if (__syncthreads_or(need)) {
      if (col_ok) {
        K sel[MAXS], mn[MAXS];
        uint32_t cn[MAXS];
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
          sel[s] = s < nq ? pref[(s << logC) + c] : NAN_KEY;
          mn[s] = NAN_KEY;
          cn[s] = 0;
        }
#pragma unroll 4
        for (int r = r0; r < len; r += rstep) {
          const K key = enc_key<V>(values[(int64_t)perm[start + r] * ldm + col]);
#pragma unroll
          for (int s = 0; s < MAXS; ++s)
            if (s < nq) {
              cn[s] += key <= sel[s];
              if (key > sel[s] && key < mn[s]) mn[s] = key;
            }
        }
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
          if (s < nq) {
            atomicAdd(&cle[(s << logC) + c], cn[s]);
            lds_min(&succ[(s << logC) + c], mn[s]);
          }
      }
      __syncthreads();
    }
  }

  if (owner && col_ok) {
    int64_t actual = 0, lo_i = 0, hi_i = 0;
    K klo = NAN_KEY, khi = NAN_KEY;
    if (len > 0) {
      actual = (int64_t)len - (int64_t)nanc[c];
      if (actual > 0) quantile_ranks(actual, my_q, lo_i, hi_i);
      klo = pref[tid];
      khi = (hi_i == lo_i || (int64_t)cle[tid] >= lo_i + 2) ? klo : succ[tid];
    }
    auto key_at = [=](int64_t k) { return k == lo_i ? klo : khi; };
    out[((int64_t)my_s * ngroups + g) * m + col] =
        quantile_of_sorted<V>(key_at, len, actual, my_q, skipna);
    if (out_count && my_s == 0) out_count[g * m + col] = actual;
  }
}

template <typename V>
int run_quantile_select_cols(fh_call* c, int nq) {
  c->path_used = 3;
  if (c->ngroups == 0 || c->m == 0) return 0;
  auto kern = k_radixsel_cols<V>;
  const int skipna = (c->flags & FH_SKIPNAN) ? 1 : 0;
  /* more q than one launch has slots for: batches of pl.slots */
  for (int b0 = 0; b0 < nq;) {
    fh_selcols_plan pl;
    if (!fh_selcols_plan_for(nq - b0, (int)sizeof(V), &pl)) return 22;
    const int nb = std::min(nq - b0, pl.slots);
    if (pl.lds_bytes > 64 * 1024)
      FHQ_CHECK(hipFuncSetAttribute((const void*)kern,
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)pl.lds_bytes));
    const int64_t ntiles = (c->m + pl.C - 1) / pl.C;
    /* one-dimensional grid, sliced in groups as launch_sortsel_cols does */
    const int64_t gstep = std::max<int64_t>(1, (int64_t)0x7FFFFFFF / ntiles);
    for (int64_t g0 = 0; g0 < c->ngroups; g0 += gstep) {
      const int64_t ng = std::min<int64_t>(gstep, c->ngroups - g0);
      hipLaunchKernelGGL(kern, dim3((unsigned)(ng * ntiles)), dim3(pl.block),
                         (size_t)pl.lds_bytes, (hipStream_t)c->stream,
                         (const V*)c->values, (const int32_t*)c->labels,
                         (const int32_t*)c->perm, c->n, c->m, c->ldm, c->ngroups, g0,
                         ntiles, pl.logC, c->means + b0, nb, skipna,
                         (double*)c->out_sum + (int64_t)b0 * c->ngroups * c->m,
                         b0 == 0 ? c->out_count : (int64_t*)nullptr);
      FHQ_CHECK(hipGetLastError());
    }
    b0 += nb;
  }
  return 0;
}

template <typename V, typename L>
int run_quantile(fh_call* c, const double* q_dev, int nq, double* out) {
  hipStream_t stream = (hipStream_t)c->stream;
  const int skipna = (c->flags & FH_SKIPNAN) ? 1 : 0;
  const int64_t n = c->n, ngroups = c->ngroups;
  char* scr = (char*)c->scratch;
  constexpr bool PACKED = sizeof(V) == 4;

  int64_t off0 = 0;
  auto carve = [&](int64_t b) {
    int64_t o = off0;
    off0 += ((b + 255) / 256) * 256;
    return o;
  };

  const int grid = (int)std::min<int64_t>((n + 255) / 256, 2048) + 1;
  if (PACKED) {
    uint64_t* kin = (uint64_t*)(scr + carve(n * 8));
    uint64_t* kout = (uint64_t*)(scr + carve(n * 8));
    int64_t* off = (int64_t*)(scr + carve((ngroups + 1) * 8));
    size_t temp_bytes = 0;
    (void)rocprim::radix_sort_keys(nullptr, temp_bytes, kin, kout, (size_t)n, 0, 64, stream);
    void* temp = scr + carve((int64_t)temp_bytes);
    if (off0 > c->scratch_bytes) return 3;
    hipLaunchKernelGGL((k_qpack32<V, L>), dim3(grid), dim3(256), 0, stream,
                       (const V*)c->values, (const L*)c->labels,
                       (const L*)c->labels2, n, ngroups, c->g0, c->g1, kin);
    FHQ_CHECK(hipGetLastError());
    FHQ_CHECK(rocprim::radix_sort_keys(temp, temp_bytes, kin, kout, (size_t)n, 0, 64, stream));
    int ob = (int)((ngroups + 1 + 255) / 256);
    hipLaunchKernelGGL((k_qoffsets<true>), dim3(ob), dim3(256), 0, stream, kout,
                       (const uint32_t*)nullptr, n, ngroups, off);
    FHQ_CHECK(hipGetLastError());
    if (nq == 0) { /* mode */
      int mb = (int)((ngroups + 255) / 256);
      hipLaunchKernelGGL((k_mode<V, true>), dim3(mb), dim3(256), 0, stream,
                         kout, n, off, ngroups, skipna, (V*)out);
      FHQ_CHECK(hipGetLastError());
      return 0;
    }
    int qb = (int)((ngroups * nq + 255) / 256);
    hipLaunchKernelGGL((k_quantile<V, true>), dim3(qb), dim3(256), 0, stream,
                       kout, n, off, ngroups, q_dev, nq, skipna, out);
    FHQ_CHECK(hipGetLastError());
    return 0;
  }

  uint64_t* e_in = (uint64_t*)(scr + carve(n * 8));
  uint64_t* e_out = (uint64_t*)(scr + carve(n * 8));
  uint32_t* c_in = (uint32_t*)(scr + carve(n * 4));
  uint32_t* c_out = (uint32_t*)(scr + carve(n * 4));
  int64_t* off = (int64_t*)(scr + carve((ngroups + 1) * 8));
  size_t t1 = 0, t2 = 0;
  (void)rocprim::radix_sort_pairs(nullptr, t1, e_in, e_out, c_in, c_out, (size_t)n, 0, 64, stream);
  (void)rocprim::radix_sort_pairs(nullptr, t2, c_out, c_in, e_out, e_in, (size_t)n, 0, 32, stream);
  void* temp = scr + carve((int64_t)std::max(t1, t2));
  if (off0 > c->scratch_bytes) return 3;
  hipLaunchKernelGGL((k_qpack64<V, L>), dim3(grid), dim3(256), 0, stream,
                     (const V*)c->values, (const L*)c->labels,
                     (const L*)c->labels2, n, ngroups, c->g0, c->g1, e_in, c_in);
  FHQ_CHECK(hipGetLastError());
  /* sort by encoded value, then stably by code: values ascend within runs */
  FHQ_CHECK(rocprim::radix_sort_pairs(temp, t1, e_in, e_out, c_in, c_out, (size_t)n, 0, 64, stream));
  FHQ_CHECK(rocprim::radix_sort_pairs(temp, t2, c_out, c_in, e_out, e_in, (size_t)n, 0, 32, stream));
  /* sorted codes now in c_in, matching encoded values in e_in */
  int ob = (int)((ngroups + 1 + 255) / 256);
  hipLaunchKernelGGL((k_qoffsets<false>), dim3(ob), dim3(256), 0, stream, e_in,
                     c_in, n, ngroups, off);
  FHQ_CHECK(hipGetLastError());
  if (nq == 0) { /* mode */
    int mb = (int)((ngroups + 255) / 256);
    hipLaunchKernelGGL((k_mode<V, false>), dim3(mb), dim3(256), 0, stream,
                       e_in, n, off, ngroups, skipna, (V*)out);
    FHQ_CHECK(hipGetLastError());
    return 0;
  }
  int qb = (int)((ngroups * nq + 255) / 256);
  hipLaunchKernelGGL((k_quantile<V, false>), dim3(qb), dim3(256), 0, stream,
                     e_in, n, off, ngroups, q_dev, nq, skipna, out);
  FHQ_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int64_t fh_quantile_scratch_bytes(const fh_call* c) {
  const int64_t n = c->n, ngroups = c->ngroups;
  size_t temp = 0;
  int64_t bytes = 0;
  auto al = [](int64_t b) { return ((b + 255) / 256) * 256; };
  if (c->vdtype == FH_F32 || c->vdtype == FH_I32) {
    (void)rocprim::radix_sort_keys(nullptr, temp, (const uint64_t*)nullptr,
                             (uint64_t*)nullptr, (size_t)n, 0, 64, 0);
    bytes = 2 * al(n * 8) + al((ngroups + 1) * 8) + al((int64_t)temp);
  } else {
    size_t t1 = 0, t2 = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t1, (const uint64_t*)nullptr,
                              (uint64_t*)nullptr, (const uint32_t*)nullptr,
                              (uint32_t*)nullptr, (size_t)n, 0, 64, 0);
    (void)rocprim::radix_sort_pairs(nullptr, t2, (const uint32_t*)nullptr,
                              (uint32_t*)nullptr, (const uint64_t*)nullptr,
                              (uint64_t*)nullptr, (size_t)n, 0, 32, 0);
    bytes = 2 * al(n * 8) + 2 * al(n * 4) + al((ngroups + 1) * 8) +
            al((int64_t)std::max(t1, t2));
  }
  return bytes;
}

/* grouped quantiles: `means` carries the device q array (f64[nq], smuggled
 * through the existing struct field), g0 (when labels2 is NULL) is unused,
 * out_sum receives f64[nq*ngroups] results (NaN for empty groups, all-NaN
 * groups under skipna, and NaN-containing groups without skipna) */
int fh_grouped_quantile(fh_call* c, int nq) {
  /* nq == 0: grouped mode — out_sum then holds value-dtype[ngroups] */
  if (!c || !c->values || !c->labels || !c->out_sum) return 6;
  if (nq > 0 && !c->means) return 6;
  const double* q_dev = c->means;
  double* out = (double*)c->out_sum;
  switch (c->vdtype) {
    case FH_F32:
      return c->ldtype == FH_L_I64 ? run_quantile<float, int64_t>(c, q_dev, nq, out)
                                   : run_quantile<float, int32_t>(c, q_dev, nq, out);
    case FH_F64:
      return c->ldtype == FH_L_I64 ? run_quantile<double, int64_t>(c, q_dev, nq, out)
                                   : run_quantile<double, int32_t>(c, q_dev, nq, out);
    case FH_I64:
      return c->ldtype == FH_L_I64 ? run_quantile<int64_t, int64_t>(c, q_dev, nq, out)
                                   : run_quantile<int64_t, int32_t>(c, q_dev, nq, out);
    case FH_I32:
      return c->ldtype == FH_L_I64 ? run_quantile<int32_t, int64_t>(c, q_dev, nq, out)
                                   : run_quantile<int32_t, int32_t>(c, q_dev, nq, out);
    default:
      return 9;
  }
}

/* column form (include/floxhip.h): sort each group's rows in LDS */
int64_t fh_quantile_cols_max_rows(int vdtype) {
  switch (vdtype) {
    case FH_F32:
    case FH_I32:
      return fh_qcols_capacity(4);
    case FH_F64:
    case FH_I64:
      return fh_qcols_capacity(8);
    default:
      return 0;
  }
}

int fh_grouped_quantile_cols(fh_call* c, int nq, int64_t max_seg_rows) {
  if (!c || !c->values || !c->labels || !c->perm || !c->out_sum) return 21;
  if (nq < 0 || (nq > 0 && !c->means)) return 21;
  if (c->n < 0 || c->m < 0 || c->ngroups < 0 || c->n >= (1LL << 31)) return 21;
  switch (c->vdtype) {
    case FH_F32: return run_quantile_cols<float>(c, nq, max_seg_rows);
    case FH_F64: return run_quantile_cols<double>(c, nq, max_seg_rows);
    case FH_I64: return run_quantile_cols<int64_t>(c, nq, max_seg_rows);
    case FH_I32: return run_quantile_cols<int32_t>(c, nq, max_seg_rows);
    default: return 9;
  }
}

/* column form for groups of any length (include/floxhip.h): radix selection */
int fh_grouped_quantile_select_cols(fh_call* c, int nq) {
  if (!c || !c->values || !c->labels || !c->perm || !c->out_sum || !c->means) return 22;
  if (nq < 1) return 22;
  if (c->n < 0 || c->m < 0 || c->ngroups < 0 || c->n >= (1LL << 31)) return 22;
  switch (c->vdtype) {
    case FH_F32: return run_quantile_select_cols<float>(c, nq);
    case FH_F64: return run_quantile_select_cols<double>(c, nq);
    case FH_I64: return run_quantile_select_cols<int64_t>(c, nq);
    case FH_I32: return run_quantile_select_cols<int32_t>(c, nq);
    default: return 9;
  }
}

}  /* extern "C" */
