/* floxhip — grouped scans (cumsum / nancumsum / ffill / bfill).
 *
 * Re-implements the reference's eager scan path (flox/scan.py:101-352
 * groupby_scan -> chunk_scan; flox/aggregate_flox.py:269-325 ffill /
 * _np_grouped_scan): rows are stably sorted by group code so each group is
 * one contiguous run IN ORIGINAL ROW ORDER, a device scan-by-key runs the
 * per-group recurrence, and results scatter back through the permutation.
 *
 * Ops: 0 = cumsum (NaN poisons the rest of its group, like np.cumsum),
 *      1 = nancumsum (NaN contributes 0, np.nancumsum),
 *      2 = ffill, 3 = bfill (carry last/next non-NaN within the group).
 * Rows whose labels fall outside the expected groups form their own
 * trailing group, exactly like the reference's NaN-sentinel group
 * (factorize.py:201-210).
 */

#include <hip/hip_runtime.h>
#include <cstring>
#include <cstdint>
#include <rocprim/rocprim.hpp>

#include "../../include/floxhip.h"
#include "../../include/floxhip_scanrows.h"

#define FHS_CHECK(x)                             \
  do {                                           \
    hipError_t _e = (x);                         \
    if (_e != hipSuccess) return (int)_e + 1000; \
  } while (0)

namespace {

enum { SCAN_CUMSUM = 0, SCAN_NANCUMSUM = 1, SCAN_FFILL = 2, SCAN_BFILL = 3 };

template <typename V>
struct FillPair {
  V v;
  int32_t valid;
};

template <typename V>
struct FillOp {
  __device__ FillPair<V> operator()(const FillPair<V>& a, const FillPair<V>& b) const {
    return b.valid ? b : a;
  }
};

template <typename V>
__device__ __forceinline__ bool snan(V v) {
  if (std::is_same<V, float>::value || std::is_same<V, double>::value) return v != v;
  return false;
}

template <typename L>
__global__ void k_spack(const L* __restrict__ labels, const L* __restrict__ labels2,
                        int64_t n, int64_t ngroups, int64_t g0, int64_t g1,
                        uint32_t* __restrict__ codes, uint32_t* __restrict__ idx) {
  const bool twolab = labels2 != nullptr;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int64_t code;
    const int64_t l0 = (int64_t)labels[i];
    if (twolab) {
      const int64_t l1 = (int64_t)labels2[i];
      code = ((uint64_t)l0 >= (uint64_t)g0 || (uint64_t)l1 >= (uint64_t)g1)
                 ? ngroups
                 : l0 * g1 + l1;
    } else {
      code = ((uint64_t)l0 >= (uint64_t)ngroups) ? ngroups : l0;
    }
    codes[i] = (uint32_t)code;
    idx[i] = (uint32_t)i;
  }
}

/* gather values into sorted order, building the scan input; perm == NULL
 * means the labels were already sorted (FH_SORTED_LABELS) and rows are
 * read in place */
template <typename V, int OP>
__global__ void k_sgather(const V* __restrict__ values, const uint32_t* __restrict__ perm,
                          int64_t n, V* __restrict__ sv, FillPair<V>* __restrict__ sp) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    /* bfill scans the reversed sequence */
    const int64_t j = (OP == SCAN_BFILL) ? (n - 1 - i) : i;
    const V v = values[perm ? (int64_t)perm[j] : j];
    if (OP == SCAN_CUMSUM) {
      sv[i] = v;
    } else if (OP == SCAN_NANCUMSUM) {
      sv[i] = snan(v) ? (V)0 : v;
    } else {
      sp[i].v = v;
      sp[i].valid = snan(v) ? 0 : 1;
    }
  }
}

template <int OP>
__global__ void k_skeys_rev(const uint32_t* __restrict__ codes_sorted, int64_t n,
                            uint32_t* __restrict__ rkeys) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    rkeys[i] = codes_sorted[n - 1 - i];
}

/* scatter results back to original row order */
template <typename V, int OP>
__global__ void k_sscatter(const V* __restrict__ sv, const FillPair<V>* __restrict__ sp,
                           const uint32_t* __restrict__ perm, int64_t n,
                           V* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const double NAN_ = __longlong_as_double(0x7FF8000000000000ll);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t j = (OP == SCAN_BFILL) ? (n - 1 - i) : i;
    const int64_t o = perm ? (int64_t)perm[j] : j;
    if (OP == SCAN_CUMSUM || OP == SCAN_NANCUMSUM) {
      out[o] = sv[i];
    } else {
      const FillPair<V> p = sp[i];
      out[o] = p.valid ? p.v : (V)NAN_; /* leading gap stays NaN */
    }
  }
}

template <typename V, typename L, int OP>
int run_scan(fh_call* c, V* out) {
  hipStream_t stream = (hipStream_t)c->stream;
  const int64_t n = c->n;
  char* scr = (char*)c->scratch;
  int64_t o = 0;
  auto carve = [&](int64_t b) {
    int64_t r = o;
    o += ((b + 255) / 256) * 256;
    return r;
  };
  uint32_t* codes = (uint32_t*)(scr + carve(n * 4));
  uint32_t* codes_s = (uint32_t*)(scr + carve(n * 4));
  uint32_t* idx = (uint32_t*)(scr + carve(n * 4));
  uint32_t* perm = (uint32_t*)(scr + carve(n * 4));
  constexpr bool IS_FILL = OP == SCAN_FFILL || OP == SCAN_BFILL;
  V* sv = nullptr;
  V* sv2 = nullptr;
  FillPair<V>* sp = nullptr;
  FillPair<V>* sp2 = nullptr;
  uint32_t* rkeys = nullptr;
  if (IS_FILL) {
    sp = (FillPair<V>*)(scr + carve(n * (int64_t)sizeof(FillPair<V>)));
    sp2 = (FillPair<V>*)(scr + carve(n * (int64_t)sizeof(FillPair<V>)));
  } else {
    sv = (V*)(scr + carve(n * (int64_t)sizeof(V)));
    sv2 = (V*)(scr + carve(n * (int64_t)sizeof(V)));
  }
  if (OP == SCAN_BFILL) rkeys = (uint32_t*)(scr + carve(n * 4));

  size_t ts = 0, tscan = 0;
  (void)rocprim::radix_sort_pairs(nullptr, ts, codes, codes_s, idx, perm, (size_t)n, 0, 32, stream);
  if (IS_FILL)
    (void)rocprim::inclusive_scan_by_key(nullptr, tscan, codes_s, sp, sp2, (size_t)n,
                                   FillOp<V>(), rocprim::equal_to<uint32_t>(), stream);
  else
    (void)rocprim::inclusive_scan_by_key(nullptr, tscan, codes_s, sv, sv2, (size_t)n,
                                   rocprim::plus<V>(), rocprim::equal_to<uint32_t>(), stream);
  void* temp = scr + carve((int64_t)std::max(ts, tscan));
  if (o > c->scratch_bytes) return 3;

  const int grid = (int)std::min<int64_t>((n + 255) / 256, 2048) + 1;
  const bool presorted = (c->flags & FH_SORTED_LABELS) != 0;
  if (presorted) {
    /* caller guarantees nondecreasing in-range labels (the reference's
     * issorted fast path, aggregate_flox.py:9-23): pack the u32 keys but
     * skip the radix sort, gather and scatter in place */
    hipLaunchKernelGGL((k_spack<L>), dim3(grid), dim3(256), 0, stream,
                       (const L*)c->labels, (const L*)c->labels2, n, c->ngroups,
                       c->g0, c->g1, codes_s, idx);
    FHS_CHECK(hipGetLastError());
    perm = nullptr;
  } else {
    hipLaunchKernelGGL((k_spack<L>), dim3(grid), dim3(256), 0, stream,
                       (const L*)c->labels, (const L*)c->labels2, n, c->ngroups,
                       c->g0, c->g1, codes, idx);
    FHS_CHECK(hipGetLastError());
    FHS_CHECK(rocprim::radix_sort_pairs(temp, ts, codes, codes_s, idx, perm,
                                        (size_t)n, 0, 32, stream));
  }
  hipLaunchKernelGGL((k_sgather<V, OP>), dim3(grid), dim3(256), 0, stream,
                     (const V*)c->values, perm, n, sv, sp);
  FHS_CHECK(hipGetLastError());
  const uint32_t* keys = codes_s;
  if (OP == SCAN_BFILL) {
    hipLaunchKernelGGL((k_skeys_rev<OP>), dim3(grid), dim3(256), 0, stream,
                       codes_s, n, rkeys);
    FHS_CHECK(hipGetLastError());
    keys = rkeys;
  }
  if (IS_FILL)
    FHS_CHECK(rocprim::inclusive_scan_by_key(temp, tscan, keys, sp, sp2, (size_t)n,
                                             FillOp<V>(), rocprim::equal_to<uint32_t>(), stream));
  else
    FHS_CHECK(rocprim::inclusive_scan_by_key(temp, tscan, keys, sv, sv2, (size_t)n,
                                             rocprim::plus<V>(), rocprim::equal_to<uint32_t>(), stream));
  hipLaunchKernelGGL((k_sscatter<V, OP>), dim3(grid), dim3(256), 0, stream, sv2,
                     sp2, perm, n, out);
  FHS_CHECK(hipGetLastError());
  return 0;
}

/* ---- column form: grouped scans over the leading axis --------------------
 * The walk of floxhip.hip's column kernels (rows in group order through the
 * stable sort's perm, code/perm tiles staged in LDS, lanes along columns, VC
 * columns per thread) with a store per element instead of a flush per group:
 * each thread keeps ONE running value per column in a register, restarts it
 * where the code changes, and writes it to out[perm[i] * ldo + c]. Every run
 * of equal codes is a segment, the -1 run included (the reference's
 * NaN-sentinel group, factorize.py:201-210). cur_g and acc live across the
 * staging tiles, so a segment may span any number of them. A workgroup owns
 * (column tile, chunk); a chunk is a whole number of segments, so no carry
 * crosses workgroups. bfill is ffill with the chunk walked from its last row
 * to its first. SCOLS_ROWS rows are loaded before the first of them is
 * consumed (values and out never alias), which keeps that many independent
 * loads in flight per thread. Addresses are row * ldm + c0 and row * ldo + c0
 * in 64 bits. */
constexpr int SCOLS_BLOCK = 256;
constexpr int SCOLS_TTILE = 2048; /* rows per staged tile, as COLS_TTILE */
#ifndef FH_SCOLS_ROWS
#define FH_SCOLS_ROWS 4
#endif
constexpr int SCOLS_ROWS = FH_SCOLS_ROWS;
/* columns per thread by value size: one 16-B vector, k_order_cols' caps */
#ifndef FH_SCOLS_VC4B
#define FH_SCOLS_VC4B 4
#endif
#ifndef FH_SCOLS_VC8B
#define FH_SCOLS_VC8B 2
#endif
template <typename V>
constexpr int SCOLS_VC = sizeof(V) == 4 ? FH_SCOLS_VC4B : FH_SCOLS_VC8B;

template <typename V, int N>
struct alignas(sizeof(V) * N) ScanVec {
  V v[N];
};

/* one row of one column: `first` marks a segment's first row in walk order.
 * The first row initialises the sums, so -0.0 survives as in np.cumsum;
 * int64 wraps (added as unsigned). */
template <typename V, int OP>
__device__ __forceinline__ V scan_step(V acc, V v, bool first) {
  if (OP == SCAN_FFILL || OP == SCAN_BFILL) return (first || !snan(v)) ? v : acc;
  const V x = (OP == SCAN_NANCUMSUM && snan(v)) ? (V)0 : v;
  if (first) return x;
  if (std::is_same<V, int64_t>::value) return (V)((uint64_t)acc + (uint64_t)x);
  return acc + x;
}

template <typename V, int OP, int VC>
__launch_bounds__(SCOLS_BLOCK) __global__ void k_scan_cols(
    const V* __restrict__ values, const int* __restrict__ codes_sorted,
    const int* __restrict__ perm, int64_t n_t, int64_t m, int64_t ldm, int64_t ldo,
    const int64_t* __restrict__ chunk_offs, V* __restrict__ out) {
  constexpr bool REV = OP == SCAN_BFILL;
  __shared__ int s_code[SCOLS_TTILE];
  __shared__ int s_perm[SCOLS_TTILE];

  const int64_t c0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * VC;
  const bool col_act = c0 < m;
  const bool full = c0 + VC <= m;
  int64_t t_begin = 0, t_end = n_t;
  if (chunk_offs) {
    t_begin = chunk_offs[blockIdx.y];
    t_end = chunk_offs[blockIdx.y + 1];
  }

  V acc[VC];
#pragma unroll
  for (int k = 0; k < VC; ++k) acc[k] = (V)0;
  int cur_g = INT32_MIN; /* no code: codes are >= -1 */

  const int64_t ntiles = (t_end - t_begin + SCOLS_TTILE - 1) / SCOLS_TTILE;
  for (int64_t tt = 0; tt < ntiles; ++tt) {
    const int64_t t0 = t_begin + (REV ? ntiles - 1 - tt : tt) * SCOLS_TTILE;
    const int nt = (int)((t_end - t0 < SCOLS_TTILE) ? (t_end - t0) : SCOLS_TTILE);
    __syncthreads();
    for (int i = threadIdx.x; i < nt; i += blockDim.x) {
      s_code[i] = codes_sorted[t0 + i];
      s_perm[i] = perm[t0 + i];
    }
    __syncthreads();
    if (!col_act) continue; /* block-uniform trip count: the barriers still meet */
    for (int i0 = 0; i0 < nt; i0 += SCOLS_ROWS) {
      ScanVec<V, VC> x[SCOLS_ROWS];
      int g[SCOLS_ROWS];
      int64_t row[SCOLS_ROWS];
#pragma unroll
      for (int u = 0; u < SCOLS_ROWS; ++u) {
        if (i0 + u >= nt) break;
        const int i = REV ? nt - 1 - (i0 + u) : i0 + u;
        g[u] = s_code[i];
        row[u] = (int64_t)s_perm[i];
        const V* src = values + row[u] * ldm + c0;
        if (VC > 1 && full) {
          x[u] = *reinterpret_cast<const ScanVec<V, VC>*>(src);
        } else {
#pragma unroll
          for (int k = 0; k < VC; ++k)
            if (c0 + k < m) x[u].v[k] = src[k];
        }
      }
#pragma unroll
      for (int u = 0; u < SCOLS_ROWS; ++u) {
        if (i0 + u >= nt) break;
        const bool first = g[u] != cur_g;
        cur_g = g[u];
        ScanVec<V, VC> y;
#pragma unroll
        for (int k = 0; k < VC; ++k) {
          acc[k] = scan_step<V, OP>(acc[k], x[u].v[k], first);
          y.v[k] = acc[k];
        }
        V* dst = out + row[u] * ldo + c0;
        if (VC > 1 && full) {
          *reinterpret_cast<ScanVec<V, VC>*>(dst) = y;
        } else {
#pragma unroll
          for (int k = 0; k < VC; ++k)
            if (c0 + k < m) dst[k] = y.v[k];
        }
      }
    }
  }
}

/* launcher of k_scan_cols: the vector form needs both row strides a multiple
 * of VC and both bases 16-B aligned (cols_plan's rule, applied to the output
 * too), else one column per thread. Narrow arrays take smaller workgroups:
 * the grid is column tiles x chunks, and fewer lanes per tile make more of
 * them. */
template <typename V, int OP>
int launch_scan_cols(fh_call* c, int64_t ldo) {
  hipStream_t stream = (hipStream_t)c->stream;
  int vc = SCOLS_VC<V>;
  if (c->ldm % vc != 0 || ldo % vc != 0 || ((uintptr_t)c->values % 16) != 0 ||
      ((uintptr_t)c->out_sum % 16) != 0)
    vc = 1;
  const bool chunks = c->chunk_offsets != nullptr && c->nchunks > 0;
  const int64_t nch = chunks ? c->nchunks : 1;
  const int64_t lanes = (c->m + vc - 1) / vc;
  int block = SCOLS_BLOCK;
  while (block > 64 && ((lanes + block - 1) / block) * nch < 1024) block >>= 1;
  const int64_t ncolblk = (lanes + block - 1) / block;
  if (ncolblk > INT32_MAX) return 23;
  dim3 grid((uint32_t)ncolblk, (uint32_t)nch);
  const int64_t* offs = chunks ? (const int64_t*)c->chunk_offsets : nullptr;
  auto launch = [&](auto vcc) -> int {
    hipLaunchKernelGGL((k_scan_cols<V, OP, decltype(vcc)::value>), grid, dim3(block), 0,
                       stream, (const V*)c->values, (const int*)c->labels,
                       (const int*)c->perm, c->n, c->m, c->ldm, ldo, offs,
                       (V*)c->out_sum);
    FHS_CHECK(hipGetLastError());
    return 0;
  };
  const int rc = vc > 1 ? launch(std::integral_constant<int, SCOLS_VC<V>>{})
                        : launch(std::integral_constant<int, 1>{});
  if (rc) return rc;
  c->path_used = 3;
  return 0;
}

/* sums for f32/f64/i64, fills for f32/f64 */
template <typename V>
int dispatch_scan_cols(fh_call* c, int op, int64_t ldo) {
  switch (op) {
    case SCAN_CUMSUM: return launch_scan_cols<V, SCAN_CUMSUM>(c, ldo);
    case SCAN_NANCUMSUM: return launch_scan_cols<V, SCAN_NANCUMSUM>(c, ldo);
    default: break;
  }
  if constexpr (!std::is_same<V, int64_t>::value) {
    if (op == SCAN_FFILL) return launch_scan_cols<V, SCAN_FFILL>(c, ldo);
    if (op == SCAN_BFILL) return launch_scan_cols<V, SCAN_BFILL>(c, ldo);
  }
  return 24;
}

/* ---- row form: grouped scans along the contiguous axis of an (m x n) array --
 * The (lead_M, N) layout with the grouped (time) axis last: values[r * ldm + t].
 * A single-wave workgroup owns R lead rows and walks the time axis in tiles of
 * T steps (include/floxhip_scanrows.h has the plan and the LDS layout). Per
 * tile: the R x T values come in coalesced along t (16 lanes x 16 B cover one
 * row's 256 B; element-wise where a base or a stride breaks the alignment) and
 * are laid out [t][R + 1] in LDS; the tile's T codes are staged once; lane r
 * walks the T steps of row r in time order and overwrites the tile with the
 * results; the tile goes out coalesced along t. The code at a step is the same
 * for every row, so the walk's branches are wave-uniform: a lane keeps the
 * running value of the current group in a register and, where the code
 * changes, parks it at carry[slot * R + r] and fetches the new group's (slot =
 * code + 1, the -1 steps being a group of their own). Lane r owns row r for
 * the whole kernel, so its state lives in registers across tiles. Where a
 * group starts is the same for every row too: s_first[slot] takes the walk
 * position of the group's first step (an LDS atomicMin per staged code), and a
 * step that finds its own position there starts its group, which is what lets
 * a sum's first row initialise it and leaves the carries uninitialised. The
 * vector form holds the next tile's loads in registers across the walk. bfill
 * is ffill with tiles and steps walked from the last time step. */
template <typename V, int OP, int R, bool VEC>
__launch_bounds__(FH_SCANROWS_BLOCK) __global__ void k_scan_rows(
    const V* __restrict__ values, const int* __restrict__ labels, int64_t m, int n,
    int64_t ldm, int64_t ldo, int ngroups, V* __restrict__ out) {
  constexpr bool REV = OP == SCAN_BFILL;
  constexpr int T = FH_SCANROWS_TILE_BYTES / (int)sizeof(V);
  constexpr int P = R + 1;                /* LDS pitch of one time step */
  constexpr int VL = 16 / (int)sizeof(V); /* values per 16-B vector */
  constexpr int NL = R / 4;               /* vectors per lane per tile: 4 rows per instruction */
  constexpr int WU = 8;                   /* steps read before the first is consumed */
  static_assert(T <= FH_SCANROWS_BLOCK, "one staged code per lane");
  extern __shared__ __align__(16) unsigned char s_raw[];
  V* s_carry = reinterpret_cast<V*>(s_raw);
  V* s_tile = s_carry + (ngroups + 1) * R;
  int* s_code = reinterpret_cast<int*>(s_tile + T * P);
  int* s_first = s_code + T;

  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int vrow = lane / 16;         /* vector form: row within a group of 4 */
  const int vt = (lane % 16) * VL;    /* and first step of this lane's vector */
  const int ntiles = (n + T - 1) / T;

  for (int i = lane; i <= ngroups; i += FH_SCANROWS_BLOCK) s_first[i] = INT32_MAX;

  ScanVec<V, VL> x[NL];
  int code_next = -1;
  auto fetch = [&](int tt) {
    const int t0 = (REV ? ntiles - 1 - tt : tt) * T;
    const int nt = n - t0 < T ? n - t0 : T;
    if (lane < nt) code_next = labels[t0 + lane];
    if (!VEC) return;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int r = j * 4 + vrow;
#pragma unroll
      for (int k = 0; k < VL; ++k) x[j].v[k] = (V)0;
      if (r0 + r >= m) continue;
      const V* src = values + (r0 + r) * ldm + t0 + vt;
      if (vt + VL <= nt) {
        x[j] = *reinterpret_cast<const ScanVec<V, VL>*>(src);
      } else {
#pragma unroll
        for (int k = 0; k < VL; ++k)
          if (vt + k < nt) x[j].v[k] = src[k];
      }
    }
  };
  if (ntiles > 0) fetch(0);

  int cur = -1; /* no slot: slots are >= 0 */
  V acc = (V)0;
  for (int tt = 0; tt < ntiles; ++tt) {
    const int t0 = (REV ? ntiles - 1 - tt : tt) * T;
    const int nt = n - t0 < T ? n - t0 : T;
    __syncthreads(); /* the previous tile is out; s_first is initialised */
    if (VEC) {
#pragma unroll
      for (int j = 0; j < NL; ++j)
#pragma unroll
        for (int k = 0; k < VL; ++k) s_tile[(vt + k) * P + j * 4 + vrow] = x[j].v[k];
    } else {
#pragma unroll 8
      for (int e = lane; e < R * T; e += FH_SCANROWS_BLOCK) {
        const int r = e / T, t = e % T;
        if (r0 + r < m && t < nt) s_tile[t * P + r] = values[(r0 + r) * ldm + t0 + t];
      }
    }
    int slot = 0, w = 0;
    if (lane < nt) {
      /* a code outside [-1, ngroups) breaks the contract; it joins the -1 group
       * instead of indexing past the carries */
      slot = (code_next < 0 || code_next >= ngroups) ? 0 : code_next + 1;
      w = REV ? n - 1 - (t0 + lane) : t0 + lane;
      atomicMin(&s_first[slot], w);
    }
    __syncthreads();
    if (lane < nt) s_code[lane] = slot | (s_first[slot] == w ? INT32_MIN : 0);
    if (tt + 1 < ntiles) fetch(tt + 1);
    __syncthreads();

    if (lane < R) {
      for (int i0 = 0; i0 < nt; i0 += WU) {
        V xv[WU];
        int pc[WU];
#pragma unroll
        for (int u = 0; u < WU; ++u) {
          if (i0 + u >= nt) break;
          const int idx = REV ? nt - 1 - (i0 + u) : i0 + u;
          xv[u] = s_tile[idx * P + lane];
          pc[u] = s_code[idx];
        }
#pragma unroll
        for (int u = 0; u < WU; ++u) {
          if (i0 + u >= nt) break;
          const int p = __builtin_amdgcn_readfirstlane(pc[u]);
          const int sl = p & INT32_MAX;
          const bool first = p < 0;
          if (sl != cur) {
            if (cur >= 0) s_carry[cur * R + lane] = acc;
            if (!first) acc = s_carry[sl * R + lane];
            cur = sl;
          }
          acc = scan_step<V, OP>(acc, xv[u], first);
          xv[u] = acc;
        }
#pragma unroll
        for (int u = 0; u < WU; ++u) {
          if (i0 + u >= nt) break;
          const int idx = REV ? nt - 1 - (i0 + u) : i0 + u;
          s_tile[idx * P + lane] = xv[u];
        }
      }
    }
    __syncthreads();

    if (VEC) {
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const int r = j * 4 + vrow;
        if (r0 + r >= m) continue;
        ScanVec<V, VL> y;
#pragma unroll
        for (int k = 0; k < VL; ++k) y.v[k] = s_tile[(vt + k) * P + r];
        V* dst = out + (r0 + r) * ldo + t0 + vt;
        if (vt + VL <= nt) {
          *reinterpret_cast<ScanVec<V, VL>*>(dst) = y;
        } else {
#pragma unroll
          for (int k = 0; k < VL; ++k)
            if (vt + k < nt) dst[k] = y.v[k];
        }
      }
    } else {
#pragma unroll 8
      for (int e = lane; e < R * T; e += FH_SCANROWS_BLOCK) {
        const int r = e / T, t = e % T;
        if (r0 + r < m && t < nt) out[(r0 + r) * ldo + t0 + t] = s_tile[t * P + r];
      }
    }
  }
}

/* launcher of k_scan_rows: the vector form needs both row strides a multiple
 * of the vector and both bases 16-B aligned (tiles start at multiples of 256
 * B, so every vector of an aligned row is aligned). Dynamic LDS beyond 64 KiB
 * needs the function attribute raised first. */
template <typename V, int OP, int R>
int launch_scan_rows_r(fh_call* c, int64_t ldo, const fh_scanrows_plan& pl) {
  hipStream_t stream = (hipStream_t)c->stream;
  constexpr int VL = 16 / (int)sizeof(V);
  const bool vec = c->ldm % VL == 0 && ldo % VL == 0 && ((uintptr_t)c->values % 16) == 0 &&
                   ((uintptr_t)c->out_sum % 16) == 0;
  const int64_t nblk = (c->m + R - 1) / R;
  if (nblk > INT32_MAX) return 23;
  auto launch = [&](auto vecc) -> int {
    auto kern = k_scan_rows<V, OP, R, decltype(vecc)::value>;
    if (pl.lds_bytes > 64 * 1024)
      FHS_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)pl.lds_bytes));
    hipLaunchKernelGGL(kern, dim3((uint32_t)nblk), dim3(FH_SCANROWS_BLOCK),
                       (size_t)pl.lds_bytes, stream, (const V*)c->values,
                       (const int*)c->labels, c->m, (int)c->n, c->ldm, ldo, (int)c->ngroups,
                       (V*)c->out_sum);
    FHS_CHECK(hipGetLastError());
    return 0;
  };
  const int rc = vec ? launch(std::true_type{}) : launch(std::false_type{});
  if (rc) return rc;
  c->path_used = 3;
  return 0;
}

template <typename V, int OP>
int launch_scan_rows(fh_call* c, int64_t ldo) {
  fh_scanrows_plan pl;
  if (!fh_scanrows_plan_for((int)sizeof(V), c->ngroups, &pl)) return 25;
  switch (pl.R) {
    case 64: return launch_scan_rows_r<V, OP, 64>(c, ldo, pl);
    case 32: return launch_scan_rows_r<V, OP, 32>(c, ldo, pl);
    default: return launch_scan_rows_r<V, OP, 16>(c, ldo, pl);
  }
}

/* sums for f32/f64/i64, fills for f32/f64 */
template <typename V>
int dispatch_scan_rows(fh_call* c, int op, int64_t ldo) {
  switch (op) {
    case SCAN_CUMSUM: return launch_scan_rows<V, SCAN_CUMSUM>(c, ldo);
    case SCAN_NANCUMSUM: return launch_scan_rows<V, SCAN_NANCUMSUM>(c, ldo);
    default: break;
  }
  if constexpr (!std::is_same<V, int64_t>::value) {
    if (op == SCAN_FFILL) return launch_scan_rows<V, SCAN_FFILL>(c, ldo);
    if (op == SCAN_BFILL) return launch_scan_rows<V, SCAN_BFILL>(c, ldo);
  }
  return 24;
}

int scan_rows_value_bytes(int vdtype) {
  return vdtype == FH_F32 ? 4 : (vdtype == FH_F64 || vdtype == FH_I64) ? 8 : 0;
}

template <typename V, typename L>
int dispatch_scan_op(fh_call* c, int op, V* out) {
  switch (op) {
    case SCAN_CUMSUM: return run_scan<V, L, SCAN_CUMSUM>(c, out);
    case SCAN_NANCUMSUM: return run_scan<V, L, SCAN_NANCUMSUM>(c, out);
    case SCAN_FFILL: return run_scan<V, L, SCAN_FFILL>(c, out);
    case SCAN_BFILL: return run_scan<V, L, SCAN_BFILL>(c, out);
    default: return 4;
  }
}

}  // namespace

extern "C" {

int64_t fh_scan_scratch_bytes(const fh_call* c) {
  const int64_t n = c->n;
  auto al = [](int64_t b) { return ((b + 255) / 256) * 256; };
  const int64_t vsz = (c->vdtype == FH_F64 || c->vdtype == FH_I64) ? 8 : 4;
  const int64_t psz = (c->vdtype == FH_F64 || c->vdtype == FH_I64) ? 16 : 8;
  size_t ts = 0, t2 = 0, t3 = 0;
  (void)rocprim::radix_sort_pairs(nullptr, ts, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                            (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n,
                            0, 32, 0);
  (void)rocprim::inclusive_scan_by_key(nullptr, t2, (const uint32_t*)nullptr,
                                 (const double*)nullptr, (double*)nullptr, (size_t)n,
                                 rocprim::plus<double>(), rocprim::equal_to<uint32_t>(), 0);
  /* the fill ops scan 16-byte pairs, which need more rocprim temp */
  (void)rocprim::inclusive_scan_by_key(nullptr, t3, (const uint32_t*)nullptr,
                                 (const FillPair<double>*)nullptr, (FillPair<double>*)nullptr,
                                 (size_t)n, FillOp<double>(), rocprim::equal_to<uint32_t>(), 0);
  /* 4 x u32 arrays + reversed keys + 2 scan buffers (pair-sized upper bound) */
  return 5 * al(n * 4) + 2 * al(n * psz) +
         al((int64_t)std::max(ts, std::max(t2, t3))) + 2 * al(n * vsz);
}

/* grouped scan; op: 0 cumsum, 1 nancumsum, 2 ffill, 3 bfill.
 * out_sum receives value-dtype[n] in ORIGINAL row order. */
int fh_grouped_scan(fh_call* c, int op) {
  if (!c || !c->values || !c->labels || !c->out_sum) return 6;
  switch (c->vdtype) {
    case FH_F32:
      return c->ldtype == FH_L_I64 ? dispatch_scan_op<float, int64_t>(c, op, (float*)c->out_sum)
                                   : dispatch_scan_op<float, int32_t>(c, op, (float*)c->out_sum);
    case FH_F64:
      return c->ldtype == FH_L_I64 ? dispatch_scan_op<double, int64_t>(c, op, (double*)c->out_sum)
                                   : dispatch_scan_op<double, int32_t>(c, op, (double*)c->out_sum);
    case FH_I64:
      return c->ldtype == FH_L_I64 ? dispatch_scan_op<int64_t, int64_t>(c, op, (int64_t*)c->out_sum)
                                   : dispatch_scan_op<int64_t, int32_t>(c, op, (int64_t*)c->out_sum);
    case FH_I32:
      return c->ldtype == FH_L_I64 ? dispatch_scan_op<int32_t, int64_t>(c, op, (int32_t*)c->out_sum)
                                   : dispatch_scan_op<int32_t, int32_t>(c, op, (int32_t*)c->out_sum);
    default:
      return 9;
  }
}

/* grouped scan over the leading axis of an (n x m) array, in place on the
 * caller's strided view (include/floxhip.h has the contract). No scratch, no
 * host sync; every refusal returns before any launch. */
int fh_grouped_scan_cols(fh_call* c, int op, int64_t ldo) {
  if (!c || !c->values || !c->labels || !c->perm || !c->out_sum) return 22;
  /* a single row has no stride to speak of; chunks ride gridDim.y */
  if (c->n < 0 || c->m < 0 || c->n > INT32_MAX ||
      (c->n > 1 && (c->ldm < c->m || ldo < c->m)) || c->nchunks < 0 ||
      (c->chunk_offsets && c->nchunks > 65535))
    return 23;
  if (op < SCAN_CUMSUM || op > SCAN_BFILL) return 24;
  if (c->vdtype != FH_F32 && c->vdtype != FH_F64 && c->vdtype != FH_I64) return 24;
  if (c->vdtype == FH_I64 && op >= SCAN_FFILL) return 24;
  if (c->n == 0 || c->m == 0) {
    c->path_used = 3;
    return 0;
  }
  switch (c->vdtype) {
    case FH_F32: return dispatch_scan_cols<float>(c, op, ldo);
    case FH_F64: return dispatch_scan_cols<double>(c, op, ldo);
    default: return dispatch_scan_cols<int64_t>(c, op, ldo);
  }
}

/* grouped scan along the contiguous axis of an (m x n) array, in place on the
 * caller's strided rows (include/floxhip.h has the contract). No scratch, no
 * host sync, no chunk plan; every refusal returns before any launch. */
int fh_grouped_scan_rows(fh_call* c, int op, int64_t ldo) {
  if (!c || !c->values || !c->labels || !c->out_sum) return 22;
  /* a single row has no stride to speak of */
  if (c->n < 0 || c->m < 0 || c->ngroups < 0 || c->n > INT32_MAX ||
      (c->m > 1 && (c->ldm < c->n || ldo < c->n)))
    return 23;
  if (op < SCAN_CUMSUM || op > SCAN_BFILL) return 24;
  if (c->vdtype != FH_F32 && c->vdtype != FH_F64 && c->vdtype != FH_I64) return 24;
  if (c->vdtype == FH_I64 && op >= SCAN_FFILL) return 24;
  if (c->ngroups > fh_scanrows_max_groups(scan_rows_value_bytes(c->vdtype))) return 25;
  if (c->n == 0 || c->m == 0) {
    c->path_used = 3;
    return 0;
  }
  switch (c->vdtype) {
    case FH_F32: return dispatch_scan_rows<float>(c, op, ldo);
    case FH_F64: return dispatch_scan_rows<double>(c, op, ldo);
    default: return dispatch_scan_rows<int64_t>(c, op, ldo);
  }
}

int64_t fh_scan_rows_max_groups(int vdtype) {
  return fh_scanrows_max_groups(scan_rows_value_bytes(vdtype));
}

int fh_scan_rows_plan(int vdtype, int64_t ngroups, int* row_tile, int* time_tile) {
  const int vb = scan_rows_value_bytes(vdtype);
  if (!vb) return 24;
  if (ngroups < 0) return 23;
  fh_scanrows_plan pl;
  if (!fh_scanrows_plan_for(vb, ngroups, &pl)) return 25;
  if (row_tile) *row_tile = pl.R;
  if (time_tile) *time_tile = pl.T;
  return 0;
}

}  /* extern "C" */
