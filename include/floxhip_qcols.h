/* floxhip — tile plan of the sort-in-LDS column kernel
 * (fh_grouped_quantile_cols, flox_amd/csrc/floxhip_quantile.hip).
 *
 * One workgroup stages one group's rows for a tile of C columns in LDS as
 * P x C order-preserving keys ([row][column]), sorts every column there with
 * a bitonic network and answers quantiles / the mode from the sorted keys.
 * This header picks (P, C, LDS bytes, block size) from the caller's bound on
 * a group's row count and the key size. It has no HIP dependency: the host
 * launcher, the kernel and a CPU test (tests/qcols_plan_host.cpp) share it.
 *
 *   P   next power of two >= max_seg_rows (the network's width; the kernel
 *       sorts only the next power of two >= the segment it actually finds)
 *   C   columns per tile: the largest power of two <= FH_QCOLS_MAX_COLS with
 *       P*C*key_bytes within half the LDS, so that two workgroups share a CU
 *       and one loads while the other sorts; where even the minimum column
 *       count (16 for 4-byte keys, 8 for 8-byte keys: 64 B of one row per
 *       request) misses that, the whole LDS is the budget
 *   capacity: the largest P whose minimum tile fits the whole LDS
 */
#ifndef FLOXHIP_QCOLS_H
#define FLOXHIP_QCOLS_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FH_QCOLS_HD __host__ __device__
#else
#define FH_QCOLS_HD
#endif

/* gfx950 LDS per workgroup, as in floxhip.hip */
#define FH_QCOLS_LDS_MAX ((int64_t)160 * 1024 - 512)
#define FH_QCOLS_MAX_COLS 64

typedef struct fh_qcols_plan {
  int64_t P;         /* rows of the staged tile, a power of two */
  int C;             /* columns of the staged tile, a power of two */
  int logC;
  int64_t lds_bytes; /* P * C * key_bytes */
  int block;         /* threads per workgroup */
  int blocks_per_cu; /* 2 under the half-LDS budget, else 1 */
} fh_qcols_plan;

FH_QCOLS_HD static inline int fh_qcols_min_cols(int key_bytes) {
  return key_bytes == 4 ? 16 : 8;
}

/* longest segment the kernel can stage for this key size (0 for a key size
 * that is neither 4 nor 8) */
FH_QCOLS_HD static inline int64_t fh_qcols_capacity(int key_bytes) {
  if (key_bytes != 4 && key_bytes != 8) return 0;
  int64_t P = 1;
  while (2 * P * fh_qcols_min_cols(key_bytes) * key_bytes <= FH_QCOLS_LDS_MAX) P *= 2;
  return P;
}

/* 1 and *out filled in, or 0 where max_seg_rows is outside [1, capacity] or
 * the key size is unknown (*out untouched) */
FH_QCOLS_HD static inline int fh_qcols_plan_for(int64_t max_seg_rows, int key_bytes,
                                                fh_qcols_plan* out) {
  const int64_t cap = fh_qcols_capacity(key_bytes);
  if (max_seg_rows < 1 || max_seg_rows > cap) return 0;
  int64_t P = 1;
  while (P < max_seg_rows) P *= 2;
  const int minC = fh_qcols_min_cols(key_bytes);
  int64_t budget = FH_QCOLS_LDS_MAX / 2;
  int per_cu = 2;
  if (P * minC * key_bytes > budget) {
    budget = FH_QCOLS_LDS_MAX;
    per_cu = 1;
  }
  int C = FH_QCOLS_MAX_COLS, logC = 6;
  while (C > minC && P * C * key_bytes > budget) {
    C /= 2;
    --logC;
  }
  out->P = P;
  out->C = C;
  out->logC = logC;
  out->lds_bytes = P * C * key_bytes;
  /* 16 waves per CU either way: two workgroups of 512 or one of 1024 */
  out->block = per_cu == 2 ? 512 : 1024;
  out->blocks_per_cu = per_cu;
  return 1;
}

#endif /* FLOXHIP_QCOLS_H */
