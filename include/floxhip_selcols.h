/* floxhip — tile plan of the radix-select column kernel
 * (fh_grouped_quantile_select_cols, flox_amd/csrc/floxhip_quantile.hip).
 *
 * One workgroup serves one group's rows for a tile of C columns. It keeps no
 * rows: per pass it reads the segment once and counts one digit of the
 * order-preserving keys into an LDS histogram [slot][bin][column] of 32-bit
 * counters, one slot per target rank, then narrows every slot's key prefix by
 * the bin its rank falls in. The workspace does not depend on the segment
 * length, so there is no capacity. This header picks (C, slots per batch,
 * digit bits, passes, LDS bytes, block size) from the number of ranks the
 * caller wants and the key size. It has no HIP dependency: the host launcher,
 * the kernel and a CPU test (tests/selcols_plan_host.cpp) share it.
 *
 *   slots   min(wanted, FH_SELCOLS_MAX_SLOTS); a call with more q than that
 *           is served in batches
 *   C       the largest power of two <= FH_SELCOLS_MAX_COLS whose histogram
 *           fits half the LDS, so that two workgroups share a CU; where even
 *           FH_SELCOLS_MIN_COLS misses that, the whole LDS is the budget
 *   LDS     slots * 2^digit_bits * C counters, plus per (slot, column) the
 *           key prefix, the successor key, the remaining rank and the
 *           count of keys <= the selected one, plus a NaN count per column
 */
#ifndef FLOXHIP_SELCOLS_H
#define FLOXHIP_SELCOLS_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FH_SELCOLS_HD __host__ __device__
#else
#define FH_SELCOLS_HD
#endif

/* gfx950 LDS per workgroup, as in floxhip_qcols.h */
#define FH_SELCOLS_LDS_MAX ((int64_t)160 * 1024 - 512)
#define FH_SELCOLS_MAX_COLS 64
#define FH_SELCOLS_MIN_COLS 16
#define FH_SELCOLS_MAX_SLOTS 4
#define FH_SELCOLS_DIGIT_BITS 8

typedef struct fh_selcols_plan {
  int C;             /* columns per tile, a power of two */
  int logC;
  int slots;         /* target ranks served by one launch */
  int digit_bits;
  int passes;        /* key bits / digit_bits */
  int64_t lds_bytes;
  int block;         /* threads per workgroup, a power of two >= slots * C */
  int blocks_per_cu; /* 2 under the half-LDS budget, else 1 */
} fh_selcols_plan;

FH_SELCOLS_HD static inline int64_t fh_selcols_lds_bytes(int slots, int C, int key_bytes) {
  const int64_t hist = (int64_t)slots * (1 << FH_SELCOLS_DIGIT_BITS) * C * 4;
  /* prefix + successor keys, remaining rank + count of keys <= selected */
  const int64_t per_slot = (int64_t)slots * C * (2 * key_bytes + 8);
  return hist + per_slot + (int64_t)C * 4;
}

/* 1 and *out filled in, or 0 where slots_wanted < 1 or the key size is
 * unknown (*out untouched) */
FH_SELCOLS_HD static inline int fh_selcols_plan_for(int slots_wanted, int key_bytes,
                                                    fh_selcols_plan* out) {
  if (slots_wanted < 1 || (key_bytes != 4 && key_bytes != 8)) return 0;
  const int slots = slots_wanted < FH_SELCOLS_MAX_SLOTS ? slots_wanted : FH_SELCOLS_MAX_SLOTS;
  int64_t budget = FH_SELCOLS_LDS_MAX / 2;
  int per_cu = 2;
  if (fh_selcols_lds_bytes(slots, FH_SELCOLS_MIN_COLS, key_bytes) > budget) {
    budget = FH_SELCOLS_LDS_MAX;
    per_cu = 1;
  }
  int C = FH_SELCOLS_MAX_COLS, logC = 6;
  while (C > FH_SELCOLS_MIN_COLS && fh_selcols_lds_bytes(slots, C, key_bytes) > budget) {
    C /= 2;
    --logC;
  }
  if (fh_selcols_lds_bytes(slots, C, key_bytes) > budget) return 0;
  out->C = C;
  out->logC = logC;
  out->slots = slots;
  out->digit_bits = FH_SELCOLS_DIGIT_BITS;
  out->passes = key_bytes * 8 / FH_SELCOLS_DIGIT_BITS;
  out->lds_bytes = fh_selcols_lds_bytes(slots, C, key_bytes);
  /* 16 waves per CU either way: two workgroups of 512 or one of 1024 */
  out->block = per_cu == 2 ? 512 : 1024;
  out->blocks_per_cu = per_cu;
  return 1;
}

#endif /* FLOXHIP_SELCOLS_H */
