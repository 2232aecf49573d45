/* floxhip — tile plan of the row form of the grouped scans
 * (fh_grouped_scan_rows, flox_amd/csrc/floxhip_scan.hip).
 *
 * One single-wave workgroup owns a tile of R lead rows of a (lead_M, N) array
 * whose grouped (time) axis is the contiguous one, and walks that axis in
 * tiles of T steps: the R x T values are staged in LDS, one lane per lead row
 * walks the T steps in order, and the finished tile is written back. A row's
 * running value of every group but the current one waits in LDS, at
 * carry[(code + 1) * R + r]. This header picks (R, T, LDS bytes) from the
 * value size and the group count. It has no HIP dependency: the host
 * launcher, the kernel and a CPU test (tests/scanrows_plan_host.cpp) share it.
 *
 *   T    256 bytes of one row: 64 steps of 4-byte values, 32 of 8-byte ones.
 *        One row of a tile is then two whole 128-B lines, loaded by 16 lanes
 *        with one 16-B vector each.
 *   R    the largest of 64 / 32 / 16 whose workspace fits a quarter of the
 *        LDS, so that at least four workgroups share a CU and one's walk
 *        overlaps the others' loads and stores (a workgroup is one wave, and
 *        its three phases do not overlap each other); where even 16 rows miss
 *        that, 16 rows under the whole LDS; beyond that the call is refused.
 *   LDS  carries (ngroups + 1) * R values, the tile T * (R + 1) values (the
 *        odd row pitch keeps the walk's per-row reads and writes free of bank
 *        conflicts), T staged codes, and per group the walk position of its
 *        first step (ngroups + 1 ints), from which the kernel knows where a
 *        group starts without a flag per row.
 */
#ifndef FLOXHIP_SCANROWS_H
#define FLOXHIP_SCANROWS_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FH_SCANROWS_HD __host__ __device__
#else
#define FH_SCANROWS_HD
#endif

/* gfx950 LDS per workgroup, as in floxhip_qcols.h */
#define FH_SCANROWS_LDS_MAX ((int64_t)160 * 1024 - 512)
#define FH_SCANROWS_MAX_ROWS 64
#define FH_SCANROWS_MIN_ROWS 16
#define FH_SCANROWS_TILE_BYTES 256
#define FH_SCANROWS_BLOCK 64

typedef struct fh_scanrows_plan {
  int R;             /* lead rows per workgroup: 64, 32 or 16 */
  int T;             /* time steps per tile */
  int64_t lds_bytes;
  int blocks_per_cu; /* workgroups the LDS lets share a CU */
} fh_scanrows_plan;

FH_SCANROWS_HD static inline int fh_scanrows_time_tile(int value_bytes) {
  return FH_SCANROWS_TILE_BYTES / value_bytes;
}

/* layout, in this order: carries, tile, codes, first positions */
FH_SCANROWS_HD static inline int64_t fh_scanrows_lds_bytes(int R, int value_bytes,
                                                           int64_t ngroups) {
  const int64_t T = fh_scanrows_time_tile(value_bytes);
  return (ngroups + 1) * R * value_bytes + T * (R + 1) * value_bytes + T * 4 +
         (ngroups + 1) * 4;
}

/* the largest ngroups served for this value size; 0 for an unknown size */
FH_SCANROWS_HD static inline int64_t fh_scanrows_max_groups(int value_bytes) {
  if (value_bytes != 4 && value_bytes != 8) return 0;
  const int64_t fixed = fh_scanrows_lds_bytes(FH_SCANROWS_MIN_ROWS, value_bytes, -1);
  const int64_t per_group = (int64_t)FH_SCANROWS_MIN_ROWS * value_bytes + 4;
  return (FH_SCANROWS_LDS_MAX - fixed) / per_group - 1;
}

/* 1 and *out filled in, or 0 where the value size is unknown, ngroups is
 * negative or nothing fits (*out untouched) */
FH_SCANROWS_HD static inline int fh_scanrows_plan_for(int value_bytes, int64_t ngroups,
                                                      fh_scanrows_plan* out) {
  if ((value_bytes != 4 && value_bytes != 8) || ngroups < 0) return 0;
  if (ngroups > fh_scanrows_max_groups(value_bytes)) return 0;
  int R = FH_SCANROWS_MAX_ROWS;
  while (R > FH_SCANROWS_MIN_ROWS &&
         fh_scanrows_lds_bytes(R, value_bytes, ngroups) > FH_SCANROWS_LDS_MAX / 4)
    R /= 2;
  const int64_t bytes = fh_scanrows_lds_bytes(R, value_bytes, ngroups);
  if (bytes > FH_SCANROWS_LDS_MAX) return 0;
  out->R = R;
  out->T = fh_scanrows_time_tile(value_bytes);
  out->lds_bytes = bytes;
  out->blocks_per_cu = (int)(FH_SCANROWS_LDS_MAX / bytes);
  return 1;
}

#endif /* FLOXHIP_SCANROWS_H */
