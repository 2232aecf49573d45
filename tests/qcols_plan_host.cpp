/* Host check of the sort-in-LDS column kernel's tile plan
 * (include/floxhip_qcols.h): the definitions the launcher and the kernel
 * use, compiled for the CPU. Built and run by tests/test_cols_sorted_cpu.py
 * with -fsanitize=address,undefined; exit status 0 = every check passed. */
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../include/floxhip_qcols.h"

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAIL %s:%d: %s (rows %lld, key %d)\n", __FILE__,      \
                  __LINE__, #cond, (long long)rows, key);                \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static bool pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

int main() {
  const int64_t lds_max = (int64_t)160 * 1024 - 512;
  for (int key : {4, 8}) {
    int64_t rows = 0;
    const int64_t cap = fh_qcols_capacity(key);
    CHECK(cap == 2048);
    const int minC = key == 4 ? 16 : 8;
    CHECK(fh_qcols_min_cols(key) == minC);
    /* the capacity is the largest power of two whose minimum tile fits */
    CHECK(cap * minC * key <= lds_max && 2 * cap * minC * key > lds_max);
    for (rows = 1; rows <= cap; ++rows) {
      fh_qcols_plan pl = {-1, -1, -1, -1, -1, -1};
      CHECK(fh_qcols_plan_for(rows, key, &pl) == 1);
      CHECK(pow2(pl.P) && pl.P >= rows && (pl.P == 1 || pl.P / 2 < rows));
      CHECK(pow2(pl.C) && pl.C >= minC && pl.C <= 64 && (1 << pl.logC) == pl.C);
      CHECK(pl.lds_bytes == pl.P * pl.C * key);
      CHECK(pl.lds_bytes <= lds_max);
      CHECK(pl.blocks_per_cu == 1 || pl.blocks_per_cu == 2);
      /* two workgroups per CU wherever the minimum tile fits half the LDS */
      CHECK((pl.blocks_per_cu == 2) == (pl.P * minC * key <= lds_max / 2));
      CHECK(pl.blocks_per_cu * pl.lds_bytes <= lds_max);
      /* C is the largest that fits the budget */
      CHECK(pl.C == 64 || 2 * pl.lds_bytes * pl.blocks_per_cu > lds_max);
      CHECK(pl.block == (pl.blocks_per_cu == 2 ? 512 : 1024));
      CHECK(pl.block >= pl.C && pl.block % pl.C == 0);
    }
    for (int64_t bad : {cap + 1, (int64_t)0, (int64_t)-5, (int64_t)1 << 40}) {
      rows = bad;
      fh_qcols_plan pl = {-7, -7, -7, -7, -7, -7};
      CHECK(fh_qcols_plan_for(rows, key, &pl) == 0);
      CHECK(pl.P == -7 && pl.C == -7 && pl.lds_bytes == -7); /* untouched */
    }
  }
  {
    int64_t rows = 10;
    int key = 2;
    fh_qcols_plan pl = {-7, -7, -7, -7, -7, -7};
    CHECK(fh_qcols_capacity(key) == 0);
    CHECK(fh_qcols_plan_for(rows, key, &pl) == 0);
  }
  if (failures == 0) std::printf("qcols plan host checks OK\n");
  return failures != 0;
}
