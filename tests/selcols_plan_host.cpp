/* Host-only checks of the radix-select column kernel's tile plan
 * (include/floxhip_selcols.h). Built and run by tests/test_cols_select_cpu.py
 * under AddressSanitizer and UBSan; no GPU, no HIP. */
#include <cstdio>
#include <cstdlib>

#include "../include/floxhip_selcols.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

static bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

int main() {
  const int key_sizes[] = {4, 8};
  for (int kb : key_sizes) {
    /* the launcher asks for the q that remain: any positive count */
    for (int want = 1; want <= 3 * FH_SELCOLS_MAX_SLOTS + 1; ++want) {
      fh_selcols_plan pl;
      CHECK(fh_selcols_plan_for(want, kb, &pl) == 1);
      CHECK(pl.slots >= 1 && pl.slots <= FH_SELCOLS_MAX_SLOTS);
      CHECK(pl.slots == (want < FH_SELCOLS_MAX_SLOTS ? want : FH_SELCOLS_MAX_SLOTS));
      /* LDS: within the budget, and the bytes the kernel lays out */
      CHECK(pl.lds_bytes <= FH_SELCOLS_LDS_MAX);
      CHECK(pl.blocks_per_cu * pl.lds_bytes <= FH_SELCOLS_LDS_MAX);
      const int64_t nsc = (int64_t)pl.slots * pl.C;
      const int64_t laid_out = nsc * (1 << pl.digit_bits) * 4 /* histograms */
                               + 2 * nsc * kb                 /* prefix, successor */
                               + 2 * nsc * 4                  /* rank, count <= */
                               + (int64_t)pl.C * 4;           /* NaN counts */
      CHECK(pl.lds_bytes == laid_out);
      CHECK(pl.lds_bytes == fh_selcols_lds_bytes(pl.slots, pl.C, kb));
      /* the keys behind the histograms stay 8-byte aligned */
      CHECK((nsc * (1 << pl.digit_bits) * 4) % 8 == 0);
      /* tile and block */
      CHECK(pow2(pl.C) && pl.C == (1 << pl.logC));
      CHECK(pl.C >= FH_SELCOLS_MIN_COLS && pl.C <= FH_SELCOLS_MAX_COLS);
      CHECK(pow2(pl.block) && pl.block >= pl.C && pl.block <= 1024);
      /* one thread owns one (slot, column) */
      CHECK(pl.block >= pl.slots * pl.C);
      CHECK(pl.blocks_per_cu == 1 || pl.blocks_per_cu == 2);
      CHECK(pl.blocks_per_cu * pl.block == 1024);
      /* digits: whole passes, most significant digit first down to bit 0 */
      CHECK(pl.digit_bits == FH_SELCOLS_DIGIT_BITS && pl.digit_bits >= 1 && pl.digit_bits <= 16);
      CHECK((kb * 8) % pl.digit_bits == 0);
      CHECK(pl.passes == kb * 8 / pl.digit_bits);
      CHECK(kb * 8 - pl.digit_bits * pl.passes == 0);
    }
    /* one slot gets the widest tile, two workgroups per CU */
    fh_selcols_plan one;
    CHECK(fh_selcols_plan_for(1, kb, &one) == 1);
    CHECK(one.C == FH_SELCOLS_MAX_COLS && one.blocks_per_cu == 2);
  }
  /* refusals leave *out alone */
  fh_selcols_plan pl;
  pl.C = -5;
  const int bad_keys[] = {0, 1, 2, 3, 5, 16, -4};
  for (int kb : bad_keys) CHECK(fh_selcols_plan_for(1, kb, &pl) == 0);
  CHECK(fh_selcols_plan_for(0, 4, &pl) == 0);
  CHECK(fh_selcols_plan_for(-1, 8, &pl) == 0);
  CHECK(pl.C == -5);
  std::printf("selcols plan host checks OK\n");
  return 0;
}
