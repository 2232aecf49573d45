/* Host-only checks of the row-form grouped scan's tile plan
 * (include/floxhip_scanrows.h). Built and run by tests/test_rows_scan_cpu.py
 * under AddressSanitizer and UBSan; no GPU, no HIP. */
#include <cstdio>
#include <cstdlib>

#include "../include/floxhip_scanrows.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

int main() {
  const int sizes[] = {4, 8};
  int64_t max_groups[2] = {0, 0};
  for (int s = 0; s < 2; ++s) {
    const int vb = sizes[s];
    const int64_t mg = fh_scanrows_max_groups(vb);
    max_groups[s] = mg;
    CHECK(mg >= 1);
    int last_R = FH_SCANROWS_MAX_ROWS;
    for (int64_t ng = 0; ng <= mg; ++ng) {
      fh_scanrows_plan pl;
      CHECK(fh_scanrows_plan_for(vb, ng, &pl) == 1);
      /* the row tile is one of the allowed set and never grows with ngroups */
      CHECK(pl.R == 64 || pl.R == 32 || pl.R == 16);
      CHECK(pl.R <= FH_SCANROWS_MAX_ROWS && pl.R >= FH_SCANROWS_MIN_ROWS);
      CHECK(pl.R <= last_R);
      last_R = pl.R;
      /* one lane per lead row, one staged code per lane */
      CHECK(pl.R <= FH_SCANROWS_BLOCK);
      CHECK(pl.T >= 1 && pl.T <= FH_SCANROWS_BLOCK);
      CHECK(pl.T * vb == FH_SCANROWS_TILE_BYTES);
      /* whole 16-B vectors per row of a tile, 16 lanes per row, 4 rows per
       * instruction */
      CHECK((pl.T * vb) % 16 == 0 && (pl.T * vb) / 16 == FH_SCANROWS_BLOCK / 4);
      CHECK(pl.R % 4 == 0);
      /* LDS: the bytes the kernel lays out, within the declared budget */
      const int64_t carries = (ng + 1) * pl.R * vb;
      const int64_t tile = (int64_t)pl.T * (pl.R + 1) * vb;
      const int64_t laid_out = carries + tile + (int64_t)pl.T * 4 + (ng + 1) * 4;
      CHECK(pl.lds_bytes == laid_out);
      CHECK(pl.lds_bytes == fh_scanrows_lds_bytes(pl.R, vb, ng));
      CHECK(pl.lds_bytes <= FH_SCANROWS_LDS_MAX);
      CHECK(FH_SCANROWS_LDS_MAX <= (int64_t)160 * 1024);
      /* the tile behind the carries and the ints behind the tile stay aligned */
      CHECK(carries % 8 == 0 && (carries + tile) % 4 == 0);
      CHECK(pl.blocks_per_cu >= 1);
      CHECK(pl.blocks_per_cu * pl.lds_bytes <= FH_SCANROWS_LDS_MAX);
      /* a wider tile is taken only where four workgroups still share a CU */
      if (pl.R > FH_SCANROWS_MIN_ROWS) CHECK(pl.blocks_per_cu >= 4);
      /* slot * R + lane stays far inside int */
      CHECK((ng + 1) * pl.R < ((int64_t)1 << 30));
    }
    CHECK(last_R == FH_SCANROWS_MIN_ROWS); /* the tile has shrunk by max_groups */
    /* few groups get the widest tile */
    fh_scanrows_plan few;
    CHECK(fh_scanrows_plan_for(vb, 24, &few) == 1 && few.R == FH_SCANROWS_MAX_ROWS);
    /* refusals leave *out alone */
    fh_scanrows_plan pl;
    pl.R = -5;
    CHECK(fh_scanrows_plan_for(vb, mg + 1, &pl) == 0);
    CHECK(fh_scanrows_plan_for(vb, mg + 1000000, &pl) == 0);
    CHECK(fh_scanrows_plan_for(vb, -1, &pl) == 0);
    CHECK(pl.R == -5);
    CHECK(fh_scanrows_lds_bytes(FH_SCANROWS_MIN_ROWS, vb, mg + 1) > FH_SCANROWS_LDS_MAX);
  }
  CHECK(max_groups[1] <= max_groups[0]);
  fh_scanrows_plan pl;
  pl.R = -5;
  const int bad[] = {0, 1, 2, 3, 5, 16, -4};
  for (int vb : bad) {
    CHECK(fh_scanrows_plan_for(vb, 1, &pl) == 0);
    CHECK(fh_scanrows_max_groups(vb) == 0);
  }
  CHECK(pl.R == -5);
  std::printf("scanrows plan host checks OK\n");
  return 0;
}
