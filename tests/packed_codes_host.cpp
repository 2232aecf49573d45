/* Host check of the packed label-code format (include/floxhip_codes.h): the
 * definitions the reduce kernel and the packer use, compiled for the CPU.
 * Built and run by tests/test_packed_codes_cpu.py with
 * -fsanitize=address,undefined; exit status 0 = every check passed. */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../include/floxhip_codes.h"

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

template <int W>
static void round_trip(std::mt19937& rng) {
  const uint32_t none = fh_code_sentinel(W);
  CHECK(none == (1u << W) - 1u);
  std::uniform_int_distribution<uint32_t> any(0, none);
  for (int rep = 0; rep < 2000; ++rep) {
    uint32_t code[FH_LANE_SLOTS], back[FH_LANE_SLOTS];
    /* exactly W/2 dwords each: the sanitizer sees a write past them */
    std::vector<uint32_t> packed(W / 2);
    for (int s = 0; s < FH_LANE_SLOTS; ++s) code[s] = any(rng);
    /* the sentinel and the largest real code, at moving slots */
    code[rep % FH_LANE_SLOTS] = none;
    code[(rep / FH_LANE_SLOTS + 1 + rep) % FH_LANE_SLOTS] = none - 1;
    if (rep == 0)
      for (int s = 0; s < FH_LANE_SLOTS; ++s) code[s] = none;
    if (rep == 1)
      for (int s = 0; s < FH_LANE_SLOTS; ++s) code[s] = s & 1 ? none - 1 : 0u;
    fh_pack16<W>(code, packed.data());
    fh_unpack16<W>(packed.data(), back);
    CHECK(std::memcmp(code, back, sizeof code) == 0);
    for (int s = 0; s < FH_LANE_SLOTS; ++s)
      CHECK(fh_unpack1<W>(packed.data(), s) == code[s]);
  }
}

template <int W>
static void tile_layout() {
  /* (lane, slot) -> row is a bijection onto the tile's 1024 rows */
  for (int64_t tile : {(int64_t)0, (int64_t)3, (int64_t)5000000}) {
    std::vector<int> seen(FH_TILE_ROWS, 0);
    for (int lane = 0; lane < FH_TILE_LANES; ++lane)
      for (int s = 0; s < FH_LANE_SLOTS; ++s) {
        const int64_t row = fh_tile_row(tile, lane, s);
        CHECK(row >= tile * FH_TILE_ROWS && row < (tile + 1) * FH_TILE_ROWS);
        if (row >= tile * FH_TILE_ROWS && row < (tile + 1) * FH_TILE_ROWS)
          ++seen[row - tile * FH_TILE_ROWS];
        /* the 4 slots of one j are 4 consecutive rows: one 16-B value load */
        CHECK(fh_tile_row(tile, lane, s) == fh_tile_row(tile, lane, s & ~3) + (s & 3));
      }
    for (int r = 0; r < FH_TILE_ROWS; ++r) CHECK(seen[r] == 1);
  }
  /* (lane, dword) -> byte offset tiles the tile's bytes exactly once */
  std::vector<int> bytes(fh_tile_bytes(W), 0);
  for (int lane = 0; lane < FH_TILE_LANES; ++lane)
    for (int d = 0; d < W / 2; ++d) {
      const int off = fh_plane_offset(d, lane);
      CHECK(off % 4 == 0 && off >= 0 && off + 4 <= fh_tile_bytes(W));
      if (off >= 0 && off + 4 <= fh_tile_bytes(W))
        for (int b = 0; b < 4; ++b) ++bytes[off + b];
    }
  for (int64_t b = 0; b < fh_tile_bytes(W); ++b) CHECK(bytes[b] == 1);
  /* the wide planes are aligned for their loads */
  for (int lane = 0; lane < FH_TILE_LANES; ++lane) {
    CHECK(fh_plane_offset(0, lane) % 16 == 0);
    CHECK(fh_plane_offset(4, lane) % 8 == 0);
    CHECK(fh_plane_offset(5, lane) == fh_plane_offset(4, lane) + 4);
  }
  CHECK(fh_tile_bytes(W) % 16 == 0);
}

int main() {
  std::mt19937 rng(12345);
  round_trip<12>(rng);
  round_trip<14>(rng);
  tile_layout<12>();
  tile_layout<14>();

  const int64_t ns[] = {0, 1, 1023, 1024, 1025};
  const int64_t tiles[] = {0, 1, 1, 1, 2};
  for (int i = 0; i < 5; ++i) {
    CHECK(fh_packed_bytes(ns[i], 12) == tiles[i] * 128 * 12);
    CHECK(fh_packed_bytes(ns[i], 14) == tiles[i] * 128 * 14);
  }
  CHECK(fh_packed_bytes(1000000000, 14) == 976563LL * 1792);
  CHECK(fh_packed_bytes(10, 16) == -1 && fh_packed_bytes(10, 8) == -1);
  CHECK(fh_packed_bytes(-1, 12) == -1);
  CHECK(fh_tile_bytes(12) == 1536 && fh_tile_bytes(14) == 1792);

  CHECK(fh_code_width(1) == 12 && fh_code_width(4094) == 12);
  CHECK(fh_code_width(4095) == 14 && fh_code_width(16382) == 14);
  CHECK(fh_code_width(16383) == 16 && fh_code_width(65534) == 16);
  /* the sentinel of the chosen width is never a group */
  for (int64_t ng : {1, 4094, 4095, 16382})
    CHECK((int64_t)fh_code_sentinel(fh_code_width(ng)) >= ng);

  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("packed codes host checks OK\n");
  return 0;
}
