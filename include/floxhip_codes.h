/* floxhip — packed label codes: the cached form of FH_L_P12 / FH_L_P14.
 *
 * One definition of the format, shared by the reduce kernel, the packer and
 * the host test (tests/packed_codes_host.cpp). Everything here is plain
 * integer arithmetic and compiles for host and device alike.
 *
 * Width W is 12 bits for ngroups <= 4094, 14 bits for ngroups <= 16382,
 * else 16 (the plain uint16 stream, not handled here). The all-ones W-bit
 * value means "row in no group": it is >= ngroups by construction, so the
 * kernel's ordinary bounds check drops it.
 *
 * A tile is 1024 consecutive rows, handled by one 64-lane wave. Lane l owns
 * rows  tile*1024 + j*256 + l*4 + k  for j, k in 0..3  (slot s = 4j + k), so
 * that for every j the wave reads 256 consecutive values, 4 per lane. A
 * lane's 16 codes are a little-endian string of 16*W bits, slot s at bit
 * s*W: W/2 dwords. A tile stores them as planes, each 64 * width bytes with
 * lane l at l * width, so that every code load is one fully coalesced wave
 * instruction:
 *   dwords 0..3  16-B plane at tile byte offset 0
 *   dwords 4..5   8-B plane at 1024
 *   dword  6      4-B plane at 1536            (W = 14 only)
 * The buffer is whole tiles, ceil(n/1024) * 128 * W bytes; slots of rows
 * >= n hold the sentinel. The layout does not depend on the value dtype.
 */
#ifndef FLOXHIP_CODES_H
#define FLOXHIP_CODES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FH_HD __host__ __device__ inline
#else
#define FH_HD inline
#endif

enum {
  FH_TILE_ROWS = 1024,  /* rows per tile (one wave) */
  FH_TILE_LANES = 64,
  FH_LANE_SLOTS = 16,   /* codes per lane per tile */
  FH_PLANE8_OFF = 1024, /* byte offset of the 8-B plane in a tile */
  FH_PLANE4_OFF = 1536, /* ... of the 4-B plane (W = 14) */
};

/* code width for a group count: 12, 14, or 16 (= the uint16 form) */
FH_HD int fh_code_width(int64_t ngroups) {
  return ngroups <= 4094 ? 12 : ngroups <= 16382 ? 14 : 16;
}

FH_HD uint32_t fh_code_sentinel(int w) { return (1u << w) - 1u; }

/* bytes of one tile / of the packed buffer for n rows; -1 for a bad width */
FH_HD int64_t fh_tile_bytes(int w) { return (int64_t)(FH_TILE_ROWS / 8) * w; }
FH_HD int64_t fh_packed_bytes(int64_t n, int w) {
  if ((w != 12 && w != 14) || n < 0) return -1;
  return ((n + FH_TILE_ROWS - 1) / FH_TILE_ROWS) * fh_tile_bytes(w);
}

/* (tile, lane, slot) -> row */
FH_HD int64_t fh_tile_row(int64_t tile, int lane, int slot) {
  return tile * FH_TILE_ROWS + (slot >> 2) * 256 + lane * 4 + (slot & 3);
}

/* byte offset, within its tile, of dword d of lane l's packed codes */
FH_HD int fh_plane_offset(int d, int lane) {
  return d < 4 ? lane * 16 + d * 4
         : d < 6 ? FH_PLANE8_OFF + lane * 8 + (d - 4) * 4
                 : FH_PLANE4_OFF + lane * 4;
}

/* 16 codes (each < 2^W) -> W/2 dwords */
template <int W>
FH_HD void fh_pack16(const uint32_t* code, uint32_t* out) {
  static_assert(W == 12 || W == 14, "packed widths are 12 and 14 bits");
  for (int d = 0; d < W / 2; ++d) out[d] = 0u;
  for (int s = 0; s < FH_LANE_SLOTS; ++s) {
    const int bit = s * W, d = bit >> 5, sh = bit & 31;
    const uint32_t c = code[s] & ((1u << W) - 1u);
    out[d] |= c << sh;
    if (sh + W > 32) out[d + 1] |= c >> (32 - sh);
  }
}

/* code of slot s from a lane's W/2 dwords; with s a compile-time constant
 * (an unrolled loop) this is one bit-field extract, or a funnel shift and a
 * mask where the code straddles two dwords */
template <int W>
FH_HD uint32_t fh_unpack1(const uint32_t* in, int s) {
  static_assert(W == 12 || W == 14, "packed widths are 12 and 14 bits");
  const int bit = s * W, d = bit >> 5, sh = bit & 31;
  uint32_t c = in[d] >> sh;
  if (sh + W > 32) c |= in[d + 1] << (32 - sh);
  return c & ((1u << W) - 1u);
}

template <int W>
FH_HD void fh_unpack16(const uint32_t* in, uint32_t* code) {
  for (int s = 0; s < FH_LANE_SLOTS; ++s) code[s] = fh_unpack1<W>(in, s);
}

#endif /* FLOXHIP_CODES_H */
