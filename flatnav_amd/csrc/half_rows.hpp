// half_rows.hpp -- part of the gfx950 search engine, free of HIP (device code includes it through distance.hpp, the host code
// through runtime.hpp, tests/half_rows_harness.cpp as it is).  The HALF-WIDTH MIRROR of a float32 vector table: every rule
// of it is stated here once -- which rows can have one, where a 16-byte chunk of a float32 row lives in its mirror row, when a
// float32 value survives binary16, and how one row is converted.
//
// A float32 index whose every element is exactly representable in IEEE binary16 (SIFT / BIGANN / MNIST delivered as float32,
// small-integer or coarsely quantised embeddings) is searched from a private copy of its rows at half the bytes.  Queries stay
// float32, and so does every operand of the arithmetic: widening binary16 is exact, the mirror keeps the float32 kernel's
// summation order (below), so every distance keeps its bits.
//
// Layout.  The float32 FULL path (distance.hpp, batch_dists) gives lane g of a vector's G-lane group the chunks
// c0 + cu * G + g, cu = 0 .. CU - 1, of every span [c0, c0 + G * CU) and accumulates them in that order.  A mirror row is
// row_bytes / 2 bytes of 16-byte UNITS; unit  c0 / 2 + j * G + g  (j = 0 .. CU / 2 - 1) holds, as 4 + 4 binary16 values,
// chunk c0 + (2j) * G + g followed by chunk c0 + (2j + 1) * G + g: lane g loads its CU / 2 units of a span with 16-byte loads
// that cover G * 16 contiguous bytes per instruction, and meets its chunks in the float32 order.  CU must be even.
#pragma once
#include <stdint.h>

#include "../../include/flatnav_hip.h"
#include "search_types.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FNV_HALF_HD __host__ __device__
#else
#define FNV_HALF_HD
#endif

namespace fnv_dev {

// Rows that can have a mirror: float32, whole spans (FULL), no side table, an even number of loads per lane and span --
// kCfgs {8,2} {8,4} {16,4} {32,4} {64,4}: rows of 64, 128, 256, 512 and 1024 k float32 elements, and rows padded to those.
inline bool half_rows_eligible(int data_type, int cfg, bool full, uint32_t tail_chunks) {
  return data_type == FNV_DTYPE_FLOAT32 && full && tail_chunks == 0 && cfg >= 0 && cfg < kNumCfgs && kCfgs[cfg].CU % 2 == 0;
}
template <class RowGeometry>  // (launch_plan.hpp's RowGeometry)
inline bool half_rows_eligible(int data_type, const RowGeometry& g) {
  return half_rows_eligible(data_type, g.cfg, g.full, g.tail_chunks);
}

// Where float32 chunk `c` of a row lives in the mirror row: the unit, and which half of it (0: bytes 0-7, 1: bytes 8-15).
struct HalfUnit {
  uint32_t unit, half;
};
FNV_HALF_HD inline HalfUnit half_unit_of_chunk(uint32_t c, uint32_t G, uint32_t CU) {
  const uint32_t span = G * CU;
  const uint32_t c0 = c / span * span, r = c - c0;
  const uint32_t cu = r / G, g = r % G;
  return HalfUnit{c0 / 2 + (cu / 2) * G + g, cu & 1u};
}

// ... and back: the first of the two chunks in mirror unit `u` (the second one is G chunks further on).
FNV_HALF_HD inline uint32_t half_first_chunk_of_unit(uint32_t u, uint32_t G, uint32_t CU) {
  const uint32_t span_units = G * CU / 2;
  const uint32_t r = u % span_units;
  return u / span_units * (G * CU) + (r / G) * 2 * G + r % G;
}

// binary16 <-> float32 on bit patterns.  half_bits_trunc drops what binary16 cannot hold (no rounding): for a value that
// binary16 represents it is the exact conversion, and for every other value widening its result gives back other bits.
FNV_HALF_HD inline uint16_t half_bits_trunc(uint32_t f) {
  const uint32_t sign = (f >> 16) & 0x8000u, e = (f >> 23) & 0xFFu, m = f & 0x7FFFFFu;
  if (e == 0xFFu) return (uint16_t)(sign | 0x7C00u | (m >> 13));  // inf; NaN: the payload's top ten bits
  const int e32 = (int)e - 127;
  if (e32 > 15) return (uint16_t)(sign | 0x7C00u);                 // too large: not representable
  if (e32 >= -14) return (uint16_t)(sign | (uint32_t)(e32 + 15) << 10 | (m >> 13));
  const int shift = 13 + (-14 - e32);                              // binary16 subnormals: multiples of 2^-24
  if (e == 0u || shift > 24) return (uint16_t)sign;                // zero, float32 subnormals, below 2^-24
  return (uint16_t)(sign | ((m | 0x800000u) >> shift));
}
FNV_HALF_HD inline uint32_t half_bits_widen(uint16_t h) {
  const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, e = ((uint32_t)h >> 10) & 0x1Fu, m = (uint32_t)h & 0x3FFu;
  if (e == 0x1Fu) return sign | 0x7F800000u | (m << 13);
  if (e != 0u) return sign | (e + 112u) << 23 | (m << 13);
  if (m == 0u) return sign;
  int p = 9;  // leading bit of a subnormal: m * 2^-24 = 1.xxx * 2^(p - 24)
  while (!(m >> p)) p--;
  return sign | (uint32_t)(103 + p) << 23 | ((m << (23 - p)) & 0x7FFFFFu);
}
// Lossless: the float32 BIT PATTERN survives narrow-then-widen.  -0, binary16 subnormals, +-inf and the NaNs whose payload fits
// pass; 1/3, 2049, 65520, 2^-25 and NaNs that would change do not.
FNV_HALF_HD inline bool half_lossless(uint32_t f) { return half_bits_widen(half_bits_trunc(f)) == f; }

// One row: `row` = nchunks float32 chunks (4 values each, as bit patterns), `mirror` = nchunks * 4 binary16 values in the layout
// above.  Returns whether every element was lossless (the mirror row is only meaningful then).
FNV_HALF_HD inline bool half_convert_row(const uint32_t* row, uint16_t* mirror, uint32_t nchunks, uint32_t G, uint32_t CU) {
  bool ok = true;
  for (uint32_t c = 0; c < nchunks; c++) {
    const HalfUnit u = half_unit_of_chunk(c, G, CU);
    for (uint32_t k = 0; k < 4; k++) {
      const uint32_t f = row[c * 4 + k];
      const uint16_t h = half_bits_trunc(f);
      ok = ok && half_bits_widen(h) == f;
      mirror[u.unit * 8 + u.half * 4 + k] = h;
    }
  }
  return ok;
}

// What fnv_index_half_rows reports as a handle's mirror state.
enum : int { HALF_NONE = 0, HALF_LIVE = 1, HALF_DROPPED = 2, HALF_INELIGIBLE = 3 };

}  // namespace fnv_dev
