// distance_model_harness.cpp -- batch_dists (flatnav_amd/csrc/distance.hpp) for ONE (query, row) pair, lane by lane on the CPU:
// the reference of tests/test_distance_model.py (CPU) and tests/test_gpu_distance_bits.py (every reported distance, bit for
// bit).  Compiled with g++ as a shared library (ctypes); tests/half_rows_harness.cpp includes this file for the two emulations
// it used to hold (hrh_dist_f32, hrh_dist_half).  Compile with -ffp-contract=off: nothing but the written std::fmaf may fuse.
//
// What is restated: lane g of a G-lane group takes chunks g, g + G, ... of every span of G * CU chunks; a lane keeps two
// partial sums fed by fused multiply-adds (Dist<T, METRIC>::chunk); the lane's sum is a.x + a.y; group_sum<G> adds the lanes in
// its butterfly; finish ends it.  One function per branch of batch_dists: FULL rows, clamped rows, split rows, mirror rows.
// What is NOT restated: any layout rule -- (G, CU, FULL, tail_chunks, nchunks, q_chunks) come from the planner
// (tests/row_classes.py), the query and the row arrive zero padded to q_chunks chunks.
//
// One deviation at a time can be switched on (`mutant`): the model must be one that a wrong kernel would fail.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../flatnav_amd/csrc/half_rows.hpp"  // binary16 widening; search_types.h: kCfgs

namespace dm {

using namespace fnv_dev;

enum : int {
  MUT_NONE = 0,
  MUT_REVERSED = 1,     // m1: a lane's chunk order within a span reversed
  MUT_ACC = 2,          // m2: elements (dots) 0 1 2 3 .. feed acc x x y y .. instead of x y x y ..  (swapping x and y wholesale
                        //     is no deviation: a.x + a.y commutes)
  MUT_LEFT_RIGHT = 3,   // m3: group_sum replaced by a left-to-right sum of the lanes
  MUT_UNFUSED = 4,      // m4: every fused multiply-add replaced by multiply, round, add
  MUT_SKIP = 5,         // m5: clamped steps skipped rather than executed with zeros
  MUT_FLUSH_HALF = 6    // m6: binary16 subnormals flushed on widening
};
// float16 IP.  DOT_NONE: the kernels' arithmetic, one fused multiply-add per element.  The others: the candidate semantics of
// v_dot2_f32_f16, which the kernels used before it was read off the hardware (profiles/distance_bits.md) -- four two-element
// dots per chunk into a.x, a.y, a.x, a.y; kept so that the recorded probe (tests/golden/probes/dot2_probe.npz) stays checkable on the
// CPU.  Bits 0-1 = the form, bit 2 = binary16 subnormal inputs flushed, bit 3 = f32 subnormal accumulator / results flushed.
enum : int { DOT_NONE = -1 };
enum : int { DOT_EXACT = 0, DOT_FMA_01 = 1, DOT_FMA_10 = 2, DOT_PAIR_THEN_ADD = 3, DOT_FLUSH_IN = 4, DOT_FLUSH_F32 = 8 };

struct Form {
  int epc;       // elements per 16-byte chunk: 4 (float32) or 8 (float16, widened)
  int metric;
  int mutant;
  int dot;       // float16 IP only: DOT_NONE, or a candidate of the retired two-element dot
};

inline float as_float(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
inline uint32_t as_bits(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

// ---- exact sums: a 320-bit two's-complement integer in units of 2^-149 (every f32, and every product of two widened binary16
// values, is a whole number of them below 2^130) ----------------------------------------------------------------------------------
struct Wide {
  static constexpr int L = 10;
  uint32_t w[L] = {0};
  void add(double v) {  // v: a whole number of 2^-149, |v| < 2^130
    if (v == 0.0) return;
    int e;
    const double m = frexp(fabs(v), &e);
    uint64_t mant = (uint64_t)ldexp(m, 53);
    int shift = e - 53 + 149;
    while (shift < 0) {
      mant >>= 1;  // (trailing zeros: v is a multiple of 2^-149)
      shift++;
    }
    uint32_t t[L] = {0};
    const int limb = shift / 32, bit = shift % 32;
    const unsigned __int128 wide = (unsigned __int128)mant << bit;
    for (int i = 0; i < 4 && limb + i < L; i++) t[limb + i] = (uint32_t)(wide >> (32 * i));
    uint64_t carry = 0;
    if (v > 0) {
      for (int i = 0; i < L; i++) {
        const uint64_t s = (uint64_t)w[i] + t[i] + carry;
        w[i] = (uint32_t)s;
        carry = s >> 32;
      }
    } else {
      for (int i = 0; i < L; i++) {
        const uint64_t s = (uint64_t)w[i] - t[i] - carry;
        w[i] = (uint32_t)s;
        carry = (s >> 32) & 1u;
      }
    }
  }
  // round to nearest, ties to even; `zero_sign`: the sign of an exact zero (the IEEE sum's)
  float to_float(bool negative_zero) const {
    uint32_t m[L];
    memcpy(m, w, sizeof(m));
    const bool neg = (m[L - 1] >> 31) != 0;
    if (neg) {
      uint64_t carry = 1;
      for (int i = 0; i < L; i++) {
        const uint64_t s = (uint64_t)(uint32_t)~m[i] + carry;
        m[i] = (uint32_t)s;
        carry = s >> 32;
      }
    }
    int top = -1;
    for (int i = L * 32 - 1; i >= 0; i--)
      if ((m[i / 32] >> (i % 32)) & 1u) {
        top = i;
        break;
      }
    if (top < 0) return negative_zero ? -0.0f : 0.0f;
    auto bit = [&](int i) { return i < 0 ? 0u : (m[i / 32] >> (i % 32)) & 1u; };
    const int shift = top > 23 ? top - 23 : 0;
    uint32_t keep = 0;
    for (int i = top; i >= shift; i--) keep = keep << 1 | bit(i);
    if (shift > 0) {
      bool sticky = false;
      for (int i = shift - 2; i >= 0 && !sticky; i--) sticky = bit(i) != 0;
      if (bit(shift - 1) && (sticky || (keep & 1u))) keep++;  // (2^24 is representable: ldexp takes it)
    }
    const float r = (float)ldexp((double)keep, shift - 149);  // exact, or +inf beyond the range
    return neg ? -r : r;
  }
};

// a + b in double with its rounding error (Knuth): a + b = s + e exactly
inline double two_sum(double a, double b, double& e) {
  const double s = a + b, bb = s - a;
  e = (a - (s - bb)) + (b - bb);
  return s;
}
// The exact sum of the terms rounded ONCE to f32.  Fast path: where the double sums carry no error the double IS the exact
// sum, and its conversion rounds once; otherwise the wide integer.
inline float exact_sum_f32(double p0, double p1, double c) {
  double e1, e2;
  const double s = two_sum(two_sum(p0, p1, e1), c, e2);
  if (e1 == 0.0 && e2 == 0.0 && s != 0.0) return (float)s;
  Wide w;
  w.add(p0), w.add(p1), w.add(c);
  return w.to_float(std::signbit(p0) && std::signbit(p1) && std::signbit(c));  // an exact zero: -0 only if every term is -0
}

inline float flush_f32(float v) { return (v != 0.f && fabsf(v) < 1.17549435e-38f) ? copysignf(0.f, v) : v; }
inline float flush_half(float v) { return (v != 0.f && fabsf(v) < 6.103515625e-05f) ? copysignf(0.f, v) : v; }  // |v| < 2^-14

// v_dot2_f32_f16 on widened operands: a0 * b0 + a1 * b1 + c under the candidate semantics of `mode`
float dot2(float a0, float b0, float a1, float b1, float c, int mode) {
  if (mode & DOT_FLUSH_IN) a0 = flush_half(a0), b0 = flush_half(b0), a1 = flush_half(a1), b1 = flush_half(b1);
  const bool ftz = (mode & DOT_FLUSH_F32) != 0;
  if (ftz) c = flush_f32(c);
  const double p0 = (double)a0 * (double)b0, p1 = (double)a1 * (double)b1;  // exact: 11 x 11 bits
  float r;
  switch (mode & 3) {
    case DOT_EXACT: {
      r = exact_sum_f32(p0, p1, (double)c);
      break;
    }
    case DOT_FMA_01: {
      float t = std::fmaf(a0, b0, c);
      if (ftz) t = flush_f32(t);
      r = std::fmaf(a1, b1, t);
      break;
    }
    case DOT_FMA_10: {
      float t = std::fmaf(a1, b1, c);
      if (ftz) t = flush_f32(t);
      r = std::fmaf(a0, b0, t);
      break;
    }
    default: {
      float t = exact_sum_f32(p0, p1, -0.0);
      if (ftz) t = flush_f32(t);
      r = t + c;
      break;
    }
  }
  return ftz ? flush_f32(r) : r;
}

struct Acc {
  float x = 0.f, y = 0.f;
};
inline float mul_add(float a, float b, float c, const Form& f) {
  if (f.mutant == MUT_UNFUSED) {
    const float p = a * b;
    return p + c;
  }
  return std::fmaf(a, b, c);
}
// Dist<T, METRIC>::chunk on widened values: x = one query chunk, y = one row chunk.
//   float32 (4 elements):  packed differences, then two packed fmas: elements 0, 2 into a.x and 1, 3 into a.y
//   float16 L2 (8):        per pair t = x - y (one f32 rounding, v_fma_mix_f32), fma(t, t, acc): element 2k into a.x, 2k + 1 into a.y
//   float16 IP (8):        fma(x, y, acc) per element (v_fma_mix_f32): element 2k into a.x, 2k + 1 into a.y
void chunk(Acc& a, const float* x, const float* y, const Form& f) {
  const bool grouped = f.mutant == MUT_ACC;
  if (f.epc == 8 && f.metric != FNV_METRIC_L2 && f.dot != DOT_NONE) {
    for (int d = 0; d < 4; d++) {
      float& t = ((grouped ? d >> 1 : d) & 1) ? a.y : a.x;
      t = dot2(x[2 * d], y[2 * d], x[2 * d + 1], y[2 * d + 1], t, f.dot);
    }
    return;
  }
  for (int k = 0; k < f.epc; k++) {
    float& t = ((grouped ? k >> 1 : k) & 1) ? a.y : a.x;
    if (f.metric == FNV_METRIC_L2) {
      const float d = x[k] - y[k];
      t = mul_add(d, d, t, f);
    } else {
      t = mul_add(x[k], y[k], t, f);
    }
  }
}
// group_sum<G>: every step adds the partner's value of the step before
float group_sum(std::vector<float> v, int G, int mutant = MUT_NONE) {
  if (mutant == MUT_LEFT_RIGHT) {
    float s = v[0];
    for (int i = 1; i < G; i++) s = s + v[i];
    return s;
  }
  auto step = [&](auto partner) {
    std::vector<float> w(v.size());
    for (int i = 0; i < G; i++) w[i] = v[i] + v[partner(i)];
    v = w;
  };
  step([](int i) { return i ^ 1; });
  step([](int i) { return i ^ 2; });
  if (G >= 8) step([](int i) { return (i & ~7) | (7 - (i & 7)); });
  if (G >= 16) step([](int i) { return (i & ~15) | (15 - (i & 15)); });
  if (G >= 32) step([](int i) { return i ^ 16; });
  if (G >= 64) step([](int i) { return i ^ 32; });
  for (int i = 1; i < G; i++)
    if (memcmp(&v[i], &v[0], 4) != 0) return NAN;  // (all lanes of a group end with the same bits)
  return v[0];
}
float finish(float s, int metric) { return metric == FNV_METRIC_L2 ? s : 1.0f - s; }

// FULL and clamped rows: lane g takes chunks c0 + cu * G + g in the order of cu, span after span.  Every lane runs all CU steps
// of every span; beyond the row (non-FULL rows only) the row operand is the query's chunk, which is zero there.
float dist_spans(const float* q, const float* row, uint32_t nchunks, int G, int CU, const Form& f) {
  std::vector<float> lane(G);
  for (int g = 0; g < G; g++) {
    Acc a;
    for (uint32_t c0 = 0; c0 < nchunks; c0 += G * CU)
      for (int i = 0; i < CU; i++) {
        const int cu = f.mutant == MUT_REVERSED ? CU - 1 - i : i;
        const uint32_t c = c0 + cu * G + g;
        const bool in_row = c < nchunks;
        if (!in_row && f.mutant == MUT_SKIP) continue;
        chunk(a, q + (size_t)f.epc * c, (in_row ? row : q) + (size_t)f.epc * c, f);
      }
    lane[g] = a.x + a.y;
  }
  return finish(group_sum(lane, G, f.mutant), f.metric);
}
// Split rows (G = 8, CU = 3, not FULL): chunks g, g + 8, g + 16 from the main part, then chunk 24 + g from the side table -- a
// zero chunk for lanes g >= tail_chunks -- against chunk 24 + g of the query.  `row`: the main part's 24 chunks followed by the
// side table's.
float dist_split(const float* q, const float* row, uint32_t tail_chunks, const Form& f) {
  const int G = 8, CU = 3;
  const float zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  std::vector<float> lane(G);
  for (int g = 0; g < G; g++) {
    Acc a;
    for (int i = 0; i <= CU; i++) {
      const int cu = f.mutant == MUT_REVERSED ? CU - i : i;
      const uint32_t c = cu * G + g;
      const bool has = cu < CU || (uint32_t)g < tail_chunks;
      if (!has && f.mutant == MUT_SKIP) continue;
      chunk(a, q + (size_t)f.epc * c, has ? row + (size_t)f.epc * c : zero, f);
    }
    lane[g] = a.x + a.y;
  }
  return finish(group_sum(lane, G, f.mutant), f.metric);
}
// The mirror kernel: lane g loads units c0 / 2 + j * G + g and multiplies the first four values with query chunk
// c0 + (2j) * G + g, the last four with chunk c0 + (2j + 1) * G + g.  `swap`: the two halves of every unit change places.
float dist_mirror(const float* q, const uint16_t* mirror, uint32_t nchunks, int G, int CU, int swap, const Form& f) {
  std::vector<float> lane(G);
  for (int g = 0; g < G; g++) {
    Acc a;
    for (uint32_t c0 = 0; c0 < nchunks; c0 += G * CU)
      for (int j = 0; j < CU / 2; j++) {
        const uint16_t* u = mirror + (size_t)(c0 / 2 + j * G + g) * 8;
        float y[8];
        for (int k = 0; k < 8; k++) y[k] = as_float(half_bits_widen(u[swap ? (k + 4) % 8 : k]));
        chunk(a, q + 4 * (c0 + (2 * j) * G + g), y, f);
        chunk(a, q + 4 * (c0 + (2 * j + 1) * G + g), y + 4, f);
      }
    lane[g] = a.x + a.y;
  }
  return finish(group_sum(lane, G, f.mutant), f.metric);
}

}  // namespace dm

extern "C" {

// The float32 kernel on FULL rows, and the mirror kernel (tests/test_half_rows.py, tests/test_distance_model.py).
float hrh_dist_f32(const float* q, const float* row, uint32_t nchunks, int G, int CU, int metric) {
  return dm::dist_spans(q, row, nchunks, G, CU, dm::Form{4, metric, dm::MUT_NONE, dm::DOT_NONE});
}
float hrh_dist_half(const float* q, const uint16_t* mirror, uint32_t nchunks, int G, int CU, int metric, int swap) {
  return dm::dist_mirror(q, mirror, nchunks, G, CU, swap, dm::Form{4, metric, dm::MUT_NONE, dm::DOT_NONE});
}

int dm_num_cfgs() { return fnv_dev::kNumCfgs; }
void dm_cfg(int cfg, int* G, int* CU) {
  *G = fnv_dev::kCfgs[cfg].G;
  *CU = fnv_dev::kCfgs[cfg].CU;
}
// One two-element dot on binary16 bit patterns and an f32 accumulator's bits -> the result's bits.
uint32_t dm_dot2(uint16_t a0, uint16_t b0, uint16_t a1, uint16_t b1, uint32_t c, int mode) {
  using namespace dm;
  return as_bits(dot2(as_float(fnv_dev::half_bits_widen(a0)), as_float(fnv_dev::half_bits_widen(b0)), as_float(fnv_dev::half_bits_widen(a1)),
                      as_float(fnv_dev::half_bits_widen(b1)), as_float(c), mode));
}
// The distance bits of every (query, row): out[nq][n].  `half` = 0: Q and X hold float32, 1: binary16 bit patterns; both
// [.][q_chunks * elements per chunk], zero padded (a split row: the main part's chunks, then the side table's).  Returns 0, or
// 1 for a geometry batch_dists has no branch for.
int dm_distances(int half, int metric, const void* Q, int64_t nq, const void* X, int64_t n, int cfg, int full, uint32_t tail_chunks,
                 uint32_t nchunks, uint32_t q_chunks, int mutant, int dot_mode, uint32_t* out) {
  using namespace dm;
  if (cfg < 0 || cfg >= fnv_dev::kNumCfgs) return 1;
  const int G = fnv_dev::kCfgs[cfg].G, CU = fnv_dev::kCfgs[cfg].CU;
  const uint32_t per_span = (uint32_t)(G * CU);
  const bool split = tail_chunks != 0;
  if (split ? (G != 8 || CU != 3 || full || nchunks != per_span || q_chunks != nchunks + G || tail_chunks > (uint32_t)G)
            : (q_chunks != (nchunks + per_span - 1) / per_span * per_span || (full != 0) != (nchunks % per_span == 0)))
    return 1;
  const Form f{half ? 8 : 4, metric, mutant, dot_mode};
  const size_t width = (size_t)q_chunks * f.epc;
  auto widen = [&](const void* src, int64_t rows) {
    std::vector<float> v((size_t)rows * width);
    if (!half) {
      memcpy(v.data(), src, v.size() * 4);
    } else {
      const uint16_t* h = (const uint16_t*)src;
      for (size_t i = 0; i < v.size(); i++) {
        const float w = as_float(fnv_dev::half_bits_widen(h[i]));
        v[i] = mutant == MUT_FLUSH_HALF ? flush_half(w) : w;
      }
    }
    return v;
  };
  const std::vector<float> q = widen(Q, nq), x = widen(X, n);
  for (int64_t i = 0; i < nq; i++)
    for (int64_t j = 0; j < n; j++) {
      const float* qi = q.data() + i * width;
      const float* xj = x.data() + j * width;
      const float d = split ? dist_split(qi, xj, tail_chunks, f) : dist_spans(qi, xj, nchunks, G, CU, f);
      out[i * n + j] = as_bits(d);
    }
  return 0;
}

}  // extern "C"
