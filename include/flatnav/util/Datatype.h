// flatnav/util/Datatype.h -- element-type tags of the host API (own implementation).
//
// Mirrors the public names of the reference's include/flatnav/util/Datatype.h:11-186 so user
// code compiles unchanged: flatnav::util::DataType, name(), type(), size(),
// type_for_data_type<>, for_each_data_type<>.  The ordinal of each enumerator is part of the
// on-disk index format (it is the first int32 of a saved index, Index.h:136 of the reference)
// and of the C ABI (FNV_DTYPE_*), so the order below must never change.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string_view>
#include <utility>
#if defined(__F16C__)
#include <immintrin.h>
#endif

namespace flatnav::util {

// Storage type of a float16 index element: the 16 bits of an IEEE binary16 value (the host compiler has no _Float16 in
// C++ on x86).  Distances never compute in half precision: widen() is exact, and the host kernels run in float on the
// widened values (HostKernels.h).  narrow() rounds to nearest, ties to even -- numpy's float32 -> float16.
struct float16_t {
  std::uint16_t bits;
};
static_assert(sizeof(float16_t) == 2, "float16_t must be two bytes");

inline float widen(float16_t h) {
#if defined(__F16C__)
  return _cvtsh_ss(h.bits);
#else
  const std::uint32_t sign = static_cast<std::uint32_t>(h.bits & 0x8000u) << 16;
  std::uint32_t exp = (h.bits >> 10) & 0x1Fu, man = h.bits & 0x3FFu, u;
  if (exp == 0x1Fu) {
    u = sign | 0x7F800000u | (man << 13);  // inf / NaN
  } else if (exp != 0) {
    u = sign | ((exp + 112u) << 23) | (man << 13);
  } else if (man == 0) {
    u = sign;
  } else {  // subnormal: renormalise
    int e = -1;
    do {
      man <<= 1;
      ++e;
    } while (!(man & 0x400u));
    u = sign | ((112u - static_cast<std::uint32_t>(e)) << 23) | ((man & 0x3FFu) << 13);
  }
  float f;
  std::memcpy(&f, &u, 4);
  return f;
#endif
}

inline float16_t narrow(float f) {
#if defined(__F16C__)
  return float16_t{static_cast<std::uint16_t>(_cvtss_sh(f, _MM_FROUND_TO_NEAREST_INT))};
#else
  std::uint32_t u;
  std::memcpy(&u, &f, 4);
  const std::uint16_t sign = static_cast<std::uint16_t>((u >> 16) & 0x8000u);
  const std::uint32_t a = u & 0x7FFFFFFFu;
  if (a >= 0x7F800000u) return float16_t{static_cast<std::uint16_t>(sign | 0x7C00u | (a > 0x7F800000u ? 0x200u : 0u))};
  if (a >= 0x477FF000u) return float16_t{static_cast<std::uint16_t>(sign | 0x7C00u)};  // rounds to >= 2^16: inf
  if (a < 0x38800000u) {  // below 2^-14: subnormal (or zero) result, one rounding of the exact value
    const std::uint32_t shift = 126u - (a >> 23);
    if (shift > 24u) return float16_t{sign};
    const std::uint32_t m = (a & 0x7FFFFFu) | 0x800000u;
    std::uint32_t r = m >> shift;
    const std::uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (r & 1u))) ++r;
    return float16_t{static_cast<std::uint16_t>(sign | r)};
  }
  std::uint32_t r = a - 0x38000000u;  // rebias 127 -> 15, keep 13 extra mantissa bits
  r = (r + 0xFFFu + ((r >> 13) & 1u)) >> 13;
  return float16_t{static_cast<std::uint16_t>(sign | r)};
#endif
}

// n elements at once (F16C: eight per instruction).
inline void widen(const float16_t* src, float* dst, std::size_t n) {
  std::size_t i = 0;
#if defined(__F16C__)
  for (; i + 8 <= n; i += 8)
    _mm256_storeu_ps(dst + i, _mm256_cvtph_ps(_mm_loadu_si128(reinterpret_cast<const __m128i*>(src + i))));
#endif
  for (; i < n; ++i) dst[i] = widen(src[i]);
}

inline void narrow(const float* src, float16_t* dst, std::size_t n) {
  std::size_t i = 0;
#if defined(__F16C__)
  for (; i + 8 <= n; i += 8)
    _mm_storeu_si128(reinterpret_cast<__m128i*>(dst + i), _mm256_cvtps_ph(_mm256_loadu_ps(src + i), _MM_FROUND_TO_NEAREST_INT));
#endif
  for (; i < n; ++i) dst[i] = narrow(src[i]);
}

enum class DataType : int {
  uint8 = 0, uint16 = 1, uint32 = 2, uint64 = 3,
  int8 = 4, int16 = 5, int32 = 6, int64 = 7,
  float16 = 8, float32 = 9, float64 = 10,
  undefined = 11
};

namespace detail {
struct DataTypeRow {
  DataType tag;
  const char* label;
  std::size_t bytes;
};
inline constexpr DataTypeRow kDataTypeTable[] = {
    {DataType::uint8, "uint8", 1},     {DataType::uint16, "uint16", 2},   {DataType::uint32, "uint32", 4},
    {DataType::uint64, "uint64", 8},   {DataType::int8, "int8", 1},       {DataType::int16, "int16", 2},
    {DataType::int32, "int32", 4},     {DataType::int64, "int64", 8},     {DataType::float16, "float16", 2},
    {DataType::float32, "float32", 4}, {DataType::float64, "float64", 8},
};
}  // namespace detail

inline constexpr const char* name(DataType t) {
  for (const auto& row : detail::kDataTypeTable)
    if (row.tag == t) return row.label;
  return "undefined";
}

inline constexpr DataType type(const std::string_view& label) {
  for (const auto& row : detail::kDataTypeTable)
    if (label == row.label) return row.tag;
  return DataType::undefined;
}

inline constexpr std::size_t size(DataType t) {
  for (const auto& row : detail::kDataTypeTable)
    if (row.tag == t) return row.bytes;
  return 0;
}

// DataType -> C++ element type, for the four element types an index can hold.
template <DataType>
struct type_for_data_type;
template <>
struct type_for_data_type<DataType::float32> { using type = float; };
template <>
struct type_for_data_type<DataType::float16> { using type = float16_t; };
template <>
struct type_for_data_type<DataType::int8> { using type = std::int8_t; };
template <>
struct type_for_data_type<DataType::uint8> { using type = std::uint8_t; };

// for_each_data_type<F, tags...>::apply(f) calls f.template operator()<tag>() for each tag.
template <typename F, DataType... tags>
struct for_each_data_type {
  static void apply(F&& f) { (f.template operator()<tags>(), ...); }
};

}  // namespace flatnav::util
