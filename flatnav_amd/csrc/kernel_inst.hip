// kernel_inst.hip -- one compilation = the instantiations of ONE kernel family for ONE (element type, metric):
//   hipcc -c -DFNV_INST_T=float -DFNV_INST_TAG=f32 -DFNV_INST_METRIC=0 -DFNV_INST_MTAG=l2 -DFNV_INST_FAMILY=4 -DFNV_INST_FNAME=merged ...
// The families (ordinal, name) are listed in kernel_table.h (FNV_FOR_EACH_FAMILY).
// flatnav_amd/build.py compiles the 104 combinations in parallel and links them with the host units -- and eighteen more for the
// row format f32h (float32 queries on the half-width mirror, half_rows.hpp; -DFNV_INST_T=fnv_dev::f32h -DFNV_INST_HALF_ROWS):
// the exact family (without the entry scan) and the merged-beam families with their DIRECT forms, for the row configurations
// a mirror exists for.
#include <hip/hip_runtime.h>

#include "kernel_table.h"
#include "kernels.hpp"
#include "merged_beam.hpp"
#include "scan.hpp"
#include "wire.hpp"

#define FNV_CAT_(a, b, c, d, e, f) a##b##c##d##e##f
#define FNV_CAT(a, b, c, d, e, f) FNV_CAT_(a, b, c, d, e, f)

namespace fnv_dev {

typedef FNV_INST_T T;
constexpr int METRIC = FNV_INST_METRIC;

// ROW(slot, kernel template, extra template arguments...) fills slot[cfg][full] for the eight row configurations
#ifdef FNV_INST_HALF_ROWS  // ... for the FULL rows with an even CU (half_rows_eligible); every other slot stays null
#define FNV_ROW(slot, K, ...)                                          \
  static_assert(FULL, "mirror rows are FULL rows");                    \
  slot[1][1] = K<T, METRIC, 8, 2, true __VA_ARGS__>;                   \
  slot[2][1] = K<T, METRIC, 8, 4, true __VA_ARGS__>;                   \
  slot[3][1] = K<T, METRIC, 16, 4, true __VA_ARGS__>;                  \
  slot[4][1] = K<T, METRIC, 32, 4, true __VA_ARGS__>;                  \
  slot[5][1] = K<T, METRIC, 64, 4, true __VA_ARGS__>;
#else
#define FNV_ROW(slot, K, ...)                                          \
  slot[0][FULL] = K<T, METRIC, 8, 1, FULL __VA_ARGS__>;                \
  slot[1][FULL] = K<T, METRIC, 8, 2, FULL __VA_ARGS__>;                \
  slot[2][FULL] = K<T, METRIC, 8, 4, FULL __VA_ARGS__>;                \
  slot[3][FULL] = K<T, METRIC, 16, 4, FULL __VA_ARGS__>;               \
  slot[4][FULL] = K<T, METRIC, 32, 4, FULL __VA_ARGS__>;               \
  slot[5][FULL] = K<T, METRIC, 64, 4, FULL __VA_ARGS__>;               \
  slot[6][FULL] = K<T, METRIC, 64, 3, FULL __VA_ARGS__>;               \
  slot[7][FULL] = K<T, METRIC, 8, 3, FULL __VA_ARGS__>;
#endif

template <bool FULL>
static void fill_rows(KernelTable& t) {
#if FNV_INST_FAMILY == 0
  FNV_ROW(t.exact, beam_search_kernel)
#ifndef FNV_INST_HALF_ROWS  // (K0 stages float32 rows in LDS: it keeps reading the float32 table)
  FNV_ROW(t.scan, entry_scan_kernel)
#endif
#elif FNV_INST_FAMILY == 12
  FNV_ROW(t.exact_f, beam_search_filtered_kernel)
#elif FNV_INST_FAMILY == 13
  FNV_ROW(t.flat, exhaustive_scan_kernel)
#elif FNV_INST_FAMILY == 14
  FNV_ROW(t.flat_g, exhaustive_scan_grouped_kernel)
#elif FNV_INST_FAMILY >= 4 && FNV_INST_FAMILY <= 11
  constexpr int kFormOfFamily[4] = {3, 1, 0, 2};  // families 4-7 (and 8-11): MB_R / one / no (LDS) / two register chunks
  constexpr int form = kFormOfFamily[(FNV_INST_FAMILY - 4) % 4];
  constexpr bool direct = FNV_INST_FAMILY >= 8;
  FNV_ROW(t.merged[form][direct], beam_search_merged_kernel, , kBeamFormR[form], direct)
#else
  FNV_ROW(t.select, wire_select_kernel)
  FNV_ROW(t.connect, wire_connect_kernel)
#endif
}

void FNV_CAT(fill_, FNV_INST_FNAME, _, FNV_INST_TAG, _, FNV_INST_MTAG)(KernelTable& t) {
#ifndef FNV_INST_HALF_ROWS
  fill_rows<false>(t);
#endif
  fill_rows<true>(t);
}

}  // namespace fnv_dev
