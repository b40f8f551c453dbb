// kernel_table.h -- part of the gfx950 search engine: how the host code finds a kernel instantiation.
// Every kernel is a template over <element type, metric, G lanes per vector, CU loads per lane, FULL rows>; the
// instantiations are compiled in separate translation units (kernel_inst.hip, once per element type x metric x
// kernel family, in parallel -- one unit with all of them takes a quarter of an hour) and registered here.
#pragma once
#include "scan_select.hpp"
#include "search_params.h"
#include "wire.hpp"

namespace fnv_dev {

typedef void (*kernel_fn)(const SearchParams);
typedef void (*wire_fn)(const WireParams);
typedef void (*scan_fn)(const ScanParams);
typedef void (*scan_grouped_fn)(const GroupedScanParams);

// All kernels for one (element type, metric): [row configuration][FULL rows].
struct KernelTable {
  kernel_fn exact[kNumCfgs][2];        // beam_search_kernel (two heaps, libstdc++-exact)
  kernel_fn exact_f[kNumCfgs][2];      // beam_search_filtered_kernel (the same, results restricted to a node bitmap)
  kernel_fn scan[kNumCfgs][2];         // entry_scan_kernel (K0)
  kernel_fn merged[kNumBeamForms][2][kNumCfgs][2];  // beam_search_merged_kernel, [beam form][DIRECT form] first
  wire_fn select[kNumCfgs][2];         // wire_select_kernel
  wire_fn connect[kNumCfgs][2];        // wire_connect_kernel
  scan_fn flat[kNumCfgs][2];           // exhaustive_scan_kernel (scan.hpp: the exhaustive search)
  scan_grouped_fn flat_g[kNumCfgs][2]; // exhaustive_scan_grouped_kernel (... with one filter per query)
};

// X(element type, type tag, metric ordinal, metric tag)
#define FNV_FOR_EACH_TYPE_METRIC(X) \
  X(float, f32, 0, l2) X(float, f32, 1, ip) X(uint8_t, u8, 0, l2) X(uint8_t, u8, 1, ip) X(int8_t, i8, 0, l2) X(int8_t, i8, 1, ip) \
  X(_Float16, f16, 0, l2) X(_Float16, f16, 1, ip)

// The kernel families, X(ordinal, name): one compilation of kernel_inst.hip (-DFNV_INST_FAMILY=ordinal -DFNV_INST_FNAME=name)
// per family and (type, metric) defines the filler fill_<name>_<type tag>_<metric tag>.  0 the exact two-heap kernel + entry
// scan, 12 its filtered form, 3 the wiring kernels, 4-7 the merged beam in MB_R / 1 / 0 (LDS) / 2 register chunks, 8-11 the
// DIRECT forms of 4-7 (small launches on small indexes: the visited set is a bitmap in LDS), 13 the exhaustive search's scan, 14 its grouped form.
#define FNV_FOR_EACH_FAMILY(X, ...)                                                                              \
  X(0, exact, __VA_ARGS__) X(12, exact_f, __VA_ARGS__) X(3, wire, __VA_ARGS__) X(4, merged, __VA_ARGS__)         \
  X(5, merged1, __VA_ARGS__) X(6, merged0, __VA_ARGS__) X(7, merged2, __VA_ARGS__) X(8, merged_d, __VA_ARGS__)   \
  X(9, merged1_d, __VA_ARGS__) X(10, merged0_d, __VA_ARGS__) X(11, merged2_d, __VA_ARGS__) X(13, scan, __VA_ARGS__)   \
  X(14, scan_g, __VA_ARGS__)

// The row format f32h (float32 queries on the half-width mirror of a float32 table, half_rows.hpp) has the exact family (without
// the entry scan) and the merged-beam families with their DIRECT forms only, for the FULL rows with an even CU; its tables'
// other slots are null.  X(metric ordinal, tag)
#define FNV_FOR_EACH_HALF_ROWS_METRIC(X) X(0, l2) X(1, ip)
#define FNV_FOR_EACH_HALF_ROWS_FAMILY(X, ...)                                                                            \
  X(0, exact, __VA_ARGS__) X(4, merged, __VA_ARGS__) X(5, merged1, __VA_ARGS__) X(6, merged0, __VA_ARGS__)               \
  X(7, merged2, __VA_ARGS__) X(8, merged_d, __VA_ARGS__) X(9, merged1_d, __VA_ARGS__) X(10, merged0_d, __VA_ARGS__)      \
  X(11, merged2_d, __VA_ARGS__)

#define FNV_DECLARE_FILLER(ordinal, family, tag, mtag) void fill_##family##_##tag##_##mtag(KernelTable& t);
#define FNV_DECLARE_FILLERS(T, tag, M, mtag) FNV_FOR_EACH_FAMILY(FNV_DECLARE_FILLER, tag, mtag)
FNV_FOR_EACH_TYPE_METRIC(FNV_DECLARE_FILLERS)
#undef FNV_DECLARE_FILLERS
#define FNV_DECLARE_FILLERS(M, mtag) FNV_FOR_EACH_HALF_ROWS_FAMILY(FNV_DECLARE_FILLER, f32h, mtag)
FNV_FOR_EACH_HALF_ROWS_METRIC(FNV_DECLARE_FILLERS)
#undef FNV_DECLARE_FILLERS
#undef FNV_DECLARE_FILLER

}  // namespace fnv_dev
