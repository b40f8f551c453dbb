// python_module.cpp -- pybind11 extension `flatnav_amd._core` (own implementation).
//
// Python surface of the reference's `flatnav._core` (python-bindings/src/flatnav/bindings.cpp:
// 426-539): submodules `index` (create(), IndexL2Float / IndexIPFloat / IndexL2Uint8 /
// IndexIPUint8 / IndexL2Int8 / IndexIPInt8, and IndexL2Float16 / IndexIPFloat16) and `data_type` (DataType), enum MetricType,
// __version__.  Methods, argument names, defaults, returned dtypes/shapes and raised exception
// types follow the reference; `search` hands the whole batch to the GPU in one call
// (flatnav::Index::searchBatch -> C ABI fnv_search_batch) instead of looping on the host.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cctype>
#include <cstdint>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include <flatnav/distances/InnerProductDistance.h>
#include <flatnav/distances/SquaredL2Distance.h>
#include <flatnav/index/Index.h>

namespace py = pybind11;
using flatnav::Index;
using flatnav::distances::InnerProductDistance;
using flatnav::distances::MetricType;
using flatnav::distances::SquaredL2Distance;
using flatnav::util::DataType;

namespace {

template <typename T>
using dense_array = py::array_t<T, py::array::c_style | py::array::forcecast>;

// Index wrapper exposed to Python.  dist_t fixes metric and element type; labels are int32.
template <typename dist_t, DataType kType>
class PyIndex : public std::enable_shared_from_this<PyIndex<dist_t, kType>> {
  using element_t = typename flatnav::util::type_for_data_type<kType>::type;
  using index_t = Index<dist_t, int>;

  int _dim;
  int _next_label = 0;
  std::unique_ptr<index_t> _index;

  // `a` as a C-contiguous array of the index element type.  float16 goes through numpy (pybind11 has no half type):
  // np.ascontiguousarray(a, float16) rounds float32 / float64 to nearest even, as forcecast turns float64 into float32.
  static py::array elements(const py::array& a) {
    if constexpr (kType == DataType::float16)
      return py::module_::import("numpy").attr("ascontiguousarray")(a, "float16").cast<py::array>();
    else
      return a.cast<dense_array<element_t>>();
  }

 public:
  explicit PyIndex(std::unique_ptr<index_t> loaded) : _dim(static_cast<int>(loaded->dataDimension())), _index(std::move(loaded)) {}

  PyIndex(int dim, int dataset_size, int max_edges_per_node, bool verbose, bool collect_stats)
      : _dim(dim),
        _index(new index_t(dist_t::create(static_cast<size_t>(dim)), dataset_size, max_edges_per_node, collect_stats, kType)) {
    if (verbose) {
      const double gb = static_cast<double>(_index->getTotalIndexMemory() + _index->mutexesAllocatedMemory()) / 1e9;
      py::print("Total allocated index memory:", gb, "GB");
      _index->getIndexSummary();
    }
  }

  // add(data, ef_construction, num_initializations=100, labels=None)   [bindings.cpp:64-119, 326-335]
  // device=True (extension): the insertions' beam searches run on the GPU in batches (Index::addBatchDevice).
  void add(const py::array& data_any, int ef_construction, int num_initializations, py::object labels, bool device,
           uint32_t device_max_batch, bool device_wiring, uint32_t device_bootstrap) {
    py::array data = elements(data_any);
    if (data.ndim() != 2 || data.shape(1) != _dim)
      throw std::invalid_argument("Data has incorrect dimensions. data.ndim() = `" + std::to_string(data.ndim()) +
                                  "`. Expected 2D array with dimensions (num_vectors, dim).");
    const size_t count = static_cast<size_t>(data.shape(0));
    std::vector<int> ids;
    if (labels.is_none()) {
      ids.resize(count);
      std::iota(ids.begin(), ids.end(), 0);
    } else {
      try {
        ids = py::cast<std::vector<int>>(labels);
      } catch (const py::cast_error&) {
        throw std::invalid_argument("Invalid labels provided.");
      }
      if (ids.size() != count) throw std::invalid_argument("Incorrect number of labels.");
    }
    void* raw = const_cast<void*>(data.data());
    py::gil_scoped_release release;  // the builder spawns its own threads
    if (device) {
      typename index_t::DeviceBuildOptions opt;
      if (device_max_batch) opt.max_batch = device_max_batch;
      if (device_bootstrap) opt.bootstrap = device_bootstrap;
      opt.wire_on_device = device_wiring;
      _index->template addBatchDevice<element_t>(raw, ids, ef_construction, num_initializations, opt);
    } else {
      _index->template addBatch<element_t>(raw, ids, ef_construction, num_initializations);
    }
  }

  // allocate_nodes(data) -> self   [bindings.cpp:308-324]: vectors only, no edges (used before
  // build_graph_links); labels continue from the wrapper's own counter.
  std::shared_ptr<PyIndex> allocateNodes(const py::array& data_any) {
    if constexpr (kType == DataType::float16) {  // rows are stored as float16 (the other types keep the reference's float rows)
      py::array data = elements(data_any);
      if (data.ndim() != 2 || data.shape(1) != _dim) throw std::invalid_argument("Data has incorrect dimensions.");
      for (py::ssize_t row = 0; row < data.shape(0); ++row) {
        uint32_t node;
        int label = _next_label++;
        _index->allocateNode(const_cast<void*>(data.data(row, 0)), label, node);
      }
      return this->shared_from_this();
    }
    dense_array<float> data = data_any.cast<dense_array<float>>();
    if (data.ndim() != 2 || data.shape(1) != _dim) throw std::invalid_argument("Data has incorrect dimensions.");
    for (py::ssize_t row = 0; row < data.shape(0); ++row) {
      uint32_t node;
      int label = _next_label++;
      _index->allocateNode(const_cast<float*>(data.data(row)), label, node);
    }
    return this->shared_from_this();
  }

  // The frame of every batched search: the queries as elements, the shape and K checks (`exhaustive`: K has an upper bound),
  // prepare(nq) -- the form's own arguments, still under the GIL --, the output arrays, run(qptr, nq, dptr, lptr) with the GIL
  // released (the GPU works; other Python threads may run), and the (float32[Q,K], int32[Q,K]) tuple.
  template <typename Prepare, typename Run>
  py::tuple searchBatched(const py::array& queries_any, int K, bool exhaustive, Prepare prepare, Run run) {
    py::array queries = elements(queries_any);
    if (queries.ndim() != 2 || queries.shape(1) != _dim) throw std::invalid_argument("Queries have incorrect dimensions.");
    if (exhaustive && (K <= 0 || K > 1024)) throw std::invalid_argument("K of an exhaustive search must be between 1 and 1024.");
    if (K <= 0) throw std::invalid_argument("K must be positive.");
    const py::ssize_t nq = queries.shape(0);
    prepare(nq);
    py::array_t<float> dist({nq, static_cast<py::ssize_t>(K)});
    py::array_t<int> labels({nq, static_cast<py::ssize_t>(K)});
    {
      const void* qptr = queries.data();
      float* dptr = dist.mutable_data();
      int* lptr = labels.mutable_data();
      py::gil_scoped_release release;
      run(qptr, static_cast<uint64_t>(nq), dptr, lptr);
    }
    return py::make_tuple(dist, labels);
  }

  // search(queries, K, ef_search, num_initializations=100) -> (float32[Q,K], int32[Q,K])
  py::tuple search(const py::array& queries_any, int K, int ef_search, int num_initializations) {
    std::vector<int32_t> counts;
    py::tuple out = searchBatched(
        queries_any, K, false, [&](py::ssize_t nq) { counts.resize(static_cast<size_t>(nq)); },
        [&](const void* qptr, uint64_t nq, float* dptr, int* lptr) {
          _index->searchBatch(qptr, nq, K, ef_search, num_initializations, dptr, lptr, counts.data());
        });
    for (int32_t count : counts)  // bindings.cpp:184-189
      if (count != K)
        throw std::runtime_error("Search did not return the expected number of results. Expected " + std::to_string(K) +
                                 " but got " + std::to_string(count) + ".");
    return out;
  }

  // `allowed` (1-D bool mask indexed by label, or 1-D integer array of labels) -> the C ABI's bitmap over label values
  static void packAllowed(const py::array& allowed_any, std::vector<uint8_t>& bits, uint64_t& n_bits) {
    if (allowed_any.ndim() != 1) throw std::invalid_argument("allowed must be a 1-D bool mask or a 1-D array of labels.");
    constexpr uint64_t kMaxBits = uint64_t(1) << 31;
    if (allowed_any.dtype().kind() == 'b') {
      auto mask = allowed_any.cast<dense_array<bool>>();
      n_bits = static_cast<uint64_t>(mask.size());
      if (n_bits > kMaxBits) throw std::invalid_argument("allowed mask longer than 2^31 labels.");
      bits.assign((n_bits + 7) / 8, 0);
      for (uint64_t i = 0; i < n_bits; ++i)
        if (mask.data()[i]) bits[i >> 3] |= static_cast<uint8_t>(1u << (i & 7));
    } else if (allowed_any.size() == 0 || allowed_any.dtype().kind() == 'i' || allowed_any.dtype().kind() == 'u') {
      auto ids = allowed_any.cast<dense_array<int64_t>>();
      int64_t top = -1;
      for (py::ssize_t i = 0; i < ids.size(); ++i) {
        if (ids.data()[i] < 0) throw std::invalid_argument("allowed labels must be non-negative.");
        top = std::max(top, ids.data()[i]);
      }
      n_bits = static_cast<uint64_t>(top + 1);
      if (n_bits > kMaxBits) throw std::invalid_argument("allowed label does not fit an int32 label.");
      bits.assign((n_bits + 7) / 8, 0);
      for (py::ssize_t i = 0; i < ids.size(); ++i) bits[static_cast<size_t>(ids.data()[i]) >> 3] |= static_cast<uint8_t>(1u << (ids.data()[i] & 7));
    } else {
      throw std::invalid_argument("allowed must be a bool mask or an integer array of labels.");
    }
  }

  // search_filtered(queries, K, ef_search, allowed, num_initializations=100) -> (float32[Q,K], int32[Q,K]): the k-NN among the
  // nodes whose label is allowed; `allowed` = 1-D bool mask indexed by label, or 1-D integer array of labels (order and
  // duplicates ignored, a negative label raises ValueError).  Short rows are padded with (+inf, -1), never raised on.
  py::tuple searchFiltered(const py::array& queries_any, int K, int ef_search, const py::array& allowed_any, int num_initializations) {
    std::vector<uint8_t> bits;
    uint64_t n_bits = 0;
    return searchBatched(
        queries_any, K, false, [&](py::ssize_t) { packAllowed(allowed_any, bits, n_bits); },
        [&](const void* qptr, uint64_t nq, float* dptr, int* lptr) {
          _index->searchBatchFiltered(qptr, nq, K, ef_search, num_initializations, bits.empty() ? nullptr : bits.data(), n_bits, dptr, lptr,
                                      nullptr);
        });
  }

  // search_exhaustive(queries, K, allowed=None) -> (float32[Q,K], int32[Q,K]): the exact K nearest among all nodes, or among
  // those whose label is allowed (`allowed` as for search_filtered), by one device scan; sorted by (distance, node id).
  // Short rows are padded with (+inf, -1), never raised on.
  py::tuple searchExhaustive(const py::array& queries_any, int K, const py::object& allowed_obj) {
    std::vector<uint8_t> bits;
    uint64_t n_bits = 0;
    const bool use_filter = !allowed_obj.is_none();
    return searchBatched(
        queries_any, K, true,
        [&](py::ssize_t) {
          if (!use_filter) return;
          py::array allowed_any = py::array::ensure(allowed_obj);
          if (!allowed_any) throw std::invalid_argument("allowed must be a bool mask or an integer array of labels.");
          packAllowed(allowed_any, bits, n_bits);
        },
        [&](const void* qptr, uint64_t nq, float* dptr, int* lptr) {
          _index->searchBatchExhaustive(qptr, nq, K, bits.empty() ? nullptr : bits.data(), n_bits, use_filter, dptr, lptr, nullptr);
        });
  }

  // `filters` (a sequence of what packAllowed takes, or a 2-D bool mask [F, labels]) -> the C ABI's filter table: F rows of
  // `stride` bytes, n_bits = the largest of the filters' own
  static void packFilters(const py::object& filters_obj, std::vector<uint8_t>& table, uint64_t& n_filters, uint64_t& stride,
                          uint64_t& n_bits) {
    std::vector<std::vector<uint8_t>> rows;
    n_bits = 0;
    auto add = [&](const py::handle& one) {
      py::array a = py::array::ensure(one);
      if (!a) throw std::invalid_argument("a filter must be a bool mask or an integer array of labels.");
      rows.emplace_back();
      uint64_t nb = 0;
      packAllowed(a, rows.back(), nb);
      n_bits = std::max(n_bits, nb);
    };
    if (py::isinstance<py::array>(filters_obj) && py::reinterpret_borrow<py::array>(filters_obj).ndim() == 2) {
      py::array mask = py::reinterpret_borrow<py::array>(filters_obj);
      if (mask.dtype().kind() != 'b') throw std::invalid_argument("a 2-D filter table must be a bool mask [filters, labels].");
    }
    for (py::handle one : filters_obj) add(one);
    n_filters = rows.size();
    stride = (n_bits + 7) / 8;
    table.assign(static_cast<size_t>(n_filters * stride), 0);
    for (size_t f = 0; f < rows.size(); ++f) std::copy(rows[f].begin(), rows[f].end(), table.begin() + static_cast<py::ssize_t>(f * stride));
  }
  static std::vector<int32_t> queryFilter(const py::array& qf_any, py::ssize_t nq, uint64_t n_filters) {
    if (qf_any.ndim() != 1 || qf_any.shape(0) != nq) throw std::invalid_argument("query_filter must hold one entry per query.");
    if (qf_any.size() && qf_any.dtype().kind() != 'i' && qf_any.dtype().kind() != 'u')
      throw std::invalid_argument("query_filter must be an integer array.");
    auto v = qf_any.cast<dense_array<int64_t>>();
    std::vector<int32_t> out(static_cast<size_t>(nq));
    for (py::ssize_t q = 0; q < nq; ++q) {
      if (v.data()[q] < -1 || v.data()[q] >= static_cast<int64_t>(n_filters))
        throw std::invalid_argument("query_filter[" + std::to_string(q) + "] is neither -1 nor a filter of the table.");
      out[static_cast<size_t>(q)] = static_cast<int32_t>(v.data()[q]);
    }
    return out;
  }

  struct FilterTable {  // the grouped forms' own arguments as the C ABI takes them
    std::vector<uint8_t> table;
    uint64_t n_filters = 0, stride = 0, n_bits = 0;
    std::vector<int32_t> query_filter;
    void pack(const py::object& filters_obj, const py::array& query_filter_any, py::ssize_t nq) {
      packFilters(filters_obj, table, n_filters, stride, n_bits);
      query_filter = queryFilter(query_filter_any, nq, n_filters);
    }
    const uint8_t* data() const { return table.empty() ? nullptr : table.data(); }
  };

  // search_filtered_grouped(queries, K, ef_search, filters, query_filter, num_initializations=100): search_filtered with one
  // allowed set per query (query_filter[q] = its filter's row in `filters`, -1 = none), in one launch.
  py::tuple searchFilteredGrouped(const py::array& queries_any, int K, int ef_search, const py::object& filters_obj,
                                  const py::array& query_filter_any, int num_initializations) {
    FilterTable f;
    return searchBatched(
        queries_any, K, false, [&](py::ssize_t nq) { f.pack(filters_obj, query_filter_any, nq); },
        [&](const void* qptr, uint64_t nq, float* dptr, int* lptr) {
          _index->searchBatchFilteredGrouped(qptr, nq, K, ef_search, num_initializations, f.data(), f.n_filters, f.stride, f.n_bits,
                                             f.query_filter.data(), dptr, lptr, nullptr);
        });
  }

  // search_exhaustive_grouped(queries, K, filters, query_filter): search_exhaustive with one allowed set per query.
  py::tuple searchExhaustiveGrouped(const py::array& queries_any, int K, const py::object& filters_obj, const py::array& query_filter_any) {
    FilterTable f;
    return searchBatched(
        queries_any, K, true, [&](py::ssize_t nq) { f.pack(filters_obj, query_filter_any, nq); },
        [&](const void* qptr, uint64_t nq, float* dptr, int* lptr) {
          _index->searchBatchExhaustiveGrouped(qptr, nq, K, f.data(), f.n_filters, f.stride, f.n_bits, f.query_filter.data(), dptr, lptr,
                                               nullptr);
        });
  }

  // search_single(query, K, ef_search, num_initializations=100) -> (float32[K], int32[K])
  py::tuple searchSingle(const py::array& query_any, int K, int ef_search, int num_initializations) {
    py::array query = elements(query_any);
    if (query.ndim() != 1 || query.shape(0) != _dim) throw std::invalid_argument("Query has incorrect dimensions.");
    auto top = _index->search(query.data(), K, ef_search, num_initializations);
    if (static_cast<int>(top.size()) != K)  // bindings.cpp:134-137
      throw std::runtime_error("Search did not return the expected number of results. Expected " + std::to_string(K) +
                               " but got " + std::to_string(top.size()) + ".");
    py::array_t<float> dist(static_cast<py::ssize_t>(K));
    py::array_t<int> labels(static_cast<py::ssize_t>(K));
    for (int i = 0; i < K; ++i) {
      dist.mutable_data()[i] = top[static_cast<size_t>(i)].first;
      labels.mutable_data()[i] = top[static_cast<size_t>(i)].second;
    }
    return py::make_tuple(dist, labels);
  }

  uint64_t getQueryDistanceComputations() {  // returns AND resets (bindings.cpp:270-274)
    const uint64_t v = _index->distanceComputations();
    _index->resetStats();
    return v;
  }
  void buildGraphLinks(const std::string& mtx_filename) { _index->buildGraphLinks(mtx_filename); }
  std::vector<std::vector<uint32_t>> getGraphOutdegreeTable() { return _index->getGraphOutdegreeTable(); }
  uint32_t getMaxEdgesPerNode() { return static_cast<uint32_t>(_index->maxEdgesPerNode()); }
  void reorder(const std::vector<std::string>& strategies) {
    for (const auto& s : strategies) {
      std::string lower = s;
      std::transform(lower.begin(), lower.end(), lower.begin(), [](unsigned char c) { return std::tolower(c); });
      if (lower != "gorder" && lower != "rcm")
        throw std::invalid_argument("`" + s + "` is not a supported graph re-ordering strategy.");
    }
    _index->doGraphReordering(strategies);
  }
  void setNumThreads(uint32_t n) { _index->setNumThreads(n); }
  uint32_t getNumThreads() { return _index->getNumThreads(); }
  void save(const std::string& filename) { _index->saveIndex(filename); }
  static std::shared_ptr<PyIndex> loadIndex(const std::string& filename) {
    return std::make_shared<PyIndex>(index_t::loadIndex(filename));
  }

  // ---- additions for the GPU build (not in the reference) -------------------------------------
  void setDevice(int ordinal) { _index->setDevice(ordinal); }
  void setDevices(const std::vector<int>& ordinals) { _index->setDevices(ordinals); }
  std::vector<int> devices() { return _index->devices(); }
  void syncDevice() { _index->syncDevice(); }
  void setFilterRouting(int64_t scan_max_allowed, bool scan_on_overflow) { _index->setFilterRouting(scan_max_allowed, scan_on_overflow); }
  uintptr_t deviceHandle() { return reinterpret_cast<uintptr_t>(_index->deviceHandle()); }
  uint64_t currentNumNodes() { return _index->currentNumNodes(); }
  // zero-copy view of the AoS node store (for tests: graph-equality checks against the oracle)
  py::array_t<uint8_t> rawBlob() {
    const uint64_t n = _index->getTotalIndexMemory();
    return py::array_t<uint8_t>({static_cast<py::ssize_t>(n)}, {1},
                                reinterpret_cast<const uint8_t*>(_index->rawIndexMemory()), py::cast(this->shared_from_this()));
  }
  size_t nodeSizeBytes() { return _index->nodeSizeBytes(); }
  size_t dataSizeBytes() { return _index->dataSizeBytes(); }
};

template <typename dist_t, DataType kType>
void bindIndex(py::module_& m, const char* name) {
  using T = PyIndex<dist_t, kType>;
  py::class_<T, std::shared_ptr<T>>(m, name)
      .def("add", &T::add, py::arg("data"), py::arg("ef_construction"), py::arg("num_initializations") = 100,
           py::arg("labels") = py::none(), py::kw_only(), py::arg("device") = false, py::arg("device_max_batch") = 0,
           py::arg("device_wiring") = true, py::arg("device_bootstrap") = 0,
           "Insert vectors (rows of `data`, cast to the index data type) into the graph.  device=True: the insertions "
           "run on the GPU in batches (deterministic; same graph family as the host builder; device_max_batch=1 "
           "inserts one node at a time and reproduces the single-threaded host / reference graph byte for byte on "
           "data whose distances are exact).  device_bootstrap: nodes inserted on the host before the first batch "
           "(default 2048).")
      .def("allocate_nodes", &T::allocateNodes, py::arg("data"),
           "Store vectors without creating edges (follow with build_graph_links).")
      .def("search_single", &T::searchSingle, py::arg("query"), py::arg("K"), py::arg("ef_search"),
           py::arg("num_initializations") = 100, "k-NN of one query on the GPU -> (distances[K], labels[K]).")
      .def("search", &T::search, py::arg("queries"), py::arg("K"), py::arg("ef_search"),
           py::arg("num_initializations") = 100,
           "Batched k-NN on the GPU (one kernel launch) -> (distances[Q,K] float32, labels[Q,K] int32).")
      .def("search_filtered", &T::searchFiltered, py::arg("queries"), py::arg("K"), py::arg("ef_search"), py::arg("allowed"),
           py::arg("num_initializations") = 100,
           "Batched k-NN among the nodes whose label is allowed (`allowed`: bool mask indexed by label, or integer labels) "
           "-> (distances[Q,K] float32, labels[Q,K] int32), rows padded with (+inf, -1) when fewer than K are allowed.")
      .def("search_exhaustive", &T::searchExhaustive, py::arg("queries"), py::arg("K"), py::arg("allowed") = py::none(),
           "Exact k-NN by one device scan over all nodes, or over the nodes whose label is allowed (`allowed` as for "
           "search_filtered) -> (distances[Q,K] float32, labels[Q,K] int32) sorted by (distance, node id), rows padded with "
           "(+inf, -1) when there are fewer than K candidates.  1 <= K <= 1024.")
      .def("search_filtered_grouped", &T::searchFilteredGrouped, py::arg("queries"), py::arg("K"), py::arg("ef_search"),
           py::arg("filters"), py::arg("query_filter"), py::arg("num_initializations") = 100,
           "search_filtered with one allowed set per query, in one launch: `filters` = a sequence of filters (each as `allowed` of "
           "search_filtered) or a 2-D bool mask [F, labels]; query_filter[q] = the filter query q uses, -1 = none.")
      .def("search_exhaustive_grouped", &T::searchExhaustiveGrouped, py::arg("queries"), py::arg("K"), py::arg("filters"),
           py::arg("query_filter"),
           "search_exhaustive with one allowed set per query, in one launch (`filters` / `query_filter` as for "
           "search_filtered_grouped; -1 = every node).  1 <= K <= 1024.")
      .def("get_query_distance_computations", &T::getQueryDistanceComputations,
           "Distance evaluations since the last call (needs collect_stats=True); resets the counter.")
      .def("save", &T::save, py::arg("filename"), "Write the index in flatnav's binary format.")
      .def("build_graph_links", &T::buildGraphLinks, py::arg("mtx_filename"),
           "Import edges from a MatrixMarket file written by the hnswlib fork's save_base_layer_graph.")
      .def("get_graph_outdegree_table", &T::getGraphOutdegreeTable, "Out-neighbour lists of every node.")
      .def("reorder", &T::reorder, py::arg("strategies"), "Relabel nodes with 'gorder' and/or 'rcm'.")
      .def("set_num_threads", &T::setNumThreads, py::arg("num_threads"), "Host threads used by add().")
      .def_static("load_index", &T::loadIndex, py::arg("filename"), "Load an index written by save().")
      .def_property_readonly("max_edges_per_node", &T::getMaxEdgesPerNode)
      .def_property_readonly("num_threads", &T::getNumThreads)
      // GPU-build additions
      .def("set_device", &T::setDevice, py::arg("ordinal"), "Use this one GPU.")
      .def("set_devices", &T::setDevices, py::arg("ordinals"),
           "GPUs that each hold a replica of the index; batched searches are sharded over them (default: the "
           "FLATNAV_DEVICES environment variable -- 'all' = every visible GPU --, else the primary GPU only).")
      .def_property_readonly("devices", &T::devices)
      .def("sync_device", &T::syncDevice, "Upload pending changes to HBM now instead of at the next search.")
      .def("set_filter_routing", &T::setFilterRouting, py::arg("scan_max_allowed") = 0, py::arg("scan_on_overflow") = false,
           "Filter routing of search_filtered / search_filtered_grouped: a query whose filter allows at most scan_max_allowed "
           "nodes (0 = off), and with scan_on_overflow one whose search runs out of candidate room (instead of the call "
           "raising), is answered by the exhaustive scan -- that row is search_exhaustive's.")
      .def("device_handle", &T::deviceHandle, "fnv_index_t of the device mirror as an integer.")
      .def("_raw_blob", &T::rawBlob)
      .def_property_readonly("_node_size_bytes", &T::nodeSizeBytes)
      .def_property_readonly("_data_size_bytes", &T::dataSizeBytes)
      .def_property_readonly("_cur_num_nodes", &T::currentNumNodes);
}

template <DataType kType>
py::object makeIndex(const std::string& distance_type, int dim, int dataset_size, int max_edges_per_node, bool verbose,
                     bool collect_stats) {
  std::string lower = distance_type;
  std::transform(lower.begin(), lower.end(), lower.begin(), [](unsigned char c) { return std::tolower(c); });
  if (lower != "l2" && lower != "angular")  // bindings.cpp:397-407
    throw std::invalid_argument("Invalid distance type: `" + lower +
                                "` during index construction. Valid options include `l2` and `angular`.");
  if (lower == "l2")
    return py::cast(std::make_shared<PyIndex<SquaredL2Distance<kType>, kType>>(dim, dataset_size, max_edges_per_node,
                                                                              verbose, collect_stats));
  return py::cast(std::make_shared<PyIndex<InnerProductDistance<kType>, kType>>(dim, dataset_size, max_edges_per_node,
                                                                                verbose, collect_stats));
}

}  // namespace

PYBIND11_MODULE(_core, m) {
  m.doc() = "flatnav_amd: MI355X-native flat navigable-small-world index (search on gfx950 through a C ABI)";
  m.attr("__version__") = "0.1.0";

  auto data_type = m.def_submodule("data_type");
  py::enum_<DataType>(data_type, "DataType")
      .value("float32", DataType::float32)
      .value("int8", DataType::int8)
      .value("uint8", DataType::uint8)
      .value("float16", DataType::float16)
      .export_values();

  py::enum_<MetricType>(m, "MetricType").value("L2", MetricType::L2).value("IP", MetricType::IP);

  auto index = m.def_submodule("index");
  bindIndex<SquaredL2Distance<DataType::float32>, DataType::float32>(index, "IndexL2Float");
  bindIndex<SquaredL2Distance<DataType::int8>, DataType::int8>(index, "IndexL2Int8");
  bindIndex<SquaredL2Distance<DataType::uint8>, DataType::uint8>(index, "IndexL2Uint8");
  bindIndex<InnerProductDistance<DataType::float32>, DataType::float32>(index, "IndexIPFloat");
  bindIndex<InnerProductDistance<DataType::int8>, DataType::int8>(index, "IndexIPInt8");
  bindIndex<InnerProductDistance<DataType::uint8>, DataType::uint8>(index, "IndexIPUint8");
  bindIndex<SquaredL2Distance<DataType::float16>, DataType::float16>(index, "IndexL2Float16");
  bindIndex<InnerProductDistance<DataType::float16>, DataType::float16>(index, "IndexIPFloat16");

  index.def(
      "create",
      [](const std::string& distance_type, int dim, int dataset_size, int max_edges_per_node, DataType index_data_type,
         bool verbose, bool collect_stats) -> py::object {
        switch (index_data_type) {
          case DataType::float32:
            return makeIndex<DataType::float32>(distance_type, dim, dataset_size, max_edges_per_node, verbose, collect_stats);
          case DataType::int8:
            return makeIndex<DataType::int8>(distance_type, dim, dataset_size, max_edges_per_node, verbose, collect_stats);
          case DataType::uint8:
            return makeIndex<DataType::uint8>(distance_type, dim, dataset_size, max_edges_per_node, verbose, collect_stats);
          case DataType::float16:
            return makeIndex<DataType::float16>(distance_type, dim, dataset_size, max_edges_per_node, verbose, collect_stats);
          default:
            throw std::runtime_error("Unsupported data type");
        }
      },
      py::arg("distance_type"), py::arg("dim"), py::arg("dataset_size"), py::arg("max_edges_per_node"),
      py::arg("index_data_type") = DataType::float32, py::arg("verbose") = false, py::arg("collect_stats") = false,
      "Create an index: distance_type 'l2' or 'angular' (1 - <x,y>, inputs are NOT normalised for you).");
}
