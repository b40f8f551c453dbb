// Drives flatnav::Index through every path of its device mirror (include/flatnav/index/DeviceMirror.h) against the recording
// C ABI of tests/cpp/fake_hip_abi.cpp: plain g++, no HIP library, no GPU.  stdout is the log -- a "-- scenario" line, what the
// driver did ("> ...") and what reached the library -- which tests/test_device_mirror_cpu.py compares with
// tests/golden/device_mirror_calls.txt.  Only the public surface of Index is used.  argv[1]: a directory for one small file.
//
// Store: 600 x 16 float32 (small integer values: every host distance is exact, so the graph bytes and their checksums do not
// depend on how the compiler vectorises), M = 8, one host thread, std::mt19937(7).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include <flatnav/distances/SquaredL2Distance.h>
#include <flatnav/index/Index.h>

extern "C" void fake_fail_next(const char* name);
extern "C" void fake_note(const char* line);

using L2 = flatnav::distances::SquaredL2Distance<flatnav::util::DataType::float32>;
using TestIndex = flatnav::Index<L2, int>;

static const int N = 600, DIM = 16, M = 8, EF_BUILD = 24, EF = 20, K = 5, N_INIT = 16;
static std::vector<float> g_data, g_queries;

static void note(const std::string& s) { fake_note(s.c_str()); }
static void scenario(const std::string& s) { note("-- scenario " + s); }

struct Fixture {
  std::unique_ptr<TestIndex> index;
  int next_row = 0;
  explicit Fixture(int rows, bool collect_stats = false) : index(new TestIndex(L2::create(DIM), N, M, collect_stats)) {
    index->setNumThreads(1);
    add(rows);
  }
  void add(int rows) {
    for (int i = 0; i < rows; ++i, ++next_row) {
      int label = 1000 + next_row;
      index->add(g_data.data() + static_cast<size_t>(next_row) * DIM, label, EF_BUILD, N_INIT);
    }
    note("> host add: " + std::to_string(rows) + " nodes, " + std::to_string(index->currentNumNodes()) + " in the store");
  }
};

// Runs `call`, logs how it ended.
template <typename F>
static void attempt(const std::string& what, F&& call) {
  note("> " + what);
  try {
    call();
    note("  returned");
  } catch (const std::invalid_argument& e) {
    note(std::string("  threw invalid_argument: ") + e.what());
  } catch (const std::runtime_error& e) {
    note(std::string("  threw runtime_error: ") + e.what());
  }
}

static void search(TestIndex& index, uint64_t nq, int n_init = N_INIT) {
  std::vector<float> dist(nq * K);
  std::vector<int> labels(nq * K);
  std::vector<int32_t> count(nq);
  attempt("searchBatch nq=" + std::to_string(nq),
          [&] { index.searchBatch(g_queries.data(), nq, K, EF, n_init, dist.data(), labels.data(), count.data()); });
}

static std::string listOf(const std::vector<int>& v) {
  std::string s;
  for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string(v[i]);
  return s;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  std::mt19937 rng(7);
  g_data.resize(static_cast<size_t>(N) * DIM);
  g_queries.resize(static_cast<size_t>(320) * DIM);
  for (float& v : g_data) v = static_cast<float>(rng() % 64u);
  for (float& v : g_queries) v = static_cast<float>(rng() % 64u);
  unsetenv("FLATNAV_DEVICES");

  {
    Fixture f(300);
    scenario("1: first search on a part-filled store, then a second search");
    search(*f.index, 8);
    search(*f.index, 8);
    scenario("2: append 10 nodes");
    f.add(10);
    search(*f.index, 8);
    scenario("3: an append that dirties more than a quarter of the rows");
    f.add(150);
    search(*f.index, 8);
    scenario("4: the store filled to capacity after a rebuild");
    f.add(140);
    search(*f.index, 8);
    search(*f.index, 8);
  }
  {
    Fixture f(300);
    scenario("5: a failing write during an increment");
    search(*f.index, 8);
    for (const char* name : {"write_nodes", "write_links", "set_live"}) {
      f.add(5);
      note(std::string("> fail next ") + name);
      fake_fail_next(name);
      search(*f.index, 8);
      search(*f.index, 8);
    }
  }
  {
    scenario("6: buildGraphLinks and doGraphReordering");
    Fixture f(0);
    for (int i = 0; i < N; ++i) {
      int label = i;
      TestIndex::node_id_t id;
      f.index->allocateNode(g_data.data() + static_cast<size_t>(i) * DIM, label, id);
    }
    const std::string mtx = dir + "/ring.mtx";
    {
      std::ofstream out(mtx);
      out << "%%MatrixMarket matrix coordinate pattern general\n" << N << " " << N << " " << M << "\n";
      for (int i = 0; i < N; ++i)
        for (int j = 1; j <= M; ++j) out << i + 1 << " " << (i + j * 7) % N + 1 << "\n";
    }
    search(*f.index, 8);
    attempt("buildGraphLinks", [&] { f.index->buildGraphLinks(mtx); });
    search(*f.index, 8);
    attempt("doGraphReordering gorder, rcm", [&] { f.index->doGraphReordering({"gorder", "rcm"}); });
    search(*f.index, 8);
  }
  {
    Fixture f(300);
    scenario("7: setDevice(1), then setDevices with the list it already has");
    search(*f.index, 8);
    attempt("setDevice 1", [&] { f.index->setDevice(1); });
    search(*f.index, 8);
    attempt("setDevices 1", [&] { f.index->setDevices({1}); });
    search(*f.index, 8);
    note("  device=" + std::to_string(f.index->device()) + " devices=" + listOf(f.index->devices()));

    scenario("8: three devices");
    attempt("setDevices 0,1,2", [&] { f.index->setDevices({0, 1, 2}); });
    search(*f.index, 100);
    search(*f.index, 191);
    search(*f.index, 192);
    search(*f.index, 200);
    f.add(5);
    search(*f.index, 200);
    f.add(5);
    note("> fail next refresh");
    fake_fail_next("refresh");
    search(*f.index, 200);
    attempt("setDevices 0,1,2,1", [&] { f.index->setDevices({0, 1, 2, 1}); });
    note("> fail next replicate");
    fake_fail_next("replicate");
    search(*f.index, 300);
    search(*f.index, 300);
    attempt("setDevices (empty)", [&] { f.index->setDevices({}); });
  }
  {
    scenario("9: FLATNAV_DEVICES=all with replicate failing");
    setenv("FLATNAV_DEVICES", "all", 1);
    Fixture f(300);
    note("> fail next replicate");
    fake_fail_next("replicate");
    search(*f.index, 200);
    search(*f.index, 200);
    note("  device=" + std::to_string(f.index->device()) + " devices=" + listOf(f.index->devices()));
    setenv("FLATNAV_DEVICES", "2,0", 1);
    Fixture g(300);
    note("> FLATNAV_DEVICES=2,0");
    note("  devices=" + listOf(g.index->devices()));
    search(*g.index, 200);
    unsetenv("FLATNAV_DEVICES");
  }
  {
    scenario("10: setFilterRouting");
    Fixture f(300);
    std::vector<uint8_t> bits(N / 8 + 1, 0x55);
    std::vector<float> dist(8 * K);
    std::vector<int> labels(8 * K);
    auto filtered = [&] {
      attempt("searchBatchFiltered nq=8", [&] {
        f.index->searchBatchFiltered(g_queries.data(), 8, K, EF, N_INIT, bits.data(), N, dist.data(), labels.data());
      });
    };
    attempt("setFilterRouting 50, true (no mirror yet)", [&] { f.index->setFilterRouting(50, true); });
    filtered();
    attempt("setDevice 1", [&] { f.index->setDevice(1); });
    filtered();
    attempt("setFilterRouting 20, false (mirror present)", [&] { f.index->setFilterRouting(20, false); });
    attempt("setFilterRouting -1, true", [&] { f.index->setFilterRouting(-1, true); });
    f.add(5);
    filtered();
    attempt("setFilterRouting 0, false", [&] { f.index->setFilterRouting(0, false); });
    attempt("setDevice 0", [&] { f.index->setDevice(0); });
    filtered();
  }
  {
    scenario("11: collect_stats: the five batched forms and the three single-query forms");
    Fixture f(300, true);
    const uint64_t nq = 7;
    std::vector<uint8_t> bits(3 * 80, 0xff);
    std::vector<int32_t> query_filter{0, 1, 2, -1, 0, 1, 2};
    std::vector<float> dist(nq * K);
    std::vector<int> labels(nq * K);
    std::vector<int32_t> count(nq);
    auto counted = [&](const std::string& what, auto&& call) {
      f.index->resetStats();
      attempt(what, call);
      note("  distanceComputations=" + std::to_string(f.index->distanceComputations()));
    };
    TestIndex& ix = *f.index;
    for (int n_init : {N_INIT, 0}) {
      counted("searchBatch n_init=" + std::to_string(n_init),
              [&] { ix.searchBatch(g_queries.data(), nq, K, EF, n_init, dist.data(), labels.data(), count.data()); });
      counted("searchBatchFiltered n_init=" + std::to_string(n_init), [&] {
        ix.searchBatchFiltered(g_queries.data(), nq, K, EF, n_init, bits.data(), N, dist.data(), labels.data(), count.data());
      });
      counted("searchBatchFilteredGrouped n_init=" + std::to_string(n_init), [&] {
        ix.searchBatchFilteredGrouped(g_queries.data(), nq, K, EF, n_init, bits.data(), 3, 80, N, query_filter.data(), dist.data(),
                                      labels.data(), count.data());
      });
    }
    counted("searchBatchExhaustive", [&] {
      ix.searchBatchExhaustive(g_queries.data(), nq, K, bits.data(), N, true, dist.data(), labels.data(), count.data());
    });
    counted("searchBatchExhaustiveGrouped", [&] {
      ix.searchBatchExhaustiveGrouped(g_queries.data(), nq, K, bits.data(), 3, 80, N, query_filter.data(), dist.data(), labels.data());
    });
    auto show = [&](const std::vector<TestIndex::dist_label_t>& r) {
      std::string s = "  results=" + std::to_string(r.size()) + ":";
      for (const auto& p : r) s += " (" + std::to_string(static_cast<int>(p.first)) + "," + std::to_string(p.second) + ")";
      note(s);
    };
    counted("search", [&] { show(ix.search(g_queries.data(), K, EF, N_INIT)); });
    counted("search (default n_init)", [&] { show(ix.search(g_queries.data(), 3, EF)); });
    counted("search n_init=0", [&] { show(ix.search(g_queries.data(), K, EF, 0)); });
    counted("searchFiltered", [&] { show(ix.searchFiltered(g_queries.data(), K, EF, bits.data(), N, N_INIT)); });
    counted("searchExhaustive", [&] { show(ix.searchExhaustive(g_queries.data(), K)); });
    counted("searchExhaustive filtered", [&] { show(ix.searchExhaustive(g_queries.data(), 2, bits.data(), N, true)); });
    note("> fail next search");
    fake_fail_next("search");
    counted("search", [&] { show(ix.search(g_queries.data(), K, EF, N_INIT)); });
  }
  {
    scenario("12: addBatchDevice");
    TestIndex::DeviceBuildOptions opt;
    opt.bootstrap = 100;
    opt.max_batch = 128;
    for (int variant = 0; variant < 3; ++variant) {
      Fixture f(0, true);
      std::vector<int> labels(400);
      for (int i = 0; i < 400; ++i) labels[i] = 5000 + i;
      opt.wire_on_device = variant != 1;
      if (variant == 2) {
        note("> fail next insert_batch");
        fake_fail_next("insert_batch");
      }
      attempt(std::string("addBatchDevice 400 rows, ") + (opt.wire_on_device ? "device wiring" : "host wiring"),
              [&] { f.index->template addBatchDevice<float>(g_data.data(), labels, EF_BUILD, N_INIT, opt); });
      note("  nodes=" + std::to_string(f.index->currentNumNodes()) + " distanceComputations=" +
           std::to_string(f.index->distanceComputations()));
      search(*f.index, 8);
      if (variant == 0) {  // a second batch onto the mirror the first one left
        std::vector<int> more(150, 7);
        attempt("addBatchDevice 150 rows, device wiring",
                [&] { f.index->template addBatchDevice<float>(g_data.data() + 400 * DIM, more, EF_BUILD, N_INIT, opt); });
        search(*f.index, 8);
        attempt("addBatchDevice 150 rows: too many",
                [&] { f.index->template addBatchDevice<float>(g_data.data(), more, EF_BUILD, N_INIT, opt); });
      }
    }
  }
  {
    scenario("13: deviceHandle, syncDevice, destruction");
    Fixture f(300);
    attempt("setDevices 0,1,2", [&] { f.index->setDevices({0, 1, 2}); });
    search(*f.index, 200);
    f.add(5);
    attempt("deviceHandle", [&] { note(f.index->deviceHandle() ? "  handle" : "  no handle"); });
    f.add(5);
    attempt("syncDevice", [&] { f.index->syncDevice(); });
    attempt("syncDevice", [&] { f.index->syncDevice(); });
    note("> destruction");
  }
  std::fflush(stdout);
  return 0;
}
