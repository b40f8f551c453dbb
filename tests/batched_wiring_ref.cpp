// batched_wiring_ref.cpp -- CPU model of the batched device builder's wiring rule (fnv_index_insert_batch, the rule stated
// at the head of flatnav_amd/csrc/wire.hpp), written from the rule's words for the tests (tests/batched_wiring_ref.py loads
// it with ctypes).  Not part of the product.
//
// Inputs: the AoS blob of the whole table (node = [data][M uint32 links][int32 label]; live nodes [0, first) wired, the
// batch's records [first, first + count) present), and the batch's beams -- per new node the ef_construction nearest live
// nodes, closest first, as a search with K = ef = ef_construction returns them (node ids).
//
//   select, per new node u = first + i with C beam entries, keep = max(M / 2, 1):
//     C < keep : keep all of them, as the beam's own heap pops them: farthest first, equal distances in the order the heap
//                gives them up.  The beam handed in has been through the search's std::sort (Index.h:402), which for up to 16
//                entries is libstdc++'s insertion sort and leaves equal distances in pop order, so that order is the beam's
//                own; a longer short beam with equal distances is refused (return 2), its pop order cannot be told.
//                (The device search hands its beam to the wiring kernel with equal distances in REVERSE pop order and the
//                kernel reads it backwards; the two agree on the row.)
//     else     : order the beam by (distance ascending, id descending); walk it and keep a candidate c unless some already
//                kept k has d(k, c) < d(u, c); stop at `keep` kept.  The kept nodes are pushed, closest first, into a
//                std::priority_queue keyed on distance only; popping it empty gives the row order.
//     row(u) = those nodes, then self ids.  One request (target = kept node, requester = u) per kept node, in row order.
//   group the requests by target, stably: ascending new node, within a node its row order.
//   connect, per target v: candidates = v's members (entries != v) in slot order, then its requesters in order, taken until
//     cap = max(ef_construction, 4 M) candidates are held.  More than M held: keys d(v, .), order by (key ascending, id
//     descending, position), prune with the same rule to at most M; the kept nodes in pop order become the candidate list.
//     Repeat while requesters remain.  Never pruned: requesters fill the free (self id) slots in slot order, members stay.
//     Pruned: row = the final candidate list, then self ids.
//
// The pruning is written candidate-major (each candidate against the kept so far), as the reference's selectNeighbors is.
// Distances: float32 sums of the element values (the tests use integer-valued data with sums below 2^24, so every distance
// is exact and the summation order cannot matter); integer types through exact int64 sums.  L2 = sum (x - y)^2,
// inner product = 1 - sum x y.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <queue>
#include <utility>
#include <vector>

namespace {

typedef std::pair<float, uint32_t> Item;  // (key, node id)
struct ByDistance {
  bool operator()(const Item& a, const Item& b) const { return a.first < b.first; }
};

enum Counter {
  MAX_REQUESTERS,        // largest number of requesters of one target
  CHUNKED_TARGETS,       // targets whose requesters exceeded cap - members
  PRUNED_THEN_EXTENDED,  // targets pruned, then given more requesters without another prune
  SHARED_FREE_SLOTS,     // never pruned targets that took two or more requesters into free slots
  BLOCK_CROSSING_RUNS,   // targets whose run in the grouped request list crosses a multiple of 64
  WIDE_PRUNES,           // prunes over more than 64 candidates (select and connect)
  EQUAL_KEY_POPS,        // consecutive pops with equal keys among the kept
  SHORT_BEAM_NODES,      // new nodes with C < keep
  TARGETS,               // targets in all
  PRUNED_TARGETS,        // targets pruned at least once
  WIDE_PRUNES_CONNECT,   // the connect step's share of WIDE_PRUNES
  REQUESTS,              // requests in all
  N_COUNTERS
};

struct Model {
  const uint8_t* blob;
  uint64_t node_size, data_size, dim;
  uint32_t M;
  int dtype, ip;
  uint64_t* ctr;
  int64_t dump;  // node whose pruning is printed to stderr, or -1

  const uint8_t* data(uint32_t n) const { return blob + (uint64_t)n * node_size; }

  float dist(uint32_t a, uint32_t b) const {
    const uint8_t *pa = data(a), *pb = data(b);
    if (dtype == 9) {
      const float* x = reinterpret_cast<const float*>(pa);
      const float* y = reinterpret_cast<const float*>(pb);
      float s = 0.f;
      for (uint64_t i = 0; i < dim; i++) {
        if (ip) {
          s += x[i] * y[i];
        } else {
          const float t = x[i] - y[i];
          s += t * t;
        }
      }
      return ip ? 1.0f - s : s;
    }
    int64_t s = 0;
    for (uint64_t i = 0; i < dim; i++) {
      const int x = dtype == 0 ? (int)pa[i] : (int)(int8_t)pa[i];
      const int y = dtype == 0 ? (int)pb[i] : (int)(int8_t)pb[i];
      s += ip ? x * y : (x - y) * (x - y);
    }
    return ip ? 1.0f - (float)s : (float)s;
  }

  // (key ascending, id descending, position): a stable sort keeps the position order of what compares equal
  static void order(std::vector<Item>& c) {
    std::stable_sort(c.begin(), c.end(), [](const Item& a, const Item& b) {
      return a.first < b.first || (a.first == b.first && a.second > b.second);
    });
  }

  // the ordered candidates of `base` (keys = distances to base) -> the kept ones, in the order they are handed out
  std::vector<uint32_t> prune(uint32_t base, const std::vector<Item>& ordered, size_t keep, bool connect) {
    if (ordered.size() > 64) {
      ctr[WIDE_PRUNES]++;
      if (connect) ctr[WIDE_PRUNES_CONNECT]++;
    }
    std::vector<Item> saved;
    for (const Item& c : ordered) {
      if (saved.size() >= keep) break;
      bool keep_it = true;
      for (const Item& k : saved)
        if (dist(k.second, c.second) < c.first) {
          keep_it = false;
          break;
        }
      if (keep_it) saved.push_back(c);
    }
    std::priority_queue<Item, std::vector<Item>, ByDistance> heap;
    for (const Item& k : saved) heap.push(k);
    std::vector<uint32_t> out;
    float last = 0.f;
    while (!heap.empty()) {
      if (!out.empty() && heap.top().first == last) ctr[EQUAL_KEY_POPS]++;
      last = heap.top().first;
      out.push_back(heap.top().second);
      heap.pop();
    }
    if (dump == (int64_t)base) {
      fprintf(stderr, "node %u %s prune, %zu candidates (key id):", base, connect ? "connect" : "select", ordered.size());
      for (const Item& c : ordered) fprintf(stderr, " (%g %u)", c.first, c.second);
      fprintf(stderr, "\n  kept, in pop order:");
      for (uint32_t k : out) fprintf(stderr, " %u", k);
      fprintf(stderr, "\n");
    }
    return out;
  }
};

}  // namespace

extern "C" {

int bwr_n_counters() { return N_COUNTERS; }

// links_out [first + count][M]; counters [bwr_n_counters()].  Returns 0, 1 for arguments it cannot take, 2 for a short beam whose pop order is unknown.
int bwr_insert_batch(const uint8_t* blob, uint64_t node_size, uint64_t data_size, uint32_t M, int dtype, int metric, uint64_t dim,
                     uint64_t first, uint64_t count, int ef_construction, const float* beam_dist, const int32_t* beam_ids,
                     const int32_t* beam_count, uint32_t* links_out, uint64_t* counters, int64_t dump_node) {
  const uint64_t esize = dtype == 9 ? 4 : 1;
  if (!blob || !links_out || !counters || M == 0 || ef_construction <= 0 || first == 0 || (dtype != 9 && dtype != 0 && dtype != 4) ||
      data_size < dim * esize || node_size < data_size + 4ull * M + 4 || (metric != 0 && metric != 1))
    return 1;
  std::fill(counters, counters + N_COUNTERS, 0ull);
  Model m{blob, node_size, data_size, dim, M, dtype, metric == 1, counters, dump_node};
  const uint64_t total = first + count;
  const size_t W = (size_t)ef_construction;
  const size_t keep = std::max<size_t>(M / 2, 1);
  const size_t cap = std::max<size_t>(W, 4 * (size_t)M);
  for (uint64_t n = 0; n < total; n++) std::memcpy(links_out + n * M, blob + n * node_size + data_size, 4ull * M);

  // ---- select ------------------------------------------------------------------------------------------------------
  std::vector<std::pair<uint32_t, uint32_t>> requests;  // (target, requester), in emission order
  for (uint64_t i = 0; i < count; i++) {
    const uint32_t u = (uint32_t)(first + i);
    const int c_raw = beam_count[i];
    if (c_raw < 0 || (size_t)c_raw > W) return 1;
    const size_t C = (size_t)c_raw;
    std::vector<uint32_t> row;
    if (C < keep) {
      m.ctr[SHORT_BEAM_NODES]++;
      std::vector<Item> all;
      for (size_t j = 0; j < C; j++) all.push_back(Item(beam_dist[i * W + j], (uint32_t)beam_ids[i * W + j]));
      for (size_t j = 1; j < C; j++) {
        if (all[j].first < all[j - 1].first) return 1;  // not closest first
        if (all[j].first == all[j - 1].first && C > 16) return 2;
      }
      std::stable_sort(all.begin(), all.end(), [](const Item& a, const Item& b) { return a.first > b.first; });
      for (const Item& a : all) row.push_back(a.second);
    } else {
      std::vector<Item> cand;
      for (size_t j = 0; j < C; j++) cand.push_back(Item(beam_dist[i * W + j], (uint32_t)beam_ids[i * W + j]));
      Model::order(cand);
      row = m.prune(u, cand, keep, false);
    }
    for (size_t j = 0; j < M; j++) links_out[(uint64_t)u * M + j] = j < row.size() ? row[j] : u;
    for (uint32_t v : row) {
      if (v >= first) return 1;  // a beam holds live nodes only
      requests.push_back(std::make_pair(v, u));
    }
  }
  // ---- group by target, stably ---------------------------------------------------------------------------------------
  std::stable_sort(requests.begin(), requests.end(),
                   [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first < b.first; });
  m.ctr[REQUESTS] = requests.size();
  // ---- connect -------------------------------------------------------------------------------------------------------
  for (size_t start = 0; start < requests.size();) {
    const uint32_t v = requests[start].first;
    size_t end = start;
    while (end < requests.size() && requests[end].first == v) end++;
    const size_t R = end - start;
    uint32_t* row = links_out + (uint64_t)v * M;
    std::vector<uint32_t> cand;
    for (size_t j = 0; j < M; j++)
      if (row[j] != v) cand.push_back(row[j]);
    const size_t members = cand.size();
    m.ctr[TARGETS]++;
    m.ctr[MAX_REQUESTERS] = std::max<uint64_t>(m.ctr[MAX_REQUESTERS], R);
    if (R > cap - members) m.ctr[CHUNKED_TARGETS]++;
    if (start / 64 != (end - 1) / 64) m.ctr[BLOCK_CROSSING_RUNS]++;
    bool pruned = false, extended = false;
    size_t r = start;
    do {
      const size_t before = cand.size();
      while (r < end && cand.size() < cap) cand.push_back(requests[r++].second);
      if (cand.size() > M) {
        std::vector<Item> keyed;
        for (uint32_t c : cand) keyed.push_back(Item(m.dist(v, c), c));
        Model::order(keyed);
        cand = m.prune(v, keyed, M, true);
        pruned = true;
      } else if (pruned && cand.size() > before) {
        extended = true;
      }
    } while (r < end);
    if (pruned) {
      m.ctr[PRUNED_TARGETS]++;
      if (extended) m.ctr[PRUNED_THEN_EXTENDED]++;
      for (size_t j = 0; j < M; j++) row[j] = j < cand.size() ? cand[j] : v;
    } else {
      if (R >= 2) m.ctr[SHARED_FREE_SLOTS]++;
      size_t next = members;  // cand = members, then the requesters
      for (size_t j = 0; j < M && next < cand.size(); j++)
        if (row[j] == v) row[j] = cand[next++];
    }
    start = end;
  }
  return 0;
}

}  // extern "C"
