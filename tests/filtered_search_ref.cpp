// filtered_search_ref.cpp -- CPU restatement of the engine's FILTERED search (include/flatnav_hip.h,
// fnv_search_batch_filtered), written from its documented semantics for the tests (tests/filtered_ref.py loads it with
// ctypes).  Not part of the product.
//
// It reads an index blob in the oracle's AoS layout (node = [data][M uint32 links][int32 label]) and runs, per query:
//   entry, d0 = the sampled scan (nodes 0, step, 2*step, ...; first strict minimum)   -- ignores the filter
//   candidates.push(-d0, entry); visited.add(entry); if allowed(entry): neighbors.push(d0, entry); max_dist = d0
//   while candidates not empty:
//     top = candidates.top(); if -top.d > max_dist and |neighbors| >= B: stop            (B = max(ef, K))
//     candidates.pop(); n_hops++
//     for nb in links(top) in link order, not visited:
//       visited.add(nb); d = dist(q, nb); n_dist++
//       if |neighbors| < B or d < max_dist:
//         candidates.push(-d, nb)                                                       (every node navigates)
//         if allowed(nb): neighbors.push(d, nb); if |neighbors| > B: neighbors.pop(); max_dist = neighbors.top().d
//   drain neighbors by popping, std::sort by distance, truncate to K, node -> label, pad with (+inf, -1)
// allowed(n) = label(n) in [0, n_bits) and bit (label & 7) of byte (label >> 3) of the bitmap is set.
// Heaps are std::priority_queue ordered by distance only, as in the engine.  Distances follow the oracle's definitions:
// float32 = 16 partial sums and a fixed pairwise tree (no FP contraction), integer types = exact int64 sums.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <queue>
#include <utility>
#include <vector>

namespace {

typedef std::pair<float, uint32_t> Item;
struct ByDistance {
  bool operator()(const Item& a, const Item& b) const { return a.first < b.first; }
};
typedef std::priority_queue<Item, std::vector<Item>, ByDistance> Heap;

float sum16(const float* a) {
  float h[8], g[4];
  for (int i = 0; i < 8; i++) h[i] = a[i] + a[i + 8];
  for (int i = 0; i < 4; i++) g[i] = h[i] + h[i + 4];
  return (g[0] + g[2]) + (g[1] + g[3]);
}

float dist_f32(const float* x, const float* y, size_t d, bool ip) {
  float part[16] = {0};
  size_t i = 0;
  for (; i + 16 <= d; i += 16)
    for (int j = 0; j < 16; j++) {
      if (ip) {
        part[j] += x[i + j] * y[i + j];
      } else {
        const float t = x[i + j] - y[i + j];
        part[j] += t * t;
      }
    }
  for (int j = 0; i < d; i++, j++) {
    if (ip) {
      part[j] += x[i] * y[i];
    } else {
      const float t = x[i] - y[i];
      part[j] += t * t;
    }
  }
  return ip ? 1.0f - sum16(part) : sum16(part);
}

template <typename T>
float dist_int(const T* x, const T* y, size_t d, bool ip) {
  int64_t s = 0;
  for (size_t i = 0; i < d; i++) {
    const int a = (int)x[i], b = (int)y[i];
    s += ip ? (int64_t)(a * b) : (int64_t)((a - b) * (a - b));
  }
  return ip ? 1.0f - (float)s : (float)s;
}

// data types as the oracle numbers them: 9 float32, 0 uint8, 4 int8
struct Blob {
  const uint8_t* mem;
  uint64_t node_size, data_size, n;
  uint32_t M, dim;
  int dtype;
  bool ip;
  const uint8_t* data(uint32_t i) const { return mem + (uint64_t)i * node_size; }
  const uint32_t* links(uint32_t i) const { return reinterpret_cast<const uint32_t*>(data(i) + data_size); }
  int32_t label(uint32_t i) const {
    int32_t l;
    std::memcpy(&l, data(i) + data_size + (uint64_t)M * 4, 4);
    return l;
  }
  float dist(const void* q, uint32_t i) const {
    if (dtype == 9) {
      static thread_local float a[9216], b[9216];  // (unaligned-safe copies, off the stack; dim <= 9216 is checked by the caller)
      std::memcpy(a, q, dim * 4);
      std::memcpy(b, data(i), dim * 4);
      return dist_f32(a, b, dim, ip);
    }
    if (dtype == 0) return dist_int((const uint8_t*)q, (const uint8_t*)data(i), dim, ip);
    return dist_int((const int8_t*)q, (const int8_t*)data(i), dim, ip);
  }
};

}  // namespace

extern "C" int fsr_search(const uint8_t* blob, uint64_t node_size, uint64_t data_size, uint32_t M, uint64_t n_nodes, int dtype,
                          int metric, uint32_t dim, const void* queries, uint64_t nq, int K, int ef, int n_init,
                          const uint8_t* bits, uint64_t n_bits, float* out_d, int32_t* out_l, int32_t* out_cnt,
                          uint64_t* out_ndist, uint64_t* out_nhops) {
  if (dtype != 9 && dtype != 0 && dtype != 4) return 1;
  if (dim == 0 || dim > 9216 || n_nodes == 0 || K <= 0 || ef <= 0 || n_init <= 0) return 1;
  const Blob b{blob, node_size, data_size, n_nodes, M, dim, dtype, metric != 0};
  const size_t esize = dtype == 9 ? 4 : 1;
  const size_t B = (size_t)std::max(ef, K);
  std::vector<uint32_t> seen(n_nodes, 0);  // visited: seen[i] == stamp
  uint32_t stamp = 0;
  for (uint64_t qi = 0; qi < nq; qi++) {
    const void* q = (const uint8_t*)queries + qi * dim * esize;
    auto allowed = [&](uint32_t node) {
      const int32_t L = b.label(node);
      return L >= 0 && (uint64_t)L < n_bits && ((bits[(uint32_t)L >> 3] >> (L & 7)) & 1u);
    };
    // entry point: sampled scan
    uint64_t step = n_nodes / (uint64_t)n_init;
    if (step == 0) step = 1;
    float d0 = std::numeric_limits<float>::max();
    uint32_t entry = 0;
    for (uint64_t node = 0; node < n_nodes; node += step) {
      const float d = b.dist(q, (uint32_t)node);
      if (d < d0) {
        d0 = d;
        entry = (uint32_t)node;
      }
    }
    stamp++;
    Heap cand, nbr;
    uint64_t nd = 0, nh = 0;
    float max_dist = d0;
    cand.push(Item(-d0, entry));
    seen[entry] = stamp;
    if (allowed(entry)) nbr.push(Item(d0, entry));
    while (!cand.empty()) {
      const Item top = cand.top();
      if (-top.first > max_dist && nbr.size() >= B) break;
      cand.pop();
      nh++;
      const uint32_t* ln = b.links(top.second);
      for (uint32_t m = 0; m < M; m++) {
        const uint32_t nb = ln[m];
        if (seen[nb] == stamp) continue;
        seen[nb] = stamp;
        const float d = b.dist(q, nb);
        nd++;
        if (nbr.size() < B || d < max_dist) {
          cand.push(Item(-d, nb));
          if (allowed(nb)) {
            nbr.push(Item(d, nb));
            if (nbr.size() > B) nbr.pop();
            max_dist = nbr.top().first;
          }
        }
      }
    }
    std::vector<Item> res;
    while (!nbr.empty()) {
      res.push_back(nbr.top());
      nbr.pop();
    }
    std::sort(res.begin(), res.end(), [](const Item& x, const Item& y) { return x.first < y.first; });
    const int cnt = (int)std::min<size_t>(res.size(), (size_t)K);
    for (int k = 0; k < K; k++) {
      out_d[qi * K + k] = k < cnt ? res[k].first : std::numeric_limits<float>::infinity();
      out_l[qi * K + k] = k < cnt ? b.label(res[k].second) : -1;
    }
    out_cnt[qi] = cnt;
    out_ndist[qi] = nd;
    out_nhops[qi] = nh;
  }
  return 0;
}
