// Mean-affinity agglomeration of a region graph on the host (exaspim_agglomerate; semantics in
// include/exaspim_affinity.h). No device code: the graph has K fragments, not voxels.
//
// A heap of edges ordered by the rule's total order (larger mean first, by cross-multiplication in 128-bit
// integers; then the smaller lo, then the smaller hi of the current root ids), with lazy invalidation:
// an entry counts only while its edge is alive and carries the edge's current version, and every live
// edge has one such entry with the current root ids of its ends.
//
// A set of fragments is held by a HANDLE (the id of one of its fragments), its root id (the smallest id,
// which the rule and the numbering speak of) is name[handle]. An edge is a record between two handles;
// there is at most one per pair, found through one hash map keyed by the pair. Each handle lists its
// edges (the list may also hold edges that have died or moved on; they are skipped). A merge keeps the
// handle with the longer list and walks the shorter one: an edge to a neighbour the kept handle has an
// edge to as well is pooled into that one, any other is moved over. So an edge is walked O(log) times
// however large a hub grows. An edge gets a new entry when its mean changes (pooling) or the root id of
// one of its ends does. When the kept handle's root id changes (it absorbed a smaller id), that is all
// its edges: the one step proportional to the larger list, taken only when a set meets a new smallest id.
#include <algorithm>
#include <queue>
#include <unordered_map>
#include <vector>

#include "common.h"

namespace exaspim {
namespace {

typedef unsigned __int128 u128;

struct Edge {
    int32_t a, b;        // handles
    uint64_t count, sum;
    uint32_t version;
    bool alive;
};

struct Entry {
    uint64_t count, sum;
    int32_t lo, hi;
    int32_t edge;
    uint32_t version;
};

// "x comes after y": std::priority_queue pops the entry no other one comes before
struct After {
    bool operator()(const Entry& x, const Entry& y) const {
        const u128 l = (u128)x.sum * y.count, r = (u128)y.sum * x.count;
        if (l != r) return l < r;
        if (x.lo != y.lo) return x.lo > y.lo;
        return x.hi > y.hi;
    }
};

}  // namespace
}  // namespace exaspim

using namespace exaspim;

extern "C" int exaspim_agglomerate(const int32_t* edges, const int64_t* counts, const uint64_t* sums,
                                   int64_t n_edges, const int64_t* sizes, int32_t n_labels, float threshold,
                                   int64_t min_size, int32_t* table, int32_t* n_segments) {
    EXA_CHECK_ARG(sizes && table && n_segments && n_labels >= 0 && n_edges >= 0 && n_edges <= 2147483647ll,
                  "agglomerate: NULL argument, negative n_labels or n_edges outside 0 .. 2^31 - 1");
    EXA_CHECK_ARG(n_edges == 0 || (edges && counts && sums), "agglomerate: NULL edge list");
    EXA_CHECK_ARG(threshold == threshold, "agglomerate: the threshold is NaN");
    const int32_t K = n_labels;
    // Pooled counts and sums are sums of the input's: with all counts together within 2^39 every pooled
    // count stays within 2^39 and every pooled sum within 2^63, so neither wraps its uint64_t and each
    // product below stays within 2^102.
    const uint64_t kMaxTotal = 1ull << 39;
    u128 total_count = 0;   // up to 2^31 edges of up to 2^34 each: 2^65
    for (int64_t e = 0; e < n_edges; ++e) {
        const int32_t lo = edges[2 * e], hi = edges[2 * e + 1];
        EXA_CHECK_ARG(lo >= 1 && lo < hi && hi <= K, "agglomerate: edge %lld is (%d, %d), needs 1 <= lo < hi <= %d",
                      (long long)e, lo, hi, K);
        EXA_CHECK_ARG(e == 0 || edges[2 * e - 2] < lo || (edges[2 * e - 2] == lo && edges[2 * e - 1] < hi),
                      "agglomerate: the edge list is not sorted by (lo, hi) without repeats at edge %lld", (long long)e);
        EXA_CHECK_ARG(counts[e] >= 1 && counts[e] <= (1ll << 34) && sums[e] <= ((uint64_t)counts[e] << 24),
                      "agglomerate: edge %lld has count %lld and sum %llu, needs 1 <= count <= 2^34 and sum <= count * 2^24",
                      (long long)e, (long long)counts[e], (unsigned long long)sums[e]);
        total_count += (uint64_t)counts[e];
    }
    if (total_count > kMaxTotal) {
        char digits[24];   // below 2^65: at most 20 digits, in two halves
        const u128 half = 10000000000ull;
        if (total_count >= half)
            snprintf(digits, sizeof digits, "%llu%010llu", (unsigned long long)(total_count / half),
                     (unsigned long long)(total_count % half));
        else
            snprintf(digits, sizeof digits, "%llu", (unsigned long long)total_count);
        set_error("agglomerate: the counts add up to %s, needs a total of at most 2^39 = %llu (parallel edges are "
                  "pooled in 64 bits)", digits, (unsigned long long)kMaxTotal);
        return EXASPIM_E_INVALID;
    }
    for (int32_t l = 0; l <= K; ++l)
        EXA_CHECK_ARG(sizes[l] >= 0, "agglomerate: sizes[%d] is negative", l);

    // merge iff merge_all or sum > m * count (common.h)
    const MergeBound bound = merge_bound(threshold);
    const bool merge_all = bound.merge_all;
    const uint64_t m = bound.m;

    std::vector<Edge> edge((size_t)n_edges);
    std::vector<std::vector<int32_t>> adj((size_t)K + 1);
    std::vector<int32_t> parent((size_t)K + 1), name((size_t)K + 1);
    for (int32_t l = 0; l <= K; ++l) parent[l] = name[l] = l;
    auto pair_key = [](int32_t x, int32_t y) {
        return x < y ? (uint64_t)(uint32_t)x << 32 | (uint32_t)y : (uint64_t)(uint32_t)y << 32 | (uint32_t)x;
    };
    std::unordered_map<uint64_t, int32_t> between;   // pair of handles -> their edge
    between.reserve((size_t)n_edges);
    std::priority_queue<Entry, std::vector<Entry>, After> heap;
    {
        std::vector<Entry> first((size_t)n_edges);
        for (int64_t e = 0; e < n_edges; ++e) {
            edge[e] = Edge{edges[2 * e], edges[2 * e + 1], (uint64_t)counts[e], sums[e], 0, true};
            adj[edge[e].a].push_back((int32_t)e);
            adj[edge[e].b].push_back((int32_t)e);
            between.emplace(pair_key(edge[e].a, edge[e].b), (int32_t)e);
            first[e] = Entry{edge[e].count, edge[e].sum, edge[e].a, edge[e].b, (int32_t)e, 0};
        }
        heap = std::priority_queue<Entry, std::vector<Entry>, After>(After(), std::move(first));
    }
    // a new version of the edge and the entry that goes with it
    auto renew = [&](int32_t e) {
        Edge& x = edge[e];
        x.version++;
        const int32_t na = name[x.a], nb = name[x.b];
        heap.push(Entry{x.count, x.sum, std::min(na, nb), std::max(na, nb), e, x.version});
    };

    while (!heap.empty()) {
        const Entry top = heap.top();
        heap.pop();
        if (!edge[top.edge].alive || edge[top.edge].version != top.version) continue;
        if (!merge_all && !((u128)top.sum > (u128)m * top.count)) break;   // the best one stays: so do all
        int32_t big = edge[top.edge].a, small = edge[top.edge].b;
        if (adj[big].size() < adj[small].size()) std::swap(big, small);
        edge[top.edge].alive = false;
        between.erase(pair_key(big, small));
        parent[top.hi] = top.lo;   // root ids: the larger goes under the smaller
        if (name[big] != top.lo) {
            name[big] = top.lo;
            std::vector<int32_t>& list = adj[big];
            size_t kept = 0;
            for (size_t i = 0; i < list.size(); ++i) {
                const int32_t e = list[i];
                if (!edge[e].alive || (edge[e].a != big && edge[e].b != big)) continue;
                list[kept++] = e;
                renew(e);
            }
            list.resize(kept);
        }
        // a moved edge whose end keeps its root id keeps its entry: mean and ids are what they were
        const bool small_renamed = name[small] != top.lo;
        for (const int32_t e : adj[small]) {
            Edge& x = edge[e];
            if (!x.alive || (x.a != small && x.b != small)) continue;
            const int32_t w = x.a == small ? x.b : x.a;
            between.erase(pair_key(small, w));
            const auto common = between.find(pair_key(big, w));
            if (common != between.end()) {   // parallel edges to a common neighbour add up
                edge[common->second].count += x.count;
                edge[common->second].sum += x.sum;
                x.alive = false;
                renew(common->second);
            } else {                         // the edge is the kept handle's now; w's list holds it already
                (x.a == small ? x.a : x.b) = big;
                between.emplace(pair_key(big, w), e);
                adj[big].push_back(e);
                if (small_renamed) renew(e);
            }
        }
        std::vector<int32_t>().swap(adj[small]);
    }

    // parent[l] < l for every merged l, so one ascending pass gives root(l) = the set's smallest id
    std::vector<int64_t> total((size_t)K + 1, 0);
    for (int32_t l = 1; l <= K; ++l) {
        if (parent[l] != l) parent[l] = parent[parent[l]];
        total[parent[l]] += sizes[l];
    }
    int32_t next = 0;
    table[0] = 0;
    for (int32_t l = 1; l <= K; ++l) {
        if (parent[l] == l)
            table[l] = total[l] > min_size ? ++next : 0;
        else
            table[l] = table[parent[l]];
    }
    *n_segments = next;
    return EXASPIM_OK;
}
