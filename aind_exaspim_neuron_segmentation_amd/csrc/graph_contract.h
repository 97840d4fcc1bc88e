// What premerge.hip and dominant.hip share: the region graph as the kernels see it, the exact 128-bit
// comparison of two means, the bid of an edge for a fragment's best[] word, and the tail of a round once
// every fragment knows its set: the numbering of the sets by their smallest member (label_scan.h's scan
// with SetHead), map[] and sizes' of the other members, and the contraction of the edges into the table
// of edge_table.h. Device code in a header: every file that includes it gets its own copies (anonymous
// namespace), as with label_scan.h and edge_table.h.
#pragma once

#include "edge_table.h"

namespace exaspim {
namespace {

constexpr unsigned kNone = 0xFFFFFFFFu;   // best[f]: no bid yet (an edge index is at most 2^31 - 2)

struct Graph {
    const int* edges;                  // (E, 2)
    const unsigned long long* count;   // int64 in the ABI, >= 1
    const unsigned long long* sum;
    const long long* sizes;            // K + 1
    long long n_edges;
    int n_labels;
};

// a * b in 128 bits
struct Wide {
    unsigned long long hi, lo;
};
__device__ __forceinline__ Wide wide_mul(unsigned long long a, unsigned long long b) {
    return Wide{__umul64hi(a, b), a * b};
}
__device__ __forceinline__ int wide_cmp(const Wide& x, const Wide& y) {
    if (x.hi != y.hi) return x.hi < y.hi ? -1 : 1;
    return x.lo == y.lo ? 0 : x.lo < y.lo ? -1 : 1;
}

// the two ends of edge e, or false if they are no fragments of the graph
__device__ __forceinline__ bool ends_of(const Graph& g, long long e, int* a, int* b) {
    const int lo = g.edges[2 * e], hi = g.edges[2 * e + 1];
    *a = lo;
    *b = hi;
    return lo >= 1 && hi >= 1 && lo <= g.n_labels && hi <= g.n_labels && lo != hi;
}

__device__ __forceinline__ int other_end(const Graph& g, unsigned e, int f) {
    const int lo = g.edges[2 * (size_t)e], hi = g.edges[2 * (size_t)e + 1];
    return lo == f ? hi : lo;
}

// exaspim_agglomerate's test of a contact of count c >= 1 and sum s: merge_all, or s > m * c
__device__ __forceinline__ bool mergeable(unsigned long long c, unsigned long long s, unsigned long long m,
                                          bool merge_all) {
    if (merge_all) return true;
    const Wide bound = wide_mul(m, c);
    return bound.hi == 0 && s > bound.lo;
}

// Edge e (count c, sum s, other end w) bids for best[f]: larger mean first, then the smaller neighbour
// id, then (only a list with repeated pairs gets here) the smaller edge index.
__device__ void bid(const Graph& g, unsigned* best, int f, unsigned e, unsigned long long c,
                    unsigned long long s, int w) {
    unsigned cur = __hip_atomic_load(best + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        if (cur != kNone) {
            const int order = wide_cmp(wide_mul(s, g.count[cur]), wide_mul(g.sum[cur], c));
            const int w2 = other_end(g, cur, f);
            const bool better = order > 0 || (order == 0 && (w < w2 || (w == w2 && e < cur)));
            if (!better) return;
        }
        const unsigned seen = atomicCAS(best + f, cur, e);
        if (seen == cur) return;
        cur = seen;   // somebody else got in: compare with that one
    }
}

// the scan's predicate and sink: the smallest member of every set, in id order, is numbered 1 .. K'
struct SetHead {
    const int* root;
    const int* min_id;
    int* map;
    __device__ __forceinline__ bool operator()(size_t v) const { return v >= 1 && min_id[root[v]] == (int)v; }
    __device__ __forceinline__ void operator()(size_t v, bool flag, int rank) const {
        if (flag) map[v] = rank + 1;
    }
};

// map[] of the members that are not their set's smallest (those entries are only written here, the
// smallest members' only read), and the sizes of the sets
__global__ __launch_bounds__(kThreads) void finish_map(const int* __restrict__ root, const int* __restrict__ min_id,
                                                      const long long* __restrict__ sizes, int* map,
                                                      unsigned long long* sizes_out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < n; f += stride) {
        if (f == 0) {
            map[0] = 0;
            sizes_out[0] = (unsigned long long)sizes[0];
            continue;
        }
        const int head = min_id[root[f]];
        const int j = map[head];
        if (head != (int)f) map[f] = j;
        atomicAdd(sizes_out + j, (unsigned long long)sizes[f]);
    }
}

// One thread per edge: both ends through map[], what is left into the table. skip_empty: a row of
// count 0 is no contact and is left out (the pre-merge takes its rows as they come).
__global__ __launch_bounds__(kThreads) void contract(Graph g, const int* __restrict__ map, Table to,
                                                    bool skip_empty) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < g.n_edges; e += stride) {
        int a, b;
        if (!ends_of(g, e, &a, &b)) continue;
        if (skip_empty && g.count[e] == 0) continue;
        const int la = map[a], lb = map[b];
        if (la == lb) continue;
        global_add(to, edge_key(la, lb), g.count[e], g.sum[e]);
    }
}

}  // namespace
}  // namespace exaspim
