// One round of the dominant-edge contraction of a region graph on the device
// (exaspim_region_graph_contract_dominant; the definition and the theorem are in
// include/exaspim_affinity.h, the proof in DESIGN 6j): a mergeable edge whose mean is strictly larger than
// that of every other mergeable edge at both of its ends is the edge exaspim_agglomerate merges before any
// other at those two fragments, so it is contracted here and the host starts from fewer fragments with
// the same result.
//
// Passes, each a launch of its own on the caller's stream (no lock, no grid-wide barrier, no workgroup
// that waits for another one; the number of launches is a constant):
//   memsets      best := none, tied := 0, the table's keys := empty, its counts and sums := 0, sizes' := 0,
//                state := 0;
//   choose       one thread per edge: a mergeable edge bids for the best[] word of both its ends
//                (graph_contract.h's compare-and-swap loop: the winner is the maximum of a total order);
//   mark_ties    one thread per edge: a mergeable edge that lost at an end but whose mean equals the
//                winner's sets tied[] of that end. Every writer stores the same value, so the order of
//                arrival does not matter; only an edge that ties the maximum can make it less than strict;
//   resolve      one thread per fragment: f and p are a pair iff the same edge is the best of both and
//                neither is tied; parent[] of both is the smaller id, of everybody else itself;
//   scan_*       label_scan.h's three passes with "f is its set's smallest member": K' and map[] of those;
//   finish_map   map[] of every pair's larger member, sizes'[map[f]] += sizes[f] by 64-bit atomicAdd;
//   contract     one thread per edge: both ends through map[], what is left into the table of
//                edge_table.h;
//   scan_*       the occupied slots become the edge list, E'.
// A set has at most two members, so nothing follows pointers: parent[parent[f]] == parent[f], and parent[]
// serves as the root and as the smallest member of SetHead and finish_map at once. An edge with an end
// outside 1 .. K, with equal ends or with count 0 is skipped by every pass, so nothing read from device
// memory becomes an address unchecked: best[] holds only edges that passed the check, parent[] only
// their ends.
#include "graph_contract.h"

namespace exaspim {
namespace {

// the ends, count and sum of row e if it is a mergeable contact between two fragments of the graph
__device__ __forceinline__ bool mergeable_row(const Graph& g, long long e, unsigned long long m, bool merge_all,
                                              int* a, int* b, unsigned long long* c, unsigned long long* s) {
    if (!ends_of(g, e, a, b)) return false;
    *c = g.count[e];
    *s = g.sum[e];
    return *c != 0 && mergeable(*c, *s, m, merge_all);   // count 0: no contact at all, it has no mean
}

__global__ __launch_bounds__(kThreads) void dominant_choose(Graph g, unsigned long long m, bool merge_all,
                                                           unsigned* best) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < g.n_edges; e += stride) {
        int a, b;
        unsigned long long c, s;
        if (!mergeable_row(g, e, m, merge_all, &a, &b, &c, &s)) continue;
        bid(g, best, a, (unsigned)e, c, s, b);
        bid(g, best, b, (unsigned)e, c, s, a);
    }
}

// best[] is complete and only read: every mergeable edge at f bid for best[f], so it is not "none" here
__global__ __launch_bounds__(kThreads) void dominant_mark_ties(Graph g, unsigned long long m, bool merge_all,
                                                              const unsigned* __restrict__ best, int* tied) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < g.n_edges; e += stride) {
        int a, b;
        unsigned long long c, s;
        if (!mergeable_row(g, e, m, merge_all, &a, &b, &c, &s)) continue;
        const int ends[2] = {a, b};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const unsigned w = best[ends[i]];
            if (w == (unsigned)e || w == kNone) continue;
            if (wide_cmp(wide_mul(s, g.count[w]), wide_mul(g.sum[w], c)) == 0) tied[ends[i]] = 1;
        }
    }
}

// parent[f] = the smaller id of f's pair, or f
__global__ __launch_bounds__(kThreads) void dominant_resolve(Graph g, const unsigned* __restrict__ best,
                                                            const int* __restrict__ tied,
                                                            int* __restrict__ parent) {
    const size_t n = (size_t)g.n_labels + 1, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < n; f += stride) {
        int head = (int)f;
        const unsigned e = f ? best[f] : kNone;
        if (e != kNone && !tied[f]) {
            const int p = other_end(g, e, (int)f);
            if (best[p] == e && !tied[p] && p < head) head = p;
        }
        parent[f] = head;
    }
}

struct DominantLayout {
    Layout table;
    size_t best_off, tied_off, parent_off, blocks_off, bytes;
    long long n_scan_blocks;   // of the scan over the K + 1 fragments
};

DominantLayout dominant_layout(int32_t n_labels, int64_t capacity) {
    DominantLayout l;
    l.table = layout_of(capacity);
    const size_t per_label = align_up(((size_t)n_labels + 1) * 4, 256);
    l.n_scan_blocks = ((long long)n_labels + 1 + kScanBlock - 1) / kScanBlock;
    l.best_off = l.table.bytes;
    l.tied_off = l.best_off + per_label;
    l.parent_off = l.tied_off + per_label;
    l.blocks_off = l.parent_off + per_label;
    l.bytes = l.blocks_off + align_up((size_t)l.n_scan_blocks * 4, 256);
    return l;
}

}  // namespace
}  // namespace exaspim

using namespace exaspim;

extern "C" size_t exaspim_region_graph_contract_dominant_workspace_bytes(int32_t n_labels, int64_t edge_capacity) {
    if (n_labels < 0) {
        set_error("region_graph_contract_dominant_workspace_bytes: n_labels must not be negative, got %d", n_labels);
        return 0;
    }
    if (!valid_capacity(edge_capacity)) {
        set_error("region_graph_contract_dominant_workspace_bytes: edge_capacity must be a power of two in "
                  "1 .. 2^30, got %lld", (long long)edge_capacity);
        return 0;
    }
    return dominant_layout(n_labels, edge_capacity).bytes;
}

extern "C" int exaspim_region_graph_contract_dominant(const int32_t* edges_dev, const int64_t* count_dev,
                                                      const uint64_t* sum_dev, const int64_t* sizes_dev,
                                                      int64_t n_edges, int32_t n_labels, float threshold,
                                                      int64_t edge_capacity, int32_t* edges_out_dev,
                                                      int64_t* count_out_dev, uint64_t* sum_out_dev,
                                                      int64_t* sizes_out_dev, int32_t* map_dev, int32_t* state_dev,
                                                      void* workspace_dev, size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(sizes_dev && edges_out_dev && count_out_dev && sum_out_dev && sizes_out_dev && map_dev &&
                      state_dev && workspace_dev,
                  "region_graph_contract_dominant: NULL argument");
    EXA_CHECK_ARG(n_labels >= 0 && n_edges >= 0 && n_edges <= 2147483647ll,
                  "region_graph_contract_dominant: negative n_labels or n_edges outside 0 .. 2^31 - 1");
    EXA_CHECK_ARG(n_edges == 0 || (edges_dev && count_dev && sum_dev),
                  "region_graph_contract_dominant: NULL edge list");
    EXA_CHECK_ARG(threshold == threshold, "region_graph_contract_dominant: the threshold is NaN");
    EXA_CHECK_ARG(valid_capacity(edge_capacity),
                  "region_graph_contract_dominant: edge_capacity must be a power of two in 1 .. 2^30, got %lld",
                  (long long)edge_capacity);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 &&
                      (((uintptr_t)edges_dev | (uintptr_t)edges_out_dev | (uintptr_t)map_dev |
                        (uintptr_t)state_dev) & 3) == 0 &&
                      (((uintptr_t)count_dev | (uintptr_t)sum_dev | (uintptr_t)sizes_dev | (uintptr_t)count_out_dev |
                        (uintptr_t)sum_out_dev | (uintptr_t)sizes_out_dev) & 7) == 0,
                  "region_graph_contract_dominant: misaligned buffer");
    const DominantLayout l = dominant_layout(n_labels, edge_capacity);
    if (workspace_bytes < l.bytes) {
        set_error("region_graph_contract_dominant: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace_dev);
    // state_dev = (K', E', overflow): the table's two state words are the last two
    const Table to{reinterpret_cast<unsigned long long*>(ws + l.table.keys_off),
                   reinterpret_cast<unsigned long long*>(ws + l.table.counts_off),
                   reinterpret_cast<unsigned long long*>(ws + l.table.sums_off), (unsigned)(edge_capacity - 1),
                   state_dev + 1};
    int* table_blocks = reinterpret_cast<int*>(ws + l.table.blocks_off);
    unsigned* best = reinterpret_cast<unsigned*>(ws + l.best_off);
    int* tied = reinterpret_cast<int*>(ws + l.tied_off);
    int* parent = reinterpret_cast<int*>(ws + l.parent_off);
    int* label_blocks = reinterpret_cast<int*>(ws + l.blocks_off);
    unsigned long long* sizes_out = reinterpret_cast<unsigned long long*>(sizes_out_dev);
    const Graph g{edges_dev, reinterpret_cast<const unsigned long long*>(count_dev),
                  reinterpret_cast<const unsigned long long*>(sum_dev), reinterpret_cast<const long long*>(sizes_dev),
                  (long long)n_edges, n_labels};
    const MergeBound bound = merge_bound(threshold);
    const size_t n = (size_t)n_labels + 1;

    EXA_CHECK_HIP(hipMemsetAsync(best, 0xFF, n * 4, s));
    EXA_CHECK_HIP(hipMemsetAsync(tied, 0, n * 4, s));
    EXA_CHECK_HIP(hipMemsetAsync(to.keys, 0xFF, (size_t)edge_capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(to.counts, 0, (size_t)edge_capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(to.sums, 0, (size_t)edge_capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(sizes_out, 0, n * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(state_dev, 0, 3 * sizeof(int32_t), s));
    const unsigned edge_grid = capped_grid((size_t)n_edges, kThreads), label_grid = capped_grid(n, kThreads);
    dominant_choose<<<edge_grid, kThreads, 0, s>>>(g, bound.m, bound.merge_all, best);
    dominant_mark_ties<<<edge_grid, kThreads, 0, s>>>(g, bound.m, bound.merge_all, best, tied);
    dominant_resolve<<<label_grid, kThreads, 0, s>>>(g, best, tied, parent);
    // a set's root and its smallest member are the same fragment, and parent[] of that one is itself
    const SetHead head{parent, parent, map_dev};
    const unsigned label_scan_grid = (unsigned)l.n_scan_blocks;
    scan_count<<<label_scan_grid, kThreads, 0, s>>>(head, label_blocks, n);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(label_blocks, l.n_scan_blocks, state_dev);
    scan_assign<<<label_scan_grid, kThreads, 0, s>>>(head, label_blocks, n);
    finish_map<<<label_grid, kThreads, 0, s>>>(parent, parent, g.sizes, map_dev, sizes_out, n);
    contract<<<edge_grid, kThreads, 0, s>>>(g, map_dev, to, true);
    const UsedSlot used{to.keys, to.counts, to.sums, edges_out_dev, reinterpret_cast<long long*>(count_out_dev),
                        reinterpret_cast<unsigned long long*>(sum_out_dev)};
    const unsigned table_scan_grid = (unsigned)l.table.n_scan_blocks;
    scan_count<<<table_scan_grid, kThreads, 0, s>>>(used, table_blocks, (size_t)edge_capacity);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(table_blocks, l.table.n_scan_blocks, state_dev + 1 + kEdges);
    scan_assign<<<table_scan_grid, kThreads, 0, s>>>(used, table_blocks, (size_t)edge_capacity);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}
