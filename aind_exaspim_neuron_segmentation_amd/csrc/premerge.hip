// One round of the size-floor pre-merge of a region graph on the device (exaspim_region_graph_premerge;
// the definition is in include/exaspim_affinity.h, the reasoning in DESIGN 6h): every fragment smaller
// than the floor joins the neighbour across its best mergeable contact, chains collapse at once, and the
// graph is contracted, so that the host agglomeration starts from far fewer fragments.
//
// Passes, each a launch of its own on the caller's stream (no lock, no grid-wide barrier, no workgroup
// that waits for another one; the number of launches depends on n_labels alone, never on device data):
//   memsets      best := none, the table's keys := empty, its counts and sums := 0, sizes' := 0, state := 0;
//   choose       one thread per edge: a mergeable edge bids for the best[] word of each tiny end in a
//                32-bit atomicCAS loop (graph_contract.h, shared with dominant.hip like the round's tail
//                from the numbering on). The order of bids is total, so the winner is the maximum
//                whatever order they arrive in;
//   resolve      one thread per fragment: the other end of best[f], or f itself; of a mutual pair the
//                smaller id keeps itself. Written to a second array, best[] is only read;
//   double       parent'[f] = parent[parent[f]] between two buffers, ceil(log2 K) + 1 times: a chain of
//                K fragments (a tube of basins with rising means) ends at its root after that many;
//   set_min      atomicMin of the member ids at each root;
//   scan_*       label_scan.h's three passes with "f is its set's smallest member": K' and map[] of those;
//   finish_map   map[] of every other member, sizes'[map[f]] += sizes[f] by 64-bit atomicAdd;
//   contract     one thread per edge: both ends through map[], what is left into the table of
//                edge_table.h (region_graph.hip's claim-and-add);
//   scan_*       the occupied slots become the edge list, E'.
// An edge with an end outside 1 .. K or with equal ends is skipped by choose and by contract, so nothing
// read from device memory becomes an address unchecked: best[] holds only edges that passed the check,
// parent[] only their ends.
#include "graph_contract.h"

namespace exaspim {
namespace {

__global__ __launch_bounds__(kThreads) void choose(Graph g, unsigned long long m, bool merge_all, long long floor,
                                                  unsigned* best) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < g.n_edges; e += stride) {
        int a, b;
        if (!ends_of(g, e, &a, &b)) continue;
        const unsigned long long c = g.count[e], s = g.sum[e];
        if (c == 0) continue;   // no contact at all: it has no mean
        if (!mergeable(c, s, m, merge_all)) continue;
        if (g.sizes[a] < floor) bid(g, best, a, (unsigned)e, c, s, b);
        if (g.sizes[b] < floor) bid(g, best, b, (unsigned)e, c, s, a);
    }
}

// parent[f] = f's choice after rule 4, min_id[f] = f
__global__ __launch_bounds__(kThreads) void resolve(Graph g, const unsigned* __restrict__ best,
                                                   int* __restrict__ parent, int* __restrict__ min_id) {
    const size_t n = (size_t)g.n_labels + 1, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < n; f += stride) {
        int p = (int)f;
        const unsigned e = f ? best[f] : kNone;
        if (e != kNone) {
            p = other_end(g, e, (int)f);
            const unsigned back = best[p];
            // a mutual pair: the smaller id drops its choice and becomes the root
            if (back != kNone && other_end(g, back, p) == (int)f && (int)f < p) p = (int)f;
        }
        parent[f] = p;
        min_id[f] = (int)f;
    }
}

__global__ __launch_bounds__(kThreads) void double_parents(const int* __restrict__ from, int* __restrict__ to,
                                                          size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < n; f += stride) to[f] = from[from[f]];
}

__global__ __launch_bounds__(kThreads) void set_min(const int* __restrict__ root, int* min_id, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < n; f += stride) {
        const int r = root[f];
        if (r != (int)f) atomicMin(min_id + r, (int)f);
    }
}

struct PremergeLayout {
    Layout table;
    size_t best_off, parent_a_off, parent_b_off, min_off, blocks_off, bytes;
    long long n_scan_blocks;   // of the scan over the K + 1 fragments
};

PremergeLayout premerge_layout(int32_t n_labels, int64_t capacity) {
    PremergeLayout l;
    l.table = layout_of(capacity);
    const size_t per_label = align_up(((size_t)n_labels + 1) * 4, 256);
    l.n_scan_blocks = ((long long)n_labels + 1 + kScanBlock - 1) / kScanBlock;
    l.best_off = l.table.bytes;
    l.parent_a_off = l.best_off + per_label;
    l.parent_b_off = l.parent_a_off + per_label;
    l.min_off = l.parent_b_off + per_label;
    l.blocks_off = l.min_off + per_label;
    l.bytes = l.blocks_off + align_up((size_t)l.n_scan_blocks * 4, 256);
    return l;
}

}  // namespace
}  // namespace exaspim

using namespace exaspim;

extern "C" size_t exaspim_region_graph_premerge_workspace_bytes(int32_t n_labels, int64_t edge_capacity) {
    if (n_labels < 0) {
        set_error("region_graph_premerge_workspace_bytes: n_labels must not be negative, got %d", n_labels);
        return 0;
    }
    if (!valid_capacity(edge_capacity)) {
        set_error("region_graph_premerge_workspace_bytes: edge_capacity must be a power of two in 1 .. 2^30, "
                  "got %lld", (long long)edge_capacity);
        return 0;
    }
    return premerge_layout(n_labels, edge_capacity).bytes;
}

extern "C" int exaspim_region_graph_premerge(const int32_t* edges_dev, const int64_t* count_dev,
                                             const uint64_t* sum_dev, const int64_t* sizes_dev, int64_t n_edges,
                                             int32_t n_labels, float threshold, int64_t size_floor,
                                             int64_t edge_capacity, int32_t* edges_out_dev, int64_t* count_out_dev,
                                             uint64_t* sum_out_dev, int64_t* sizes_out_dev, int32_t* map_dev,
                                             int32_t* state_dev, void* workspace_dev, size_t workspace_bytes,
                                             void* stream) {
    EXA_CHECK_ARG(sizes_dev && edges_out_dev && count_out_dev && sum_out_dev && sizes_out_dev && map_dev &&
                      state_dev && workspace_dev,
                  "region_graph_premerge: NULL argument");
    EXA_CHECK_ARG(n_labels >= 0 && n_edges >= 0 && n_edges <= 2147483647ll,
                  "region_graph_premerge: negative n_labels or n_edges outside 0 .. 2^31 - 1");
    EXA_CHECK_ARG(n_edges == 0 || (edges_dev && count_dev && sum_dev), "region_graph_premerge: NULL edge list");
    EXA_CHECK_ARG(threshold == threshold, "region_graph_premerge: the threshold is NaN");
    EXA_CHECK_ARG(valid_capacity(edge_capacity),
                  "region_graph_premerge: edge_capacity must be a power of two in 1 .. 2^30, got %lld",
                  (long long)edge_capacity);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 &&
                      (((uintptr_t)edges_dev | (uintptr_t)edges_out_dev | (uintptr_t)map_dev |
                        (uintptr_t)state_dev) & 3) == 0 &&
                      (((uintptr_t)count_dev | (uintptr_t)sum_dev | (uintptr_t)sizes_dev | (uintptr_t)count_out_dev |
                        (uintptr_t)sum_out_dev | (uintptr_t)sizes_out_dev) & 7) == 0,
                  "region_graph_premerge: misaligned buffer");
    const PremergeLayout l = premerge_layout(n_labels, edge_capacity);
    if (workspace_bytes < l.bytes) {
        set_error("region_graph_premerge: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
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
    int* parent = reinterpret_cast<int*>(ws + l.parent_a_off);
    int* spare = reinterpret_cast<int*>(ws + l.parent_b_off);
    int* min_id = reinterpret_cast<int*>(ws + l.min_off);
    int* label_blocks = reinterpret_cast<int*>(ws + l.blocks_off);
    unsigned long long* sizes_out = reinterpret_cast<unsigned long long*>(sizes_out_dev);
    const Graph g{edges_dev, reinterpret_cast<const unsigned long long*>(count_dev),
                  reinterpret_cast<const unsigned long long*>(sum_dev), reinterpret_cast<const long long*>(sizes_dev),
                  (long long)n_edges, n_labels};
    const MergeBound bound = merge_bound(threshold);
    const size_t n = (size_t)n_labels + 1;

    EXA_CHECK_HIP(hipMemsetAsync(best, 0xFF, n * 4, s));
    EXA_CHECK_HIP(hipMemsetAsync(to.keys, 0xFF, (size_t)edge_capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(to.counts, 0, (size_t)edge_capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(to.sums, 0, (size_t)edge_capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(sizes_out, 0, n * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(state_dev, 0, 3 * sizeof(int32_t), s));
    const unsigned edge_grid = capped_grid((size_t)n_edges, kThreads), label_grid = capped_grid(n, kThreads);
    if (size_floor > 0) choose<<<edge_grid, kThreads, 0, s>>>(g, bound.m, bound.merge_all, size_floor, best);
    resolve<<<label_grid, kThreads, 0, s>>>(g, best, parent, min_id);
    // a chain is at most K - 1 steps long and a launch doubles what every pointer spans
    int launches = 1;
    while ((1ll << (launches - 1)) < (long long)n_labels) ++launches;
    for (int i = 0; i < launches; ++i) {
        double_parents<<<label_grid, kThreads, 0, s>>>(parent, spare, n);
        int* t = parent;
        parent = spare;
        spare = t;
    }
    set_min<<<label_grid, kThreads, 0, s>>>(parent, min_id, n);
    const SetHead head{parent, min_id, map_dev};
    const unsigned label_scan_grid = (unsigned)l.n_scan_blocks;
    scan_count<<<label_scan_grid, kThreads, 0, s>>>(head, label_blocks, n);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(label_blocks, l.n_scan_blocks, state_dev);
    scan_assign<<<label_scan_grid, kThreads, 0, s>>>(head, label_blocks, n);
    finish_map<<<label_grid, kThreads, 0, s>>>(parent, min_id, g.sizes, map_dev, sizes_out, n);
    contract<<<edge_grid, kThreads, 0, s>>>(g, map_dev, to, false);
    const UsedSlot used{to.keys, to.counts, to.sums, edges_out_dev, reinterpret_cast<long long*>(count_out_dev),
                        reinterpret_cast<unsigned long long*>(sum_out_dev)};
    const unsigned table_scan_grid = (unsigned)l.table.n_scan_blocks;
    scan_count<<<table_scan_grid, kThreads, 0, s>>>(used, table_blocks, (size_t)edge_capacity);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(table_blocks, l.table.n_scan_blocks, state_dev + 1 + kEdges);
    scan_assign<<<table_scan_grid, kThreads, 0, s>>>(used, table_blocks, (size_t)edge_capacity);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}
