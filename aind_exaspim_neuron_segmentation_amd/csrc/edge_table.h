// What region_graph.hip, premerge.hip and dominant.hip share: the global open-addressing table of edges (a 64-bit
// key, count and sum per slot), its claim-and-add, the scan's predicate and sink that turn the occupied
// slots into the edge list, and the workspace layout of one such table. Device code in a header: every
// file that includes it gets its own copies (anonymous namespace), as with label_scan.h.
#pragma once

#include "label_scan.h"

namespace exaspim {
namespace {

constexpr unsigned long long kEmpty = ~0ull;   // no key: lo and hi are at most 2^31 - 1
constexpr int kEdges = 0, kOverflow = 1;       // state words

struct Table {
    unsigned long long* keys;
    unsigned long long* counts;
    unsigned long long* sums;
    unsigned mask;   // capacity - 1
    int* state;
};

__device__ __forceinline__ unsigned long long mix(unsigned long long k) {
    k *= 0x9E3779B97F4A7C15ull;
    return k ^ (k >> 29);
}

__device__ __forceinline__ unsigned long long edge_key(int a, int b) {
    const unsigned lo = (unsigned)(a < b ? a : b), hi = (unsigned)(a < b ? b : a);
    return (unsigned long long)lo << 32 | hi;
}

// count[key] += cnt, sum[key] += sum in the global table
__device__ void global_add(const Table& g, unsigned long long key, unsigned long long cnt,
                           unsigned long long sum) {
    unsigned slot = (unsigned)(mix(key) >> 32) & g.mask;
    for (unsigned p = 0; p <= g.mask; ++p, slot = (slot + 1) & g.mask) {
        // a table that has overflowed is unusable: do not walk it again for every later key
        if ((p & 63) == 0 && __hip_atomic_load(g.state + kOverflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        unsigned long long k = __hip_atomic_load(g.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kEmpty) {
            k = atomicCAS(g.keys + slot, kEmpty, key);
            if (k == kEmpty) k = key;
        }
        if (k == key) {
            atomicAdd(g.counts + slot, cnt);
            atomicAdd(g.sums + slot, sum);
            return;
        }
    }
    atomicExch(g.state + kOverflow, 1);
}

// the scan's predicate and sink: occupied slots, in slot order, become the edge list
struct UsedSlot {
    const unsigned long long* keys;
    const unsigned long long* counts;
    const unsigned long long* sums;
    int* edges;
    long long* count_out;
    unsigned long long* sum_out;
    __device__ __forceinline__ bool operator()(size_t v) const { return keys[v] != kEmpty; }
    __device__ __forceinline__ void operator()(size_t v, bool flag, int rank) const {
        if (!flag) return;
        const unsigned long long key = keys[v];
        edges[2 * (size_t)rank] = (int)(key >> 32);
        edges[2 * (size_t)rank + 1] = (int)(unsigned)key;
        count_out[rank] = (long long)counts[v];
        sum_out[rank] = sums[v];
    }
};

// a table of "capacity" slots and the block sums of the scan over them
struct Layout {
    size_t keys_off, counts_off, sums_off, blocks_off, bytes;
    long long n_scan_blocks;
};

constexpr int64_t kMaxEdgeCapacity = 1ll << 30;

bool valid_capacity(int64_t c) { return c >= 1 && c <= kMaxEdgeCapacity && (c & (c - 1)) == 0; }

Layout layout_of(int64_t capacity) {
    Layout l;
    l.n_scan_blocks = (capacity + kScanBlock - 1) / kScanBlock;
    l.keys_off = 0;
    l.counts_off = align_up((size_t)capacity * 8, 256);
    l.sums_off = 2 * l.counts_off;
    l.blocks_off = 3 * l.counts_off;
    l.bytes = l.blocks_off + align_up((size_t)l.n_scan_blocks * 4, 256);
    return l;
}

}  // namespace
}  // namespace exaspim
