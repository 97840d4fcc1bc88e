// The region graph of a labelled volume (exaspim_region_graph; semantics in include/exaspim_affinity.h):
// for every pair of adjacent labels the number of voxel edges between them and the sum of their
// affinities, quantised to integers so that the sums do not depend on the order in which atomics
// land; and the number of voxels per label. DESIGN 6e.
//
// Passes, each a launch of its own on the caller's stream (no lock, no grid-wide barrier, no workgroup
// that waits for another one):
//   memsets      the global table's keys := empty, its counts and sums := 0, sizes := 0, state := 0;
//   tile_graph   a workgroup owns 8 x 8 x 32 tiles. It loads the tile's labels with their +1 halo in z,
//                y and x into LDS, adds every contribution -- an edge (lo, hi): 1 and q(a); a run of
//                equal labels in a wave (l, l): its length -- to an open-addressing table in LDS, and
//                flushes one global update per distinct key and tile: edges into the global table,
//                (l, l) into sizes[l]. What finds no LDS slot within kLdsProbes goes straight to the
//                global table / sizes;
//   scan_*       label_scan.h's three passes over the slots: the occupied ones, in slot order, become
//                the edge list.
// The global table is claimed slot by slot with a 64-bit atomicCAS on the empty key, then two 64-bit
// atomicAdds. A probe sequence visits every slot at most once, so it ends; when it ends without a
// slot, or the overflow flag is already up, the contribution is dropped and the flag raised: the host
// reads it once, with the edge count.
#include "label_scan.h"

namespace exaspim {
namespace {

constexpr unsigned long long kEmpty = ~0ull;   // no key: lo and hi are at most 2^31 - 1
constexpr int kLdsSlots = 2048;                // LDS table of a tile: 20 B per slot
constexpr int kLdsProbes = 16;
constexpr int kHZ = kTZ + 1, kHY = kTY + 1, kHX = kTX + 1;   // the tile with its +1 halo
constexpr int kHaloVox = kHZ * kHY * kHX;                    // 2673
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

// q(a): NaN and everything below 0 to 0, everything above 1 to 2^24; a * 2^24 is exact in float32
__device__ __forceinline__ unsigned quantise(float a) {
    a = a > 0.f ? a : 0.f;
    a = a < 1.f ? a : 1.f;
    return __float2uint_rn(a * 16777216.f);
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

struct LdsTable {
    unsigned long long* keys;
    unsigned long long* sums;
    unsigned* counts;
};

// the same in the tile's table; false if no slot was found within kLdsProbes
__device__ __forceinline__ bool lds_add(const LdsTable& t, unsigned long long key, unsigned cnt, unsigned sum) {
    unsigned slot = (unsigned)(mix(key) >> 40) & (kLdsSlots - 1);
    for (int p = 0; p < kLdsProbes; ++p, slot = (slot + 1) & (kLdsSlots - 1)) {
        unsigned long long k = *reinterpret_cast<volatile unsigned long long*>(t.keys + slot);
        if (k == kEmpty) {
            k = atomicCAS(t.keys + slot, kEmpty, key);
            if (k == kEmpty) k = key;
        }
        if (k == key) {
            atomicAdd(t.counts + slot, cnt);
            if (sum) atomicAdd(t.sums + slot, (unsigned long long)sum);
            return true;
        }
    }
    return false;
}

__device__ __forceinline__ unsigned long long edge_key(int a, int b) {
    const unsigned lo = (unsigned)(a < b ? a : b), hi = (unsigned)(a < b ? b : a);
    return (unsigned long long)lo << 32 | hi;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void tile_graph(const int* __restrict__ labels, const T* __restrict__ aff,
                                                      Dims dm, int n_labels, int tiles_x, int tiles_y,
                                                      long long n_tiles, unsigned long long* sizes, Table g) {
    __shared__ int hl[kHaloVox];   // the label, or -1 for what is no label or outside the volume
    __shared__ unsigned long long lkeys[kLdsSlots];
    __shared__ unsigned long long lsums[kLdsSlots];
    __shared__ unsigned lcounts[kLdsSlots];
    const LdsTable lt{lkeys, lsums, lcounts};
    const int t = threadIdx.x, lane = t & 63;
    for (int s = t; s < kLdsSlots; s += kThreads) {
        lkeys[s] = kEmpty;
        lsums[s] = 0;
        lcounts[s] = 0;
    }
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tx = (int)(tile % tiles_x), ty = (int)((tile / tiles_x) % tiles_y);
        const int tz = (int)(tile / ((long long)tiles_x * tiles_y));
        const int x0 = tx * kTX, y0 = ty * kTY, z0 = tz * kTZ;
        for (int i = t; i < kHaloVox; i += kThreads) {
            const int hx = i % kHX, hy = (i / kHX) % kHY, hz = i / (kHX * kHY);
            const int x = x0 + hx, y = y0 + hy, z = z0 + hz;
            int l = -1;
            if (x < dm.w && y < dm.h && z < dm.d) {
                l = labels[((size_t)z * dm.h + y) * dm.w + x];
                if ((unsigned)l > (unsigned)n_labels) l = -1;
            }
            hl[i] = l;
        }
        __syncthreads();   // also: the table is empty (initialised above, or by the previous flush)
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int i = t + kThreads * k;
            const int lx = i & (kTX - 1), ly = (i >> 5) & (kTY - 1), lz = i >> 8;
            const int h = (lz * kHY + ly) * kHX + lx;
            const int la = hl[h];
            // voxels per label: lanes of a wave hold consecutive voxels of two tile rows, a run of
            // lanes with the same label adds its length once, from its first lane
            const int val = la >= 0 ? la : -1 - lane;
            const int prev = __shfl_up(val, 1);
            const bool head = lane == 0 || prev != val;
            const unsigned long long heads = __ballot(head);
            if (la >= 0 && head) {
                const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
                const unsigned len = above ? (unsigned)__ffsll((long long)above) : 64u - lane;
                if (!lds_add(lt, edge_key(la, la), len, 0)) atomicAdd(sizes + la, (unsigned long long)len);
            }
            if (la > 0) {
                // the halo holds -1 beyond the volume, so an edge that leaves it is no edge
                const int nb[3] = {hl[h + kHY * kHX], hl[h + kHX], hl[h + 1]};
                const size_t v = ((size_t)(z0 + lz) * dm.h + (y0 + ly)) * dm.w + (x0 + lx);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int lb = nb[c];
                    if (lb > 0 && lb != la) {
                        const unsigned q = quantise(widen<T>(aff[(size_t)c * dm.n + v]));
                        const unsigned long long key = edge_key(la, lb);
                        if (!lds_add(lt, key, 1, q)) global_add(g, key, 1, q);
                    }
                }
            }
        }
        __syncthreads();
        // one global update per distinct key of the tile; the slots are left empty for the next one
        for (int s = t; s < kLdsSlots; s += kThreads) {
            const unsigned long long key = lkeys[s];
            if (key == kEmpty) continue;
            const unsigned lo = (unsigned)(key >> 32), hi = (unsigned)key;
            if (lo == hi)
                atomicAdd(sizes + lo, (unsigned long long)lcounts[s]);
            else
                global_add(g, key, lcounts[s], lsums[s]);
            lkeys[s] = kEmpty;
            lsums[s] = 0;
            lcounts[s] = 0;
        }
        __syncthreads();   // hl and the table are reused by the next tile
    }
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

using namespace exaspim;

extern "C" size_t exaspim_region_graph_workspace_bytes(const int32_t dims[3], int32_t n_labels,
                                                       int64_t edge_capacity) {
    Dims dm;
    if (!valid_dims(dims, &dm)) {
        set_error("region_graph_workspace_bytes: dims must be positive with a product of at most 2^31 - 1");
        return 0;
    }
    if (n_labels < 0) {
        set_error("region_graph_workspace_bytes: n_labels must not be negative, got %d", n_labels);
        return 0;
    }
    if (!valid_capacity(edge_capacity)) {
        set_error("region_graph_workspace_bytes: edge_capacity must be a power of two in 1 .. 2^30, got %lld",
                  (long long)edge_capacity);
        return 0;
    }
    return layout_of(edge_capacity).bytes;
}

extern "C" int exaspim_region_graph(const int32_t* labels_dev, const void* aff_dev, int32_t aff_dtype,
                                    const int32_t dims[3], int32_t n_labels, int64_t edge_capacity,
                                    int32_t* edges_dev, int64_t* count_dev, uint64_t* sum_dev,
                                    int64_t* sizes_dev, int32_t* n_edges_dev, void* workspace_dev,
                                    size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && aff_dev && dims && edges_dev && count_dev && sum_dev && sizes_dev && n_edges_dev &&
                      workspace_dev,
                  "region_graph: NULL argument");
    EXA_CHECK_ARG(aff_dtype == EXASPIM_AFF_F32 || aff_dtype == EXASPIM_AFF_F16,
                  "region_graph: aff_dtype %d is neither EXASPIM_AFF_F32 nor EXASPIM_AFF_F16", aff_dtype);
    Dims dm;
    EXA_CHECK_ARG(valid_dims(dims, &dm), "region_graph: dims must be positive with a product of at most 2^31 - 1");
    EXA_CHECK_ARG(n_labels >= 0, "region_graph: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(valid_capacity(edge_capacity),
                  "region_graph: edge_capacity must be a power of two in 1 .. 2^30, got %lld",
                  (long long)edge_capacity);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && ((uintptr_t)labels_dev & 3) == 0 &&
                      ((uintptr_t)edges_dev & 3) == 0 && ((uintptr_t)n_edges_dev & 3) == 0 &&
                      ((uintptr_t)count_dev & 7) == 0 && ((uintptr_t)sum_dev & 7) == 0 &&
                      ((uintptr_t)sizes_dev & 7) == 0 &&
                      ((uintptr_t)aff_dev & (aff_dtype == EXASPIM_AFF_F32 ? 3 : 1)) == 0,
                  "region_graph: misaligned buffer");
    const Layout l = layout_of(edge_capacity);
    if (workspace_bytes < l.bytes) {
        set_error("region_graph: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace_dev);
    const Table g{reinterpret_cast<unsigned long long*>(ws + l.keys_off),
                  reinterpret_cast<unsigned long long*>(ws + l.counts_off),
                  reinterpret_cast<unsigned long long*>(ws + l.sums_off), (unsigned)(edge_capacity - 1), n_edges_dev};
    int* block_sums = reinterpret_cast<int*>(ws + l.blocks_off);
    unsigned long long* sizes = reinterpret_cast<unsigned long long*>(sizes_dev);

    EXA_CHECK_HIP(hipMemsetAsync(g.keys, 0xFF, (size_t)edge_capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(g.counts, 0, (size_t)edge_capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(g.sums, 0, (size_t)edge_capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(sizes, 0, ((size_t)n_labels + 1) * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(n_edges_dev, 0, 2 * sizeof(int32_t), s));
    const int tiles_x = (dm.w + kTX - 1) / kTX, tiles_y = (dm.h + kTY - 1) / kTY;
    const long long n_tiles = (long long)tiles_x * tiles_y * ((dm.d + kTZ - 1) / kTZ);
    const unsigned grid = capped_grid((size_t)n_tiles, 1);
    if (aff_dtype == EXASPIM_AFF_F32)
        tile_graph<float><<<grid, kThreads, 0, s>>>(labels_dev, static_cast<const float*>(aff_dev), dm, n_labels,
                                                    tiles_x, tiles_y, n_tiles, sizes, g);
    else
        tile_graph<_Float16><<<grid, kThreads, 0, s>>>(labels_dev, static_cast<const _Float16*>(aff_dev), dm,
                                                       n_labels, tiles_x, tiles_y, n_tiles, sizes, g);
    const UsedSlot used{g.keys, g.counts, g.sums, edges_dev, reinterpret_cast<long long*>(count_dev),
                        reinterpret_cast<unsigned long long*>(sum_dev)};
    const unsigned scan_grid = (unsigned)l.n_scan_blocks;
    scan_count<<<scan_grid, kThreads, 0, s>>>(used, block_sums, (size_t)edge_capacity);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(block_sums, l.n_scan_blocks, n_edges_dev + kEdges);
    scan_assign<<<scan_grid, kThreads, 0, s>>>(used, block_sums, (size_t)edge_capacity);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" int exaspim_apply_label_table(int32_t* labels_dev, size_t n, const int32_t* table_dev, int32_t table_len,
                                         void* stream) {
    EXA_CHECK_ARG(labels_dev && table_dev && ((uintptr_t)labels_dev & 3) == 0 && ((uintptr_t)table_dev & 3) == 0,
                  "apply_label_table: NULL or misaligned buffer");
    EXA_CHECK_ARG(table_len >= 1, "apply_label_table: table_len must be positive, got %d", table_len);
    if (n == 0) return EXASPIM_OK;
    apply_table<<<capped_grid((n + 3) / 4, kThreads), kThreads, 0, (hipStream_t)stream>>>(labels_dev, table_dev,
                                                                                        table_len - 1, n);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}
