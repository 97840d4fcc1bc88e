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
//
// The same graph for a volume that arrives in z slabs (exaspim_region_graph_stream_*): the
// global table, a 64-bit voxel count per provisional id and two planes carried from slab to slab (the
// last plane's ids and its quantised z affinities) are the caller's. Per slab:
//   seam_graph   one thread per (y, x) of the seam above the slab: carried id, this slab's first-plane
//                id, carried q, through a workgroup's LDS table and one flush, as in tile_graph;
//   tile_graph   the slab as a volume of its own, (l, l) runs into the counts per id;
//   carry_planes the slab's last plane of ids and q(channel 0) for the next seam.
// finish: retarget walks the provisional table, maps both ends of every key through the caller's table
// and re-adds what is left into a second table, retarget_sizes does the same for the voxel counts, and
// the scan turns the second table into the edge list. The provisional table is only read.
#include "edge_table.h"

namespace exaspim {
namespace {

constexpr int kLdsSlots = 2048;                // LDS table of a tile: 20 B per slot
constexpr int kLdsProbes = 16;
constexpr int kHZ = kTZ + 1, kHY = kTY + 1, kHX = kTX + 1;   // the tile with its +1 halo
constexpr int kHaloVox = kHZ * kHY * kHX;                    // 2673

// q(a): NaN and everything below 0 to 0, everything above 1 to 2^24; a * 2^24 is exact in float32
__device__ __forceinline__ unsigned quantise(float a) {
    a = a > 0.f ? a : 0.f;
    a = a < 1.f ? a : 1.f;
    return __float2uint_rn(a * 16777216.f);
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

__device__ __forceinline__ void lds_clear(const LdsTable& t) {
    for (int s = threadIdx.x; s < kLdsSlots; s += kThreads) {
        t.keys[s] = kEmpty;
        t.sums[s] = 0;
        t.counts[s] = 0;
    }
}

// one global update per distinct key of the workgroup's table: edges into the global table, (l, l) into
// sizes[l]; the slots are left empty. The caller synchronises before and after.
__device__ __forceinline__ void lds_flush(const LdsTable& t, const Table& g, unsigned long long* sizes) {
    for (int s = threadIdx.x; s < kLdsSlots; s += kThreads) {
        const unsigned long long key = t.keys[s];
        if (key == kEmpty) continue;
        const unsigned lo = (unsigned)(key >> 32), hi = (unsigned)key;
        if (lo == hi)
            atomicAdd(sizes + lo, (unsigned long long)t.counts[s]);
        else
            global_add(g, key, t.counts[s], t.sums[s]);
        t.keys[s] = kEmpty;
        t.sums[s] = 0;
        t.counts[s] = 0;
    }
}

// The whole-volume call and the slab call share this kernel: a slab is a volume of its own whose (l, l)
// runs go to the counts per provisional id, and whose table the caller has not reset.
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
    lds_clear(lt);
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
        lds_flush(lt, g, sizes);
        __syncthreads();   // hl and the table are reused by the next tile
    }
}

// ---- the streamed form ---------------------------------------------------------------------------
constexpr int kSeamPerBlock = 16 * kThreads;   // (y, x) positions a workgroup of seam_graph pools

// The seam above a slab: the edge from the previous slab's last plane (its carried ids and carried q)
// to this slab's first plane, at every (y, x). A face where two large fragments meet puts the whole
// plane on one key, so the contributions are pooled in LDS like a tile's: one global update per
// distinct key and workgroup.
__global__ __launch_bounds__(kThreads) void seam_graph(const int* __restrict__ above,
                                                      const unsigned* __restrict__ above_q,
                                                      const int* __restrict__ below, int plane, int id_capacity,
                                                      Table g) {
    __shared__ unsigned long long lkeys[kLdsSlots];
    __shared__ unsigned long long lsums[kLdsSlots];
    __shared__ unsigned lcounts[kLdsSlots];
    const LdsTable lt{lkeys, lsums, lcounts};
    lds_clear(lt);
    __syncthreads();
    const long long stride = (long long)gridDim.x * kSeamPerBlock;
    for (long long base = (long long)blockIdx.x * kSeamPerBlock; base < plane; base += stride) {
#pragma unroll
        for (int k = 0; k < kSeamPerBlock / kThreads; ++k) {
            const long long i = base + k * kThreads + threadIdx.x;
            if (i >= plane) break;
            const int la = above[i], lb = below[i];
            if (la > 0 && lb > 0 && la != lb && la <= id_capacity && lb <= id_capacity) {
                const unsigned q = above_q[i];
                const unsigned long long key = edge_key(la, lb);
                if (!lds_add(lt, key, 1, q)) global_add(g, key, 1, q);
            }
        }
    }
    __syncthreads();
    lds_flush(lt, g, nullptr);   // no (l, l) key was added
}

// What the next seam needs of a slab: its last plane of ids, and q of that plane's z affinities. Four
// voxels per thread where all four pointers allow.
template <typename T>
__global__ __launch_bounds__(kThreads) void carry_planes(const int* __restrict__ last_ids,
                                                        const T* __restrict__ last_aff, int* __restrict__ ids_out,
                                                        unsigned* __restrict__ q_out, int plane) {
    struct alignas(4 * sizeof(T)) T4 { T v[4]; };
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool wide = (((uintptr_t)last_ids | (uintptr_t)ids_out | (uintptr_t)q_out) & 15) == 0 &&
                      ((uintptr_t)last_aff & (4 * sizeof(T) - 1)) == 0;
    const size_t quads = wide ? (size_t)plane / 4 : 0;
    for (size_t i = first; i < quads; i += stride) {
        reinterpret_cast<int4*>(ids_out)[i] = reinterpret_cast<const int4*>(last_ids)[i];
        const T4 a = reinterpret_cast<const T4*>(last_aff)[i];
        uint4 q;
        q.x = quantise(widen<T>(a.v[0])); q.y = quantise(widen<T>(a.v[1]));
        q.z = quantise(widen<T>(a.v[2])); q.w = quantise(widen<T>(a.v[3]));
        reinterpret_cast<uint4*>(q_out)[i] = q;
    }
    for (size_t i = quads * 4 + first; i < (size_t)plane; i += stride) {
        ids_out[i] = last_ids[i];
        q_out[i] = quantise(widen<T>(last_aff[i]));
    }
}

// finish: every occupied slot of the provisional table, its two ids through the caller's table, into
// the second table. An id at or beyond table_len, an end outside 1 .. n_labels and equal ends drop it.
__global__ __launch_bounds__(kThreads) void retarget(Table from, const int* __restrict__ table, int table_len,
                                                    int n_labels, Table to) {
    const size_t slots = (size_t)from.mask + 1, stride = (size_t)gridDim.x * blockDim.x;
    size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    // an overflowed provisional table makes the output as unusable as an overflowed second one
    if (s == 0 && from.state[kOverflow]) atomicExch(to.state + kOverflow, 1);
    for (; s < slots; s += stride) {
        const unsigned long long key = from.keys[s];
        if (key == kEmpty) continue;
        const unsigned a = (unsigned)(key >> 32), b = (unsigned)key;
        if (a >= (unsigned)table_len || b >= (unsigned)table_len) continue;
        const int la = table[a], lb = table[b];
        if (la < 1 || lb < 1 || la > n_labels || lb > n_labels || la == lb) continue;
        global_add(to, edge_key(la, lb), from.counts[s], from.sums[s]);
    }
}

// sizes[table[id]] += sizes_by_id[id]; ids the table does not hold, or maps outside 0 .. n_labels, are
// background
__global__ __launch_bounds__(kThreads) void retarget_sizes(const unsigned long long* __restrict__ sizes_by_id,
                                                          size_t n_ids, const int* __restrict__ table, int table_len,
                                                          int n_labels, unsigned long long* sizes) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < n_ids; id += stride) {
        const unsigned long long c = sizes_by_id[id];
        if (c == 0) continue;
        int l = id < (size_t)table_len ? table[id] : 0;
        if ((unsigned)l > (unsigned)n_labels) l = 0;
        atomicAdd(sizes + l, c);
    }
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

namespace exaspim {
namespace {

// the descriptor's own fields, checked before anything is launched; "plane" = dims[1] * dims[2]
const char* stream_fault(const exaspim_region_graph_stream* st, int* plane) {
    if (!st) return "NULL descriptor";
    if (st->dims[0] <= 0 || st->dims[1] <= 0 || st->dims[2] <= 0) return "dims must be positive";
    const long long p = (long long)st->dims[1] * st->dims[2];
    if (p > 2147483647ll) return "a plane of more than 2^31 - 1 voxels";
    *plane = (int)p;
    if (st->id_capacity < 1 || st->id_capacity > 2147483646) return "id_capacity must be 1 .. 2^31 - 2";
    if (!valid_capacity(st->edge_capacity)) return "edge_capacity must be a power of two in 1 .. 2^30";
    if (st->next_z < 0 || st->next_z > st->dims[0]) return "next_z outside the volume";
    if (!st->keys_dev || !st->counts_dev || !st->sums_dev || !st->sizes_by_id_dev || !st->seam_ids_dev ||
        !st->seam_q_dev || !st->state_dev)
        return "NULL buffer in the descriptor";
    if ((((uintptr_t)st->keys_dev | (uintptr_t)st->counts_dev | (uintptr_t)st->sums_dev |
          (uintptr_t)st->sizes_by_id_dev) & 7) != 0 ||
        (((uintptr_t)st->seam_ids_dev | (uintptr_t)st->seam_q_dev | (uintptr_t)st->state_dev) & 3) != 0)
        return "misaligned buffer in the descriptor";
    return nullptr;
}

Table table_of(const exaspim_region_graph_stream* st) {
    return Table{reinterpret_cast<unsigned long long*>(st->keys_dev),
                 reinterpret_cast<unsigned long long*>(st->counts_dev),
                 reinterpret_cast<unsigned long long*>(st->sums_dev), (unsigned)(st->edge_capacity - 1),
                 st->state_dev};
}

}  // namespace
}  // namespace exaspim

extern "C" int exaspim_region_graph_stream_slab(exaspim_region_graph_stream* st, const int32_t* labels_dev,
                                                const void* aff_dev, int32_t aff_dtype,
                                                const int32_t slab_dims[3], int32_t z0, void* stream) {
    int plane = 0;
    const char* fault = stream_fault(st, &plane);
    EXA_CHECK_ARG(!fault, "region_graph_stream_slab: %s", fault);
    EXA_CHECK_ARG(labels_dev && aff_dev && slab_dims, "region_graph_stream_slab: NULL argument");
    EXA_CHECK_ARG(aff_dtype == EXASPIM_AFF_F32 || aff_dtype == EXASPIM_AFF_F16,
                  "region_graph_stream_slab: aff_dtype %d is neither EXASPIM_AFF_F32 nor EXASPIM_AFF_F16", aff_dtype);
    Dims dm;
    EXA_CHECK_ARG(valid_dims(slab_dims, &dm),
                  "region_graph_stream_slab: slab_dims must be positive with a product of at most 2^31 - 1");
    EXA_CHECK_ARG(dm.h == st->dims[1] && dm.w == st->dims[2],
                  "region_graph_stream_slab: a slab of (y, x) = (%d, %d) in a volume of (%d, %d)", dm.h, dm.w,
                  st->dims[1], st->dims[2]);
    EXA_CHECK_ARG(z0 == st->next_z, "region_graph_stream_slab: slab out of order: z0 = %d, %d planes were pushed", z0,
                  st->next_z);
    EXA_CHECK_ARG((long long)z0 + dm.d <= st->dims[0],
                  "region_graph_stream_slab: planes [%d, %lld) reach beyond the volume's %d", z0,
                  (long long)z0 + dm.d, st->dims[0]);
    EXA_CHECK_ARG(((uintptr_t)labels_dev & 3) == 0 &&
                      ((uintptr_t)aff_dev & (aff_dtype == EXASPIM_AFF_F32 ? 3 : 1)) == 0,
                  "region_graph_stream_slab: misaligned buffer");
    hipStream_t s = (hipStream_t)stream;
    const Table g = table_of(st);
    unsigned long long* sizes = reinterpret_cast<unsigned long long*>(st->sizes_by_id_dev);
    const size_t capacity = (size_t)st->edge_capacity;
    if (z0 == 0) {
        EXA_CHECK_HIP(hipMemsetAsync(g.keys, 0xFF, capacity * 8, s));
        EXA_CHECK_HIP(hipMemsetAsync(g.counts, 0, capacity * 8, s));
        EXA_CHECK_HIP(hipMemsetAsync(g.sums, 0, capacity * 8, s));
        EXA_CHECK_HIP(hipMemsetAsync(sizes, 0, ((size_t)st->id_capacity + 1) * 8, s));
        EXA_CHECK_HIP(hipMemsetAsync(st->state_dev, 0, 2 * sizeof(int32_t), s));
    } else {
        seam_graph<<<capped_grid((size_t)plane, kSeamPerBlock), kThreads, 0, s>>>(
            st->seam_ids_dev, st->seam_q_dev, labels_dev, plane, st->id_capacity, g);
    }
    const int tiles_x = (dm.w + kTX - 1) / kTX, tiles_y = (dm.h + kTY - 1) / kTY;
    const long long n_tiles = (long long)tiles_x * tiles_y * ((dm.d + kTZ - 1) / kTZ);
    const unsigned grid = capped_grid((size_t)n_tiles, 1);
    const bool carries = z0 + dm.d < st->dims[0];   // the volume's last plane carries nothing
    const size_t last = (size_t)(dm.d - 1) * plane;
    const unsigned carry_grid = capped_grid(((size_t)plane + 3) / 4, kThreads);
    if (aff_dtype == EXASPIM_AFF_F32) {
        const float* aff = static_cast<const float*>(aff_dev);
        tile_graph<float><<<grid, kThreads, 0, s>>>(labels_dev, aff, dm, st->id_capacity, tiles_x, tiles_y, n_tiles,
                                                    sizes, g);
        if (carries)
            carry_planes<float><<<carry_grid, kThreads, 0, s>>>(labels_dev + last, aff + last, st->seam_ids_dev,
                                                                st->seam_q_dev, plane);
    } else {
        const _Float16* aff = static_cast<const _Float16*>(aff_dev);
        tile_graph<_Float16><<<grid, kThreads, 0, s>>>(labels_dev, aff, dm, st->id_capacity, tiles_x, tiles_y,
                                                       n_tiles, sizes, g);
        if (carries)
            carry_planes<_Float16><<<carry_grid, kThreads, 0, s>>>(labels_dev + last, aff + last, st->seam_ids_dev,
                                                                   st->seam_q_dev, plane);
    }
    EXA_CHECK_HIP(hipGetLastError());
    st->next_z = z0 + dm.d;
    return EXASPIM_OK;
}

extern "C" size_t exaspim_region_graph_stream_finish_workspace_bytes(int64_t edge_capacity) {
    if (!valid_capacity(edge_capacity)) {
        set_error("region_graph_stream_finish_workspace_bytes: edge_capacity must be a power of two in 1 .. 2^30, "
                  "got %lld", (long long)edge_capacity);
        return 0;
    }
    return layout_of(edge_capacity).bytes;
}

extern "C" int exaspim_region_graph_stream_finish(const exaspim_region_graph_stream* st, const int32_t* table_dev,
                                                  int32_t table_len, int32_t n_labels, int32_t* edges_dev,
                                                  int64_t* count_dev, uint64_t* sum_dev, int64_t* sizes_dev,
                                                  int32_t* n_edges_dev, void* workspace_dev, size_t workspace_bytes,
                                                  void* stream) {
    int plane = 0;
    const char* fault = stream_fault(st, &plane);
    EXA_CHECK_ARG(!fault, "region_graph_stream_finish: %s", fault);
    EXA_CHECK_ARG(table_dev && edges_dev && count_dev && sum_dev && sizes_dev && n_edges_dev && workspace_dev,
                  "region_graph_stream_finish: NULL argument");
    EXA_CHECK_ARG(st->next_z == st->dims[0],
                  "region_graph_stream_finish: finish before the last plane: %d of %d planes were pushed", st->next_z,
                  st->dims[0]);
    EXA_CHECK_ARG(table_len >= 1, "region_graph_stream_finish: table_len must be positive, got %d", table_len);
    EXA_CHECK_ARG(n_labels >= 0, "region_graph_stream_finish: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && ((uintptr_t)table_dev & 3) == 0 &&
                      ((uintptr_t)edges_dev & 3) == 0 && ((uintptr_t)n_edges_dev & 3) == 0 &&
                      ((uintptr_t)count_dev & 7) == 0 && ((uintptr_t)sum_dev & 7) == 0 &&
                      ((uintptr_t)sizes_dev & 7) == 0,
                  "region_graph_stream_finish: misaligned buffer");
    const int64_t capacity = st->edge_capacity;
    const Layout l = layout_of(capacity);
    if (workspace_bytes < l.bytes) {
        set_error("region_graph_stream_finish: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace_dev);
    const Table from = table_of(st);
    const Table to{reinterpret_cast<unsigned long long*>(ws + l.keys_off),
                   reinterpret_cast<unsigned long long*>(ws + l.counts_off),
                   reinterpret_cast<unsigned long long*>(ws + l.sums_off), (unsigned)(capacity - 1), n_edges_dev};
    int* block_sums = reinterpret_cast<int*>(ws + l.blocks_off);
    unsigned long long* sizes = reinterpret_cast<unsigned long long*>(sizes_dev);

    EXA_CHECK_HIP(hipMemsetAsync(to.keys, 0xFF, (size_t)capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(to.counts, 0, (size_t)capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(to.sums, 0, (size_t)capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(sizes, 0, ((size_t)n_labels + 1) * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(n_edges_dev, 0, 2 * sizeof(int32_t), s));
    retarget<<<capped_grid((size_t)capacity, kThreads), kThreads, 0, s>>>(from, table_dev, table_len, n_labels, to);
    const size_t n_ids = (size_t)st->id_capacity + 1;
    retarget_sizes<<<capped_grid(n_ids, kThreads), kThreads, 0, s>>>(
        reinterpret_cast<const unsigned long long*>(st->sizes_by_id_dev), n_ids, table_dev, table_len, n_labels,
        sizes);
    const UsedSlot used{to.keys, to.counts, to.sums, edges_dev, reinterpret_cast<long long*>(count_dev),
                        reinterpret_cast<unsigned long long*>(sum_dev)};
    const unsigned scan_grid = (unsigned)l.n_scan_blocks;
    scan_count<<<scan_grid, kThreads, 0, s>>>(used, block_sums, (size_t)capacity);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(block_sums, l.n_scan_blocks, n_edges_dev + kEdges);
    scan_assign<<<scan_grid, kThreads, 0, s>>>(used, block_sums, (size_t)capacity);
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
