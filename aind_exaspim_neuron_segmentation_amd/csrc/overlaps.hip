// The overlap table of two label volumes (exaspim_label_overlaps*; semantics in include/exaspim_affinity.h):
// for every ordered pair (label in a, label in b) that occurs at some voxel, the number of voxels that carry
// it. Everything <= 0 is background and counts as 0. 64-bit integer counts, so the result does not depend on
// the order in which atomics land, and the table is additive over voxels: any number of adds, of any lengths,
// give the table of their concatenation. DESIGN 6u.
//
// Passes, each a launch of its own on the caller's stream (no lock, no grid-wide barrier, no workgroup that
// waits for another one):
//   reset         memsets: the global table's keys := empty, its counts := 0, the overflow word := 0;
//   overlaps_add  a workgroup strides over chunks of kOvChunk voxels of the flat range. A lane takes four
//                 consecutive voxels, with 16-byte loads where the quad is whole; runs of equal pairs are
//                 collapsed to (key, length) inside the lane and, for lanes whose four voxels agree, across the
//                 wave (tile_graph's shuffle / ballot run heads); (key, length) goes to an open-addressing table
//                 in LDS, and what finds no slot within kOvProbes straight to the global table. The LDS table
//                 is kept from chunk to chunk and flushed -- one global update per distinct key -- after a
//                 chunk in which some lane found no slot, and when the workgroup ends;
//   scan_*        label_scan.h's three passes over the slots: the occupied ones, in slot order, become the
//                 rows. They only read the table; the block sums are the only workspace words they write.
// The global table has two columns (a 64-bit key and a 64-bit count per slot), claimed slot by slot with a
// 64-bit atomicCAS on the empty key as edge_table.h's is; its overflow word lives in the workspace because the
// table outlives the call that made it.
#include "edge_table.h"

namespace exaspim {
namespace {

constexpr int kOvRounds = 4;                              // quads per lane and chunk
constexpr int kOvChunk = 4 * kThreads * kOvRounds;        // 4096 voxels
constexpr unsigned kOvMaxGrid = 2048;                     // workgroups of overlaps_add at the most
constexpr int kOvSlots = 2048;                            // LDS table of a workgroup: 12 B per slot
constexpr int kOvProbes = 16;
constexpr long long kOvMaxVoxels = 2147483647ll;          // per add

struct PairTable {
    unsigned long long* keys;
    unsigned long long* counts;
    unsigned mask;   // capacity - 1
    int* overflow;   // one word in the workspace
};

// the ordered pair: a' in the high half, b' in the low one; v' = v if v > 0 else 0
__device__ __forceinline__ unsigned long long pair_key(int a, int b) {
    const unsigned ua = a > 0 ? (unsigned)a : 0u, ub = b > 0 ? (unsigned)b : 0u;
    return (unsigned long long)ua << 32 | ub;
}

// count[key] += cnt in the global table (edge_table.h's global_add without the sums)
__device__ void pair_add(const PairTable& g, unsigned long long key, unsigned long long cnt) {
    unsigned slot = (unsigned)(mix(key) >> 32) & g.mask;
    for (unsigned p = 0; p <= g.mask; ++p, slot = (slot + 1) & g.mask) {
        // a table that has overflowed is unusable: do not walk it again for every later key
        if ((p & 63) == 0 && __hip_atomic_load(g.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        unsigned long long k = __hip_atomic_load(g.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kEmpty) {
            k = atomicCAS(g.keys + slot, kEmpty, key);
            if (k == kEmpty) k = key;
        }
        if (k == key) {
            atomicAdd(g.counts + slot, cnt);
            return;
        }
    }
    atomicExch(g.overflow, 1);
}

// the same in the workgroup's table; false if no slot was found within kOvProbes
__device__ __forceinline__ bool lds_pair_add(unsigned long long* keys, unsigned* counts, unsigned long long key,
                                             unsigned cnt) {
    unsigned slot = (unsigned)(mix(key) >> 40) & (kOvSlots - 1);
    for (int p = 0; p < kOvProbes; ++p, slot = (slot + 1) & (kOvSlots - 1)) {
        unsigned long long k = *reinterpret_cast<volatile unsigned long long*>(keys + slot);
        if (k == kEmpty) {
            k = atomicCAS(keys + slot, kEmpty, key);
            if (k == kEmpty) k = key;
        }
        if (k == key) {
            atomicAdd(counts + slot, cnt);
            return true;
        }
    }
    return false;
}

// one global update per distinct key of the workgroup's table; the slots are left empty. The caller
// synchronises before and after.
__device__ __forceinline__ void lds_pair_flush(unsigned long long* keys, unsigned* counts, const PairTable& g) {
    for (int s = threadIdx.x; s < kOvSlots; s += kThreads) {
        const unsigned long long key = keys[s];
        if (key == kEmpty) continue;
        pair_add(g, key, counts[s]);
        keys[s] = kEmpty;
        counts[s] = 0;
    }
}

// Voxel i of the call is "virtual" voxel i + pad, pad = the number of int32 between the 16-byte boundary at or
// below a and a itself: a quad of virtual voxels 4 j .. 4 j + 3 that lies inside the range is one aligned
// 16-byte load of a, and of b where b has the same pad (wide_b). The first and the last quad may be partial:
// their voxels, and every voxel of b elsewhere, are loaded one by one and only inside [0, n).
__global__ __launch_bounds__(kThreads) void overlaps_add(const int* __restrict__ a, const int* __restrict__ b,
                                                        long long n, int pad, int wide_b, long long n_chunks,
                                                        PairTable g) {
    __shared__ unsigned long long lkeys[kOvSlots];
    __shared__ unsigned lcounts[kOvSlots];
    // "some lane of this chunk found no slot": the chunks of a workgroup take the two words in turn, so that
    // the word a chunk reads between its two barriers is cleared after the second one and next written after
    // the following chunk's
    __shared__ int lspilled[2];
    const int t = threadIdx.x, lane = t & 63;
    for (int s = t; s < kOvSlots; s += kThreads) {
        lkeys[s] = kEmpty;
        lcounts[s] = 0;
    }
    if (t < 2) lspilled[t] = 0;
    __syncthreads();
    const long long end = n + pad;
    int turn = 0;
    for (long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x, turn ^= 1) {
        volatile int* spilled = lspilled + turn;
        auto add = [&](unsigned long long key, unsigned len) {
            if (!lds_pair_add(lkeys, lcounts, key, len)) {
                *spilled = 1;
                pair_add(g, key, len);
            }
        };
#pragma unroll
        for (int r = 0; r < kOvRounds; ++r) {
            const long long u = chunk * kOvChunk + ((long long)r * kThreads + t) * 4;
            unsigned long long key[4] = {0, 0, 0, 0};
            unsigned valid = 0;
            if (u >= pad && u + 4 <= end) {
                const long long i = u - pad;
                const int4 va = *reinterpret_cast<const int4*>(a + i);
                int4 vb;
                if (wide_b) {
                    vb = *reinterpret_cast<const int4*>(b + i);
                } else {
                    vb.x = b[i]; vb.y = b[i + 1]; vb.z = b[i + 2]; vb.w = b[i + 3];
                }
                key[0] = pair_key(va.x, vb.x); key[1] = pair_key(va.y, vb.y);
                key[2] = pair_key(va.z, vb.z); key[3] = pair_key(va.w, vb.w);
                valid = 15;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long long i = u + k - pad;
                    if (i >= 0 && i < n) {
                        key[k] = pair_key(a[i], b[i]);
                        valid |= 1u << k;
                    }
                }
            }
            // Lanes of a wave hold consecutive quads. A lane whose four pairs agree is a link of a run of
            // such lanes, which adds its length once, from its first lane; every other lane is a run head of
            // its own under a value no key has (bit 63) and adds the runs inside its quad itself.
            const bool uniform = valid == 15 && key[0] == key[1] && key[1] == key[2] && key[2] == key[3];
            const unsigned long long val = uniform ? key[0] : (1ull << 63 | (unsigned)lane);
            const unsigned long long prev = __shfl_up(val, 1);
            const bool head = lane == 0 || prev != val;
            const unsigned long long heads = __ballot(head);
            if (uniform) {
                if (head) {
                    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
                    const unsigned lanes = above ? (unsigned)__ffsll((long long)above) : 64u - lane;
                    add(key[0], 4 * lanes);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!(valid >> k & 1)) continue;
                    if (k > 0 && (valid >> (k - 1) & 1) && key[k - 1] == key[k]) continue;   // not a run's first
                    unsigned len = 1;
                    for (int j = k + 1; j < 4 && (valid >> j & 1) && key[j] == key[k]; ++j) ++len;
                    add(key[k], len);
                }
            }
        }
        // a chunk that found the table full leaves it fresh for the next one: the keys change along the range
        __syncthreads();
        if (*spilled) lds_pair_flush(lkeys, lcounts, g);
        __syncthreads();
        if (t == 0) *spilled = 0;
    }
    lds_pair_flush(lkeys, lcounts, g);
}

// the scan's predicate and sink: occupied slots, in slot order, become the rows; slot 0's thread copies the
// overflow word
struct UsedPair {
    const unsigned long long* keys;
    const unsigned long long* counts;
    const int* overflow;
    int* pairs;
    long long* count_out;
    int* state;
    __device__ __forceinline__ bool operator()(size_t v) const { return keys[v] != kEmpty; }
    __device__ __forceinline__ void operator()(size_t v, bool flag, int rank) const {
        if (v == 0) state[kOverflow] = *overflow != 0;
        if (!flag) return;
        const unsigned long long key = keys[v];
        pairs[2 * (size_t)rank] = (int)(key >> 32);
        pairs[2 * (size_t)rank + 1] = (int)(unsigned)key;
        count_out[rank] = (long long)counts[v];
    }
};

// a table of "capacity" slots, its overflow word and the block sums of the scan over the slots
struct PairLayout {
    size_t keys_off, counts_off, overflow_off, blocks_off, bytes;
    long long n_scan_blocks;
};

PairLayout pair_layout_of(int64_t capacity) {
    PairLayout l;
    l.n_scan_blocks = (capacity + kScanBlock - 1) / kScanBlock;
    l.keys_off = 0;
    l.counts_off = align_up((size_t)capacity * 8, 256);
    l.overflow_off = 2 * l.counts_off;
    l.blocks_off = l.overflow_off + 256;
    l.bytes = l.blocks_off + align_up((size_t)l.n_scan_blocks * 4, 256);
    return l;
}

PairTable pair_table_of(void* workspace_dev, const PairLayout& l, int64_t capacity) {
    char* ws = static_cast<char*>(workspace_dev);
    return PairTable{reinterpret_cast<unsigned long long*>(ws + l.keys_off),
                     reinterpret_cast<unsigned long long*>(ws + l.counts_off), (unsigned)(capacity - 1),
                     reinterpret_cast<int*>(ws + l.overflow_off)};
}

// The refusals, decided from the values alone, in the name of the entry point "fn". 0, or the code to return.
int check_table(const char* fn, int64_t capacity, const void* workspace_dev, size_t workspace_bytes) {
    if (!valid_capacity(capacity)) {
        set_error("%s: pair_capacity must be a power of two in 1 .. 2^30, got %lld", fn, (long long)capacity);
        return EXASPIM_E_INVALID;
    }
    if (!workspace_dev) {
        set_error("%s: NULL argument", fn);
        return EXASPIM_E_INVALID;
    }
    if (((uintptr_t)workspace_dev & 15) != 0) {
        set_error("%s: misaligned buffer", fn);
        return EXASPIM_E_INVALID;
    }
    const size_t need = pair_layout_of(capacity).bytes;
    if (workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    return EXASPIM_OK;
}

int check_volumes(const char* fn, const int32_t* a_dev, const int32_t* b_dev, int64_t n) {
    if (n < 0 || n > kOvMaxVoxels) {
        set_error("%s: n must be 0 .. 2^31 - 1, got %lld", fn, (long long)n);
        return EXASPIM_E_INVALID;
    }
    if (!a_dev || !b_dev) {
        set_error("%s: NULL argument", fn);
        return EXASPIM_E_INVALID;
    }
    if ((((uintptr_t)a_dev | (uintptr_t)b_dev) & 3) != 0) {
        set_error("%s: misaligned buffer", fn);
        return EXASPIM_E_INVALID;
    }
    return EXASPIM_OK;
}

int check_outputs(const char* fn, const int32_t* pairs_dev, const int64_t* count_dev, const int32_t* state_dev) {
    if (!pairs_dev || !count_dev || !state_dev) {
        set_error("%s: NULL argument", fn);
        return EXASPIM_E_INVALID;
    }
    if ((((uintptr_t)pairs_dev | (uintptr_t)state_dev) & 3) != 0 || ((uintptr_t)count_dev & 7) != 0) {
        set_error("%s: misaligned buffer", fn);
        return EXASPIM_E_INVALID;
    }
    return EXASPIM_OK;
}

// the three steps behind the entry points: the arguments have been checked
int launch_reset(int64_t capacity, void* workspace_dev, hipStream_t s) {
    const PairLayout l = pair_layout_of(capacity);
    const PairTable g = pair_table_of(workspace_dev, l, capacity);
    EXA_CHECK_HIP(hipMemsetAsync(g.keys, 0xFF, (size_t)capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(g.counts, 0, (size_t)capacity * 8, s));
    EXA_CHECK_HIP(hipMemsetAsync(g.overflow, 0, sizeof(int), s));
    return EXASPIM_OK;
}

int launch_add(const int32_t* a_dev, const int32_t* b_dev, int64_t n, int64_t capacity, void* workspace_dev,
               hipStream_t s) {
    if (n == 0) return EXASPIM_OK;
    const PairTable g = pair_table_of(workspace_dev, pair_layout_of(capacity), capacity);
    const int pad = (int)(((uintptr_t)a_dev >> 2) & 3);
    const int wide_b = (int)(((uintptr_t)b_dev >> 2) & 3) == pad;
    const long long n_chunks = ((long long)n + pad + kOvChunk - 1) / kOvChunk;
    const unsigned grid = (unsigned)(n_chunks < (long long)kOvMaxGrid ? n_chunks : (long long)kOvMaxGrid);
    overlaps_add<<<grid, kThreads, 0, s>>>(a_dev, b_dev, (long long)n, pad, wide_b, n_chunks, g);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

int launch_finish(int64_t capacity, void* workspace_dev, int32_t* pairs_dev, int64_t* count_dev, int32_t* state_dev,
                  hipStream_t s) {
    const PairLayout l = pair_layout_of(capacity);
    const PairTable g = pair_table_of(workspace_dev, l, capacity);
    int* block_sums = reinterpret_cast<int*>(static_cast<char*>(workspace_dev) + l.blocks_off);
    const UsedPair used{g.keys, g.counts, g.overflow, pairs_dev, reinterpret_cast<long long*>(count_dev), state_dev};
    const unsigned scan_grid = (unsigned)l.n_scan_blocks;
    scan_count<<<scan_grid, kThreads, 0, s>>>(used, block_sums, (size_t)capacity);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(block_sums, l.n_scan_blocks, state_dev + kEdges);
    scan_assign<<<scan_grid, kThreads, 0, s>>>(used, block_sums, (size_t)capacity);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

}  // namespace
}  // namespace exaspim

using namespace exaspim;

extern "C" size_t exaspim_label_overlaps_workspace_bytes(int64_t pair_capacity) {
    if (!valid_capacity(pair_capacity)) {
        set_error("label_overlaps_workspace_bytes: pair_capacity must be a power of two in 1 .. 2^30, got %lld",
                  (long long)pair_capacity);
        return 0;
    }
    return pair_layout_of(pair_capacity).bytes;
}

extern "C" int exaspim_label_overlaps_reset(int64_t pair_capacity, void* workspace_dev, size_t workspace_bytes,
                                            void* stream) {
    if (const int rc = check_table("label_overlaps_reset", pair_capacity, workspace_dev, workspace_bytes)) return rc;
    return launch_reset(pair_capacity, workspace_dev, (hipStream_t)stream);
}

extern "C" int exaspim_label_overlaps_add(const int32_t* a_dev, const int32_t* b_dev, int64_t n,
                                          int64_t pair_capacity, void* workspace_dev, size_t workspace_bytes,
                                          void* stream) {
    if (const int rc = check_volumes("label_overlaps_add", a_dev, b_dev, n)) return rc;
    if (const int rc = check_table("label_overlaps_add", pair_capacity, workspace_dev, workspace_bytes)) return rc;
    return launch_add(a_dev, b_dev, n, pair_capacity, workspace_dev, (hipStream_t)stream);
}

extern "C" int exaspim_label_overlaps_finish(int64_t pair_capacity, void* workspace_dev, size_t workspace_bytes,
                                             int32_t* pairs_dev, int64_t* count_dev, int32_t* state_dev,
                                             void* stream) {
    if (const int rc = check_outputs("label_overlaps_finish", pairs_dev, count_dev, state_dev)) return rc;
    if (const int rc = check_table("label_overlaps_finish", pair_capacity, workspace_dev, workspace_bytes)) return rc;
    return launch_finish(pair_capacity, workspace_dev, pairs_dev, count_dev, state_dev, (hipStream_t)stream);
}

extern "C" int exaspim_label_overlaps(const int32_t* a_dev, const int32_t* b_dev, int64_t n, int64_t pair_capacity,
                                      int32_t* pairs_dev, int64_t* count_dev, int32_t* state_dev,
                                      void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (const int rc = check_volumes("label_overlaps", a_dev, b_dev, n)) return rc;
    if (const int rc = check_outputs("label_overlaps", pairs_dev, count_dev, state_dev)) return rc;
    if (const int rc = check_table("label_overlaps", pair_capacity, workspace_dev, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = launch_reset(pair_capacity, workspace_dev, s)) return rc;
    if (const int rc = launch_add(a_dev, b_dev, n, pair_capacity, workspace_dev, s)) return rc;
    return launch_finish(pair_capacity, workspace_dev, pairs_dev, count_dev, state_dev, s);
}
