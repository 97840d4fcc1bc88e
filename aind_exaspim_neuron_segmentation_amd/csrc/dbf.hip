// The distance-to-boundary field of a labelled volume and the per-label table a skeletoniser crops and
// roots its segments with (exaspim_dbf, exaspim_segment_table; semantics in include/exaspim_affinity.h).
// DESIGN 6i. Everything in integers: squared distances, nothing rounded.
//
// exaspim_dbf, three passes, each a launch of its own on the caller's stream (no atomics, no lock, no
// workgroup that waits for another one):
//   dbf_x     a workgroup owns a row. The ends [a, b] of every voxel's run of equal labels come from a
//             forward max-scan of "index of the last label change" and a backward min-scan of "index of
//             the next one" over chunks of kThreads voxels, with a carry between chunks: the forward
//             carry is a register, the backward one a table in LDS that a first sweep over the row
//             fills (the first run end of every chunk). f = min((p - a + 1)^2, (b - p + 1)^2), a side
//             that ends at the face only under black_border.
//   dbf_axis  along y (from the output buffer into the workspace), then along z (back): one thread per
//             voxel, lanes along x, so the probe at offset +-k is one row segment per wave whatever the
//             axis. best = f(p); k = 1, 2, ... in both directions while k^2 < best: inside the run
//             best = min(best, f(q) + k^2), at the first voxel of another label or past the face under
//             black_border best = min(best, k^2) and the direction closes. Exact, since everything
//             at offset k is at least k^2; the cost is the window depth, sqrt(result) probes, and the
//             whole run where f is DBF_INF.
// exaspim_segment_table: table_init (sizes and keys 0, boxes empty), table_pass, table_finish.
//   table_pass  one thread per voxel; a run of equal labels inside a wave and a row is reduced in the
//               wave (its length from the ballot of run heads, its largest key by a segmented
//               shuffle scan) and its first lane updates the table: a 64-bit atomicAdd for the size,
//               int32 atomicMin / atomicMax for the box, a 64-bit atomicMax for the key
//               (dbf biased to unsigned << 32 | 0xFFFFFFFF - index: the largest value, then the
//               smallest index). Minima and maxima are monotone, so a plain load that already
//               covers the run's value spares the atomic; the result is a pure function of the input.
//               The run lengths are pooled per workgroup in a small open-addressing table in LDS, as
//               region_graph.hip's tiles pool theirs, and flushed once: a neurite a few voxels wide
//               is millions of short runs on one word of sizes. The voxels labelled 0 have a count
//               and nothing else: summed per wave, then per workgroup, one atomic each.
#include <algorithm>

#include "label_scan.h"

namespace exaspim {
namespace {

constexpr int kDbfInf = EXASPIM_DBF_INF;
// (W + 1)^2 < 2^31 - 1 bounds a row at 46339 voxels: the table of chunk carries of dbf_x
constexpr int kMaxRow = 46339;
constexpr int kMaxChunks = (kMaxRow + kThreads - 1) / kThreads;   // 182

// dims whose squared diagonal, one layer of border included, stays below DBF_INF
bool valid_diagonal(const Dims& dm) {
    unsigned long long s = 0;
    const int e[3] = {dm.d, dm.h, dm.w};
    for (int i = 0; i < 3; ++i) s += ((unsigned long long)e[i] + 1) * ((unsigned long long)e[i] + 1);
    return s < (unsigned long long)kDbfInf;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}

__global__ __launch_bounds__(kThreads) void dbf_x(const int* __restrict__ labels, int* __restrict__ out, Dims dm,
                                                 int border) {
    __shared__ int first_end[kMaxChunks + 1];   // [c]: the first run end at or after chunk c's first voxel
    __shared__ int wave_last[kThreads / 64], wave_first[kThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int w = dm.w, chunks = (w + kThreads - 1) / kThreads;
    const long long rows = (long long)dm.d * dm.h;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const int* l = labels + (size_t)row * w;
        int* o = out + (size_t)row * w;
        __syncthreads();   // the previous row's table is no longer read
        for (int c = t; c <= chunks; c += kThreads) first_end[c] = kDbfInf;
        __syncthreads();
        // sweep 1: the first run end of every chunk (p ends a run iff it is the row's last voxel or the
        // next label differs)
        for (int c = 0; c < chunks; ++c) {
            const int p = c * kThreads + t;
            int e = kDbfInf;
            if (p < w && (p == w - 1 || l[p + 1] != l[p])) e = p;
            e = wave_min(e);
            if (lane == 0 && e != kDbfInf) atomicMin(&first_end[c], e);
        }
        __syncthreads();
        if (t == 0)
            for (int c = chunks - 1; c >= 0; --c) first_end[c] = min(first_end[c], first_end[c + 1]);
        __syncthreads();
        // sweep 2: both scans per chunk, the field
        int carry_start = 0;   // the last run start before this chunk
        for (int c = 0; c < chunks; ++c) {
            const int p = c * kThreads + t;
            const bool in = p < w;
            const int me = in ? l[p] : 0;
            int a = -1, b = kDbfInf;
            if (in && (p == 0 || l[p - 1] != me)) a = p;
            if (in && (p == w - 1 || l[p + 1] != me)) b = p;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(a, d), down = __shfl_down(b, d);
                if (lane >= d) a = max(a, up);
                if (lane + d < 64) b = min(b, down);
            }
            __syncthreads();   // the previous chunk's wave values are no longer read
            if (lane == 63) wave_last[wave] = a;
            if (lane == 0) wave_first[wave] = b;
            __syncthreads();
            int last = -1;
#pragma unroll
            for (int wv = 0; wv < kThreads / 64; ++wv) {
                if (wv < wave) a = max(a, wave_last[wv]);
                if (wv > wave) b = min(b, wave_first[wv]);
                last = max(last, wave_last[wv]);
            }
            a = max(a, carry_start);
            b = min(b, first_end[c + 1]);
            carry_start = max(carry_start, last);
            if (in) {
                int f = 0;
                if (me > 0) {
                    // a run that reaches a face is bounded there only by the border layer
                    const int left = (a > 0 || border) ? p - a + 1 : 0, right = (b < w - 1 || border) ? b - p + 1 : 0;
                    const int near = left && right ? min(left, right) : left + right;
                    f = near ? near * near : kDbfInf;
                }
                o[p] = f;
            }
        }
    }
}

// One axis of length len whose neighbours are "stride" voxels apart: y (stride w) or z (stride h * w).
__global__ __launch_bounds__(kThreads) void dbf_axis(const int* __restrict__ labels, const int* __restrict__ in,
                                                    int* __restrict__ out, size_t n, int len, int stride,
                                                    int border) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += step) {
        const int me = labels[v];
        if (me <= 0) {
            out[v] = 0;
            continue;
        }
        const int p = (int)((v / (size_t)stride) % (size_t)len);
        int best = in[v];
        bool below = true, above = true;   // directions still open
        // k <= len <= 46339, so k * k fits; f + k * k stays below DBF_INF by the diagonal bound
        for (int k = 1; (below || above) && k * k < best; ++k) {
            const int k2 = k * k;
            const size_t off = (size_t)k * (size_t)stride;
            if (below) {
                if (p - k < 0) {
                    if (border) best = min(best, k2);
                    below = false;
                } else if (labels[v - off] != me) {
                    best = min(best, k2);
                    below = false;
                } else {
                    const int f = in[v - off];
                    if (f != kDbfInf) best = min(best, f + k2);
                }
            }
            if (above) {
                if (p + k >= len) {
                    if (border) best = min(best, k2);
                    above = false;
                } else if (labels[v + off] != me) {
                    best = min(best, k2);
                    above = false;
                } else {
                    const int f = in[v + off];
                    if (f != kDbfInf) best = min(best, f + k2);
                }
            }
        }
        out[v] = best;
    }
}

// ---- the table -------------------------------------------------------------------------------------
constexpr int kBoxEmptyLo = 2147483647, kBoxEmptyHi = -1;
constexpr int kPoolSlots = 512, kPoolProbes = 8;   // voxel counts a workgroup of table_pass pools in LDS

__global__ __launch_bounds__(kThreads) void table_init(unsigned long long* sizes, int* boxes,
                                                      unsigned long long* keys, size_t rows) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += step) {
        sizes[r] = 0;
        keys[r] = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            boxes[r * 6 + i] = kBoxEmptyLo;
            boxes[r * 6 + 3 + i] = kBoxEmptyHi;
        }
    }
}

// order-preserving int32 -> the key's upper word, and (dbf, index) -> key
__device__ __forceinline__ unsigned long long peak_key(int dbf, unsigned index) {
    return ((unsigned long long)((unsigned)dbf ^ 0x80000000u) << 32) | (0xFFFFFFFFu - index);
}

// a whole (never torn) load of a table entry that other workgroups update
template <typename T>
__device__ __forceinline__ T seen(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void table_pass(const int* __restrict__ labels, const int* __restrict__ dbf,
                                                      Dims dm, int n_labels, unsigned long long* sizes, int* boxes,
                                                      unsigned long long* keys) {
    __shared__ unsigned long long block_zeros;
    __shared__ int pool_label[kPoolSlots];        // -1: empty
    __shared__ unsigned pool_count[kPoolSlots];   // a workgroup sees fewer than 2^32 voxels
    const int lane = threadIdx.x & 63;
    const size_t n = (size_t)dm.n, step = (size_t)gridDim.x * kThreads;
    if (threadIdx.x == 0) block_zeros = 0;
    for (int s = threadIdx.x; s < kPoolSlots; s += kThreads) {
        pool_label[s] = -1;
        pool_count[s] = 0;
    }
    __syncthreads();
    unsigned long long zeros = 0;   // voxels labelled 0 this wave has seen: most of a neurite volume, one word
    // the trip count is the same in every lane of the workgroup: the shuffles below see all 64
    for (size_t base = (size_t)blockIdx.x * kThreads; base < n; base += step) {
        const size_t v = base + threadIdx.x;
        int l = -1, x = 0;
        unsigned long long key = 0;
        if (v < n) {
            l = labels[v];
            if ((unsigned)l > (unsigned)n_labels) l = -1;   // negative or beyond the table: never an address
            x = (int)(v % (size_t)dm.w);
            if (l > 0) key = peak_key(dbf ? dbf[v] : 0, (unsigned)v);
        }
        // row 0 has a count and nothing else: summed per wave and workgroup, one atomic at the end
        zeros += (unsigned long long)__popcll(__ballot(l == 0));
        if (l == 0) l = -1;
        // runs: equal labels in consecutive lanes of one row
        const int val = l >= 0 ? l : -1 - lane;
        const int prev = __shfl_up(val, 1);
        const bool head = lane == 0 || prev != val || x == 0;
        const unsigned long long heads = __ballot(head);
        const int mine = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // my run's first lane
        // the largest key of [lane, end of the run]
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long other = __shfl_down(key, d);
            const int theirs = __shfl_down(mine, d);
            if (lane + d < 64 && theirs == mine && other > key) key = other;
        }
        if (l >= 0 && head) {
            const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
            const int len = later ? __ffsll((long long)later) : 64 - lane;
            // the run's length into the workgroup's pool; what finds no slot within kPoolProbes goes straight out
            bool pooled = false;
            unsigned slot = (((unsigned)l * 2654435761u) >> 16) & (kPoolSlots - 1);
            for (int probe = 0; probe < kPoolProbes && !pooled; ++probe, slot = (slot + 1) & (kPoolSlots - 1)) {
                int k = *reinterpret_cast<volatile int*>(pool_label + slot);
                if (k == -1) {
                    k = atomicCAS(pool_label + slot, -1, l);
                    if (k == -1) k = l;
                }
                if (k == l) {
                    atomicAdd(pool_count + slot, (unsigned)len);
                    pooled = true;
                }
            }
            if (!pooled) atomicAdd(sizes + l, (unsigned long long)len);
            const int y = (int)((v / (size_t)dm.w) % (size_t)dm.h), z = (int)(v / ((size_t)dm.w * dm.h));
            int* box = boxes + (size_t)l * 6;
            // monotone values: a load that already covers this run's spares the atomic, whatever its age
            if (seen(box + 0) > z) atomicMin(box + 0, z);
            if (seen(box + 1) > y) atomicMin(box + 1, y);
            if (seen(box + 2) > x) atomicMin(box + 2, x);
            if (seen(box + 3) < z) atomicMax(box + 3, z);
            if (seen(box + 4) < y) atomicMax(box + 4, y);
            if (seen(box + 5) < x + len - 1) atomicMax(box + 5, x + len - 1);
            if (seen(keys + l) < key) atomicMax(keys + l, key);
        }
    }
    if (lane == 0 && zeros) atomicAdd(&block_zeros, zeros);
    __syncthreads();
    if (threadIdx.x == 0 && block_zeros) atomicAdd(sizes, block_zeros);
    for (int s = threadIdx.x; s < kPoolSlots; s += kThreads)
        if (pool_label[s] >= 0) atomicAdd(sizes + pool_label[s], (unsigned long long)pool_count[s]);
}

// keys -> peak, peak_index; inclusive box maxima -> half-open; the rows of absent labels and row 0
__global__ __launch_bounds__(kThreads) void table_finish(const unsigned long long* __restrict__ sizes,
                                                        const unsigned long long* __restrict__ keys, int* boxes,
                                                        int* peak, int* peak_index, size_t rows) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += step) {
        const bool present = r > 0 && sizes[r] != 0;
        int* box = boxes + r * 6;
        if (present) {
            const unsigned long long key = keys[r];
            box[3] += 1; box[4] += 1; box[5] += 1;
            peak[r] = (int)((unsigned)(key >> 32) ^ 0x80000000u);
            peak_index[r] = (int)(0xFFFFFFFFu - (unsigned)key);
        } else {
#pragma unroll
            for (int i = 0; i < 6; ++i) box[i] = 0;
            peak[r] = 0;
            peak_index[r] = -1;
        }
    }
}

}  // namespace

int launch_dbf_pass(int axis, const int32_t* labels, const int32_t* in, int32_t* out, const int32_t dims[3],
                    int black_border, hipStream_t s) {
    Dims dm;
    if (!valid_dims(dims, &dm) || !valid_diagonal(dm) || axis < 0 || axis > 2) return EXASPIM_E_INVALID;
    if (axis == 2)
        dbf_x<<<capped_grid((size_t)dm.d * dm.h, 1), kThreads, 0, s>>>(labels, out, dm, black_border);
    else if (axis == 1)
        dbf_axis<<<capped_grid((size_t)dm.n, kThreads), kThreads, 0, s>>>(labels, in, out, (size_t)dm.n, dm.h, dm.w,
                                                                          black_border);
    else
        dbf_axis<<<capped_grid((size_t)dm.n, kThreads), kThreads, 0, s>>>(labels, in, out, (size_t)dm.n, dm.d,
                                                                          dm.h * dm.w, black_border);
    return EXASPIM_OK;
}

}  // namespace exaspim

using namespace exaspim;

namespace {
const char* const kDimsMessage =
    "dims must be positive with a product of at most 2^31 - 1 and (D+1)^2 + (H+1)^2 + (W+1)^2 below 2^31 - 1";
}

extern "C" size_t exaspim_dbf_workspace_bytes(const int32_t dims[3]) {
    Dims dm;
    if (!valid_dims(dims, &dm) || !valid_diagonal(dm)) {
        set_error("dbf_workspace_bytes: %s", kDimsMessage);
        return 0;
    }
    return align_up((size_t)dm.n * sizeof(int32_t), 16);
}

extern "C" int exaspim_dbf(const int32_t* labels_dev, const int32_t dims[3], int32_t black_border,
                           int32_t* dbf_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && dims && dbf_dev && workspace_dev, "dbf: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(valid_dims(dims, &dm) && valid_diagonal(dm), "dbf: %s", kDimsMessage);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && ((uintptr_t)labels_dev & 3) == 0 &&
                      ((uintptr_t)dbf_dev & 3) == 0,
                  "dbf: misaligned buffer");
    const size_t need = align_up((size_t)dm.n * sizeof(int32_t), 16);
    if (workspace_bytes < need) {
        set_error("dbf: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    int32_t* mid = static_cast<int32_t*>(workspace_dev);
    const int border = black_border != 0;
    launch_dbf_pass(2, labels_dev, nullptr, dbf_dev, dims, border, s);
    launch_dbf_pass(1, labels_dev, dbf_dev, mid, dims, border, s);
    launch_dbf_pass(0, labels_dev, mid, dbf_dev, dims, border, s);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" size_t exaspim_segment_table_workspace_bytes(int32_t n_labels) {
    if (n_labels < 0) {
        set_error("segment_table_workspace_bytes: n_labels must not be negative, got %d", n_labels);
        return 0;
    }
    return align_up(((size_t)n_labels + 1) * sizeof(unsigned long long), 16);
}

extern "C" int exaspim_segment_table(const int32_t* labels_dev, const int32_t* dbf_dev, const int32_t dims[3],
                                     int32_t n_labels, int64_t* sizes_dev, int32_t* boxes_dev, int32_t* peak_dev,
                                     int32_t* peak_index_dev, void* workspace_dev, size_t workspace_bytes,
                                     void* stream) {
    EXA_CHECK_ARG(labels_dev && dims && sizes_dev && boxes_dev && peak_dev && peak_index_dev && workspace_dev,
                  "segment_table: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(valid_dims(dims, &dm) && valid_diagonal(dm), "segment_table: %s", kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "segment_table: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && ((uintptr_t)sizes_dev & 7) == 0 &&
                      (((uintptr_t)labels_dev | (uintptr_t)dbf_dev | (uintptr_t)boxes_dev | (uintptr_t)peak_dev |
                        (uintptr_t)peak_index_dev) & 3) == 0,
                  "segment_table: misaligned buffer");
    const size_t rows = (size_t)n_labels + 1;
    const size_t need = align_up(rows * sizeof(unsigned long long), 16);
    if (workspace_bytes < need) {
        set_error("segment_table: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* sizes = reinterpret_cast<unsigned long long*>(sizes_dev);
    unsigned long long* keys = static_cast<unsigned long long*>(workspace_dev);
    table_init<<<capped_grid(rows, kThreads), kThreads, 0, s>>>(sizes, boxes_dev, keys, rows);
    // a few workgroups per CU that stride over the volume: the voxels labelled 0 cost one atomic per workgroup
    const unsigned table_grid = std::min(capped_grid((size_t)dm.n, kThreads), 4096u);
    table_pass<<<table_grid, kThreads, 0, s>>>(labels_dev, dbf_dev, dm, n_labels, sizes, boxes_dev, keys);
    table_finish<<<capped_grid(rows, kThreads), kThreads, 0, s>>>(sizes, keys, boxes_dev, peak_dev, peak_index_dev,
                                                                  rows);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}
