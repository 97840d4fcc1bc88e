// What the label kernels of components.hip and region_graph.hip share: the tile of the LDS passes, the
// launch geometry, the three-pass prefix sum over a predicate and a sink, and the table look-up.
// Kernels in a header: every file that includes it gets its own copies (anonymous namespace).
#pragma once

#include "common.h"

namespace exaspim {
namespace {

constexpr int kTZ = 8, kTY = 8, kTX = 32;            // tile of the LDS pass (z, y, x)
constexpr int kTileVox = kTZ * kTY * kTX;            // 2048
constexpr int kThreads = 256;
constexpr int kPerThread = kTileVox / kThreads;      // 8
constexpr int kScanBlock = 2048;                     // voxels per block of the prefix sum
constexpr int kScanRounds = kScanBlock / kThreads;   // 8
constexpr int kSumThreads = 1024, kSumPerThread = 4; // the middle pass of the scan

struct Dims {
    int d, h, w;
    int n;   // d * h * w <= 2^31 - 1
};

bool valid_dims(const int32_t dims[3], Dims* dm) {
    if (!dims) return false;
    long long n = 1;
    for (int i = 0; i < 3; ++i) {
        if (dims[i] <= 0) return false;
        n *= dims[i];
        if (n > 2147483647ll) return false;
    }
    *dm = Dims{dims[0], dims[1], dims[2], (int)n};
    return true;
}

__host__ __device__ inline unsigned capped_grid(size_t items, unsigned per_block) {
    const size_t blocks = (items + per_block - 1) / per_block;
    return (unsigned)(blocks < 65536 ? (blocks ? blocks : 1) : 65536);
}

template <typename T>
__device__ __forceinline__ float widen(T v);
template <>
__device__ __forceinline__ float widen<float>(float v) { return v; }
template <>
__device__ __forceinline__ float widen<_Float16>(_Float16 v) { return (float)v; }

// ---- the three-pass prefix sum -----------------------------------------------------------------
// scan_count and scan_assign run one workgroup per block of kScanBlock items: n <= 2^31 - 1 gives
// at most 2^20 of them, which one launch holds. PRED(v) says whether item v is numbered, SINK(v,
// flag, rank) takes its 0-based rank among the numbered ones; the whole-volume call, the streamed
// slabs, the streamed table and the region graph's edge list share the three passes and differ in
// these two.

// exclusive prefix of "flag" over the block's threads, and the block's total
__device__ __forceinline__ int block_exclusive(bool flag, int* wave_sums, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long ball = __ballot(flag);
    const int below = __popcll(ball & ((1ull << lane) - 1ull));
    __syncthreads();   // wave_sums may still be read from the previous round
    if (lane == 0) wave_sums[wave] = __popcll(ball);
    __syncthreads();
    int before = 0, sum = 0;
    for (int wv = 0; wv < kThreads / 64; ++wv) {
        const int s = wave_sums[wv];
        if (wv < wave) before += s;
        sum += s;
    }
    *total = sum;
    return before + below;
}

template <typename PRED>
__global__ __launch_bounds__(kThreads) void scan_count(PRED pred, int* __restrict__ block_sums, size_t n) {
    __shared__ int wave_sums[kThreads / 64];
    const size_t b = blockIdx.x;
    int count = 0;
    for (int r = 0; r < kScanRounds; ++r) {
        const size_t v = b * kScanBlock + r * kThreads + threadIdx.x;
        const bool flag = v < n && pred(v);
        int total;
        block_exclusive(flag, wave_sums, &total);
        count += total;
    }
    if (threadIdx.x == 0) block_sums[b] = count;
}

// one workgroup: block_sums -> exclusive prefix in place, total -> *n_segments
__global__ __launch_bounds__(kSumThreads) void scan_block_sums(int* block_sums, long long n_blocks,
                                                              int* n_segments) {
    __shared__ int wave_sums[kSumThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (long long base = 0; base < n_blocks; base += kSumThreads * kSumPerThread) {
        const long long first = base + (long long)threadIdx.x * kSumPerThread;
        int v[kSumPerThread], mine = 0;
#pragma unroll
        for (int k = 0; k < kSumPerThread; ++k) {
            v[k] = first + k < n_blocks ? block_sums[first + k] : 0;
            mine += v[k];
        }
        int incl = mine;   // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        __syncthreads();
        if (lane == 63) wave_sums[wave] = incl;
        __syncthreads();
        int before = carry, sum = 0;
        for (int wv = 0; wv < kSumThreads / 64; ++wv) {
            const int s = wave_sums[wv];
            if (wv < wave) before += s;
            sum += s;
        }
        int run = before + incl - mine;
#pragma unroll
        for (int k = 0; k < kSumPerThread; ++k) {
            if (first + k < n_blocks) block_sums[first + k] = run;
            run += v[k];
        }
        carry += sum;
    }
    if (threadIdx.x == 0) *n_segments = carry;
}

template <typename PRED>
__global__ __launch_bounds__(kThreads) void scan_assign(PRED pred, const int* __restrict__ block_sums, size_t n) {
    __shared__ int wave_sums[kThreads / 64];
    const size_t b = blockIdx.x;
    int offset = block_sums[b];
    for (int r = 0; r < kScanRounds; ++r) {
        const size_t v = b * kScanBlock + r * kThreads + threadIdx.x;
        const bool flag = v < n && pred(v);
        int total;
        const int rank = block_exclusive(flag, wave_sums, &total);
        if (v < n) pred(v, flag, offset + rank);
        offset += total;
    }
}

// ---- the table look-up -------------------------------------------------------------------------
// labels[v] = table[labels[v]] in place, four voxels per thread where the pointer allows; a value
// that is no id (negative, beyond the capacity) becomes 0 instead of an index
__global__ __launch_bounds__(kThreads) void apply_table(int* labels, const int* __restrict__ table, int capacity,
                                                       size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    auto map = [&](int id) { return (unsigned)id <= (unsigned)capacity ? table[id] : 0; };
    const size_t quads = ((uintptr_t)labels & 15) == 0 ? n / 4 : 0;
    int4* l4 = reinterpret_cast<int4*>(labels);
    for (size_t g = first; g < quads; g += stride) {
        int4 v = l4[g];
        v.x = map(v.x); v.y = map(v.y); v.z = map(v.z); v.w = map(v.w);
        l4[g] = v;
    }
    for (size_t g = quads * 4 + first; g < n; g += stride) labels[g] = map(labels[g]);
}

}  // namespace
}  // namespace exaspim
