// Connected components of thresholded affinities on the device, with the reference's small-segment
// filter and contiguous renumbering (exaspim_components; semantics in include/exaspim_affinity.h).
//
// A block-based union-find. parent[] lives in the caller's label array; the invariant everywhere is
// parent[v] <= v, so a chain of parents strictly decreases and ends in a fixed point (a root), and
// links are only ever made with atomicMin on the larger of two roots: the root of a finished set is
// its smallest linear index, whatever order the atomics landed in. Passes, each a launch of its own
// on the caller's stream (no grid-wide barrier, no workgroup ever waits for another one):
//   (a) edge_mask_*   affinities -> one byte per voxel: bit 0/1/2 = edge to z+1 / y+1 / x+1 is on,
//                     bit 3 = the voxel itself can belong to a segment (12 or 6 B/voxel read once);
//   (b) tile_pass     8 x 8 x 32 tiles merged in LDS, parent[v] = global index of the tile-local root;
//   (c) face_merge    unions across tile faces in global memory;
//   (d) flatten       parent[v] = root(v);
//   (e) sizes         aux[root] += 1 per non-root voxel, one atomic per run of equal roots in a wave;
//   (f) scan_*        a flag per kept root and a three-pass exclusive prefix sum over the flags;
//   (g) relabel       labels[v] = new id of root(v), in place.
// Every retry loop is a lock-free union whose larger root strictly decreases per iteration; a stale
// read of parent[] only yields an older ancestor of the same set, and the value atomicMin returns
// decides, so no loop depends on when another workgroup's stores become visible.
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

constexpr unsigned kBitZ = 1, kBitY = 2, kBitX = 4, kBitOn = 8;

struct Dims {
    int d, h, w;
    int n;   // d * h * w <= 2^31 - 1
};

__host__ __device__ inline unsigned capped_grid(size_t items, unsigned per_block) {
    const size_t blocks = (items + per_block - 1) / per_block;
    return (unsigned)(blocks < 65536 ? (blocks ? blocks : 1) : 65536);
}

// ---- (a) edge mask ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ float widen(T v);
template <>
__device__ __forceinline__ float widen<float>(float v) { return v; }
template <>
__device__ __forceinline__ float widen<_Float16>(_Float16 v) { return (float)v; }

// VEC voxels along x per thread (VEC * sizeof(T) = 16 bytes, or VEC = 1); w % VEC == 0, so a group
// never straddles a row and every channel base stays 16-byte aligned.
template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void edge_mask_affinity(const T* __restrict__ aff,
                                                              unsigned char* __restrict__ mask, Dims dm,
                                                              float thr) {
    struct alignas(sizeof(T) * VEC) Pack { T v[VEC]; };
    struct alignas(VEC) Bytes { unsigned char b[VEC]; };
    const size_t groups = (size_t)dm.n / VEC;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const unsigned i = (unsigned)(g * VEC);
        const unsigned row = i / (unsigned)dm.w, x0 = i - row * (unsigned)dm.w;
        const unsigned z = row / (unsigned)dm.h, y = row - z * (unsigned)dm.h;
        const Pack az = *reinterpret_cast<const Pack*>(aff + i);
        const Pack ay = *reinterpret_cast<const Pack*>(aff + (size_t)dm.n + i);
        const Pack ax = *reinterpret_cast<const Pack*>(aff + 2 * (size_t)dm.n + i);
        const bool zin = (int)z < dm.d - 1, yin = (int)y < dm.h - 1;
        Bytes out;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            unsigned m = kBitOn;
            if (zin && widen<T>(az.v[k]) >= thr) m |= kBitZ;
            if (yin && widen<T>(ay.v[k]) >= thr) m |= kBitY;
            if ((int)(x0 + k) < dm.w - 1 && widen<T>(ax.v[k]) >= thr) m |= kBitX;
            out.b[k] = (unsigned char)m;
        }
        *reinterpret_cast<Bytes*>(mask + i) = out;
    }
}

// foreground mode: a voxel is on iff p >= thr, an edge iff both of its ends are
template <typename T>
__global__ __launch_bounds__(kThreads) void edge_mask_foreground(const T* __restrict__ p,
                                                                unsigned char* __restrict__ mask, Dims dm,
                                                                float thr) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const unsigned hw = (unsigned)dm.h * (unsigned)dm.w;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < (size_t)dm.n; g += stride) {
        const unsigned i = (unsigned)g;
        const unsigned row = i / (unsigned)dm.w, x = i - row * (unsigned)dm.w;
        const unsigned z = row / (unsigned)dm.h, y = row - z * (unsigned)dm.h;
        unsigned m = 0;
        if (widen<T>(p[i]) >= thr) {
            m = kBitOn;
            if ((int)z < dm.d - 1 && widen<T>(p[i + hw]) >= thr) m |= kBitZ;
            if ((int)y < dm.h - 1 && widen<T>(p[i + dm.w]) >= thr) m |= kBitY;
            if ((int)x < dm.w - 1 && widen<T>(p[i + 1]) >= thr) m |= kBitX;
        }
        mask[i] = (unsigned char)m;
    }
}

// ---- the lock-free union --------------------------------------------------------------------
// LOAD(p, i) reads p[i] in a way that is not cached in a register across iterations.
struct LdsLoad {
    __device__ __forceinline__ int operator()(const int* p, int i) const {
        return *reinterpret_cast<const volatile int*>(p + i);
    }
};
struct GlobalLoad {
    __device__ __forceinline__ int operator()(const int* p, int i) const {
        return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

template <typename LOAD>
__device__ __forceinline__ int find_root(const int* parent, int v) {
    LOAD load;
    for (int p = load(parent, v); p != v; p = load(parent, v)) v = p;
    return v;
}

// Each iteration either returns or replaces the larger of the two roots by a smaller index.
template <typename LOAD>
__device__ __forceinline__ void unite(int* parent, int a, int b) {
    for (;;) {
        a = find_root<LOAD>(parent, a);
        b = find_root<LOAD>(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + b, a);
        if (old == b) return;   // b was a root and now hangs under a
        b = old;                // b had been linked meanwhile: go on with what it pointed to
    }
}

// ---- (b) tile pass ---------------------------------------------------------------------------
// Local index i = (lz * 8 + ly) * 32 + lx orders a tile's voxels like their global linear indices,
// so the smallest local index of a set is its smallest global one too.
__global__ __launch_bounds__(kThreads) void tile_pass(const unsigned char* __restrict__ mask,
                                                     int* __restrict__ parent, Dims dm, int tiles_x,
                                                     int tiles_y, long long n_tiles) {
    __shared__ int lp[kTileVox];
    const int t = threadIdx.x, lane = t & 63, lx = t & 31;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tx = (int)(tile % tiles_x), ty = (int)((tile / tiles_x) % tiles_y);
        const int tz = (int)(tile / ((long long)tiles_x * tiles_y));
        const int x = tx * kTX + lx;
        unsigned bits[kPerThread];
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int i = t + kThreads * k;
            const int ly = (i >> 5) & (kTY - 1), lz = i >> 8;
            const int y = ty * kTY + ly, z = tz * kTZ + lz;
            unsigned m = 0;
            if (x < dm.w && y < dm.h && z < dm.d) m = mask[((size_t)z * dm.h + y) * dm.w + x];
            // edges that leave the tile are face_merge's
            if (lx == kTX - 1) m &= ~kBitX;
            if (ly == kTY - 1) m &= ~kBitY;
            if (lz == kTZ - 1) m &= ~kBitZ;
            bits[k] = m;
            // a row of 32 voxels is half a wave: start of this voxel's run of on x edges
            const unsigned long long ball = __ballot((m & kBitX) != 0);
            const unsigned rowbits = (unsigned)(ball >> (lane & 32));
            const unsigned off_below = ~rowbits & ((1u << lx) - 1u);
            const int start = off_below ? 32 - __clz((int)off_below) : 0;
            lp[i] = (i & ~31) + start;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int i = t + kThreads * k;
            if (bits[k] & kBitY) unite<LdsLoad>(lp, i, i + kTX);
            if (bits[k] & kBitZ) unite<LdsLoad>(lp, i, i + kTX * kTY);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int i = t + kThreads * k;
            const int y = ty * kTY + ((i >> 5) & (kTY - 1)), z = tz * kTZ + (i >> 8);
            if (x < dm.w && y < dm.h && z < dm.d) {
                const int r = find_root<LdsLoad>(lp, i);
                const int rz = tz * kTZ + (r >> 8), ry = ty * kTY + ((r >> 5) & (kTY - 1));
                const int rx = tx * kTX + (r & 31);
                parent[((size_t)z * dm.h + y) * dm.w + x] = (int)(((size_t)rz * dm.h + ry) * dm.w + rx);
            }
        }
        __syncthreads();   // lp is reused by the next tile
    }
}

// ---- (c) face merge --------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void face_merge(const unsigned char* __restrict__ mask, int* parent,
                                                      Dims dm) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const unsigned hw = (unsigned)dm.h * (unsigned)dm.w;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < (size_t)dm.n; g += stride) {
        const unsigned m = mask[g];
        if (!(m & (kBitX | kBitY | kBitZ))) continue;
        const unsigned i = (unsigned)g;
        const unsigned row = i / (unsigned)dm.w, x = i - row * (unsigned)dm.w;
        const unsigned z = row / (unsigned)dm.h, y = row - z * (unsigned)dm.h;
        // the mask holds no edge that leaves the volume, so i + 1, i + w, i + hw are voxels
        if ((m & kBitX) && (x & (kTX - 1)) == kTX - 1) unite<GlobalLoad>(parent, (int)i, (int)(i + 1));
        if ((m & kBitY) && (y & (kTY - 1)) == kTY - 1) unite<GlobalLoad>(parent, (int)i, (int)(i + dm.w));
        if ((m & kBitZ) && (z & (kTZ - 1)) == kTZ - 1) unite<GlobalLoad>(parent, (int)i, (int)(i + hw));
    }
}

// ---- (d) flatten -----------------------------------------------------------------------------
// No union runs here, so roots are fixed; a concurrent store of another thread only replaces a
// parent by the root of the same chain.
__global__ __launch_bounds__(kThreads) void flatten(int* parent, int n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < (size_t)n; g += stride) {
        const int v = (int)g;
        const int p = parent[v];
        if (p == v) continue;
        const int r = find_root<GlobalLoad>(parent, p);
        if (r != p) parent[v] = r;
    }
}

// ---- (e) sizes -------------------------------------------------------------------------------
// aux[r] = number of voxels other than r whose root is r (aux zeroed before). Lanes of a wave hold
// consecutive voxels: a run of lanes with the same root adds once, from its first lane. Integer
// adds: the sums do not depend on their order.
__global__ __launch_bounds__(kThreads) void sizes(const int* __restrict__ parent, int* aux, int n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    const size_t rounds = ((size_t)n + stride - 1) / stride;   // whole waves stay in the loop together
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t it = 0; it < rounds; ++it, g += stride) {
        const bool in = g < (size_t)n;
        const int root = in ? parent[g] : -1 - lane;     // out-of-range lanes: distinct, never added
        const int prev = __shfl_up(root, 1);
        const bool head = lane == 0 || prev != root;
        const unsigned long long heads = __ballot(head);
        if (in && head) {
            const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
            const int len = above ? __ffsll((long long)above) : 64 - lane;
            const int add = len - (root == (int)g ? 1 : 0);
            if (add > 0) atomicAdd(aux + root, add);
        }
    }
}

// ---- (f) renumbering -------------------------------------------------------------------------
// scan_count and scan_assign run one workgroup per block of kScanBlock voxels: n <= 2^31 - 1 gives
// at most 2^20 of them, which one launch holds.
__device__ __forceinline__ bool kept_root(const int* parent, const unsigned char* mask, const int* aux,
                                          size_t v, int min_size) {
    return parent[v] == (int)v && (mask[v] & kBitOn) && aux[v] >= min_size;   // size = aux + 1 > min_size
}

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

__global__ __launch_bounds__(kThreads) void scan_count(const int* __restrict__ parent,
                                                      const unsigned char* __restrict__ mask,
                                                      const int* __restrict__ aux, int* __restrict__ block_sums,
                                                      int n, int min_size) {
    __shared__ int wave_sums[kThreads / 64];
    const size_t b = blockIdx.x;
    int count = 0;
    for (int r = 0; r < kScanRounds; ++r) {
        const size_t v = b * kScanBlock + r * kThreads + threadIdx.x;
        const bool flag = v < (size_t)n && kept_root(parent, mask, aux, v, min_size);
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

// aux[v] = new id (1 ...) of a kept root, 0 for everything else
__global__ __launch_bounds__(kThreads) void scan_assign(const int* __restrict__ parent,
                                                       const unsigned char* __restrict__ mask, int* aux,
                                                       const int* __restrict__ block_sums, int n, int min_size) {
    __shared__ int wave_sums[kThreads / 64];
    const size_t b = blockIdx.x;
    int offset = block_sums[b];
    for (int r = 0; r < kScanRounds; ++r) {
        const size_t v = b * kScanBlock + r * kThreads + threadIdx.x;
        const bool flag = v < (size_t)n && kept_root(parent, mask, aux, v, min_size);
        int total;
        const int rank = block_exclusive(flag, wave_sums, &total);
        if (v < (size_t)n) aux[v] = flag ? offset + rank + 1 : 0;
        offset += total;
    }
}

// ---- (g) relabel -----------------------------------------------------------------------------
// labels is the flattened parent array: a thread reads only its own entry of it before writing it.
__global__ __launch_bounds__(kThreads) void relabel(int* labels, const int* __restrict__ aux, int n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < (size_t)n; g += stride)
        labels[g] = aux[labels[g]];
}

// ---- workspace -------------------------------------------------------------------------------
struct Layout {
    size_t aux_off, mask_off, sums_off, bytes;
    long long n_scan_blocks;
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

Layout layout_of(const Dims& dm) {
    Layout l;
    l.n_scan_blocks = ((long long)dm.n + kScanBlock - 1) / kScanBlock;
    l.aux_off = 0;
    l.mask_off = align_up((size_t)dm.n * 4, 256);
    l.sums_off = l.mask_off + align_up((size_t)dm.n, 256);
    l.bytes = l.sums_off + align_up((size_t)l.n_scan_blocks * 4, 256);
    return l;
}

template <typename T>
void launch_edge_mask(const void* src, int channels, unsigned char* mask, const Dims& dm, float thr,
                      hipStream_t stream) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const T* p = static_cast<const T*>(src);
    if (channels == 1) {
        edge_mask_foreground<T><<<capped_grid((size_t)dm.n, kThreads), kThreads, 0, stream>>>(p, mask, dm, thr);
    } else if (dm.w % VEC == 0 && ((uintptr_t)src & 15) == 0) {
        edge_mask_affinity<T, VEC><<<capped_grid((size_t)dm.n / VEC, kThreads), kThreads, 0, stream>>>(p, mask, dm, thr);
    } else {
        edge_mask_affinity<T, 1><<<capped_grid((size_t)dm.n, kThreads), kThreads, 0, stream>>>(p, mask, dm, thr);
    }
}

}  // namespace
}  // namespace exaspim

using namespace exaspim;

extern "C" size_t exaspim_components_workspace_bytes(const int32_t dims[3]) {
    Dims dm;
    if (!valid_dims(dims, &dm)) {
        set_error("components_workspace_bytes: dims must be positive with a product of at most 2^31 - 1");
        return 0;
    }
    return layout_of(dm).bytes;
}

extern "C" int exaspim_components(const void* aff_dev, int32_t aff_dtype, int32_t channels,
                                  const int32_t dims[3], float threshold, int64_t min_size,
                                  int32_t* labels_dev, int32_t* n_segments_dev, void* workspace_dev,
                                  size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(aff_dev && labels_dev && n_segments_dev && workspace_dev && dims, "components: NULL argument");
    EXA_CHECK_ARG(aff_dtype == EXASPIM_AFF_F32 || aff_dtype == EXASPIM_AFF_F16,
                  "components: aff_dtype %d is neither EXASPIM_AFF_F32 nor EXASPIM_AFF_F16", aff_dtype);
    EXA_CHECK_ARG(channels == 3 || channels == 1, "components: channels must be 3 or 1, got %d", channels);
    Dims dm;
    EXA_CHECK_ARG(valid_dims(dims, &dm),
                  "components: dims must be positive with a product of at most 2^31 - 1");
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && ((uintptr_t)labels_dev & 3) == 0 &&
                      ((uintptr_t)aff_dev & (aff_dtype == EXASPIM_AFF_F32 ? 3 : 1)) == 0,
                  "components: misaligned buffer");
    const Layout l = layout_of(dm);
    if (workspace_bytes < l.bytes) {
        set_error("components: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
        return EXASPIM_E_WORKSPACE;
    }
    // a one-voxel segment has no affinity (img_util.get_affinity_channels): in affinity mode it is
    // background whatever min_size says; in foreground mode an on voxel alone is a segment of size 1
    const int64_t floor_size = channels == 3 ? 1 : 0;
    const int64_t ms = min_size < floor_size ? floor_size : min_size;
    const int min_eff = ms > 2147483647ll ? 2147483647 : (int)ms;

    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace_dev);
    int* aux = reinterpret_cast<int*>(ws + l.aux_off);
    unsigned char* mask = reinterpret_cast<unsigned char*>(ws + l.mask_off);
    int* sums = reinterpret_cast<int*>(ws + l.sums_off);
    int* parent = labels_dev;

    EXA_CHECK_HIP(hipMemsetAsync(aux, 0, (size_t)dm.n * 4, s));
    if (aff_dtype == EXASPIM_AFF_F32)
        launch_edge_mask<float>(aff_dev, channels, mask, dm, threshold, s);
    else
        launch_edge_mask<_Float16>(aff_dev, channels, mask, dm, threshold, s);
    const int tiles_x = (dm.w + kTX - 1) / kTX, tiles_y = (dm.h + kTY - 1) / kTY;
    const long long n_tiles = (long long)tiles_x * tiles_y * ((dm.d + kTZ - 1) / kTZ);
    tile_pass<<<capped_grid((size_t)n_tiles, 1), kThreads, 0, s>>>(mask, parent, dm, tiles_x, tiles_y, n_tiles);
    const unsigned grid = capped_grid((size_t)dm.n, kThreads);
    face_merge<<<grid, kThreads, 0, s>>>(mask, parent, dm);
    flatten<<<grid, kThreads, 0, s>>>(parent, dm.n);
    sizes<<<grid, kThreads, 0, s>>>(parent, aux, dm.n);
    const unsigned scan_grid = (unsigned)l.n_scan_blocks;
    scan_count<<<scan_grid, kThreads, 0, s>>>(parent, mask, aux, sums, dm.n, min_eff);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(sums, l.n_scan_blocks, n_segments_dev);
    scan_assign<<<scan_grid, kThreads, 0, s>>>(parent, mask, aux, sums, dm.n, min_eff);
    relabel<<<grid, kThreads, 0, s>>>(parent, aux, dm.n);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}
