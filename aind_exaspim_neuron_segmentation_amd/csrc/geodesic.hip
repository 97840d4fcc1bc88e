// The geodesic distance-from-source field of every label at once (exaspim_geodesic_begin, _sweeps,
// _farthest; semantics in include/exaspim_affinity.h). DESIGN 6l. A label-correcting relaxation over the
// 8 x 8 x 32 tiles of label_scan.h: float32 additions and minima only, so the least fixed point it stops
// at is, bit for bit, what a serial float32 Dijkstra returns, whatever the order of relaxation.
//
//   geodesic_init     field = +inf on foreground, 0 on background; both flag arrays and the header cleared.
//   geodesic_sources  one thread per row of sources: a valid row zeroes its voxel and flags the voxel's
//                     tile and the tiles that see the voxel in their halo for the first sweep, an invalid
//                     one is counted.
//   geodesic_sweep    one workgroup per tile (grid capped, stride). A tile whose flag is clear returns. An
//                     active tile clears its flag, loads labels and field with a one-voxel halo into LDS
//                     (10 x 10 x 34 x 8 bytes), and relaxes there until no voxel of the tile changes, at
//                     most kTileVox + 1 rounds (Bellman-Ford's bound: a shortest path inside the tile has
//                     at most kTileVox edges, and round k makes every voxel final whose path has k). A
//                     thread owns a z column of eight voxels; a half-wave reads 32 consecutive words of a
//                     row, which the 32 banks of ds_read_b32 serve without a conflict whatever the row
//                     stride. The 26 same-label tests are taken once, into a bit mask that replaces the
//                     voxel's label word in LDS. Then the voxels that fell are stored, and if one of them
//                     lies on the tile's outer layer the tiles that see it in their halo -- faces, edges
//                     and corners -- are flagged for the NEXT sweep, in the other flag array.
//   geodesic_publish  one thread: the count of tiles flagged for the next sweep and the invalid rows go
//                     to state[], the arrays swap.
// No workgroup waits for another. Within a sweep a tile may read a neighbour's voxel before or after the
// neighbour stores it: aligned 4-byte accesses do not tear, both values are sums along a real path and so
// upper bounds of the answer, and the writer flags the reader for the next sweep in either case.
//   far_init, far_pass, far_finish  the farthest table: a 64-bit atomic maximum of (field bits,
//                     2^32 - 1 - index) per label over the finite voxels, runs of equal labels reduced
//                     inside a wave first, as dbf.hip's table does.
//
// The parental field of a converged field and the paths read off it (exaspim_geodesic_parents_begin,
// _sweeps, _finish, exaspim_trace_paths). An edge u -> v is tight iff fl32(d[u] + w(u -> v)) has
// the bits of d[v]; hops is the breadth-first distance from the source over tight edges, an integer least
// fixed point; the parent is the tight predecessor with one hop less and the smallest index.
//   hops_init         hops = -1 everywhere; both flag arrays and the header cleared.
//   hops_seed         one thread per row of sources: a valid row whose field word is +0.0 gets hops 0 and
//                     flags as geodesic_sources does, any other row that is not -1 is counted.
//   hops_sweep        geodesic_sweep's shape over the same two LDS arrays: the 26 tight tests are taken once
//                     into the mask that replaces the label word, then hops (halo included) replaces the
//                     field and is relaxed in unsigned arithmetic, where -1 is the largest value.
//   parents_pick      one thread per voxel, global memory only: the parent, and the orphans (finite field, no
//                     source, no tight predecessor) counted with one atomic per wave.
//   trace_paths       one thread per target: at most hops[target] steps along parents, written back to front.
//
// Fields and hops seeded from a list (exaspim_geodesic_reseed, exaspim_geodesic_parents_begin_seeds; DESIGN
// 6o): any number of seeds per label, duplicates allowed. Zeroing a converged field at further seeds and
// sweeping again gives the field of all seeds, bit for bit: every old value is a sum along a real path from a
// voxel that is still a seed, so an upper bound, and the relaxation stops only where no edge can lower one.
//   reseed_clear      both flag arrays and the header cleared; the field is left as it is.
//   reseed_seeds      a grid-stride thread per seed: a valid seed (in the volume, its label in 1..K) gets +0.0 and
//                     flags as geodesic_sources does, an invalid one is counted and writes nothing. Two seeds of
//                     one voxel store the same word.
//   hops_seed_list    hops_seed over the list: a valid seed whose field word is +0.0 gets hops 0.
#include "label_scan.h"

namespace exaspim {
namespace {

constexpr int kHZ = kTZ + 2, kHY = kTY + 2, kHX = kTX + 2;   // the tile with its halo
constexpr int kHaloVox = kHZ * kHY * kHX;                    // 3400
constexpr unsigned kInfBits = 0x7F800000u;
constexpr unsigned kSqrt2Bits = 0x3FB504F3u, kSqrt3Bits = 0x3FDDB3D7u;   // fl32(sqrt 2), fl32(sqrt 3)

// the head of the workspace; the two flag arrays follow
struct Header {
    int parity;      // flags + parity * tiles is read by the next sweep, the other array written
    int count[2];    // tiles flagged in either array
    int invalid;     // source rows that name no voxel of their label
};

struct Tiles {
    int nz, ny, nx;
    long long n;
};

Tiles tiles_of(const Dims& dm) {
    Tiles t;
    t.nz = (dm.d + kTZ - 1) / kTZ;
    t.ny = (dm.h + kTY - 1) / kTY;
    t.nx = (dm.w + kTX - 1) / kTX;
    t.n = (long long)t.nz * t.ny * t.nx;   // at most 2^31 / 8
    return t;
}

size_t workspace_need(const Dims& dm) {
    return align_up(sizeof(Header), 16) + align_up(2 * (size_t)tiles_of(dm).n * sizeof(int), 16);
}

__device__ __forceinline__ void flag_tile(int* flags, int* count, long long tile) {
    if (atomicExch(flags + tile, 1) == 0) atomicAdd(count, 1);
}

__global__ __launch_bounds__(kThreads) void geodesic_init(const int* __restrict__ labels, float* __restrict__ field,
                                                         size_t n, Header* hdr, int* flags, size_t n_flags) {
    const size_t step = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (first == 0) *hdr = Header{0, {0, 0}, 0};
    for (size_t i = first; i < n_flags; i += step) flags[i] = 0;
    for (size_t v = first; v < n; v += step) field[v] = __uint_as_float(labels[v] > 0 ? kInfBits : 0u);
}

__global__ __launch_bounds__(kThreads) void geodesic_sources(const int* __restrict__ labels,
                                                            const int* __restrict__ sources, int n_labels,
                                                            float* field, Dims dm, Tiles tl, Header* hdr,
                                                            int* flags) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x + 1; r <= (size_t)n_labels; r += step) {
        const int s = sources[r];
        if (s == -1) continue;
        if (s < 0 || s >= dm.n || labels[s] != (int)r) {
            atomicAdd(&hdr->invalid, 1);
            continue;
        }
        field[s] = 0.0f;
        const int x = s % dm.w, y = (s / dm.w) % dm.h, z = s / (dm.w * dm.h);
        // the source's tile and, where the source lies on its outer layer, the tiles that see it in their
        // halo: the source itself never falls in a sweep, so nobody else would flag them
        for (int tz = (z - 1) / kTZ; tz <= (z + 1) / kTZ; ++tz)
            for (int ty = (y - 1) / kTY; ty <= (y + 1) / kTY; ++ty)
                for (int tx = (x - 1) / kTX; tx <= (x + 1) / kTX; ++tx)
                    if (tz < tl.nz && ty < tl.ny && tx < tl.nx)
                        flag_tile(flags, &hdr->count[0], ((long long)tz * tl.ny + ty) * tl.nx + tx);
    }
}

__global__ void geodesic_publish(Header* hdr, int* state, int swap) {
    int p = hdr->parity;
    if (swap) {
        hdr->count[p] = 0;   // every tile flagged there has run and cleared its flag
        p ^= 1;
        hdr->parity = p;
    }
    state[0] = hdr->count[p];
    state[1] = hdr->invalid;
}

__device__ __forceinline__ float fmin2(float a, float b) { return a < b ? a : b; }

template <bool COST>
__global__ __launch_bounds__(kThreads) void geodesic_sweep(const int* __restrict__ labels,
                                                          const float* __restrict__ cost, float* field, Dims dm,
                                                          Tiles tl, int n_labels, Header* hdr, int* flags) {
    __shared__ float f[kHaloVox];
    __shared__ int lab[kHaloVox];
    __shared__ unsigned reach;   // bit (dz + 1) * 9 + (dy + 1) * 3 + dx + 1: that neighbouring tile sees a fallen voxel
    const int parity = hdr->parity;
    if (hdr->count[parity] == 0) return;   // converged: the remaining sweeps of a call are empty
    int* const current = flags + (size_t)parity * tl.n;
    int* const next = flags + (size_t)(parity ^ 1) * tl.n;
    int* const next_count = &hdr->count[parity ^ 1];
    const int t = threadIdx.x, lx = t & 31, ly = t >> 5;
    const float inf = __uint_as_float(kInfBits);
    const float step1 = 1.0f, step2 = __uint_as_float(kSqrt2Bits), step3 = __uint_as_float(kSqrt3Bits);

    for (long long tile = blockIdx.x; tile < tl.n; tile += gridDim.x) {
        if (current[tile] == 0) continue;   // uniform over the workgroup
        __syncthreads();                    // everyone has read the flag, and the previous tile's LDS is done with
        if (t == 0) {
            current[tile] = 0;
            reach = 0;
        }
        const int tx = (int)(tile % tl.nx), ty = (int)((tile / tl.nx) % tl.ny), tz = (int)(tile / ((long long)tl.nx * tl.ny));
        const int z0 = tz * kTZ, y0 = ty * kTY, x0 = tx * kTX;
        // labels and field with the halo; outside the volume and outside 1..K: label 0, which joins nothing
        for (int i = t; i < kHaloVox; i += kThreads) {
            const int hx = i % kHX, hy = (i / kHX) % kHY, hz = i / (kHX * kHY);
            const int z = z0 + hz - 1, y = y0 + hy - 1, x = x0 + hx - 1;
            int l = 0;
            float d = inf;
            if (z >= 0 && z < dm.d && y >= 0 && y < dm.h && x >= 0 && x < dm.w) {
                const size_t v = ((size_t)z * dm.h + y) * dm.w + x;
                l = labels[v];
                if ((unsigned)l > (unsigned)n_labels) l = 0;
                if (l) d = field[v];
            }
            lab[i] = l;
            f[i] = d;
        }
        __syncthreads();

        // my column: the same-label neighbours of each voxel, and in cost mode the weight of entering it
        const int base = kHX * kHY + (ly + 1) * kHX + lx + 1;   // (z, y, x) = (0, ly, lx) of the tile
        unsigned mask[kPerThread];
        float w[kPerThread];
        bool any = false;
#pragma unroll
        for (int r = 0; r < kPerThread; ++r) {
            const int c = base + r * kHX * kHY;
            const int me = lab[c];
            unsigned m = 0;
            if (me) {
                int bit = 0;
#pragma unroll
                for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (dz == 0 && dy == 0 && dx == 0) continue;
                            if (lab[c + (dz * kHY + dy) * kHX + dx] == me) m |= 1u << bit;
                            ++bit;
                        }
            }
            w[r] = 0.0f;
            if (COST && m) {
                const float cv = cost[((size_t)(z0 + r) * dm.h + (y0 + ly)) * dm.w + (x0 + lx)];
                w[r] = cv >= 0.0f ? fabsf(cv) : inf;   // -0.0 is 0; negative and NaN cannot be entered
                if (!(w[r] < inf)) m = 0;
            }
            mask[r] = m;
            any |= m != 0;
        }
        // the labels are done with: a voxel's word now holds its mask, read again in every round (a mask kept
        // in a register would have its 26 tests hoisted out of the loop, into hundreds of lane masks)
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kPerThread; ++r) lab[base + r * kHX * kHY] = (int)mask[r];

        unsigned fell = 0;
        for (int round = 0; round <= kTileVox; ++round) {
            int changed = 0;
            if (any) {
#pragma unroll
                for (int r = 0; r < kPerThread; ++r) {
                    const int c = base + r * kHX * kHY;
                    const unsigned m = (unsigned)lab[c];
                    if (!m) continue;
                    float m1 = inf, m2 = inf, m3 = inf;   // by the number of coordinates that differ
                    int bit = 0;
#pragma unroll
                    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                            for (int dx = -1; dx <= 1; ++dx) {
                                if (dz == 0 && dy == 0 && dx == 0) continue;
                                const float raw = f[c + (dz * kHY + dy) * kHX + dx];
                                const float d = (m >> bit) & 1u ? raw : inf;
                                const int differ = (dz != 0) + (dy != 0) + (dx != 0);
                                if (differ == 1) m1 = fmin2(m1, d);
                                else if (differ == 2) m2 = fmin2(m2, d);
                                else m3 = fmin2(m3, d);
                                ++bit;
                            }
                    // x + w is monotone in x, so the minimum of the sums is the sum at the minimum
                    float best;
                    if (COST) best = fmin2(fmin2(m1, m2), m3) + w[r];
                    else best = fmin2(fmin2(m1 + step1, m2 + step2), m3 + step3);
                    if (best < f[c]) {
                        f[c] = best;
                        fell |= 1u << r;
                        changed = 1;
                    }
                }
            }
            if (!__syncthreads_or(changed)) break;
        }

        // the voxels that fell, and who sees them
        if (fell) {
            unsigned seen_by = 0;
#pragma unroll
            for (int r = 0; r < kPerThread; ++r)
                if ((fell >> r) & 1u)
                    field[((size_t)(z0 + r) * dm.h + (y0 + ly)) * dm.w + (x0 + lx)] = f[base + r * kHX * kHY];
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz) {
                if (dz == -1 && !(fell & 1u)) continue;
                if (dz == 1 && !(fell >> (kTZ - 1) & 1u)) continue;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
                    if ((dy == -1 && ly != 0) || (dy == 1 && ly != kTY - 1)) continue;
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if ((dx == -1 && lx != 0) || (dx == 1 && lx != kTX - 1)) continue;
                        if (dz || dy || dx) seen_by |= 1u << ((dz + 1) * 9 + (dy + 1) * 3 + dx + 1);
                    }
                }
            }
            if (seen_by) atomicOr(&reach, seen_by);
        }
        __syncthreads();
        if (t < 27 && ((reach >> t) & 1u)) {
            const int nz = tz + t / 9 - 1, ny = ty + (t / 3) % 3 - 1, nx = tx + t % 3 - 1;
            if (nz >= 0 && nz < tl.nz && ny >= 0 && ny < tl.ny && nx >= 0 && nx < tl.nx)
                flag_tile(next, next_count, ((long long)nz * tl.ny + ny) * tl.nx + nx);
        }
    }
}

// ---- the farthest table ----------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void far_init(unsigned long long* keys, size_t rows) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += step) keys[r] = 0;
}

__global__ __launch_bounds__(kThreads) void far_pass(const int* __restrict__ labels, const float* __restrict__ field,
                                                    size_t n, int n_labels, unsigned long long* keys) {
    const int lane = threadIdx.x & 63;
    const size_t step = (size_t)gridDim.x * kThreads;
    // the trip count is the same in every lane of the workgroup: the shuffles below see all 64
    for (size_t base = (size_t)blockIdx.x * kThreads; base < n; base += step) {
        const size_t v = base + threadIdx.x;
        int l = -1;
        unsigned long long key = 0;
        if (v < n) {
            l = labels[v];
            const unsigned bits = __float_as_uint(field[v]);
            // finite and non-negative: the bits order like the values, and bit 63 marks a key that was set
            if (l >= 1 && l <= n_labels && bits < kInfBits)
                key = (1ull << 63) | ((unsigned long long)bits << 32) | (0xFFFFFFFFu - (unsigned)v);
            else
                l = -1;
        }
        const int val = l >= 0 ? l : -1 - lane;
        const int prev = __shfl_up(val, 1);
        const bool head = lane == 0 || prev != val;
        const unsigned long long heads = __ballot(head);
        const int mine = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // my run's first lane
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long other = __shfl_down(key, d);
            const int theirs = __shfl_down(mine, d);
            if (lane + d < 64 && theirs == mine && other > key) key = other;
        }
        if (l >= 0 && head &&
            __hip_atomic_load(keys + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key)
            atomicMax(keys + l, key);
    }
}

__global__ __launch_bounds__(kThreads) void far_finish(const unsigned long long* __restrict__ keys, float* far_value,
                                                      int* far_index, size_t rows) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += step) {
        const unsigned long long key = keys[r];
        const bool set = r > 0 && (key >> 63);
        far_value[r] = set ? __uint_as_float((unsigned)(key >> 32) & 0x7FFFFFFFu) : 0.0f;
        far_index[r] = set ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
    }
}

// ---- hops, parents and paths -----------------------------------------------------------
constexpr unsigned kNoHops = 0xFFFFFFFFu;   // -1: read as unsigned the largest value, so a minimum needs no "infinity"

__device__ __forceinline__ bool finite_bits(unsigned b) { return (b & 0x7FFFFFFFu) < kInfBits; }

// the weight of entering a voxel in cost mode: -0.0 is 0; negative, NaN and +inf cannot be entered
__device__ __forceinline__ float entering_weight(float cv) { return cv >= 0.0f ? fabsf(cv) : __uint_as_float(kInfBits); }

__device__ __forceinline__ float euclid_step(int differ) {
    return differ == 1 ? 1.0f : __uint_as_float(differ == 2 ? kSqrt2Bits : kSqrt3Bits);
}

__global__ __launch_bounds__(kThreads) void hops_init(int* __restrict__ hops, size_t n, Header* hdr, int* flags,
                                                     size_t n_flags) {
    const size_t step = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (first == 0) *hdr = Header{0, {0, 0}, 0};
    for (size_t i = first; i < n_flags; i += step) flags[i] = 0;
    for (size_t v = first; v < n; v += step) hops[v] = -1;
}

__global__ __launch_bounds__(kThreads) void hops_seed(const int* __restrict__ labels, const int* __restrict__ sources,
                                                     int n_labels, const float* __restrict__ field, int* hops, Dims dm,
                                                     Tiles tl, Header* hdr, int* flags) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x + 1; r <= (size_t)n_labels; r += step) {
        const int s = sources[r];
        if (s == -1) continue;
        // a source whose field word is not +0.0 belongs to another field: the row counts as invalid
        if (s < 0 || s >= dm.n || labels[s] != (int)r || __float_as_uint(field[s]) != 0u) {
            atomicAdd(&hdr->invalid, 1);
            continue;
        }
        hops[s] = 0;
        const int x = s % dm.w, y = (s / dm.w) % dm.h, z = s / (dm.w * dm.h);
        for (int tz = (z - 1) / kTZ; tz <= (z + 1) / kTZ; ++tz)
            for (int ty = (y - 1) / kTY; ty <= (y + 1) / kTY; ++ty)
                for (int tx = (x - 1) / kTX; tx <= (x + 1) / kTX; ++tx)
                    if (tz < tl.nz && ty < tl.ny && tx < tl.nx)
                        flag_tile(flags, &hdr->count[0], ((long long)tz * tl.ny + ty) * tl.nx + tx);
    }
}

// ---- seeds from a list -----------------------------------------------------------------
// the seed's tile and the tiles that see it in their halo, as geodesic_sources flags them
__device__ __forceinline__ void flag_around(int s, const Dims& dm, const Tiles& tl, Header* hdr, int* flags) {
    const int x = s % dm.w, y = (s / dm.w) % dm.h, z = s / (dm.w * dm.h);
    for (int tz = (z - 1) / kTZ; tz <= (z + 1) / kTZ; ++tz)
        for (int ty = (y - 1) / kTY; ty <= (y + 1) / kTY; ++ty)
            for (int tx = (x - 1) / kTX; tx <= (x + 1) / kTX; ++tx)
                if (tz < tl.nz && ty < tl.ny && tx < tl.nx)
                    flag_tile(flags, &hdr->count[0], ((long long)tz * tl.ny + ty) * tl.nx + tx);
}

__global__ __launch_bounds__(kThreads) void reseed_clear(Header* hdr, int* flags, size_t n_flags) {
    const size_t step = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (first == 0) *hdr = Header{0, {0, 0}, 0};
    for (size_t i = first; i < n_flags; i += step) flags[i] = 0;
}

__global__ __launch_bounds__(kThreads) void reseed_seeds(const int* __restrict__ labels, const int* __restrict__ seeds,
                                                        long long n_seeds, int n_labels, float* field, Dims dm,
                                                        Tiles tl, Header* hdr, int* flags) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n_seeds; i += step) {
        const int s = seeds[i];
        int l = 0;
        if (s >= 0 && s < dm.n) l = labels[s];
        if (l < 1 || l > n_labels) {
            atomicAdd(&hdr->invalid, 1);
            continue;
        }
        field[s] = 0.0f;
        flag_around(s, dm, tl, hdr, flags);
    }
}

__global__ __launch_bounds__(kThreads) void hops_seed_list(const int* __restrict__ labels,
                                                          const int* __restrict__ seeds, long long n_seeds,
                                                          int n_labels, const float* __restrict__ field, int* hops,
                                                          Dims dm, Tiles tl, Header* hdr, int* flags) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n_seeds; i += step) {
        const int s = seeds[i];
        int l = 0;
        if (s >= 0 && s < dm.n) l = labels[s];
        // a seed whose field word is not +0.0 belongs to another field: the row counts as invalid
        if (l < 1 || l > n_labels || __float_as_uint(field[s]) != 0u) {
            atomicAdd(&hdr->invalid, 1);
            continue;
        }
        hops[s] = 0;
        flag_around(s, dm, tl, hdr, flags);
    }
}

template <bool COST>
__global__ __launch_bounds__(kThreads) void hops_sweep(const int* __restrict__ labels, const float* __restrict__ cost,
                                                      const float* __restrict__ field, int* hops, Dims dm, Tiles tl,
                                                      int n_labels, Header* hdr, int* flags) {
    __shared__ unsigned f[kHaloVox];   // the field's bits, then hops
    __shared__ int lab[kHaloVox];      // the labels, then the masks of tight predecessors
    __shared__ unsigned reach;         // as in geodesic_sweep
    const int parity = hdr->parity;
    if (hdr->count[parity] == 0) return;
    int* const current = flags + (size_t)parity * tl.n;
    int* const next = flags + (size_t)(parity ^ 1) * tl.n;
    int* const next_count = &hdr->count[parity ^ 1];
    const int t = threadIdx.x, lx = t & 31, ly = t >> 5;

    for (long long tile = blockIdx.x; tile < tl.n; tile += gridDim.x) {
        if (current[tile] == 0) continue;   // uniform over the workgroup
        __syncthreads();
        if (t == 0) {
            current[tile] = 0;
            reach = 0;
        }
        const int tx = (int)(tile % tl.nx), ty = (int)((tile / tl.nx) % tl.ny), tz = (int)(tile / ((long long)tl.nx * tl.ny));
        const int z0 = tz * kTZ, y0 = ty * kTY, x0 = tx * kTX;
        // labels and field with the halo; outside the volume, outside 1..K and not finite: label 0, no edge
        for (int i = t; i < kHaloVox; i += kThreads) {
            const int hx = i % kHX, hy = (i / kHX) % kHY, hz = i / (kHX * kHY);
            const int z = z0 + hz - 1, y = y0 + hy - 1, x = x0 + hx - 1;
            int l = 0;
            unsigned d = kInfBits;
            if (z >= 0 && z < dm.d && y >= 0 && y < dm.h && x >= 0 && x < dm.w) {
                const size_t v = ((size_t)z * dm.h + y) * dm.w + x;
                l = labels[v];
                if ((unsigned)l > (unsigned)n_labels) l = 0;
                if (l) {
                    d = __float_as_uint(field[v]);
                    if (!finite_bits(d)) l = 0;
                }
            }
            lab[i] = l;
            f[i] = d;
        }
        __syncthreads();

        // my column: the tight predecessors of each voxel
        const int base = kHX * kHY + (ly + 1) * kHX + lx + 1;   // (z, y, x) = (0, ly, lx) of the tile
        unsigned mask[kPerThread];
#pragma unroll
        for (int r = 0; r < kPerThread; ++r) {
            const int c = base + r * kHX * kHY;
            const int me = lab[c];
            unsigned m = 0;
            float w = 0.0f;
            bool open = me != 0;
            if (COST && open) {
                w = entering_weight(cost[((size_t)(z0 + r) * dm.h + (y0 + ly)) * dm.w + (x0 + lx)]);
                open = w < __uint_as_float(kInfBits);
            }
            if (open) {
                const unsigned mine = f[c];
                int bit = 0;
#pragma unroll
                for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (dz == 0 && dy == 0 && dx == 0) continue;
                            const int u = c + (dz * kHY + dy) * kHX + dx;
                            const float step = COST ? w : euclid_step((dz != 0) + (dy != 0) + (dx != 0));
                            // one IEEE float32 addition, the one the field was built with
                            if (lab[u] == me && __float_as_uint(__uint_as_float(f[u]) + step) == mine) m |= 1u << bit;
                            ++bit;
                        }
            }
            mask[r] = m;
        }
        __syncthreads();   // labels and field are done with
        bool any = false;
#pragma unroll
        for (int r = 0; r < kPerThread; ++r) {
            lab[base + r * kHX * kHY] = (int)mask[r];
            any |= mask[r] != 0;
        }
        for (int i = t; i < kHaloVox; i += kThreads) {
            const int hx = i % kHX, hy = (i / kHX) % kHY, hz = i / (kHX * kHY);
            const int z = z0 + hz - 1, y = y0 + hy - 1, x = x0 + hx - 1;
            unsigned h = kNoHops;
            if (z >= 0 && z < dm.d && y >= 0 && y < dm.h && x >= 0 && x < dm.w)
                h = (unsigned)hops[((size_t)z * dm.h + y) * dm.w + x];
            f[i] = h;
        }
        __syncthreads();

        // at most kTileVox + 1 rounds: a shortest chain of tight edges inside the tile has at most kTileVox
        unsigned fell = 0;
        for (int round = 0; round <= kTileVox; ++round) {
            int changed = 0;
            if (any) {
#pragma unroll
                for (int r = 0; r < kPerThread; ++r) {
                    const int c = base + r * kHX * kHY;
                    const unsigned m = (unsigned)lab[c];
                    if (!m) continue;
                    unsigned best = kNoHops;
                    int bit = 0;
#pragma unroll
                    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                            for (int dx = -1; dx <= 1; ++dx) {
                                if (dz == 0 && dy == 0 && dx == 0) continue;
                                const unsigned raw = f[c + (dz * kHY + dy) * kHX + dx];
                                const unsigned h = (m >> bit) & 1u ? raw : kNoHops;
                                best = h < best ? h : best;
                                ++bit;
                            }
                    // kNoHops + 1 would wrap to a source's 0
                    if (best != kNoHops && best + 1u < f[c]) {
                        f[c] = best + 1u;
                        fell |= 1u << r;
                        changed = 1;
                    }
                }
            }
            if (!__syncthreads_or(changed)) break;
        }

        // the voxels that fell, and who sees them
        if (fell) {
            unsigned seen_by = 0;
#pragma unroll
            for (int r = 0; r < kPerThread; ++r)
                if ((fell >> r) & 1u)
                    hops[((size_t)(z0 + r) * dm.h + (y0 + ly)) * dm.w + (x0 + lx)] = (int)f[base + r * kHX * kHY];
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz) {
                if (dz == -1 && !(fell & 1u)) continue;
                if (dz == 1 && !(fell >> (kTZ - 1) & 1u)) continue;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
                    if ((dy == -1 && ly != 0) || (dy == 1 && ly != kTY - 1)) continue;
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if ((dx == -1 && lx != 0) || (dx == 1 && lx != kTX - 1)) continue;
                        if (dz || dy || dx) seen_by |= 1u << ((dz + 1) * 9 + (dy + 1) * 3 + dx + 1);
                    }
                }
            }
            if (seen_by) atomicOr(&reach, seen_by);
        }
        __syncthreads();
        if (t < 27 && ((reach >> t) & 1u)) {
            const int nz = tz + t / 9 - 1, ny = ty + (t / 3) % 3 - 1, nx = tx + t % 3 - 1;
            if (nz >= 0 && nz < tl.nz && ny >= 0 && ny < tl.ny && nx >= 0 && nx < tl.nx)
                flag_tile(next, next_count, ((long long)nz * tl.ny + ny) * tl.nx + nx);
        }
    }
}

// parents only written; labels, cost, field and hops only read: no thread depends on another's result
template <bool COST>
__global__ __launch_bounds__(kThreads) void parents_pick(const int* __restrict__ labels, const float* __restrict__ cost,
                                                        const float* __restrict__ field, const int* __restrict__ hops,
                                                        Dims dm, int n_labels, int* __restrict__ parents, int* orphans) {
    const size_t n = (size_t)dm.n, step = (size_t)gridDim.x * kThreads;
    // the trip count is the same in every lane of the workgroup: the ballot below sees all 64
    for (size_t first = (size_t)blockIdx.x * kThreads; first < n; first += step) {
        const size_t v = first + threadIdx.x;
        bool orphan = false;
        if (v < n) {
            const int me = labels[v], h = hops[v];
            const unsigned mine = __float_as_uint(field[v]);
            int parent = h == 0 ? (int)v : -1;
            if (h != 0 && me >= 1 && me <= n_labels && finite_bits(mine)) {
                float w = 0.0f;
                bool open = true;
                if (COST) {
                    w = entering_weight(cost[v]);
                    open = w < __uint_as_float(kInfBits);
                }
                bool tight = false;
                if (open) {
                    const int x = (int)(v % dm.w), y = (int)((v / dm.w) % dm.h), z = (int)(v / ((size_t)dm.w * dm.h));
                    // in the order of the linear index: the first predecessor with one hop less is the smallest
                    for (int dz = -1; dz <= 1; ++dz) {
                        if (z + dz < 0 || z + dz >= dm.d) continue;
                        for (int dy = -1; dy <= 1; ++dy) {
                            if (y + dy < 0 || y + dy >= dm.h) continue;
                            for (int dx = -1; dx <= 1; ++dx) {
                                if ((dz == 0 && dy == 0 && dx == 0) || x + dx < 0 || x + dx >= dm.w) continue;
                                const size_t u = ((size_t)(z + dz) * dm.h + (y + dy)) * dm.w + (x + dx);
                                if (labels[u] != me) continue;
                                const unsigned theirs = __float_as_uint(field[u]);
                                if (!finite_bits(theirs)) continue;
                                const float s = COST ? w : euclid_step((dz != 0) + (dy != 0) + (dx != 0));
                                if (__float_as_uint(__uint_as_float(theirs) + s) != mine) continue;
                                tight = true;
                                if (parent < 0 && h >= 1 && hops[u] == h - 1) parent = (int)u;
                            }
                        }
                    }
                }
                orphan = !tight;
            }
            parents[v] = parent;
        }
        const unsigned long long ball = __ballot(orphan);
        if ((threadIdx.x & 63) == 0 && ball) atomicAdd(orphans, __popcll(ball));
    }
}

__global__ __launch_bounds__(kThreads) void trace_paths(const int* __restrict__ parents, const int* __restrict__ hops,
                                                       int n, const int* __restrict__ targets, int n_targets,
                                                       const long long* __restrict__ offsets, int* __restrict__ paths,
                                                       long long capacity, int* state) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n_targets; i += step) {
        const int target = targets[i];
        const int h = target >= 0 && target < n ? hops[target] : -1;
        const long long at = offsets[i], end = offsets[i + 1];
        if (h < 0 || at < 0 || end > capacity || end - at != (long long)h + 1) {
            atomicAdd(state, 1);   // the row is left unwritten
            continue;
        }
        int cur = target;
        bool broken = false;
        for (int k = h; k >= 0; --k) {   // at most h steps, whatever parents holds
            paths[at + k] = cur;
            const int p = parents[cur];
            if (k == 0) {
                broken = p != cur;   // the walk ends on a self-parent, the source
                break;
            }
            if (p < 0 || p >= n || p == cur) {
                broken = true;
                break;
            }
            cur = p;
        }
        if (broken) atomicAdd(state + 1, 1);
    }
}

const char* const kDimsMessage = "dims must be positive with a product of at most 2^31 - 1";

// what exaspim_fill_holes takes: the bound on the squared diagonal of exaspim_dbf belongs to its squared
// integer distances and has no part here
bool geodesic_dims(const int32_t dims[3], Dims* dm) { return valid_dims(dims, dm); }

bool aligned4(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 3) == 0;
}

}  // namespace
}  // namespace exaspim

using namespace exaspim;

extern "C" size_t exaspim_geodesic_workspace_bytes(const int32_t dims[3]) {
    Dims dm;
    if (!geodesic_dims(dims, &dm)) {
        set_error("geodesic_workspace_bytes: %s", kDimsMessage);
        return 0;
    }
    return workspace_need(dm);
}

extern "C" int exaspim_geodesic_begin(const int32_t* labels_dev, const int32_t dims[3], const int32_t* sources_dev,
                                      int32_t n_labels, float* field_dev, int32_t* state_dev, void* workspace_dev,
                                      size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && dims && sources_dev && field_dev && state_dev && workspace_dev,
                  "geodesic_begin: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(geodesic_dims(dims, &dm), "geodesic_begin: %s", kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "geodesic_begin: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && aligned4(labels_dev, sources_dev, field_dev, state_dev),
                  "geodesic_begin: misaligned buffer");
    const size_t need = workspace_need(dm);
    if (workspace_bytes < need) {
        set_error("geodesic_begin: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const Tiles tl = tiles_of(dm);
    Header* hdr = static_cast<Header*>(workspace_dev);
    int* flags = reinterpret_cast<int*>(static_cast<char*>(workspace_dev) + align_up(sizeof(Header), 16));
    geodesic_init<<<capped_grid((size_t)dm.n, kThreads), kThreads, 0, s>>>(labels_dev, field_dev, (size_t)dm.n, hdr,
                                                                           flags, 2 * (size_t)tl.n);
    geodesic_sources<<<capped_grid((size_t)n_labels, kThreads), kThreads, 0, s>>>(labels_dev, sources_dev, n_labels,
                                                                                  field_dev, dm, tl, hdr, flags);
    geodesic_publish<<<1, 1, 0, s>>>(hdr, state_dev, 0);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" int exaspim_geodesic_sweeps(const int32_t* labels_dev, const float* cost_dev, const int32_t dims[3],
                                       int32_t n_labels, float* field_dev, int32_t sweeps, int32_t* state_dev,
                                       void* workspace_dev, size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && dims && field_dev && state_dev && workspace_dev, "geodesic_sweeps: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(geodesic_dims(dims, &dm), "geodesic_sweeps: %s", kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "geodesic_sweeps: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(sweeps >= 1, "geodesic_sweeps: sweeps must be at least 1, got %d", sweeps);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && aligned4(labels_dev, cost_dev, field_dev, state_dev),
                  "geodesic_sweeps: misaligned buffer");
    const size_t need = workspace_need(dm);
    if (workspace_bytes < need) {
        set_error("geodesic_sweeps: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const Tiles tl = tiles_of(dm);
    Header* hdr = static_cast<Header*>(workspace_dev);
    int* flags = reinterpret_cast<int*>(static_cast<char*>(workspace_dev) + align_up(sizeof(Header), 16));
    const unsigned grid = capped_grid((size_t)tl.n, 1);
    for (int i = 0; i < sweeps; ++i) {
        if (cost_dev)
            geodesic_sweep<true><<<grid, kThreads, 0, s>>>(labels_dev, cost_dev, field_dev, dm, tl, n_labels, hdr, flags);
        else
            geodesic_sweep<false><<<grid, kThreads, 0, s>>>(labels_dev, nullptr, field_dev, dm, tl, n_labels, hdr,
                                                           flags);
        geodesic_publish<<<1, 1, 0, s>>>(hdr, state_dev, 1);
    }
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" size_t exaspim_geodesic_farthest_workspace_bytes(int32_t n_labels) {
    if (n_labels < 0) {
        set_error("geodesic_farthest_workspace_bytes: n_labels must not be negative, got %d", n_labels);
        return 0;
    }
    return align_up(((size_t)n_labels + 1) * sizeof(unsigned long long), 16);
}

extern "C" int exaspim_geodesic_farthest(const int32_t* labels_dev, const float* field_dev, const int32_t dims[3],
                                         int32_t n_labels, float* far_value_dev, int32_t* far_index_dev,
                                         void* workspace_dev, size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && field_dev && dims && far_value_dev && far_index_dev && workspace_dev,
                  "geodesic_farthest: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(geodesic_dims(dims, &dm), "geodesic_farthest: %s", kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "geodesic_farthest: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && aligned4(labels_dev, field_dev, far_value_dev, far_index_dev),
                  "geodesic_farthest: misaligned buffer");
    const size_t rows = (size_t)n_labels + 1;
    const size_t need = align_up(rows * sizeof(unsigned long long), 16);
    if (workspace_bytes < need) {
        set_error("geodesic_farthest: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* keys = static_cast<unsigned long long*>(workspace_dev);
    far_init<<<capped_grid(rows, kThreads), kThreads, 0, s>>>(keys, rows);
    far_pass<<<capped_grid((size_t)dm.n, kThreads), kThreads, 0, s>>>(labels_dev, field_dev, (size_t)dm.n, n_labels,
                                                                      keys);
    far_finish<<<capped_grid(rows, kThreads), kThreads, 0, s>>>(keys, far_value_dev, far_index_dev, rows);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

// ---- hops, parents and paths ---------------------------------------------------------------------------
extern "C" int exaspim_geodesic_parents_begin(const int32_t* labels_dev, const int32_t dims[3],
                                              const int32_t* sources_dev, int32_t n_labels, const float* field_dev,
                                              int32_t* hops_dev, int32_t* state_dev, void* workspace_dev,
                                              size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && dims && sources_dev && field_dev && hops_dev && state_dev && workspace_dev,
                  "geodesic_parents_begin: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(geodesic_dims(dims, &dm), "geodesic_parents_begin: %s", kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "geodesic_parents_begin: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && aligned4(labels_dev, sources_dev, field_dev, hops_dev) &&
                      aligned4(state_dev),
                  "geodesic_parents_begin: misaligned buffer");
    const size_t need = workspace_need(dm);
    if (workspace_bytes < need) {
        set_error("geodesic_parents_begin: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const Tiles tl = tiles_of(dm);
    Header* hdr = static_cast<Header*>(workspace_dev);
    int* flags = reinterpret_cast<int*>(static_cast<char*>(workspace_dev) + align_up(sizeof(Header), 16));
    hops_init<<<capped_grid((size_t)dm.n, kThreads), kThreads, 0, s>>>(hops_dev, (size_t)dm.n, hdr, flags,
                                                                       2 * (size_t)tl.n);
    hops_seed<<<capped_grid((size_t)n_labels, kThreads), kThreads, 0, s>>>(labels_dev, sources_dev, n_labels, field_dev,
                                                                           hops_dev, dm, tl, hdr, flags);
    geodesic_publish<<<1, 1, 0, s>>>(hdr, state_dev, 0);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" int exaspim_geodesic_reseed(const int32_t* labels_dev, const int32_t dims[3], int32_t n_labels,
                                       const int32_t* seeds_dev, int64_t n_seeds, float* field_dev, int32_t* state_dev,
                                       void* workspace_dev, size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && dims && field_dev && state_dev && workspace_dev, "geodesic_reseed: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(geodesic_dims(dims, &dm), "geodesic_reseed: %s", kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "geodesic_reseed: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(n_seeds >= 0, "geodesic_reseed: n_seeds must not be negative, got %lld", (long long)n_seeds);
    EXA_CHECK_ARG(n_seeds == 0 || seeds_dev, "geodesic_reseed: NULL argument");
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && aligned4(labels_dev, seeds_dev, field_dev, state_dev),
                  "geodesic_reseed: misaligned buffer");
    const size_t need = workspace_need(dm);
    if (workspace_bytes < need) {
        set_error("geodesic_reseed: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const Tiles tl = tiles_of(dm);
    Header* hdr = static_cast<Header*>(workspace_dev);
    int* flags = reinterpret_cast<int*>(static_cast<char*>(workspace_dev) + align_up(sizeof(Header), 16));
    reseed_clear<<<capped_grid(2 * (size_t)tl.n, kThreads), kThreads, 0, s>>>(hdr, flags, 2 * (size_t)tl.n);
    if (n_seeds > 0)
        reseed_seeds<<<capped_grid((size_t)n_seeds, kThreads), kThreads, 0, s>>>(
            labels_dev, seeds_dev, (long long)n_seeds, n_labels, field_dev, dm, tl, hdr, flags);
    geodesic_publish<<<1, 1, 0, s>>>(hdr, state_dev, 0);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" int exaspim_geodesic_parents_begin_seeds(const int32_t* labels_dev, const int32_t dims[3], int32_t n_labels,
                                                    const int32_t* seeds_dev, int64_t n_seeds, const float* field_dev,
                                                    int32_t* hops_dev, int32_t* state_dev, void* workspace_dev,
                                                    size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && dims && field_dev && hops_dev && state_dev && workspace_dev,
                  "geodesic_parents_begin_seeds: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(geodesic_dims(dims, &dm), "geodesic_parents_begin_seeds: %s", kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "geodesic_parents_begin_seeds: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(n_seeds >= 0, "geodesic_parents_begin_seeds: n_seeds must not be negative, got %lld",
                  (long long)n_seeds);
    EXA_CHECK_ARG(n_seeds == 0 || seeds_dev, "geodesic_parents_begin_seeds: NULL argument");
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && aligned4(labels_dev, seeds_dev, field_dev, hops_dev) &&
                      aligned4(state_dev),
                  "geodesic_parents_begin_seeds: misaligned buffer");
    const size_t need = workspace_need(dm);
    if (workspace_bytes < need) {
        set_error("geodesic_parents_begin_seeds: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const Tiles tl = tiles_of(dm);
    Header* hdr = static_cast<Header*>(workspace_dev);
    int* flags = reinterpret_cast<int*>(static_cast<char*>(workspace_dev) + align_up(sizeof(Header), 16));
    hops_init<<<capped_grid((size_t)dm.n, kThreads), kThreads, 0, s>>>(hops_dev, (size_t)dm.n, hdr, flags,
                                                                       2 * (size_t)tl.n);
    if (n_seeds > 0)
        hops_seed_list<<<capped_grid((size_t)n_seeds, kThreads), kThreads, 0, s>>>(
            labels_dev, seeds_dev, (long long)n_seeds, n_labels, field_dev, hops_dev, dm, tl, hdr, flags);
    geodesic_publish<<<1, 1, 0, s>>>(hdr, state_dev, 0);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" int exaspim_geodesic_parents_sweeps(const int32_t* labels_dev, const float* cost_dev, const float* field_dev,
                                               const int32_t dims[3], int32_t n_labels, int32_t* hops_dev,
                                               int32_t sweeps, int32_t* state_dev, void* workspace_dev,
                                               size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && field_dev && dims && hops_dev && state_dev && workspace_dev,
                  "geodesic_parents_sweeps: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(geodesic_dims(dims, &dm), "geodesic_parents_sweeps: %s", kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "geodesic_parents_sweeps: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(sweeps >= 1, "geodesic_parents_sweeps: sweeps must be at least 1, got %d", sweeps);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && aligned4(labels_dev, cost_dev, field_dev, hops_dev) &&
                      aligned4(state_dev),
                  "geodesic_parents_sweeps: misaligned buffer");
    const size_t need = workspace_need(dm);
    if (workspace_bytes < need) {
        set_error("geodesic_parents_sweeps: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const Tiles tl = tiles_of(dm);
    Header* hdr = static_cast<Header*>(workspace_dev);
    int* flags = reinterpret_cast<int*>(static_cast<char*>(workspace_dev) + align_up(sizeof(Header), 16));
    const unsigned grid = capped_grid((size_t)tl.n, 1);
    for (int i = 0; i < sweeps; ++i) {
        if (cost_dev)
            hops_sweep<true><<<grid, kThreads, 0, s>>>(labels_dev, cost_dev, field_dev, hops_dev, dm, tl, n_labels, hdr,
                                                       flags);
        else
            hops_sweep<false><<<grid, kThreads, 0, s>>>(labels_dev, nullptr, field_dev, hops_dev, dm, tl, n_labels, hdr,
                                                        flags);
        geodesic_publish<<<1, 1, 0, s>>>(hdr, state_dev, 1);
    }
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" int exaspim_geodesic_parents_finish(const int32_t* labels_dev, const float* cost_dev, const float* field_dev,
                                               const int32_t* hops_dev, const int32_t dims[3], int32_t n_labels,
                                               int32_t* parents_dev, int32_t* state_dev, void* stream) {
    EXA_CHECK_ARG(labels_dev && field_dev && hops_dev && dims && parents_dev && state_dev,
                  "geodesic_parents_finish: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(geodesic_dims(dims, &dm), "geodesic_parents_finish: %s", kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "geodesic_parents_finish: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(aligned4(labels_dev, cost_dev, field_dev, hops_dev) && aligned4(parents_dev, state_dev),
                  "geodesic_parents_finish: misaligned buffer");
    hipStream_t s = (hipStream_t)stream;
    EXA_CHECK_HIP(hipMemsetAsync(state_dev + 2, 0, sizeof(int32_t), s));
    const unsigned grid = capped_grid((size_t)dm.n, kThreads);
    if (cost_dev)
        parents_pick<true><<<grid, kThreads, 0, s>>>(labels_dev, cost_dev, field_dev, hops_dev, dm, n_labels, parents_dev,
                                                     state_dev + 2);
    else
        parents_pick<false><<<grid, kThreads, 0, s>>>(labels_dev, nullptr, field_dev, hops_dev, dm, n_labels, parents_dev,
                                                      state_dev + 2);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" int exaspim_trace_paths(const int32_t* parents_dev, const int32_t* hops_dev, const int32_t dims[3],
                                   const int32_t* targets_dev, int32_t n_targets, const int64_t* offsets_dev,
                                   int32_t* paths_dev, int64_t paths_capacity, int32_t* state_dev, void* stream) {
    EXA_CHECK_ARG(parents_dev && hops_dev && dims && offsets_dev && state_dev, "trace_paths: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(geodesic_dims(dims, &dm), "trace_paths: %s", kDimsMessage);
    EXA_CHECK_ARG(n_targets >= 0, "trace_paths: n_targets must not be negative, got %d", n_targets);
    EXA_CHECK_ARG(paths_capacity >= 0, "trace_paths: paths_capacity must not be negative, got %lld",
                  (long long)paths_capacity);
    EXA_CHECK_ARG(n_targets == 0 || (targets_dev && paths_dev), "trace_paths: NULL argument");
    EXA_CHECK_ARG(aligned4(parents_dev, hops_dev, targets_dev, paths_dev) && aligned4(state_dev) &&
                      ((uintptr_t)offsets_dev & 7) == 0,
                  "trace_paths: misaligned buffer");
    hipStream_t s = (hipStream_t)stream;
    EXA_CHECK_HIP(hipMemsetAsync(state_dev, 0, 2 * sizeof(int32_t), s));
    if (n_targets > 0)
        trace_paths<<<capped_grid((size_t)n_targets, kThreads), kThreads, 0, s>>>(
            parents_dev, hops_dev, dm.n, targets_dev, n_targets, reinterpret_cast<const long long*>(offsets_dev),
            paths_dev, (long long)paths_capacity, state_dev);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}
