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
//
// The streamed form (exaspim_components_stream_*) labels a volume that arrives in z slabs.
// A slab runs passes (a) to (e) as they are; instead of (f)/(g)'s final numbering every slab-local root
// that can still matter gets a provisional id (slab_ids: the same three-pass scan, offset by the
// running id count on the device), seam_union joins ids across the plane between two slabs in a
// second union-find over ids, and after the last slab table_* turn the id forest into
// table[provisional id] -> final label, which apply_table writes over the slabs.
//
// Watershed fragments (exaspim_watershed_fragments) differ in pass (a) alone:
// edge_mask_watershed writes the same mask byte from each voxel's steepest edge and its neighbours',
// and passes (b) to (g) run on it as they are. Their streamed form (exaspim_watershed_stream_slab)
// is the streamed components with edge_mask_watershed_slab as pass (a): it reads one carried plane of z
// affinities below the slab, hands two bits per edge across the seam above it to the next slab, which
// resolves them, and seam_affinity carries the plane on.
//
// Enclosed cavities (exaspim_fill_holes) are the components of a labelled volume's background:
// edge_mask_background writes the mask byte from the labels, passes (b) to (d) run on it as they are into
// a parent array in the workspace, and survey_faces, survey and fill decide per cavity and write the labels.
#include <algorithm>

#include "label_scan.h"

namespace exaspim {
namespace {

// the tile, the launch geometry, Dims, widen, scan_* and apply_table: label_scan.h
constexpr unsigned kBitZ = 1, kBitY = 2, kBitX = 4, kBitOn = 8;

// ---- (a) edge mask ---------------------------------------------------------------------------
// VEC voxels along x per thread (VEC * sizeof(T) = 16 bytes, or VEC = 1); w % VEC == 0, so a group
// never straddles a row and every channel base stays 16-byte aligned.
template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void edge_mask_affinity(const T* __restrict__ aff,
                                                              unsigned char* __restrict__ mask, Dims dm,
                                                              float thr, unsigned char* __restrict__ seam) {
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
        if (seam && !zin) {   // streamed slabs: the z edges that leave the slab, one byte per (y, x)
            Bytes sb;
#pragma unroll
            for (int k = 0; k < VEC; ++k) sb.b[k] = widen<T>(az.v[k]) >= thr ? 1 : 0;
            *reinterpret_cast<Bytes*>(seam + (i - ((unsigned)dm.n - (unsigned)dm.h * (unsigned)dm.w))) = sb;
        }
    }
}

// foreground mode: a voxel is on iff p >= thr, an edge iff both of its ends are
template <typename T>
__global__ __launch_bounds__(kThreads) void edge_mask_foreground(const T* __restrict__ p,
                                                                unsigned char* __restrict__ mask, Dims dm,
                                                                float thr, unsigned char* __restrict__ seam) {
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
        // streamed slabs: the last plane's on bits, the half of a seam edge this slab knows
        if (seam && (int)z == dm.d - 1) seam[i - ((unsigned)dm.n - hw)] = m ? 1 : 0;
    }
}

// ---- (a') watershed edge mask (exaspim_watershed_fragments) -------------------------------
// A voxel's steepest edge as a code: 0 none, else 1 .. 6 = the edge to -z, -y, -x, +x, +y, +z, which
// is the order of the other end's linear index. The candidates are offered in that order and replace
// the best so far only when strictly larger, so the first of equal values stays; "best" starts at low,
// which makes "eligible" (a > low, NaN never) and "larger than the best" one comparison. An edge that
// leaves the volume is offered as low itself: never eligible.
constexpr unsigned kToLowZ = 1, kToLowY = 2, kToLowX = 3, kToHighX = 4, kToHighY = 5, kToHighZ = 6;

__device__ __forceinline__ unsigned steepest(float mz, float my, float mx, float px, float py, float pz,
                                             float low) {
    float best = low;
    unsigned code = 0;
    if (mz > best) { best = mz; code = kToLowZ; }
    if (my > best) { best = my; code = kToLowY; }
    if (mx > best) { best = mx; code = kToLowX; }
    if (px > best) { best = px; code = kToHighX; }
    if (py > best) { best = py; code = kToHighY; }
    if (pz > best) { best = pz; code = kToHighZ; }
    return code;
}

// the code of one in-volume voxel from six scalar loads: the halo, whose voxels belong to other tiles
template <typename T>
__device__ __forceinline__ unsigned steepest_at(const T* __restrict__ aff, const Dims& dm, int z, int y, int x,
                                                float low) {
    const size_t n = (size_t)dm.n, hw = (size_t)dm.h * dm.w;
    const size_t i = ((size_t)z * dm.h + y) * dm.w + x;
    const float mz = z > 0 ? widen<T>(aff[i - hw]) : low;
    const float my = y > 0 ? widen<T>(aff[n + i - dm.w]) : low;
    const float mx = x > 0 ? widen<T>(aff[2 * n + i - 1]) : low;
    const float px = x < dm.w - 1 ? widen<T>(aff[2 * n + i]) : low;
    const float py = y < dm.h - 1 ? widen<T>(aff[n + i]) : low;
    const float pz = z < dm.d - 1 ? widen<T>(aff[i]) : low;
    return steepest(mz, my, mx, px, py, pz, low);
}

// One 8 x 8 x 32 tile per round of a workgroup. Step 1: the steepest edge of every voxel of the tile
// (VEC voxels along x per thread and load, as in edge_mask_affinity: w % VEC == 0, so a group is inside
// the volume or outside it as a whole) and of the one-voxel halo on the three high faces, as one byte
// per voxel in LDS. Step 2, after the barrier: an eligible edge v -- v + e is on iff its value is >= high
// or it is the steepest edge of v or of v + e. Affinities are read through L1/L2: every value is needed
// by its two ends, and both reads of it come from this workgroup except on the tile's faces.
// kBitOn is set for every voxel, as edge_mask_affinity sets it: a voxel without an on edge stays a set
// of one voxel, which the size floor of affinity mode removes.
constexpr int kCodeRow = kTX + 8;                               // 33 codes per row, rows 8-byte aligned
constexpr int kCodeBytes = (kTZ + 1) * (kTY + 1) * kCodeRow;    // 3240
constexpr int kHaloZ = kTY * kTX, kHaloY = kTZ * kTX, kHaloX = kTZ * kTY;

template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void edge_mask_watershed(const T* __restrict__ aff,
                                                               unsigned char* __restrict__ mask, Dims dm,
                                                               float low, float high, int tiles_x, int tiles_y,
                                                               long long n_tiles) {
    struct alignas(sizeof(T) * VEC) Pack { T v[VEC]; };
    struct alignas(VEC) Bytes { unsigned char b[VEC]; };
    constexpr int kGroupsPerRow = kTX / VEC;
    constexpr int kRounds = kTileVox / (kThreads * VEC);
    __shared__ __attribute__((aligned(16))) unsigned char code[kCodeBytes];
    const int t = threadIdx.x;
    const size_t n = (size_t)dm.n, hw = (size_t)dm.h * dm.w;
    // Neighbouring tiles read each other's face planes. Workgroups go round the 8 XCDs in turn, each with an
    // L2 of its own, so workgroup b takes tile (b % 8) * (grid / 8) + b / 8: an XCD works on a contiguous
    // run of tiles (a bijection on the first grid & ~7 workgroups, the rest keep their own; it decides
    // speed only: 0.59 against 0.69 ms at 512^3).
    const unsigned full = gridDim.x & ~7u;
    const unsigned first = blockIdx.x < full ? (blockIdx.x & 7u) * (full >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    for (long long tile = first; tile < n_tiles; tile += gridDim.x) {
        const int tx = (int)(tile % tiles_x), ty = (int)((tile / tiles_x) % tiles_y);
        const int tz = (int)(tile / ((long long)tiles_x * tiles_y));
        const int z0 = tz * kTZ, y0 = ty * kTY, x0 = tx * kTX;
        // per voxel k of round r: bit k of elig = edge to +z/+y/+x eligible, of sure = eligible and
        // (>= high or this voxel's steepest edge)
        unsigned elig_z[kRounds], elig_y[kRounds], elig_x[kRounds];
        unsigned sure_z[kRounds], sure_y[kRounds], sure_x[kRounds];
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int j = t + kThreads * r;
            const int row = j / kGroupsPerRow, lx = (j - row * kGroupsPerRow) * VEC;
            const int ly = row & (kTY - 1), lz = row >> 3;
            const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
            Bytes c;
#pragma unroll
            for (int k = 0; k < VEC; ++k) c.b[k] = 0;
            elig_z[r] = elig_y[r] = elig_x[r] = sure_z[r] = sure_y[r] = sure_x[r] = 0;
            if (z < dm.d && y < dm.h && x < dm.w) {
                const size_t i = ((size_t)z * dm.h + y) * dm.w + x;
                const bool zin = z < dm.d - 1, yin = y < dm.h - 1;
                const Pack az = *reinterpret_cast<const Pack*>(aff + i);
                const Pack ay = *reinterpret_cast<const Pack*>(aff + n + i);
                const Pack ax = *reinterpret_cast<const Pack*>(aff + 2 * n + i);
                Pack bz = az, by = ay;   // overwritten where the lower neighbour exists
                if (z > 0) bz = *reinterpret_cast<const Pack*>(aff + i - hw);
                if (y > 0) by = *reinterpret_cast<const Pack*>(aff + n + i - dm.w);
                float prev_x = x > 0 ? widen<T>(aff[2 * n + i - 1]) : low;
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float pz = zin ? widen<T>(az.v[k]) : low;
                    const float py = yin ? widen<T>(ay.v[k]) : low;
                    const float px = x + k < dm.w - 1 ? widen<T>(ax.v[k]) : low;
                    const float mz = z > 0 ? widen<T>(bz.v[k]) : low;
                    const float my = y > 0 ? widen<T>(by.v[k]) : low;
                    const unsigned cv = steepest(mz, my, prev_x, px, py, pz, low);
                    prev_x = px;   // only read where x + k + 1 exists, and then px is the in-volume value
                    c.b[k] = (unsigned char)cv;
                    const unsigned ez = pz > low, ey = py > low, ex = px > low;
                    elig_z[r] |= ez << k;
                    elig_y[r] |= ey << k;
                    elig_x[r] |= ex << k;
                    sure_z[r] |= (ez & (unsigned)(pz >= high || cv == kToHighZ)) << k;
                    sure_y[r] |= (ey & (unsigned)(py >= high || cv == kToHighY)) << k;
                    sure_x[r] |= (ex & (unsigned)(px >= high || cv == kToHighX)) << k;
                }
            }
            *reinterpret_cast<Bytes*>(code + (lz * (kTY + 1) + ly) * kCodeRow + lx) = c;
        }
        // the halo: plane z0 + 8, plane y0 + 8, column x0 + 32 (no corners: no edge of the tile ends there)
        for (int j = t; j < kHaloZ + kHaloY + kHaloX; j += kThreads) {
            int lz, ly, lx;
            if (j < kHaloZ) {
                lz = kTZ; ly = j >> 5; lx = j & (kTX - 1);
            } else if (j < kHaloZ + kHaloY) {
                lz = (j - kHaloZ) >> 5; ly = kTY; lx = j & (kTX - 1);
            } else {
                lz = (j - kHaloZ - kHaloY) >> 3; ly = j & (kTY - 1); lx = kTX;
            }
            const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
            unsigned cv = 0;
            if (z < dm.d && y < dm.h && x < dm.w) cv = steepest_at<T>(aff, dm, z, y, x, low);
            code[(lz * (kTY + 1) + ly) * kCodeRow + lx] = (unsigned char)cv;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int j = t + kThreads * r;
            const int row = j / kGroupsPerRow, lx = (j - row * kGroupsPerRow) * VEC;
            const int ly = row & (kTY - 1), lz = row >> 3;
            const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
            if (z < dm.d && y < dm.h && x < dm.w) {
                const unsigned char* here = code + (lz * (kTY + 1) + ly) * kCodeRow + lx;
                Bytes out;
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    unsigned m = kBitOn;
                    const unsigned up_z = here[k + (kTY + 1) * kCodeRow], up_y = here[k + kCodeRow], up_x = here[k + 1];
                    if (((sure_z[r] >> k) & 1u) | (((elig_z[r] >> k) & 1u) & (unsigned)(up_z == kToLowZ))) m |= kBitZ;
                    if (((sure_y[r] >> k) & 1u) | (((elig_y[r] >> k) & 1u) & (unsigned)(up_y == kToLowY))) m |= kBitY;
                    if (((sure_x[r] >> k) & 1u) | (((elig_x[r] >> k) & 1u) & (unsigned)(up_x == kToLowX))) m |= kBitX;
                    out.b[k] = (unsigned char)m;
                }
                *reinterpret_cast<Bytes*>(mask + ((size_t)z * dm.h + y) * dm.w + x) = out;
            }
        }
        __syncthreads();   // code is reused by the next tile
    }
}

// ---- (a'') watershed edge mask of a streamed slab (exaspim_watershed_stream_slab) -----------
// edge_mask_watershed for planes [z0, z0 + d) of a volume. What differs is the two faces across z:
//   below  carry_aff is the previous slab's last plane of z affinities as float32 (NULL for the volume's first
//          slab): the -z edges of the slab's plane 0;
//   above  unless the slab ends the volume (final), the z entries of its last plane are real edges and are
//          offered as +z. Their bit in the mask stays clear, as in the streamed components: the edge is
//          handed on as two bits per (y, x) in seam, bit 0 eligible, bit 1 sure (eligible and >= high or the
//          steepest edge of its lower end).
// carry_bits holds those two bits of the previous slab. Once a tile's codes are in LDS, one thread per (y, x) of
// plane 0 turns them into the edge's final state in place: 1 iff sure, or eligible and that voxel's steepest
// edge is -z. seam_mark and seam_union, later launches, read that byte. No other thread reads or writes it.
struct SlabSeam {
    const float* carry_aff;      // float32[h * w], NULL: the volume's first slab
    unsigned char* carry_bits;   // uint8[h * w], resolved in place; NULL with carry_aff
    unsigned char* seam;         // uint8[h * w], written; NULL: the volume's last slab (final)
};

// steepest_at for a slab: plane 0 takes -z from the carried plane, the last plane offers its real +z
template <typename T>
__device__ __forceinline__ unsigned steepest_at_slab(const T* __restrict__ aff, const Dims& dm, int z, int y, int x,
                                                     float low, const float* __restrict__ carry_aff, bool final) {
    const size_t n = (size_t)dm.n, hw = (size_t)dm.h * dm.w;
    const size_t p = (size_t)y * dm.w + x, i = (size_t)z * hw + p;
    float mz = low;
    if (z > 0) mz = widen<T>(aff[i - hw]);
    else if (carry_aff) mz = carry_aff[p];
    const float my = y > 0 ? widen<T>(aff[n + i - dm.w]) : low;
    const float mx = x > 0 ? widen<T>(aff[2 * n + i - 1]) : low;
    const float px = x < dm.w - 1 ? widen<T>(aff[2 * n + i]) : low;
    const float py = y < dm.h - 1 ? widen<T>(aff[n + i]) : low;
    const float pz = (z < dm.d - 1 || !final) ? widen<T>(aff[i]) : low;
    return steepest(mz, my, mx, px, py, pz, low);
}

// What a voxel knows of its three high edges travels with its code in the same LDS byte, where the sibling
// holds six words of bits per round in registers across the barrier: the seam's work needs those registers,
// and 64 of them are the eighth wave per SIMD. Per axis a state, 0 not eligible, 1 eligible, 2 sure (eligible
// and (>= high or this voxel's steepest edge)); byte = code | (sz + 3 sy + 9 sx) << 3, at most 6 | 26 << 3.
__device__ __forceinline__ unsigned pack_states(unsigned code, unsigned sz, unsigned sy, unsigned sx) {
    return code | ((sz + 3u * sy + 9u * sx) << 3);
}

// the three states of a byte; s / 9 and r / 3 as multiply and shift, exact for s <= 26 and r <= 8
__device__ __forceinline__ void unpack_states(unsigned byte, unsigned& sz, unsigned& sy, unsigned& sx) {
    const unsigned s = byte >> 3;
    sx = (s * 57u) >> 9;
    const unsigned r = s - 9u * sx;
    sy = (r * 11u) >> 5;
    sz = r - 3u * sy;
}

template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void edge_mask_watershed_slab(const T* __restrict__ aff,
                                                                    unsigned char* __restrict__ mask, Dims dm,
                                                                    float low, float high, int tiles_x, int tiles_y,
                                                                    long long n_tiles, SlabSeam sm) {
    struct alignas(sizeof(T) * VEC) Pack { T v[VEC]; };
    struct alignas(VEC) Bytes { unsigned char b[VEC]; };
    struct alignas(16) Floats { float v[4]; };
    constexpr int kGroupsPerRow = kTX / VEC;
    constexpr int kRounds = kTileVox / (kThreads * VEC);
    __shared__ __attribute__((aligned(16))) unsigned char code[kCodeBytes];
    const size_t n = (size_t)dm.n, hw = (size_t)dm.h * dm.w;
    const bool final = sm.seam == nullptr;
    // the XCD tile order of edge_mask_watershed
    const unsigned full = gridDim.x & ~7u;
    const unsigned first = blockIdx.x < full ? (blockIdx.x & 7u) * (full >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    for (long long tile = first; tile < n_tiles; tile += gridDim.x) {
        const int tx = (int)(tile % tiles_x), ty = (int)((tile / tiles_x) % tiles_y);
        const int tz = (int)(tile / ((long long)tiles_x * tiles_y));
        const int z0 = tz * kTZ, y0 = ty * kTY, x0 = tx * kTX;
        // The thread's index, opaque to the compiler and taken again for every tile: what is derived from it
        // (rows, LDS addresses, their constants) is otherwise hoisted out of this loop and held in registers
        // through it; this way it is a few VALU instructions per tile.
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int j = t + kThreads * r;
            const int row = j / kGroupsPerRow, lx = (j - row * kGroupsPerRow) * VEC;
            const int ly = row & (kTY - 1), lz = row >> 3;
            const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
            Bytes c;
#pragma unroll
            for (int k = 0; k < VEC; ++k) c.b[k] = 0;
            if (z < dm.d && y < dm.h && x < dm.w) {
                const size_t p = (size_t)y * dm.w + x, i = (size_t)z * hw + p;
                // the +z edges of the slab's last plane are real unless it is the volume's last
                const bool zin = z < dm.d - 1 || !final, yin = y < dm.h - 1;
                const bool below = z == 0 && sm.carry_aff != nullptr;   // plane 0 of a slab that is not the first
                const Pack az = *reinterpret_cast<const Pack*>(aff + i);
                const Pack ay = *reinterpret_cast<const Pack*>(aff + n + i);
                const Pack ax = *reinterpret_cast<const Pack*>(aff + 2 * n + i);
                Pack bz = az, by = ay;   // overwritten where the lower neighbour exists
                // The carried plane is float32, narrowed back to the slab's type: exact, it was widened from it.
                if constexpr (VEC * sizeof(T) == 16) {
                    // one 16-byte load, of the plane below in the slab or of the first four carried values
                    const void* zsrc = below ? (const void*)(sm.carry_aff + p) : (const void*)(aff + i - hw);
                    if (z > 0 || below) bz = *reinterpret_cast<const Pack*>(zsrc);
                    if constexpr (sizeof(T) == 2) {
                        if (below) {
                            Floats lo;
                            __builtin_memcpy(&lo, &bz, 16);
                            const Floats hi = *reinterpret_cast<const Floats*>(sm.carry_aff + p + 4);
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                bz.v[k] = (T)lo.v[k];
                                bz.v[4 + k] = (T)hi.v[k];
                            }
                        }
                    }
                } else {
                    if (z > 0) bz = *reinterpret_cast<const Pack*>(aff + i - hw);
                    if (below) bz.v[0] = (T)sm.carry_aff[p];
                }
                if (y > 0) by = *reinterpret_cast<const Pack*>(aff + n + i - dm.w);
                float prev_x = x > 0 ? widen<T>(aff[2 * n + i - 1]) : low;
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float pz = zin ? widen<T>(az.v[k]) : low;
                    const float py = yin ? widen<T>(ay.v[k]) : low;
                    const float px = x + k < dm.w - 1 ? widen<T>(ax.v[k]) : low;
                    const float mz = z > 0 || below ? widen<T>(bz.v[k]) : low;
                    const float my = y > 0 ? widen<T>(by.v[k]) : low;
                    const unsigned cv = steepest(mz, my, prev_x, px, py, pz, low);
                    prev_x = px;   // only read where x + k + 1 exists, and then px is the in-volume value
                    const unsigned ez = pz > low, ey = py > low, ex = px > low;
                    c.b[k] = (unsigned char)pack_states(cv, ez + (ez & (unsigned)(pz >= high || cv == kToHighZ)),
                                                        ey + (ey & (unsigned)(py >= high || cv == kToHighY)),
                                                        ex + (ex & (unsigned)(px >= high || cv == kToHighX)));
                }
            }
            *reinterpret_cast<Bytes*>(code + (lz * (kTY + 1) + ly) * kCodeRow + lx) = c;
        }
        // the halo: plane z0 + 8, plane y0 + 8, column x0 + 32 (no corners: no edge of the tile ends there);
        // a bare code, the states of a halo voxel are its own tile's
        for (int j = t; j < kHaloZ + kHaloY + kHaloX; j += kThreads) {
            int lz, ly, lx;
            if (j < kHaloZ) {
                lz = kTZ; ly = j >> 5; lx = j & (kTX - 1);
            } else if (j < kHaloZ + kHaloY) {
                lz = (j - kHaloZ) >> 5; ly = kTY; lx = j & (kTX - 1);
            } else {
                lz = (j - kHaloZ - kHaloY) >> 3; ly = j & (kTY - 1); lx = kTX;
            }
            const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
            unsigned cv = 0;
            if (z < dm.d && y < dm.h && x < dm.w) cv = steepest_at_slab<T>(aff, dm, z, y, x, low, sm.carry_aff, final);
            code[(lz * (kTY + 1) + ly) * kCodeRow + lx] = (unsigned char)cv;
        }
        __syncthreads();
        // The two seams, where this tile touches one: a plane of the tile is 8 x 32 voxels, one per thread, and
        // what a seam edge needs of its end in this slab is that voxel's byte.
        {
            const int ly = t >> 5, lx = t & (kTX - 1);
            const int y = y0 + ly, x = x0 + lx;
            const size_t p = (size_t)y * dm.w + x;
            if (tz == 0 && sm.carry_bits && y < dm.h && x < dm.w) {
                // the edge below plane 0 is on iff sure, or eligible and this voxel's steepest edge
                const unsigned cb = sm.carry_bits[p], cv = code[ly * kCodeRow + lx] & 7u;
                sm.carry_bits[p] = (unsigned char)(((cb >> 1) | (cb & (unsigned)(cv == kToLowZ))) & 1u);
            }
            const int lz = dm.d - 1 - z0;   // the slab's last plane, if it is in this tile
            if (!final && lz < kTZ && y < dm.h && x < dm.w) {
                unsigned sz, sy, sx;
                unpack_states(code[(lz * (kTY + 1) + ly) * kCodeRow + lx], sz, sy, sx);
                sm.seam[p] = (unsigned char)((sz != 0) | ((sz == 2) << 1));   // bit 0 eligible, bit 1 sure
            }
        }
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int j = t + kThreads * r;
            const int row = j / kGroupsPerRow, lx = (j - row * kGroupsPerRow) * VEC;
            const int ly = row & (kTY - 1), lz = row >> 3;
            const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
            if (z < dm.d && y < dm.h && x < dm.w) {
                const unsigned char* here = code + (lz * (kTY + 1) + ly) * kCodeRow + lx;
                const Bytes mine = *reinterpret_cast<const Bytes*>(here);
                const bool zin = z < dm.d - 1;   // the last plane's z edges are the seam's, not the mask's
                Bytes out;
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    unsigned m = kBitOn, sz, sy, sx;
                    unpack_states(mine.b[k], sz, sy, sx);
                    const unsigned up_z = here[k + (kTY + 1) * kCodeRow] & 7u, up_y = here[k + kCodeRow] & 7u;
                    const unsigned up_x = here[k + 1] & 7u;
                    if (zin && (sz == 2 || (sz == 1 && up_z == kToLowZ))) m |= kBitZ;
                    if (sy == 2 || (sy == 1 && up_y == kToLowY)) m |= kBitY;
                    if (sx == 2 || (sx == 1 && up_x == kToLowX)) m |= kBitX;
                    out.b[k] = (unsigned char)m;
                }
                *reinterpret_cast<Bytes*>(mask + ((size_t)z * dm.h + y) * dm.w + x) = out;
            }
        }
        __syncthreads();   // code is reused by the next tile
    }
}

// seam_aff[p] = float32 of the z affinity of the slab's last plane: the next slab's -z edges. A launch of its
// own after the mask, which reads the plane the slab before this one left there.
template <typename T>
__global__ __launch_bounds__(kThreads) void seam_affinity(const T* __restrict__ last_plane, float* __restrict__ seam_aff,
                                                         size_t hw) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += stride)
        seam_aff[p] = widen<T>(last_plane[p]);
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
// The predicates and sinks of label_scan.h's three passes: the whole-volume call, the streamed slabs
// and the streamed table.
constexpr int kSeamMark = (int)0x80000000;   // streamed slabs: aux bit "this root has a seam edge"

// the whole volume: kept roots, aux[v] = new id (1 ...) of a kept root, 0 for everything else
struct KeptRoot {
    const int* parent;
    const unsigned char* mask;
    int* aux;
    int min_size;
    __device__ __forceinline__ bool operator()(size_t v) const {
        return parent[v] == (int)v && (mask[v] & kBitOn) && aux[v] >= min_size;   // size = aux + 1 > min_size
    }
    __device__ __forceinline__ void operator()(size_t v, bool flag, int rank) const { aux[v] = flag ? rank + 1 : 0; }
};

// a slab: roots that are large enough on their own or have an edge across a seam (the
// singleton rule). aux[v] = provisional id = *ids_used + rank + 1, with its size and itself as parent
// in the id table; an id beyond the capacity is not written anywhere and becomes 0 (slab_advance
// raises the overflow flag).
struct SlabRoot {
    const int* parent;
    const unsigned char* mask;
    int* aux;
    int min_size;
    const int* ids_used;
    int capacity;
    int* id_parent;
    long long* id_count;
    __device__ __forceinline__ bool operator()(size_t v) const {
        if (parent[v] != (int)v || !(mask[v] & kBitOn)) return false;
        const int a = aux[v];
        return a < 0 || a >= min_size;
    }
    __device__ __forceinline__ void operator()(size_t v, bool flag, int rank) const {
        int out = 0;
        if (flag) {
            const long long id = (long long)*ids_used + rank + 1;
            if (id <= capacity) {
                out = (int)id;
                id_parent[id] = out;
                id_count[id] = (long long)(aux[v] & ~kSeamMark) + 1;
            }
        }
        aux[v] = out;
    }
};

// the id table after the last slab: roots whose summed size passes the filter, ids 1 .. *ids_used
struct TableRoot {
    const int* id_parent;
    const long long* id_count;
    const int* ids_used;
    long long min_size;
    int* table;
    __device__ __forceinline__ bool operator()(size_t v) const {
        return v >= 1 && v <= (size_t)*ids_used && id_parent[v] == (int)v && id_count[v] > min_size;
    }
    __device__ __forceinline__ void operator()(size_t v, bool flag, int rank) const { table[v] = flag ? rank + 1 : 0; }
};

// ---- (g) relabel -----------------------------------------------------------------------------
// labels is the flattened parent array: a thread reads only its own entry of it before writing it.
__global__ __launch_bounds__(kThreads) void relabel(int* labels, const int* __restrict__ aux, int n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < (size_t)n; g += stride)
        labels[g] = aux[labels[g]];
}

// ---- enclosed cavities (exaspim_fill_holes) -------------------------------------------------
// The cavities of a labelled volume are the components of its background: edge_mask_background writes the
// mask byte of pass (a) from the labels, passes (b) to (d) run on it as they are into a parent array in
// the workspace (a foreground voxel has no bit set and stays a root of its own), and three passes follow:
//   survey_faces  every background voxel on a face of the volume marks its cavity open: lo[root] = 0;
//   survey        lo[root] = the smallest, hi[root] = the largest positive label next to the cavity;
//   fill          a background voxel whose root has lo == hi > 0 becomes that label.
constexpr int kNoLabel = 2147483647;   // lo of a cavity nobody has reported a neighbour of (hi: 0)

// VEC voxels along x per thread (16-byte loads, or VEC = 1); w % VEC == 0, so a group never straddles a
// row. A bit is set iff this voxel and the next one along the axis are both background.
template <int VEC>
__global__ __launch_bounds__(kThreads) void edge_mask_background(const int* __restrict__ labels,
                                                                unsigned char* __restrict__ mask, Dims dm) {
    struct alignas(4 * VEC) Pack { int v[VEC]; };
    struct alignas(VEC) Bytes { unsigned char b[VEC]; };
    const size_t groups = (size_t)dm.n / VEC;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const unsigned hw = (unsigned)dm.h * (unsigned)dm.w;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const unsigned i = (unsigned)(g * VEC);
        const unsigned row = i / (unsigned)dm.w, x0 = i - row * (unsigned)dm.w;
        const unsigned z = row / (unsigned)dm.h, y = row - z * (unsigned)dm.h;
        const bool zin = (int)z < dm.d - 1, yin = (int)y < dm.h - 1;
        const Pack me = *reinterpret_cast<const Pack*>(labels + i);
        Pack up_z = me, up_y = me;   // overwritten where the upper neighbour exists
        if (zin) up_z = *reinterpret_cast<const Pack*>(labels + i + hw);
        if (yin) up_y = *reinterpret_cast<const Pack*>(labels + i + (unsigned)dm.w);
        // the voxel after the group; past the row's end a foreground value stands for "no edge"
        const int after = (int)(x0 + VEC) < dm.w ? labels[i + VEC] : 1;
        Bytes out;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            unsigned m = 0;
            if (me.v[k] <= 0) {
                m = kBitOn;
                if (zin && up_z.v[k] <= 0) m |= kBitZ;
                if (yin && up_y.v[k] <= 0) m |= kBitY;
                if ((k + 1 < VEC ? me.v[(k + 1) % VEC] : after) <= 0) m |= kBitX;
            }
            out.b[k] = (unsigned char)m;
        }
        *reinterpret_cast<Bytes*>(mask + i) = out;
    }
}

// The six faces as three pairs of planes, one thread per face voxel (edges and corners more than once,
// and both planes of an axis of length 1 are the same one: every store is the same 0). parent is flattened.
__global__ __launch_bounds__(kThreads) void survey_faces(const int* __restrict__ labels,
                                                        const int* __restrict__ parent, int* lo, Dims dm) {
    const size_t hw = (size_t)dm.h * dm.w, dw = (size_t)dm.d * dm.w, dh = (size_t)dm.d * dm.h;
    const size_t total = 2 * (hw + dw + dh);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        size_t j = g, z, y, x;
        if (j < 2 * hw) {
            z = j < hw ? 0 : (size_t)dm.d - 1;
            if (j >= hw) j -= hw;
            y = j / (size_t)dm.w;
            x = j - y * (size_t)dm.w;
        } else if (j < 2 * (hw + dw)) {
            j -= 2 * hw;
            y = j < dw ? 0 : (size_t)dm.h - 1;
            if (j >= dw) j -= dw;
            z = j / (size_t)dm.w;
            x = j - z * (size_t)dm.w;
        } else {
            j -= 2 * (hw + dw);
            x = j < dh ? 0 : (size_t)dm.w - 1;
            if (j >= dh) j -= dh;
            z = j / (size_t)dm.h;
            y = j - z * (size_t)dm.h;
        }
        const size_t v = (z * dm.h + y) * dm.w + x;
        if (labels[v] > 0) continue;
        const int r = parent[v];
        if (lo[r] != 0) lo[r] = 0;   // a stale read only repeats the store
    }
}

// One thread per voxel. A background voxel offers the positive labels among its six neighbours to its
// cavity's root; a neighbour across an on edge of the mask is background and is not read. lo[root] == 0
// was stored by survey_faces, a launch that has finished: such a cavity is open for good and its voxels
// read nothing more, which is nearly every voxel of a neurite volume (its background is one cavity).
// Lanes of a wave hold consecutive voxels: a run of lanes with the same root is reduced in the wave and
// its first lane updates the two words, and only where a whole load does not already cover the run's
// value. Minima and maxima: the result does not depend on the order in which they arrive.
__global__ __launch_bounds__(kThreads) void survey(const int* __restrict__ labels,
                                                  const unsigned char* __restrict__ mask,
                                                  const int* __restrict__ parent, int* lo, int* hi, Dims dm) {
    const size_t n = (size_t)dm.n, stride = (size_t)gridDim.x * blockDim.x;
    const unsigned hw = (unsigned)dm.h * (unsigned)dm.w;
    const int lane = threadIdx.x & 63;
    const size_t rounds = (n + stride - 1) / stride;   // whole waves stay in the loop together
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t it = 0; it < rounds; ++it, g += stride) {
        int root = -1 - lane;   // foreground and out-of-range lanes: distinct, never an address
        int mn = kNoLabel, mx = 0;
        if (g < n) {
            const unsigned m = mask[g];
            if (m & kBitOn) {
                root = parent[g];
                // a plain load, through L1: only the launch before this one stores a 0, this one's minima are
                // positive, and any other value read here, whatever its age, only means "not marked open"
                if (lo[root] != 0) {
                    const unsigned i = (unsigned)g;
                    const unsigned row = i / (unsigned)dm.w, x = i - row * (unsigned)dm.w;
                    const unsigned z = row / (unsigned)dm.h, y = row - z * (unsigned)dm.h;
                    auto offer = [&](int l) {
                        if (l > 0) {
                            mn = min(mn, l);
                            mx = max(mx, l);
                        }
                    };
                    if (z > 0) offer(labels[i - hw]);
                    if (y > 0) offer(labels[i - (unsigned)dm.w]);
                    if (x > 0) offer(labels[i - 1]);
                    // the mask holds no edge that leaves the volume: a cleared bit may be the face
                    if (!(m & kBitX) && (int)x < dm.w - 1) offer(labels[i + 1]);
                    if (!(m & kBitY) && (int)y < dm.h - 1) offer(labels[i + (unsigned)dm.w]);
                    if (!(m & kBitZ) && (int)z < dm.d - 1) offer(labels[i + hw]);
                }
            }
        }
        if (!__ballot(mx > 0)) continue;   // the same in every lane of the wave
        const int prev = __shfl_up(root, 1);
        const bool head = lane == 0 || prev != root;
        const unsigned long long heads = __ballot(head);
        const int mine = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // my run's first lane
        // the smallest and the largest offer of [lane, end of the run]
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int other_mn = __shfl_down(mn, d), other_mx = __shfl_down(mx, d);
            const int theirs = __shfl_down(mine, d);
            if (lane + d < 64 && theirs == mine) {
                mn = min(mn, other_mn);
                mx = max(mx, other_mx);
            }
        }
        if (head && mx > 0) {
            if (__hip_atomic_load(lo + root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mn) atomicMin(lo + root, mn);
            if (__hip_atomic_load(hi + root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mx) atomicMax(hi + root, mx);
        }
    }
}

// out[v] = labels[v], or the one label around the cavity of a background voxel whose cavity is a hole.
// out may be labels: a thread reads only its own voxel of it before writing it. counts[0] += holes (counted
// at the cavity's root voxel), counts[1] += filled voxels: summed per wave, one 64-bit add each.
__global__ __launch_bounds__(kThreads) void fill(const int* labels, const int* __restrict__ parent,
                                                const int* __restrict__ lo, const int* __restrict__ hi, int* out,
                                                unsigned long long* counts, int n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    const size_t rounds = ((size_t)n + stride - 1) / stride;   // whole waves stay in the loop together
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long holes = 0, voxels = 0;
    for (size_t it = 0; it < rounds; ++it, g += stride) {
        bool filled = false, at_root = false;
        if (g < (size_t)n) {
            int l = labels[g];
            if (l <= 0) {
                const int r = parent[g];
                const int a = lo[r];
                if (a > 0 && a == hi[r]) {
                    l = a;
                    filled = true;
                    at_root = r == (int)g;
                }
            }
            out[g] = l;
        }
        voxels += (unsigned long long)__popcll(__ballot(filled));
        holes += (unsigned long long)__popcll(__ballot(at_root));
    }
    if (lane == 0 && voxels) atomicAdd(counts + 1, voxels);
    if (lane == 0 && holes) atomicAdd(counts, holes);
}

// ---- the 26-connected pieces of a label volume (exaspim_label_pieces) -----------------------
// A piece is a maximal 26-connected set of voxels with one label in 1 .. K. No mask: the edges are read off
// the labels. Every voxel looks at its 13 neighbours that come before it in linear order, four rows of three
// (dz, dy) = (-1, -1), (-1, 0), (-1, 1), (0, -1) and the voxel before it along x. Within a row the middle voxel
// stands for its two x neighbours where it carries the label itself: the three are then joined along x,
// by whoever owns that edge, so one union is enough. Passes:
//   pieces_tile_pass   the unions inside an 8 x 8 x 32 tile, in LDS; parent[v] = global index of the tile's root,
//                      count[tile's root] = the voxels of its set inside the tile, a plain store;
//   pieces_seam_merge  the unions whose other end lies in another tile, in global memory;
//   flatten            as it is; a background voxel is a root of its own;
//   pieces_sizes       count[root] += count[tile's root]: one atomic per tile a piece runs through, not one per
//                      run of voxels as in sizes, which a few large pieces turn into a few hot words;
//   scan_*             PieceRoot: foreground roots of at least dust voxels, numbered in index order;
//   pieces_relabel     pieces[v] = number of root(v), 0 for background and dust; counts the dust roots.
__device__ __forceinline__ int piece_label(int l, int k) { return (unsigned)l - 1u < (unsigned)k ? l : 0; }

// LDS: the tile's labels, parents and counts and one flag per wave, 3 * 8192 + 16 bytes
__global__ __launch_bounds__(kThreads) void pieces_tile_pass(const int* __restrict__ labels,
                                                            int* __restrict__ parent, int* __restrict__ count,
                                                            Dims dm, int n_labels, int tiles_x, int tiles_y,
                                                            long long n_tiles) {
    __shared__ int ll[kTileVox];
    __shared__ int lp[kTileVox];
    __shared__ int lc[kTileVox];
    __shared__ int wave_any[kThreads / 64];
    const int t = threadIdx.x, lane = t & 63, lx = t & 31, ly = t >> 5;   // voxel k of a thread: lz = k
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tx = (int)(tile % tiles_x), ty = (int)((tile / tiles_x) % tiles_y);
        const int tz = (int)(tile / ((long long)tiles_x * tiles_y));
        const int x = tx * kTX + lx, y = ty * kTY + ly;
        const bool column = x < dm.w && y < dm.h;
        int lab[kPerThread];
        bool any = false;
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int z = tz * kTZ + k;
            lab[k] = 0;
            if (column && z < dm.d) lab[k] = piece_label(labels[((size_t)z * dm.h + y) * dm.w + x], n_labels);
            any |= lab[k] != 0;
        }
        const unsigned long long some = __ballot(any);
        if (lane == 0) wave_any[t >> 6] = some != 0;
        __syncthreads();
        bool tile_any = false;
#pragma unroll
        for (int wv = 0; wv < kThreads / 64; ++wv) tile_any |= wave_any[wv] != 0;
        if (!tile_any) {   // the same in every thread: nothing to unite, every voxel its own root
#pragma unroll
            for (int k = 0; k < kPerThread; ++k) {
                const int z = tz * kTZ + k;
                if (column && z < dm.d) {
                    const size_t v = ((size_t)z * dm.h + y) * dm.w + x;
                    parent[v] = (int)v;
                }
            }
            __syncthreads();   // wave_any is written again by the next tile
            continue;
        }
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int i = t + kThreads * k;
            // a row of 32 voxels is half a wave: start of this voxel's run of one label along x
            const int before = __shfl_up(lab[k], 1);
            const bool joined = lx > 0 && lab[k] != 0 && before == lab[k];
            const unsigned long long ball = __ballot(joined);
            const unsigned rowbits = (unsigned)(ball >> (lane & 32));
            const unsigned off = ~rowbits & (0xFFFFFFFFu >> (31 - lx));   // bit 0 is never set in rowbits
            ll[i] = lab[k];
            lc[i] = 0;
            lp[i] = (i & ~31) + 31 - __clz((int)off);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int i = t + kThreads * k;
            const int mine = ll[i];
            if (mine == 0) continue;
            auto row = [&](int dz, int dy) {
                if (k + dz < 0 || ly + dy < 0 || ly + dy >= kTY) return;   // another tile's: pieces_seam_merge
                const int j = i + dz * (kTY * kTX) + dy * kTX;
                if (ll[j] == mine) {
                    unite<LdsLoad>(lp, i, j);
                    return;
                }
                if (lx > 0 && ll[j - 1] == mine) unite<LdsLoad>(lp, i, j - 1);
                if (lx < kTX - 1 && ll[j + 1] == mine) unite<LdsLoad>(lp, i, j + 1);
            };
            row(-1, -1);
            row(-1, 0);
            row(-1, 1);
            row(0, -1);
        }
        __syncthreads();
        // the voxel count of every tile-local root
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int i = t + kThreads * k;
            if (ll[i] != 0) atomicAdd(lc + find_root<LdsLoad>(lp, i), 1);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int i = t + kThreads * k;
            const int z = tz * kTZ + k;
            if (column && z < dm.d) {
                const int r = find_root<LdsLoad>(lp, i);
                const int rz = tz * kTZ + (r >> 8), ry = ty * kTY + ((r >> 5) & (kTY - 1));
                const int rx = tx * kTX + (r & 31);
                const size_t v = ((size_t)z * dm.h + y) * dm.w + x;
                parent[v] = (int)(((size_t)rz * dm.h + ry) * dm.w + rx);
                if (r == i && ll[i] != 0) count[v] = lc[i];   // every other word of count stays 0
            }
        }
        __syncthreads();   // ll, lp, lc and wave_any are reused by the next tile
    }
}

// count[root] += count[v] for every tile-local root v that is not its piece's root (parent is flattened). A word
// that is read here to be added is never added to: only a piece's root receives, and a root adds nothing.
__global__ __launch_bounds__(kThreads) void pieces_sizes(const int* __restrict__ parent, int* count, int n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < (size_t)n; g += stride) {
        const int r = parent[g];
        if (r == (int)g) continue;
        const int c = count[g];
        if (c > 0) atomicAdd(count + r, c);
    }
}

// One thread per voxel; only a foreground voxel on the low z, either y or either x face of its tile has an
// earlier neighbour in another tile. A neighbour is read only where it lies inside the volume.
__global__ __launch_bounds__(kThreads) void pieces_seam_merge(const int* __restrict__ labels, int* parent, Dims dm,
                                                             int n_labels) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int hw = dm.h * dm.w;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < (size_t)dm.n; g += stride) {
        const int i = (int)g;
        const int rowi = i / dm.w, x = i - rowi * dm.w;
        const int z = rowi / dm.h, y = rowi - z * dm.h;
        const int lx = x & (kTX - 1), ly = y & (kTY - 1), lz = z & (kTZ - 1);
        if (lz != 0 && ly != 0 && ly != kTY - 1 && lx != 0 && lx != kTX - 1) continue;
        const int mine = piece_label(labels[g], n_labels);
        if (mine == 0) continue;
        auto row = [&](int dz, int dy) {
            if (z + dz < 0 || y + dy < 0 || y + dy >= dm.h) return;
            const bool outside = (dz < 0 && lz == 0) || (dy < 0 && ly == 0) || (dy > 0 && ly == kTY - 1);
            const int j = i + dz * hw + dy * dm.w;
            if (piece_label(labels[j], n_labels) == mine) {
                if (outside) unite<GlobalLoad>(parent, i, j);
                return;
            }
            if (x > 0 && (outside || lx == 0) && piece_label(labels[j - 1], n_labels) == mine)
                unite<GlobalLoad>(parent, i, j - 1);
            if (x < dm.w - 1 && (outside || lx == kTX - 1) && piece_label(labels[j + 1], n_labels) == mine)
                unite<GlobalLoad>(parent, i, j + 1);
        };
        row(-1, -1);
        row(-1, 0);
        row(-1, 1);
        row(0, -1);
        if (lx == 0 && x > 0 && piece_label(labels[i - 1], n_labels) == mine) unite<GlobalLoad>(parent, i, i - 1);
    }
}

// kept pieces: foreground roots of at least dust voxels; aux[v] = the piece's number (1 ...), 0 for every other
// voxel. aux holds pieces_sizes' count at a root: the piece's voxels.
struct PieceRoot {
    const int* parent;
    const int* labels;
    int* aux;
    int n_labels;
    long long dust;
    __device__ __forceinline__ bool operator()(size_t v) const {
        return parent[v] == (int)v && piece_label(labels[v], n_labels) != 0 && (long long)aux[v] >= dust;
    }
    __device__ __forceinline__ void operator()(size_t v, bool flag, int rank) const { aux[v] = flag ? rank + 1 : 0; }
};

// pieces is the flattened parent array: a thread reads only its own entry of it before writing it. A foreground
// root whose aux is 0 is a dust piece: counted per wave, one add each.
__global__ __launch_bounds__(kThreads) void pieces_relabel(const int* __restrict__ labels, int* pieces,
                                                          const int* __restrict__ aux, int* dust_count, int n_labels,
                                                          int n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    const size_t rounds = ((size_t)n + stride - 1) / stride;   // whole waves stay in the loop together
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int dust = 0;
    for (size_t it = 0; it < rounds; ++it, g += stride) {
        bool dusty = false;
        if (g < (size_t)n) {
            int out = 0;
            if (piece_label(labels[g], n_labels) != 0) {
                const int r = pieces[g];
                out = aux[r];
                dusty = out == 0 && r == (int)g;
            }
            pieces[g] = out;
        }
        dust += __popcll(__ballot(dusty));
    }
    if (lane == 0 && dust) atomicAdd(dust_count, dust);
}

// ---- pieces with open faces (exaspim_label_pieces_open) ---------------------------------------
// A piece with a voxel on an open face goes on in the block next door: its size here says nothing, so it is
// kept whatever its count. The passes are exaspim_label_pieces' with one more after pieces_sizes:
//   pieces_mark_open   one thread per pixel of the open faces: count[root] |= kOpenMark;
//   scan_*             OpenPieceRoot: foreground roots that are marked or of at least dust voxels.
// A count is at most 2^31 - 1, so the sign bit is free (kSeamMark of the streamed slabs is the precedent).
constexpr int kOpenMark = (int)0x80000000;
constexpr unsigned kOpenGrid = 2048;   // a few workgroups per CU that stride over the pixels, as border.hip's

// The pixels of the open faces, packed plane after plane in the order of border.hip: z = 0, z = D - 1 (H x W
// each), y = 0, y = H - 1 (D x W), x = 0, x = W - 1 (D x H). first[f] is face f's first packed pixel, first[6]
// the total; a closed face is empty: first[f + 1] == first[f].
struct OpenPlanes {
    long long first[7];
};

OpenPlanes open_planes_of(const Dims& dm, uint32_t open_faces) {
    const long long size[3] = {(long long)dm.h * dm.w, (long long)dm.d * dm.w, (long long)dm.d * dm.h};
    OpenPlanes op;
    op.first[0] = 0;
    for (int f = 0; f < 6; ++f) op.first[f + 1] = op.first[f] + ((open_faces >> f) & 1u ? size[f >> 1] : 0);
    return op;
}

// Every thread of a face that is one piece aims at one word: the word is read first and the atomic issued only
// where the mark is not there yet (DESIGN 6q on hot words). The plain read may be stale, which costs one more
// atomicOr of a bit that is already set. Nobody else writes count during this launch, and parent is final.
__global__ __launch_bounds__(kThreads) void pieces_mark_open(const int* __restrict__ labels,
                                                            const int* __restrict__ parent, int* count, Dims dm,
                                                            int n_labels, OpenPlanes op) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)op.first[6]; i += stride) {
        int face = 0;
        long long first = 0;
#pragma unroll
        for (int f = 1; f < 6; ++f) {   // the last face that starts at or before i: it is not empty
            if ((long long)i >= op.first[f]) face = f, first = op.first[f];
        }
        const int local = (int)((long long)i - first);   // below the plane's pixels <= d h w
        int z, y, x;
        if (face < 2) {
            y = local / dm.w, x = local - y * dm.w, z = face == 0 ? 0 : dm.d - 1;
        } else if (face < 4) {
            z = local / dm.w, x = local - z * dm.w, y = face == 2 ? 0 : dm.h - 1;
        } else {
            z = local / dm.h, y = local - z * dm.h, x = face == 4 ? 0 : dm.w - 1;
        }
        const size_t v = ((size_t)z * dm.h + y) * dm.w + x;
        if (piece_label(labels[v], n_labels) == 0) continue;
        int* word = count + parent[v];
        if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0) atomicOr(word, kOpenMark);
    }
}

// kept pieces of a block: foreground roots that are marked open or of at least dust voxels. small counts the
// marked ones below dust: one add per such piece, by the thread that numbers it.
struct OpenPieceRoot {
    const int* parent;
    const int* labels;
    int* aux;
    int* small;
    int n_labels;
    long long dust;
    __device__ __forceinline__ bool operator()(size_t v) const {
        if (parent[v] != (int)v || piece_label(labels[v], n_labels) == 0) return false;
        const int c = aux[v];
        return c < 0 || (long long)c >= dust;
    }
    __device__ __forceinline__ void operator()(size_t v, bool flag, int rank) const {
        if (flag) {
            const int c = aux[v];
            if (c < 0 && (long long)(c & ~kOpenMark) < dust) atomicAdd(small, 1);
        }
        aux[v] = flag ? rank + 1 : 0;
    }
};

// ---- streamed slabs -----------------------------------------------------------------
// state words on the device
constexpr int kIdsUsed = 0, kOverflow = 1, kSegments = 2, kSlabIds = 3;

// After sizes: aux[root] |= kSeamMark for every root with an edge across a seam of this slab. carry
// (the previous slab's last plane: z-edge bits, in foreground mode on bits) is NULL for the volume's
// first slab, seam (this slab's last plane, the same) for its last one. parent is flattened.
__global__ __launch_bounds__(kThreads) void seam_mark(const int* __restrict__ parent,
                                                     const unsigned char* __restrict__ mask, int* aux, Dims dm,
                                                     const unsigned char* __restrict__ carry,
                                                     const unsigned char* __restrict__ seam) {
    const size_t hw = (size_t)dm.h * dm.w, last = (size_t)dm.n - hw;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += stride) {
        if (carry && carry[p] && (mask[p] & kBitOn)) atomicOr(aux + parent[p], kSeamMark);
        if (seam && seam[p]) atomicOr(aux + parent[last + p], kSeamMark);
    }
}

// labels holds provisional ids. Joins, in the union-find over ids, the two ends of every on edge
// between the previous slab's last plane (carry_ids, carry) and this slab's first one. An id of 0
// only occurs after an overflow, which finish reports.
__global__ __launch_bounds__(kThreads) void seam_union(const int* __restrict__ labels,
                                                      const unsigned char* __restrict__ mask,
                                                      const int* __restrict__ carry_ids,
                                                      const unsigned char* __restrict__ carry, int* id_parent,
                                                      size_t hw) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += stride) {
        if (!carry[p] || !(mask[p] & kBitOn)) continue;
        const int a = carry_ids[p], b = labels[p];
        if (a > 0 && b > 0) unite<GlobalLoad>(id_parent, a, b);
    }
}

// What the next slab needs of this one: its last plane of ids and of seam bits; and the running id
// count moves on by this slab's ids, saturating at the capacity with the overflow flag raised.
__global__ __launch_bounds__(kThreads) void slab_advance(const int* __restrict__ last_plane,
                                                        const unsigned char* __restrict__ seam,
                                                        int* __restrict__ carry_ids,
                                                        unsigned char* __restrict__ carry, size_t hw, int* state,
                                                        int capacity) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        long long used = (long long)state[kIdsUsed] + state[kSlabIds];
        if (used > capacity) {
            used = capacity;
            state[kOverflow] = 1;
        }
        state[kIdsUsed] = (int)used;
    }
    if (!seam) return;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += stride) {
        carry_ids[p] = last_plane[p];
        carry[p] = seam[p];
    }
}

// ---- the id table after the last slab ----
// id_parent[id] = root(id) for ids 1 .. *ids_used (flatten over ids: no union runs any more)
__global__ __launch_bounds__(kThreads) void table_flatten(int* id_parent, const int* __restrict__ state) {
    const size_t n = (size_t)state[kIdsUsed] + 1;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x + 1; g < n; g += stride) {
        const int p = id_parent[g];
        if (p == (int)g) continue;
        const int r = find_root<GlobalLoad>(id_parent, p);
        if (r != p) id_parent[g] = r;
    }
}

// id_count[root] += id_count[id] for every id that is not a root: 64-bit integer adds, any order
__global__ __launch_bounds__(kThreads) void table_sum(const int* __restrict__ id_parent, long long* id_count,
                                                     const int* __restrict__ state) {
    const size_t n = (size_t)state[kIdsUsed] + 1;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x + 1; g < n; g += stride) {
        const int r = id_parent[g];
        if (r != (int)g)
            atomicAdd(reinterpret_cast<unsigned long long*>(id_count + r), (unsigned long long)id_count[g]);
    }
}

// table[id] = table[root(id)] for the ids that are not roots (scan_assign gave the roots theirs)
__global__ __launch_bounds__(kThreads) void table_spread(const int* __restrict__ id_parent, int* table,
                                                        const int* __restrict__ state) {
    const size_t n = (size_t)state[kIdsUsed] + 1;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x + 1; g < n; g += stride) {
        const int r = id_parent[g];
        if (r != (int)g) table[g] = table[r];
    }
}

// ---- workspace -------------------------------------------------------------------------------
struct Layout {
    size_t aux_off, mask_off, sums_off, bytes;
    long long n_scan_blocks;
};

Layout layout_of(const Dims& dm) {
    Layout l;
    l.n_scan_blocks = ((long long)dm.n + kScanBlock - 1) / kScanBlock;
    l.aux_off = 0;
    l.mask_off = align_up((size_t)dm.n * 4, 256);
    l.sums_off = l.mask_off + align_up((size_t)dm.n, 256);
    l.bytes = l.sums_off + align_up((size_t)l.n_scan_blocks * 4, 256);
    return l;
}

// a streamed slab: the whole-volume layout of its dims, then the plane of seam bits it hands on
struct SlabLayout {
    Layout base;
    size_t seam_off, bytes;
};

SlabLayout slab_layout_of(const Dims& dm) {
    SlabLayout l;
    l.base = layout_of(dm);
    l.seam_off = l.base.bytes;
    l.bytes = l.seam_off + align_up((size_t)dm.h * dm.w, 256);
    return l;
}

// exaspim_fill_holes: the parent array, the two survey words and the mask, 13 bytes per voxel
struct HolesLayout {
    size_t parent_off, lo_off, hi_off, mask_off, bytes;
};

HolesLayout holes_layout_of(const Dims& dm) {
    HolesLayout l;
    const size_t words = align_up((size_t)dm.n * 4, 256);
    l.parent_off = 0;
    l.lo_off = words;
    l.hi_off = 2 * words;
    l.mask_off = 3 * words;
    l.bytes = l.mask_off + align_up((size_t)dm.n, 256);
    return l;
}

// exaspim_label_pieces: the voxel counts, which become the piece numbers, and the scan's block sums; the parent
// array is the caller's output volume
struct PiecesLayout {
    size_t aux_off, sums_off, bytes;
    long long n_scan_blocks;
};

PiecesLayout pieces_layout_of(const Dims& dm) {
    PiecesLayout l;
    l.n_scan_blocks = ((long long)dm.n + kScanBlock - 1) / kScanBlock;
    l.aux_off = 0;
    l.sums_off = align_up((size_t)dm.n * 4, 256);
    l.bytes = l.sums_off + align_up((size_t)l.n_scan_blocks * 4, 256);
    return l;
}

constexpr int kMaxCapacity = 2147483646;   // ids 1 .. capacity, capacity + 1 table entries

long long table_scan_blocks(int capacity) { return ((long long)capacity + 1 + kScanBlock - 1) / kScanBlock; }

// what every streamed entry point checks of the descriptor; NULL if it is sound, else what is wrong
const char* stream_fault(const exaspim_components_stream* st) {
    if (!st) return "NULL stream descriptor";
    if (st->channels != 3 && st->channels != 1) return "channels must be 3 or 1";
    if (st->dims[0] <= 0 || st->dims[1] <= 0 || st->dims[2] <= 0 ||
        (long long)st->dims[1] * st->dims[2] > 2147483647ll)
        return "dims must be positive with dims[1] * dims[2] of at most 2^31 - 1";
    if (st->capacity < 1 || st->capacity > kMaxCapacity) return "capacity must be 1 .. 2^31 - 2";
    if (!st->id_parent_dev || !st->id_count_dev || !st->table_dev || !st->state_dev || !st->seam_ids_dev ||
        !st->seam_bits_dev)
        return "NULL device buffer in the stream descriptor";
    if (((uintptr_t)st->id_parent_dev & 3) || ((uintptr_t)st->id_count_dev & 7) || ((uintptr_t)st->table_dev & 3) ||
        ((uintptr_t)st->state_dev & 3) || ((uintptr_t)st->seam_ids_dev & 3))
        return "misaligned device buffer in the stream descriptor";
    if (st->next_z < 0 || st->next_z > st->dims[0]) return "next_z outside the volume";
    return nullptr;
}

// the size filter's floor: a one-voxel segment has no affinity (img_util.get_affinity_channels), so in
// affinity mode it is background whatever min_size says; in foreground mode an on voxel alone is a
// segment of size 1
int64_t floored_min_size(int channels, int64_t min_size) {
    const int64_t floor_size = channels == 3 ? 1 : 0;
    return min_size < floor_size ? floor_size : min_size;
}

template <typename T>
void launch_edge_mask(const void* src, int channels, unsigned char* mask, const Dims& dm, float thr,
                      hipStream_t stream, unsigned char* seam = nullptr) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const T* p = static_cast<const T*>(src);
    if (channels == 1) {
        edge_mask_foreground<T><<<capped_grid((size_t)dm.n, kThreads), kThreads, 0, stream>>>(p, mask, dm, thr, seam);
    } else if (dm.w % VEC == 0 && ((uintptr_t)src & 15) == 0) {
        edge_mask_affinity<T, VEC><<<capped_grid((size_t)dm.n / VEC, kThreads), kThreads, 0, stream>>>(p, mask, dm, thr, seam);
    } else {
        edge_mask_affinity<T, 1><<<capped_grid((size_t)dm.n, kThreads), kThreads, 0, stream>>>(p, mask, dm, thr, seam);
    }
}

template <typename T>
void launch_watershed_mask(const void* src, unsigned char* mask, const Dims& dm, float low, float high,
                           hipStream_t stream) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const T* p = static_cast<const T*>(src);
    const int tiles_x = (dm.w + kTX - 1) / kTX, tiles_y = (dm.h + kTY - 1) / kTY;
    const long long n_tiles = (long long)tiles_x * tiles_y * ((dm.d + kTZ - 1) / kTZ);
    const unsigned grid = capped_grid((size_t)n_tiles, 1);
    if (dm.w % VEC == 0 && ((uintptr_t)src & 15) == 0)
        edge_mask_watershed<T, VEC><<<grid, kThreads, 0, stream>>>(p, mask, dm, low, high, tiles_x, tiles_y, n_tiles);
    else
        edge_mask_watershed<T, 1><<<grid, kThreads, 0, stream>>>(p, mask, dm, low, high, tiles_x, tiles_y, n_tiles);
}

int clamped_min_size(int64_t ms) { return ms > 2147483647ll ? 2147483647 : (int)ms; }

// passes (b) to (g) of the whole-volume call: the mask (and the zeroed aux) are in the workspace
void label_from_mask(const Dims& dm, const Layout& l, char* ws, int min_eff, int* parent, int* n_segments_dev,
                     hipStream_t s) {
    int* aux = reinterpret_cast<int*>(ws + l.aux_off);
    const unsigned char* mask = reinterpret_cast<const unsigned char*>(ws + l.mask_off);
    int* sums = reinterpret_cast<int*>(ws + l.sums_off);
    const int tiles_x = (dm.w + kTX - 1) / kTX, tiles_y = (dm.h + kTY - 1) / kTY;
    const long long n_tiles = (long long)tiles_x * tiles_y * ((dm.d + kTZ - 1) / kTZ);
    tile_pass<<<capped_grid((size_t)n_tiles, 1), kThreads, 0, s>>>(mask, parent, dm, tiles_x, tiles_y, n_tiles);
    const unsigned grid = capped_grid((size_t)dm.n, kThreads);
    face_merge<<<grid, kThreads, 0, s>>>(mask, parent, dm);
    flatten<<<grid, kThreads, 0, s>>>(parent, dm.n);
    sizes<<<grid, kThreads, 0, s>>>(parent, aux, dm.n);
    const unsigned scan_grid = (unsigned)l.n_scan_blocks;
    const KeptRoot kept{parent, mask, aux, min_eff};
    scan_count<<<scan_grid, kThreads, 0, s>>>(kept, sums, (size_t)dm.n);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(sums, l.n_scan_blocks, n_segments_dev);
    scan_assign<<<scan_grid, kThreads, 0, s>>>(kept, sums, (size_t)dm.n);
    relabel<<<grid, kThreads, 0, s>>>(parent, aux, dm.n);
}

}  // namespace

int launch_fill_holes_passes(const int32_t* labels, const int32_t dims[3], int32_t* out, int64_t* counts,
                             void* workspace, int first, int last, hipStream_t s) {
    Dims dm;
    if (!valid_dims(dims, &dm) || first < 0 || last >= kFillHolesPasses) return EXASPIM_E_INVALID;
    const HolesLayout l = holes_layout_of(dm);
    char* ws = static_cast<char*>(workspace);
    int* parent = reinterpret_cast<int*>(ws + l.parent_off);
    int* lo = reinterpret_cast<int*>(ws + l.lo_off);
    int* hi = reinterpret_cast<int*>(ws + l.hi_off);
    unsigned char* mask = reinterpret_cast<unsigned char*>(ws + l.mask_off);
    const int tiles_x = (dm.w + kTX - 1) / kTX, tiles_y = (dm.h + kTY - 1) / kTY;
    const long long n_tiles = (long long)tiles_x * tiles_y * ((dm.d + kTZ - 1) / kTZ);
    const unsigned grid = capped_grid((size_t)dm.n, kThreads);
    for (int pass = first; pass <= last; ++pass) {
        switch (pass) {
        case 0:
            if (dm.w % 4 == 0 && ((uintptr_t)labels & 15) == 0)
                edge_mask_background<4><<<capped_grid((size_t)dm.n / 4, kThreads), kThreads, 0, s>>>(labels, mask, dm);
            else
                edge_mask_background<1><<<grid, kThreads, 0, s>>>(labels, mask, dm);
            break;
        case 1:
            tile_pass<<<capped_grid((size_t)n_tiles, 1), kThreads, 0, s>>>(mask, parent, dm, tiles_x, tiles_y, n_tiles);
            break;
        case 2:
            face_merge<<<grid, kThreads, 0, s>>>(mask, parent, dm);
            break;
        case 3:
            flatten<<<grid, kThreads, 0, s>>>(parent, dm.n);
            break;
        case 4: {
            EXA_CHECK_HIP(hipMemsetD32Async(lo, kNoLabel, (size_t)dm.n, s));
            EXA_CHECK_HIP(hipMemsetAsync(hi, 0, (size_t)dm.n * 4, s));
            const size_t faces = 2 * ((size_t)dm.h * dm.w + (size_t)dm.d * dm.w + (size_t)dm.d * dm.h);
            survey_faces<<<capped_grid(faces, kThreads), kThreads, 0, s>>>(labels, parent, lo, dm);
            survey<<<grid, kThreads, 0, s>>>(labels, mask, parent, lo, hi, dm);
            break;
        }
        default:
            EXA_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s));
            fill<<<grid, kThreads, 0, s>>>(labels, parent, lo, hi, out, reinterpret_cast<unsigned long long*>(counts),
                                           dm.n);
            break;
        }
    }
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

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
    const int min_eff = clamped_min_size(floored_min_size(channels, min_size));
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace_dev);
    EXA_CHECK_HIP(hipMemsetAsync(ws + l.aux_off, 0, (size_t)dm.n * 4, s));
    unsigned char* mask = reinterpret_cast<unsigned char*>(ws + l.mask_off);
    if (aff_dtype == EXASPIM_AFF_F32)
        launch_edge_mask<float>(aff_dev, channels, mask, dm, threshold, s);
    else
        launch_edge_mask<_Float16>(aff_dev, channels, mask, dm, threshold, s);
    label_from_mask(dm, l, ws, min_eff, labels_dev, n_segments_dev, s);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" size_t exaspim_watershed_workspace_bytes(const int32_t dims[3]) {
    Dims dm;
    if (!valid_dims(dims, &dm)) {
        set_error("watershed_workspace_bytes: dims must be positive with a product of at most 2^31 - 1");
        return 0;
    }
    return layout_of(dm).bytes;
}

extern "C" int exaspim_watershed_fragments(const void* aff_dev, int32_t aff_dtype, const int32_t dims[3],
                                           float low, float high, int64_t min_size, int32_t* labels_dev,
                                           int32_t* n_fragments_dev, void* workspace_dev,
                                           size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(aff_dev && labels_dev && n_fragments_dev && workspace_dev && dims,
                  "watershed_fragments: NULL argument");
    EXA_CHECK_ARG(aff_dtype == EXASPIM_AFF_F32 || aff_dtype == EXASPIM_AFF_F16,
                  "watershed_fragments: aff_dtype %d is neither EXASPIM_AFF_F32 nor EXASPIM_AFF_F16", aff_dtype);
    Dims dm;
    EXA_CHECK_ARG(valid_dims(dims, &dm),
                  "watershed_fragments: dims must be positive with a product of at most 2^31 - 1");
    EXA_CHECK_ARG(low == low && high == high, "watershed_fragments: low or high is a NaN");
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && ((uintptr_t)labels_dev & 3) == 0 &&
                      ((uintptr_t)aff_dev & (aff_dtype == EXASPIM_AFF_F32 ? 3 : 1)) == 0,
                  "watershed_fragments: misaligned buffer");
    const Layout l = layout_of(dm);
    if (workspace_bytes < l.bytes) {
        set_error("watershed_fragments: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
        return EXASPIM_E_WORKSPACE;
    }
    const int min_eff = clamped_min_size(floored_min_size(3, min_size));
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace_dev);
    EXA_CHECK_HIP(hipMemsetAsync(ws + l.aux_off, 0, (size_t)dm.n * 4, s));
    unsigned char* mask = reinterpret_cast<unsigned char*>(ws + l.mask_off);
    if (aff_dtype == EXASPIM_AFF_F32)
        launch_watershed_mask<float>(aff_dev, mask, dm, low, high, s);
    else
        launch_watershed_mask<_Float16>(aff_dev, mask, dm, low, high, s);
    label_from_mask(dm, l, ws, min_eff, labels_dev, n_fragments_dev, s);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" size_t exaspim_fill_holes_workspace_bytes(const int32_t dims[3]) {
    Dims dm;
    if (!valid_dims(dims, &dm)) {
        set_error("fill_holes_workspace_bytes: dims must be positive with a product of at most 2^31 - 1");
        return 0;
    }
    return holes_layout_of(dm).bytes;
}

extern "C" int exaspim_fill_holes(const int32_t* labels_dev, const int32_t dims[3], int32_t* out_dev,
                                  int64_t* counts_dev, void* workspace_dev, size_t workspace_bytes,
                                  void* stream) {
    EXA_CHECK_ARG(labels_dev && dims && out_dev && counts_dev && workspace_dev, "fill_holes: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(valid_dims(dims, &dm), "fill_holes: dims must be positive with a product of at most 2^31 - 1");
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && ((uintptr_t)counts_dev & 7) == 0 &&
                      (((uintptr_t)labels_dev | (uintptr_t)out_dev) & 3) == 0,
                  "fill_holes: misaligned buffer");
    const size_t need = holes_layout_of(dm).bytes;
    if (workspace_bytes < need) {
        set_error("fill_holes: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    return launch_fill_holes_passes(labels_dev, dims, out_dev, counts_dev, workspace_dev, 0, kFillHolesPasses - 1,
                                    (hipStream_t)stream);
}

extern "C" size_t exaspim_label_pieces_workspace_bytes(const int32_t dims[3]) {
    Dims dm;
    if (!valid_dims(dims, &dm)) {
        set_error("label_pieces_workspace_bytes: dims must be positive with a product of at most 2^31 - 1");
        return 0;
    }
    return pieces_layout_of(dm).bytes;
}

extern "C" int exaspim_label_pieces(const int32_t* labels_dev, const int32_t dims[3], int32_t n_labels,
                                    int64_t dust_threshold, int32_t* pieces_dev, int32_t* state_dev,
                                    void* workspace_dev, size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && dims && pieces_dev && state_dev && workspace_dev, "label_pieces: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(valid_dims(dims, &dm), "label_pieces: dims must be positive with a product of at most 2^31 - 1");
    EXA_CHECK_ARG(n_labels >= 0, "label_pieces: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(dust_threshold >= 0, "label_pieces: dust_threshold must not be negative, got %lld",
                  (long long)dust_threshold);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 &&
                      (((uintptr_t)labels_dev | (uintptr_t)pieces_dev | (uintptr_t)state_dev) & 3) == 0,
                  "label_pieces: misaligned buffer");
    EXA_CHECK_ARG(pieces_dev != labels_dev, "label_pieces: pieces_dev must not be labels_dev");
    const PiecesLayout l = pieces_layout_of(dm);
    if (workspace_bytes < l.bytes) {
        set_error("label_pieces: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace_dev);
    int* aux = reinterpret_cast<int*>(ws + l.aux_off);
    int* sums = reinterpret_cast<int*>(ws + l.sums_off);
    int* parent = pieces_dev;
    EXA_CHECK_HIP(hipMemsetAsync(aux, 0, (size_t)dm.n * 4, s));
    EXA_CHECK_HIP(hipMemsetAsync(state_dev, 0, 2 * sizeof(int32_t), s));
    const int tiles_x = (dm.w + kTX - 1) / kTX, tiles_y = (dm.h + kTY - 1) / kTY;
    const long long n_tiles = (long long)tiles_x * tiles_y * ((dm.d + kTZ - 1) / kTZ);
    pieces_tile_pass<<<capped_grid((size_t)n_tiles, 1), kThreads, 0, s>>>(labels_dev, parent, aux, dm, n_labels,
                                                                          tiles_x, tiles_y, n_tiles);
    const unsigned grid = capped_grid((size_t)dm.n, kThreads);
    pieces_seam_merge<<<grid, kThreads, 0, s>>>(labels_dev, parent, dm, n_labels);
    flatten<<<grid, kThreads, 0, s>>>(parent, dm.n);
    pieces_sizes<<<grid, kThreads, 0, s>>>(parent, aux, dm.n);
    const unsigned scan_grid = (unsigned)l.n_scan_blocks;
    const PieceRoot kept{parent, labels_dev, aux, n_labels, (long long)dust_threshold};
    scan_count<<<scan_grid, kThreads, 0, s>>>(kept, sums, (size_t)dm.n);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(sums, l.n_scan_blocks, state_dev);
    scan_assign<<<scan_grid, kThreads, 0, s>>>(kept, sums, (size_t)dm.n);
    pieces_relabel<<<grid, kThreads, 0, s>>>(labels_dev, parent, aux, state_dev + 1, n_labels, dm.n);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" size_t exaspim_label_pieces_open_workspace_bytes(const int32_t dims[3]) {
    Dims dm;
    if (!valid_dims(dims, &dm)) {
        set_error("label_pieces_open_workspace_bytes: dims must be positive with a product of at most 2^31 - 1");
        return 0;
    }
    return pieces_layout_of(dm).bytes;
}

extern "C" int exaspim_label_pieces_open(const int32_t* labels_dev, const int32_t dims[3], int32_t n_labels,
                                         int64_t dust_threshold, uint32_t open_faces, int32_t* pieces_dev,
                                         int32_t* state_dev, void* workspace_dev, size_t workspace_bytes,
                                         void* stream) {
    EXA_CHECK_ARG(labels_dev && dims && pieces_dev && state_dev && workspace_dev, "label_pieces_open: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(valid_dims(dims, &dm),
                  "label_pieces_open: dims must be positive with a product of at most 2^31 - 1");
    EXA_CHECK_ARG(n_labels >= 0, "label_pieces_open: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(dust_threshold >= 0, "label_pieces_open: dust_threshold must not be negative, got %lld",
                  (long long)dust_threshold);
    EXA_CHECK_ARG(open_faces < 64u, "label_pieces_open: open_faces has six bits, got %u", open_faces);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 &&
                      (((uintptr_t)labels_dev | (uintptr_t)pieces_dev | (uintptr_t)state_dev) & 3) == 0,
                  "label_pieces_open: misaligned buffer");
    EXA_CHECK_ARG(pieces_dev != labels_dev, "label_pieces_open: pieces_dev must not be labels_dev");
    const PiecesLayout l = pieces_layout_of(dm);
    if (workspace_bytes < l.bytes) {
        set_error("label_pieces_open: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace_dev);
    int* aux = reinterpret_cast<int*>(ws + l.aux_off);
    int* sums = reinterpret_cast<int*>(ws + l.sums_off);
    int* parent = pieces_dev;
    EXA_CHECK_HIP(hipMemsetAsync(aux, 0, (size_t)dm.n * 4, s));
    EXA_CHECK_HIP(hipMemsetAsync(state_dev, 0, 3 * sizeof(int32_t), s));
    const int tiles_x = (dm.w + kTX - 1) / kTX, tiles_y = (dm.h + kTY - 1) / kTY;
    const long long n_tiles = (long long)tiles_x * tiles_y * ((dm.d + kTZ - 1) / kTZ);
    pieces_tile_pass<<<capped_grid((size_t)n_tiles, 1), kThreads, 0, s>>>(labels_dev, parent, aux, dm, n_labels,
                                                                          tiles_x, tiles_y, n_tiles);
    const unsigned grid = capped_grid((size_t)dm.n, kThreads);
    pieces_seam_merge<<<grid, kThreads, 0, s>>>(labels_dev, parent, dm, n_labels);
    flatten<<<grid, kThreads, 0, s>>>(parent, dm.n);
    pieces_sizes<<<grid, kThreads, 0, s>>>(parent, aux, dm.n);
    if (open_faces) {
        const OpenPlanes op = open_planes_of(dm, open_faces);
        const unsigned open_grid = std::min(capped_grid((size_t)op.first[6], kThreads), kOpenGrid);
        pieces_mark_open<<<open_grid, kThreads, 0, s>>>(labels_dev, parent, aux, dm, n_labels, op);
    }
    const unsigned scan_grid = (unsigned)l.n_scan_blocks;
    const OpenPieceRoot kept{parent, labels_dev, aux, state_dev + 2, n_labels, (long long)dust_threshold};
    scan_count<<<scan_grid, kThreads, 0, s>>>(kept, sums, (size_t)dm.n);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(sums, l.n_scan_blocks, state_dev);
    scan_assign<<<scan_grid, kThreads, 0, s>>>(kept, sums, (size_t)dm.n);
    pieces_relabel<<<grid, kThreads, 0, s>>>(labels_dev, parent, aux, state_dev + 1, n_labels, dm.n);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

// ---- the streamed form ---------------------------------------------------------------------------
extern "C" size_t exaspim_components_stream_slab_workspace_bytes(const int32_t slab_dims[3]) {
    Dims dm;
    if (!valid_dims(slab_dims, &dm)) {
        set_error("components_stream_slab_workspace_bytes: dims must be positive with a product of at most 2^31 - 1");
        return 0;
    }
    return slab_layout_of(dm).bytes;
}

extern "C" size_t exaspim_components_stream_finish_workspace_bytes(int32_t capacity) {
    if (capacity < 1 || capacity > kMaxCapacity) {
        set_error("components_stream_finish_workspace_bytes: capacity must be 1 .. 2^31 - 2");
        return 0;
    }
    return align_up((size_t)table_scan_blocks(capacity) * 4, 256);
}

extern "C" int exaspim_components_stream_slab(exaspim_components_stream* st, const void* aff_dev,
                                              int32_t aff_dtype, const int32_t slab_dims[3], int32_t z0,
                                              int32_t* labels_dev, void* workspace_dev, size_t workspace_bytes,
                                              void* stream) {
    const char* fault = stream_fault(st);
    EXA_CHECK_ARG(!fault, "components_stream_slab: %s", fault);
    EXA_CHECK_ARG(aff_dev && labels_dev && workspace_dev && slab_dims, "components_stream_slab: NULL argument");
    EXA_CHECK_ARG(aff_dtype == EXASPIM_AFF_F32 || aff_dtype == EXASPIM_AFF_F16,
                  "components_stream_slab: aff_dtype %d is neither EXASPIM_AFF_F32 nor EXASPIM_AFF_F16", aff_dtype);
    Dims dm;
    EXA_CHECK_ARG(valid_dims(slab_dims, &dm),
                  "components_stream_slab: slab dims must be positive with a product of at most 2^31 - 1");
    EXA_CHECK_ARG(dm.h == st->dims[1] && dm.w == st->dims[2],
                  "components_stream_slab: the slab is %d x %d in (y, x), the volume %d x %d", dm.h, dm.w,
                  st->dims[1], st->dims[2]);
    EXA_CHECK_ARG(z0 == st->next_z, "components_stream_slab: slabs go in z order, the next one starts at %d, not %d",
                  st->next_z, z0);
    EXA_CHECK_ARG((long long)z0 + dm.d <= st->dims[0],
                  "components_stream_slab: planes [%d, %lld) leave the volume of depth %d", z0, (long long)z0 + dm.d,
                  st->dims[0]);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && ((uintptr_t)labels_dev & 3) == 0 &&
                      ((uintptr_t)aff_dev & (aff_dtype == EXASPIM_AFF_F32 ? 3 : 1)) == 0,
                  "components_stream_slab: misaligned buffer");
    const SlabLayout l = slab_layout_of(dm);
    if (workspace_bytes < l.bytes) {
        set_error("components_stream_slab: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
        return EXASPIM_E_WORKSPACE;
    }
    const int64_t ms = floored_min_size(st->channels, st->min_size);
    const int min_eff = ms > 2147483647ll ? 2147483647 : (int)ms;
    const bool first = z0 == 0, last = z0 + dm.d == st->dims[0];

    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace_dev);
    int* aux = reinterpret_cast<int*>(ws + l.base.aux_off);
    unsigned char* mask = reinterpret_cast<unsigned char*>(ws + l.base.mask_off);
    int* sums = reinterpret_cast<int*>(ws + l.base.sums_off);
    unsigned char* seam = last ? nullptr : reinterpret_cast<unsigned char*>(ws + l.seam_off);
    const unsigned char* carry = first ? nullptr : st->seam_bits_dev;
    int* parent = labels_dev;
    const size_t hw = (size_t)dm.h * dm.w;

    if (first) {   // a new volume: no ids yet, id 0 is the background's
        EXA_CHECK_HIP(hipMemsetAsync(st->state_dev, 0, 4 * sizeof(int32_t), s));
        EXA_CHECK_HIP(hipMemsetAsync(st->id_parent_dev, 0, sizeof(int32_t), s));
        EXA_CHECK_HIP(hipMemsetAsync(st->id_count_dev, 0, sizeof(int64_t), s));
    }
    EXA_CHECK_HIP(hipMemsetAsync(aux, 0, (size_t)dm.n * 4, s));
    if (aff_dtype == EXASPIM_AFF_F32)
        launch_edge_mask<float>(aff_dev, st->channels, mask, dm, st->threshold, s, seam);
    else
        launch_edge_mask<_Float16>(aff_dev, st->channels, mask, dm, st->threshold, s, seam);
    const int tiles_x = (dm.w + kTX - 1) / kTX, tiles_y = (dm.h + kTY - 1) / kTY;
    const long long n_tiles = (long long)tiles_x * tiles_y * ((dm.d + kTZ - 1) / kTZ);
    tile_pass<<<capped_grid((size_t)n_tiles, 1), kThreads, 0, s>>>(mask, parent, dm, tiles_x, tiles_y, n_tiles);
    const unsigned grid = capped_grid((size_t)dm.n, kThreads), plane_grid = capped_grid(hw, kThreads);
    face_merge<<<grid, kThreads, 0, s>>>(mask, parent, dm);
    flatten<<<grid, kThreads, 0, s>>>(parent, dm.n);
    sizes<<<grid, kThreads, 0, s>>>(parent, aux, dm.n);
    if (carry || seam) seam_mark<<<plane_grid, kThreads, 0, s>>>(parent, mask, aux, dm, carry, seam);
    const SlabRoot ids{parent, mask, aux, min_eff, st->state_dev + kIdsUsed, st->capacity, st->id_parent_dev,
                       reinterpret_cast<long long*>(st->id_count_dev)};
    const unsigned scan_grid = (unsigned)l.base.n_scan_blocks;
    scan_count<<<scan_grid, kThreads, 0, s>>>(ids, sums, (size_t)dm.n);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(sums, l.base.n_scan_blocks, st->state_dev + kSlabIds);
    scan_assign<<<scan_grid, kThreads, 0, s>>>(ids, sums, (size_t)dm.n);
    relabel<<<grid, kThreads, 0, s>>>(parent, aux, dm.n);
    if (carry) seam_union<<<plane_grid, kThreads, 0, s>>>(parent, mask, st->seam_ids_dev, carry, st->id_parent_dev, hw);
    slab_advance<<<seam ? plane_grid : 1, kThreads, 0, s>>>(parent + ((size_t)dm.n - hw), seam, st->seam_ids_dev,
                                                           st->seam_bits_dev, hw, st->state_dev, st->capacity);
    EXA_CHECK_HIP(hipGetLastError());
    st->next_z = z0 + dm.d;
    return EXASPIM_OK;
}

extern "C" int exaspim_components_stream_finish(const exaspim_components_stream* st, void* workspace_dev,
                                                size_t workspace_bytes, void* stream) {
    const char* fault = stream_fault(st);
    EXA_CHECK_ARG(!fault, "components_stream_finish: %s", fault);
    EXA_CHECK_ARG(st->next_z == st->dims[0], "components_stream_finish: %d of %d planes have been pushed",
                  st->next_z, st->dims[0]);
    EXA_CHECK_ARG(workspace_dev && ((uintptr_t)workspace_dev & 15) == 0,
                  "components_stream_finish: NULL or misaligned workspace");
    const long long n_blocks = table_scan_blocks(st->capacity);
    const size_t need = align_up((size_t)n_blocks * 4, 256);
    if (workspace_bytes < need) {
        set_error("components_stream_finish: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    int* sums = static_cast<int*>(workspace_dev);
    long long* counts = reinterpret_cast<long long*>(st->id_count_dev);
    const size_t entries = (size_t)st->capacity + 1;
    const unsigned grid = capped_grid(entries, kThreads);
    table_flatten<<<grid, kThreads, 0, s>>>(st->id_parent_dev, st->state_dev);
    table_sum<<<grid, kThreads, 0, s>>>(st->id_parent_dev, counts, st->state_dev);
    const TableRoot roots{st->id_parent_dev, counts, st->state_dev + kIdsUsed,
                          (long long)floored_min_size(st->channels, st->min_size), st->table_dev};
    scan_count<<<(unsigned)n_blocks, kThreads, 0, s>>>(roots, sums, entries);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(sums, n_blocks, st->state_dev + kSegments);
    scan_assign<<<(unsigned)n_blocks, kThreads, 0, s>>>(roots, sums, entries);
    table_spread<<<grid, kThreads, 0, s>>>(st->id_parent_dev, st->table_dev, st->state_dev);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

extern "C" int exaspim_components_stream_apply(const exaspim_components_stream* st, int32_t* labels_dev, size_t n,
                                               void* stream) {
    const char* fault = stream_fault(st);
    EXA_CHECK_ARG(!fault, "components_stream_apply: %s", fault);
    EXA_CHECK_ARG(labels_dev && ((uintptr_t)labels_dev & 3) == 0, "components_stream_apply: NULL or misaligned labels");
    if (n == 0) return EXASPIM_OK;
    apply_table<<<capped_grid((n + 3) / 4, kThreads), kThreads, 0, (hipStream_t)stream>>>(labels_dev, st->table_dev,
                                                                                        st->capacity, n);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

// ---- watershed fragments of a volume that arrives in z slabs -----------------------------------
namespace exaspim {
namespace {

template <typename T>
void launch_watershed_slab_mask(const void* src, unsigned char* mask, const Dims& dm, float low, float high,
                                const SlabSeam& sm, float* seam_aff, hipStream_t stream) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const T* p = static_cast<const T*>(src);
    const size_t hw = (size_t)dm.h * dm.w;
    const int tiles_x = (dm.w + kTX - 1) / kTX, tiles_y = (dm.h + kTY - 1) / kTY;
    const long long n_tiles = (long long)tiles_x * tiles_y * ((dm.d + kTZ - 1) / kTZ);
    const unsigned grid = capped_grid((size_t)n_tiles, 1);
    // the carried plane of affinities is read in 16-byte groups as well
    if (dm.w % VEC == 0 && (((uintptr_t)src | (uintptr_t)sm.carry_aff) & 15) == 0)
        edge_mask_watershed_slab<T, VEC><<<grid, kThreads, 0, stream>>>(p, mask, dm, low, high, tiles_x, tiles_y,
                                                                        n_tiles, sm);
    else
        edge_mask_watershed_slab<T, 1><<<grid, kThreads, 0, stream>>>(p, mask, dm, low, high, tiles_x, tiles_y,
                                                                      n_tiles, sm);
    if (sm.seam)
        seam_affinity<T><<<capped_grid(hw, kThreads), kThreads, 0, stream>>>(p + ((size_t)dm.n - hw), seam_aff, hw);
}

}  // namespace
}  // namespace exaspim

extern "C" size_t exaspim_watershed_stream_slab_workspace_bytes(const int32_t slab_dims[3]) {
    Dims dm;
    if (!valid_dims(slab_dims, &dm)) {
        set_error("watershed_stream_slab_workspace_bytes: dims must be positive with a product of at most 2^31 - 1");
        return 0;
    }
    return slab_layout_of(dm).bytes;
}

extern "C" int exaspim_watershed_stream_slab(exaspim_watershed_stream* wst, const void* aff_dev, int32_t aff_dtype,
                                             const int32_t slab_dims[3], int32_t z0, int32_t* labels_dev,
                                             void* workspace_dev, size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(wst, "watershed_stream_slab: NULL stream descriptor");
    exaspim_components_stream* st = &wst->base;
    const char* fault = stream_fault(st);
    EXA_CHECK_ARG(!fault, "watershed_stream_slab: %s", fault);
    EXA_CHECK_ARG(st->channels == 3, "watershed_stream_slab: channels must be 3, got %d", st->channels);
    EXA_CHECK_ARG(wst->seam_aff_dev && ((uintptr_t)wst->seam_aff_dev & 3) == 0,
                  "watershed_stream_slab: NULL or misaligned seam_aff_dev");
    EXA_CHECK_ARG(wst->low == wst->low && wst->high == wst->high, "watershed_stream_slab: low or high is a NaN");
    EXA_CHECK_ARG(aff_dev && labels_dev && workspace_dev && slab_dims, "watershed_stream_slab: NULL argument");
    EXA_CHECK_ARG(aff_dtype == EXASPIM_AFF_F32 || aff_dtype == EXASPIM_AFF_F16,
                  "watershed_stream_slab: aff_dtype %d is neither EXASPIM_AFF_F32 nor EXASPIM_AFF_F16", aff_dtype);
    Dims dm;
    EXA_CHECK_ARG(valid_dims(slab_dims, &dm),
                  "watershed_stream_slab: slab dims must be positive with a product of at most 2^31 - 1");
    EXA_CHECK_ARG(dm.h == st->dims[1] && dm.w == st->dims[2],
                  "watershed_stream_slab: the slab is %d x %d in (y, x), the volume %d x %d", dm.h, dm.w,
                  st->dims[1], st->dims[2]);
    EXA_CHECK_ARG(z0 == st->next_z, "watershed_stream_slab: slabs go in z order, the next one starts at %d, not %d",
                  st->next_z, z0);
    EXA_CHECK_ARG((long long)z0 + dm.d <= st->dims[0],
                  "watershed_stream_slab: planes [%d, %lld) leave the volume of depth %d", z0, (long long)z0 + dm.d,
                  st->dims[0]);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && ((uintptr_t)labels_dev & 3) == 0 &&
                      ((uintptr_t)aff_dev & (aff_dtype == EXASPIM_AFF_F32 ? 3 : 1)) == 0,
                  "watershed_stream_slab: misaligned buffer");
    const SlabLayout l = slab_layout_of(dm);
    if (workspace_bytes < l.bytes) {
        set_error("watershed_stream_slab: workspace of %zu bytes, %zu needed", workspace_bytes, l.bytes);
        return EXASPIM_E_WORKSPACE;
    }
    const int min_eff = clamped_min_size(floored_min_size(3, st->min_size));
    const bool first = z0 == 0, last = z0 + dm.d == st->dims[0];

    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace_dev);
    int* aux = reinterpret_cast<int*>(ws + l.base.aux_off);
    unsigned char* mask = reinterpret_cast<unsigned char*>(ws + l.base.mask_off);
    int* sums = reinterpret_cast<int*>(ws + l.base.sums_off);
    // seam: this slab's eligible and sure bits, every eligible one a mark on the lower side (the upper end's
    // choice is not known yet); carry: the previous slab's, resolved by the mask kernel to on or off
    unsigned char* seam = last ? nullptr : reinterpret_cast<unsigned char*>(ws + l.seam_off);
    unsigned char* carry = first ? nullptr : st->seam_bits_dev;
    int* parent = labels_dev;
    const size_t hw = (size_t)dm.h * dm.w;

    if (first) {   // a new volume: no ids yet, id 0 is the background's
        EXA_CHECK_HIP(hipMemsetAsync(st->state_dev, 0, 4 * sizeof(int32_t), s));
        EXA_CHECK_HIP(hipMemsetAsync(st->id_parent_dev, 0, sizeof(int32_t), s));
        EXA_CHECK_HIP(hipMemsetAsync(st->id_count_dev, 0, sizeof(int64_t), s));
    }
    EXA_CHECK_HIP(hipMemsetAsync(aux, 0, (size_t)dm.n * 4, s));
    const SlabSeam sm{first ? nullptr : wst->seam_aff_dev, carry, seam};
    if (aff_dtype == EXASPIM_AFF_F32)
        launch_watershed_slab_mask<float>(aff_dev, mask, dm, wst->low, wst->high, sm, wst->seam_aff_dev, s);
    else
        launch_watershed_slab_mask<_Float16>(aff_dev, mask, dm, wst->low, wst->high, sm, wst->seam_aff_dev, s);
    const int tiles_x = (dm.w + kTX - 1) / kTX, tiles_y = (dm.h + kTY - 1) / kTY;
    const long long n_tiles = (long long)tiles_x * tiles_y * ((dm.d + kTZ - 1) / kTZ);
    tile_pass<<<capped_grid((size_t)n_tiles, 1), kThreads, 0, s>>>(mask, parent, dm, tiles_x, tiles_y, n_tiles);
    const unsigned grid = capped_grid((size_t)dm.n, kThreads), plane_grid = capped_grid(hw, kThreads);
    face_merge<<<grid, kThreads, 0, s>>>(mask, parent, dm);
    flatten<<<grid, kThreads, 0, s>>>(parent, dm.n);
    sizes<<<grid, kThreads, 0, s>>>(parent, aux, dm.n);
    if (carry || seam) seam_mark<<<plane_grid, kThreads, 0, s>>>(parent, mask, aux, dm, carry, seam);
    const SlabRoot ids{parent, mask, aux, min_eff, st->state_dev + kIdsUsed, st->capacity, st->id_parent_dev,
                       reinterpret_cast<long long*>(st->id_count_dev)};
    const unsigned scan_grid = (unsigned)l.base.n_scan_blocks;
    scan_count<<<scan_grid, kThreads, 0, s>>>(ids, sums, (size_t)dm.n);
    scan_block_sums<<<1, kSumThreads, 0, s>>>(sums, l.base.n_scan_blocks, st->state_dev + kSlabIds);
    scan_assign<<<scan_grid, kThreads, 0, s>>>(ids, sums, (size_t)dm.n);
    relabel<<<grid, kThreads, 0, s>>>(parent, aux, dm.n);
    if (carry) seam_union<<<plane_grid, kThreads, 0, s>>>(parent, mask, st->seam_ids_dev, carry, st->id_parent_dev, hw);
    slab_advance<<<seam ? plane_grid : 1, kThreads, 0, s>>>(parent + ((size_t)dm.n - hw), seam, st->seam_ids_dev,
                                                           st->seam_bits_dev, hw, st->state_dev, st->capacity);
    EXA_CHECK_HIP(hipGetLastError());
    st->next_z = z0 + dm.d;
    return EXASPIM_OK;
}
