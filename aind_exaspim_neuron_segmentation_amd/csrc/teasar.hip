// TEASAR's loop for every label at once (exaspim_teasar_begin, _round, _apply; semantics in
// include/exaspim_affinity.h). DESIGN 6n. The single-parental-field form: every path is read off one
// parental field (kimimaro's fix_branching=False), a branch stops at its junction with the skeleton, and
// only the cubes around the new vertices are invalidated, each minus the cube of the vertex before it.
// Integers and bit patterns only; the one piece of floating point, the radius, is three rounded double
// operations (the file is built with -ffp-contract=off, FLAGS_teasar in the Makefile).
//
// One byte of state per voxel: bit 0 "still valid", bit 1 "on the skeleton".
//
//   teasar_init            the state byte of every voxel from labels, sources, hops and daf; the counters and
//                          the per-label "finished" words cleared.
//   teasar_round_init      the keys and the round's counters cleared.
//   teasar_targets         geodesic.hip's far_pass over the valid voxels: the state byte is read first,
//                          labels and daf only where it says valid, a wave without a valid voxel does nothing
//                          more; a 64-bit atomic maximum of (daf bits, 2^32 - 1 - index) per label, runs of
//                          equal labels reduced inside a wave first.
//   teasar_branch_lengths  one thread per label: the target from the key, then the walk along parents to the
//                          first skeleton voxel or the source, at most hops[target] steps, every index
//                          range-checked; the number of new vertices, the junction, and the counters.
//   teasar_given_lengths   exaspim_teasar_round_given's form of teasar_branch_lengths: a label whose
//                          row of "given" is not -1 takes that voxel as its target if it is an eligible voxel of
//                          the label, whether it is still valid or not; a row that is not is counted in the sixth
//                          state word and read as -1; a given target on the skeleton is no branch.
//   teasar_branch_write    one thread per label: the same walk, now writing voxels, radii and each entry's
//                          previous vertex back to front, and setting the skeleton bit.
//   teasar_invalidate<ROOTS>  the hot path. ROOTS = false: grid x over the round's new vertices, grid y over
//                          the items of one vertex: the vertex's cube minus the previous vertex's cube, both
//                          clipped to the volume and the label's box, as at most six disjoint slabs whose
//                          voxels are numbered along x first, so a wave reads state bytes and labels of
//                          consecutive addresses. ROOTS = true: grid x over the labels whose branch has no
//                          junction (round 1), whose first vertex has a whole cube, spread over a large grid y.
//                          A byte is read, and if it says valid and the label matches, written back with bit 0
//                          clear: two writers of one byte write the same value, and bit 1 does not change
//                          during the launch.
#include <cmath>

#include "label_scan.h"

namespace exaspim {
namespace {

constexpr unsigned kInfBits = 0x7F800000u;
constexpr unsigned char kValid = 1, kSkeleton = 2;
constexpr int kStateWords = 5;       // live, broken, new vertices, branches without a junction, refused rows
constexpr int kGivenWord = 5;        // exaspim_teasar_round_given's sixth word: the given targets it refused
constexpr unsigned kDiffGridY = 4;   // a difference of two cubes is a few faces
// a whole cube may be the whole bounding box: about 2^18 workgroups over the labels and a cube's items
unsigned root_grid_y(int n_labels) {
    const unsigned y = 262144u / (unsigned)(n_labels > 0 ? n_labels : 1);
    return y < 4 ? 4 : (y > 1024 ? 1024 : y);
}

size_t keys_bytes(int n_labels) { return align_up(((size_t)n_labels + 1) * sizeof(unsigned long long), 16); }
size_t workspace_need(int n_labels) { return keys_bytes(n_labels) + align_up(((size_t)n_labels + 1) * sizeof(int), 16); }

__device__ __forceinline__ bool valid_source(const int* __restrict__ labels, const int* __restrict__ sources, int l,
                                             int n) {
    const int s = sources[l];
    return s >= 0 && s < n && labels[s] == l;
}

__global__ __launch_bounds__(kThreads) void teasar_init(const int* __restrict__ labels, const int* __restrict__ sources,
                                                       const int* __restrict__ hops, const float* __restrict__ daf,
                                                       int n, int n_labels, unsigned char* __restrict__ mask, int* state,
                                                       int* finished) {
    const size_t step = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (first < (size_t)kStateWords) state[first] = 0;
    for (size_t r = first; r <= (size_t)n_labels; r += step) finished[r] = 0;
    for (size_t v = first; v < (size_t)n; v += step) {
        const int l = labels[v];
        bool ok = l >= 1 && l <= n_labels && hops[v] >= 0 && __float_as_uint(daf[v]) < kInfBits;
        ok = ok && valid_source(labels, sources, l, n);
        mask[v] = ok ? kValid : 0;
    }
}

__global__ __launch_bounds__(kThreads) void teasar_round_init(unsigned long long* keys, size_t rows, int* state,
                                                             bool given) {
    const size_t step = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (first < 4) state[first] = 0;   // the refused rows of exaspim_teasar_apply add up over the rounds
    if (given && first == (size_t)kGivenWord) state[first] = 0;
    for (size_t r = first; r < rows; r += step) keys[r] = 0;
}

__global__ __launch_bounds__(kThreads) void teasar_targets(const unsigned char* __restrict__ mask,
                                                          const int* __restrict__ labels,
                                                          const float* __restrict__ daf, size_t n, int n_labels,
                                                          unsigned long long* keys) {
    const int lane = threadIdx.x & 63;
    const size_t step = (size_t)gridDim.x * kThreads;
    // the trip count is the same in every lane of the workgroup: the shuffles below see all 64
    for (size_t base = (size_t)blockIdx.x * kThreads; base < n; base += step) {
        const size_t v = base + threadIdx.x;
        const bool valid = v < n && (mask[v] & kValid);
        if (__ballot(valid) == 0) continue;   // uniform over the wave: an invalid voxel costs its byte
        int l = -1;
        unsigned long long key = 0;
        if (valid) {
            l = labels[v];
            const unsigned bits = __float_as_uint(daf[v]);
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

// The walk of step (2) from "target" along parents to the first skeleton voxel or the source: at most
// hops[target] steps, whatever parents holds. Returns false for a broken walk.
__device__ __forceinline__ bool walk_branch(int target, const int* __restrict__ parents, const int* __restrict__ hops,
                                            const unsigned char* __restrict__ mask, int n, long long* count,
                                            int* junc) {
    const int h = hops[target];
    bool broken = h < 0;
    int cur = target;
    for (int k = h; k >= 0; --k) {
        if (mask[cur] & kSkeleton) {
            *junc = cur;
            break;
        }
        ++*count;
        const int p = parents[cur];
        if (k == 0) {
            broken = p != cur;   // without a junction the walk ends on a self-parent, the source
            break;
        }
        if (p < 0 || p >= n || p == cur) {
            broken = true;
            break;
        }
        cur = p;
    }
    return !broken;
}

// the walk's outcome into the label's rows and the round's counters
__device__ __forceinline__ void count_branch(bool whole, size_t r, int* target, long long* count, int* junc,
                                             int* finished, int* state) {
    if (!whole) {
        atomicAdd(state + 1, 1);
        finished[r] = 1;
        *target = *junc = -1;
        *count = 0;
    } else {
        atomicAdd(state + 0, 1);
        atomicAdd(state + 2, (int)*count);
        if (*junc < 0) atomicAdd(state + 3, 1);
    }
}

__global__ __launch_bounds__(kThreads) void teasar_branch_lengths(const unsigned long long* __restrict__ keys,
                                                                 const int* __restrict__ parents,
                                                                 const int* __restrict__ hops,
                                                                 const unsigned char* __restrict__ mask, int n,
                                                                 int n_labels, int* __restrict__ targets,
                                                                 long long* __restrict__ lengths,
                                                                 int* __restrict__ junction, int* finished, int* state) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r <= (size_t)n_labels; r += step) {
        const unsigned long long key = keys[r];
        int target = -1, junc = -1;
        long long count = 0;
        if (r > 0 && (key >> 63) && !finished[r]) {
            target = (int)(0xFFFFFFFFu - (unsigned)key);   // below n: the key was made from a voxel's index
            const bool whole = walk_branch(target, parents, hops, mask, n, &count, &junc);
            count_branch(whole, r, &target, &count, &junc, finished, state);
        }
        targets[r] = target;
        lengths[r] = count;
        junction[r] = junc;
    }
}

// teasar_branch_lengths with this round's given target per label: given[r] == -1 leaves the label to its key.
// Any other row must name an eligible voxel of label r, or it is counted in state[kGivenWord] and read as -1.
// A given target that is on the skeleton already is no branch: the label has none this round, is not counted
// and is not finished.
__global__ __launch_bounds__(kThreads) void teasar_given_lengths(
    const unsigned long long* __restrict__ keys, const int* __restrict__ given, const int* __restrict__ labels,
    const float* __restrict__ daf, const int* __restrict__ parents, const int* __restrict__ hops,
    const unsigned char* __restrict__ mask, int n, int n_labels, int* __restrict__ targets,
    long long* __restrict__ lengths, int* __restrict__ junction, int* finished, int* state) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r <= (size_t)n_labels; r += step) {
        const unsigned long long key = keys[r];
        int target = -1, junc = -1;
        long long count = 0;
        if (r > 0 && !finished[r]) {
            int g = given[r];
            if (g != -1) {
                const bool ok = g >= 0 && g < n && labels[g] == (int)r && hops[g] >= 0 &&
                                __float_as_uint(daf[g]) < kInfBits;
                if (!ok) {
                    atomicAdd(state + kGivenWord, 1);
                    g = -1;
                }
            }
            if (g >= 0) {
                if (!(mask[g] & kSkeleton)) {
                    target = g;
                    const bool whole = walk_branch(target, parents, hops, mask, n, &count, &junc);
                    count_branch(whole, r, &target, &count, &junc, finished, state);
                }
            } else if (key >> 63) {
                target = (int)(0xFFFFFFFFu - (unsigned)key);
                const bool whole = walk_branch(target, parents, hops, mask, n, &count, &junc);
                count_branch(whole, r, &target, &count, &junc, finished, state);
            }
        }
        targets[r] = target;
        lengths[r] = count;
        junction[r] = junc;
    }
}

// min(cap, floor(fl64(fl64(scale * sqrt64(d2)) + konst))): the comparison is taken in double
__device__ __forceinline__ int radius_of(int dbf, double scale, double konst, int cap) {
#pragma clang fp contract(off)
    const double d2 = (double)(dbf > 0 ? dbf : 0);
    const double product = scale * sqrt(d2);
    const double r = floor(product + konst);
    return r < (double)cap ? (int)r : cap;
}

__global__ __launch_bounds__(kThreads) void teasar_branch_write(
    const int* __restrict__ parents, const int* __restrict__ dbf, int n, int n_labels, double scale, double konst, int cap,
    unsigned char* mask, const int* __restrict__ targets, const long long* __restrict__ lengths,
    const int* __restrict__ junction, const long long* __restrict__ offsets, int* __restrict__ voxels,
    int* __restrict__ radii, int* __restrict__ before, long long n_new, int* state) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x + 1; r <= (size_t)n_labels; r += step) {
        const long long len = lengths[r];
        if (len == 0) continue;
        const long long at = offsets[r], end = offsets[r + 1];
        int cur = targets[r];
        if (len < 0 || at < 0 || end > n_new || end - at != len || cur < 0 || cur >= n) {
            atomicAdd(state + 4, 1);   // the row is left unwritten
            continue;
        }
        for (long long k = len - 1; k >= 0; --k) {
            const int p = parents[cur];
            voxels[at + k] = cur;
            radii[at + k] = radius_of(dbf[cur], scale, konst, cap);
            before[at + k] = k == 0 ? junction[r] : p;
            // my label's voxel: no other thread of the launch touches the byte. r >= 0, so a vertex is invalid
            // after its round; cleared here as well, a box of the caller's that leaves the vertex out cannot
            // make it the target again and the loop endless
            mask[cur] = kSkeleton;
            if (k == 0) break;
            if (p < 0 || p >= n) {   // not the walk teasar_branch_lengths took
                atomicAdd(state + 4, 1);
                break;
            }
            cur = p;
        }
    }
}

struct Box {
    int z0, y0, x0, z1, y1, x1;   // half-open
    __device__ bool empty() const { return z1 <= z0 || y1 <= y0 || x1 <= x0; }
};

__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// the cube of radius r around voxel v, clipped to the volume and to the label's box
__device__ __forceinline__ Box clipped_cube(int v, int r, const Dims& dm, const int* __restrict__ box) {
    const int x = v % dm.w, y = (v / dm.w) % dm.h, z = v / (dm.w * dm.h);
    Box b;
    b.z0 = imax(z - r, imax(box[0], 0));
    b.y0 = imax(y - r, imax(box[1], 0));
    b.x0 = imax(x - r, imax(box[2], 0));
    b.z1 = imin(z + r + 1, imin(box[3], dm.d));
    b.y1 = imin(y + r + 1, imin(box[4], dm.h));
    b.x1 = imin(x + r + 1, imin(box[5], dm.w));
    return b;
}

// clears bit 0 of the label's voxels in [z0, z1) x [y0, y1) x [x0, x1), which lies inside the volume: item
// "first", then every "step"-th. The volume has fewer than 2^31 voxels and step is at most 2^10 * 2^8.
__device__ __forceinline__ void clear_slab(unsigned char* mask, const int* __restrict__ labels, const Dims& dm, int label,
                                           int z0, int z1, int y0, int y1, int x0, int x1, unsigned first,
                                           unsigned step) {
    if (z1 <= z0 || y1 <= y0 || x1 <= x0) return;
    const unsigned nx = (unsigned)(x1 - x0), ny = (unsigned)(y1 - y0);
    const unsigned items = (unsigned)(z1 - z0) * ny * nx;
    for (unsigned i = first; i < items; i += step) {
        const unsigned row = i / nx;
        const int x = x0 + (int)(i - row * nx), y = y0 + (int)(row % ny), z = z0 + (int)(row / ny);
        const size_t q = ((size_t)z * dm.h + y) * dm.w + x;
        const unsigned char m = mask[q];
        if ((m & kValid) && labels[q] == label) mask[q] = m & (unsigned char)~kValid;
    }
}

template <bool ROOTS>
__global__ __launch_bounds__(kThreads) void teasar_invalidate(
    const int* __restrict__ labels, const int* __restrict__ dbf, const int* __restrict__ boxes, Dims dm, int n_labels,
    double scale, double konst, int cap, unsigned char* mask, const long long* __restrict__ lengths,
    const int* __restrict__ junction, const long long* __restrict__ offsets, const int* __restrict__ voxels,
    const int* __restrict__ radii, const int* __restrict__ before, long long n_new) {
    const unsigned first = blockIdx.y * kThreads + threadIdx.x, step = gridDim.y * kThreads;
    const long long rows = ROOTS ? (long long)n_labels : n_new;
    for (long long i = blockIdx.x; i < rows; i += gridDim.x) {   // uniform over the workgroup
        long long at = i;
        if (ROOTS) {
            const long long r = i + 1;
            if (lengths[r] <= 0 || junction[r] >= 0) continue;
            at = offsets[r];
            if (at < 0 || at >= n_new) continue;
        }
        const int p = voxels[at];
        if (p < 0 || p >= dm.n) continue;   // an entry teasar_branch_write refused
        const int prev = before[at];
        if (ROOTS != (prev < 0)) continue;   // a whole cube is the other launch's
        const int label = labels[p];
        if (label < 1 || label > n_labels) continue;
        const int* box = boxes + 6 * (size_t)label;
        const Box a = clipped_cube(p, imin(imax(radii[at], 0), cap), dm, box);
        if (a.empty()) continue;
        if (ROOTS) {
            clear_slab(mask, labels, dm, label, a.z0, a.z1, a.y0, a.y1, a.x0, a.x1, first, step);
            continue;
        }
        if (prev >= dm.n) continue;
        const Box b = clipped_cube(prev, radius_of(dbf[prev], scale, konst, cap), dm, box);
        // the intersection; where it is empty nothing of the cube has been cleared by the previous vertex
        const int iz0 = imax(a.z0, b.z0), iz1 = imin(a.z1, b.z1);
        const int iy0 = imax(a.y0, b.y0), iy1 = imin(a.y1, b.y1);
        const int ix0 = imax(a.x0, b.x0), ix1 = imin(a.x1, b.x1);
        if (iz1 <= iz0 || iy1 <= iy0 || ix1 <= ix0) {
            clear_slab(mask, labels, dm, label, a.z0, a.z1, a.y0, a.y1, a.x0, a.x1, first, step);
            continue;
        }
        // z-slabs over the full y/x extent, y-slabs with z in the intersection, x-slabs with z and y in it
        clear_slab(mask, labels, dm, label, a.z0, iz0, a.y0, a.y1, a.x0, a.x1, first, step);
        clear_slab(mask, labels, dm, label, iz1, a.z1, a.y0, a.y1, a.x0, a.x1, first, step);
        clear_slab(mask, labels, dm, label, iz0, iz1, a.y0, iy0, a.x0, a.x1, first, step);
        clear_slab(mask, labels, dm, label, iz0, iz1, iy1, a.y1, a.x0, a.x1, first, step);
        clear_slab(mask, labels, dm, label, iz0, iz1, iy0, iy1, a.x0, ix0, first, step);
        clear_slab(mask, labels, dm, label, iz0, iz1, iy0, iy1, ix1, a.x1, first, step);
    }
}

const char* const kDimsMessage = "dims must be positive with a product of at most 2^31 - 1";

bool aligned4(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 3) == 0;
}
bool aligned8(const void* a, const void* b = nullptr) { return (((uintptr_t)a | (uintptr_t)b) & 7) == 0; }

}  // namespace
}  // namespace exaspim

using namespace exaspim;

extern "C" size_t exaspim_teasar_workspace_bytes(const int32_t dims[3], int32_t n_labels) {
    Dims dm;
    if (!valid_dims(dims, &dm)) {
        set_error("teasar_workspace_bytes: %s", kDimsMessage);
        return 0;
    }
    if (n_labels < 0) {
        set_error("teasar_workspace_bytes: n_labels must not be negative, got %d", n_labels);
        return 0;
    }
    return workspace_need(n_labels);
}

extern "C" int exaspim_teasar_begin(const int32_t* labels_dev, const int32_t* sources_dev, const int32_t* hops_dev,
                                    const float* daf_dev, const int32_t dims[3], int32_t n_labels, uint8_t* mask_dev,
                                    int32_t* state_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && sources_dev && hops_dev && daf_dev && dims && mask_dev && state_dev && workspace_dev,
                  "teasar_begin: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(valid_dims(dims, &dm), "teasar_begin: %s", kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "teasar_begin: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && aligned4(labels_dev, sources_dev, hops_dev, daf_dev) &&
                      aligned4(state_dev),
                  "teasar_begin: misaligned buffer");
    const size_t need = workspace_need(n_labels);
    if (workspace_bytes < need) {
        set_error("teasar_begin: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    int* finished = reinterpret_cast<int*>(static_cast<char*>(workspace_dev) + keys_bytes(n_labels));
    teasar_init<<<capped_grid((size_t)dm.n, kThreads), kThreads, 0, s>>>(labels_dev, sources_dev, hops_dev, daf_dev, dm.n,
                                                                         n_labels, mask_dev, state_dev, finished);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

namespace {

// exaspim_teasar_round (given_dev == nullptr) and exaspim_teasar_round_given
int teasar_round(const char* name, const int32_t* labels_dev, const float* daf_dev, const int32_t* parents_dev,
                 const int32_t* hops_dev, const int32_t dims[3], int32_t n_labels, const uint8_t* mask_dev,
                 const int32_t* given_dev, bool given, int32_t* targets_dev, int64_t* lengths_dev,
                 int32_t* junction_dev, int32_t* state_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && daf_dev && parents_dev && hops_dev && dims && mask_dev && targets_dev && lengths_dev &&
                      junction_dev && state_dev && workspace_dev && (given_dev || !given),
                  "%s: NULL argument", name);
    Dims dm;
    EXA_CHECK_ARG(valid_dims(dims, &dm), "%s: %s", name, kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "%s: n_labels must not be negative, got %d", name, n_labels);
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 && aligned4(labels_dev, daf_dev, parents_dev, hops_dev) &&
                      aligned4(targets_dev, junction_dev, state_dev, given_dev) && aligned8(lengths_dev),
                  "%s: misaligned buffer", name);
    const size_t need = workspace_need(n_labels);
    if (workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)n_labels + 1;
    unsigned long long* keys = static_cast<unsigned long long*>(workspace_dev);
    int* finished = reinterpret_cast<int*>(static_cast<char*>(workspace_dev) + keys_bytes(n_labels));
    teasar_round_init<<<capped_grid(rows, kThreads), kThreads, 0, s>>>(keys, rows, state_dev, given);
    teasar_targets<<<capped_grid((size_t)dm.n, kThreads), kThreads, 0, s>>>(mask_dev, labels_dev, daf_dev, (size_t)dm.n,
                                                                            n_labels, keys);
    if (given)
        teasar_given_lengths<<<capped_grid(rows, kThreads), kThreads, 0, s>>>(
            keys, given_dev, labels_dev, daf_dev, parents_dev, hops_dev, mask_dev, dm.n, n_labels, targets_dev,
            reinterpret_cast<long long*>(lengths_dev), junction_dev, finished, state_dev);
    else
        teasar_branch_lengths<<<capped_grid(rows, kThreads), kThreads, 0, s>>>(
            keys, parents_dev, hops_dev, mask_dev, dm.n, n_labels, targets_dev,
            reinterpret_cast<long long*>(lengths_dev), junction_dev, finished, state_dev);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

}  // namespace

extern "C" int exaspim_teasar_round(const int32_t* labels_dev, const float* daf_dev, const int32_t* parents_dev,
                                    const int32_t* hops_dev, const int32_t dims[3], int32_t n_labels,
                                    const uint8_t* mask_dev, int32_t* targets_dev, int64_t* lengths_dev,
                                    int32_t* junction_dev, int32_t* state_dev, void* workspace_dev,
                                    size_t workspace_bytes, void* stream) {
    return teasar_round("teasar_round", labels_dev, daf_dev, parents_dev, hops_dev, dims, n_labels, mask_dev, nullptr,
                        false, targets_dev, lengths_dev, junction_dev, state_dev, workspace_dev, workspace_bytes, stream);
}

extern "C" int exaspim_teasar_round_given(const int32_t* labels_dev, const float* daf_dev, const int32_t* parents_dev,
                                          const int32_t* hops_dev, const int32_t dims[3], int32_t n_labels,
                                          const uint8_t* mask_dev, const int32_t* given_dev, int32_t* targets_dev,
                                          int64_t* lengths_dev, int32_t* junction_dev, int32_t* state_dev,
                                          void* workspace_dev, size_t workspace_bytes, void* stream) {
    return teasar_round("teasar_round_given", labels_dev, daf_dev, parents_dev, hops_dev, dims, n_labels, mask_dev,
                        given_dev, true, targets_dev, lengths_dev, junction_dev, state_dev, workspace_dev,
                        workspace_bytes, stream);
}

extern "C" int exaspim_teasar_apply(const int32_t* labels_dev, const int32_t* parents_dev, const int32_t* dbf_dev,
                                    const int32_t* boxes_dev, const int32_t dims[3], int32_t n_labels, double scale,
                                    double konst, uint8_t* mask_dev, const int32_t* targets_dev,
                                    const int64_t* lengths_dev, const int32_t* junction_dev, const int64_t* offsets_dev,
                                    int32_t* voxels_dev, int32_t* radii_dev, int32_t* before_dev, int64_t n_new,
                                    int64_t capacity, int32_t n_roots, int32_t* state_dev, void* stream) {
    EXA_CHECK_ARG(labels_dev && parents_dev && dbf_dev && boxes_dev && dims && mask_dev && targets_dev && lengths_dev &&
                      junction_dev && offsets_dev && state_dev,
                  "teasar_apply: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(valid_dims(dims, &dm), "teasar_apply: %s", kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "teasar_apply: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(n_new >= 0 && n_new <= dm.n, "teasar_apply: n_new must be in 0 .. the number of voxels, got %lld",
                  (long long)n_new);
    EXA_CHECK_ARG(n_roots >= 0, "teasar_apply: n_roots must not be negative, got %d", n_roots);
    EXA_CHECK_ARG(std::isfinite(scale) && scale >= 0.0 && std::isfinite(konst) && konst >= 0.0,
                  "teasar_apply: scale and const must be finite and not negative, got %g and %g", scale, konst);
    EXA_CHECK_ARG(capacity >= n_new, "teasar_apply: capacity of %lld entries, %lld needed", (long long)capacity,
                  (long long)n_new);
    EXA_CHECK_ARG(n_new == 0 || (voxels_dev && radii_dev && before_dev), "teasar_apply: NULL argument");
    EXA_CHECK_ARG(aligned4(labels_dev, parents_dev, dbf_dev, boxes_dev) && aligned4(targets_dev, junction_dev, state_dev) &&
                      aligned4(voxels_dev, radii_dev, before_dev) && aligned8(lengths_dev, offsets_dev),
                  "teasar_apply: misaligned buffer");
    if (n_new == 0 || n_labels == 0) return EXASPIM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int cap = dm.d > dm.h ? (dm.d > dm.w ? dm.d : dm.w) : (dm.h > dm.w ? dm.h : dm.w);
    const long long* lengths = reinterpret_cast<const long long*>(lengths_dev);
    const long long* offsets = reinterpret_cast<const long long*>(offsets_dev);
    teasar_branch_write<<<capped_grid((size_t)n_labels, kThreads), kThreads, 0, s>>>(
        parents_dev, dbf_dev, dm.n, n_labels, scale, konst, cap, mask_dev, targets_dev, lengths, junction_dev, offsets,
        voxels_dev, radii_dev, before_dev, (long long)n_new, state_dev);
    if (n_roots > 0)
        teasar_invalidate<true><<<dim3(capped_grid((size_t)n_labels, 1), root_grid_y(n_labels)), kThreads, 0, s>>>(
            labels_dev, dbf_dev, boxes_dev, dm, n_labels, scale, konst, cap, mask_dev, lengths, junction_dev, offsets,
            voxels_dev, radii_dev, before_dev, (long long)n_new);
    teasar_invalidate<false><<<dim3(capped_grid((size_t)n_new, 1), kDiffGridY), kThreads, 0, s>>>(
        labels_dev, dbf_dev, boxes_dev, dm, n_labels, scale, konst, cap, mask_dev, lengths, junction_dev, offsets,
        voxels_dev, radii_dev, before_dev, (long long)n_new);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}
