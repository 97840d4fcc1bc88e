// The border targets of a labelled volume (exaspim_border_targets; semantics in include/exaspim_affinity.h).
// DESIGN 6p. Where a face of the volume cuts a label, the target is the centre of the cut: per 8-connected
// component of one label on one of the six faces, the pixel with the largest squared in-plane distance e to
// a pixel of another label or to a position just outside the plane, ties to the smallest voxel index.
// Everything in integers, nothing rounded, and a pure function of the labels.
//
// The six planes are packed one after the other: z = 0, z = D - 1 (H x W each), y = 0, y = H - 1 (D x W),
// x = 0, x = W - 1 (D x H): P = 2 (HW + DW + DH) pixels, each with its plane, row r and column c. Six
// launches on the caller's stream, one thread per pixel, no LDS, no workgroup that waits for another one:
//   border_gather  the label of every pixel, 0 where it is not in 1..K; parent = itself, key = 0; the two
//                  state words cleared. The two x faces are stride-W reads of one word: D H of them.
//   border_axis    dbf.hip's window pass with the black border, per plane: first along the columns of a
//                  row with nothing to start from (the value is the squared distance to the run's nearer
//                  end, at most min(c + 1, w - c)^2), then along the rows with that as f. best = f(p);
//                  k = 1, 2, ... in both directions while k^2 < best. e is taken on labels: a nearest pixel
//                  outside the component never has the component's label.
//   border_union   8-connected union-find over the packed pixels: every foreground pixel is united with its
//                  west, north-west, north and north-east neighbours of the same plane and label. parent[i]
//                  <= i and only ever decreases (atomicMin on a root), so there is no cycle and a stale read
//                  is an older ancestor; the union that loses a race goes on from what it displaced.
//   border_peaks   parents are final: per foreground pixel its root, and a 64-bit atomicMax of (e << 32 |
//                  0xFFFFFFFF - voxel index) into the root's key.
//   border_emit    keys are final: a root whose target voxel is not also the target of a component on a
//                  face of lower number takes a slot from the counter and writes its row if the slot is
//                  below the capacity.
#include <algorithm>

#include "label_scan.h"

namespace exaspim {
namespace {

// a few workgroups per CU that stride over the pixels
constexpr unsigned kBorderGrid = 2048;

unsigned border_grid(size_t pixels) { return std::min(capped_grid(pixels, kThreads), kBorderGrid); }

struct Pixel {
    int base, h, w;   // the plane's first packed pixel, its rows and columns
    int face, r, c;
};

__host__ __device__ inline long long face_pixels(const Dims& dm) {
    return 2 * ((long long)dm.h * dm.w + (long long)dm.d * dm.w + (long long)dm.d * dm.h);
}

__device__ __forceinline__ int face_base(int face, const Dims& dm) {
    const int hw = dm.h * dm.w, dw = dm.d * dm.w, dh = dm.d * dm.h;
    return face < 2 ? face * hw : face < 4 ? 2 * hw + (face - 2) * dw : 2 * hw + 2 * dw + (face - 4) * dh;
}

__device__ __forceinline__ Pixel locate(int i, const Dims& dm) {
    const int hw = dm.h * dm.w, dw = dm.d * dm.w, dh = dm.d * dm.h;
    Pixel p;
    if (i < 2 * hw) {
        p.face = i >= hw;
        p.h = dm.h, p.w = dm.w;
    } else if (i < 2 * hw + 2 * dw) {
        p.face = 2 + (i - 2 * hw >= dw);
        p.h = dm.d, p.w = dm.w;
    } else {
        p.face = 4 + (i - 2 * hw - 2 * dw >= dh);
        p.h = dm.d, p.w = dm.h;
    }
    p.base = face_base(p.face, dm);
    const int local = i - p.base;
    p.r = local / p.w;
    p.c = local - p.r * p.w;
    return p;
}

__device__ __forceinline__ int voxel_of(const Pixel& p, const Dims& dm) {
    int z, y, x;
    if (p.face < 2) {
        z = p.face == 0 ? 0 : dm.d - 1, y = p.r, x = p.c;
    } else if (p.face < 4) {
        z = p.r, y = p.face == 2 ? 0 : dm.h - 1, x = p.c;
    } else {
        z = p.r, y = p.c, x = p.face == 4 ? 0 : dm.w - 1;
    }
    return (z * dm.h + y) * dm.w + x;   // below d * h * w
}

// the packed pixel of voxel (z, y, x) on "face", or -1 if the face does not hold it
__device__ __forceinline__ int pixel_on(int face, int z, int y, int x, const Dims& dm) {
    const int base = face_base(face, dm);
    switch (face) {
        case 0: return z == 0 ? base + y * dm.w + x : -1;
        case 1: return z == dm.d - 1 ? base + y * dm.w + x : -1;
        case 2: return y == 0 ? base + z * dm.w + x : -1;
        case 3: return y == dm.h - 1 ? base + z * dm.w + x : -1;
        case 4: return x == 0 ? base + z * dm.h + y : -1;
        default: return x == dm.w - 1 ? base + z * dm.h + y : -1;
    }
}

// a whole load of a word that other workgroups update
template <typename T>
__device__ __forceinline__ T seen(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void border_gather(const int* __restrict__ labels, Dims dm, int n_labels,
                                                         int pixels, int* __restrict__ lab, int* __restrict__ parent,
                                                         unsigned long long* __restrict__ keys, int* state) {
    const size_t step = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (first < 2) state[first] = 0;
    for (size_t i = first; i < (size_t)pixels; i += step) {
        const Pixel p = locate((int)i, dm);
        const int l = labels[voxel_of(p, dm)];
        lab[i] = (l >= 1 && l <= n_labels) ? l : 0;
        parent[i] = (int)i;
        keys[i] = 0;
    }
}

// One axis of every plane: along == 0 the columns of a row (neighbours 1 apart, "in" is not read: nothing
// is known yet), along == 1 the rows of a column (neighbours w apart). A position outside the plane counts
// as another label.
__global__ __launch_bounds__(kThreads) void border_axis(const int* __restrict__ lab, const int* __restrict__ in,
                                                       int* __restrict__ out, Dims dm, int pixels, int along) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)pixels; i += step) {
        const int me = lab[i];
        if (me == 0) {
            out[i] = 0;
            continue;
        }
        const Pixel p = locate((int)i, dm);
        const int at = along ? p.r : p.c, len = along ? p.h : p.w, stride = along ? p.w : 1;
        // the black border bounds the answer of this axis, so no probe leaves the line; and no e of the plane
        // exceeds cap^2 <= 23172^2, so a row value clamped there serves every column pass alike and fits
        const int cap = min(p.h, p.w) / 2 + 1;
        const int edge = min(min(at + 1, len - at), cap);
        int best = edge * edge;
        if (along) best = min(best, in[i]);
        for (int k = 1; k * k < best; ++k) {   // k < edge: both probes are inside the line
            const int k2 = k * k;
            const size_t lo = i - (size_t)k * stride, hi = i + (size_t)k * stride;
            if (lab[lo] != me || lab[hi] != me) {
                best = k2;
                break;
            }
            if (along) best = min(best, min(in[lo], in[hi]) + k2);
        }
        out[i] = best;
    }
}

__device__ __forceinline__ int find_root(const int* parent, int i) {
    for (int p = seen(parent + i); p != i; p = seen(parent + i)) i = p;   // parent[i] <= i: it ends
    return i;
}

__device__ __forceinline__ void unite(int* parent, int a, int b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = atomicMin(parent + a, b);   // a > b
        if (old == a) return;                        // a was a root and now hangs under b
        a = old;                                     // a hung under old already: old and b are still to be joined
    }
}

__global__ __launch_bounds__(kThreads) void border_union(const int* __restrict__ lab, Dims dm, int pixels,
                                                        int* parent) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)pixels; i += step) {
        const int me = lab[i];
        if (me == 0) continue;
        const Pixel p = locate((int)i, dm);
        if (p.c > 0 && lab[i - 1] == me) unite(parent, (int)i, (int)i - 1);
        if (p.r > 0) {
            const size_t up = i - (size_t)p.w;
            if (lab[up] == me) unite(parent, (int)i, (int)up);
            if (p.c > 0 && lab[up - 1] == me) unite(parent, (int)i, (int)up - 1);
            if (p.c + 1 < p.w && lab[up + 1] == me) unite(parent, (int)i, (int)up + 1);
        }
    }
}

__global__ __launch_bounds__(kThreads) void border_peaks(const int* __restrict__ lab, const int* __restrict__ e,
                                                        const int* __restrict__ parent, Dims dm, int pixels,
                                                        unsigned long long* keys) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)pixels; i += step) {
        if (lab[i] == 0) continue;
        int root = (int)i;
        for (int p = parent[root]; p != root; p = parent[root]) root = p;   // final since the launch before
        const Pixel p = locate((int)i, dm);
        const unsigned long long key =
            ((unsigned long long)(unsigned)e[i] << 32) | (0xFFFFFFFFu - (unsigned)voxel_of(p, dm));
        if (seen(keys + root) < key) atomicMax(keys + root, key);
    }
}

__global__ __launch_bounds__(kThreads) void border_emit(const int* __restrict__ lab, const int* __restrict__ parent,
                                                       const unsigned long long* __restrict__ keys, Dims dm,
                                                       int pixels, int* __restrict__ out_labels,
                                                       int* __restrict__ out_voxels, int capacity, int* state) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)pixels; i += step) {
        if (lab[i] == 0 || parent[i] != (int)i) continue;
        const Pixel p = locate((int)i, dm);
        const int v = (int)(0xFFFFFFFFu - (unsigned)keys[i]);   // a voxel of this component: below d * h * w
        const int x = v % dm.w, y = (v / dm.w) % dm.h, z = v / (dm.w * dm.h);
        // the same voxel as the target of a face of lower number (an edge, a corner, two faces that coincide)
        bool twice = false;
        for (int face = 0; face < p.face && !twice; ++face) {
            const int j = pixel_on(face, z, y, x, dm);
            if (j < 0) continue;
            int root = j;   // the voxel has my label there too: a foreground pixel
            for (int q = parent[root]; q != root; q = parent[root]) root = q;
            twice = (int)(0xFFFFFFFFu - (unsigned)keys[root]) == v;
        }
        if (twice) continue;
        const int slot = atomicAdd(state, 1);   // at most P <= 2^31 - 1 rows
        if (slot < capacity) {
            out_labels[slot] = lab[i];
            out_voxels[slot] = v;
        }
    }
}

const char* const kDimsMessage =
    "dims must be positive with a product of at most 2^31 - 1 and at most 2^31 - 1 face pixels, 2 (HW + DW + DH)";

bool valid_faces(const int32_t dims[3], Dims* dm) { return valid_dims(dims, dm) && face_pixels(*dm) <= 2147483647ll; }

// lab, the row pass, e and parent (int32 each), then the keys
size_t workspace_need(const Dims& dm) {
    const size_t pixels = (size_t)face_pixels(dm);
    return 4 * align_up(pixels * sizeof(int), 16) + align_up(pixels * sizeof(unsigned long long), 16);
}

}  // namespace
}  // namespace exaspim

using namespace exaspim;

extern "C" size_t exaspim_border_targets_workspace_bytes(const int32_t dims[3]) {
    Dims dm;
    if (!valid_faces(dims, &dm)) {
        set_error("border_targets_workspace_bytes: %s", kDimsMessage);
        return 0;
    }
    return workspace_need(dm);
}

extern "C" int exaspim_border_targets(const int32_t* labels_dev, const int32_t dims[3], int32_t n_labels,
                                      int32_t* out_labels_dev, int32_t* out_voxels_dev, int32_t capacity,
                                      int32_t* state_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(labels_dev && dims && state_dev && workspace_dev, "border_targets: NULL argument");
    Dims dm;
    EXA_CHECK_ARG(valid_faces(dims, &dm), "border_targets: %s", kDimsMessage);
    EXA_CHECK_ARG(n_labels >= 0, "border_targets: n_labels must not be negative, got %d", n_labels);
    EXA_CHECK_ARG(capacity >= 0, "border_targets: capacity must not be negative, got %d", capacity);
    EXA_CHECK_ARG(capacity == 0 || (out_labels_dev && out_voxels_dev), "border_targets: NULL argument");
    EXA_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0 &&
                      (((uintptr_t)labels_dev | (uintptr_t)out_labels_dev | (uintptr_t)out_voxels_dev |
                        (uintptr_t)state_dev) & 3) == 0,
                  "border_targets: misaligned buffer");
    const size_t need = workspace_need(dm);
    if (workspace_bytes < need) {
        set_error("border_targets: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return EXASPIM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const int pixels = (int)face_pixels(dm);
    const size_t plane = align_up((size_t)pixels * sizeof(int), 16);
    char* ws = static_cast<char*>(workspace_dev);
    int* lab = reinterpret_cast<int*>(ws);
    int* rows = reinterpret_cast<int*>(ws + plane);
    int* e = reinterpret_cast<int*>(ws + 2 * plane);
    int* parent = reinterpret_cast<int*>(ws + 3 * plane);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + 4 * plane);
    const unsigned grid = border_grid((size_t)pixels);
    border_gather<<<grid, kThreads, 0, s>>>(labels_dev, dm, n_labels, pixels, lab, parent, keys, state_dev);
    border_axis<<<grid, kThreads, 0, s>>>(lab, nullptr, rows, dm, pixels, 0);
    border_axis<<<grid, kThreads, 0, s>>>(lab, rows, e, dm, pixels, 1);
    border_union<<<grid, kThreads, 0, s>>>(lab, dm, pixels, parent);
    border_peaks<<<grid, kThreads, 0, s>>>(lab, e, parent, dm, pixels, keys);
    border_emit<<<grid, kThreads, 0, s>>>(lab, parent, keys, dm, pixels, out_labels_dev, out_voxels_dev, capacity,
                                          state_dev);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}
