// Shared declarations of the exaspim_affinity HIP extension (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/exaspim_affinity.h"

namespace exaspim {

// ---- error reporting (thread-local message behind exaspim_last_error) ----
void set_error(const char* fmt, ...);
const char* get_error();

#define EXA_CHECK_ARG(cond, ...)                 \
    do {                                         \
        if (!(cond)) {                           \
            ::exaspim::set_error(__VA_ARGS__);   \
            return EXASPIM_E_INVALID;            \
        }                                        \
    } while (0)

#define EXA_CHECK_HIP(expr)                                                  \
    do {                                                                     \
        hipError_t _e = (expr);                                              \
        if (_e != hipSuccess) {                                              \
            ::exaspim::set_error("%s failed: %s (%s:%d)", #expr,             \
                                 hipGetErrorString(_e), __FILE__, __LINE__); \
            return EXASPIM_E_HIP;                                            \
        }                                                                    \
    } while (0)

// ---- device helper shared by the convolution epilogues ------------------------
// One voxel's 16-channel record of a chunk plane (32 B in a 16-bit type) leaves the accumulators
// of a 32 x 32 MFMA tile split over the two half-waves: lane r holds channels 8q .. 8q + 3 of its
// voxel, lane r + 32 channels 8q + 4 .. 8q + 7 (q = 0 .. 3). v_permlane32_swap exchanges the upper
// half of group q with the lower half of group q + 1, after which lane r holds the record's first
// 16 bytes (channels 0 .. 7 of the pair) and lane r + 32 the second 16 (channels 8 .. 15): one
// 16-byte store per lane and chunk plane, 32 whole records per instruction, no LDS round trip.
__device__ __forceinline__ uint4 record_half(uint2 lo_group, uint2 hi_group) {
    const auto r0 = __builtin_amdgcn_permlane32_swap(lo_group.x, hi_group.x, false, false);
    const auto r1 = __builtin_amdgcn_permlane32_swap(lo_group.y, hi_group.y, false, false);
    return make_uint4(r0[0], r1[0], r0[1], r1[1]);
}


// 16-byte MUBUF store with a scalar offset (range-checked against the descriptor: an offset at or
// beyond its size is dropped by the hardware). gfx950 needs a wait state between such a store and a
// vector-ALU write of its data registers -- tools/store_hazard.hip: without one 0.5 % of the stored
// words are the NEW register contents (5 % with an immediate soffset, where one wait state is still
// not enough and two are). hipcc's hazard recognizer guards only the form without a register soffset,
// and with a single wait state, so the store carries its own s_nop 1. (Being inline assembly it is also
// invisible to hipcc's s_waitcnt bookkeeping: nothing ever waits on these stores but the end of the
// kernel -- which is what the epilogues want -- AND to its hazard recognizer: a descriptor or offset
// SGPR written by the vector ALU right before (v_readlane of a spilled SGPR, v_readfirstlane) needs
// five wait states before a memory instruction reads it, which hipcc inserts for its own instructions
// only; without the leading s_nop 4 the store of the pooled epilogue went out with a half-restored
// descriptor and faulted.)
typedef unsigned int exa_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void buf_store16(const uint4& v, __amdgpu_buffer_rsrc_t rsrc, unsigned voff,
                                            unsigned soff) {
    const exa_u32x4 d = {v.x, v.y, v.z, v.w};
    const unsigned ssoff = __builtin_amdgcn_readfirstlane(soff);   // (wave-uniform by contract)
    asm volatile("s_nop 4\n\tbuffer_store_dwordx4 %0, %1, %2, %3 offen\n\ts_nop 1"
                 :: "v"(d), "v"(voff), "s"(rsrc), "s"(ssoff) : "memory");
}

// The same store through the compiler's builtin, for code whose later waits should COUNT it (a load
// issued before it is then waited for with s_waitcnt vmcnt(#younger operations) instead of being made
// to wait for the store as well). The scheduling fences keep any vector-ALU write of the data registers
// from being placed between the store and its wait states.
__device__ __forceinline__ void buf_store16_counted(const uint4& v, __amdgpu_buffer_rsrc_t rsrc, unsigned voff,
                                                    unsigned soff) {
    const exa_u32x4 d = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_raw_buffer_store_b128(d, rsrc, (int)voff, (int)__builtin_amdgcn_readfirstlane(soff), 0);
    asm volatile("s_nop 1");
    __builtin_amdgcn_sched_barrier(0);
}

// ---- device helpers shared by the fp16 stores and the max-pools ---------------
// Saturating float -> half: beyond +-65504 the largest finite half instead of +-inf, a NaN stays
// NaN. (v_med3_f32 alone returns the lower bound for a NaN input, and hipcc folds it so as well.)
__device__ __forceinline__ float sat_f16(float v) {
    return v != v ? v : __builtin_amdgcn_fmed3f(v, -65504.f, 65504.f);
}

// The max-pools propagate NaN like torch's max_pool3d, with the same bits whatever the order in
// which a window is reduced (the fused and the separate pool are held to each other bit for bit).
// float32: fmaxf for numbers, the canonical quiet NaN if either input is one.
__device__ __forceinline__ float max_nan(float a, float b) {
    return (a != a || b != b) ? __uint_as_float(0x7fc00000u) : fmaxf(a, b);
}
__device__ __forceinline__ uint4 max_nan4(const uint4& a, const uint4& b) {
    return make_uint4(__float_as_uint(max_nan(__uint_as_float(a.x), __uint_as_float(b.x))),
                      __float_as_uint(max_nan(__uint_as_float(a.y), __uint_as_float(b.y))),
                      __float_as_uint(max_nan(__uint_as_float(a.z), __uint_as_float(b.z))),
                      __float_as_uint(max_nan(__uint_as_float(a.w), __uint_as_float(b.w))));
}
// bf16 and f16 order like sign-magnitude integers: flipping the magnitude bits of negative
// values, x ^ ((x >> 15) & 0x7fff) per 16-bit half, makes them order like two's-complement
// shorts, so a packed integer maximum picks the larger float; the map is its own inverse.
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned key16x2(unsigned x) {
    const s16x2 m = __builtin_bit_cast(s16x2, x) >> (short)15;   // 0 or -1 per half
    return x ^ (__builtin_bit_cast(unsigned, m) & 0x7fff7fffu);
}
// The ordering key of a value: key16x2 after the sign of a NaN is cleared, so that every NaN
// (a magnitude above INF16, the bits of +inf: 0x7c00 f16, 0x7f80 bf16) orders above +inf.
// The inverse of a key is key16x2.
template <unsigned INF16>
__device__ __forceinline__ unsigned okey16x2(unsigned x) {
    const u16x2 mag = __builtin_bit_cast(u16x2, x & 0x7fff7fffu);
    const auto nan = mag > (u16x2){(unsigned short)INF16, (unsigned short)INF16};   // -1 per NaN half
    return key16x2(x & ~(__builtin_bit_cast(unsigned, nan) & 0x80008000u));
}
__device__ __forceinline__ unsigned maxkey16x2(unsigned ka, unsigned kb) {
    return __builtin_bit_cast(
        unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, ka), __builtin_bit_cast(s16x2, kb)));
}
__device__ __forceinline__ uint4 key16(const uint4& v) {
    return make_uint4(key16x2(v.x), key16x2(v.y), key16x2(v.z), key16x2(v.w));
}
template <unsigned INF16>
__device__ __forceinline__ uint4 okey16(const uint4& v) {
    return make_uint4(okey16x2<INF16>(v.x), okey16x2<INF16>(v.y), okey16x2<INF16>(v.z), okey16x2<INF16>(v.w));
}
__device__ __forceinline__ uint4 maxkey16(const uint4& a, const uint4& b) {
    return make_uint4(maxkey16x2(a.x, b.x), maxkey16x2(a.y, b.y), maxkey16x2(a.z, b.z), maxkey16x2(a.w, b.w));
}

// ---- the arithmetic of the 1x1x1 head --------------------------------------------
// One definition for head_kernel (layers.hip) and the fused head of the bf16x3 convolution
// (conv3d.hip: conv3x3x3_x3_head), which are held to each other bit for bit although the two files
// are compiled with different -ffp-contract settings: nothing in here may be contracted or
// reassociated, every fused multiply-add is written out.
// acc + sum of f[j] * w[j], j ascending, one fmaf per channel
template <int N>
__device__ __forceinline__ float head_dot(float acc, const float (&f)[N], const float* w) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < N; ++j) acc = fmaf(f[j], w[j], acc);
    return acc;
}
// the logit, or its sigmoid (inference.py:158)
__device__ __forceinline__ float head_activation(float r, int apply_sigmoid) {
#pragma clang fp contract(off)
    if (apply_sigmoid) r = 1.f / (1.f + expf(-r));
    return r;
}

// ---- network plan ---------------------------------------------------------
// Channel counts are padded to multiples of 32 inside the workspace so that
// every MFMA convolution sees whole 32-wide output tiles and whole 32-byte
// input chunks; padded weights and biases are zero, so padded channels carry
// exact zeros through LeakyReLU, max-pool and interpolation.
constexpr int kChannelPad = 32;
constexpr int kNumMfmaConvs = 17;  // every 3x3x3 conv except inc.0 (Cin = 1)

inline int pad_channels(int c) { return (c + kChannelPad - 1) / kChannelPad * kChannelPad; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// The merge test of the agglomeration and of the pre-merge: an edge merges iff merge_all or
// sum > m * count, m = rint((1 - T) * 2^24), i.e. iff 1 - mean affinity < T up to the grid of q;
// m <= 0 merges nothing that has sum 0 and everything else, m >= 2^24 nothing at all.
struct MergeBound {
    uint64_t m;
    bool merge_all;
};
inline MergeBound merge_bound(float threshold) {
    const double md = __builtin_rint((1.0 - (double)threshold) * 16777216.0);
    return MergeBound{md < 0.0 ? 0 : md > 16777216.0 ? 16777216ull : (uint64_t)md, md < 0.0};
}
// Type the activations are stored in between kernels: EXASPIM_DT_BF16X3 keeps them float32 (only
// its 3x3x3 MFMA convolutions are its own; every other layer runs the float32 kernel).
inline int storage_dtype(int dtype) { return dtype == EXASPIM_DT_BF16X3 ? EXASPIM_DT_F32 : dtype; }
inline int dtype_size(int dtype) { return storage_dtype(dtype) == EXASPIM_DT_F32 ? 4 : 2; }

struct ConvLayer {
    int ca_real = 0, cb_real = 0;  // real input channels from source A / B
    int ca = 0, cb = 0;            // padded
    int cout_real = 0, cout = 0;   // real / padded output channels
    size_t w_off = 0;              // packed weights (compute dtype; bf16x3: a hi and a lo bf16 fragment
                                   // per (16-channel chunk, tap, 32-cout tile)), bytes
    size_t b_off = 0;              // folded bias, float[cout], bytes
    size_t p_off = 0;              // offset of this conv's block in params
};

// ConvTranspose3d(k=2, s=2) of an Up block (UNet3D(trilinear=False))
struct ConvTLayer {
    int cin_real = 0, cin = 0;     // real / padded input channels
    int cout_real = 0, cout = 0;   // real / padded output channels
    size_t w_off = 0;              // packed weights [chunk][phase 8][tile][lane][16 B]
    size_t b_off = 0;              // bias, float[cout]
    size_t p_off = 0;              // offset of (weight, bias) in params
};

struct UNetPlan {
    int channels[5] = {0, 0, 0, 0, 0};
    int out_channels = 0;
    int dtype = 0;                  // EXASPIM_DT_* (without flags)
    bool convt = false;             // EXASPIM_UP_CONVT
    ConvTLayer up[4];               // up1.up .. up4.up (convt only)
    int c0 = 0, c0p = 0;            // inc.0 output channels real / padded
    size_t first_p_off = 0;         // params offset of inc.0
    size_t first_w_off = 0;         // float[27][c0p]
    size_t first_b_off = 0;         // float[c0p]
    ConvLayer conv[kNumMfmaConvs];  // inc.3, down1.0 ... up4.3
    size_t head_p_off = 0;
    size_t head_w_off = 0;          // float[out_channels][c0p]
    size_t head_b_off = 0;          // float[out_channels]
    size_t packed_bytes = 0;
    size_t n_params = 0;
};

// Builds the plan; returns false (and sets the error) on invalid arguments.
bool make_plan(const int32_t channels[5], int32_t out_channels, int32_t dtype,
               UNetPlan* plan);

int pack_weights(const UNetPlan& plan, const float* params, void* packed_host);

// ---- kernel launchers (conv3d.hip / layers.hip / prepost.hip) -------------
struct ConvArgs {
    const void* src_a;
    const void* src_b;
    int ca, cb;          // padded channel counts of the two sources (cb may be 0)
    const void* weights; // packed fragments
    // Carry out (row mode, conv3x3x3_zpipe_rowz): planes [out_z0, out_z1) of this launch's output, as the
    // row launch stores them (own frame and x neighbour), go to carry_dst as well, at plane - out_shift of
    // the same per-patch layout, and their pooled planes to carry_pool_dst at pooled plane - out_shift / 2:
    // the later batch whose patches start out_shift planes further down z finds them where it would have
    // written them itself. Null: off. Outside row mode (conv3x3x3_t14_carry, the 16-bit 64-cout layers of level
    // 1): the same per patch, carry_pool_dst exactly when pool_dst is set. (These two take the place of two pointers that fed removed kernels:
    // the kernel-argument block of every other convolution kernel keeps its layout and hence its code.)
    void* carry_dst = nullptr;
    void* carry_pool_dst = nullptr;
    const float* bias;
    void* dst;
    int cout;            // padded
    int n, d, h, w;      // batch of patches and their spatial size at this level
    float slope;
    // Optional fused OutConv (unet3d.py:318) + sigmoid (inference.py:158): when
    // head_out is set (32-cout layers only) the conv's activations are not stored;
    // the 1x1x1 head runs on the accumulators and writes NCDHW float32.
    const float* head_w = nullptr;  // float[head_oc][32]
    const float* head_b = nullptr;  // float[head_oc]
    float* head_out = nullptr;      // float (n, head_oc, d, h, w)
    int head_oc = 0;
    int head_sigmoid = 0;
    // Region of output voxels the caller needs, [org, org + ext) per axis (z, y, x);
    // ext = 0 means the whole patch. predict() trims the outputs of every patch
    // (inference.py:161-162), so the last two convolutions only produce what survives:
    // tiles start at org, whole tiles outside the region are never launched and
    // stores are masked to it. Voxels outside the region are left untouched.
    int org[3] = {0, 0, 0};
    int ext[3] = {0, 0, 0};
    // Optional fused MaxPool3d(2) (unet3d.py:195) of this conv's output, written to
    // pool_dst as (n, cout, d/2, h/2, w/2) in the same layout (every tile shape but 6^3:
    // ask conv_can_fuse_pool first); saves re-reading the whole skip tensor.
    void* pool_dst = nullptr;
    // Row mode (z-column kernel with the fused max-pool, 16-bit types, whole patches): the n patches
    // are one row along x, each starting row_stride voxels after the previous one. The tiles walk the
    // row's 16-wide strip columns once instead of every patch's own: patch i computes local x in
    // [o/2, row_stride + o/2) (o = w - row_stride; the first patch from 0, the last one to w) in its
    // own frame, and a column that its neighbour holds too is stored to both, except the
    // neighbour's two outermost x (and pooled x) whose inputs reach its zero padding. Those are left
    // for launch_conv3x3x3_thin and launch_maxpool2_xcols. 0: off.
    int row_stride = 0;
    // Carry in (row mode, or conv3x3x3_t14_carry): planes [in_z0, in_z1) of dst and their pooled planes of pool_dst are already
    // there (an earlier launch's carry out). Whole z tiles of the depth the launcher picks, even bounds;
    // the tile walk leaves them out and nothing is written for them. Empty: off. (The row-mode border launch,
    // kRowStageBordersCarry, masks its own 8-plane tiles at in_z0: the range need not be whole tiles of its.)
    unsigned short in_z0 = 0, in_z1 = 0;
    // Optional scratch for split-K (t14 kernel): launches with too few workgroups to fill
    // the device cut the input-channel chunks into up to 4 ranges, every range writes its
    // float32 partial sums here and a second kernel adds them in a fixed order.
    float* partial = nullptr;
    size_t partial_patch_bytes = 0;   // scratch bytes per patch of the batch
    int ksplit = 1;      // set by the launcher
    // carry out: even bounds, any alignment to the tiles (narrow types: the carry fields fill what was
    // padding, so the argument block of every kernel keeps its size; planes up to 254 are plenty)
    unsigned char out_z0 = 0, out_z1 = 0;
    unsigned short out_shift = 0;
#ifdef EXASPIM_TRACE
    // tools/conv_trace.hip only: 16 x 64-bit cycle stamps per wave (never in the library build)
    unsigned long long* trace = nullptr;
#endif
};

// Rows carried along y (row mode, conv3x3x3_zpipe_rowzy only: a second kernel argument of that symbol, so
// ConvArgs and the argument block of every other kernel stay as they are). The launch computes
// {planes outside [in_z0, in_z1)} x {rows outside [in_y0, in_y1)} and stores again only what it computes:
//  * carry in: rows [in_y0, in_y1) of dst and their pooled rows of pool_dst are already there. Whole 8-row
//    tiles, inside [2, h - 2); the tile walk leaves them out. Empty: off.
//  * y carry out: rows [out_y0, out_y1) of every plane the launch stores go to y_dst / y_pool_dst as well, at
//    row - out_shift_y (pooled: half of it), own frame and x neighbour like the z carry. Even bounds. Null: off.
//  * diagonal carry out: planes [out_z0, out_z1) x rows [out_y0, out_y1) go to d_dst / d_pool_dst at
//    plane - out_shift and row - out_shift_y: the block that neither the z nor the y successor computes,
//    because each takes it over from this launch. Needs both the z and the y carry out. Null: off.
struct ConvCarryY {
    void* y_dst = nullptr;
    void* y_pool_dst = nullptr;
    void* d_dst = nullptr;
    void* d_pool_dst = nullptr;
    unsigned short in_y0 = 0, in_y1 = 0;
    unsigned short out_y0 = 0, out_y1 = 0;
    unsigned short out_shift_y = 0;
};
inline bool conv_has_carry_y(const ConvCarryY& y) {
    return y.y_dst || y.y_pool_dst || y.d_dst || y.d_pool_dst || y.in_y0 || y.in_y1 || y.out_y0 || y.out_y1 || y.out_shift_y;
}

// Host-side record of the last convolution configuration this thread launched (the launcher's
// __PRETTY_FUNCTION__, template arguments included) and its split-K factor: read by the tests'
// layer probe (layer_probe.hip) to assert which dispatch path a case took.
struct ConvLaunchRecord {
    const char* config = "";
    int ksplit = 0;
    bool row = false;    // the launch ran conv3x3x3_zpipe_row (ConvArgs::row_stride) ...
    bool carry_y = false;  // the launch ran conv3x3x3_zpipe_rowzy (a field of ConvCarryY set)
    bool carry = false;  // ... or conv3x3x3_zpipe_rowz / conv3x3x3_t14_carry / conv3x3x3_t14_borders_carry (a carry field of ConvArgs set)
};
ConvLaunchRecord& last_conv_launch();
// The same for the inc.0 and upsampling launchers (layers.hip): the name of the kernel variant
// the last launch_conv_first / launch_upsample2 of this thread ran.
const char*& last_layer_kernel();

int launch_conv3x3x3(int dtype, const ConvArgs& a, hipStream_t stream);
// Thin remainders of a region along y or x (at most 4 voxels thick) on 2-voxel-thick
// tiles: what is left when the z-column kernel's 8 x 16 tiles cover only the multiple-of-
// tile part of a trimmed region. 32-cout slices only.
int launch_conv3x3x3_thin(int dtype, const ConvArgs& a, hipStream_t stream);
// y / x extent of "ext" the z-column kernel should cover with whole tiles when the
// remainder goes to launch_conv3x3x3_thin: the largest multiple of the tile if the
// remainder is 1..4 voxels, else ext itself
int conv_zcol_main_extent(int ext, int axis);
bool conv_can_fuse_head(int cout, int w, int head_oc, int dtype = EXASPIM_DT_F32);
// EXASPIM_DT_BF16X3 only: the convolution of launch_conv3x3x3 (same sums, same order) with the 1x1x1
// head on its accumulators. head_out / head_w / head_b / head_oc / head_sigmoid must be set; dst is
// never written; the region [org, org + ext) is covered with masked 4 x 8 x 16 tiles (no thin
// remainders, no split-K). head_out gets the bits launch_head gives on the stored activations.
// Needs conv_x3_can_fuse_head: cout 32, w a multiple of 16, 1..4 outputs.
int launch_conv3x3x3_x3_head(const ConvArgs& a, hipStream_t stream);
bool conv_x3_can_fuse_head(int cout, int w, int head_oc);
bool conv_can_fuse_pool(int dtype, int cout, int d, int h, int w);
// Row mode (ConvArgs::row_stride) runs on this layer and row geometry: a 16-bit z-column layer whose
// fused max-pool covers whole patches (fused_pool_whole_patch: the caller's conv_can_fuse_pool, a pool
// destination and an untrimmed region), n >= 2 patches of width w a multiple of the 16-wide tiles, an
// overlap w - row_stride that is a positive multiple of 32 and at most the stride. The one predicate of
// launch_conv3x3x3's argument check and of the engine's choice between the row and the per-patch path.
bool conv_row_mode_ok(int dtype, int cout, int n, int w, int row_stride, bool fused_pool_whole_patch);
// A row-mode convolution and the launches that finish it (a.row_stride > 0, a.pool_dst set), in this
// order: the row launch (launch_conv3x3x3), launch_conv3x3x3_thin on x in [0, 2) of patches 1 .. n-1
// and on x in [w - 2, w) of patches 0 .. n-2 in each patch's own frame, then launch_maxpool2_xcols on
// the pooled columns 0 and w/2 - 1 of every patch. stages: which of them to run (the engine: all;
// the tests' layer probe looks at what each one leaves behind).
constexpr int kRowStageMain = 1, kRowStageThin = 2, kRowStagePool = 4;
constexpr int kRowStagesAll = kRowStageMain | kRowStageThin | kRowStagePool;
// kRowStageBorders: what Thin and Pool do, in one launch after them -- the thin-along-x tiles of both faces
// as two jobs of one grid, each tile writing the pooled column it holds (conv3x3x3_t14 with ZORD and POOL).
// The convolution has launch_conv3x3x3_thin's bits, the pooled columns launch_maxpool2_xcols's. The engine
// runs Main | Borders (EXASPIM_OPT_ROW_SEPARATE_BORDERS: Main | Thin | Pool).
constexpr int kRowStageBorders = 8;
constexpr int kRowStagesFused = kRowStageMain | kRowStageBorders;
// kRowStageBordersCarry: the border launch honouring the carry fields of ConvArgs (conv3x3x3_t14_borders_carry):
// it computes and stores no plane of [in_z0, in_z1) -- any even range, no whole border tiles needed -- and stores
// planes [out_z0, out_z1) of its columns and pooled columns a second time, like the main launch. After Main |
// BordersCarry of a predecessor the successor's buffers hold every x of the carried planes, and nothing reads
// planes [in_z0 + 1, in_z1 - 1) of the source. With no carry field set it is kRowStageBorders; kRowStageBorders
// itself clears the fields and writes every plane.
constexpr int kRowStageBordersCarry = 16;
constexpr int kRowStagesCarry = kRowStageMain | kRowStageBordersCarry;
// y (optional): rows carried along y by the main launch (ConvCarryY, conv3x3x3_zpipe_rowzy). The border launches
// are as without it: they compute every row of their columns, in the batch's own buffers and the z target.
int launch_conv3x3x3_row(int dtype, const ConvArgs& a, int stages, hipStream_t stream, const ConvCarryY* y = nullptr);
// Tile depth of the z-column kernel on a 32-cout slice of depth d without a fused head (launch_typed)
int conv_zcol_tile_depth(int d);
// Tile depth of the row-mode border launch at depth d (launch_row_borders)
int conv_row_borders_tile_depth(int d);
// Carried planes outside row mode (conv3x3x3_t14_carry): the tile depth if launch_conv3x3x3 runs this launch
// (dtype, shape, channels, split-K scratch of a) on the configuration that has a carry symbol, else 0
constexpr int kCarryT14TZ = 4;
int conv_carry_t14_tile_depth(int dtype, const ConvArgs& a);
// (engine.hip) the level-1 plane range a forward of depth d takes over from the one shift_z planes up, for tiles
// of tz planes; {0, 0}: none
void carry1_span_of_tiles(int tz, int d, int shift_z, int32_t out[2]);
#ifndef EXASPIM_TRACE
static_assert(sizeof(ConvArgs) == 184, "ConvArgs: the carry fields fill padding, the argument block keeps its size");
#endif

// xpad: scratch for the zero-bordered copy of x, n * (d+2)(h+2)(wd+2) floats
// first_no_strips: keep the per-group kernel (the tests hold it to the row-strip kernel bit for bit)
// [skip_z0, skip_z1): output planes no later launch reads (conv_first_skip_planes). The row-strip kernel stores
// nothing to them; every other variant ignores the range and writes all planes, a legal superset. The planes
// that are written have the same bits either way.
int launch_conv_first(int dtype, const float* x, float* xpad, const float* w, const float* bias,
                      void* dst, int n, int d, int h, int wd, int c0p, float slope,
                      hipStream_t stream, bool first_no_strips = false, int skip_z0 = 0, int skip_z1 = 0);
// Planes of inc.3's source that no computed tile of a row sequence Main | BordersCarry reads when planes
// [in_z0, in_z1) are carried in: both launches compute [0, in_z0) and [in_z1, d) only, and a computed plane reads
// its two neighbours, so [in_z0 + 1, in_z1 - 1). Empty ({0, 0}) without a carry in or for a range of 2 planes.
void conv_first_skip_planes(int d, int in_z0, int in_z1, int32_t out[2]);
// ConvTranspose3d(k=2, s=2): (n, d, h, w, cin) -> (n, 2d, 2h, 2w, cout), bias, no activation
int launch_convt2(int dtype, const void* src, const void* weights, const float* bias, void* dst,
                  int n, int d, int h, int w, int cin, int cout, hipStream_t stream);
int launch_maxpool2(int dtype, const void* src, void* dst, int n, int d, int h, int w,
                    int c, hipStream_t stream);  // d,h,w = INPUT size
// The same maxima (same bits, NaN included) for two output x columns only, ox0 and ox1, every
// z and y: the pooled columns a row-mode launch leaves to this (ConvArgs::row_stride)
int launch_maxpool2_xcols(int dtype, const void* src, void* dst, int n, int d, int h, int w,
                          int c, int ox0, int ox1, hipStream_t stream);
// d,h,w = INPUT size; output voxels within "margin" of a face are not computed
// margin_hi (optional, int[3]): output voxels within margin_hi[axis] >= margin of an axis' HIGH face are not
// needed either. The row-strip kernel skips them (along z down to a whole number of its runs); every other
// variant computes the symmetric superset. The voxels that are computed have the same bits either way.
int launch_upsample2(int dtype, const void* src, void* dst, int n, int d, int h, int w,
                     int c, int margin, hipStream_t stream, bool plain_kernel = false, bool per_thread = false,
                     const int* margin_hi = nullptr);
// *out = max(*out, largest |value| in the tensor) as float bits (out zeroed by the caller)
int launch_absmax(int dtype, const void* src, size_t bytes, float* out, hipStream_t stream);
int launch_head(int dtype, const void* src, const float* w, const float* bias,
                float* out, int n, int d, int h, int wd, int c0p, int out_channels,
                int apply_sigmoid, hipStream_t stream);
// (dbf.hip) one pass of exaspim_dbf: axis 2 (x) writes f to out from the labels alone ("in" is not read),
// axis 1 (y) and axis 0 (z) read the previous pass's field from "in", which must not be "out".
// EXASPIM_E_INVALID for dims exaspim_dbf refuses; the pointers are the caller's to check.
int launch_dbf_pass(int axis, const int32_t* labels, const int32_t* in, int32_t* out, const int32_t dims[3],
                    int black_border, hipStream_t stream);
// (components.hip) the passes first .. last of exaspim_fill_holes, which runs all of them: 0 the background's
// edge mask, 1 tile_pass, 2 face_merge, 3 flatten, 4 the survey (its two words reset, the faces, the
// neighbours), 5 the fill (counts zeroed first). Each pass reads what the ones before it left in the
// workspace. EXASPIM_E_INVALID for dims exaspim_fill_holes refuses; the pointers are the caller's to check.
constexpr int kFillHolesPasses = 6;
int launch_fill_holes_passes(const int32_t* labels, const int32_t dims[3], int32_t* out, int64_t* counts,
                             void* workspace, int first, int last, hipStream_t stream);

}  // namespace exaspim
