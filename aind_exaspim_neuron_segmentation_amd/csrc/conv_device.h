// Device helpers shared by the 3x3x3 convolution kernels (conv3d.hip): the dtype tags, the MFMA, max,
// store and buffer-load wrappers, LeakyReLU, and the constants the kernels were tuned to.
#pragma once

#include "common.h"

namespace exaspim {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// kInf16: the bits of +inf of a 16-bit type (the max-pools' NaN test, common.h: okey16)
struct F32Tag { static constexpr int kG = 4; static constexpr int kCode = EXASPIM_DT_F32; static constexpr unsigned kInf16 = 0x7f80; };
struct BF16Tag { static constexpr int kG = 8; static constexpr int kCode = EXASPIM_DT_BF16; static constexpr unsigned kInf16 = 0x7f80; };
struct F16Tag { static constexpr int kG = 8; static constexpr int kCode = EXASPIM_DT_F16; static constexpr unsigned kInf16 = 0x7c00; };

template <typename Tag>
__device__ __forceinline__ void mma(f32x16& acc, const uint4& wf, const uint4& xf);

template <>
__device__ __forceinline__ void mma<F32Tag>(f32x16& acc, const uint4& wf, const uint4& xf) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(wf.x), __uint_as_float(xf.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(wf.y), __uint_as_float(xf.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(wf.z), __uint_as_float(xf.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(wf.w), __uint_as_float(xf.w), acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma<BF16Tag>(f32x16& acc, const uint4& wf, const uint4& xf) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wf),
                                                  __builtin_bit_cast(bf16x8, xf), acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma<F16Tag>(f32x16& acc, const uint4& wf, const uint4& xf) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wf),
                                                 __builtin_bit_cast(f16x8, xf), acc, 0, 0, 0);
}

// In-place form for the z-column kernel: destination tied to the addend ("+v"). Left to the
// register allocator, many MFMAs of the unrolled tap loop got a destination different from
// their addend (both accumulator copies live for a while) and the kernel, already at its
// 256 registers, spilled; a spilled value comes back through a scratch load whose wait also
// waits for every prefetch load and store still in flight.
template <typename Tag>
__device__ __forceinline__ void mma_inplace(f32x16& acc, const uint4& wf, const uint4& xf) { mma<Tag>(acc, wf, xf); }
template <>
__device__ __forceinline__ void mma_inplace<BF16Tag>(f32x16& acc, const uint4& wf, const uint4& xf) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0"
                 : "+v"(acc) : "v"(__builtin_bit_cast(u32x4_t, wf)), "v"(__builtin_bit_cast(u32x4_t, xf)));
}
template <>
__device__ __forceinline__ void mma_inplace<F16Tag>(f32x16& acc, const uint4& wf, const uint4& xf) {
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0"
                 : "+v"(acc) : "v"(__builtin_bit_cast(u32x4_t, wf)), "v"(__builtin_bit_cast(u32x4_t, xf)));
}

// LeakyReLU with 0 <= slope <= 1 is max(v, slope * v): one multiply and one bare v_max_f32
// (fmaxf would put a canonicalising v_max in front of it)
__device__ __forceinline__ float leaky(float v, float slope) {
    const float sv = v * slope;
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(sv));
    return r;
}

// A copy of a value the compiler cannot see through. The persistent z-column kernel sits at its
// register ceiling; hipcc hoists every lane-derived constant of the per-tile prologue and of the
// epilogue (LDS addresses of the bias, row / column of the lane, ...) out of the tile loop and
// then SPILLS them: each came back through a scratch_load whose s_waitcnt vmcnt(0) also waited
// for the previous tile's output stores and the prefetch in flight (four serialised round trips
// at every tile top, three in every epilogue). Deriving such values from an opaque copy of the
// lane index (fresh_lane) inside the loop makes them a few VALU instructions per tile instead.
// lane index (= threadIdx.x & 63 for the 1-D workgroups here) from the hardware, two VALU
// instructions without any input register; volatile, so never hoisted and never kept
__device__ __forceinline__ int fresh_lane() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// element-wise maximum of two 16-byte channel groups in the storage type (exact: the
// inputs are already rounded, the larger one is returned bit for bit)
template <typename Tag>
__device__ __forceinline__ uint4 max16(const uint4& a, const uint4& b);
template <>
__device__ __forceinline__ uint4 max16<F32Tag>(const uint4& a, const uint4& b) {
    return max_nan4(a, b);
}
// bf16 and f16: on ordering keys (common.h: okey16 / key16x2), NaN above everything
template <>
__device__ __forceinline__ uint4 max16<BF16Tag>(const uint4& a, const uint4& b) {
    return key16(maxkey16(okey16<BF16Tag::kInf16>(a), okey16<BF16Tag::kInf16>(b)));
}
template <>
__device__ __forceinline__ uint4 max16<F16Tag>(const uint4& a, const uint4& b) {
    return key16(maxkey16(okey16<F16Tag::kInf16>(a), okey16<F16Tag::kInf16>(b)));
}

// 16-byte buffer load with hardware range check: an offset at or beyond the
// descriptor's size returns zeros, which is how the conv's zero padding (and
// the tail of the staging list) is produced without branches.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned kOutOfRange = 0x80000000u;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint4 buf_load16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, (int)soff, 0);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// store 4 consecutive output channels of one voxel
template <typename Tag>
__device__ __forceinline__ void store4(void* dst, size_t elem_off, float a, float b, float c, float d);
template <>
__device__ __forceinline__ void store4<F32Tag>(void* dst, size_t off, float a, float b, float c, float d) {
    *reinterpret_cast<float4*>(static_cast<float*>(dst) + off) = make_float4(a, b, c, d);
}
template <>
__device__ __forceinline__ void store4<BF16Tag>(void* dst, size_t off, float a, float b, float c, float d) {
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    bf16x4 v = {(__bf16)a, (__bf16)b, (__bf16)c, (__bf16)d};
    *reinterpret_cast<bf16x4*>(static_cast<__bf16*>(dst) + off) = v;
}
template <>
__device__ __forceinline__ void store4<F16Tag>(void* dst, size_t off, float a, float b, float c, float d) {
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    // saturate to the largest finite half: an activation beyond +-65504 is stored as
    // +-65504 instead of +-inf, a NaN as NaN (common.h: sat_f16, epilogue only)
    a = sat_f16(a);
    b = sat_f16(b);
    c = sat_f16(c);
    d = sat_f16(d);
    f16x4 v = {(_Float16)a, (_Float16)b, (_Float16)c, (_Float16)d};
    *reinterpret_cast<f16x4*>(static_cast<_Float16*>(dst) + off) = v;
}

// the same four channels packed into 8 bytes (16-bit storage types), for stores straight from
// registers
template <typename Tag>
__device__ __forceinline__ uint2 pack4(float a, float b, float c, float d);
template <>
__device__ __forceinline__ uint2 pack4<BF16Tag>(float a, float b, float c, float d) {
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    const bf16x4 v = {(__bf16)a, (__bf16)b, (__bf16)c, (__bf16)d};
    return __builtin_bit_cast(uint2, v);
}
template <>
__device__ __forceinline__ uint2 pack4<F16Tag>(float a, float b, float c, float d) {
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    a = sat_f16(a);   // saturating, like store4
    b = sat_f16(b);
    c = sat_f16(c);
    d = sat_f16(d);
    const f16x4 v = {(_Float16)a, (_Float16)b, (_Float16)c, (_Float16)d};
    return __builtin_bit_cast(uint2, v);
}
template <>
__device__ __forceinline__ uint2 pack4<F32Tag>(float, float, float, float) { return make_uint2(0u, 0u); }   // (unused)

// Tap loops run at a raised wave priority (s_setprio): a CU holds two workgroups, and while one is in
// its prologue / staging / epilogue (VALU, LDS writes, stores) the other one's MFMA issue should not
// queue behind it. Measured inside 512^3 steps (us per launch, two alternating repeats, r03): levels
// 0 / 1 / 2 / 3 of the z-column kernel: inc.3 803 / 786 / 783 / 785, up4.0 803 / 788 / 788 / 789,
// up4.3 499 / 486 / 484 / 486, up3.3 171 / 166 / 166 / 166; level 2 in conv3x3x3_t14 as well: the
// 17 convolutions sum to 4617 instead of 4644 us per batch. 16-bit types only: with float32 operands
// (four 16-pass MFMAs per chunk-tap) the same hint makes conv3x3x3_t14 8 - 30 % SLOWER (512^3, batch 8:
// down2.0 458 -> 608 us, up2.0 1808 -> 2439, the 17 convolutions 19.7 -> 21.5 ms per batch) and leaves
// the z-column kernel where it was.
constexpr int kSetprio = 2;      // conv3x3x3_zpipe
constexpr int kSetprioT14 = 2;   // conv3x3x3_t14, conv3x3x3_x3
// planes per tile of the trimmed fused-head launch of the z-column kernel (launch_typed)
constexpr int kHeadTZ = 5;
#ifndef EXASPIM_ABLATE
#define EXASPIM_ABLATE 0   // tools/power_probe.sh only (results wrong on purpose): 1 = no prefetch loads, 4 = no LDS staging writes
#endif
// Phase stamps for tools/conv_trace.hip (compiled out of the library).
#ifdef EXASPIM_TRACE
#define EXA_TRACE(ev)                                                                          \
    do {                                                                                       \
        if (a.trace && lane == 0)                                                              \
            a.trace[trace_rec + (ev)] = __builtin_readcyclecounter();                          \
    } while (0)
#else
#define EXA_TRACE(ev) do { } while (0)
#endif

}  // namespace exaspim
