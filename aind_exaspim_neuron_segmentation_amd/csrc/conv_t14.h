// conv3x3x3_t14 (weights through a register ring) and the split-K reduction; see conv3d.hip.
#pragma once

#include "conv_device.h"

namespace exaspim {

// ---- conv3x3x3_t14: register-staged prefetch (async-STAGE split), deeper operand
// pipelining and an LDS-transposed epilogue -------------------------------------
// The tiling and the LDS image of the head of conv3d.hip. Against the plain scheme:
//  * the next chunk's halo pieces are loaded global -> VGPR late in the current
//    chunk's tap loop (after every weight load of the chunk has been issued, so
//    the in-order vmcnt never makes a weight wait behind the prefetch), and are
//    written to LDS after the chunk's last MFMA: HBM/L2 latency hides under MFMAs
//    of the same workgroup instead of relying on a second workgroup;
//  * x fragments are double-buffered per tap (all MT reads of tap t+1 in flight
//    under the MFMAs of tap t);
//  * outputs go through LDS so every store instruction writes whole 16-byte
//    pieces of consecutive voxel records (1 KiB contiguous per instruction when
//    the tile row is 16 voxels of 32 channels).
// ZORD: walk the 27 taps in the z-column kernel's order (in-plane tap outermost, dz
// innermost) instead of dz-major, so that a voxel gets the same bits from either kernel
// (the thin remainders of a region next to z-column tiles).
// POOL: the epilogue also writes the layer's MaxPool3d(2) (the input of the next Down block,
// unet3d.py:194-196) to a.pool_dst: every wave parks all its output groups in LDS, and after one
// workgroup barrier any thread can take the maximum over a 2 x 2 x 2 block of the tile (planes z
// and z + 1 belong to different waves). The skip tensor is not read again and the separate
// max-pool launch disappears. Same bits as maxpool2_kernel: the maximum of stored values.
// ZORD and POOL together are the border launch of inc.3's row mode (launch_conv3x3x3_row, kRowStageBorders;
// TX = 2): tiles_x counts two jobs instead of tiles along x -- job 0 is x in [0, 2) of patches 1 .. n-1, job 1
// x in [w - 2, w) of patches 0 .. n-2, each in the patch's own frame -- and org / ext of the x axis are not
// read. The 2-wide tile holds exactly one pooled column, 0 respectively w/2 - 1, which the epilogue writes.
// The body of both kernels is conv_t14_body.inc.
// CARRY (conv3x3x3_t14_carry, the 16-bit 4 x 8 x 16 tile of level 1 with or without POOL): planes carried along
// z as in conv3x3x3_zpipe_rowz (ConvArgs::in_z0 .. out_shift), per patch: tiles_z counts the z tiles that are
// left, and the voxels of planes [out_z0, out_z1) are stored a second time, out_shift planes up, to carry_dst
// (POOL: their pooled planes to carry_pool_dst as well).
template <typename Tag, int TZ, int TY, int TX, int WAVES_M, int WAVES_N, int MT, int NT, int MINW, int PD,
          bool ZORD = false, bool POOL = false>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64, MINW) void conv3x3x3_t14(
    ConvArgs a, int tiles_z, int tiles_y, int tiles_x) {
    constexpr bool CARRY = false;
#include "conv_t14_body.inc"
}

// With planes carried along z (ConvArgs::in_z0 .. out_shift). A symbol of its own, and the body as text in both:
// conv3x3x3_t14 keeps its code (as a function inlined into the two, the body compiles differently: every one
// of the 52 conv3x3x3_t14 kernels came out with other instructions).
template <typename Tag, int TZ, int TY, int TX, int WAVES_M, int WAVES_N, int MT, int NT, int MINW, int PD, bool POOL>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64, MINW) void conv3x3x3_t14_carry(
    ConvArgs a, int tiles_z, int tiles_y, int tiles_x) {
    constexpr bool ZORD = false, CARRY = true;
#include "conv_t14_body.inc"
}

// The border launch of inc.3's row mode (ZORD and POOL, the TZ x 16 x 2 tile) with planes carried along z
// (launch_conv3x3x3_row, kRowStageBordersCarry). Carry in [in_z0, in_z1), even bounds and any alignment to the
// tiles: tiles_z counts the tiles over [0, in_z0) and [in_z1, d), the first segment's last tile is masked at
// in_z0, and no plane or pooled plane of the range is computed or stored. Carry out as conv3x3x3_t14_carry's,
// for both jobs in the patch's own frame: the successor's buffers then hold every x of the carried planes.
// A symbol of its own for the reason above: conv3x3x3_t14's border instantiations keep their code.
template <typename Tag, int TZ, int MT>
__global__ __launch_bounds__(256, 4) void conv3x3x3_t14_borders_carry(
    ConvArgs a, int tiles_z, int tiles_y, int tiles_x) {
    constexpr int TY = 16, TX = 2, WAVES_M = 4, WAVES_N = 1, NT = 1, PD = 3;
    constexpr bool ZORD = true, POOL = true, CARRY = true;
#include "conv_t14_body.inc"
}

// Split-K reduction: adds the float32 partial sums of the chunk ranges in range order, then
// bias, LeakyReLU and the conversion, and writes four channels of one voxel in the blocked
// layout. One thread per (voxel, 4 channels).
template <typename Tag>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ partial,
                                                            const float* __restrict__ bias,
                                                            void* __restrict__ dst, size_t nvox_all,
                                                            size_t patch_vox, int cout, int ksplit,
                                                            float slope) {
    constexpr int ES = 16 / Tag::kG;
    constexpr int KC = 2 * Tag::kG;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int quads = cout >> 2;
    if (i >= nvox_all * quads) return;
    const size_t v = i / quads;
    const int c = (int)(i - v * quads) * 4;
    float4 s = *reinterpret_cast<const float4*>(bias + c);
    for (int k = 0; k < ksplit; ++k) {
        const float4 p = *reinterpret_cast<const float4*>(partial + ((size_t)k * nvox_all + v) * cout + c);
        s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
    }
    const size_t nb = v / patch_vox, vox = v - nb * patch_vox;
    char* out = static_cast<char*>(dst) + (((size_t)nb * (cout / KC) + c / KC) * patch_vox + vox) * 32 +
                (c % KC) * ES;
    store4<Tag>(out, 0, leaky(s.x, slope), leaky(s.y, slope), leaky(s.z, slope), leaky(s.w, slope));
}

}  // namespace exaspim
