// 3x3x3 convolution (+ folded BatchNorm bias + LeakyReLU) as an implicit GEMM
// on the gfx950 matrix cores. Replaces every nn.Conv3d(k=3,p=1) ->
// BatchNorm3d(eval) -> LeakyReLU(0.01) triple of the reference's DoubleConv
// (machine_learning/unet3d.py:142-149) except inc.0 (Cin = 1, layers.hip), and
// torch.cat([skip, up], dim=1) (unet3d.py:288) by reading two sources.
//
// Layout. Activations are blocked channels-last: the (padded) channels are cut
// into chunks of 32 bytes (8 x f32 / 16 x 16-bit = the K of one MFMA step) and
// every chunk is its own plane, (N, C/chunk, D, H, W, 32 B). A row of voxels of
// one chunk is contiguous, which is what both sides of the kernel want: the K
// dimension (27 taps x Cin) is walked chunk by chunk, and the texture addresser
// handles a load instruction per 64-byte segment, so staging whole halo rows of
// one chunk costs a quarter of gathering one 16-byte piece per voxel record.
// One workgroup owns a TZ x TY x TX block of output voxels of one patch and a
// slice of 32 * NT output channels. Per chunk the (TZ+2)(TY+2)(TX+2) halo block
// sits in LDS as two planes of 16-byte channel groups, [group][halo voxel]; the
// conv's zero padding comes from range-checked buffer loads that return zeros
// outside the patch. A wave's MFMA B operand (activations, voxel on the lane) is
// ONE ds_read_b128 per (tap, 32 voxels): lanes 0-31 read group 0, lanes 32-63
// group 1. The A operand is a weight fragment in the order plan.cpp packs
// (1 KiB per wave-instruction).
//
// D = W(32 cout x K) * X(K x 32 voxels): the accumulator keeps the voxel on the
// lane and 4-channel runs in registers; the epilogue (LeakyReLU, convert; the
// folded bias is the accumulators' initial value) goes through LDS so every
// global store instruction writes 32 whole voxel records of one chunk plane.
//
// f32 uses v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain, 4 per chunk-tap),
// bf16/f16 use v_mfma_f32_32x32x16_{bf16,f16} (one per chunk-tap).
//
// Two kernels share this scheme:
//   conv3x3x3_zpipe 32-cout slices (53 % of the FLOPs): wave = a column of the
//                   tile, one LDS read feeds the three dz taps, the chunk's
//                   weights are shared through LDS, operand reads run a fixed
//                   distance ahead of the MFMAs;
//   conv3x3x3_t14   wider slices and the small pyramid levels: weights stream
//                   from L2 through a register ring.
// Both prefetch the next chunk global -> VGPR under the current chunk's MFMAs.
//
// This file is the one translation unit: the launchers, the dispatch, the predicates and the
// public entry points. The kernels live in headers it includes: conv_device.h (shared device
// helpers), conv_t14.h, conv_zcol.h (conv3x3x3_zpipe) and conv_x3.h (EXASPIM_DT_BF16X3).

#include <cstdlib>

#include "common.h"
#include "conv_device.h"
#include "conv_t14.h"
#include "conv_x3.h"
#include "conv_zcol.h"

namespace exaspim {

#ifdef EXASPIM_TRACE
int g_variant = 0;   // tools/conv_trace.hip: 3/5/6 = operand prefetch distance, +10 = one tile per workgroup
#endif

ConvLaunchRecord& last_conv_launch() {
    static thread_local ConvLaunchRecord rec;
    return rec;
}

// workgroup slots of the device for a kernel that runs MINW workgroups per CU
static int resident_workgroups(int per_cu) {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        cus = n;
    }
    return cus * per_cu;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Tiles of TZ x TY x TX voxels over the voxels the caller needs, [org, org + ext) on every axis, of
// each of n patches; ex = the x extent (a.ext[2]; row mode: the whole row's, with n = 1).
struct TileGrid {
    int tz, ty, tx;
    long long blocks;   // tz * ty * tx * n
};
static int tile_grid(const ConvArgs& a, int TZ, int TY, int TX, int ex, int n, TileGrid& g) {
    g.tz = cdiv(a.ext[0], TZ), g.ty = cdiv(a.ext[1], TY), g.tx = cdiv(ex, TX);
    g.blocks = (long long)g.tz * g.ty * g.tx * n;
    if (g.blocks <= 0 || g.blocks > 0x7fffffffLL) {
        set_error("conv: grid of %lld blocks out of range", g.blocks);
        return EXASPIM_E_INVALID;
    }
    return EXASPIM_OK;
}

// Split-K factor of a t14 / x3 launch whose chunks come in `units` (chunks, or chunk pairs), with
// `slices` cout slices per tile: when a launch of a nominal batch (16 patches) cannot give every CU
// two workgroups, up to 4 ranges of units (one at least per range), if the scratch holds the partial
// sums. The split changes the order in which a voxel's products are summed, so it is a function of
// the layer and the patch size only, never of the batch size: a patch gets the same bits whichever
// batch it travels in (predict_streaming relies on that; short batches merely fill the device less
// well).
static int choose_ksplit(const ConvArgs& a, const TileGrid& g, int slices, int units) {
    const bool whole = a.ext[0] == a.d && a.ext[1] == a.h && a.ext[2] == a.w;
    constexpr int kNominalBatch = 16;
    const long long wgs = (long long)g.tz * g.ty * g.tx * kNominalBatch * slices;
    if (!a.partial || !whole || wgs * 2 > resident_workgroups(2)) return 1;
    int ks = (int)(resident_workgroups(2) / wgs);
    if (ks > 4) ks = 4;
    if (ks > units) ks = units;
    const size_t patch_vox = (size_t)a.d * a.h * a.w;
    while (ks > 1 && (size_t)ks * patch_vox * a.cout * sizeof(float) > a.partial_patch_bytes) --ks;
    return ks;
}

// a carry field of ConvArgs is set
static bool conv_has_carry(const ConvArgs& a) {
    return a.carry_dst || a.carry_pool_dst || a.in_z0 || a.in_z1 || a.out_z0 || a.out_z1;
}

template <typename Tag, int TZ, int TY, int TX, int MINW, int D, int HEAD = 0, bool POOL = false>
static int launch_zpipe(const ConvArgs& a, hipStream_t stream) {
    // (row mode: the strip columns of the row, which the 16-wide tiles divide: launch_conv3x3x3
    // checked its geometry)
    const bool row = POOL && HEAD == 0 && Tag::kG == 8 && a.row_stride > 0;
    TileGrid g;
    if (int rc = row ? tile_grid(a, TZ, TY, TX, a.n * a.row_stride + a.w - a.row_stride, 1, g)
                     : tile_grid(a, TZ, TY, TX, a.ext[2], a.n, g))
        return rc;
    // carry in (ConvArgs::in_z0): the z tiles already present are left out of the walk
    const bool carry = row && conv_has_carry(a);
    if (carry) {
        g.tz -= (a.in_z1 - a.in_z0) / TZ;
        g.blocks = (long long)g.tz * g.ty * g.tx;
    }
    const int tz = g.tz, ty = g.ty, tx = g.tx;
    const long long blocks = g.blocks;
    // persistent workgroups: as many as the device holds at once (a multiple of the 8
    // XCDs), each walking its share of the tile list with cross-tile prefetch
    const int slices = a.cout / 32;
    long long wgs = resident_workgroups(MINW) / slices / 8 * 8;
    if (wgs < 8) wgs = 8;
    if (wgs > blocks) wgs = blocks;
#ifdef EXASPIM_TRACE
    if (g_variant >= 10 && g_variant < 20) wgs = blocks;
    // (tools/conv_trace.hip: one workgroup per CU shows what a wave's tap loop does with the matrix pipe to itself)
    if (const char* e = getenv("EXASPIM_TRACE_WGS_PER_CU")) wgs = resident_workgroups(1) * (long long)atoi(e) / slices / 8 * 8;
#endif
    dim3 grid((unsigned)wgs, slices);
    last_conv_launch() = {__PRETTY_FUNCTION__, 1};
    if constexpr (POOL && HEAD == 0 && Tag::kG == 8) {
        if (carry) {
            last_conv_launch().carry = true;
            conv3x3x3_zpipe_rowz<Tag, TZ, TY, TX, MINW, D><<<grid, TY * TX * 2, 0, stream>>>(a, tz, ty, tx);
            EXA_CHECK_HIP(hipGetLastError());
            return EXASPIM_OK;
        }
        if (row) {
            last_conv_launch().row = true;
            conv3x3x3_zpipe_row<Tag, TZ, TY, TX, MINW, D><<<grid, TY * TX * 2, 0, stream>>>(a, tz, ty, tx);
            EXA_CHECK_HIP(hipGetLastError());
            return EXASPIM_OK;
        }
    }
    conv3x3x3_zpipe<Tag, TZ, TY, TX, MINW, D, HEAD, POOL><<<grid, TY * TX * 2, 0, stream>>>(a, tz, ty, tx);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

// The row launch with rows carried along y (ConvCarryY) on top of the z carry: launch_zpipe's grid for the
// row-mode fused-pool instantiation, less the y tiles already present. (a: row arguments checked, so this is
// the configuration launch_typed picks for the layer; y: checked by check_row_y_args.)
template <typename Tag, int TZ>
static int launch_zpipe_rowzy(const ConvArgs& a, const ConvCarryY& y, hipStream_t stream) {
    constexpr int TY = 8, TX = 16, MINW = 2, D = 4;
    TileGrid g;
    if (int rc = tile_grid(a, TZ, TY, TX, a.n * a.row_stride + a.w - a.row_stride, 1, g)) return rc;
    g.tz -= (a.in_z1 - a.in_z0) / TZ;
    g.ty -= (y.in_y1 - y.in_y0) / TY;
    g.blocks = (long long)g.tz * g.ty * g.tx;
    const int slices = a.cout / 32;
    long long wgs = resident_workgroups(MINW) / slices / 8 * 8;
    if (wgs < 8) wgs = 8;
    if (wgs > g.blocks) wgs = g.blocks;
    dim3 grid((unsigned)wgs, slices);
    last_conv_launch() = {__PRETTY_FUNCTION__, 1};
    last_conv_launch().carry = true;
    last_conv_launch().carry_y = true;
    conv3x3x3_zpipe_rowzy<Tag, TZ, TY, TX, MINW, D><<<grid, TY * TX * 2, 0, stream>>>(a, y, g.tz, g.ty, g.tx);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

// ---- host side: pick a tile configuration per layer -----------------------

template <typename Tag, int TZ, int TY, int TX, int WAVES_M, int WAVES_N, int MT, int NT, int MINW, int PD = 3,
          bool ZORD = false, bool POOL = false>
static int launch_cfg(const ConvArgs& a, hipStream_t stream) {
    constexpr int NWG = WAVES_N * NT * 32;
    if (a.cout % NWG != 0) {
        set_error("conv: cout %d not a multiple of the %d-channel tile", a.cout, NWG);
        return EXASPIM_E_INVALID;
    }
    TileGrid g;
    if (int rc = tile_grid(a, TZ, TY, TX, a.ext[2], a.n, g)) return rc;
    ConvArgs b = a;
    b.ksplit = a.head_out ? 1 : choose_ksplit(a, g, a.cout / NWG, (a.ca + a.cb) / (2 * Tag::kG));   // (chunks)
    // carried planes (ConvArgs::in_z0 .. out_shift): the one configuration with a carry symbol, never split;
    // the z tiles already present are left out of the grid
    constexpr bool kCarryCfg = Tag::kG == 8 && TZ == kCarryT14TZ && TY == 8 && TX == 16 && WAVES_M == 4 && WAVES_N == 1 &&
                               MT == 4 && NT == 2 && MINW == 2 && PD == 3 && !ZORD;
    const bool carry = conv_has_carry(a);
    if (carry) {
        EXA_CHECK_ARG(kCarryCfg && b.ksplit == 1, "conv: this launch has no carried planes (tile configuration%s)",
                      b.ksplit > 1 ? ", split-K" : "");
        g.tz -= (a.in_z1 - a.in_z0) / TZ;
        g.blocks = (long long)g.tz * g.ty * g.tx * a.n;
    }
    const int tz = g.tz, ty = g.ty, tx = g.tx;
    const size_t nvox_all = (size_t)a.n * a.d * a.h * a.w;
    dim3 grid((unsigned)g.blocks, a.cout / NWG, b.ksplit);
    last_conv_launch() = {__PRETTY_FUNCTION__, b.ksplit};
    if constexpr (kCarryCfg) {
        if (carry) {
            last_conv_launch().carry = true;
            conv3x3x3_t14_carry<Tag, TZ, TY, TX, WAVES_M, WAVES_N, MT, NT, MINW, PD, POOL>
                <<<grid, WAVES_M * WAVES_N * 64, 0, stream>>>(b, tz, ty, tx);
            EXA_CHECK_HIP(hipGetLastError());
            return EXASPIM_OK;
        }
    }
    if (POOL && b.ksplit > 1) {
        // a split layer's output exists only after the reduction: its max-pool stays a launch of
        // its own (tiny layers; the split is a function of the layer, so is this choice)
        b.pool_dst = nullptr;
        conv3x3x3_t14<Tag, TZ, TY, TX, WAVES_M, WAVES_N, MT, NT, MINW, PD, ZORD, false>
            <<<grid, WAVES_M * WAVES_N * 64, 0, stream>>>(b, tz, ty, tx);
    } else {
        conv3x3x3_t14<Tag, TZ, TY, TX, WAVES_M, WAVES_N, MT, NT, MINW, PD, ZORD, POOL>
            <<<grid, WAVES_M * WAVES_N * 64, 0, stream>>>(b, tz, ty, tx);
    }
    EXA_CHECK_HIP(hipGetLastError());
    if (b.ksplit > 1) {
        const size_t items = nvox_all * (a.cout / 4);
        splitk_reduce_kernel<Tag><<<(unsigned)((items + 255) / 256), 256, 0, stream>>>(
            a.partial, a.bias, a.dst, nvox_all, (size_t)a.d * a.h * a.w, a.cout, b.ksplit, a.slope);
        EXA_CHECK_HIP(hipGetLastError());
        if (POOL)
            return launch_maxpool2(Tag::kCode, a.dst, a.pool_dst, a.n, a.d, a.h, a.w, a.cout, stream);
    }
    return EXASPIM_OK;
}

template <typename Tag> struct ES_of { static constexpr int value = 16 / Tag::kG; };   // bytes per element

// t14 configuration with or without the fused max-pool
template <typename Tag, int TZ, int TY, int TX, int WAVES_M, int WAVES_N, int MT, int NT, int MINW>
static int launch_cfg_pool(const ConvArgs& a, hipStream_t stream) {
    // (16-bit types only: with float32 records the parked groups of the 64-cout shapes take
    // 139 KB of LDS and the CU would hold one workgroup; conv_can_fuse_pool says no for those)
    if constexpr (ES_of<Tag>::value == 2) {
        if (a.pool_dst)
            return launch_cfg<Tag, TZ, TY, TX, WAVES_M, WAVES_N, MT, NT, MINW, 3, false, true>(a, stream);
    }
    return launch_cfg<Tag, TZ, TY, TX, WAVES_M, WAVES_N, MT, NT, MINW>(a, stream);
}

// 32-cout slice on z-column tiles of TZ planes, with or without the fused head
template <typename Tag, int TZ, int D>
static int launch_zpipe_head(const ConvArgs& a, hipStream_t stream) {
    if (a.head_out && a.cout == 32) {
        switch (a.head_oc) {
            case 1: return launch_zpipe<Tag, TZ, 8, 16, 2, D, 1>(a, stream);
            case 2: return launch_zpipe<Tag, TZ, 8, 16, 2, D, 2>(a, stream);
            case 3: return launch_zpipe<Tag, TZ, 8, 16, 2, D, 3>(a, stream);
            case 4: return launch_zpipe<Tag, TZ, 8, 16, 2, D, 4>(a, stream);
        }
    }
    if (a.pool_dst) return launch_zpipe<Tag, TZ, 8, 16, 2, D, 0, true>(a, stream);
    return launch_zpipe<Tag, TZ, 8, 16, 2, D>(a, stream);
}

template <typename Tag, int TZ>
static int launch_zpipe_d(const ConvArgs& a, hipStream_t stream) {
#ifdef EXASPIM_TRACE
    if (g_variant % 10 == 3) return launch_zpipe_head<Tag, TZ, 3>(a, stream);
    if (g_variant % 10 == 5) return launch_zpipe_head<Tag, TZ, 5>(a, stream);
#endif
    return launch_zpipe_head<Tag, TZ, 4>(a, stream);
}

template <typename Tag>
static int launch_typed(const ConvArgs& a, hipStream_t stream) {
    // Widest x extent first: the tile shapes follow the 96/48/24/12/6 pyramid of
    // a 96^3 patch; any other size runs on the closest shape with masking.
    if (a.w >= 16 && a.w % 16 == 0) {
        // 32-cout slices: z-column tiles with the chunk's weights shared through LDS
#ifdef EXASPIM_TRACE
        if (g_variant >= 20) return launch_zpipe_d<Tag, 6>(a, stream);
#endif
        if (a.cout % 64 != 0) {
            // the fused-head launch of the trimmed forward covers 80 planes: 16 tiles of 5 instead of 14 of 6
            // (4.8 % fewer planes; up4.3 459 -> 439 us inside 512^3 steps, same bits: a voxel's taps and
            // chunks accumulate in the same order whatever the tile)
            if (a.head_out && a.cout == 32 && a.ext[0] % 6 != 0 && a.ext[0] % kHeadTZ == 0) {
                switch (a.head_oc) {
                    case 1: return launch_zpipe<Tag, kHeadTZ, 8, 16, 2, 4, 1>(a, stream);
                    case 2: return launch_zpipe<Tag, kHeadTZ, 8, 16, 2, 4, 2>(a, stream);
                    case 3: return launch_zpipe<Tag, kHeadTZ, 8, 16, 2, 4, 3>(a, stream);
                    case 4: return launch_zpipe<Tag, kHeadTZ, 8, 16, 2, 4, 4>(a, stream);
                }
            }
            // 6-plane tiles when the depth divides (96, 48, 24): more dz reuse per LDS read
            if (conv_zcol_tile_depth(a.d) == 6) return launch_zpipe_d<Tag, 6>(a, stream);
            return launch_zpipe_d<Tag, 4>(a, stream);
        }
        if (a.pool_dst) return launch_cfg_pool<Tag, 4, 8, 16, 4, 1, 4, 2, 2>(a, stream);
        return launch_cfg<Tag, 4, 8, 16, 4, 1, 4, 2, 2>(a, stream);
    }
    if (a.w > 12) {
        if (a.cout % 64 == 0) return launch_cfg_pool<Tag, 4, 4, 24, 4, 1, 3, 2, 2>(a, stream);
        return launch_cfg_pool<Tag, 4, 4, 24, 4, 1, 3, 1, 2>(a, stream);
    }
    if (a.w > 6) {
        // 256 couts and more: 32-cout slices on two-wave workgroups fill the 256 CUs better
        // than 128-cout slices (144 tiles per batch of 16 at the 12^3 level)
        if (a.cout % 256 == 0) return launch_cfg_pool<Tag, 4, 4, 12, 2, 1, 3, 1, 2>(a, stream);
        if (a.cout % 128 == 0) return launch_cfg_pool<Tag, 4, 4, 12, 2, 2, 3, 2, 2>(a, stream);
        if (a.cout % 64 == 0) return launch_cfg_pool<Tag, 4, 4, 12, 2, 2, 3, 1, 2>(a, stream);
        return launch_cfg_pool<Tag, 4, 4, 12, 2, 1, 3, 1, 2>(a, stream);
    }
    // 6^3 level: the whole patch is one tile; 32-cout slices on four waves give the most
    // workgroups (16 patches x 8 slices for 256 couts)
    return launch_cfg<Tag, 6, 6, 6, 4, 1, 2, 1, 2>(a, stream);
}

template <int TZ, int TY, int TX, int WAVES_M, int WAVES_N, int MT, int NT, int MINW, int PD>
static int launch_x3(const ConvArgs& a, hipStream_t stream) {
    constexpr int NWG = WAVES_N * NT * 32;
    if (a.cout % NWG != 0) {
        set_error("conv: cout %d not a multiple of the %d-channel tile", a.cout, NWG);
        return EXASPIM_E_INVALID;
    }
    TileGrid g;
    if (int rc = tile_grid(a, TZ, TY, TX, a.ext[2], a.n, g)) return rc;
    const int tz = g.tz, ty = g.ty, tx = g.tx;
    ConvArgs b = a;
    b.ksplit = choose_ksplit(a, g, a.cout / NWG, (a.ca + a.cb) / 16);   // (chunk pairs)
    const size_t patch_vox_all = (size_t)a.d * a.h * a.w;
    const size_t nvox_all = (size_t)a.n * patch_vox_all;
    dim3 grid((unsigned)g.blocks, a.cout / NWG, b.ksplit);
    last_conv_launch() = {__PRETTY_FUNCTION__, b.ksplit};
    conv3x3x3_x3<TZ, TY, TX, WAVES_M, WAVES_N, MT, NT, MINW, PD>
        <<<grid, WAVES_M * WAVES_N * 64, 0, stream>>>(b, tz, ty, tx);
    EXA_CHECK_HIP(hipGetLastError());
    if (b.ksplit > 1) {
        const size_t items = nvox_all * (a.cout / 4);
        splitk_reduce_kernel<F32Tag><<<(unsigned)((items + 255) / 256), 256, 0, stream>>>(
            a.partial, a.bias, a.dst, nvox_all, patch_vox_all, a.cout, b.ksplit, a.slope);
        EXA_CHECK_HIP(hipGetLastError());
    }
    return EXASPIM_OK;
}

// bf16x3: tile shapes by the x extent, like launch_typed; every layer on conv3x3x3_x3
static int launch_typed_x3(const ConvArgs& a, hipStream_t stream) {
    if (a.w >= 16 && a.w % 16 == 0) {
        // 64 couts per workgroup on 2-plane tiles: with four 32-voxel groups per wave the two cout tiles'
        // accumulators, the operand buffers and the staged pair do not fit 256 registers
        if (a.cout % 64 == 0) return launch_x3<2, 8, 16, 4, 1, 2, 2, 2, 3>(a, stream);
        return launch_x3<4, 8, 16, 4, 1, 4, 1, 2, 3>(a, stream);
    }
    if (a.w > 12) {
        if (a.cout % 64 == 0) return launch_x3<4, 4, 24, 4, 1, 3, 2, 2, 1>(a, stream);
        return launch_x3<4, 4, 24, 4, 1, 3, 1, 2, 3>(a, stream);
    }
    if (a.w > 6) {
        // (the shapes of launch_typed at this level)
        if (a.cout % 256 == 0) return launch_x3<4, 4, 12, 2, 1, 3, 1, 2, 3>(a, stream);
        if (a.cout % 128 == 0) return launch_x3<4, 4, 12, 2, 2, 3, 2, 2, 2>(a, stream);
        if (a.cout % 64 == 0) return launch_x3<4, 4, 12, 2, 2, 3, 1, 2, 3>(a, stream);
        return launch_x3<4, 4, 12, 2, 1, 3, 1, 2, 3>(a, stream);
    }
    return launch_x3<6, 6, 6, 4, 1, 2, 1, 2, 3>(a, stream);
}

// thin remainders of a region: 8 x 2 x 16 (thin along y) or 8 x 16 x 2 (thin along x) tiles
static int launch_thin_typed_x3(const ConvArgs& a, hipStream_t stream) {
    if (a.ext[1] <= a.ext[2]) return launch_x3<8, 2, 16, 4, 1, 2, 1, 2, 3>(a, stream);
    return launch_x3<8, 16, 2, 4, 1, 2, 1, 2, 3>(a, stream);
}

template <int HEAD>
static int launch_x3_head(const ConvArgs& a, hipStream_t stream) {
    TileGrid g;
    if (int rc = tile_grid(a, kX3HeadTZ, kX3HeadTY, kX3HeadTX, a.ext[2], a.n, g)) return rc;
    last_conv_launch() = {__PRETTY_FUNCTION__, 1};
    conv3x3x3_x3_head<HEAD><<<dim3((unsigned)g.blocks, 1, 1), 256, 0, stream>>>(a, g.tz, g.ty, g.tx);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

bool conv_can_fuse_pool(int dtype, int cout, int d, int h, int w) {
    if (d % 2 != 0 || h % 2 != 0 || w % 2 != 0) return false;
    if (dtype == EXASPIM_DT_BF16X3) return false;   // conv3x3x3_x3 has no fused max-pool
    // the layers launch_typed sends to the z-column kernel (any dtype) ...
    if (cout % 64 != 0 && w >= 16 && w % 16 == 0) return true;
    // ... and, in the 16-bit modes, every other tile shape but the single-tile 6^3 one
    return dtype != EXASPIM_DT_F32 && w > 6;
}

// the layer shape every fused head runs on: the 32-cout level-0 tile on 16-wide rows, 1 .. 4 outputs
static bool head_shape_ok(int cout, int w, int head_oc) {
    return cout == 32 && w >= 16 && w % 16 == 0 && head_oc >= 1 && head_oc <= 4;
}
// (what launch_conv3x3x3 accepts: bf16x3 has its fused head behind a launcher of its own)
bool conv_can_fuse_head(int cout, int w, int head_oc, int dtype) {
    return dtype != EXASPIM_DT_BF16X3 && head_shape_ok(cout, w, head_oc);
}
// (what launch_conv3x3x3_x3_head accepts)
bool conv_x3_can_fuse_head(int cout, int w, int head_oc) { return head_shape_ok(cout, w, head_oc); }

// ext = 0 stands for the whole axis; the region must lie inside the patch
static int resolve_region(ConvArgs& a) {
    const int dims[3] = {a.d, a.h, a.w};
    for (int i = 0; i < 3; ++i) {
        if (a.ext[i] == 0 && a.org[i] == 0) a.ext[i] = dims[i];
        EXA_CHECK_ARG(a.org[i] >= 0 && a.ext[i] > 0 && a.org[i] + a.ext[i] <= dims[i],
                      "conv: region [%d, %d) outside axis %d of a %dx%dx%d patch", a.org[i],
                      a.org[i] + a.ext[i], i, a.d, a.h, a.w);
    }
    return EXASPIM_OK;
}

int conv_zcol_tile_depth(int d) { return d % 6 == 0 ? 6 : 4; }

int conv_carry_t14_tile_depth(int dtype, const ConvArgs& a) {
    // launch_typed sends a 64-cout slice on 16-wide rows to the 4 x 8 x 16 configuration of conv3x3x3_t14, the
    // one launch_cfg has a carry symbol for; launch_cfg refuses carried planes on any other and on a split launch
    if (dtype_size(dtype) != 2 || dtype == EXASPIM_DT_BF16X3 || a.head_out || a.row_stride != 0) return 0;
    if (!(a.w >= 16 && a.w % 16 == 0 && a.cout % 64 == 0 && a.d % kCarryT14TZ == 0)) return 0;
    ConvArgs b = a;
    for (int i = 0; i < 3; ++i) b.org[i] = b.ext[i] = 0;
    if (resolve_region(b) != EXASPIM_OK) return 0;
    TileGrid g;
    if (tile_grid(b, kCarryT14TZ, 8, 16, b.ext[2], b.n, g) != EXASPIM_OK) return 0;
    return choose_ksplit(b, g, b.cout / 64, (b.ca + b.cb) / 16) == 1 ? kCarryT14TZ : 0;
}

int conv_zcol_main_extent(int ext, int axis) {
    const int tile = axis == 1 ? 8 : 16;   // the z-column kernel's TY / TX
    const int rem = ext % tile;
    return (axis != 0 && ext > tile && rem >= 1 && rem <= 4) ? ext - rem : ext;
}

bool conv_row_mode_ok(int dtype, int cout, int n, int w, int row_stride, bool fused_pool_whole_patch) {
    // the strip columns must line up with the 16-wide z-column tiles of every patch, and a shared
    // column must keep its neighbour's two outermost x inside it
    const int o = w - row_stride;
    return dtype_size(dtype) == 2 && fused_pool_whole_patch && cout % 64 != 0 &&
           w % 16 == 0 && n >= 2 && row_stride > 0 && o > 0 && o % 32 == 0 && row_stride >= o;
}

// (a: region resolved)
static int check_row_args(int dtype, const ConvArgs& a) {
    const bool whole = a.ext[0] == a.d && a.ext[1] == a.h && a.ext[2] == a.w;
    EXA_CHECK_ARG(conv_row_mode_ok(dtype, a.cout, a.n, a.w, a.row_stride,
                                   a.pool_dst && !a.head_out && whole &&
                                       conv_can_fuse_pool(dtype, a.cout, a.d, a.h, a.w)),
                  "conv: row mode needs a 16-bit fused-pool z-column layer, whole patches, n >= 2 and "
                  "an overlap that is a multiple of 32 and at most the stride (w %d, stride %d, n %d)",
                  a.w, a.row_stride, a.n);
    // carry: planes whose inputs stay clear of the zero padding along z, [2, d - 2), in whole plane pairs
    const int tzd = conv_zcol_tile_depth(a.d);
    EXA_CHECK_ARG(a.in_z0 <= a.in_z1 && a.in_z0 % 2 == 0 && a.in_z1 % 2 == 0 && a.in_z0 % tzd == 0 && a.in_z1 % tzd == 0 &&
                      (a.in_z0 == a.in_z1 || (a.in_z0 >= 2 && a.in_z1 <= a.d - 2)),
                  "conv: carry in [%d, %d) must be whole %d-plane tiles with even bounds inside [2, %d)", (int)a.in_z0,
                  (int)a.in_z1, tzd, a.d - 2);
    const bool out = a.carry_dst || a.carry_pool_dst || a.out_z0 || a.out_z1;
    EXA_CHECK_ARG(!out || (a.carry_dst && a.carry_pool_dst && a.out_z0 < a.out_z1 && a.out_z0 % 2 == 0 && a.out_z1 % 2 == 0 &&
                           a.out_z0 >= 2 && a.out_z1 <= a.d - 2 && a.out_shift > 0 && a.out_shift % 2 == 0 &&
                           (int)a.out_z0 - a.out_shift >= 2),
                  "conv: carry out [%d, %d) shifted by %d needs both targets, even bounds and source and target planes "
                  "inside [2, %d)", (int)a.out_z0, (int)a.out_z1, a.out_shift, a.d - 2);
    return EXASPIM_OK;
}

// Rows carried along y (ConvCarryY; a: row arguments checked). Carry in: whole 8-row tiles of the z-column
// kernel inside [2, h - 2). Carry out: even bounds, source and target rows inside [2, h - 2); it stores again
// only rows this launch computes, so a range that meets the rows carried in is refused. The diagonal target
// needs both carries out.
static int check_row_y_args(const ConvArgs& a, const ConvCarryY& y) {
    constexpr int TY = 8;
    EXA_CHECK_ARG(y.in_y0 <= y.in_y1 && y.in_y0 % TY == 0 && y.in_y1 % TY == 0 &&
                      (y.in_y0 == y.in_y1 || (y.in_y0 >= 2 && y.in_y1 <= a.h - 2)),
                  "conv: y carry in [%d, %d) must be whole %d-row tiles inside [2, %d)", (int)y.in_y0, (int)y.in_y1, TY,
                  a.h - 2);
    const bool out = y.y_dst || y.y_pool_dst || y.d_dst || y.d_pool_dst || y.out_y0 || y.out_y1 || y.out_shift_y;
    EXA_CHECK_ARG(!out || (y.y_dst && y.y_pool_dst && y.out_y0 < y.out_y1 && y.out_y0 % 2 == 0 && y.out_y1 % 2 == 0 &&
                           y.out_y0 >= 2 && y.out_y1 <= a.h - 2 && y.out_shift_y > 0 && y.out_shift_y % 2 == 0 &&
                           (int)y.out_y0 - y.out_shift_y >= 2),
                  "conv: y carry out [%d, %d) shifted by %d needs both targets, even bounds and source and target rows "
                  "inside [2, %d)", (int)y.out_y0, (int)y.out_y1, (int)y.out_shift_y, a.h - 2);
    EXA_CHECK_ARG(!out || y.in_y0 == y.in_y1 || y.out_y0 >= y.in_y1 || y.out_y1 <= y.in_y0,
                  "conv: y carry out [%d, %d) overlaps the rows carried in, [%d, %d)", (int)y.out_y0, (int)y.out_y1,
                  (int)y.in_y0, (int)y.in_y1);
    EXA_CHECK_ARG(!y.d_dst == !y.d_pool_dst && (!y.d_dst || (out && a.carry_dst)),
                  "conv: the diagonal carry out needs both targets and both the z and the y carry out");
    EXA_CHECK_ARG(!y.d_dst || a.in_z0 == a.in_z1 || a.out_z0 >= a.in_z1 || a.out_z1 <= a.in_z0,
                  "conv: carry out [%d, %d) overlaps the planes carried in, [%d, %d)", (int)a.out_z0, (int)a.out_z1,
                  (int)a.in_z0, (int)a.in_z1);
    return EXASPIM_OK;
}

// Carried planes without row mode (conv3x3x3_t14_carry; a: region resolved): planes whose inputs stay clear of
// the zero padding along z, [2, d - 2), in whole tiles and whole plane pairs
static int check_carry_args(int dtype, const ConvArgs& a, bool whole) {
    const int tzd = conv_carry_t14_tile_depth(dtype, a);
    EXA_CHECK_ARG(tzd > 0 && whole,
                  "conv: carried planes need row mode or a whole-patch 16-bit 64-cout-slice layer on 16-wide rows "
                  "that is not split (%dx%dx%d, cout %d)", a.d, a.h, a.w, a.cout);
    EXA_CHECK_ARG(a.in_z0 <= a.in_z1 && a.in_z0 % 2 == 0 && a.in_z1 % 2 == 0 && a.in_z0 % tzd == 0 && a.in_z1 % tzd == 0 &&
                      (a.in_z0 == a.in_z1 || (a.in_z0 >= 2 && a.in_z1 <= a.d - 2)),
                  "conv: carry in [%d, %d) must be whole %d-plane tiles with even bounds inside [2, %d)", (int)a.in_z0,
                  (int)a.in_z1, tzd, a.d - 2);
    const bool out = a.carry_dst || a.carry_pool_dst || a.out_z0 || a.out_z1;
    EXA_CHECK_ARG(!out || (a.carry_dst && !a.carry_pool_dst == !a.pool_dst && a.out_z0 < a.out_z1 && a.out_z0 % 2 == 0 &&
                           a.out_z1 % 2 == 0 && a.out_z0 >= 2 && a.out_z1 <= a.d - 2 && a.out_shift > 0 &&
                           a.out_shift % 2 == 0 && (int)a.out_z0 - a.out_shift >= 2),
                  "conv: carry out [%d, %d) shifted by %d needs a target (a pooled one exactly with a fused max-pool), "
                  "even bounds and source and target planes inside [2, %d)", (int)a.out_z0, (int)a.out_z1, a.out_shift,
                  a.d - 2);
    return EXASPIM_OK;
}

// The argument checks the public launchers share; `checks` names the ones a launcher makes.
enum : unsigned { kCheckPadded = 1, kCheckEmpty = 2, kCheckSlope = 4, kCheckPatchBytes = 8, kCheckAll = 15 };
static int check_conv_args(int dtype, const ConvArgs& a, unsigned checks) {
    const int kc = dtype == EXASPIM_DT_F32 ? 8 : 16;   // (bf16x3: a pair of float32 chunk planes)
    EXA_CHECK_ARG(!(checks & kCheckPadded) || (a.ca % kc == 0 && a.cb % kc == 0 && a.cout % 32 == 0 && a.ca > 0),
                  "conv: channels (%d,%d)->%d not padded", a.ca, a.cb, a.cout);
    EXA_CHECK_ARG(!(checks & kCheckEmpty) || (a.n > 0 && a.d > 0 && a.h > 0 && a.w > 0), "conv: empty input");
    EXA_CHECK_ARG(!(checks & kCheckSlope) || (a.slope >= 0.f && a.slope <= 1.f),
                  "conv: LeakyReLU slope %g outside [0, 1]", a.slope);
    // the staging loads address one patch of one source with 32-bit buffer offsets
    const unsigned long long rec = (unsigned long long)a.d * a.h * a.w * (a.ca > a.cb ? a.ca : a.cb) * dtype_size(dtype);
    EXA_CHECK_ARG(!(checks & kCheckPatchBytes) || rec < 0x80000000ULL,
                  "conv: one patch of one source is %llu bytes (>= 2 GiB)", rec);
    return EXASPIM_OK;
}

int launch_conv3x3x3(int dtype, const ConvArgs& a_in, hipStream_t stream) {
    ConvArgs a = a_in;
    if (int rc = check_conv_args(dtype, a, kCheckAll)) return rc;
    if (int rc = resolve_region(a)) return rc;
    const bool whole = a.ext[0] == a.d && a.ext[1] == a.h && a.ext[2] == a.w;
    EXA_CHECK_ARG(!a.pool_dst || (conv_can_fuse_pool(dtype, a.cout, a.d, a.h, a.w) && !a.head_out && whole),
                  "conv: fused max-pool needs an even, untrimmed patch (16-bit modes: wider than 6 voxels; "
                  "float32: a 32-cout-slice layer)");
    EXA_CHECK_ARG(!a.head_out || conv_can_fuse_head(a.cout, a.w, a.head_oc, dtype),
                  "conv: fused head needs cout 32, w %% 16 == 0, 1..4 outputs (and not bf16x3)");
    if (a.row_stride > 0) {
        if (int rc = check_row_args(dtype, a)) return rc;
    } else if (conv_has_carry(a)) {
        if (int rc = check_carry_args(dtype, a, whole)) return rc;
    }
    switch (dtype) {
        case EXASPIM_DT_F32: return launch_typed<F32Tag>(a, stream);
        case EXASPIM_DT_BF16: return launch_typed<BF16Tag>(a, stream);
        case EXASPIM_DT_F16: return launch_typed<F16Tag>(a, stream);
        case EXASPIM_DT_BF16X3: return launch_typed_x3(a, stream);
    }
    set_error("conv: unknown dtype %d", dtype);
    return EXASPIM_E_INVALID;
}

int launch_conv3x3x3_x3_head(const ConvArgs& a_in, hipStream_t stream) {
    ConvArgs a = a_in;
    if (int rc = check_conv_args(EXASPIM_DT_BF16X3, a, kCheckAll)) return rc;
    EXA_CHECK_ARG(conv_x3_can_fuse_head(a.cout, a.w, a.head_oc),
                  "conv: bf16x3 fused head needs cout 32, w %% 16 == 0 and 1..4 outputs (cout %d, w %d, %d outputs)",
                  a.cout, a.w, a.head_oc);
    EXA_CHECK_ARG(a.head_out && a.head_w && a.head_b, "conv: bf16x3 fused head: NULL head pointer");
    EXA_CHECK_ARG(!a.pool_dst && a.row_stride == 0, "conv: bf16x3 fused head has no fused max-pool or row mode");
    if (int rc = resolve_region(a)) return rc;
    a.partial = nullptr;   // no split-K: the head needs a voxel's whole sum
    a.ksplit = 1;
    switch (a.head_oc) {
        case 1: return launch_x3_head<1>(a, stream);
        case 2: return launch_x3_head<2>(a, stream);
        case 3: return launch_x3_head<3>(a, stream);
        default: return launch_x3_head<4>(a, stream);
    }
}

template <typename Tag>
static int launch_thin_typed(const ConvArgs& a, hipStream_t stream) {
    // 2-voxel-thick tiles: thin along y (TZ x 2 x 16) or along x (TZ x 16 x 2), four waves. A wave owns
    // TZ / 4 groups of 32 voxels, so a weight fragment fetched through the L2 ring feeds that many
    // MFMAs and the z halo is shared by more planes: measured inside 512^3 steps on up4.0's two
    // remainders (82 planes, rocprofv3, us per launch) thin along y 54.2 / 42.3 - 44.5 / 36.0 for
    // TZ = 4 / 8 / 12 (three workgroups per CU for 12), thin along x 56.6 / 45.7 / 47.4 - 51.9 (its
    // 2-voxel rows keep 50 % LDS bank conflicts). The depth is picked per launch: padded planes x
    // the relative cost per plane from those measurements.
    const int ez = a.ext[0];
    auto planes = [&](int tz) { return (ez + tz - 1) / tz * tz; };
    if (a.ext[1] <= a.ext[2]) {
        const float c4 = planes(4) * 1.00f, c8 = planes(8) * 0.76f, c12 = planes(12) * 0.66f;
        if (c12 <= c8 && c12 <= c4) return launch_cfg<Tag, 12, 2, 16, 4, 1, 3, 1, 3, 3, true>(a, stream);
        if (c8 <= c4) return launch_cfg<Tag, 8, 2, 16, 4, 1, 2, 1, 4, 3, true>(a, stream);
        return launch_cfg<Tag, 4, 2, 16, 4, 1, 1, 1, 4, 3, true>(a, stream);
    }
    if (planes(8) * 0.78f <= planes(4) * 1.00f) return launch_cfg<Tag, 8, 16, 2, 4, 1, 2, 1, 4, 3, true>(a, stream);
    return launch_cfg<Tag, 4, 16, 2, 4, 1, 1, 1, 4, 3, true>(a, stream);
}

int launch_conv3x3x3_thin(int dtype, const ConvArgs& a_in, hipStream_t stream) {
    ConvArgs a = a_in;
    if (int rc = check_conv_args(dtype, a, kCheckPadded | kCheckEmpty)) return rc;   // (as ever: no slope or size check here)
    EXA_CHECK_ARG(!a.pool_dst && !a.head_out && a.row_stride == 0 && !conv_has_carry(a),
                  "conv: thin tiles have no fused pool, head, row mode or carried planes");
    if (int rc = resolve_region(a)) return rc;
    a.partial = nullptr;   // no split-K on a partial region
    switch (dtype) {
        case EXASPIM_DT_F32: return launch_thin_typed<F32Tag>(a, stream);
        case EXASPIM_DT_BF16: return launch_thin_typed<BF16Tag>(a, stream);
        case EXASPIM_DT_F16: return launch_thin_typed<F16Tag>(a, stream);
        case EXASPIM_DT_BF16X3: return launch_thin_typed_x3(a, stream);
    }
    set_error("conv: unknown dtype %d", dtype);
    return EXASPIM_E_INVALID;
}

// Row mode, both border faces in one launch (kRowStageBorders): 2-voxel-thick tiles along x like
// launch_thin_typed's, tiles_x = the two jobs of conv3x3x3_t14's ZORD + POOL instantiation
template <typename Tag, int TZ, int MT>
static int launch_row_borders_cfg(const ConvArgs& a, hipStream_t stream) {
    const int tz = cdiv(a.d, TZ), ty = cdiv(a.h, 16);
    const long long blocks = (long long)tz * ty * 2 * (a.n - 1);
    if (blocks <= 0 || blocks > 0x7fffffffLL) {
        set_error("conv: grid of %lld blocks out of range", blocks);
        return EXASPIM_E_INVALID;
    }
    last_conv_launch() = {__PRETTY_FUNCTION__, 1};
    conv3x3x3_t14<Tag, TZ, 16, 2, 4, 1, MT, 1, 4, 3, true, true>
        <<<dim3((unsigned)blocks, a.cout / 32, 1), 256, 0, stream>>>(a, tz, ty, 2);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

// the tile depth launch_thin_typed picks for tiles thin along x
int conv_row_borders_tile_depth(int d) {
    auto planes = [&](int tz) { return (d + tz - 1) / tz * tz; };
    return planes(8) * 0.78f <= planes(4) * 1.00f ? 8 : 4;
}

// ... with planes carried along z (kRowStageBordersCarry, conv3x3x3_t14_borders_carry): the z tiles cover
// [0, in_z0) and [in_z1, d) only
template <typename Tag, int TZ, int MT>
static int launch_row_borders_carry_cfg(const ConvArgs& a, hipStream_t stream) {
    const int tz = cdiv(a.in_z0, TZ) + cdiv(a.d - a.in_z1, TZ), ty = cdiv(a.h, 16);
    const long long blocks = (long long)tz * ty * 2 * (a.n - 1);
    if (blocks <= 0 || blocks > 0x7fffffffLL) {
        set_error("conv: grid of %lld blocks out of range", blocks);
        return EXASPIM_E_INVALID;
    }
    last_conv_launch() = {__PRETTY_FUNCTION__, 1};
    last_conv_launch().carry = true;
    conv3x3x3_t14_borders_carry<Tag, TZ, MT>
        <<<dim3((unsigned)blocks, a.cout / 32, 1), 256, 0, stream>>>(a, tz, ty, 2);
    EXA_CHECK_HIP(hipGetLastError());
    return EXASPIM_OK;
}

// (a: whole patches, row arguments checked; carry fields set: the launch honours them)
template <typename Tag>
static int launch_row_borders(const ConvArgs& a_in, hipStream_t stream) {
    ConvArgs a = a_in;
    a.partial = nullptr;   // no split-K
    a.ksplit = 1;
    a.row_stride = 0;
    const bool deep = conv_row_borders_tile_depth(a.d) == 8;
    if (conv_has_carry(a))
        return deep ? launch_row_borders_carry_cfg<Tag, 8, 2>(a, stream) : launch_row_borders_carry_cfg<Tag, 4, 1>(a, stream);
    if (deep) return launch_row_borders_cfg<Tag, 8, 2>(a, stream);
    return launch_row_borders_cfg<Tag, 4, 1>(a, stream);
}

int launch_conv3x3x3_row(int dtype, const ConvArgs& a, int stages, hipStream_t stream, const ConvCarryY* y) {
    ConvArgs b = a;
    if (int rc = check_conv_args(dtype, a, kCheckEmpty)) return rc;   // (the main stage checks the rest)
    if (int rc = resolve_region(b)) return rc;
    if (int rc = check_row_args(dtype, b)) return rc;
    const bool carry_y = y && conv_has_carry_y(*y);
    if (carry_y) {
        if (int rc = check_row_y_args(b, *y)) return rc;
    }
    // (the planes carried in are not computed by the border launch either: nothing could store them a second time)
    EXA_CHECK_ARG(!(stages & kRowStageBordersCarry) || a.in_z0 == a.in_z1 || a.out_z0 == a.out_z1 ||
                      a.out_z0 >= a.in_z1 || a.out_z1 <= a.in_z0,
                  "conv: carry out [%d, %d) overlaps the planes carried in, [%d, %d)", (int)a.out_z0, (int)a.out_z1,
                  (int)a.in_z0, (int)a.in_z1);
    int r = EXASPIM_OK;
    if ((stages & kRowStageMain) && carry_y) {
        // (the main launch alone takes rows over: the border launches compute every row of their columns)
        r = check_conv_args(dtype, a, kCheckAll);
        const bool six = conv_zcol_tile_depth(a.d) == 6;
        if (r == EXASPIM_OK)    // (check_row_args: a 16-bit type, whole patches, the fused pool, no head)
            r = dtype == EXASPIM_DT_F16 ? (six ? launch_zpipe_rowzy<F16Tag, 6>(b, *y, stream) : launch_zpipe_rowzy<F16Tag, 4>(b, *y, stream))
                                        : (six ? launch_zpipe_rowzy<BF16Tag, 6>(b, *y, stream) : launch_zpipe_rowzy<BF16Tag, 4>(b, *y, stream));
    } else if (stages & kRowStageMain) {
        r = launch_conv3x3x3(dtype, a, stream);
    }
    // x in [0, 2) of patches 1 .. n-1 and [w - 2, w) of patches 0 .. n-2, then pooled x 0 and
    // w/2 - 1 of every patch
    b.pool_dst = nullptr;
    b.row_stride = 0;
    b.carry_dst = b.carry_pool_dst = nullptr;   // (the border launches write every plane, and only dst / pool_dst)
    b.in_z0 = b.in_z1 = b.out_z0 = b.out_z1 = 0;
    b.out_shift = 0;
    b.n = a.n - 1;
    b.ext[2] = 2;
    if (r == EXASPIM_OK && (stages & kRowStageThin)) {
        const size_t vox = (size_t)a.d * a.h * a.w;
        b.src_a = static_cast<const char*>(a.src_a) + vox * a.ca * dtype_size(dtype);
        b.dst = static_cast<char*>(a.dst) + vox * a.cout * dtype_size(dtype);
        r = launch_conv3x3x3_thin(dtype, b, stream);
        if (r == EXASPIM_OK) {
            b.org[2] = a.w - 2;
            b.src_a = a.src_a;
            b.dst = a.dst;
            r = launch_conv3x3x3_thin(dtype, b, stream);
        }
    }
    if (r == EXASPIM_OK && (stages & kRowStagePool))
        r = launch_maxpool2_xcols(dtype, a.dst, a.pool_dst, a.n, a.d, a.h, a.w, a.cout, 0, a.w / 2 - 1, stream);
    if (r == EXASPIM_OK && (stages & kRowStageBorders)) {
        r = check_conv_args(dtype, a, kCheckPadded);
        ConvArgs c = a;
        for (int i = 0; i < 3; ++i) { c.org[i] = b.org[i]; c.ext[i] = b.ext[i]; }   // (resolved: whole patches)
        c.carry_dst = c.carry_pool_dst = nullptr;
        c.in_z0 = c.in_z1 = c.out_z0 = c.out_z1 = 0;
        c.out_shift = 0;
        c.org[2] = 0;
        if (r == EXASPIM_OK)    // (check_row_args: a 16-bit type)
            r = dtype == EXASPIM_DT_F16 ? launch_row_borders<F16Tag>(c, stream) : launch_row_borders<BF16Tag>(c, stream);
    }
    if (r == EXASPIM_OK && (stages & kRowStageBordersCarry)) {
        // the same launch honouring the carry fields (check_row_args: even bounds inside [2, d - 2))
        r = check_conv_args(dtype, a, kCheckPadded);
        ConvArgs c = a;
        for (int i = 0; i < 3; ++i) { c.org[i] = b.org[i]; c.ext[i] = b.ext[i]; }   // (resolved: whole patches)
        c.org[2] = 0;
        if (r == EXASPIM_OK)
            r = dtype == EXASPIM_DT_F16 ? launch_row_borders<F16Tag>(c, stream) : launch_row_borders<BF16Tag>(c, stream);
    }
    return r;
}

}  // namespace exaspim
