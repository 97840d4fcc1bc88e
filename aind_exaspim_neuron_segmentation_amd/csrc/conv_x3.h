// conv3x3x3_x3 / conv3x3x3_x3_head: the EXASPIM_DT_BF16X3 convolution; see conv3d.hip.
#pragma once

#include "conv_device.h"

namespace exaspim {

// ---- conv3x3x3_x3: EXASPIM_DT_BF16X3, float32-grade sums on the bf16 matrix pipe ----------
// Activations are float32 in memory (8 channels per 32-byte chunk plane, the F32Tag layout) and
// the kernel stores float32; inside, one K = 16 step of v_mfma_f32_32x32x16_bf16 consumes TWO
// chunk planes (lanes 0-31: the 8 channels of chunk 2p, lanes 32-63: those of chunk 2p + 1;
// padded channel counts are multiples of 32, so a pair never straddles the two sources). While a
// pair's halo block is staged global -> VGPR -> LDS every value v is split into
//     hi = bf16(v) (round to nearest even),  lo = bf16(v - float(hi)),
// and LDS holds a hi image and a lo image, each in the [group][halo voxel] form of 16-byte
// (8 x bf16) slots the 16-bit kernels read with one ds_read_b128 per (tap, 32 voxels). The
// weights come split the same way from the host (plan.cpp), a hi and a lo fragment per (pair,
// tap, cout tile), through the register ring of conv3x3x3_t14.
// Order of a voxel's sum, the same on every tile shape (main, thin, trimmed or not), so that
// every dispatch path gives a voxel the same bits: chunk pairs ascending (a split-K range
// after the other, the split being a function of the layer shape alone), taps dz-major, and per
// (pair, tap) the three products w_hi * x_hi, w_hi * x_lo, w_lo * x_hi; w_lo * x_lo is dropped.
// The rest is conv3x3x3_t14 without its POOL variant: the next pair's pieces are loaded
// late in the tap loop and split + written to LDS after its last MFMA, x fragments are double-
// buffered per tap, and float32 records leave through an LDS transposition.
__device__ __forceinline__ unsigned bf16_pair(float a, float b) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned, v);
}
// four float32 (bits in v) -> their four hi parts and four lo parts, 8 bytes each
__device__ __forceinline__ void split_bf16x3(const uint4& v, uint2& hi, uint2& lo) {
    const float f0 = __uint_as_float(v.x), f1 = __uint_as_float(v.y);
    const float f2 = __uint_as_float(v.z), f3 = __uint_as_float(v.w);
    hi.x = bf16_pair(f0, f1);
    hi.y = bf16_pair(f2, f3);
    lo.x = bf16_pair(f0 - __uint_as_float(hi.x << 16), f1 - __uint_as_float(hi.x & 0xffff0000u));
    lo.y = bf16_pair(f2 - __uint_as_float(hi.y << 16), f3 - __uint_as_float(hi.y & 0xffff0000u));
}

// HEAD > 0 (conv3x3x3_x3_head): the epilogue runs the 1x1x1 head with HEAD outputs on the float32
// records instead of storing them, see there.
template <int TZ, int TY, int TX, int WAVES_M, int WAVES_N, int MT, int NT, int PD, int HEAD>
__device__ __forceinline__ void x3_body(const ConvArgs& a, int tiles_z, int tiles_y, int tiles_x) {
    constexpr int HZ = TZ + 2, HY = TY + 2, HX = TX + 2;
    constexpr int PLS = HY * HX;                    // plane stride (slots)
    constexpr int HV = HZ * PLS;                    // slots of one channel-group plane = halo voxels
    constexpr int IMG = 2 * HV;                     // slots of one image (two channel groups)
    constexpr int NWAVES = WAVES_M * WAVES_N;
    constexpr int NTHREADS = NWAVES * 64;
    constexpr int TILE_VOX = TZ * TY * TX;
    constexpr int NITEMS = (2 * HV + NTHREADS - 1) / NTHREADS;   // 16-byte pieces per thread and chunk plane
    constexpr int RECB = NT * 32 * 4;               // bytes of one voxel's output slice (float32)
    constexpr int RECP = RECB + 16;                 // padded LDS stride
    constexpr int EPI_UNITS = NWAVES * 32 * RECP / 16;
    constexpr int LDS_UNITS = 2 * IMG > EPI_UNITS ? 2 * IMG : EPI_UNITS;
    constexpr int ISSUE_T = 26 - PD > 0 ? 26 - PD : 0;
    static_assert(WAVES_M * MT * 32 >= TILE_VOX, "tile not covered by the waves");

    static_assert(HEAD == 0 || NT == 1, "the head reads whole 32-channel records");

    __shared__ __attribute__((aligned(16))) uint4 lds[LDS_UNITS];
    // head weights [HEAD][32] and bias [HEAD], visible after the barrier behind the first stage_store;
    // the HEAD == 0 kernels declare nothing, so their LDS size is that of `lds` alone
    float* head_s = nullptr;
    if constexpr (HEAD > 0) {
        __shared__ __attribute__((aligned(16))) float head_lds[HEAD * 32 + 4];
        head_s = head_lds;
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N;
    const int wn = wave % WAVES_N;
    const int half = lane >> 5;
    if constexpr (HEAD > 0) {
        if (tid < HEAD * 32) head_s[tid] = a.head_w[tid];
        if (tid < HEAD) head_s[HEAD * 32 + tid] = a.head_b[tid];
    }
    // (16-wide rows: second row of a 32-voxel group in rotated x order, see conv3x3x3_t14)
    const int r = (TX == 16 && (lane & 16)) ? 16 + (((lane & 15) - HX) & 15) : (lane & 31);

    int bid;
    {
        const int nblk = gridDim.x, q = nblk >> 3, rem = nblk & 7;
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        bid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + slot;
    }
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y; bid /= tiles_y;
    const int tz = bid % tiles_z; bid /= tiles_z;
    const int nb = bid;
    const int z0 = a.org[0] + tz * TZ, y0 = a.org[1] + ty * TY, x0 = a.org[2] + tx * TX;
    const int zend = a.org[0] + a.ext[0], yend = a.org[1] + a.ext[1], xend = a.org[2] + a.ext[2];

    const int ntiles = a.cout >> 5;
    const int ntile0 = (blockIdx.y * WAVES_N + wn) * NT;

    int base[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int m = (wm * MT + mt) * 32 + r;
        m = m < TILE_VOX ? m : TILE_VOX - 1;
        const int z = m / (TY * TX), y = (m / TX) % TY, x = m % TX;
        base[mt] = z * PLS + y * HX + x + half * HV;
    }

    // staging piece i = tid + it * NTHREADS is 16-byte half i & 1 (channels 4 (i & 1) .. + 3) of halo
    // voxel i >> 1 of a chunk plane: consecutive lanes read consecutive bytes of a halo row. The same
    // offsets serve both planes of the pair.
    const size_t patch_vox = (size_t)a.d * a.h * a.w;
    unsigned voffs[NITEMS];
#pragma unroll
    for (int it = 0; it < NITEMS; ++it) {
        const int i = tid + it * NTHREADS;
        const int hv = i >> 1;
        const int hz = hv / PLS, hy = (hv / HX) % HY, hx = hv % HX;
        const int gz = z0 + hz - 1, gy = y0 + hy - 1, gx = x0 + hx - 1;
        const bool ok = i < 2 * HV && (unsigned)gz < (unsigned)a.d &&
                        (unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w;
        voffs[it] = ok ? (unsigned)((gz * a.h + gy) * a.w + gx) * 32u + (i & 1) * 16u : kOutOfRange;
    }

    f32x16 acc[MT][NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            // (split-K ranges start from zero; the reduction adds the bias)
            float4 b = *reinterpret_cast<const float4*>(a.bias + (ntile0 + nt) * 32 + 8 * q + 4 * half);
            if (a.ksplit > 1) b = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                acc[mt][nt][4 * q + 0] = b.x; acc[mt][nt][4 * q + 1] = b.y;
                acc[mt][nt][4 * q + 2] = b.z; acc[mt][nt][4 * q + 3] = b.w;
            }
        }

    // this workgroup's range of chunk pairs (all of them unless split-K)
    const int npairs_all = (a.ca + a.cb) / 16;
    const int pbeg = (int)blockIdx.z * npairs_all / a.ksplit;
    const int pend = ((int)blockIdx.z + 1) * npairs_all / a.ksplit;
    uint4 stg[2][NITEMS];

    auto stage_load = [&](int p) {
        const char* src;
        int cs, ch0;
        if (p * 16 < a.ca) {
            src = static_cast<const char*>(a.src_a); cs = a.ca; ch0 = p * 16;
        } else {
            src = static_cast<const char*>(a.src_b); cs = a.cb; ch0 = p * 16 - a.ca;
        }
        const size_t patchb = patch_vox * cs * 4;   // bytes of one patch of this source
        const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(src + (size_t)nb * patchb, patchb);
        const unsigned plane = (unsigned)patch_vox * 32u;
        const unsigned cbase = (unsigned)(ch0 / 8) * plane;   // chunk plane 2p of this source
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int it = 0; it < NITEMS; ++it) stg[g][it] = buf_load16(rsrc, voffs[it], cbase + g * plane);
    };
    // split and write: 8 bytes of the hi image and 8 of the lo image per piece
    auto stage_store = [&]() {
        uint2* const l8 = reinterpret_cast<uint2*>(lds);
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int it = 0; it < NITEMS; ++it) {
                const int i = tid + it * NTHREADS;
                if (i < 2 * HV) {
                    uint2 hi, lo;
                    split_bf16x3(stg[g][it], hi, lo);
                    l8[(g * HV) * 2 + i] = hi;
                    l8[(IMG + g * HV) * 2 + i] = lo;
                }
            }
    };

    // weight ring: [tap][cout tile][hi, lo], primed for the first PD taps of a pair before the
    // barriers in front of it
    uint4 wring[PD + 1][NT][2];
    auto wfrag = [&](int p, int t, int nt, int part) {
        return static_cast<const uint4*>(a.weights) +
               ((((size_t)p * 27 + t) * ntiles + ntile0 + nt) * 2 + part) * 64 + lane;
    };
    auto prime_weights = [&](int p) {
#pragma unroll
        for (int t = 0; t < PD; ++t)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                wring[t][nt][0] = *wfrag(p, t, nt, 0);
                wring[t][nt][1] = *wfrag(p, t, nt, 1);
            }
    };
    stage_load(pbeg);
    prime_weights(pbeg);
    stage_store();
    __syncthreads();

    for (int p = pbeg; p < pend; ++p) {
        uint4 xf[2][MT][2];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            xf[0][mt][0] = lds[base[mt]];
            xf[0][mt][1] = lds[IMG + base[mt]];
        }
        const bool more = p + 1 < pend;
        __builtin_amdgcn_s_setprio(kSetprioT14);
#pragma unroll
        for (int t = 0; t < 27; ++t) {
            if (t + PD < 27) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    wring[(t + PD) % (PD + 1)][nt][0] = *wfrag(p, t + PD, nt, 0);
                    wring[(t + PD) % (PD + 1)][nt][1] = *wfrag(p, t + PD, nt, 1);
                }
            }
            if (t == ISSUE_T && more) stage_load(p + 1);
            if (t + 1 < 27) {
                const int tn = t + 1;
                const int tapoff = (tn / 9) * PLS + ((tn / 3) % 3) * HX + tn % 3;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    xf[tn & 1][mt][0] = lds[base[mt] + tapoff];
                    xf[tn & 1][mt][1] = lds[IMG + base[mt] + tapoff];
                }
            }
            // the three products, each over all of the wave's accumulators before the next one:
            // consecutive MFMAs never depend on each other when the wave has more than one
#pragma unroll
            for (int part = 0; part < 3; ++part)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        mma<BF16Tag>(acc[mt][nt], wring[t % (PD + 1)][nt][part == 2], xf[t & 1][mt][part == 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(0);
        if (more) prime_weights(p + 1);
        __syncthreads();  // every wave is done reading this pair's images
        if (more) {
            stage_store();
            __syncthreads();
        }
    }

    if (HEAD == 0 && a.ksplit > 1) {
        // ---- split-K: float32 partial sums, [range][patch][voxel][cout] ------------------
        float* const part = a.partial + ((size_t)blockIdx.z * a.n + nb) * patch_vox * a.cout;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int m = (wm * MT + mt) * 32 + r;
            const int z = m / (TY * TX), y = (m / TX) % TY, x = m % TX;
            const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
            if (m < TILE_VOX && gz < zend && gy < yend && gx < xend) {
                float* rec = part + (((size_t)gz * a.h + gy) * a.w + gx) * a.cout;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        *reinterpret_cast<float4*>(rec + (ntile0 + nt) * 32 + 8 * q + 4 * half) =
                            make_float4(acc[mt][nt][4 * q], acc[mt][nt][4 * q + 1], acc[mt][nt][4 * q + 2],
                                        acc[mt][nt][4 * q + 3]);
            }
        }
        return;
    }

    // ---- epilogue: LeakyReLU, float32 records transposed through LDS ------------------
    char* wl = reinterpret_cast<char*>(lds) + wave * (32 * RECP);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cl = nt * 32 + 8 * q + 4 * half;  // channel inside the slice
                store4<F32Tag>(wl, (size_t)(r * RECP) / 4 + cl,
                               leaky(acc[mt][nt][4 * q + 0], a.slope), leaky(acc[mt][nt][4 * q + 1], a.slope),
                               leaky(acc[mt][nt][4 * q + 2], a.slope), leaky(acc[mt][nt][4 * q + 3], a.slope));
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if constexpr (HEAD > 0) {
            // ---- fused head: the two lanes of a voxel (lane, lane + 32) walk its record in channel
            // order, lane half h for outputs h and h + 2: head_kernel's sum (common.h: head_dot,
            // head_activation) on the values head_kernel would read back, hence its bits. Only
            // head_out is written, NCDHW float32, voxels of the region only.
            constexpr int NK = (HEAD + 1) / 2;
            const int vv = lane & 31;
            const int m = (wm * MT + mt) * 32 + vv;
            const int z = m / (TY * TX), y = (m / TX) % TY, x = m % TX;
            const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
            const bool ok = m < TILE_VOX && gz < zend && gy < yend && gx < xend;
            const size_t vox = ((size_t)gz * a.h + gy) * a.w + gx;
            const float4* const rec = reinterpret_cast<const float4*>(wl + vv * RECP);
            int oc[NK];
            float hacc[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                oc[k] = half + 2 * k < HEAD ? half + 2 * k : HEAD - 1;   // (a lane without an output repeats the last)
                hacc[k] = head_s[HEAD * 32 + oc[k]];
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 lo4 = rec[2 * g], hi4 = rec[2 * g + 1];
                const float f[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
#pragma unroll
                for (int k = 0; k < NK; ++k) hacc[k] = head_dot(hacc[k], f, head_s + oc[k] * 32 + g * 8);
            }
#pragma unroll
            for (int k = 0; k < NK; ++k)
                if (ok && half + 2 * k < HEAD)
                    a.head_out[((size_t)nb * HEAD + half + 2 * k) * patch_vox + vox] =
                        head_activation(hacc[k], a.head_sigmoid);
        } else {
            // one store instruction = one chunk plane's 32 voxel records (32 B each)
            constexpr int NPL = RECB / 32;           // chunk planes of this wave's output slice
            const int vv = lane >> 1, sub = lane & 1;
            const int m = (wm * MT + mt) * 32 + vv;
            const int z = m / (TY * TX), y = (m / TX) % TY, x = m % TX;
            const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
            const bool ok = m < TILE_VOX && gz < zend && gy < yend && gx < xend;
            const size_t vox = ((size_t)gz * a.h + gy) * a.w + gx;
            char* const dplane = static_cast<char*>(a.dst) +
                                 ((size_t)nb * (a.cout / 8) + ntile0 * 4) * patch_vox * 32;
#pragma unroll
            for (int ck = 0; ck < NPL; ++ck) {
                const uint4 val = *reinterpret_cast<const uint4*>(wl + vv * RECP + (ck * 2 + sub) * 16);
                if (ok)
                    *reinterpret_cast<uint4*>(dplane + ((size_t)ck * patch_vox + vox) * 32 + sub * 16) = val;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

template <int TZ, int TY, int TX, int WAVES_M, int WAVES_N, int MT, int NT, int MINW, int PD>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64, MINW) void conv3x3x3_x3(
    ConvArgs a, int tiles_z, int tiles_y, int tiles_x) {
    x3_body<TZ, TY, TX, WAVES_M, WAVES_N, MT, NT, PD, 0>(a, tiles_z, tiles_y, tiles_x);
}

// The level-0 32-cout tile (4 x 8 x 16, four waves, four 32-voxel groups per wave) with the 1x1x1 head
// (HEAD = 1 .. 4 outputs, optional sigmoid) in place of the store of the activations: up4.3 of the
// bf16x3 mode. The stored activation of this mode IS the float32 register value, so the fused head
// gives the bits of launch_head on the stored tensor.
constexpr int kX3HeadTZ = 4, kX3HeadTY = 8, kX3HeadTX = 16;
template <int HEAD>
__global__ __launch_bounds__(256, 2) void conv3x3x3_x3_head(ConvArgs a, int tiles_z, int tiles_y, int tiles_x) {
    x3_body<kX3HeadTZ, kX3HeadTY, kX3HeadTX, 4, 1, 4, 1, 3, HEAD>(a, tiles_z, tiles_y, tiles_x);
}

}  // namespace exaspim
