// conv3x3x3_zpipe / conv3x3x3_zpipe_row: the z-column kernel of the 32-cout slices; see conv3d.hip.
#pragma once

#include "conv_device.h"

namespace exaspim {

// ---- conv3x3x3_zpipe: z-column tiles for the 32-cout slices ----------------------------
// A wave owns one 32-voxel (y, x) group of the tile times all TZ planes (TZ
// accumulators). For a fixed in-plane tap g = (dy, dx) the operand fragment of
// input plane zin is the B operand of up to three MFMAs (dz = 0, 1, 2 -> output
// planes zin, zin-1, zin-2): (TZ + 2) LDS reads per 3 * TZ MFMAs. The chunk's 27
// weight fragments are staged in LDS too (one copy per workgroup instead of one L2
// read per wave).
//
// Shaped by two measurements (tools/conv_trace.hip): a workgroup spends ~45 % of
// its life outside the tap loops, so most of the time a SIMD has ONE wave feeding
// its matrix pipe, and a wave whose operand reads sit right before the MFMAs that
// use them reaches only ~70 % alone. Hence
//  * the tap loop is one flat sequence of 9 * (TZ + 2) steps (g, zin); the operand
//    fragment of step s + D is read from LDS before the MFMAs of step s into a ring
//    of D + 1 registers, the next tap's three weight fragments are read one tap
//    ahead, and a scheduling fence per step pins that order, so LDS latency hides
//    under the wave's own MFMAs;
//  * the next chunk's global loads are dealt one per step;
//  * staging maps (column, 16-byte group) pairs to lanes, so with the blocked
//    layout a load instruction covers whole halo rows of contiguous bytes (the
//    texture addresser works per 64-byte segment: 16 cycles per instruction
//    instead of 64 with one voxel record per lane).
template <typename Tag, int TZ, int TY, int TX, int MINW, int D, int HEAD, bool POOL, bool ROW, bool CARRY = false,
          bool CARRYY = false>
__device__ __forceinline__ void zpipe_body(const ConvArgs& a, int tiles_z, int tiles_y, int tiles_x,
                                           const ConvCarryY& cy = ConvCarryY{}) {
    constexpr int G = Tag::kG;
    constexpr int KC = 2 * G;
    constexpr int ES = 16 / G;
    constexpr int HZ = TZ + 2, HY = TY + 2, HX = TX + 2;
    constexpr int HXP = HX;                // row stride (slots)
    constexpr int PLANE = HY * HXP;        // slots per halo plane
    constexpr int HVP = HZ * PLANE;        // slots per channel group
    // stride between the two channel-group planes: an odd multiple of 128 bytes, so the
    // lane pair that stages one voxel (group 0, group 1) writes different LDS banks
    constexpr int GS = HVP + (24 - HVP % 16) % 16;
    constexpr int NWAVES = TY * TX / 32;
    constexpr int NTHREADS = NWAVES * 64;
    constexpr int NPAIR = 2 * HY * HX;     // (column, group) pairs of the halo block
    constexpr int REM = NPAIR > NTHREADS ? NPAIR - NTHREADS : 0;
    constexpr int SEC = (REM * HZ + NTHREADS - 1) / NTHREADS;
    constexpr int NITEMS = HZ + SEC;       // halo pieces per thread
    constexpr int RECB = 32 * ES;
    constexpr int RECP = RECB + 16;        // padded LDS stride of the output transposition
    constexpr int EPI_UNITS = NWAVES * 32 * RECP / 16;
    constexpr int WUNITS = 27 * 64;        // the chunk's weight fragments in LDS
    constexpr int WITEMS = (WUNITS + NTHREADS - 1) / NTHREADS;
    constexpr int XUNITS = 2 * GS > EPI_UNITS ? 2 * GS : EPI_UNITS;
    constexpr int LDS_UNITS = XUNITS + WUNITS;
    constexpr int NS = 9 * HZ;             // steps per chunk
    constexpr int R = D + 1;               // operand ring
    // steps between two staged pieces (see the tap loop). Stride 1 / 2 / 3 inside a 1024^3 step (us per
    // launch, same box): up3.3 + up4.0 510 / 490 / 496, inc.3 831 / 801 / 801, up4.3 with the fused head
    // 514 / 496 / 536. Tiles whose pieces do not fit into the steps at stride 2 fall back to 1.
    constexpr int kLoadStride = 2;
    constexpr int LOAD_STRIDE = kLoadStride * (NITEMS + WITEMS) <= NS ? kLoadStride : 1;
    static_assert(TY * TX % 32 == 0 && NPAIR <= 2 * NTHREADS, "tile shape");
    static_assert(LOAD_STRIDE * (NITEMS + WITEMS) <= NS, "the staged pieces fit into the steps");

    __shared__ __attribute__((aligned(16))) uint4 lds[LDS_UNITS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    // Voxel of the 32-group this lane works on. With 16-wide rows the group is two
    // rows whose LDS slots differ by HXP; taking the second row's x in rotated
    // order, x = (i - HXP) mod 16, puts lane 16+i on bank slot i (mod 16), the
    // complement of what its ds_read_b128 lane group already uses: no conflicts.
    const int r = (TX == 16 && (lane & 16)) ? 16 + (((lane & 15) - HXP) & 15) : (lane & 31);

    // Tiles of this workgroup. The tile list is cut into 8 contiguous ranges, one per
    // XCD (workgroups are dealt round-robin to the XCDs, so blockIdx.x & 7 is the XCD);
    // the workgroups of an XCD walk their range together, slot by slot, so tiles that
    // share halo planes are resident in the same L2 at the same time. With as many
    // workgroups as tiles this is the plain one-tile-per-workgroup order.
    // row mode (ConvArgs::row_stride): tiles_x counts the strip columns of the whole row
    constexpr bool row = ROW;
    static_assert(!ROW || (POOL && ES == 2 && HEAD == 0), "row mode: 16-bit fused-pool epilogue");
    // carry (ConvArgs::in_z0 .. out_shift): tiles_z counts the z tiles that are left
    static_assert(!CARRY || ROW, "carry: row mode only");
    // carry along y (ConvCarryY): tiles_y counts the y tiles that are left
    static_assert(!CARRYY || (CARRY && TY % 2 == 0 && TX == 16), "y carry: on top of the z carry, a wave owns a row pair");
    const int total = tiles_z * tiles_y * tiles_x * (row ? 1 : a.n);
    int t_first, t_count, t_step;
    {
        const int q = total >> 3, rem = total & 7;
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        t_first = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + slot;
        t_count = q + (xcd < rem ? 1 : 0) - slot;        // tiles left from t_first on
        t_step = (gridDim.x + 7 - xcd) >> 3;             // workgroups on this XCD
    }
    if (t_count <= 0) return;
    const int ntiles = a.cout >> 5;
    const int ntile0 = blockIdx.y;

    struct Tile {
        int z0, y0, x0, nb;
    };
    // row mode: strip column cx (row x = 16 cx) belongs to patch clamp((16 cx - o/2) / stride, 0, n - 1)
    auto row_tile_at = [&](int id) {
        Tile t;
        const int s = a.row_stride, ho = (a.w - s) >> 1;
        const int rx = (id % tiles_x) * TX; id /= tiles_x;
        const int nb = min(max(rx - ho, 0) / s, a.n - 1);
        t.x0 = __builtin_amdgcn_readfirstlane(rx - nb * s);
        if constexpr (CARRYY) {
            int ty = id % tiles_y; id /= tiles_y;
            if (ty >= cy.in_y0 / TY) ty += (cy.in_y1 - cy.in_y0) / TY;   // (the y tiles already present)
            t.y0 = __builtin_amdgcn_readfirstlane(ty * TY);
        } else {
            t.y0 = __builtin_amdgcn_readfirstlane((id % tiles_y) * TY); id /= tiles_y;
        }
        int tz = id % tiles_z;
        if (CARRY && tz >= a.in_z0 / TZ) tz += (a.in_z1 - a.in_z0) / TZ;   // (the z tiles already present)
        t.z0 = __builtin_amdgcn_readfirstlane(tz * TZ);
        t.nb = __builtin_amdgcn_readfirstlane(nb);
        return t;
    };
    auto tile_at = [&](int id) {
        if (row) return row_tile_at(id);
        Tile t;
        // (x fastest. Measured alternative, z fastest -- whole z-columns resident in an XCD's L2
        // together so that neighbours share their two halo planes: HBM reads 1363 -> 1429 MB per
        // inc.3 launch, 1 % slower.) The divisions run on the vector ALU; readfirstlane puts the
        // wave-uniform results back into scalar registers.
        t.x0 = __builtin_amdgcn_readfirstlane(a.org[2] + (id % tiles_x) * TX); id /= tiles_x;
        t.y0 = __builtin_amdgcn_readfirstlane(a.org[1] + (id % tiles_y) * TY); id /= tiles_y;
        t.z0 = __builtin_amdgcn_readfirstlane(a.org[0] + (id % tiles_z) * TZ); id /= tiles_z;
        id = __builtin_amdgcn_readfirstlane(id);
        t.nb = id;
        return t;
    };

    const int pos = wave * 32 + r;  // this lane's position inside the plane
    const int col = (pos / TX) * HXP + (pos % TX) + half * GS;

    // ---- staging map ----------------------------------------------------------
    // primary: thread t < NPAIR moves pair t = (column t / 2, group t & 1), all HZ
    // planes (one vector offset; plane and chunk ride in the scalar offset).
    // secondary: the REM pairs beyond NTHREADS, piece q = t + k * NTHREADS is
    // plane q / REM of pair NTHREADS + q % REM (own vector offset each).
    // LDS slots do not depend on the tile; the global offsets are set per tile.
    const int plane_vox = a.h * a.w;
    const size_t patch_vox = (size_t)a.d * plane_vox;
    const bool p_ok = tid < NPAIR;
    const int p_hy = (tid >> 1) / HX, p_hx = (tid >> 1) % HX, p_kg = tid & 1;
    const int p_slot = p_kg * GS + p_hy * HXP + p_hx;
    unsigned p_voff;      // byte offset inside a z-plane of a chunk plane (or out of range)
    unsigned s_voff[SEC > 0 ? SEC : 1];
    int s_slot[SEC > 0 ? SEC : 1];
#pragma unroll
    for (int k = 0; k < SEC; ++k) {
        const int q = tid + k * NTHREADS;
        const int pr = NTHREADS + q % REM, hz = q / REM;
        const int c = pr >> 1, kg = pr & 1;
        s_slot[k] = q < REM * HZ ? kg * GS + hz * PLANE + (c / HX) * HXP + c % HX : -1;
    }
    auto set_offsets = [&](const Tile& t) {
        if constexpr (CARRY) {
            // (the carry stores' scalars take the registers the hoisted p_hy / p_hx / p_kg lived in: the
            // pair is derived again per tile from an opaque lane index, see fresh_lane())
            const int ft = wave * 64 + fresh_lane();
            const int gy = t.y0 + (ft >> 1) / HX - 1, gx = t.x0 + (ft >> 1) % HX - 1;
            const bool in = ft < NPAIR && (unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w;
            p_voff = in ? (unsigned)(gy * a.w + gx) * 32u + (ft & 1) * 16u : kOutOfRange;
        } else {
            const int gy = t.y0 + p_hy - 1, gx = t.x0 + p_hx - 1;
            const bool in = p_ok && (unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w;
            p_voff = in ? (unsigned)(gy * a.w + gx) * 32u + p_kg * 16u : kOutOfRange;
        }
#pragma unroll
        for (int k = 0; k < SEC; ++k) {
            const int q = tid + k * NTHREADS;
            const int pr = NTHREADS + q % REM, hz = q / REM;
            const int c = pr >> 1, kg = pr & 1;
            const int gz = t.z0 + hz - 1, gy = t.y0 + c / HX - 1, gx = t.x0 + c % HX - 1;
            const bool in = q < REM * HZ && (unsigned)gz < (unsigned)a.d &&
                            (unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w;
            s_voff[k] = in ? (unsigned)((gz * a.h + gy) * a.w + gx) * 32u + kg * 16u : kOutOfRange;
        }
    };
    // weight fragments: piece i = tid + it * NTHREADS is element (i & 63) of tap i >> 6
    const unsigned wvoff = (((tid >> 6) * ntiles) * 64 + (tid & 63)) * 16u;

    // the slice's folded bias, kept in LDS: every tile's accumulators start from it
    __shared__ __attribute__((aligned(16))) float bias_s[32];
    if (tid < 32) bias_s[tid] = a.bias[ntile0 * 32 + tid];
    // the fused head's weights and bias live there too (read back once per tile)
    __shared__ __attribute__((aligned(16))) float head_s[HEAD > 0 ? HEAD * 32 + 4 : 4];
    if (HEAD > 0) {
        if (tid < HEAD * 32) head_s[tid] = a.head_w[tid];
        if (tid < HEAD) head_s[HEAD * 32 + tid] = a.head_b[tid];
    }

    const int nchunks = (a.ca + a.cb) / KC;
    uint4 stg[NITEMS + WITEMS];  // halo pieces, then weight fragments
    uint4* const wlds = lds + XUNITS;
    const __amdgpu_buffer_rsrc_t wrsrc = make_rsrc(a.weights, (size_t)nchunks * 27 * ntiles * 1024);

    // where chunk c of patch nb lives: descriptor of the patch of its source, offset of its plane
    struct ChunkSrc {
        __amdgpu_buffer_rsrc_t rsrc;
        __amdgpu_buffer_rsrc_t none;   // the same with zero records: every load returns zeros
        unsigned cbase;
    };
    auto chunk_src = [&](int c, int nb) {
        const char* src;
        int cs, ch0;
        if (c * KC < a.ca) {
            src = static_cast<const char*>(a.src_a); cs = a.ca; ch0 = c * KC;
        } else {
            src = static_cast<const char*>(a.src_b); cs = a.cb; ch0 = c * KC - a.ca;
        }
        const size_t patchb = patch_vox * cs * ES;  // bytes of one patch of this source
        return ChunkSrc{make_rsrc(src + (size_t)nb * patchb, patchb), make_rsrc(src + (size_t)nb * patchb, 0),
                        (unsigned)(ch0 / KC) * (unsigned)patch_vox * 32u};
    };
    // piece i of chunk c of the tile whose first plane is z0: global -> stg[i]
    auto load_piece = [&](const ChunkSrc& cs, int c, int z0, int i) {
        if (i < NITEMS) {
            if (i < HZ) {
                // A z-halo plane outside the patch is loaded through the zero-record descriptor (the
                // range check returns zeros) rather than set to zero in a branch: writing the staging
                // registers there made hipcc wait for EVERY load in flight (s_waitcnt vmcnt(0) in the
                // middle of the tap loop of every first and last tile of a column).
                const int gz = z0 + i - 1;  // wave-uniform
                stg[i] = (unsigned)gz < (unsigned)a.d
                             ? buf_load16(cs.rsrc, p_voff, cs.cbase + (unsigned)gz * plane_vox * 32u)
                             : buf_load16(cs.none, p_voff, 0);
            } else {
                stg[i] = buf_load16(cs.rsrc, s_voff[i - HZ], cs.cbase);
            }
        } else {
            const int it = i - NITEMS;
            // taps it * NWAVES + wave; the last round covers taps < 27 only
            stg[i] = it * NWAVES + wave < 27
                         ? buf_load16(wrsrc, wvoff, ((c * 27 + it * NWAVES) * ntiles + ntile0) * 1024)
                         : make_uint4(0, 0, 0, 0);
        }
    };
    auto stage_store = [&]() {
        if ((EXASPIM_ABLATE & 4) && stg[0].x != 0x12345u) return;
        if (p_ok) {
#pragma unroll
            for (int hz = 0; hz < HZ; ++hz) lds[p_slot + hz * PLANE] = stg[hz];
        }
#pragma unroll
        for (int k = 0; k < SEC; ++k)
            if (s_slot[k] >= 0) lds[s_slot[k]] = stg[HZ + k];
#pragma unroll
        for (int it = 0; it < WITEMS; ++it) {
            const int i = tid + it * NTHREADS;
            if (i < WUNITS) wlds[i] = stg[NITEMS + it];
        }
    };

    int tile_id = t_first;
    Tile cur = tile_at(tile_id);
    set_offsets(cur);
    {
        const ChunkSrc cs0 = chunk_src(0, cur.nb);
#pragma unroll
        for (int i = 0; i < NITEMS + WITEMS; ++i) load_piece(cs0, 0, cur.z0, i);
    }
    stage_store();

    for (;;) {
#ifdef EXASPIM_TRACE
        const size_t trace_rec = ((size_t)tile_id * NWAVES + wave) * 16;
        if (a.trace && lane == 0)
            a.trace[trace_rec + 15] =
                ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |
                (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);
#endif
        EXA_TRACE(0);
        EXA_TRACE(1);
        __syncthreads();   // this tile's first chunk (and, the first time, the bias) is in LDS
        // register 4q+k of a lane is channel 8q + 4*half + k of the slice
        f32x16 acc[TZ];
        const int half_t = fresh_lane() >> 5;   // (recomputed per tile, see fresh_lane())
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 b = *reinterpret_cast<const float4*>(bias_s + 8 * q + 4 * half_t);
#pragma unroll
            for (int mt = 0; mt < TZ; ++mt) {
                acc[mt][4 * q + 0] = b.x; acc[mt][4 * q + 1] = b.y;
                acc[mt][4 * q + 2] = b.z; acc[mt][4 * q + 3] = b.w;
            }
        }
        EXA_TRACE(2);

        // During the last chunk the first chunk of the workgroup's NEXT tile is
        // prefetched, so only the first tile of a workgroup pays the global latency.
        t_count -= t_step;
        const bool has_next = t_count > 0;
        Tile nxt = cur;
        for (int c = 0; c < nchunks; ++c) {
            const bool more = c + 1 < nchunks;
            const bool pre = more || has_next;
            if (!more && has_next) {
                nxt = tile_at(tile_id + t_step);
                set_offsets(nxt);   // every load of the current tile has been issued
            }
            const ChunkSrc csn = chunk_src(more ? c + 1 : 0, more ? cur.nb : nxt.nb);
            const int cn = more ? c + 1 : 0, zn = more ? cur.z0 : nxt.z0;
            uint4 xr[R];       // operand ring: fragment of step s lives in xr[s % R]
            // weight fragments (dz) of tap g: fragment dz is used in steps zin = dz ..
            // dz + TZ - 1 of its tap, so the next tap's fragment takes over the register
            // as soon as that window closes (two steps before its own window opens)
            uint4 wb[3];
#pragma unroll
            for (int dz = 0; dz < 3; ++dz) wb[dz] = wlds[(dz * 9) * 64 + lane];
#pragma unroll
            for (int s = 0; s < D; ++s)
                xr[s % R] = lds[col + (s % HZ) * PLANE + ((s / HZ) / 3) * HXP + (s / HZ) % 3];
            __builtin_amdgcn_sched_barrier(0);
            if (ES == 2) __builtin_amdgcn_s_setprio(kSetprio);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int g = s / HZ, zin = s % HZ;
                if (s + D < NS) {
                    const int g2 = (s + D) / HZ, z2 = (s + D) % HZ;
                    xr[(s + D) % R] = lds[col + z2 * PLANE + (g2 / 3) * HXP + g2 % 3];
                }
#ifdef EXASPIM_TRACE
                // 2-chunk layers leave stamps 9..11 free: quarter marks inside the first chunk's loop
                if (nchunks == 2 && c == 0 && s > 0 && s % (NS / 4) == 0 && s / (NS / 4) <= 3) EXA_TRACE(8 + s / (NS / 4));
#endif
                if (g + 1 < 9 && zin >= TZ) wb[zin - TZ] = wlds[((zin - TZ) * 9 + g + 1) * 64 + lane];
                if (g > 0 && zin == 0) wb[2] = wlds[(2 * 9 + g) * 64 + lane];
                // one staged piece every LOAD_STRIDE steps: issued back to back in the first steps
                // the loads of all eight waves of a CU queue up in the texture addresser, and the
                // MFMAs behind a load that cannot issue wait with it (the first quarter of the loop
                // took 5.1 k cycles, the others 1.3-1.8 k; spread out 3.2 k: tools/conv_trace.hip)
                if (!(EXASPIM_ABLATE & 1) && pre && s % LOAD_STRIDE == 0 && s / LOAD_STRIDE < NITEMS + WITEMS)
                    load_piece(csn, cn, zn, s / LOAD_STRIDE);
#pragma unroll
                for (int dz = 0; dz < 3; ++dz) {
                    const int z = zin - dz;
                    if (z >= 0 && z < TZ) mma_inplace<Tag>(acc[z], wb[dz], xr[s % R]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (ES == 2) __builtin_amdgcn_s_setprio(0);
            // The 16-bit MFMAs above are inline assembly (mma_inplace), so hipcc's hazard recognizer does
            // not know that the accumulators were written by the matrix pipe: the wait states between an
            // 8-pass MFMA and the first vector-ALU read of its destination (the epilogue) are spelled out
            // here instead of being left to whatever happens to stand in between.
            if (ES == 2) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 1");
            if (c < 4) EXA_TRACE(3 + 3 * c);
            __syncthreads();   // every wave is done reading this chunk's image
            if (c < 4) EXA_TRACE(4 + 3 * c);
            if (more) {
                stage_store();
                __syncthreads();
                if (c < 3) EXA_TRACE(5 + 3 * c);
            }
        }
        // The next tile's prefetched pieces are waited for HERE, before the epilogue issues its stores
        // (the empty asm makes every staged register "used", so hipcc puts the s_waitcnt for the
        // prefetch loads in front of it; afterwards they are plain values). Left to the staging behind
        // the epilogue, that wait is s_waitcnt vmcnt(0) and also covers the epilogue's stores -- a tile
        // boundary then costs a full store round trip. (A counted wait, vmcnt(#stores), behind
        // unconditional range-checked stores would do as well -- range-dropped stores retire in order
        // with older loads, tools/vmcnt_order.hip -- but the epilogue's stores go through buf_store16,
        // whose inline assembly hipcc cannot count.)
        if (has_next) {
#pragma unroll
            for (int i = 0; i < NITEMS + WITEMS; ++i)
                asm volatile("" : "+v"(stg[i].x), "+v"(stg[i].y), "+v"(stg[i].z), "+v"(stg[i].w));
        }

        // the lane's coordinates inside the tile, recomputed per tile (see fresh_lane())
        const int lane_e = fresh_lane();
        const int half_e = lane_e >> 5;
        const int r_e = (TX == 16 && (lane_e & 16)) ? 16 + (((lane_e & 15) - HXP) & 15) : (lane_e & 31);
        const int pos_e = wave * 32 + r_e;
        if (HEAD > 0) {
            // ---- fused head: OutConv 1x1x1 (+ sigmoid) on the accumulators -----------
            // lane (voxel r, half h) holds channels 8q + 4h + j of its voxel: a 16-term
            // partial dot product per output, completed by the other half-wave.
            // Channel quads outermost, so only 4 weights per output are live at a time
            // (the next tile's staged pieces occupy most of the register file here).
            float part[TZ][HEAD > 0 ? HEAD : 1];
#pragma unroll
            for (int z = 0; z < TZ; ++z)
#pragma unroll
                for (int o = 0; o < HEAD; ++o) part[z][o] = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 hw[HEAD > 0 ? HEAD : 1];
#pragma unroll
                for (int o = 0; o < HEAD; ++o)
                    hw[o] = *reinterpret_cast<const float4*>(head_s + o * 32 + 8 * q + 4 * half_e);
#pragma unroll
                for (int z = 0; z < TZ; ++z) {
                    float v0 = acc[z][4 * q + 0], v1 = acc[z][4 * q + 1];
                    float v2 = acc[z][4 * q + 2], v3 = acc[z][4 * q + 3];
                    v0 = leaky(v0, a.slope);
                    v1 = leaky(v1, a.slope);
                    v2 = leaky(v2, a.slope);
                    v3 = leaky(v3, a.slope);
#pragma unroll
                    for (int o = 0; o < HEAD; ++o)
                        part[z][o] = fmaf(v3, hw[o].w, fmaf(v2, hw[o].z, fmaf(v1, hw[o].y, fmaf(v0, hw[o].x, part[z][o]))));
                }
            }
            const size_t plane = (size_t)a.h * a.w;
            const int gy = cur.y0 + pos_e / TX, gx = cur.x0 + pos_e % TX;
            // (unconditional range-checked stores, see the direct epilogue below; outputs are dealt
            // to the two half-waves: even ones are stored by lanes 0-31, odd ones by lanes 32-63)
            const bool okyx = gy < a.org[1] + a.ext[1] && gx < a.org[2] + a.ext[2];
            float* const hpatch = a.head_out + (size_t)cur.nb * HEAD * a.d * plane;
            const size_t hbytes = (size_t)HEAD * a.d * plane * sizeof(float);
            const unsigned hvoff[2] = {okyx && half_e == 0 ? (unsigned)(gy * a.w + gx) * 4u : kOutOfRange,
                                       okyx && half_e == 1 ? (unsigned)(gy * a.w + gx) * 4u : kOutOfRange};
#pragma unroll
            for (int z = 0; z < TZ; ++z) {
                const int gz = cur.z0 + z;
                const __amdgpu_buffer_rsrc_t hrsrc = make_rsrc(hpatch, gz < a.org[0] + a.ext[0] ? hbytes : (size_t)0);
#pragma unroll
                for (int o = 0; o < HEAD; ++o) {
                    float t = part[z][o] + __shfl_xor(part[z][o], 32) + head_s[HEAD * 32 + o];
                    if (a.head_sigmoid) t = 1.f / (1.f + expf(-t));
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(t), hrsrc, (int)hvoff[o & 1],
                                                          (int)((unsigned)(o * a.d + gz) * (unsigned)plane * 4u), 0);
                }
            }
        } else if (ES == 2 && !POOL) {
            // ---- epilogue: LeakyReLU, records assembled with v_permlane32_swap ------
            // (16-bit types without the fused max-pool: nothing goes through LDS, so the next
            // tile's first chunk can be written to the image right behind this)
            char* const dplane = static_cast<char*>(a.dst) +
                                 ((size_t)cur.nb * (a.cout / KC) + ntile0 * 2) * patch_vox * 32;
            const int gy = cur.y0 + pos_e / TX, gx = cur.x0 + pos_e % TX;
            const bool okyx = gy < a.org[1] + a.ext[1] && gx < a.org[2] + a.ext[2];
            // Every store is ISSUED, as a range-checked buffer store: a lane outside the region gets
            // an out-of-range offset and a plane outside it the zero-record descriptor, and the
            // hardware drops the write -- no branch, no per-store address arithmetic on the vector ALU.
            // (buf_store16: hazard-safe and invisible to hipcc's wait counts, see common.h.)
            const unsigned ovoff = okyx ? (unsigned)(gy * a.w + gx) * 32u + half_e * 16u : kOutOfRange;
#pragma unroll
            for (int z = 0; z < TZ; ++z) {
                uint2 grp[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    grp[q] = pack4<Tag>(leaky(acc[z][4 * q + 0], a.slope), leaky(acc[z][4 * q + 1], a.slope),
                                        leaky(acc[z][4 * q + 2], a.slope), leaky(acc[z][4 * q + 3], a.slope));
                const int gz = cur.z0 + z;     // wave-uniform
#pragma unroll
                for (int ck = 0; ck < 2; ++ck) {
                    const uint4 rec = record_half(grp[2 * ck], grp[2 * ck + 1]);
                    const unsigned soff = ((unsigned)ck * (unsigned)patch_vox + (unsigned)gz * (unsigned)plane_vox) * 32u;
                    // (descriptor with zero records for a plane outside the region: a scalar select, no branch)
                    const __amdgpu_buffer_rsrc_t orsrc =
                        make_rsrc(dplane, gz < a.org[0] + a.ext[0] ? (size_t)2 * patch_vox * 32 : (size_t)0);
                    buf_store16(rec, orsrc, ovoff, soff);
                }
            }
        } else if (ES == 2 && POOL) {
            // ---- epilogue with the fused max-pool, 16-bit types: the layer's own output leaves the
            // registers like in the branch above (v_permlane32_swap, no LDS); of a PAIR of planes only the
            // element-wise maximum goes to LDS, as order-preserving keys, and a pooled piece is the maximum
            // over the 2 x 2 records of its row pair there. Against parking all six planes: half the LDS
            // writes, a third of the reads, no read-back for the 12 output stores. Maximum of the stored
            // (rounded, saturated) values like maxpool2_kernel: same bits.
            static_assert(!(ES == 2 && POOL) || (TZ % 2 == 0 && TY % 2 == 0 && TX == 16), "pooled tile shape");
            constexpr int CPT = 2;
            char* wl = reinterpret_cast<char*>(lds) + wave * ((TZ / 2) * 32 * RECP);
            char* const dplane = static_cast<char*>(a.dst) +
                                 ((size_t)cur.nb * (a.cout / KC) + ntile0 * 2) * patch_vox * 32;
            const int gy = cur.y0 + pos_e / TX, gx = cur.x0 + pos_e % TX;
            const bool okyx = gy < a.org[1] + a.ext[1] && gx < a.org[2] + a.ext[2];
            const unsigned ovoff = okyx ? (unsigned)(gy * a.w + gx) * 32u + half_e * 16u : kOutOfRange;
            // row mode, a column the neighbour holds too: the same records go to the neighbour's frame,
            // but for its two outermost x (their receptive field reaches its own zero padding)
            // [stride, stride + o/2) is the next patch's [0, o/2), [o/2, o) the previous one's [w - o/2, w)
            // (wave-uniform, recomputed here rather than carried through the tap loop with the tile; the
            // shift rides in the descriptor's base, so the lanes keep ovoff: no extra vector register)
            const int rs = a.row_stride, rho = (a.w - rs) >> 1;
            const bool nnext = row && cur.x0 >= rs && cur.x0 < rs + rho && cur.nb + 1 < a.n;
            const bool nprev = row && cur.x0 >= rho && cur.x0 < 2 * rho && cur.nb >= 1;
            const bool shared = nnext || nprev;
            const int nshift = nnext ? -rs : nprev ? rs : 0;
            const int nnb = cur.nb + (nnext ? 1 : nprev ? -1 : 0);
            const int ngx = gx + nshift;
            const bool nlane = ngx >= 2 && ngx < a.w - 2;
            const int nbase = nshift * 32;   // (the records end where the neighbour's patch ends)
            char* const nplane = static_cast<char*>(a.dst) + nbase +
                                 ((size_t)nnb * (a.cout / KC) + ntile0 * 2) * patch_vox * 32;
            const size_t nbytes = (size_t)((long long)2 * patch_vox * 32 - nbase);
            // carry out: the same records once more, to carry_dst at plane - out_shift (the shift rides in
            // the descriptors' bases too; a plane outside [out_z0, out_z1) gets zero records)
            const bool cout_on = CARRY && a.carry_dst != nullptr;
            const long long cshift = (long long)a.out_shift * plane_vox * 32;
            char* const cplane = static_cast<char*>(a.carry_dst) - cshift +
                                 ((size_t)cur.nb * (a.cout / KC) + ntile0 * 2) * patch_vox * 32;
            char* const cnplane = static_cast<char*>(a.carry_dst) - cshift + nbase +
                                  ((size_t)nnb * (a.cout / KC) + ntile0 * 2) * patch_vox * 32;
            // y and diagonal carry out (ConvCarryY): a wave's row pair starts at an even row and the bounds are
            // even, so "row in [out_y0, out_y1)" is wave-uniform and rides in the descriptors like the plane
            bool y_on = false, d_on = false;
            long long yshift = 0;
            if constexpr (CARRYY) {
                const int wy = cur.y0 + 2 * wave;
                const bool yrow = wy >= cy.out_y0 && wy < cy.out_y1;
                y_on = cy.y_dst != nullptr && yrow;
                d_on = cy.d_dst != nullptr && yrow;
                yshift = (long long)cy.out_shift_y * a.w * 32;
            }
#pragma unroll
            for (int zp = 0; zp < TZ / 2; ++zp) {
                uint2 grp[2][4];
#pragma unroll
                for (int zz = 0; zz < 2; ++zz)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        grp[zz][q] = pack4<Tag>(leaky(acc[2 * zp + zz][4 * q + 0], a.slope), leaky(acc[2 * zp + zz][4 * q + 1], a.slope),
                                                leaky(acc[2 * zp + zz][4 * q + 2], a.slope), leaky(acc[2 * zp + zz][4 * q + 3], a.slope));
#pragma unroll
                for (int q = 0; q < 4; ++q) {      // the pair's maximum, as keys, where the pooling pass finds it
                    const uint2 km = make_uint2(maxkey16x2(okey16x2<Tag::kInf16>(grp[0][q].x), okey16x2<Tag::kInf16>(grp[1][q].x)),
                                                maxkey16x2(okey16x2<Tag::kInf16>(grp[0][q].y), okey16x2<Tag::kInf16>(grp[1][q].y)));
                    *reinterpret_cast<uint2*>(wl + zp * (32 * RECP) + r_e * RECP + (8 * q + 4 * half_e) * ES) = km;
                }
#pragma unroll
                for (int zz = 0; zz < 2; ++zz) {
                    const int gz = cur.z0 + 2 * zp + zz;     // wave-uniform
                    const __amdgpu_buffer_rsrc_t orsrc =
                        make_rsrc(dplane, gz < a.org[0] + a.ext[0] ? (size_t)2 * patch_vox * 32 : (size_t)0);
                    // (a plane beyond the patch of a masked last z tile must not reach the neighbour either: its
                    // offset would still lie inside the descriptor, in the first planes of the second chunk)
                    const __amdgpu_buffer_rsrc_t nrsrc = make_rsrc(nplane, gz < a.org[0] + a.ext[0] ? nbytes : (size_t)0);
#pragma unroll
                    for (int ck = 0; ck < 2; ++ck) {
                        const uint4 rec = record_half(grp[zz][2 * ck], grp[zz][2 * ck + 1]);
                        buf_store16(rec, orsrc, ovoff, ((unsigned)ck * (unsigned)patch_vox + (unsigned)gz * (unsigned)plane_vox) * 32u);
                        if (shared)
                            buf_store16(rec, nrsrc, nlane ? ovoff : kOutOfRange, ((unsigned)ck * (unsigned)patch_vox + (unsigned)gz * (unsigned)plane_vox) * 32u);
                        if (CARRY && cout_on) {
                            const bool cz = gz >= a.out_z0 && gz < a.out_z1;
                            buf_store16(rec, make_rsrc(cplane, cz ? (size_t)2 * patch_vox * 32 : (size_t)0), ovoff,
                                        ((unsigned)ck * (unsigned)patch_vox + (unsigned)gz * (unsigned)plane_vox) * 32u);
                            if (shared)
                                buf_store16(rec, make_rsrc(cnplane, cz ? nbytes : (size_t)0), nlane ? ovoff : kOutOfRange,
                                            ((unsigned)ck * (unsigned)patch_vox + (unsigned)gz * (unsigned)plane_vox) * 32u);
                        }
                        if constexpr (CARRYY) if (y_on) {    // (every plane of the patch this tile stores)
                            const bool yz = gz < a.org[0] + a.ext[0];
                            const size_t poff = ((size_t)cur.nb * (a.cout / KC) + ntile0 * 2) * patch_vox * 32;
                            buf_store16(rec, make_rsrc(static_cast<char*>(cy.y_dst) - yshift + poff, yz ? (size_t)2 * patch_vox * 32 : (size_t)0),
                                        ovoff, ((unsigned)ck * (unsigned)patch_vox + (unsigned)gz * (unsigned)plane_vox) * 32u);
                            if (shared) {
                                const size_t npoff = ((size_t)nnb * (a.cout / KC) + ntile0 * 2) * patch_vox * 32;
                                buf_store16(rec, make_rsrc(static_cast<char*>(cy.y_dst) - yshift + nbase + npoff, yz ? nbytes : (size_t)0),
                                            nlane ? ovoff : kOutOfRange,
                                            ((unsigned)ck * (unsigned)patch_vox + (unsigned)gz * (unsigned)plane_vox) * 32u);
                            }
                        }
                        if constexpr (CARRYY) if (d_on) {
                            const bool dz = gz >= a.out_z0 && gz < a.out_z1;
                            const size_t poff = ((size_t)cur.nb * (a.cout / KC) + ntile0 * 2) * patch_vox * 32;
                            buf_store16(rec, make_rsrc(static_cast<char*>(cy.d_dst) - cshift - yshift + poff, dz ? (size_t)2 * patch_vox * 32 : (size_t)0),
                                        ovoff, ((unsigned)ck * (unsigned)patch_vox + (unsigned)gz * (unsigned)plane_vox) * 32u);
                            if (shared) {
                                const size_t npoff = ((size_t)nnb * (a.cout / KC) + ntile0 * 2) * patch_vox * 32;
                                buf_store16(rec, make_rsrc(static_cast<char*>(cy.d_dst) - cshift - yshift + nbase + npoff, dz ? nbytes : (size_t)0),
                                            nlane ? ovoff : kOutOfRange,
                                            ((unsigned)ck * (unsigned)patch_vox + (unsigned)gz * (unsigned)plane_vox) * 32u);
                            }
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            {
                // the wave's 2 rows x 16 voxels x TZ / 2 plane pairs give TZ / 2 x 8 pooled voxels; a piece is
                // one 16-byte group of one of them (record = row * 16 + x)
                constexpr int NP = (TZ / 2) * 8 * CPT * 2;
                const int pd = a.d >> 1, ph = a.h >> 1, pw2 = a.w >> 1;
                const size_t pvox = (size_t)pd * ph * pw2;
                char* const pplane = static_cast<char*>(a.pool_dst) +
                                     ((size_t)cur.nb * (a.cout / KC) + ntile0 * CPT) * pvox * 32;
                const __amdgpu_buffer_rsrc_t prsrc = make_rsrc(pplane, (size_t)CPT * pvox * 32);
                char* const npplane = static_cast<char*>(a.pool_dst) + nbase / 2 +
                                      ((size_t)nnb * (a.cout / KC) + ntile0 * CPT) * pvox * 32;
                const __amdgpu_buffer_rsrc_t nprsrc = make_rsrc(npplane, (size_t)((long long)CPT * pvox * 32 - nbase / 2));
                // carry out of the pooled planes [out_z0 / 2, out_z1 / 2), at pooled plane - out_shift / 2
                const long long cpshift = (long long)(a.out_shift >> 1) * ph * pw2 * 32;
                char* const cpplane = static_cast<char*>(a.carry_pool_dst) - cpshift +
                                      ((size_t)cur.nb * (a.cout / KC) + ntile0 * CPT) * pvox * 32;
                char* const cnpplane = static_cast<char*>(a.carry_pool_dst) - cpshift + nbase / 2 +
                                       ((size_t)nnb * (a.cout / KC) + ntile0 * CPT) * pvox * 32;
#pragma unroll
                for (int p0 = 0; p0 < NP; p0 += 64) {
                    const int p = p0 + lane_e;
                    const bool live = p < NP;        // (a lane without a piece works on piece 0; its store is dropped)
                    const int pc = live ? p : 0;
                    const int zp = pc / (8 * CPT * 2), rem = pc % (8 * CPT * 2);
                    const int ck = rem / 16, xp = (rem % 16) >> 1, sb = rem & 1;
                    const char* rec = wl + zp * (32 * RECP) + (2 * xp) * RECP + (ck * 2 + sb) * 16;
                    uint4 m = *reinterpret_cast<const uint4*>(rec);
#pragma unroll
                    for (int k = 1; k < 4; ++k)
                        m = maxkey16(m, *reinterpret_cast<const uint4*>(rec + (k >> 1) * 16 * RECP + (k & 1) * RECP));
                    m = key16(m);
                    const int qz = cur.z0 / 2 + zp, qy = cur.y0 / 2 + wave, qx = cur.x0 / 2 + xp;
                    const unsigned pvoff = live && qz < pd && qy < ph && qx < pw2
                                               ? (unsigned)((ck * (int)pvox + (qz * ph + qy) * pw2 + qx) * 32 + sb * 16)
                                               : kOutOfRange;
                    buf_store16(m, prsrc, pvoff, 0u);
                    if (shared) {   // (pooled x 0 and w / 2 - 1 of the neighbour: from its own outermost x)
                        const int nqx = qx + nshift / 2;
                        buf_store16(m, nprsrc, nqx >= 1 && nqx < pw2 - 1 ? pvoff : kOutOfRange, 0u);
                    }
                    if (CARRY && cout_on) {   // (the plane pair is per lane here)
                        const unsigned cpvoff = 2 * qz >= a.out_z0 && 2 * qz < a.out_z1 ? pvoff : kOutOfRange;
                        buf_store16(m, make_rsrc(cpplane, (size_t)CPT * pvox * 32), cpvoff, 0u);
                        if (shared) {
                            const int nqx = qx + nshift / 2;
                            buf_store16(m, make_rsrc(cnpplane, (size_t)((long long)CPT * pvox * 32 - nbase / 2)),
                                        nqx >= 1 && nqx < pw2 - 1 ? cpvoff : kOutOfRange, 0u);
                        }
                    }
                    if constexpr (CARRYY) if (y_on || d_on) {   // (pooled row qy = wy / 2: the wave's own, in the range with wy)
                        const long long ypshift = (long long)(cy.out_shift_y >> 1) * pw2 * 32;
                        const size_t ppoff = ((size_t)cur.nb * (a.cout / KC) + ntile0 * CPT) * pvox * 32;
                        const size_t nppoff = ((size_t)nnb * (a.cout / KC) + ntile0 * CPT) * pvox * 32;
                        const int nqx = qx + nshift / 2;
                        const bool nq = nqx >= 1 && nqx < pw2 - 1;
                        if (y_on) {
                            buf_store16(m, make_rsrc(static_cast<char*>(cy.y_pool_dst) - ypshift + ppoff, (size_t)CPT * pvox * 32), pvoff, 0u);
                            if (shared)
                                buf_store16(m, make_rsrc(static_cast<char*>(cy.y_pool_dst) - ypshift + nbase / 2 + nppoff,
                                                         (size_t)((long long)CPT * pvox * 32 - nbase / 2)),
                                            nq ? pvoff : kOutOfRange, 0u);
                        }
                        if (d_on) {
                            const unsigned dpvoff = 2 * qz >= a.out_z0 && 2 * qz < a.out_z1 ? pvoff : kOutOfRange;
                            buf_store16(m, make_rsrc(static_cast<char*>(cy.d_pool_dst) - cpshift - ypshift + ppoff, (size_t)CPT * pvox * 32), dpvoff, 0u);
                            if (shared)
                                buf_store16(m, make_rsrc(static_cast<char*>(cy.d_pool_dst) - cpshift - ypshift + nbase / 2 + nppoff,
                                                         (size_t)((long long)CPT * pvox * 32 - nbase / 2)),
                                            nq ? dpvoff : kOutOfRange, 0u);
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } else {
            // ---- epilogue: LeakyReLU, transposed through LDS (float32: the 16-bit types left above) ----
            // One store instruction writes one chunk plane's 32 voxel records (32 B
            // each): two runs of 512 contiguous bytes when the tile row is 16 voxels.
            // The (dead) halo and weight image gives every wave room for TB planes at
            // once, so the LDS round trips and the stores of a batch overlap.
            constexpr int CPT = RECB / 32;                       // chunk planes of a 32-cout slice
            constexpr int TB_MAX = LDS_UNITS * 16 / (NWAVES * 32 * RECP);
            // with the fused max-pool a batch must hold whole pairs of planes
            constexpr int TB = POOL ? ((TB_MAX >= TZ ? TZ : TB_MAX) & ~1)
                                    : (TB_MAX >= TZ ? TZ : (TB_MAX >= (TZ + 1) / 2 ? (TZ + 1) / 2 : 1));
            static_assert(!POOL || (TB >= 2 && TZ % 2 == 0 && TY % 2 == 0 && TX == 16), "pooled tile shape");
            char* wl = reinterpret_cast<char*>(lds) + wave * (TB * 32 * RECP);
            char* const dplane = static_cast<char*>(a.dst) +
                                 ((size_t)cur.nb * (a.cout / KC) + ntile0 * CPT) * patch_vox * 32;
            const int vv = lane_e >> 1, sub = lane_e & 1;
            const int po = wave * 32 + vv;
            const int ogy = cur.y0 + po / TX, ogx = cur.x0 + po % TX;
#pragma unroll
            for (int zb = 0; zb < TZ; zb += TB) {
#pragma unroll
                for (int z = zb; z < zb + TB && z < TZ; ++z) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int cl = 8 * q + 4 * half_e;
                        // LeakyReLU with 0 <= slope <= 1 is max(v, slope * v)
                        float v0 = acc[z][4 * q + 0], v1 = acc[z][4 * q + 1];
                        float v2 = acc[z][4 * q + 2], v3 = acc[z][4 * q + 3];
                        v0 = leaky(v0, a.slope);
                        v1 = leaky(v1, a.slope);
                        v2 = leaky(v2, a.slope);
                        v3 = leaky(v3, a.slope);
                        store4<Tag>(wl + (z - zb) * (32 * RECP), (size_t)(r_e * RECP) / ES + cl, v0, v1, v2, v3);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int z = zb; z < zb + TB && z < TZ; ++z) {
                    const int gz = cur.z0 + z;
                    // (unconditional range-checked stores, see the direct epilogue above)
                    const bool tokyx = ogy < a.org[1] + a.ext[1] && ogx < a.org[2] + a.ext[2];
                    const unsigned tvoff = tokyx ? (unsigned)(ogy * a.w + ogx) * 32u + sub * 16u : kOutOfRange;
                    const __amdgpu_buffer_rsrc_t trsrc =
                        make_rsrc(dplane, gz < a.org[0] + a.ext[0] ? (size_t)CPT * patch_vox * 32 : (size_t)0);
#pragma unroll
                    for (int ck = 0; ck < CPT; ++ck) {
                        const uint4 val = *reinterpret_cast<const uint4*>(
                            wl + (z - zb) * (32 * RECP) + vv * RECP + (ck * 2 + sub) * 16);
                        buf_store16(val, trsrc, tvoff,
                                    ((unsigned)ck * (unsigned)patch_vox + (unsigned)gz * (unsigned)plane_vox) * 32u);
                    }
                }
                if (POOL) {
                    // MaxPool3d(2) of the planes in LDS: the wave's 2 rows x 16 voxels x TB planes
                    // give TB/2 x 8 pooled voxels; a piece is one 16-byte group of one of them,
                    // the maximum over its 2 x 2 x 2 source records (record = row * 16 + x).
                    constexpr int NP = (TB / 2) * 8 * CPT * 2;
                    const int pd = a.d >> 1, ph = a.h >> 1, pw2 = a.w >> 1;
                    const size_t pvox = (size_t)pd * ph * pw2;
                    char* const pplane = static_cast<char*>(a.pool_dst) +
                                         ((size_t)cur.nb * (a.cout / KC) + ntile0 * CPT) * pvox * 32;
                    const __amdgpu_buffer_rsrc_t prsrc = make_rsrc(pplane, (size_t)CPT * pvox * 32);
#pragma unroll
                    for (int p0 = 0; p0 < NP; p0 += 64) {
                        const int p = p0 + lane_e;
                        // a lane without a piece works on piece 0 and its store is dropped by the range
                        // check: no branch around the LDS reads or the store (see the direct epilogue)
                        const bool live0 = p < NP;
                        const int pc = live0 ? p : 0;
                        const int zp = pc / (8 * CPT * 2), rem = pc % (8 * CPT * 2);
                        const int ck = rem / 16, xp = (rem % 16) >> 1, sb = rem & 1;
                        const bool live = live0 && zb + 2 * zp + 1 < TZ;
                        const int zr = zb + 2 * zp + 1 < TZ ? zp : 0;     // (rows that exist in the batch)
                        const char* rec = wl + (2 * zr) * (32 * RECP) + (2 * xp) * RECP + (ck * 2 + sb) * 16;
                        uint4 m = *reinterpret_cast<const uint4*>(rec);
                        if (ES == 2) m = okey16<Tag::kInf16>(m);   // 16-bit types: compare order-preserving keys
#pragma unroll
                        for (int k = 1; k < 8; ++k) {
                            const uint4 v = *reinterpret_cast<const uint4*>(
                                rec + (k >> 2) * (32 * RECP) + ((k >> 1) & 1) * 16 * RECP + (k & 1) * RECP);
                            m = ES == 2 ? maxkey16(m, okey16<Tag::kInf16>(v)) : max16<Tag>(m, v);
                        }
                        if (ES == 2) m = key16(m);
                        const int qz = (cur.z0 + zb) / 2 + zp, qy = cur.y0 / 2 + wave, qx = cur.x0 / 2 + xp;
                        const unsigned pvoff =
                            live && qz < pd && qy < ph && qx < pw2
                                ? (unsigned)((ck * (int)pvox + (qz * ph + qy) * pw2 + qx) * 32 + sb * 16)
                                : kOutOfRange;
                        buf_store16(m, prsrc, pvoff, 0u);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        EXA_TRACE(14);
        if (!has_next) break;
        // the transposition buffers are free again (the fused head and the direct epilogue never used them)
        if (!(HEAD > 0 || (ES == 2 && !POOL))) __syncthreads();
        stage_store();
        tile_id += t_step;
        cur = nxt;
    }
}

template <typename Tag, int TZ, int TY, int TX, int MINW, int D, int HEAD = 0, bool POOL = false>
__global__ __launch_bounds__(TY* TX * 2, MINW) void conv3x3x3_zpipe(
    ConvArgs a, int tiles_z, int tiles_y, int tiles_x) {
    zpipe_body<Tag, TZ, TY, TX, MINW, D, HEAD, POOL, false>(a, tiles_z, tiles_y, tiles_x);
}

// Row mode (ConvArgs::row_stride) of the fused-pool instantiation, 16-bit types: a symbol of its own, so
// the row walk and the neighbour stores cost the per-patch kernel no registers
template <typename Tag, int TZ, int TY, int TX, int MINW, int D>
__global__ __launch_bounds__(TY* TX * 2, MINW) void conv3x3x3_zpipe_row(
    ConvArgs a, int tiles_z, int tiles_y, int tiles_x) {
    zpipe_body<Tag, TZ, TY, TX, MINW, D, 0, true, true>(a, tiles_z, tiles_y, tiles_x);
}

// Row mode with planes carried along z (ConvArgs::in_z0 .. out_shift): z tiles an earlier launch left in
// dst are not computed, and a plane range of this launch's stores goes to a second tensor as well. A symbol
// of its own again: conv3x3x3_zpipe_row keeps its code.
template <typename Tag, int TZ, int TY, int TX, int MINW, int D>
__global__ __launch_bounds__(TY* TX * 2, MINW) void conv3x3x3_zpipe_rowz(
    ConvArgs a, int tiles_z, int tiles_y, int tiles_x) {
    zpipe_body<Tag, TZ, TY, TX, MINW, D, 0, true, true, true>(a, tiles_z, tiles_y, tiles_x);
}

// ... and rows carried along y on top (ConvCarryY, a second argument of this symbol only): y tiles an earlier
// launch left in dst are not computed either, and the rows that feed the y and the diagonal successor are stored
// to their tensors as well. conv3x3x3_zpipe_rowz keeps its code.
template <typename Tag, int TZ, int TY, int TX, int MINW, int D>
__global__ __launch_bounds__(TY* TX * 2, MINW) void conv3x3x3_zpipe_rowzy(
    ConvArgs a, ConvCarryY cy, int tiles_z, int tiles_y, int tiles_x) {
    zpipe_body<Tag, TZ, TY, TX, MINW, D, 0, true, true, true, true>(a, tiles_z, tiles_y, tiles_x, cy);
}

}  // namespace exaspim
