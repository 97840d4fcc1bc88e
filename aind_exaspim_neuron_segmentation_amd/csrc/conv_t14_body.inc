// Body of conv3x3x3_t14, conv3x3x3_t14_carry and conv3x3x3_t14_borders_carry (conv_t14.h), included inside the kernel: the template
// parameters, a, tiles_z, tiles_y, tiles_x and the constant CARRY are the including kernel's.
    constexpr int G = Tag::kG;
    constexpr int KC = 2 * G;
    constexpr int ES = 16 / G;
    constexpr int HZ = TZ + 2, HY = TY + 2, HX = TX + 2;
    // Row stride of the LDS image (slots). A 32-voxel group of a 24-wide tile is a
    // row tail plus a row head; with a stride of 8 (mod 16) slots the two pieces fall
    // on complementary banks for every ds_read_b128 lane group (PMC: bank-conflict
    // cycles 50 % -> 17 % of the LDS-active cycles, which drop by 39 %; the launch time
    // does not move, LDS is not what limits this kernel). Padding is never touched.
    // (12-wide rows: a ds_read_b128 lane group of 16 voxels always wraps a 12-voxel row, and with the dense
    // row stride of 14 slots the two pieces share bank slots -- the counters show 50 % conflict cycles at
    // the 12^3 level. A row stride of 28 slots (= 12 mod 16, conflict-free for all 27 taps by enumeration,
    // channel groups 8 slots apart mod 16 for the staging writes) was measured in round 3 and, like round
    // 2's attempt, is SLOWER: down3.0 58 -> 66 us, down3.3 107 -> 127, up1.0 204 -> 243 per batch -- twice
    // the LDS image and a wider staging scatter cost more than the conflicts. Dense rows stay.)
    constexpr int HXS = TX == 24 ? 40 : HX;
    constexpr int PLS = HY * HXS;                   // plane stride
    constexpr int HV = HZ * PLS;                    // slots of a channel-group plane
    constexpr int HVD = HZ * HY * HX;               // halo voxels (staging enumerates these)
    constexpr int NWAVES = WAVES_M * WAVES_N;
    constexpr int NTHREADS = NWAVES * 64;
    constexpr int TILE_VOX = TZ * TY * TX;
    constexpr int NITEMS = (2 * HVD + NTHREADS - 1) / NTHREADS;
    constexpr int RECB = NT * 32 * ES;              // bytes of one voxel's output slice
    constexpr int RECP = RECB + 16;                 // padded LDS stride (8-way -> 2-way conflicts)
    constexpr int EPI_UNITS = NWAVES * (POOL ? MT : 1) * 32 * RECP / 16;   // POOL: all MT groups at once
    constexpr int IMG = 2 * HV;                     // slots of one image (two channel groups)
    constexpr int LDS_UNITS = IMG > EPI_UNITS ? IMG : EPI_UNITS;
    static_assert(!POOL || (WAVES_M * MT * 32 == TZ * TY * TX && TZ % 2 == 0 && TY % 2 == 0 && TX % 2 == 0),
                  "pooled tile shape");
    constexpr int ISSUE_T = 26 - PD > 0 ? 26 - PD : 0;  // tap at which the prefetch is issued
    static_assert(WAVES_M * MT * 32 >= TILE_VOX, "tile not covered by the waves");

    __shared__ __attribute__((aligned(16))) uint4 lds[LDS_UNITS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N;
    const int wn = wave % WAVES_N;
    const int half = lane >> 5;
    // 16-wide rows: second row of a 32-voxel group in rotated x order, x = (i - HX)
    // mod 16, so its lanes use the bank slots the first row leaves free (see zpipe)
    const int r = (TX == 16 && (lane & 16)) ? 16 + (((lane & 15) - HX) & 15) : (lane & 31);

    int bid;
    {
        const int nblk = gridDim.x, q = nblk >> 3, rem = nblk & 7;
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        bid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + slot;
    }
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y; bid /= tiles_y;
    int tz = bid % tiles_z; bid /= tiles_z;
    constexpr bool BORDERS = ZORD && POOL;
    // CARRY with BORDERS (conv3x3x3_t14_borders_carry): the z tiles lie over the two segments [0, in_z0) and
    // [in_z1, d), the first segment's last tile masked at in_z0 -- the carried range need not be whole tiles
    constexpr bool BCARRY = CARRY && BORDERS;
    if (CARRY && !BORDERS && tz >= a.in_z0 / TZ) tz += (a.in_z1 - a.in_z0) / TZ;   // (the z tiles already present)
    static_assert(!CARRY || (ES == 2 && (!ZORD || BORDERS)), "carry: 16-bit types, whole-patch or border tiles");
    const int nb = BORDERS && tx == 0 ? bid + 1 : bid;
    const int seg0 = BCARRY ? (a.in_z0 + TZ - 1) / TZ : 0;   // tiles of the first segment
    const bool low = BCARRY && tz < seg0;
    const int z0 = BCARRY && !low ? a.in_z1 + (tz - seg0) * TZ : a.org[0] + tz * TZ, y0 = a.org[1] + ty * TY;
    const int x0 = BORDERS ? (tx == 0 ? 0 : a.w - TX) : a.org[2] + tx * TX;
    const int zend = low ? (int)a.in_z0 : a.org[0] + a.ext[0], yend = a.org[1] + a.ext[1];
    const int xend = BORDERS ? x0 + TX : a.org[2] + a.ext[2];

    const int ntiles = a.cout >> 5;
    const int ntile0 = (blockIdx.y * WAVES_N + wn) * NT;

    int base[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int m = (wm * MT + mt) * 32 + r;
        m = m < TILE_VOX ? m : TILE_VOX - 1;
        const int z = m / (TY * TX), y = (m / TX) % TY, x = m % TX;
        base[mt] = z * PLS + y * HXS + x + half * HV;
    }

    // staging piece i = tid + it * NTHREADS is 16-byte group i & 1 of halo voxel
    // i >> 1: consecutive lanes read consecutive bytes of a halo row of the chunk plane
    const size_t patch_vox = (size_t)a.d * a.h * a.w;
    unsigned voffs[NITEMS];
#pragma unroll
    for (int it = 0; it < NITEMS; ++it) {
        const int i = tid + it * NTHREADS;
        const int hv = i >> 1;
        const int hz = hv / (HY * HX), hy = (hv / HX) % HY, hx = hv % HX;
        const int gz = z0 + hz - 1, gy = y0 + hy - 1, gx = x0 + hx - 1;
        const bool ok = i < 2 * HVD && (unsigned)gz < (unsigned)a.d &&
                        (unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w;
        voffs[it] = ok ? (unsigned)((gz * a.h + gy) * a.w + gx) * 32u + (i & 1) * 16u : kOutOfRange;
    }

    // accumulators start from the folded bias: register 4q+k of a lane is channel
    // 8q + 4*half + k of its slice (no bias pass in the epilogue)
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

    // this workgroup's range of input-channel chunks (all of them unless split-K)
    const int nchunks_all = (a.ca + a.cb) / KC;
    const int cbeg = (int)blockIdx.z * nchunks_all / a.ksplit;
    const int nchunks = ((int)blockIdx.z + 1) * nchunks_all / a.ksplit;
    uint4 stg[NITEMS];

    auto stage_load = [&](int c) {
        const char* src;
        int cs, ch0;
        if (c * KC < a.ca) {
            src = static_cast<const char*>(a.src_a); cs = a.ca; ch0 = c * KC;
        } else {
            src = static_cast<const char*>(a.src_b); cs = a.cb; ch0 = c * KC - a.ca;
        }
        const size_t patchb = patch_vox * cs * ES;  // bytes of one patch of this source
        const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(src + (size_t)nb * patchb, patchb);
        const unsigned cbase = (unsigned)(ch0 / KC) * (unsigned)patch_vox * 32u;  // chunk plane
#pragma unroll
        for (int it = 0; it < NITEMS; ++it) stg[it] = buf_load16(rsrc, voffs[it], cbase);
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int it = 0; it < NITEMS; ++it) {
            const int i = tid + it * NTHREADS;
            const int hv = i >> 1;
            if (i < 2 * HVD) lds[(i & 1) * HV + (hv / (HY * HX)) * PLS + ((hv / HX) % HY) * HXS + hv % HX] = stg[it];
        }
    };

#ifdef EXASPIM_TRACE
    const size_t trace_rec = ((size_t)blockIdx.x * NWAVES + wave) * 16;
    if (a.trace && lane == 0)
        a.trace[trace_rec + 15] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |
                                  (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);
#endif
    // step t of the tap loop handles tap tap_of(t) = dz * 9 + dy * 3 + dx
    constexpr auto tap_of = [](int t) { return ZORD ? (t % 3) * 9 + t / 3 : t; };
    // Weight ring, primed for the first PD taps of a chunk BEFORE the barriers in front of it
    // (in the prologue next to the staging loads, later right after the previous chunk's last
    // tap): the L2 latency of a chunk's first fragments passes under the wait for the staged
    // image instead of after it.
    uint4 wring[PD + 1][NT];
    auto prime_weights = [&](int c) {
        const uint4* wp = static_cast<const uint4*>(a.weights) + ((size_t)c * 27 * ntiles + ntile0) * 64 + lane;
#pragma unroll
        for (int t = 0; t < PD; ++t)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) wring[t][nt] = wp[((size_t)tap_of(t) * ntiles + nt) * 64];
    };
    EXA_TRACE(0);
    stage_load(cbeg);
    prime_weights(cbeg);
    EXA_TRACE(1);
    stage_store();
    __syncthreads();
    EXA_TRACE(2);

    for (int c = cbeg; c < nchunks; ++c) {
        const uint4* wp = static_cast<const uint4*>(a.weights) +
                          ((size_t)c * 27 * ntiles + ntile0) * 64 + lane;

        uint4 xf[2][MT];
        {
            constexpr int t0 = tap_of(0);
            constexpr int tapoff0 = (t0 / 9) * PLS + ((t0 / 3) % 3) * HXS + t0 % 3;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) xf[0][mt] = lds[base[mt] + tapoff0];
        }

        const bool more = c + 1 < nchunks;
        if (ES == 2) __builtin_amdgcn_s_setprio(kSetprioT14);
#pragma unroll
        for (int t = 0; t < 27; ++t) {
            if (t + PD < 27) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    wring[(t + PD) % (PD + 1)][nt] = wp[((size_t)tap_of(t + PD) * ntiles + nt) * 64];
            }
            if (t == ISSUE_T && more) stage_load(c + 1);
#ifdef EXASPIM_TRACE
            // 2-chunk layers leave stamps 9..11 free: marks after taps 7, 14 and 21 of the first chunk
            if (nchunks_all == 2 && c == cbeg && t > 0 && t % 7 == 0 && t / 7 <= 3) EXA_TRACE(8 + t / 7);
#endif
            if (t + 1 < 27) {
                const int tn = tap_of(t + 1);
                const int tapoff = (tn / 9) * PLS + ((tn / 3) % 3) * HXS + tn % 3;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) xf[(t + 1) & 1][mt] = lds[base[mt] + tapoff];
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    mma<Tag>(acc[mt][nt], wring[t % (PD + 1)][nt], xf[t & 1][mt]);
            // keep each tap's {prefetch issue, fragment reads, MFMAs} together: without
            // this fence hipcc hoists and sinks them across taps and the loop runs ~20 % slower
            __builtin_amdgcn_sched_barrier(0);
        }
        if (ES == 2) __builtin_amdgcn_s_setprio(0);
        if (more) prime_weights(c + 1);
        if (c - cbeg < 4) EXA_TRACE(3 + 3 * (c - cbeg));
        __syncthreads();  // every wave is done reading this chunk's image
        if (c - cbeg < 4) EXA_TRACE(4 + 3 * (c - cbeg));
        if (more) {
            stage_store();
            __syncthreads();
            if (c - cbeg < 3) EXA_TRACE(5 + 3 * (c - cbeg));
        }
    }

    if (a.ksplit > 1) {
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
        EXA_TRACE(14);
        return;
    }

    // ---- epilogue: bias + LeakyReLU, transposed through LDS ------------------
    const bool cz_on = CARRY && a.carry_dst != nullptr;
    char* wl = reinterpret_cast<char*>(lds) + wave * ((POOL ? MT : 1) * 32 * RECP);
    if (POOL) {
        // all groups first: group mt of wave w sits at ((w * MT + mt) * 32 + voxel) * RECP
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cl = nt * 32 + 8 * q + 4 * half;
                    store4<Tag>(wl + mt * (32 * RECP), (size_t)(r * RECP) / ES + cl,
                                leaky(acc[mt][nt][4 * q + 0], a.slope), leaky(acc[mt][nt][4 * q + 1], a.slope),
                                leaky(acc[mt][nt][4 * q + 2], a.slope), leaky(acc[mt][nt][4 * q + 3], a.slope));
                }
        __syncthreads();
        constexpr int NPL = RECB / 32;
        {   // the layer's own output, as below
            const int vv = lane >> 1, sub = lane & 1;
            char* const dplane = static_cast<char*>(a.dst) +
                                 ((size_t)nb * (a.cout / KC) + ntile0 * (32 / KC)) * patch_vox * 32;
            // carry out: the same record once more, out_shift planes up in carry_dst
            char* const cplane = static_cast<char*>(a.carry_dst) - (size_t)a.out_shift * a.h * a.w * 32 +
                                 ((size_t)nb * (a.cout / KC) + ntile0 * (32 / KC)) * patch_vox * 32;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int m = (wm * MT + mt) * 32 + vv;
                const int z = m / (TY * TX), y = (m / TX) % TY, x = m % TX;
                const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
                const bool ok = gz < zend && gy < yend && gx < xend;
                const size_t vox = ((size_t)gz * a.h + gy) * a.w + gx;
#pragma unroll
                for (int ck = 0; ck < NPL; ++ck) {
                    const uint4 val = *reinterpret_cast<const uint4*>(
                        wl + mt * (32 * RECP) + vv * RECP + (ck * 2 + sub) * 16);
                    if (ok)
                        *reinterpret_cast<uint4*>(dplane + ((size_t)ck * patch_vox + vox) * 32 + sub * 16) = val;
                    if (CARRY && ok && cz_on && gz >= a.out_z0 && gz < a.out_z1)
                        *reinterpret_cast<uint4*>(cplane + ((size_t)ck * patch_vox + vox) * 32 + sub * 16) = val;
                }
            }
        }
        // MaxPool3d(2): piece p = 16-byte group "sub" of pooled voxel (pz, py, px) in chunk plane ck
        // of cout slice wn; lanes run along (px, sub), so a row of the pooled tile is one run of
        // TX / 2 x 32 contiguous bytes
        constexpr int PX = TX / 2, PY = TY / 2, PZ = TZ / 2;
        constexpr int NPIECE = 2 * PX * PY * PZ * NPL * WAVES_N;
        const int pd = a.d >> 1, ph = a.h >> 1, pw2 = a.w >> 1;
        const size_t pvox = (size_t)pd * ph * pw2;
        const char* const lb = reinterpret_cast<const char*>(lds);
#pragma unroll
        for (int p0 = 0; p0 < NPIECE; p0 += NTHREADS) {
            const int pp = p0 + tid;
            const int sub = pp & 1, px = (pp >> 1) % PX;
            int rest = (pp >> 1) / PX;
            const int py = rest % PY; rest /= PY;
            const int pz = rest % PZ; rest /= PZ;
            const int ck = rest % NPL, pwn = rest / NPL;
            const int qz = (z0 >> 1) + pz, qy = (y0 >> 1) + py, qx = (x0 >> 1) + px;
            // (BCARRY: a pooled plane of the masked tile belongs to the carried range, whose planes this tile's
            // LDS image does not hold; z0 and zend are even, so a pooled pair is never split)
            if (pp < NPIECE && qz < pd && qy < ph && qx < pw2 && (!BCARRY || 2 * qz < zend)) {
                uint4 mx;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int m = ((2 * pz + (k >> 2)) * TY + 2 * py + ((k >> 1) & 1)) * TX + 2 * px + (k & 1);
                    const int w_src = (m / (MT * 32)) * WAVES_N + pwn;      // wave that produced it
                    const uint4 v = *reinterpret_cast<const uint4*>(
                        lb + (size_t)((w_src * MT + (m / 32) % MT) * 32 + m % 32) * RECP + (ck * 2 + sub) * 16);
                    if (ES == 2) mx = k == 0 ? okey16<Tag::kInf16>(v) : maxkey16(mx, okey16<Tag::kInf16>(v));   // order-preserving keys
                    else mx = k == 0 ? v : max16<Tag>(mx, v);
                }
                if (ES == 2) mx = key16(mx);
                const int ptile = (blockIdx.y * WAVES_N + pwn) * NT;   // first 32-cout tile of that slice
                char* const pplane = static_cast<char*>(a.pool_dst) +
                                     ((size_t)nb * (a.cout / KC) + ptile * (32 / KC) + ck) * pvox * 32;
                *reinterpret_cast<uint4*>(pplane + (((size_t)qz * ph + qy) * pw2 + qx) * 32 + sub * 16) = mx;
                if (CARRY && cz_on && 2 * qz >= a.out_z0 && 2 * qz < a.out_z1) {
                    // carry out of the pooled planes [out_z0 / 2, out_z1 / 2), at pooled plane - out_shift / 2
                    char* const cpplane = static_cast<char*>(a.carry_pool_dst) +
                                          ((size_t)nb * (a.cout / KC) + ptile * (32 / KC) + ck) * pvox * 32;
                    *reinterpret_cast<uint4*>(cpplane + (((size_t)(qz - (a.out_shift >> 1)) * ph + qy) * pw2 + qx) * 32 +
                                              sub * 16) = mx;
                }
            }
        }
        EXA_TRACE(14);
        return;
    }
    if (ES == 2) {
        // 16-bit types: records assembled with v_permlane32_swap (record_half), no LDS round trip
        char* const dplane = static_cast<char*>(a.dst) +
                             ((size_t)nb * (a.cout / KC) + ntile0 * (32 / KC)) * patch_vox * 32;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int m = (wm * MT + mt) * 32 + r;
            const int z = m / (TY * TX), y = (m / TX) % TY, x = m % TX;
            const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
            const bool ok = m < TILE_VOX && gz < zend && gy < yend && gx < xend;
            char* const dvox = dplane + (((size_t)gz * a.h + gy) * a.w + gx) * 32 + half * 16;
            // carry out: the same record once more, out_shift planes up in carry_dst
            char* const cvox = static_cast<char*>(a.carry_dst) + (dvox - static_cast<char*>(a.dst)) -
                               (size_t)a.out_shift * a.h * a.w * 32;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                uint2 grp[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    grp[q] = pack4<Tag>(leaky(acc[mt][nt][4 * q + 0], a.slope), leaky(acc[mt][nt][4 * q + 1], a.slope),
                                        leaky(acc[mt][nt][4 * q + 2], a.slope), leaky(acc[mt][nt][4 * q + 3], a.slope));
#pragma unroll
                for (int ck = 0; ck < 2; ++ck) {
                    const uint4 rec = record_half(grp[2 * ck], grp[2 * ck + 1]);
                    if (ok) *reinterpret_cast<uint4*>(dvox + (size_t)(nt * 2 + ck) * patch_vox * 32) = rec;
                    if (CARRY && ok && cz_on && gz >= a.out_z0 && gz < a.out_z1)
                        *reinterpret_cast<uint4*>(cvox + (size_t)(nt * 2 + ck) * patch_vox * 32) = rec;
                }
            }
        }
        EXA_TRACE(14);
        return;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cl = nt * 32 + 8 * q + 4 * half;  // channel inside the slice
                // LeakyReLU with 0 <= slope <= 1 is max(v, slope * v)
                float v0 = acc[mt][nt][4 * q + 0], v1 = acc[mt][nt][4 * q + 1];
                float v2 = acc[mt][nt][4 * q + 2], v3 = acc[mt][nt][4 * q + 3];
                v0 = leaky(v0, a.slope);
                v1 = leaky(v1, a.slope);
                v2 = leaky(v2, a.slope);
                v3 = leaky(v3, a.slope);
                store4<Tag>(wl, (size_t)(r * RECP) / ES + cl, v0, v1, v2, v3);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // one store instruction = one chunk plane's 32 voxel records (32 B each)
        constexpr int NPL = RECB / 32;           // chunk planes of this wave's output slice
        const int vv = lane >> 1, sub = lane & 1;
        const int m = (wm * MT + mt) * 32 + vv;
        const int z = m / (TY * TX), y = (m / TX) % TY, x = m % TX;
        const int gz = z0 + z, gy = y0 + y, gx = x0 + x;
        const bool ok = m < TILE_VOX && gz < zend && gy < yend && gx < xend;
        const size_t vox = ((size_t)gz * a.h + gy) * a.w + gx;
        char* const dplane = static_cast<char*>(a.dst) +
                             ((size_t)nb * (a.cout / KC) + ntile0 * (32 / KC)) * patch_vox * 32;
#pragma unroll
        for (int ck = 0; ck < NPL; ++ck) {
            const uint4 val = *reinterpret_cast<const uint4*>(wl + vv * RECP + (ck * 2 + sub) * 16);
            if (ok)
                *reinterpret_cast<uint4*>(dplane + ((size_t)ck * patch_vox + vox) * 32 + sub * 16) = val;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    EXA_TRACE(14);
