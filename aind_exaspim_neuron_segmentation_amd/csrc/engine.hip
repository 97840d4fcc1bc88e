// UNet3D.forward (machine_learning/unet3d.py:77-105) as a fixed sequence of
// kernel launches on the caller's stream, plus the extern "C" model API.
//
// Workspace: per pyramid level l (voxels n*d*h*w / 8^l) three channels-last
// buffers -- skip[l] (x1..x4, alive until the decoder consumes them), A[l] and
// B[l] (ping-pong) -- each sized for the widest tensor stored at that level.

#include <algorithm>
#include <cstdlib>
#include <new>
#include <string_view>

#include "common.h"

namespace exaspim {

constexpr float kLeakySlope = 0.01f;  // unet3d.py:145,148

struct Workspace {
    size_t skip[5], a[5], b[5];
    size_t xpad;  // zero-bordered float32 copy of the input patches (inc.0)
    size_t bytes;
};

}  // namespace exaspim

// Optional per-layer timing with HIP events recorded on the launch stream
// (exaspim_unet_timing_*): a ring of event pairs around the MFMA convolutions
// selected by a layer mask.
struct LayerTimer {
    static constexpr int kRing = 16384;
    uint32_t mask = 0;
    int next = 0, used = 0;
    hipEvent_t start[kRing], stop[kRing];
    int layer[kRing];
    bool created = false;
};

struct exaspim_unet {
    exaspim::UNetPlan plan;
    int device;
    const char* packed;  // device image (caller-owned)
    LayerTimer* timer = nullptr;
    uint32_t options = 0;   // EXASPIM_OPT_* (exaspim_unet_set_options)
};

namespace exaspim {

static bool level_dims_ok(int d, int h, int w) {
    return d > 0 && h > 0 && w > 0 && d % 16 == 0 && h % 16 == 0 && w % 16 == 0;
}

// pyramid level of the i-th MFMA conv (inc.3 = 0 ... up4.3 = 16)
static int conv_level(int i) {
    if (i == 0) return 0;
    if (i <= 8) return (i + 1) / 2;          // down1..down4 -> 1..4
    return 3 - (i - 9) / 2;                  // up1..up4 -> 3..0
}

// Planes [out[0], out[1]) of a forward's own frame that hold what a forward shift_z planes earlier computed at
// its planes + shift_z: the whole tiles (of the depth inc.3's launcher picks) inside [2, d - shift_z - 2),
// even bounds. Empty: {0, 0}.
static void carry_span(int d, int shift_z, int32_t out[2]) {
    out[0] = out[1] = 0;
    if (shift_z <= 0 || shift_z % 2 != 0 || shift_z >= d) return;
    const int tz = conv_zcol_tile_depth(d);
    const int step = tz % 2 == 0 ? tz : 2 * tz;
    const int lo = (2 + step - 1) / step * step, hi = (d - shift_z - 2) / step * step;
    // (a whole number of tiles whichever way: bounds are multiples of the tile depth and even)
    if (lo < hi && hi + shift_z <= 254) { out[0] = lo; out[1] = hi; }
}

// The same along y: rows of a forward's own frame that hold what a forward shift_y rows earlier computed at its
// rows + shift_y: the whole 8-row tiles of the z-column kernel inside [2, h - shift_y - 2). Empty: {0, 0}.
static void carry_row_span(int h, int shift_y, int32_t out[2]) {
    out[0] = out[1] = 0;
    if (shift_y <= 0 || shift_y % 2 != 0 || shift_y >= h) return;
    constexpr int ty = 8;
    const int lo = ty, hi = (h - shift_y - 2) / ty * ty;
    if (lo < hi) { out[0] = lo; out[1] = hi; }
}

// What inc.0 need not write when inc.3 takes planes [in_z0, in_z1) over (common.h)
void conv_first_skip_planes(int d, int in_z0, int in_z1, int32_t out[2]) {
    out[0] = out[1] = 0;
    if (in_z0 < 0 || in_z1 > d || in_z1 - in_z0 <= 2) return;
    out[0] = in_z0 + 1;
    out[1] = in_z1 - 1;
}

// Tile depth of down1.0 and down1.3 if the launcher runs both on the configuration that can carry planes and
// down1.3 writes its own max-pool (the forward of a batch of n patches d x h x w), else 0
static int carry1_tile_depth(const exaspim_unet* e, int n, int d, int h, int w) {
    const UNetPlan& p = e->plan;
    if ((e->options & (EXASPIM_OPT_SEPARATE_POOL | EXASPIM_OPT_SEPARATE_DEEP_POOLS)) ||
        !conv_can_fuse_pool(p.dtype, p.conv[2].cout, d >> 1, h >> 1, w >> 1))
        return 0;
    int tz = 0;
    for (int idx = 1; idx <= 2; ++idx) {
        static float scratch;   // (forward() offers split-K scratch of this size; only its presence is read here)
        ConvArgs a{};
        a.ca = p.conv[idx].ca; a.cb = p.conv[idx].cb; a.cout = p.conv[idx].cout;
        a.n = n; a.d = d >> 1; a.h = h >> 1; a.w = w >> 1;
        a.partial = &scratch;
        a.partial_patch_bytes = (size_t)(d + 2) * (h + 2) * (w + 2) * sizeof(float);
        const int t = conv_carry_t14_tile_depth(p.dtype, a);
        if (t == 0 || (tz != 0 && t != tz)) return 0;
        tz = t;
    }
    return tz;
}

// carry_span for the second level, in level-1 planes: the whole tiles inside [3, d/2 - shift_z/2 - 3) -- down1.3
// is clear of the zero padding along z on planes [3, d/2 - 3), down1.0 on one more either side, and the pooled
// planes pair up only for an even level-1 shift. Empty unless the first level carries too. tz: the tile depth of
// the two layers (even).
void carry1_span_of_tiles(int tz, int d, int shift_z, int32_t out[2]) {
    out[0] = out[1] = 0;
    int32_t l0[2];
    carry_span(d, shift_z, l0);
    if (l0[0] >= l0[1] || shift_z % 4 != 0 || tz <= 0 || tz % 2 != 0) return;
    const int d1 = d / 2, s1 = shift_z / 2;
    const int lo = (3 + tz - 1) / tz * tz, hi = (d1 - s1 - 3) / tz * tz;
    if (lo < hi && hi + s1 <= 254) { out[0] = lo; out[1] = hi; }
}
static void carry1_span(const exaspim_unet* e, int n, int d, int h, int w, int shift_z, int32_t out[2]) {
    carry1_span_of_tiles(carry1_tile_depth(e, n, d, h, w), d, shift_z, out);   // (no configuration that carries: depth 0)
}

static Workspace make_workspace(const UNetPlan& p, int n, int d, int h, int w) {
    // widest tensor stored at each level: every input and output of its convs
    // (the pooled / upsampled tensors are inputs of the level's first conv)
    int maxc[5] = {p.c0p, 0, 0, 0, 0};
    for (int i = 0; i < kNumMfmaConvs; ++i) {
        const ConvLayer& L = p.conv[i];
        int& m = maxc[conv_level(i)];
        m = std::max(m, std::max(std::max(L.ca, L.cb), L.cout));
    }
    const size_t es = dtype_size(p.dtype);
    Workspace ws;
    size_t off = 0;
    for (int l = 0; l < 5; ++l) {
        const size_t vox = (size_t)n * (d >> l) * (h >> l) * (w >> l);
        const size_t sz = align_up(vox * maxc[l] * es, 256);
        ws.skip[l] = off; off += (l < 4 ? sz : 0);
        ws.a[l] = off; off += sz;
        ws.b[l] = off; off += sz;
    }
    ws.xpad = off;
    off += align_up((size_t)n * (d + 2) * (h + 2) * (w + 2) * sizeof(float), 256);
    ws.bytes = off;
    return ws;
}

// x: float32 patches, or (x == nullptr) x_prepared: the first convolution's operand layout
// absmax (optional): float[1 + kNumMfmaConvs + 4], the largest |activation| inc.0, every MFMA
// convolution and every ConvTranspose3d stored (range probe: nothing is fused away, nothing trimmed)
// row_stride > 0: the caller says the n patches are one row along x, row_stride voxels apart
// keep_hi (optional, int32[3]): of the trimmed outputs the caller keeps local [trim, keep_hi[axis]) only -- a
// patch that ends beyond the volume, whose far part the stitch drops. Checked by the entry point; plans
// that do not trim ignore it.
static int forward(exaspim_unet* e, const float* x, float* out, int n, int d, int h, int w,
                   int apply_sigmoid, int trim, void* workspace, size_t workspace_bytes,
                   hipStream_t stream, const void* x_prepared = nullptr, float* absmax = nullptr,
                   int row_stride = 0, const int32_t* keep_hi = nullptr, const exaspim_unet_carry* carry = nullptr,
                   const exaspim_unet_carry1* carry1 = nullptr, const exaspim_unet_carry_y* carry_y = nullptr) {
    const UNetPlan& p = e->plan;
    const Workspace ws = make_workspace(p, n, d, h, w);
    if (workspace_bytes < ws.bytes) {
        set_error("forward: workspace %zu bytes < required %zu", workspace_bytes, ws.bytes);
        return EXASPIM_E_WORKSPACE;
    }
    char* base = static_cast<char*>(workspace);
    auto skip = [&](int l) { return (void*)(base + ws.skip[l]); };
    auto A = [&](int l) { return (void*)(base + ws.a[l]); };
    auto B = [&](int l) { return (void*)(base + ws.b[l]); };
    const int dt = p.dtype;
    int rc;

    // the last conv (up4.3) can run the 1x1x1 head on its accumulators
    // (the bf16x3 mode through a launcher of its own, launch_conv3x3x3_x3_head, whose head has the bits
    // of the separate launch; its max-pools are launches of their own and it has no row mode)
    // EXASPIM_OPT_SEPARATE_HEAD: the head as its own launch over the whole patch, hence nothing trimmed
    const bool x3 = dt == EXASPIM_DT_BF16X3;
    const int last_cout = p.conv[kNumMfmaConvs - 1].cout;
    const bool fuse_head = !absmax && !(e->options & EXASPIM_OPT_SEPARATE_HEAD) &&
                           (x3 ? conv_x3_can_fuse_head(last_cout, w, p.out_channels)
                               : conv_can_fuse_head(last_cout, w, p.out_channels, dt));
    // With the head fused, voxels within "trim" of a patch face are never read again:
    // up4.3 skips them, and up4.0 everything its 3x3x3 consumer does not reach.
    const bool trimmed = fuse_head && trim > 0 && 2 * trim < d && 2 * trim < h && 2 * trim < w;
    // ... and voxels from khi on (clipped forward: the patch reaches beyond the volume there) neither
    int khi[3] = {d - trim, h - trim, w - trim};
    if (trimmed && keep_hi)
        for (int i = 0; i < 3; ++i) khi[i] = keep_hi[i];
    // conv 2l (inc.3, down1.3, down2.3, down3.3) can write its own max-pool, the input of level l + 1
    // (EXASPIM_OPT_SEPARATE_POOL, set per handle: run the stand-alone max-pool launches instead -- the
    // tests hold the two to each other bit for bit)
    const bool separate_pool = (e->options & EXASPIM_OPT_SEPARATE_POOL) != 0;
    const bool separate_deep = (e->options & EXASPIM_OPT_SEPARATE_DEEP_POOLS) != 0;   // only inc.3 keeps its pool
    bool fuse_pool[4];
    for (int l = 0; l < 4; ++l)
        fuse_pool[l] = !separate_pool && !(separate_deep && l > 0) && conv_can_fuse_pool(p.dtype, p.conv[2 * l].cout, d >> l, h >> l, w >> l);
    // Row mode of inc.3 (ConvArgs::row_stride): a column two neighbours share is computed once, the
    // two outermost x of every patch face that borders a neighbour and their pooled column are
    // recomputed in the patch's own frame by the border launch that follows (launch_conv3x3x3_row;
    // EXASPIM_OPT_ROW_SEPARATE_BORDERS: by two thin-tile launches and a column max-pool). Same
    // bits: a voxel's products are summed in the same order on every tile shape.
    // (EXASPIM_OPT_PER_PATCH_ENCODER: every patch on its own, as without a row.)
    const bool row = !absmax && !(e->options & EXASPIM_OPT_PER_PATCH_ENCODER) &&
                     conv_row_mode_ok(dt, p.conv[0].cout, n, w, row_stride, fuse_pool[0]);
    // carried planes (exaspim_unet_forward_prepared_carry): x1 and its max-pool live in the caller's buffers
    if (carry) {
        int32_t span[2];
        const int shift = carry->out_skip ? carry->out_shift : 0;
        const bool in = carry->in_z[0] != 0 || carry->in_z[1] != 0;
        EXA_CHECK_ARG(row && carry->own_skip && carry->own_pool && carry->reserved == 0,
                      "forward: carried planes need row mode at this geometry and both own buffers");
        EXA_CHECK_ARG(!carry->out_skip == !carry->out_pool, "forward: carry out needs both targets or neither");
        const int tzd = conv_zcol_tile_depth(d);
        // the range a successor may take over is what exaspim_unet_carry_planes gives for its shift; a range
        // carried in must be whole tiles with even bounds inside [2, d - 2)
        if (in)
            EXA_CHECK_ARG(carry->in_z[0] >= 2 && carry->in_z[0] < carry->in_z[1] && carry->in_z[1] <= d - 2 &&
                              carry->in_z[0] % tzd == 0 && carry->in_z[1] % tzd == 0 && carry->in_z[0] % 2 == 0 &&
                              carry->in_z[1] % 2 == 0,
                          "forward: carry in [%d, %d) is not whole %d-plane tiles with even bounds inside [2, %d)",
                          carry->in_z[0], carry->in_z[1], tzd, d - 2);
        if (shift || carry->out_skip) {
            carry_span(d, shift, span);
            EXA_CHECK_ARG(shift > 0 && span[0] < span[1] && carry->out_z[0] == span[0] + shift &&
                              carry->out_z[1] == span[1] + shift && carry->out_z[1] <= 254,
                          "forward: carry out [%d, %d) shifted by %d is not the range a forward %d planes down takes over",
                          carry->out_z[0], carry->out_z[1], shift, shift);
            // (the planes carried in are not computed here: their tiles run no epilogue that could store them again)
            EXA_CHECK_ARG(!in || carry->out_z[0] >= carry->in_z[1] || carry->out_z[1] <= carry->in_z[0],
                          "forward: carry out [%d, %d) overlaps the planes carried in, [%d, %d)", carry->out_z[0],
                          carry->out_z[1], carry->in_z[0], carry->in_z[1]);
        }
    }
    // rows carried along y (exaspim_unet_forward_prepared_carry_y): the row launch of inc.3 alone
    ConvCarryY cy;
    if (carry_y) {
        const bool in = carry_y->in_y[0] != 0 || carry_y->in_y[1] != 0;
        const bool out_y = carry_y->out_skip_y || carry_y->out_pool_y || carry_y->out_shift_y || carry_y->out_y[0] || carry_y->out_y[1];
        EXA_CHECK_ARG(carry && row && carry_y->reserved == 0,
                      "forward: carried rows need the first level's carry struct and row mode at this geometry");
        EXA_CHECK_ARG(!carry_y->out_skip_y == !carry_y->out_pool_y && !carry_y->out_skip_d == !carry_y->out_pool_d,
                      "forward: y and diagonal carry out need both targets or neither");
        if (in)
            EXA_CHECK_ARG(carry_y->in_y[0] >= 2 && carry_y->in_y[0] < carry_y->in_y[1] && carry_y->in_y[1] <= h - 2 &&
                              carry_y->in_y[0] % 8 == 0 && carry_y->in_y[1] % 8 == 0,
                          "forward: y carry in [%d, %d) is not whole 8-row tiles inside [2, %d)", carry_y->in_y[0],
                          carry_y->in_y[1], h - 2);
        if (out_y) {
            int32_t span[2];
            const int shift = carry_y->out_skip_y ? carry_y->out_shift_y : 0;
            carry_row_span(h, shift, span);
            EXA_CHECK_ARG(shift > 0 && span[0] < span[1] && carry_y->out_y[0] == span[0] + shift &&
                              carry_y->out_y[1] == span[1] + shift,
                          "forward: y carry out [%d, %d) shifted by %d is not the range a forward %d rows on takes over",
                          carry_y->out_y[0], carry_y->out_y[1], shift, shift);
            EXA_CHECK_ARG(!in || carry_y->out_y[0] >= carry_y->in_y[1] || carry_y->out_y[1] <= carry_y->in_y[0],
                          "forward: y carry out [%d, %d) overlaps the rows carried in, [%d, %d)", carry_y->out_y[0],
                          carry_y->out_y[1], carry_y->in_y[0], carry_y->in_y[1]);
        }
        EXA_CHECK_ARG(!carry_y->out_skip_d || (carry->out_skip && carry_y->out_skip_y),
                      "forward: the diagonal carry out needs both the z and the y carry out");
        if (!(e->options & EXASPIM_OPT_CARRY_NO_ROWS)) {
            cy.in_y0 = (unsigned short)carry_y->in_y[0];
            cy.in_y1 = (unsigned short)carry_y->in_y[1];
            if (carry_y->out_skip_y) {
                cy.y_dst = carry_y->out_skip_y;
                cy.y_pool_dst = carry_y->out_pool_y;
                cy.d_dst = carry_y->out_skip_d;
                cy.d_pool_dst = carry_y->out_pool_d;
                cy.out_y0 = (unsigned short)carry_y->out_y[0];
                cy.out_y1 = (unsigned short)carry_y->out_y[1];
                cy.out_shift_y = (unsigned short)carry_y->out_shift_y;
            }
        }
    }
    // With a carry in the border launch leaves the carried planes out as well and carries out whenever the main
    // launch does (kRowStageBordersCarry), and inc.0 skips the planes neither launch reads.
    // EXASPIM_OPT_CARRY_MAIN_ONLY, or the three-launch borders: only the main launch carries, the border launch
    // and inc.0 write every plane. An option of the handle: predecessor and successor agree on who writes the
    // border columns of the carried planes.
    const bool carry_borders = carry && !(e->options & (EXASPIM_OPT_CARRY_MAIN_ONLY | EXASPIM_OPT_ROW_SEPARATE_BORDERS));
    int32_t first_skip[2] = {0, 0};
    if (carry_borders) conv_first_skip_planes(d, carry->in_z[0], carry->in_z[1], first_skip);
    void* const x1 = carry ? carry->own_skip : skip(0);
    void* const x1_pool = carry ? carry->own_pool : A(1);
    // ... and (exaspim_unet_forward_prepared_carry1) down1.0's output, x2 and its max-pool
    if (carry1) {
        EXA_CHECK_ARG(carry && carry1->own_mid1 && carry1->own_skip1 && carry1->own_pool2 && carry1->reserved == 0,
                      "forward: carried planes of the second level need those of the first and all three own buffers");
        EXA_CHECK_ARG(!carry1->out_mid1 == !carry1->out_skip1 && !carry1->out_mid1 == !carry1->out_pool2,
                      "forward: second-level carry out needs all three targets or none");
        const int tz1 = carry1_tile_depth(e, n, d, h, w);
        EXA_CHECK_ARG(tz1 > 0, "forward: down1.0 and down1.3 cannot carry planes at this geometry, dtype or option set");
        if (carry1->in_z[0] != 0 || carry1->in_z[1] != 0)
            EXA_CHECK_ARG((carry->in_z[0] != 0 || carry->in_z[1] != 0) && carry1->in_z[0] >= 3 &&
                              carry1->in_z[0] < carry1->in_z[1] && carry1->in_z[1] <= d / 2 - 3 &&
                              carry1->in_z[0] % tz1 == 0 && carry1->in_z[1] % tz1 == 0,
                          "forward: second-level carry in [%d, %d) needs a first-level carry in and whole %d-plane tiles "
                          "inside [3, %d)", carry1->in_z[0], carry1->in_z[1], tz1, d / 2 - 3);
        if (carry1->out_mid1 || carry1->out_shift) {
            int32_t span[2];
            const int shift1 = carry1->out_mid1 ? carry1->out_shift : 0;
            carry1_span(e, n, d, h, w, 2 * shift1, span);
            EXA_CHECK_ARG(shift1 > 0 && carry->out_skip && carry->out_shift == 2 * shift1 && span[0] < span[1] &&
                              carry1->out_z[0] == span[0] + shift1 && carry1->out_z[1] == span[1] + shift1,
                          "forward: second-level carry out [%d, %d) shifted by %d is not the range a forward %d planes down "
                          "takes over, or the first level does not carry out by twice the shift",
                          carry1->out_z[0], carry1->out_z[1], shift1, 2 * shift1);
            EXA_CHECK_ARG(carry1->out_z[0] >= carry1->in_z[1] || carry1->out_z[1] <= carry1->in_z[0],
                          "forward: second-level carry out [%d, %d) overlaps the planes carried in, [%d, %d)",
                          carry1->out_z[0], carry1->out_z[1], carry1->in_z[0], carry1->in_z[1]);
        }
    }
    void* const mid1 = carry1 ? carry1->own_mid1 : B(1);
    void* const skip1 = carry1 ? carry1->own_skip1 : skip(1);
    void* const pool2 = carry1 ? carry1->own_pool2 : A(2);
    auto conv = [&](int idx, const void* sa, const void* sb, void* dst, int l) -> int {
        const ConvLayer& L = p.conv[idx];
        ConvArgs a;
        // the last conv of an encoder level writes its 2x2x2 max-pool (the next level's input) too
        // split-K scratch: the zero-bordered input copy is dead once inc.0 has run
        a.partial = reinterpret_cast<float*>(base + ws.xpad);
        a.partial_patch_bytes = (size_t)(d + 2) * (h + 2) * (w + 2) * sizeof(float);
        if (idx <= 6 && idx % 2 == 0 && fuse_pool[idx / 2]) a.pool_dst = idx == 0 ? x1_pool : idx == 2 ? pool2 : A(idx / 2 + 1);
        // up4.3 produces [trim, khi) (khi = size - trim unless clipped), up4.0 one voxel more on every face
        const bool last = idx == kNumMfmaConvs - 1, last_but_one = idx == kNumMfmaConvs - 2;
        const int margin = !trimmed ? 0 : last ? trim : last_but_one ? trim - 1 : 0;
        const int full[3] = {d >> l, h >> l, w >> l};
        for (int i = 0; i < 3; ++i) {
            a.org[i] = margin;
            a.ext[i] = trimmed && (last || last_but_one) ? khi[i] + (last ? 0 : 1) - margin : full[i];
        }
        // When the region is a few voxels more than whole z-column tiles along y or x (82 =
        // 10 x 8 + 2 = 5 x 16 + 2 for the default patch), the z-column kernel covers the whole
        // tiles and two launches on 2-voxel-thick tiles the rest, instead of a ninth row and a
        // sixth column of mostly masked 8 x 16 tiles (924 tiles for 718 tiles' worth of voxels).
        int rem_y = 0, rem_x = 0;
        const bool has_head = idx == kNumMfmaConvs - 1 && fuse_head;   // the head runs on masked main tiles only
        if (margin > 0 && !has_head && L.cout % 64 != 0 && full[2] % 16 == 0) {
            rem_y = a.ext[1] - conv_zcol_main_extent(a.ext[1], 1);
            rem_x = a.ext[2] - conv_zcol_main_extent(a.ext[2], 2);
            a.ext[1] -= rem_y;
            a.ext[2] -= rem_x;
        }
        if (idx == kNumMfmaConvs - 1 && fuse_head) {
            a.head_w = reinterpret_cast<const float*>(e->packed + p.head_w_off);
            a.head_b = reinterpret_cast<const float*>(e->packed + p.head_b_off);
            a.head_out = out;
            a.head_oc = p.out_channels;
            a.head_sigmoid = apply_sigmoid;
        }
        a.src_a = sa; a.src_b = sb; a.ca = L.ca; a.cb = L.cb;
        a.weights = e->packed + L.w_off;
        a.bias = reinterpret_cast<const float*>(e->packed + L.b_off);
        a.dst = dst; a.cout = L.cout;
        a.n = n; a.d = d >> l; a.h = h >> l; a.w = w >> l;
        a.slope = kLeakySlope;
        if (idx == 0 && row) a.row_stride = row_stride;
        if (idx == 0 && carry) {
            a.in_z0 = (unsigned short)carry->in_z[0];
            a.in_z1 = (unsigned short)carry->in_z[1];
            if (carry->out_skip) {
                a.carry_dst = carry->out_skip;
                a.carry_pool_dst = carry->out_pool;
                a.out_z0 = (unsigned char)carry->out_z[0];
                a.out_z1 = (unsigned char)carry->out_z[1];
                a.out_shift = (unsigned short)carry->out_shift;
            }
        }
        if ((idx == 1 || idx == 2) && carry1) {
            a.in_z0 = (unsigned short)carry1->in_z[0];
            a.in_z1 = (unsigned short)carry1->in_z[1];
            if (carry1->out_mid1) {
                a.carry_dst = idx == 1 ? carry1->out_mid1 : carry1->out_skip1;
                a.carry_pool_dst = idx == 1 ? nullptr : carry1->out_pool2;
                a.out_z0 = (unsigned char)carry1->out_z[0];
                a.out_z1 = (unsigned char)carry1->out_z[1];
                a.out_shift = (unsigned short)carry1->out_shift;
            }
        }
        LayerTimer* t = e->timer;
        const bool timed = t && (t->mask >> idx & 1u) && t->used < LayerTimer::kRing;
        int slot = 0;
        if (timed) {
            slot = t->next;
            EXA_CHECK_HIP(hipEventRecord(t->start[slot], stream));
        }
        // (row mode: the row launch, then the border launch that finishes it)
        int r = x3 && has_head      ? launch_conv3x3x3_x3_head(a, stream)
                : a.row_stride > 0 ? launch_conv3x3x3_row(dt, a, (e->options & EXASPIM_OPT_ROW_SEPARATE_BORDERS) ? kRowStagesAll
                                                                 : carry_borders ? kRowStagesCarry : kRowStagesFused, stream,
                                                        idx == 0 ? &cy : nullptr)
                                   : launch_conv3x3x3(dt, a, stream);
        if (timed && r == EXASPIM_OK) {
            EXA_CHECK_HIP(hipEventRecord(t->stop[slot], stream));
            t->layer[slot] = idx;
            t->next = (slot + 1) % LayerTimer::kRing;
            t->used++;
        }
        if (r == EXASPIM_OK && rem_y > 0) {      // rows [org_y + main, org_y + main + rem_y), every x of the region
            ConvArgs b = a;
            b.org[1] = a.org[1] + a.ext[1]; b.ext[1] = rem_y;
            b.ext[2] = a.ext[2] + rem_x;
            r = launch_conv3x3x3_thin(dt, b, stream);
        }
        if (r == EXASPIM_OK && rem_x > 0) {      // columns beyond the whole tiles, rows of the main part
            ConvArgs b = a;
            b.org[2] = a.org[2] + a.ext[2]; b.ext[2] = rem_x;
            r = launch_conv3x3x3_thin(dt, b, stream);
        }
        if (r == EXASPIM_OK && absmax)
            r = launch_absmax(dt, dst, (size_t)n * (d >> l) * (h >> l) * (w >> l) * L.cout * dtype_size(dt),
                              absmax + 1 + idx, stream);
        return r;
    };
#define RUN(expr) do { rc = (expr); if (rc) return rc; } while (0)

    // encoder (unet3d.py:93-97)
    RUN(launch_conv_first(dt, x, x ? reinterpret_cast<float*>(base + ws.xpad)
                                   : const_cast<float*>(static_cast<const float*>(x_prepared)),
                          reinterpret_cast<const float*>(e->packed + p.first_w_off),
                          reinterpret_cast<const float*>(e->packed + p.first_b_off), A(0), n, d,
                          h, w, p.c0p, kLeakySlope, stream, (e->options & EXASPIM_OPT_FIRST_PER_GROUP) != 0,
                          first_skip[0], first_skip[1]));
    if (absmax) RUN(launch_absmax(dt, A(0), (size_t)n * d * h * w * p.c0p * dtype_size(dt), absmax, stream));
    RUN(conv(0, A(0), nullptr, x1, 0));                           // x1
    if (carry_y && carry_y->encoder_event)    // every carry out of this forward has been issued
        EXA_CHECK_HIP(hipEventRecord(static_cast<hipEvent_t>(carry_y->encoder_event), stream));
    for (int l = 1; l <= 4; ++l) {
        const ConvLayer& L0 = p.conv[2 * l - 1];
        const void* prev = l == 1 ? x1 : l == 2 ? skip1 : skip(l - 1);
        if (!fuse_pool[l - 1])
            RUN(launch_maxpool2(dt, prev, A(l), n, d >> (l - 1), h >> (l - 1), w >> (l - 1), L0.ca,
                                stream));
        void* const mid = l == 1 ? mid1 : B(l);
        RUN(conv(2 * l - 1, l == 1 ? x1_pool : l == 2 ? pool2 : A(l), nullptr, mid, l));
        RUN(conv(2 * l, mid, nullptr, l == 1 ? skip1 : l < 4 ? skip(l) : A(l), l));  // x2..x4, x5 in A(4)
    }
    // decoder (unet3d.py:100-103): y = DoubleConv(cat[skip, up(prev)])
    const void* prev = A(4);
    for (int l = 3; l >= 0; --l) {
        const int i0 = 9 + 2 * (3 - l);  // up1.0 = conv[9], up2.0 = conv[11], ...
        const ConvLayer& L0 = p.conv[i0];
        if (p.convt) {
            const ConvTLayer& U = p.up[3 - l];
            RUN(launch_convt2(dt, prev, e->packed + U.w_off,
                              reinterpret_cast<const float*>(e->packed + U.b_off), A(l), n,
                              d >> (l + 1), h >> (l + 1), w >> (l + 1), U.cin, U.cout, stream));
            if (absmax)     // (a transposed convolution is not bounded by its input like the interpolation is)
                RUN(launch_absmax(dt, A(l), (size_t)n * (d >> l) * (h >> l) * (w >> l) * U.cout * dtype_size(dt),
                                  absmax + 1 + kNumMfmaConvs + (3 - l), stream));
        } else {
            // up4.0 reads the upsampled tensor one voxel beyond its own trimmed output
            const bool ups_trimmed = trimmed && l == 0 && trim > 2;
            const int ups_hi[3] = {std::max(d - khi[0] - 2, 0), std::max(h - khi[1] - 2, 0), std::max(w - khi[2] - 2, 0)};
            RUN(launch_upsample2(dt, prev, A(l), n, d >> (l + 1), h >> (l + 1), w >> (l + 1), L0.cb,
                                 ups_trimmed ? trim - 2 : 0, stream,
                                 (e->options & EXASPIM_OPT_PLAIN_UPSAMPLE) != 0,
                                 (e->options & EXASPIM_OPT_UPSAMPLE_PER_THREAD) != 0, ups_trimmed ? ups_hi : nullptr));
        }
        RUN(conv(i0, l == 0 ? x1 : l == 1 ? skip1 : skip(l), A(l), B(l), l));
        RUN(conv(i0 + 1, B(l), nullptr, A(l), l));
        prev = A(l);
    }
    if (!fuse_head)
    RUN(launch_head(dt, prev, reinterpret_cast<const float*>(e->packed + p.head_w_off),
                    reinterpret_cast<const float*>(e->packed + p.head_b_off), out, n, d, h, w,
                    p.c0p, p.out_channels, apply_sigmoid, stream));
#undef RUN
    return EXASPIM_OK;
}

}  // namespace exaspim

using namespace exaspim;

extern "C" int exaspim_abi_version(void) { return EXASPIM_ABI_VERSION; }
extern "C" const char* exaspim_last_error(void) { return get_error(); }

extern "C" size_t exaspim_unet_param_count(const int32_t channels[5], int32_t out_channels,
                                           int32_t dtype) {
    UNetPlan p;
    if (!make_plan(channels, out_channels, dtype, &p)) return 0;
    return p.n_params;
}

extern "C" size_t exaspim_unet_packed_bytes(const int32_t channels[5], int32_t out_channels,
                                            int32_t dtype) {
    UNetPlan p;
    if (!make_plan(channels, out_channels, dtype, &p)) return 0;
    return p.packed_bytes;
}

extern "C" int exaspim_unet_pack_weights(const int32_t channels[5], int32_t out_channels,
                                         int32_t dtype, const float* params, size_t n_params,
                                         void* packed_host, size_t packed_bytes) {
    UNetPlan p;
    if (!make_plan(channels, out_channels, dtype, &p)) return EXASPIM_E_INVALID;
    EXA_CHECK_ARG(params && packed_host, "pack_weights: NULL pointer");
    EXA_CHECK_ARG(n_params == p.n_params, "pack_weights: got %zu parameters, expected %zu",
                  n_params, p.n_params);
    EXA_CHECK_ARG(packed_bytes == p.packed_bytes, "pack_weights: buffer %zu bytes, expected %zu",
                  packed_bytes, p.packed_bytes);
    return pack_weights(p, params, packed_host);
}

extern "C" int exaspim_unet_create(const int32_t channels[5], int32_t out_channels,
                                   int32_t dtype, int32_t device, const void* packed_dev,
                                   size_t packed_bytes, exaspim_unet** out) {
    EXA_CHECK_ARG(out != nullptr && packed_dev != nullptr, "create: NULL pointer");
    UNetPlan p;
    if (!make_plan(channels, out_channels, dtype, &p)) return EXASPIM_E_INVALID;
    EXA_CHECK_ARG(packed_bytes == p.packed_bytes, "create: packed image %zu bytes, expected %zu",
                  packed_bytes, p.packed_bytes);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        set_error("create: device %d not available (%d HIP devices visible)", device, ndev);
        return EXASPIM_E_NODEVICE;
    }
    hipDeviceProp_t prop;
    EXA_CHECK_HIP(hipGetDeviceProperties(&prop, device));
    if (std::string_view(prop.gcnArchName).substr(0, 6) != "gfx950") {
        set_error("create: device %d is %s; this library is built for gfx950 only", device,
                  prop.gcnArchName);
        return EXASPIM_E_NODEVICE;
    }
    exaspim_unet* e = new (std::nothrow) exaspim_unet;
    EXA_CHECK_ARG(e != nullptr, "create: out of host memory");
    e->plan = p;
    e->device = device;
    e->packed = static_cast<const char*>(packed_dev);
    *out = e;
    return EXASPIM_OK;
}

extern "C" void exaspim_unet_destroy(exaspim_unet* h) {
    if (!h) return;
    if (h->timer) {
        if (h->timer->created)
            for (int i = 0; i < LayerTimer::kRing; ++i) {
                (void)hipEventDestroy(h->timer->start[i]);
                (void)hipEventDestroy(h->timer->stop[i]);
            }
        delete h->timer;
    }
    delete h;
}

extern "C" int exaspim_unet_timing_begin(exaspim_unet* h, uint32_t conv_mask) {
    EXA_CHECK_ARG(h != nullptr, "timing_begin: NULL handle");
    if (!h->timer) h->timer = new (std::nothrow) LayerTimer;
    EXA_CHECK_ARG(h->timer != nullptr, "timing_begin: out of host memory");
    LayerTimer* t = h->timer;
    if (!t->created) {
        for (int i = 0; i < LayerTimer::kRing; ++i) {
            EXA_CHECK_HIP(hipEventCreate(&t->start[i]));
            EXA_CHECK_HIP(hipEventCreate(&t->stop[i]));
        }
        t->created = true;
    }
    t->mask = conv_mask;
    t->next = 0;
    t->used = 0;
    return EXASPIM_OK;
}

extern "C" int exaspim_unet_timing_read(exaspim_unet* h, double ms_sum[17], int32_t count[17]) {
    EXA_CHECK_ARG(h && h->timer && ms_sum && count, "timing_read: timing was not started");
    LayerTimer* t = h->timer;
    for (int i = 0; i < kNumMfmaConvs; ++i) { ms_sum[i] = 0.0; count[i] = 0; }
    for (int s = 0; s < t->used; ++s) {
        EXA_CHECK_HIP(hipEventSynchronize(t->stop[s]));
        float ms = 0.f;
        EXA_CHECK_HIP(hipEventElapsedTime(&ms, t->start[s], t->stop[s]));
        ms_sum[t->layer[s]] += ms;
        count[t->layer[s]]++;
    }
    t->mask = 0;
    t->used = 0;
    t->next = 0;
    return EXASPIM_OK;
}

extern "C" size_t exaspim_unet_workspace_bytes(const exaspim_unet* h, int32_t n, int32_t d,
                                               int32_t hgt, int32_t w) {
    if (!h || n <= 0 || !level_dims_ok(d, hgt, w)) {
        set_error("workspace_bytes: bad arguments (n %d, patch %dx%dx%d must be multiples of 16)",
                  n, d, hgt, w);
        return 0;
    }
    return make_workspace(h->plan, n, d, hgt, w).bytes;
}

extern "C" int exaspim_unet_forward(exaspim_unet* h, const float* x_dev, float* out_dev,
                                    int32_t n, int32_t d, int32_t hgt, int32_t w,
                                    int32_t apply_sigmoid, void* workspace_dev,
                                    size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(h && x_dev && out_dev && workspace_dev, "forward: NULL pointer");
    EXA_CHECK_ARG(n > 0, "forward: empty batch");
    // The reference's Up.forward pads only two axes by the wrong differences
    // (unet3d.py:281-287), so torch.cat raises for sizes that are not multiples
    // of 16; the same sizes are rejected here.
    EXA_CHECK_ARG(level_dims_ok(d, hgt, w),
                  "forward: patch %dx%dx%d: every dimension must be a positive multiple of 16",
                  d, hgt, w);
    return forward(h, x_dev, out_dev, n, d, hgt, w, apply_sigmoid, 0, workspace_dev, workspace_bytes,
                   (hipStream_t)stream);
}

extern "C" int exaspim_unet_input_layout(const exaspim_unet* h) {
    if (!h) return EXASPIM_E_INVALID;
    switch (h->plan.dtype) {
        case EXASPIM_DT_F32:
        case EXASPIM_DT_BF16X3: return EXASPIM_IN_PADDED_F32;
        case EXASPIM_DT_F16: return EXASPIM_IN_PADDED_SPLIT_F16;
        case EXASPIM_DT_BF16: return EXASPIM_IN_PADDED_SPLIT_BF16;
    }
    return EXASPIM_E_INVALID;
}

extern "C" int exaspim_unet_forward_prepared(exaspim_unet* h, const void* x_prepared_dev, float* out_dev,
                                             int32_t n, int32_t d, int32_t hgt, int32_t w,
                                             int32_t apply_sigmoid, int32_t trim,
                                             void* workspace_dev, size_t workspace_bytes,
                                             void* stream) {
    EXA_CHECK_ARG(h && x_prepared_dev && out_dev && workspace_dev, "forward: NULL pointer");
    EXA_CHECK_ARG(n > 0, "forward: empty batch");
    EXA_CHECK_ARG(trim >= 0, "forward: negative trim %d", trim);
    EXA_CHECK_ARG(level_dims_ok(d, hgt, w),
                  "forward: patch %dx%dx%d: every dimension must be a positive multiple of 16",
                  d, hgt, w);
    return forward(h, nullptr, out_dev, n, d, hgt, w, apply_sigmoid, trim, workspace_dev,
                   workspace_bytes, (hipStream_t)stream, x_prepared_dev);
}

extern "C" int exaspim_unet_forward_prepared_row(exaspim_unet* h, const void* x_prepared_dev, float* out_dev,
                                                 int32_t n, int32_t d, int32_t hgt, int32_t w,
                                                 int32_t apply_sigmoid, int32_t trim, int32_t row_stride,
                                                 void* workspace_dev, size_t workspace_bytes,
                                                 void* stream) {
    EXA_CHECK_ARG(h && x_prepared_dev && out_dev && workspace_dev, "forward: NULL pointer");
    EXA_CHECK_ARG(n > 0, "forward: empty batch");
    EXA_CHECK_ARG(trim >= 0, "forward: negative trim %d", trim);
    EXA_CHECK_ARG(row_stride >= 0, "forward: negative row stride %d", row_stride);
    EXA_CHECK_ARG(level_dims_ok(d, hgt, w),
                  "forward: patch %dx%dx%d: every dimension must be a positive multiple of 16",
                  d, hgt, w);
    return forward(h, nullptr, out_dev, n, d, hgt, w, apply_sigmoid, trim, workspace_dev,
                   workspace_bytes, (hipStream_t)stream, x_prepared_dev, nullptr, row_stride);
}

extern "C" int exaspim_unet_forward_prepared_clipped(exaspim_unet* h, const void* x_prepared_dev, float* out_dev,
                                                     int32_t n, int32_t d, int32_t hgt, int32_t w,
                                                     int32_t apply_sigmoid, int32_t trim, int32_t row_stride,
                                                     const int32_t keep_hi[3], void* workspace_dev,
                                                     size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(h && x_prepared_dev && out_dev && workspace_dev && keep_hi, "forward: NULL pointer");
    EXA_CHECK_ARG(n > 0, "forward: empty batch");
    EXA_CHECK_ARG(trim >= 0, "forward: negative trim %d", trim);
    EXA_CHECK_ARG(row_stride >= 0, "forward: negative row stride %d", row_stride);
    EXA_CHECK_ARG(level_dims_ok(d, hgt, w),
                  "forward: patch %dx%dx%d: every dimension must be a positive multiple of 16",
                  d, hgt, w);
    const int size[3] = {d, hgt, w};
    for (int i = 0; i < 3; ++i)
        EXA_CHECK_ARG(keep_hi[i] > trim && keep_hi[i] <= size[i] - trim,
                      "forward: keep_hi[%d] = %d outside (%d, %d] (trim %d of %d voxels)", i, keep_hi[i], trim,
                      size[i] - trim, trim, size[i]);
    return forward(h, nullptr, out_dev, n, d, hgt, w, apply_sigmoid, trim, workspace_dev,
                   workspace_bytes, (hipStream_t)stream, x_prepared_dev, nullptr, row_stride, keep_hi);
}

extern "C" int exaspim_unet_carry_planes(const exaspim_unet* h, int32_t n, int32_t d, int32_t hgt, int32_t w,
                                         int32_t row_stride, int32_t shift_z, int32_t out[2]) {
    EXA_CHECK_ARG(h && out, "carry_planes: NULL pointer");
    out[0] = out[1] = 0;
    EXA_CHECK_ARG(n > 0 && level_dims_ok(d, hgt, w) && row_stride >= 0 && shift_z > 0,
                  "carry_planes: bad arguments (n %d, patch %dx%dx%d, row stride %d, shift %d)", n, d, hgt, w,
                  row_stride, shift_z);
    // the conditions under which forward() runs inc.3 in row mode
    const UNetPlan& p = h->plan;
    const bool fused = !(h->options & EXASPIM_OPT_SEPARATE_POOL) && conv_can_fuse_pool(p.dtype, p.conv[0].cout, d, hgt, w);
    if ((h->options & EXASPIM_OPT_PER_PATCH_ENCODER) || !conv_row_mode_ok(p.dtype, p.conv[0].cout, n, w, row_stride, fused))
        return EXASPIM_OK;
    carry_span(d, shift_z, out);
    return EXASPIM_OK;
}

extern "C" int exaspim_unet_carry_rows(const exaspim_unet* h, int32_t n, int32_t d, int32_t hgt, int32_t w,
                                       int32_t row_stride, int32_t shift_y, int32_t out[2]) {
    EXA_CHECK_ARG(h && out, "carry_rows: NULL pointer");
    out[0] = out[1] = 0;
    EXA_CHECK_ARG(n > 0 && level_dims_ok(d, hgt, w) && row_stride >= 0 && shift_y > 0,
                  "carry_rows: bad arguments (n %d, patch %dx%dx%d, row stride %d, shift %d)", n, d, hgt, w,
                  row_stride, shift_y);
    // the conditions under which forward() runs inc.3 in row mode (exaspim_unet_carry_planes)
    const UNetPlan& p = h->plan;
    const bool fused = !(h->options & EXASPIM_OPT_SEPARATE_POOL) && conv_can_fuse_pool(p.dtype, p.conv[0].cout, d, hgt, w);
    if ((h->options & (EXASPIM_OPT_PER_PATCH_ENCODER | EXASPIM_OPT_CARRY_NO_ROWS)) ||
        !conv_row_mode_ok(p.dtype, p.conv[0].cout, n, w, row_stride, fused))
        return EXASPIM_OK;
    carry_row_span(hgt, shift_y, out);
    return EXASPIM_OK;
}

extern "C" int exaspim_unet_carry1_planes(const exaspim_unet* h, int32_t n, int32_t d, int32_t hgt, int32_t w,
                                          int32_t row_stride, int32_t shift_z, int32_t out[2]) {
    int32_t l0[2];
    EXA_CHECK_ARG(out, "carry_planes: NULL pointer");
    out[0] = out[1] = 0;
    // (the argument checks and the conditions of the first level's row mode)
    if (int rc = exaspim_unet_carry_planes(h, n, d, hgt, w, row_stride, shift_z, l0)) return rc;
    if (l0[0] < l0[1]) carry1_span(h, n, d, hgt, w, shift_z, out);
    return EXASPIM_OK;
}

extern "C" int exaspim_unet_forward_prepared_carry(exaspim_unet* h, const void* x_prepared_dev, float* out_dev,
                                                   int32_t n, int32_t d, int32_t hgt, int32_t w,
                                                   int32_t apply_sigmoid, int32_t trim, int32_t row_stride,
                                                   const int32_t keep_hi[3], const exaspim_unet_carry* carry,
                                                   void* workspace_dev, size_t workspace_bytes, void* stream) {
    return exaspim_unet_forward_prepared_carry1(h, x_prepared_dev, out_dev, n, d, hgt, w, apply_sigmoid, trim, row_stride,
                                                keep_hi, carry, nullptr, workspace_dev, workspace_bytes, stream);
}

extern "C" int exaspim_unet_forward_prepared_carry1(exaspim_unet* h, const void* x_prepared_dev, float* out_dev,
                                                    int32_t n, int32_t d, int32_t hgt, int32_t w,
                                                    int32_t apply_sigmoid, int32_t trim, int32_t row_stride,
                                                    const int32_t keep_hi[3], const exaspim_unet_carry* carry,
                                                    const exaspim_unet_carry1* carry1, void* workspace_dev,
                                                    size_t workspace_bytes, void* stream) {
    return exaspim_unet_forward_prepared_carry_y(h, x_prepared_dev, out_dev, n, d, hgt, w, apply_sigmoid, trim, row_stride,
                                                 keep_hi, carry, carry1, nullptr, workspace_dev, workspace_bytes, stream);
}

extern "C" int exaspim_unet_forward_prepared_carry_y(exaspim_unet* h, const void* x_prepared_dev, float* out_dev,
                                                     int32_t n, int32_t d, int32_t hgt, int32_t w,
                                                     int32_t apply_sigmoid, int32_t trim, int32_t row_stride,
                                                     const int32_t keep_hi[3], const exaspim_unet_carry* carry,
                                                     const exaspim_unet_carry1* carry1,
                                                     const exaspim_unet_carry_y* carry_y, void* workspace_dev,
                                                     size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(h && x_prepared_dev && out_dev && workspace_dev && keep_hi && carry, "forward: NULL pointer");
    EXA_CHECK_ARG(n > 0, "forward: empty batch");
    EXA_CHECK_ARG(trim >= 0, "forward: negative trim %d", trim);
    EXA_CHECK_ARG(row_stride >= 0, "forward: negative row stride %d", row_stride);
    EXA_CHECK_ARG(level_dims_ok(d, hgt, w),
                  "forward: patch %dx%dx%d: every dimension must be a positive multiple of 16",
                  d, hgt, w);
    const int size[3] = {d, hgt, w};
    for (int i = 0; i < 3; ++i)
        EXA_CHECK_ARG(keep_hi[i] > trim && keep_hi[i] <= size[i] - trim,
                      "forward: keep_hi[%d] = %d outside (%d, %d] (trim %d of %d voxels)", i, keep_hi[i], trim,
                      size[i] - trim, trim, size[i]);
    return forward(h, nullptr, out_dev, n, d, hgt, w, apply_sigmoid, trim, workspace_dev,
                   workspace_bytes, (hipStream_t)stream, x_prepared_dev, nullptr, row_stride, keep_hi, carry, carry1,
                   carry_y);
}

extern "C" int exaspim_unet_forward_trimmed(exaspim_unet* h, const float* x_dev, float* out_dev,
                                            int32_t n, int32_t d, int32_t hgt, int32_t w,
                                            int32_t apply_sigmoid, int32_t trim,
                                            void* workspace_dev, size_t workspace_bytes,
                                            void* stream) {
    EXA_CHECK_ARG(h && x_dev && out_dev && workspace_dev, "forward: NULL pointer");
    EXA_CHECK_ARG(n > 0, "forward: empty batch");
    EXA_CHECK_ARG(trim >= 0, "forward: negative trim %d", trim);
    EXA_CHECK_ARG(level_dims_ok(d, hgt, w),
                  "forward: patch %dx%dx%d: every dimension must be a positive multiple of 16",
                  d, hgt, w);
    return forward(h, x_dev, out_dev, n, d, hgt, w, apply_sigmoid, trim, workspace_dev,
                   workspace_bytes, (hipStream_t)stream);
}

extern "C" int exaspim_unet_forward_absmax(exaspim_unet* h, const float* x_dev, float* out_dev,
                                           int32_t n, int32_t d, int32_t hgt, int32_t w,
                                           int32_t apply_sigmoid, float* absmax_dev,
                                           void* workspace_dev, size_t workspace_bytes, void* stream) {
    EXA_CHECK_ARG(h && x_dev && out_dev && workspace_dev && absmax_dev, "forward_absmax: NULL pointer");
    EXA_CHECK_ARG(n > 0, "forward: empty batch");
    EXA_CHECK_ARG(level_dims_ok(d, hgt, w),
                  "forward: patch %dx%dx%d: every dimension must be a positive multiple of 16",
                  d, hgt, w);
    return forward(h, x_dev, out_dev, n, d, hgt, w, apply_sigmoid, 0, workspace_dev, workspace_bytes,
                   (hipStream_t)stream, nullptr, absmax_dev);
}

extern "C" int exaspim_unet_set_options(exaspim_unet* h, uint32_t options) {
    EXA_CHECK_ARG(h != nullptr, "set_options: NULL handle");
    EXA_CHECK_ARG((options & ~(uint32_t)(EXASPIM_OPT_SEPARATE_POOL | EXASPIM_OPT_SEPARATE_DEEP_POOLS | EXASPIM_OPT_PLAIN_UPSAMPLE | EXASPIM_OPT_FIRST_PER_GROUP |
                                          EXASPIM_OPT_UPSAMPLE_PER_THREAD | EXASPIM_OPT_PER_PATCH_ENCODER |
                                          EXASPIM_OPT_SEPARATE_HEAD | EXASPIM_OPT_ROW_SEPARATE_BORDERS |
                                          EXASPIM_OPT_CARRY_MAIN_ONLY | EXASPIM_OPT_CARRY_NO_ROWS)) == 0,
                  "set_options: unknown option bits 0x%x", options);
    h->options = options;
    return EXASPIM_OK;
}
