// Test-only C entry points over the internal layer launchers (common.h), so that the suite
// (tests/test_gpu_layers.py) can drive every dispatch path of one layer on its own and check it
// against a float64 reference. Linked from the product's objects into libexaspim_layer_probe.so;
// not part of include/exaspim_affinity.h or its ABI.

#include "common.h"

using namespace exaspim;

extern "C" {

const char* probe_last_error(void) { return get_error(); }

// __PRETTY_FUNCTION__ of the last convolution launcher this thread ran, and its split-K factor
const char* probe_last_config(void) { return last_conv_launch().config; }
int probe_last_ksplit(void) { return last_conv_launch().ksplit; }
void probe_reset_config(void) {
    last_conv_launch() = ConvLaunchRecord{};
    last_layer_kernel() = "";
}
// 1 if that launch was the row-mode kernel (conv3x3x3_zpipe_row), whose configuration string is the one
// of the per-patch fused-pool launch
int probe_last_row(void) { return last_conv_launch().row ? 1 : 0; }
// kernel variant of the last launch_conv_first / launch_upsample2
const char* probe_last_layer_kernel(void) { return last_layer_kernel(); }

// One convolution through launch_conv3x3x3 (thin = 0) or launch_conv3x3x3_thin (thin = 1).
// dtype: any EXASPIM_DT_* (EXASPIM_DT_BF16X3: float32 tensors, weights in its hi / lo fragments).
// region: org[3], ext[3] (z, y, x); head_* may be null / 0, pool_dst and partial may be null.
int probe_conv3x3x3(int thin, int dtype, const void* src_a, const void* src_b, int ca, int cb,
                    const void* weights, const float* bias, void* dst, int cout, int n, int d, int h,
                    int w, float slope, const int32_t* region, void* pool_dst, float* partial,
                    size_t partial_patch_bytes, const float* head_w, const float* head_b,
                    float* head_out, int head_oc, int head_sigmoid, hipStream_t stream) {
    ConvArgs a{};
    a.src_a = src_a;
    a.src_b = src_b;
    a.ca = ca;
    a.cb = cb;
    a.weights = weights;
    a.bias = bias;
    a.dst = dst;
    a.cout = cout;
    a.n = n;
    a.d = d;
    a.h = h;
    a.w = w;
    a.slope = slope;
    for (int i = 0; i < 3; ++i) {
        a.org[i] = region ? region[i] : 0;
        a.ext[i] = region ? region[3 + i] : 0;
    }
    a.pool_dst = pool_dst;
    a.partial = partial;
    a.partial_patch_bytes = partial_patch_bytes;
    a.head_w = head_w;
    a.head_b = head_b;
    a.head_out = head_out;
    a.head_oc = head_oc;
    a.head_sigmoid = head_sigmoid;
    return thin ? launch_conv3x3x3_thin(dtype, a, stream) : launch_conv3x3x3(dtype, a, stream);
}

// The bf16x3 convolution with its fused head (launch_conv3x3x3_x3_head); the argument list of
// probe_conv3x3x3, of which thin, dtype, pool_dst and partial must be 0 / EXASPIM_DT_BF16X3 / null.
int probe_conv3x3x3_x3_head(int thin, int dtype, const void* src_a, const void* src_b, int ca, int cb,
                            const void* weights, const float* bias, void* dst, int cout, int n, int d, int h,
                            int w, float slope, const int32_t* region, void* pool_dst, float* partial,
                            size_t partial_patch_bytes, const float* head_w, const float* head_b,
                            float* head_out, int head_oc, int head_sigmoid, hipStream_t stream) {
    EXA_CHECK_ARG(!thin && dtype == EXASPIM_DT_BF16X3 && !partial,
                  "probe: the bf16x3 head launcher has no thin tiles, no other dtype and no split-K");
    ConvArgs a{};
    a.src_a = src_a;
    a.src_b = src_b;
    a.ca = ca;
    a.cb = cb;
    a.weights = weights;
    a.bias = bias;
    a.dst = dst;
    a.cout = cout;
    a.n = n;
    a.d = d;
    a.h = h;
    a.w = w;
    a.slope = slope;
    for (int i = 0; i < 3; ++i) {
        a.org[i] = region ? region[i] : 0;
        a.ext[i] = region ? region[3 + i] : 0;
    }
    a.pool_dst = pool_dst;
    a.head_w = head_w;
    a.head_b = head_b;
    a.head_out = head_out;
    a.head_oc = head_oc;
    a.head_sigmoid = head_sigmoid;
    return launch_conv3x3x3_x3_head(a, stream);
}

// The engine's row-mode sequence (launch_conv3x3x3_row) on one source: stages is a mask of 1 = the row
// launch, 2 = the two thin-tile launches, 4 = the column max-pool. After stage 1 alone the launch record
// is the row launch's.
int probe_conv3x3x3_row(int dtype, const void* src, int ca, const void* weights, const float* bias, void* dst,
                        int cout, int n, int d, int h, int w, float slope, int row_stride, void* pool_dst,
                        int stages, hipStream_t stream) {
    ConvArgs a{};
    a.src_a = src;
    a.ca = ca;
    a.weights = weights;
    a.bias = bias;
    a.dst = dst;
    a.cout = cout;
    a.n = n;
    a.d = d;
    a.h = h;
    a.w = w;
    a.slope = slope;
    a.row_stride = row_stride;
    a.pool_dst = pool_dst;
    return launch_conv3x3x3_row(dtype, a, stages, stream);
}

// probe_conv3x3x3_row with planes carried along z (ConvArgs::in_z0 .. out_shift); carry[0..4] = in_z0, in_z1,
// out_z0, out_z1, out_shift. 1 from probe_last_carry if the last launch ran conv3x3x3_zpipe_rowz or (stage 16)
// conv3x3x3_t14_borders_carry.
int probe_conv3x3x3_row_carry(int dtype, const void* src, int ca, const void* weights, const float* bias, void* dst,
                              int cout, int n, int d, int h, int w, float slope, int row_stride, void* pool_dst,
                              const int32_t* carry, void* carry_dst, void* carry_pool_dst, int stages,
                              hipStream_t stream) {
    EXA_CHECK_ARG(carry != nullptr, "probe: NULL carry");
    for (int i = 0; i < 5; ++i)   // (what ConvArgs' narrow fields hold)
        EXA_CHECK_ARG(carry[i] >= 0 && carry[i] <= (i == 2 || i == 3 ? 254 : 65534), "probe: carry[%d] = %d out of range", i, carry[i]);
    ConvArgs a{};
    a.src_a = src;
    a.ca = ca;
    a.weights = weights;
    a.bias = bias;
    a.dst = dst;
    a.cout = cout;
    a.n = n;
    a.d = d;
    a.h = h;
    a.w = w;
    a.slope = slope;
    a.row_stride = row_stride;
    a.pool_dst = pool_dst;
    a.in_z0 = (unsigned short)carry[0];
    a.in_z1 = (unsigned short)carry[1];
    a.out_z0 = (unsigned char)carry[2];
    a.out_z1 = (unsigned char)carry[3];
    a.out_shift = (unsigned short)carry[4];
    a.carry_dst = carry_dst;
    a.carry_pool_dst = carry_pool_dst;
    return launch_conv3x3x3_row(dtype, a, stages, stream);
}
int probe_last_carry(void) { return last_conv_launch().carry ? 1 : 0; }

// ... and rows carried along y (ConvCarryY): carry_y[0..4] = in_y0, in_y1, out_y0, out_y1, out_shift_y; targets[0..3]
// = y_dst, y_pool_dst, d_dst, d_pool_dst (each may be null). 1 from probe_last_carry_y if the last launch ran
// conv3x3x3_zpipe_rowzy.
int probe_conv3x3x3_row_carry_y(int dtype, const void* src, int ca, const void* weights, const float* bias, void* dst,
                                int cout, int n, int d, int h, int w, float slope, int row_stride, void* pool_dst,
                                const int32_t* carry, void* carry_dst, void* carry_pool_dst, const int32_t* carry_y,
                                void* const* targets, int stages, hipStream_t stream) {
    EXA_CHECK_ARG(carry != nullptr && carry_y != nullptr && targets != nullptr, "probe: NULL carry");
    for (int i = 0; i < 5; ++i) {   // (what the narrow fields hold)
        EXA_CHECK_ARG(carry[i] >= 0 && carry[i] <= (i == 2 || i == 3 ? 254 : 65534), "probe: carry[%d] = %d out of range", i, carry[i]);
        EXA_CHECK_ARG(carry_y[i] >= 0 && carry_y[i] <= 65534, "probe: carry_y[%d] = %d out of range", i, carry_y[i]);
    }
    ConvArgs a{};
    a.src_a = src;
    a.ca = ca;
    a.weights = weights;
    a.bias = bias;
    a.dst = dst;
    a.cout = cout;
    a.n = n;
    a.d = d;
    a.h = h;
    a.w = w;
    a.slope = slope;
    a.row_stride = row_stride;
    a.pool_dst = pool_dst;
    a.in_z0 = (unsigned short)carry[0];
    a.in_z1 = (unsigned short)carry[1];
    a.out_z0 = (unsigned char)carry[2];
    a.out_z1 = (unsigned char)carry[3];
    a.out_shift = (unsigned short)carry[4];
    a.carry_dst = carry_dst;
    a.carry_pool_dst = carry_pool_dst;
    ConvCarryY y;
    y.in_y0 = (unsigned short)carry_y[0];
    y.in_y1 = (unsigned short)carry_y[1];
    y.out_y0 = (unsigned short)carry_y[2];
    y.out_y1 = (unsigned short)carry_y[3];
    y.out_shift_y = (unsigned short)carry_y[4];
    y.y_dst = targets[0];
    y.y_pool_dst = targets[1];
    y.d_dst = targets[2];
    y.d_pool_dst = targets[3];
    return launch_conv3x3x3_row(dtype, a, stages, stream, &y);
}
int probe_last_carry_y(void) { return last_conv_launch().carry_y ? 1 : 0; }

// One whole-patch convolution through launch_conv3x3x3 with planes carried along z outside row mode
// (conv3x3x3_t14_carry); carry[0..4] as above, partial may be null (with scratch the launcher may split).
int probe_conv3x3x3_carry(int dtype, const void* src, int ca, const void* weights, const float* bias, void* dst,
                          int cout, int n, int d, int h, int w, float slope, void* pool_dst, float* partial,
                          size_t partial_patch_bytes, const int32_t* carry, void* carry_dst, void* carry_pool_dst,
                          hipStream_t stream) {
    EXA_CHECK_ARG(carry != nullptr, "probe: NULL carry");
    for (int i = 0; i < 5; ++i)   // (what ConvArgs' narrow fields hold)
        EXA_CHECK_ARG(carry[i] >= 0 && carry[i] <= (i == 2 || i == 3 ? 254 : 65534), "probe: carry[%d] = %d out of range", i, carry[i]);
    ConvArgs a{};
    a.src_a = src;
    a.ca = ca;
    a.weights = weights;
    a.bias = bias;
    a.dst = dst;
    a.cout = cout;
    a.n = n;
    a.d = d;
    a.h = h;
    a.w = w;
    a.slope = slope;
    a.pool_dst = pool_dst;
    a.partial = partial;
    a.partial_patch_bytes = partial_patch_bytes;
    a.in_z0 = (unsigned short)carry[0];
    a.in_z1 = (unsigned short)carry[1];
    a.out_z0 = (unsigned char)carry[2];
    a.out_z1 = (unsigned char)carry[3];
    a.out_shift = (unsigned short)carry[4];
    a.carry_dst = carry_dst;
    a.carry_pool_dst = carry_pool_dst;
    return launch_conv3x3x3(dtype, a, stream);
}
void probe_carry1_span(int tz, int d, int shift_z, int32_t* out) { carry1_span_of_tiles(tz, d, shift_z, out); }
// conv_carry_t14_tile_depth for a whole-patch launch of this shape
int probe_conv_carry_tile_depth(int dtype, int ca, int cout, int n, int d, int h, int w, size_t partial_patch_bytes) {
    ConvArgs a{};
    a.ca = ca;
    a.cout = cout;
    a.n = n;
    a.d = d;
    a.h = h;
    a.w = w;
    static float scratch;   // (only its presence is read)
    a.partial = partial_patch_bytes ? &scratch : nullptr;
    a.partial_patch_bytes = partial_patch_bytes;
    return conv_carry_t14_tile_depth(dtype, a);
}

int probe_conv_row_mode_ok(int dtype, int cout, int n, int w, int row_stride, int fused_pool_whole_patch) {
    return conv_row_mode_ok(dtype, cout, n, w, row_stride, fused_pool_whole_patch != 0) ? 1 : 0;
}

int probe_conv_first(int dtype, const float* x, float* xpad, const float* w, const float* bias,
                     void* dst, int n, int d, int h, int wd, int c0p, float slope, int per_group,
                     hipStream_t stream) {
    return launch_conv_first(dtype, x, xpad, w, bias, dst, n, d, h, wd, c0p, slope, stream, per_group != 0);
}

// launch_conv_first with output planes [skip_z0, skip_z1) nobody reads
int probe_conv_first_planes(int dtype, const float* x, float* xpad, const float* w, const float* bias,
                            void* dst, int n, int d, int h, int wd, int c0p, float slope, int per_group,
                            int skip_z0, int skip_z1, hipStream_t stream) {
    return launch_conv_first(dtype, x, xpad, w, bias, dst, n, d, h, wd, c0p, slope, stream, per_group != 0, skip_z0,
                             skip_z1);
}
// the planes inc.0 skips when inc.3 takes [in_z0, in_z1) over
void probe_conv_first_skip_planes(int d, int in_z0, int in_z1, int32_t* out) { conv_first_skip_planes(d, in_z0, in_z1, out); }
// the tile depths of inc.3's two launches at depth d: out[0] the main launch's, out[1] the border launch's
void probe_row_tile_depths(int d, int32_t* out) {
    out[0] = conv_zcol_tile_depth(d);
    out[1] = conv_row_borders_tile_depth(d);
}

int probe_maxpool2(int dtype, const void* src, void* dst, int n, int d, int h, int w, int c,
                   hipStream_t stream) {
    return launch_maxpool2(dtype, src, dst, n, d, h, w, c, stream);
}

int probe_maxpool2_xcols(int dtype, const void* src, void* dst, int n, int d, int h, int w, int c, int ox0,
                         int ox1, hipStream_t stream) {
    return launch_maxpool2_xcols(dtype, src, dst, n, d, h, w, c, ox0, ox1, stream);
}

int probe_upsample2(int dtype, const void* src, void* dst, int n, int d, int h, int w, int c,
                    int margin, int plain_kernel, int per_thread, hipStream_t stream) {
    return launch_upsample2(dtype, src, dst, n, d, h, w, c, margin, stream, plain_kernel != 0,
                            per_thread != 0);
}

// ... with a per-axis margin at the high faces (margin_hi[3] as engine.hip derives it from keep_hi)
int probe_upsample2_hi(int dtype, const void* src, void* dst, int n, int d, int h, int w, int c,
                       int margin, const int margin_hi[3], int plain_kernel, int per_thread,
                       hipStream_t stream) {
    return launch_upsample2(dtype, src, dst, n, d, h, w, c, margin, stream, plain_kernel != 0,
                            per_thread != 0, margin_hi);
}

int probe_convt2(int dtype, const void* src, const void* weights, const float* bias, void* dst, int n,
                 int d, int h, int w, int cin, int cout, hipStream_t stream) {
    return launch_convt2(dtype, src, weights, bias, dst, n, d, h, w, cin, cout, stream);
}

int probe_head(int dtype, const void* src, const float* w, const float* bias, float* out, int n,
               int d, int h, int wd, int c0p, int out_channels, int apply_sigmoid, hipStream_t stream) {
    return launch_head(dtype, src, w, bias, out, n, d, h, wd, c0p, out_channels, apply_sigmoid, stream);
}

// The plan's view of MFMA convolution `layer` (0 = inc.3 .. 16 = up4.3): out[0..7] =
// ca_real, cb_real, ca, cb, cout_real, cout, w_off, b_off (byte offsets into the packed image
// of exaspim_unet_pack_weights with the same channels / out_channels / dtype).
int probe_plan_conv(const int32_t channels[5], int32_t out_channels, int32_t dtype, int layer,
                    int64_t out[8]) {
    UNetPlan p;
    if (!make_plan(channels, out_channels, dtype, &p)) return EXASPIM_E_INVALID;
    EXA_CHECK_ARG(layer >= 0 && layer < kNumMfmaConvs, "probe: layer %d out of range", layer);
    const ConvLayer& L = p.conv[layer];
    const int64_t v[8] = {L.ca_real, L.cb_real, L.ca, L.cb, L.cout_real, L.cout, (int64_t)L.w_off,
                          (int64_t)L.b_off};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return EXASPIM_OK;
}

// One pass of exaspim_dbf on its own (launch_dbf_pass), for tools/dbf_rate.py to time the passes apart.
int probe_dbf_pass(int axis, const int32_t* labels, const int32_t* in, int32_t* out, const int32_t dims[3],
                   int black_border, hipStream_t stream) {
    EXA_CHECK_ARG(labels && out && dims && (axis == 2 || (in && in != out)), "probe_dbf_pass: NULL or aliased buffer");
    return launch_dbf_pass(axis, labels, in, out, dims, black_border, stream);
}

// The passes first .. last of exaspim_fill_holes on their own (launch_fill_holes_passes), for
// tools/holes_rate.py to time them apart. The workspace is one of exaspim_fill_holes_workspace_bytes(dims).
int probe_fill_holes_passes(const int32_t* labels, const int32_t dims[3], int32_t* out, int64_t* counts,
                            void* workspace, int first, int last, hipStream_t stream) {
    EXA_CHECK_ARG(labels && dims && out && counts && workspace, "probe_fill_holes_passes: NULL buffer");
    EXA_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)counts & 7) == 0,
                  "probe_fill_holes_passes: misaligned buffer");
    return launch_fill_holes_passes(labels, dims, out, counts, workspace, first, last, stream);
}

}  // extern "C"
