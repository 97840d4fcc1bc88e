/*
 * exaspim_affinity.h -- C ABI of the MI355X (gfx950) sliding-window 3D-UNet
 * affinity-inference path.
 *
 * The reference (AllenNeuralDynamics/aind-exaspim-neuron-segmentation) has no
 * FFI on this path: it is plain Python over torch. The entry points below are
 * what a binding for that path needs; each one names the reference code it
 * replaces (paths relative to src/aind_exaspim_neuron_segmentation/). The
 * reference-side ctypes stub a maintainer would add is in INTEGRATION.md.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch types.
 *  - Every function that can fail returns int: 0 = ok, negative = error
 *    (EXASPIM_E_*); exaspim_last_error() returns a thread-local message.
 *  - "dev" pointers are HIP device pointers owned by the caller (e.g.
 *    torch.Tensor.data_ptr()); the library never allocates or frees device
 *    memory and never synchronises the device. Kernels are enqueued on the
 *    caller's HIP stream ("stream", a hipStream_t passed as void*; NULL = the
 *    default stream).
 *  - Volumes are C-ordered (z, y, x). Activations handed across the ABI are
 *    NCDHW float32, like the reference's tensors; the blocked channels-last
 *    layout used between kernels (one plane of 32-byte voxel records per
 *    32-byte channel chunk) is internal to the workspace.
 */
#ifndef EXASPIM_AFFINITY_H
#define EXASPIM_AFFINITY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: exaspim_export_f16 added (entry points are only ever added within a major line);
 * 4: exaspim_unet_forward_prepared, exaspim_unet_input_layout, exaspim_gather_patches_as
 *    (EXASPIM_IN_*): batches written in the first convolution's operand layout;
 * 5: exaspim_unet_forward_absmax, exaspim_histogram_wide (EXASPIM_VOX_F64),
 *    exaspim_unet_set_options (replaces an environment switch);
 *    later within 5: exaspim_unet_forward_prepared_row, EXASPIM_OPT_PER_PATCH_ENCODER;
 *    later within 5: EXASPIM_DT_BF16X3 (a value every "dtype" argument accepts; no new entry point);
 *    later within 5: exaspim_synth_volume_neurite_u16;
 *    later within 5: exaspim_components, exaspim_components_workspace_bytes (EXASPIM_AFF_*)
 *    later within 5: exaspim_unet_forward_prepared_clipped, EXASPIM_OPT_ROW_SEPARATE_BORDERS;
 *    later within 5: exaspim_components_stream_slab / _finish / _apply and their workspace queries
 *    (struct exaspim_components_stream): the components of a volume that arrives in z slabs;
 *    later within 5: exaspim_region_graph (and its workspace query), exaspim_agglomerate,
 *    exaspim_apply_label_table: mean-affinity agglomeration of components;
 *    later within 5: exaspim_unet_carry_planes, exaspim_unet_forward_prepared_carry (struct
 *    exaspim_unet_carry): first-level planes carried from one z slab of patches to the next;
 *    later within 5: exaspim_region_graph_stream_slab / _finish and the finish workspace query (struct
 *    exaspim_region_graph_stream): the region graph of a volume that arrives in z slabs;
 *    later within 5: exaspim_unet_carry1_planes, exaspim_unet_forward_prepared_carry1 (struct
 *    exaspim_unet_carry1): second-level planes carried along z as well;
 *    later within 5: exaspim_watershed_fragments, exaspim_watershed_workspace_bytes: steepest-ascent
 *    watershed fragments for the agglomeration;
 *    later within 5: exaspim_region_graph_premerge (and its workspace query): tiny fragments merged on
 *    the device before the host agglomeration;
 *    later within 5: EXASPIM_OPT_CARRY_MAIN_ONLY (no new entry point);
 *    later within 5: exaspim_dbf, exaspim_segment_table (and their workspace queries, EXASPIM_DBF_INF):
 *    the distance-to-boundary field and the per-label table a skeletoniser starts from;
 *    later within 5: exaspim_region_graph_contract_dominant (and its workspace query): the exact
 *    contraction of dominant edges on the device before the host agglomeration;
 *    later within 5: exaspim_unet_carry_rows, exaspim_unet_forward_prepared_carry_y (struct
 *    exaspim_unet_carry_y), EXASPIM_OPT_CARRY_NO_ROWS: first-level rows carried along y as well;
 *    later within 5: exaspim_fill_holes (and its workspace query): the enclosed cavities of every label
 *    closed on the device before the distance-to-boundary field is taken;
 *    later within 5: exaspim_geodesic_begin, exaspim_geodesic_sweeps, exaspim_geodesic_farthest (and their
 *    workspace queries): the geodesic distance-from-source field of every label and its farthest voxels;
 *    later within 5: exaspim_geodesic_parents_begin, exaspim_geodesic_parents_sweeps,
 *    exaspim_geodesic_parents_finish, exaspim_trace_paths: the parental field of that field and the paths
 *    read off it;
 *    later within 5: exaspim_geodesic_reseed, exaspim_geodesic_parents_begin_seeds: fields and hops seeded from
 *    a list, any number of seeds per label, and a converged field re-seeded in place (TEASAR's fix_branching);
 *    later within 5: exaspim_teasar_begin, exaspim_teasar_round, exaspim_teasar_apply (and their workspace
 *    query): TEASAR's loop of targets, branches and invalidation for every label at once;
 *    later within 5: exaspim_watershed_stream_slab and its workspace query (struct
 *    exaspim_watershed_stream): watershed fragments of a volume that arrives in z slabs;
 *    later within 5: exaspim_label_overlaps, exaspim_label_overlaps_reset / _add / _finish (and their
 *    workspace query): the overlap table of two label volumes, whole or piece by piece */
#define EXASPIM_ABI_VERSION 5

/* error codes */
#define EXASPIM_OK 0
#define EXASPIM_E_INVALID (-1)   /* bad argument (shape, dtype, NULL)        */
#define EXASPIM_E_HIP (-2)       /* HIP runtime error (message has details)  */
#define EXASPIM_E_WORKSPACE (-3) /* workspace too small                      */
#define EXASPIM_E_NODEVICE (-4)  /* no usable gfx950 device                  */

/* compute dtype of the network (activations and weights between kernels;
 * accumulation is always float32) */
#define EXASPIM_DT_F32 0  /* exact f32 MFMA (v_mfma_f32_32x32x2_f32)        */
#define EXASPIM_DT_BF16 1 /* bf16 storage, v_mfma_f32_32x32x16_bf16         */
#define EXASPIM_DT_F16 2  /* f16 storage,  v_mfma_f32_32x32x16_f16          */
/* float32-grade convolutions on the bf16 matrix pipe. Activations stay float32 in memory
 * (the blocked float32 layout; inc.0, max-pool, upsampling, ConvTranspose3d, the head and
 * exaspim_unet_forward_absmax run the float32 kernels, the prepared input is
 * EXASPIM_IN_PADDED_F32). Each of the 17 3x3x3 MFMA convolutions splits both operands,
 *     hi = bf16(v) (round to nearest even),  lo = bf16(v - float(hi))
 * -- the activations while they are staged, the folded float32 weights on the host (the
 * convention of EXASPIM_IN_PADDED_SPLIT_BF16) -- and forms, per tap and 16 input channels,
 * three v_mfma_f32_32x32x16_bf16 products into one float32 accumulator, in this order:
 *     w_hi * x_hi,  w_hi * x_lo,  w_lo * x_hi        (w_lo * x_lo is dropped).
 * That keeps float32's exponent range and about 16 mantissa bits per operand (a relative
 * error of about 3 * 2^-18 per product). A value whose bf16 rounding is not finite (an
 * infinity, or beyond 3.39e38) gets a NaN low part. The folded bias, the head and inc.0
 * stay float32. The packed image holds, per (16-channel chunk, tap, 32-cout tile), a hi
 * fragment and then a lo fragment (1 KiB each, lane l: cout l % 32, channels 8 * (l / 32) ..
 * + 7 of the chunk), i.e. 4 bytes per padded weight.
 * The last convolution runs the head on its float32 accumulators, which in this mode ARE the
 * stored activations: same bits as the head launched on its own (EXASPIM_OPT_SEPARATE_HEAD).
 * exaspim_unet_forward_trimmed / _prepared with trim > 0 keep their contract in this mode too:
 * margin voxels of out_dev are left untouched and kept voxels have the bits of
 * exaspim_unet_forward (shapes whose head cannot be fused run the full pass, as in every mode). */
#define EXASPIM_DT_BF16X3 3
/* OR-ed into "dtype" wherever a network is described: the Up blocks use
 * ConvTranspose3d(k=2, s=2) instead of trilinear upsampling, i.e. the
 * reference's UNet3D(trilinear=False) (unet3d.py:254-258; 136 state_dict
 * tensors, "upN.up.weight (Cin, Cin/2, 2, 2, 2)" and "upN.up.bias" precede each
 * block's DoubleConv in the canonical parameter order). */
#define EXASPIM_UP_CONVT 0x100

/* voxel dtype of an input volume */
#define EXASPIM_VOX_U8 0
#define EXASPIM_VOX_U16 1
#define EXASPIM_VOX_I16 2
#define EXASPIM_VOX_F32 3
#define EXASPIM_VOX_F64 4 /* float64, and wider integers converted on the host: what float32 cannot carry */

typedef struct exaspim_unet exaspim_unet; /* opaque engine handle */

/* 3-D block of a (possibly larger, possibly sharded) volume. "dims" is the
 * shape of the local array, "origin" the global coordinate of its first
 * voxel, "global" the shape of the whole volume. Single-device callers pass
 * origin = 0 and global = dims. */
typedef struct exaspim_block {
    int32_t dims[3];
    int32_t origin[3];
    int32_t global[3];
} exaspim_block;

/* sliding-window geometry: predict()'s patch_shape / overlap / trim
 * (inference.py:36-38) */
typedef struct exaspim_window {
    int32_t patch[3];
    int32_t overlap[3];
    int32_t trim;
} exaspim_window;

int exaspim_abi_version(void);
const char* exaspim_last_error(void);

/* ---- model: replaces load_model() / UNet3D (inference.py:400-424,
 *      machine_learning/unet3d.py:16-336). Every "dtype" argument is one of
 *      EXASPIM_DT_*, optionally OR-ed with EXASPIM_UP_CONVT to select the
 *      UNet3D(trilinear=False) variant whose Up blocks use
 *      ConvTranspose3d(k=2, s=2) (unet3d.py:254-258) ---------------------- */

/* Number of float32 values in the canonical parameter vector for a UNet3D
 * with level widths channels[0..4] (unet3d.py:56) and "out_channels" head
 * outputs: the state_dict tensors in state_dict order, "num_batches_tracked"
 * skipped, i.e. per conv: weight(Cout,Cin,3,3,3), bias, bn.weight, bn.bias,
 * bn.running_mean, bn.running_var; with EXASPIM_UP_CONVT each Up block is
 * preceded by up.weight(Cin,Cin/2,2,2,2), up.bias; finally outc.conv.weight,
 * outc.conv.bias. Only the EXASPIM_UP_CONVT bit of "dtype" matters here. */
size_t exaspim_unet_param_count(const int32_t channels[5], int32_t out_channels,
                                int32_t dtype);

/* Size of the packed device image of the weights for a compute dtype. */
size_t exaspim_unet_packed_bytes(const int32_t channels[5], int32_t out_channels,
                                 int32_t dtype);

/* Host-only: folds eval-mode BatchNorm (eps 1e-5, unet3d.py:144,147) into the
 * preceding convolution (in float64), converts to "dtype" and lays the result
 * out in MFMA fragment order. "packed_host" receives packed_bytes bytes which
 * the caller uploads to the device unchanged. */
int exaspim_unet_pack_weights(const int32_t channels[5], int32_t out_channels,
                              int32_t dtype, const float* params, size_t n_params,
                              void* packed_host, size_t packed_bytes);

/* Binds a packed weight image that already lives on device "device". The
 * image must outlive the handle. */
int exaspim_unet_create(const int32_t channels[5], int32_t out_channels,
                        int32_t dtype, int32_t device, const void* packed_dev,
                        size_t packed_bytes, exaspim_unet** out);
void exaspim_unet_destroy(exaspim_unet* h);

/* Scratch bytes exaspim_unet_forward needs for a batch of n patches of
 * d x h x w voxels (each a multiple of 16, the constraint the reference's
 * Up.forward imposes, unet3d.py:281-288). */
size_t exaspim_unet_workspace_bytes(const exaspim_unet* h, int32_t n, int32_t d,
                                    int32_t hgt, int32_t w);

/* UNet3D.forward (unet3d.py:77-105): x_dev is float32 (n,1,d,h,w); out_dev
 * receives float32 (n,out_channels,d,h,w) logits, or sigmoid(logits) when
 * apply_sigmoid != 0 (inference.py:158). What workspace_dev holds on entry is undefined
 * (it is never cleared and the result does not depend on it), and nothing outside its first
 * workspace_bytes bytes is touched; the same holds for every exaspim_unet_forward_* below. */
int exaspim_unet_forward(exaspim_unet* h, const float* x_dev, float* out_dev,
                         int32_t n, int32_t d, int32_t hgt, int32_t w,
                         int32_t apply_sigmoid, void* workspace_dev,
                         size_t workspace_bytes, void* stream);

/* The same forward pass for a caller that discards the outputs within "trim"
 * voxels of every patch face, as _predict_batch does (inference.py:161-162:
 * outputs[..., trim:-trim, trim:-trim, trim:-trim]). Those voxels of out_dev are
 * left untouched, and the last two convolutions skip the work that only they
 * would have needed; every other voxel is bit-identical to exaspim_unet_forward.
 * trim = 0, or a trim that would leave nothing, is the full forward pass. */
int exaspim_unet_forward_trimmed(exaspim_unet* h, const float* x_dev, float* out_dev,
                                 int32_t n, int32_t d, int32_t hgt, int32_t w,
                                 int32_t apply_sigmoid, int32_t trim, void* workspace_dev,
                                 size_t workspace_bytes, void* stream);

/* The same forward pass from a batch that exaspim_gather_patches_as has already written in
 * the first convolution's operand layout (exaspim_unet_input_layout: EXASPIM_IN_PADDED_F32
 * for a float32 or bf16x3 engine, EXASPIM_IN_PADDED_SPLIT_F16 / _BF16 for the 16-bit ones):
 * x_prepared_dev is (n, d + 2, hgt + 2, w + 2) 4-byte words. _get_batch_inputs feeding
 * model(inputs) (inference.py:155-157) without the float32 patch tensor in between: one
 * launch and an 8-byte-per-voxel round trip less per batch; out_dev gets the same bits. */
int exaspim_unet_input_layout(const exaspim_unet* h);
int exaspim_unet_forward_prepared(exaspim_unet* h, const void* x_prepared_dev, float* out_dev,
                                  int32_t n, int32_t d, int32_t hgt, int32_t w,
                                  int32_t apply_sigmoid, int32_t trim, void* workspace_dev,
                                  size_t workspace_bytes, void* stream);
/* The same, for a batch whose n patches are one row along x: the same (z, y) start, each x start
 * row_stride after the previous one. Columns that neighbours share are computed once by the first
 * level's convolutions (when the engine can: 16-bit modes, an overlap w - row_stride that is a
 * multiple of 32 and at most the stride); out_dev gets the same bits. row_stride = 0: no row. */
int exaspim_unet_forward_prepared_row(exaspim_unet* h, const void* x_prepared_dev, float* out_dev,
                                      int32_t n, int32_t d, int32_t hgt, int32_t w,
                                      int32_t apply_sigmoid, int32_t trim, int32_t row_stride,
                                      void* workspace_dev, size_t workspace_bytes, void* stream);
/* The same, for a batch whose patches reach beyond the volume's high faces: of the trimmed outputs
 * the caller keeps local [trim, keep_hi[axis]) per axis (z, y, x) only, as the stitch does with
 * e = min(s + out, dim) (inference.py:101-116). trim < keep_hi[axis] <= size - trim, anything else is
 * EXASPIM_E_INVALID; keep_hi = size - trim is exaspim_unet_forward_prepared_row. The level-0 decoder skips
 * the work only the dropped voxels would have needed: they are left untouched in out_dev like the
 * trimmed margin, every kept voxel has the same bits. Plans that do not trim (trim = 0 or too large,
 * EXASPIM_OPT_SEPARATE_HEAD, shapes whose head cannot be fused) ignore keep_hi. row_stride = 0: no row. */
int exaspim_unet_forward_prepared_clipped(exaspim_unet* h, const void* x_prepared_dev, float* out_dev,
                                          int32_t n, int32_t d, int32_t hgt, int32_t w,
                                          int32_t apply_sigmoid, int32_t trim, int32_t row_stride,
                                          const int32_t keep_hi[3], void* workspace_dev,
                                          size_t workspace_bytes, void* stream);

/* Planes of the first level carried along z. A row batch whose patches start shift_z planes below an
 * earlier row batch (same x and y starts, same n and row_stride) computes, away from its own zero
 * padding, the bits that batch computed for x1 (inc.3's output) and its max-pool: its planes
 * [2, d - shift_z - 2) are the earlier batch's [2 + shift_z, d - 2).
 * exaspim_unet_carry_planes: out[0..1] = the plane range [z0, z1) of the LATER batch's frame that a forward
 * at this geometry can take over: the whole tiles of the depth inc.3's launcher picks inside that span,
 * even bounds. Empty (z0 = z1 = 0) when the engine has no row mode here (dtype, geometry, options, no
 * fused max-pool) or nothing fits. EXASPIM_E_INVALID for bad arguments. For d = 96, shift_z = 64: [6, 30). */
int exaspim_unet_carry_planes(const exaspim_unet* h, int32_t n, int32_t d, int32_t hgt, int32_t w,
                              int32_t row_stride, int32_t shift_z, int32_t out[2]);
/* own_skip / own_pool: where x1 (n, c0p, d, hgt, w) and its max-pool (n, c0p, d/2, hgt/2, w/2) live for
 * this forward, in the workspace's channels-last chunk layout and storage type, instead of inside the
 * workspace. Both required; sizes n * d * hgt * w * c0p * (2 bytes) and an eighth of it, 256-byte aligned.
 * in_z: the plane range already present in both (an earlier forward's carry out); {0, 0}: none.
 * out_skip / out_pool (both or neither), out_z, out_shift: planes out_z of this forward's x1 are stored to
 * out_skip too, at plane - out_shift, and their pooled planes to out_pool at pooled plane - out_shift / 2:
 * the own_skip / own_pool of the batch out_shift planes further down, with in_z = out_z - out_shift. */
typedef struct exaspim_unet_carry {
    void* own_skip;
    void* own_pool;
    int32_t in_z[2];
    void* out_skip;
    void* out_pool;
    int32_t out_z[2];
    int32_t out_shift;
    int32_t reserved;   /* 0 */
} exaspim_unet_carry;
/* exaspim_unet_forward_prepared_clipped with the first level's skip tensor and its max-pool in caller
 * buffers and planes carried in and / or out; out_dev gets the same bits. A request the engine cannot
 * honour (no row mode at this geometry, a range that exaspim_unet_carry_planes would not give, a missing
 * buffer) is EXASPIM_E_INVALID before anything is launched: a silent fall-back would leave the successor
 * reading planes nobody wrote. */
int exaspim_unet_forward_prepared_carry(exaspim_unet* h, const void* x_prepared_dev, float* out_dev,
                                        int32_t n, int32_t d, int32_t hgt, int32_t w,
                                        int32_t apply_sigmoid, int32_t trim, int32_t row_stride,
                                        const int32_t keep_hi[3], const exaspim_unet_carry* carry,
                                        void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same for the second level (down1.0 and down1.3, at half resolution): the later batch's down1.3 planes
 * [3, d/2 - shift_z/2 - 3) are the earlier batch's [3 + shift_z/2, d/2 - 3), its down1.0 planes one more on
 * either side. exaspim_unet_carry1_planes: out[0..1] = the plane range [z0, z1), in level-1 planes of the LATER
 * batch's frame, that a forward can take over for both layers: the whole tiles, of the depth the launcher
 * picks for them, inside that span. Empty when exaspim_unet_carry_planes is empty, when shift_z is odd, when
 * the two layers do not run the tile configuration that can carry (16-bit, 64-cout slices on rows that are a
 * multiple of 16 wide, not split, fused max-pool) or nothing fits. For d = 96, shift_z = 64: [4, 12). */
int exaspim_unet_carry1_planes(const exaspim_unet* h, int32_t n, int32_t d, int32_t hgt, int32_t w,
                               int32_t row_stride, int32_t shift_z, int32_t out[2]);
/* own_mid1: down1.0's output (n, c1p, d/2, hgt/2, w/2), own_skip1: down1.3's output x2 (same shape), own_pool2:
 * its max-pool (n, c1p, d/4, hgt/4, w/4); workspace layout and storage type, 256-byte aligned. All required.
 * in_z: the level-1 plane range already present in own_mid1 and own_skip1 (and its pooled planes in own_pool2).
 * out_mid1 / out_skip1 / out_pool2 (all or none), out_z, out_shift (level-1 planes): as in exaspim_unet_carry. */
typedef struct exaspim_unet_carry1 {
    void* own_mid1;
    void* own_skip1;
    void* own_pool2;
    int32_t in_z[2];
    void* out_mid1;
    void* out_skip1;
    void* out_pool2;
    int32_t out_z[2];
    int32_t out_shift;
    int32_t reserved;   /* 0 */
} exaspim_unet_carry1;
/* exaspim_unet_forward_prepared_carry with planes of the second level carried as well; out_dev gets the same
 * bits. carry1 needs carry (the pooled input planes of the left-out tiles arrive with the first level's carry):
 * in_z of carry1 non-empty needs in_z of carry non-empty, carry out of carry1 needs carry out of carry with
 * out_shift half of it. A request the engine cannot honour is EXASPIM_E_INVALID before anything is launched. */
int exaspim_unet_forward_prepared_carry1(exaspim_unet* h, const void* x_prepared_dev, float* out_dev,
                                         int32_t n, int32_t d, int32_t hgt, int32_t w,
                                         int32_t apply_sigmoid, int32_t trim, int32_t row_stride,
                                         const int32_t keep_hi[3], const exaspim_unet_carry* carry,
                                         const exaspim_unet_carry1* carry1, void* workspace_dev,
                                         size_t workspace_bytes, void* stream);

/* Rows of the first level carried along y, on top of the planes carried along z. A row batch whose patches start
 * shift_y rows after an earlier row batch (same x and z starts, same n and row_stride) computes, away from its own
 * zero padding along y, the bits that batch computed: its rows [2, hgt - shift_y - 2) are the earlier batch's
 * [2 + shift_y, hgt - 2). exaspim_unet_carry_rows: out[0..1] = the row range [y0, y1) of the LATER batch's frame a
 * forward can take over: the whole 8-row tiles of inc.3's row launch inside that span. Empty under the conditions
 * that leave exaspim_unet_carry_planes empty (no row mode) or when nothing fits. For hgt = 96, shift_y = 64: [8, 24).
 * Only the row launch of inc.3 takes rows over (x in [2, w - 2) of a patch face that borders a neighbour, every x of
 * the row's two outer faces); the border launch computes every row of its columns and the first convolution
 * writes every row.
 * A forward computes {planes outside carry->in_z} x {rows outside in_y} and stores again only what it computes:
 *   out_skip_y / out_pool_y (both or neither), out_y, out_shift_y: rows out_y of every plane it computes go to the
 *     y successor's own buffers at row - out_shift_y (pooled: half of it);
 *   out_skip_d / out_pool_d (both or neither; needs the z and the y carry out): planes carry->out_z x rows out_y go
 *     to the diagonal successor's own buffers, the batch out_shift planes down AND out_shift_y rows on, at
 *     plane - out_shift and row - out_shift_y. Neither the z nor the y successor computes that block -- each takes
 *     it over from this forward -- so neither can pass it on.
 * A successor with in_y must get every (plane, row) it does not compute from a predecessor that computes it: the
 * caller's plan sees to that (inference._carry_schedule). A carry out that meets the rows carried in is refused.
 * encoder_event (optional): a hipEvent_t the engine records on the stream right after inc.3's launches, when every
 * carry out of this forward has been issued: the y successor is usually the very next batch and need not wait for
 * the whole forward. */
int exaspim_unet_carry_rows(const exaspim_unet* h, int32_t n, int32_t d, int32_t hgt, int32_t w,
                            int32_t row_stride, int32_t shift_y, int32_t out[2]);
typedef struct exaspim_unet_carry_y {
    int32_t in_y[2];
    void* out_skip_y;
    void* out_pool_y;
    void* out_skip_d;
    void* out_pool_d;
    int32_t out_y[2];
    int32_t out_shift_y;
    int32_t reserved;   /* 0 */
    void* encoder_event;
} exaspim_unet_carry_y;
/* exaspim_unet_forward_prepared_carry1 (carry1 may be NULL) with rows carried along y; out_dev gets the same bits.
 * A request the engine cannot honour is EXASPIM_E_INVALID before anything is launched. */
int exaspim_unet_forward_prepared_carry_y(exaspim_unet* h, const void* x_prepared_dev, float* out_dev,
                                          int32_t n, int32_t d, int32_t hgt, int32_t w,
                                          int32_t apply_sigmoid, int32_t trim, int32_t row_stride,
                                          const int32_t keep_hi[3], const exaspim_unet_carry* carry,
                                          const exaspim_unet_carry1* carry1, const exaspim_unet_carry_y* carry_y,
                                          void* workspace_dev, size_t workspace_bytes, void* stream);

/* Range probe for the 16-bit storage modes. The reference loads ANY trained state_dict
 * (inference.py:400-424) and runs it in float32; IEEE-half storage holds |v| <= 65504 (stores
 * saturate there) with 11 significant bits. This is exaspim_unet_forward (nothing fused away,
 * nothing trimmed) that also raises absmax_dev[0] (inc.0), absmax_dev[1 + i] (i-th MFMA
 * convolution, the order of exaspim_unet_timing_begin's mask) and, with EXASPIM_UP_CONVT,
 * absmax_dev[18 + j] (up(j+1).up) to the largest |activation| the layer stored, as float32
 * (caller-zeroed float[EXASPIM_ABSMAX_SLOTS]; a NaN is reported as NaN). Run on a float32
 * engine it gives the true ranges of a checkpoint on real patches; on an f16 engine a value of
 * 65504 means a store saturated. UNet3D(compute_dtype="auto") decides with it on the first batch. */
#define EXASPIM_ABSMAX_SLOTS 22
int exaspim_unet_forward_absmax(exaspim_unet* h, const float* x_dev, float* out_dev,
                                int32_t n, int32_t d, int32_t hgt, int32_t w,
                                int32_t apply_sigmoid, float* absmax_dev, void* workspace_dev,
                                size_t workspace_bytes, void* stream);

/* Per-handle switches between bit-identical execution plans (tests and measurements; default 0):
 * SEPARATE_POOL runs every MaxPool3d(2) (unet3d.py:195) as its own launch instead of in the epilogue
 * of the convolution in front of it; SEPARATE_DEEP_POOLS does so for all but the first one. */
#define EXASPIM_OPT_SEPARATE_POOL 1u
#define EXASPIM_OPT_SEPARATE_DEEP_POOLS 2u
#define EXASPIM_OPT_PLAIN_UPSAMPLE 4u /* trilinear x2 on the un-pipelined kernel (same bits) */
#define EXASPIM_OPT_FIRST_PER_GROUP 8u /* inc.0 of the 16-bit modes group by group instead of on row strips (same bits) */
#define EXASPIM_OPT_UPSAMPLE_PER_THREAD 16u /* trimmed level-0 upsampling: per-thread pipeline instead of shared source rows (same bits) */
#define EXASPIM_OPT_PER_PATCH_ENCODER 32u /* exaspim_unet_forward_prepared_row: every patch's first level on its own (same bits) */
/* The 1x1x1 head as a launch of its own instead of fused into the last convolution; nothing is
 * trimmed then (the trimmed entry points run the full pass and write every voxel). In
 * EXASPIM_DT_BF16X3 it gives the same bits as the fused head. In the other modes the fused head
 * sums in a different order, and the 16-bit modes fuse on unrounded accumulators, so the values
 * differ within rounding. For the bit-identity tests and A/B timing. */
#define EXASPIM_OPT_SEPARATE_HEAD 64u
/* row mode of the first level: the patch faces that border a neighbour as two thin-tile launches and a
 * column max-pool instead of one launch that does both (same bits). (Bit 128 is not assigned.) */
#define EXASPIM_OPT_ROW_SEPARATE_BORDERS 256u
/* carried planes of the first level (exaspim_unet_forward_prepared_carry): only the row launch leaves the planes
 * carried in out and carries out; the border launch recomputes its columns on every plane and the first
 * convolution writes every plane (same bits). Without it the border launch carries as well, and the first
 * convolution skips the planes no launch reads. Set it on every handle of a carry chain or on none: predecessor
 * and successor must agree on who writes the border columns of the carried planes.
 * (EXASPIM_OPT_ROW_SEPARATE_BORDERS implies it.) */
#define EXASPIM_OPT_CARRY_MAIN_ONLY 512u
/* exaspim_unet_forward_prepared_carry_y: the y fields are checked and then ignored -- the forward computes every
 * row and stores nothing to the y and diagonal targets: exactly exaspim_unet_forward_prepared_carry1's launches
 * (same bits; the event is still recorded). Set it on every handle of a carry chain or on none.
 * (Bit 1024 is not assigned.) */
#define EXASPIM_OPT_CARRY_NO_ROWS 2048u
int exaspim_unet_set_options(exaspim_unet* h, uint32_t options);

/* Measurement hooks (bench.py's roofline leg). timing_begin arms HIP-event
 * timing, on the launch stream, of the MFMA convolutions whose bit is set in
 * conv_mask (bit i = i-th 3x3x3 conv after inc.0 in state_dict order: inc.3,
 * down1.0, down1.3, ... up4.0 = bit 15, up4.3 = bit 16); at most 16384 launches
 * are recorded. timing_read waits for the recorded events and returns, per
 * conv, the summed milliseconds and the number of launches, then disarms. */
int exaspim_unet_timing_begin(exaspim_unet* h, uint32_t conv_mask);
int exaspim_unet_timing_read(exaspim_unet* h, double ms_sum[17], int32_t count[17]);

/* ---- pre-processing: replaces np.minimum + img_util.normalize +
 *      _get_batch_inputs (inference.py:79-80,166-192;
 *      utils/img_util.py:362-379,405-428,504-533) ------------------------- */

/* Adds the 65536-bin histogram of min(voxel, clip) (clip applied iff
 * has_clip) over "n" voxels into hist_dev (uint64[65536], caller-zeroed).
 * 8/16-bit integer voxels are binned by value (I16: value + 32768); with a
 * fractional clip (np.minimum promotes the image to float64) every voxel above
 * it lands in bin ceil(clip), which then stands for the clip value itself. F32
 * voxels are binned by an order-preserving 32-bit key: pass 0 bins the key's
 * high 16 bits; pass 1 bins the low 16 bits of keys whose high half equals
 * "prefix"; voxels above a clip that float32 cannot hold (a float64 image, which
 * travels as float32) get the key of the float32 just above the clip, which
 * again stands for the clip value itself. Order statistics, and from them numpy's linear-interpolated
 * percentiles (img_util.py:526), follow exactly from these counts. */
int exaspim_histogram(const void* vol_dev, int32_t vox_dtype, size_t n,
                      double clip, int32_t has_clip, int32_t pass,
                      uint32_t prefix, uint64_t* hist_dev, void* stream);

/* The same for EXASPIM_VOX_F64 volumes (the reference takes ANY numeric array and works in
 * float64, inference.py:79-80, img_util.py:526-531): voxels are binned by an order-preserving
 * 64-bit key, 16 bits per pass -- pass p (0..3) bins key bits [48 - 16p, 64 - 16p) of the voxels
 * whose key bits above that field equal "prefix" (0 for pass 0). The clip is a float64 itself,
 * so min(voxel, clip) is exact. Four passes per order statistic give it exactly. */
int exaspim_histogram_wide(const void* vol_dev, int32_t vox_dtype, size_t n,
                           double clip, int32_t has_clip, int32_t pass,
                           uint64_t prefix, uint64_t* hist_dev, void* stream);

/* Builds a batch of network inputs: for patch i with global start
 * starts_dev[3*i..3*i+2] (int32 z,y,x), out[i] (float32 patch[0] x patch[1] x
 * patch[2]) = float32(clip01((min(v, clip) - mn) / denom)) evaluated in
 * float64, with v taken from the volume block and the part of the patch that
 * sticks out of the GLOBAL volume filled by numpy 'reflect' padding of the
 * in-volume part (img_util.py:378-379). denom = mx - mn + 1e-8. */
/* Layouts exaspim_gather_patches_as can write a batch in: the float32 patches above, or a
 * copy with a one-voxel zero border, (n, patch[0] + 2, patch[1] + 2, patch[2] + 2) 4-byte
 * words, holding the same float32 values or every value v split for the 16-bit matrix pipe,
 * bits(hi) | bits(lo) << 16 with hi = half(v), lo = half(v - float(hi)) (IEEE half or
 * bfloat16) -- what the engine's own padding pass makes of the float32 patch. */
#define EXASPIM_IN_F32 0
#define EXASPIM_IN_PADDED_F32 1
#define EXASPIM_IN_PADDED_SPLIT_F16 2
#define EXASPIM_IN_PADDED_SPLIT_BF16 3
int exaspim_gather_patches_as(const void* vol_dev, int32_t vox_dtype,
                              const exaspim_block* blk, const int32_t* starts_dev,
                              int32_t n, const int32_t patch[3], double clip,
                              int32_t has_clip, double mn, double denom, int32_t layout,
                              void* out_dev, void* stream);
int exaspim_gather_patches(const void* vol_dev, int32_t vox_dtype,
                           const exaspim_block* blk, const int32_t* starts_dev,
                           int32_t n, const int32_t patch[3], double clip,
                           int32_t has_clip, double mn, double denom,
                           float* out_dev, void* stream);

/* ---- post-processing: replaces the stitch loop and the final divide
 *      (inference.py:99-116,120-125) -------------------------------------- */

/* accum[c, s:e] += pred[i, c, trim:trim+(e-s)] for every patch i of the batch
 * in batch order, s = start + trim, e = min(s + patch - 2*trim, global dim),
 * restricted to the accumulator block. pred_dev is float32
 * (n, channels, patch) (the sigmoid output of exaspim_unet_forward);
 * accum_dev is float32 (channels, blk->dims). Deterministic: each voxel is
 * summed by one thread in patch order, so repeated runs are bit-identical. */
int exaspim_stitch_accumulate(const float* pred_dev, const int32_t* starts_dev,
                              int32_t n, int32_t channels,
                              const exaspim_window* win, float* accum_dev,
                              const exaspim_block* blk, void* stream);

/* accum[c, v] /= (number of patches whose trimmed output covers v) where that
 * number is non-zero (it is a product of three per-axis counts fixed by the
 * geometry alone), capped at 2048 where the reference's float16 weights stop
 * counting (inference.py:92); uncovered voxels keep 0. */
int exaspim_stitch_finalize(float* accum_dev, int32_t channels,
                            const exaspim_window* win, const exaspim_block* blk,
                            void* stream);

/* dst[i] = (IEEE half) src[i], round to nearest even, for i < n: the reduced-precision
 * export of a finalised result. The consumer of predict()'s output,
 * affinities_to_segmentation, starts with affinities.astype(np.float32)
 * (inference.py:223), so it takes a float16 array as it is; values are in [0, 1], the
 * rounding error is at most 2.4e-4. src_dev float32, dst_dev 16-bit, both 16-byte
 * aligned. */
int exaspim_export_f16(const float* src_dev, void* dst_dev, size_t n, void* stream);

/* ---- consumer front-end: connected components of thresholded affinities ---
 *      (the exactly defined part of what follows predict(): the affinity graph of
 *      utils/img_util.py:159-216 get_affinity_channels, cut at a threshold, then the size
 *      filter and renumbering of utils/img_util.py:536-559 remove_small_segments. It is NOT
 *      waterz's watershed / agglomeration, inference.py:196-237, which stays on the host.) */

/* element type of the affinities handed to exaspim_components */
#define EXASPIM_AFF_F32 0 /* float32 (predict()'s default output)                 */
#define EXASPIM_AFF_F16 1 /* IEEE half (exaspim_export_f16); widened exactly       */

/* Scratch bytes exaspim_components needs for a dims[0] x dims[1] x dims[2] (z, y, x) volume:
 * about 5 bytes per voxel. 0 (and a message) if a dim is not positive or the volume has more
 * than 2^31 - 1 voxels. */
size_t exaspim_components_workspace_bytes(const int32_t dims[3]);

/* labels_dev (int32, dims) = the connected components of the graph of "on" edges, small ones
 * removed, the rest numbered 1 .. K; *n_segments_dev = K.
 *  - channels = 3: aff_dev is (3, dims). Channel c at voxel v is the edge between v and v + e_c,
 *    e_0 = z, e_1 = y, e_2 = x (get_affinity_channels' convention); the entries at the last index
 *    along axis c leave the volume and are ignored whatever they hold. An edge is on iff
 *    float32(a) >= threshold; a NaN is off. A voxel without an on edge is background, label 0
 *    (a one-voxel segment has no affinity).
 *  - channels = 1: aff_dev is (dims), a foreground probability. A voxel is on iff p >= threshold, an
 *    edge iff both of its ends are on (6-connectivity); an on voxel alone is a component of size 1.
 *  - A component is kept iff size > min_size, strictly (img_util.py:555-558).
 *  - Kept components are numbered in the order of their smallest C-order linear index (first
 *    appearance in a raster scan); every other voxel gets 0.
 * The output is a pure function of the input: it depends neither on launch geometry nor on the
 * order in which atomics land. labels_dev doubles as the union-find's parent array while the passes
 * run; workspace_dev must be 16-byte aligned, aff_dev aligned to its element (16 bytes to get
 * the wide loads). Separate launches on "stream", no inter-workgroup waiting, nothing allocated,
 * nothing synchronised. EXASPIM_E_WORKSPACE if workspace_bytes is less than
 * exaspim_components_workspace_bytes(dims), before anything is launched; EXASPIM_E_INVALID for a
 * NULL pointer, an unknown aff_dtype, channels other than 3 or 1, a dim that is not positive, a
 * volume of more than 2^31 - 1 voxels, or a misaligned buffer (workspace_dev not 16-byte aligned,
 * labels_dev or aff_dev not aligned to its element). */
int exaspim_components(const void* aff_dev, int32_t aff_dtype, int32_t channels,
                       const int32_t dims[3], float threshold, int64_t min_size,
                       int32_t* labels_dev, int32_t* n_segments_dev, void* workspace_dev,
                       size_t workspace_bytes, void* stream);

/* ---- the same components for a volume that arrives in z slabs ----------------
 *      (DESIGN 6d). The slabs [z0, z1) of a dims[0] x dims[1] x dims[2] volume are pushed in z order,
 *      each while it sits on the device; the final labels equal, bit for bit, what exaspim_components
 *      gives on the whole volume, which may have more than 2^31 - 1 voxels (a slab may not).
 *      Semantics (edge convention, threshold rule, background, foreground mode, size filter,
 *      numbering, purity) are exaspim_components' own.
 *
 *      slab    labels the slab on its own and writes PROVISIONAL ids: 0, or an id in 1 .. capacity
 *              that is dense, grows in raster order of each slab-local component's first voxel and
 *              continues the previous slab's count. An id goes to every slab-local component that is
 *              larger than min_size on its own or has an on edge across a seam (so a voxel whose
 *              only on edge crosses a seam gets one although it is background within its slab);
 *              ids joined by an on edge between the previous slab's last plane and this slab's
 *              first one are united in a union-find over ids (atomicMin on the larger root);
 *      finish  after the last slab: sums the sizes per set of ids in 64 bits, keeps the sets with
 *              size > min_size and numbers them 1 .. K in the order of their smallest id, which is
 *              the raster order of the components' first voxels: table[id] = final label;
 *      apply   labels[v] = table[labels[v]] in place on any run of provisional labels.
 *
 *      All state is the caller's: this descriptor (host memory) and the device buffers it points to.
 *      Fill every field, next_z = 0, and keep them until the last apply. */
typedef struct exaspim_components_stream {
    int32_t dims[3];         /* the whole volume (z, y, x); dims[1] * dims[2] <= 2^31 - 1           */
    int32_t channels;        /* 3: affinities, 1: a foreground map                                  */
    float threshold;         /* on iff float32(value) >= threshold                                  */
    int32_t capacity;        /* most provisional ids the volume may use, 1 .. 2^31 - 2              */
    int64_t min_size;        /* a component is kept iff size > min_size; the same for every call    */
    int32_t next_z;          /* planes pushed so far: 0 to start, advanced by slab                  */
    int32_t reserved;        /* 0                                                                   */
    int32_t* id_parent_dev;  /* int32[capacity + 1]: the union-find over ids                        */
    int64_t* id_count_dev;   /* int64[capacity + 1]: voxels per id; after finish, per root, of its set */
    int32_t* table_dev;      /* int32[capacity + 1]: written by finish, table[0] = 0                */
    int32_t* state_dev;      /* int32[4]: ids used so far, overflow flag, K (after finish), scratch */
    int32_t* seam_ids_dev;   /* int32[dims[1] * dims[2]]: the last pushed plane's provisional ids   */
    uint8_t* seam_bits_dev;  /* uint8[dims[1] * dims[2]]: its z-edge bits (channels = 1: on bits)   */
} exaspim_components_stream;

/* Scratch bytes of one slab call for a slab_dims[0] x slab_dims[1] x slab_dims[2] slab: what
 * exaspim_components needs for a volume of that shape plus one byte per voxel of a plane. 0 (and a
 * message) if a dim is not positive or the slab has more than 2^31 - 1 voxels. */
size_t exaspim_components_stream_slab_workspace_bytes(const int32_t slab_dims[3]);

/* Scratch bytes of the finish call: 4 bytes per 2048 table entries. 0 (and a message) for a capacity
 * outside 1 .. 2^31 - 2. */
size_t exaspim_components_stream_finish_workspace_bytes(int32_t capacity);

/* Pushes planes [z0, z0 + slab_dims[0]) of the volume: aff_dev is the contiguous (channels, slab_dims)
 * tensor of aff_dtype (EXASPIM_AFF_*), labels_dev (int32, slab_dims) receives the provisional ids and
 * doubles as the slab's parent array while the passes run. z0 = 0 starts a new volume (the device
 * state is reset on the stream). The z edges of the slab's last plane are ignored only when that
 * plane is the volume's last. Needs z0 == st->next_z (slabs in z order, none twice), slab_dims[1:]
 * equal to st->dims[1:], z0 + slab_dims[0] <= st->dims[0]; then advances st->next_z.
 * More ids than st->capacity: the ids beyond it are written nowhere, their voxels get 0, and
 * state_dev[1] becomes 1, which the caller reads once after finish; the labels are then unusable.
 * Launches on "stream" only: nothing is allocated or synchronised, so the id count never visits the
 * host. Alignment: workspace_dev 16 bytes, labels_dev 4, aff_dev its element (16 for the wide
 * loads), the descriptor's int32 buffers 4 and id_count_dev 8. EXASPIM_E_WORKSPACE for fewer bytes
 * than exaspim_components_stream_slab_workspace_bytes(slab_dims), EXASPIM_E_INVALID for a NULL or
 * misaligned pointer, an unknown aff_dtype, a descriptor with channels other than 3 or 1, a dim that
 * is not positive, a plane or a slab of more than 2^31 - 1 voxels, a capacity outside 1 .. 2^31 - 2,
 * a slab out of order, of another (y, x) shape or beyond the volume: all before anything is launched
 * and with st unchanged. */
int exaspim_components_stream_slab(exaspim_components_stream* st, const void* aff_dev, int32_t aff_dtype,
                                   const int32_t slab_dims[3], int32_t z0, int32_t* labels_dev,
                                   void* workspace_dev, size_t workspace_bytes, void* stream);

/* Once, after the last slab (st->next_z == st->dims[0], else EXASPIM_E_INVALID): writes table_dev and
 * state_dev[2] = K. Sizes are summed in 64 bits, so a component may have more than 2^31 voxels.
 * workspace_dev: 16-byte aligned, exaspim_components_stream_finish_workspace_bytes(st->capacity)
 * bytes (EXASPIM_E_WORKSPACE below that). Launches only; read state_dev[1] (overflow) and
 * state_dev[2] after synchronising the stream. */
int exaspim_components_stream_finish(const exaspim_components_stream* st, void* workspace_dev,
                                     size_t workspace_bytes, void* stream);

/* labels_dev[i] = table_dev[labels_dev[i]] for i < n, in place: provisional ids to final labels, on a
 * slab, a part of one or several at once (n is not limited to 2^31). A value outside 0 .. capacity
 * becomes 0. labels_dev 4-byte aligned (16 for the wide form). One launch on "stream". */
int exaspim_components_stream_apply(const exaspim_components_stream* st, int32_t* labels_dev, size_t n,
                                    void* stream);

/* ---- mean-affinity agglomeration of components: the region graph ------------
 *      (later within ABI 5). The order of operations of the reference's
 *      affinities_to_segmentation (inference.py:196-237): over-segment into fragments, merge fragments
 *      whose contact has a high mean affinity, only then remove small segments. Fragments are
 *      exaspim_components at a threshold with min_size 0, the score is waterz's default (1 - mean
 *      affinity of the contact, merged greedily in order of score). It is NOT waterz: the fragments are
 *      connected components, not watershed basins, so the labels are not comparable with the
 *      reference's. */

/* Scratch bytes of exaspim_region_graph: 24 bytes per slot of the accumulator (a 64-bit key, count and
 * sum) plus 4 bytes per 2048 slots. 0 (and a message) if a dim is not positive, the volume has more than
 * 2^31 - 1 voxels, n_labels is negative or edge_capacity is not a power of two in 1 .. 2^30. */
size_t exaspim_region_graph_workspace_bytes(const int32_t dims[3], int32_t n_labels, int64_t edge_capacity);

/* The region graph of labels_dev (int32, dims) under aff_dev ((3, dims) of aff_dtype, EXASPIM_AFF_*, in
 * exaspim_components' edge convention: channel c at voxel v is the edge v -- v + e_c, the entries at the
 * last index along axis c are ignored whatever they hold). For every in-volume voxel edge with
 * la = labels[v], lb = labels[v + e_c], both in 1 .. n_labels and la != lb:
 *     key = (min(la, lb), max(la, lb)),  count[key] += 1,  sum[key] += q(a),
 *     q(a) = (uint32) rint(clamp(float32(a), 0, 1) * 2^24), a NaN gives 0, ties round to even.
 * count and sum are 64-bit integers: integer adds commute, so the result is a pure function of the input
 * whatever order the atomics land in. sizes_dev[l] (int64, n_labels + 1 entries) = the number of voxels
 * with label l, l = 0 (background) .. n_labels. A label outside 0 .. n_labels is counted nowhere, forms
 * no edge and never becomes an address.
 *  - Output: the E distinct keys in an UNSPECIFIED order (sort them after the download): row i of
 *    edges_dev (int32, edge_capacity x 2) = (lo, hi), count_dev[i] (int64), sum_dev[i] (uint64); all
 *    three must hold edge_capacity entries, the first E are written. n_edges_dev is int32[2]:
 *    n_edges_dev[0] = E, n_edges_dev[1] = the overflow flag.
 *  - The accumulator is an open-addressing table of edge_capacity slots (a power of two, the caller's
 *    choice) in the workspace. More distinct keys than slots: the contributions that find none are
 *    dropped and n_edges_dev[1] becomes 1, which the caller reads once, together with E; the output is
 *    then unusable. Every probe sequence is bounded by the capacity.
 * Separate launches on "stream"; no lock, no inter-workgroup waiting, nothing allocated, nothing
 * synchronised. EXASPIM_E_INVALID for a NULL pointer, an unknown aff_dtype, a dim that is not positive, a
 * volume of more than 2^31 - 1 voxels, a negative n_labels, an edge_capacity that is not a power of two
 * in 1 .. 2^30 or a misaligned buffer (workspace_dev 16 bytes, count_dev / sum_dev / sizes_dev 8, labels_dev
 * / edges_dev / n_edges_dev 4, aff_dev its element); EXASPIM_E_WORKSPACE if workspace_bytes is less than
 * exaspim_region_graph_workspace_bytes(dims, n_labels, edge_capacity): all before anything is launched. */
int exaspim_region_graph(const int32_t* labels_dev, const void* aff_dev, int32_t aff_dtype,
                         const int32_t dims[3], int32_t n_labels, int64_t edge_capacity,
                         int32_t* edges_dev, int64_t* count_dev, uint64_t* sum_dev, int64_t* sizes_dev,
                         int32_t* n_edges_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- the same region graph for a volume that arrives in z slabs ---------------
 *      (later within ABI 5). The slabs [z0, z1) of a dims[0] x dims[1] x dims[2] volume are
 *      pushed in z order, each with its int32 labels -- "provisional ids", any values, typically what
 *      exaspim_components_stream_slab wrote -- and its (3, z1 - z0, dims[1], dims[2]) affinities, while
 *      both sit on the device. The volume may have more than 2^31 - 1 voxels; a slab and a plane may not.
 *
 *      slab    every voxel edge inside the slab contributes under exaspim_region_graph's rule (both
 *              labels in 1 .. id_capacity, la != lb: key = (min, max), count += 1, sum += q(a)); the z
 *              entries of the slab's last plane form no edge inside the slab. For every (y, x) the edge
 *              from plane z0 - 1 to plane z0 contributes under the same rule with the carried id of the
 *              previous slab's last plane, this slab's first-plane id and the carried q of the previous
 *              slab's channel-0 value there. Two planes are carried from slab to slab: int32 ids and
 *              uint32 q. The volume's last plane carries nothing: its z entries are ignored whatever
 *              they hold. The same pass adds to sizes_by_id[0 .. id_capacity], 64-bit voxel counts; a
 *              label outside 0 .. id_capacity is counted nowhere and never becomes an address.
 *      finish  given any int32 table[0 .. table_len - 1] from provisional id to final label and
 *              n_labels: every accumulated key (a, b) becomes (table[a], table[b]); a key with an id at
 *              or beyond table_len, with equal ends or with an end outside 1 .. n_labels is dropped;
 *              equal final keys add their counts and sums; sizes[table[id]] += sizes_by_id[id] for ids
 *              inside the table, ids outside it or mapped outside 0 .. n_labels go to sizes[0]. The
 *              accumulator is only read, so finish may be called again with another table. Id 0 is the
 *              background of every table: it forms no edge whatever table[0] holds (label tables have
 *              table[0] = 0, and the equality below is stated for those).
 *
 *      After sorting by (lo, hi) the output equals exaspim_region_graph(table[labels], aff, n_labels) on
 *      the whole volume bit for bit, for every list of cuts: a pure function of the volume and the table.
 *      All state is the caller's: this descriptor (host memory) and the device buffers it points to.
 *      Fill every field, next_z = 0, and keep them until the last finish. */
typedef struct exaspim_region_graph_stream {
    int32_t dims[3];           /* the whole volume (z, y, x); dims[1] * dims[2] <= 2^31 - 1          */
    int32_t id_capacity;       /* the largest provisional id that counts, 1 .. 2^31 - 2              */
    int64_t edge_capacity;     /* slots of the accumulator: a power of two in 1 .. 2^30              */
    int32_t next_z;            /* planes pushed so far: 0 to start, advanced by slab                 */
    int32_t reserved;          /* 0                                                                  */
    uint64_t* keys_dev;        /* uint64[edge_capacity]: the accumulator's keys (provisional ids)    */
    uint64_t* counts_dev;      /* uint64[edge_capacity]: its counts                                  */
    uint64_t* sums_dev;        /* uint64[edge_capacity]: its sums                                    */
    int64_t* sizes_by_id_dev;  /* int64[id_capacity + 1]: voxels per provisional id                  */
    int32_t* seam_ids_dev;     /* int32[dims[1] * dims[2]]: the last pushed plane's ids              */
    uint32_t* seam_q_dev;      /* uint32[dims[1] * dims[2]]: q of its z affinities                   */
    int32_t* state_dev;        /* int32[2]: [1] = the accumulator's overflow flag                    */
} exaspim_region_graph_stream;

/* Pushes planes [z0, z0 + slab_dims[0]): labels_dev (int32, slab_dims) and aff_dev ((3, slab_dims) of
 * aff_dtype, EXASPIM_AFF_*), both contiguous. z0 = 0 starts a new volume: the accumulator, sizes_by_id and
 * the state are reset on the stream. Then, each a launch of its own: the seam above the slab, the slab's
 * tiles (exaspim_region_graph's kernel), the carried planes. Needs z0 == st->next_z, slab_dims[1:] equal
 * to st->dims[1:], z0 + slab_dims[0] <= st->dims[0]; then advances st->next_z. More distinct keys than
 * edge_capacity: the contributions that find no slot are dropped and state_dev[1] becomes 1, which finish
 * hands on. Shallow slabs need more slots than the final graph has edges: a slab cannot know that two of
 * its ids belong to one fragment. Launches on "stream" only; no lock, no inter-workgroup waiting, nothing
 * allocated, nothing synchronised. EXASPIM_E_INVALID for a NULL or misaligned pointer (the descriptor's
 * 64-bit buffers 8 bytes, its int32 buffers and labels_dev 4, aff_dev its element), an unknown aff_dtype,
 * a dim that is not positive, a plane or a slab of more than 2^31 - 1 voxels, an id_capacity outside
 * 1 .. 2^31 - 2, an edge_capacity that is not a power of two in 1 .. 2^30, a slab out of order, of another
 * (y, x) shape or beyond the volume: all before anything is launched and with st unchanged. */
int exaspim_region_graph_stream_slab(exaspim_region_graph_stream* st, const int32_t* labels_dev,
                                     const void* aff_dev, int32_t aff_dtype, const int32_t slab_dims[3],
                                     int32_t z0, void* stream);

/* Scratch bytes of the finish call: a second table of edge_capacity slots, 24 bytes each, plus 4 bytes per
 * 2048 slots. 0 (and a message) if edge_capacity is not a power of two in 1 .. 2^30. */
size_t exaspim_region_graph_stream_finish_workspace_bytes(int64_t edge_capacity);

/* After the last slab (st->next_z == st->dims[0], else EXASPIM_E_INVALID), any number of times: the region
 * graph under table_dev (int32, table_len >= 1 entries) and n_labels >= 0, in exaspim_region_graph's output
 * format: edges_dev / count_dev / sum_dev hold st->edge_capacity entries, the first E in an unspecified
 * order are written, sizes_dev has n_labels + 1 entries, n_edges_dev[0] = E, n_edges_dev[1] = 1 if the
 * accumulator or the second table overflowed (the output is then unusable). Launches on "stream" only.
 * PRECONDITION, not checked (the data is on the device): equal final keys are pooled in 64 bits, so the
 * accumulated counts must add up to at most 2^39, exaspim_agglomerate's bound; beyond 2^40 a pooled sum
 * can wrap. Counts of one volume's voxel edges (below 2^35.6 at 4096 x 2048 x 2048) are far inside it.
 * workspace_dev: 16-byte aligned, exaspim_region_graph_stream_finish_workspace_bytes(st->edge_capacity)
 * bytes, EXASPIM_E_WORKSPACE below that; EXASPIM_E_INVALID for a NULL or misaligned pointer, a bad
 * descriptor, table_len < 1 or a negative n_labels: all before anything is launched. */
int exaspim_region_graph_stream_finish(const exaspim_region_graph_stream* st, const int32_t* table_dev,
                                       int32_t table_len, int32_t n_labels, int32_t* edges_dev,
                                       int64_t* count_dev, uint64_t* sum_dev, int64_t* sizes_dev,
                                       int32_t* n_edges_dev, void* workspace_dev, size_t workspace_bytes,
                                       void* stream);

/* Host only (no device is touched). Merges the fragments 1 .. n_labels of a region graph and numbers
 * what is left: table[0 .. n_labels] (int32), table[0] = 0, *n_segments = S.
 *  - Input: n_edges rows (lo, hi) of "edges" sorted by (lo, hi) without repeats, 1 <= lo < hi <= n_labels,
 *    with 1 <= counts[i] <= 2^34 and sums[i] <= counts[i] * 2^24; sizes[0 .. n_labels] voxels per fragment.
 *    All counts together add up to at most 2^39 (a 4096 x 2048 x 2048 volume has 2^35.6 voxel edges):
 *    pooled counts then stay within 2^39 and pooled sums within 2^63, so the 64-bit pools never wrap and
 *    every 128-bit product is in range. A larger total is refused, with the total in the message.
 *  - Rule, exact in integers: m = rint((1 - (double)threshold) * 2^24). Among the CURRENT edges take the
 *    one with the largest mean sum / count (means compared by cross-multiplication in 128 bits; ties by
 *    the smaller lo, then the smaller hi, of the current root ids); merge it iff sum > m * count, else
 *    stop. Merging puts the larger root under the smaller; parallel edges to a common neighbour add their
 *    count and sum. The rule is a total order, so the result does not depend on the implementation.
 *  - A segment's size is the sum of its fragments' sizes; it is kept iff size > min_size
 *    (img_util.py:555-558), AFTER merging. Kept segments are numbered 1 .. S in the order of their root
 *    (smallest) id; with fragments numbered in raster order of their first voxel that is the raster order
 *    of the segments' first voxels. A dropped segment's fragments map to 0.
 * EXASPIM_E_INVALID for a NULL pointer, a negative n_labels or n_edges, a NaN threshold, or an edge list
 * that breaks the input rules above (the total of the counts included); table and *n_segments are then
 * not written. */
int exaspim_agglomerate(const int32_t* edges, const int64_t* counts, const uint64_t* sums, int64_t n_edges,
                        const int64_t* sizes, int32_t n_labels, float threshold, int64_t min_size,
                        int32_t* table, int32_t* n_segments);

/* labels_dev[i] = table_dev[labels_dev[i]] for i < n, in place (exaspim_components_stream_apply's kernel
 * without a stream descriptor). A value outside 0 .. table_len - 1 becomes 0 rather than an address.
 * labels_dev and table_dev 4-byte aligned (labels_dev 16 for the wide form), table_len >= 1. One launch
 * on "stream". */
int exaspim_apply_label_table(int32_t* labels_dev, size_t n, const int32_t* table_dev, int32_t table_len,
                              void* stream);

/* ---- watershed fragments for the agglomeration -------------------------------
 *      (later within ABI 5). The reference's affinities_to_segmentation calls
 *      waterz.agglomerate(aff, thresholds, aff_threshold_low=0.1, aff_threshold_high=0.9999)
 *      (inference.py:224-229), whose fragments are the basins of a steepest-ascent watershed on the
 *      affinity graph. This is that first step with an exact, order-independent definition; everything
 *      after the edge mask is exaspim_components' own code.
 *
 *      aff_dev is (3, dims) of aff_dtype (EXASPIM_AFF_*, float16 widened exactly) in exaspim_components'
 *      edge convention: channel c at voxel v is the edge v -- v + e_c, e = z, y, x; the entries at the
 *      last index along axis c are ignored whatever they hold. (waterz reads the same array as the edges
 *      v -- v - e_c; the project keeps the convention the network was trained in.)
 *       1. An edge is eligible iff float32(a) > low, strictly; a NaN is not eligible, +inf is.
 *       2. A voxel's steepest edge is the eligible edge of largest value among its up to six incident
 *          edges; among equal values the edge whose other end has the smallest C-order linear index,
 *          i.e. the first in the order -z, -y, -x, +x, +y, +z. A voxel without an eligible edge has none.
 *       3. An eligible edge is on iff a >= high, or it is the steepest edge of its lower end, or it is
 *          the steepest edge of its upper end.
 *       4. Fragments are the connected components of the graph of on edges; a voxel without an on edge
 *          is background (0). A fragment is kept iff size > max(min_size, 1), and kept fragments are
 *          numbered 1 .. K in raster order of each fragment's first voxel, as in exaspim_components.
 *      No relation between low and high is required: with high <= low every eligible edge is on.
 *
 *      This equals the serial steepest-ascent watershed (direction bits for "is the maximum, or >= high",
 *      plateau corners, breadth-first plateau division, pointer chasing with ids in raster order), label
 *      for label, on input where no voxel has two equal maximal eligible edges below high -- by the oracle
 *      in tests/, not by a run of waterz. Where such ties exist the serial algorithm depends on its
 *      visiting order and the two differ; this definition does not depend on any order. */

/* Scratch bytes of exaspim_watershed_fragments: exaspim_components_workspace_bytes' figure, about 5 bytes
 * per voxel. 0 (and a message) if a dim is not positive or the volume has more than 2^31 - 1 voxels. */
size_t exaspim_watershed_workspace_bytes(const int32_t dims[3]);

/* labels_dev (int32, dims) = the fragments defined above, *n_fragments_dev = K. A pure function of the
 * input. One launch for the edge mask (8 x 8 x 32 tiles with a one-voxel halo on the high faces, no
 * atomics), then exaspim_components' passes; launches on "stream" only, no inter-workgroup waiting,
 * nothing allocated, nothing synchronised. Buffers as for exaspim_components (aff_dev 16-byte aligned
 * and dims[2] a multiple of 16 bytes' worth of elements to get the wide loads). EXASPIM_E_WORKSPACE if
 * workspace_bytes is less than exaspim_watershed_workspace_bytes(dims); EXASPIM_E_INVALID for a NULL
 * pointer, an unknown aff_dtype, a dim that is not positive, a volume of more than 2^31 - 1 voxels, a
 * NaN low or high, or a misaligned buffer (workspace_dev not 16-byte aligned, labels_dev or aff_dev not
 * aligned to its element): all before anything is launched. */
int exaspim_watershed_fragments(const void* aff_dev, int32_t aff_dtype, const int32_t dims[3],
                                float low, float high, int64_t min_size,
                                int32_t* labels_dev, int32_t* n_fragments_dev,
                                void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- the same fragments for a volume that arrives in z slabs -----------------
 *      (later within ABI 5). The slabs of a dims[0] x dims[1] x dims[2] volume are pushed in z
 *      order as for exaspim_components_stream_slab. After exaspim_components_stream_finish and
 *      exaspim_components_stream_apply on &ws->base the labels equal, bit for bit, what
 *      exaspim_watershed_fragments gives on the whole volume with the same low, high and min_size, for every
 *      list of cuts, K (state_dev[2]) included; the volume may have more than 2^31 - 1 voxels (a slab may not).
 *      The four rules above hold word for word.
 *
 *      No plane of the next slab is needed. Channel 0 at voxel v is the edge v -- v + e_z, so the slab holds
 *      the +z edges of its own last plane. What a slab lacks are the -z edges of its first plane: the previous
 *      slab's last plane of channel 0, carried as float32 in seam_aff_dev (float16 widened exactly). Per slab
 *      [z0, z1) the steepest edges are chosen among every edge inside the slab, the real channel-0 values of
 *      plane z1 - 1 as +z edges unless z1 = dims[0] (there they are ignored whatever they hold), and the
 *      carried plane as the -z edges of plane z0 unless z0 = 0.
 *
 *      A seam edge can be switched on by the choice of its upper end, which the lower slab cannot know. For a
 *      last plane that is not the volume's the call leaves two bits per (y, x) in base.seam_bits_dev: bit 0
 *      eligible, bit 1 sure (eligible and >= high or the steepest edge of its lower end). The next call turns
 *      them into 1 (on: sure, or eligible and the first-plane voxel's steepest edge is -z) or 0 in place,
 *      before the ids are joined across the seam.
 *
 *      Ids. On the upper side of a seam a slab-local fragment gets a provisional id iff it is larger than
 *      min_size on its own or has an on edge to the carried plane: exact. On the lower side it gets one iff it
 *      is larger than min_size or has an ELIGIBLE edge across the seam, whether that edge ends up on or not:
 *      the conservative rule of exaspim_components_stream_slab's foreground mode. The final labels are the
 *      same (an id that is never joined passes or fails the size filter on its own count); the price is ids:
 *      size base.capacity for one id per voxel of a seam plane with an eligible z edge, not per on edge.
 *
 *      base.channels must be 3; base.threshold is ignored. z0 = 0 resets the state; the carried planes are
 *      never read before they are written, so none of the buffers needs initialising. */
typedef struct exaspim_watershed_stream {
    exaspim_components_stream base;  /* channels must be 3; threshold is ignored                            */
    float low;                       /* eligible iff float32(a) > low                                       */
    float high;                      /* an eligible edge with a >= high is on                               */
    float* seam_aff_dev;             /* float32[dims[1] * dims[2]]: the last pushed plane's z affinities    */
} exaspim_watershed_stream;

/* Scratch bytes of one slab call: exaspim_components_stream_slab_workspace_bytes' figure. 0 (and a message)
 * if a dim is not positive or the slab has more than 2^31 - 1 voxels. */
size_t exaspim_watershed_stream_slab_workspace_bytes(const int32_t slab_dims[3]);

/* Pushes planes [z0, z0 + slab_dims[0]) of the volume: aff_dev is the contiguous (3, slab_dims) tensor of
 * aff_dtype, labels_dev (int32, slab_dims) receives the provisional ids. Arguments, ordering, overflow and
 * alignment as for exaspim_components_stream_slab (the wide loads also need seam_aff_dev and
 * base.seam_bits_dev 16-byte aligned). One launch for the edge mask (exaspim_watershed_fragments' tiles, no
 * atomics; it also resolves the carried seam bits), one that carries the last plane's z affinities, then the
 * streamed components' passes: launches on "stream" only, no inter-workgroup waiting, nothing allocated,
 * nothing synchronised, and the id count never visits the host. EXASPIM_E_WORKSPACE for fewer bytes than
 * exaspim_watershed_stream_slab_workspace_bytes(slab_dims); EXASPIM_E_INVALID for everything
 * exaspim_components_stream_slab refuses and for base.channels other than 3, a NULL or misaligned
 * seam_aff_dev, a NaN low or high: all before anything is launched and with ws unchanged. */
int exaspim_watershed_stream_slab(exaspim_watershed_stream* ws, const void* aff_dev, int32_t aff_dtype,
                                  const int32_t slab_dims[3], int32_t z0, int32_t* labels_dev,
                                  void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- size-floor pre-merge of a region graph -----------------------------------
 *      (later within ABI 5). Watershed fragments of a large volume are millions of tiny basins,
 *      and exaspim_agglomerate on that many is slow. One ROUND joins every fragment smaller than a floor
 *      to the neighbour across its best mergeable contact and contracts the graph. It is NOT the
 *      agglomeration's rule restricted: it changes the segmentation (a tiny fragment joins its best
 *      neighbour at once, whatever that neighbour would have merged with first), so it is a named option.
 *
 *      Input: a region graph in exaspim_region_graph's format: K = n_labels fragments, E = n_edges rows
 *      (lo, hi) with 1 <= lo < hi <= K without repeats in any order, count >= 1 and sum per row,
 *      sizes[0 .. K]; a threshold T, from which m and merge_all are computed exactly as in
 *      exaspim_agglomerate (m = rint((1 - (double)T) * 2^24) clamped to 0 .. 2^24, merge_all iff the
 *      unclamped value is negative); a size floor S (int64). Everything in integers, a pure function of
 *      the input:
 *       1. An edge is mergeable iff merge_all or sum > m * count.
 *       2. A fragment f in 1 .. K is tiny iff sizes[f] < S.
 *       3. A tiny fragment with at least one mergeable edge chooses the neighbour across its mergeable
 *          edge of largest mean sum / count, compared by cross-multiplication in 128 bits; among equal
 *          means the smaller neighbour id. Other fragments choose nothing.
 *       4. If f and g choose each other, the smaller id drops its choice. Longer cycles cannot occur
 *          (means never decrease along choices, and ids strictly decrease around an all-equal cycle).
 *       5. Following choices to their end gives each fragment a root; fragments with the same root form
 *          a set.
 *       6. Sets are numbered 1 .. K' in order of their smallest member id: with fragments numbered in
 *          raster order of their first voxel so are the sets, and the order of any two sets' smallest ids
 *          is kept, so exaspim_agglomerate's ties and numbering mean what they meant before.
 *       7. map[0] = 0, map[f] = the number of f's set.
 *       8. sizes'[j] = the sum of sizes[f] over the members of set j; sizes'[0] = sizes[0].
 *       9. Every edge becomes (map[lo], map[hi]); edges inside a set vanish, edges between the same two
 *          sets add their count and sum.
 *      So: no set holds two fragments that are not tiny; the total size is kept; S <= 0 is the identity,
 *      and so is S = 1 when no fragment is empty; E' <= E. Rounds are repeated by the caller on their own
 *      output until one merges nothing (K' = K). An edge with an end outside 1 .. K or with equal ends is
 *      ignored by every rule and never becomes an address. */

/* Scratch bytes of exaspim_region_graph_premerge: a table of edge_capacity slots, 24 bytes each, plus 4
 * bytes per 2048 slots, plus 16 bytes per fragment and 4 bytes per 2048 fragments. 0 (and a message) if
 * n_labels is negative or edge_capacity is not a power of two in 1 .. 2^30. */
size_t exaspim_region_graph_premerge_workspace_bytes(int32_t n_labels, int64_t edge_capacity);

/* One round, on the device. In: edges_dev (int32, n_edges x 2), count_dev (int64), sum_dev (uint64),
 * sizes_dev (int64, n_labels + 1); they are only read. Out: the contracted graph in
 * exaspim_region_graph's output format -- edges_out_dev / count_out_dev / sum_out_dev hold edge_capacity
 * entries, the first E' in an UNSPECIFIED order are written --, sizes_out_dev (int64, n_labels + 1
 * entries: the first K' + 1 are sizes', the rest 0), map_dev (int32, n_labels + 1) and state_dev, int32[3]
 * = (K', E', the overflow flag). The contraction's accumulator is an open-addressing table of
 * edge_capacity slots in the workspace; edge_capacity >= n_edges always suffices, below that the flag
 * may come up and the edge list is then unusable (map and sizes' are not affected). Input and output
 * buffers must not overlap.
 *  - PRECONDITION, not checked here (the data is on the device and nothing is read back before the
 *    launches): 1 <= count <= 2^34 and sum <= count * 2^24 per row, and all counts together at most 2^39,
 *    exaspim_agglomerate's bounds. The table pools parallel edges in 64 bits: within the bound a pooled sum
 *    stays within 2^63 and every 128-bit comparison is exact, beyond it a pooled sum can wrap. A caller
 *    that cannot vouch for its counts reduces them first.
 *  - Passes, each a launch of its own on "stream": one thread per edge bids for its tiny ends' best edge
 *    (32-bit compare-and-swap, a total order), one thread per fragment resolves mutual pairs, pointer
 *    doubling between two buffers ceil(log2 K) + 1 times, the sets' smallest ids by atomic minimum, a
 *    prefix sum for the numbering, sizes' by 64-bit atomic adds, the edges through map into the table,
 *    a prefix sum for the edge list. The number of launches depends on n_labels only. No lock, no
 *    inter-workgroup waiting, nothing allocated, nothing synchronised.
 * EXASPIM_E_INVALID for a NULL pointer (the three edge inputs may be NULL when n_edges is 0), a negative
 * n_labels, n_edges outside 0 .. 2^31 - 1, a NaN threshold, an edge_capacity that is not a power of two
 * in 1 .. 2^30 or a misaligned buffer (workspace_dev 16 bytes, the 64-bit arrays 8, the int32 arrays 4);
 * EXASPIM_E_WORKSPACE if workspace_bytes is less than
 * exaspim_region_graph_premerge_workspace_bytes(n_labels, edge_capacity): all before anything is
 * launched. */
int exaspim_region_graph_premerge(const int32_t* edges_dev, const int64_t* count_dev, const uint64_t* sum_dev,
                                  const int64_t* sizes_dev, int64_t n_edges, int32_t n_labels,
                                  float threshold, int64_t size_floor, int64_t edge_capacity,
                                  int32_t* edges_out_dev, int64_t* count_out_dev, uint64_t* sum_out_dev,
                                  int64_t* sizes_out_dev, int32_t* map_dev, int32_t* state_dev,
                                  void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- dominant-edge contraction of a region graph -------------------------------
 *      (later within ABI 5). The reduction of the graph that changes NOTHING: one ROUND
 *      contracts every edge that exaspim_agglomerate is bound to merge before any other edge at its two
 *      ends, so the host merging starts from fewer fragments and ends with the same partition.
 *
 *      Input as for exaspim_region_graph_premerge: K = n_labels fragments, E = n_edges rows (lo, hi) with
 *      1 <= lo < hi <= K without repeats in any order, count >= 1 and sum per row, sizes[0 .. K]; m and
 *      merge_all from the threshold T exactly as in exaspim_agglomerate. Everything in integers, a pure
 *      function of the input:
 *       1. An edge is mergeable iff merge_all or sum > m * count.
 *       2. Edge e DOMINATES AT fragment f iff e is mergeable, f is an end of e, and every other mergeable
 *          row e' at f has sum_e * count_e' > sum_e' * count_e (128-bit products, strict): e's mean is
 *          strictly the largest among the mergeable edges at f.
 *       3. e is contracted iff it dominates at both its ends. The contracted edges form a matching (a
 *          strict maximum at a shared end is unique): a set is a pair or a single fragment.
 *       4. Sets are numbered 1 .. K' in order of their smallest member id; map, sizes' and the pooled
 *          edges follow rules 6 - 9 of the pre-merge round above.
 *       5. A row with an end outside 1 .. K, with equal ends or with count == 0 is ignored by every rule
 *          and never becomes an address; in particular it neither dominates nor ties anything, and it
 *          does not reach the output.
 *      So: the total size is kept, E' <= E, and a round in which no edge dominates is the identity. Equal
 *      means are never resolved here: they make an edge non-dominant, and it waits for the host, whose
 *      tie-break then applies unchanged.
 *
 *      THEOREM. For a row list without repeated pairs, exaspim_agglomerate(T, min_size) on the input
 *      graph and on the round's output, composed through map, give the same table and the same number
 *      of segments. (Until the greedy merges a dominant edge e = (i, j), every other edge at i or j has
 *      a mean strictly below e's -- pooling two edges gives a mean that is at most the larger of the
 *      two --, so no edge at i or j goes before e; e is mergeable, so the greedy reaches it; up to then
 *      the top edge of the graph is also the top edge of the graph with e contracted, no pooled edge at
 *      the merged fragment ties it, and contractions commute because pooling is additive. Numbering sets by their
 *      smallest member is monotone, so ties by current root id and the final numbering mean what they
 *      meant. DESIGN 6j has the proof.) Rounds may be repeated on their own output and stopped anywhere.
 *      NOT covered: a row list with repeated pairs. Two rows of the same pair are compared as two edges
 *      here, while exaspim_agglomerate pools them first; pool such a list before the first round (the
 *      round's own output never repeats a pair). */

/* Scratch bytes of exaspim_region_graph_contract_dominant: a table of edge_capacity slots, 24 bytes each,
 * plus 4 bytes per 2048 slots, plus 12 bytes per fragment and 4 bytes per 2048 fragments. 0 (and a
 * message) if n_labels is negative or edge_capacity is not a power of two in 1 .. 2^30. */
size_t exaspim_region_graph_contract_dominant_workspace_bytes(int32_t n_labels, int64_t edge_capacity);

/* One round, on the device. Inputs, outputs, state_dev = (K', E', the overflow flag), the table, the
 * PRECONDITION on counts and sums (1 <= count <= 2^34, sum <= count * 2^24, all counts together at most
 * 2^39; not checked here) and the refusals are those of exaspim_region_graph_premerge; there is no size
 * floor. Input and output buffers must not overlap.
 *  - Passes, each a launch of its own on "stream": one thread per edge bids for the best edge of both its
 *    ends (32-bit compare-and-swap, a total order), one thread per edge marks the ends whose best mean it
 *    equals without being the best (plain stores of one value), one thread per fragment pairs the two
 *    ends of an edge that is the best of both with neither marked, a prefix sum for the numbering, sizes'
 *    by 64-bit atomic adds, the edges through map into the table, a prefix sum for the edge list. The
 *    number of launches is a constant. No lock, no inter-workgroup waiting, nothing allocated, nothing
 *    synchronised.
 * EXASPIM_E_INVALID for a NULL pointer (the three edge inputs may be NULL when n_edges is 0), a negative
 * n_labels, n_edges outside 0 .. 2^31 - 1, a NaN threshold, an edge_capacity that is not a power of two
 * in 1 .. 2^30 or a misaligned buffer (workspace_dev 16 bytes, the 64-bit arrays 8, the int32 arrays 4);
 * EXASPIM_E_WORKSPACE if workspace_bytes is less than
 * exaspim_region_graph_contract_dominant_workspace_bytes(n_labels, edge_capacity): all before anything is
 * launched, and every output buffer is left alone. */
int exaspim_region_graph_contract_dominant(const int32_t* edges_dev, const int64_t* count_dev,
                                           const uint64_t* sum_dev, const int64_t* sizes_dev, int64_t n_edges,
                                           int32_t n_labels, float threshold, int64_t edge_capacity,
                                           int32_t* edges_out_dev, int64_t* count_out_dev, uint64_t* sum_out_dev,
                                           int64_t* sizes_out_dev, int32_t* map_dev, int32_t* state_dev,
                                           void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- distance-to-boundary field and per-label table for the skeletoniser ------
 *      (later within ABI 5). The reference's skeletonize (inference.py:257-291) hands the labels
 *      to kimimaro's TEASAR, which begins with two data-parallel stages: the distance-to-boundary field
 *      of every label at once, and per-label facts (bounding box, voxel count, the field's maximum, which
 *      is also its soma test, and where it lies) with which each segment is cropped and rooted. These are
 *      those two stages with an exact definition in integers; the serial remainder (Dijkstra on a
 *      per-label crop, the paths, SWC export) stays on the host. Checked against the oracle in tests/, not
 *      against a run of edt or kimimaro.
 *
 *      labels are int32 (dims), C order; a voxel with label <= 0 is background. EXASPIM_DBF_INF = 2^31 - 1.
 *       1. dbf[v] = 0 for a background voxel.
 *       2. For a voxel v with label L > 0, dbf[v] = the minimum of |v - u|^2 over all in-volume voxels u
 *          with labels[u] != L (background and every other label alike: touching segments bound each
 *          other), voxel centre to voxel centre, unit spacing. Squared, in integers, nothing rounded.
 *       3. With black_border != 0 the volume is surrounded by one layer of background: a voxel at index i
 *          of an axis of length n also has the candidates (i + 1)^2 and (n - i)^2 on every axis. With
 *          black_border == 0 the faces are no boundary.
 *       4. A voxel without any candidate (black_border == 0 and one label filling the volume) gets
 *          EXASPIM_DBF_INF.
 *      Volumes with (D+1)^2 + (H+1)^2 + (W+1)^2 >= 2^31 - 1 are refused, so every finite value is below
 *      EXASPIM_DBF_INF and int32 never wraps. */
#define EXASPIM_DBF_INF 2147483647

/* Scratch bytes of exaspim_dbf: one int32 field, 4 bytes per voxel rounded up to 16. 0 (and a message) if
 * a dim is not positive, the volume has more than 2^31 - 1 voxels or the diagonal bound above fails. */
size_t exaspim_dbf_workspace_bytes(const int32_t dims[3]);

/* dbf_dev (int32, dims) = the field defined above (inference.py:257-291: the first stage of
 * kimimaro.skeletonize). A pure function of the input; labels_dev is only read. Three launches on "stream"
 * (along x by run ends from two scans, then along y and along z by a window that grows while k^2 is below
 * the best value so far; the middle field lives in the workspace), no atomics, no inter-workgroup waiting,
 * nothing allocated, nothing synchronised. The cost of the y and z passes is the window depth per voxel,
 * about the square root of the result; a run whose field is still EXASPIM_DBF_INF is walked to its end.
 * EXASPIM_E_INVALID for a NULL pointer, a dim that is not positive, a volume of more than 2^31 - 1
 * voxels, the diagonal bound, or a misaligned buffer (workspace_dev 16 bytes, labels_dev and dbf_dev 4);
 * EXASPIM_E_WORKSPACE if workspace_bytes is less than exaspim_dbf_workspace_bytes(dims): all before
 * anything is launched. */
int exaspim_dbf(const int32_t* labels_dev, const int32_t dims[3], int32_t black_border,
                int32_t* dbf_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Scratch bytes of exaspim_segment_table: 8 bytes per row of the table, n_labels + 1 rows, rounded up to
 * 16. 0 (and a message) if n_labels is negative. */
size_t exaspim_segment_table_workspace_bytes(int32_t n_labels);

/* Per-label facts of a labelled volume (inference.py:257-291: what kimimaro.skeletonize crops and roots
 * each segment with), K = n_labels, every output with K + 1 rows:
 *   sizes_dev (int64)       voxels per label; row 0 counts the voxels labelled exactly 0, as
 *                           exaspim_region_graph does. Negative labels and labels above K are counted
 *                           nowhere and never become an address.
 *   boxes_dev (int32, x 6)  (z0, y0, x0, z1, y1, x1), half-open; all 0 for an absent label and for row 0.
 *   peak_dev (int32)        the largest dbf value of the label; 0 for an absent label and row 0, and
 *                           everywhere when dbf_dev is NULL.
 *   peak_index_dev (int32)  the smallest C-order linear index at which the label attains its peak; -1
 *                           for an absent label and row 0. With dbf_dev NULL: the label's first voxel in
 *                           raster order.
 * dbf_dev (int32, dims) may be NULL; it is only read, and so is labels_dev. A pure function of the input:
 * sizes by 64-bit atomic adds, boxes by int32 atomic minima and maxima, the peak by a 64-bit atomic
 * maximum of (dbf, 2^32 - 1 - index), runs of equal labels reduced inside a wave first. Three launches on
 * "stream", no inter-workgroup waiting, nothing allocated, nothing synchronised.
 * EXASPIM_E_INVALID for a NULL pointer other than dbf_dev, dims that exaspim_dbf refuses, a negative
 * n_labels or a misaligned buffer (workspace_dev 16 bytes, sizes_dev 8, the int32 arrays 4);
 * EXASPIM_E_WORKSPACE if workspace_bytes is less than exaspim_segment_table_workspace_bytes(n_labels):
 * all before anything is launched. */
int exaspim_segment_table(const int32_t* labels_dev, const int32_t* dbf_dev /* may be NULL */,
                          const int32_t dims[3], int32_t n_labels,
                          int64_t* sizes_dev, int32_t* boxes_dev, int32_t* peak_dev, int32_t* peak_index_dev,
                          void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- enclosed cavities of every label, closed (later within ABI 5) ------
 *      The reference's skeletonize (inference.py:257-291) calls kimimaro.skeletonize(..., fill_holes=True):
 *      every segment has its enclosed cavities closed before the distance-to-boundary field is taken. This
 *      is that step for all labels at once, with an exact definition in integers. It is named after the
 *      reference's keyword and checked against the two oracles in tests/ (holes_ref.py); it is not claimed
 *      to equal the fill_voids package or kimimaro.
 *
 *      labels are int32 (dims), C order.
 *       1. A voxel is background iff its label is <= 0 (exaspim_dbf's convention).
 *       2. A cavity is a 6-connected component of background voxels.
 *       3. A cavity is a hole of label L iff (a) none of its voxels lies on a face of the volume (index 0
 *          or n - 1 of any axis) and (b) the positive labels among the six neighbours of its voxels are
 *          exactly the one value L.
 *       4. Every voxel of a hole of L becomes L, negative voxels inside the hole included. Every other
 *          voxel keeps its value bit for bit.
 *      So: cavities that touch a face stay; cavities bounded by two or more labels stay (an island of
 *      another label M inside a cavity of L makes its neighbours {L, M}); a floating piece of L itself
 *      inside the cavity does not keep it open; positive voxels never change (a label enclosed by another
 *      label is not removed); with a single-voxel axis every voxel lies on a face and nothing is filled,
 *      which is what scipy.ndimage.binary_fill_holes gives on a 3-D array of depth 1.
 *      Relation to the per-label oracle: on volumes where no positive voxel lies inside the filled region
 *      of another label, the result equals the union over every L of binary_fill_holes(labels == L) with
 *      scipy's default 6-connected structure, each written as L. */

/* Scratch bytes of exaspim_fill_holes: a parent array, two survey words and a mask byte per voxel, about
 * 13 bytes per voxel. 0 (and a message) if a dim is not positive or the volume has more than 2^31 - 1
 * voxels. */
size_t exaspim_fill_holes_workspace_bytes(const int32_t dims[3]);

/* out_dev (int32, dims) = labels_dev with every hole filled, as defined above (inference.py:257-291: the
 * fill_holes=True of kimimaro.skeletonize); counts_dev[0] = the number of holes filled, counts_dev[1] =
 * the number of voxels filled. A pure function of the input. labels_dev is only read, and out_dev ==
 * labels_dev is allowed: the last pass reads and writes the same voxel only. Launches on "stream" alone:
 * the background's edge mask, the tile-local union-find of exaspim_components with its face merge and
 * flatten, a survey of each cavity (its faces first, then atomic minima and maxima of the neighbouring
 * labels per cavity root, reduced inside a wave first), and the fill; minima, maxima and integer adds, so
 * nothing depends on arrival order. No inter-workgroup waiting, nothing allocated, nothing synchronised.
 * EXASPIM_E_INVALID for a NULL pointer, a dim that is not positive, a volume of more than 2^31 - 1 voxels
 * or a misaligned buffer (workspace_dev 16 bytes, counts_dev 8, labels_dev and out_dev 4);
 * EXASPIM_E_WORKSPACE if workspace_bytes is less than exaspim_fill_holes_workspace_bytes(dims): all before
 * anything is launched, and no output is touched. */
int exaspim_fill_holes(const int32_t* labels_dev, const int32_t dims[3], int32_t* out_dev,
                       int64_t* counts_dev /* [2] */, void* workspace_dev, size_t workspace_bytes,
                       void* stream);

/* ---- geodesic distance-from-source field of every label (later within ABI 5) ------
 *      The reference's skeletonize (inference.py:257-291) hands the labels to kimimaro's TEASAR, which
 *      needs a root for every segment and the distance-from-root field (DAF): the root is the maximum of
 *      the distance-to-boundary field of a soma, otherwise the voxel farthest from an arbitrary voxel of
 *      the segment; the DAF gives TEASAR its targets and the second term of its penalty field. kimimaro
 *      takes both from one serial Dijkstra per label on the host. This is the single-source field of all
 *      labels at once, with an exact definition in float32. Checked against the two oracles in tests/
 *      (geodesic_ref.py); not claimed to equal dijkstra3d or kimimaro, whose background and unreachable
 *      conventions were not compared.
 *
 *      labels are int32 (dims), C order; a voxel with label <= 0 is background. K = n_labels.
 *      sources is int32 (K + 1): the C-order linear index of the source voxel of each label; row 0 is
 *      ignored, -1 means the label has no source. Any other row L is valid iff 0 <= s < D*H*W and
 *      labels[s] == L; an invalid row is counted and the label treated as having no source.
 *       1. Voxels u, v are adjacent iff they differ by at most 1 in every coordinate, are not equal
 *          (the 26-neighbourhood, in-volume only) and carry the same label L with 1 <= L <= K.
 *       2. The step weight w(u -> v), float32. Euclidean mode (cost NULL): 1.0f, 0x3FB504F3 (fl32(sqrt 2))
 *          or 0x3FDDB3D7 (fl32(sqrt 3)) by the number of coordinates that differ; constants, no root is
 *          taken on the device. Cost mode (cost float32, dims): w = cost[v], the cost of the voxel
 *          entered, if cost[v] >= 0 (-0.0 counts as 0); a voxel whose cost is negative, NaN or +inf
 *          cannot be entered (w = +inf).
 *       3. The field d (float32, dims) is the least solution of d[source] = 0 and
 *          d[v] = min over adjacent u of fl32(d[u] + w(u -> v)), every sum one IEEE round-to-nearest
 *          float32 addition. Adding a non-negative float32 is monotone and never decreases its argument,
 *          so the least fixed point is unique, independent of the order of relaxation, and equal bit for
 *          bit to what a heap Dijkstra computing in float32 returns.
 *       4. A background voxel gets 0.0. A foreground voxel of a label without a valid source, of a label
 *          above K, or not reachable from the source inside its label gets +inf.
 *      The farthest table (K + 1 rows): far_value (float32) the largest finite value of the label,
 *      far_index (int32) the smallest C-order index attaining it; +inf voxels are ignored; row 0, absent
 *      labels and labels without a valid source get 0.0 and -1. */

/* Scratch bytes of exaspim_geodesic_begin and _sweeps: a 16-byte header (which flag array is current, the
 * tiles flagged in either, the invalid rows) and two int32 flags per 8 x 8 x 32 tile. 0 (and a message)
 * if a dim is not positive or the volume has more than 2^31 - 1 voxels (exaspim_fill_holes' bound: the
 * squared diagonal that exaspim_dbf also bounds has no part in a float32 field). */
size_t exaspim_geodesic_workspace_bytes(const int32_t dims[3]);

/* Starts the field defined above (inference.py:257-291: the root search and the distance-from-root field
 * of kimimaro.skeletonize): field_dev = +inf on foreground and 0 on background, 0 at every valid source,
 * the tiles that hold one or see it in their halo flagged for the first sweep. state_dev[0] = the number of tiles flagged,
 * state_dev[1] = the number of invalid source rows. labels_dev and sources_dev are only read; the
 * workspace carries the flags to exaspim_geodesic_sweeps and must not be touched in between. Three
 * launches on "stream", nothing allocated, nothing synchronised.
 * EXASPIM_E_INVALID for a NULL pointer, a dim that is not positive, a volume of more than 2^31 - 1 voxels,
 * a negative n_labels or a misaligned buffer (workspace_dev 16 bytes, the rest 4);
 * EXASPIM_E_WORKSPACE if workspace_bytes is less than
 * exaspim_geodesic_workspace_bytes(dims): all before anything is launched, and no output is touched. */
int exaspim_geodesic_begin(const int32_t* labels_dev, const int32_t dims[3], const int32_t* sources_dev,
                           int32_t n_labels, float* field_dev, int32_t* state_dev /* [2] */,
                           void* workspace_dev, size_t workspace_bytes, void* stream);

/* Runs "sweeps" >= 1 sweeps of the relaxation on a field exaspim_geodesic_begin started (the same labels,
 * dims, n_labels and workspace; inference.py:257-291). A sweep is one workgroup per flagged tile: the tile
 * and a one-voxel halo are relaxed in LDS until nothing in the tile changes (at most 2049 rounds, after
 * which it has converged anyway), the voxels that fell are stored, and the tiles that see one of them in
 * their halo -- faces, edges and corners -- are flagged for the next sweep. state_dev[0] = the number of
 * tiles flagged for the sweep after the last one, 0 meaning that field_dev is the field defined above;
 * state_dev[1] = the invalid source rows, as before. Once converged, further sweeps do nothing. Tiles of
 * one sweep may read each other's voxels before or after they are stored: both values bound the answer
 * from above and the writer flags the reader, so no workgroup waits for another and the result does not
 * depend on the schedule. cost_dev (float32, dims) selects cost mode and is only read; pass the same
 * value to every call of one field. Two launches per sweep on "stream", nothing allocated, nothing
 * synchronised.
 * EXASPIM_E_INVALID for a NULL pointer other than cost_dev, dims as above, a negative n_labels,
 * sweeps < 1 or a misaligned buffer; EXASPIM_E_WORKSPACE for a short workspace: all before
 * anything is launched, and no output is touched. */
int exaspim_geodesic_sweeps(const int32_t* labels_dev, const float* cost_dev /* may be NULL */,
                            const int32_t dims[3], int32_t n_labels, float* field_dev, int32_t sweeps,
                            int32_t* state_dev /* [2] */, void* workspace_dev, size_t workspace_bytes,
                            void* stream);

/* Scratch bytes of exaspim_geodesic_farthest: 8 bytes per row, n_labels + 1 rows, rounded up to 16. 0 (and
 * a message) if n_labels is negative. */
size_t exaspim_geodesic_farthest_workspace_bytes(int32_t n_labels);

/* The farthest table of a converged field, as defined above (inference.py:257-291: kimimaro's find_root
 * and TEASAR's first target): a 64-bit atomic maximum of (field bits, 2^32 - 1 - index) per label over the
 * finite voxels, runs of equal labels reduced inside a wave first; a pure function of the input. Three
 * launches on "stream", nothing allocated, nothing synchronised. EXASPIM_E_INVALID for a NULL pointer,
 * dims as above, a negative n_labels or a misaligned buffer (workspace_dev 16 bytes, the rest 4);
 * EXASPIM_E_WORKSPACE for a short workspace: all before anything is launched. */
int exaspim_geodesic_farthest(const int32_t* labels_dev, const float* field_dev, const int32_t dims[3],
                              int32_t n_labels, float* far_value_dev, int32_t* far_index_dev,
                              void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- parental field and root paths of every label (later within ABI 5) ------------------
 *      The reference's skeletonize (inference.py:257-291) runs kimimaro's TEASAR, which takes one parental
 *      field per label over its penalty field (dijkstra3d.parental_field) and reads every path off it from
 *      a target back to the root (path_from_parents). This is the parental field of all labels at once, of
 *      a field d that exaspim_geodesic_sweeps converged on exactly these labels, sources and cost, with a
 *      definition that is exact in integers and independent of the schedule. Adjacency, K, valid sources
 *      and the weights w(u -> v) are those of the section above.
 *       1. An edge u -> v is tight iff u and v are adjacent, d[u] and d[v] are finite, v is not its label's
 *          source, and fl32(d[u] + w(u -> v)) has the bit pattern of d[v]: one IEEE round-to-nearest
 *          float32 addition, the one the field was built with.
 *       2. hops h (int32) is the least solution of h[source] = 0, h[v] = 1 + min over tight u -> v of h[u]:
 *          the breadth-first distance from the source in the directed graph of tight edges. Every voxel
 *          with finite d has one (the edge that last lowered v in a Dijkstra is tight and comes from a
 *          voxel settled earlier), and an integer least fixed point is unique and independent of any order.
 *       3. parent (int32, C-order linear index): parent[source] = the source's own index; otherwise the
 *          tight predecessor u with h[u] = h[v] - 1 that has the smallest linear index. hops fall by exactly
 *          1 along parents, so there is no cycle even on a plateau where d[u] = d[v] because a cost was
 *          absorbed; the chain from v reaches the source in h[v] steps, and re-adding the weights along it
 *          from the source reproduces d at every voxel of it, bit for bit.
 *       4. Everything else gets h = -1 and parent = -1: background, labels above K, labels without a valid
 *          source, voxels with d = +inf.
 *       5. An orphan is a voxel of a label in 1..K with finite d that is no source and has no tight
 *          predecessor. It exists only if d is not the field of these inputs (another cost, a field that
 *          is not converged, a source whose d is not 0). Orphans are counted, never guessed at.
 *       6. The path of a target t with h[t] >= 0 is the h[t] + 1 voxels source = p_0, ..., p_h = t with
 *          parent[p_i] = p_(i-1): voxel v stands at position h[v] of its path.
 *      Checked against the two oracles in tests/parents_ref.py; not claimed to equal dijkstra3d's
 *      parental_field or kimimaro, whose parents are one Dijkstra run's tie-breaks, 1-based, with 0 for
 *      "none". Hops are relaxed on the finished field, not as (d, h) pairs in one relaxation: a pair's h can
 *      be derived from a neighbour's earlier, larger d and survive when that neighbour falls and its own
 *      hop count grows, and a min-only relaxation never raises it. */

/* Starts the hops of the parental field defined above (inference.py:257-291: dijkstra3d.parental_field in
 * kimimaro.skeletonize): hops_dev = -1 everywhere and 0 at every valid source whose field word is +0.0;
 * the tiles that hold one or see it in their halo are flagged for the first sweep. A source row that is
 * invalid, or whose field is not +0.0, counts as invalid. state_dev[0] = the number of tiles flagged,
 * state_dev[1] = the number of invalid rows; state_dev holds three words, the third belongs to
 * exaspim_geodesic_parents_finish. The workspace is that of exaspim_geodesic_workspace_bytes(dims); it
 * carries the flags to exaspim_geodesic_parents_sweeps and must not be touched in between. labels_dev,
 * sources_dev and field_dev are only read. Three launches on "stream", nothing allocated, nothing
 * synchronised.
 * EXASPIM_E_INVALID for a NULL pointer, a dim that is not positive, a volume of more than 2^31 - 1 voxels,
 * a negative n_labels or a misaligned buffer (workspace_dev 16 bytes, the rest 4); EXASPIM_E_WORKSPACE for
 * a short workspace: all before anything is launched, and no output is touched. */
int exaspim_geodesic_parents_begin(const int32_t* labels_dev, const int32_t dims[3], const int32_t* sources_dev,
                                   int32_t n_labels, const float* field_dev, int32_t* hops_dev,
                                   int32_t* state_dev /* [3] */, void* workspace_dev, size_t workspace_bytes,
                                   void* stream);

/* Runs "sweeps" >= 1 sweeps of the hops relaxation exaspim_geodesic_parents_begin started (the same labels,
 * field, dims, n_labels and workspace; inference.py:257-291). A sweep is one workgroup per flagged tile: the
 * 26 tests of a tight edge are taken once per voxel of the tile, hops with a one-voxel halo are relaxed
 * in LDS as h[v] = min(h[v], 1 + min over tight u of h[u]), in unsigned arithmetic where -1 is the largest
 * value, until nothing in the tile changes (at most 2049 rounds), the voxels that fell are stored, and the
 * tiles that see one of them in their halo are flagged for the next sweep. state_dev[0] = the number of
 * tiles flagged for the sweep after the last one, 0 meaning that hops_dev is the hops defined above;
 * state_dev[1] = the invalid rows, as before. Every value written is 1 + the hops of a real tight path,
 * hence an upper bound, and the writer flags the reader: no workgroup waits for another and the result
 * does not depend on the schedule. cost_dev (float32, dims) must be what the field was built with, NULL for
 * Euclidean steps. Two launches per sweep on "stream", nothing allocated, nothing synchronised.
 * EXASPIM_E_INVALID for a NULL pointer other than cost_dev, dims as above, a negative n_labels,
 * sweeps < 1 or a misaligned buffer; EXASPIM_E_WORKSPACE for a short workspace: all before anything is
 * launched, and no output is touched. */
int exaspim_geodesic_parents_sweeps(const int32_t* labels_dev, const float* cost_dev /* may be NULL */,
                                    const float* field_dev, const int32_t dims[3], int32_t n_labels,
                                    int32_t* hops_dev, int32_t sweeps, int32_t* state_dev /* [3] */,
                                    void* workspace_dev, size_t workspace_bytes, void* stream);

/* The parents of converged hops, as defined above (inference.py:257-291: the parental field TEASAR reads
 * its paths from): per voxel with h >= 1 the tight predecessor with h - 1 and the smallest linear index,
 * a source its own index, everything else -1. state_dev[2] = the number of orphans; state_dev[0] and [1]
 * are left as they are. Every input is only read and parents_dev only written, so no result depends on a
 * word the same launch rewrites. One memset and one launch on "stream", nothing allocated, nothing
 * synchronised. EXASPIM_E_INVALID for a NULL pointer other than cost_dev, dims as above, a negative
 * n_labels or a misaligned buffer: all before anything is launched, and no output is touched. */
int exaspim_geodesic_parents_finish(const int32_t* labels_dev, const float* cost_dev /* may be NULL */,
                                    const float* field_dev, const int32_t* hops_dev, const int32_t dims[3],
                                    int32_t n_labels, int32_t* parents_dev, int32_t* state_dev /* [3] */,
                                    void* stream);

/* Reads the paths of n_targets targets off a parental field (inference.py:257-291: path_from_parents in
 * kimimaro's TEASAR). offsets_dev is int64 (n_targets + 1): row i is written to
 * paths_dev[offsets[i] .. offsets[i + 1]), source first, target last, and must be hops[targets[i]] + 1
 * long; that offsets[n_targets] <= paths_capacity is the caller's to guarantee and is checked per row on the
 * device. One thread per target walks at most hops[target] steps, so a corrupt parents array cannot spin
 * it. state_dev[0] = the targets that are out of range, have h < 0, or whose row is not h + 1 long or does
 * not lie within paths_capacity: such a row is left unwritten. state_dev[1] = the broken walks: one that
 * leaves the volume, meets -1 or does not end on a self-parent; nothing is read out of range. Duplicate
 * targets are allowed. targets_dev and paths_dev may be NULL if n_targets is 0. One memset and at most one
 * launch on "stream", nothing allocated, nothing synchronised. EXASPIM_E_INVALID for a NULL pointer, dims
 * as above, a negative n_targets or paths_capacity, or a misaligned buffer (offsets_dev 8 bytes, the rest
 * 4): all before anything is launched, and no output is touched. */
int exaspim_trace_paths(const int32_t* parents_dev, const int32_t* hops_dev, const int32_t dims[3],
                        const int32_t* targets_dev, int32_t n_targets, const int64_t* offsets_dev,
                        int32_t* paths_dev, int64_t paths_capacity, int32_t* state_dev /* [2] */, void* stream);

/* ---- fields and hops seeded from a list (later within ABI 5) --------------------------------
 *      The reference's skeletonize (inference.py:257-291) runs kimimaro.skeletonize with its default
 *      fix_branching=True: every path after the first is a shortest path on a penalty field zeroed along the
 *      earlier paths. That needs a field with several sources per label, and a way to add sources to a
 *      converged one. seeds is int32 (n_seeds): C-order linear indices, any number per label, duplicates
 *      allowed. A seed is valid iff 0 <= s < D*H*W and 1 <= labels[s] <= K. The seeded field is the field of
 *      the section above with d[s] = +0.0 at every valid seed: the least fixed point of the same float32
 *      relaxation, so bit for bit a multi-source float32 heap Dijkstra. A seed's own cost is never read; a
 *      label without a seed stays +inf. Incremental form: if d is the converged field of seeds A, then d
 *      with +0.0 stored at seeds B and relaxed again is the field of A u B, bit for bit: every old value is
 *      the float32 sum along a real path from a voxel that is still a seed, hence an upper bound; the
 *      relaxation only lowers values and ends with d[v] <= fl32(d[u] + w) on every edge, and induction
 *      along an optimal path with the monotonicity of float32 addition gives d <= the answer. Seeded hops
 *      and parents are those of the parental-field section with "the source" read as "a seed": h = 0 at
 *      every valid seed whose field word is +0.0 (any other seed counts as invalid), no tight edge enters a
 *      seed, and a seed is its own parent. Checked against the oracles in tests/fix_branching_ref.py; not
 *      claimed to equal kimimaro. */

/* Re-seeds a field (inference.py:257-291: the Dijkstra per path of kimimaro's fix_branching): clears the
 * header and both flag arrays of the workspace, so a field converged at any earlier time may be passed,
 * stores +0.0 at every valid seed and flags the seed's tile and the tiles that see it in their halo for the
 * first sweep of exaspim_geodesic_sweeps, which then runs unchanged on the same workspace. An invalid seed
 * writes nothing. state_dev[0] = the number of tiles flagged, state_dev[1] = the number of invalid seeds.
 * A field built from scratch is exaspim_geodesic_begin with every source -1, then this call. labels_dev and
 * seeds_dev are only read; seeds_dev may be NULL if n_seeds is 0. At most three launches on "stream",
 * nothing allocated, nothing synchronised.
 * EXASPIM_E_INVALID for a NULL pointer, a dim that is not positive, a volume of more than 2^31 - 1 voxels,
 * a negative n_labels or n_seeds, or a misaligned buffer (workspace_dev 16 bytes, the rest 4);
 * EXASPIM_E_WORKSPACE if workspace_bytes is less than exaspim_geodesic_workspace_bytes(dims): all before
 * anything is launched, and no output is touched. */
int exaspim_geodesic_reseed(const int32_t* labels_dev, const int32_t dims[3], int32_t n_labels,
                            const int32_t* seeds_dev, int64_t n_seeds, float* field_dev,
                            int32_t* state_dev /* [2] */, void* workspace_dev, size_t workspace_bytes,
                            void* stream);

/* exaspim_geodesic_parents_begin with the list of seeds in place of the per-label table
 * (inference.py:257-291: the parental field of every path's Dijkstra in kimimaro's fix_branching):
 * hops_dev = -1 everywhere and 0 at every valid seed whose field word is +0.0; any other seed is counted
 * in state_dev[1]. exaspim_geodesic_parents_sweeps and _finish then run unchanged. seeds_dev may be NULL if
 * n_seeds is 0. At most three launches on "stream", nothing allocated, nothing synchronised. Refusals as
 * exaspim_geodesic_reseed: all before anything is launched, and no output is touched. */
int exaspim_geodesic_parents_begin_seeds(const int32_t* labels_dev, const int32_t dims[3], int32_t n_labels,
                                         const int32_t* seeds_dev, int64_t n_seeds, const float* field_dev,
                                         int32_t* hops_dev, int32_t* state_dev /* [3] */, void* workspace_dev,
                                         size_t workspace_bytes, void* stream);

/* ---- TEASAR's loop: targets, branches, invalidation ------------------------------------------
 * What follows the fields and the parental field in the reference's skeletonize (inference.py:257-291:
 * the loop of kimimaro's TEASAR), for all labels at once, in the single-parental-field form: every path is
 * read off ONE parental field, which is kimimaro with fix_branching=False. The reference runs kimimaro with
 * its default fix_branching=True, a Dijkstra per path on a penalty field zeroed along the earlier paths:
 * that form is these three calls with the field re-seeded and the parents rebuilt before every round after
 * the first (exaspim_geodesic_reseed, exaspim_geodesic_parents_begin_seeds). fix_borders is
 * exaspim_border_targets fed to exaspim_teasar_round_given. Soma detection and its
 * spherical invalidation and anisotropy are not built, and equality with kimimaro is not claimed.
 *
 * The definition, in integers. K = n_labels. A voxel v is eligible iff its label L is in 1..K, sources[L]
 * names a voxel of L, hops[v] >= 0 and the bits of daf[v] are below 0x7F800000 (finite, sign bit clear: -0.0
 * is left out as exaspim_geodesic_farthest leaves it out). mask_dev holds one byte per voxel: bit 0 "still
 * valid", at first the eligible voxels, bit 1 "on the skeleton", at first none. Round t = 1, 2, ...: (1) the
 * target of every label that still has a valid voxel is the valid voxel with the largest daf bits, ties to
 * the smallest linear index; a label without one is finished. (2) The branch: walk parents from the target
 * to the first voxel that is on the skeleton (the junction) or to the source, a self-parent reached after
 * exactly hops[target] steps (junction -1); the new vertices are the walked voxels without the junction,
 * listed junction side first. A walk that leaves the volume, meets -1 or a self-parent early, or does not
 * end on a skeleton voxel or the source is broken: it is counted, writes nothing and finishes its label.
 * (3) The radius of a new vertex p is r(p) = min(R, floor(fl64(fl64(scale * sqrt64(max(dbf[p], 0))) +
 * const))), R = max(D, H, W), every operation one rounded double operation, the comparison taken in double.
 * (4) Every voxel q with labels[q] == L inside row L of boxes whose Chebyshev distance to a new vertex p of
 * L is at most r(p) loses bit 0; the new vertices lose bit 0 in any case (a box that leaves them out
 * cannot make the loop endless) and get bit 1. The kernels clear, per vertex, its cube minus
 * the cube of the vertex before it on the branch (the junction for the first one), which was cleared before:
 * tests/teasar_ref.py holds this form to the one that stamps whole cubes along whole paths. With parents
 * that lead from one label into another the result is unspecified, but every access stays in range. */

/* Scratch bytes of the three calls below: 8 + 4 bytes per row, n_labels + 1 rows, each part rounded up to
 * 16. 0 with the error text set for dims exaspim_fill_holes refuses or a negative n_labels. */
size_t exaspim_teasar_workspace_bytes(const int32_t dims[3], int32_t n_labels);

/* Writes the state byte of every voxel as defined above and clears state_dev (five words) and the
 * workspace's per-label words. Every other argument is only read. One launch on "stream", nothing
 * allocated, nothing synchronised. EXASPIM_E_INVALID for a NULL pointer, a dim that is not positive, a volume
 * of more than 2^31 - 1 voxels, a negative n_labels or a misaligned buffer (workspace_dev 16 bytes, mask_dev
 * none, the rest 4); EXASPIM_E_WORKSPACE for a short workspace: all before anything is launched, and no
 * output is touched. */
int exaspim_teasar_begin(const int32_t* labels_dev, const int32_t* sources_dev /* [n_labels + 1] */,
                         const int32_t* hops_dev, const float* daf_dev, const int32_t dims[3], int32_t n_labels,
                         uint8_t* mask_dev, int32_t* state_dev /* [5] */, void* workspace_dev,
                         size_t workspace_bytes, void* stream);

/* Steps (1) and (2) of one round, without writing the branch: targets_dev[L] = the target of label L or -1,
 * lengths_dev[L] (int64) = the number of its new vertices, junction_dev[L] = its junction or -1, each of
 * n_labels + 1 rows, row 0 being -1, 0, -1. state_dev[0] = the labels that have a branch this round,
 * state_dev[1] = the broken walks of this round, state_dev[2] = the sum of lengths_dev, state_dev[3] = the
 * branches without a junction; state_dev[4], the rows exaspim_teasar_apply refused since
 * exaspim_teasar_begin, is left as it is. mask_dev is only read. The target pass reads the state byte first
 * and labels and daf only where it says valid; the walk takes at most hops[target] steps and range-checks
 * every index, so corrupt parents cannot spin it or lead it out of the volume. Three launches on "stream",
 * nothing allocated, nothing synchronised. Refusals as exaspim_teasar_begin (lengths_dev 8 bytes). */
int exaspim_teasar_round(const int32_t* labels_dev, const float* daf_dev, const int32_t* parents_dev,
                         const int32_t* hops_dev, const int32_t dims[3], int32_t n_labels, const uint8_t* mask_dev,
                         int32_t* targets_dev, int64_t* lengths_dev, int32_t* junction_dev,
                         int32_t* state_dev /* [5] */, void* workspace_dev, size_t workspace_bytes, void* stream);

/* exaspim_teasar_round with targets the loop did not choose itself (kimimaro's manual_targets_before, which
 * fix_borders feeds with the border targets). given_dev is int32 (n_labels + 1): row L >= 0 is this
 * round's target of label L, -1 means the rule of step (1); row 0 is not read. With every row -1 all outputs
 * and state_dev[0..4] are those of exaspim_teasar_round, byte for byte. A given target need not be still valid
 * (bit 0); the walk of step (2) is unchanged. A given target that is on the skeleton already is no branch: the
 * label's rows are -1, 0, -1, it is not counted in state_dev[0] and it is not finished. A given row that is
 * out of range, whose voxel is not labelled L, or that is not eligible (hops < 0, or daf bits >= 0x7F800000)
 * is counted in state_dev[5], the sixth word, which this call clears first, and is read as -1. Round 1 still
 * puts every live label's source on the skeleton (nothing is on it before, so every walk ends at the source),
 * so branches without a junction occur only in round 1 and exaspim_teasar_apply runs unchanged. Three launches
 * on "stream", nothing allocated, nothing synchronised. Refusals as exaspim_teasar_round, given_dev included. */
int exaspim_teasar_round_given(const int32_t* labels_dev, const float* daf_dev, const int32_t* parents_dev,
                               const int32_t* hops_dev, const int32_t dims[3], int32_t n_labels,
                               const uint8_t* mask_dev, const int32_t* given_dev /* [n_labels + 1] */,
                               int32_t* targets_dev, int64_t* lengths_dev, int32_t* junction_dev,
                               int32_t* state_dev /* [6] */, void* workspace_dev, size_t workspace_bytes,
                               void* stream);

/* Steps (2) to (4) of the round exaspim_teasar_round prepared. offsets_dev is int64 (n_labels + 2): 0
 * followed by the inclusive cumulative sum of lengths_dev, so that label L's branch is written to
 * voxels_dev, radii_dev and before_dev at [offsets[L], offsets[L + 1]), junction side first: the vertex, its
 * radius, and the vertex before it (the junction or -1 for the first). n_new = state_dev[2] and n_roots =
 * state_dev[3] as read after exaspim_teasar_round; the three arrays hold "capacity" >= n_new entries and may
 * be NULL if n_new is 0. n_new stands in for the offsets' total, offsets[n_labels + 1], which lies on the
 * device: the host refuses capacity < n_new, and a row whose offsets do not match its length or reach beyond
 * n_new is counted in state_dev[4] and left unwritten, so every write is bounded by n_new <= capacity. boxes_dev is int32 (n_labels + 1, 6), half-open (z0, y0, x0, z1, y1, x1)
 * as exaspim_segment_table writes them; a box is clipped to the volume. The invalidation runs over the
 * round's new vertices in grid x and over the voxels of a vertex's at most six slabs in grid y; the whole
 * cubes of round 1's roots have a launch of their own (skipped if n_roots is 0) with a larger grid y. Two
 * workgroups may clear the same byte: both write the same value. At most three launches on "stream",
 * nothing allocated, nothing synchronised. EXASPIM_E_INVALID for a NULL pointer, dims as above, a negative
 * n_labels, n_new or n_roots, scale or const that is not finite or is negative, capacity < n_new, or a
 * misaligned buffer (lengths_dev and offsets_dev 8 bytes, mask_dev none, the rest 4): all before anything
 * is launched, and no output is touched. */
int exaspim_teasar_apply(const int32_t* labels_dev, const int32_t* parents_dev, const int32_t* dbf_dev,
                         const int32_t* boxes_dev, const int32_t dims[3], int32_t n_labels, double scale,
                         double konst, uint8_t* mask_dev, const int32_t* targets_dev, const int64_t* lengths_dev,
                         const int32_t* junction_dev, const int64_t* offsets_dev, int32_t* voxels_dev,
                         int32_t* radii_dev, int32_t* before_dev, int64_t n_new, int64_t capacity, int32_t n_roots,
                         int32_t* state_dev /* [5] */, void* stream);

/* ---- border targets: the centre of every cut -------------------------------------------------
 * What kimimaro.skeletonize(..., fix_borders=True) asks for (inference.py:286 of the reference): where a
 * face of the volume cuts a label, the skeleton is to end at the centre of the cut, a point the block next
 * door, which sees the same plane of voxels, picks as well. The definition is this project's own, exact in
 * integers and free of any order; equality with kimimaro, which breaks ties by closeness to a centroid, is
 * not claimed.
 *
 * K = n_labels. The six faces are the planes z = 0, z = D - 1 (H x W), y = 0, y = H - 1 (D x W), x = 0 and
 * x = W - 1 (D x H), each a 2-D array of labels. A pixel is foreground iff its label is in 1..K. For a
 * foreground pixel p, e(p) is the least squared in-plane Euclidean distance to a pixel of the same plane whose
 * label differs from p's, or to a position just outside the plane (a black border: at row i, column j of an
 * h x w plane e <= min((i + 1)^2, (h - i)^2, (j + 1)^2, (w - j)^2)); an integer, at most
 * (min(h, w) / 2 + 1)^2. A face component is an 8-connected set of pixels of one plane with one foreground
 * label; its target is its pixel with the largest e, ties to the smallest linear voxel index
 * (z H W + y W + x). The result is the set of pairs (label, voxel index) over all components of all six
 * faces; a voxel that is the target of two faces (on an edge or in a corner, or where a dimension is 1 and
 * two faces coincide) appears once. e taken on labels equals e taken on components (DESIGN 6p has the proof),
 * so only the argmax needs the components. */

/* Scratch bytes of exaspim_border_targets: 4 x 4 + 8 bytes per face pixel, P = 2 (HW + DW + DH) of them,
 * each part rounded up to 16. 0 with the error text set for dims exaspim_border_targets refuses. */
size_t exaspim_border_targets_workspace_bytes(const int32_t dims[3]);

/* The border targets of labels_dev as rows (out_labels_dev[i], out_voxels_dev[i]), in no defined order:
 * callers compare as sets or sort. state_dev[0] = the number of targets found, which may exceed "capacity":
 * rows past it are not written, every write is bounded by it, and the two arrays may be NULL if it is 0;
 * capacity = P never overflows. state_dev[1] = 0 (spare). labels_dev is only read. Six launches on "stream"
 * (gather, the distance along the columns and along the rows, an 8-connected union-find, a 64-bit atomic
 * maximum per component, the rows through a counter), nothing allocated, nothing synchronised; the result
 * is a pure function of the arguments.
 * EXASPIM_E_INVALID for a NULL pointer, a dim that is not positive, a volume of more than 2^31 - 1 voxels
 * or faces of more than 2^31 - 1 pixels, a negative n_labels or capacity, or a misaligned buffer
 * (workspace_dev 16 bytes, the rest 4); EXASPIM_E_WORKSPACE if workspace_bytes is less than
 * exaspim_border_targets_workspace_bytes(dims): all before anything is launched, and no output is touched. */
int exaspim_border_targets(const int32_t* labels_dev, const int32_t dims[3], int32_t n_labels,
                           int32_t* out_labels_dev, int32_t* out_voxels_dev, int32_t capacity,
                           int32_t* state_dev /* [2] */, void* workspace_dev, size_t workspace_bytes,
                           void* stream);

/* ---- pieces: the 26-connected components of every label, without the dust ---------------------
 * What kimimaro.skeletonize does before anything else (the reference's call, inference.py:272-290, leaves
 * dust_threshold at kimimaro's 1000): it relabels the volume by 26-connected components, drops the small ones
 * and skeletonises each of the others. The definition is this project's own, exact in integers; equality with
 * cc3d or kimimaro is not claimed, and neither is a dependency.
 *
 * K = n_labels. A voxel is foreground iff its label is in 1..K; labels above K and values <= 0 are background.
 * A piece is a maximal 26-connected set of foreground voxels with one label. Its size is its voxel count, its
 * first voxel its smallest linear index z H W + y W + x. A piece is kept iff size >= dust_threshold
 * (0 and 1 keep everything), otherwise it is dust. Kept pieces are numbered 1..P, in
 * ascending order of first voxel. Every voxel of a kept piece holds the piece's number, every other voxel 0.
 * The result is a pure function of the input.
 *
 * Two consequences hold exactly (DESIGN 6q has the proofs): exaspim_dbf of the pieces equals exaspim_dbf of
 * the labels at every voxel of a kept piece, whatever became of the dust; and exaspim_border_targets of the
 * pieces is that of the labels restricted to kept pieces, the label column mapped to piece numbers. */

/* Scratch bytes of exaspim_label_pieces: 4 bytes per voxel and 4 per 2048 voxels, each part rounded up to
 * 256. 0 with the error text set for dims exaspim_label_pieces refuses. */
size_t exaspim_label_pieces_workspace_bytes(const int32_t dims[3]);

/* pieces_dev[v] = the number of the kept piece of voxel v, or 0. state_dev[0] = P, the number of kept pieces;
 * state_dev[1] = the number of dust pieces. labels_dev is only read; pieces_dev holds the union-find's parents
 * until the last launch and must not be labels_dev. Eight launches on "stream" (the unions inside 8 x 8 x 32
 * tiles in LDS, the unions across tile faces, edges and corners, flatten, the sizes, a three-pass prefix sum over
 * the kept roots, the final numbering) and two memsets, nothing allocated, nothing synchronised.
 * EXASPIM_E_INVALID for a NULL pointer, a dim that is not positive, a volume of more than 2^31 - 1 voxels, a
 * negative n_labels or dust_threshold, pieces_dev == labels_dev, or a misaligned buffer (workspace_dev 16
 * bytes, the rest 4); EXASPIM_E_WORKSPACE if workspace_bytes is less than
 * exaspim_label_pieces_workspace_bytes(dims): all before anything is launched, and no output is touched. */
int exaspim_label_pieces(const int32_t* labels_dev, const int32_t dims[3], int32_t n_labels,
                         int64_t dust_threshold, int32_t* pieces_dev,
                         int32_t* state_dev /* [2]: kept pieces P, dust pieces */, void* workspace_dev,
                         size_t workspace_bytes, void* stream);

/* ---- pieces with open faces: the pieces of one block of a larger volume -----------------------
 * A volume too large for one call is skeletonised block by block, adjacent blocks sharing one plane. Inside a
 * block a piece that touches a shared plane goes on next door: its size here says nothing about the whole
 * piece, so the dust rule must not judge it. The definition is the one of the section above with one change.
 *
 * Bit f of open_faces names face f in the order of the border targets: z = 0, z = D - 1, y = 0, y = H - 1,
 * x = 0, x = W - 1. A piece is open iff at least one of its voxels lies on a face whose bit is set; where a
 * dimension is 1 and two faces coincide, either bit opens the plane. A piece is kept iff it is open or
 * size >= dust_threshold. Numbering (ascending order of first voxel) and the output volume are unchanged.
 * With open_faces == 0 pieces_dev and state_dev[0..1] are those of the call above byte for byte and
 * state_dev[2] is 0. The result is a pure function of the arguments.
 *
 * What this is not: a dust rule for the whole piece. Whoever joins the blocks sums what each block owns of a
 * piece and judges the sum (skeletonize_blocks in segmentation.py does); equality with cc3d, kimimaro or
 * igneous is not claimed. */

/* Scratch bytes of the call below: those of the call above. 0 with the error text set for refused dims. */
size_t exaspim_label_pieces_open_workspace_bytes(const int32_t dims[3]);

/* pieces_dev[v] = the number of the kept piece of voxel v, or 0. state_dev[0] = P, the number of kept pieces;
 * state_dev[1] = the number of dust pieces; state_dev[2] = the number of pieces kept although below the
 * threshold. The launches of the call above on "stream", as they are, and one more after the sizes where
 * open_faces is not 0: one thread per pixel of the open faces marks the sign bit of its root's count, which
 * the prefix sum's predicate reads. Two memsets, nothing allocated, nothing synchronised.
 * EXASPIM_E_INVALID for what the call above refuses, or an open_faces with a bit above bit 5;
 * EXASPIM_E_WORKSPACE if workspace_bytes is too small: all before anything is launched, and no output is
 * touched. */
int exaspim_label_pieces_open(const int32_t* labels_dev, const int32_t dims[3], int32_t n_labels,
                              int64_t dust_threshold, uint32_t open_faces, int32_t* pieces_dev,
                              int32_t* state_dev /* [3] */, void* workspace_dev, size_t workspace_bytes,
                              void* stream);

/* ---- the overlap table of two label volumes (later within ABI 5) -------------------------------
 * How much two labelings of the same voxels differ -- the variation of information, the adapted Rand error,
 * the largest-overlap agreement, "the same partition up to names" -- is a function of one small integer table,
 * and this is the table.
 *
 * a and b are flat int32 arrays of n voxels; the table has no geometry. For a label value v, v' = v if v > 0
 * else 0: everything <= 0 is background, as in exaspim_fill_holes. For every voxel, count[(a', b')] += 1. The
 * key is an ordered pair: (1, 2) and (2, 1) are different rows. Every positive int32 is a legal label,
 * 2^31 - 1 included; there is no n_labels and no label ever becomes an address. Counts are 64-bit integers:
 * the table is exact in integers, a pure function of the voxels added whatever order the atomics land in, and
 * the sum of all counts equals the number of voxels added. It is additive over voxels, so a volume added in
 * pieces of any lengths gives the table of the whole, and the total may exceed 2^31 - 1 voxels.
 *
 * The table lives in the workspace between calls: an open-addressing table of pair_capacity slots (a power of
 * two in 1 .. 2^30, the caller's choice) of a 64-bit key and a 64-bit count, an overflow word, and the block
 * sums of the scan. More distinct pairs than slots: the contributions that find no slot are dropped, never
 * written anywhere else, and state_dev[1] becomes 1; the output is then unusable.
 *     reset    the table empty.
 *     add      n voxels of a_dev and b_dev into the table, 0 <= n <= 2^31 - 1; n = 0 launches nothing. a_dev
 *              and b_dev need 4-byte alignment only (a z slab sliced from a contiguous volume starts
 *              anywhere); 16-byte loads are used wherever both addresses allow it.
 *     finish   the occupied slots as rows: row i of pairs_dev (int32, pair_capacity x 2) = (a', b'),
 *              count_dev[i] (int64), the first P in an UNSPECIFIED order (sort them after the download);
 *              state_dev[0] = P, state_dev[1] = the overflow flag. finish only reads the table: the scan's
 *              block sums are the only workspace words it writes, so it may be called twice with the same
 *              result, and again after further adds, when it reports the larger total.
 * exaspim_label_overlaps is reset + add + finish.
 *
 * What this is not: no claim of equality with skimage's, CREMI's or funlib's numbers beyond the formulas
 * stated (overlap_scores in segmentation.py states them); no matching by Hungarian assignment; no
 * per-segment error lists.
 *
 * Launches and memsets on "stream", nothing allocated, nothing synchronised. EXASPIM_E_INVALID for a NULL
 * pointer, a pair_capacity that is not a power of two in 1 .. 2^30, n outside 0 .. 2^31 - 1 or a misaligned
 * buffer (workspace_dev 16 bytes, count_dev 8, the rest 4); EXASPIM_E_WORKSPACE if workspace_bytes is less
 * than exaspim_label_overlaps_workspace_bytes(pair_capacity): all decided from the argument values before
 * anything is launched. */

/* Scratch bytes of the four calls below: 16 bytes per slot, 256 for the overflow word and 4 per 2048 slots,
 * each part rounded up to 256. 0 (and a message) if pair_capacity is not a power of two in 1 .. 2^30. */
size_t exaspim_label_overlaps_workspace_bytes(int64_t pair_capacity);

int exaspim_label_overlaps_reset(int64_t pair_capacity, void* workspace_dev, size_t workspace_bytes, void* stream);

int exaspim_label_overlaps_add(const int32_t* a_dev, const int32_t* b_dev, int64_t n, int64_t pair_capacity,
                               void* workspace_dev, size_t workspace_bytes, void* stream);

int exaspim_label_overlaps_finish(int64_t pair_capacity, void* workspace_dev, size_t workspace_bytes,
                                  int32_t* pairs_dev, int64_t* count_dev,
                                  int32_t* state_dev /* [2]: rows P, overflow */, void* stream);

int exaspim_label_overlaps(const int32_t* a_dev, const int32_t* b_dev, int64_t n, int64_t pair_capacity,
                           int32_t* pairs_dev, int64_t* count_dev, int32_t* state_dev /* [2] */,
                           void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- synthetic input for benchmarks and tests --------------------------- */

/* vol[z,y,x] = splitmix64(seed + global linear index) % 2000 as uint16. */
int exaspim_synth_volume_u16(uint16_t* vol_dev, const exaspim_block* blk,
                             uint64_t seed, void* stream);

/* The neurite-like volume: sparse bright tubes on a dim noise floor, what a percentile-normalised
 * ExaSPIM block looks like (mostly near zero, a few saturated structures). Integer arithmetic only;
 * a pure function of (seed, global coordinate), so every shard writes its own block and
 * utils/synthetic.py:synth_neurite_volume gives the same bits on the host. With g = global (z, y, x):
 *   floor(g) = 8 + splitmix64(seed + global linear index) % 32;
 *   cells c = g >> 5 per axis, h(c) = splitmix64((cz << 42 | cy << 21 | cx) ^
 *     splitmix64(seed ^ 0x6E65757269746573)), independent of the volume's shape;
 *   node(c)[a] = 32 c[a] + 4 + (byte a of h) % 24 for a = 0 (z), 1 (y), 2 (x);
 *   the edge from c to the next cell along axis a exists iff (e & 7) < 3 with e = byte 3 + a of h,
 *     has radius r = 1 + (e >> 3) % 3 and peak = 100 + (b * b * b >> 14), b = byte a of splitmix64(h),
 *     and is the segment A = node(c), B = node(c + e_a);
 *   a voxel p tests the three edges leaving its cell and the three arriving from the cell before it
 *     on each axis: d = B - A, w = p - A, dd = d.d, t = clamp(w.d, 0, dd), n = |w dd - d t|^2;
 *     n <= r^2 dd^2 gives peak, n <= (r + 1)^2 dd^2 gives peak / 2 (rounded down), else 0;
 *   vol[g] = min(65535, floor(g) + the largest of the six).
 * Nodes keep 4 voxels from the cell faces, so a tube and its halo lie inside the two cells it joins. */
int exaspim_synth_volume_neurite_u16(uint16_t* vol_dev, const exaspim_block* blk,
                                     uint64_t seed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EXASPIM_AFFINITY_H */
