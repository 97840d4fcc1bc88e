"""
ctypes binding of the C-ABI HIP extension (include/exaspim_affinity.h).

The product path has no CPU fallback: if the shared library is missing or a
call fails, an exception is raised.
"""

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libexaspim_affinity.so")

DT_F32, DT_BF16, DT_F16 = 0, 1, 2
DT_BF16X3 = 3   # EXASPIM_DT_BF16X3: float32 storage, three bf16 MFMA products per convolution step
VOX_U8, VOX_U16, VOX_I16, VOX_F32, VOX_F64 = 0, 1, 2, 3, 4
IN_F32, IN_PADDED_F32, IN_PADDED_SPLIT_F16, IN_PADDED_SPLIT_BF16 = 0, 1, 2, 3   # EXASPIM_IN_*
UP_CONVT = 0x100   # EXASPIM_UP_CONVT: OR into a dtype code for UNet3D(trilinear=False)
OPT_SEPARATE_POOL, OPT_SEPARATE_DEEP_POOLS, OPT_PLAIN_UPSAMPLE, OPT_FIRST_PER_GROUP = 1, 2, 4, 8   # EXASPIM_OPT_*
OPT_UPSAMPLE_PER_THREAD = 16
OPT_PER_PATCH_ENCODER = 32
OPT_SEPARATE_HEAD = 64   # the head as its own launch, nothing trimmed (bf16x3: same bits)
OPT_ROW_SEPARATE_BORDERS = 256   # row mode: border faces as two thin launches + a column max-pool (same bits)
OPT_CARRY_MAIN_ONLY = 512   # carried planes: the border launch and inc.0 write every plane (same bits)
OPT_CARRY_NO_ROWS = 2048    # carried rows: the y fields are ignored, every row is computed (same bits)
AFF_F32, AFF_F16 = 0, 1   # EXASPIM_AFF_*: element type of exaspim_components' input

DTYPE_CODES = {
    "fp32": DT_F32, "float32": DT_F32, "f32": DT_F32,
    "bf16": DT_BF16, "bfloat16": DT_BF16,
    "fp16": DT_F16, "float16": DT_F16, "f16": DT_F16,
    "bf16x3": DT_BF16X3,
}


class Block(ctypes.Structure):
    """exaspim_block: local dims, global origin and global shape of a block."""

    _fields_ = [
        ("dims", ctypes.c_int32 * 3),
        ("origin", ctypes.c_int32 * 3),
        ("global_", ctypes.c_int32 * 3),
    ]

    @classmethod
    def make(cls, dims, origin=None, global_shape=None):
        origin = (0, 0, 0) if origin is None else origin
        global_shape = dims if global_shape is None else global_shape
        b = cls()
        b.dims[:] = [int(v) for v in dims]
        b.origin[:] = [int(v) for v in origin]
        b.global_[:] = [int(v) for v in global_shape]
        return b


class Window(ctypes.Structure):
    """exaspim_window: patch shape, overlap and trim of the sliding window."""

    _fields_ = [
        ("patch", ctypes.c_int32 * 3),
        ("overlap", ctypes.c_int32 * 3),
        ("trim", ctypes.c_int32),
    ]

    @classmethod
    def make(cls, patch, overlap, trim):
        w = cls()
        w.patch[:] = [int(v) for v in patch]
        w.overlap[:] = [int(v) for v in overlap]
        w.trim = int(trim)
        return w


class ComponentsStreamDesc(ctypes.Structure):
    """exaspim_components_stream: the caller-owned state of a slab-by-slab labelling."""

    _fields_ = [
        ("dims", ctypes.c_int32 * 3),
        ("channels", ctypes.c_int32),
        ("threshold", ctypes.c_float),
        ("capacity", ctypes.c_int32),
        ("min_size", ctypes.c_int64),
        ("next_z", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("id_parent_dev", ctypes.c_void_p),
        ("id_count_dev", ctypes.c_void_p),
        ("table_dev", ctypes.c_void_p),
        ("state_dev", ctypes.c_void_p),
        ("seam_ids_dev", ctypes.c_void_p),
        ("seam_bits_dev", ctypes.c_void_p),
    ]


class WatershedStreamDesc(ctypes.Structure):
    """exaspim_watershed_stream: a components stream, the two thresholds and the carried plane of z affinities."""

    _fields_ = [
        ("base", ComponentsStreamDesc),
        ("low", ctypes.c_float),
        ("high", ctypes.c_float),
        ("seam_aff_dev", ctypes.c_void_p),
    ]


class RegionGraphStreamDesc(ctypes.Structure):
    """exaspim_region_graph_stream: the caller-owned state of a slab-by-slab region graph."""

    _fields_ = [
        ("dims", ctypes.c_int32 * 3),
        ("id_capacity", ctypes.c_int32),
        ("edge_capacity", ctypes.c_int64),
        ("next_z", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("keys_dev", ctypes.c_void_p),
        ("counts_dev", ctypes.c_void_p),
        ("sums_dev", ctypes.c_void_p),
        ("sizes_by_id_dev", ctypes.c_void_p),
        ("seam_ids_dev", ctypes.c_void_p),
        ("seam_q_dev", ctypes.c_void_p),
        ("state_dev", ctypes.c_void_p),
    ]


class UNetCarry(ctypes.Structure):
    """exaspim_unet_carry: the caller's buffers for the first level's skip tensor and its max-pool, the
    plane range already present in them and the range to store for the batch further down z."""

    _fields_ = [
        ("own_skip", ctypes.c_void_p),
        ("own_pool", ctypes.c_void_p),
        ("in_z", ctypes.c_int32 * 2),
        ("out_skip", ctypes.c_void_p),
        ("out_pool", ctypes.c_void_p),
        ("out_z", ctypes.c_int32 * 2),
        ("out_shift", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class UNetCarry1(ctypes.Structure):
    """exaspim_unet_carry1: the same for the second level -- down1.0's output, the level's skip tensor and its
    max-pool, plane ranges in level-1 planes."""

    _fields_ = [
        ("own_mid1", ctypes.c_void_p),
        ("own_skip1", ctypes.c_void_p),
        ("own_pool2", ctypes.c_void_p),
        ("in_z", ctypes.c_int32 * 2),
        ("out_mid1", ctypes.c_void_p),
        ("out_skip1", ctypes.c_void_p),
        ("out_pool2", ctypes.c_void_p),
        ("out_z", ctypes.c_int32 * 2),
        ("out_shift", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class UNetCarryY(ctypes.Structure):
    """exaspim_unet_carry_y: the row range already present in the forward's own buffers, the (skip, pool) of the
    y successor and of the diagonal successor with the rows to store there, and an event to record after inc.3."""

    _fields_ = [
        ("in_y", ctypes.c_int32 * 2),
        ("out_skip_y", ctypes.c_void_p),
        ("out_pool_y", ctypes.c_void_p),
        ("out_skip_d", ctypes.c_void_p),
        ("out_pool_d", ctypes.c_void_p),
        ("out_y", ctypes.c_int32 * 2),
        ("out_shift_y", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("encoder_event", ctypes.c_void_p),
    ]


_lib = None

_I32x5 = ctypes.c_int32 * 5
_I32x3 = ctypes.c_int32 * 3
_vp = ctypes.c_void_p
_sz = ctypes.c_size_t
_i32 = ctypes.c_int32

# name -> (restype, argtypes): every symbol include/exaspim_affinity.h declares
SIGNATURES = {
    "exaspim_abi_version": (_i32, []),
    "exaspim_last_error": (ctypes.c_char_p, []),
    "exaspim_unet_param_count": (_sz, [_I32x5, _i32, _i32]),
    "exaspim_unet_packed_bytes": (_sz, [_I32x5, _i32, _i32]),
    "exaspim_unet_pack_weights": (_i32, [_I32x5, _i32, _i32, _vp, _sz, _vp, _sz]),
    "exaspim_unet_create": (_i32, [_I32x5, _i32, _i32, _i32, _vp, _sz, ctypes.POINTER(_vp)]),
    "exaspim_unet_destroy": (None, [_vp]),
    "exaspim_unet_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32, _i32]),
    "exaspim_unet_forward": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "exaspim_unet_forward_trimmed": (
        _i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]
    ),
    "exaspim_unet_input_layout": (_i32, [_vp]),
    "exaspim_unet_forward_prepared": (
        _i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "exaspim_unet_forward_prepared_row": (
        _i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "exaspim_unet_forward_prepared_clipped": (
        _i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _I32x3, _vp, _sz, _vp]),
    "exaspim_unet_carry_planes": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, ctypes.c_int32 * 2]),
    "exaspim_unet_forward_prepared_carry": (
        _i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _I32x3, ctypes.POINTER(UNetCarry), _vp,
               _sz, _vp]),
    "exaspim_unet_carry1_planes": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, ctypes.c_int32 * 2]),
    "exaspim_unet_forward_prepared_carry1": (
        _i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _I32x3, ctypes.POINTER(UNetCarry),
               ctypes.POINTER(UNetCarry1), _vp, _sz, _vp]),
    "exaspim_unet_carry_rows": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, ctypes.c_int32 * 2]),
    "exaspim_unet_forward_prepared_carry_y": (
        _i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _I32x3, ctypes.POINTER(UNetCarry),
               ctypes.POINTER(UNetCarry1), ctypes.POINTER(UNetCarryY), _vp, _sz, _vp]),
    "exaspim_unet_forward_absmax": (
        _i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _sz, _vp]),
    "exaspim_unet_set_options": (_i32, [_vp, ctypes.c_uint32]),
    "exaspim_unet_timing_begin": (_i32, [_vp, ctypes.c_uint32]),
    "exaspim_unet_timing_read": (_i32, [_vp, ctypes.POINTER(ctypes.c_double * 17),
                                        ctypes.POINTER(ctypes.c_int32 * 17)]),
    "exaspim_histogram": (_i32, [_vp, _i32, _sz, ctypes.c_double, _i32, _i32, ctypes.c_uint32, _vp, _vp]),
    "exaspim_histogram_wide": (_i32, [_vp, _i32, _sz, ctypes.c_double, _i32, _i32, ctypes.c_uint64, _vp, _vp]),
    "exaspim_gather_patches": (_i32, [_vp, _i32, ctypes.POINTER(Block), _vp, _i32, _I32x3,
                                      ctypes.c_double, _i32, ctypes.c_double, ctypes.c_double, _vp, _vp]),
    "exaspim_gather_patches_as": (_i32, [_vp, _i32, ctypes.POINTER(Block), _vp, _i32, _I32x3,
                                         ctypes.c_double, _i32, ctypes.c_double, ctypes.c_double, _i32,
                                         _vp, _vp]),
    "exaspim_stitch_accumulate": (_i32, [_vp, _vp, _i32, _i32, ctypes.POINTER(Window), _vp,
                                         ctypes.POINTER(Block), _vp]),
    "exaspim_stitch_finalize": (_i32, [_vp, _i32, ctypes.POINTER(Window), ctypes.POINTER(Block), _vp]),
    "exaspim_export_f16": (_i32, [_vp, _vp, ctypes.c_size_t, _vp]),
    "exaspim_components_workspace_bytes": (_sz, [_I32x3]),
    "exaspim_components": (_i32, [_vp, _i32, _i32, _I32x3, ctypes.c_float, ctypes.c_int64, _vp, _vp, _vp,
                                  _sz, _vp]),
    "exaspim_components_stream_slab_workspace_bytes": (_sz, [_I32x3]),
    "exaspim_components_stream_finish_workspace_bytes": (_sz, [_i32]),
    "exaspim_components_stream_slab": (_i32, [ctypes.POINTER(ComponentsStreamDesc), _vp, _i32, _I32x3, _i32, _vp,
                                              _vp, _sz, _vp]),
    "exaspim_components_stream_finish": (_i32, [ctypes.POINTER(ComponentsStreamDesc), _vp, _sz, _vp]),
    "exaspim_components_stream_apply": (_i32, [ctypes.POINTER(ComponentsStreamDesc), _vp, _sz, _vp]),
    "exaspim_region_graph_workspace_bytes": (_sz, [_I32x3, _i32, ctypes.c_int64]),
    "exaspim_region_graph": (_i32, [_vp, _vp, _i32, _I32x3, _i32, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _sz, _vp]),
    "exaspim_region_graph_stream_slab": (_i32, [ctypes.POINTER(RegionGraphStreamDesc), _vp, _vp, _i32, _I32x3, _i32,
                                                _vp]),
    "exaspim_region_graph_stream_finish_workspace_bytes": (_sz, [ctypes.c_int64]),
    "exaspim_region_graph_stream_finish": (_i32, [ctypes.POINTER(RegionGraphStreamDesc), _vp, _i32, _i32, _vp, _vp,
                                                  _vp, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_agglomerate": (_i32, [_vp, _vp, _vp, ctypes.c_int64, _vp, _i32, ctypes.c_float, ctypes.c_int64,
                                   _vp, _vp]),
    "exaspim_apply_label_table": (_i32, [_vp, _sz, _vp, _i32, _vp]),
    "exaspim_region_graph_premerge_workspace_bytes": (_sz, [_i32, ctypes.c_int64]),
    "exaspim_region_graph_premerge": (_i32, [_vp, _vp, _vp, _vp, ctypes.c_int64, _i32, ctypes.c_float,
                                             ctypes.c_int64, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                             _sz, _vp]),
    "exaspim_region_graph_contract_dominant_workspace_bytes": (_sz, [_i32, ctypes.c_int64]),
    "exaspim_region_graph_contract_dominant": (_i32, [_vp, _vp, _vp, _vp, ctypes.c_int64, _i32, ctypes.c_float,
                                                      ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_watershed_workspace_bytes": (_sz, [_I32x3]),
    "exaspim_watershed_fragments": (_i32, [_vp, _i32, _I32x3, ctypes.c_float, ctypes.c_float, ctypes.c_int64, _vp,
                                           _vp, _vp, _sz, _vp]),
    "exaspim_watershed_stream_slab_workspace_bytes": (_sz, [_I32x3]),
    "exaspim_watershed_stream_slab": (_i32, [ctypes.POINTER(WatershedStreamDesc), _vp, _i32, _I32x3, _i32, _vp,
                                             _vp, _sz, _vp]),
    "exaspim_dbf_workspace_bytes": (_sz, [_I32x3]),
    "exaspim_dbf": (_i32, [_vp, _I32x3, _i32, _vp, _vp, _sz, _vp]),
    "exaspim_segment_table_workspace_bytes": (_sz, [_i32]),
    "exaspim_segment_table": (_i32, [_vp, _vp, _I32x3, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_fill_holes_workspace_bytes": (_sz, [_I32x3]),
    "exaspim_fill_holes": (_i32, [_vp, _I32x3, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_geodesic_workspace_bytes": (_sz, [_I32x3]),
    "exaspim_geodesic_begin": (_i32, [_vp, _I32x3, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_geodesic_sweeps": (_i32, [_vp, _vp, _I32x3, _i32, _vp, _i32, _vp, _vp, _sz, _vp]),
    "exaspim_geodesic_farthest_workspace_bytes": (_sz, [_i32]),
    "exaspim_geodesic_farthest": (_i32, [_vp, _vp, _I32x3, _i32, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_geodesic_parents_begin": (_i32, [_vp, _I32x3, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_geodesic_parents_sweeps": (_i32, [_vp, _vp, _vp, _I32x3, _i32, _vp, _i32, _vp, _vp, _sz, _vp]),
    "exaspim_geodesic_parents_finish": (_i32, [_vp, _vp, _vp, _vp, _I32x3, _i32, _vp, _vp, _vp]),
    "exaspim_geodesic_reseed": (_i32, [_vp, _I32x3, _i32, _vp, ctypes.c_int64, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_geodesic_parents_begin_seeds": (_i32, [_vp, _I32x3, _i32, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _sz,
                                                    _vp]),
    "exaspim_trace_paths": (_i32, [_vp, _vp, _I32x3, _vp, _i32, _vp, _vp, ctypes.c_int64, _vp, _vp]),
    "exaspim_teasar_workspace_bytes": (_sz, [_I32x3, _i32]),
    "exaspim_teasar_begin": (_i32, [_vp, _vp, _vp, _vp, _I32x3, _i32, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_teasar_round": (_i32, [_vp, _vp, _vp, _vp, _I32x3, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_teasar_round_given": (_i32, [_vp, _vp, _vp, _vp, _I32x3, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                          _vp]),
    "exaspim_teasar_apply": (_i32, [_vp, _vp, _vp, _vp, _I32x3, _i32, ctypes.c_double, ctypes.c_double, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, _i32, _vp, _vp]),
    "exaspim_border_targets_workspace_bytes": (_sz, [_I32x3]),
    "exaspim_border_targets": (_i32, [_vp, _I32x3, _i32, _vp, _vp, _i32, _vp, _vp, _sz, _vp]),
    "exaspim_label_pieces_workspace_bytes": (_sz, [_I32x3]),
    "exaspim_label_pieces": (_i32, [_vp, _I32x3, _i32, ctypes.c_int64, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_label_pieces_open_workspace_bytes": (_sz, [_I32x3]),
    "exaspim_label_pieces_open": (_i32, [_vp, _I32x3, _i32, ctypes.c_int64, ctypes.c_uint32, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_label_overlaps_workspace_bytes": (_sz, [ctypes.c_int64]),
    "exaspim_label_overlaps_reset": (_i32, [ctypes.c_int64, _vp, _sz, _vp]),
    "exaspim_label_overlaps_add": (_i32, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, _vp, _sz, _vp]),
    "exaspim_label_overlaps_finish": (_i32, [ctypes.c_int64, _vp, _sz, _vp, _vp, _vp, _vp]),
    "exaspim_label_overlaps": (_i32, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "exaspim_synth_volume_u16": (_i32, [_vp, ctypes.POINTER(Block), ctypes.c_uint64, _vp]),
    "exaspim_synth_volume_neurite_u16": (_i32, [_vp, ctypes.POINTER(Block), ctypes.c_uint64, _vp]),
}


def lib():
    """
    Loads (once) and returns the shared library with typed signatures.

    Raises
    ------
    RuntimeError
        If the extension has not been built.
    """
    global _lib
    if _lib is None:
        path = LIB_PATH
        # measurement aid (tools/ab_lib.sh): A/B another build of the same ABI without copying it
        # over the product library; never silent
        override = os.environ.get("EXASPIM_LIB")
        if override:
            import sys

            path = os.path.abspath(override)
            print(f"exaspim: EXASPIM_LIB is set, loading {path} instead of the in-tree library",
                  file=sys.stderr)
        if not os.path.exists(path):
            raise RuntimeError(
                f"HIP extension not built: {path} is missing. Build it with "
                "`make -C aind_exaspim_neuron_segmentation_amd/csrc` (or "
                "`python -c 'import __graft_entry__ as g; g.build()'`). "
                "There is no CPU fallback."
            )
        # torch first: its wheel ships a HIP runtime of its own, which this library then binds to by soname. Loaded
        # the other way round the process holds two runtimes -- the system's for this library, torch's for the
        # tensors -- and the kernels here fail with "no ROCm-capable device is detected"
        import torch  # noqa: F401

        handle = ctypes.CDLL(path)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


def last_error():
    """Returns the library's thread-local error message."""
    msg = lib().exaspim_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc, what):
    """
    Raises the Python exception matching a C-ABI error code.
    """
    if rc == 0:
        return
    msg = f"{what}: {last_error()} (code {rc})"
    if rc == -1:
        raise ValueError(msg)
    raise RuntimeError(msg)


def channels_array(channels):
    """Converts the five level widths to the int32[5] the ABI takes."""
    if len(channels) != 5:
        raise ValueError("expected five channel widths")
    return _I32x5(*[int(c) for c in channels])


def int3(values):
    """Converts a 3-tuple to int32[3]."""
    return _I32x3(*[int(v) for v in values])
