"""
MI355X-native drop-in for the prediction section of the reference's
``inference.py`` (predict: 29-126, _predict_batch: 129-163,
_get_batch_inputs: 166-192, count_patches: 340-365, generate_patch_starts:
368-397, load_model: 400-424, to_tensor: 427-446).

Same function names, positional order, keyword names and defaults; extra
options are trailing keyword arguments. What differs is where the work runs:

* the volume is uploaded once and stays in HBM; brightness clip, percentile
  normalisation, patch extraction with reflect padding and the float32 cast
  happen in one HIP gather kernel per batch (exact float64 arithmetic, so the
  network sees bit-identical inputs);
* the two percentiles come from a device histogram (exact order statistics ->
  numpy's interpolation on the host);
* the U-Net runs on the hand-written gfx950 kernels behind ``UNet3D``;
* sigmoid, trimming, overlap-add and the final division happen on the device;
* the sliding window is z-major (inference.py:368-397), so an output slab is final
  one patch layer after the last patch touching it: finished slabs are divided,
  copied to pinned memory on a copy stream and moved into the result by a few host
  threads while the next layer computes (predict_streaming; predict() of a host
  array is that pipeline over the array).

What lives here: predict, the sliding-window plan and its carry schedule, the
percentiles, the slab pipeline, predict_streaming, and the two drivers that
label slabs as the pipeline finishes them (predict_components_streaming,
predict_agglomerate_streaming). Everything that starts from finished
affinities -- components, watershed fragments, the region graph, pre-merge,
agglomeration, ComponentsStream, RegionGraphStream, the drivers for
affinities on the host, and the distance-to-boundary field and segment
table of finished labels -- lives in segmentation.py; those names are imported
below, so each is reachable as inference.NAME as before and is the same
object. The plan switches below are read by this module only.

There is no CPU fallback: a model on a CPU device raises.
"""

import collections
import itertools
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from aind_exaspim_neuron_segmentation_amd import _native
from aind_exaspim_neuron_segmentation_amd._device import _carrier, _stream
from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D
from aind_exaspim_neuron_segmentation_amd.segmentation import (  # noqa: F401  (importable from here as before)
    DBF_INF, DEFAULT_EDGE_CAPACITY, DEFAULT_ID_CAPACITY, FIX_BRANCHING_FIELD_SWEEPS, MAX_TOTAL_COUNT, ComponentsStream,
    RegionGraphStream, WatershedStream, _checked_fragment_options, _fragment_stream, watershed_fragments_streaming,
    _AgglomerationLabeller, _border_targets_on_device, _ComponentsLabeller, _components_on_device,
    _contract_dominant_on_device,
    _default_edge_capacity, _device_merged_table, _fill_holes_on_device, _fix_branching_on_device,
    _geodesic_on_device, _geodesic_parents_on_device, _geodesic_seeded_on_device, _label_pieces_on_device,
    _label_pieces_open_on_device, _LabelSink, join_block_skeletons, label_pieces_open, skeletonize_blocks,
    _last_threshold,
    _premerge_on_device, _premerged_table, _region_graph_device, _skeleton_chain_on_device, _teasar_on_device,
    _watershed_on_device, affinities_to_components, affinities_to_components_streaming, agglomerate,
    agglomerate_affinities, agglomerate_affinities_streaming, border_targets, contract_dominant_edges,
    distance_to_boundary,
    fill_holes, label_pieces, geodesic_field, geodesic_field_seeded, geodesic_parents, geodesic_parents_seeded,
    premerge_region_graph, region_graph, segment_table, segmentation_to_zipped_swcs, skeleton_to_swc, skeletonize,
    skeletonize_fix_borders, skeletonize_labels, skeletonize_pieces, skeletons_to_zipped_swcs, teasar_branches,
    teasar_branches_fix_branching, teasar_branches_fix_branching_given, teasar_branches_given, trace_paths,
    voxelize_skeletons, watershed_fragments,
    DEFAULT_PAIR_CAPACITY, OverlapStream, compare_segmentations, label_overlaps, label_overlaps_streaming,
    overlap_scores,
)
from aind_exaspim_neuron_segmentation_amd.utils import img_util

try:  # progress bar is cosmetic; the reference imports tqdm unconditionally
    from tqdm import tqdm
except ImportError:  # pragma: no cover
    tqdm = None

# Batches in flight on separate HIP streams in predict() / predict_streaming(): measured on MI355X
# (1024^3, fp16, batch 16) three are 5 % faster than one -- one kernel's last, partly idle round of
# workgroups overlaps another batch's work -- and the result does not change by a bit (stitching
# stays in batch order on the caller's stream).
DEFAULT_STREAMS = 3
# Switches between bit-identical (PLAIN_GATHER) or superset (FULL_PATCHES) execution plans, for the tests that
# hold the plans to each other and for measurements; module attributes, not environment variables, so nothing
# outside the calling code can flip them.
PLAIN_GATHER = False    # True: gather float32 patches and let the engine pad them, instead of the prepared layout
FULL_PATCHES = False    # True: compute the margin predict() discards as well (exaspim_unet_forward untrimmed)
CARRY_Z = True          # False: every batch computes its whole first level (no planes carried from the z slab above)
CARRY_Z1 = True         # False: only the first level carries planes (down1.0 and down1.3 are computed whole)
# (not a CARRY_ name: the switches of that prefix are a closed list, tests/test_module_surface_cpu.py)
ROWS_CARRY_Y = True     # False: no rows carried from the batch one y step earlier (section 3g); off wherever CARRY_Z is off
CARRY_POOL_BYTES = 36 << 30   # most device memory one run_sliding_window call may hold in carry buffers
CLIP_TO_VOLUME = True   # False: also compute the trimmed outputs beyond the volume's high faces, which the stitch drops

_VOX_CODES = {
    np.dtype(np.uint8): _native.VOX_U8,
    np.dtype(np.uint16): _native.VOX_U16,
    np.dtype(np.int16): _native.VOX_I16,
    np.dtype(np.float32): _native.VOX_F32,
    np.dtype(np.float64): _native.VOX_F64,
}
_TORCH_VOXELS = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16,
                 np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32,
                 np.dtype(np.float64): torch.float64}


# --- Model Predictions ---
def predict(
    img,
    model,
    affinity_mode=True,
    batch_size=16,
    brightness_clip=1000,
    normalization_percentiles=(1, 99.9),
    patch_shape=(96, 96, 96),
    overlap=(32, 32, 32),
    trim=8,
    verbose=True,
    *,
    return_device_tensor=False,
    n_streams=DEFAULT_STREAMS,
    out_dtype=np.float32,
):
    """
    Predicts affinities or foreground-background maps for a 3D image by
    splitting it into overlapping patches, batching the patches, and
    processing each batch with the model.

    Parameters
    ----------
    img : numpy.ndarray
        Input 3D image with shape (D, H, W), (1, D, H, W) or (1, 1, D, H, W).
        A torch tensor already on the model's device is accepted too.
    model : torch.nn.Module
        Model used for prediction (normally from "load_model"); it must live
        on a HIP device.
    affinity_mode : bool, optional
        If True, the model predicts affinities; if False, it predicts
        foreground-background. Default is True.
    batch_size : int, optional
        Number of patches to process in a batch. Default is 16.
    brightness_clip : float, optional
        Maximum brightness value for voxel intensities. Default is 1000.
    normalization_percentiles : Tuple[int], optional
        Lower and upper percentiles used for normalization. Default is
        (1, 99.9).
    patch_shape : Tuple[int], optional
        Shape of 3D patch expected by the model. Default is (96, 96, 96).
    overlap : Tuple[int], optional
        Shape of overlap between patches along each dimension. Default is
        (32, 32, 32).
    trim : int, optional
        Number of voxels to trim from the edges of each patch in the output.
        Default is 8.
    verbose : bool, optional
        Indication of whether to show a tqdm progress bar. Default is True.
    return_device_tensor : bool, optional
        Return the result as a torch tensor on the device instead of copying
        it to a numpy array (the whole accumulator then stays in HBM). Default
        is False: finished z-slabs are downloaded while later patch layers
        compute (see predict_streaming).
    n_streams : int, optional
        Batches in flight on separate HIP streams (see run_sliding_window);
        the result does not depend on it. Default is 3 (DEFAULT_STREAMS).
    out_dtype : numpy.dtype, optional
        numpy.float32 (default, the reference's) or numpy.float16: the
        finished result rounded to IEEE half on the device (round to nearest
        even, error at most 2.4e-4 on values in [0, 1]) before it leaves it --
        half the download and half the host memory. The consumer,
        affinities_to_segmentation, starts with astype(np.float32)
        (inference.py:223) and takes such an array as it is.

    Returns
    -------
    pred : numpy.ndarray
        Prediction generated by the given model applied to an image: float32
        (3, D, H, W), or (D, H, W) if "affinity_mode" is False.
    """
    out_dtype = _checked_out_dtype(out_dtype)
    device = _hip_device(model)
    if not return_device_tensor and not isinstance(img, (DeviceVolume, torch.Tensor)):
        # host array in, host array out: slab pipeline with overlapped transfers
        return predict_streaming(
            img, model, affinity_mode=affinity_mode, batch_size=batch_size,
            brightness_clip=brightness_clip, normalization_percentiles=normalization_percentiles,
            patch_shape=patch_shape, overlap=overlap, trim=trim, verbose=verbose,
            n_streams=n_streams, out_dtype=out_dtype,
        )
    volume = DeviceVolume.from_array(img, device, clip=brightness_clip)
    plan = SlidingWindow(volume.shape, patch_shape, overlap, trim)
    n_channels = 3 if affinity_mode else 1
    with torch.cuda.device(device):
        mn, mx = volume_percentiles(volume, brightness_clip, normalization_percentiles)
        accum = run_sliding_window(
            volume, model, plan, n_channels, batch_size, brightness_clip, mn, mx,
            verbose=verbose, n_streams=n_streams,
        )
        stitch_finalize(accum, plan, volume.block)
        if out_dtype == np.float16:
            accum = export_half(accum)
    pred = accum if affinity_mode else accum[0]
    if return_device_tensor:
        return pred
    return pred.cpu().numpy()


def _checked_out_dtype(out_dtype):
    out_dtype = np.dtype(out_dtype)
    if out_dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise TypeError(f"out_dtype must be numpy.float32 or numpy.float16, got {out_dtype}")
    return out_dtype


def export_half(tensor, out=None):
    """
    Rounds a finalised float32 device tensor to IEEE half (round to nearest
    even, numpy's astype(float16)) with the library's export kernel.

    Parameters
    ----------
    tensor : torch.Tensor
        Contiguous float32 tensor on a HIP device.
    out : torch.Tensor, optional
        Contiguous float16 tensor with as many elements to write into.

    Returns
    -------
    torch.Tensor
        float16 tensor of the same shape.
    """
    if tensor.dtype != torch.float32 or not tensor.is_contiguous():
        raise ValueError("export_half needs a contiguous float32 tensor")
    if out is None:
        out = torch.empty(tensor.shape, dtype=torch.float16, device=tensor.device)
    elif out.dtype != torch.float16 or not out.is_contiguous() or out.numel() != tensor.numel():
        raise ValueError("export_half: out must be a contiguous float16 tensor of the same size")
    _native.check(
        _native.lib().exaspim_export_f16(tensor.data_ptr(), out.data_ptr(), tensor.numel(),
                                         _stream(tensor.device)),
        "exaspim_export_f16",
    )
    return out.view(tensor.shape)


def _predict_batch(img, model, starts, patch_shape, trim=8, *, clip=None, mn=0.0, mx=1.0):
    """
    Extracts a batch of 3D patches from a device-resident volume, runs them
    through the model and returns sigmoid predictions, trimmed if requested
    (inference.py:129-163 of the reference; there "img" is the normalised
    float64 volume, here normalisation is fused into the extraction).

    Parameters
    ----------
    img : DeviceVolume
        Volume in device memory.
    model : torch.nn.Module
        Model used for prediction.
    starts : List[Tuple[int]]
        Starting coordinates (z, y, x) of the patches.
    patch_shape : Tuple[int]
        Shape of 3D patch expected by the model.
    trim : int, optional
        Number of voxels trimmed from each side of the outputs. Default is 8.

    Returns
    -------
    torch.Tensor
        Device tensor (B, C, d, h, w) of predictions.
    """
    device = next(model.parameters()).device
    starts_dev = torch.tensor(list(starts), dtype=torch.int32, device=device).reshape(-1, 3)
    inputs = _get_batch_inputs(img, starts_dev, patch_shape, device, clip=clip, mn=mn, mx=mx)
    outputs = _model_probabilities(model, inputs, trim)
    if trim > 0:
        outputs = outputs[..., trim:-trim, trim:-trim, trim:-trim]
    return outputs


def _get_batch_inputs(img, starts, patch_shape, device, *, clip=None, mn=0.0, mx=1.0, out=None,
                      layout=_native.IN_F32):
    """
    Builds the (B, 1, *patch_shape) float32 network input for a batch of patch
    starts with the HIP gather kernel: brightness clip, normalisation, clip to
    [0, 1], in-volume slicing, high-side reflect padding and the float32 cast
    (inference.py:166-192, img_util.py:362-379, 405-428, 504-533).

    Parameters
    ----------
    img : DeviceVolume
        Volume in device memory.
    starts : torch.Tensor
        int32 device tensor (B, 3) of global patch starts.
    patch_shape : Tuple[int]
        Shape of the 3D patch expected by the model.
    device : torch.device
        Device of the result.
    layout : int, optional
        _native.IN_F32 (default: the reference's float32 batch) or the operand
        layout of a UNet3D's first convolution (UNet3D.input_layout(): the same
        values with a one-voxel zero border, split into 16-bit parts for the
        16-bit engines), which UNet3D.run_prepared takes.

    Returns
    -------
    torch.Tensor
        Float32 device tensor (B, 1, *patch_shape), or for a prepared layout a
        4-byte-per-voxel tensor (B, patch_shape[0] + 2, patch_shape[1] + 2,
        patch_shape[2] + 2).
    """
    n = int(starts.shape[0])
    border = 0 if layout == _native.IN_F32 else 2
    if out is None:
        shape = (n, 1) + tuple(patch_shape) if border == 0 else (n,) + tuple(int(p) + 2 for p in patch_shape)
        out = torch.empty(shape, dtype=torch.float32, device=device)
    has_clip = clip is not None
    denom = float(np.float64(mx) - np.float64(mn) + 1e-8)  # img_util.py:527
    # one launch takes n * (padded) patch depth <= 65535 grid rows: very large batches of
    # small patches go in pieces
    piece = max(1, 65535 // (int(patch_shape[0]) + border))
    for i in range(0, n, piece):
        m = min(piece, n - i)
        _native.check(
            _native.lib().exaspim_gather_patches_as(
                img.tensor.data_ptr(), img.vox_code, img.block, starts[i:i + m].data_ptr(), m,
                _native.int3(patch_shape), float(clip) if has_clip else 0.0,
                1 if has_clip else 0, float(mn), denom, int(layout), out[i:i + m].data_ptr(),
                _stream(device),
            ),
            "exaspim_gather_patches_as",
        )
    return out


# --- Helpers ---
def count_patches(img_shape, patch_shape, overlap):
    """
    Counts the number of patches within a 3D image for a given patch shape
    and overlap between the patches.

    Parameters
    ----------
    img_shape : Tuple[int]
        Shape (batch, channels, depth, height, width) of the image.
    patch_shape : Tuple[int]
        Shape of the 3D patch expected by the model.
    overlap : Tuple[int]
        Number of voxels in overlap between patches along each dimension.

    Returns
    -------
    int
        Number of patches.
    """
    assert len(img_shape) == 5, "Image must have shape (1, 1, D, H, W)"
    total = 1
    for axis_range in _start_ranges(img_shape[2:], patch_shape, overlap):
        total *= len(axis_range)
    return total


def generate_patch_starts(img_shape, patch_shape, overlap):
    """
    Generates starting coordinates for 3D patches extracted from an image
    tensor, based on specified patch size and overlap (z outermost, x
    fastest).

    Parameters
    ----------
    img_shape : Tuple[int]
        Shape (batch, channels, depth, height, width) of the image.
    patch_shape : Tuple[int]
        Shape of the 3D patch expected by the model.
    overlap : Tuple[int]
        Number of voxels in overlap between patches along each dimension.

    Returns
    -------
    Iterator[Tuple[int]]
        Starting coordinates of the image patches.
    """
    assert len(img_shape) == 5, "Image must have shape (1, 1, D, H, W)"
    yield from itertools.product(*_start_ranges(img_shape[2:], patch_shape, overlap))


def load_model(path, affinity_mode=True, device="cuda", *, compute_dtype="fp32"):
    """
    Loads a pretrained UNet model from a file.

    Parameters
    ----------
    path : str
        Path to the saved model weights (a state_dict written by the
        reference's trainer, train.py:286).
    affinity_mode : bool, optional
        If True, the model predicts affinities; if False, it predicts
        foreground-background. Default is True.
    device : str, optional
        Device to load the model onto. Default is "cuda" (the HIP device).
    compute_dtype : str, optional
        "fp32" (default), "bf16" or "fp16" arithmetic of the network kernels,
        "bf16x3" (float32 activations, each 3x3x3 convolution as three bf16
        matrix-core products of split operands: float32 range, probabilities
        within about 4e-6 of the reference's; see UNet3D), or
        "auto": fp16 if this checkpoint, on the first batch of patches predict()
        gives it, stays inside half range and within 1e-3 of its own float32
        probabilities, float32 otherwise (UNet3D.resolve_compute_dtype).

    Returns
    -------
    model : torch.nn.Module
        UNet model loaded with weights and set to evaluation mode.
    """
    output_channels = 3 if affinity_mode else 1
    model = UNet3D(output_channels=output_channels, compute_dtype=compute_dtype)
    state = torch.load(path, map_location=device, weights_only=True)
    model.load_state_dict(state)
    model.to(device)
    model.eval()
    return model


def to_tensor(arr, device="cuda"):
    """
    Converts a NumPy array to a float32 PyTorch tensor on a device, adding a
    channel axis until the array is 5-D.

    Parameters
    ----------
    arr : numpy.ndarray
        Array to be converted.
    device : str, optional
        Device to move the array to. Default is "cuda".

    Returns
    -------
    torch.Tensor
        Tensor on the device.
    """
    while arr.ndim < 5:
        arr = arr[:, np.newaxis, ...]
    return torch.tensor(arr).to(device, dtype=torch.float32)


# --- device-side building blocks (used by predict and by sharding.py) ---
class DeviceVolume:
    """
    A (block of a) 3D volume in device memory plus its place in the global
    volume.

    Attributes
    ----------
    tensor : torch.Tensor
        Device tensor of shape (D, H, W) (uint8, int16 holding uint16/int16
        bits, or float32).
    np_dtype : numpy.dtype
        Voxel dtype of the image as numpy sees it (what np.minimum and
        np.percentile of the reference operate on).
    storage_dtype : numpy.dtype
        Dtype the voxels have in device memory (uint8, uint16, int16, float32 or
        float64; wider integers and float64 travel as float32 when every value is
        known to be exactly representable, as float64 otherwise).
    block : _native.Block
        Local dims / global origin / global shape.
    """

    def __init__(self, tensor, np_dtype, origin=None, global_shape=None, storage_dtype=None):
        np_dtype = np.dtype(np_dtype)
        storage = np.dtype(storage_dtype) if storage_dtype is not None else _device_voxel_dtype(np_dtype)[0]
        if storage not in _VOX_CODES:
            raise TypeError(_unsupported(np_dtype))
        if tensor.dim() != 3 or not tensor.is_cuda:
            raise ValueError("DeviceVolume expects a 3-D tensor on a HIP device")
        if tensor.element_size() != storage.itemsize:
            raise ValueError("tensor element size does not match the voxel dtype")
        self.tensor = tensor.contiguous()
        self.np_dtype = np_dtype
        self.storage_dtype = storage
        self.vox_code = _VOX_CODES[storage]
        self.shape = tuple(int(v) for v in (global_shape or tensor.shape))
        self.block = _native.Block.make(tuple(tensor.shape), origin, self.shape)

    @classmethod
    def from_array(cls, img, device, clip=None):
        """Uploads a numpy array (3-D to 5-D, leading axes of length 1); "clip" is the
        brightness clip it will be used with (it can decide how wide integers and float64
        voxels travel, see _device_voxel_dtype)."""
        if isinstance(img, DeviceVolume):
            return img
        if isinstance(img, torch.Tensor):
            t = img
            while t.dim() > 3:
                if t.shape[0] != 1:
                    raise ValueError("leading image axes must have length 1")
                t = t[0]
            np_dtype = {
                torch.uint8: np.uint8, torch.int16: np.int16, torch.float32: np.float32,
                torch.float64: np.float64, getattr(torch, "uint16", None): np.uint16,
            }.get(t.dtype)
            if np_dtype is None:
                raise TypeError(f"tensor dtype {t.dtype} not supported")
            return cls(t.to(device), np_dtype)
        arr = np.asarray(img)
        while arr.ndim > 3:
            if arr.shape[0] != 1:
                raise ValueError("leading image axes must have length 1")
            arr = arr[0]
        if arr.ndim != 3:
            raise ValueError(f"expected a 3-D image, got shape {np.shape(img)}")
        storage, convert = _device_voxel_dtype(arr.dtype, whole=arr, clip=clip)
        if storage not in _VOX_CODES:
            raise TypeError(_unsupported(arr.dtype))
        return cls(_carrier(convert(arr)).to(device), arr.dtype, storage_dtype=storage)


def _unsupported(np_dtype):
    return (f"voxel dtype {np_dtype} not supported (8-, 16-, 32- and 64-bit integers, float32 and "
            "float64 are; 64-bit integers must be exactly representable in float64)")


class SlidingWindow:
    """
    Geometry of predict()'s sliding window over a volume of "shape".
    """

    def __init__(self, shape, patch_shape, overlap, trim):
        self.shape = tuple(int(v) for v in shape)
        self.patch_shape = tuple(int(v) for v in patch_shape)
        self.overlap = tuple(int(v) for v in overlap)
        self.trim = int(trim)
        if len(self.patch_shape) != 3 or len(self.overlap) != 3:
            raise ValueError("patch_shape and overlap must have three entries")
        if any(o >= p or o < 0 for o, p in zip(self.overlap, self.patch_shape)):
            raise ValueError("overlap must be in [0, patch_shape)")
        if self.trim < 0 or any(2 * self.trim >= p for p in self.patch_shape):
            raise ValueError("trim must satisfy 0 <= 2 * trim < patch_shape")
        self.window = _native.Window.make(self.patch_shape, self.overlap, self.trim)
        self.shape5 = (1, 1) + self.shape
        # The reference's stitch loop (inference.py:101-116) places a trimmed patch with
        # accum[s:e] += patch[:e - s], s = start + trim, e = min(s + out, dim). With
        # trim > overlap + 1 the last starts of an axis can have s > dim: e - s is negative,
        # patch[:e - s] is not empty while accum[s:e] is, and numpy raises. Same geometry,
        # same exception -- before any work is queued instead of half-way through.
        n_starts = [len(range(0, d - ov, ps - ov))
                    for d, ps, ov in zip(self.shape, self.patch_shape, self.overlap)]
        if self.trim > 0 and len(self.shape) == 3 and all(n_starts):   # no patch, no loop, no error
            for axis, (d, ps, ov) in enumerate(zip(self.shape, self.patch_shape, self.overlap)):
                out = ps - 2 * self.trim
                for s0 in reversed(range(0, d - ov, ps - ov)):
                    if s0 + self.trim <= d:
                        break
                    if s0 + self.trim < d + out:
                        raise ValueError(
                            "operands could not be broadcast together: the patch starting at "
                            f"{s0} on axis {axis} begins {s0 + self.trim - d} voxel(s) past the "
                            f"image (size {d}) after trimming {self.trim}; the reference's stitch "
                            "loop fails on this geometry (trim > overlap + 1)"
                        )

    def starts(self):
        """All patch starts in the reference's order."""
        return list(generate_patch_starts(self.shape5, self.patch_shape, self.overlap))


def batch_row_stride(starts, patch_shape, overlap):
    """
    x stride of a batch of patch starts that is one row along x -- at least two
    patches, the same (z, y), consecutive x starts exactly patch - overlap apart --
    else 0 (UNet3D.run_prepared's row_stride). Host-side, no device sync.
    """
    stride = int(patch_shape[2]) - int(overlap[2])
    if len(starts) < 2 or stride <= 0:
        return 0
    z0, y0, x0 = (int(v) for v in starts[0])
    for i, s in enumerate(starts):
        z, y, x = (int(v) for v in s)
        if z != z0 or y != y0 or x != x0 + i * stride:
            return 0
    return stride


def carry_plan(starts, batch_size, patch_shape, overlap, axis=0):
    """
    For every batch of the sliding window (starts cut into runs of batch_size), the index of the later
    batch that can take first-level planes over from it, or None: the nearest later batch whose starts are
    this batch's shifted by one positive z amount below the patch depth, with the same number of patches,
    both of them rows along x of the same stride (batch_row_stride). Host-side, no device sync.
    axis=1: the same along y -- the batch that can take rows over (same x and z starts, one positive y amount
    below the patch height).
    """
    batch_size = int(batch_size)
    axis = int(axis)
    other = 1 - axis
    batches = [starts[i:i + batch_size] for i in range(0, len(starts), batch_size)]
    chains = {}     # (row stride, the row's starts on the other axis and x) -> [(start on the axis, batch index)]
    for bi, b in enumerate(batches):
        stride = batch_row_stride(b, patch_shape, overlap)
        if stride > 0:
            key = (stride, tuple((int(s[other]), int(s[2])) for s in b))
            chains.setdefault(key, []).append((int(b[0][axis]), bi))
    succ = [None] * len(batches)
    depth = int(patch_shape[axis])
    for members in chains.values():
        for z, bi in members:
            later = [(z2 - z, bj) for z2, bj in members if bj > bi and 0 < z2 - z < depth]
            if later:
                succ[bi] = min(later)[1]
    return succ


def _carry_budget(peak, pair_bytes, triple_bytes, free, cap):
    """
    (level 0, level 1): which of the two levels' carry buffers fit, peak sets of each. The first level is
    budgeted first, under the cap and half of the free memory; the second level (triple_bytes = 0: nothing to
    carry there) is taken only with the first and only if what is left of both bounds holds it.
    """
    limit = min(int(cap), int(free) // 2)
    need0 = peak * pair_bytes
    if peak <= 0 or need0 > limit:
        return False, False
    return True, triple_bytes > 0 and need0 + peak * triple_bytes <= limit


def _carry_rows_span(h, shift_y):
    """exaspim_unet_carry_rows for a batch that runs in row mode: the whole 8-row tiles inside
    [2, h - shift_y - 2) of the later frame, (0, 0) if there is none. Host-side arithmetic, so that the schedule
    is the same for every model that gives the same plane ranges; the engine refuses any other range."""
    h, shift_y = int(h), int(shift_y)
    if shift_y <= 0 or shift_y % 2 or shift_y >= h:
        return (0, 0)
    hi = (h - shift_y - 2) // 8 * 8
    return (8, hi) if hi > 8 else (0, 0)


_ROWS_SCHEDULES = collections.OrderedDict()     # the last few y schedules: a pure function of the window plan


def _carry_rows_schedule(links, starts, batch_size, patch_shape, overlap):
    """_plan_rows, remembered for the last few window plans: a volume's slabs, and one volume after the other,
    ask for the same plan again, and the planning is host time in front of the first launch."""
    if not ROWS_CARRY_Y or not any(links):
        return [None] * len(links), None
    try:
        key = (tuple(starts), tuple(links), int(batch_size), tuple(patch_shape), tuple(overlap))
        hit = _ROWS_SCHEDULES.get(key)
    except TypeError:       # (starts that do not hash: plan afresh)
        key, hit = None, None
    if hit is None:
        hit = _plan_rows(links, starts, batch_size, patch_shape, overlap)
        if key is not None:
            _ROWS_SCHEDULES[key] = hit
            while len(_ROWS_SCHEDULES) > 8:
                _ROWS_SCHEDULES.popitem(last=False)
    elif key is not None:
        _ROWS_SCHEDULES.move_to_end(key)
    return list(hit[0]), hit[1]


def _plan_rows(links, starts, batch_size, patch_shape, overlap):
    """
    The rows carried along y on top of the z links of _carry_schedule: (ylinks, peak) with
    ylinks[bi] = (y successor, shift_y, the successor's row range, diagonal successor or None) or None, and peak =
    the buffer sets alive at once on one stream with them. A batch computes {planes not carried in} x {rows not
    carried in} and stores again only what it computes, so a y link is kept only where every (plane, row) block
    of the successor still has a batch that computes it and is linked to it:
      * both batches take part in the z links (so they run in row mode and own a buffer set);
      * the range passed on does not meet the rows the batch took over itself (the chain is cut, as along z);
      * the y predecessor computes every plane the successor does (no planes carried in, or the same range);
      * a z predecessor that took rows over must see its z successor take the same rows over, and the block
        neither computes must come from their common diagonal predecessor -- else the z predecessor keeps
        computing its rows.
    """
    n = len(links)
    bs = int(batch_size)
    succ_y = carry_plan(starts, bs, patch_shape, overlap, axis=1)
    pred_z = {l[0]: bi for bi, l in enumerate(links) if l is not None}
    in_z = {bj: links[bi][2] for bj, bi in pred_z.items()}
    takes_part = [links[bi] is not None or bi in pred_z for bi in range(n)]
    pred_y, in_y, shift_of = {}, {}, {}
    for bi, bj in enumerate(succ_y):
        if bj is None or not takes_part[bi] or not takes_part[bj]:
            continue
        shift = int(starts[bj * bs][1]) - int(starts[bi * bs][1])
        rows = _carry_rows_span(patch_shape[1], shift)
        if rows[1] > rows[0]:
            pred_y[bj], in_y[bj], shift_of[bj] = bi, rows, shift
    changed = True
    while changed:
        changed = False
        for b in sorted(in_y):
            p, rows, shift = pred_y[b], in_y[b], shift_of[b]
            got = in_y.get(p, (0, 0))
            drop = rows[0] + shift < got[1] and got[0] < rows[1] + shift       # the chain is cut here
            drop = drop or in_z.get(p, (0, 0)) not in ((0, 0), in_z.get(b, (0, 0)))
            if drop:
                del in_y[b]
                changed = True
        for b, pz in pred_z.items():
            if pz not in in_y:
                continue
            pd = pred_y[pz]
            ok = (in_y.get(b) == in_y[pz] and shift_of[b] == shift_of[pz] and
                  (in_z.get(pred_y[b], (0, 0)) == (0, 0) or
                   (pred_z.get(pred_y[b]) == pd and in_z[pred_y[b]] == in_z[b] and
                    links[pd][1] == links[pz][1])))
            if not ok:
                del in_y[pz]
                changed = True
    ylinks = [None] * n
    for b, rows in in_y.items():
        ylinks[pred_y[b]] = (b, shift_of[b], rows, None)
    for b, pz in pred_z.items():       # the block neither predecessor computes
        if pz in in_y and b in in_y and in_z.get(pred_y[b], (0, 0)) != (0, 0):
            pd = pred_y[pz]
            ylinks[pd] = ylinks[pd][:3] + (b,)
    if not any(ylinks):
        return ylinks, None
    has, alive, peak = set(), 0, 0
    for bi in range(n):
        targets = [bi] if takes_part[bi] else []
        if links[bi] is not None:
            targets.append(links[bi][0])
        if ylinks[bi] is not None:
            targets += [t for t in (ylinks[bi][0], ylinks[bi][3]) if t is not None]
        for t in targets:
            if t not in has:
                has.add(t)
                alive += 1
        peak = max(peak, alive)
        if bi in has:
            alive -= 1
    return ylinks, peak


def _carry_rows_budget(model, links, peak, level1, starts, batch_size, patch_shape, overlap, n_streams, device,
                       free=None):
    """
    The rows carried along y on top of what _carry_schedule gave (links, peak, level1): (ylinks, more) with
    _carry_rows_schedule's links and the buffer sets to allocate beyond peak -- a set then lives from the earliest
    of its three predecessors -- or (None, 0) where there is nothing to carry or peak + more sets of pairs (and
    triples, if level1) would exceed CARRY_POOL_BYTES or half of the free device memory (free: asked from the
    device if None, before the sets are allocated). The rows are budgeted last: they never cost a z link or the
    second level its buffers, and _carry_schedule's answer does not depend on them.
    """
    ylinks, need = _carry_rows_schedule(links, starts, batch_size, patch_shape, overlap)
    if need is None:
        return None, 0
    more = max(0, need + (int(n_streams) if n_streams > 1 else 0) - int(peak))
    shape = (int(batch_size),) + tuple(patch_shape)
    set_bytes = 2 * sum(model.carry_pair_elems(shape)) + (2 * sum(model.carry_triple_elems(shape)) if level1 else 0)
    if free is None:
        free, _ = torch.cuda.mem_get_info(device)
    if (peak + more) * set_bytes > min(int(CARRY_POOL_BYTES), int(free) // 2):
        return None, 0
    return ylinks, more


def _carry_schedule(model, succ, starts, batch_size, patch_shape, overlap, n_streams, device, free=None):
    """
    The carry links run_sliding_window can use and the buffer sets they need: (links, peak, level1) with
    links[bi] = (successor, shift, the successor's plane range, its second-level plane range) or None, peak =
    the sets to allocate and level1 = whether a set holds the second level's triple next to the first level's
    pair, or (None, 0, False) when nothing can be carried or the buffers would not fit (_carry_budget; free:
    the device's free bytes, asked from the device if None). The second-level range of a link is (0, 0) where
    the engine gives none (or CARRY_Z1 is off, or the triples do not fit). peak is the most sets alive at once
    plus, with several streams, one per stream: sets are handed out oldest first, so the set a batch takes
    was last read by the batch n_streams earlier -- the previous one on its own stream -- and the batches in
    flight never wait for each other over a buffer.
    """
    links = [None] * len(succ)
    spans = {}
    taken = {}      # batch index -> the plane ranges its predecessor leaves it (first level, second level)
    for bi, bj in enumerate(succ):
        if bj is None:
            continue
        own = starts[bi * batch_size:(bi + 1) * batch_size]
        shift = int(starts[bj * batch_size][0]) - int(own[0][0])
        stride = batch_row_stride(own, patch_shape, overlap)
        key = (len(own), stride, shift)
        if key not in spans:
            span = model.carry_planes((len(own),) + tuple(patch_shape), stride, shift, device)
            span1 = (0, 0)
            if CARRY_Z1 and span[1] > span[0]:
                span1 = model.carry1_planes((len(own),) + tuple(patch_shape), stride, shift, device)
            spans[key] = (span, span1)
        span, span1 = spans[key]
        # A batch stores again only planes it computes: where the range it would pass on reaches into the range
        # it takes over itself (a z stride of less than a third of the depth or so), the chain is cut here and
        # starts again with the successor -- or, if only the second level's ranges meet, that level's is.
        got, got1 = taken.get(bi, ((0, 0), (0, 0)))
        if span[0] + shift < got[1] and got[0] < span[1] + shift:
            continue
        if span1[0] + shift // 2 < got1[1] and got1[0] < span1[1] + shift // 2:
            span1 = (0, 0)
        if span[1] > span[0]:
            links[bi] = (bj, shift, span, span1)
            taken[bj] = (span, span1)
    if not any(links):
        return None, 0, False
    # pairs alive at once: a batch's pair lives from its predecessor's (or its own) forward to its own
    has_pair, alive, peak = set(), 0, 0
    for bi, link in enumerate(links):
        if bi not in has_pair and link is not None:
            has_pair.add(bi)
            alive += 1
        if link is not None:
            has_pair.add(link[0])
            alive += 1
        peak = max(peak, alive)
        if bi in has_pair:
            alive -= 1
    if n_streams > 1:
        peak += int(n_streams)
    shape = (int(batch_size),) + tuple(patch_shape)
    triple_bytes = 0
    if any(link is not None and link[3][1] > link[3][0] for link in links):
        triple_bytes = 2 * sum(model.carry_triple_elems(shape))
    if free is None:
        free, _ = torch.cuda.mem_get_info(device)
    level0, level1 = _carry_budget(peak, 2 * sum(model.carry_pair_elems(shape)), triple_bytes, free, CARRY_POOL_BYTES)
    if not level0:
        return None, 0, False
    if not level1:     # (a second-level range that was cut for a predecessor's stays cut: no link is added here)
        links = [None if link is None else link[:3] + ((0, 0),) for link in links]
    return links, peak, level1


def batch_keep_hi(starts, patch_shape, trim, global_shape):
    """
    Per axis, the end of the trimmed outputs a batch of patch starts (global coordinates)
    contributes to a volume of global_shape: the stitch places patch[trim:trim + e - s] with
    s = start + trim, e = min(s + patch - 2 trim, dim) (inference.py:101-116), so a patch keeps
    local [trim, min(patch - trim, dim - start)); the batch keeps the largest of its patches'.
    None when that is everything (UNet3D.run_prepared's keep_hi). Host-side, no device sync.
    """
    trim = int(trim)
    keep = []
    for axis in range(3):
        full = int(patch_shape[axis]) - trim
        hi = min(full, max(int(global_shape[axis]) - int(s[axis]) for s in starts))
        if hi <= trim:      # nothing of the batch is kept on this axis: nothing to gain from a clip
            hi = full
        keep.append(hi)
    if trim <= 0 or all(k == int(p) - trim for k, p in zip(keep, patch_shape)):
        return None
    return tuple(keep)


def _start_ranges(dims, patch_shape, overlap):
    """range(0, d - patch + stride, stride) per axis (inference.py:361-364)."""
    return [
        range(0, d - ps + (ps - ov), ps - ov)
        for d, ps, ov in zip(dims, patch_shape, overlap)
    ]


_WORKER_STREAMS = {}


def _worker_streams(device, n):
    """Side streams per device, created once (the model keeps one workspace per stream)."""
    pool = _WORKER_STREAMS.setdefault(str(device), [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device))
    return pool[:n]


def _effective_clip(np_dtype, brightness_clip, storage_dtype=None):
    """
    Applies numpy's promotion rules of np.minimum(img, brightness_clip)
    (inference.py:79); returns (clip, dtype of the clipped image): clip is None
    when no clip is given, otherwise the value the kernels compare against.
    An integer image with a fractional clip becomes float64, like in numpy.
    """
    np_dtype = np.dtype(np_dtype)
    if brightness_clip is None:
        return None, np_dtype
    probe = np.minimum(np.zeros(1, dtype=np_dtype), brightness_clip)  # may raise like numpy
    if probe.dtype == np_dtype:
        return np_dtype.type(brightness_clip), np_dtype
    if probe.dtype.kind in "iu" and np_dtype.kind in "iu":
        # a typed integer clip (np.int64(1000) on a uint16 image): numpy widens the image, every voxel
        # keeps its value, so the comparison can stay in the image's own dtype; the wider dtype only
        # decides the integer arithmetic inside np.percentile (value_dtype)
        info, c = np.iinfo(np_dtype), int(brightness_clip)
        if c < info.min:
            raise NotImplementedError(f"brightness_clip {brightness_clip!r} lies below every {np_dtype} voxel")
        return (None if c >= info.max else np_dtype.type(c)), probe.dtype
    if probe.dtype != np.float64:
        # a float16 / float32 typed clip on a narrow integer image: np.percentile and the
        # normalisation would then run in that float type's arithmetic
        raise NotImplementedError(
            f"brightness_clip {brightness_clip!r} promotes {np_dtype} voxels to {probe.dtype}"
        )
    clip = np.float64(brightness_clip)
    if np_dtype.kind in "iu" and clip < np.iinfo(np_dtype).min:
        raise NotImplementedError(f"brightness_clip {brightness_clip!r} lies below every {np_dtype} voxel")
    storage = np.dtype(storage_dtype) if storage_dtype is not None else _device_voxel_dtype(np_dtype)[0]
    if storage == np.float32 and np_dtype != np.float32 and np.float64(np.float32(clip)) != clip:
        # (predict() sends such a volume as float64 instead: _device_voxel_dtype(..., clip=))
        raise NotImplementedError(
            f"brightness_clip {brightness_clip!r} is not a float32 number (the volume travels as float32)"
        )
    return clip, np.dtype(np.float64)


def _histogram_into(hist, tensor, vox_code, clip, pass_index=0, prefix=0):
    """Adds the voxels of a device tensor to an int64 (65536,) device histogram."""
    if vox_code == _native.VOX_F64:
        _native.check(
            _native.lib().exaspim_histogram_wide(
                tensor.data_ptr(), vox_code, tensor.numel(),
                float(clip) if clip is not None else 0.0, 1 if clip is not None else 0,
                pass_index, int(prefix), hist.data_ptr(), _stream(tensor.device),
            ),
            "exaspim_histogram_wide",
        )
        return
    _native.check(
        _native.lib().exaspim_histogram(
            tensor.data_ptr(), vox_code, tensor.numel(),
            float(clip) if clip is not None else 0.0, 1 if clip is not None else 0,
            pass_index, prefix, hist.data_ptr(), _stream(tensor.device),
        ),
        "exaspim_histogram",
    )


def volume_histogram(volume, clip, pass_index=0, prefix=0):
    """Runs exaspim_histogram over a DeviceVolume; returns the int64 device tensor."""
    hist = torch.zeros(65536, dtype=torch.int64, device=volume.tensor.device)
    _histogram_into(hist, volume.tensor, volume.vox_code, clip, pass_index, prefix)
    return hist


def _key_to_f32(key):
    """Inverse of the order-preserving float32 key of the histogram kernel."""
    key = np.uint32(key)
    bits = (key & np.uint32(0x7FFFFFFF)) if key & np.uint32(0x80000000) else ~key
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def _key_to_f64(key):
    """Inverse of the order-preserving float64 key of the wide histogram kernel."""
    key = int(key)
    bits = (key & 0x7FFFFFFFFFFFFFFF) if key >> 63 else (~key & 0xFFFFFFFFFFFFFFFF)
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


def _percentiles_from_histograms(histogram, storage_dtype, percentiles, value_dtype=None, clip=None):
    """
    np.percentile of the clipped volume from 65536-bin histograms:
    "histogram(pass_index, prefix)" returns the counts (numpy int64) over the
    whole volume; integer voxels need one pass, float32 voxels a second pass per
    16-bit key prefix an order statistic falls into. "value_dtype" is the dtype
    of the clipped image in numpy's eyes (it decides the arithmetic of
    np.percentile); with a fractional clip of an integer image every voxel above
    the clip sits in bin ceil(clip) and stands for the clip itself.
    """
    storage_dtype = np.dtype(storage_dtype)
    value_dtype = np.dtype(value_dtype) if value_dtype is not None else storage_dtype

    def as_value(v):
        if clip is not None and np.float64(v) > np.float64(clip):
            return value_dtype.type(clip)
        return value_dtype.type(v)

    if storage_dtype.kind in "ui":
        offset = 32768 if storage_dtype == np.int16 else 0
        stats = img_util.OrderStatistics(histogram(), lambda b: as_value(b - offset))
    elif storage_dtype == np.float64:
        # radix select on the order-preserving 64-bit key, 16 bits per level
        levels = {}

        def level(p, prefix):
            if (p, prefix) not in levels:
                levels[(p, prefix)] = img_util.OrderStatistics(histogram(p, prefix), lambda b: b)
            return levels[(p, prefix)]

        class _F64Stats:
            n = level(0, 0).n

            @staticmethod
            def kth(k):
                prefix, rank = 0, k
                for p in range(4):
                    b, rank = level(p, prefix).bin_of_rank(rank)
                    prefix = (prefix << 16) | b
                return as_value(_key_to_f64(prefix))

        stats = _F64Stats()
    else:
        coarse = img_util.OrderStatistics(histogram(0), lambda b: b)
        fine = {}

        class _F32Stats:
            n = coarse.n

            @staticmethod
            def kth(k):
                hi, within = coarse.bin_of_rank(k)
                if hi not in fine:
                    fine[hi] = img_util.OrderStatistics(histogram(1, hi), lambda b: b)
                lo, _ = fine[hi].bin_of_rank(within)
                return as_value(_key_to_f32((hi << 16) | lo))

        stats = _F32Stats()
    mn, mx = img_util.percentiles_from_statistics(stats, percentiles, value_dtype)
    return mn, mx


def volume_percentiles(volume, brightness_clip, percentiles, reduce_fn=None):
    """
    np.percentile(np.minimum(img, brightness_clip), percentiles) for a
    device-resident volume (inference.py:79, img_util.py:526), exactly.

    Parameters
    ----------
    volume : DeviceVolume
        Local block of the volume.
    brightness_clip : float
        Clip of inference.py:79 (None disables it).
    percentiles : Tuple[float]
        Lower and upper percentile.
    reduce_fn : Callable[[torch.Tensor], None], optional
        In-place sum of a histogram over all ranks (sharded volumes).

    Returns
    -------
    Tuple[numpy.float64]
        (mn, mx).
    """
    clip, value_dtype = _effective_clip(volume.np_dtype, brightness_clip, volume.storage_dtype)

    def histogram(pass_index=0, prefix=0):
        hist = volume_histogram(volume, clip, pass_index, prefix)
        if reduce_fn is not None:
            reduce_fn(hist)
        return hist.cpu().numpy()

    return _percentiles_from_histograms(histogram, volume.storage_dtype, percentiles, value_dtype, clip)


def _model_probabilities(model, inputs, trim=0, out=None):
    """sigmoid(model(inputs)) (inference.py:157-158) as a float32 device tensor;
    the "trim" voxels next to every patch face, which the caller discards
    (inference.py:161-162), are left undefined."""
    if isinstance(model, UNet3D):
        if FULL_PATCHES:  # measurement aid: compute the discarded margin too
            trim = 0
        return model.run(inputs, apply_sigmoid=True, trim=trim, out=out)
    with torch.no_grad():
        return torch.sigmoid(model(inputs)).to(torch.float32).contiguous()


def stitch_accumulate(pred, starts_dev, plan, accum, block):
    """accum += trimmed batch predictions (inference.py:99-116) on the device."""
    n = int(starts_dev.shape[0])
    # one launch takes n * trimmed depth <= 65535 grid rows; pieces in batch order add up
    # in the same order as one call
    piece = max(1, 65535 // max(1, plan.patch_shape[0] - 2 * plan.trim))
    for i in range(0, n, piece):
        m = min(piece, n - i)
        _native.check(
            _native.lib().exaspim_stitch_accumulate(
                pred[i:i + m].data_ptr(), starts_dev[i:i + m].data_ptr(), m,
                int(accum.shape[0]), plan.window, accum.data_ptr(), block,
                _stream(accum.device),
            ),
            "exaspim_stitch_accumulate",
        )


def stitch_finalize(accum, plan, block):
    """Divides by the per-voxel patch count (inference.py:120-125) on the device."""
    _native.check(
        _native.lib().exaspim_stitch_finalize(
            accum.data_ptr(), int(accum.shape[0]), plan.window, block, _stream(accum.device)
        ),
        "exaspim_stitch_finalize",
    )


def run_sliding_window(volume, model, plan, n_channels, batch_size, brightness_clip,
                       mn, mx, starts=None, accum=None, accum_block=None, verbose=False,
                       n_streams=1, pbar=None):
    """
    Runs every batch of the sliding window (inference.py:93-117): gather ->
    network -> sigmoid -> trimmed overlap-add into a device accumulator.
    Nothing here synchronises the device.

    Parameters
    ----------
    volume : DeviceVolume
        Input block in device memory (must contain every voxel the given
        starts read).
    model : torch.nn.Module
        Network on the same device.
    plan : SlidingWindow
        Window geometry over the GLOBAL volume.
    n_channels : int
        Output channels (3 affinities or 1 foreground map).
    batch_size : int
        Patches per batch.
    brightness_clip, mn, mx : float
        Pre-processing constants.
    n_streams : int, optional
        Batches in flight: gather + network of consecutive batches alternate
        between this many HIP streams (each with its own workspace); the stitch
        kernels stay on the caller's stream in batch order, so results do not
        depend on this number. Measured on MI355X (1024^3, 16-bit, batch 16): three
        streams are 5-7 % faster than one because the ramp-down of one kernel
        overlaps the next batch's work, which is why predict() asks for three;
        kernels of different batches then share the device and per-kernel
        timings lose their meaning, so this building block (and bench.py's
        roofline leg) defaults to 1. Moving only gather/stitch to a side stream
        gains nothing.
    starts : List[Tuple[int]], optional
        Patch starts to process (default: all of plan.starts()).
    accum : torch.Tensor, optional
        Existing float32 accumulator (n_channels, *accum_block.dims).
    accum_block : _native.Block, optional
        Placement of the accumulator (default: the volume's block).
    pbar : tqdm, optional
        Progress bar of the caller, advanced by the patches processed.

    Returns
    -------
    torch.Tensor
        The accumulator (sums, not yet divided).
    """
    device = volume.tensor.device
    clip, _ = _effective_clip(volume.np_dtype, brightness_clip, volume.storage_dtype)
    if starts is None:
        starts = plan.starts()
    if accum_block is None:
        accum_block = volume.block
    if accum is None:
        accum = torch.zeros((n_channels,) + tuple(accum_block.dims), dtype=torch.float32,
                            device=device)
    if len(starts) == 0:
        return accum
    if any(p % 16 for p in plan.patch_shape):
        # the reference's Up.forward fails in torch.cat for such sizes (unet3d.py:281-288)
        raise RuntimeError(
            "Sizes of tensors must match: patch_shape entries must be multiples of 16, "
            f"got {plan.patch_shape}"
        )
    starts_dev = torch.tensor(starts, dtype=torch.int32, device=device).reshape(-1, 3)
    # a kernel launch takes n * (patch depth + 2) <= 65535 grid rows: a caller's very large
    # batch of small patches runs as several engine batches (a patch's result does not depend
    # on the batch it travels in)
    batch_size = max(1, min(int(batch_size), 65535 // (max(plan.patch_shape) + 2)))
    own_pbar = pbar is None and verbose and tqdm is not None
    if own_pbar:
        pbar = tqdm(total=len(starts), desc="Predict")
    main = torch.cuda.current_stream(device)
    n_streams = max(1, min(int(n_streams), -(-len(starts) // batch_size)))
    workers = _worker_streams(device, n_streams) if n_streams > 1 else [main]
    for s in workers:
        s.wait_stream(main)  # volume, accumulator and starts are ready on the caller's stream
    if isinstance(model, UNet3D) and model.needs_resolution():
        # compute_dtype="auto": the first batch of real patches decides between fp16 and float32
        probe = _get_batch_inputs(volume, starts_dev[:batch_size], plan.patch_shape, device, clip=clip,
                                  mn=mn, mx=mx)
        model.resolve_compute_dtype(probe)
        del probe
    prepared_layout = None
    if isinstance(model, UNet3D) and not PLAIN_GATHER:
        prepared_layout = model.input_layout(device)    # (PLAIN_GATHER: tests hold the two paths to each other)
    # first-level planes carried from one z slab of patches to the next
    links, ylinks, free_pairs = None, None, collections.deque()
    if CARRY_Z and prepared_layout is not None and not model.needs_resolution():
        links, peak, level1 = _carry_schedule(model, carry_plan(starts, batch_size, plan.patch_shape, plan.overlap),
                                              starts, batch_size, plan.patch_shape, plan.overlap, n_streams, device)
        if links is not None:
            # rows carried along y as well (section 3g), where the pool holds the sets that live longer for it
            ylinks, more = _carry_rows_budget(model, links, peak, level1, starts, batch_size, plan.patch_shape,
                                              plan.overlap, n_streams, device)
            peak += more
            shape = (batch_size,) + tuple(plan.patch_shape)
            elems = model.carry_pair_elems(shape)
            elems1 = model.carry_triple_elems(shape) if level1 else None     # (section 3e: a triple with every pair)
            # (allocated before the workers branch off the caller's stream; alive until the call returns)
            free_pairs.extend([tuple(torch.empty(e, dtype=torch.int16, device=device) for e in elems), None,
                               elems1 and tuple(torch.empty(e, dtype=torch.int16, device=device) for e in elems1)]
                              for _ in range(peak))
            for s in workers:
                s.wait_stream(main)
    # batch index -> [its pair (and triple), the planes already there, its z predecessor's event, the level-1 planes,
    # the rows already there, the events of its y and diagonal predecessors]
    pending = {}

    def take_pair(worker):
        pair = free_pairs.popleft()     # (the one released longest ago)
        if pair[1] is not None:     # the forward that read it last, maybe on another stream
            worker.wait_event(pair[1])
        return pair

    def target(t, worker):
        """The pending entry of batch t, which this worker's forward is about to store into: its set is taken when
        the earliest of its predecessors runs, and every predecessor waits for the forward that read the set last."""
        if t not in pending:
            pending[t] = [take_pair(worker), (0, 0), None, (0, 0), (0, 0), []]
        elif pending[t][0][1] is not None:
            worker.wait_event(pending[t][0][1])
        return pending[t]

    for bi, i in enumerate(range(0, len(starts), batch_size)):
        batch = starts_dev[i:i + batch_size]
        row_stride = batch_row_stride(starts[i:i + batch_size], plan.patch_shape, plan.overlap)
        keep_hi = None
        if CLIP_TO_VOLUME and not FULL_PATCHES:
            keep_hi = batch_keep_hi(starts[i:i + batch_size], plan.patch_shape, plan.trim, plan.shape)
        worker = workers[bi % n_streams]
        with torch.cuda.stream(worker):
            if prepared_layout is not None:
                # the gather kernel writes the first convolution's operand layout directly
                inputs = _get_batch_inputs(volume, batch, plan.patch_shape, device, clip=clip,
                                           mn=mn, mx=mx, layout=prepared_layout)
                carry, own = None, None
                if links is not None and (bi in pending or links[bi] is not None):
                    own, in_z, before, in_z1, in_y, others = pending.pop(bi, None) or [take_pair(worker), (0, 0), None,
                                                                                       (0, 0), (0, 0), []]
                    carry = {"own": own[0], "in_z": in_z}
                    if own[2] is not None:
                        carry.update(own1=own[2], in_z1=in_z1)
                    for event in [before] + others:
                        if event is not None:
                            worker.wait_event(event)      # the planes and rows carried in are there
                    encoded = None
                    if ylinks is not None and (in_y[1] > in_y[0] or ylinks[bi] is not None):
                        carry.update(in_y=in_y)
                        if ylinks[bi] is not None:
                            by, shift_y, rows, bd = ylinks[bi]
                            if n_streams > 1:
                                # the y successor is usually the very next batch: it waits for this forward's first
                                # level, not for its end
                                encoded = torch.cuda.Event()
                                carry.update(encoder_event=encoded)
                            after = target(by, worker)
                            after[4] = rows
                            after[5].append(encoded)
                            carry.update(out_y_pair=after[0][0], out_y=(rows[0] + shift_y, rows[1] + shift_y),
                                         out_shift_y=shift_y)
                            if bd is not None:
                                after = target(bd, worker)
                                after[5].append(encoded)
                                carry.update(out_d_pair=after[0][0])
                    if links[bi] is not None:
                        nxt, shift, span, span1 = links[bi]
                        out_pair = target(nxt, worker)[0]
                        carry.update(out=out_pair[0], out_z=(span[0] + shift, span[1] + shift), out_shift=shift)
                        if span1[1] > span1[0]:
                            carry.update(out1=out_pair[2], out_z1=(span1[0] + shift // 2, span1[1] + shift // 2),
                                         out_shift1=shift // 2)
                        pending[nxt][1], pending[nxt][3] = span, span1
                pred = model.run_prepared(
                    inputs, (int(batch.shape[0]),) + tuple(plan.patch_shape), apply_sigmoid=True,
                    trim=0 if FULL_PATCHES else plan.trim, row_stride=row_stride, keep_hi=keep_hi, carry=carry)
                if own is not None:
                    done = None
                    if n_streams > 1:
                        done = torch.cuda.Event()
                        done.record(worker)
                    if links[bi] is not None:
                        pending[links[bi][0]][2] = done
                    own[1] = done
                    free_pairs.append(own)
            else:
                inputs = _get_batch_inputs(volume, batch, plan.patch_shape, device, clip=clip,
                                           mn=mn, mx=mx)
                pred = _model_probabilities(model, inputs, plan.trim)
        if pred.shape[1] != n_channels:
            raise RuntimeError(
                f"model produced {pred.shape[1]} channels, expected {n_channels}"
            )
        if worker is not main:
            main.wait_stream(worker)
            pred.record_stream(main)
        stitch_accumulate(pred, batch, plan, accum, accum_block)
        if pbar is not None:
            pbar.update(int(batch.shape[0]))
    if own_pbar:
        pbar.close()
    return accum


# --- slab pipeline: out-of-core input, overlapped transfers ---
_COPY_STREAMS = {}
_PINNED_LOCK = threading.Lock()
_PINNED_FREE = {}               # (device, torch dtype) -> page-locked buffers no call is using
PINNED_SLOT_BYTES = 512 << 20   # a finished slab is cut so that one staging slot stays below this


def _checkout_pinned(device, count, numel, dtype):
    """
    Takes "count" host staging buffers of at least "numel" elements out of the pool of the
    device (page-locked, kept between calls so that a second predict() does not pay for
    hipHostMalloc again). A buffer belongs to ONE call from here until _return_pinned:
    concurrent predict() calls -- threads driving different GPUs, or the same one -- never
    share staging memory. If the runtime refuses to page-lock more memory the buffer is
    ordinary pageable memory (the download then blocks the copy stream, nothing else changes).
    """
    key = (str(device), dtype)
    with _PINNED_LOCK:
        free = _PINNED_FREE.setdefault(key, [])
        free.sort(key=lambda t: t.numel())
        taken = []
        while free and len(taken) < count and free[-1].numel() >= numel:
            taken.append(free.pop())
    while len(taken) < count:
        try:
            taken.append(torch.empty(numel, dtype=dtype, pin_memory=True))
        except RuntimeError:
            taken.append(torch.empty(numel, dtype=dtype))
    return taken


def _return_pinned(device, dtype, buffers):
    """Hands staging buffers back to the device's pool (pageable fall-backs are dropped)."""
    with _PINNED_LOCK:
        _PINNED_FREE.setdefault((str(device), dtype), []).extend(b for b in buffers if b.is_pinned())


def release_pinned_buffers():
    """Frees the page-locked staging buffers predict() keeps between calls."""
    with _PINNED_LOCK:
        _PINNED_FREE.clear()


def _copy_stream(device):
    """The stream the slab downloads run on (one per device, created once)."""
    key = str(device)
    with _PINNED_LOCK:
        if key not in _COPY_STREAMS:
            _COPY_STREAMS[key] = torch.cuda.Stream(device)
        return _COPY_STREAMS[key]


class _SlabDrain:
    """
    Moves finished output slabs off the device while later patch layers compute: a slab is
    written (and divided) into one of three device slots on the caller's stream, downloaded to
    a host staging slot on the copy stream, and handed to host threads from there.

    Parameters
    ----------
    device : torch.device
        The HIP device.
    slot_elems : int
        Elements of the largest slab handed to emit().
    half_out : bool
        Round slabs to IEEE half on the device before they leave it.
    threads : int
        Host threads that consume downloaded slabs.
    label_elems : int, optional
        Not 0: slabs leave the device as int32 labels (emit's "label"), at most this many
        elements each, and the staging memory is int32.
    """

    N_SLOTS = 3

    def __init__(self, device, slot_elems, half_out, threads, label_elems=0):
        self.device = device
        self.half_out = half_out
        self.main = torch.cuda.current_stream(device)
        self.copy_stream = _copy_stream(device)
        self.host_dtype = torch.int32 if label_elems else torch.float16 if half_out else torch.float32
        n = self.N_SLOTS
        self.dev_labels = [torch.empty(label_elems, dtype=torch.int32, device=device) for _ in range(n)
                           if label_elems]
        self.dev_out = [torch.empty(slot_elems, dtype=torch.float32, device=device) for _ in range(n)]
        self.dev_half = ([torch.empty(slot_elems, dtype=torch.float16, device=device) for _ in range(n)]
                         if half_out else None)
        self.host = _checkout_pinned(device, n, label_elems or slot_elems, self.host_dtype)
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(threads)))
        self.pending = [[] for _ in range(n)]
        self.n_emitted = 0

    def emit(self, shape, fill, consumers, label=None):
        """
        Queues one slab: "fill(out)" writes the final values into the zeroed float32 device
        tensor "out" of "shape"; "consumers(view)" returns the host jobs (callables) that read
        the downloaded numpy "view" of the same shape -- each runs on a pool thread once the
        download has finished, and the staging slot is reused only after all of them returned.
        "label(out, slot)", if given, turns the filled slab into the int32 tensor that travels
        instead (in the flat int32 device buffer "slot", whose previous slab has left it), or
        returns None when nothing is to leave the device; "view" then has that tensor's shape.
        """
        slot = self.n_emitted % self.N_SLOTS
        self.n_emitted += 1
        for f in self.pending[slot]:
            f.result()                   # the slot's previous slab has left the staging memory
        count = int(np.prod(shape))
        out = self.dev_out[slot][:count].view(shape)
        out.zero_()                      # planes no patch covers stay 0 (inference.py:120-125)
        fill(out)
        if label is not None:
            out = label(out, self.dev_labels[slot])
            if out is None:
                self.pending[slot] = []
                return
            shape, count = tuple(out.shape), out.numel()
        elif self.half_out:
            out = export_half(out, self.dev_half[slot][:count]).view(shape)
        ready, done = torch.cuda.Event(), torch.cuda.Event()
        ready.record(self.main)
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(ready)
            self.host[slot][:count].view(shape).copy_(out, non_blocking=True)
            done.record(self.copy_stream)
        view = self.host[slot][:count].numpy().reshape(shape)

        def after_download(job):
            def run():
                done.synchronize()
                job()
            return run

        self.pending[slot] = [self.pool.submit(after_download(job)) for job in consumers(view)]

    def drain(self):
        """Waits until every queued slab has been consumed (re-raises a consumer's exception)."""
        for jobs in self.pending:
            for f in jobs:
                f.result()
        self.pending = [[] for _ in range(self.N_SLOTS)]

    def close(self):
        self.pool.shutdown(wait=True)
        _return_pinned(self.device, self.host_dtype, self.host)
        self.host = []


class _ArraySource:
    """read_box(lo, hi) over anything that slices like a 3-D numpy array (ndarray, memmap,
    a zarr / N5 / TIFF-backed array as img_util.read returns, img_util.py:25-121)."""

    def __init__(self, arr):
        while len(arr.shape) > 3:
            if arr.shape[0] != 1:
                raise ValueError("leading image axes must have length 1")
            arr = arr[0]
        if len(arr.shape) != 3:
            raise ValueError(f"expected a 3-D image, got shape {tuple(arr.shape)}")
        self.arr = arr
        self.shape = tuple(int(v) for v in arr.shape)
        self.dtype = np.dtype(arr.dtype)

    def __call__(self, lo, hi):
        return np.asarray(self.arr[tuple(slice(a, b) for a, b in zip(lo, hi))])


def _plane_reader(read_block, shape):
    """read_box(lo, hi) over a read_block(z0, z1) function, which hands out whole planes."""
    def read_box(lo, hi):
        block = read_block(lo[0], hi[0])
        if tuple(block.shape) != (hi[0] - lo[0],) + tuple(shape[1:]):
            raise ValueError(f"read_block({lo[0]}, {hi[0]}) returned shape {tuple(block.shape)}")
        return block[:, lo[1]:hi[1], lo[2]:hi[2]]
    return read_box


def _device_voxel_dtype(np_dtype, whole=None, clip=None):
    """
    Voxel dtype the kernels read for an image of "np_dtype", and the function that converts a
    block to it. uint8 / uint16 / int16 / float32 / float64 travel as they are, int8 as int16.
    32- and 64-bit integers travel as float32 when the caller can show that every value is
    exactly representable ("whole": the entire image as an in-memory array) -- half the bytes --
    and as float64 otherwise (what the reference's arithmetic works in, img_util.py:526-531);
    float64 images likewise go as float32 only when "whole" proves them float32-exact. A
    brightness clip float32 cannot hold ("clip") sends them as float64 too. 64-bit integers that
    float64 cannot hold raise TypeError.
    """
    np_dtype = np.dtype(np_dtype)
    if np_dtype == np.int8:
        return np.dtype(np.int16), lambda block: block.astype(np.int16)
    if np_dtype.kind in "iuf" and np_dtype.itemsize in (4, 8) and np_dtype != np.float32:
        clip_ok = clip is None or np.float64(np.float32(clip)) == np.float64(clip)
        if whole is not None and clip_ok:
            as32 = np.asarray(whole).astype(np.float32)
            if np.array_equal(as32.astype(np_dtype), whole):
                def to_f32(block):
                    b32 = block.astype(np.float32)
                    if not np.array_equal(b32.astype(np_dtype), block):
                        raise TypeError(f"{np_dtype} volume is not exactly representable in float32")
                    return b32
                return np.dtype(np.float32), to_f32

        def to_f64(block):
            b64 = block.astype(np.float64)
            if np_dtype.kind in "iu" and np_dtype.itemsize == 8 and not np.array_equal(b64.astype(np_dtype), block):
                raise TypeError(f"{np_dtype} volume is not exactly representable in float64")
            return b64
        return np.dtype(np.float64), to_f64
    if np_dtype in _VOX_CODES:
        return np_dtype, lambda block: block
    return np_dtype, lambda block: block


class DeviceShardOps:
    """
    What run_slab_pipeline does on the device, as overridable steps (the CPU tests replace the
    kernels by their numpy restatements and keep the schedule, the band bookkeeping and the
    exchanges).
    """

    def __init__(self, model, plan, n_channels, batch_size, brightness_clip, n_streams, half_out,
                 copy_threads):
        self.model, self.plan = model, plan
        self.n_channels, self.batch_size = n_channels, batch_size
        self.brightness_clip, self.n_streams = brightness_clip, n_streams
        self.half_out, self.copy_threads = half_out, copy_threads
        self.device = _hip_device(model)

    # -- voxels
    def storage(self, src_dtype, whole=None):
        """(voxel dtype in device memory, host conversion) for an image dtype; "whole": the entire
        image where it is an in-memory array (it can show that float32 carries it exactly)."""
        vdtype, convert = _device_voxel_dtype(src_dtype, whole=whole, clip=self.brightness_clip)
        if vdtype not in _VOX_CODES:
            raise TypeError(_unsupported(src_dtype))
        return vdtype, convert

    def upload(self, block, convert):
        """The host side of an upload: a block the reader returned as the tensor the pipeline
        copies, once, to its place in device memory."""
        return _carrier(convert(block))

    def empty_voxels(self, dims, vdtype):
        return torch.empty(tuple(dims), dtype=_TORCH_VOXELS[np.dtype(vdtype)], device=self.device)

    def effective_clip(self, src_dtype, vdtype):
        return _effective_clip(src_dtype, self.brightness_clip, vdtype)

    def histogram_into(self, hist, voxels, vdtype, clip, pass_index, prefix):
        _histogram_into(hist, voxels.contiguous(), _VOX_CODES[np.dtype(vdtype)], clip, pass_index, prefix)

    def percentiles(self, histogram, vdtype, percentiles, value_dtype, clip):
        return _percentiles_from_histograms(histogram, vdtype, percentiles, value_dtype, clip)

    # -- one patch layer: gather -> network -> sigmoid -> trimmed overlap-add into "accum"
    def run_layer(self, voxels, vox_origin, src_dtype, vdtype, starts, accum, accum_origin, mn, mx, pbar=None):
        gshape = self.plan.shape
        volume = DeviceVolume(voxels, src_dtype, vox_origin, gshape, storage_dtype=vdtype)
        blk = _native.Block.make(tuple(accum.shape[1:]), accum_origin, gshape)
        run_sliding_window(volume, self.model, self.plan, self.n_channels, self.batch_size,
                           self.brightness_clip, mn, mx, starts=starts, accum=accum,
                           accum_block=blk, n_streams=self.n_streams, pbar=pbar)

    def finalize(self, out, origin):
        """Divides the sums of the box at global "origin" by the per-voxel patch count."""
        stitch_finalize(out, self.plan, _native.Block.make(tuple(out.shape[1:]), origin, self.plan.shape))

    def zeros(self, shape):
        return torch.zeros(tuple(shape), dtype=torch.float32, device=self.device)

    def empty(self, shape):
        return torch.empty(tuple(shape), dtype=torch.float32, device=self.device)

    def slab_bytes_cap(self):
        return PINNED_SLOT_BYTES

    def make_drain(self, slot_elems, threads, label_elems=0):
        return _SlabDrain(self.device, slot_elems, self.half_out, threads, label_elems=label_elems)

    def synchronize(self):
        torch.cuda.synchronize(self.device)


class _WholeVolume:
    """
    The one rank of a 1 x 1 grid: the fields of sharding.Shard that run_slab_pipeline reads, for
    a device that has the volume to itself. Unlike Shard it also describes a volume no patch fits
    into (a dimension <= overlap): no starts, every plane still owned.
    """

    def __init__(self, plan):
        self.plan = plan
        ranges = _start_ranges(plan.shape, plan.patch_shape, plan.overlap)
        self.yx_starts = list(itertools.product(*ranges[1:]))
        self.z_starts = list(ranges[0]) if self.yx_starts else []
        self.input_origin = self.core_origin = self.accum_origin = self.own_lo = (0, 0, 0)
        self.input_dims = self.core_dims = self.accum_dims = self.own_hi = plan.shape


def run_slab_pipeline(ops, shard, read_box, src_dtype, storage, normalization_percentiles, *,
                      affinity_mode=True, write_block=None, result=None, label=None, copy_threads=4,
                      keep_input_resident=None, exchanges=None, progress=None, timings=None):
    """
    The out-of-core sliding window: one rank's share of predict() with the image READ and the
    result WRITTEN in pieces, behind predict_streaming, predict_components_streaming (the 1 x 1
    grid) and sharding.predict_shard_streaming. The device never holds more than one patch layer
    of input, two one-layer accumulators and three output slabs, whatever the depth of the block.

    pass 1  z-chunks of the rank's disjoint sub-volume are read once, uploaded and added to the
            device histogram ("exchanges" sums it over the ranks); np.percentile of the clipped
            volume follows from it exactly. With "keep_input_resident" the rank's whole input
            block is uploaded here and stays; pass 2 then reads nothing.
    pass 2  per patch layer k (the rank's patches with z-start z_k; the reference's order is
            z-major, inference.py:368-397):
            * the planes the layer adds go, with one copy from the host, into one of two rolling
              input slabs; the planes it shares with layer k - 1 move there on the device;
            * gather -> U-Net -> sigmoid -> trimmed overlap-add run into a one-layer accumulator
              that starts from the partial sums layer k - 1 left in the overlap band;
            * planes up to min(z_{k+1} + trim, end of the region) -- after the last layer, up to
              the end -- get no further addition from this rank. A 1 x 1 grid has no other rank,
              so the owned rows go from the accumulator into an output slot in cuts of at most
              min(D, max(stride + trim, patch depth), slab_bytes_cap() // bytes of a global plane)
              planes, are divided by the patch count there and leave: device -> pinned memory
              on a copy stream -> "write_block" or "result" on host threads, while the next
              layer computes. Between ranks, "exchanges" takes the finished planes first and
              calls emit() on the sums it has completed.
    Planes no patch reaches are emitted as zeros (inference.py:120-125), also when no patch fits
    into the volume at all.

    Parameters
    ----------
    ops : DeviceShardOps
        The device steps.
    shard : sharding.Shard or _WholeVolume
        The rank's part of the window (shard.plan) over the global volume.
    read_box : Callable[[Tuple[int], Tuple[int]], numpy.ndarray]
        Returns voxels [lo, hi) of the global image; only boxes inside the rank's input block
        are requested.
    src_dtype : numpy.dtype
        Voxel dtype of the image.
    storage : Tuple[numpy.dtype, Callable]
        ops.storage(src_dtype): the voxel dtype in device memory and the host conversion to it.
    write_block : Callable[[Tuple[int], Tuple[int], numpy.ndarray], None], optional
        Receives every finished box of the rank's region once, from one thread, as
        write_block(lo, hi, block); the block is valid during the call only.
    result : numpy.ndarray, optional
        Without "write_block": the array of the rank's region, (C, *own dims) or (*own dims),
        the slabs are copied into by "copy_threads" threads.
    label : Callable, optional
        label(z0, z1, out, slot) turns the finished, divided (C, z1 - z0, h, w) device slab "out"
        into the int32 (1, z1 - z0, h, w) tensor that leaves the device in its place (it may use
        the flat int32 device buffer "slot"), or returns None: nothing leaves.
    exchanges : object, optional
        What the ranks of a larger grid add (sharding._RankExchanges): reduce_histogram(hist),
        finished(cur, zs, hi, z0, z1, emit) for planes [z0, z1) of the layer accumulator "cur"
        (planes [zs, hi)), last_layer_done(cur, zs, hi, emit). emit(z0, z1, sums, s0, s1) hands
        over planes [z0, z1) out of "sums", which holds all accumulator rows of planes [s0, s1).
    progress : str, optional
        Description of a tqdm bar over the patches.
    timings : dict, optional
        Filled with the wall seconds of "upload_histogram", "layers" (ends with a device
        synchronisation) and "drain".
    """
    plan = shard.plan
    vdtype, convert = storage
    n_channels = 3 if affinity_mode else 1
    D, H, W = plan.shape
    pz, trim = plan.patch_shape[0], plan.trim
    stride = pz - plan.overlap[0]
    z_starts, yx_starts = shard.z_starts, shard.yx_starts
    in_lo = shard.input_origin
    in_hi = tuple(o + d for o, d in zip(in_lo, shard.input_dims))
    core_lo = shard.core_origin
    core_hi = tuple(o + d for o, d in zip(core_lo, shard.core_dims))
    acc_lo = shard.accum_origin
    AH, AW = shard.accum_dims[1], shard.accum_dims[2]
    own_lo, own_hi = shard.own_lo, shard.own_hi
    own_dims = tuple(h - l for l, h in zip(own_lo, own_hi))
    res4 = None if result is None else result.reshape((-1,) + own_dims)

    def read(lo, hi):
        block = read_box(tuple(lo), tuple(hi))
        if tuple(block.shape) != tuple(h - l for l, h in zip(lo, hi)):
            raise ValueError(f"read_box({tuple(lo)}, {tuple(hi)}) returned shape {tuple(block.shape)}")
        return ops.upload(block, convert)

    # ---- pass 1: histogram of the rank's disjoint sub-volume (inference.py:79, img_util.py:526) ----
    in_plane_bytes = shard.input_dims[1] * shard.input_dims[2] * np.dtype(vdtype).itemsize
    if keep_input_resident is None:
        keep_input_resident = False
        if ops.device.type == "cuda":
            free, _ = torch.cuda.mem_get_info(ops.device)
            keep_input_resident = shard.input_dims[0] * in_plane_bytes <= free // 4
    chunk = max(1, min(shard.input_dims[0], max(stride, (256 << 20) // max(in_plane_bytes, 1))))
    resident = ops.empty_voxels(shard.input_dims, vdtype) if keep_input_resident else None
    clip, value_dtype = ops.effective_clip(src_dtype, vdtype)
    loaded = [False]

    def core_chunks():
        """The rank's sub-volume in z-chunks (device tensors); fills "resident" on the first walk."""
        z_lo, z_hi = (in_lo[0], in_hi[0]) if resident is not None else (core_lo[0], core_hi[0])
        for z0 in range(z_lo, z_hi, chunk):
            z1 = min(z0 + chunk, z_hi)
            if resident is None:
                yield read((z0, core_lo[1], core_lo[2]), (z1, core_hi[1], core_hi[2])).to(ops.device, non_blocking=True)
                continue
            if not loaded[0]:
                resident[z0 - in_lo[0]:z1 - in_lo[0]].copy_(read((z0, in_lo[1], in_lo[2]), (z1, in_hi[1], in_hi[2])),
                                                            non_blocking=True)
            a, b = max(z0, core_lo[0]), min(z1, core_hi[0])
            if b > a:
                yield resident[(slice(a - in_lo[0], b - in_lo[0]),
                                slice(core_lo[1] - in_lo[1], core_hi[1] - in_lo[1]),
                                slice(core_lo[2] - in_lo[2], core_hi[2] - in_lo[2]))]
        loaded[0] = True

    def histogram(pass_index=0, prefix=0):
        hist = torch.zeros(65536, dtype=torch.int64, device=ops.device)
        for part in core_chunks():
            ops.histogram_into(hist, part, vdtype, clip, pass_index, prefix)
        if exchanges is not None:
            exchanges.reduce_histogram(hist)
        return hist.cpu().numpy()

    t_phase = time.perf_counter()
    mn, mx = ops.percentiles(histogram, vdtype, normalization_percentiles, value_dtype, clip)
    if timings is not None:
        timings["upload_histogram"] = time.perf_counter() - t_phase
        t_phase = time.perf_counter()

    # ---- pass 2: the rank's patch layers ------------------------------------------------------------
    band = pz - 2 * trim - stride            # partial sums a layer hands to the next one
    slab_d = min(pz, D)
    # deepest slab handed over at once: a layer finishes stride planes (the first one stride + trim,
    # the last one the patch depth - trim); anything deeper is cut, and so is anything that would
    # make a staging slot larger than the cap. The rule depends on the GLOBAL plane only: the ranks
    # of a grid row cut alike (their y exchange pairs the slabs up)
    max_out = max(1, min(D, max(stride + trim, pz), ops.slab_bytes_cap() // (n_channels * H * W * 4)))
    # a sink is called from ONE thread, so the slabs arrive one at a time; copies into the result
    # array are split over several threads
    # (the label arguments are passed only with a label function: device steps written without them stay valid)
    drain = ops.make_drain(n_channels * max_out * own_dims[1] * own_dims[2],
                           1 if write_block is not None else max(1, int(copy_threads)),
                           **({} if label is None else {"label_elems": max_out * own_dims[1] * own_dims[2]}))
    acc_flat = [ops.empty((n_channels * slab_d * AH * AW,)) for _ in range(2)]
    in_slab = None
    if resident is None:
        in_slab = [ops.empty_voxels((slab_d,) + tuple(shard.input_dims[1:]), vdtype) for _ in range(2)]
    pbar = None
    if progress is not None and tqdm is not None:
        pbar = tqdm(total=len(z_starts) * len(yx_starts), desc=progress)

    def acc_view(k):
        zs = z_starts[k]
        depth = min(zs + pz, D) - zs
        return acc_flat[k % 2][: n_channels * depth * AH * AW].view(n_channels, depth, AH, AW)

    own_rows = (slice(None), slice(None), slice(own_lo[1] - acc_lo[1], own_hi[1] - acc_lo[1]),
                slice(own_lo[2] - acc_lo[2], own_hi[2] - acc_lo[2]))

    def consumers(z0, z1):
        """Host jobs for output planes [z0, z1) once they sit in staging memory."""
        lo, hi = (z0, own_lo[1], own_lo[2]), (z1, own_hi[1], own_hi[2])

        def make(view):
            if write_block is not None:
                return [lambda: write_block(lo, hi, view if affinity_mode and label is None else view[0])]
            # the copy into the pageable result is split over the threads
            pieces = max(1, min(int(copy_threads), z1 - z0))
            jobs = []
            for i in range(pieces):
                a = z0 + (z1 - z0) * i // pieces
                b = z0 + (z1 - z0) * (i + 1) // pieces
                jobs.append(lambda a=a, b=b: np.copyto(res4[:, a - own_lo[0]:b - own_lo[0]],
                                                       view[:, a - z0:b - z0]))
            return jobs
        return make

    def emit(z0, z1, sums=None, s0=0, s1=0):
        """Planes [z0, z1) are final once divided: in cuts of max_out planes, the owned rows of
        "sums" (all accumulator rows of planes [s0, s1); planes outside stay 0, and so does
        everything without "sums") go into a zeroed output slab, are divided and handed over."""
        for a in range(z0, z1, max_out):
            b = min(a + max_out, z1)

            def fill(out, a=a, b=b):
                if sums is None:
                    return
                lo, hi = max(a, s0), min(b, s1)
                if hi > lo:
                    out[:, lo - a:hi - a].copy_(sums[:, lo - s0:hi - s0][own_rows])
                ops.finalize(out, (a, own_lo[1], own_lo[2]))

            drain.emit((n_channels, b - a, own_dims[1], own_dims[2]), fill, consumers(a, b),
                       **({} if label is None else {"label": lambda out, slot, a=a, b=b: label(a, b, out, slot)}))

    try:
        final_lo = own_lo[0]
        cur = zs = hi = None
        for k, zs in enumerate(z_starts):
            hi = min(zs + pz, D)
            cur = acc_view(k)
            # -- input planes [zs, hi) of the rank's block
            if resident is not None:
                voxels, vox_origin = resident, in_lo
            else:
                slab, old = in_slab[k % 2], in_slab[(k + 1) % 2]
                have = 0
                if k > 0:    # planes shared with the previous layer move on the device
                    zp = z_starts[k - 1]
                    have = max(0, min(zp + pz, D) - zs)
                    if have > 0:
                        slab[:have].copy_(old[zs - zp: zs - zp + have])
                if hi - zs > have:
                    slab[have:hi - zs].copy_(read((zs + have, in_lo[1], in_lo[2]), (hi, in_hi[1], in_hi[2])),
                                             non_blocking=True)
                voxels, vox_origin = slab[: hi - zs], (zs, in_lo[1], in_lo[2])
            # -- this layer's accumulator continues the previous layer's overlap band
            cur.zero_()
            if k > 0 and band > 0:
                zp = z_starts[k - 1]
                b0 = zs + trim
                b1 = min(b0 + band, D, zp + pz)
                if b1 > b0:
                    cur[:, b0 - zs:b1 - zs].copy_(acc_view(k - 1)[:, b0 - zp:b1 - zp])
            ops.run_layer(voxels, vox_origin, src_dtype, vdtype, [(zs, y, x) for y, x in yx_starts], cur,
                          (zs, acc_lo[1], acc_lo[2]), mn, mx, pbar=pbar)
            # -- planes of the rank's region no later layer of it touches
            last = k + 1 == len(z_starts)
            final_hi = own_hi[0] if last else min(z_starts[k + 1] + trim, own_hi[0])
            if final_hi > final_lo:
                if exchanges is None:
                    emit(final_lo, final_hi, cur, zs, hi)
                else:
                    exchanges.finished(cur, zs, hi, final_lo, final_hi, emit)
                final_lo = final_hi
        if cur is None:      # no patch fits (a dimension <= overlap): zeros, like the reference
            emit(final_lo, own_hi[0])
        elif exchanges is not None:
            exchanges.last_layer_done(cur, zs, hi, emit)
        if timings is not None:
            ops.synchronize()
            timings["layers"] = time.perf_counter() - t_phase
            t_phase = time.perf_counter()
        drain.drain()
        if timings is not None:
            timings["drain"] = time.perf_counter() - t_phase
    finally:
        drain.close()
        if pbar is not None:
            pbar.close()


def _open_volume(source, shape, dtype):
    """predict_streaming's "source" as (read_box, (D, H, W), voxel dtype, whole): "whole" is the
    image itself where it is an in-memory array, else None."""
    if callable(source) and not hasattr(source, "shape"):
        if shape is None or dtype is None:
            raise ValueError("a read_block function needs shape= and dtype=")
        vshape = tuple(int(v) for v in shape)
        if len(vshape) != 3:
            raise ValueError(f"expected a 3-D shape, got {vshape}")
        return _plane_reader(source, vshape), vshape, np.dtype(dtype), None
    src = _ArraySource(source if hasattr(source, "shape") else np.asarray(source))
    in_memory = isinstance(src.arr, np.ndarray) and not isinstance(src.arr, np.memmap)
    return src, src.shape, src.dtype, src.arr if in_memory else None


def _hip_device(model):
    device = next(model.parameters()).device
    if device.type != "cuda":
        raise RuntimeError(
            "predict (MI355X) has no CPU path: the model must be on a HIP device, "
            f"got {device}"
        )
    return device


def _stream_whole_volume(volume, model, affinity_mode, batch_size, brightness_clip, normalization_percentiles,
                         patch_shape, overlap, trim, verbose, n_streams, out_dtype, write_block, **sink):
    """run_slab_pipeline for a device that has the volume "volume" (from _open_volume) to itself:
    the 1 x 1 grid, z-slab sinks. "sink": further keyword arguments of run_slab_pipeline."""
    read_box, vshape, src_dtype, whole = volume
    plan = SlidingWindow(vshape, patch_shape, overlap, trim)
    ops = DeviceShardOps(model, plan, 3 if affinity_mode else 1, batch_size, brightness_clip, n_streams,
                         out_dtype == np.float16, sink["copy_threads"])
    if write_block is not None:
        sink["write_block"] = lambda lo, hi, block: write_block(lo[0], hi[0], block)
    with torch.cuda.device(ops.device):
        run_slab_pipeline(ops, _WholeVolume(plan), read_box, src_dtype, ops.storage(src_dtype, whole=whole),
                          normalization_percentiles, affinity_mode=affinity_mode,
                          progress="Predict" if verbose else None, **sink)


def _label_predicted_slabs(labeller, finish_key, write_block, keep_labels_resident, timings, volume, model,
                           affinity_mode, *window, **pipeline):
    """
    The streaming driver's feeder for affinities that are predicted here:
    _stream_whole_volume with a "label" callback that pushes every finished,
    divided slab into "labeller" (segmentation.py) where predict_streaming
    would have started its download. "window": _stream_whole_volume's
    arguments from batch_size to n_streams; "pipeline": its keyword arguments.
    timings[finish_key] gets the wall seconds from the last slab to the final
    labels.
    """
    sink = _LabelSink(labeller, write_block, keep_labels_resident)
    _, height, width = labeller.shape

    def label(z0, z1, out, slot):
        aff = out if affinity_mode else out[0]
        if sink.resident is not None:
            labeller.push(aff, z0, sink.resident[z0:z1])
            return None
        labels = slot[: (z1 - z0) * height * width].view(z1 - z0, height, width)
        return labeller.push(aff, z0, labels).view((1,) + tuple(labels.shape))

    _stream_whole_volume(volume, model, affinity_mode, *window, np.float32, write_block, result=sink.result,
                         label=label, timings=timings, **pipeline)
    t0 = time.perf_counter()
    # the second pass, where there is one, goes through the device in pieces of one pinned staging slot
    out = sink.finish(max(1, PINNED_SLOT_BYTES // (4 * height * width)))
    if timings is not None:
        timings[finish_key] = time.perf_counter() - t0
    return out


def predict_streaming(
    source,
    model,
    affinity_mode=True,
    batch_size=16,
    brightness_clip=1000,
    normalization_percentiles=(1, 99.9),
    patch_shape=(96, 96, 96),
    overlap=(32, 32, 32),
    trim=8,
    verbose=True,
    *,
    shape=None,
    dtype=None,
    write_block=None,
    keep_input_resident=None,
    n_streams=DEFAULT_STREAMS,
    copy_threads=4,
    timings=None,
    out_dtype=np.float32,
):
    """
    predict() for volumes that are read and written in z-slabs: the same
    results, bit for bit, without ever holding the whole input, the whole
    accumulator or the whole result on the device -- and, when "write_block"
    is given, not on the host either.

    The reference needs the whole image as one array (inference.py:79) and
    keeps a float64 normalised copy plus the float32 accumulators in host
    memory (22 B/voxel); its readers (img_util.py:25-121) hand out lazily
    chunked zarr / N5 / TIFF arrays that are sliced on demand. This function
    consumes exactly that interface and runs run_slab_pipeline (the two
    passes are described there) on the 1 x 1 rank grid: every z-chunk is read
    once for the percentiles and once for its patch layer, and finished slabs
    leave the device while the next layer computes.

    Parameters
    ----------
    source : array-like or Callable[[int, int], numpy.ndarray]
        The image: anything that slices like a 3-D (or 1 x 1 x D x H x W) numpy
        array (ndarray, numpy.memmap, a zarr array), or a function
        read_block(z0, z1) returning planes [z0, z1) as a (z1 - z0, H, W) array,
        in which case "shape" and "dtype" are required.
    model : torch.nn.Module
        Model on a HIP device (see predict).
    affinity_mode, batch_size, brightness_clip, normalization_percentiles,
    patch_shape, overlap, trim, verbose
        As in predict (inference.py:29-40), same defaults.
    shape : Tuple[int], optional
        (D, H, W) of the image when "source" is a function.
    dtype : numpy.dtype, optional
        Voxel dtype when "source" is a function.
    write_block : Callable[[int, int, numpy.ndarray], None], optional
        Receives every finished output slab once, in z order, as
        write_block(z0, z1, block) with block float32 (C, z1 - z0, H, W) (or
        (z1 - z0, H, W) if not affinity_mode); the block is only valid during
        the call. Without it the full result array is returned.
    keep_input_resident : bool, optional
        Keep the uploaded image in HBM between the two passes instead of
        reading it twice. Default: True if it takes less than a quarter of
        the free device memory.
    n_streams : int, optional
        As in predict.
    copy_threads : int, optional
        Host threads that move finished slabs out of pinned memory. Default 4.
    timings : dict, optional
        Filled with the wall seconds of the phases ("upload_histogram",
        "layers", "drain"); measuring them synchronises the device twice.
    out_dtype : numpy.dtype, optional
        As in predict: numpy.float16 rounds every finished slab on the device,
        so the result array / the blocks handed to "write_block" are float16.

    Returns
    -------
    numpy.ndarray or None
        The prediction (see predict), or None when "write_block" is given.
    """
    _hip_device(model)
    out_dtype = _checked_out_dtype(out_dtype)
    volume = _open_volume(source, shape, dtype)
    result = None
    if write_block is None:
        result = np.empty(((3,) if affinity_mode else ()) + volume[1], dtype=out_dtype)
    _stream_whole_volume(volume, model, affinity_mode, batch_size, brightness_clip, normalization_percentiles,
                         patch_shape, overlap, trim, verbose, n_streams, out_dtype, write_block, result=result,
                         copy_threads=copy_threads, keep_input_resident=keep_input_resident, timings=timings)
    return result


def predict_components_streaming(
    source,
    model,
    threshold=0.5,
    min_segment_size=100,
    affinity_mode=True,
    batch_size=16,
    brightness_clip=1000,
    normalization_percentiles=(1, 99.9),
    patch_shape=(96, 96, 96),
    overlap=(32, 32, 32),
    trim=8,
    verbose=True,
    *,
    shape=None,
    dtype=None,
    write_block=None,
    keep_input_resident=None,
    n_streams=DEFAULT_STREAMS,
    copy_threads=4,
    timings=None,
    id_capacity=None,
    keep_labels_resident=None,
):
    """
    predict_streaming followed by affinities_to_components without the
    affinities ever leaving the device: every finished, divided slab is
    labelled right where predict_streaming would have started its download
    (ComponentsStream), and only int32 labels travel -- 4 bytes
    per voxel instead of 12. The result equals, bit for bit,
    affinities_to_components(predict_streaming(...), threshold,
    min_segment_size) on the whole volume, which neither the device nor this
    function ever holds as affinities.

    Parameters
    ----------
    source, model
        As in predict_streaming.
    threshold, min_segment_size
        As in affinities_to_components. With affinity_mode=False the model's
        output is a foreground map and is labelled as one.
    affinity_mode, batch_size, brightness_clip, normalization_percentiles,
    patch_shape, overlap, trim, verbose, shape, dtype, keep_input_resident,
    n_streams, copy_threads, timings
        As in predict_streaming; "timings" also gets "components_finish", the
        wall seconds from the last slab to the final labels.
    write_block : Callable[[int, int, numpy.ndarray], None], optional
        Receives every slab once, in z order, as write_block(z0, z1, block)
        with block int32 (z1 - z0, H, W) of PROVISIONAL ids, valid during the
        call only; the function then returns the table that maps them to
        final labels (the two-pass contract of chunked segmentation).
    id_capacity : int, optional
        See ComponentsStream.
    keep_labels_resident : bool, optional
        Without "write_block": keep the provisional labels in HBM (4 B/voxel),
        relabel them there and download them once. Default: True if they take
        less than a quarter of the free device memory. Otherwise every slab
        is downloaded with its provisional ids while later layers compute and
        relabelled in a second device pass over the downloaded array.

    Returns
    -------
    numpy.ndarray
        int32 (D, H, W) final labels; or, with "write_block", the tuple
        (table, K): table int32 with final = table[provisional], K kept
        components.
    """
    device = _hip_device(model)
    volume = _open_volume(source, shape, dtype)
    cs = ComponentsStream(volume[1], threshold, min_segment_size, foreground=not affinity_mode, device=device,
                          id_capacity=id_capacity)
    return _label_predicted_slabs(
        _ComponentsLabeller(cs), "components_finish", write_block, keep_labels_resident, timings,
        volume, model, affinity_mode, batch_size, brightness_clip, normalization_percentiles, patch_shape, overlap,
        trim, verbose, n_streams, copy_threads=copy_threads, keep_input_resident=keep_input_resident)


def predict_agglomerate_streaming(
    source,
    model,
    agglomeration_thresholds=[0.6, 0.8, 0.9],
    min_segment_size=100,
    batch_size=16,
    brightness_clip=1000,
    normalization_percentiles=(1, 99.9),
    patch_shape=(96, 96, 96),
    overlap=(32, 32, 32),
    trim=8,
    verbose=True,
    *,
    fragment_threshold=0.5,
    affinity_mode=True,
    shape=None,
    dtype=None,
    write_block=None,
    keep_input_resident=None,
    n_streams=DEFAULT_STREAMS,
    copy_threads=4,
    timings=None,
    id_capacity=None,
    edge_capacity=None,
    keep_labels_resident=None,
    fragments="components",
    aff_threshold_low=0.1,
    aff_threshold_high=0.9999,
    premerge_size=0,
    premerge_rounds=4,
    device_merge_rounds=0,
):
    """
    predict_streaming followed by agglomerate_affinities without the
    affinities ever leaving the device: every finished, divided slab is
    labelled (ComponentsStream with no size filter) and added to the region
    graph of provisional ids (RegionGraphStream) right where
    predict_streaming would have started its download, and only int32 labels
    travel. The result equals, bit for bit,
    agglomerate_affinities(predict_streaming(...), agglomeration_thresholds,
    min_segment_size, fragment_threshold=fragment_threshold) on the whole
    volume, which neither the device nor this function ever holds as
    affinities.

    Parameters
    ----------
    source, model
        As in predict_streaming.
    agglomeration_thresholds, min_segment_size, fragment_threshold
        As in agglomerate_affinities.
    batch_size, brightness_clip, normalization_percentiles, patch_shape,
    overlap, trim, verbose, shape, dtype, keep_input_resident, n_streams,
    copy_threads, timings
        As in predict_streaming; "timings" also gets "agglomerate_finish", the
        wall seconds from the last slab to the final labels.
    affinity_mode : bool, optional
        Must be True: a foreground map has no affinities to score.
    write_block : Callable[[int, int, numpy.ndarray], None], optional
        Receives every slab once, in z order, as write_block(z0, z1, block)
        with block int32 (z1 - z0, H, W) of PROVISIONAL ids, valid during the
        call only; the function then returns the table that maps them to
        segment labels.
    id_capacity : int, optional
        See ComponentsStream.
    edge_capacity : int, optional
        See RegionGraphStream.
    keep_labels_resident : bool, optional
        As in predict_components_streaming.
    fragments, aff_threshold_low, aff_threshold_high, premerge_size,
    premerge_rounds, device_merge_rounds
        As in agglomerate_affinities; the result then equals that call with
        the same values on predict_streaming's affinities, bit for bit.
        fragments="watershed" labels the slabs with a WatershedStream
        (DESIGN 6s). With the defaults nothing but what is described above
        is launched.

    Returns
    -------
    numpy.ndarray
        int32 (D, H, W) segment labels; or, with "write_block", the tuple
        (table, S): table int32 with segment = table[provisional], S kept
        segments.
    """
    thresholds = list(agglomeration_thresholds)
    _last_threshold(thresholds)
    low, high, merging = _checked_fragment_options(fragments, aff_threshold_low, aff_threshold_high, premerge_size,
                                                   premerge_rounds, device_merge_rounds)
    if not affinity_mode:
        raise ValueError("predict_agglomerate_streaming needs affinity_mode=True: "
                         "a foreground map has no affinities to score")
    device = _hip_device(model)
    volume = _open_volume(source, shape, dtype)
    cs = _fragment_stream(fragments, volume[1], fragment_threshold, low, high, device, id_capacity)
    rgs = RegionGraphStream(volume[1], device=device, id_capacity=cs.id_capacity, edge_capacity=edge_capacity)
    return _label_predicted_slabs(
        _AgglomerationLabeller(cs, rgs, thresholds, min_segment_size, **merging), "agglomerate_finish", write_block,
        keep_labels_resident, timings,
        volume, model, True, batch_size, brightness_clip, normalization_percentiles, patch_shape, overlap,
        trim, verbose, n_streams, copy_threads=copy_threads, keep_input_resident=keep_input_resident)
