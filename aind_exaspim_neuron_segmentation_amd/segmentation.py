"""
Labels from affinities on the MI355X: what follows the prediction section
of the reference's ``inference.py`` (affinities_to_segmentation: 196-237)
with exactly defined parts.

* connected components of thresholded affinities (affinities_to_components,
  DESIGN 6c) and watershed fragments (watershed_fragments);
* the region graph of a labelled volume, the pre-merge of tiny fragments and
  the exact contraction of dominant edges on the device, and the
  mean-affinity agglomeration on the host (region_graph,
  premerge_region_graph, contract_dominant_edges, agglomerate,
  agglomerate_affinities);
* what the reference's skeletonize (257-291) starts from: the enclosed
  cavities of every label closed (fill_holes), then the
  distance-to-boundary field of all labels and the per-label table of sizes,
  boxes and field maxima (distance_to_boundary, segment_table);
* TEASAR's next whole-volume stage: the 26-connected geodesic distance of
  every voxel from its label's source, bit for bit a float32 Dijkstra, and
  each label's farthest voxel (geodesic_field); then the parental
  field of that field by an order-free definition of its own and the paths
  from the sources to given targets (geodesic_parents, trace_paths, DESIGN
  6m);
* the same for volumes that arrive in z slabs (ComponentsStream,
  RegionGraphStream) and the one streaming driver behind
  affinities_to_components_streaming and agglomerate_affinities_streaming
  here and predict_components_streaming and predict_agglomerate_streaming
  in inference.py;
* how much two label volumes differ: the overlap table of ordered label
  pairs on the device, whole or piece by piece, and the variation of
  information, adapted Rand error and largest-overlap agreement read off it
  on the host (label_overlaps, OverlapStream, label_overlaps_streaming,
  compare_segmentations, overlap_scores).

Every name is importable from inference.py as before. This module does not
import inference.py and reads none of its plan switches. There is no CPU
fallback: a tensor on a CPU device raises.
"""

import ctypes
import time

import numpy as np
import torch

from aind_exaspim_neuron_segmentation_amd import _native
from aind_exaspim_neuron_segmentation_amd._device import _carrier, _stream

_AFF_CODES = {torch.float32: _native.AFF_F32, torch.float16: _native.AFF_F16}
_AFF_DTYPES = (np.float32, np.float16)


def _upload_device(fn):
    """cuda:0, where numpy arguments are uploaded to; RuntimeError in the name of the public function "fn"
    if there is no HIP device."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"{fn} (MI355X) has no CPU path and no HIP device is present")
    return torch.device("cuda:0")


def _on_device(a, fn, what="affinities", dtypes=_AFF_DTYPES, check=None, arrays_only=False):
    """
    The front matter of the single-shot entry points: a torch tensor is
    returned as it is; a numpy array goes through the dtype whitelist, then
    through "check" (the caller's own test of its shape, if any), and is
    uploaded to cuda:0. Anything else raises TypeError, or with arrays_only
    is returned for the ..._on_device function behind "fn" to refuse.
    """
    if isinstance(a, np.ndarray):
        if a.dtype not in dtypes:
            raise TypeError(f"{what} must be {' or '.join(str(np.dtype(d)) for d in dtypes)}, got {a.dtype}")
        if check is not None:
            check(a)
        device = _upload_device(fn)
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if not arrays_only and not isinstance(a, torch.Tensor):
        raise TypeError(f"{what} must be a torch tensor or a numpy array, got {type(a).__name__}")
    return a


def _workspace_bytes(name, *args):
    """What the library's size query "name" (an ..._workspace_bytes function) asks for these arguments; a 0 is
    its refusal, raised as ValueError with the library's message."""
    need = getattr(_native.lib(), name)(*args)
    if need == 0:
        raise ValueError(_native.last_error())
    return need


def _downloaded(out, device, keep_on_device=False):
    """The download tail: the tuple "out" of tensors on "device" as numpy arrays, or as it is if they are to stay."""
    if keep_on_device:
        return out
    with torch.cuda.device(device):
        return tuple(t.cpu().numpy() for t in out)


def _checked_integer(fn, name, value, least=None, most_bits=None, optional=False):
    """
    The one check of an integer argument "name" of the public function "fn":
    TypeError unless it is an int or a numpy integer (a bool is neither),
    ValueError below "least" or above 2^most_bits - 1. None passes iff
    "optional". n_labels' "negative" message alone names no function; tests
    match on it as it stands.
    """
    if value is None and optional:
        return
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"{fn}: {name} must be an integer, got {type(value).__name__}")
    if least is not None and value < least:
        who = name if name == "n_labels" else f"{fn}: {name}"
        raise ValueError(f"{who} must {'not be negative' if least == 0 else f'be at least {least}'}, got {value}")
    if most_bits is not None and value > 2**most_bits - 1:
        raise ValueError(f"{fn}: {name} must be at most 2^{most_bits} - 1, got {value}")


def _checked_real(fn, name, value):
    """The one check of a real argument: TypeError unless it is a real number, ValueError unless finite and >= 0."""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise TypeError(f"{fn}: {name} must be a real number, got {type(value).__name__}")
    if not np.isfinite(value) or value < 0:
        raise ValueError(f"{fn}: {name} must be finite and not negative, got {value}")


def _apply_table(labels, table):
    """labels[i] = table[labels[i]] in place (exaspim_apply_label_table), both int32 on one device; returns labels."""
    with torch.cuda.device(labels.device):
        _native.check(
            _native.lib().exaspim_apply_label_table(labels.data_ptr(), labels.numel(), table.data_ptr(),
                                                    table.numel(), _stream(labels.device)),
            "exaspim_apply_label_table",
        )
    return labels


def _label_on_device(affinities, workspace_bytes, kernel, middle):
    """
    The common tail of _components_on_device and _watershed_on_device, after
    their argument checks: sizes the workspace, allocates labels, count and
    workspace and launches "kernel" (both are names of library functions).
    "middle" maps the int3 of the dims to the kernel's arguments between the
    affinities' dtype code and the labels pointer.
    """
    dims = tuple(int(v) for v in affinities.shape[-3:])
    if min(dims) < 1:
        raise ValueError(f"empty volume {dims}")
    affinities = affinities.contiguous()
    device = affinities.device
    lib = _native.lib()
    need = _workspace_bytes(workspace_bytes, _native.int3(dims))
    with torch.cuda.device(device):
        labels = torch.empty(dims, dtype=torch.int32, device=device)
        count = torch.empty(1, dtype=torch.int32, device=device)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        _native.check(
            getattr(lib, kernel)(affinities.data_ptr(), _AFF_CODES[affinities.dtype], *middle(_native.int3(dims)),
                                 labels.data_ptr(), count.data_ptr(), workspace.data_ptr(), need, _stream(device)),
            kernel,
        )
    return labels, count


def _components_on_device(affinities, threshold=0.5, min_segment_size=100):
    """
    exaspim_components on a device tensor: the labels and the number of kept
    segments, both left on the device (nothing is synchronised).

    Parameters
    ----------
    affinities : torch.Tensor
        float32 or float16 tensor on a HIP device, (3, D, H, W) affinities or
        (D, H, W) foreground probabilities.
    threshold : float, optional
        Rounded to float32; an edge (a voxel, in foreground mode) is on iff
        its value is >= it. Default is 0.5.
    min_segment_size : int, optional
        Components are kept iff they have more voxels than this. Default is 100.

    Returns
    -------
    labels : torch.Tensor
        int32 (D, H, W): 0 for background, 1 ... K in raster order of each
        component's first voxel.
    count : torch.Tensor
        int32 (1,): K.
    """
    if not isinstance(affinities, torch.Tensor):
        raise TypeError(f"_components_on_device needs a torch tensor, got {type(affinities).__name__}")
    if affinities.dtype not in _AFF_CODES:
        raise TypeError(f"affinities must be float32 or float16, got {affinities.dtype}")
    if affinities.dim() == 4:
        if affinities.shape[0] != 3:
            raise ValueError(f"4-D affinities must be (3, D, H, W), got {tuple(affinities.shape)}")
        channels = 3
    elif affinities.dim() == 3:
        channels = 1
    else:
        raise ValueError("affinities must be (3, D, H, W) or a (D, H, W) foreground map, "
                         f"got {affinities.dim()} dimensions")
    if affinities.device.type != "cuda":
        raise RuntimeError(
            "affinities_to_components (MI355X) has no CPU path: the tensor must be on a HIP device, "
            f"got {affinities.device}"
        )
    return _label_on_device(
        affinities, "exaspim_components_workspace_bytes", "exaspim_components",
        lambda dims: (channels, dims, float(np.float32(threshold)), int(min_segment_size)))


def affinities_to_components(affinities, threshold=0.5, min_segment_size=100, *,
                             return_device_tensor=False):
    """
    Labels the connected components of thresholded affinities on the device
    and removes small ones.

    What this is: the affinity graph in the reference's own convention
    (img_util.get_affinity_channels, img_util.py:159-216: channel c at voxel v
    is the edge between v and v + e_c, e = z, y, x; the entries at the last
    index along axis c are ignored) cut at "threshold", its connected
    components, then the reference's size filter (img_util.py:555-558: kept
    iff size > min_segment_size) and a contiguous renumbering in raster order
    of each component's first voxel. A voxel without an on edge is background.
    A 3-D input is a foreground map: voxels >= threshold are on and
    6-connected, and an on voxel alone is a component of size 1.

    What this is not: waterz's watershed / agglomeration, which the
    reference's affinities_to_segmentation runs (inference.py:196-237). That
    stays a CPU library; nothing here merges or splits by affinity scores.

    Parameters
    ----------
    affinities : torch.Tensor or numpy.ndarray
        float32 or float16, (3, D, H, W) or (D, H, W): a tensor on a HIP
        device (e.g. from predict(..., return_device_tensor=True)), or a numpy
        array, which is uploaded to cuda:0. D * H * W must not exceed 2^31 - 1.
    threshold : float, optional
        Rounded to float32; on iff float32(value) >= it, NaN is off. Default
        is 0.5.
    min_segment_size : int, optional
        Default is 100.
    return_device_tensor : bool, optional
        Return the labels as a device tensor instead of a numpy array.
        Default is False.

    Returns
    -------
    numpy.ndarray or torch.Tensor
        int32 (D, H, W) labels: 4 bytes per voxel leave the device instead of
        the 12 of the affinities.
    """
    def check(array):
        if array.ndim not in (3, 4):
            raise ValueError("affinities must be (3, D, H, W) or a (D, H, W) foreground map, "
                             f"got {array.ndim} dimensions")

    affinities = _on_device(affinities, "affinities_to_components", check=check, arrays_only=True)
    labels, _ = _components_on_device(affinities, threshold, min_segment_size)
    if return_device_tensor:
        return labels
    return labels.cpu().numpy()


# --- Watershed fragments ---
def _check_watershed_shape(affinities):
    if affinities.ndim != 4 or affinities.shape[0] != 3:
        raise ValueError(f"watershed_fragments needs (3, D, H, W) affinities, got {tuple(affinities.shape)}; "
                         "a foreground map has no affinities")


def _watershed_on_device(affinities, low=0.1, high=0.9999, min_segment_size=0):
    """
    exaspim_watershed_fragments on a device tensor: the labels and the number
    of kept fragments, both left on the device (nothing is synchronised).

    Parameters
    ----------
    affinities : torch.Tensor
        float32 or float16 (3, D, H, W) tensor on a HIP device.
    low, high : float, optional
        Rounded to float32; see watershed_fragments. Defaults are 0.1 and
        0.9999.
    min_segment_size : int, optional
        Fragments are kept iff they have more voxels than this. Default is 0.

    Returns
    -------
    labels : torch.Tensor
        int32 (D, H, W): 0 for background, 1 ... K in raster order of each
        fragment's first voxel.
    count : torch.Tensor
        int32 (1,): K.
    """
    if not isinstance(affinities, torch.Tensor):
        raise TypeError(f"_watershed_on_device needs a torch tensor, got {type(affinities).__name__}")
    if affinities.dtype not in _AFF_CODES:
        raise TypeError(f"affinities must be float32 or float16, got {affinities.dtype}")
    _check_watershed_shape(affinities)
    low, high = float(np.float32(low)), float(np.float32(high))
    if low != low or high != high:
        raise ValueError(f"aff_threshold_low and aff_threshold_high must not be NaN, got {low} and {high}")
    if affinities.device.type != "cuda":
        raise RuntimeError(
            "watershed_fragments (MI355X) has no CPU path: the tensor must be on a HIP device, "
            f"got {affinities.device}"
        )
    return _label_on_device(
        affinities, "exaspim_watershed_workspace_bytes", "exaspim_watershed_fragments",
        lambda dims: (dims, low, high, int(min_segment_size)))


def watershed_fragments(affinities, aff_threshold_low=0.1, aff_threshold_high=0.9999, min_segment_size=0, *,
                        return_device_tensor=False):
    """
    Labels the basins of a steepest-ascent watershed on the affinity graph on
    the device: the fragments the reference's affinities_to_segmentation
    starts from (inference.py:224-229, waterz.agglomerate(...,
    aff_threshold_low=0.1, aff_threshold_high=0.9999)).

    What this is, exactly: in the project's edge convention (channel c at
    voxel v is the edge between v and v + e_c, e = z, y, x; the entries at the
    last index along axis c are ignored), (1) an edge is eligible iff
    float32(a) > aff_threshold_low, strictly (NaN never, +inf always); (2) a
    voxel's steepest edge is its eligible incident edge of largest value,
    among equal values the one whose other end has the smallest C-order
    linear index (the order -z, -y, -x, +x, +y, +z); (3) an eligible edge is
    on iff a >= aff_threshold_high or it is the steepest edge of one of its
    two ends; (4) fragments are the connected components of the on edges, a
    voxel without an on edge is background, a fragment is kept iff it has
    more than max(min_segment_size, 1) voxels, and kept fragments are
    numbered 1 ... K in raster order of each fragment's first voxel. No
    relation between the two thresholds is required: with high <= low every
    eligible edge is on.

    What equals what: this equals the serial steepest-ascent watershed
    (direction bits, plateau corners, breadth-first plateau division, pointer
    chasing with ids in raster order) label for label on tie-free input, i.e.
    where no voxel has two equal maximal eligible edges below
    aff_threshold_high, by the oracle in tests/ (watershed_ref.py). Where
    such ties exist the serial algorithm depends on its visiting order and
    the two differ; this definition depends on no order. It has not been
    compared with waterz itself, which also reads the same array as the
    edges v -- v - e_c; the project keeps the convention the network was
    trained in.

    Parameters
    ----------
    affinities : torch.Tensor or numpy.ndarray
        float32 or float16 (3, D, H, W): a tensor on a HIP device (e.g. from
        predict(..., return_device_tensor=True)), or a numpy array, which is
        uploaded to cuda:0. D * H * W must not exceed 2^31 - 1. A 3-D
        foreground map has no affinities and raises ValueError.
    aff_threshold_low, aff_threshold_high : float, optional
        Rounded to float32, not NaN. Defaults are 0.1 and 0.9999, the
        reference's.
    min_segment_size : int, optional
        Default is 0: every fragment is kept (the reference filters after
        the agglomeration).
    return_device_tensor : bool, optional
        Return the labels as a device tensor instead of a numpy array.
        Default is False.

    Returns
    -------
    numpy.ndarray or torch.Tensor
        int32 (D, H, W) labels.
    """
    affinities = _on_device(affinities, "watershed_fragments", check=_check_watershed_shape, arrays_only=True)
    labels, _ = _watershed_on_device(affinities, aff_threshold_low, aff_threshold_high, min_segment_size)
    if return_device_tensor:
        return labels
    return labels.cpu().numpy()


# --- Mean-affinity agglomeration of components ---
# Slots of the region graph's accumulator unless the caller says otherwise (edge_capacity): 48 bytes of
# device memory each (24 in the table, 24 in the compacted list), so 192 MiB at most; a small volume
# gets the next power of two above twice the 3 edges per voxel it can have at all.
DEFAULT_EDGE_CAPACITY = 1 << 22


def _default_edge_capacity(voxels):
    want = 6 * int(voxels)
    return min(DEFAULT_EDGE_CAPACITY, 1 << max(want - 1, 0).bit_length())


def _region_graph_device(labels, affinities, n_labels, edge_capacity=None):
    """
    exaspim_region_graph on device tensors and the one read of its state: the
    graph stays on the device.

    Returns
    -------
    edges, counts, sums : torch.Tensor
        int32 (capacity, 2), int64 (capacity,), int64 (capacity,) holding
        uint64 bits: the first n_edges rows in an unspecified order.
    sizes : torch.Tensor
        int64 (n_labels + 1,).
    n_edges : int
    capacity : int

    Raises
    ------
    RuntimeError
        If the volume has more distinct pairs of adjacent labels than
        edge_capacity.
    """
    if labels.dtype != torch.int32 or labels.dim() != 3:
        raise TypeError(f"labels must be a 3-D int32 tensor, got {labels.dtype} with {labels.dim()} dimensions")
    if affinities.dtype not in _AFF_CODES:
        raise TypeError(f"affinities must be float32 or float16, got {affinities.dtype}")
    dims = tuple(int(v) for v in labels.shape)
    if affinities.dim() != 4 or tuple(affinities.shape) != (3,) + dims:
        raise ValueError(f"affinities must be (3, D, H, W) = {(3,) + dims}, got {tuple(affinities.shape)}; "
                         "a foreground map has no affinities to score")
    if min(dims) < 1:
        raise ValueError(f"empty volume {dims}")
    if labels.device.type != "cuda" or affinities.device != labels.device:
        raise RuntimeError("region_graph (MI355X) has no CPU path: labels and affinities must be on one HIP "
                           f"device, got {labels.device} and {affinities.device}")
    n_labels = int(n_labels)
    if n_labels < 0:
        raise ValueError(f"n_labels must not be negative, got {n_labels}")
    capacity = _default_edge_capacity(np.prod(dims, dtype=np.int64)) if edge_capacity is None else int(edge_capacity)
    labels, affinities = labels.contiguous(), affinities.contiguous()
    device = labels.device
    lib = _native.lib()
    need = _workspace_bytes("exaspim_region_graph_workspace_bytes", _native.int3(dims), n_labels, capacity)
    with torch.cuda.device(device):
        edges = torch.empty((capacity, 2), dtype=torch.int32, device=device)
        counts = torch.empty(capacity, dtype=torch.int64, device=device)
        sums = torch.empty(capacity, dtype=torch.int64, device=device)   # uint64 bits
        sizes = torch.empty(n_labels + 1, dtype=torch.int64, device=device)
        state = torch.empty(2, dtype=torch.int32, device=device)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        _native.check(
            lib.exaspim_region_graph(labels.data_ptr(), affinities.data_ptr(), _AFF_CODES[affinities.dtype],
                                     _native.int3(dims), n_labels, capacity, edges.data_ptr(), counts.data_ptr(),
                                     sums.data_ptr(), sizes.data_ptr(), state.data_ptr(), workspace.data_ptr(),
                                     need, _stream(device)),
            "exaspim_region_graph",
        )
        n_edges, overflow = (int(v) for v in state.cpu())   # the one read of the device state
        if overflow:
            raise RuntimeError(
                f"region_graph: the volume has more pairs of adjacent labels than edge_capacity={capacity}; "
                "run it again with a larger edge_capacity (a power of two)")
    return edges, counts, sums, sizes, n_edges, capacity


def _region_graph_on_device(labels, affinities, n_labels, edge_capacity=None):
    """
    exaspim_region_graph on device tensors, then the one small download.

    Returns
    -------
    edges : numpy.ndarray
        int32 (E, 2), rows (lo, hi) sorted by (lo, hi).
    counts : numpy.ndarray
        int64 (E,): voxel edges between the two labels.
    sums : numpy.ndarray
        uint64 (E,): the sum of q(affinity) over them, q in units of 2^-24.
    sizes : numpy.ndarray
        int64 (n_labels + 1,): voxels per label, index 0 the background.

    Raises
    ------
    RuntimeError
        If the volume has more distinct pairs of adjacent labels than
        edge_capacity.
    """
    edges, counts, sums, sizes, n_edges, _ = _region_graph_device(labels, affinities, n_labels, edge_capacity)
    with torch.cuda.device(labels.device):
        return _download_graph(edges, counts, sums, sizes, n_edges)


def _download_graph(edges, counts, sums, sizes, n_edges):
    """The first n_edges rows of a device graph, and its sizes, as numpy arrays sorted by (lo, hi)."""
    edges_h = edges[:n_edges].cpu().numpy().reshape(-1, 2)
    counts_h = counts[:n_edges].cpu().numpy()
    sums_h = sums[:n_edges].cpu().numpy().view(np.uint64)
    sizes_h = sizes.cpu().numpy()
    order = np.lexsort((edges_h[:, 1], edges_h[:, 0]))   # slot order depends on arrival: sort by (lo, hi)
    return (np.ascontiguousarray(edges_h[order]), np.ascontiguousarray(counts_h[order]),
            np.ascontiguousarray(sums_h[order]), sizes_h)


def region_graph(labels, affinities, *, edge_capacity=None):
    """
    The region graph of a labelled volume on the device: for every pair of
    adjacent labels the number of voxel edges between them and the sum of
    their affinities, and the number of voxels per label.

    For every in-volume voxel edge (img_util.get_affinity_channels'
    convention: channel c at voxel v is the edge between v and v + e_c,
    e = z, y, x; the entries at the last index along axis c are ignored)
    whose two labels are positive and differ: key = (smaller, larger label),
    count[key] += 1, sum[key] += q(a) with q(a) = rint(clamp(float32(a), 0,
    1) * 2^24), NaN as 0. Counts and sums are 64-bit integers, so the result
    does not depend on the order in which the device adds them.

    Parameters
    ----------
    labels : torch.Tensor or numpy.ndarray
        int32 (D, H, W); labels <= 0 are background.
    affinities : torch.Tensor or numpy.ndarray
        float32 or float16 (3, D, H, W). Device tensors are used where they
        are; numpy arrays are uploaded to cuda:0.
    edge_capacity : int, optional
        Slots of the device hash table, a power of two. Default is the
        smaller of 2^22 and the next power of two >= 6 * D * H * W.

    Returns
    -------
    edges : numpy.ndarray
        int32 (E, 2), rows (lo, hi) sorted by (lo, hi).
    counts : numpy.ndarray
        int64 (E,).
    sums : numpy.ndarray
        uint64 (E,), in units of 2^-24: sums / counts / 2^24 is the mean
        affinity of the contact.
    sizes : numpy.ndarray
        int64 (labels.max() + 1,): voxels per label, index 0 the voxels
        labelled 0 (negative labels are counted nowhere).
    """
    labels = _on_device(labels, "region_graph", "labels", (np.int32,))
    affinities = _on_device(affinities, "region_graph")
    if labels.dtype != torch.int32 or labels.dim() != 3:
        raise TypeError(f"labels must be a 3-D int32 tensor, got {labels.dtype} with {labels.dim()} dimensions")
    n_labels = max(int(labels.max()), 0) if labels.numel() else 0
    return _region_graph_on_device(labels, affinities, n_labels, edge_capacity)


def _last_threshold(agglomeration_thresholds):
    """The threshold that decides (the reference keeps only the last segmentation, deque(maxlen=1))."""
    thresholds = [float(t) for t in agglomeration_thresholds]
    if not thresholds:
        raise ValueError("agglomeration_thresholds is empty")
    if any(t != t for t in thresholds):
        raise ValueError(f"agglomeration_thresholds holds a NaN: {thresholds}")
    if any(b < a for a, b in zip(thresholds, thresholds[1:])):
        raise ValueError(f"agglomeration_thresholds must be non-decreasing, got {thresholds}")
    return thresholds[-1]


def agglomerate(edges, counts, sums, sizes, agglomeration_thresholds=(0.6, 0.8, 0.9), min_segment_size=100):
    """
    Merges the fragments of a region graph by the mean affinity of their
    contacts (exaspim_agglomerate: host code, no device is touched).

    Among the current edges the one with the largest mean sum / count goes
    first (ties: the smaller lo, then the smaller hi, of the current root
    ids); it is merged iff sum > rint((1 - T) * 2^24) * count, T the last
    threshold rounded to float32, i.e. iff 1 - mean affinity < T; the larger
    root goes under the smaller and parallel edges to a common neighbour add
    their counts and sums. All comparisons are exact integer ones. Then a
    segment is kept iff the sizes of its fragments sum to more than
    min_segment_size, and kept segments are numbered 1 ... S by their
    smallest fragment id.

    Parameters
    ----------
    edges, counts, sums, sizes : numpy.ndarray
        What region_graph returns: K = len(sizes) - 1 fragments. Every count
        is in 1 .. 2^34, every sum at most count * 2^24, and all counts
        together add up to at most 2^39 (sixteen times the voxel edges of a
        4096 x 2048 x 2048 volume): pooled counts and sums then never wrap
        their 64 bits. A larger total raises ValueError.
    agglomeration_thresholds : sequence of float, optional
        Non-decreasing; only the last one decides. Default is (0.6, 0.8, 0.9).
    min_segment_size : int, optional
        Default is 100.

    Returns
    -------
    table : numpy.ndarray
        int32 (K + 1,): fragment id -> segment label, table[0] = 0.
    count : int
        S, the number of kept segments.
    """
    threshold = _last_threshold(agglomeration_thresholds)
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    sums = np.ascontiguousarray(sums, dtype=np.uint64)
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    if sizes.ndim != 1 or sizes.size < 1 or counts.shape != (edges.shape[0],) or sums.shape != counts.shape:
        raise ValueError("agglomerate needs edges (E, 2), counts (E,), sums (E,) and sizes (K + 1,)")
    table = np.zeros(sizes.size, np.int32)
    n_segments = ctypes.c_int32(0)
    _native.check(
        _native.lib().exaspim_agglomerate(edges.ctypes.data, counts.ctypes.data, sums.ctypes.data, edges.shape[0],
                                          sizes.ctypes.data, sizes.size - 1, float(np.float32(threshold)),
                                          int(min_segment_size), table.ctypes.data, ctypes.addressof(n_segments)),
        "exaspim_agglomerate",
    )
    return table, int(n_segments.value)


def _checked_premerge(size_floor, rounds):
    """(size_floor, rounds) as ints; ValueError for negatives and non-integers, before any device call."""
    for what, v, least in (("the size floor", size_floor, 0), ("the number of rounds", rounds, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what} must be an integer, got {v!r}")
        if v < least:
            raise ValueError(f"{what} must be at least {least}, got {v}")
    if size_floor >= 1 << 63:
        raise ValueError(f"the size floor must fit in 63 bits, got {size_floor}")
    return int(size_floor), int(rounds)


# All counts of a region graph together: exaspim_agglomerate refuses more, and the device tables of the
# pre-merge pool parallel edges in 64 bits, which is exact up to here (include/exaspim_affinity.h).
MAX_TOTAL_COUNT = 1 << 39


def _check_total_count(counts, what):
    """
    ValueError unless the int64 counts (a numpy array or a tensor, reduced
    where they live) add up to at most 2^39. The high and the low 32 bits are
    summed apart, so the total is exact for any values of up to 2^31 rows.
    """
    total = (int((counts >> 32).sum()) << 32) + int((counts & 0xFFFFFFFF).sum())
    if not 0 <= total <= MAX_TOTAL_COUNT:
        raise ValueError(f"{what}: the counts add up to {total}, needs a total of at most 2^39 = {MAX_TOTAL_COUNT} "
                         "(parallel edges are pooled in 64 bits)")


def _rounds_on_device(kernel, extra, fn, is_last, edges, counts, sums, sizes, n_edges, threshold, rounds, capacity,
                      timings=None, total_checked=False):
    """
    The round loop behind _premerge_on_device and _contract_dominant_on_device:
    the library function "kernel" (whose arguments between the threshold and
    the capacity are "extra") on a graph that is on the device, each round on
    the previous one's output, until is_last(K, K') says so or "rounds" have
    run. One 12-byte read of the state per round; the maps are composed on
    the device (exaspim_apply_label_table on the composed map). "fn" is the
    public function in whose name errors are raised.
    """
    device = sizes.device
    n_labels = int(sizes.numel()) - 1
    lib = _native.lib()
    stream = _stream(device)
    history, events = [], []
    with torch.cuda.device(device):
        if not total_checked and n_edges:
            _check_total_count(counts[:n_edges], fn)
        composed = None
        need = _workspace_bytes(kernel + "_workspace_bytes", n_labels, capacity)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        state = torch.empty(3, dtype=torch.int32, device=device)
        spare = None   # the buffers the round after next may write: never the caller's
        for _ in range(rounds):
            k = int(sizes.numel()) - 1
            if spare is None:
                out = (torch.empty((capacity, 2), dtype=torch.int32, device=device),
                       torch.empty(capacity, dtype=torch.int64, device=device),
                       torch.empty(capacity, dtype=torch.int64, device=device))
            else:
                out, spare = spare, None
            sizes_out = torch.empty(k + 1, dtype=torch.int64, device=device)
            mapping = torch.empty(k + 1, dtype=torch.int32, device=device)
            if timings is not None:
                events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                events[-1][0].record()
            _native.check(
                getattr(lib, kernel)(edges.data_ptr(), counts.data_ptr(), sums.data_ptr(), sizes.data_ptr(), n_edges,
                                     k, float(np.float32(threshold)), *extra, capacity, out[0].data_ptr(),
                                     out[1].data_ptr(), out[2].data_ptr(), sizes_out.data_ptr(), mapping.data_ptr(),
                                     state.data_ptr(), workspace.data_ptr(), need, stream),
                kernel,
            )
            if composed is None:
                composed = mapping
            else:
                _apply_table(composed, mapping)
            if timings is not None:
                events[-1][1].record()
            k_new, e_new, overflow = (int(v) for v in state.cpu())   # the round's one read of the device
            if overflow:
                raise RuntimeError(
                    f"{fn}: the contracted graph found no room in edge_capacity={capacity} "
                    "slots; run it again with a larger edge_capacity (a power of two)")
            if history:   # this round's input was an earlier round's output: free for the next one
                spare = (edges, counts, sums)
            edges, counts, sums = out
            sizes, n_edges = sizes_out[:k_new + 1], e_new
            history.append((k_new, e_new))
            if is_last(k, k_new):
                break
        if timings is not None:
            torch.cuda.synchronize(device)
            timings.extend(a.elapsed_time(b) for a, b in events)
    return edges, counts, sums, sizes, n_edges, composed, history


def _premerge_on_device(edges, counts, sums, sizes, n_edges, threshold, size_floor, rounds, capacity,
                        timings=None, total_checked=False):
    """
    Rounds of exaspim_region_graph_premerge on a graph that is on the device,
    each on the previous one's output, until one merges nothing or "rounds"
    have run. One 12-byte read of the state per round; the maps are composed
    on the device (exaspim_apply_label_table on the composed map).

    The counts must add up to at most 2^39 (the precondition of
    exaspim_region_graph_premerge): unless total_checked says the caller has
    seen to it, one reduction of the counts on the device checks it, and a
    larger total raises ValueError before the first round.

    Parameters
    ----------
    edges, counts, sums, sizes : torch.Tensor
        The graph in exaspim_region_graph's output format (sums holds uint64
        bits); edges, counts and sums hold at least n_edges rows. Only read.
    timings : list, optional
        If given, HIP events time every round and the milliseconds are
        appended (a measurement aid: it synchronises once at the end).

    Returns
    -------
    edges, counts, sums, sizes : torch.Tensor
        The reduced graph: n_edges rows in an unspecified order, K' + 1 sizes.
    n_edges : int
    composed : torch.Tensor
        int32 (K + 1,): fragment id -> id in the reduced graph.
    history : list of (int, int)
        (K', E') after every round that ran.
    """
    return _rounds_on_device("exaspim_region_graph_premerge", (size_floor,), "premerge_region_graph",
                             lambda k, k_new: k_new == k, edges, counts, sums, sizes, n_edges, threshold, rounds,
                             capacity, timings, total_checked)


def _dominant_round_is_last(k, k_new):
    """The cost rule of the dominant rounds: one that removes fewer than max(1, K // 64) fragments is the last."""
    return k - k_new < max(1, k // 64)


def _contract_dominant_on_device(edges, counts, sums, sizes, n_edges, threshold, rounds, capacity,
                                 timings=None, total_checked=False):
    """
    Rounds of exaspim_region_graph_contract_dominant on a graph that is on
    the device, each on the previous one's output; arguments, the check of
    the total count and the returned tuple are those of _premerge_on_device.

    Stopping rule: at most "rounds" rounds, and a round that removes fewer
    than max(1, K // 64) of its K fragments is the last. A chain of rising
    means contracts one pair per round, and the host does such a tail faster
    than launches do. The result of agglomerating the reduced graph does not
    depend on where the rounds stop, so this is purely a cost rule.
    """
    return _rounds_on_device("exaspim_region_graph_contract_dominant", (), "contract_dominant_edges",
                             _dominant_round_is_last, edges, counts, sums, sizes, n_edges, threshold, rounds,
                             capacity, timings, total_checked)


def _graph_arguments(fn, edges, counts, sums, sizes):
    """
    The front matter of premerge_region_graph and contract_dominant_edges:
    the four arrays of a region graph, all numpy (their total count is
    checked on the host, before any device is asked for, and they are
    uploaded to cuda:0) or all tensors on one HIP device.

    Returns
    -------
    edges, counts, sums, sizes : torch.Tensor
    n_edges : int
    device : torch.device
    on_host : bool
        The arrays came from the host, so their total count is checked.
    """
    given = (edges, counts, sums, sizes)
    on_host = not any(isinstance(a, torch.Tensor) for a in given)
    if all(isinstance(a, torch.Tensor) for a in given):
        device = sizes.device
        if device.type != "cuda" or any(a.device != device for a in given):
            raise RuntimeError(f"{fn} (MI355X) has no CPU path: the graph must be on one HIP device")
        edges, counts, sums, sizes = (a.contiguous() for a in given)
    elif not on_host:
        raise TypeError(f"{fn} needs the four arrays all on the host or all on the device")
    else:
        # the counts are on the host: their total is checked here, before any device is asked for
        _check_total_count(np.asarray(counts, dtype=np.int64), fn)
        device = _upload_device(fn)
        edges = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)).to(device)
        counts = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).to(device)
        sums = torch.from_numpy(np.ascontiguousarray(sums, dtype=np.uint64).view(np.int64)).to(device)
        sizes = torch.from_numpy(np.ascontiguousarray(sizes, dtype=np.int64)).to(device)
    if (edges.dtype != torch.int32 or counts.dtype != torch.int64 or sums.dtype != torch.int64
            or sizes.dtype != torch.int64):
        raise TypeError(f"{fn} needs int32 edges and 64-bit counts, sums and sizes")
    n_edges = int(counts.numel())
    if (sizes.dim() != 1 or sizes.numel() < 1 or edges.numel() != 2 * n_edges or sums.numel() != n_edges):
        raise ValueError(f"{fn} needs edges (E, 2), counts (E,), sums (E,) and sizes (K + 1,)")
    return edges, counts, sums, sizes, n_edges, device, on_host


def premerge_region_graph(edges, counts, sums, sizes, threshold, size_floor, *, rounds=4, edge_capacity=None):
    """
    Merges the tiny fragments of a region graph into their best neighbours
    on the device (exaspim_region_graph_premerge), so that
    agglomerate starts from far fewer fragments.

    One round: an edge is mergeable iff sum > rint((1 - T) * 2^24) * count
    (agglomerate's test at threshold T); every fragment with fewer than
    size_floor voxels that has a mergeable edge joins the neighbour across
    its mergeable edge of largest mean (equal means: the smaller neighbour
    id; of two fragments that choose each other the smaller id stays), whole
    chains at once; the sets are numbered by their smallest member id, sizes
    add up, edges inside a set vanish and parallel edges add their counts and
    sums. Rounds run on their own output until one merges nothing or
    "rounds" of them have run. All comparisons are exact integer ones.

    This is not agglomerate's rule: a tiny fragment joins its best neighbour
    at once, whatever that neighbour would have merged with first, so
    agglomerating the reduced graph can give another segmentation than
    agglomerating the input. size_floor 0 (and 1, when no fragment is empty)
    returns the input.

    Parameters
    ----------
    edges, counts, sums, sizes : numpy.ndarray or torch.Tensor
        What region_graph returns, or the same on a HIP device (sums may be
        int64 holding uint64 bits); numpy arrays are uploaded to cuda:0. The
        counts must add up to at most 2^39, agglomerate's bound (the device
        pools parallel edges in 64 bits): one reduction of the counts, on the
        side they live on, checks it, and a larger total raises ValueError
        before the first round.
    threshold : float
        T of the mergeable test: the last agglomeration threshold.
    size_floor : int
        Fragments below this many voxels are merged. Not negative.
    rounds : int, optional
        The most rounds to run. Default is 4.
    edge_capacity : int, optional
        Slots of the device hash table, a power of two. Default is the next
        power of two >= 2 * E.

    Returns
    -------
    edges, counts, sums, sizes : numpy.ndarray
        The reduced graph in region_graph's format, sorted by (lo, hi).
    mapping : numpy.ndarray
        int32 (K + 1,): fragment id -> id in the reduced graph, map[0] = 0.
    history : list of int
        The number of fragments after every round that ran.
    """
    size_floor, rounds = _checked_premerge(size_floor, rounds)
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("the threshold is NaN")
    edges, counts, sums, sizes, n_edges, device, on_host = _graph_arguments("premerge_region_graph", edges, counts,
                                                                          sums, sizes)
    capacity = 1 << max(2 * n_edges - 1, 0).bit_length() if edge_capacity is None else int(edge_capacity)
    edges, counts, sums, sizes, n_edges, composed, history = _premerge_on_device(
        edges, counts, sums, sizes, n_edges, threshold, size_floor, rounds, capacity, total_checked=on_host)
    with torch.cuda.device(device):
        graph = _download_graph(edges, counts, sums, sizes, n_edges)
        mapping = composed.cpu().numpy()
    return graph + (mapping, [k for k, _ in history])


def _checked_rounds(what, rounds, least):
    """rounds as an int; ValueError for non-integers and values below "least", before any device call."""
    if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)):
        raise ValueError(f"{what} must be an integer, got {rounds!r}")
    if rounds < least:
        raise ValueError(f"{what} must be at least {least}, got {rounds}")
    return int(rounds)


def contract_dominant_edges(edges, counts, sums, sizes, threshold, *, rounds=64, edge_capacity=None):
    """
    Contracts the dominant edges of a region graph on the device
    (exaspim_region_graph_contract_dominant): agglomerate on the
    reduced graph, composed through the mapping, gives exactly the table and
    the segment count it gives on the input.

    One round: an edge is mergeable iff sum > rint((1 - T) * 2^24) * count
    (agglomerate's test at threshold T); it is dominant iff it is mergeable
    and its mean is strictly larger than that of every other mergeable edge
    at either of its ends (128-bit cross products); every dominant edge is
    contracted: its two fragments become one set, numbered with the
    singletons by smallest member id, sizes add up, and parallel edges add
    their counts and sums. The greedy merging takes a dominant edge before
    any other edge at its two ends, which is why nothing changes. Equal means
    are not resolved here: such edges wait for agglomerate, whose tie-break
    then applies unchanged. A round that removes fewer than max(1, K // 64)
    of its K fragments is the last (the host does a thin tail faster than
    launches do).

    Parameters
    ----------
    edges, counts, sums, sizes : numpy.ndarray or torch.Tensor
        What region_graph returns (no pair twice), or the same on a HIP
        device (sums may be int64 holding uint64 bits); numpy arrays are
        uploaded to cuda:0. The counts must add up to at most 2^39, as for
        premerge_region_graph, and a larger total raises ValueError before
        the first round.
    threshold : float
        T of the mergeable test: the last agglomeration threshold.
    rounds : int, optional
        The most rounds to run, at least 1. Default is 64.
    edge_capacity : int, optional
        Slots of the device hash table, a power of two. Default is the next
        power of two >= 2 * E.

    Returns
    -------
    edges, counts, sums, sizes : numpy.ndarray
        The reduced graph in region_graph's format, sorted by (lo, hi).
    mapping : numpy.ndarray
        int32 (K + 1,): fragment id -> id in the reduced graph, map[0] = 0.
    history : list of int
        The number of fragments after every round that ran.
    """
    rounds = _checked_rounds("the number of rounds", rounds, 1)
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("the threshold is NaN")
    edges, counts, sums, sizes, n_edges, device, on_host = _graph_arguments("contract_dominant_edges", edges, counts,
                                                                          sums, sizes)
    capacity = 1 << max(2 * n_edges - 1, 0).bit_length() if edge_capacity is None else int(edge_capacity)
    edges, counts, sums, sizes, n_edges, composed, history = _contract_dominant_on_device(
        edges, counts, sums, sizes, n_edges, threshold, rounds, capacity, total_checked=on_host)
    with torch.cuda.device(device):
        graph = _download_graph(edges, counts, sums, sizes, n_edges)
        mapping = composed.cpu().numpy()
    return graph + (mapping, [k for k, _ in history])


def _premerged_table(labels, affinities, n_fragments, thresholds, min_segment_size, edge_capacity, premerge_size,
                     premerge_rounds, stats=None):
    """
    The fragment -> segment table of agglomerate_affinities with a size
    floor, as a device tensor: the region graph stays on the device, the
    pre-merge rounds run there, only the reduced graph is downloaded and
    agglomerated, and the final table is composed with the rounds' map on the
    device. "stats", a dict, receives the rounds' history, their device
    milliseconds, the host merging time and the number of segments.
    """
    device = labels.device
    edges, counts, sums, sizes, n_edges, capacity = _region_graph_device(labels, affinities, n_fragments,
                                                                         edge_capacity)
    timings = None if stats is None else []
    edges, counts, sums, sizes, n_edges, composed, history = _premerge_on_device(
        edges, counts, sums, sizes, n_edges, thresholds[-1], premerge_size, premerge_rounds, capacity, timings)
    with torch.cuda.device(device):
        graph = _download_graph(edges, counts, sums, sizes, n_edges)
        t0 = time.perf_counter()
        table, n_segments = agglomerate(*graph, thresholds, min_segment_size)
        host_ms = (time.perf_counter() - t0) * 1e3
        _apply_table(composed, torch.from_numpy(table).to(device))
    if stats is not None:
        stats.update(fragments=n_fragments, history=history, round_ms=timings, host_ms=host_ms,
                     segments=n_segments)
    return composed


def _device_merged_table(labels, affinities, n_fragments, thresholds, min_segment_size, edge_capacity, premerge_size,
                         premerge_rounds, device_merge_rounds, stats=None):
    """
    The fragment -> segment table of agglomerate_affinities with
    device_merge_rounds > 0, as a device tensor: the region graph stays on
    the device, the pre-merge rounds run there if premerge_size > 0, then up
    to device_merge_rounds dominant rounds, only the reduced graph is
    downloaded and agglomerated, and the final table is composed with the
    rounds' maps on the device. "stats", a dict, receives the history and the
    device milliseconds of both kinds of round, the host merging time and the
    number of segments.
    """
    device = labels.device
    edges, counts, sums, sizes, n_edges, capacity = _region_graph_device(labels, affinities, n_fragments,
                                                                         edge_capacity)
    timings = None if stats is None else ([], [])
    composed, premerge_history = None, []
    if premerge_size:
        edges, counts, sums, sizes, n_edges, composed, premerge_history = _premerge_on_device(
            edges, counts, sums, sizes, n_edges, thresholds[-1], premerge_size, premerge_rounds, capacity,
            timings and timings[0])
    # a contraction keeps the total count or lowers it: what the pre-merge has checked stays checked
    edges, counts, sums, sizes, n_edges, dominant, history = _contract_dominant_on_device(
        edges, counts, sums, sizes, n_edges, thresholds[-1], device_merge_rounds, capacity, timings and timings[1],
        total_checked=composed is not None)
    with torch.cuda.device(device):
        composed = dominant if composed is None else _apply_table(composed, dominant)
        graph = _download_graph(edges, counts, sums, sizes, n_edges)
        t0 = time.perf_counter()
        table, n_segments = agglomerate(*graph, thresholds, min_segment_size)
        host_ms = (time.perf_counter() - t0) * 1e3
        _apply_table(composed, torch.from_numpy(table).to(device))
    if stats is not None:
        stats.update(fragments=n_fragments, premerge_history=premerge_history, premerge_round_ms=timings[0],
                     history=history, round_ms=timings[1], host_ms=host_ms, segments=n_segments)
    return composed


def agglomerate_affinities(affinities, agglomeration_thresholds=[0.6, 0.8, 0.9], min_segment_size=100, *,
                           fragment_threshold=0.5, edge_capacity=None, return_device_tensor=False,
                           fragments="components", aff_threshold_low=0.1, aff_threshold_high=0.9999,
                           premerge_size=0, premerge_rounds=4, device_merge_rounds=0):
    """
    Segments affinities by mean-affinity agglomeration of fragments, in the
    reference's order of operations.

    What this is: the three steps of the reference's
    affinities_to_segmentation (inference.py:196-237) with exactly defined
    parts. (1) Fragments: with fragments="components", the default, the
    connected components of the affinity graph cut at fragment_threshold
    (affinities_to_components with no size filter); with
    fragments="watershed" the basins of a steepest-ascent watershed between
    aff_threshold_low and aff_threshold_high (watershed_fragments with no
    size filter), which is the kind of fragment the reference starts from.
    (2) Fragments whose contact surface has a high mean affinity are merged,
    greedily in order of the score waterz uses by default, 1 - mean affinity
    of the contact, while that score is below the last agglomeration
    threshold (see agglomerate for the exact integer rule). The contact
    counts and affinity sums come from one pass on the device
    (exaspim_region_graph), the merging runs on the host on the graph of
    fragments. (3) Only then segments of at most min_segment_size voxels are
    removed (img_util.py:555-558) and the rest is numbered 1 ... S in raster
    order of each segment's first voxel. The positional arguments and their
    defaults are those of affinities_to_segmentation.

    What this is not: waterz. Connected components at a threshold are not
    watershed basins: one voxel edge above fragment_threshold fuses two
    neurites for good, and agglomeration only merges. The watershed
    fragments equal the serial steepest-ascent watershed on tie-free input
    (no voxel with two equal maximal eligible edges below
    aff_threshold_high), label for label, by the oracle in tests/
    (watershed_ref.py); where affinities tie, the serial algorithm depends
    on its visiting order and the two differ. Neither kind has been compared
    with waterz itself, which reads the same array as the edges v -- v - e_c
    while the project keeps the convention the network was trained in, so
    the name differs on purpose. Only the segmentation of the last threshold
    is returned, as in the reference (deque(maxlen=1)); greedy merging in
    score order makes it independent of the intermediate stops.

    Parameters
    ----------
    affinities : torch.Tensor or numpy.ndarray
        float32 or float16 (3, D, H, W): a tensor on a HIP device (e.g. from
        predict(..., return_device_tensor=True)), or a numpy array, which is
        uploaded to cuda:0. A 3-D foreground map has no affinities to score.
    agglomeration_thresholds : sequence of float, optional
        Non-decreasing. Default is [0.6, 0.8, 0.9].
    min_segment_size : int, optional
        Default is 100.
    fragment_threshold : float, optional
        Used with fragments="components". Default is 0.5.
    edge_capacity : int, optional
        See region_graph.
    return_device_tensor : bool, optional
        Return the labels as a device tensor instead of a numpy array.
        Default is False.
    fragments : {"components", "watershed"}, optional
        The kind of fragments. Default is "components".
    aff_threshold_low, aff_threshold_high : float, optional
        Used with fragments="watershed". Defaults are 0.1 and 0.9999, the
        reference's.
    premerge_size : int, optional
        0, the default, is the path described above. A positive value
        CHANGES THE SEGMENTATION: before the host merging, every fragment
        with fewer than premerge_size voxels joins, on the device, the
        neighbour across its contact of largest mean affinity among those
        the last threshold would merge (premerge_region_graph), whole chains
        at once and whatever that neighbour would itself have merged with
        first; the greedy merging then starts from the reduced graph, which
        is the only one downloaded. Watershed fragments of a large volume are
        millions of tiny basins, and this is what makes the host step
        affordable there. 1 gives the labels of 0 (no fragment is empty).
        Negative values and non-integers raise ValueError.
    premerge_rounds : int, optional
        The most pre-merge rounds; they stop when one merges nothing.
        Default is 4.
    device_merge_rounds : int, optional
        0, the default, is the path described above. R > 0 changes where
        the work is done and nothing else: the labels are those of
        device_merge_rounds=0, bit for bit. Without premerge_size those are
        the labels agglomerate_affinities has always defined; with it, they
        are the labels of the same call without dominant rounds. The region
        graph stays on the device, the pre-merge rounds run first if
        premerge_size > 0, then up to R rounds contract every dominant edge
        (contract_dominant_edges: a mergeable contact whose mean affinity is
        strictly the largest at both its fragments, which the greedy merging
        takes before any other contact of the two), and only the reduced
        graph is downloaded and merged on the host. Negative values and
        non-integers raise ValueError.

    Returns
    -------
    numpy.ndarray or torch.Tensor
        int32 (D, H, W) labels: 4 bytes per voxel leave the device.
    """
    thresholds = list(agglomeration_thresholds)
    _last_threshold(thresholds)
    premerge_size, premerge_rounds = _checked_premerge(premerge_size, premerge_rounds)
    device_merge_rounds = _checked_rounds("device_merge_rounds", device_merge_rounds, 0)
    if fragments not in ("components", "watershed"):
        raise ValueError(f'fragments must be "components" or "watershed", got {fragments!r}')

    def check(a):
        if a.ndim != 4 or a.shape[0] != 3:
            raise ValueError(f"agglomerate_affinities needs (3, D, H, W) affinities, got {tuple(a.shape)}; "
                             "a foreground map has no affinities to score")

    if isinstance(affinities, torch.Tensor):   # an array's shape is checked after its dtype, before the upload
        check(affinities)
    affinities = _on_device(affinities, "agglomerate_affinities", check=check).contiguous()
    if fragments == "watershed":
        labels, count = _watershed_on_device(affinities, aff_threshold_low, aff_threshold_high, 0)
    else:
        labels, count = _components_on_device(affinities, fragment_threshold, 0)
    n_fragments = int(count.cpu()[0])
    device = labels.device
    if device_merge_rounds:
        table_dev = _device_merged_table(labels, affinities, n_fragments, thresholds, min_segment_size,
                                         edge_capacity, premerge_size, premerge_rounds, device_merge_rounds)
    elif premerge_size:
        table_dev = _premerged_table(labels, affinities, n_fragments, thresholds, min_segment_size, edge_capacity,
                                     premerge_size, premerge_rounds)
    else:
        edges, counts, sums, sizes = _region_graph_on_device(labels, affinities, n_fragments, edge_capacity)
        table, _ = agglomerate(edges, counts, sums, sizes, thresholds, min_segment_size)
        with torch.cuda.device(device):
            table_dev = torch.from_numpy(table).to(device)
    _apply_table(labels, table_dev)
    if return_device_tensor:
        return labels
    return labels.cpu().numpy()


# What distance_to_boundary gives a voxel that has no boundary at all (EXASPIM_DBF_INF)
DBF_INF = 2**31 - 1


def _checked_labels(labels, fn, what="labels"):
    """
    The front matter of distance_to_boundary and segment_table: labels as a
    contiguous int32 (D, H, W) tensor on a HIP device and its dims. A numpy
    array is checked before any device is asked for. "what" names the
    argument in the messages.
    """

    def check(a):
        if a.ndim != 3:
            raise ValueError(f"{fn}: {what} must be (D, H, W), got {tuple(a.shape)}")
        if min(a.shape) < 1:
            raise ValueError(f"{fn}: empty volume {tuple(a.shape)}")

    labels = _on_device(labels, fn, what, (np.int32,), check=check)
    if labels.dtype != torch.int32:
        raise TypeError(f"{what} must be int32, got {labels.dtype}")
    check(labels)
    if labels.device.type != "cuda":
        raise RuntimeError(f"{fn} (MI355X) has no CPU path: {what} must be on a HIP device, got {labels.device}")
    return labels.contiguous(), tuple(int(v) for v in labels.shape)


_TORCH_DTYPES = {np.int32: torch.int32, np.float32: torch.float32}


# Shape rules of _checked_arrays' rows: rule(a, reference's shape) is None, or what the argument "must ..."
def _like_labels(a, shape):
    """Of the labels' shape."""
    return None if tuple(a.shape) == tuple(shape) else f"have the labels' shape {tuple(shape)}"


def _row_per_label(n_labels):
    """(K + 1,): one row per label and row 0, n_labels + 1 of them if n_labels is given."""
    def rule(a, _):
        if a.ndim != 1 or a.shape[0] < 1 or (n_labels is not None and a.shape[0] != n_labels + 1):
            return "be (K + 1,)" if n_labels is None else f"be (n_labels + 1 = {n_labels + 1},)"
    return rule


def _listed(a, _):
    """(S,): a list of any length, an empty one included."""
    return None if a.ndim == 1 else "be (S,)"


def _six_per_row(a, shape):
    """(rows, 6), rows those of the table it goes with."""
    return None if tuple(a.shape) == (shape[0], 6) else f"be ({shape[0]}, 6) as sources has {shape[0]} rows"


def _checked_arrays(fn, labels, rows):
    """
    The front matter of every function that takes arrays next to a labels
    volume, once, after the caller has checked its scalars: (2) every numpy
    array is checked before any of them is uploaded; (3) if labels is a
    tensor, every tensor next to it is checked before an array next to it is
    uploaded; (4) labels go through _checked_labels; (5) every argument is
    uploaded, checked for dtype, shape and device and made contiguous, in the
    order of the rows. Within (2) and (3) the dtypes of all rows come first,
    then their shapes.

    A row is (name, value, numpy dtype, shape rule, reference, optional). The
    rule is checked against the shape of its reference: None (the rule needs
    none), "labels", or the name of an earlier row, which must be 1-D. A rule
    that refers to a row is checked in (2) or (3) as soon as either of the
    two is an array, or a tensor. An optional argument may be None.

    Returns (labels, dims, values): the values as contiguous tensors on the
    labels' device, None for an absent one, in the order of the rows.
    """
    given = {name: value for name, value, *_ in rows}

    def check_dtype(name, a, dtype):
        if a.dtype != (dtype if isinstance(a, np.ndarray) else _TORCH_DTYPES[dtype]):
            raise TypeError(f"{name} must be {np.dtype(dtype)}, got {a.dtype}")

    def check_shape(name, a, rule, shape):
        must = rule(a, shape)
        if must is not None:
            raise ValueError(f"{fn}: {name} must {must}, got {tuple(a.shape)}")

    def check_all(kind):
        """Of the arguments that are of "kind", numpy arrays or tensors."""
        for name, a, dtype, _, _, _ in rows:
            if isinstance(a, kind):
                check_dtype(name, a, dtype)
        for name, a, _, rule, reference, _ in rows:
            if reference is None or reference == "labels":
                if isinstance(a, kind) and (reference is None or isinstance(labels, (np.ndarray, torch.Tensor))):
                    check_shape(name, a, rule, None if reference is None else labels.shape)
            else:
                other = given[reference]
                if ((isinstance(a, kind) or isinstance(other, kind)) and isinstance(a, (np.ndarray, torch.Tensor))
                        and isinstance(other, (np.ndarray, torch.Tensor)) and other.ndim == 1):
                    check_shape(name, a, rule, other.shape)

    check_all(np.ndarray)      # every array is checked before any of them is uploaded
    if isinstance(labels, torch.Tensor):   # a tensor is refused before an array next to it is uploaded
        check_all(torch.Tensor)
    labels, dims = _checked_labels(labels, fn)
    device = labels.device
    out = {"labels": labels}
    for name, a, dtype, rule, reference, optional in rows:
        if a is not None or not optional:
            a = _on_device(a, fn, name, (dtype,))
            check_dtype(name, a, dtype)
            check_shape(name, a, rule, None if reference is None else out[reference].shape)
            if a.device != device:
                raise RuntimeError(f"{fn}: {name} must be on the labels' device {device}, got {a.device}")
            a = a.contiguous()
        out[name] = a
    return labels, dims, [out[name] for name, *_ in rows]


def _fill_holes_on_device(labels):
    """
    exaspim_fill_holes on a device tensor: the filled labels and the two
    counts, both left on the device (nothing is synchronised).

    Parameters
    ----------
    labels : torch.Tensor
        int32 (D, H, W) tensor on a HIP device. It is only read.

    Returns
    -------
    filled : torch.Tensor
        int32 (D, H, W), a new tensor.
    counts : torch.Tensor
        int64 (2,): the number of holes filled and the number of voxels
        filled.
    """
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"_fill_holes_on_device needs a torch tensor, got {type(labels).__name__}")
    labels, dims = _checked_labels(labels, "fill_holes")
    device = labels.device
    lib = _native.lib()
    need = _workspace_bytes("exaspim_fill_holes_workspace_bytes", _native.int3(dims))
    with torch.cuda.device(device):
        filled = torch.empty(dims, dtype=torch.int32, device=device)
        counts = torch.empty(2, dtype=torch.int64, device=device)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        _native.check(
            lib.exaspim_fill_holes(labels.data_ptr(), _native.int3(dims), filled.data_ptr(), counts.data_ptr(),
                                   workspace.data_ptr(), need, _stream(device)),
            "exaspim_fill_holes",
        )
    return filled, counts


def fill_holes(labels, *, return_counts=False, return_device_tensor=False):
    """
    Closes the enclosed cavities of every label at once, on the device: what
    the reference's skeletonize (inference.py:257-291) asks of
    kimimaro.skeletonize with fill_holes=True before the distance-to-boundary
    field is taken, so that a few dark voxels inside a soma or a thick neurite
    do not bound the field from the inside.

    What this is, exactly, in integers: a voxel is background iff labels <= 0
    (distance_to_boundary's convention). A cavity is a 6-connected component
    of background voxels. A cavity is a hole of label L iff (1) none of its
    voxels lies on a face of the volume, i.e. at index 0 or n - 1 of any
    axis, and (2) the positive labels among the six neighbours of its voxels
    are exactly the one value L. Every voxel of a hole of L becomes L,
    negative voxels inside the hole included; every other voxel keeps its
    value bit for bit. So cavities that touch a face stay; cavities bounded
    by two or more labels stay, and so does a cavity that also holds an
    island of another label M (its neighbours are {L, M}); a cavity that holds
    a floating piece of L itself is filled; positive voxels never change, so a
    label enclosed by another label is not removed; with a single-voxel axis
    every voxel lies on a face and nothing is filled, which is what
    scipy.ndimage.binary_fill_holes gives on a 3-D array of depth 1.

    What equals what: for every L take binary_fill_holes(labels == L) with
    scipy's default 6-connected structure. On volumes where no positive voxel
    lies inside the filled region of another label, the result equals the
    union of that per-label fill over every L (tests/holes_ref.py holds the
    two forms to each other).

    What this is not: the name follows the reference's keyword; the result
    is not claimed to equal the fill_voids package or kimimaro, neither of
    which the project or its tests depend on. No slab-streamed form, no
    removal of labels enclosed by other labels, no fix_borders.

    Parameters
    ----------
    labels : torch.Tensor or numpy.ndarray
        int32 (D, H, W): a tensor on a HIP device (e.g. from
        agglomerate_affinities(..., return_device_tensor=True)), or a numpy
        array, which is uploaded to cuda:0. It is only read, never changed.
        D * H * W must not exceed 2^31 - 1.
    return_counts : bool, optional
        Also return the number of holes and of voxels filled (one read of
        the device). Default is False.
    return_device_tensor : bool, optional
        Return the labels as a device tensor instead of a numpy array.
        Default is False.

    Returns
    -------
    numpy.ndarray or torch.Tensor
        int32 (D, H, W), a new array or tensor; with return_counts the tuple
        (labels, n_holes, n_voxels), the two counts as ints.

    Raises
    ------
    TypeError
        If labels is not int32.
    ValueError
        If labels is not 3-D, is empty or has more than 2^31 - 1 voxels.
    RuntimeError
        If labels is a tensor on a CPU device, or there is no HIP device to
        upload an array to.
    """
    labels, _ = _checked_labels(labels, "fill_holes")
    filled, counts = _fill_holes_on_device(labels)
    with torch.cuda.device(filled.device):
        out = filled if return_device_tensor else filled.cpu().numpy()
        if return_counts:
            n_holes, n_voxels = (int(v) for v in counts.cpu())
            return out, n_holes, n_voxels
    return out


def distance_to_boundary(labels, *, black_border=False, return_device_tensor=False):
    """
    The distance-to-boundary field of every label at once, on the device:
    for each foreground voxel the squared distance to the nearest voxel of
    another label.

    What this is: the field TEASAR starts from -- the reference's
    skeletonize (inference.py:257-291) runs kimimaro.skeletonize, which asks
    the edt package for it -- with an exact definition in integers. A voxel
    with labels <= 0 is background and gets 0. A voxel v with label L > 0
    gets the minimum of |v - u|^2 over all in-volume voxels u with
    labels[u] != L, background and every other label alike (two touching
    segments bound each other), voxel centre to voxel centre at unit
    spacing. With black_border the volume counts as surrounded by one layer
    of background: index i of an axis of length n also has the candidates
    (i + 1)^2 and (n - i)^2. A voxel with no candidate at all (one label
    filling the volume, no black_border) gets DBF_INF. The values are
    squared and nothing is rounded; the caller takes the root.

    What this is not: compared with edt, which the tests do not depend on
    (the oracle in tests/dbf_ref.py is brute force and a per-label scipy
    EDT); anisotropic (the reference passes (1, 1, 1));
    TEASAR's paths or its fix_borders, which stay with the host
    skeletoniser. The reference fills holes first: fill_holes does that on
    the device, and this function takes the labels as they are given.

    Parameters
    ----------
    labels : torch.Tensor or numpy.ndarray
        int32 (D, H, W): a tensor on a HIP device (e.g. from
        agglomerate_affinities(..., return_device_tensor=True)), or a numpy
        array, which is uploaded to cuda:0. It is only read.
    black_border : bool, optional
        Treat the volume's faces as boundaries. Default is False.
    return_device_tensor : bool, optional
        Return the field as a device tensor instead of a numpy array.
        Default is False.

    Returns
    -------
    numpy.ndarray or torch.Tensor
        int32 (D, H, W), squared distances.

    Raises
    ------
    TypeError
        If labels is not int32.
    ValueError
        If labels is not 3-D, is empty, or (D+1)^2 + (H+1)^2 + (W+1)^2
        reaches 2^31 - 1.
    RuntimeError
        If labels is a tensor on a CPU device, or there is no HIP device to
        upload an array to.
    """
    labels, dims = _checked_labels(labels, "distance_to_boundary")
    device = labels.device
    lib = _native.lib()
    need = _workspace_bytes("exaspim_dbf_workspace_bytes", _native.int3(dims))
    with torch.cuda.device(device):
        dbf = torch.empty(dims, dtype=torch.int32, device=device)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        _native.check(
            lib.exaspim_dbf(labels.data_ptr(), _native.int3(dims), int(bool(black_border)), dbf.data_ptr(),
                            workspace.data_ptr(), need, _stream(device)),
            "exaspim_dbf",
        )
        if return_device_tensor:
            return dbf
        return dbf.cpu().numpy()


def segment_table(labels, dbf=None, *, n_labels=None, return_device_tensors=False):
    """
    Per-label facts of a labelled volume, on the device: voxel count,
    bounding box, the largest value of a distance-to-boundary field and
    where it lies.

    What this is: what a skeletoniser crops and roots each segment with
    (inference.py:257-291: kimimaro.skeletonize crops every label to its
    bounding box, starts TEASAR at the field's maximum and compares that
    maximum with soma_detection_threshold), as one pass over labels and
    dbf. Every output has K + 1 rows, K = n_labels, and is a pure function
    of the input.

    What this is not: TEASAR. The paths, fix_borders and the SWC export
    stay with the host skeletoniser, which downloads the field and this
    table instead of recomputing an EDT of the whole volume (fill_holes is a
    function of its own here, run on the labels before the field).

    Parameters
    ----------
    labels : torch.Tensor or numpy.ndarray
        int32 (D, H, W), as for distance_to_boundary.
    dbf : torch.Tensor or numpy.ndarray, optional
        int32, of the labels' shape, on the labels' device (an array is
        uploaded to cuda:0): distance_to_boundary's result, or any other
        field. Default is None: peak is 0 and peak_index the first voxel.
    n_labels : int, optional
        K. Default is max(labels.max(), 0), one read of the device. Labels
        above K and negative labels are counted nowhere.
    return_device_tensors : bool, optional
        Return device tensors instead of numpy arrays. Default is False.

    Returns
    -------
    sizes : numpy.ndarray or torch.Tensor
        int64 (K + 1,): voxels per label; row 0 counts the voxels labelled
        exactly 0, as region_graph does.
    boxes : numpy.ndarray or torch.Tensor
        int32 (K + 1, 6): (z0, y0, x0, z1, y1, x1), half-open; zeros for an
        absent label and for row 0.
    peak : numpy.ndarray or torch.Tensor
        int32 (K + 1,): the largest dbf value of the label; 0 for an absent
        label, for row 0 and without dbf.
    peak_index : numpy.ndarray or torch.Tensor
        int32 (K + 1,): the smallest C-order linear index at which the
        label attains its peak (numpy.unravel_index gives z, y, x); -1 for
        an absent label and for row 0.

    Raises
    ------
    TypeError
        If labels or dbf is not int32.
    ValueError
        If labels is not 3-D or is empty, dbf has another shape, n_labels
        is negative, or the dims are ones distance_to_boundary refuses.
    RuntimeError
        If labels is a tensor on a CPU device, dbf is on another device, or
        there is no HIP device to upload an array to.
    """
    if isinstance(dbf, np.ndarray):   # both arrays are checked before either is uploaded
        if dbf.dtype != np.int32:
            raise TypeError(f"dbf must be int32, got {dbf.dtype}")
        if isinstance(labels, np.ndarray) and dbf.shape != labels.shape:
            raise ValueError(f"segment_table: dbf must have the labels' shape {labels.shape}, got {dbf.shape}")
    labels, dims = _checked_labels(labels, "segment_table")
    device = labels.device
    if dbf is not None:
        dbf = _on_device(dbf, "segment_table", "dbf", (np.int32,))
        if dbf.dtype != torch.int32:
            raise TypeError(f"dbf must be int32, got {dbf.dtype}")
        if tuple(dbf.shape) != dims:
            raise ValueError(f"segment_table: dbf must have the labels' shape {dims}, got {tuple(dbf.shape)}")
        if dbf.device != device:
            raise RuntimeError(f"segment_table: dbf must be on the labels' device {device}, got {dbf.device}")
        dbf = dbf.contiguous()
    if n_labels is None:
        n_labels = max(int(labels.max()), 0)   # the one read of the device
    n_labels = int(n_labels)
    if n_labels < 0:
        raise ValueError(f"n_labels must not be negative, got {n_labels}")
    lib = _native.lib()
    need = _workspace_bytes("exaspim_segment_table_workspace_bytes", n_labels)
    with torch.cuda.device(device):
        sizes = torch.empty(n_labels + 1, dtype=torch.int64, device=device)
        boxes = torch.empty((n_labels + 1, 6), dtype=torch.int32, device=device)
        peak = torch.empty(n_labels + 1, dtype=torch.int32, device=device)
        peak_index = torch.empty(n_labels + 1, dtype=torch.int32, device=device)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        _native.check(
            lib.exaspim_segment_table(labels.data_ptr(), None if dbf is None else dbf.data_ptr(), _native.int3(dims),
                                      n_labels, sizes.data_ptr(), boxes.data_ptr(), peak.data_ptr(),
                                      peak_index.data_ptr(), workspace.data_ptr(), need, _stream(device)),
            "exaspim_segment_table",
        )
    return _downloaded((sizes, boxes, peak, peak_index), device, return_device_tensors)


def _border_targets_on_device(labels, n_labels):
    """
    exaspim_border_targets on a checked device tensor, then the rows sorted by
    (label, voxel) and deduplicated with torch. One read of the device, the
    count. Returns two int32 (T,) device tensors.
    """
    dims = tuple(int(v) for v in labels.shape)
    device = labels.device
    lib = _native.lib()
    dims3 = _native.int3(dims)
    need = _workspace_bytes("exaspim_border_targets_workspace_bytes", dims3)
    d, h, w = dims
    capacity = 2 * (h * w + d * w + d * h)   # every face pixel a component of its own: it never overflows
    with torch.cuda.device(device):
        out_labels = torch.empty(capacity, dtype=torch.int32, device=device)
        out_voxels = torch.empty(capacity, dtype=torch.int32, device=device)
        state = torch.empty(2, dtype=torch.int32, device=device)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        _native.check(
            lib.exaspim_border_targets(labels.data_ptr(), dims3, n_labels, out_labels.data_ptr(),
                                       out_voxels.data_ptr(), capacity, state.data_ptr(), workspace.data_ptr(), need,
                                       _stream(device)),
            "exaspim_border_targets",
        )
        found = int(state.cpu()[0])   # the one read
        if found < 0 or found > capacity:
            raise RuntimeError(f"border_targets: {found} targets reported for {capacity} face pixels")
        key = (out_labels[:found].to(torch.int64) << 32) | out_voxels[:found].to(torch.int64)
        key = torch.unique_consecutive(torch.sort(key).values)
        return (key >> 32).to(torch.int32), (key & 0xFFFFFFFF).to(torch.int32)


def border_targets(labels, *, n_labels=None, return_device_tensors=False):
    """
    The centre of every cut: where a face of the volume cuts a label, the
    voxel of the cut cross-section that lies deepest inside it, on the device.

    What this is: what kimimaro.skeletonize(..., fix_borders=True) asks for
    (the reference's skeletonize, inference.py:286): a skeleton that ends at
    the centre of the cut, a point the block next door, which sees the same
    plane of voxels, picks as well, so the skeletons of adjacent blocks can
    be joined. Exactly, in integers: K = n_labels. The six faces are the
    planes z = 0, z = D - 1, y = 0, y = H - 1, x = 0 and x = W - 1. A pixel
    of a face is foreground iff its label is in 1..K. e(p) of a foreground
    pixel is the least squared in-plane Euclidean distance to a pixel of the
    same plane with another label, or to a position just outside the plane
    (a black border). A face component is an 8-connected set of pixels of
    one plane with one foreground label; its target is its pixel with the
    largest e, ties to the smallest linear voxel index z * H * W + y * W + x.
    The result is the set of (label, voxel index) over all components of all
    six faces: a voxel that is the target of two faces appears once.

    What this is not: kimimaro, which breaks ties by closeness to a
    centroid; equality with it is not claimed. The result depends on the
    face's plane of labels alone, which is what makes the two sides of a seam
    agree.

    Parameters
    ----------
    labels : torch.Tensor or numpy.ndarray
        int32 (D, H, W): a tensor on a HIP device, or a numpy array, which
        is uploaded to cuda:0. It is only read.
    n_labels : int, optional
        K. Default is max(labels.max(), 0), one read of the device. Labels
        above K and labels <= 0 are background.
    return_device_tensors : bool, optional
        Return device tensors instead of numpy arrays. Default is False.

    Returns
    -------
    target_labels, target_voxels : numpy.ndarray or torch.Tensor
        int32 (T,): sorted by (label, voxel index), no pair twice.

    Raises
    ------
    TypeError
        If labels is not int32 or n_labels is not an integer.
    ValueError
        If labels is not 3-D or is empty, n_labels is negative, or the
        volume has more than 2^31 - 1 voxels or face pixels.
    RuntimeError
        If labels is a tensor on a CPU device, or there is no HIP device to
        upload an array to.
    """
    _checked_integer("border_targets", "n_labels", n_labels, least=0, optional=True)
    labels, _ = _checked_labels(labels, "border_targets")
    out = _border_targets_on_device(labels, _label_count(labels, n_labels, "border_targets"))
    return _downloaded(out, labels.device, return_device_tensors)


def _label_pieces_on_device(labels, n_labels, dust_threshold=0):
    """
    exaspim_label_pieces on a checked device tensor. Returns the int32
    (D, H, W) volume of piece numbers and the int32 (2,) state (kept pieces,
    dust pieces), both left on the device: nothing is synchronised.
    """
    dims = tuple(int(v) for v in labels.shape)
    device = labels.device
    lib = _native.lib()
    dims3 = _native.int3(dims)
    need = _workspace_bytes("exaspim_label_pieces_workspace_bytes", dims3)
    with torch.cuda.device(device):
        pieces = torch.empty(dims, dtype=torch.int32, device=device)
        state = torch.empty(2, dtype=torch.int32, device=device)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        _native.check(
            lib.exaspim_label_pieces(labels.data_ptr(), dims3, int(n_labels), int(dust_threshold), pieces.data_ptr(),
                                     state.data_ptr(), workspace.data_ptr(), need, _stream(device)),
            "exaspim_label_pieces",
        )
    return pieces, state


def _piece_tables_on_device(labels, pieces, state):
    """
    The tables of label_pieces from its volume: P (the one read of the
    device), then segment_table of the pieces and a gather of the labels at
    the first voxels. Returns (P, piece_label, piece_size, piece_first) with
    device tensors of P rows.
    """
    with torch.cuda.device(labels.device):
        n_pieces = int(state.cpu()[0])   # the one read
        sizes, _, _, first = segment_table(pieces, n_labels=n_pieces, return_device_tensors=True)
        piece_size, piece_first = sizes[1:].contiguous(), first[1:].contiguous()
        piece_label = labels.reshape(-1)[piece_first.to(torch.int64)].contiguous()
    return n_pieces, piece_label, piece_size, piece_first


def _checked_pieces_scalars(fn, n_labels, dust_threshold):
    """n_labels (or None) and dust_threshold of label_pieces and skeletonize_pieces, before any device is asked for."""
    _checked_integer(fn, "n_labels", n_labels, least=0, most_bits=31, optional=True)
    _checked_integer(fn, "dust_threshold", dust_threshold, least=0)
    return min(int(dust_threshold), 2**63 - 1)


def label_pieces(labels, *, n_labels=None, dust_threshold=0, return_device_tensors=False):
    """
    Every 26-connected piece of every label, numbered, without the dust, on
    the device.

    What this is: what kimimaro.skeletonize does before anything else (the
    reference's call, inference.py:272-290, leaves dust_threshold at
    kimimaro's 1000): the volume is relabelled by 26-connected components
    and the small ones are dropped, so that a label in several pieces gets a
    skeleton per piece. Exactly, in integers: K = n_labels. A voxel is
    foreground iff its label is in 1..K. A piece is a maximal 26-connected
    set of foreground voxels with one label; its size is its voxel count, its
    first voxel its smallest linear index z * H * W + y * W + x. A piece is
    kept iff size >= dust_threshold (0 and 1 keep everything), otherwise it
    is dust. Kept pieces are numbered 1..P in ascending order of first
    voxel; every voxel of a kept piece holds that number, every other voxel
    0. A pure function of the input.

    Two consequences hold exactly: distance_to_boundary(pieces) equals
    distance_to_boundary(labels) at every voxel of a kept piece, and
    border_targets(pieces) is border_targets(labels) restricted to kept
    pieces, with the label column mapped to piece numbers.

    What this is not: cc3d or kimimaro; equality with either is not claimed,
    and neither is a dependency. No slab-streamed form.

    Parameters
    ----------
    labels : torch.Tensor or numpy.ndarray
        int32 (D, H, W): a tensor on a HIP device, or a numpy array, which
        is uploaded to cuda:0. It is only read.
    n_labels : int, optional
        K. Default is max(labels.max(), 0), one more read of the device.
        Labels above K and labels <= 0 are background.
    dust_threshold : int, optional
        Pieces of fewer voxels are dropped. Default is 0.
    return_device_tensors : bool, optional
        Return device tensors instead of numpy arrays. Default is False.

    Returns
    -------
    pieces : numpy.ndarray or torch.Tensor
        int32 (D, H, W).
    piece_label : numpy.ndarray or torch.Tensor
        int32 (P,): the label of piece i + 1.
    piece_size : numpy.ndarray or torch.Tensor
        int64 (P,): its voxel count.
    piece_first : numpy.ndarray or torch.Tensor
        int32 (P,): its first voxel, strictly ascending.

    Raises
    ------
    TypeError
        If labels is not int32, or n_labels or dust_threshold is not an
        integer.
    ValueError
        If labels is not 3-D, is empty or has more than 2^31 - 1 voxels, or
        n_labels or dust_threshold is negative.
    RuntimeError
        If labels is a tensor on a CPU device, or there is no HIP device to
        upload an array to.
    """
    dust_threshold = _checked_pieces_scalars("label_pieces", n_labels, dust_threshold)
    labels, _ = _checked_labels(labels, "label_pieces")
    with torch.cuda.device(labels.device):
        if n_labels is None:
            n_labels = max(int(labels.max()), 0)
        pieces, state = _label_pieces_on_device(labels, int(n_labels), dust_threshold)
        _, piece_label, piece_size, piece_first = _piece_tables_on_device(labels, pieces, state)
    return _downloaded((pieces, piece_label, piece_size, piece_first), labels.device, return_device_tensors)


def _swept_until_settled(launch, state, sweeps_per_read, max_sweeps, fn, refusal):
    """
    The sweep loop of the three field passes after their begin call: the first
    read of "state" (word 0 the tiles flagged, word 1 the rows the begin call
    refused: ValueError(refusal(that count)) if any), then launch(batch) and
    one read of word 0 until no tile is flagged, the batch sweeps_per_read
    clipped to what max_sweeps leaves; RuntimeError in the name of "fn" once
    max_sweeps have run and a tile is still flagged. Returns what the callers
    put into "stats": sweeps (launched), reads (of the state) and
    tiles_flagged (the count found at each read, the one after begin first).
    """
    flagged, invalid = (int(v) for v in state.cpu()[:2])   # the first read of the state
    if invalid:
        raise ValueError(refusal(invalid))
    sweeps, reads, history = 0, 1, [flagged]
    while flagged:
        if max_sweeps is not None and sweeps >= max_sweeps:
            raise RuntimeError(f"{fn}: not converged after {sweeps} sweeps (max_sweeps={max_sweeps}), "
                               f"{flagged} tile(s) still flagged")
        batch = sweeps_per_read if max_sweeps is None else min(sweeps_per_read, max_sweeps - sweeps)
        launch(batch)
        sweeps += batch
        flagged = int(state.cpu()[0])
        reads += 1
        history.append(flagged)
    return dict(sweeps=sweeps, reads=reads, tiles_flagged=history)


def _geodesic_on_device(labels, sources, cost=None, sweeps_per_read=32, max_sweeps=None, farthest=False,
                        stats=None):
    """
    exaspim_geodesic_begin, then exaspim_geodesic_sweeps(sweeps_per_read) and
    one 8-byte read of the state until no tile is flagged; with "farthest"
    exaspim_geodesic_farthest on the converged field. Everything stays on the
    device. The arguments are geodesic_field's, already checked: contiguous
    tensors on one HIP device.

    Parameters
    ----------
    labels : torch.Tensor
        int32 (D, H, W) on a HIP device.
    sources : torch.Tensor
        int32 (K + 1,) on the same device.
    cost : torch.Tensor, optional
        float32 (D, H, W) on the same device, or None for Euclidean steps.
    sweeps_per_read : int, optional
        Sweeps launched between two reads of the state. Default is 32.
    max_sweeps : int, optional
        RuntimeError once more sweeps than this have been launched without
        convergence. Default is None.
    farthest : bool, optional
        Also build the farthest table. Default is False.
    stats : dict, optional
        Receives "sweeps" (launched), "reads" (of the state) and
        "tiles_flagged" (the count found at each read, the one after begin
        first).

    Returns
    -------
    field : torch.Tensor
        float32 (D, H, W).
    far_value, far_index : torch.Tensor or None
        float32 and int32 (K + 1,), or None without "farthest".
    """
    dims = tuple(int(v) for v in labels.shape)
    n_labels = int(sources.numel()) - 1
    device = labels.device
    lib = _native.lib()
    dims3 = _native.int3(dims)
    need = _workspace_bytes("exaspim_geodesic_workspace_bytes", dims3)
    with torch.cuda.device(device):
        stream = _stream(device)
        field = torch.empty(dims, dtype=torch.float32, device=device)
        state = torch.empty(2, dtype=torch.int32, device=device)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        _native.check(
            lib.exaspim_geodesic_begin(labels.data_ptr(), dims3, sources.data_ptr(), n_labels, field.data_ptr(),
                                       state.data_ptr(), workspace.data_ptr(), need, stream),
            "exaspim_geodesic_begin",
        )

        def sweeps(batch):
            _native.check(
                lib.exaspim_geodesic_sweeps(labels.data_ptr(), None if cost is None else cost.data_ptr(), dims3,
                                            n_labels, field.data_ptr(), batch, state.data_ptr(),
                                            workspace.data_ptr(), need, stream),
                "exaspim_geodesic_sweeps",
            )

        swept = _swept_until_settled(
            sweeps, state, sweeps_per_read, max_sweeps, "geodesic_field",
            lambda invalid: f"geodesic_field: {invalid} row(s) of sources name no voxel of their label "
                            "(a row L must be -1 or the linear index of a voxel with labels == L)")
        if stats is not None:
            stats.update(swept)
        far_value = far_index = None
        if farthest:
            far_need = lib.exaspim_geodesic_farthest_workspace_bytes(n_labels)
            far_value = torch.empty(n_labels + 1, dtype=torch.float32, device=device)
            far_index = torch.empty(n_labels + 1, dtype=torch.int32, device=device)
            far_workspace = torch.empty(far_need, dtype=torch.uint8, device=device)
            _native.check(
                lib.exaspim_geodesic_farthest(labels.data_ptr(), field.data_ptr(), dims3, n_labels,
                                              far_value.data_ptr(), far_index.data_ptr(), far_workspace.data_ptr(),
                                              far_need, stream),
                "exaspim_geodesic_farthest",
            )
    return field, far_value, far_index


def _checked_geodesic_arguments(fn, labels, sources, cost, n_labels, sweeps_per_read, max_sweeps, field=None,
                                seed_list=False):
    """
    The front matter geodesic_field and geodesic_parents share: every argument
    checked in one order, arrays before any device is asked for, then labels,
    sources and cost as contiguous tensors on one HIP device. "field", which
    geodesic_parents alone has, is float32 of the labels' shape as cost is and
    is checked after it. With seed_list "sources" is a list of seeds, int32
    (S,) with S >= 0, whatever n_labels is. Returns (labels, dims, sources,
    cost, field).
    """
    for name, value in (("sweeps_per_read", sweeps_per_read), ("max_sweeps", max_sweeps)):
        _checked_integer(fn, name, value, optional=name == "max_sweeps")   # both are integers before either's range
    _checked_integer(fn, "sweeps_per_read", sweeps_per_read, least=1)
    _checked_integer(fn, "max_sweeps", max_sweeps, least=0, optional=True)
    _checked_integer(fn, "n_labels", n_labels, least=0, optional=True)
    listed = (("seeds", sources, np.int32, _listed, None, False) if seed_list else
              ("sources", sources, np.int32, _row_per_label(n_labels), None, False))
    labels, dims, (sources, cost, field) = _checked_arrays(fn, labels, (
        listed, ("cost", cost, np.float32, _like_labels, "labels", True),
        ("field", field, np.float32, _like_labels, "labels", True)))
    return labels, dims, sources, cost, field


def geodesic_field(labels, sources, *, cost=None, n_labels=None, sweeps_per_read=32, max_sweeps=None,
                   return_farthest=False, return_device_tensors=False, stats=None):
    """
    The geodesic distance of every voxel from the source of its label, for
    all labels at once, on the device, and each label's farthest voxel.

    What this is: the whole-volume stage of TEASAR that follows the
    distance-to-boundary field. The reference's skeletonize
    (inference.py:257-291) runs kimimaro.skeletonize, which roots every
    segment and takes its distance-from-root field (DAF) from one serial
    Dijkstra per label on the host. Here, exactly, in float32: labels <= 0
    is background; K = len(sources) - 1; sources[L] is the C-order linear
    index of the source voxel of label L, or -1 for none (row 0 is ignored).
    Two voxels are adjacent iff they differ by at most 1 in every coordinate
    (the 26-neighbourhood, in-volume) and carry the same label in 1..K. A
    step costs 1.0f, fl32(sqrt 2) = 0x3FB504F3 or fl32(sqrt 3) = 0x3FDDB3D7
    by the number of coordinates that differ; with "cost" it costs cost[v],
    the cost of the voxel entered (-0.0 counts as 0; a voxel whose cost is
    negative, NaN or +inf cannot be entered). The field d is the least
    solution of d[source] = 0, d[v] = min over adjacent u of
    fl32(d[u] + w(u -> v)), every sum one round-to-nearest float32 addition.
    Adding a non-negative float32 is monotone and never decreases its
    argument, so that solution is unique, does not depend on the order of
    relaxation, and equals bit for bit what a heap Dijkstra computing in
    float32 returns. Background gets 0.0; a foreground voxel of a label
    without a source, of a label above K, or not reachable from the source
    inside its label gets +inf. The farthest table: far_value[L] is the
    largest finite value of label L, far_index[L] the smallest C-order index
    attaining it; 0.0 and -1 for row 0, absent labels and labels without a
    source.

    Two recipes. find_root (a segment without a soma): take
    segment_table(labels)'s peak_index without a field, each label's first
    voxel, as sources; then far_index is the root, and a second call with
    sources=far_index is the DAF. Soma roots: segment_table(labels, dbf)'s
    peak_index, the maximum of the distance-to-boundary field, as sources.

    How: begin, then sweeps_per_read sweeps and one 8-byte read of the
    state, until no tile is flagged. Every sweep but the last makes at least
    one more voxel final, so at most (foreground voxels + 1) sweeps run;
    the count grows with the tortuosity of the longest segment measured in
    8 x 8 x 32 tiles.

    What this is not: equal to dijkstra3d or kimimaro (their background and
    unreachable conventions were not compared; neither is a dependency of
    the project or its tests); the parental field or path extraction (those
    are geodesic_parents and trace_paths); rolling invalidation, fix_borders
    or the SWC export; anisotropic (the reference passes (1, 1, 1));
    multi-source; slab-streamed.

    Parameters
    ----------
    labels : torch.Tensor or numpy.ndarray
        int32 (D, H, W): a tensor on a HIP device, or a numpy array, which
        is uploaded to cuda:0. It is only read.
    sources : torch.Tensor or numpy.ndarray
        int32 (K + 1,), as above; on the labels' device if a tensor.
    cost : torch.Tensor or numpy.ndarray, optional
        float32 of the labels' shape, on the labels' device if a tensor.
        Default is None: Euclidean steps.
    n_labels : int, optional
        K, if given checked against len(sources) - 1. Default is None.
    sweeps_per_read : int, optional
        Sweeps launched between two reads of the state. Default is 32.
    max_sweeps : int, optional
        Raise RuntimeError if the field has not converged after this many
        sweeps. Default is None.
    return_farthest : bool, optional
        Also return (far_value, far_index). Default is False.
    return_device_tensors : bool, optional
        Return device tensors instead of numpy arrays. Default is False.
    stats : dict, optional
        Receives "sweeps", "reads" and "tiles_flagged" (see
        _geodesic_on_device).

    Returns
    -------
    numpy.ndarray or torch.Tensor
        float32 (D, H, W); with return_farthest the tuple
        (field, far_value, far_index), float32 and int32 (K + 1,).

    Raises
    ------
    TypeError
        If labels or sources is not int32, cost is not float32, or
        sweeps_per_read or max_sweeps is not an integer.
    ValueError
        If labels is not 3-D or is empty, sources is not (K + 1,), cost has
        another shape, sweeps_per_read < 1, max_sweeps < 0, the volume has
        more than 2^31 - 1 voxels, or a row of sources names no voxel of its
        label (found at the first read of the device).
    RuntimeError
        If labels is a tensor on a CPU device, sources or cost is on
        another device, there is no HIP device to upload an array to, or
        max_sweeps is exceeded.
    """
    labels, dims, sources, cost, _ = _checked_geodesic_arguments(
        "geodesic_field", labels, sources, cost, n_labels, sweeps_per_read, max_sweeps)
    device = labels.device
    field, far_value, far_index = _geodesic_on_device(
        labels, sources, cost, int(sweeps_per_read), None if max_sweeps is None else int(max_sweeps),
        bool(return_farthest), stats)
    out = _downloaded((field, far_value, far_index) if return_farthest else (field,), device, return_device_tensors)
    return out if return_farthest else out[0]


def _geodesic_parents_on_device(labels, sources, field=None, cost=None, sweeps_per_read=32, max_sweeps=None,
                                stats=None, seeds=None, n_labels=None, out=None, fn="geodesic_parents"):
    """
    geodesic_parents on checked device tensors: the field from
    _geodesic_on_device if none is given, exaspim_geodesic_parents_begin, then
    exaspim_geodesic_parents_sweeps(sweeps_per_read) and one 12-byte read of
    the state until no tile is flagged, exaspim_geodesic_parents_finish and
    one more read. Everything stays on the device.

    Parameters
    ----------
    labels, sources, cost, sweeps_per_read, max_sweeps
        As in _geodesic_on_device.
    field : torch.Tensor, optional
        float32 (D, H, W) on the labels' device: the converged field of these
        labels, sources and cost. Default is None: it is computed first.
    stats : dict, optional
        Receives "sweeps", "reads" and "tiles_flagged" of the hops pass, and
        under "field" those of the field pass if it ran here.
    seeds : torch.Tensor, optional
        int32 (S,) on the labels' device: a list of seeds in place of
        "sources", which is then ignored (exaspim_geodesic_parents_begin_seeds);
        "field" and "n_labels" must be given. Default is None.
    n_labels : int, optional
        K with "seeds". Default is None: len(sources) - 1.
    out : tuple of torch.Tensor, optional
        (parents, hops) to write into. Default is None: they are allocated.
    fn : str, optional
        The name the messages carry.

    Returns
    -------
    parents, hops : torch.Tensor
        int32 (D, H, W).

    Raises
    ------
    ValueError
        For invalid rows of sources and for orphans.
    RuntimeError
        If max_sweeps is exceeded.
    """
    dims = tuple(int(v) for v in labels.shape)
    if seeds is None:
        n_labels = int(sources.numel()) - 1
    device = labels.device
    if field is None:
        field_stats = {}
        field, _, _ = _geodesic_on_device(labels, sources, cost, sweeps_per_read, max_sweeps, False, field_stats)
        if stats is not None:
            stats["field"] = field_stats
    lib = _native.lib()
    dims3 = _native.int3(dims)
    need = _workspace_bytes("exaspim_geodesic_workspace_bytes", dims3)
    cost_ptr = None if cost is None else cost.data_ptr()
    with torch.cuda.device(device):
        stream = _stream(device)
        if out is None:
            hops = torch.empty(dims, dtype=torch.int32, device=device)
            parents = torch.empty(dims, dtype=torch.int32, device=device)
        else:
            parents, hops = out
        state = torch.zeros(3, dtype=torch.int32, device=device)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        if seeds is None:
            _native.check(
                lib.exaspim_geodesic_parents_begin(labels.data_ptr(), dims3, sources.data_ptr(), n_labels,
                                                   field.data_ptr(), hops.data_ptr(), state.data_ptr(),
                                                   workspace.data_ptr(), need, stream),
                "exaspim_geodesic_parents_begin",
            )
        else:
            n_seeds = int(seeds.numel())
            _native.check(
                lib.exaspim_geodesic_parents_begin_seeds(labels.data_ptr(), dims3, n_labels,
                                                         seeds.data_ptr() if n_seeds else None, n_seeds,
                                                         field.data_ptr(), hops.data_ptr(), state.data_ptr(),
                                                         workspace.data_ptr(), need, stream),
                "exaspim_geodesic_parents_begin_seeds",
            )

        def sweeps(batch):
            _native.check(
                lib.exaspim_geodesic_parents_sweeps(labels.data_ptr(), cost_ptr, field.data_ptr(), dims3, n_labels,
                                                    hops.data_ptr(), batch, state.data_ptr(), workspace.data_ptr(),
                                                    need, stream),
                "exaspim_geodesic_parents_sweeps",
            )

        def refusal(invalid):
            if seeds is not None:
                return f"{fn}: {invalid} seed(s) name no voxel of a label in 1..{n_labels} with a field of 0"
            return (f"{fn}: {invalid} row(s) of sources name no voxel of their label with a field of 0 "
                    "(a row L must be -1 or the linear index of a voxel with labels == L and field == 0)")

        swept = _swept_until_settled(sweeps, state, sweeps_per_read, max_sweeps, fn, refusal)
        _native.check(
            lib.exaspim_geodesic_parents_finish(labels.data_ptr(), cost_ptr, field.data_ptr(), hops.data_ptr(), dims3,
                                                n_labels, parents.data_ptr(), state.data_ptr(), stream),
            "exaspim_geodesic_parents_finish",
        )
        orphans = int(state.cpu()[2])
        swept["reads"] += 1
        if stats is not None:
            stats.update(swept)
        if orphans:
            raise ValueError(f"{fn}: {orphans} voxel(s) with a finite field have no tight predecessor: field is not "
                             f"the geodesic field of these labels, {'sources' if seeds is None else 'seeds'} and cost")
    return parents, hops


def geodesic_parents(labels, sources, *, field=None, cost=None, n_labels=None, sweeps_per_read=32, max_sweeps=None,
                     return_hops=False, return_device_tensors=False, stats=None):
    """
    The parental field of every label's geodesic field, on the device: for
    every voxel the neighbour that leads back to the source of its label.

    What this is: the step of TEASAR that follows the fields. The reference's
    skeletonize (inference.py:257-291) runs kimimaro.skeletonize, which takes
    one parental field per label over its penalty field
    (dijkstra3d.parental_field) from a serial Dijkstra on the host and reads
    every path off it. Here, exactly, in integers: labels, sources, cost,
    adjacency, K and the weights w(u -> v) are geodesic_field's, and d is
    "field", the converged result of geodesic_field on exactly these inputs.
    An edge u -> v is tight iff u and v are adjacent, d[u] and d[v] are
    finite, v is not its label's source, and fl32(d[u] + w(u -> v)) has the
    bit pattern of d[v] (the one float32 addition the field was built with).
    hops h (int32) is the least solution of h[source] = 0,
    h[v] = 1 + min over tight u -> v of h[u]: the breadth-first distance from
    the source over tight edges. Every voxel with finite d has one, and as an
    integer least fixed point it is unique and independent of any order.
    parents (int32, C-order linear index): a source gets its own index; any
    other voxel the tight predecessor u with h[u] = h[v] - 1 that has the
    smallest linear index. hops fall by exactly 1 along parents, so there is
    no cycle even on a plateau where d[u] = d[v] because a cost was absorbed;
    the chain from v reaches the source in h[v] steps, and re-adding the
    weights along it reproduces d bit for bit. Everything else gets h = -1
    and parent = -1: background, labels above K, labels without a source,
    voxels with d = +inf. A voxel with finite d that is no source and has no
    tight predecessor (an orphan) exists only if field is not the field of
    these inputs; orphans are counted and raise, never guessed at.

    The TEASAR chain, all on the device: the DAF from the root,
    daf = geodesic_field(labels, roots); the penalty "cost" from the DBF and
    the DAF with torch element-wise operations; pdrf =
    geodesic_field(labels, roots, cost=cost, return_farthest=True); parents,
    hops = geodesic_parents(labels, roots, field=pdrf, cost=cost,
    return_hops=True); trace_paths(parents, hops, far_index) with the
    far_index of the DAF. Only the path voxels leave the card.

    What this is not: equal to dijkstra3d.parental_field or kimimaro (their
    parents are one Dijkstra run's tie-breaks, 1-based with 0 for "none";
    neither is a dependency of the project or its tests); rolling
    invalidation or the choice of the next target, fix_borders, the SWC
    export; anisotropic; multi-source; slab-streamed.

    Parameters
    ----------
    labels, sources, cost, n_labels, sweeps_per_read, max_sweeps
        As in geodesic_field.
    field : torch.Tensor or numpy.ndarray, optional
        float32 of the labels' shape, on the labels' device if a tensor: the
        converged geodesic_field of these labels, sources and cost. Default
        is None: it is computed first, on the device.
    return_hops : bool, optional
        Also return hops. Default is False.
    return_device_tensors : bool, optional
        Return device tensors instead of numpy arrays. Default is False.
    stats : dict, optional
        Receives "sweeps", "reads" and "tiles_flagged" of the hops pass (see
        _geodesic_parents_on_device).

    Returns
    -------
    numpy.ndarray or torch.Tensor
        int32 (D, H, W) parents; with return_hops the tuple (parents, hops).

    Raises
    ------
    TypeError
        As geodesic_field; also if field is not float32.
    ValueError
        As geodesic_field; also if field has another shape, a source's field
        is not 0, or there are orphans: field is not the geodesic field of
        these labels, sources and cost.
    RuntimeError
        As geodesic_field.
    """
    labels, dims, sources, cost, field = _checked_geodesic_arguments(
        "geodesic_parents", labels, sources, cost, n_labels, sweeps_per_read, max_sweeps, field)
    parents, hops = _geodesic_parents_on_device(
        labels, sources, field, cost, int(sweeps_per_read), None if max_sweeps is None else int(max_sweeps), stats)
    out = _downloaded((parents, hops) if return_hops else (parents,), labels.device, return_device_tensors)
    return out if return_hops else out[0]


def trace_paths(parents, hops, targets, *, return_device_tensors=False):
    """
    The paths from the sources to "targets" read off a parental field, on the
    device (the reference's skeletonize, inference.py:257-291: kimimaro's
    path_from_parents).

    The path of a target t with hops[t] >= 0 is the hops[t] + 1 voxels
    source = p_0, ..., p_h = t with parents[p_i] = p_(i-1): voxel v stands at
    position hops[v] of its path. Path i is
    voxels[offsets[i]:offsets[i + 1]], source first; offsets is the
    exclusive cumulative sum of hops[targets] + 1, taken on the device. One
    thread walks each target and takes at most hops[target] steps.

    Parameters
    ----------
    parents, hops : torch.Tensor or numpy.ndarray
        int32 (D, H, W), geodesic_parents' results: tensors on one HIP
        device, or numpy arrays, which are uploaded to cuda:0.
    targets : torch.Tensor or numpy.ndarray
        int32 (T,), T >= 0: C-order linear indices; duplicates are allowed.
    return_device_tensors : bool, optional
        Return device tensors instead of numpy arrays. Default is False.

    Returns
    -------
    voxels : numpy.ndarray or torch.Tensor
        int32 (N,), N the sum of the path lengths.
    offsets : numpy.ndarray or torch.Tensor
        int64 (T + 1,).

    Raises
    ------
    TypeError
        If parents, hops or targets is not int32.
    ValueError
        If parents is not 3-D or is empty, hops has another shape, targets is
        not 1-D, or a target is out of range or has hops < 0.
    RuntimeError
        If parents is a tensor on a CPU device, hops or targets is on another
        device, there is no HIP device to upload an array to, or a walk is
        broken: it leaves the volume, meets -1 or does not end on a source.
    """
    fn = "trace_paths"

    def check_hops(a, shape):
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{fn}: hops must have the parents' shape {tuple(shape)}, got {tuple(a.shape)}")

    def check_targets(a):
        if a.ndim != 1:
            raise ValueError(f"{fn}: targets must be (T,), got {tuple(a.shape)}")

    for what, a in (("hops", hops), ("targets", targets)):
        if isinstance(a, np.ndarray) and a.dtype != np.int32:
            raise TypeError(f"{what} must be int32, got {a.dtype}")
        if isinstance(a, torch.Tensor) and a.dtype != torch.int32:
            raise TypeError(f"{what} must be int32, got {a.dtype}")
    if isinstance(hops, (np.ndarray, torch.Tensor)) and isinstance(parents, (np.ndarray, torch.Tensor)):
        check_hops(hops, parents.shape)
    if isinstance(targets, (np.ndarray, torch.Tensor)):
        check_targets(targets)
    parents, dims = _checked_labels(parents, fn, "parents")
    device = parents.device
    hops = _on_device(hops, fn, "hops", (np.int32,))
    targets = _on_device(targets, fn, "targets", (np.int32,))
    for what, a in (("hops", hops), ("targets", targets)):
        if a.dtype != torch.int32:
            raise TypeError(f"{what} must be int32, got {a.dtype}")
        if a.device != device:
            raise RuntimeError(f"{fn}: {what} must be on the parents' device {device}, got {a.device}")
    check_hops(hops, dims)
    check_targets(targets)
    hops, targets = hops.contiguous(), targets.contiguous()
    n, n_targets = int(parents.numel()), int(targets.numel())
    lib = _native.lib()
    with torch.cuda.device(device):
        offsets = torch.zeros(n_targets + 1, dtype=torch.int64, device=device)
        total = 0
        if n_targets:
            wide = targets.to(torch.int64)
            inside = (wide >= 0) & (wide < n)
            lengths = torch.where(inside, hops.reshape(-1)[wide.clamp(0, n - 1)].to(torch.int64), -1) + 1
            bad = int((lengths < 1).sum())      # the read that also orders the sizes below
            if bad:
                raise ValueError(f"{fn}: {bad} target(s) out of range or with hops < 0 (not reached from a source)")
            torch.cumsum(lengths, 0, out=offsets[1:])
            total = int(offsets[-1])
        voxels = torch.empty(total, dtype=torch.int32, device=device)
        state = torch.zeros(2, dtype=torch.int32, device=device)
        _native.check(
            lib.exaspim_trace_paths(parents.data_ptr(), hops.data_ptr(), _native.int3(dims),
                                    targets.data_ptr() if n_targets else None, n_targets, offsets.data_ptr(),
                                    voxels.data_ptr() if total else None, total, state.data_ptr(), _stream(device)),
            "exaspim_trace_paths",
        )
        refused, broken = (int(v) for v in state.cpu())
        if refused or broken:
            raise RuntimeError(f"{fn}: {broken} broken walk(s) and {refused} refused row(s): parents and hops are not "
                               "the results of one geodesic_parents call")
    return _downloaded((voxels, offsets), device, return_device_tensors)


def _checked_teasar_scalars(fn, scale, const, max_paths):
    """scale and const are finite real numbers >= 0, max_paths is None or an integer >= 1."""
    _checked_real(fn, "scale", scale)
    _checked_real(fn, "const", const)
    _checked_integer(fn, "max_paths", max_paths, least=1, optional=True)


def _checked_teasar_arguments(fn, labels, sources, dbf, daf, parents, hops, boxes, scale, const, n_labels, max_paths,
                              fields=None):
    """
    The front matter of teasar_branches, in _checked_geodesic_arguments'
    manner: the scalars first, then every array before any of them is
    uploaded, then tensors next to a labels tensor, then everything as
    contiguous tensors on the labels' device. Returns (labels, dims, sources,
    dbf, daf, parents, hops, boxes or None, scale, const). With
    fields=(cost, field), teasar_branches_fix_branching's two float32 volumes,
    these two, parents and hops may be None and are returned as None, and
    (cost, field) is appended to the result.
    """
    _checked_teasar_scalars(fn, scale, const, max_paths)
    _checked_integer(fn, "n_labels", n_labels, least=0, optional=True)
    rows = [("sources", sources, np.int32, _row_per_label(n_labels), None, False),
            ("boxes", boxes, np.int32, _six_per_row, "sources", True),
            ("dbf", dbf, np.int32, _like_labels, "labels", False),
            ("daf", daf, np.float32, _like_labels, "labels", False),
            ("parents", parents, np.int32, _like_labels, "labels", fields is not None),
            ("hops", hops, np.int32, _like_labels, "labels", fields is not None)]
    if fields is not None:
        rows += [("cost", fields[0], np.float32, _like_labels, "labels", True),
                 ("field", fields[1], np.float32, _like_labels, "labels", True)]
    labels, dims, out = _checked_arrays(fn, labels, rows)
    sources, boxes, dbf, daf, parents, hops = out[:6]
    return (labels, dims, sources, dbf, daf, parents, hops, boxes, float(scale), float(const)) + tuple(out[6:])


def _pre_check_targets_before(fn, targets_before):
    """What of targets_before can be refused before anything is uploaded or launched."""
    if targets_before is None:
        return
    if not isinstance(targets_before, (tuple, list)) or len(targets_before) != 2:
        raise TypeError(f"{fn}: targets_before must be a pair (target_labels, target_voxels) as border_targets "
                        f"returns it, got {type(targets_before).__name__}")
    for what, a in zip(("target_labels", "target_voxels"), targets_before):
        if not isinstance(a, (np.ndarray, torch.Tensor)):
            raise TypeError(f"{fn}: targets_before's {what} must be a torch tensor or a numpy array, got "
                            f"{type(a).__name__}")
        if a.dtype not in (np.int32, torch.int32):
            raise TypeError(f"{fn}: targets_before's {what} must be int32, got {a.dtype}")
        if a.ndim != 1:
            raise ValueError(f"{fn}: targets_before's {what} must be 1-D, got {tuple(a.shape)}")
    if targets_before[0].shape[0] != targets_before[1].shape[0]:
        raise ValueError(f"{fn}: targets_before's two arrays must have one length, got "
                         f"{targets_before[0].shape[0]} and {targets_before[1].shape[0]}")


def _checked_targets_before(fn, targets_before, device):
    """targets_before as None or two contiguous int32 (T,) tensors on "device"."""
    _pre_check_targets_before(fn, targets_before)
    if targets_before is None:
        return None
    out = []
    for what, a in zip(("target_labels", "target_voxels"), targets_before):
        a = _on_device(a, fn, what, (np.int32,))
        if a.device != device:
            raise RuntimeError(f"{fn}: targets_before's {what} must be on the labels' device {device}, got {a.device}")
        out.append(a.contiguous())
    return tuple(out)


def _teasar_on_device(labels, sources, dbf, daf, parents, hops, boxes, scale, const, max_paths=None, stats=None,
                      on_round=None, update=None, fn="teasar_branches", targets_before=None):
    """
    teasar_branches on checked device tensors: exaspim_teasar_begin, then per
    round exaspim_teasar_round, one 20-byte read of the state, the cumulative
    sum of the lengths with torch and exaspim_teasar_apply. Everything stays on
    the device.

    With targets_before, two int32 (T,) device tensors (labels, voxels): after
    exaspim_teasar_begin the rows whose voxel is not eligible are dropped, the
    rest sorted by (label, voxel) and deduplicated with torch, and rounds
    1..M, M the largest number of rows of one label (one read), run
    exaspim_teasar_round_given (a 24-byte state) with, per label, its t-th
    row or -1. A given round without a branch launches no
    exaspim_teasar_apply and appends nothing, but counts as a round and is
    reported to on_round; the loop ends only once t > M and no label is live.
    With update, a given round is known to exist without the probe: update runs
    before round t iff a round since the last update added vertices.

    Parameters
    ----------
    labels, sources, dbf, daf, parents, hops, boxes : torch.Tensor
        As in teasar_branches, contiguous, on one HIP device.
    scale, const : float
    max_paths : int, optional
    stats : dict, optional
        As in teasar_branches.
    on_round : callable, optional
        Called after every round with (round, mask), mask the uint8 (D, H, W)
        state of every voxel: bit 0 still valid, bit 1 on the skeleton.
    update : callable, optional
        The fix_branching form. exaspim_teasar_round of a round t >= 2 is first
        run on the parents of the round before, only to learn whether a label
        is live (those parents still end on the skeleton, and the call writes
        nothing a second call does not write again); if one is,
        update(t, vertices of round t - 1) returns the (parents, hops) of
        round t and the call is repeated on them. Default is None: one
        parental field for every round.
    fn : str, optional
        The name the messages carry.

    Returns
    -------
    voxels, radii, before : torch.Tensor
        int32 (N,): the vertices, their radii and the vertex before each (the
        junction for a branch's first vertex, -1 for a root).
    offsets : torch.Tensor
        int64 (B + 1,).
    branch_label, branch_round, branch_junction : torch.Tensor
        int32 (B,).

    Raises
    ------
    RuntimeError
        For a broken walk or a refused row, or a round that reports fewer new
        vertices than live labels (the loop would not end).
    """
    dims = tuple(int(v) for v in labels.shape)
    n_labels = int(sources.numel()) - 1
    device = labels.device
    lib = _native.lib()
    dims3 = _native.int3(dims)
    need = _workspace_bytes("exaspim_teasar_workspace_bytes", dims3, n_labels)
    with torch.cuda.device(device):
        stream = _stream(device)
        mask = torch.empty(dims, dtype=torch.uint8, device=device)
        state = torch.empty(5 if targets_before is None else 6, dtype=torch.int32, device=device)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        targets = torch.empty(n_labels + 1, dtype=torch.int32, device=device)
        lengths = torch.empty(n_labels + 1, dtype=torch.int64, device=device)
        junction = torch.empty(n_labels + 1, dtype=torch.int32, device=device)
        offsets = torch.zeros(n_labels + 2, dtype=torch.int64, device=device)
        _native.check(
            lib.exaspim_teasar_begin(labels.data_ptr(), sources.data_ptr(), hops.data_ptr(), daf.data_ptr(), dims3,
                                     n_labels, mask.data_ptr(), state.data_ptr(), workspace.data_ptr(), need, stream),
            "exaspim_teasar_begin",
        )
        rounds, reads, refused, refused_given = 0, 0, 0, 0
        per_round, live_history, new_history, empty_rounds = [], [], [], []
        given_rounds = 0
        if targets_before is not None:
            # the table of given targets: eligible rows only, sorted by (label, voxel), each once
            n = labels.numel()
            t_labels, t_voxels = (t.to(torch.int64) for t in targets_before)
            in_range = (t_labels >= 1) & (t_labels <= n_labels) & (t_voxels >= 0) & (t_voxels < n)
            eligible = in_range & ((mask.reshape(-1)[t_voxels.clamp(0, n - 1)] & 1) != 0)
            key = torch.unique_consecutive(torch.sort((t_labels[eligible] << 32) | t_voxels[eligible]).values)
            given_voxels = (key & 0xFFFFFFFF).to(torch.int32)
            counts = torch.bincount(key >> 32, minlength=n_labels + 1)
            starts = torch.cumsum(counts, 0) - counts
            bad, given_rounds = (int(v) for v in torch.stack([(~in_range).sum(), counts.max()]).cpu())   # one read
            if bad:
                raise ValueError(f"{fn}: {bad} row(s) of targets_before name a label outside 1..{n_labels} or a voxel "
                                 f"outside the volume")

        def walk(round_given=None):
            """exaspim_teasar_round (or _given) on the current parents and the read of its state."""
            if round_given is None:
                _native.check(
                    lib.exaspim_teasar_round(labels.data_ptr(), daf.data_ptr(), parents.data_ptr(), hops.data_ptr(),
                                             dims3, n_labels, mask.data_ptr(), targets.data_ptr(), lengths.data_ptr(),
                                             junction.data_ptr(), state.data_ptr(), workspace.data_ptr(), need,
                                             stream),
                    "exaspim_teasar_round",
                )
            else:
                row = (starts + (round_given - 1)).clamp(max=given_voxels.numel() - 1)
                given = torch.where(counts >= round_given, given_voxels[row], -1).to(torch.int32).contiguous()
                _native.check(
                    lib.exaspim_teasar_round_given(labels.data_ptr(), daf.data_ptr(), parents.data_ptr(),
                                                   hops.data_ptr(), dims3, n_labels, mask.data_ptr(), given.data_ptr(),
                                                   targets.data_ptr(), lengths.data_ptr(), junction.data_ptr(),
                                                   state.data_ptr(), workspace.data_ptr(), need, stream),
                    "exaspim_teasar_round_given",
                )
            return tuple(int(v) for v in state.cpu())

        pending = False   # the last round with a branch has not been handed to update yet
        while max_paths is None or rounds < max_paths:
            if rounds < given_rounds:
                # a given round exists without a probe: its fields are built first, if the skeleton has grown
                if update is not None and pending:
                    parents, hops = update(rounds + 1, per_round[-1][0])
                    pending = False
                live, broken, n_new, n_roots, refused, refused_given = walk(rounds + 1)   # the round's one read
                reads += 1
                if broken or refused or refused_given:
                    break
            else:
                live, broken, n_new, n_roots, refused = walk()[:5]   # the round's one read
                reads += 1
                if broken or refused:
                    break
                if live == 0:
                    break
                if update is not None and pending:
                    # the round exists: only now are its field, hops and parents built, and the walk taken on them
                    parents, hops = update(rounds + 1, per_round[-1][0])
                    pending = False
                    live, broken, n_new, n_roots, refused = walk()[:5]
                    reads += 1
                    if broken or refused:
                        break
                    if live == 0:
                        raise RuntimeError(f"{fn}: round {rounds + 1} had a live label on the parents of the round "
                                           "before and has none on its own: the state bytes changed between two calls")
            if n_new < live:
                # a live label's target is valid, so not on the skeleton: its branch holds at least the target.
                # Fewer vertices than branches is no answer to these arguments, and the loop would never end
                raise RuntimeError(f"{fn}: round {rounds + 1} reports {live} live label(s) and {n_new} new vertices: "
                                   "exaspim_teasar_round took a target that is already on the skeleton, so the per-label "
                                   "keys or the state bytes it read are not the ones this call wrote")
            rounds += 1
            live_history.append(live)
            new_history.append(n_new)
            if live == 0:   # a given round whose targets are all on the skeleton: nothing to apply or append
                empty_rounds.append(rounds)
                if on_round is not None:
                    on_round(rounds, mask)
                continue
            torch.cumsum(lengths, 0, out=offsets[1:])
            voxels = torch.empty(n_new, dtype=torch.int32, device=device)
            radii = torch.empty(n_new, dtype=torch.int32, device=device)
            before = torch.empty(n_new, dtype=torch.int32, device=device)
            _native.check(
                lib.exaspim_teasar_apply(labels.data_ptr(), parents.data_ptr(), dbf.data_ptr(), boxes.data_ptr(), dims3,
                                         n_labels, scale, const, mask.data_ptr(), targets.data_ptr(), lengths.data_ptr(),
                                         junction.data_ptr(), offsets.data_ptr(), voxels.data_ptr(), radii.data_ptr(),
                                         before.data_ptr(), n_new, n_new, n_roots, state.data_ptr(), stream),
                "exaspim_teasar_apply",
            )
            # the labels that have a branch, ascending: a stable sort needs no read, "live" is known already
            rows = torch.argsort((lengths == 0).to(torch.uint8), stable=True)[:live]
            per_round.append((voxels, radii, before, lengths[rows], rows.to(torch.int32), junction[rows], rounds))
            pending = True
            if on_round is not None:
                on_round(rounds, mask)
        else:
            refused = int(state.cpu()[4])   # max_paths cut the loop: the last round's rows have not been read
            reads += 1
        if stats is not None:
            stats.update(rounds=rounds, reads=reads, vertices=new_history, live_labels=live_history)
            if targets_before is not None:
                stats.update(given_rounds=given_rounds, empty_rounds=empty_rounds)
        if refused_given:
            raise RuntimeError(f"{fn}: exaspim_teasar_round_given refused {refused_given} given target(s) in round "
                               f"{rounds + 1}: a row of targets_before names a voxel of another label")
        if broken or refused:
            raise RuntimeError(f"{fn}: {broken} broken walk(s) and {refused} refused row(s): parents and hops are not "
                               "the results of one geodesic_parents call on these labels and sources")

        def joined(i, dtype):
            parts = [r[i] for r in per_round]
            return torch.cat(parts) if parts else torch.empty(0, dtype=dtype, device=device)

        sizes = joined(3, torch.int64)
        out_offsets = torch.zeros(sizes.numel() + 1, dtype=torch.int64, device=device)
        if sizes.numel():
            torch.cumsum(sizes, 0, out=out_offsets[1:])
        branch_round = [torch.full((r[4].numel(),), r[6], dtype=torch.int32, device=device) for r in per_round]
        branch_round = torch.cat(branch_round) if branch_round else torch.empty(0, dtype=torch.int32, device=device)
    return (joined(0, torch.int32), joined(1, torch.int32), joined(2, torch.int32), out_offsets,
            joined(4, torch.int32), branch_round, joined(5, torch.int32))


def teasar_branches(labels, sources, dbf, daf, parents, hops, *, scale, const, boxes=None, n_labels=None,
                    max_paths=None, return_device_tensors=False, stats=None):
    """
    TEASAR's loop for every label at once, on the device: the choice of the
    next target, the branch read off the parental field, and the rolling
    invalidation, until no label has a valid voxel left. Only the skeleton's
    vertices leave the card.

    What this is: the loop of kimimaro's TEASAR, which the reference's
    skeletonize (inference.py:257-291) runs per label on the host, in the
    single-parental-field form: every path is read off ONE parental field,
    which is kimimaro with fix_branching=False. Exactly, in integers:
    K = len(sources) - 1. A voxel v is eligible iff its label L is in 1..K,
    sources[L] names a voxel of L, hops[v] >= 0 and daf[v] is finite with
    the sign bit clear (-0.0 is left out, as geodesic_field's farthest table
    leaves it out). One byte of state per voxel holds "still valid", at first
    the eligible voxels, and "on the skeleton", at first none. Round
    t = 1, 2, ..., all labels in lock-step (labels never interact, so this
    equals K serial loops):

    1. Target: per label the valid voxel with the largest daf bit pattern,
       ties to the smallest C-order linear index. A label without a valid
       voxel is finished; when none is live the loop ends.
    2. Branch: parents are walked from the target to the first voxel on the
       skeleton (the junction) or to the source, a self-parent (round 1:
       junction -1). The new vertices are the walked voxels without the
       junction, listed in ascending hops. The walk takes at most
       hops[target] steps and range-checks every index; one that leaves the
       volume, meets -1 or does not end on a skeleton voxel or the source is
       broken and raises.
    3. Radius: r(p) = min(max(D, H, W), floor(fl64(fl64(scale *
       sqrt64(max(dbf[p], 0))) + const))), one rounded double operation each,
       numpy's np.floor(np.float64(scale) * np.sqrt(d2) + np.float64(const)).
    4. Invalidation: every voxel q with labels[q] == L, inside L's bounding
       box, within Chebyshev distance r(p) of a new vertex p of L becomes
       invalid; other labels' voxels inside the cube are untouched. Then the
       new vertices are marked as on the skeleton.

    Stopping at the junction and clearing, per vertex, its cube minus the
    cube of the vertex before it gives the same valid voxels after every
    round and the same vertices as tracing every path to the root and
    rolling a whole cube along all of it (tests/teasar_ref.py holds the two
    forms to each other); the work per vertex is then a cube's surface.

    What this is not: equal to kimimaro, which is no dependency of the
    project or its tests. The reference runs kimimaro with its default
    fix_branching=True, a Dijkstra per path on a penalty field zeroed along
    the earlier paths; this is the fix_branching=False form. Soma mode (the
    soma_* parameters and the spherical invalidation around a soma root),
    anisotropy, several sources per label and a slab-streamed
    form are not built. (The fix_branching=True form is
    teasar_branches_fix_branching, on fields seeded from the skeleton:
    geodesic_field_seeded and geodesic_parents_seeded.)
    Targets the loop does not choose itself, which fix_borders needs, are
    teasar_branches_given.

    Parameters
    ----------
    labels : torch.Tensor or numpy.ndarray
        int32 (D, H, W): a tensor on a HIP device, or a numpy array, which
        is uploaded to cuda:0. It is only read.
    sources : torch.Tensor or numpy.ndarray
        int32 (K + 1,): the roots, as for geodesic_field.
    dbf : torch.Tensor or numpy.ndarray
        int32 of the labels' shape: squared distances,
        distance_to_boundary's result or any other field.
    daf : torch.Tensor or numpy.ndarray
        float32 of the labels' shape: the priority field; TEASAR uses the
        Euclidean geodesic_field from the roots.
    parents, hops : torch.Tensor or numpy.ndarray
        int32 of the labels' shape: geodesic_parents of the penalty field.
    scale, const : float
        Finite and not negative.
    boxes : torch.Tensor or numpy.ndarray, optional
        int32 (K + 1, 6) from segment_table. Default is None:
        segment_table(labels) is taken here.
    n_labels : int, optional
        K, if given checked against len(sources) - 1. Default is None.
    max_paths : int, optional
        Stop after this many rounds. Default is None.
    return_device_tensors : bool, optional
        Return device tensors instead of numpy arrays. Default is False.
    stats : dict, optional
        Receives "rounds", "reads" (of the 20-byte state, one per round),
        "vertices" (new vertices per round) and "live_labels" (labels with a
        branch per round).

    Returns
    -------
    voxels : numpy.ndarray or torch.Tensor
        int32 (N,): the new vertices, rounds concatenated, then labels
        ascending, then hops ascending within a branch.
    radii : numpy.ndarray or torch.Tensor
        int32 (N,): the invalidation radius of each vertex.
    offsets : numpy.ndarray or torch.Tensor
        int64 (B + 1,): the branch boundaries in voxels.
    branch_label, branch_round, branch_junction : numpy.ndarray or torch.Tensor
        int32 (B,): each branch's label, round (from 1) and junction voxel,
        -1 in round 1.

    Raises
    ------
    TypeError
        If an array or tensor has the wrong dtype, scale or const is not a
        real number, or n_labels or max_paths is not an integer.
    ValueError
        If labels is not 3-D or is empty, a field has another shape, sources
        is not (K + 1,), boxes is not (K + 1, 6), scale or const is negative
        or not finite, max_paths < 1, or the volume has more than 2^31 - 1
        voxels.
    RuntimeError
        If labels is a tensor on a CPU device, another argument is on
        another device, there is no HIP device to upload an array to, a
        walk is broken, or a round reports fewer new vertices than live
        labels.
    """
    return _teasar_branches("teasar_branches", labels, sources, dbf, daf, parents, hops, scale, const, boxes, n_labels,
                            max_paths, return_device_tensors, stats, None)


def _teasar_branches(fn, labels, sources, dbf, daf, parents, hops, scale, const, boxes, n_labels, max_paths,
                     return_device_tensors, stats, targets_before, fields=None):
    """
    teasar_branches and teasar_branches_given: the arguments checked, the loop, the results downloaded. With
    fields=(cost, field), teasar_branches_fix_branching and its _given form: what is None of field, parents and
    hops is computed first, and the loop is _fix_branching_on_device's.
    """
    _pre_check_targets_before(fn, targets_before)
    checked = _checked_teasar_arguments(fn, labels, sources, dbf, daf, parents, hops, boxes, scale, const, n_labels,
                                        max_paths, fields)
    labels, dims, sources, dbf, daf, parents, hops, boxes, scale, const = checked[:10]
    targets_before = _checked_targets_before(fn, targets_before, labels.device)
    if boxes is None:
        boxes = segment_table(labels, n_labels=int(sources.numel()) - 1, return_device_tensors=True)[1]
    max_paths = None if max_paths is None else int(max_paths)
    if fields is None:
        out = _teasar_on_device(labels, sources, dbf, daf, parents, hops, boxes, scale, const, max_paths, stats,
                                fn=fn, targets_before=targets_before)
    else:
        cost, field = checked[10:]
        if field is None:
            field, _, _ = _geodesic_on_device(labels, sources, cost)
        if parents is None or hops is None:
            parents, hops = _geodesic_parents_on_device(labels, sources, field, cost)
        out = _fix_branching_on_device(labels, sources, dbf, daf, cost, field, parents, hops, boxes, scale, const,
                                       max_paths, stats, targets_before=targets_before, fn=fn)
    return _downloaded(out[:2] + out[3:], labels.device, return_device_tensors)


def teasar_branches_given(labels, sources, dbf, daf, parents, hops, targets_before, *, scale, const, boxes=None,
                          n_labels=None, max_paths=None, return_device_tensors=False, stats=None):
    """
    teasar_branches with targets the loop does not choose itself: what
    kimimaro calls manual_targets_before, which its fix_borders feeds with
    the border targets (the reference's skeletonize, inference.py:286), so
    that a skeleton ends at the centre of every cut.

    What this is: teasar_branches' definition with one change to step (1),
    per label, so that a label's result still does not depend on any other
    label. The rows of targets_before whose voxel is not eligible are dropped
    (a label in 26-disconnected pieces has such rows), the rest are taken per
    label in ascending voxel index, each once. In
    round t a label that has at least t given targets takes its t-th one in
    place of step (1); a label that has run out takes the target of step (1)
    as ever. A given target need not be still valid; the walk of step (2)
    is unchanged. A given target that is on the skeleton already is no
    branch: the label has none in that round and is not finished. Round 1
    still puts every live label's source on the skeleton. The loop
    ends only when every label has run out of given targets and none is
    live. With no eligible row the calls and launches are teasar_branches'.

    What this is not: kimimaro. Equality with it is not claimed, and
    max_paths counts rounds, given rounds and rounds without any
    branch included, which is not kimimaro's rule: it counts the paths
    after the given ones.

    Parameters
    ----------
    labels, sources, dbf, daf, parents, hops, scale, const, boxes, n_labels, max_paths, return_device_tensors
        As in teasar_branches.
    targets_before : tuple
        (target_labels, target_voxels), int32 (T,) each, as border_targets
        returns them: arrays, or tensors on the labels' device; any order,
        a pair may occur twice. None means teasar_branches.
    stats : dict, optional
        teasar_branches' entries, and "given_rounds" (the largest number of
        given targets of one label) and "empty_rounds" (the rounds in which
        no label had a branch; they are counted in "rounds" and have 0 in
        "vertices" and "live_labels").

    Returns
    -------
    voxels, radii, offsets, branch_label, branch_round, branch_junction
        As teasar_branches; branch_round counts every round, empty ones
        included.

    Raises
    ------
    TypeError, ValueError, RuntimeError
        As teasar_branches; TypeError if targets_before is not a pair of
        int32 arrays or tensors, ValueError if they are not 1-D of one
        length or a row names a label outside 1..K or a voxel outside the
        volume, RuntimeError if a row's voxel has another label.
    """
    return _teasar_branches("teasar_branches_given", labels, sources, dbf, daf, parents, hops, scale, const, boxes,
                            n_labels, max_paths, return_device_tensors, stats, targets_before)


def _skeleton_chain_on_device(labels, scale, const, pdrf_exponent, pdrf_scale, fill_holes, max_paths,
                              fix_branching=False, stats=None, fix_borders=False):
    """
    The nine stages of skeletonize_labels on a checked device tensor, nothing
    downloaded in between but the words each stage reads for itself. Returns
    a dict of device tensors: "labels" (filled if asked), "dbf", "boxes",
    "roots", "daf", "cost", "parents", "hops", and _teasar_on_device's
    "voxels", "radii", "before", "offsets", "branch_label", "branch_round",
    "branch_junction". With fix_branching the last stage is
    teasar_branches_fix_branching's loop ("parents" and "hops" are round 1's);
    "stats" receives the loop's. With fix_borders, border_targets of the
    labels the chain skeletonises (after fill_holes) goes into the loop as
    targets_before and is returned as "border_targets".
    """
    device = labels.device
    with torch.cuda.device(device):
        if fill_holes:
            labels, _ = _fill_holes_on_device(labels)
        k = max(int(labels.max()), 0)   # the one read of the front matter
        dbf = distance_to_boundary(labels, return_device_tensor=True)
        _, boxes, peak, _ = segment_table(labels, dbf, n_labels=k, return_device_tensors=True)
        first = segment_table(labels, n_labels=k, return_device_tensors=True)[3]
        _, _, roots = _geodesic_on_device(labels, first, farthest=True)
        daf, far_value, _ = _geodesic_on_device(labels, roots, farthest=True)
        rows = labels.clamp(0, k).to(torch.int64)   # labels above K do not occur; negative ones read row 0
        root_peak = peak.to(torch.float32).sqrt()[rows]
        far = far_value[rows]
        zero = torch.zeros((), dtype=torch.float32, device=device)
        depth = torch.where(root_peak > 0, (1 - dbf.to(torch.float32).sqrt() / root_peak) ** pdrf_exponent * pdrf_scale,
                            zero)
        cost = (depth + torch.where(far > 0, daf / far, zero)).to(torch.float32).contiguous()
        del rows, root_peak, far, depth
        pdrf, _, _ = _geodesic_on_device(labels, roots, cost)
        parents, hops = _geodesic_parents_on_device(labels, roots, pdrf, cost)
        names = ("voxels", "radii", "before", "offsets", "branch_label", "branch_round", "branch_junction")
        given = _border_targets_on_device(labels, k) if fix_borders else None
        if fix_branching:
            loop = _fix_branching_on_device(labels, roots, dbf, daf, cost, pdrf, parents, hops, boxes, scale, const,
                                            max_paths, stats, targets_before=given)
        else:
            del pdrf
            loop = _teasar_on_device(labels, roots, dbf, daf, parents, hops, boxes, scale, const, max_paths, stats,
                                     targets_before=given)
        out = dict(zip(names, loop))
        if fix_borders:
            out["border_targets"] = given
    out.update(labels=labels, dbf=dbf, boxes=boxes, roots=roots, daf=daf, cost=cost, parents=parents, hops=hops)
    return out


def skeletonize_labels(labels, *, scale=1.25, const=450.0, pdrf_exponent=4, pdrf_scale=100000.0, fill_holes=True,
                       max_paths=None):
    """
    From labels to skeletons with nothing downloaded between the stages: what
    the reference's skeletonize (inference.py:257-291) asks of
    kimimaro.skeletonize, with the reference's teasar_params as defaults.

    The chain: (1) fill_holes, if asked; (2) distance_to_boundary; (3)
    segment_table; (4) the roots by geodesic_field's find-root recipe: each
    label's first voxel as source, then that field's far_index; (5) the DAF,
    geodesic_field from the roots, and its farthest values; (6) the penalty,
    with torch float32 element-wise operations,
    cost = pdrf_scale * (1 - sqrt(dbf) / sqrt(peak[L])) ** pdrf_exponent
    + daf / far_value[L], the maxima per label gathered through labels and
    either term 0 where its divisor is 0; (7) geodesic_field(cost=cost);
    (8) geodesic_parents; (9) teasar_branches.

    What this is not: kimimaro. The loop is the single-parental-field form of
    TEASAR (kimimaro's fix_branching=False), not the reference's default
    fix_branching=True, which re-runs a Dijkstra per path on a penalty zeroed
    along the earlier paths. Soma detection and its spherical invalidation
    (the soma_* parameters) and anisotropy are not built, and
    equality with kimimaro is not claimed. The reference passes
    fix_borders=True; this function does not end skeletons at the centres of
    the cuts, skeletonize_fix_borders does. A piece of a label that the root's
    piece does not touch gets no skeleton; skeletonize_pieces gives every piece
    one. (skeletonize is this chain with the
    fix_branching=True loop, teasar_branches_fix_branching, as its last
    stage.)

    Parameters
    ----------
    labels : torch.Tensor or numpy.ndarray
        int32 (D, H, W): a tensor on a HIP device, or a numpy array, which
        is uploaded to cuda:0. It is only read.
    scale, const : float, optional
        The invalidation radius is scale * sqrt(dbf) + const voxels.
        Defaults are 1.25 and 450.0.
    pdrf_exponent : int, optional
        Default is 4.
    pdrf_scale : float, optional
        Default is 100000.0.
    fill_holes : bool, optional
        Close the enclosed cavities of every label first. Default is True.
    max_paths : int, optional
        At most this many paths per label. Default is None.

    Returns
    -------
    dict
        label -> (vertices, parent, radius): vertices int32 (n, 3), array
        indices in axis order (z, y, x); parent int32 (n,), the row of each
        vertex's parent on the skeleton, -1 for the root; radius float32
        (n,), sqrt(dbf). Labels without a skeleton are absent.

    Raises
    ------
    TypeError, ValueError, RuntimeError
        As fill_holes, distance_to_boundary, geodesic_field, geodesic_parents
        and teasar_branches; TypeError or ValueError for a pdrf_exponent that
        is no integer >= 0 or a pdrf_scale that is not finite and >= 0.
    """
    return _skeletons_of_labels("skeletonize_labels", labels, scale, const, pdrf_exponent, pdrf_scale, fill_holes,
                                max_paths, False)


def _checked_chain_scalars(fn, scale, const, pdrf_exponent, pdrf_scale, max_paths, fix_borders):
    """The scalars of the skeletonize functions, before any device is asked for."""
    if not isinstance(fix_borders, (bool, np.bool_)):
        raise TypeError(f"{fn}: fix_borders must be a bool, got {type(fix_borders).__name__}")
    _checked_integer(fn, "pdrf_exponent", pdrf_exponent, least=0)
    _checked_real(fn, "pdrf_scale", pdrf_scale)
    _checked_teasar_scalars(fn, scale, const, max_paths)


def _skeletons_of_labels(fn, labels, scale, const, pdrf_exponent, pdrf_scale, fill_holes, max_paths, fix_branching,
                         fix_borders=False):
    """
    skeletonize_labels and skeletonize: the arguments checked, the chain, and the dict put together on the host.
    """
    _checked_chain_scalars(fn, scale, const, pdrf_exponent, pdrf_scale, max_paths, fix_borders)
    labels, dims = _checked_labels(labels, fn)
    chain = _skeleton_chain_on_device(labels, float(scale), float(const), int(pdrf_exponent), float(pdrf_scale),
                                      bool(fill_holes), None if max_paths is None else int(max_paths),
                                      bool(fix_branching), fix_borders=bool(fix_borders))
    return _chain_to_skeletons(fn, chain, dims)


def _chain_to_skeletons(fn, chain, dims):
    """The dict of _skeletons_of_labels from _skeleton_chain_on_device's tensors, put together on the host."""
    with torch.cuda.device(chain["labels"].device):
        voxels, before, offsets, branch_label = (chain[k] for k in ("voxels", "before", "offsets", "branch_label"))
        radius = chain["dbf"].reshape(-1)[voxels.to(torch.int64)].to(torch.float32).sqrt()
        voxels, before, offsets, branch_label, radius = (
            t.cpu().numpy() for t in (voxels, before, offsets, branch_label, radius))
    vertex_label = np.repeat(branch_label, np.diff(offsets))
    out = {}
    for row in np.unique(vertex_label):
        mine = np.nonzero(vertex_label == row)[0]
        vox, prev = voxels[mine], before[mine]
        order = np.argsort(vox, kind="stable")
        at = np.searchsorted(vox[order], np.maximum(prev, 0))
        parent = np.where(prev >= 0, order[np.minimum(at, len(order) - 1)], -1).astype(np.int32)
        if not np.array_equal(vox[parent[prev >= 0]], prev[prev >= 0]):
            raise RuntimeError(f"{fn}: a vertex of label {row} has a parent that is not on the skeleton")
        vertices = np.stack(np.unravel_index(vox, dims), axis=1).astype(np.int32)
        out[int(row)] = (vertices, parent, radius[mine].astype(np.float32))
    return out


def skeleton_to_swc(vertices, parent, radius):
    """
    One skeleton of skeletonize_labels as the text of an SWC file, on the
    host: what the loop of the reference's skeletons_to_zipped_swcs writes
    into its archive. One line per vertex, "id type x y z radius parent":
    ids are 1-based rows, type is 0, the coordinates are the vertex's array
    indices in axis order, and the parent is the 1-based row of the parent,
    -1 for the root.

    Parameters
    ----------
    vertices : numpy.ndarray
        (n, 3), integers or floats.
    parent : numpy.ndarray
        (n,) integers: rows, -1 for a root.
    radius : numpy.ndarray
        (n,) floats.

    Returns
    -------
    str
        n lines, each ended by a newline.

    Raises
    ------
    ValueError
        If the shapes do not belong together or a parent is no row.
    """
    vertices, parent, radius = np.asarray(vertices), np.asarray(parent), np.asarray(radius)
    n = vertices.shape[0] if vertices.ndim == 2 else -1
    if vertices.ndim != 2 or vertices.shape[1] != 3 or parent.shape != (n,) or radius.shape != (n,):
        raise ValueError(f"skeleton_to_swc: vertices must be (n, 3) and parent and radius (n,), got "
                         f"{vertices.shape}, {parent.shape} and {radius.shape}")
    if not np.issubdtype(parent.dtype, np.integer):
        raise ValueError(f"skeleton_to_swc: parent must hold integers, got {parent.dtype}")
    if n and (parent.min() < -1 or parent.max() >= n):
        raise ValueError("skeleton_to_swc: a parent is neither -1 nor a row of vertices")
    lines = []
    for i in range(n):
        x, y, z = (f"{float(c):g}" for c in vertices[i])
        up = int(parent[i])
        lines.append(f"{i + 1} 0 {x} {y} {z} {float(radius[i]):g} {up + 1 if up >= 0 else -1}\n")
    return "".join(lines)


# ---- fields seeded from a list, and TEASAR's fix_branching loop on them ----------------------------
def _geodesic_seeded_on_device(fn, labels, n_labels, seeds, cost=None, field=None, sweeps_per_read=32,
                               max_sweeps=None, stats=None):
    """
    geodesic_field_seeded on checked device tensors. Without "field" the field
    is started by exaspim_geodesic_begin with every source -1; with it, the
    given tensor, a converged field of these labels and cost, is re-seeded IN
    PLACE. Then exaspim_geodesic_reseed, and exaspim_geodesic_sweeps
    (sweeps_per_read) with one 8-byte read of the state until no tile is
    flagged. Everything stays on the device.

    Parameters
    ----------
    fn : str
        The name the messages carry.
    labels : torch.Tensor
        int32 (D, H, W) on a HIP device.
    n_labels : int
        K.
    seeds : torch.Tensor
        int32 (S,), S >= 0, on the same device.
    cost, sweeps_per_read, max_sweeps
        As in _geodesic_on_device.
    field : torch.Tensor, optional
        float32 (D, H, W), contiguous, on the same device; written.
    stats : dict, optional
        Receives "sweeps", "reads" and "tiles_flagged".

    Returns
    -------
    torch.Tensor
        float32 (D, H, W): "field" if it was given.

    Raises
    ------
    ValueError
        For seeds that name no voxel of a label in 1..K.
    RuntimeError
        If max_sweeps is exceeded.
    """
    dims = tuple(int(v) for v in labels.shape)
    device = labels.device
    lib = _native.lib()
    dims3 = _native.int3(dims)
    need = _workspace_bytes("exaspim_geodesic_workspace_bytes", dims3)
    cost_ptr = None if cost is None else cost.data_ptr()
    n_seeds = int(seeds.numel())
    with torch.cuda.device(device):
        stream = _stream(device)
        state = torch.empty(2, dtype=torch.int32, device=device)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        if field is None:
            field = torch.empty(dims, dtype=torch.float32, device=device)
            nowhere = torch.full((n_labels + 1,), -1, dtype=torch.int32, device=device)
            _native.check(
                lib.exaspim_geodesic_begin(labels.data_ptr(), dims3, nowhere.data_ptr(), n_labels, field.data_ptr(),
                                           state.data_ptr(), workspace.data_ptr(), need, stream),
                "exaspim_geodesic_begin",
            )
        _native.check(
            lib.exaspim_geodesic_reseed(labels.data_ptr(), dims3, n_labels, seeds.data_ptr() if n_seeds else None,
                                        n_seeds, field.data_ptr(), state.data_ptr(), workspace.data_ptr(), need,
                                        stream),
            "exaspim_geodesic_reseed",
        )

        def sweeps(batch):
            _native.check(
                lib.exaspim_geodesic_sweeps(labels.data_ptr(), cost_ptr, dims3, n_labels, field.data_ptr(), batch,
                                            state.data_ptr(), workspace.data_ptr(), need, stream),
                "exaspim_geodesic_sweeps",
            )

        swept = _swept_until_settled(
            sweeps, state, sweeps_per_read, max_sweeps, fn,
            lambda invalid: f"{fn}: {invalid} seed(s) name no voxel of a label in 1..{n_labels} (a seed must be the "
                            "linear index of a voxel whose label is in 1..K)")
        if stats is not None:
            stats.update(swept)
    return field


def _label_count(labels, n_labels, fn):
    """K: n_labels checked, or the largest label, read from the device."""
    if n_labels is None:
        with torch.cuda.device(labels.device):
            return max(int(labels.max()), 0)
    return int(n_labels)


def geodesic_field_seeded(labels, seeds, *, cost=None, field=None, n_labels=None, sweeps_per_read=32, max_sweeps=None,
                          return_device_tensor=False, stats=None):
    """
    The geodesic distance of every voxel from the nearest seed of its label,
    for all labels at once, on the device: geodesic_field with any number of
    sources per label, and the way to add sources to a converged field.

    What this is: the primitive under kimimaro's fix_branching=True, which
    the reference's skeletonize (inference.py:257-291) runs: every path after
    the first is a shortest path on a penalty field zeroed along the earlier
    paths. Exactly, in float32: labels, adjacency, "cost" and the weights
    w(u -> v) are geodesic_field's; K is n_labels, or the largest label.
    "seeds" is a list of C-order linear indices, any number per label,
    duplicates allowed; a seed is valid iff it lies in the volume and its
    label is in 1..K. The field d is the least solution of d[s] = +0.0 at
    every seed s and d[v] = min over adjacent u of fl32(d[u] + w(u -> v)):
    bit for bit what a multi-source float32 heap Dijkstra returns, whatever
    the order of relaxation. A seed's own cost is never read. Background gets
    0.0; a label without a seed stays +inf.

    The incremental form: with "field", the converged field of these labels
    and cost and of seeds A, the result is the field of A and "seeds"
    together, bit for bit: every old value is the float32 sum along a real
    path from a voxel that is still a seed, hence an upper bound, and the
    relaxation only lowers values until d[v] <= fl32(d[u] + w) holds on every
    edge. The caller's field is copied, never written. Zeroing the cost along
    a connected set that holds the root and keeping the root as the only
    source (kimimaro's wording) gives the same field.

    What this is not: kimimaro or dijkstra3d (neither is a dependency of the
    project or its tests; equality is not claimed); a farthest table (take
    geodesic_field's on a single-source field); anisotropic; slab-streamed.

    Parameters
    ----------
    labels : torch.Tensor or numpy.ndarray
        int32 (D, H, W): a tensor on a HIP device, or a numpy array, which
        is uploaded to cuda:0. It is only read.
    seeds : torch.Tensor or numpy.ndarray
        int32 (S,), S >= 0; on the labels' device if a tensor.
    cost : torch.Tensor or numpy.ndarray, optional
        float32 of the labels' shape. Default is None: Euclidean steps.
    field : torch.Tensor or numpy.ndarray, optional
        float32 of the labels' shape: a converged field to add the seeds to.
        Default is None: the field is built from scratch.
    n_labels : int, optional
        K. Default is None: the largest label, read from the device.
    sweeps_per_read : int, optional
        Sweeps launched between two reads of the state. Default is 32.
    max_sweeps : int, optional
        Raise RuntimeError if the field has not converged after this many
        sweeps. Default is None.
    return_device_tensor : bool, optional
        Return a device tensor instead of a numpy array. Default is False.
    stats : dict, optional
        Receives "sweeps", "reads" and "tiles_flagged".

    Returns
    -------
    numpy.ndarray or torch.Tensor
        float32 (D, H, W).

    Raises
    ------
    TypeError
        If labels or seeds is not int32, cost or field is not float32, or
        n_labels, sweeps_per_read or max_sweeps is not an integer.
    ValueError
        If labels is not 3-D or is empty, seeds is not 1-D, cost or field has
        another shape, sweeps_per_read < 1, max_sweeps < 0, n_labels < 0, the
        volume has more than 2^31 - 1 voxels, or a seed names no voxel of a
        label in 1..K (found at the first read of the device).
    RuntimeError
        If labels is a tensor on a CPU device, another argument is on another
        device, there is no HIP device to upload an array to, or max_sweeps
        is exceeded.
    """
    fn = "geodesic_field_seeded"
    labels, dims, seeds, cost, field = _checked_geodesic_arguments(
        fn, labels, seeds, cost, n_labels, sweeps_per_read, max_sweeps, field, seed_list=True)
    k = _label_count(labels, n_labels, fn)
    with torch.cuda.device(labels.device):
        if field is not None:
            field = field.clone()
        out = _geodesic_seeded_on_device(fn, labels, k, seeds, cost, field, int(sweeps_per_read),
                                         None if max_sweeps is None else int(max_sweeps), stats)
        return out if return_device_tensor else out.cpu().numpy()


def geodesic_parents_seeded(labels, seeds, field, *, cost=None, n_labels=None, sweeps_per_read=32, max_sweeps=None,
                            return_hops=False, return_device_tensors=False, stats=None):
    """
    The parental field of a seeded field, on the device: for every voxel the
    neighbour that leads back to the nearest seed of its label.

    What this is: geodesic_parents with "the source" read as "a seed", the
    parental field kimimaro's fix_branching=True takes per path (the
    reference's skeletonize, inference.py:257-291). "field" is the converged
    geodesic_field_seeded of exactly these labels, seeds and cost. hops h is
    the least solution of h[s] = 0 at every valid seed s whose field word is
    +0.0 (any other seed counts as invalid) and h[v] = 1 + min over tight
    u -> v of h[u]; no tight edge enters a seed; a seed is its own parent;
    any other voxel's parent is the tight predecessor with one hop less and
    the smallest linear index. The chain from v reaches a seed in h[v] steps,
    and re-adding the weights along it reproduces the field bit for bit.
    Everything else is geodesic_parents'.

    What this is not: kimimaro or dijkstra3d.parental_field; equality is not
    claimed.

    Parameters
    ----------
    labels, seeds, cost, n_labels, sweeps_per_read, max_sweeps
        As in geodesic_field_seeded.
    field : torch.Tensor or numpy.ndarray
        float32 of the labels' shape, on the labels' device if a tensor.
    return_hops : bool, optional
        Also return hops. Default is False.
    return_device_tensors : bool, optional
        Return device tensors instead of numpy arrays. Default is False.
    stats : dict, optional
        Receives "sweeps", "reads" and "tiles_flagged" of the hops pass.

    Returns
    -------
    numpy.ndarray or torch.Tensor
        int32 (D, H, W) parents; with return_hops the tuple (parents, hops).

    Raises
    ------
    TypeError
        As geodesic_field_seeded; also if field is None.
    ValueError
        As geodesic_field_seeded; also if a seed's field is not 0, or there
        are orphans: field is not the seeded field of these labels, seeds and
        cost.
    RuntimeError
        As geodesic_field_seeded.
    """
    fn = "geodesic_parents_seeded"
    if field is None:
        raise TypeError(f"{fn}: field must be a torch tensor or a numpy array, got NoneType")
    labels, dims, seeds, cost, field = _checked_geodesic_arguments(
        fn, labels, seeds, cost, n_labels, sweeps_per_read, max_sweeps, field, seed_list=True)
    k = _label_count(labels, n_labels, fn)
    parents, hops = _geodesic_parents_on_device(
        labels, None, field, cost, int(sweeps_per_read), None if max_sweeps is None else int(max_sweeps), stats,
        seeds=seeds, n_labels=k, fn=fn)
    out = _downloaded((parents, hops) if return_hops else (parents,), labels.device, return_device_tensors)
    return out if return_hops else out[0]


# Sweeps between two reads of the state in an incremental field pass: a re-seeded field settles within a few
# tiles of the new branch, and every sweep launched after it has converged is an empty launch.
FIX_BRANCHING_FIELD_SWEEPS = 8


def _fix_branching_on_device(labels, sources, dbf, daf, cost, field, parents, hops, boxes, scale, const,
                             max_paths=None, stats=None, on_round=None, targets_before=None,
                             fn="teasar_branches_fix_branching"):
    """
    teasar_branches_fix_branching on checked device tensors: _teasar_on_device
    with an update before the walk of every round t >= 2 that exists. The
    update re-seeds a copy of "field" with the vertices of round t - 1
    (exaspim_geodesic_reseed and sweeps), then rebuilds hops and parents with
    all vertices so far as seeds (exaspim_geodesic_parents_begin_seeds, sweeps,
    finish) into tensors of its own. field, parents and hops, those of
    (labels, sources, cost), are only read; the copies are made at the first
    update, so a call with one round allocates none. Returns
    _teasar_on_device's tuple; "stats" additionally receives "updates",
    "field_sweeps" and "hops_sweeps" (one entry per update). With
    targets_before an update is skipped where no vertex has been added since
    the last one (the round before was empty).
    """
    dims = tuple(int(v) for v in labels.shape)
    n_labels = int(sources.numel()) - 1
    device = labels.device
    own, vertices, field_sweeps, hops_sweeps = {}, [], [], []

    def update(t, fresh):
        with torch.cuda.device(device):
            if not own:
                own["field"] = field.clone()
                own["parents"] = torch.empty(dims, dtype=torch.int32, device=device)
                own["hops"] = torch.empty(dims, dtype=torch.int32, device=device)
            vertices.append(fresh)
            field_stats, hops_stats = {}, {}
            _geodesic_seeded_on_device(fn, labels, n_labels, fresh, cost, own["field"], FIX_BRANCHING_FIELD_SWEEPS,
                                       None, field_stats)
            # every vertex of every label: a finished label's zeroed voxels would otherwise count as orphans
            out = _geodesic_parents_on_device(labels, None, own["field"], cost, stats=hops_stats,
                                              seeds=torch.cat(vertices), n_labels=n_labels,
                                              out=(own["parents"], own["hops"]), fn=fn)
            field_sweeps.append(field_stats["sweeps"])
            hops_sweeps.append(hops_stats["sweeps"])
        return out

    result = _teasar_on_device(labels, sources, dbf, daf, parents, hops, boxes, scale, const, max_paths, stats,
                               on_round, update, fn, targets_before)
    if stats is not None:
        stats.update(updates=len(field_sweeps), field_sweeps=field_sweeps, hops_sweeps=hops_sweeps)
    return result


def teasar_branches_fix_branching(labels, sources, dbf, daf, cost, *, scale, const, field=None, parents=None,
                                  hops=None, boxes=None, n_labels=None, max_paths=None, return_device_tensors=False,
                                  stats=None):
    """
    TEASAR's loop in the fix_branching=True form, for every label at once, on
    the device: every path after the first is a shortest path of the penalty
    field re-seeded from the skeleton, so a branch leaves the skeleton where
    that is cheapest instead of running beside it towards the root.

    What this is: the loop the reference's skeletonize (inference.py:257-291)
    asks of kimimaro.skeletonize with its default fix_branching=True. Round 1
    is teasar_branches' round 1, on the field, parents and hops of (labels,
    sources, cost). Before the walk of round t >= 2, (1) the penalty field is
    re-seeded with the vertices of round t - 1, incrementally
    (geodesic_field_seeded's argument: the result is the field seeded from
    the whole skeleton, which is also the field of the cost zeroed along the
    skeleton with the root as the only source, kimimaro's wording), and (2)
    hops and parents are rebuilt with all skeleton vertices of all labels as
    seeds (geodesic_parents_seeded; finished labels included, so that
    "no orphans" keeps its meaning). Targets, radii, cubes, the lock-step of
    the labels and max_paths are exactly teasar_branches'; daf is never
    touched. The walk stops at the first voxel on the skeleton, which with
    seeded parents is the self-parent reached after exactly hops[target]
    steps: the junction. No field, hops or parents work is launched for a
    round that turns out not to exist: updates == rounds - 1, and where every
    label has one path (the reference's const = 450 on a volume whose labels
    fit a 450-voxel cube) the call costs what teasar_branches costs plus one
    more pass over the state bytes.

    What this is not: kimimaro, which is no dependency of the project or its
    tests, and equality with it is not claimed; the definition is this
    project's own, exact and free of any order, and checked against two host
    oracles (tests/fix_branching_ref.py).
    Soma mode, anisotropy and a slab-streamed form are not built.
    (With given targets, which fix_borders needs:
    teasar_branches_fix_branching_given.)

    Parameters
    ----------
    labels, sources, dbf, daf, scale, const, boxes, n_labels, max_paths
        As in teasar_branches.
    cost : torch.Tensor or numpy.ndarray or None
        float32 of the labels' shape: the penalty whose field the paths are
        shortest paths of. None means Euclidean steps.
    field : torch.Tensor or numpy.ndarray, optional
        float32 of the labels' shape: geodesic_field(labels, sources,
        cost=cost). Default is None: it is computed here. Never modified.
    parents, hops : torch.Tensor or numpy.ndarray, optional
        int32 of the labels' shape: geodesic_parents of that field. If either
        is None both are computed here. Never modified.
    return_device_tensors : bool, optional
        Return device tensors instead of numpy arrays. Default is False.
    stats : dict, optional
        Receives teasar_branches' entries ("reads" counts two per round after
        the first) and "updates", "field_sweeps" and "hops_sweeps": the sweeps
        launched by the field pass and by the hops pass of each update.

    Returns
    -------
    voxels, radii, offsets, branch_label, branch_round, branch_junction
        As teasar_branches.

    Raises
    ------
    TypeError, ValueError, RuntimeError
        As teasar_branches, geodesic_field and geodesic_parents.
    """
    return _teasar_branches("teasar_branches_fix_branching", labels, sources, dbf, daf, parents, hops, scale, const,
                            boxes, n_labels, max_paths, return_device_tensors, stats, None, (cost, field))


def teasar_branches_fix_branching_given(labels, sources, dbf, daf, cost, targets_before, *, scale, const, field=None,
                                        parents=None, hops=None, boxes=None, n_labels=None, max_paths=None,
                                        return_device_tensors=False, stats=None):
    """
    teasar_branches_fix_branching with given targets: the loop the
    reference's skeletonize (inference.py:257-291) asks of
    kimimaro.skeletonize with fix_branching=True and fix_borders=True, once
    targets_before is border_targets' result.

    What this is: teasar_branches_given's rule for the target (per label,
    its t-th given target in round t, then the target of step (1)) on
    teasar_branches_fix_branching's fields. A given round is known to exist
    without the probe call. The update before round t re-seeds with every
    vertex added since the last update and is skipped if there is none, so
    once a round is empty updates == rounds - 1 no longer holds: updates ==
    rounds - 1 - (the entries of stats["empty_rounds"] below rounds). A
    given target on the skeleton is a seed of the rebuilt parents, its own
    parent with hops 0: no branch.

    What this is not: kimimaro; equality with it is not claimed, and
    max_paths counts every round.

    Parameters
    ----------
    labels, sources, dbf, daf, cost, scale, const, field, parents, hops, boxes, n_labels, max_paths, return_device_tensors
        As in teasar_branches_fix_branching.
    targets_before : tuple
        As in teasar_branches_given.
    stats : dict, optional
        teasar_branches_fix_branching's entries and teasar_branches_given's
        "given_rounds" and "empty_rounds".

    Returns
    -------
    voxels, radii, offsets, branch_label, branch_round, branch_junction
        As teasar_branches_given.

    Raises
    ------
    TypeError, ValueError, RuntimeError
        As teasar_branches_fix_branching and teasar_branches_given.
    """
    return _teasar_branches("teasar_branches_fix_branching_given", labels, sources, dbf, daf, parents, hops, scale,
                            const, boxes, n_labels, max_paths, return_device_tensors, stats, targets_before,
                            (cost, field))


def skeletonize(segmentation, *, fix_branching=True, scale=1.25, const=450.0, pdrf_exponent=4, pdrf_scale=100000.0,
                fill_holes=True, max_paths=None):
    """
    The reference's skeletonize (inference.py:257-291) under its own name and
    in its own form: skeletonize_labels' chain with, by default, the
    fix_branching=True loop (teasar_branches_fix_branching) as its last
    stage, and the reference's teasar_params as defaults.

    What this is not: kimimaro. The skeletons are not osteoid Skeleton
    objects but skeletonize_labels' plain tuples, and equality with kimimaro
    is not claimed: the definition of every stage is this project's own.
    Soma detection and its spherical invalidation (the soma_* parameters)
    and anisotropy are not built. The reference passes fix_borders=True;
    this function keeps the skeletons of earlier versions, and
    skeletonize_fix_borders is the form that ends them at the centres of the
    cuts. skeletonize_pieces skeletonises every 26-connected piece of a
    label, not the root's alone.

    Parameters
    ----------
    segmentation : torch.Tensor or numpy.ndarray
        int32 (D, H, W): a tensor on a HIP device, or a numpy array, which
        is uploaded to cuda:0. It is only read.
    fix_branching : bool, optional
        True: re-seed the penalty field from the skeleton before every path
        after the first. False: skeletonize_labels' chain, one parental
        field. Default is True.
    scale, const, pdrf_exponent, pdrf_scale, fill_holes, max_paths
        As in skeletonize_labels.

    Returns
    -------
    dict
        label -> (vertices, parent, radius), as skeletonize_labels.

    Raises
    ------
    TypeError, ValueError, RuntimeError
        As skeletonize_labels; TypeError if fix_branching is not a bool.
    """
    if not isinstance(fix_branching, (bool, np.bool_)):
        raise TypeError(f"skeletonize: fix_branching must be a bool, got {type(fix_branching).__name__}")
    return _skeletons_of_labels("skeletonize", segmentation, scale, const, pdrf_exponent, pdrf_scale, fill_holes,
                                max_paths, bool(fix_branching))


def skeletonize_fix_borders(segmentation, *, fix_borders=True, fix_branching=True, scale=1.25, const=450.0,
                            pdrf_exponent=4, pdrf_scale=100000.0, fill_holes=True, max_paths=None):
    """
    skeletonize with the reference's fix_borders=True (inference.py:286):
    wherever a face of the volume cuts a segment, the skeleton is made to
    end at the centre of the cut cross-section. The block next door sees the
    same plane of voxels and picks the same point, so the skeletons of
    adjacent blocks can be joined; without it a branch ends at whichever
    voxel of the cut is geodesically farthest from the root, a corner of the
    cross-section about which the two sides of a seam disagree.

    What this is: skeletonize's chain; border_targets of the labels the chain
    skeletonises (after fill_holes) goes into the loop as given targets
    (teasar_branches_fix_branching_given, or teasar_branches_given with
    fix_branching=False). skeletonize and skeletonize_labels themselves keep
    the skeletons of earlier versions, which is why this is a function of
    its own although the reference passes the switch to the one call.

    What this is not: kimimaro, which breaks the ties of a cut's centre by
    closeness to a centroid; equality with it is not claimed. max_paths
    counts every round, the given ones included. A piece of a label
    that the root's piece does not touch gets no skeleton and its border
    targets are dropped; skeletonize_pieces is the form that keeps them.

    Parameters
    ----------
    segmentation, fix_branching, scale, const, pdrf_exponent, pdrf_scale, fill_holes, max_paths
        As in skeletonize.
    fix_borders : bool, optional
        False gives skeletonize. Default is True.

    Returns
    -------
    dict
        label -> (vertices, parent, radius), as skeletonize_labels.

    Raises
    ------
    TypeError, ValueError, RuntimeError
        As skeletonize; TypeError if fix_borders is not a bool.
    """
    if not isinstance(fix_branching, (bool, np.bool_)):
        raise TypeError(f"skeletonize_fix_borders: fix_branching must be a bool, got {type(fix_branching).__name__}")
    return _skeletons_of_labels("skeletonize_fix_borders", segmentation, scale, const, pdrf_exponent, pdrf_scale,
                                fill_holes, max_paths, bool(fix_branching), fix_borders)


def _skeletons_of_pieces(fn, labels, scale, const, pdrf_exponent, pdrf_scale, fill_holes, max_paths, fix_branching,
                         fix_borders, dust_threshold):
    """
    skeletonize_pieces after its checks: fill_holes on the labels, their
    pieces, the chain on the pieces, and every label's forest put together on
    the host from the trees of its pieces.
    """
    labels, dims = _checked_labels(labels, fn)
    with torch.cuda.device(labels.device):
        if fill_holes:
            labels, _ = _fill_holes_on_device(labels)
        k = max(int(labels.max()), 0)
        pieces, state = _label_pieces_on_device(labels, k, dust_threshold)
        n_pieces, piece_label, _, _ = _piece_tables_on_device(labels, pieces, state)
        if n_pieces == 0:
            return {}
        piece_label = piece_label.cpu().numpy()
    chain = _skeleton_chain_on_device(pieces, float(scale), float(const), int(pdrf_exponent), float(pdrf_scale),
                                      False, None if max_paths is None else int(max_paths), bool(fix_branching),
                                      fix_borders=bool(fix_borders))
    trees = _chain_to_skeletons(fn, chain, dims)
    out = {}
    for piece in sorted(trees):   # ascending piece number
        out.setdefault(int(piece_label[piece - 1]), []).append(trees[piece])
    for label, mine in out.items():
        starts = np.cumsum([0] + [len(tree[1]) for tree in mine[:-1]])
        out[label] = (np.concatenate([tree[0] for tree in mine]),
                      np.concatenate([np.where(tree[1] >= 0, tree[1] + start, -1).astype(np.int32)
                                      for tree, start in zip(mine, starts)]),
                      np.concatenate([tree[2] for tree in mine]))
    return out


def skeletonize_pieces(segmentation, *, dust_threshold=1000, fix_borders=True, fix_branching=True, scale=1.25,
                       const=450.0, pdrf_exponent=4, pdrf_scale=100000.0, fill_holes=True, max_paths=None):
    """
    skeletonize_fix_borders on every 26-connected piece of every label, with
    kimimaro's default dust_threshold: the reference's call
    (inference.py:272-290) leaves that at 1000, and kimimaro.skeletonize
    relabels the volume by 26-connected components, drops those below the
    threshold and merges the component skeletons back under the original
    label. A neurite that leaves a block and comes back is two pieces of one
    label inside that block: the other functions skeletonise the root's
    piece alone and drop the border targets of the rest; this one gives every
    kept piece its tree and its cut centres.

    What this is: (1) fill_holes on the labels, if asked, so that a floating
    piece inside a cavity of its own label is absorbed first; (2)
    label_pieces(dust_threshold=dust_threshold); (3) skeletonize_fix_borders'
    chain on the volume of pieces, without a second fill_holes; (4) on the
    host, the entry of a label is a forest: the trees of its kept pieces
    concatenated in ascending piece number, each tree's rows exactly those
    the chain gives that piece, parents offset into the concatenation, one
    -1 per tree. A label with only dust is absent. max_paths counts per
    piece, every round, the given ones included. skeleton_to_swc,
    skeletons_to_zipped_swcs and voxelize_skeletons take forests as they are.

    What this is not: kimimaro or cc3d; equality with either is not claimed:
    the definition of every stage is this project's own. Soma detection
    and anisotropy are not built; skeletonize_blocks is the form for a
    volume in blocks, with the trees joined across the cuts.
    skeletonize, skeletonize_labels, skeletonize_fix_borders and
    segmentation_to_zipped_swcs keep the skeletons of earlier versions.

    Parameters
    ----------
    segmentation, fix_borders, fix_branching, scale, const, pdrf_exponent, pdrf_scale, fill_holes, max_paths
        As in skeletonize_fix_borders.
    dust_threshold : int, optional
        Pieces of fewer voxels get no skeleton. Default is 1000.

    Returns
    -------
    dict
        label -> (vertices, parent, radius), as skeletonize_labels, with
        one parent of -1 per kept piece of the label.

    Raises
    ------
    TypeError, ValueError, RuntimeError
        As skeletonize_fix_borders; TypeError or ValueError for a
        dust_threshold that is no integer >= 0.
    """
    if not isinstance(fix_branching, (bool, np.bool_)):
        raise TypeError(f"skeletonize_pieces: fix_branching must be a bool, got {type(fix_branching).__name__}")
    dust_threshold = _checked_pieces_scalars("skeletonize_pieces", None, dust_threshold)
    _checked_chain_scalars("skeletonize_pieces", scale, const, pdrf_exponent, pdrf_scale, max_paths, fix_borders)
    return _skeletons_of_pieces("skeletonize_pieces", segmentation, scale, const, pdrf_exponent, pdrf_scale,
                                fill_holes, max_paths, bool(fix_branching), fix_borders, dust_threshold)


def _checked_open_faces(fn, open_faces):
    """open_faces of label_pieces_open as the C call's mask: bit f for face f. Six bools, nothing else."""
    if isinstance(open_faces, (str, bytes)) or not hasattr(open_faces, "__len__"):
        raise TypeError(f"{fn}: open_faces must be a sequence of six bools, got {type(open_faces).__name__}")
    faces = list(open_faces)
    if len(faces) != 6:
        raise ValueError(f"{fn}: open_faces must have six entries (z = 0, z = D - 1, y = 0, y = H - 1, x = 0, "
                         f"x = W - 1), got {len(faces)}")
    for face in faces:
        if not isinstance(face, (bool, np.bool_)):
            raise TypeError(f"{fn}: open_faces must be a sequence of six bools, got an entry of type "
                            f"{type(face).__name__}")
    return sum(1 << f for f, face in enumerate(faces) if face)


def _label_pieces_open_on_device(labels, n_labels, open_mask, dust_threshold=0):
    """
    exaspim_label_pieces_open on a checked device tensor; open_mask is the
    C call's: bit f for face f. Returns the int32 (D, H, W) volume of piece
    numbers and the int32 (3,) state (kept pieces, dust pieces, pieces kept
    although below the threshold), both left on the device: nothing is
    synchronised.
    """
    dims = tuple(int(v) for v in labels.shape)
    device = labels.device
    lib = _native.lib()
    dims3 = _native.int3(dims)
    need = _workspace_bytes("exaspim_label_pieces_open_workspace_bytes", dims3)
    with torch.cuda.device(device):
        pieces = torch.empty(dims, dtype=torch.int32, device=device)
        state = torch.empty(3, dtype=torch.int32, device=device)
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        _native.check(
            lib.exaspim_label_pieces_open(labels.data_ptr(), dims3, int(n_labels), int(dust_threshold), int(open_mask),
                                          pieces.data_ptr(), state.data_ptr(), workspace.data_ptr(), need,
                                          _stream(device)),
            "exaspim_label_pieces_open",
        )
    return pieces, state


def _face_planes(volume, mask):
    """The planes of a (D, H, W) tensor or array that the faces of "mask" name, as views, in face order."""
    planes = (volume[0], volume[-1], volume[:, 0], volume[:, -1], volume[:, :, 0], volume[:, :, -1])
    return [plane for f, plane in enumerate(planes) if mask >> f & 1]


def label_pieces_open(labels, open_faces, *, n_labels=None, dust_threshold=0, return_device_tensors=False):
    """
    label_pieces for one block of a larger volume: a piece that touches an
    open face, a face behind which the volume goes on, is kept whatever its
    size, on the device.

    What this is: label_pieces' definition with one change. The faces are
    border_targets': z = 0, z = D - 1, y = 0, y = H - 1, x = 0, x = W - 1. A
    piece is open iff at least one of its voxels lies on a face whose entry
    of open_faces is True (where a dimension is 1 and two faces coincide,
    either entry opens the plane). A piece is kept iff it is open or size >=
    dust_threshold: inside a block the size of a piece that is cut says
    nothing about the whole piece, so the dust rule must not judge it;
    skeletonize_blocks judges the whole piece after the join. Numbering and
    everything else are label_pieces'; with no face open the first four
    results are label_pieces' exactly. A pure function of the input.

    What this is not: cc3d or kimimaro; equality with either is not claimed.

    Parameters
    ----------
    labels, n_labels, dust_threshold, return_device_tensors
        As in label_pieces.
    open_faces : sequence of six bools
        In the face order above.

    Returns
    -------
    pieces, piece_label, piece_size, piece_first
        As label_pieces.
    piece_open : numpy.ndarray or torch.Tensor
        bool (P,): whether piece i + 1 has a voxel on an open face.

    Raises
    ------
    TypeError, ValueError, RuntimeError
        As label_pieces; TypeError if open_faces is not a sequence of bools,
        ValueError if it has not six entries.
    """
    dust_threshold = _checked_pieces_scalars("label_pieces_open", n_labels, dust_threshold)
    mask = _checked_open_faces("label_pieces_open", open_faces)
    labels, _ = _checked_labels(labels, "label_pieces_open")
    with torch.cuda.device(labels.device):
        if n_labels is None:
            n_labels = max(int(labels.max()), 0)
        pieces, state = _label_pieces_open_on_device(labels, int(n_labels), mask, dust_threshold)
        n_pieces, piece_label, piece_size, piece_first = _piece_tables_on_device(labels, pieces, state)
        touched = torch.zeros(n_pieces + 1, dtype=torch.bool, device=labels.device)
        for plane in _face_planes(pieces, mask):
            touched[plane.reshape(-1).to(torch.int64)] = True
        piece_open = touched[1:].contiguous()
    return _downloaded((pieces, piece_label, piece_size, piece_first, piece_open), labels.device,
                       return_device_tensors)


def _block_spans(n, b):
    """The blocks of skeletonize_blocks along an axis of n voxels with block length b: (start, end) pairs."""
    spans, start = [], 0
    while not spans or start < n - 1:
        spans.append((start, min(start + b, n)))
        start += b - 1
    return spans


_TREE_KEYS = ("block", "piece", "label", "owned_size", "vertices", "parent", "radius", "border_rows")


def _checked_tree_records(trees):
    """join_block_skeletons' records, checked and sorted by (block, piece)."""
    fn = "join_block_skeletons"
    if not isinstance(trees, (list, tuple)):
        raise TypeError(f"{fn}: trees must be a list of records, got {type(trees).__name__}")
    out = []
    for i, tree in enumerate(trees):
        if not isinstance(tree, dict):
            raise TypeError(f"{fn}: record {i} must be a dict, got {type(tree).__name__}")
        missing = [k for k in _TREE_KEYS if k not in tree]
        if missing:
            raise ValueError(f"{fn}: record {i} lacks {', '.join(missing)}")
        for k in ("block", "piece", "label", "owned_size"):
            _checked_integer(fn, f"record {i}'s {k}", tree[k], least=1 if k == "piece" else 0)
        vertices, parent, radius, rows = (np.asarray(tree[k]) for k in ("vertices", "parent", "radius", "border_rows"))
        n = len(parent)
        if vertices.ndim != 2 or vertices.shape != (n, 3) or parent.ndim != 1 or radius.shape != (n,) or n == 0:
            raise ValueError(f"{fn}: record {i} must have vertices (n, 3), parent (n,) and radius (n,) with n >= 1")
        if vertices.dtype.kind not in "iu" or parent.dtype.kind not in "iu" or rows.dtype.kind not in "iub":
            raise TypeError(f"{fn}: record {i}'s vertices, parent and border_rows must be integers")
        if vertices.min() < 0:
            raise ValueError(f"{fn}: record {i} has a negative coordinate")
        if np.count_nonzero(parent == -1) != 1 or parent.min() < -1 or parent.max() >= n:
            raise ValueError(f"{fn}: record {i}'s parent must hold one -1 and otherwise rows of the record")
        rows = rows.astype(np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= n or len(np.unique(rows)) != len(rows)):
            raise ValueError(f"{fn}: record {i}'s border_rows must be distinct rows of the record")
        out.append(dict(block=int(tree["block"]), piece=int(tree["piece"]), label=int(tree["label"]),
                        owned_size=int(tree["owned_size"]), vertices=vertices.astype(np.int64),
                        parent=parent.astype(np.int64), radius=radius.astype(np.float32), border_rows=rows))
    out.sort(key=lambda t: (t["block"], t["piece"]))
    for a, b in zip(out, out[1:]):
        if (a["block"], a["piece"]) == (b["block"], b["piece"]):
            raise ValueError(f"{fn}: two records for piece {a['piece']} of block {a['block']}")
    return out


def join_block_skeletons(trees, dust_threshold=0, stats=None):
    """
    The trees of skeletonize_blocks' blocks joined at the cuts, on the host:
    every label's forest for the whole volume.

    What this is, exactly. A record is a dict with "block" (the block's
    number in block order), "piece" (its number in the block), "label",
    "owned_size" (the piece's voxels that this block owns), "vertices"
    (n, 3) in global (z, y, x), "parent" (n,) with one -1, "radius" (n,) and
    "border_rows", the rows that are border targets in their own block. The
    order of the list does not matter: trees are taken in ascending (block,
    piece). A joint is a global voxel at which two or more trees of one label
    have a border-target vertex. Joints are taken in ascending (z, y, x),
    which is ascending linear index; within a joint the first tree is the
    anchor and every other tree is united with it (union-find), its vertex
    there identified with the anchor's, the radius the smaller of the two:
    each block's field saw only its own side, so each is an upper bound. A
    tree that is already in the anchor's component is skipped: both vertices
    stay and the skip is counted, because the output is a forest and cannot
    hold the ring. A component's root is the root of its first tree, its
    parents are re-oriented from there, its rows are its trees' rows in
    order, an identified vertex at its first occurrence. A component whose
    trees' owned sizes sum to less than dust_threshold is dropped. A
    label's entry is its components in order of first tree, one -1 each.

    What this is not: igneous' or kimimaro's merge; equality with either is
    not claimed. The duplicate vertex of a skipped joint is not removed.

    Parameters
    ----------
    trees : list of dict
        The records.
    dust_threshold : int, optional
        Default is 0.
    stats : dict, optional
        Receives "trees", "joints", "skipped_joints", "dust_components" and
        "join_seconds".

    Returns
    -------
    dict
        label -> (vertices int32 (n, 3), parent int32 (n,), radius float32
        (n,)), what skeleton_to_swc, skeletons_to_zipped_swcs and
        voxelize_skeletons take.

    Raises
    ------
    TypeError, ValueError
        For records that are not as described, a dust_threshold that is no
        integer >= 0, or stats that is not a dict.
    """
    fn = "join_block_skeletons"
    started = time.perf_counter()
    _checked_integer(fn, "dust_threshold", dust_threshold, least=0)
    if stats is not None and not isinstance(stats, dict):
        raise TypeError(f"{fn}: stats must be a dict, got {type(stats).__name__}")
    trees = _checked_tree_records(trees)
    counts = np.array([len(t["parent"]) for t in trees], dtype=np.int64)
    first_node = np.concatenate([[0], np.cumsum(counts)])
    n_nodes = int(first_node[-1])
    tree_of = np.repeat(np.arange(len(trees)), counts)
    vertices = np.concatenate([t["vertices"] for t in trees]) if trees else np.zeros((0, 3), np.int64)
    radius = np.concatenate([t["radius"] for t in trees]) if trees else np.zeros(0, np.float32)
    parent = np.concatenate([np.where(t["parent"] >= 0, t["parent"] + s, -1)
                             for t, s in zip(trees, first_node)]) if trees else np.zeros(0, np.int64)
    label = np.array([t["label"] for t in trees], dtype=np.int64)

    # the joints: border-target vertices of one label at one voxel, in ascending (label, voxel, tree)
    at = np.concatenate([t["border_rows"] + s for t, s in zip(trees, first_node)]) if trees else np.zeros(0, np.int64)
    at = at[np.lexsort((at, vertices[at, 2], vertices[at, 1], vertices[at, 0], label[tree_of[at]]))]
    key = np.column_stack([label[tree_of[at]], vertices[at]])
    new = np.ones(len(at), dtype=bool)
    new[1:] = (key[1:] != key[:-1]).any(axis=1)
    groups = np.split(at, np.nonzero(new)[0][1:]) if len(at) else []
    joints = [g for g in groups if tree_of[g[0]] != tree_of[g[-1]]]      # sorted by tree: two trees at least
    # label by label, ascending voxel within each: no tree has two labels, so this is the order of ascending voxel
    leader = list(range(len(trees)))

    def find(t):
        while leader[t] != t:
            leader[t] = leader[leader[t]]
            t = leader[t]
        return t

    same = np.arange(n_nodes)
    skipped = 0
    for group in joints:
        anchor = int(group[0])
        for node in group[1:]:
            a, b = find(int(tree_of[anchor])), find(int(tree_of[node]))
            if a == b:
                skipped += 1
                continue
            leader[max(a, b)] = min(a, b)      # the leader is the component's first tree
            same[node] = anchor
            radius[anchor] = min(radius[anchor], radius[node])
    component = np.array([find(t) for t in range(len(trees))], dtype=np.int64)
    owned = np.zeros(len(trees), dtype=object)
    for t, c in enumerate(component):
        owned[c] += trees[t]["owned_size"]

    # parents re-oriented from every component's root at once: a breadth-first search over the forest
    kept = same == np.arange(n_nodes)
    child = np.nonzero(parent >= 0)[0]
    ends = np.stack([same[child], same[parent[child]]])
    ends = np.concatenate([ends, ends[::-1]], axis=1)
    order = np.argsort(ends[0], kind="stable")
    source, target = ends[0][order], ends[1][order]
    begin = np.searchsorted(source, np.arange(n_nodes + 1))
    leaders = component == np.arange(len(trees))      # a component's first tree: its root is the component's
    roots = np.nonzero(parent == -1)[0][leaders]      # one -1 per tree, in tree order
    towards = np.full(n_nodes, -2, dtype=np.int64)
    towards[roots] = -1
    front = roots
    while len(front):
        lengths = begin[front + 1] - begin[front]
        edge = np.repeat(begin[front] - np.concatenate([[0], np.cumsum(lengths)[:-1]]), lengths) + np.arange(
            int(lengths.sum()))
        here, there = np.repeat(front, lengths), target[edge]
        fresh = towards[there] == -2
        towards[there[fresh]] = here[fresh]
        front = there[fresh]
    if (towards[kept] == -2).any():
        raise RuntimeError(f"{fn}: a vertex is not connected to its component's root")

    # rows: by label in order of first surviving tree, by component in order of first tree, then as they come
    alive = np.array([owned[c] >= dust_threshold for c in component], dtype=bool)
    rows = np.nonzero(kept & alive[tree_of])[0] if n_nodes else np.zeros(0, np.int64)
    rows = rows[np.argsort(component[tree_of[rows]], kind="stable")]
    out = {}
    for t in np.nonzero(alive & leaders)[0]:
        out.setdefault(int(label[t]), None)
    position = np.full(n_nodes, -1, dtype=np.int64)
    row_label = label[tree_of[rows]]
    for value in out:
        mine = rows[row_label == value]
        position[mine] = np.arange(len(mine))
        up = towards[mine]
        out[value] = (vertices[mine].astype(np.int32),
                      np.where(up >= 0, position[np.maximum(up, 0)], -1).astype(np.int32), radius[mine])
    if stats is not None:
        stats.update(trees=len(trees), joints=len(joints), skipped_joints=skipped,
                     dust_components=int(np.count_nonzero(leaders & ~alive)),
                     join_seconds=time.perf_counter() - started)
    return out


def _checked_block_source(fn, segmentation, block_shape, device):
    """
    skeletonize_blocks' segmentation, block_shape and device, before any
    device is asked for: ((D, H, W), block_shape, device, read), where
    read(z0, z1, y0, y1, x0, x1) gives that block as a contiguous int32
    device tensor and reads nothing else of the segmentation.
    """
    on_device = isinstance(segmentation, torch.Tensor)
    if not on_device and not (hasattr(segmentation, "shape") and hasattr(segmentation, "dtype")
                              and hasattr(segmentation, "__getitem__")):
        raise TypeError(f"{fn}: segmentation must be a torch tensor, a numpy array or an object with shape, dtype and "
                        f"three-slice indexing, got {type(segmentation).__name__}")
    if segmentation.dtype != (torch.int32 if on_device else np.int32):
        raise TypeError(f"segmentation must be int32, got {segmentation.dtype}")
    shape = tuple(int(v) for v in segmentation.shape)
    if len(shape) != 3:
        raise ValueError(f"{fn}: segmentation must be (D, H, W), got {shape}")
    if min(shape) < 1:
        raise ValueError(f"{fn}: empty volume {shape}")
    if isinstance(block_shape, (str, bytes)) or not hasattr(block_shape, "__len__") or len(block_shape) != 3:
        raise ValueError(f"{fn}: block_shape must be three integers, got {block_shape!r}")
    for b in block_shape:
        _checked_integer(fn, "block_shape", b, least=2)
    block_shape = tuple(int(b) for b in block_shape)
    if int(np.prod([min(b, n) for b, n in zip(block_shape, shape)], dtype=object)) > 2**31 - 1:
        raise ValueError(f"{fn}: a block of {block_shape} has more than 2^31 - 1 voxels")
    if on_device:
        if segmentation.device.type != "cuda":
            raise RuntimeError(f"{fn} (MI355X) has no CPU path: segmentation must be on a HIP device, got "
                               f"{segmentation.device}")
        if device is not None and torch.device(device) != segmentation.device:
            raise ValueError(f"{fn}: device {device} is not the segmentation's, {segmentation.device}")
        device = segmentation.device
    else:
        device = _upload_device(fn) if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"{fn} (MI355X) has no CPU path: device must be a HIP device, got {device}")

    def read(z0, z1, y0, y1, x0, x1):
        crop = segmentation[z0:z1, y0:y1, x0:x1]
        if on_device:
            return crop.contiguous()
        crop = np.asarray(crop)
        if crop.dtype != np.int32 or crop.shape != (z1 - z0, y1 - y0, x1 - x0):
            raise TypeError(f"{fn}: segmentation[{z0}:{z1}, {y0}:{y1}, {x0}:{x1}] gave {crop.dtype} {crop.shape}")
        return torch.from_numpy(np.ascontiguousarray(crop)).to(device)

    return shape, block_shape, device, read


def skeletonize_blocks(segmentation, block_shape=(512, 512, 512), *, dust_threshold=1000, fix_branching=True,
                       scale=1.25, const=450.0, pdrf_exponent=4, pdrf_scale=100000.0, fill_holes=True,
                       max_paths=None, device=None, stats=None):
    """
    skeletonize_pieces for a volume that does not fit the device in one
    piece, or has more than 2^31 - 1 voxels: block by block, the trees joined
    at the cuts. The reference's last step (inference.py:240-291)
    for the volumes predict_streaming and agglomerate_affinities_streaming
    were built for.

    What this is. Along an axis of n voxels with block length b, block i
    starts at i (b - 1), for i = 0, 1, ... while the start is below n - 1
    (one block for n = 1), and ends at min(start + b, n): adjacent blocks
    share exactly one plane and every block has at least two. A block's low
    face is open iff it is not the first, its high face iff it is not the
    last. Blocks run in raster order of (iz, iy, ix), the block order. Per
    block: the crop is uploaded; fill_holes, if asked, runs on the block, so a
    cavity that a cut opens is not filled (fill_holes never changes a voxel
    of a face, so both sides of a cut keep seeing the same plane); a block
    without a positive label is skipped; label_pieces_open with the block's
    open faces and dust_threshold; each piece's owned size, its voxels
    outside the block's open high planes, so that every voxel of the volume
    is owned by exactly one block; skeletonize_pieces' chain with
    fix_borders=True on the pieces. Every tree goes to the host with its
    vertices in global coordinates and its border-target rows, and nothing
    of a block stays on the device. join_block_skeletons then joins the
    trees where both sides of a cut ended a branch at the same voxel, and
    drops the components whose owned sizes sum to less than dust_threshold:
    the dust rule judges the whole piece, not what one block sees of it.

    What holds (DESIGN 6r has the proofs): with one block the result is
    skeletonize_pieces(fix_borders=True) array for array; with
    max_paths=None every cut cross-section's centre is a vertex on both
    sides; with fill_holes=False as well, the components are exactly the
    26-connected pieces of the whole volume and the dust decisions are
    label_pieces' on the whole volume; every child and parent are
    26-adjacent and every vertex lies in its label.

    What this is not: the skeleton of the undivided volume (fields and
    invalidation see one block), kimimaro, or igneous' merge; equality with
    any of them is not claimed. Soma mode, anisotropy, a sharded form, overlaps
    of more than one plane and 64-bit labels are not built. A ring across a
    cut keeps a duplicate vertex (a skipped joint).

    Parameters
    ----------
    segmentation : numpy.ndarray, torch.Tensor or array-like
        int32 (D, H, W): a numpy array; a memmap or zarr-like object with
        shape, dtype and three-slice indexing, of which only
        segmentation[z0:z1, y0:y1, x0:x1] is ever read; or a tensor on a HIP
        device. D H W may exceed 2^31 - 1; a block may not.
    block_shape : tuple of int, optional
        Every entry at least 2. Default is (512, 512, 512).
    dust_threshold : int, optional
        Pieces of the whole volume with fewer voxels get no skeleton.
        Default is 1000.
    fix_branching, scale, const, pdrf_exponent, pdrf_scale, max_paths
        As in skeletonize_pieces; max_paths counts per piece of a block.
    fill_holes : bool, optional
        Per block. Default is True.
    device : torch.device, optional
        Where blocks of a host volume are uploaded to. Default is cuda:0.
    stats : dict, optional
        Receives "blocks", "blocks_skipped" (no positive label, or nothing
        but dust), "open_small_pieces" (pieces kept in their block although
        below the threshold), "chain_seconds", and join_block_skeletons'
        "trees", "joints", "skipped_joints", "dust_components" and
        "join_seconds".

    Returns
    -------
    dict
        label -> (vertices, parent, radius), as skeletonize_pieces, the
        vertices in the coordinates of the whole volume.

    Raises
    ------
    TypeError, ValueError, RuntimeError
        As skeletonize_pieces; TypeError for a segmentation that is not
        int32 or has no shape, dtype and indexing, or stats that is not a
        dict; ValueError for a block_shape that is not three integers >= 2 or
        holds more than 2^31 - 1 voxels.
    """
    fn = "skeletonize_blocks"
    if not isinstance(fix_branching, (bool, np.bool_)):
        raise TypeError(f"{fn}: fix_branching must be a bool, got {type(fix_branching).__name__}")
    if stats is not None and not isinstance(stats, dict):
        raise TypeError(f"{fn}: stats must be a dict, got {type(stats).__name__}")
    dust_threshold = _checked_pieces_scalars(fn, None, dust_threshold)
    _checked_chain_scalars(fn, scale, const, pdrf_exponent, pdrf_scale, max_paths, True)
    shape, block_shape, device, read = _checked_block_source(fn, segmentation, block_shape, device)
    spans = [_block_spans(n, b) for n, b in zip(shape, block_shape)]
    trees, blocks, skipped, open_small, chain_seconds = [], 0, 0, 0, 0.0
    for iz, (z0, z1) in enumerate(spans[0]):
        for iy, (y0, y1) in enumerate(spans[1]):
            for ix, (x0, x1) in enumerate(spans[2]):
                block, blocks = blocks, blocks + 1
                faces = [iz > 0, iz < len(spans[0]) - 1, iy > 0, iy < len(spans[1]) - 1, ix > 0,
                         ix < len(spans[2]) - 1]
                mask = sum(1 << f for f, face in enumerate(faces) if face)
                labels = read(z0, z1, y0, y1, x0, x1)
                dims = tuple(int(v) for v in labels.shape)
                with torch.cuda.device(device):
                    if fill_holes:
                        labels, _ = _fill_holes_on_device(labels)
                    k = max(int(labels.max()), 0)
                    if k == 0:
                        skipped += 1
                        continue
                    pieces, state = _label_pieces_open_on_device(labels, k, mask, dust_threshold)
                    n_pieces, piece_label, _, _ = _piece_tables_on_device(labels, pieces, state)
                    open_small += int(state.cpu()[2])
                    if n_pieces == 0:
                        skipped += 1
                        continue
                    own = pieces.clone()
                    for plane in _face_planes(own, mask & 0b101010):
                        plane.zero_()
                    owned = segment_table(own, n_labels=n_pieces, return_device_tensors=True)[0][1:].cpu().numpy()
                    piece_label = piece_label.cpu().numpy()
                    del own, labels
                    started = time.perf_counter()
                    chain = _skeleton_chain_on_device(pieces, float(scale), float(const), int(pdrf_exponent),
                                                      float(pdrf_scale), False,
                                                      None if max_paths is None else int(max_paths),
                                                      bool(fix_branching), fix_borders=True)
                    found = _chain_to_skeletons(fn, chain, dims)
                    target_piece, target_voxel = (t.cpu().numpy() for t in chain["border_targets"])
                    chain_seconds += time.perf_counter() - started
                    del chain, pieces, state
                for piece in sorted(found):
                    vertices, parent, radius = found[piece]
                    voxel = np.ravel_multi_index(tuple(vertices.T), dims)
                    rows = np.nonzero(np.isin(voxel, target_voxel[target_piece == piece]))[0]
                    trees.append(dict(block=block, piece=int(piece), label=int(piece_label[piece - 1]),
                                      owned_size=int(owned[piece - 1]),
                                      vertices=vertices + np.array([z0, y0, x0], dtype=np.int32), parent=parent,
                                      radius=radius, border_rows=rows))
    joined = {}
    out = join_block_skeletons(trees, dust_threshold, joined)
    if stats is not None:
        stats.update(joined, blocks=blocks, blocks_skipped=skipped, open_small_pieces=open_small,
                     chain_seconds=chain_seconds)
    return out


def skeletons_to_zipped_swcs(skeleton_dict, zip_path):
    """
    Saves skeletons as SWC files inside a ZIP archive, on the host (the
    reference's function of this name): one entry "<label>.swc" per skeleton,
    its text skeleton_to_swc's. An existing file is overwritten.

    Parameters
    ----------
    skeleton_dict : dict
        label -> (vertices, parent, radius), as skeletonize returns it.
    zip_path : str or path-like
        The archive to write.

    Raises
    ------
    ValueError
        As skeleton_to_swc, before anything is written.
    """
    import zipfile

    entries = [(f"{segment_id}.swc", skeleton_to_swc(*skeleton)) for segment_id, skeleton in skeleton_dict.items()]
    with zipfile.ZipFile(zip_path, "w") as zip_writer:
        for filename, text in entries:
            zip_writer.writestr(filename, text)


def segmentation_to_zipped_swcs(segmentation, zip_path):
    """
    From a segmentation to an archive of SWC files in one call (the
    reference's function of this name): skeletonize, then
    skeletons_to_zipped_swcs.

    Parameters
    ----------
    segmentation : torch.Tensor or numpy.ndarray
        As in skeletonize.
    zip_path : str or path-like
        The archive to write; an existing file is overwritten.
    """
    skeletons_to_zipped_swcs(skeletonize(segmentation), zip_path)


def voxelize_skeletons(skeleton_dict, img_shape):
    """
    Skeletons as a labelled volume, on the host (the reference's function of
    this name): every vertex's voxel holds its label, everything else 0. Where
    two skeletons share a voxel the later entry of the dict wins.

    Parameters
    ----------
    skeleton_dict : dict
        label -> (vertices, parent, radius), or label -> anything with a
        "vertices" attribute; vertices are (n, 3) array indices (z, y, x).
    img_shape : tuple of int
        (D, H, W).

    Returns
    -------
    numpy.ndarray
        Integers (numpy's default int), of shape img_shape.

    Raises
    ------
    ValueError
        If img_shape is not three positive integers, vertices are not (n, 3),
        or an index lies outside the volume (the reference's indexing would
        wrap a negative one around).
    """
    img_shape = tuple(int(v) for v in img_shape)
    if len(img_shape) != 3 or min(img_shape) < 1:
        raise ValueError(f"voxelize_skeletons: img_shape must be a non-empty (D, H, W), got {img_shape}")
    img = np.zeros(img_shape, dtype=int)
    for segment_id, skeleton in skeleton_dict.items():
        vertices = skeleton.vertices if hasattr(skeleton, "vertices") else skeleton[0]
        voxels = np.asarray(vertices).astype(int)
        if voxels.ndim != 2 or voxels.shape[1] != 3:
            raise ValueError(f"voxelize_skeletons: the vertices of {segment_id} must be (n, 3), got {voxels.shape}")
        if voxels.size and (voxels.min() < 0 or (voxels >= np.array(img_shape)).any()):
            raise ValueError(f"voxelize_skeletons: a vertex of {segment_id} lies outside the volume {img_shape}")
        img[tuple(voxels.T)] = segment_id
    return img


# Provisional ids a streamed labelling may use unless the caller says otherwise (id_capacity): 16 bytes
# of device memory each, so 256 MiB at most; a volume with fewer voxels gets as many ids as voxels.
DEFAULT_ID_CAPACITY = 1 << 24


def _stream_geometry(name, shape, device, id_capacity):
    """(shape, device, id_capacity) of the stream class "name", checked and with the defaults filled in."""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"shape must be a non-empty (D, H, W), got {shape}")
    if shape[1] * shape[2] > 2**31 - 1:
        raise ValueError(f"a plane of {shape[1]} x {shape[2]} voxels exceeds 2^31 - 1")
    device = torch.device("cuda:0" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"{name} (MI355X) has no CPU path: it needs a HIP device, got {device}")
    if id_capacity is None:
        id_capacity = min(DEFAULT_ID_CAPACITY, shape[0] * shape[1] * shape[2])
    id_capacity = int(id_capacity)
    if not 1 <= id_capacity <= 2**31 - 2:
        raise ValueError(f"id_capacity must be 1 .. 2^31 - 2, got {id_capacity}")
    return shape, device, id_capacity


class ComponentsStream:
    """
    affinities_to_components for a volume that arrives in z slabs:
    every slab is labelled while it sits on the device, components are joined
    across the seams between slabs, and the final labels equal, bit for bit,
    those of the whole volume -- which may have more than 2^31 - 1 voxels and
    never has to be anywhere in one piece.

        cs = ComponentsStream((D, H, W), threshold, min_segment_size)
        for slab in slabs_in_z_order:          # (3, d, H, W) device tensors
            provisional = cs.push(slab)        # int32 (d, H, W), provisional ids
            ...keep or download provisional...
        table, k = cs.finish()                 # provisional id -> final label
        cs.apply(provisional)                  # in place, any run of voxels

    Parameters
    ----------
    shape : Tuple[int]
        (D, H, W) of the whole volume; H * W and every slab must stay within
        2^31 - 1 voxels, D * H * W need not.
    threshold, min_segment_size
        As in affinities_to_components.
    foreground : bool, optional
        Slabs are (d, H, W) foreground probabilities instead of (3, d, H, W)
        affinities. Default is False.
    device : torch.device, optional
        Default is cuda:0.
    id_capacity : int, optional
        Most provisional ids the volume may use (1 .. 2^31 - 2). An id goes
        to every slab-local component with more than min_segment_size voxels
        and to every one with an edge across a seam, so shallow slabs of noisy
        affinities need more. The id count stays on the device while slabs are
        pushed; finish() raises if it went past the capacity. 16 bytes of
        device memory per id. Default: DEFAULT_ID_CAPACITY (2^24), or the
        number of voxels if that is less.
    """

    # what a subclass with another slab call replaces (WatershedStream)
    _name = "ComponentsStream"
    _slab_call = "exaspim_components_stream_slab"

    def __init__(self, shape, threshold=0.5, min_segment_size=100, *, foreground=False, device=None,
                 id_capacity=None):
        self.foreground = bool(foreground)
        self._allocate(shape, device, id_capacity, _native.ComponentsStreamDesc(), threshold, min_segment_size)
        self._slab_desc = self.desc

    def _allocate(self, shape, device, id_capacity, desc, threshold, min_segment_size):
        """The device state and the descriptor "desc" (an exaspim_components_stream) that points to it."""
        shape, device, id_capacity = _stream_geometry(self._name, shape, device, id_capacity)
        self.shape, self.device, self.id_capacity = shape, device, id_capacity
        self.finished = False
        plane = shape[1] * shape[2]
        with torch.cuda.device(device):
            self.id_parent = torch.empty(id_capacity + 1, dtype=torch.int32, device=device)
            self.id_count = torch.empty(id_capacity + 1, dtype=torch.int64, device=device)
            self.table = torch.empty(id_capacity + 1, dtype=torch.int32, device=device)
            self.state = torch.zeros(4, dtype=torch.int32, device=device)
            self.seam_ids = torch.empty(plane, dtype=torch.int32, device=device)
            self.seam_bits = torch.empty(plane, dtype=torch.uint8, device=device)
        self.workspace = None
        d = self.desc = desc
        d.dims[:] = shape
        d.channels = 1 if self.foreground else 3
        d.threshold = float(np.float32(threshold))
        d.capacity = id_capacity
        d.min_size = int(min_segment_size)
        d.next_z = 0
        d.id_parent_dev, d.id_count_dev = self.id_parent.data_ptr(), self.id_count.data_ptr()
        d.table_dev, d.state_dev = self.table.data_ptr(), self.state.data_ptr()
        d.seam_ids_dev, d.seam_bits_dev = self.seam_ids.data_ptr(), self.seam_bits.data_ptr()

    @property
    def next_z(self):
        """Planes pushed so far."""
        return int(self.desc.next_z)

    def _scratch(self, need):
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.workspace

    def push(self, slab, z0=None, out=None):
        """
        Labels the next slab. Nothing is synchronised.

        Parameters
        ----------
        slab : torch.Tensor
            float32 or float16 on the stream's device: (3, d, H, W), or
            (d, H, W) in foreground mode, planes [next_z, next_z + d).
        z0 : int, optional
            The slab's first plane, checked against next_z. Default: next_z.
        out : torch.Tensor, optional
            Contiguous int32 (d, H, W) device tensor to write into.

        Returns
        -------
        torch.Tensor
            int32 (d, H, W) provisional ids (0: certainly background).
        """
        if self.finished:
            raise RuntimeError(f"{self._name}: push() after finish()")
        if not isinstance(slab, torch.Tensor):
            raise TypeError(f"push needs a torch tensor, got {type(slab).__name__}")
        if slab.dtype not in _AFF_CODES:
            raise TypeError(f"slab must be float32 or float16, got {slab.dtype}")
        if slab.device != self.device:
            raise RuntimeError(f"slab is on {slab.device}, the stream on {self.device}")
        want_dims = 3 if self.foreground else 4
        if slab.dim() != want_dims or (not self.foreground and slab.shape[0] != 3):
            raise ValueError("slab must be " + ("(d, H, W)" if self.foreground else "(3, d, H, W)") +
                             f", got {tuple(slab.shape)}")
        dims = tuple(int(v) for v in slab.shape[-3:])
        if min(dims) < 1:
            raise ValueError(f"empty slab {dims}")
        slab = slab.contiguous()
        lib = _native.lib()
        need = _workspace_bytes(self._slab_call + "_workspace_bytes", _native.int3(dims))
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty(dims, dtype=torch.int32, device=self.device)
            elif (out.dtype != torch.int32 or tuple(out.shape) != dims or not out.is_contiguous()
                  or out.device != self.device):
                raise ValueError(f"out must be a contiguous int32 {dims} tensor on {self.device}")
            ws = self._scratch(need)
            _native.check(
                getattr(lib, self._slab_call)(
                    ctypes.byref(self._slab_desc), slab.data_ptr(), _AFF_CODES[slab.dtype], _native.int3(dims),
                    self.next_z if z0 is None else int(z0), out.data_ptr(), ws.data_ptr(), need,
                    _stream(self.device)),
                self._slab_call,
            )
        return out

    def finish(self):
        """
        After the last slab: the table from provisional ids to final labels.
        Reads the device's id count and overflow flag, once (this synchronises).

        Returns
        -------
        table : torch.Tensor
            int32 (id_capacity + 1,) on the device, table[0] = 0.
        count : int
            K, the number of kept components.

        Raises
        ------
        RuntimeError
            If the volume needed more provisional ids than id_capacity.
        """
        if self.finished:
            raise RuntimeError(f"{self._name}: finish() called twice")
        lib = _native.lib()
        need = lib.exaspim_components_stream_finish_workspace_bytes(self.id_capacity)
        with torch.cuda.device(self.device):
            ws = self._scratch(need)
            _native.check(
                lib.exaspim_components_stream_finish(ctypes.byref(self.desc), ws.data_ptr(), need,
                                                     _stream(self.device)),
                "exaspim_components_stream_finish",
            )
            self.finished = True
            used, overflow, count, _ = (int(v) for v in self.state.cpu())
        if overflow:
            raise RuntimeError(
                f"{self._name}: the volume needs more than id_capacity={self.id_capacity} provisional ids; "
                "the labels handed out are unusable. Label it again with a larger id_capacity (or deeper slabs)")
        self.ids_used = used
        return self.table, count

    def apply(self, labels):
        """Provisional ids -> final labels, in place, on a contiguous int32 device tensor of any shape."""
        if not self.finished:
            raise RuntimeError(f"{self._name}: apply() before finish()")
        if (not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or labels.device != self.device
                or not labels.is_contiguous()):
            raise ValueError(f"apply needs a contiguous int32 tensor on {self.device}")
        with torch.cuda.device(self.device):
            _native.check(
                _native.lib().exaspim_components_stream_apply(ctypes.byref(self.desc), labels.data_ptr(),
                                                              labels.numel(), _stream(self.device)),
                "exaspim_components_stream_apply",
            )
        return labels


class WatershedStream(ComponentsStream):
    """
    watershed_fragments for a volume that arrives in z slabs: the
    final labels equal, bit for bit, those of the whole volume, which may
    have more than 2^31 - 1 voxels and never has to be anywhere in one piece.
    push, finish, apply, next_z and ids_used are ComponentsStream's.

        ws = WatershedStream((D, H, W), 0.1, 0.9999)
        for slab in slabs_in_z_order:          # (3, d, H, W) device tensors
            provisional = ws.push(slab)
        table, k = ws.finish()
        ws.apply(provisional)

    No plane of the next slab is needed: channel 0 at voxel v is the edge
    v -- v + e_z, so a slab holds the +z edges of its own last plane. What is
    carried is that plane's z affinities as float32 (the next slab's -z
    edges) and two bits per (y, x), eligible and sure, which the next slab
    resolves once it knows the choice of the edge's upper end.

    Parameters
    ----------
    shape : Tuple[int]
        (D, H, W) of the whole volume; H * W and every slab must stay within
        2^31 - 1 voxels, D * H * W need not.
    aff_threshold_low, aff_threshold_high, min_segment_size
        As in watershed_fragments.
    device : torch.device, optional
        Default is cuda:0.
    id_capacity : int, optional
        As in ComponentsStream, with one difference that costs ids, never
        labels: below a seam a slab cannot know whether an eligible z edge
        will be switched on from above, so every slab-local fragment with an
        ELIGIBLE edge across the seam gets an id (the conservative rule of
        foreground mode), not only those with an on edge. Above a seam the
        rule is exact. Watershed fragments are small, so count about one id
        per voxel of a seam plane.
    """

    _name = "WatershedStream"
    _slab_call = "exaspim_watershed_stream_slab"

    def __init__(self, shape, aff_threshold_low=0.1, aff_threshold_high=0.9999, min_segment_size=0, *, device=None,
                 id_capacity=None):
        low, high = float(np.float32(aff_threshold_low)), float(np.float32(aff_threshold_high))
        if low != low or high != high:
            raise ValueError(f"aff_threshold_low and aff_threshold_high must not be NaN, got {low} and {high}")
        self.foreground = False
        d = self._slab_desc = _native.WatershedStreamDesc()
        self._allocate(shape, device, id_capacity, d.base, 0.0, min_segment_size)
        with torch.cuda.device(self.device):
            self.seam_aff = torch.empty(self.shape[1] * self.shape[2], dtype=torch.float32, device=self.device)
        d.low, d.high, d.seam_aff_dev = low, high, self.seam_aff.data_ptr()


def _labels_fit_on_device(device, shape):
    """The provisional labels of the whole volume stay in HBM if they take under a quarter of what is free."""
    free, _ = torch.cuda.mem_get_info(device)
    return int(np.prod(shape, dtype=np.int64)) * 4 <= free // 4


def _relabel_host_array(table, result, planes):
    """The second pass when the provisional labels did not stay on the device: "planes" at a time they
    go up, through the device table and back into the same host array."""
    for z0 in range(0, result.shape[0], planes):
        part = torch.from_numpy(result[z0:z0 + planes]).to(table.device)
        result[z0:z0 + planes] = _apply_table(part, table).cpu().numpy()


# --- The streaming driver ---
# A labeller is what the four streaming entry points build and the driver below runs: .device, .shape (D, H, W),
# push(slab, z0, out) -> the slab's provisional ids (written into "out" if that is a tensor), and, after the
# last slab, finish() -> (table, count): the int32 device table provisional id -> final label, cut to the ids
# in use, and the number of kept labels. Relabelling is one look-up in that table for either kind
# (_apply_table: the kernel behind ComponentsStream.apply as well, with the same arguments up to the cut).
class _ComponentsLabeller:
    """Connected components: a ComponentsStream."""

    def __init__(self, cs):
        self.cs, self.device, self.shape = cs, cs.device, cs.shape

    def push(self, slab, z0, out):
        return self.cs.push(slab, z0, out)

    def finish(self):
        table, count = self.cs.finish()
        return table[: self.cs.ids_used + 1], count


class _LabelSink:
    """
    Where the labels of a streamed volume go, decided once for every driver:
    with "write_block" the caller takes the provisional ids slab by slab and
    gets the table; otherwise they stay in HBM (resident), are relabelled
    there and downloaded once, or, where they do not fit, are collected in a
    host array (result) that takes a second pass through the device.
    """

    def __init__(self, labeller, write_block, keep_labels_resident):
        self.labeller, self.write_block = labeller, write_block
        device, shape = labeller.device, labeller.shape
        if write_block is not None:
            keep_labels_resident = False
        elif keep_labels_resident is None:
            keep_labels_resident = _labels_fit_on_device(device, shape)
        self.resident = torch.empty(shape, dtype=torch.int32, device=device) if keep_labels_resident else None
        self.result = None
        if write_block is None and not keep_labels_resident:
            self.result = np.empty(shape, dtype=np.int32)

    def finish(self, planes):
        """After the last slab: the entry point's return value. "planes": the second pass's step."""
        with torch.cuda.device(self.labeller.device):
            table, count = self.labeller.finish()
            if self.write_block is not None:
                return table.cpu().numpy(), count
            if self.resident is not None:
                return _apply_table(self.resident, table).cpu().numpy()
            _relabel_host_array(table, self.result, planes)
        return self.result


def _label_host_slabs(labeller, source, slab_depth, write_block, keep_labels_resident):
    """The feeder for affinities on the host: source[..., z0:z1, :, :] goes up "slab_depth" planes at a time."""
    sink = _LabelSink(labeller, write_block, keep_labels_resident)
    device, depth = labeller.device, labeller.shape[0]
    with torch.cuda.device(device):
        for z0 in range(0, depth, slab_depth):
            z1 = min(z0 + slab_depth, depth)
            slab = _carrier(np.asarray(source[..., z0:z1, :, :])).to(device)
            labels = labeller.push(slab, z0, None if sink.resident is None else sink.resident[z0:z1])
            if write_block is not None:
                write_block(z0, z1, labels.cpu().numpy())
            elif sink.result is not None:
                sink.result[z0:z1] = labels.cpu().numpy()
    return sink.finish(slab_depth)


def affinities_to_components_streaming(source, threshold=0.5, min_segment_size=100, *, slab_depth,
                                       write_block=None, id_capacity=None, device=None,
                                       keep_labels_resident=None):
    """
    affinities_to_components for affinities that sit in a host array, a
    memmap or a zarr-like array too large for the device (or for 2^31 - 1
    voxels): z slabs of "slab_depth" planes are uploaded and labelled one
    after the other (ComponentsStream), and the result is the whole volume's.

    Parameters
    ----------
    source : array-like
        float32 or float16, (3, D, H, W) affinities or a (D, H, W) foreground
        map; only source[..., z0:z1, :, :] is ever read.
    threshold, min_segment_size
        As in affinities_to_components.
    slab_depth : int
        Planes per slab; slab_depth * H * W must stay within 2^31 - 1.
    write_block : Callable[[int, int, numpy.ndarray], None], optional
        The two-pass contract of chunked segmentation: receives every slab
        once, in z order, as write_block(z0, z1, block) with block int32
        (z1 - z0, H, W) of PROVISIONAL ids; the function then returns the
        table that maps them to final labels instead of the labels.
    id_capacity : int, optional
        See ComponentsStream.
    device : torch.device, optional
        Default is cuda:0.
    keep_labels_resident : bool, optional
        Keep the provisional labels in HBM and relabel them there. Default:
        True if they take less than a quarter of the free device memory;
        otherwise they are relabelled slab by slab in a second device pass
        over the downloaded array.

    Returns
    -------
    numpy.ndarray
        int32 (D, H, W) final labels; or, with "write_block", the tuple
        (table, K): table int32 with final = table[provisional], K kept
        components.
    """
    if not hasattr(source, "shape") or not hasattr(source, "dtype"):
        source = np.asarray(source)
    if np.dtype(source.dtype) not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise TypeError(f"affinities must be float32 or float16, got {source.dtype}")
    shape = tuple(int(v) for v in source.shape)
    if len(shape) == 4 and shape[0] == 3:
        foreground = False
    elif len(shape) == 3:
        foreground = True
    else:
        raise ValueError(f"affinities must be (3, D, H, W) or a (D, H, W) foreground map, got shape {shape}")
    vshape = shape[-3:]
    slab_depth = int(slab_depth)
    if slab_depth < 1:
        raise ValueError(f"slab_depth must be positive, got {slab_depth}")
    if not torch.cuda.is_available():
        raise RuntimeError("affinities_to_components_streaming (MI355X) has no CPU path and no HIP device is present")
    cs = ComponentsStream(vshape, threshold, min_segment_size, foreground=foreground, device=device,
                          id_capacity=id_capacity)
    return _label_host_slabs(_ComponentsLabeller(cs), source, slab_depth, write_block, keep_labels_resident)


def _checked_host_affinities(fn, source, slab_depth):
    """(source, (D, H, W), slab_depth) of a streamed function that needs (3, D, H, W) affinities on the host."""
    if not hasattr(source, "shape") or not hasattr(source, "dtype"):
        source = np.asarray(source)
    if np.dtype(source.dtype) not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise TypeError(f"affinities must be float32 or float16, got {source.dtype}")
    shape = tuple(int(v) for v in source.shape)
    if len(shape) != 4 or shape[0] != 3:
        raise ValueError(f"{fn} needs (3, D, H, W) affinities, got {shape}; a foreground map has no affinities")
    slab_depth = int(slab_depth)
    if slab_depth < 1:
        raise ValueError(f"slab_depth must be positive, got {slab_depth}")
    return source, shape[-3:], slab_depth


def watershed_fragments_streaming(source, aff_threshold_low=0.1, aff_threshold_high=0.9999, min_segment_size=0, *,
                                  slab_depth, write_block=None, id_capacity=None, device=None,
                                  keep_labels_resident=None):
    """
    watershed_fragments for affinities that sit in a host array, a memmap or
    a zarr-like array too large for the device (or for 2^31 - 1 voxels): z
    slabs of "slab_depth" planes are uploaded and labelled one after the
    other (WatershedStream), and the result is the whole volume's, bit for
    bit, whatever the slab depth.

    Parameters
    ----------
    source : array-like
        float32 or float16 (3, D, H, W); only source[..., z0:z1, :, :] is ever
        read. A foreground map has no affinities.
    aff_threshold_low, aff_threshold_high, min_segment_size
        As in watershed_fragments.
    slab_depth : int
        Planes per slab; slab_depth * H * W must stay within 2^31 - 1.
    write_block, device, keep_labels_resident
        As in affinities_to_components_streaming.
    id_capacity : int, optional
        See WatershedStream.

    Returns
    -------
    numpy.ndarray
        int32 (D, H, W) final labels; or, with "write_block", the tuple
        (table, K): table int32 with final = table[provisional], K kept
        fragments.
    """
    source, vshape, slab_depth = _checked_host_affinities("watershed_fragments_streaming", source, slab_depth)
    low, high = float(np.float32(aff_threshold_low)), float(np.float32(aff_threshold_high))
    if low != low or high != high:
        raise ValueError(f"aff_threshold_low and aff_threshold_high must not be NaN, got {low} and {high}")
    if not torch.cuda.is_available():
        raise RuntimeError("watershed_fragments_streaming (MI355X) has no CPU path and no HIP device is present")
    ws = WatershedStream(vshape, low, high, min_segment_size, device=device, id_capacity=id_capacity)
    return _label_host_slabs(_ComponentsLabeller(ws), source, slab_depth, write_block, keep_labels_resident)


class RegionGraphStream:
    """
    region_graph for a volume that arrives in z slabs: every slab
    is pushed with its labels -- provisional ids, e.g. ComponentsStream's --
    and its affinities while both sit on the device; finish() maps the ids
    through a table and returns the region graph of the final labels, bit for
    bit what region_graph gives on table[labels] of the whole volume, which
    may have more than 2^31 - 1 voxels and never has to be anywhere in one
    piece.

        cs = ComponentsStream((D, H, W), fragment_threshold, 0)
        rgs = RegionGraphStream((D, H, W))
        for slab in slabs_in_z_order:              # (3, d, H, W) device tensors
            rgs.push(cs.push(slab), slab)
        table, k = cs.finish()
        edges, counts, sums, sizes = rgs.finish(table, k)

    Two planes are carried from slab to slab, the last plane's ids and its
    quantised z affinities: ComponentsStream's own seam plane has already
    moved on to the current slab when the graph sees it.

    Parameters
    ----------
    shape : Tuple[int]
        (D, H, W) of the whole volume; H * W and every slab must stay within
        2^31 - 1 voxels, D * H * W need not.
    device : torch.device, optional
        Default is cuda:0.
    id_capacity : int, optional
        The largest id that counts (1 .. 2^31 - 2): labels beyond it are
        counted nowhere. 8 bytes of device memory per id. Default:
        DEFAULT_ID_CAPACITY (2^24), or the number of voxels if that is less,
        as in ComponentsStream.
    edge_capacity : int, optional
        Slots of the accumulator, a power of two; 24 bytes each, and as many
        again while finish() runs. It holds pairs of PROVISIONAL ids: a slab
        cannot know that two of its ids belong to one fragment, so shallow
        slabs need more slots than the final graph has edges. Default is the
        smaller of 2^22 and the next power of two >= 6 * D * H * W.
    """

    def __init__(self, shape, *, device=None, id_capacity=None, edge_capacity=None):
        shape, device, id_capacity = _stream_geometry("RegionGraphStream", shape, device, id_capacity)
        if edge_capacity is None:
            edge_capacity = _default_edge_capacity(shape[0] * shape[1] * shape[2])
        edge_capacity = int(edge_capacity)
        if not 1 <= edge_capacity <= 1 << 30 or edge_capacity & (edge_capacity - 1):
            raise ValueError(f"edge_capacity must be a power of two in 1 .. 2^30, got {edge_capacity}")
        self.shape, self.device = shape, device
        self.id_capacity, self.edge_capacity = id_capacity, edge_capacity
        plane = shape[1] * shape[2]
        with torch.cuda.device(device):
            self.keys = torch.empty(edge_capacity, dtype=torch.int64, device=device)     # uint64 bits
            self.counts = torch.empty(edge_capacity, dtype=torch.int64, device=device)
            self.sums = torch.empty(edge_capacity, dtype=torch.int64, device=device)
            self.sizes_by_id = torch.empty(id_capacity + 1, dtype=torch.int64, device=device)
            self.seam_ids = torch.empty(plane, dtype=torch.int32, device=device)
            self.seam_q = torch.empty(plane, dtype=torch.int32, device=device)            # uint32 bits
            self.state = torch.zeros(2, dtype=torch.int32, device=device)
        d = self.desc = _native.RegionGraphStreamDesc()
        d.dims[:] = shape
        d.id_capacity, d.edge_capacity, d.next_z = id_capacity, edge_capacity, 0
        d.keys_dev, d.counts_dev, d.sums_dev = self.keys.data_ptr(), self.counts.data_ptr(), self.sums.data_ptr()
        d.sizes_by_id_dev = self.sizes_by_id.data_ptr()
        d.seam_ids_dev, d.seam_q_dev = self.seam_ids.data_ptr(), self.seam_q.data_ptr()
        d.state_dev = self.state.data_ptr()

    @property
    def next_z(self):
        """Planes pushed so far."""
        return int(self.desc.next_z)

    def push(self, labels, slab, z0=None):
        """
        Adds the next slab to the graph. Nothing is synchronised.

        Parameters
        ----------
        labels : torch.Tensor
            int32 (d, H, W) on the stream's device: the slab's ids.
        slab : torch.Tensor
            float32 or float16 (3, d, H, W) on the same device, planes
            [next_z, next_z + d).
        z0 : int, optional
            The slab's first plane, checked against next_z. Default: next_z.
        """
        if not isinstance(labels, torch.Tensor) or not isinstance(slab, torch.Tensor):
            raise TypeError(f"push needs torch tensors, got {type(labels).__name__} and {type(slab).__name__}")
        if labels.dtype != torch.int32:
            raise TypeError(f"labels must be int32, got {labels.dtype}")
        if slab.dtype not in _AFF_CODES:
            raise TypeError(f"slab must be float32 or float16, got {slab.dtype}")
        if labels.device != self.device or slab.device != self.device:
            raise RuntimeError(f"labels are on {labels.device} and the slab on {slab.device}, the stream on "
                               f"{self.device}")
        if slab.dim() != 4 or slab.shape[0] != 3:
            raise ValueError(f"slab must be (3, d, H, W), got {tuple(slab.shape)}; "
                             "a foreground map has no affinities to score")
        dims = tuple(int(v) for v in slab.shape[-3:])
        if tuple(labels.shape) != dims:
            raise ValueError(f"labels must be (d, H, W) = {dims}, got {tuple(labels.shape)}")
        if min(dims) < 1:
            raise ValueError(f"empty slab {dims}")
        labels, slab = labels.contiguous(), slab.contiguous()
        with torch.cuda.device(self.device):
            _native.check(
                _native.lib().exaspim_region_graph_stream_slab(
                    ctypes.byref(self.desc), labels.data_ptr(), slab.data_ptr(), _AFF_CODES[slab.dtype],
                    _native.int3(dims), self.next_z if z0 is None else int(z0), _stream(self.device)),
                "exaspim_region_graph_stream_slab",
            )

    def finish(self, table, n_labels):
        """
        After the last slab: the region graph of table[ids]. Reads the edge
        count and the overflow flag, once (this synchronises). The accumulated
        graph of ids is left as it is, so finish may be called again with
        another table.

        Parameters
        ----------
        table : torch.Tensor or numpy.ndarray
            int32 (n,): id -> final label; ids at or beyond n are background.
        n_labels : int
            Final labels are 1 .. n_labels; what the table maps elsewhere
            forms no edge and counts as background.

        Returns
        -------
        edges, counts, sums, sizes
            As region_graph returns them, sorted by (lo, hi).

        Raises
        ------
        RuntimeError
            If the slabs had more distinct pairs of adjacent ids than
            edge_capacity.
        """
        edges, counts, sums, sizes, n_edges = self.finish_on_device(table, n_labels)
        with torch.cuda.device(self.device):
            return _download_graph(edges, counts, sums, sizes, n_edges)

    def finish_on_device(self, table, n_labels):
        """
        finish() without the download: the same launches and the same one read
        of the state, and the graph of the final labels stays on the device
        (as _region_graph_device is to _region_graph_on_device).

        Returns
        -------
        edges, counts, sums : torch.Tensor
            int32 (edge_capacity, 2), int64 (edge_capacity,), int64
            (edge_capacity,) holding uint64 bits: the first n_edges rows in an
            unspecified order.
        sizes : torch.Tensor
            int64 (n_labels + 1,).
        n_edges : int
        """
        if isinstance(table, np.ndarray):
            if table.dtype != np.dtype(np.int32):
                raise TypeError(f"table must be int32, got {table.dtype}")
            table = torch.from_numpy(np.ascontiguousarray(table)).to(self.device)
        if not isinstance(table, torch.Tensor):
            raise TypeError(f"table must be a torch tensor or a numpy array, got {type(table).__name__}")
        if table.dtype != torch.int32 or table.dim() != 1 or table.numel() < 1:
            raise TypeError(f"table must be a non-empty 1-D int32 tensor, got {table.dtype} {tuple(table.shape)}")
        if table.device != self.device:
            raise RuntimeError(f"table is on {table.device}, the stream on {self.device}")
        n_labels = int(n_labels)
        if n_labels < 0:
            raise ValueError(f"n_labels must not be negative, got {n_labels}")
        if self.next_z != self.shape[0]:
            raise RuntimeError(f"RegionGraphStream: finish() after {self.next_z} of {self.shape[0]} planes")
        table = table.contiguous()
        capacity = self.edge_capacity
        lib = _native.lib()
        need = _workspace_bytes("exaspim_region_graph_stream_finish_workspace_bytes", capacity)
        with torch.cuda.device(self.device):
            edges = torch.empty((capacity, 2), dtype=torch.int32, device=self.device)
            counts = torch.empty(capacity, dtype=torch.int64, device=self.device)
            sums = torch.empty(capacity, dtype=torch.int64, device=self.device)   # uint64 bits
            sizes = torch.empty(n_labels + 1, dtype=torch.int64, device=self.device)
            state = torch.empty(2, dtype=torch.int32, device=self.device)
            workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            _native.check(
                lib.exaspim_region_graph_stream_finish(
                    ctypes.byref(self.desc), table.data_ptr(), min(table.numel(), 2**31 - 1), n_labels,
                    edges.data_ptr(), counts.data_ptr(), sums.data_ptr(), sizes.data_ptr(), state.data_ptr(),
                    workspace.data_ptr(), need, _stream(self.device)),
                "exaspim_region_graph_stream_finish",
            )
            n_edges, overflow = (int(v) for v in state.cpu())   # the one read of the device state
            if overflow:
                raise RuntimeError(
                    f"RegionGraphStream: the slabs have more pairs of adjacent provisional ids than "
                    f"edge_capacity={capacity}. Shallow slabs need more slots than the final graph has edges: "
                    "two ids of one fragment look like two fragments until finish. Run it again with a larger "
                    "edge_capacity (a power of two) or deeper slabs")
        return edges, counts, sums, sizes, n_edges


def _agglomerate_streams(cs, rgs, thresholds, min_segment_size, premerge_size=0, premerge_rounds=4,
                         device_merge_rounds=0):
    """
    After the last slab of both streams: the fragments' graph, its merging on
    the host, and the table provisional id -> segment, composed on the device
    by sending the fragment table itself through the segment table. With
    premerge_size or device_merge_rounds the graph stays on the device for
    the pre-merge and the dominant rounds, as in _device_merged_table, only
    the reduced graph is downloaded, and the rounds' maps are composed onto
    the fragment table on the device as well.

    Returns
    -------
    table : torch.Tensor
        int32 (ids_used + 1,) on the device: segment[fragment[id]].
    count : int
        S, the number of kept segments.
    """
    fragment_table, n_fragments = cs.finish()
    if not premerge_size and not device_merge_rounds:
        edges, counts, sums, sizes = rgs.finish(fragment_table[: cs.ids_used + 1], n_fragments)
        segment_table, n_segments = agglomerate(edges, counts, sums, sizes, thresholds, min_segment_size)
        with torch.cuda.device(cs.device):
            table = _apply_table(fragment_table[: cs.ids_used + 1].clone(),
                                 torch.from_numpy(segment_table).to(cs.device))
        return table, n_segments
    edges, counts, sums, sizes, n_edges = rgs.finish_on_device(fragment_table[: cs.ids_used + 1], n_fragments)
    capacity = rgs.edge_capacity
    with torch.cuda.device(cs.device):
        table = fragment_table[: cs.ids_used + 1].clone()
        if premerge_size:
            edges, counts, sums, sizes, n_edges, composed, _ = _premerge_on_device(
                edges, counts, sums, sizes, n_edges, thresholds[-1], premerge_size, premerge_rounds, capacity)
            _apply_table(table, composed)
        if device_merge_rounds:
            # a contraction keeps the total count or lowers it: what the pre-merge has checked stays checked
            edges, counts, sums, sizes, n_edges, dominant, _ = _contract_dominant_on_device(
                edges, counts, sums, sizes, n_edges, thresholds[-1], device_merge_rounds, capacity,
                total_checked=bool(premerge_size))
            _apply_table(table, dominant)
        graph = _download_graph(edges, counts, sums, sizes, n_edges)
        segment_table, n_segments = agglomerate(*graph, thresholds, min_segment_size)
        _apply_table(table, torch.from_numpy(segment_table).to(cs.device))
    return table, n_segments


class _AgglomerationLabeller:
    """Mean-affinity agglomeration: a ComponentsStream or a WatershedStream with no size filter and a
    RegionGraphStream of its ids; "merging": the keywords of _agglomerate_streams' device rounds."""

    def __init__(self, cs, rgs, thresholds, min_segment_size, **merging):
        self.cs, self.rgs, self.device, self.shape = cs, rgs, cs.device, cs.shape
        self.thresholds, self.min_segment_size, self.merging = thresholds, min_segment_size, merging

    def push(self, slab, z0, out):
        labels = self.cs.push(slab, z0, out)
        self.rgs.push(labels, slab, z0)
        return labels

    def finish(self):
        return _agglomerate_streams(self.cs, self.rgs, self.thresholds, self.min_segment_size, **self.merging)


def _checked_fragment_options(fragments, aff_threshold_low, aff_threshold_high, premerge_size, premerge_rounds,
                              device_merge_rounds):
    """The fragment and device-merging keywords of the streamed agglomerations, checked as agglomerate_affinities
    checks them: (low, high) rounded to float32 and the keywords of _agglomerate_streams."""
    premerge_size, premerge_rounds = _checked_premerge(premerge_size, premerge_rounds)
    device_merge_rounds = _checked_rounds("device_merge_rounds", device_merge_rounds, 0)
    if fragments not in ("components", "watershed"):
        raise ValueError(f'fragments must be "components" or "watershed", got {fragments!r}')
    low, high = float(np.float32(aff_threshold_low)), float(np.float32(aff_threshold_high))
    if fragments == "watershed" and (low != low or high != high):
        raise ValueError(f"aff_threshold_low and aff_threshold_high must not be NaN, got {low} and {high}")
    return low, high, dict(premerge_size=premerge_size, premerge_rounds=premerge_rounds,
                           device_merge_rounds=device_merge_rounds)


def _fragment_stream(fragments, shape, fragment_threshold, low, high, device, id_capacity):
    """The stream of fragments, no size filter: connected components at a threshold or watershed basins."""
    if fragments == "watershed":
        return WatershedStream(shape, low, high, 0, device=device, id_capacity=id_capacity)
    return ComponentsStream(shape, fragment_threshold, 0, device=device, id_capacity=id_capacity)


def agglomerate_affinities_streaming(source, agglomeration_thresholds=[0.6, 0.8, 0.9], min_segment_size=100, *,
                                     fragment_threshold=0.5, slab_depth, write_block=None, id_capacity=None,
                                     edge_capacity=None, device=None, keep_labels_resident=None,
                                     fragments="components", aff_threshold_low=0.1, aff_threshold_high=0.9999,
                                     premerge_size=0, premerge_rounds=4, device_merge_rounds=0):
    """
    agglomerate_affinities for affinities that sit in a host array, a memmap
    or a zarr-like array too large for the device (or for 2^31 - 1 voxels):
    z slabs of "slab_depth" planes are uploaded one after the other, each is
    labelled (ComponentsStream with no size filter) and added to the region
    graph of provisional ids (RegionGraphStream) while it sits on the device;
    at the end the graph of fragments is merged on the host and the
    provisional labels go through the composed table segment[fragment[id]]
    once. The result equals agglomerate_affinities on the whole volume, bit
    for bit.

    Parameters
    ----------
    source : array-like
        float32 or float16 (3, D, H, W); only source[..., z0:z1, :, :] is ever
        read. A foreground map has no affinities to score.
    agglomeration_thresholds, min_segment_size, fragment_threshold
        As in agglomerate_affinities.
    slab_depth : int
        Planes per slab; slab_depth * H * W must stay within 2^31 - 1.
    write_block : Callable[[int, int, numpy.ndarray], None], optional
        Receives every slab once, in z order, as write_block(z0, z1, block)
        with block int32 (z1 - z0, H, W) of PROVISIONAL ids; the function then
        returns the table that maps them to segment labels.
    id_capacity : int, optional
        See ComponentsStream.
    edge_capacity : int, optional
        See RegionGraphStream.
    device : torch.device, optional
        Default is cuda:0.
    keep_labels_resident : bool, optional
        As in affinities_to_components_streaming.
    fragments, aff_threshold_low, aff_threshold_high, premerge_size,
    premerge_rounds, device_merge_rounds
        As in agglomerate_affinities, and with the same result as the
        whole-volume call with the same values, bit for bit.
        fragments="watershed" labels the slabs with a WatershedStream
         instead of a ComponentsStream; with premerge_size or
        device_merge_rounds the graph of fragments stays on the device for
        those rounds after the last slab. With the defaults nothing but
        what is described above is launched.

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
    if not hasattr(source, "shape") or not hasattr(source, "dtype"):
        source = np.asarray(source)
    if np.dtype(source.dtype) not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise TypeError(f"affinities must be float32 or float16, got {source.dtype}")
    shape = tuple(int(v) for v in source.shape)
    if len(shape) != 4 or shape[0] != 3:
        raise ValueError(f"agglomerate_affinities_streaming needs (3, D, H, W) affinities, got {shape}; "
                         "a foreground map has no affinities to score")
    vshape = shape[-3:]
    slab_depth = int(slab_depth)
    if slab_depth < 1:
        raise ValueError(f"slab_depth must be positive, got {slab_depth}")
    if not torch.cuda.is_available():
        raise RuntimeError("agglomerate_affinities_streaming (MI355X) has no CPU path and no HIP device is present")
    cs = _fragment_stream(fragments, vshape, fragment_threshold, low, high, device, id_capacity)
    rgs = RegionGraphStream(vshape, device=cs.device, id_capacity=cs.id_capacity, edge_capacity=edge_capacity)
    return _label_host_slabs(_AgglomerationLabeller(cs, rgs, thresholds, min_segment_size, **merging), source,
                             slab_depth, write_block, keep_labels_resident)


# ---- the overlap table of two label volumes, and the scores read off it ---------------------------
DEFAULT_PAIR_CAPACITY = 1 << 22
_MAX_ADD_VOXELS = 2**31 - 1
_BACKGROUND_MODES = ("a", "both_zero", "none")


def _default_pair_capacity(voxels):
    want = 2 * int(voxels)
    return min(DEFAULT_PAIR_CAPACITY, 1 << max(want - 1, 0).bit_length())


def _checked_pair_capacity(fn, pair_capacity, voxels=None):
    if pair_capacity is None:
        return DEFAULT_PAIR_CAPACITY if voxels is None else _default_pair_capacity(voxels)
    _checked_integer(fn, "pair_capacity", pair_capacity)
    pair_capacity = int(pair_capacity)
    if not 1 <= pair_capacity <= 1 << 30 or pair_capacity & (pair_capacity - 1):
        raise ValueError(f"{fn}: pair_capacity must be a power of two in 1 .. 2^30, got {pair_capacity}")
    return pair_capacity


class OverlapStream:
    """
    The overlap table of two label volumes that arrive piece by piece (DESIGN
    6u): label_overlaps' table of everything added so far, which may be more
    than 2^31 - 1 voxels and never has to be anywhere in one piece.

        table = OverlapStream(1 << 20)
        for a_block, b_block in blocks:            # equal shapes, any shapes
            table.add(a_block, b_block)
        pairs, counts = table.finish()

    The table is additive over voxels and its counts are integers, so the
    result does not depend on how the voxels are cut into blocks or on the
    order of the blocks. finish() only reads the table: it may be called
    twice, and again after further add()s.

    Parameters
    ----------
    pair_capacity : int
        Slots of the device hash table, a power of two in 1 .. 2^30; 16 bytes
        each. It must hold every distinct pair (a', b').
    device : torch.device, optional
        Default is cuda:0.
    """

    def __init__(self, pair_capacity, device=None):
        self.pair_capacity = _checked_pair_capacity("OverlapStream", pair_capacity)
        device = _upload_device("OverlapStream") if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"OverlapStream (MI355X) has no CPU path: device must be a HIP device, got {device}")
        self.device = device
        self.voxels = 0
        self._bytes = _workspace_bytes("exaspim_label_overlaps_workspace_bytes", self.pair_capacity)
        with torch.cuda.device(device):
            self._workspace = torch.empty(self._bytes, dtype=torch.uint8, device=device)
            _native.check(
                _native.lib().exaspim_label_overlaps_reset(self.pair_capacity, self._workspace.data_ptr(),
                                                           self._bytes, _stream(device)),
                "exaspim_label_overlaps_reset",
            )

    def _block(self, block, what):
        if isinstance(block, np.ndarray):
            if block.dtype != np.int32:
                raise TypeError(f"{what} must be int32, got {block.dtype}")
            return _carrier(block).to(self.device)
        if not isinstance(block, torch.Tensor):
            raise TypeError(f"{what} must be a torch tensor or a numpy array, got {type(block).__name__}")
        if block.dtype != torch.int32:
            raise TypeError(f"{what} must be int32, got {block.dtype}")
        if block.device != self.device:
            raise RuntimeError(f"OverlapStream.add (MI355X) has no CPU path: {what} must be on {self.device}, got "
                               f"{block.device}")
        return block.contiguous()

    def add(self, a_block, b_block):
        """Adds the voxels of two int32 blocks of equal shape, device tensors or numpy arrays, to the table."""
        a, b = self._block(a_block, "a_block"), self._block(b_block, "b_block")
        if a.shape != b.shape:
            raise ValueError(f"OverlapStream.add: a_block and b_block must have one shape, got "
                             f"{tuple(a.shape)} and {tuple(b.shape)}")
        a, b = a.reshape(-1), b.reshape(-1)
        lib = _native.lib()
        with torch.cuda.device(self.device):
            for start in range(0, a.numel(), _MAX_ADD_VOXELS):
                n = min(_MAX_ADD_VOXELS, a.numel() - start)
                _native.check(
                    lib.exaspim_label_overlaps_add(a.data_ptr() + 4 * start, b.data_ptr() + 4 * start, n,
                                                   self.pair_capacity, self._workspace.data_ptr(), self._bytes,
                                                   _stream(self.device)),
                    "exaspim_label_overlaps_add",
                )
        self.voxels += a.numel()

    def finish_on_device(self):
        """(pairs int32 (capacity, 2), counts int64 (capacity,), P): the first P rows, in an unspecified order."""
        capacity, device = self.pair_capacity, self.device
        with torch.cuda.device(device):
            pairs = torch.empty((capacity, 2), dtype=torch.int32, device=device)
            counts = torch.empty(capacity, dtype=torch.int64, device=device)
            state = torch.empty(2, dtype=torch.int32, device=device)
            _native.check(
                _native.lib().exaspim_label_overlaps_finish(capacity, self._workspace.data_ptr(), self._bytes,
                                                            pairs.data_ptr(), counts.data_ptr(), state.data_ptr(),
                                                            _stream(device)),
                "exaspim_label_overlaps_finish",
            )
            n_pairs, overflow = (int(v) for v in state.cpu())   # the one read of the device state
        if overflow:
            raise RuntimeError(
                f"label_overlaps: the volumes have more distinct pairs of labels than pair_capacity={capacity}; "
                "run it again with a larger pair_capacity (a power of two)")
        return pairs, counts, n_pairs

    def finish(self, return_device_tensors=False):
        """
        The table of everything added so far: pairs int32 (P, 2), rows
        (a', b') sorted by (a', b'), and counts int64 (P,). With
        return_device_tensors the first P rows as device tensors in the
        table's own, unspecified order.
        """
        pairs, counts, n_pairs = self.finish_on_device()
        if return_device_tensors:
            return pairs[:n_pairs], counts[:n_pairs]
        with torch.cuda.device(self.device):
            pairs_h = pairs[:n_pairs].cpu().numpy().reshape(-1, 2)
            counts_h = counts[:n_pairs].cpu().numpy()
        order = np.lexsort((pairs_h[:, 1], pairs_h[:, 0]))   # slot order depends on arrival: sort by (a', b')
        return np.ascontiguousarray(pairs_h[order]), np.ascontiguousarray(counts_h[order])


def label_overlaps(a, b, *, pair_capacity=None, return_device_tensors=False):
    """
    The overlap table of two label volumes on the device: for
    every ordered pair (label in a, label in b) that occurs at some voxel,
    the number of voxels that carry it.

    For a label value v, v' = v if v > 0 else 0: everything <= 0 is
    background, as in fill_holes. For every voxel count[(a', b')] += 1. The
    pair is ordered: (1, 2) and (2, 1) are different rows. Every positive
    int32 is a legal label; no label becomes an address. Counts are 64-bit
    integers, so the result does not depend on the order in which the device
    adds them, and they sum to D * H * W.

    Parameters
    ----------
    a, b : torch.Tensor or numpy.ndarray
        int32 (D, H, W) of equal shape. Device tensors (on one HIP device)
        are used where they are; numpy arrays are uploaded to cuda:0.
    pair_capacity : int, optional
        Slots of the device hash table, a power of two; 16 bytes each.
        Default is the smaller of 2^22 and the next power of two >= 2 * D *
        H * W.
    return_device_tensors : bool, optional
        Return the rows as device tensors, in the table's own unspecified
        order.

    Returns
    -------
    pairs : numpy.ndarray
        int32 (P, 2), rows (a', b') sorted by (a', b').
    counts : numpy.ndarray
        int64 (P,).

    Raises
    ------
    RuntimeError
        If the volumes have more distinct pairs than pair_capacity; the
        message asks for a larger one.
    """
    a, dims = _checked_labels(a, "label_overlaps", "a")
    b, dims_b = _checked_labels(b, "label_overlaps", "b")
    if dims != dims_b:
        raise ValueError(f"label_overlaps: a and b must have one shape, got {dims} and {dims_b}")
    if a.device != b.device:
        raise RuntimeError(f"label_overlaps (MI355X) has no CPU path: a and b must be on one HIP device, got "
                           f"{a.device} and {b.device}")
    capacity = _checked_pair_capacity("label_overlaps", pair_capacity, int(np.prod(dims, dtype=np.int64)))
    stream = OverlapStream(capacity, a.device)
    stream.add(a, b)
    return stream.finish(return_device_tensors)


def _checked_label_source(fn, source, what):
    """(source, (D, H, W)) of a streamed function that needs int32 labels on the host."""
    if not hasattr(source, "shape") or not hasattr(source, "dtype") or not hasattr(source, "__getitem__"):
        source = np.asarray(source)
    if isinstance(source, torch.Tensor) or np.dtype(source.dtype) != np.dtype(np.int32):
        raise TypeError(f"{fn}: {what} must be a host array of int32, got {type(source).__name__} of {source.dtype}")
    shape = tuple(int(v) for v in source.shape)
    if len(shape) != 3:
        raise ValueError(f"{fn}: {what} must be (D, H, W), got {shape}")
    if min(shape) < 1:
        raise ValueError(f"{fn}: empty volume {shape}")
    return source, shape


def label_overlaps_streaming(source_a, source_b, *, slab_depth, pair_capacity=None, device=None):
    """
    label_overlaps for volumes that sit in host arrays, memmaps or zarr-like
    arrays too large for the device (or for 2^31 - 1 voxels): z slabs of
    "slab_depth" planes of both are uploaded and added one after the other
    (OverlapStream). The table is additive over voxels, so the result is the
    whole volume's, array for array, whatever the slab depth.

    Parameters
    ----------
    source_a, source_b : array-like
        int32 (D, H, W) of equal shape; only source[z0:z1] is ever read.
    slab_depth : int
        Planes per slab; slab_depth * H * W must stay within 2^31 - 1.
    pair_capacity : int, optional
        As in label_overlaps; the default is 2^22 or the next power of two
        >= 2 * D * H * W if that is less.
    device : torch.device, optional
        Default is cuda:0.

    Returns
    -------
    pairs, counts : numpy.ndarray
        As label_overlaps gives them.
    """
    fn = "label_overlaps_streaming"
    source_a, shape = _checked_label_source(fn, source_a, "source_a")
    source_b, shape_b = _checked_label_source(fn, source_b, "source_b")
    if shape != shape_b:
        raise ValueError(f"{fn}: source_a and source_b must have one shape, got {shape} and {shape_b}")
    _checked_integer(fn, "slab_depth", slab_depth)
    slab_depth = int(slab_depth)
    if slab_depth < 1:
        raise ValueError(f"slab_depth must be positive, got {slab_depth}")
    if min(slab_depth, shape[0]) * shape[1] * shape[2] > _MAX_ADD_VOXELS:
        raise ValueError(f"{fn}: a slab of {slab_depth} planes of {shape[1:]} has more than 2^31 - 1 voxels")
    capacity = _checked_pair_capacity(fn, pair_capacity, shape[0] * shape[1] * shape[2])
    stream = OverlapStream(capacity, device)
    for z0 in range(0, shape[0], slab_depth):
        z1 = min(z0 + slab_depth, shape[0])
        blocks = []
        for source, what in ((source_a, "source_a"), (source_b, "source_b")):
            block = np.asarray(source[z0:z1])
            if block.dtype != np.int32 or block.shape != (z1 - z0,) + shape[1:]:
                raise TypeError(f"{fn}: {what}[{z0}:{z1}] gave {block.dtype} {block.shape}")
            blocks.append(block)
        stream.add(*blocks)
    return stream.finish()


def overlap_scores(pairs, counts, *, background="a"):
    """
    The scores of two labelings read off their overlap table, on the host
    (no GPU): the variation of information with its split and merge terms,
    the adapted Rand error with its precision and recall, the Rand index,
    the largest-overlap agreement and "the same partition up to names".

    background says which rows count. "a" drops the rows with a' = 0: the
    SNEMI3D / CREMI convention with a the ground truth, whose background is
    not scored; b's 0 is then an ordinary segment. "both_zero" drops only
    the row (0, 0). "none" drops nothing. Write n_ij for the counts of the
    kept rows, a_i and b_j for their marginals and N for their sum.

    Parameters
    ----------
    pairs : numpy.ndarray
        Integer (P, 2), rows (a', b'), each pair at most once.
    counts : numpy.ndarray
        Integer (P,), positive.
    background : {"a", "both_zero", "none"}

    Returns
    -------
    dict
        n : int, N.
        segments_a, segments_b, pairs : int, the numbers of distinct a', of
            distinct b' and of kept rows.
        voi_split : float, H(B|A) = H(A,B) - H(A) in bits (log2): float64,
            math.fsum over the rows sorted by (a', b').
        voi_merge : float, H(A|B), computed the same way.
        voi : float, voi_split + voi_merge.
        rand_precision : float, (sum n_ij^2 - N) / (sum b_j^2 - N).
        rand_recall : float, (sum n_ij^2 - N) / (sum a_i^2 - N).
        adapted_rand_error : float, 1 - 2 p r / (p + r).
        rand_index : float, the fraction of voxel pairs on which the two
            labelings agree (together in both or apart in both):
            1 - (sum a_i^2 + sum b_j^2 - 2 sum n_ij^2) / (N (N - 1)).
        largest_overlap_agreement : float, whatever "background" says: the
            sum over a' >= 1 of the largest count of a row (a', b'), b' = 0
            included, divided by (the table's total - the count of (0, 0)).
        same_partition : bool, true iff every a' occurs in exactly one kept
            row and every b' in exactly one: the kept table is a bijection
            between the labels.
    The Rand quantities are exact: Python integers and fractions.Fraction
    until the final float(). Where a denominator is 0 (no voxel pair to
    judge: N < 2, or every segment a single voxel) precision, recall and the
    Rand index are 1.0, the error is 0.0 where p + r is 0 as well, and an
    empty agreement is 1.0; an empty table has voi 0.0 and same_partition
    True.

    What this is not: no claim of equality with skimage's, CREMI's or
    funlib's numbers beyond the formulas stated here; no matching by
    Hungarian assignment; no per-segment error lists.
    """
    import math
    from fractions import Fraction

    if background not in _BACKGROUND_MODES:
        raise ValueError(f"overlap_scores: background must be one of {_BACKGROUND_MODES}, got {background!r}")
    pairs, counts = np.asarray(pairs), np.asarray(counts)
    if pairs.dtype.kind not in "iu" or counts.dtype.kind not in "iu":
        raise TypeError(f"overlap_scores: pairs and counts must be integer arrays, got {pairs.dtype} and {counts.dtype}")
    if pairs.ndim != 2 or pairs.shape[1] != 2 or counts.shape != (pairs.shape[0],):
        raise ValueError(f"overlap_scores: pairs must be (P, 2) and counts (P,), got {pairs.shape} and {counts.shape}")
    rows = sorted(zip((int(v) for v in pairs[:, 0]), (int(v) for v in pairs[:, 1]), (int(v) for v in counts)))
    if any(c <= 0 for _, _, c in rows):
        raise ValueError("overlap_scores: counts must be positive")
    if any(rows[i][:2] == rows[i + 1][:2] for i in range(len(rows) - 1)):
        raise ValueError("overlap_scores: a pair occurs in more than one row")

    # the largest-overlap agreement looks at the whole table
    total = sum(c for _, _, c in rows)
    zero = sum(c for i, j, c in rows if i == 0 and j == 0)
    best = {}
    for i, j, c in rows:
        if i >= 1 and c > best.get(i, 0):
            best[i] = c
    agreement = float(Fraction(sum(best.values()), total - zero)) if total > zero else 1.0

    if background == "a":
        rows = [r for r in rows if r[0] != 0]
    elif background == "both_zero":
        rows = [r for r in rows if r[0] != 0 or r[1] != 0]
    n = sum(c for _, _, c in rows)
    a_sizes, b_sizes, a_rows, b_rows = {}, {}, {}, {}
    for i, j, c in rows:
        a_sizes[i] = a_sizes.get(i, 0) + c
        b_sizes[j] = b_sizes.get(j, 0) + c
        a_rows[i] = a_rows.get(i, 0) + 1
        b_rows[j] = b_rows.get(j, 0) + 1

    # H(B|A) = -sum n_ij / N log2(n_ij / a_i), one term per row, each >= 0
    split = math.fsum(c / n * (math.log2(a_sizes[i]) - math.log2(c)) for i, j, c in rows) if n else 0.0
    merge = math.fsum(c / n * (math.log2(b_sizes[j]) - math.log2(c)) for i, j, c in rows) if n else 0.0

    sum_ij = sum(c * c for _, _, c in rows)
    sum_a = sum(c * c for c in a_sizes.values())
    sum_b = sum(c * c for c in b_sizes.values())
    precision = Fraction(sum_ij - n, sum_b - n) if sum_b > n else Fraction(1)
    recall = Fraction(sum_ij - n, sum_a - n) if sum_a > n else Fraction(1)
    error = 1 - 2 * precision * recall / (precision + recall) if precision + recall > 0 else Fraction(0)
    rand = 1 - Fraction(sum_a + sum_b - 2 * sum_ij, n * (n - 1)) if n > 1 else Fraction(1)
    return {
        "n": n,
        "segments_a": len(a_sizes),
        "segments_b": len(b_sizes),
        "pairs": len(rows),
        "voi_split": split,
        "voi_merge": merge,
        "voi": split + merge,
        "rand_precision": float(precision),
        "rand_recall": float(recall),
        "adapted_rand_error": float(error),
        "rand_index": float(rand),
        "largest_overlap_agreement": agreement,
        "same_partition": all(v == 1 for v in a_rows.values()) and all(v == 1 for v in b_rows.values()),
    }


def compare_segmentations(a, b, *, background="a", pair_capacity=None):
    """
    overlap_scores of label_overlaps(a, b): the table on the device, the
    scores on the host. a is the ground truth where there is one
    (background="a" leaves its background out, the SNEMI3D / CREMI
    convention). See overlap_scores for the fields and for what this is not.
    """
    if background not in _BACKGROUND_MODES:
        raise ValueError(f"compare_segmentations: background must be one of {_BACKGROUND_MODES}, got {background!r}")
    pairs, counts = label_overlaps(a, b, pair_capacity=pair_capacity)
    return overlap_scores(pairs, counts, background=background)
