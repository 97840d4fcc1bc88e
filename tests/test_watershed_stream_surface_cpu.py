"""
The surface of the streamed watershed fragments without a GPU, in the manner of test_blocks_surface_cpu.py: the new
names are the same objects under inference, their signatures and defaults, the keywords the streamed agglomerations
gained (at the end of their lists, with agglomerate_affinities' names, defaults, checks and messages), the
signatures that stay, the C symbols are exported, declared and bound, the descriptor's layout, the ABI version
stays, the header says what the definition is and what it costs, and every refusal that needs no device: the C
call's and the workspace query's on the host, and the argument checks of the Python layer.
"""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd import _native, inference, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exaspim_watershed_stream_slab_workspace_bytes", "exaspim_watershed_stream_slab"]
NAMES = ["WatershedStream", "watershed_fragments_streaming", "ComponentsStream", "RegionGraphStream",
         "agglomerate_affinities_streaming"]
MERGING = dict(fragments="components", aff_threshold_low=0.1, aff_threshold_high=0.9999, premerge_size=0,
               premerge_rounds=4, device_merge_rounds=0)


def header():
    return open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()


@pytest.mark.parametrize("name", NAMES)
def test_name_is_the_same_object_under_inference(name):
    assert getattr(inference, name) is getattr(segmentation, name)
    assert getattr(segmentation, name).__module__.endswith(".segmentation")


def keyword_only(fn):
    return {n: p.default for n, p in inspect.signature(fn).parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}


def positional(fn):
    return [(n, p.default) for n, p in inspect.signature(fn).parameters.items()
            if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and n != "self"]


def test_the_signatures():
    empty = inspect.Parameter.empty
    assert positional(segmentation.WatershedStream.__init__) == [
        ("shape", empty), ("aff_threshold_low", 0.1), ("aff_threshold_high", 0.9999), ("min_segment_size", 0)]
    assert keyword_only(segmentation.WatershedStream.__init__) == dict(device=None, id_capacity=None)
    assert positional(segmentation.watershed_fragments_streaming) == [
        ("source", empty), ("aff_threshold_low", 0.1), ("aff_threshold_high", 0.9999), ("min_segment_size", 0)]
    assert keyword_only(segmentation.watershed_fragments_streaming) == dict(
        slab_depth=empty, write_block=None, id_capacity=None, device=None, keep_labels_resident=None)
    # thresholds and the size default are those of the whole-volume function
    whole = inspect.signature(segmentation.watershed_fragments).parameters
    for name in ("aff_threshold_low", "aff_threshold_high", "min_segment_size"):
        assert whole[name].default == inspect.signature(segmentation.watershed_fragments_streaming).parameters[name].default


def test_the_stream_class_shares_the_components_streams_code():
    ws, cs = segmentation.WatershedStream, segmentation.ComponentsStream
    assert issubclass(ws, cs)
    for name in ("push", "finish", "apply", "next_z", "_scratch", "_allocate"):
        assert getattr(ws, name) is getattr(cs, name), name
    assert ws._slab_call == "exaspim_watershed_stream_slab" and cs._slab_call == "exaspim_components_stream_slab"
    assert list(inspect.signature(cs.__init__).parameters) == [
        "self", "shape", "threshold", "min_segment_size", "foreground", "device", "id_capacity"]


@pytest.mark.parametrize("fn", [segmentation.agglomerate_affinities_streaming, inference.predict_agglomerate_streaming])
def test_the_streamed_agglomerations_gained_keywords_at_the_end(fn):
    keywords = keyword_only(fn)
    assert list(keywords)[-len(MERGING):] == list(MERGING)
    whole = inspect.signature(segmentation.agglomerate_affinities).parameters
    for name, default in MERGING.items():
        assert keywords[name] == default == whole[name].default, name
    before = list(keywords)[:-len(MERGING)]
    if fn is segmentation.agglomerate_affinities_streaming:
        assert before == ["fragment_threshold", "slab_depth", "write_block", "id_capacity", "edge_capacity", "device",
                          "keep_labels_resident"]
        assert [n for n, _ in positional(fn)] == ["source", "agglomeration_thresholds", "min_segment_size"]
    else:
        assert before == ["fragment_threshold", "affinity_mode", "shape", "dtype", "write_block", "keep_input_resident",
                          "n_streams", "copy_threads", "timings", "id_capacity", "edge_capacity", "keep_labels_resident"]


def test_the_region_graph_stream_has_a_finish_that_stays_on_the_device():
    rgs = segmentation.RegionGraphStream
    assert list(inspect.signature(rgs.finish).parameters) == ["self", "table", "n_labels"]
    assert list(inspect.signature(rgs.finish_on_device).parameters) == ["self", "table", "n_labels"]
    assert list(inspect.signature(segmentation._agglomerate_streams).parameters) == [
        "cs", "rgs", "thresholds", "min_segment_size", "premerge_size", "premerge_rounds", "device_merge_rounds"]


def test_the_name_of_the_reference_stays_unused():
    assert not hasattr(inference, "affinities_to_segmentation") and not hasattr(segmentation, "affinities_to_segmentation")


# ---- the C ABI -----------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound():
    lib = _native.lib()
    text = header()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None
        assert len(re.findall(r"^(?:int|size_t) " + name + r"\(", text, re.M)) == 1, name
        assert name in _native.SIGNATURES
    declared = re.search(r"int exaspim_watershed_stream_slab\((.*?)\);", text, re.S).group(1)
    assert len(declared.split(",")) == len(_native.SIGNATURES["exaspim_watershed_stream_slab"][1]) == 9
    assert lib.exaspim_abi_version() == 5 and "#define EXASPIM_ABI_VERSION 5" in text
    assert re.search(r"later within 5: exaspim_watershed_stream_slab", text)


def test_the_descriptor_is_the_components_streams_plus_three_fields():
    d, base = _native.WatershedStreamDesc, _native.ComponentsStreamDesc
    assert [f[0] for f in d._fields_] == ["base", "low", "high", "seam_aff_dev"]
    assert d.base.offset == 0 and d.base.size == ctypes.sizeof(base)
    assert d.low.offset == ctypes.sizeof(base) and d.high.offset == d.low.offset + 4
    assert d.seam_aff_dev.offset == d.low.offset + 8 and ctypes.sizeof(d) == ctypes.sizeof(base) + 16
    struct = re.search(r"typedef struct exaspim_watershed_stream \{(.*?)\} exaspim_watershed_stream;", header(), re.S)
    fields = re.findall(r"^\s*(\S[^;]*?)\s*(\w+);", struct.group(1), re.M)
    assert [name for _, name in fields] == ["base", "low", "high", "seam_aff_dev"]
    assert [kind for kind, _ in fields] == ["exaspim_components_stream", "float", "float", "float*"]


def test_the_header_states_the_definition_and_the_cost():
    text = " ".join(" ".join(re.sub(r"^\s*\*", "", line) for line in header().splitlines()).split())
    for phrase in ("exaspim_watershed_fragments gives on the whole volume", "No plane of the next slab is needed",
                   "bit 0 eligible, bit 1 sure", "the price is ids", "base.threshold is ignored",
                   "never read before they are written"):
        assert phrase in text, phrase
    doc = " ".join(segmentation.WatershedStream.__doc__.split())
    assert "costs ids, never labels" in doc and "ELIGIBLE" in doc


def good_descriptor():
    """A descriptor that passes every check of the host, pointing at nothing real: the refusals come before any
    launch, so the pointers are never followed."""
    d = _native.WatershedStreamDesc()
    b = d.base
    b.dims[:] = (9, 9, 33)
    b.channels, b.threshold, b.capacity, b.min_size, b.next_z = 3, 0.5, 100, 0, 0
    for i, name in enumerate(("id_parent_dev", "id_count_dev", "table_dev", "state_dev", "seam_ids_dev", "seam_bits_dev")):
        setattr(b, name, 0x10000 * (i + 1))
    d.low, d.high, d.seam_aff_dev = 0.1, 0.9999, 0x80000
    return d


def slab_call(d, aff=0x100000, dtype=_native.AFF_F32, dims=(4, 9, 33), z0=0, labels=0x200000, ws=0x300000, need=1 << 30):
    return _native.lib().exaspim_watershed_stream_slab(ctypes.byref(d) if d is not None else None, aff, dtype,
                                                       _native.int3(dims), z0, labels, ws, need, None)


REFUSALS = [
    ("channels must be 3", lambda d: setattr(d.base, "channels", 1), {}),
    ("channels must be 3", lambda d: setattr(d.base, "channels", 4), {}),
    ("seam_aff_dev", lambda d: setattr(d, "seam_aff_dev", None), {}),
    ("seam_aff_dev", lambda d: setattr(d, "seam_aff_dev", 0x80002), {}),
    ("NaN", lambda d: setattr(d, "low", float("nan")), {}),
    ("NaN", lambda d: setattr(d, "high", float("nan")), {}),
    ("dims must be positive", lambda d: d.base.dims.__setitem__(0, 0), {}),
    ("capacity must be", lambda d: setattr(d.base, "capacity", 2**31 - 1), {}),
    ("NULL device buffer", lambda d: setattr(d.base, "table_dev", None), {}),
    ("misaligned device buffer", lambda d: setattr(d.base, "id_count_dev", 0x20004), {}),
    ("next_z outside", lambda d: setattr(d.base, "next_z", -1), {}),
    ("NULL argument", None, dict(aff=None)),
    ("NULL argument", None, dict(labels=None)),
    ("NULL argument", None, dict(ws=None)),
    ("aff_dtype", None, dict(dtype=5)),
    ("slab dims must be positive", None, dict(dims=(0, 9, 33))),
    ("(y, x)", None, dict(dims=(4, 9, 32))),
    ("z order", None, dict(z0=1)),
    ("leave the volume", None, dict(dims=(10, 9, 33))),
    ("misaligned buffer", None, dict(ws=0x300008)),
    ("misaligned buffer", None, dict(labels=0x200002)),
    ("misaligned buffer", None, dict(aff=0x100002)),
    ("misaligned buffer", None, dict(aff=0x100001, dtype=_native.AFF_F16)),
]


@pytest.mark.parametrize("message,spoil,call", REFUSALS, ids=[f"{i}-{r[0]}" for i, r in enumerate(REFUSALS)])
def test_the_c_call_refuses_on_the_host_with_the_descriptor_unchanged(message, spoil, call):
    d = good_descriptor()
    if spoil:
        spoil(d)
    before = bytes(d)
    assert slab_call(d, **call) == -1
    assert message in _native.last_error() and _native.last_error().startswith("watershed_stream_slab: ")
    assert bytes(d) == before


def test_a_null_descriptor_and_a_short_workspace():
    assert slab_call(None) == -1 and "NULL stream descriptor" in _native.last_error()
    lib = _native.lib()
    need = lib.exaspim_watershed_stream_slab_workspace_bytes(_native.int3((4, 9, 33)))
    assert need == lib.exaspim_components_stream_slab_workspace_bytes(_native.int3((4, 9, 33))) > 5 * 4 * 9 * 33
    d = good_descriptor()
    before = bytes(d)
    assert slab_call(d, need=need - 1) == -3 and "workspace" in _native.last_error()
    assert bytes(d) == before
    for dims in ((0, 9, 33), (4, -1, 33), (65536, 65536, 1)):
        assert lib.exaspim_watershed_stream_slab_workspace_bytes(_native.int3(dims)) == 0
        assert "watershed_stream_slab_workspace_bytes" in _native.last_error()


# ---- the Python layer ----------------------------------------------------------------------------------------
def test_the_stream_class_refuses_without_a_device():
    ws = segmentation.WatershedStream
    with pytest.raises(ValueError, match="NaN"):
        ws((4, 4, 4), float("nan"), 0.9)
    with pytest.raises(ValueError, match="NaN"):
        ws((4, 4, 4), 0.1, float("nan"))
    with pytest.raises(ValueError, match="non-empty"):
        ws((4, 4), 0.1, 0.9)
    with pytest.raises(ValueError, match="non-empty"):
        ws((4, 0, 4), 0.1, 0.9)
    with pytest.raises(ValueError, match="exceeds 2\\^31 - 1"):
        ws((2, 65536, 65536))
    with pytest.raises(RuntimeError, match="WatershedStream \\(MI355X\\) has no CPU path"):
        ws((4, 4, 4), device="cpu")
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="id_capacity must be"):
            ws((4, 4, 4), id_capacity=0)


def test_the_host_function_refuses_without_a_device():
    fn = segmentation.watershed_fragments_streaming
    aff = np.zeros((3, 4, 5, 6), np.float32)
    with pytest.raises(TypeError, match="float32 or float16"):
        fn(aff.astype(np.float64), slab_depth=2)
    with pytest.raises(ValueError, match=r"needs \(3, D, H, W\) affinities"):
        fn(aff[0], slab_depth=2)
    with pytest.raises(ValueError, match=r"needs \(3, D, H, W\) affinities"):
        fn(aff[:2], slab_depth=2)
    with pytest.raises(ValueError, match="slab_depth must be positive"):
        fn(aff, slab_depth=0)
    with pytest.raises(ValueError, match="NaN"):
        fn(aff, float("nan"), slab_depth=2)
    with pytest.raises(TypeError):
        fn(aff)      # slab_depth has no default
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(aff, slab_depth=2)


BAD_OPTIONS = [
    (dict(fragments="basins"), 'fragments must be "components" or "watershed"'),
    (dict(premerge_size=-1), "the size floor must be at least 0"),
    (dict(premerge_size=1.5), "the size floor must be an integer"),
    (dict(premerge_size=True), "the size floor must be an integer"),
    (dict(premerge_rounds=0), "the number of rounds must be at least 1"),
    (dict(device_merge_rounds=-1), "device_merge_rounds"),
    (dict(device_merge_rounds=2.0), "device_merge_rounds"),
    (dict(fragments="watershed", aff_threshold_low=float("nan")), "must not be NaN"),
    (dict(fragments="watershed", aff_threshold_high=float("nan")), "must not be NaN"),
]


@pytest.mark.parametrize("options,message", BAD_OPTIONS, ids=[str(i) for i in range(len(BAD_OPTIONS))])
def test_the_streamed_agglomerations_check_as_agglomerate_affinities_does(options, message):
    aff = np.zeros((3, 4, 5, 6), np.float32)
    raised = []
    for call in (lambda: segmentation.agglomerate_affinities(aff, **options),
                 lambda: segmentation.agglomerate_affinities_streaming(aff, slab_depth=2, **options),
                 lambda: inference.predict_agglomerate_streaming(aff, None, **options)):
        try:
            call()
        except ValueError as e:
            raised.append(str(e))
        except RuntimeError:      # the whole-volume call looks at a NaN only after the upload, which needs a device
            assert "NaN" in message
            raised.append(None)
    assert len(raised) == 3 and all(r is None or message in r for r in raised), raised
    assert raised[1] is not None and raised[1] == raised[2]
    if raised[0] is not None:
        assert raised[0] == raised[1]
