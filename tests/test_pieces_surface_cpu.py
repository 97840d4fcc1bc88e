"""
The surface of label_pieces and skeletonize_pieces without a GPU, in the manner of test_border_surface_cpu.py: the
new names are the same objects under inference, their signatures, the signatures that stay, the C symbols are
exported, declared and bound with the right number of arguments, the ABI version stays, the header and the
docstrings say what the definition is and is not, the workspace query refuses on the host, and the argument checks
that need no device.
"""

import inspect
import os
import re

import numpy as np
import pytest

from aind_exaspim_neuron_segmentation_amd import _native, inference, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exaspim_label_pieces_workspace_bytes", "exaspim_label_pieces"]
NAMES = ["label_pieces", "skeletonize_pieces", "_label_pieces_on_device"]


def header():
    return open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()


@pytest.mark.parametrize("name", NAMES)
def test_name_is_the_same_object_under_inference(name):
    assert getattr(inference, name) is getattr(segmentation, name)
    assert getattr(segmentation, name).__module__.endswith(".segmentation")


def test_the_signatures():
    keyword, empty = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty

    def check(fn, positional, keywords):
        parameters = inspect.signature(fn).parameters
        assert list(parameters) == positional + list(keywords)
        for name in positional:
            assert parameters[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
            assert parameters[name].default is empty
        for name, default in keywords.items():
            assert parameters[name].kind is keyword, name
            assert parameters[name].default is default or parameters[name].default == default, name

    check(segmentation.label_pieces, ["labels"], dict(n_labels=None, dust_threshold=0, return_device_tensors=False))
    check(segmentation.skeletonize_pieces, ["segmentation"],
          dict(dust_threshold=1000, fix_borders=True, fix_branching=True, scale=1.25, const=450.0, pdrf_exponent=4,
               pdrf_scale=100000.0, fill_holes=True, max_paths=None))


def test_the_older_signatures_stay():
    assert list(inspect.signature(segmentation.skeletonize).parameters) == [
        "segmentation", "fix_branching", "scale", "const", "pdrf_exponent", "pdrf_scale", "fill_holes", "max_paths"]
    assert list(inspect.signature(segmentation.skeletonize_fix_borders).parameters) == [
        "segmentation", "fix_borders", "fix_branching", "scale", "const", "pdrf_exponent", "pdrf_scale", "fill_holes",
        "max_paths"]
    assert list(inspect.signature(segmentation.skeletonize_labels).parameters) == [
        "labels", "scale", "const", "pdrf_exponent", "pdrf_scale", "fill_holes", "max_paths"]
    assert list(inspect.signature(segmentation.segmentation_to_zipped_swcs).parameters) == ["segmentation", "zip_path"]
    assert list(inspect.signature(segmentation._skeleton_chain_on_device).parameters) == [
        "labels", "scale", "const", "pdrf_exponent", "pdrf_scale", "fill_holes", "max_paths", "fix_branching", "stats",
        "fix_borders"]
    assert list(inspect.signature(segmentation.segment_table).parameters) == [
        "labels", "dbf", "n_labels", "return_device_tensors"]


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_and_bound(name):
    text = header()
    assert re.search(r"^(size_t|int) " + name + r"\(", text, re.M), name
    assert name in _native.SIGNATURES
    restype, argtypes = _native.SIGNATURES[name]
    declaration = re.search(r"^(?:size_t|int) " + name + r"\((.*?)\);", text, re.M | re.S).group(1)
    declaration = re.sub(r"/\*.*?\*/", "", declaration, flags=re.S)
    assert len(argtypes) == len(declaration.split(",")), (name, declaration)
    assert restype is (_native._sz if name.endswith("_bytes") else _native._i32)
    assert getattr(_native.lib(), name) is not None


def test_the_abi_version_stays():
    assert int(re.search(r"#define\s+EXASPIM_ABI_VERSION\s+(\d+)", header()).group(1)) == 5
    assert _native.lib().exaspim_abi_version() == 5


def test_the_header_states_the_definition():
    text = header()
    section = " ".join(text[text.index("pieces: the 26-connected components of every label"):].split())
    for phrase in ("inference.py:272-290", "not claimed", "maximal 26-connected", "in 1..K", "size >= dust_threshold",
                   "0 and 1 keep everything", "ascending order of first voxel", "smallest linear index",
                   "pure function", "exaspim_dbf of the pieces", "restricted to kept pieces",
                   "must not be labels_dev", "nothing allocated, nothing synchronised", "no output is touched",
                   "state_dev[1] = the number of dust pieces"):
        assert phrase in section, phrase


@pytest.mark.parametrize("name", ["label_pieces", "skeletonize_pieces"])
def test_the_docstrings_say_not_kimimaro(name):
    doc = " ".join(getattr(segmentation, name).__doc__.split())
    for phrase in ("inference.py:272-290", "What this is not", "kimimaro", "not claimed", "26-connected"):
        assert phrase in doc, phrase
    if name == "skeletonize_pieces":
        assert "max_paths counts per piece" in doc and "forest" in doc
    for older in ("skeletonize", "skeletonize_labels", "skeletonize_fix_borders"):
        assert "skeletonize_pieces" in getattr(segmentation, older).__doc__      # each points to the form that has it


def test_the_workspace_query_refuses_on_the_host():
    lib = _native.lib()
    assert lib.exaspim_label_pieces_workspace_bytes(_native.int3((3, 4, 5))) == 256 + 256
    assert lib.exaspim_label_pieces_workspace_bytes(_native.int3((1, 1, 1))) == 256 + 256
    assert lib.exaspim_label_pieces_workspace_bytes(_native.int3((512, 512, 512))) == 4 * 2**27 + 4 * 2**16
    for dims in ((3, 0, 5), (3, -4, 5), (2048, 1024, 1024)):
        assert lib.exaspim_label_pieces_workspace_bytes(_native.int3(dims)) == 0, dims
        assert "dims" in _native.last_error()


def test_the_call_refuses_on_the_host_before_any_device_is_touched():
    """Every refusal is decided from the arguments' values alone: the pointers are never followed."""
    lib = _native.lib()
    dims = _native.int3((3, 4, 5))
    good = [0x1000, dims, 2, 0, 0x2000, 0x3000, 0x4000, 512, None]
    for at, value in ((0, None), (4, None), (5, None), (6, None), (1, _native.int3((0, 4, 5))), (2, -1), (3, -1),
                      (0, 0x1002), (4, 0x2001), (5, 0x3002), (6, 0x4008), (4, 0x1000)):
        args = list(good)
        args[at] = value
        assert lib.exaspim_label_pieces(*args) == -1, (at, value)
        assert _native.last_error().startswith("label_pieces:"), _native.last_error()
    args = list(good)
    args[7] = 511
    assert lib.exaspim_label_pieces(*args) == -3


def test_argument_checks_that_need_no_device():
    labels = np.zeros((3, 4, 5), dtype=np.int32)
    for fn in (segmentation.label_pieces, segmentation.skeletonize_pieces):
        for bad in (1.5, "3", True, None):
            with pytest.raises(TypeError, match="dust_threshold must be an integer"):
                fn(labels, dust_threshold=bad)
        with pytest.raises(ValueError, match="dust_threshold must not be negative"):
            fn(labels, dust_threshold=-1)
        with pytest.raises(TypeError, match="int32"):
            fn(labels.astype(np.int64))
        with pytest.raises(ValueError, match=r"\(D, H, W\)"):
            fn(labels[0])
        with pytest.raises(ValueError, match="empty volume"):
            fn(labels[:, :0])
        with pytest.raises(TypeError, match="torch tensor or a numpy array"):
            fn([[[1]]])
    for bad in (1.5, "3", True):
        with pytest.raises(TypeError, match="n_labels must be an integer"):
            segmentation.label_pieces(labels, n_labels=bad)
    with pytest.raises(ValueError, match="n_labels must not be negative"):
        segmentation.label_pieces(labels, n_labels=-1)
    for bad in (1, None, "yes", np.int32(1)):
        with pytest.raises(TypeError, match="fix_borders must be a bool"):
            segmentation.skeletonize_pieces(labels, fix_borders=bad)
    with pytest.raises(TypeError, match="fix_branching must be a bool"):
        segmentation.skeletonize_pieces(labels, fix_branching=1)
    with pytest.raises(ValueError, match="max_paths"):
        segmentation.skeletonize_pieces(labels, max_paths=0)
