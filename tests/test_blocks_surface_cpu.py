"""
The surface of label_pieces_open, skeletonize_blocks and join_block_skeletons without a GPU, in the manner of
test_pieces_surface_cpu.py: the new names are the same objects under inference, their signatures, the signatures
that stay, the C symbols are exported, declared and bound with the right number of arguments, the ABI version stays,
the header and the docstrings say what the definition is and is not, the C call and the workspace query refuse on
the host (an open_faces of 64 among the refusals), and the argument checks that need no device.
"""

import inspect
import os
import re

import numpy as np
import pytest

from aind_exaspim_neuron_segmentation_amd import _native, inference, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exaspim_label_pieces_open_workspace_bytes", "exaspim_label_pieces_open"]
NAMES = ["label_pieces_open", "skeletonize_blocks", "join_block_skeletons", "_label_pieces_open_on_device"]


def header():
    return open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()


@pytest.mark.parametrize("name", NAMES)
def test_name_is_the_same_object_under_inference(name):
    assert getattr(inference, name) is getattr(segmentation, name)
    assert getattr(segmentation, name).__module__.endswith(".segmentation")


def test_the_signatures():
    keyword, empty = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty

    def check(fn, positional, keywords, defaults=()):
        parameters = inspect.signature(fn).parameters
        assert list(parameters) == positional + list(defaults) + list(keywords)
        for name in positional:
            assert parameters[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
            assert parameters[name].default is empty
        for name, default in dict(defaults).items():
            assert parameters[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
            assert parameters[name].default == default, name
        for name, default in keywords.items():
            assert parameters[name].kind is keyword, name
            assert parameters[name].default is default or parameters[name].default == default, name

    check(segmentation.label_pieces_open, ["labels", "open_faces"],
          dict(n_labels=None, dust_threshold=0, return_device_tensors=False))
    check(segmentation.skeletonize_blocks, ["segmentation"],
          dict(dust_threshold=1000, fix_branching=True, scale=1.25, const=450.0, pdrf_exponent=4, pdrf_scale=100000.0,
               fill_holes=True, max_paths=None, device=None, stats=None), dict(block_shape=(512, 512, 512)))
    check(segmentation.join_block_skeletons, ["trees"], {}, dict(dust_threshold=0, stats=None))


def test_the_older_signatures_stay():
    assert list(inspect.signature(segmentation.label_pieces).parameters) == [
        "labels", "n_labels", "dust_threshold", "return_device_tensors"]
    assert list(inspect.signature(segmentation._label_pieces_on_device).parameters) == [
        "labels", "n_labels", "dust_threshold"]
    assert list(inspect.signature(segmentation.skeletonize_pieces).parameters) == [
        "segmentation", "dust_threshold", "fix_borders", "fix_branching", "scale", "const", "pdrf_exponent",
        "pdrf_scale", "fill_holes", "max_paths"]
    assert list(inspect.signature(segmentation.segmentation_to_zipped_swcs).parameters) == ["segmentation", "zip_path"]
    assert list(inspect.signature(segmentation._skeleton_chain_on_device).parameters) == [
        "labels", "scale", "const", "pdrf_exponent", "pdrf_scale", "fill_holes", "max_paths", "fix_branching", "stats",
        "fix_borders"]


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
    text = header().replace("\n * ", "\n")      # a phrase may run over the end of a comment line
    section = " ".join(text[text.index("pieces with open faces: the pieces of one block"):].split())
    for phrase in ("DESIGN 6r", "Bit f of open_faces names face f",
                   "z = 0, z = D - 1, y = 0, y = H - 1, x = 0, x = W - 1",
                   "open iff at least one of its voxels lies on a face whose bit is set",
                   "either bit opens the plane", "kept iff it is open or size >= dust_threshold",
                   "ascending order of first voxel", "byte for byte", "state_dev[2] is 0", "pure function",
                   "What this is not", "not claimed", "a bit above bit 5", "no output is touched",
                   "state_dev[2] = the number of pieces kept although below the threshold",
                   "nothing allocated, nothing synchronised"):
        assert phrase in section, phrase


def test_the_docstrings_say_what_this_is_and_is_not():
    for name in ("label_pieces_open", "skeletonize_blocks", "join_block_skeletons"):
        doc = " ".join(getattr(segmentation, name).__doc__.split())
        for phrase in ("What this is", "What this is not", "not claimed", "kimimaro"):
            assert phrase in doc, (name, phrase)
    doc = " ".join(segmentation.skeletonize_blocks.__doc__.split())
    for phrase in ("inference.py:240-291", "share exactly one plane", "a cavity that a cut opens is not filled",
                   "owned by exactly one block", "DESIGN 6r", "only segmentation[z0:z1, y0:y1, x0:x1] is ever read",
                   "may exceed 2^31 - 1", "igneous", "array for array", "skipped joint"):
        assert phrase in doc, phrase
    doc = " ".join(segmentation.join_block_skeletons.__doc__.split())
    for phrase in ("the smaller of the two", "upper bound", "cannot hold the ring", "ascending (block, piece)",
                   "order of the list does not matter"):
        assert phrase in doc, phrase


def test_the_workspace_query_refuses_on_the_host():
    lib = _native.lib()
    for dims in ((3, 4, 5), (1, 1, 1), (512, 512, 512), (2, 513, 513)):
        assert lib.exaspim_label_pieces_open_workspace_bytes(_native.int3(dims)) == \
            lib.exaspim_label_pieces_workspace_bytes(_native.int3(dims)) > 0
    assert lib.exaspim_label_pieces_open_workspace_bytes(_native.int3((3, 4, 5))) == 256 + 256
    for dims in ((3, 0, 5), (3, -4, 5), (2048, 1024, 1024)):
        assert lib.exaspim_label_pieces_open_workspace_bytes(_native.int3(dims)) == 0, dims
        assert "dims" in _native.last_error() and _native.last_error().startswith("label_pieces_open_workspace_bytes")


def test_the_call_refuses_on_the_host_before_any_device_is_touched():
    """Every refusal is decided from the arguments' values alone: the pointers are never followed."""
    lib = _native.lib()
    dims = _native.int3((3, 4, 5))
    good = [0x1000, dims, 2, 0, 63, 0x2000, 0x3000, 0x4000, 512, None]
    for at, value in ((0, None), (5, None), (6, None), (7, None), (1, _native.int3((0, 4, 5))), (2, -1), (3, -1),
                      (4, 64), (4, 65), (4, 1 << 31), (4, 2**32 - 1), (0, 0x1002), (5, 0x2001), (6, 0x3002),
                      (7, 0x4008), (5, 0x1000)):
        args = list(good)
        args[at] = value
        assert lib.exaspim_label_pieces_open(*args) == -1, (at, value)
        assert _native.last_error().startswith("label_pieces_open:"), _native.last_error()
        if at == 4:
            assert "open_faces" in _native.last_error()
    args = list(good)
    args[8] = 511
    assert lib.exaspim_label_pieces_open(*args) == -3


def test_argument_checks_that_need_no_device():
    labels = np.zeros((3, 4, 5), dtype=np.int32)
    closed = [False] * 6
    for bad in (None, 3, "101010", 0b101010):
        with pytest.raises(TypeError, match="open_faces must be a sequence of six bools"):
            segmentation.label_pieces_open(labels, bad)
    for bad in ([1, 0, 0, 0, 0, 0], [None] * 6, [np.int32(1)] * 6):
        with pytest.raises(TypeError, match="open_faces must be a sequence of six bools"):
            segmentation.label_pieces_open(labels, bad)
    for bad in ([], [True] * 5, [False] * 7):
        with pytest.raises(ValueError, match="open_faces must have six entries"):
            segmentation.label_pieces_open(labels, bad)
    assert segmentation._checked_open_faces("f", (True, False, np.bool_(True), False, False, True)) == 0b100101
    for bad in (1.5, "3", True, None):
        with pytest.raises(TypeError, match="dust_threshold must be an integer"):
            segmentation.label_pieces_open(labels, closed, dust_threshold=bad)
        with pytest.raises(TypeError, match="dust_threshold must be an integer"):
            segmentation.skeletonize_blocks(labels, dust_threshold=bad)
    with pytest.raises(ValueError, match="dust_threshold must not be negative"):
        segmentation.label_pieces_open(labels, closed, dust_threshold=-1)
    with pytest.raises(ValueError, match="n_labels must not be negative"):
        segmentation.label_pieces_open(labels, closed, n_labels=-1)
    with pytest.raises(TypeError, match="int32"):
        segmentation.label_pieces_open(labels.astype(np.int64), closed)
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        segmentation.label_pieces_open(labels[0], closed)

    blocks = segmentation.skeletonize_blocks
    for bad in (labels.astype(np.int64), labels.astype(np.uint32), labels.astype(np.float32)):
        with pytest.raises(TypeError, match="int32"):
            blocks(bad)
    for bad in ([[[1]]], None, 5):
        with pytest.raises(TypeError, match="shape, dtype"):
            blocks(bad)
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        blocks(labels[0])
    with pytest.raises(ValueError, match="empty volume"):
        blocks(labels[:, :0])
    for bad in ((4, 4), 4, "444", (4, 4, 4, 4)):
        with pytest.raises(ValueError, match="block_shape must be three integers"):
            blocks(labels, bad)
    with pytest.raises(TypeError, match="block_shape must be an integer"):
        blocks(labels, (4, 4.0, 4))
    with pytest.raises(ValueError, match="block_shape must be at least 2"):
        blocks(labels, (4, 1, 4))
    with pytest.raises(ValueError, match="more than 2\\^31 - 1 voxels"):
        blocks(np.lib.stride_tricks.as_strided(labels, (2048, 1024, 1024), (0, 0, 0)), (2048, 1024, 1024))
    with pytest.raises(TypeError, match="fix_branching must be a bool"):
        blocks(labels, fix_branching=1)
    with pytest.raises(ValueError, match="max_paths"):
        blocks(labels, max_paths=0)
    with pytest.raises(TypeError, match="stats must be a dict"):
        blocks(labels, stats=[])
    with pytest.raises(RuntimeError, match="no CPU path"):
        blocks(labels, device="cpu")
