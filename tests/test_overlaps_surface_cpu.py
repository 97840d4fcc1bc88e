"""
The surface of label_overlaps, OverlapStream, label_overlaps_streaming, compare_segmentations and overlap_scores
without a GPU, in the manner of test_blocks_surface_cpu.py: the new names are the same objects under inference,
their signatures, the five C symbols are exported, declared and bound with the right number of arguments, the ABI
version stays, the header says what the definition is and is not, the workspace query's values and refusals,
every host-side refusal of the four calls with pointers that are never followed, and the argument checks that
need no device.
"""

import inspect
import os
import re

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd import _native, inference, segmentation
from aind_exaspim_neuron_segmentation_amd.inference import (  # noqa: F401  (the surface this file is about)
    OverlapStream, compare_segmentations, label_overlaps, label_overlaps_streaming, overlap_scores,
)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exaspim_label_overlaps_workspace_bytes", "exaspim_label_overlaps_reset", "exaspim_label_overlaps_add",
           "exaspim_label_overlaps_finish", "exaspim_label_overlaps"]
NAMES = ["label_overlaps", "OverlapStream", "label_overlaps_streaming", "compare_segmentations", "overlap_scores",
         "DEFAULT_PAIR_CAPACITY"]


def header():
    return open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()


@pytest.mark.parametrize("name", NAMES)
def test_name_is_the_same_object_under_inference(name):
    assert getattr(inference, name) is getattr(segmentation, name)
    if name != "DEFAULT_PAIR_CAPACITY":
        assert getattr(segmentation, name).__module__.endswith(".segmentation")


def test_the_signatures():
    keyword, empty = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty

    def check(fn, positional, keywords, defaults=()):
        parameters = inspect.signature(fn).parameters
        assert list(parameters) == positional + list(dict(defaults)) + list(keywords)
        for name in positional:
            assert parameters[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
            assert parameters[name].default is empty
        for name, default in dict(defaults).items():
            assert parameters[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
            assert parameters[name].default == default, name
        for name, default in keywords.items():
            assert parameters[name].kind is keyword, name
            assert parameters[name].default is default or parameters[name].default == default, name

    check(segmentation.label_overlaps, ["a", "b"], dict(pair_capacity=None, return_device_tensors=False))
    check(segmentation.OverlapStream, ["pair_capacity"], {}, dict(device=None))
    check(segmentation.OverlapStream.add, ["self", "a_block", "b_block"], {})
    assert list(inspect.signature(segmentation.OverlapStream.finish).parameters)[0] == "self"
    check(segmentation.label_overlaps_streaming, ["source_a", "source_b"],
          dict(slab_depth=empty, pair_capacity=None, device=None))
    check(segmentation.compare_segmentations, ["a", "b"], dict(background="a", pair_capacity=None))
    check(segmentation.overlap_scores, ["pairs", "counts"], dict(background="a"))
    assert segmentation.DEFAULT_PAIR_CAPACITY == 1 << 22
    assert [segmentation._default_pair_capacity(v) for v in (1, 2, 3, 1000, 1 << 21, (1 << 21) + 1, 512**3)] == \
        [2, 4, 8, 2048, 1 << 22, 1 << 22, 1 << 22]


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
    assert re.search(r"later within 5: exaspim_label_overlaps", header())


def test_the_header_states_the_definition():
    text = header().replace("\n * ", "\n")      # a phrase may run over the end of a comment line
    section = " ".join(text[text.index("the overlap table of two label volumes (DESIGN 6u"):].split())
    section = section[:section.index("synthetic input for benchmarks and tests")]
    for phrase in ("ordered pair", "everything <= 0 is background", "exact in integers",
                   "finish only reads the table", "nothing allocated, nothing synchronised", "What this is not",
                   "no claim of equality with skimage's, CREMI's or funlib's numbers beyond the formulas stated",
                   "no matching by Hungarian assignment", "no per-segment error lists", "2^31 - 1 included",
                   "no label ever becomes an address", "the sum of all counts equals the number of voxels added",
                   "4-byte alignment only", "UNSPECIFIED order", "reset + add + finish"):
        assert phrase in section, phrase


def test_the_docstrings_say_what_this_is_and_is_not():
    doc = " ".join(segmentation.overlap_scores.__doc__.split())
    for phrase in ("What this is not", "Hungarian", "per-segment", "SNEMI3D / CREMI", "math.fsum", "fractions.Fraction",
                   "Where a denominator is 0", "b' = 0 included", "bijection"):
        assert phrase in doc, phrase
    doc = " ".join(segmentation.label_overlaps.__doc__.split())
    for phrase in ("ordered", "everything <= 0 is background", "DESIGN 6u", "next power of two >= 2 * D * H * W"):
        assert phrase in doc, phrase


def test_the_workspace_query():
    lib = _native.lib()

    def rounded(v):
        return (v + 255) // 256 * 256

    for capacity in (1, 2, 16, 2048, 4096, 1 << 22, 1 << 30):
        want = 2 * rounded(8 * capacity) + 256 + rounded(4 * ((capacity + 2047) // 2048))
        assert lib.exaspim_label_overlaps_workspace_bytes(capacity) == want, capacity
    assert lib.exaspim_label_overlaps_workspace_bytes(1) == 1024
    for capacity in (0, 3, -1, -4, 6, (1 << 30) + 1, 1 << 31, 1 << 40):
        assert lib.exaspim_label_overlaps_workspace_bytes(capacity) == 0, capacity
        assert _native.last_error().startswith("label_overlaps_workspace_bytes:")
        assert "pair_capacity" in _native.last_error()


A, B, WS, PAIRS, COUNTS, STATE = 0x1000, 0x2004, 0x3000, 0x4000, 0x5000, 0x6004      # never followed
NEED = 2 * 256 + 256 + 256      # capacity 16


def refusals(name, good, bad, short):
    """Every (position, value) of "bad" alone makes the call return -1 with a message in its name; the workspace
    one byte short gives -3."""
    fn = getattr(_native.lib(), "exaspim_" + name)
    for at, value in bad:
        args = list(good)
        args[at] = value
        assert fn(*args) == -1, (name, at, value)
        assert _native.last_error().startswith(name + ":"), (name, _native.last_error())
    args = list(good)
    args[short] = NEED - 1
    assert fn(*args) == -3, name
    assert _native.last_error().startswith(name + ":") and "workspace" in _native.last_error()


BAD_CAPACITIES = (0, 3, 1 << 31, -16)


def test_reset_refuses_on_the_host():
    assert _native.lib().exaspim_label_overlaps_workspace_bytes(16) == NEED
    refusals("label_overlaps_reset", [16, WS, NEED, None],
             [(0, c) for c in BAD_CAPACITIES] + [(1, None), (1, WS + 2), (1, WS + 8)], 2)


def test_add_refuses_on_the_host():
    refusals("label_overlaps_add", [A, B, 100, 16, WS, NEED, None],
             [(3, c) for c in BAD_CAPACITIES] + [(0, None), (1, None), (4, None), (0, A + 2), (1, B + 2), (0, A + 1),
                                                 (4, WS + 2), (2, -1), (2, 1 << 31), (2, 1 << 40)], 5)
    # n = 0 launches nothing: pointers that are never followed, and no device is needed
    assert _native.lib().exaspim_label_overlaps_add(A, B, 0, 16, WS, NEED, None) == 0
    for offset in range(0, 16, 4):      # any 4-byte alignment of a and of b is accepted: refused only for n
        assert _native.lib().exaspim_label_overlaps_add(A + offset, B + 12 - offset, -1, 16, WS, NEED, None) == -1
        assert "n must be" in _native.last_error()


def test_finish_refuses_on_the_host():
    refusals("label_overlaps_finish", [16, WS, NEED, PAIRS, COUNTS, STATE, None],
             [(0, c) for c in BAD_CAPACITIES] + [(1, None), (3, None), (4, None), (5, None), (1, WS + 2),
                                                 (3, PAIRS + 2), (4, COUNTS + 2), (4, COUNTS + 4), (5, STATE + 2)], 2)


def test_the_whole_call_refuses_on_the_host():
    refusals("label_overlaps", [A, B, 100, 16, PAIRS, COUNTS, STATE, WS, NEED, None],
             [(3, c) for c in BAD_CAPACITIES] + [(0, None), (1, None), (4, None), (5, None), (6, None), (7, None),
                                                 (0, A + 2), (1, B + 2), (4, PAIRS + 2), (5, COUNTS + 2),
                                                 (5, COUNTS + 4), (6, STATE + 2), (7, WS + 2), (2, -1), (2, 1 << 31)],
             8)


def test_argument_checks_that_need_no_device():
    a = np.zeros((3, 4, 5), dtype=np.int32)
    for fn in (segmentation.label_overlaps, segmentation.compare_segmentations):
        for bad in (a.astype(np.int64), a.astype(np.uint32), a.astype(np.float32)):
            with pytest.raises(TypeError, match="int32"):
                fn(bad, a)
        with pytest.raises(ValueError, match=r"\(D, H, W\)"):
            fn(a[0], a[0])
        with pytest.raises(ValueError, match="empty volume"):
            fn(a[:, :0], a[:, :0])
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(torch.zeros((3, 4, 5), dtype=torch.int32), torch.zeros((3, 4, 5), dtype=torch.int32))
    with pytest.raises(ValueError, match="background"):
        segmentation.compare_segmentations(a, a, background="x")
    with pytest.raises(ValueError, match="background"):
        segmentation.overlap_scores(np.zeros((0, 2), np.int32), np.zeros(0, np.int64), background="x")

    streaming = segmentation.label_overlaps_streaming
    for bad in (a.astype(np.int64), a.astype(np.float32)):
        with pytest.raises(TypeError, match="int32"):
            streaming(bad, a, slab_depth=2)
        with pytest.raises(TypeError, match="int32"):
            streaming(a, bad, slab_depth=2)
    with pytest.raises(TypeError, match="host array"):
        streaming(torch.zeros((3, 4, 5), dtype=torch.int32), a, slab_depth=2)
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        streaming(a[0], a[0], slab_depth=2)
    with pytest.raises(ValueError, match="empty volume"):
        streaming(a[:0], a[:0], slab_depth=2)
    with pytest.raises(ValueError, match="one shape"):
        streaming(a, a[:2], slab_depth=2)
    with pytest.raises(ValueError, match="slab_depth must be positive"):
        streaming(a, a, slab_depth=0)
    with pytest.raises(TypeError, match="slab_depth must be an integer"):
        streaming(a, a, slab_depth=2.0)
    for bad in (0, 3, 1 << 31, -4):
        with pytest.raises(ValueError, match="pair_capacity must be a power of two"):
            streaming(a, a, slab_depth=2, pair_capacity=bad)
        with pytest.raises(ValueError, match="pair_capacity must be a power of two"):
            segmentation.OverlapStream(bad)
    with pytest.raises(TypeError, match="pair_capacity must be an integer"):
        segmentation.OverlapStream(16.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        segmentation.OverlapStream(16, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        streaming(a, a, slab_depth=2, device="cpu")
    with pytest.raises(ValueError, match="more than 2\\^31 - 1 voxels"):
        big = np.lib.stride_tricks.as_strided(a, (2048, 1024, 1024), (0, 0, 0))
        streaming(big, big, slab_depth=2048)
