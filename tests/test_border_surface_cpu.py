"""
The surface of border_targets and of the given-target loops without a GPU: the new names are the same objects under
inference, their signatures, the signatures that stay, the C symbols are exported, declared and bound with the
right number of arguments, the header and the docstrings say what the definition is and is not, the workspace query
refuses on the host, and the argument checks that need no device.
"""

import inspect
import os
import re

import numpy as np
import pytest

from aind_exaspim_neuron_segmentation_amd import _native, inference, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exaspim_border_targets_workspace_bytes", "exaspim_border_targets", "exaspim_teasar_round_given"]
NAMES = ["border_targets", "teasar_branches_given", "teasar_branches_fix_branching_given", "skeletonize_fix_borders",
         "_border_targets_on_device"]


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

    check(segmentation.border_targets, ["labels"], dict(n_labels=None, return_device_tensors=False))
    check(segmentation.teasar_branches_given, ["labels", "sources", "dbf", "daf", "parents", "hops", "targets_before"],
          dict(scale=empty, const=empty, boxes=None, n_labels=None, max_paths=None, return_device_tensors=False,
               stats=None))
    check(segmentation.teasar_branches_fix_branching_given, ["labels", "sources", "dbf", "daf", "cost", "targets_before"],
          dict(scale=empty, const=empty, field=None, parents=None, hops=None, boxes=None, n_labels=None,
               max_paths=None, return_device_tensors=False, stats=None))
    check(segmentation.skeletonize_fix_borders, ["segmentation"],
          dict(fix_borders=True, fix_branching=True, scale=1.25, const=450.0, pdrf_exponent=4, pdrf_scale=100000.0,
               fill_holes=True, max_paths=None))
    # the loops' drivers take the targets as their last keyword and default to today's calls
    for fn in (segmentation._teasar_on_device, segmentation._fix_branching_on_device):
        assert inspect.signature(fn).parameters["targets_before"].default is None
    assert inspect.signature(segmentation._skeleton_chain_on_device).parameters["fix_borders"].default is False


def test_the_older_signatures_stay():
    assert list(inspect.signature(segmentation.teasar_branches).parameters) == [
        "labels", "sources", "dbf", "daf", "parents", "hops", "scale", "const", "boxes", "n_labels", "max_paths",
        "return_device_tensors", "stats"]
    assert list(inspect.signature(segmentation.skeletonize).parameters) == [
        "segmentation", "fix_branching", "scale", "const", "pdrf_exponent", "pdrf_scale", "fill_holes", "max_paths"]


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


def test_the_round_entries_differ_by_the_given_row_alone():
    old = _native.SIGNATURES["exaspim_teasar_round"][1]
    new = _native.SIGNATURES["exaspim_teasar_round_given"][1]
    assert len(new) == len(old) + 1 and new[:7] == old[:7] and new[7] is _native._vp and new[8:] == old[7:]


def test_the_abi_version_stays():
    assert int(re.search(r"#define\s+EXASPIM_ABI_VERSION\s+(\d+)", header()).group(1)) == 5


def test_the_header_states_the_definition():
    text = header()
    section = " ".join(text[text.index("border targets: the centre of every cut"):].split())
    for phrase in ("inference.py:286", "fix_borders=True", "not claimed", "centroid", "8-connected", "black border",
                   "smallest linear voxel index", "appears once", "may exceed", "no defined order",
                   "nothing allocated, nothing synchronised", "2^31 - 1"):
        assert phrase in section, phrase
    given = " ".join(text[text.index("exaspim_teasar_round with targets the loop did not choose"):].split())
    for phrase in ("manual_targets_before", "byte for byte", "not finished", "state_dev[5]", "0x7F800000",
                   "only in round 1"):
        assert phrase in given, phrase


@pytest.mark.parametrize("name", ["border_targets", "teasar_branches_given", "teasar_branches_fix_branching_given",
                                  "skeletonize_fix_borders"])
def test_the_docstrings_say_not_kimimaro(name):
    doc = " ".join(getattr(segmentation, name).__doc__.split())
    for phrase in ("inference.py:", "What this is not", "kimimaro", "not claimed"):
        assert phrase in doc, phrase
    if name != "border_targets":
        assert "max_paths counts" in doc
    for older in ("teasar_branches", "teasar_branches_fix_branching", "skeletonize", "skeletonize_labels"):
        assert "fix_borders" in getattr(segmentation, older).__doc__      # each points to the form that has it


def test_the_workspace_query_refuses_on_the_host():
    lib = _native.lib()
    assert lib.exaspim_border_targets_workspace_bytes(_native.int3((3, 4, 5))) == 4 * 384 + 752
    assert lib.exaspim_border_targets_workspace_bytes(_native.int3((1, 1, 1))) == 4 * 32 + 48
    for dims in ((3, 0, 5), (3, -4, 5), (2048, 1024, 1024), (1, 1, 2**30)):
        assert lib.exaspim_border_targets_workspace_bytes(_native.int3(dims)) == 0, dims
        assert "dims" in _native.last_error()
    assert lib.exaspim_border_targets_workspace_bytes(_native.int3((1024, 1024, 1024))) == 24 * 6 * 2**20


def test_argument_checks_that_need_no_device():
    labels = np.zeros((3, 4, 5), dtype=np.int32)
    for bad in (1.5, "3", True):
        with pytest.raises(TypeError, match="n_labels must be an integer"):
            segmentation.border_targets(labels, n_labels=bad)
    with pytest.raises(ValueError, match="n_labels must not be negative"):
        segmentation.border_targets(labels, n_labels=-1)
    with pytest.raises(TypeError, match="int32"):
        segmentation.border_targets(labels.astype(np.int64))
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        segmentation.border_targets(labels[0])
    with pytest.raises(ValueError, match="empty volume"):
        segmentation.border_targets(labels[:, :0])
    with pytest.raises(TypeError, match="torch tensor or a numpy array"):
        segmentation.border_targets([[[1]]])
    volumes = [labels] * 4
    sources = np.array([-1, 0], dtype=np.int32)
    one = np.zeros(1, dtype=np.int32)
    cases = [("pair", TypeError, "a pair"), ((one,), TypeError, "a pair"), ((one, [0]), TypeError, "torch tensor or"),
             ((one, one.astype(np.int64)), TypeError, "must be int32"),
             ((one, np.zeros((1, 1), dtype=np.int32)), ValueError, "must be 1-D"),
             ((one, np.zeros(2, dtype=np.int32)), ValueError, "one length")]
    for bad, error, match in cases:
        with pytest.raises(error, match=match):      # before anything is uploaded
            segmentation.teasar_branches_given(labels, sources, labels, labels.astype(np.float32), labels, labels, bad,
                                               scale=1.0, const=0.0)
        with pytest.raises(error, match=match):
            segmentation.teasar_branches_fix_branching_given(labels, sources, labels, labels.astype(np.float32), None,
                                                             bad, scale=1.0, const=0.0)
    for bad in (1, None, "yes", np.int32(1)):
        with pytest.raises(TypeError, match="fix_borders must be a bool"):
            segmentation.skeletonize_fix_borders(labels, fix_borders=bad)
    with pytest.raises(TypeError, match="fix_branching must be a bool"):
        segmentation.skeletonize_fix_borders(labels, fix_branching=1)
    del volumes
