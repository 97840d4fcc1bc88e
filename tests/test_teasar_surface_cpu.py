"""
The surface of teasar_branches, skeletonize_labels and skeleton_to_swc, without a GPU: the names under
inference and segmentation are the same objects, segmentation still does not import inference, the entry
points are declared in the header and bound in _native with matching argument counts, the ABI version stays
5, header and docstrings say which form of TEASAR this is, every argument check fires before any device or
library is asked for, and skeleton_to_swc writes a hand-made tree.
"""

import ast
import inspect
import os
import re

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd import _native, inference, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exaspim_teasar_workspace_bytes", "exaspim_teasar_begin", "exaspim_teasar_round", "exaspim_teasar_apply"]


def header():
    return open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()


@pytest.mark.parametrize("name", ["teasar_branches", "skeletonize_labels", "skeleton_to_swc", "_teasar_on_device"])
def test_name_is_the_same_object_under_inference(name):
    assert getattr(inference, name) is getattr(segmentation, name)
    assert getattr(segmentation, name).__module__.endswith(".segmentation")


def test_segmentation_still_does_not_import_inference():
    tree = ast.parse(inspect.getsource(segmentation))
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            assert not any(a.name.endswith("inference") for a in node.names), ast.dump(node)
        if isinstance(node, ast.ImportFrom):
            assert not (node.module or "").endswith("inference"), ast.dump(node)
            assert not any(a.name == "inference" for a in node.names), ast.dump(node)
    assert "inference" not in vars(segmentation)


def test_the_signatures():
    parameters = inspect.signature(segmentation.teasar_branches).parameters
    assert list(parameters) == ["labels", "sources", "dbf", "daf", "parents", "hops", "scale", "const", "boxes",
                                "n_labels", "max_paths", "return_device_tensors", "stats"]
    for name in ("scale", "const"):
        assert parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
        assert parameters[name].default is inspect.Parameter.empty
    for name, default in dict(boxes=None, n_labels=None, max_paths=None, return_device_tensors=False,
                              stats=None).items():
        assert parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and parameters[name].default == default
    parameters = inspect.signature(segmentation.skeletonize_labels).parameters
    assert list(parameters) == ["labels", "scale", "const", "pdrf_exponent", "pdrf_scale", "fill_holes", "max_paths"]
    defaults = dict(scale=1.25, const=450.0, pdrf_exponent=4, pdrf_scale=100000.0, fill_holes=True, max_paths=None)
    for name, default in defaults.items():      # the reference's teasar_params
        assert parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and parameters[name].default == default
    assert list(inspect.signature(segmentation.skeleton_to_swc).parameters) == ["vertices", "parent", "radius"]


@pytest.mark.parametrize("fn", [segmentation.teasar_branches, segmentation.skeletonize_labels])
def test_the_docstrings_say_which_form_this_is(fn):
    doc = " ".join(fn.__doc__.split())
    for phrase in ("inference.py:257-291", "fix_branching=False", "fix_branching=True", "What this is not",
                   "kimimaro", "soma_*", "spherical invalidation", "fix_borders", "anisotropy"):
        assert phrase in doc, phrase


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


def test_the_abi_version_stays():
    assert int(re.search(r"#define\s+EXASPIM_ABI_VERSION\s+(\d+)", header()).group(1)) == 5


def test_the_header_states_the_definition():
    text = header()
    section = " ".join(text[text.index("TEASAR's loop: targets, branches, invalidation"):].split())
    for phrase in ("inference.py:257-291", "fix_branching=False", "fix_branching=True", "not claimed", "0x7F800000",
                   "largest daf bits", "smallest linear index", "junction", "sqrt64", "Chebyshev", "fix_borders",
                   "anisotropy", "spherical invalidation", "nothing allocated, nothing synchronised"):
        assert phrase in section, phrase


def test_the_workspace_query_refuses_on_the_host():
    lib = _native.lib()
    assert lib.exaspim_teasar_workspace_bytes(_native.int3((3, 4, 5)), 0) == 32
    assert lib.exaspim_teasar_workspace_bytes(_native.int3((3, 4, 5)), 122) == 984 + 8 + 492 + 4
    for dims in ((3, 0, 5), (3, -4, 5), (2048, 1024, 1024)):
        assert lib.exaspim_teasar_workspace_bytes(_native.int3(dims), 3) == 0, dims
        assert "dims" in _native.last_error()
    assert lib.exaspim_teasar_workspace_bytes(_native.int3((2047, 1024, 1024)), 3) > 0
    assert lib.exaspim_teasar_workspace_bytes(_native.int3((3, 4, 5)), -1) == 0 and "n_labels" in _native.last_error()


@pytest.fixture
def no_device(monkeypatch):
    """Any question to the device fails the test: the refusals below come first."""

    def asked(*a, **kw):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(torch.cuda, "is_available", asked)
    monkeypatch.setattr(_native, "lib", asked)


def arguments(make=np.asarray):
    shape = (3, 4, 5)
    return dict(labels=make(np.ones(shape, dtype=np.int32)), sources=make(np.array([-1, 0], dtype=np.int32)),
                dbf=make(np.ones(shape, dtype=np.int32)), daf=make(np.ones(shape, dtype=np.float32)),
                parents=make(np.zeros(shape, dtype=np.int32)), hops=make(np.zeros(shape, dtype=np.int32)))


def call(args, **kw):
    args = dict(args)
    keywords = dict(scale=1.25, const=2.0)
    keywords.update(kw)
    return segmentation.teasar_branches(*(args[k] for k in ("labels", "sources", "dbf", "daf", "parents", "hops")),
                                        **keywords)


def test_numpy_arguments_are_refused_before_any_device_is_asked_for(no_device):
    good = arguments()
    for name in ("labels", "sources", "dbf", "parents", "hops"):
        for dtype in (np.int64, np.uint32, np.float32, np.int16, bool):
            with pytest.raises(TypeError, match=f"{name} must be int32"):
                call(dict(good, **{name: good[name].astype(dtype)}))
    for dtype in (np.float64, np.float16, np.int32):
        with pytest.raises(TypeError, match="daf must be float32"):
            call(dict(good, daf=good["daf"].astype(dtype)))
    with pytest.raises(TypeError, match="boxes must be int32"):
        call(good, boxes=np.zeros((2, 6), dtype=np.int64))
    for bad in (good["labels"][0], good["labels"][None]):
        with pytest.raises(ValueError):
            call(dict(good, labels=bad))
    with pytest.raises(ValueError, match="empty"):
        empty = {k: (v[:, :0] if v.ndim == 3 else v) for k, v in good.items()}
        call(empty)
    with pytest.raises(TypeError):
        call(dict(good, labels=good["labels"].tolist()))
    for name in ("dbf", "daf", "parents", "hops"):
        for bad in (good[name][0], good[name][:, :3], good[name].reshape(5, 4, 3)):
            with pytest.raises(ValueError, match=f"{name} must have the labels' shape"):
                call(dict(good, **{name: bad}))
    for bad in (good["sources"][None], good["sources"][:0], np.int32(3)):
        with pytest.raises(ValueError, match=r"sources must be \(K \+ 1,\)"):
            call(dict(good, sources=np.asarray(bad)))
    with pytest.raises(ValueError, match=r"n_labels \+ 1 = 3"):
        call(good, n_labels=2)
    for bad in (np.zeros((3, 6), dtype=np.int32), np.zeros((2, 5), dtype=np.int32), np.zeros(12, dtype=np.int32)):
        with pytest.raises(ValueError, match=r"boxes must be \(2, 6\)"):
            call(good, boxes=bad)
    for name in ("scale", "const"):
        for bad in ("1", None, True, [1.0], 1j):
            with pytest.raises(TypeError, match=f"{name} must be a real number"):
                call(good, **{name: bad})
        for bad in (-1.0, -1e-300, float("inf"), float("nan"), -float("inf")):
            with pytest.raises(ValueError, match=f"{name} must be finite and not negative"):
                call(good, **{name: bad})
    with pytest.raises(TypeError):      # scale and const have no defaults here
        segmentation.teasar_branches(*arguments().values())
    for bad in (1.0, "3", True, np.float32(2)):
        with pytest.raises(TypeError, match="max_paths must be an integer"):
            call(good, max_paths=bad)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="max_paths must be at least 1"):
            call(good, max_paths=bad)
    with pytest.raises(TypeError, match="n_labels must be an integer"):
        call(good, n_labels=1.0)
    with pytest.raises(ValueError, match="n_labels"):
        call(good, n_labels=-1)


def test_tensor_arguments_are_refused_before_the_library_is_loaded(no_device):
    good = arguments(torch.from_numpy)
    for name in ("labels", "sources", "dbf", "parents", "hops"):
        with pytest.raises(TypeError, match=f"{name} must be int32"):
            call(dict(good, **{name: good[name].long()}))
    with pytest.raises(TypeError, match="daf must be float32"):
        call(dict(good, daf=good["daf"].double()))
    for name in ("dbf", "daf", "parents", "hops"):
        with pytest.raises(ValueError, match=f"{name} must have the labels' shape"):
            call(dict(good, **{name: good[name][:, :, :4]}))
    with pytest.raises(ValueError, match=r"boxes must be \(2, 6\)"):
        call(good, boxes=torch.zeros((3, 6), dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        call({k: (v[0] if v.ndim == 3 else v) for k, v in good.items()})
    with pytest.raises(RuntimeError, match="teasar_branches .* no CPU path"):
        call(good)


def test_skeletonize_labels_refuses_before_any_device_is_asked_for(no_device):
    fn = segmentation.skeletonize_labels
    good = np.ones((3, 4, 5), dtype=np.int32)
    with pytest.raises(TypeError, match="labels must be int32"):
        fn(good.astype(np.int64))
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        fn(good[0])
    for name in ("scale", "const", "pdrf_scale"):
        with pytest.raises(TypeError, match=f"{name} must be a real number"):
            fn(good, **{name: "1"})
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=f"{name} must be finite and not negative"):
                fn(good, **{name: bad})
    for bad in (4.0, True, "4"):
        with pytest.raises(TypeError, match="pdrf_exponent must be an integer"):
            fn(good, pdrf_exponent=bad)
    with pytest.raises(ValueError, match="pdrf_exponent must not be negative"):
        fn(good, pdrf_exponent=-1)
    with pytest.raises(TypeError, match="max_paths must be an integer"):
        fn(good, max_paths=1.5)
    with pytest.raises(ValueError, match="max_paths must be at least 1"):
        fn(good, max_paths=0)
    with pytest.raises(RuntimeError, match="skeletonize_labels .* no CPU path"):
        fn(torch.from_numpy(good))


def test_without_a_hip_device_the_upload_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="teasar_branches .* no HIP device"):
        call(arguments())
    with pytest.raises(RuntimeError, match="skeletonize_labels .* no HIP device"):
        segmentation.skeletonize_labels(np.ones((3, 4, 5), dtype=np.int32))


def test_skeleton_to_swc_on_a_hand_made_tree():
    #      0 -- 1 -- 2
    #           |
    #           3 -- 4
    vertices = np.array([[5, 6, 7], [5, 6, 8], [5, 6, 9], [6, 6, 8], [7, 6, 8]], dtype=np.int32)
    parent = np.array([-1, 0, 1, 1, 3], dtype=np.int32)
    radius = np.array([1.0, 1.5, 2.0, np.sqrt(np.float32(2)), 0.0], dtype=np.float32)
    text = segmentation.skeleton_to_swc(vertices, parent, radius)
    lines = text.splitlines()
    assert text.endswith("\n") and len(lines) == 5
    assert lines[0] == "1 0 5 6 7 1 -1"
    assert lines[1] == "2 0 5 6 8 1.5 1"
    assert lines[2] == "3 0 5 6 9 2 2"
    assert lines[4] == "5 0 7 6 8 0 4"
    for i, line in enumerate(lines):
        fields = line.split()
        assert len(fields) == 7 and int(fields[0]) == i + 1 and fields[1] == "0"
        assert [float(f) for f in fields[2:5]] == vertices[i].tolist()
        assert np.float32(fields[5]) == pytest.approx(radius[i], rel=1e-5)
        assert int(fields[6]) == (parent[i] + 1 if parent[i] >= 0 else -1)
    assert segmentation.skeleton_to_swc(np.zeros((0, 3)), np.zeros(0, dtype=np.int32), np.zeros(0)) == ""
    with pytest.raises(ValueError, match="vertices must be"):
        segmentation.skeleton_to_swc(vertices[:, :2], parent, radius)
    with pytest.raises(ValueError, match="vertices must be"):
        segmentation.skeleton_to_swc(vertices, parent[:4], radius)
    with pytest.raises(ValueError, match="neither -1 nor a row"):
        segmentation.skeleton_to_swc(vertices, np.array([-1, 0, 1, 1, 5]), radius)
    with pytest.raises(ValueError, match="integers"):
        segmentation.skeleton_to_swc(vertices, parent.astype(np.float32), radius)
