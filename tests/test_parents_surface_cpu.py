"""
The surface of geodesic_parents and trace_paths, without a GPU: the names under inference and segmentation are
the same objects, the entry points are declared in the header and bound in _native with matching argument
counts, the ABI version stays 5, the header cites the reference's lines and states the definition, and the
Python layer refuses arguments of a wrong dtype, rank or shape, and tensors it cannot take, before any device
or library is asked for.
"""

import inspect
import os
import re

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd import _native, inference, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exaspim_geodesic_parents_begin", "exaspim_geodesic_parents_sweeps", "exaspim_geodesic_parents_finish",
           "exaspim_trace_paths"]


def header():
    return open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()


@pytest.mark.parametrize("name", ["geodesic_parents", "_geodesic_parents_on_device", "trace_paths"])
def test_name_is_the_same_object_under_inference(name):
    assert getattr(inference, name) is getattr(segmentation, name)
    assert getattr(segmentation, name).__module__.endswith(".segmentation")


def test_the_signatures():
    parameters = inspect.signature(segmentation.geodesic_parents).parameters
    assert list(parameters) == ["labels", "sources", "field", "cost", "n_labels", "sweeps_per_read", "max_sweeps",
                                "return_hops", "return_device_tensors", "stats"]
    defaults = dict(field=None, cost=None, n_labels=None, sweeps_per_read=32, max_sweeps=None, return_hops=False,
                    return_device_tensors=False, stats=None)
    for name, default in defaults.items():
        assert parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and parameters[name].default == default
    doc = segmentation.geodesic_parents.__doc__
    for phrase in ("tight", "hops", "smallest", "inference.py:257-291", "What this is not", "dijkstra3d", "orphan",
                   "bit for bit", "trace_paths", "far_index", "cost=cost"):
        assert phrase in doc, phrase
    parameters = inspect.signature(segmentation.trace_paths).parameters
    assert list(parameters) == ["parents", "hops", "targets", "return_device_tensors"]
    assert parameters["return_device_tensors"].kind is inspect.Parameter.KEYWORD_ONLY
    assert parameters["return_device_tensors"].default is False
    assert "inference.py:257-291" in segmentation.trace_paths.__doc__
    # geodesic_field keeps its signature and now points here
    assert "return_farthest" in inspect.signature(segmentation.geodesic_field).parameters
    assert "geodesic_parents" in segmentation.geodesic_field.__doc__


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_and_bound(name):
    text = header()
    assert re.search(r"^int " + name + r"\(", text, re.M), name
    assert name in _native.SIGNATURES
    restype, argtypes = _native.SIGNATURES[name]
    declaration = re.search(r"^int " + name + r"\((.*?)\);", text, re.M | re.S).group(1)
    declaration = re.sub(r"/\*.*?\*/", "", declaration, flags=re.S)
    assert len(argtypes) == len(declaration.split(",")), (name, declaration)
    assert restype is _native._i32


def test_the_abi_version_stays():
    assert int(re.search(r"#define\s+EXASPIM_ABI_VERSION\s+(\d+)", header()).group(1)) == 5


@pytest.mark.parametrize("name", SYMBOLS)
def test_the_entry_points_cite_the_reference(name):
    text = header()
    comment = text[:re.search(r"^int " + name + r"\(", text, re.M).start()].rsplit("/*", 1)[1]
    assert "inference.py:257-291" in comment


def test_the_header_states_the_definition():
    text = header()
    section = text[text.index("parental field and root paths of every label"):]
    for phrase in ("tight", "hops", "smallest", "not claimed to equal dijkstra3d", "least solution", "orphan",
                   "may be NULL", "bit for bit", "inference.py:257-291"):
        assert phrase in section, phrase


@pytest.fixture
def no_device(monkeypatch):
    """Any question to the device fails the test: the refusals below come first."""

    def asked(*a, **kw):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(torch.cuda, "is_available", asked)
    monkeypatch.setattr(_native, "lib", asked)


def test_numpy_arguments_are_refused_before_any_device_is_asked_for(no_device):
    fn = segmentation.geodesic_parents
    good = np.ones((3, 4, 5), dtype=np.int32)
    src = np.array([-1, 0], dtype=np.int32)
    cost = np.ones((3, 4, 5), dtype=np.float32)
    for kw in ({}, {"return_hops": True}, {"return_device_tensors": True}, {"cost": cost}, {"field": cost}):
        for dtype in (np.int64, np.uint32, np.float32, np.int16, bool):
            with pytest.raises(TypeError, match="labels must be int32"):
                fn(good.astype(dtype), src, **kw)
            with pytest.raises(TypeError, match="sources must be int32"):
                fn(good, src.astype(dtype), **kw)
        plain = {} if "cost" in kw or "field" in kw else kw
        for bad in (good[0], good[None], good[0, 0]):
            with pytest.raises(ValueError, match=r"\(D, H, W\)"):
                fn(bad, src, **plain)
        with pytest.raises(ValueError, match="empty"):
            fn(np.zeros((3, 0, 5), dtype=np.int32), src, **plain)
        with pytest.raises(TypeError):
            fn(good.tolist(), src, **kw)
        for bad in (src[None], src[:0], np.int32(3)):
            with pytest.raises(ValueError, match=r"sources must be \(K \+ 1,\)"):
                fn(good, np.asarray(bad), **kw)
        with pytest.raises(ValueError, match=r"n_labels \+ 1 = 3"):
            fn(good, src, n_labels=2, **kw)
    for what in ("cost", "field"):
        for dtype in (np.float64, np.float16, np.int32):
            with pytest.raises(TypeError, match=what + " must be float32"):
                fn(good, src, **{what: cost.astype(dtype)})
        for bad in (cost[0], cost[:, :3], cost.reshape(5, 4, 3)):
            with pytest.raises(ValueError, match=what + " must have the labels' shape"):
                fn(good, src, **{what: bad})
    for bad in (1.0, "3", None, True, np.float32(2)):
        with pytest.raises(TypeError, match="sweeps_per_read must be an integer"):
            fn(good, src, sweeps_per_read=bad)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="sweeps_per_read must be at least 1"):
            fn(good, src, sweeps_per_read=bad)
    with pytest.raises(TypeError, match="max_sweeps must be an integer"):
        fn(good, src, max_sweeps=2.5)
    with pytest.raises(ValueError, match="max_sweeps"):
        fn(good, src, max_sweeps=-1)
    with pytest.raises(ValueError, match="n_labels"):
        fn(good, src, n_labels=-1)


def test_tensor_arguments_are_refused_before_the_library_is_loaded(no_device):
    fn = segmentation.geodesic_parents
    good = torch.ones((3, 4, 5), dtype=torch.int32)
    src = torch.tensor([-1, 0], dtype=torch.int32)
    with pytest.raises(TypeError, match="labels must be int32"):
        fn(good.long(), src)
    with pytest.raises(TypeError, match="sources must be int32"):
        fn(good, src.long())
    with pytest.raises(TypeError, match="cost must be float32"):
        fn(good, src, cost=good.double())
    with pytest.raises(TypeError, match="field must be float32"):
        fn(good, src, field=good.double())
    with pytest.raises(ValueError, match="cost must have the labels' shape"):
        fn(good, src, cost=torch.ones((3, 4, 4)))
    with pytest.raises(ValueError, match="field must have the labels' shape"):
        fn(good, src, field=torch.ones((3, 4, 4)))
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        fn(good[0], src)
    with pytest.raises(ValueError, match="empty"):
        fn(good[:, :0], src)
    with pytest.raises(RuntimeError, match="geodesic_parents .* no CPU path"):
        fn(good, src)


def test_trace_paths_refuses_before_any_device_is_asked_for(no_device):
    fn = segmentation.trace_paths
    good = np.zeros((3, 4, 5), dtype=np.int32)
    targets = np.array([0, 3], dtype=np.int32)
    for dtype in (np.int64, np.float32, np.uint32):
        with pytest.raises(TypeError, match="parents must be int32"):
            fn(good.astype(dtype), good, targets)
        with pytest.raises(TypeError, match="hops must be int32"):
            fn(good, good.astype(dtype), targets)
        with pytest.raises(TypeError, match="targets must be int32"):
            fn(good, good, targets.astype(dtype))
    with pytest.raises(ValueError, match="hops must have the parents' shape"):
        fn(good, good[:, :3], targets)
    with pytest.raises(ValueError, match=r"targets must be \(T,\)"):
        fn(good, good, targets[None])
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        fn(good[0], good[0], targets)
    with pytest.raises(TypeError):
        fn(good.tolist(), good, targets)
    tensor = torch.zeros((3, 4, 5), dtype=torch.int32)
    with pytest.raises(TypeError, match="hops must be int32"):
        fn(tensor, tensor.long(), torch.tensor([0], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="trace_paths .* no CPU path"):
        fn(tensor, tensor, torch.tensor([0], dtype=torch.int32))


def test_without_a_hip_device_the_upload_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    labels, src = np.ones((3, 4, 5), dtype=np.int32), np.array([-1, 0], dtype=np.int32)
    with pytest.raises(RuntimeError, match="geodesic_parents .* no HIP device"):
        segmentation.geodesic_parents(labels, src)
    with pytest.raises(RuntimeError, match="trace_paths .* no HIP device"):
        segmentation.trace_paths(labels, labels, np.array([0], dtype=np.int32))


def test_the_library_exports_the_symbols():
    lib = _native.lib()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None
