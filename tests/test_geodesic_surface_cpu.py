"""
The surface of geodesic_field, without a GPU: the names under inference and segmentation are the same
objects, the entry points are declared in the header and bound in _native with matching argument counts,
the ABI version stays 5, the header cites the reference's lines and states the definition, and the Python
layer refuses arguments of a wrong dtype, rank or shape, and tensors it cannot take, before any device or
library is asked for.
"""

import inspect
import os
import re

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd import _native, inference, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exaspim_geodesic_workspace_bytes", "exaspim_geodesic_begin", "exaspim_geodesic_sweeps",
           "exaspim_geodesic_farthest_workspace_bytes", "exaspim_geodesic_farthest"]


def header():
    return open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()


@pytest.mark.parametrize("name", ["geodesic_field", "_geodesic_on_device"])
def test_name_is_the_same_object_under_inference(name):
    assert getattr(inference, name) is getattr(segmentation, name)
    assert getattr(segmentation, name).__module__.endswith(".segmentation")


def test_the_signature():
    parameters = inspect.signature(segmentation.geodesic_field).parameters
    assert list(parameters) == ["labels", "sources", "cost", "n_labels", "sweeps_per_read", "max_sweeps",
                                "return_farthest", "return_device_tensors", "stats"]
    defaults = dict(cost=None, n_labels=None, sweeps_per_read=32, max_sweeps=None, return_farthest=False,
                    return_device_tensors=False, stats=None)
    for name, default in defaults.items():
        assert parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and parameters[name].default == default
    doc = segmentation.geodesic_field.__doc__
    for phrase in ("labels <= 0", "26-neighbourhood", "0x3FB504F3", "0x3FDDB3D7", "inference.py:257-291",
                   "What this is not", "dijkstra3d", "find_root", "Soma roots", "peak_index", "far_index",
                   "bit for bit"):
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


@pytest.mark.parametrize("name", ["exaspim_geodesic_begin", "exaspim_geodesic_sweeps", "exaspim_geodesic_farthest"])
def test_the_entry_points_cite_the_reference(name):
    text = header()
    comment = text[:re.search(r"^int " + name + r"\(", text, re.M).start()].rsplit("/*", 1)[1]
    assert "inference.py:257-291" in comment


def test_the_header_states_the_definition():
    text = header()
    section = text[text.index("geodesic distance-from-source field of every label"):]
    for phrase in ("0x3FB504F3", "0x3FDDB3D7", "least solution", "monotone", "-0.0", "NaN", "may be NULL",
                   "not claimed to equal dijkstra3d"):
        assert phrase in section, phrase


@pytest.fixture
def no_device(monkeypatch):
    """Any question to the device fails the test: the refusals below come first."""

    def asked(*a, **kw):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(torch.cuda, "is_available", asked)
    monkeypatch.setattr(_native, "lib", asked)


def test_numpy_arguments_are_refused_before_any_device_is_asked_for(no_device):
    fn = segmentation.geodesic_field
    good = np.ones((3, 4, 5), dtype=np.int32)
    src = np.array([-1, 0], dtype=np.int32)
    cost = np.ones((3, 4, 5), dtype=np.float32)
    for kw in ({}, {"return_farthest": True}, {"return_device_tensors": True}, {"cost": cost}):
        for dtype in (np.int64, np.uint32, np.float32, np.int16, bool):
            with pytest.raises(TypeError, match="labels must be int32"):
                fn(good.astype(dtype), src, **kw)
            with pytest.raises(TypeError, match="sources must be int32"):
                fn(good, src.astype(dtype), **kw)
        for bad in (good[0], good[None], good[0, 0]):
            with pytest.raises(ValueError, match=r"\(D, H, W\)"):
                fn(bad, src, **({} if "cost" in kw else kw))
        with pytest.raises(ValueError, match="empty"):
            fn(np.zeros((3, 0, 5), dtype=np.int32), src, **({} if "cost" in kw else kw))
        with pytest.raises(TypeError):
            fn(good.tolist(), src, **kw)
        for bad in (src[None], src[:0], np.int32(3)):
            with pytest.raises(ValueError, match=r"sources must be \(K \+ 1,\)"):
                fn(good, np.asarray(bad), **kw)
        with pytest.raises(ValueError, match=r"n_labels \+ 1 = 3"):
            fn(good, src, n_labels=2, **kw)
    for dtype in (np.float64, np.float16, np.int32):
        with pytest.raises(TypeError, match="cost must be float32"):
            fn(good, src, cost=cost.astype(dtype))
    for bad in (cost[0], cost[:, :3], cost.reshape(5, 4, 3)):
        with pytest.raises(ValueError, match="cost must have the labels' shape"):
            fn(good, src, cost=bad)
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
    fn = segmentation.geodesic_field
    good = torch.ones((3, 4, 5), dtype=torch.int32)
    src = torch.tensor([-1, 0], dtype=torch.int32)
    with pytest.raises(TypeError, match="labels must be int32"):
        fn(good.long(), src)
    with pytest.raises(TypeError, match="sources must be int32"):
        fn(good, src.long())
    with pytest.raises(TypeError, match="cost must be float32"):
        fn(good, src, cost=good.double())
    with pytest.raises(ValueError, match="cost must have the labels' shape"):
        fn(good, src, cost=torch.ones((3, 4, 4)))
    with pytest.raises(ValueError, match=r"\(D, H, W\)"):
        fn(good[0], src)
    with pytest.raises(ValueError, match="empty"):
        fn(good[:, :0], src)
    with pytest.raises(RuntimeError, match="geodesic_field .* no CPU path"):
        fn(good, src)


def test_without_a_hip_device_the_upload_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="geodesic_field .* no HIP device"):
        segmentation.geodesic_field(np.ones((3, 4, 5), dtype=np.int32), np.array([-1, 0], dtype=np.int32))


def test_the_workspace_queries_refuse_on_the_host():
    """The size functions run on the host alone: 0 and a message for what the calls refuse."""
    lib = _native.lib()
    for dims, tiles in (((3, 4, 5), 1), ((1, 1, 1), 1), ((9, 9, 33), 8), ((64, 256, 256), 8 * 32 * 8),
                        ((262152, 9, 9), 65538)):
        need = lib.exaspim_geodesic_workspace_bytes(_native.int3(dims))
        assert 16 + 8 * tiles <= need <= 16 + 8 * tiles + 16 and need % 16 == 0, dims      # header, two int32 flags
    for dims in ((3, 0, 5), (3, -4, 5), (2048, 1024, 1024)):
        assert lib.exaspim_geodesic_workspace_bytes(_native.int3(dims)) == 0, dims
        assert "dims" in _native.last_error()
    assert lib.exaspim_geodesic_workspace_bytes(_native.int3((2047, 1024, 1024))) > 0
    assert lib.exaspim_geodesic_farthest_workspace_bytes(0) == 16
    assert lib.exaspim_geodesic_farthest_workspace_bytes(122) == 984 + 8 and 123 * 8 == 984
    assert lib.exaspim_geodesic_farthest_workspace_bytes(-1) == 0 and "n_labels" in _native.last_error()
