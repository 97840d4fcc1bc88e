"""
The surface of fill_holes, without a GPU: the names under inference and segmentation are the same objects,
the two entry points are declared in the header and bound in _native with matching argument counts, the
header cites the reference's lines, and the Python layer refuses numpy arguments of a wrong dtype, rank or
shape, and tensors it cannot take, before any device or library is asked for.
"""

import inspect
import os
import re

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd import _native, inference, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exaspim_fill_holes_workspace_bytes", "exaspim_fill_holes"]


def header():
    return open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()


@pytest.mark.parametrize("name", ["fill_holes", "_fill_holes_on_device"])
def test_name_is_the_same_object_under_inference(name):
    assert getattr(inference, name) is getattr(segmentation, name)
    assert getattr(segmentation, name).__module__.endswith(".segmentation")


def test_the_signature():
    parameters = inspect.signature(segmentation.fill_holes).parameters
    assert list(parameters) == ["labels", "return_counts", "return_device_tensor"]
    for name in ("return_counts", "return_device_tensor"):
        assert parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and parameters[name].default is False
    doc = segmentation.fill_holes.__doc__
    for phrase in ("labels <= 0", "6-connected", "binary_fill_holes", "inference.py:257-291", "fill_voids"):
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


def test_the_entry_point_cites_the_reference():
    text = header()
    comment = text[:re.search(r"^int exaspim_fill_holes\(", text, re.M).start()].rsplit("/*", 1)[1]
    assert "inference.py:257-291" in comment
    assert "out_dev ==" in comment and "labels_dev" in comment      # in-place use is part of the contract


@pytest.fixture
def no_device(monkeypatch):
    """Any question to the device fails the test: the refusals below come first."""

    def asked(*a, **kw):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(torch.cuda, "is_available", asked)
    monkeypatch.setattr(_native, "lib", asked)


def test_numpy_arguments_are_refused_before_any_device_is_asked_for(no_device):
    good = np.ones((3, 4, 5), dtype=np.int32)
    for kw in ({}, {"return_counts": True}, {"return_device_tensor": True}):
        for dtype in (np.int64, np.uint32, np.float32, np.int16, bool):
            with pytest.raises(TypeError, match="int32"):
                segmentation.fill_holes(good.astype(dtype), **kw)
        for bad in (good[0], good[None], good[0, 0]):
            with pytest.raises(ValueError, match=r"\(D, H, W\)"):
                segmentation.fill_holes(bad, **kw)
        with pytest.raises(ValueError, match="empty"):
            segmentation.fill_holes(np.zeros((3, 0, 5), dtype=np.int32), **kw)
        with pytest.raises(TypeError):
            segmentation.fill_holes(good.tolist(), **kw)


def test_tensor_arguments_are_refused_before_the_library_is_loaded(no_device):
    good = torch.ones((3, 4, 5), dtype=torch.int32)
    for fn in (segmentation.fill_holes, segmentation._fill_holes_on_device):
        with pytest.raises(TypeError, match="int32"):
            fn(good.long())
        with pytest.raises(ValueError, match=r"\(D, H, W\)"):
            fn(good[0])
        with pytest.raises(ValueError, match="empty"):
            fn(good[:, :0])
        with pytest.raises(RuntimeError, match="fill_holes .* no CPU path"):
            fn(good)
    with pytest.raises(TypeError, match="torch tensor"):
        segmentation._fill_holes_on_device(np.ones((3, 4, 5), dtype=np.int32))


def test_without_a_hip_device_the_upload_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="fill_holes .* no HIP device"):
        segmentation.fill_holes(np.ones((3, 4, 5), dtype=np.int32))


def test_the_workspace_query_refuses_on_the_host():
    """The size function runs on the host alone: 0 and a message for what the call refuses."""
    lib = _native.lib()
    for dims, n in (((3, 4, 5), 60), ((1, 1, 1), 1), ((64, 256, 256), 1 << 22)):
        need = lib.exaspim_fill_holes_workspace_bytes(_native.int3(dims))
        assert 13 * n <= need <= 13 * n + 4 * 256 and need % 16 == 0, dims      # parent 4, mask 1, lo 4, hi 4
    for dims in ((3, 0, 5), (3, -4, 5), (2048, 1024, 1024)):
        assert lib.exaspim_fill_holes_workspace_bytes(_native.int3(dims)) == 0, dims
        assert "dims" in _native.last_error()
    assert lib.exaspim_fill_holes_workspace_bytes(_native.int3((2047, 1024, 1024))) > 0
