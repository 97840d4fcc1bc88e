"""
The surface of the distance-to-boundary field and the segment table, without a GPU: the names under
inference and segmentation are the same objects, the four entry points are declared in the header and
bound in _native, and the Python layer refuses numpy arguments of a wrong dtype, rank or shape before
any device is asked for.
"""

import os
import re

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd import _native, inference, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exaspim_dbf_workspace_bytes", "exaspim_dbf", "exaspim_segment_table_workspace_bytes",
           "exaspim_segment_table"]


@pytest.mark.parametrize("name", ["distance_to_boundary", "segment_table", "DBF_INF"])
def test_name_is_the_same_object_under_inference(name):
    assert getattr(inference, name) is getattr(segmentation, name)
    if callable(getattr(segmentation, name)):
        assert getattr(segmentation, name).__module__.endswith(".segmentation")


def test_the_constant():
    assert segmentation.DBF_INF == 2**31 - 1 == np.iinfo(np.int32).max
    header = open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()
    assert int(re.search(r"#define\s+EXASPIM_DBF_INF\s+(\d+)", header).group(1)) == segmentation.DBF_INF


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_and_bound(name):
    header = open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()
    assert re.search(r"^(size_t|int) " + name + r"\(", header, re.M), name
    assert name in _native.SIGNATURES
    restype, argtypes = _native.SIGNATURES[name]
    declaration = re.search(r"^(?:size_t|int) " + name + r"\((.*?)\);", header, re.M | re.S).group(1)
    declaration = re.sub(r"/\*.*?\*/", "", declaration, flags=re.S)
    assert len(argtypes) == len(declaration.split(",")), (name, declaration)
    assert restype is (_native._sz if name.endswith("_bytes") else _native._i32)


def test_both_entry_points_cite_the_reference():
    header = open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()
    for name in ("exaspim_dbf", "exaspim_segment_table"):
        comment = header[:re.search(r"^int " + name + r"\(", header, re.M).start()].rsplit("/*", 1)[1]
        assert "inference.py:257-291" in comment, name


@pytest.fixture
def no_device(monkeypatch):
    """Any question to the device fails the test: the refusals below come first."""

    def asked(*a, **kw):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(torch.cuda, "is_available", asked)
    monkeypatch.setattr(_native, "lib", asked)


def test_numpy_arguments_are_refused_before_any_device_is_asked_for(no_device):
    good = np.ones((3, 4, 5), dtype=np.int32)
    for fn in (segmentation.distance_to_boundary, segmentation.segment_table):
        for dtype in (np.int64, np.uint32, np.float32, np.int16):
            with pytest.raises(TypeError, match="int32"):
                fn(good.astype(dtype))
        for bad in (good[0], good[None], good[0, 0]):
            with pytest.raises(ValueError, match=r"\(D, H, W\)"):
                fn(bad)
        with pytest.raises(ValueError, match="empty"):
            fn(np.zeros((3, 0, 5), dtype=np.int32))
        with pytest.raises(TypeError):
            fn(good.tolist())
    with pytest.raises(TypeError, match="dbf must be int32"):
        segmentation.segment_table(good, good.astype(np.float32))
    with pytest.raises(ValueError, match="labels' shape"):
        segmentation.segment_table(good, good[:2])


def test_tensor_arguments_are_refused_before_the_library_is_loaded(no_device):
    good = torch.ones((3, 4, 5), dtype=torch.int32)
    for fn in (segmentation.distance_to_boundary, segmentation.segment_table):
        with pytest.raises(TypeError, match="int32"):
            fn(good.long())
        with pytest.raises(ValueError, match=r"\(D, H, W\)"):
            fn(good[0])
        with pytest.raises(ValueError, match="empty"):
            fn(good[:, :0])
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(good)


def test_without_a_hip_device_the_upload_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    good = np.ones((3, 4, 5), dtype=np.int32)
    with pytest.raises(RuntimeError, match="distance_to_boundary .* no HIP device"):
        segmentation.distance_to_boundary(good)
    with pytest.raises(RuntimeError, match="segment_table .* no HIP device"):
        segmentation.segment_table(good, good)


def test_workspace_queries_refuse_on_the_host():
    """The size functions run on the host alone: 0 and a message for what the calls refuse."""
    lib = _native.lib()
    assert lib.exaspim_dbf_workspace_bytes(_native.int3((3, 4, 5))) == 240
    assert lib.exaspim_dbf_workspace_bytes(_native.int3((1, 1, 1))) == 16
    for dims in ((3, 0, 5), (3, -4, 5), (2048, 1024, 1024), (1, 1, 46340), (32768, 32768, 1)):
        assert lib.exaspim_dbf_workspace_bytes(_native.int3(dims)) == 0, dims
        assert "dims" in _native.last_error()
    assert lib.exaspim_dbf_workspace_bytes(_native.int3((1, 1, 46339))) == 4 * 46339 + 4
    assert lib.exaspim_segment_table_workspace_bytes(0) == 16
    assert lib.exaspim_segment_table_workspace_bytes(2) == 32
    assert lib.exaspim_segment_table_workspace_bytes(-1) == 0
    assert "n_labels" in _native.last_error()
