"""
The streamed components' ABI without a GPU: the workspace queries, and that a call with a bad
descriptor or argument is refused with a message before anything could be launched.
"""

import ctypes
import os

import pytest

from aind_exaspim_neuron_segmentation_amd import _native


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _native.lib()


def descriptor(**kw):
    d = _native.ComponentsStreamDesc()
    d.dims[:] = kw.pop("dims", (24, 40, 72))
    d.channels, d.threshold, d.capacity, d.min_size = 3, 0.5, 1000, 100
    for name in ("id_parent_dev", "id_count_dev", "table_dev", "state_dev", "seam_ids_dev", "seam_bits_dev"):
        setattr(d, name, 0x1000)      # never dereferenced: every call below is refused first
    for name, value in kw.items():
        setattr(d, name, value)
    return d


def test_workspace_queries(lib):
    whole = lib.exaspim_components_workspace_bytes(_native.int3((8, 40, 72)))
    need = lib.exaspim_components_stream_slab_workspace_bytes(_native.int3((8, 40, 72)))
    assert need == whole + -(-40 * 72 // 256) * 256
    assert lib.exaspim_components_stream_slab_workspace_bytes(_native.int3((2048, 1024, 1024))) == 0
    assert "2^31 - 1" in _native.last_error()
    assert lib.exaspim_components_stream_finish_workspace_bytes(1) == 256
    assert lib.exaspim_components_stream_finish_workspace_bytes(2**31 - 2) == 2**20 * 4
    assert lib.exaspim_components_stream_finish_workspace_bytes(0) == 0
    assert lib.exaspim_components_stream_finish_workspace_bytes(2**31 - 1) == 0


@pytest.mark.parametrize("fields,word", [
    (dict(channels=2), "channels"),
    (dict(capacity=0), "capacity"),
    (dict(capacity=2**31 - 1), "capacity"),
    (dict(dims=(4, 65536, 65536)), "dims"),
    (dict(dims=(0, 4, 4)), "dims"),
    (dict(table_dev=None), "NULL"),
    (dict(id_count_dev=0x1004), "misaligned"),
    (dict(next_z=25), "next_z"),
])
def test_a_bad_descriptor_is_refused(lib, fields, word):
    d = descriptor(**fields)
    dims = _native.int3((8,) + tuple(d.dims[1:]))
    for rc in (lib.exaspim_components_stream_slab(ctypes.byref(d), 0x1000, _native.AFF_F32, dims, d.next_z, 0x1000,
                                                  0x1000, 1 << 40, None),
               lib.exaspim_components_stream_finish(ctypes.byref(d), 0x1000, 1 << 40, None),
               lib.exaspim_components_stream_apply(ctypes.byref(d), 0x1000, 16, None)):
        assert rc == -1 and word in _native.last_error()


def test_bad_slab_arguments_are_refused(lib):
    d = descriptor(next_z=8)
    ref = ctypes.byref(d)
    dims = _native.int3((8, 40, 72))

    def slab(aff=0x1000, code=_native.AFF_F32, dims=dims, z0=8, labels=0x1000, ws=0x1000, nbytes=1 << 40):
        return lib.exaspim_components_stream_slab(ref, aff, code, dims, z0, labels, ws, nbytes, None)

    for kw, word in ((dict(z0=0), "z order"), (dict(z0=16), "z order"), (dict(code=7), "aff_dtype"),
                     (dict(dims=_native.int3((8, 40, 71))), "(y, x)"), (dict(dims=_native.int3((8, 39, 72))), "(y, x)"),
                     (dict(dims=_native.int3((17, 40, 72))), "leave the volume"), (dict(labels=None), "NULL"),
                     (dict(ws=0x1004), "misaligned"), (dict(labels=0x1002), "misaligned"),
                     (dict(aff=0x1002), "misaligned")):
        assert slab(**kw) == -1 and word in _native.last_error(), kw
    assert slab(nbytes=1000) == -3 and "workspace" in _native.last_error()
    assert slab(aff=0x1002, code=_native.AFF_F16, nbytes=1000) == -3      # a half is aligned to 2 bytes
    assert d.next_z == 8
    assert lib.exaspim_components_stream_finish(ref, 0x1000, 1 << 40, None) == -1
    assert "8 of 24 planes" in _native.last_error()
    d.next_z = 24
    assert lib.exaspim_components_stream_finish(ref, 0x1000, 255, None) == -3
    assert lib.exaspim_components_stream_finish(ref, 0x1004, 256, None) == -1
    assert lib.exaspim_components_stream_apply(ref, 0x1002, 16, None) == -1
