"""
CPU-only checks of the clipped trimmed forward's host side: the header declares the entry and the library
exports it, and inference.batch_keep_hi gives, per batch, what a brute-force pass over the stitch's own
placement rule (accum[s:e] += patch[:e - s], e = min(s + out, dim)) keeps.
"""

import os
import re

import numpy as np
import pytest

from aind_exaspim_neuron_segmentation_amd import _native, inference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_clipped_entry():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    header = open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()
    m = re.search(r"int\s+exaspim_unet_forward_prepared_clipped\s*\(([^;]*)\);", header)
    assert m, "the header does not declare exaspim_unet_forward_prepared_clipped"
    assert "const int32_t keep_hi[3]" in m.group(1) and "row_stride" in m.group(1)
    assert re.search(r"#define\s+EXASPIM_ABI_VERSION\s+5\b", header)
    lib = _native.lib()
    assert lib.exaspim_unet_forward_prepared_clipped is not None
    assert lib.exaspim_abi_version() == 5
    # no device is needed to be turned away: a NULL handle is an invalid argument
    rc = lib.exaspim_unet_forward_prepared_clipped(None, None, None, 1, 32, 32, 32, 1, 8, 0, _native.int3((24, 24, 24)),
                                                   None, 0, None)
    assert rc == -1


def _brute_force(starts, patch, trim, dims):
    """Largest local index + 1 that any patch of the batch contributes to the volume, per axis, by walking
    the voxels of the trimmed patch one by one; None if that is the whole trimmed patch on every axis."""
    keep = []
    for a in range(3):
        hi = 0
        for s in starts:
            for local in range(trim, patch[a] - trim):
                if s[a] + local < dims[a]:
                    hi = max(hi, local + 1)
        keep.append(hi if hi > trim else patch[a] - trim)
    return None if all(k == p - trim for k, p in zip(keep, patch)) else tuple(keep)


@pytest.mark.parametrize("dims,patch,overlap,trim,batch,origin", [
    ((1024, 1024, 1024), (96, 96, 96), (32, 32, 32), 8, 16, None),
    ((160, 160, 224), (96, 96, 96), (32, 32, 32), 8, 2, None),
    ((160, 160, 224), (32, 32, 96), (8, 8, 32), 4, 3, None),
    ((200, 168, 230), (64, 64, 64), (16, 16, 16), 8, 5, None),          # batches that wrap around rows
    ((1024, 1024, 1024), (96, 96, 96), (32, 32, 32), 8, 16, (512, 768, 0)),   # a shard: only starts from its origin on
])
def test_batch_keep_hi_matches_the_stitch_rule(dims, patch, overlap, trim, batch, origin):
    plan = inference.SlidingWindow(dims, patch, overlap, trim)
    starts = plan.starts()
    if origin is not None:
        starts = [s for s in starts if all(v >= o for v, o in zip(s, origin))]
        assert starts and starts[0] == origin
    seen = set()
    for i in range(0, len(starts), batch):
        b = starts[i:i + batch]
        got = inference.batch_keep_hi(b, patch, trim, dims)
        key = tuple(min(s[a] for s in b) for a in range(3))
        if key not in seen:     # (the brute force once per distinct geometry)
            seen.add(key)
            assert got == _brute_force(b, patch, trim, dims), (b[0], b[-1])
        if got is not None:
            assert all(trim < k <= p - trim for k, p in zip(got, patch))
    if dims == (1024, 1024, 1024) and origin is None:
        clipped = [inference.batch_keep_hi(starts[i:i + batch], patch, trim, dims) for i in range(0, len(starts), batch)]
        assert len(clipped) == 256 and sum(c is not None for c in clipped) == 31
        assert set(clipped) == {None, (64, 88, 88), (88, 64, 88), (64, 64, 88)}


def test_batch_keep_hi_without_a_trim_is_none():
    assert inference.batch_keep_hi([(0, 0, 0)], (32, 32, 32), 0, (16, 16, 16)) is None
    assert np.all(np.array(inference.batch_keep_hi([(0, 0, 0), (0, 0, 24)], (32, 32, 32), 4, (40, 20, 40))) == (28, 20, 28))
