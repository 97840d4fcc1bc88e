"""
WatershedStream, watershed_fragments_streaming and the streamed agglomeration with watershed fragments and device
rounds, with torch.empty and numpy.empty poisoned (-m gpu), in the manner of tests/test_gpu_poisoned_blocks.py:
every entry point runs twice under 0x00, then under 0xFF, 0x7F and 0x01; every returned array must have the bits of
the 0x00 run, and the 0xFF run is held to the whole-volume oracle of tests/watershed_ref.py. Inputs are made before
the context is entered: only the wrappers' own allocations are poisoned -- the id tables, the three carried planes
(0xFF: NaN bits in the plane of z affinities, all bits set in the seam bits), the slab workspace, the resident
labels, the region graph's accumulator and everything the device rounds allocate behind them.

A result that depends on the fill is a read of memory that nothing wrote.
"""

import numpy as np
import pytest
import torch

import watershed_ref
from aind_exaspim_neuron_segmentation_amd import inference
from test_gpu_dbf import dev  # noqa: F401  (fixture)
from test_gpu_poisoned_python import under_every_fill

pytestmark = pytest.mark.gpu

SHAPE = (17, 16, 64)


def affinities(dtype=np.float32):
    return np.ascontiguousarray(watershed_ref.random_affinities("uniform", (17, 17, 65))[:, :, :16, :64]).astype(dtype)


def test_watershed_stream(dev, monkeypatch):      # noqa: F811
    aff = affinities()
    t = torch.from_numpy(aff).to(dev)
    want, k = watershed_ref.fragments(aff, 0.3, 0.7, 3)

    def run():
        ws = inference.WatershedStream(SHAPE, 0.3, 0.7, 3, device=dev)
        parts = [ws.push(t[:, z0:z1]) for z0, z1 in ((0, 8), (8, 9), (9, 17))]
        table, count = ws.finish()
        return torch.cat([ws.apply(p) for p in parts]), table[: ws.ids_used + 1].clone(), np.int64(count)

    def hold(out):
        np.testing.assert_array_equal(out[0].cpu().numpy(), want)
        assert int(out[2]) == k

    under_every_fill(monkeypatch, "WatershedStream", run, hold)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_watershed_fragments_streaming(dev, monkeypatch, dtype):      # noqa: F811
    aff = affinities(dtype)
    want, _ = watershed_ref.fragments(aff, 0.3, 0.7, 0)

    def run():
        return (inference.watershed_fragments_streaming(aff, 0.3, 0.7, slab_depth=5, keep_labels_resident=True),
                inference.watershed_fragments_streaming(aff, 0.3, 0.7, slab_depth=9, keep_labels_resident=False))

    def hold(out):
        for got in out:
            np.testing.assert_array_equal(got, want)

    under_every_fill(monkeypatch, "watershed_fragments_streaming", run, hold, host_result=True)


def test_agglomerate_affinities_streaming_with_device_rounds(dev, monkeypatch):      # noqa: F811
    aff = affinities()
    options = dict(fragments="watershed", aff_threshold_low=0.3, aff_threshold_high=0.7, premerge_size=100,
                   device_merge_rounds=64)
    want = inference.agglomerate_affinities(aff, [0.45], 5, **options)

    def run():
        return inference.agglomerate_affinities_streaming(aff, [0.45], 5, slab_depth=5, **options)

    def hold(out):
        np.testing.assert_array_equal(out, want)

    under_every_fill(monkeypatch, "agglomerate_affinities_streaming", run, hold)
