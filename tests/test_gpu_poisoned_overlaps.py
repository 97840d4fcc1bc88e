"""
label_overlaps, compare_segmentations, OverlapStream and label_overlaps_streaming with torch.empty and numpy.empty
poisoned (-m gpu), in the manner of tests/test_gpu_poisoned_blocks.py: every entry point runs twice under 0x00,
then under 0xFF, 0x7F and 0x01; every returned array must have the bits of the 0x00 run, and the 0xFF run is held
to the oracle of tests/overlaps_ref.py. Inputs are made before the context is entered: only the wrappers' own
allocations are poisoned -- the workspace that holds the table's keys, counts and overflow word until reset has
run, the rows and counts behind row P, and the two state words.

A result that depends on the fill is a read of memory that nothing wrote.
"""

import numpy as np
import pytest

import overlaps_ref
from aind_exaspim_neuron_segmentation_amd import inference
from test_gpu_dbf import dev  # noqa: F401  (fixture)
from test_gpu_poisoned_python import under_every_fill

pytestmark = pytest.mark.gpu


def pair_of_volumes():
    rng = np.random.default_rng(17)
    shape = (9, 19, 70)
    a = overlaps_ref.blocky(rng, shape, 12, 40)
    b = np.where(rng.random(shape) < 0.9, a, overlaps_ref.blocky(rng, shape, 7, 25)).astype(np.int32)
    a[rng.random(shape) < 0.02] = -3
    return a, b


def test_label_overlaps_and_compare_segmentations(dev, monkeypatch):      # noqa: F811
    a, b = pair_of_volumes()
    want = overlaps_ref.table_unique(a, b)
    want_scores = overlaps_ref.scores(*want, "a")

    def run():
        scores = inference.compare_segmentations(a, b)
        numbers = np.array([scores[k] for k in sorted(scores)], dtype=np.float64)
        return inference.label_overlaps(a, b), inference.label_overlaps(a, b, pair_capacity=1 << 10), numbers

    def hold(out):
        for got in out[:2]:
            for g, w in zip(got, want):
                assert g.dtype == w.dtype
                np.testing.assert_array_equal(g, w)
        keys = sorted(want_scores)
        assert out[2][keys.index("n")] == want_scores["n"]
        assert out[2][keys.index("rand_precision")] == float(want_scores["rand_precision"])

    under_every_fill(monkeypatch, "label_overlaps", run, hold)


def test_the_streamed_forms(dev, monkeypatch):      # noqa: F811
    a, b = pair_of_volumes()
    want = overlaps_ref.table_unique(a, b)

    def run():
        stream = inference.OverlapStream(1 << 10)
        stream.add(a[:4], b[:4])
        first = stream.finish()
        stream.add(a[4:], b[4:])
        return first, stream.finish(), inference.label_overlaps_streaming(a, b, slab_depth=2)

    def hold(out):
        for g, w in zip(out[0], overlaps_ref.table_unique(a[:4], b[:4])):
            np.testing.assert_array_equal(g, w)
        for got in out[1:]:
            for g, w in zip(got, want):
                assert g.dtype == w.dtype
                np.testing.assert_array_equal(g, w)

    under_every_fill(monkeypatch, "label_overlaps_streaming", run, hold)
