"""
label_pieces and skeletonize_pieces with torch.empty and numpy.empty poisoned (-m gpu), in the manner of
tests/test_gpu_poisoned_border.py, whose helper this file uses: every entry point runs twice under 0x00, then under
0xFF, 0x7F and 0x01; every returned array must have the bits of the 0x00 run, and the 0xFF run is held to the
oracle of tests/pieces_ref.py. Inputs are made before the context is entered: only the wrappers' own allocations
are poisoned -- the volume of pieces, which holds the union-find's parents first, the two state words, the counts
that become the numbers, the scan's block sums, and everything the chain allocates behind them.

A result that depends on the fill is a read of memory that nothing wrote.
"""

import numpy as np
import pytest

import fix_borders_ref as fx
import pieces_ref
from aind_exaspim_neuron_segmentation_amd import inference
from test_gpu_dbf import dev  # noqa: F401  (fixture)
from test_gpu_poisoned_python import under_every_fill

pytestmark = pytest.mark.gpu


def test_label_pieces(dev, monkeypatch):      # noqa: F811
    labels = pieces_ref.random_volume(42, (9, 19, 70), k=4, fill=0.4)      # tiles that are not whole, one of them empty
    labels[:, 8:16, 32:64] = 0
    assert labels.max() == 5      # random_volume gives -1 .. k + 1: the default K is 5
    want = pieces_ref.flood_fill(labels, 5), pieces_ref.flood_fill(labels, 3, 3)
    assert want[1][4] >= 1

    def run():
        return inference.label_pieces(labels), inference.label_pieces(labels, n_labels=3, dust_threshold=3)

    def hold(out):
        for got, expected in zip(out, want):
            for a, b in zip(got, expected[:4]):
                assert a.dtype == b.dtype
                np.testing.assert_array_equal(a, b)

    under_every_fill(monkeypatch, "label_pieces", run, hold)


def test_skeletonize_pieces(dev, monkeypatch):      # noqa: F811
    labels = np.array(fx.faces_pieces()[0])

    def run():
        return inference.skeletonize_pieces(labels, dust_threshold=2, scale=1.25, const=0.0)

    def hold(out):
        assert sorted(out) == [1, 4] and (out[1][1] == -1).sum() == 2
        pieces = pieces_ref.flood_fill(labels, 4, 2)[0]
        number = pieces[tuple(out[1][0].T)]
        assert set(number.tolist()) == {1, 3} and (np.diff(number) >= 0).all()      # piece 2 is label 4

    under_every_fill(monkeypatch, "skeletonize_pieces", run, hold)
