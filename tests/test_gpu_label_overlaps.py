"""
exaspim_label_overlaps* on the device against the packed-numpy.unique oracle of tests/overlaps_ref.py, bit for bit
after sorting (-m gpu). Direct C calls go into poisoned buffers with guard words behind each, as
test_gpu_region_graph.py's Call does: shapes and alignments around the chunk, run patterns, the keys at the ends of
the range, a table that ends exactly full and one that overflows by one pair, a launch beyond the grid cap,
accumulation over several adds; then the Python layer: label_overlaps, compare_segmentations, OverlapStream and
label_overlaps_streaming.
"""

import os
import re

import numpy as np
import pytest
import torch

import label_symmetry
import overlaps_ref
from aind_exaspim_neuron_segmentation_amd import _native, inference
from test_gpu_dbf import dev  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

GUARD = 64
SLACK = 8      # int32 in front of and behind every input, poisoned with labels the output must not show
POISON_LABEL = 1234567


def constants():
    """The add kernel's constants, read from its source: voxels per chunk, the grid cap, the LDS slots."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "aind_exaspim_neuron_segmentation_amd", "csrc", "overlaps.hip")).read()
    rounds = int(re.search(r"constexpr int kOvRounds = (\d+);", text).group(1))
    assert re.search(r"constexpr int kOvChunk = 4 \* kThreads \* kOvRounds;", text)
    cap = int(re.search(r"constexpr unsigned kOvMaxGrid = (\d+);", text).group(1))
    slots = int(re.search(r"constexpr int kOvSlots = (\d+);", text).group(1))
    return 4 * 256 * rounds, cap, slots


C, GRID_CAP, LDS_SLOTS = constants()


class Table:
    """One table in a poisoned workspace, and poisoned outputs, each with GUARD words behind it."""

    def __init__(self, dev, capacity):      # noqa: F811
        self.dev, self.capacity = dev, int(capacity)
        self.lib = _native.lib()
        self.need = self.lib.exaspim_label_overlaps_workspace_bytes(self.capacity)
        assert self.need >= 16 * self.capacity, _native.last_error()
        c = self.capacity
        self.ws = torch.full((self.need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.pairs = torch.full((2 * c + GUARD,), -1234567, dtype=torch.int32, device=dev)
        self.counts = torch.full((c + GUARD,), -7654321, dtype=torch.int64, device=dev)
        self.state = torch.full((2 + GUARD,), -3333333, dtype=torch.int32, device=dev)
        self.kept = []      # the inputs stay alive until the table is read

    def upload(self, values, offset):
        """values behind "offset" int32 of a 16-byte aligned buffer, poisoned labels around them: its pointer."""
        values = np.ascontiguousarray(values, dtype=np.int32).ravel()
        host = np.full(offset + values.size + SLACK, POISON_LABEL, dtype=np.int32)
        host[offset:offset + values.size] = values
        t = torch.from_numpy(host).to(self.dev)
        assert t.data_ptr() % 16 == 0
        self.kept.append(t)
        return t.data_ptr() + 4 * offset

    def reset(self):
        assert self.lib.exaspim_label_overlaps_reset(self.capacity, self.ws.data_ptr(), self.need, None) == 0

    def add(self, a, b, offset_a=0, offset_b=0):
        n = int(np.asarray(a).size)
        assert np.asarray(b).size == n
        rc = self.lib.exaspim_label_overlaps_add(self.upload(a, offset_a), self.upload(b, offset_b), n,
                                                 self.capacity, self.ws.data_ptr(), self.need, None)
        assert rc == 0, _native.last_error()

    def finish(self):
        rc = self.lib.exaspim_label_overlaps_finish(self.capacity, self.ws.data_ptr(), self.need,
                                                    self.pairs.data_ptr(), self.counts.data_ptr(),
                                                    self.state.data_ptr(), None)
        assert rc == 0, _native.last_error()
        return self.result()

    def whole(self, a, b, offset_a=0, offset_b=0):
        n = int(np.asarray(a).size)
        rc = self.lib.exaspim_label_overlaps(self.upload(a, offset_a), self.upload(b, offset_b), n, self.capacity,
                                             self.pairs.data_ptr(), self.counts.data_ptr(), self.state.data_ptr(),
                                             self.ws.data_ptr(), self.need, None)
        assert rc == 0, _native.last_error()
        return self.result()

    def guards_intact(self):
        c = self.capacity
        return bool((self.pairs[2 * c:] == -1234567).all() and (self.counts[c:] == -7654321).all()
                    and (self.state[2:] == -3333333).all() and (self.ws[self.need:] == 0xA5).all())

    def result(self):
        """((pairs, counts) sorted by (a', b'), the overflow flag); what lies behind row P is still poison."""
        torch.cuda.synchronize()
        assert self.guards_intact()
        n_pairs, overflow = (int(v) for v in self.state[:2].cpu())
        assert 0 <= n_pairs <= self.capacity and overflow in (0, 1)
        assert bool((self.pairs[2 * n_pairs:] == -1234567).all() and (self.counts[n_pairs:] == -7654321).all())
        pairs = self.pairs[:2 * n_pairs].cpu().numpy().reshape(-1, 2)
        counts = self.counts[:n_pairs].cpu().numpy()
        order = np.lexsort((pairs[:, 1], pairs[:, 0]))
        return (pairs[order], counts[order]), overflow


def assert_same(got, want):
    for g, w, name in zip(got, want, ("pairs", "counts")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=name)


def capacity_for(pairs):
    return max(16, 1 << (2 * int(pairs) - 1).bit_length())


def check(dev, a, b, offset_a=0, offset_b=0, capacity=None):      # noqa: F811
    want = overlaps_ref.table_unique(a, b)
    table = Table(dev, capacity or capacity_for(len(want[1])))
    got, overflow = table.whole(a, b, offset_a, offset_b)
    assert overflow == 0
    assert_same(got, want)
    assert int(got[1].sum()) == np.asarray(a).size
    return want


def runs(rng, n, longest, top):
    """n labels 1 .. top in runs of random lengths up to "longest"."""
    lengths = rng.integers(1, longest + 1, size=n)
    return np.repeat(rng.integers(1, top + 1, size=n), lengths)[:n].astype(np.int32)


SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_quad_the_wave_and_the_chunk_at_every_alignment(dev, n):      # noqa: F811
    """a and b start 0 .. 3 int32 behind a 16-byte boundary, independently: whole quads of both, whole quads of a
    with b read one by one, and the partial quads at both ends. The poisoned labels around the inputs must not
    show up: no voxel outside [0, n) is read into the table."""
    rng = np.random.default_rng(n)
    a, b = runs(rng, n, 9, 5), runs(rng, n, 7, 4)
    want = overlaps_ref.table_unique(a, b)
    assert not (want[0] == POISON_LABEL).any()
    for offset_a in range(4):
        for offset_b in range(4):
            table = Table(dev, 64)
            got, overflow = table.whole(a, b, offset_a, offset_b)
            assert overflow == 0, (offset_a, offset_b)
            assert_same(got, want)


def test_one_constant_pair_over_several_chunks(dev):      # noqa: F811
    n = 5 * C + 17
    a, b = np.full(n, 7, dtype=np.int32), np.full(n, 9, dtype=np.int32)
    (pairs, counts), _ = check(dev, a, b), None
    assert pairs.tolist() == [[7, 9]] and counts.tolist() == [n]


def test_every_voxel_its_own_pair_overflows_the_workgroups_table(dev):      # noqa: F811
    """Three chunks of distinct pairs: C > the LDS table's slots, so most contributions take the direct path."""
    n = 3 * C
    assert C > LDS_SLOTS
    a = np.arange(1, n + 1, dtype=np.int32)
    b = (np.arange(n, dtype=np.int32) % 5) + 1
    pairs, counts = check(dev, a, b)
    assert len(counts) == n and (counts == 1).all()


def test_run_lengths_cycling_through_one_to_two_hundred(dev):      # noqa: F811
    """Runs that start and end at every position of a lane's quad, of a wave and of a chunk."""
    lengths = np.tile(np.arange(1, 201), 3)
    ids = (np.arange(len(lengths)) % 11 + 1).astype(np.int32)
    a = np.repeat(ids, lengths)
    assert a.size > 2 * C + C // 2
    b = np.repeat((np.arange(len(lengths)) % 3 + 1).astype(np.int32), lengths)
    for offset in (0, 1):
        check(dev, a, b, offset, offset)


def test_runs_of_a_and_b_that_change_at_different_places(dev):      # noqa: F811
    n = 2 * C + 100
    a = (np.arange(n) // 37 % 6 + 1).astype(np.int32)
    b = ((np.arange(n) + 11) // 53 % 4 + 1).astype(np.int32)
    assert ((np.diff(a) != 0) & (np.diff(b) != 0)).sum() < ((np.diff(a) != 0) | (np.diff(b) != 0)).sum()
    check(dev, a, b)
    check(dev, a, b, 2, 3)


def test_the_pair_is_ordered(dev):      # noqa: F811
    a = np.array([1] * 10 + [2] * 7 + [1] * 3, dtype=np.int32)
    b = np.array([2] * 10 + [1] * 7 + [1] * 3, dtype=np.int32)
    pairs, counts = check(dev, a, b)
    assert pairs.tolist() == [[1, 1], [1, 2], [2, 1]] and counts.tolist() == [3, 10, 7]


def test_everything_at_or_below_zero_is_background_and_the_largest_label_is_a_label(dev):      # noqa: F811
    low, top = overlaps_ref.INT32_MIN, overlaps_ref.INT32_MAX
    a = np.array([0, -1, low, -5, top, top, top, 3, low, top], dtype=np.int32)
    b = np.array([-7, 0, low, 4, top, top, -1, top, 5, low], dtype=np.int32)
    pairs, counts = check(dev, a, b)
    assert pairs.tolist() == [[0, 0], [0, 4], [0, 5], [3, top], [top, 0], [top, top]]
    assert counts.tolist() == [3, 1, 1, 1, 2, 2]
    # whole quads of the largest pair: its key is not the empty key, and every voxel is counted
    n = C + 8
    pairs, counts = check(dev, np.full(n, top, dtype=np.int32), np.full(n, top, dtype=np.int32))
    assert pairs.tolist() == [[top, top]] and counts.tolist() == [n]


def test_ids_spaced_by_the_workgroup_tables_size(dev):      # noqa: F811
    """label_symmetry's L -> 2048 (L - 1) + 1 on both volumes."""
    assert label_symmetry.LDS_SLOTS == LDS_SLOTS
    rng = np.random.default_rng(3)
    n = 2 * C + 5
    a, b = runs(rng, n, 6, 300), runs(rng, n, 8, 200)
    spaced = label_symmetry.label_maps(300, 0)["one_home_slot"]
    want = check(dev, spaced[a], spaced[b])
    plain = overlaps_ref.table_unique(a, b)
    np.testing.assert_array_equal(want[1], plain[1])      # the same rows under the monotone renaming
    np.testing.assert_array_equal(want[0], spaced[plain[0]])


def test_a_table_that_ends_exactly_full(dev):      # noqa: F811
    capacity = 256
    a = np.repeat(np.arange(1, capacity + 1, dtype=np.int32), 3)
    b = np.ones_like(a)
    table = Table(dev, capacity)
    got, overflow = table.whole(a, b)
    assert overflow == 0 and len(got[1]) == capacity
    assert_same(got, overlaps_ref.table_unique(a, b))


def test_one_pair_more_than_the_capacity(dev):      # noqa: F811
    capacity = 256
    a = np.repeat(np.arange(1, capacity + 2, dtype=np.int32), 3)
    b = np.ones_like(a)
    table = Table(dev, capacity)
    (pairs, counts), overflow = table.whole(a, b)      # result() checks the guards and what lies behind row P
    assert overflow == 1 and len(counts) <= capacity
    assert int(counts.sum()) < a.size and (counts > 0).all()
    with pytest.raises(RuntimeError, match="larger pair_capacity"):
        inference.label_overlaps(a.reshape(1, 1, -1), b.reshape(1, 1, -1), pair_capacity=capacity)


def test_a_launch_beyond_the_grid_cap(dev):      # noqa: F811
    """More than twice the voxels one capped launch covers in one pass: every workgroup strides at least twice
    more. The labels vary along the range, so a chunk that is skipped or taken twice changes the table."""
    n = 2 * GRID_CAP * C + C + 5
    assert n > 2 * GRID_CAP * C and (n + C - 1) // C > 2 * GRID_CAP
    i = np.arange(n, dtype=np.int64)
    a = (i // 3001 + 1).astype(np.int32)
    b = (i // 7919 % 97 + 1).astype(np.int32)
    want = overlaps_ref.table_unique(a, b)
    assert len(want[1]) > n // 3001
    table = Table(dev, capacity_for(len(want[1])))
    got, overflow = table.whole(a, b, 1, 1)
    assert overflow == 0
    assert_same(got, want)


def test_accumulation_over_several_adds(dev):      # noqa: F811
    rng = np.random.default_rng(11)
    x = (runs(rng, C + 77, 9, 6), runs(rng, C + 77, 5, 7))
    y = (runs(rng, 301, 4, 9), runs(rng, 301, 30, 3))
    z = (runs(rng, 2 * C, 12, 5), runs(rng, 2 * C, 3, 11))
    table = Table(dev, 1024)
    table.reset()
    table.add(*x, 0, 0)
    table.add(*y, 3, 1)
    got, overflow = table.finish()
    want = overlaps_ref.table_unique(np.concatenate([x[0], y[0]]), np.concatenate([x[1], y[1]]))
    assert overflow == 0
    assert_same(got, want)
    again, overflow = table.finish()      # finish only reads the table
    assert overflow == 0
    assert_same(again, want)
    # n = 0 launches nothing and changes nothing: the pointers are not followed
    before = table.ws[:table.need].clone()
    assert table.lib.exaspim_label_overlaps_add(0x1000, 0x2000, 0, table.capacity, table.ws.data_ptr(), table.need,
                                                None) == 0
    torch.cuda.synchronize()
    assert torch.equal(before, table.ws[:table.need])
    table.add(*z, 2, 2)
    got, overflow = table.finish()
    assert overflow == 0
    assert_same(got, overlaps_ref.table_unique(np.concatenate([x[0], y[0], z[0]]),
                                               np.concatenate([x[1], y[1], z[1]])))
    # the whole call is reset + add + finish
    one = Table(dev, 1024)
    got, overflow = one.whole(*x)
    assert overflow == 0
    assert_same(got, overlaps_ref.table_unique(*x))


# ---- the Python layer --------------------------------------------------------------------------------------------
SHAPE = (20, 9, 33)
_VOLUMES = {}


def volumes():
    """(a, b) of SHAPE, read-only: a made by affinities_to_components, b its premerge-like perturbation (the
    smallest segments given to a neighbour in id, a few voxels to the background)."""
    if not _VOLUMES:
        aff, threshold = label_symmetry.component_affinities(SHAPE, 5)
        a = inference.affinities_to_components(np.ascontiguousarray(aff), threshold, 0)
        assert a.dtype == np.int32 and a.max() >= 8
        sizes = np.bincount(a.ravel())
        table = np.arange(len(sizes), dtype=np.int32)
        small = [l for l in np.argsort(sizes) if l > 0][:len(sizes) // 3]
        table[small] = [l + 1 if l + 1 < len(sizes) else l - 1 for l in small]
        b = table[a]
        b[np.random.default_rng(2).random(SHAPE) < 0.02] = 0
        a.setflags(write=False)
        b.setflags(write=False)
        _VOLUMES["ab"] = (a, b, overlaps_ref.table_unique(a, b))
    return _VOLUMES["ab"]


def test_label_overlaps_on_numpy_and_on_device_inputs(dev):      # noqa: F811
    a, b, want = volumes()
    assert_same(inference.label_overlaps(a, b), want)
    assert_same(inference.label_overlaps(a, b), want)      # two runs give identical arrays
    a_dev, b_dev = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    assert_same(inference.label_overlaps(a_dev, b_dev, pair_capacity=1 << 12), want)
    pairs, counts = inference.label_overlaps(a_dev, b_dev, return_device_tensors=True)
    assert pairs.device == counts.device == a_dev.device and pairs.dtype == torch.int32 and counts.dtype == torch.int64
    pairs, counts = pairs.cpu().numpy(), counts.cpu().numpy()
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    assert_same((pairs[order], counts[order]), want)
    # a slice that starts 4 bytes behind a 16-byte boundary, as it is
    flat_a, flat_b = a_dev.reshape(-1)[1:1 + 19 * 9 * 33].reshape(19, 9, 33), b_dev.reshape(-1)[:19 * 9 * 33]
    assert flat_a.data_ptr() % 16 == 4 and flat_a.is_contiguous()
    assert_same(inference.label_overlaps(flat_a, flat_b.reshape(19, 9, 33)),
                overlaps_ref.table_unique(a.ravel()[1:1 + 19 * 9 * 33], b.ravel()[:19 * 9 * 33]))


@pytest.mark.parametrize("background", ["a", "both_zero", "none"])
def test_compare_segmentations_against_the_second_writing(dev, background):      # noqa: F811
    from test_overlaps_ref_cpu import assert_scores

    a, b, want = volumes()
    assert_scores(inference.compare_segmentations(a, b, background=background),
                  overlaps_ref.scores(*want, background))
    assert_scores(inference.compare_segmentations(a, a, background=background),
                  overlaps_ref.scores(*overlaps_ref.table_unique(a, a), background))


def test_same_partition_under_a_renaming_and_not_after_one_voxel_moves(dev):      # noqa: F811
    a, _, _ = volumes()
    renamed = label_symmetry.relabel_volume(a, label_symmetry.label_maps(int(a.max()), 4)["sparse"])
    for background in ("a", "both_zero", "none"):
        got = inference.compare_segmentations(a, renamed, background=background)
        assert got["same_partition"] is True and got["voi"] == 0.0 and got["adapted_rand_error"] == 0.0
    moved = renamed.copy()
    sizes = np.bincount(a.ravel())
    sizes[0] = 0
    assert sizes.max() >= 2      # the voxel leaves a segment that goes on without it
    z, y, x = (int(v[0]) for v in np.nonzero(a == sizes.argmax()))
    moved[z, y, x] = int(renamed.max()) + 1
    for background in ("a", "both_zero", "none"):
        got = inference.compare_segmentations(a, moved, background=background)
        assert got["same_partition"] is False and got["voi"] > 0.0


@pytest.mark.parametrize("slab_depth", [1, 3, 7, 20])
def test_the_streamed_forms_equal_the_whole_volume(dev, slab_depth):      # noqa: F811
    a, b, want = volumes()
    assert_same(inference.label_overlaps_streaming(a, b, slab_depth=slab_depth), want)
    stream = inference.OverlapStream(1 << 12)
    a_dev, b_dev = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    for z0 in range(0, SHAPE[0], slab_depth):      # device slabs as they are sliced, numpy slabs in turn
        if (z0 // slab_depth) % 2:
            stream.add(a[z0:z0 + slab_depth], b[z0:z0 + slab_depth])
        else:
            stream.add(a_dev[z0:z0 + slab_depth], b_dev[z0:z0 + slab_depth])
    assert stream.voxels == a.size
    assert_same(stream.finish(), want)
    assert_same(stream.finish(), want)


def test_streaming_from_a_memmap(dev, tmp_path):      # noqa: F811
    a, b, want = volumes()
    maps = []
    for name, v in (("a", a), ("b", b)):
        m = np.memmap(tmp_path / f"{name}.bin", dtype=np.int32, mode="w+", shape=SHAPE)
        m[:] = v
        m.flush()
        maps.append(np.memmap(tmp_path / f"{name}.bin", dtype=np.int32, mode="r", shape=SHAPE))
    assert_same(inference.label_overlaps_streaming(*maps, slab_depth=3), want)
