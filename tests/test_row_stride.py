"""inference.batch_row_stride: which batches of patch starts the engine may treat as one row along x."""
from aind_exaspim_neuron_segmentation_amd import inference

P, O = (96, 96, 96), (32, 32, 32)


def test_a_row_of_patches():
    assert inference.batch_row_stride([(0, 64, 64 * i) for i in range(16)], P, O) == 64
    assert inference.batch_row_stride([(32, 0, 128), (32, 0, 192)], P, O) == 64
    assert inference.batch_row_stride([(0, 0, 0), (0, 0, 32)], (64, 64, 64), (32, 32, 32)) == 32


def test_not_a_row():
    assert inference.batch_row_stride([(0, 0, 0)], P, O) == 0                         # one patch
    assert inference.batch_row_stride([], P, O) == 0
    assert inference.batch_row_stride([(0, 0, 0), (0, 64, 0)], P, O) == 0            # along y
    assert inference.batch_row_stride([(0, 0, 896), (0, 0, 960), (0, 64, 0)], P, O) == 0   # two rows
    assert inference.batch_row_stride([(0, 0, 0), (0, 0, 128)], P, O) == 0           # a gap
    assert inference.batch_row_stride([(0, 0, 64), (0, 0, 0)], P, O) == 0            # descending
    assert inference.batch_row_stride([(0, 0, 0), (0, 0, 64)], P, (32, 32, 96)) == 0  # no stride


def test_the_last_clamped_start_ends_the_row():
    # a start clamped to the volume's end is closer than the stride to its neighbour
    assert inference.batch_row_stride([(0, 0, 0), (0, 0, 64), (0, 0, 100)], P, O) == 0
    assert inference.batch_row_stride([(0, 0, 0), (0, 0, 64)], P, O) == 64


def test_plan_starts_batched_by_rows():
    plan = inference.SlidingWindow((160, 160, 352), P, O, 8)
    starts = plan.starts()
    xs = len(inference._start_ranges((160, 160, 352), P, O)[2])
    assert xs == 5
    rows = [starts[i:i + xs] for i in range(0, len(starts), xs)]
    assert all(inference.batch_row_stride(r, P, O) == 64 for r in rows)
    assert inference.batch_row_stride(starts[3:7], P, O) == 0


def test_sharded_starts():
    from aind_exaspim_neuron_segmentation_amd import sharding

    plan = inference.SlidingWindow((224, 160, 352), P, O, 8)
    for rank in range(2):
        starts = sharding.Shard(plan, (2, 1), rank).starts
        assert starts and len(starts) % 5 == 0
        for i in range(0, len(starts), 5):
            assert inference.batch_row_stride(starts[i:i + 5], P, O) == 64
        assert inference.batch_row_stride(starts[:6], P, O) == 0
