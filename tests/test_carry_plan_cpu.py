"""inference.carry_plan (which later batch takes first-level planes over from which) against a brute-force
search over the patch starts. Host side only."""

import pytest

from aind_exaspim_neuron_segmentation_amd import inference

# (volume, patch, overlap, batch size)
GEOMETRIES = {
    "1024^3 / 96 / 32, batch 16": ((1024, 1024, 1024), (96, 96, 96), (32, 32, 32), 16),
    "ragged last batch": ((224, 96, 352), (96, 96, 96), (32, 32, 32), 5),
    "half rows, batch 8": ((224, 160, 1024), (96, 96, 96), (32, 32, 32), 8),
    "one slab": ((96, 224, 352), (96, 96, 96), (32, 32, 32), 5),
    "unequal overlaps": ((128, 96, 256), (64, 32, 96), (48, 8, 32), 4),
    "rows that straddle batches": ((128, 96, 256), (64, 32, 96), (48, 8, 32), 3),
    "batch of one patch": ((224, 96, 160), (96, 96, 96), (32, 32, 32), 1),
}


def _brute_force(starts, batch_size, patch, overlap):
    batches = [starts[i:i + batch_size] for i in range(0, len(starts), batch_size)]
    stride = [inference.batch_row_stride(b, patch, overlap) for b in batches]
    out = []
    for i, a in enumerate(batches):
        best = None
        for j in range(i + 1, len(batches)):
            b = batches[j]
            if len(a) != len(b) or stride[i] <= 0 or stride[i] != stride[j]:
                continue
            shift = int(b[0][0]) - int(a[0][0])
            if not 0 < shift < patch[0]:
                continue
            if all((int(p[0]) + shift, int(p[1]), int(p[2])) == tuple(int(v) for v in q) for p, q in zip(a, b)):
                if best is None or shift < best[0]:
                    best = (shift, j)
        out.append(None if best is None else best[1])
    return out


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_carry_plan_is_the_brute_force_search(name):
    shape, patch, overlap, batch_size = GEOMETRIES[name]
    starts = list(inference.generate_patch_starts((1, 1) + shape, patch, overlap))
    got = inference.carry_plan(starts, batch_size, patch, overlap)
    assert got == _brute_force(starts, batch_size, patch, overlap)
    n_batches = -(-len(starts) // batch_size)
    assert len(got) == n_batches
    assert all(s is None or s > i for i, s in enumerate(got))
    linked = [s for s in got if s is not None]
    assert len(linked) == len(set(linked)), "a batch has two predecessors"


def test_bench_geometry_counts():
    shape, patch, overlap, batch_size = GEOMETRIES["1024^3 / 96 / 32, batch 16"]
    starts = list(inference.generate_patch_starts((1, 1) + shape, patch, overlap))
    got = inference.carry_plan(starts, batch_size, patch, overlap)
    assert len(got) == 256 and sum(s is not None for s in got) == 240
    has_pred = set(s for s in got if s is not None)
    assert not any(b in has_pred for b in range(16)), "a batch of the first slab has a predecessor"
    assert all(s == i + 16 for i, s in enumerate(got) if s is not None)


def test_special_cases():
    shape, patch, overlap, batch_size = GEOMETRIES["one slab"]
    starts = list(inference.generate_patch_starts((1, 1) + shape, patch, overlap))
    assert set(inference.carry_plan(starts, batch_size, patch, overlap)) == {None}
    shape, patch, overlap, batch_size = GEOMETRIES["batch of one patch"]
    starts = list(inference.generate_patch_starts((1, 1) + shape, patch, overlap))
    assert set(inference.carry_plan(starts, batch_size, patch, overlap)) == {None}    # one patch is no row
    shape, patch, overlap, batch_size = GEOMETRIES["ragged last batch"]
    starts = list(inference.generate_patch_starts((1, 1) + shape, patch, overlap))
    got = inference.carry_plan(starts, batch_size, patch, overlap)
    assert any(s is not None for s in got)
    shape, patch, overlap, batch_size = GEOMETRIES["unequal overlaps"]
    starts = list(inference.generate_patch_starts((1, 1) + shape, patch, overlap))
    got = inference.carry_plan(starts, batch_size, patch, overlap)
    # z stride 16 under a depth of 64: the nearest of three qualifying batches is taken
    z = [int(starts[i * batch_size][0]) for i in range(len(got))]
    assert all(z[s] - z[i] == 16 for i, s in enumerate(got) if s is not None) and any(s is not None for s in got)
    assert inference.carry_plan([], 4, patch, overlap) == []
