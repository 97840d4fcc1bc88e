"""The cases of test_gpu_window_fuzz.py and what the host model of the carry rule (carry_ref.py) plans for them.
No device: test_window_fuzz_cases_cpu.py holds the committed list to the conditions that make it worth running."""

import os

import numpy as np

from aind_exaspim_neuron_segmentation_amd import inference
from carry_ref import _RowModel, row_mode

MAX_PATCHES, MAX_PATCH_VOXELS = 48, 5_000_000
# EXASPIM_FUZZ_WINDOW_CASES / EXASPIM_FUZZ_SEED widen the hunt by hand; the committed run is 12 generated cases
COMMITTED_CASES, COMMITTED_SEED = 12, 136
N_CASES = int(os.environ.get("EXASPIM_FUZZ_WINDOW_CASES", str(COMMITTED_CASES)))
SEED = int(os.environ.get("EXASPIM_FUZZ_SEED", str(COMMITTED_SEED)))

# Planned on the host; what each is for is what test_window_fuzz_cases_cpu.py asserts of it
HAND = [
    dict(shape=(120, 72, 96), patch=(48, 32, 64), overlap=(24, 8, 32), trim=4, batch=2),
    dict(shape=(120, 72, 160), patch=(48, 32, 64), overlap=(24, 8, 32), trim=4, batch=3),
    dict(shape=(112, 56, 96), patch=(48, 32, 64), overlap=(32, 8, 32), trim=4, batch=2),
    dict(shape=(64, 24, 96), patch=(32, 16, 64), overlap=(16, 8, 32), trim=4, batch=2),
    dict(shape=(120, 72, 96), patch=(48, 32, 64), overlap=(24, 8, 32), trim=4, batch=4),
    # rows of three patches that overlap by 16 along x: rows to carry_plan, but the engine runs no row mode
    dict(shape=(120, 32, 150), patch=(48, 32, 64), overlap=(24, 8, 16), trim=4, batch=3),
]


def _axis(rng, n, patch, overlap, ragged):
    """A length with exactly n patch starts (range(0, dim - overlap, stride)): the last patch fits exactly, or
    reaches 1 .. stride - 1 voxels beyond the volume, which it then reflects."""
    stride = patch - overlap
    r = int(rng.integers(1, stride)) if ragged else 0
    return n * stride + overlap - r


def generated(n, seed):
    rng = np.random.default_rng(seed)
    pick = lambda options: options[int(rng.integers(0, len(options)))]   # noqa: E731
    out = []
    for i in range(n):
        patch = (pick((32, 48, 48, 64)), pick((16, 32)), pick((64, 64, 96)))
        # even z shifts: around half the depth, and under a third of it, where a batch would have to pass on
        # planes it takes over itself and the chain is cut
        shift = pick({32: (16, 16, 8, 12, 24), 48: (24, 24, 16, 12, 20, 32), 64: (32, 32, 16, 24, 20, 40)}[patch[0]])
        overlap = (patch[0] - shift, pick((8, 8, 12, patch[1] // 2)), 32 if rng.random() < 0.8 else 16)
        counts = [int(rng.integers(2, 5)), int(rng.integers(1, 4)), int(rng.integers(2, 5))]
        while (np.prod(counts) > MAX_PATCHES or np.prod(counts) * np.prod(patch) > MAX_PATCH_VOXELS):
            axis = int(np.argmax([c - lo for c, lo in zip(counts, (2, 1, 2))]))
            counts[axis] -= 1
        shape = tuple(_axis(rng, c, p, o, rng.random() < 0.7) for c, p, o in zip(counts, patch, overlap))
        row = counts[2]
        u = rng.random()
        if u < 0.5:
            batch = row
        elif u < 0.65:
            batch = max(d for d in range(1, row) if row % d == 0)
        elif u < 0.8:
            batch = row + 1
        else:
            batch = 2 * row
        out.append(dict(shape=shape, patch=patch, overlap=overlap, trim=pick((0, 2, 4, 4)), batch=batch,
                        seed=300 + i))
    return out


def cases(n=N_CASES, seed=SEED):
    """The generated cases, then the hand-written ones."""
    return generated(n, seed) + [dict(c, seed=400 + i) for i, c in enumerate(HAND)]


def case_id(case):
    return "{}-p{}-o{}-t{}-b{}".format(*("x".join(map(str, case[k])) for k in ("shape", "patch", "overlap")),
                                        case["trim"], case["batch"])


def plan(case, model=None, n_streams=1):
    """What inference plans for a case with every switch on and no memory bound: the batches, carry_plan's
    successors and _carry_schedule's (links, peak, level1) for `model` (default: the host model of the engine)."""
    model = _RowModel() if model is None else model
    shape, patch, overlap, batch = case["shape"], case["patch"], case["overlap"], case["batch"]
    starts = list(inference.generate_patch_starts((1, 1) + tuple(shape), patch, overlap))
    succ = inference.carry_plan(starts, batch, patch, overlap)
    links, peak, level1 = inference._carry_schedule(model, succ, starts, batch, patch, overlap, n_streams, None,
                                                    free=1 << 60)
    batches = [starts[i:i + batch] for i in range(0, len(starts), batch)]
    return dict(starts=starts, batches=batches, succ=succ, links=links or [None] * len(batches), peak=peak,
                level1=level1)


def traits(case, model=None):
    """The properties of a case's plan that test_window_fuzz_cases_cpu.py counts."""
    model = _RowModel() if model is None else model
    p = plan(case, model)
    patch, overlap, trim, shape = case["patch"], case["overlap"], case["trim"], case["shape"]
    links, batches = p["links"], p["batches"]
    rows = [getattr(model, "row_mode", row_mode)(len(b), patch[2], inference.batch_row_stride(b, patch, overlap))
            for b in batches]
    clipped = [inference.batch_keep_hi(b, patch, trim, shape) is not None for b in batches]

    def could_carry(bi, bj):
        b = batches[bi]
        span = model.carry_planes((len(b),) + tuple(patch), inference.batch_row_stride(b, patch, overlap),
                                  int(batches[bj][0][0]) - int(b[0][0]))
        return span[1] > span[0]

    return dict(
        patches=len(p["starts"]), batches=len(batches), rows=sum(rows),
        links=sum(l is not None for l in links),
        far=sum(l is not None and l[0] - bi > 1 for bi, l in enumerate(links)),
        level1=sum(l is not None and l[3][1] > l[3][0] for l in links),
        cuts=sum(l is None and bj is not None and could_carry(bi, bj)
                 for bi, (l, bj) in enumerate(zip(links, p["succ"]))),
        clipped_links=sum(l is not None and (clipped[bi] or clipped[l[0]]) for bi, l in enumerate(links)),
        mixed=0 < sum(rows) < len(rows),
        distances=sorted({l[0] - bi for bi, l in enumerate(links) if l is not None}),
    )
