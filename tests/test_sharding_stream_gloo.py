"""
sharding.predict_shard_streaming on CPU (gloo, world sizes 1, 2, 4 and 8 = the 4 x 2 grid):
reader -> rank blocks -> sink. The device steps (upload, histogram, gather + network + stitch
of a patch layer, the final division, the download pipeline) are replaced by numpy restatements
through the function's own `ops` hook; the schedule under test is the product's: which boxes
of the image a rank reads, the rolling input slab, the one-layer accumulators, the parked
z-band planes, the per-slab y exchange, the z exchange at the end, the boxes handed to the sink.

The assembled result must equal predict_shard's whole-accumulator route (accumulate everything,
exchange_output_bands, divide) BIT FOR BIT, with float patch outputs whose sums depend on the
order of the additions.

The loop is inference.run_slab_pipeline, the one predict_streaming and predict_components_streaming
run on the 1 x 1 grid of a whole volume; the cases at the end drive it the way they do: the slab
cuts a sink sees, the label sink, a volume no patch fits into, the read_block(z0, z1) adapter.
"""

import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from aind_exaspim_neuron_segmentation_amd import inference, sharding
from aind_exaspim_neuron_segmentation_amd.utils import img_util, synthetic

PATCH, TRIM, CHANNELS = (32, 32, 32), 4, 3
GEOMETRIES = {
    # overlap 16: stride 16, 8-voxel bands cross every rank face (and corners are forwarded)
    "bands": ((104, 88, 56), (16, 16, 16)),
    # overlap 8: trimmed outputs tile exactly, nothing crosses a face (empty band boxes)
    "tiling": ((104, 88, 56), (8, 8, 8)),
    # overlap 4 < trim... not allowed by the window; overlap 24: band 16 = two layers deep
    "deep": ((136, 72, 40), (24, 24, 24)),
}


def fake_patch_output(start):
    """Deterministic float stand-in for sigmoid(model(patch)), keyed by the patch start."""
    seed = (start[0] * 1000 + start[1]) * 1000 + start[2]
    u = synthetic._uniform01("patch", CHANNELS * int(np.prod(PATCH)), seed)
    return u.astype(np.float32).reshape((CHANNELS,) + PATCH)


def add_patch(accum, origin, start, gshape):
    """numpy restatement of exaspim_stitch_accumulate for one patch on a block at "origin"."""
    out = [p - 2 * TRIM for p in PATCH]
    pred = fake_patch_output(start)
    s0 = [si + TRIM for si in start]
    e = [min(a + o, d) for a, o, d in zip(s0, out, gshape)]
    dst = tuple(slice(a - o, b - o) for a, b, o in zip(s0, e, origin))
    src = tuple(slice(TRIM, TRIM + b - a) for a, b in zip(s0, e))
    accum[(slice(None),) + dst] += pred[(slice(None),) + src]


def weights(plan):
    wgt = np.zeros(plan.shape, np.float32)
    out = [p - 2 * TRIM for p in PATCH]
    for s in plan.starts():
        s0 = [si + TRIM for si in s]
        e = [min(a + o, d) for a, o, d in zip(s0, out, plan.shape)]
        wgt[tuple(slice(a, b) for a, b in zip(s0, e))] += 1
    return wgt


class SyncDrain:
    """The download pipeline without a device: fill, then run the consumers at once."""

    def __init__(self, label_elems=0):
        self.label_slot = torch.empty(label_elems, dtype=torch.int32)

    def emit(self, shape, fill, consumers, label=None):
        out = torch.zeros(shape, dtype=torch.float32)
        fill(out)
        if label is not None:
            out = label(out, self.label_slot)
            if out is None:
                return
        for job in consumers(out.numpy()):
            job()

    def drain(self):
        pass

    def close(self):
        pass


class NumpyShardOps:
    """numpy restatements of DeviceShardOps' steps; also checks what the schedule feeds them."""

    device = torch.device("cpu")

    def __init__(self, plan, shard, gvol, slab_planes):
        self.plan, self.shard, self.gvol = plan, shard, gvol
        self.wgt = weights(plan)
        self.slab_planes = slab_planes
        self.read_voxels = 0

    def storage(self, src_dtype):
        assert np.dtype(src_dtype) == np.uint16
        return np.dtype(np.uint16), lambda block: block

    def upload(self, block, convert):
        self.read_voxels += int(block.size)
        return torch.from_numpy(np.ascontiguousarray(convert(block)).astype(np.int32))

    def empty_voxels(self, dims, vdtype):
        return torch.full(tuple(dims), -1, dtype=torch.int32)

    def effective_clip(self, src_dtype, vdtype):
        return np.uint16(1000), np.dtype(np.uint16)

    def histogram_into(self, hist, voxels, vdtype, clip, pass_index, prefix):
        v = np.minimum(voxels.numpy(), int(clip)).ravel()
        assert v.min() >= 0
        hist += torch.from_numpy(np.bincount(v, minlength=65536))

    def percentiles(self, histogram, vdtype, percentiles, value_dtype, clip):
        stats = img_util.OrderStatistics(histogram(), lambda b: np.uint16(b))
        return img_util.percentiles_from_statistics(stats, percentiles, np.uint16)

    def run_layer(self, voxels, vox_origin, src_dtype, vdtype, starts, accum, accum_origin, mn, mx, pbar=None):
        g = self.plan.shape
        for s in starts:
            # every voxel the patch reads lies inside what the schedule put on the "device", and
            # holds the global volume's value there
            lo = tuple(s)
            hi = tuple(min(a + p, d) for a, p, d in zip(s, PATCH, g))
            loc = tuple(slice(a - o, b - o) for a, b, o in zip(lo, hi, vox_origin))
            assert all(sl.start >= 0 and sl.stop <= n for sl, n in zip(loc, voxels.shape)), (s, vox_origin)
            np.testing.assert_array_equal(voxels[loc].numpy(), self.gvol[tuple(slice(a, b) for a, b in zip(lo, hi))])
            add_patch(accum.numpy(), accum_origin, s, g)

    def finalize(self, out, origin):
        sl = tuple(slice(o, o + n) for o, n in zip(origin, out.shape[1:]))
        w = self.wgt[sl]
        np.divide(out.numpy(), w, out=out.numpy(), where=w != 0)

    def zeros(self, shape):
        return torch.zeros(tuple(shape), dtype=torch.float32)

    def empty(self, shape):
        return torch.full(tuple(shape), float("nan"), dtype=torch.float32)

    def slab_bytes_cap(self):
        g = self.plan.shape
        return self.slab_planes * CHANNELS * g[1] * g[2] * 4

    def make_drain(self, slot_elems, threads, label_elems=0):
        return SyncDrain(label_elems)

    def synchronize(self):
        pass


def reference_route(plan, shard, group):
    """predict_shard's route on the CPU: whole accumulator, exchange_output_bands, divide."""
    accum = np.zeros((CHANNELS,) + shard.accum_dims, np.float32)
    for s in shard.starts:
        add_patch(accum, shard.accum_origin, s, plan.shape)
    accum_t = torch.from_numpy(accum)
    if group is not None:
        sharding.exchange_output_bands(accum_t, shard, group)
    own = sharding.owned_result(accum_t, shard).numpy().copy()
    w = weights(plan)[tuple(slice(a, b) for a, b in zip(shard.own_lo, shard.own_hi))]
    np.divide(own, w, out=own, where=w != 0)
    return own


def run_rank(rank, world, geometry, resident, slab_planes):
    gshape, overlap = GEOMETRIES[geometry]
    group = dist.group.WORLD if world > 1 else None
    plan = inference.SlidingWindow(gshape, PATCH, overlap, TRIM)
    shard = sharding.Shard(plan, sharding.rank_grid(world), rank)
    gvol = synthetic.synth_volume(gshape, seed=3)
    want = reference_route(plan, shard, group)

    # (a) array-like source, whole region returned
    ops = NumpyShardOps(plan, shard, gvol, slab_planes)
    got = sharding.predict_shard_streaming(gvol, None, plan, shard, group=group, ops=ops,
                                           keep_input_resident=resident)
    assert got.shape == want.shape and got.dtype == np.float32
    np.testing.assert_array_equal(got, want)
    # the rank read its own block only: sub-volume once for the histogram + block once for the
    # patches (resident: the block once)
    core, block = int(np.prod(shard.core_dims)), int(np.prod(shard.input_dims))
    assert ops.read_voxels <= (block if resident else core + block * 2), (ops.read_voxels, core, block)

    # (b) read_box function + write_block sink: boxes tile the region exactly once
    requested = []

    def read_box(lo, hi):
        requested.append((lo, hi))
        in_lo = shard.input_origin
        in_hi = tuple(o + d for o, d in zip(in_lo, shard.input_dims))
        assert all(a >= l and b <= h for a, b, l, h in zip(lo, hi, in_lo, in_hi)), (lo, hi, in_lo, in_hi)
        return gvol[tuple(slice(a, b) for a, b in zip(lo, hi))]

    cover = np.zeros(want.shape[1:], np.int32)
    parts = np.full(want.shape, np.nan, np.float32)

    def sink(lo, hi, block):
        sl = tuple(slice(a - o, b - o) for a, b, o in zip(lo, hi, shard.own_lo))
        assert block.shape == (CHANNELS,) + tuple(b - a for a, b in zip(lo, hi))
        cover[sl] += 1
        parts[(slice(None),) + sl] = block

    ops2 = NumpyShardOps(plan, shard, gvol, slab_planes)
    out = sharding.predict_shard_streaming(read_box, None, plan, shard, group=group, ops=ops2,
                                           dtype=np.uint16, write_block=sink, keep_input_resident=resident)
    assert out is None and requested
    assert cover.min() == 1 and cover.max() == 1
    np.testing.assert_array_equal(parts, want)
    return shard, got


def _worker(rank, world, port, failures, geometry, resident, slab_planes):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        shard, got = run_rank(rank, world, geometry, resident, slab_planes)
        # the ranks' regions assemble to the single-process overlap-add (order of the band sums
        # differs from one process at rank faces: 1 ulp)
        gshape, overlap = GEOMETRIES[geometry]
        parts = [None] * world
        dist.gather_object((shard.own_lo, shard.own_hi, got), parts if rank == 0 else None, dst=0)
        if rank == 0:
            plan = inference.SlidingWindow(gshape, PATCH, overlap, TRIM)
            full = np.full((CHANNELS,) + gshape, np.nan, np.float32)
            for lo, hi, arr in parts:
                full[(slice(None),) + tuple(slice(a, b) for a, b in zip(lo, hi))] = arr
            assert not np.isnan(full).any()
            one = sharding.Shard(plan, (1, 1), 0)
            np.testing.assert_allclose(full, reference_route(plan, one, None), rtol=0, atol=2e-6)
    except Exception as exc:  # surface the failure in the parent
        failures.put(f"rank {rank}: {type(exc).__name__}: {exc}")
        raise
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,geometry,resident,slab_planes", [
    (2, "bands", False, 5), (4, "bands", True, 3), (8, "bands", False, 7), (8, "deep", False, 4),
    (4, "tiling", False, 6), (2, "deep", True, 100),
])
def test_streamed_shards_equal_the_whole_accumulator_route(world, geometry, resident, slab_planes):
    ctx = mp.get_context("spawn")
    failures = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, failures, geometry, resident, slab_planes))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    msgs = []
    while not failures.empty():
        msgs.append(failures.get())
    assert not msgs, msgs
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


@pytest.mark.parametrize("geometry", ["bands", "tiling", "deep"])
def test_single_rank_streaming_needs_no_group(geometry):
    """World size 1: no neighbours, nothing parked, no exchange; the same code path as the ranks'."""
    run_rank(0, 1, geometry, False, 3)


# --- the same loop on the 1 x 1 grid of a device that has the volume to itself: what -----------
# --- predict_streaming and predict_components_streaming hand to inference.run_slab_pipeline -----
WHOLE_GEOMETRIES = dict(GEOMETRIES, nofit=((40, 88, 12), (16, 16, 16)))   # nofit: x <= overlap, no patch fits
# the (z0, z1) a sink sees when the slot cap (100 planes) cuts nothing: layer k finishes planes up
# to z_{k+1} + trim, the last layer the rest
UNCUT = {
    "bands": [(0, 20), (20, 36), (36, 52), (52, 68), (68, 84), (84, 104)],
    "tiling": [(0, 28), (28, 52), (52, 76), (76, 104)],
    "deep": [(0, 12)] + [(z, z + 8) for z in range(12, 108, 8)] + [(108, 136)],
}


def run_whole(geometry, cap_planes, resident=False, read_box=None, **sink):
    gshape, overlap = WHOLE_GEOMETRIES[geometry]
    plan = inference.SlidingWindow(gshape, PATCH, overlap, TRIM)
    whole = inference._WholeVolume(plan)
    gvol = synthetic.synth_volume(gshape, seed=3)
    ops = NumpyShardOps(plan, whole, gvol, cap_planes)
    if read_box is None:
        read_box = inference._ArraySource(gvol)
    inference.run_slab_pipeline(ops, whole, read_box, np.dtype(np.uint16), ops.storage(np.uint16), (1, 99.9),
                                keep_input_resident=resident, **sink)
    return plan, ops


def expected_cuts(plan, cap_planes):
    """The cut rule, restated: finished ranges in pieces of min(D, max(stride + trim, patch_z), cap)."""
    D, pz = plan.shape[0], PATCH[0]
    stride = pz - plan.overlap[0]
    z = list(range(0, D - plan.overlap[0], stride))
    piece = min(D, max(stride + TRIM, pz), cap_planes)
    cuts, lo = [], 0
    for k in range(len(z)):
        hi = D if k + 1 == len(z) else min(z[k + 1] + TRIM, D)
        cuts += [(a, min(a + piece, hi)) for a in range(lo, hi, piece)]
        lo = hi
    return cuts


@pytest.fixture(scope="module")
def whole_reference():
    """reference_route of the 1 x 1 shard per geometry, computed once and never written to."""
    cache = {}

    def get(geometry):
        if geometry not in cache:
            gshape, overlap = GEOMETRIES[geometry]
            plan = inference.SlidingWindow(gshape, PATCH, overlap, TRIM)
            want = reference_route(plan, sharding.Shard(plan, (1, 1), 0), None)
            want.flags.writeable = False
            cache[geometry] = want
        return cache[geometry]
    return get


@pytest.mark.parametrize("geometry", ["bands", "tiling", "deep"])
@pytest.mark.parametrize("cap_planes", [3, 100])
def test_whole_volume_slabs_follow_the_cut_rule(geometry, cap_planes, whole_reference):
    gshape = GEOMETRIES[geometry][0]
    seen = []
    parts = np.full((CHANNELS,) + gshape, np.nan, np.float32)

    def sink(lo, hi, block):
        assert (lo[1:], hi[1:]) == ((0, 0), gshape[1:])
        seen.append((lo[0], hi[0]))
        parts[:, lo[0]:hi[0]] = block

    plan, _ = run_whole(geometry, cap_planes, write_block=sink)
    assert seen == expected_cuts(plan, cap_planes)
    if cap_planes == 100:
        assert seen == UNCUT[geometry]
    else:
        assert max(b - a for a, b in seen) == 3
    np.testing.assert_array_equal(parts, whole_reference(geometry))


@pytest.mark.parametrize("geometry,cap_planes", [("bands", 3), ("tiling", 100), ("deep", 5)])
def test_whole_volume_label_sink(geometry, cap_planes, whole_reference):
    gshape = GEOMETRIES[geometry][0]
    D, H, W = gshape
    calls = []
    divided = np.full((CHANNELS,) + gshape, np.nan, np.float32)

    def label(z0, z1, out, slot):
        assert tuple(out.shape) == (CHANNELS, z1 - z0, H, W)
        calls.append((z0, z1))
        divided[:, z0:z1] = out.numpy()
        ids = slot[: (z1 - z0) * H * W].view(1, z1 - z0, H, W)
        ids.copy_(torch.arange(ids.numel(), dtype=torch.int32).view(ids.shape) + z0 * H * W)   # = the voxel's index
        return ids

    voxel_index = np.arange(D * H * W, dtype=np.int32).reshape(gshape)
    handed = []
    got = np.full(gshape, -1, np.int32)

    def sink(lo, hi, block):
        handed.append((lo[0], hi[0]))
        assert block.dtype == np.int32 and block.shape == (hi[0] - lo[0], H, W)
        got[lo[0]:hi[0]] = block

    plan, _ = run_whole(geometry, cap_planes, write_block=sink, label=label)
    # once per slab, in z order, contiguous over [0, D): the cuts a float sink sees
    assert calls == expected_cuts(plan, cap_planes) and handed == calls
    assert calls[0][0] == 0 and calls[-1][1] == D and all(a[1] == b[0] for a, b in zip(calls, calls[1:]))
    np.testing.assert_array_equal(divided, whole_reference(geometry))      # it saw the divided values
    np.testing.assert_array_equal(got, voxel_index)                        # the sink got what it returned
    # ... and so does a result array
    result = np.full(gshape, -1, np.int32)
    run_whole(geometry, cap_planes, result=result, label=label)
    np.testing.assert_array_equal(result, voxel_index)
    assert calls == 2 * expected_cuts(plan, cap_planes)
    # a label function that keeps its labels (returns None) is called as often, and nothing is handed over
    kept = []
    untouched = np.full(gshape, -1, np.int32)
    run_whole(geometry, cap_planes, result=untouched, label=lambda z0, z1, out, slot: kept.append((z0, z1)))
    assert kept == expected_cuts(plan, cap_planes) and (untouched == -1).all()
    run_whole(geometry, cap_planes, write_block=lambda lo, hi, block: pytest.fail("handed over"),
              label=lambda z0, z1, out, slot: None)


@pytest.mark.parametrize("cap_planes", [3, 100])
def test_whole_volume_no_patch_fits(cap_planes, monkeypatch):
    gshape = WHOLE_GEOMETRIES["nofit"][0]
    monkeypatch.setattr(NumpyShardOps, "run_layer", lambda self, *a, **k: pytest.fail("run_layer without a patch"))
    seen = []
    cover = np.zeros(gshape[0], np.int32)

    def sink(lo, hi, block):
        assert (lo[1:], hi[1:]) == ((0, 0), gshape[1:]) and block.shape == (CHANNELS, hi[0] - lo[0]) + gshape[1:]
        assert not block.any()
        seen.append((lo[0], hi[0]))
        cover[lo[0]:hi[0]] += 1

    run_whole("nofit", cap_planes, write_block=sink)
    assert (cover == 1).all()
    piece = min(32, cap_planes)      # min(D, max(stride + trim, patch_z), cap) with D = 40
    assert seen == [(a, min(a + piece, 40)) for a in range(0, 40, piece)]
    result = np.full((CHANNELS,) + gshape, np.nan, np.float32)
    run_whole("nofit", cap_planes, result=result)
    assert not result.any()
    with pytest.raises(ValueError):      # (the rank geometry of a larger grid has no such case)
        sharding.Shard(inference.SlidingWindow(gshape, PATCH, WHOLE_GEOMETRIES["nofit"][1], TRIM), (1, 1), 0)


@pytest.mark.parametrize("geometry", ["bands", "tiling", "deep"])
@pytest.mark.parametrize("resident", [False, True])
def test_read_block_adapter_requests(geometry, resident, whole_reference):
    gshape = GEOMETRIES[geometry][0]
    gvol = synthetic.synth_volume(gshape, seed=3)
    requests = np.zeros(gshape[0], np.int32)

    def read_block(z0, z1):
        assert 0 <= z0 < z1 <= gshape[0], (z0, z1)
        requests[z0:z1] += 1
        return gvol[z0:z1]

    result = np.full((CHANNELS,) + gshape, np.nan, np.float32)
    run_whole(geometry, 100, resident=resident, read_box=inference._plane_reader(read_block, gshape), result=result)
    assert requests.min() >= 1 and requests.max() <= (1 if resident else 2), requests
    np.testing.assert_array_equal(result, whole_reference(geometry))
