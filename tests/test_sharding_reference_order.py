"""
predict_shard(reference_order=True) on CPU: the z chain (sharding._z_band) with the ranks as
threads and sharding._p2p replaced by in-memory mailboxes, as in test_sharding_fuzz.py, but with
patch values that do NOT add exactly, so the order of the float32 additions shows. A rank starts
from its -z neighbour's band, adds its own patches in the reference's order and hands its band on;
every owned region must then hold the bits of the single-process overlap-add in plan.starts()
order. The default exchange (sum per rank, then add the bands) must differ somewhere on the same
data, or the comparison would show nothing.
"""

import queue
import threading

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd import inference, sharding


class _Group:
    def __init__(self, rank, mail):
        self.rank, self.mail = rank, mail


def _mailbox_p2p(ops, group):
    for kind, tensor, peer in ops:
        if kind == "send":
            group.mail[(group.rank, peer)].put(tensor.clone())
    for kind, tensor, peer in ops:
        if kind == "recv":
            tensor.copy_(group.mail[(peer, group.rank)].get(timeout=60))


def _patch_values(start, lo, hi):
    """Stand-in for a patch's trimmed output on the global box [lo, hi): float32 values in (0, 1)
    with full mantissas that depend on the patch and on the voxel."""
    zz, yy, xx = np.meshgrid(*(np.arange(a, b, dtype=np.uint64) for a, b in zip(lo, hi)), indexing="ij")
    h = (zz * np.uint64(73856093)) ^ (yy * np.uint64(19349663)) ^ (xx * np.uint64(83492791))
    h = (h + np.uint64(start[0] * 5 + start[1] * 11 + start[2] * 13 + 1)) * np.uint64(2654435761)
    return (((h >> np.uint64(8)) % np.uint64(1 << 24)).astype(np.float32) + np.float32(0.5)) / np.float32(1 << 24)


def _accumulate(plan, accum, origin, starts):
    """accum += every patch, one after the other in the given order (the stitch kernel's order)."""
    g, p, t = plan.shape, plan.patch_shape, plan.trim
    for s in starts:
        lo = tuple(a + t for a in s)
        hi = tuple(min(a + ps - 2 * t, d) for a, ps, d in zip(lo, p, g))
        if any(h <= l for l, h in zip(lo, hi)):
            continue
        dst = tuple(slice(a - o, b - o) for a, b, o in zip(lo, hi, origin))
        accum[(0,) + dst] += _patch_values(s, lo, hi)


def _run_ranks(plan, shards, step):
    world = len(shards)
    mail = {(a, b): queue.Queue() for a in range(world) for b in range(world)}
    out, errors = [None] * world, []

    def run(rank):
        try:
            out[rank] = step(shards[rank], _Group(rank, mail))
        except Exception as exc:        # noqa: BLE001 - reported by the main thread
            errors.append(f"rank {rank}: {type(exc).__name__}: {exc}")

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors[:2]
    return out


def _chain(plan):
    def step(sh, group):
        accum = torch.zeros((1,) + sh.accum_dims, dtype=torch.float32)
        sharding._z_band(accum, sh, group, receive=True)
        _accumulate(plan, accum.numpy(), sh.accum_origin, sh.starts)
        sharding._z_band(accum, sh, group, receive=False)
        return sharding.owned_result(accum, sh).numpy()
    return step


def _default(plan):
    def step(sh, group):
        accum = torch.zeros((1,) + sh.accum_dims, dtype=torch.float32)
        _accumulate(plan, accum.numpy(), sh.accum_origin, sh.starts)
        sharding.exchange_output_bands(accum, sh, group)
        return sharding.owned_result(accum, sh).numpy()
    return step


# (shape, patch, overlap, trim, z ranks): the default geometry scaled down by 4; an odd volume whose
# last patches are clipped, three ranks of one layer each; four ranks with two layers on the first
GEOMETRIES = [
    ((40, 40, 40), (24, 24, 24), (8, 8, 8), 2, 2),
    ((53, 37, 41), (24, 16, 24), (8, 6, 10), 2, 3),
    ((90, 30, 26), (24, 16, 16), (8, 8, 8), 1, 4),
    ((44, 20, 20), (16, 16, 16), (2, 8, 8), 3, 3),      # overlap below the trim: gaps at the rank faces
]


@pytest.mark.parametrize("shape,patch,overlap,trim,gz", GEOMETRIES)
def test_z_chain_has_the_single_process_bits(shape, patch, overlap, trim, gz, monkeypatch):
    plan = inference.SlidingWindow(shape, patch, overlap, trim)
    shards = [sharding.Shard(plan, (gz, 1), r) for r in range(gz)]
    monkeypatch.setattr(sharding, "_p2p", _mailbox_p2p)
    want = np.zeros((1,) + plan.shape, np.float32)
    _accumulate(plan, want, (0, 0, 0), plan.starts())
    got = np.full_like(want, np.nan)
    for sh, own in zip(shards, _run_ranks(plan, shards, _chain(plan))):
        got[(slice(None),) + tuple(slice(a, b) for a, b in zip(sh.own_lo, sh.own_hi))] = own
    assert got.tobytes() == want.tobytes(), int((got != want).sum())


def test_default_exchange_differs_on_the_same_data(monkeypatch):
    shape, patch, overlap, trim, gz = GEOMETRIES[0]
    plan = inference.SlidingWindow(shape, patch, overlap, trim)
    shards = [sharding.Shard(plan, (gz, 1), r) for r in range(gz)]
    monkeypatch.setattr(sharding, "_p2p", _mailbox_p2p)
    want = np.zeros((1,) + plan.shape, np.float32)
    _accumulate(plan, want, (0, 0, 0), plan.starts())
    got = np.full_like(want, np.nan)
    for sh, own in zip(shards, _run_ranks(plan, shards, _default(plan))):
        got[(slice(None),) + tuple(slice(a, b) for a, b in zip(sh.own_lo, sh.own_hi))] = own
    assert (got != want).any()
    np.testing.assert_allclose(got, want, rtol=0, atol=8 * 2.0 ** -22)    # sums below 8: a few ulps at most


def test_reference_order_refuses_a_y_split():
    plan = inference.SlidingWindow((40, 40, 40), (24, 24, 24), (8, 8, 8), 2)
    shard = sharding.Shard(plan, (2, 2), 0)
    with pytest.raises(ValueError, match="splits z only"):
        sharding.predict_shard(None, None, plan, shard, reference_order=True)
