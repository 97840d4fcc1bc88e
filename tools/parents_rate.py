"""
Pass times and sweep counts of the parental field and the path tracing (run on the MI355X box):
    python tools/parents_rate.py [--size 512] [--reps 5] [--check-budget-s 60] [--out FILE]

Labels, roots and the distance-from-root field (DAF) as in tools/geodesic_rate.py: the neurite-like size^3
affinities, agglomerate_affinities(fragments="watershed", premerge_size=100), fill_holes, each label's first
voxel, its farthest voxel as the root, the field from the roots. Then, on that field (Euclidean steps):
  daf      inference._geodesic_on_device from the roots without the farthest table: the pass of the parent
           commit that the hops pass has the shape of, timed in the same run as the yardstick;
  hops     exaspim_geodesic_parents_begin and _sweeps;
  parents  exaspim_geodesic_parents_finish alone;
  trace    exaspim_trace_paths alone from every label's far_index, and inference.trace_paths with its
           offsets (a gather, a cumulative sum and two reads) included.
Per pass, with HIP events, the median of --reps runs after one warm-up: "ms" with batches of 32 sweeps and a
read of the state after each, "ms_one_batch" with all the sweeps the pass needs in one batch. From one run
with a read after every sweep: the sweeps needed (the last one finds nothing to do), the active tile
executions (the sum over the sweeps of the tiles flagged) and the largest number of tiles active in one sweep.
Check: on the labels whose bounding box is smallest, as many as fit into --check-budget-s, parents and hops
are compared with tests/parents_ref.py jacobi on the label's crop and the crop's own numpy field.
Writes one JSON object to --out (default profiles/parents_<size>.json) and prints it.
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-budget-s", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import geodesic_ref
    import parents_ref
    from aind_exaspim_neuron_segmentation_amd import _native, inference
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    dev = torch.device("cuda:0")
    lib = _native.lib()

    def neurite_affinities(n):      # tools/geodesic_rate.py's
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        raw = torch.empty((n, n, n), dtype=torch.int16, device=dev)
        _native.check(lib.exaspim_synth_volume_neurite_u16(raw.data_ptr(), _native.Block.make((n, n, n)), 0, None),
                      "synth_neurite")
        on = ((raw.to(torch.int32) & 0xFFFF) > synthetic.NEURITE_FLOOR_MAX).float()
        del raw
        p = torch.nn.functional.avg_pool3d(on[None, None], 3, stride=1, padding=1, count_include_pad=True)[0, 0]
        del on
        aff = torch.rand((3, n, n, n), dtype=torch.float32, device=dev, generator=gen).mul_(0.6).add_(0.4)
        aff[0, :-1] *= torch.minimum(p[:-1], p[1:])
        aff[1, :, :-1] *= torch.minimum(p[:, :-1], p[:, 1:])
        aff[2, :, :, :-1] *= torch.minimum(p[:, :, :-1], p[:, :, 1:])
        return aff

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def median_ms(fn):
        timed(fn)      # warm-up
        return round(statistics.median(timed(fn) for _ in range(args.reps)), 3)

    n = args.size
    aff = neurite_affinities(n)
    capacity = max(1 << 16, 1 << (n ** 3 // 8 - 1).bit_length())
    labels = inference.agglomerate_affinities(aff, fragments="watershed", premerge_size=100, edge_capacity=capacity,
                                              return_device_tensor=True)
    del aff
    labels, _ = inference._fill_holes_on_device(labels)
    torch.cuda.empty_cache()
    k = int(labels.max())
    shape = tuple(labels.shape)
    dims = _native.int3(shape)
    sizes, boxes, _, first = inference.segment_table(labels, n_labels=k, return_device_tensors=True)
    _, _, roots = inference._geodesic_on_device(labels, first, farthest=True)
    daf_stats = {}
    daf, _, far_index = inference._geodesic_on_device(labels, roots, sweeps_per_read=1, farthest=True, stats=daf_stats)
    tiles = 1
    for extent, tile in zip(shape, (8, 8, 32)):
        tiles *= -(-extent // tile)
    report = {
        "tool": f"tools/parents_rate.py --size {n} --reps {args.reps}", "device": torch.cuda.get_device_name(0),
        "shape": list(shape), "labels": k, "foreground_voxels": int((labels > 0).sum()),
        "tiles": tiles, "timing": f"HIP events, median of {args.reps} after a warm-up",
    }
    flagged = daf_stats["tiles_flagged"]
    report["daf"] = {
        "ms": median_ms(lambda: inference._geodesic_on_device(labels, roots)),
        "ms_one_batch": median_ms(lambda: inference._geodesic_on_device(
            labels, roots, sweeps_per_read=max(daf_stats["sweeps"], 1))),
        "sweeps_needed": daf_stats["sweeps"], "active_tile_executions": int(sum(flagged[:-1])),
        "largest_active_tiles_in_a_sweep": int(max(flagged)),
    }
    print(json.dumps({"daf": report["daf"]}), flush=True)

    # the hops pass through the C ABI, so that begin + sweeps and finish are timed apart
    need = lib.exaspim_geodesic_workspace_bytes(dims)
    hops = torch.empty(shape, dtype=torch.int32, device=dev)
    parents = torch.empty(shape, dtype=torch.int32, device=dev)
    state = torch.zeros(3, dtype=torch.int32, device=dev)
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)

    def hops_pass(batch, history=None):
        _native.check(lib.exaspim_geodesic_parents_begin(labels.data_ptr(), dims, roots.data_ptr(), k, daf.data_ptr(),
                                                         hops.data_ptr(), state.data_ptr(), workspace.data_ptr(), need,
                                                         None), "exaspim_geodesic_parents_begin")
        now, invalid = state.cpu().tolist()[:2]
        assert invalid == 0
        launched = 0
        while now:
            if history is not None:
                history.append(now)
            _native.check(lib.exaspim_geodesic_parents_sweeps(labels.data_ptr(), None, daf.data_ptr(), dims, k,
                                                              hops.data_ptr(), batch, state.data_ptr(),
                                                              workspace.data_ptr(), need, None),
                          "exaspim_geodesic_parents_sweeps")
            launched += batch
            now = int(state.cpu()[0])
        return launched

    def finish():
        _native.check(lib.exaspim_geodesic_parents_finish(labels.data_ptr(), None, daf.data_ptr(), hops.data_ptr(), dims,
                                                          k, parents.data_ptr(), state.data_ptr(), None),
                      "exaspim_geodesic_parents_finish")

    history = []
    needed = hops_pass(1, history)
    report["hops"] = {
        "ms": median_ms(lambda: hops_pass(32)),
        "ms_one_batch": median_ms(lambda: hops_pass(max(needed, 1))),
        "sweeps_needed": needed, "active_tile_executions": int(sum(history)),
        "largest_active_tiles_in_a_sweep": int(max(history + [0])), "largest_hops": int(hops.max()),
    }
    print(json.dumps({"hops": report["hops"]}), flush=True)
    report["parents"] = {"ms": median_ms(finish), "orphans": int(state.cpu()[2]),
                         "voxels_with_a_parent": int((parents >= 0).sum())}
    print(json.dumps({"parents": report["parents"]}), flush=True)

    targets = far_index[1:][far_index[1:] >= 0].contiguous()
    voxels, offsets = inference.trace_paths(parents, hops, targets, return_device_tensors=True)
    trace_state = torch.zeros(2, dtype=torch.int32, device=dev)

    def trace_alone():
        _native.check(lib.exaspim_trace_paths(parents.data_ptr(), hops.data_ptr(), dims, targets.data_ptr(),
                                              int(targets.numel()), offsets.data_ptr(), voxels.data_ptr(),
                                              int(voxels.numel()), trace_state.data_ptr(), None), "exaspim_trace_paths")

    lengths = (offsets[1:] - offsets[:-1])
    report["trace"] = {
        "targets": int(targets.numel()), "path_voxels": int(voxels.numel()), "longest_path": int(lengths.max()),
        "ms_kernel": median_ms(trace_alone),
        "ms_with_offsets": median_ms(lambda: inference.trace_paths(parents, hops, targets, return_device_tensors=True)),
        "state": trace_state.cpu().tolist(),
    }
    print(json.dumps({"trace": report["trace"]}), flush=True)

    # parents and hops of the labels with the smallest boxes against the oracle
    boxes_host, roots_host = boxes.cpu().numpy(), roots.cpu().numpy()
    volume = np.prod(boxes_host[:, 3:] - boxes_host[:, :3], axis=1)
    order = [int(row) for row in np.argsort(volume) if 0 < volume[row] <= 2_000_000]      # what a numpy round can afford
    t0 = time.perf_counter()
    checked, equal = 0, True
    for row in order:
        if time.perf_counter() - t0 > args.check_budget_s:
            break
        z0, y0, x0, z1, y1, x1 = (int(v) for v in boxes_host[row])
        crop = labels[z0:z1, y0:y1, x0:x1].cpu().numpy()
        crop = np.where(crop == row, crop, 0)
        z, y, x = np.unravel_index(int(roots_host[row]), shape)
        local = np.full(row + 1, -1, dtype=np.int32)
        local[row] = np.ravel_multi_index((z - z0, y - y0, x - x0), crop.shape)
        want_parents, want_hops, orphans, _ = parents_ref.jacobi(crop, local, geodesic_ref.relaxation(crop, local))
        sel = crop == row
        got_hops = hops[z0:z1, y0:y1, x0:x1].cpu().numpy()
        got = parents[z0:z1, y0:y1, x0:x1].cpu().numpy()
        gz, gy, gx = np.unravel_index(np.maximum(got, 0), shape)      # global indices into the crop's
        inside = (got >= 0) & (gz >= z0) & (gz < z1) & (gy >= y0) & (gy < y1) & (gx >= x0) & (gx < x1)
        as_local = np.where(inside, ((gz - z0) * crop.shape[1] + (gy - y0)) * crop.shape[2] + (gx - x0), -1)
        equal = (equal and orphans == 0 and bool(np.array_equal(got_hops[sel], want_hops[sel]))
                 and bool(np.array_equal(as_local[sel], want_parents[sel])))
        checked += 1
    report["check"] = {
        "comparator": "tests/parents_ref.py jacobi (numpy) on each label's crop, int32",
        "labels_checked": checked, "labels_with_a_box_of_at_most_2e6_voxels": len(order), "all_equal": equal,
        "host_wall_s": round(time.perf_counter() - t0, 1),
    }
    text = json.dumps(report, indent=1)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", f"parents_{n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
