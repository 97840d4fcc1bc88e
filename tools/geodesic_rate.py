"""
Pass times and sweep counts of the geodesic distance-from-source field (run on the MI355X box):
    python tools/geodesic_rate.py [--size 512] [--reps 5] [--check-budget-s 60] [--out FILE]

Labels: inference.agglomerate_affinities(fragments="watershed", premerge_size=100,
return_device_tensor=True) on the neurite-like size^3 affinities of tools/dbf_rate.py, then fill_holes.
Two passes of inference._geodesic_on_device with the farthest table, as a skeletoniser would run them:
  find_root  sources = segment_table(labels)'s peak_index without a field (each label's first voxel);
             its far_index are the roots;
  daf        sources = those roots: the distance-from-root field.
Per pass, with HIP events, the median of --reps runs after one warm-up:
  ms            begin, sweeps in batches of 32 with an 8-byte read of the state after each, farthest: the
                device time a caller sees, the idle time of the reads included;
  ms_one_batch  the same with all the sweeps the pass needs in one batch (two reads in all);
  ms_farthest   exaspim_geodesic_farthest alone;
and from one run with a read after every sweep: the sweeps needed (the last one finds nothing to do), the
active tile executions (the sum over the sweeps of the tiles flagged) and the largest number of tiles
active in one sweep. Every sweep launches one workgroup per tile of the volume; an idle one reads a flag.
Check: on the labels whose bounding box is smallest, as many as fit into --check-budget-s, the device's
field is compared bit for bit with tests/geodesic_ref.py relaxation on the label's crop (a numpy
relaxation in float32 on this host; not dijkstra3d, not kimimaro).
Writes one JSON object to --out (default profiles/geodesic_<size>.json) and prints it.
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
    from aind_exaspim_neuron_segmentation_amd import _native, inference
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    dev = torch.device("cuda:0")
    lib = _native.lib()

    def neurite_affinities(n):
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
        return statistics.median(timed(fn) for _ in range(args.reps))

    n = args.size
    aff = neurite_affinities(n)
    capacity = max(1 << 16, 1 << (n ** 3 // 8 - 1).bit_length())
    labels = inference.agglomerate_affinities(aff, fragments="watershed", premerge_size=100, edge_capacity=capacity,
                                              return_device_tensor=True)
    del aff
    labels, _ = inference._fill_holes_on_device(labels)
    torch.cuda.empty_cache()
    k = int(labels.max())
    dims = _native.int3(tuple(labels.shape))
    sizes, boxes, _, first = inference.segment_table(labels, n_labels=k, return_device_tensors=True)
    tiles = 1
    for extent, tile in zip(labels.shape, (8, 8, 32)):
        tiles *= -(-extent // tile)
    report = {
        "tool": f"tools/geodesic_rate.py --size {n} --reps {args.reps}", "device": torch.cuda.get_device_name(0),
        "shape": list(labels.shape), "labels": k, "foreground_voxels": int((labels > 0).sum()),
        "tiles": tiles, "timing": f"HIP events, median of {args.reps} after a warm-up",
    }

    def one_pass(name, sources):
        stats = {}
        field, far_value, far_index = inference._geodesic_on_device(labels, sources, sweeps_per_read=1, farthest=True,
                                                                    stats=stats)
        flagged = stats["tiles_flagged"]
        needed = stats["sweeps"]
        far_need = lib.exaspim_geodesic_farthest_workspace_bytes(k)
        far_ws = torch.empty(far_need, dtype=torch.uint8, device=dev)

        def farthest_alone():
            _native.check(lib.exaspim_geodesic_farthest(labels.data_ptr(), field.data_ptr(), dims, k,
                                                        far_value.data_ptr(), far_index.data_ptr(), far_ws.data_ptr(),
                                                        far_need, None), "exaspim_geodesic_farthest")

        batched = {}
        report[name] = {
            "ms": round(median_ms(lambda: inference._geodesic_on_device(labels, sources, farthest=True, stats=batched)), 3),
            "sweeps_launched_in_batches_of_32": None,
            "ms_one_batch": round(median_ms(lambda: inference._geodesic_on_device(
                labels, sources, sweeps_per_read=max(needed, 1), farthest=True)), 3),
            "ms_farthest": round(median_ms(farthest_alone), 3),
            "sweeps_needed": needed,
            "active_tile_executions": int(sum(flagged[:-1])),
            "largest_active_tiles_in_a_sweep": int(max(flagged)),
            "largest_finite_distance": float(far_value.max()),
            "labels_with_unreached_voxels": int((torch.bincount(labels[torch.isinf(field)].long(), minlength=k + 1)
                                                 > 0).sum()),
        }
        report[name]["sweeps_launched_in_batches_of_32"] = batched["sweeps"]
        print(json.dumps({name: report[name]}), flush=True)
        return field, far_index

    _, roots = one_pass("find_root", first)
    daf, _ = one_pass("daf", roots)

    # bit-for-bit check of the DAF on the labels with the smallest boxes
    boxes_host, roots_host = boxes.cpu().numpy(), roots.cpu().numpy()
    volume = np.prod(boxes_host[:, 3:] - boxes_host[:, :3], axis=1)
    order = [int(row) for row in np.argsort(volume) if 0 < volume[row] <= 2_000_000]      # what a numpy round can afford
    t0 = time.perf_counter()
    checked, equal = 0, True
    shape = tuple(labels.shape)
    for row in order:
        if time.perf_counter() - t0 > args.check_budget_s:
            break
        z0, y0, x0, z1, y1, x1 = (int(v) for v in boxes_host[row])
        crop = labels[z0:z1, y0:y1, x0:x1].cpu().numpy()
        z, y, x = np.unravel_index(int(roots_host[row]), shape)
        local = np.full(row + 1, -1, dtype=np.int32)
        local[row] = np.ravel_multi_index((z - z0, y - y0, x - x0), crop.shape)
        want = geodesic_ref.relaxation(np.where(crop == row, crop, 0), local)
        got = daf[z0:z1, y0:y1, x0:x1].cpu().numpy()
        sel = crop == row
        equal = equal and bool(np.array_equal(geodesic_ref.bits(got)[sel], geodesic_ref.bits(want)[sel]))
        checked += 1
    report["check"] = {
        "comparator": "tests/geodesic_ref.py relaxation (numpy, float32) on each label's crop, int32 bit patterns",
        "labels_checked": checked, "labels_with_a_box_of_at_most_2e6_voxels": len(order), "all_equal": equal,
        "host_wall_s": round(time.perf_counter() - t0, 1),
    }
    text = json.dumps(report, indent=1)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", f"geodesic_{n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
