"""
border_targets and the fix_borders chain on the device (run on the MI355X box):
    python tools/border_rate.py [--size 512] [--reps 5] [--out FILE]

Labels as in tools/fix_branching_rate.py: the neurite-like size^3 affinities,
agglomerate_affinities(fragments="watershed", premerge_size=100), fill_holes. Recorded:
  border_targets_ms   exaspim_border_targets with the sort and the read of the count (HIP events, the median of
                      --reps runs after one warm-up), and the kernels alone through the C ABI into buffers made once;
  host_oracle_s       tests/border_ref.py's per-component distance transform on the same labels, downloaded, with
                      "equal": the device's rows are the oracle's;
  targets             the number of targets, the labels that have one, the largest number of one label;
  skeletonize         the chain from the filled labels (inference._skeleton_chain_on_device, the reference's
                      teasar_params, fix_branching=True) without and with fix_borders: rounds, given and empty
                      rounds, updates, vertices, and the wall time of one run after a warm-up.
Nothing here is a pass criterion. Writes one JSON object to --out (default profiles/border_targets_<size>.json)
and prints it.
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import border_ref
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
    k = max(int(labels.max()), 0)
    shape = tuple(labels.shape)
    dims = _native.int3(shape)
    pixels = 2 * (shape[1] * shape[2] + shape[0] * shape[2] + shape[0] * shape[1])
    report = {
        "tool": f"tools/border_rate.py --size {n} --reps {args.reps}",
        "device": torch.cuda.get_device_name(0), "shape": list(shape), "labels": k, "face_pixels": pixels,
        "foreground_face_pixels": int(sum(int((labels.select(a, i) > 0).sum()) for a in range(3) for i in (0, -1))),
        "timing": f"HIP events, median of {args.reps} after a warm-up",
    }

    # the kernels alone, then the Python entry point (allocations, the read of the count, the sort)
    need = lib.exaspim_border_targets_workspace_bytes(dims)
    out_l = torch.empty(pixels, dtype=torch.int32, device=dev)
    out_v = torch.empty(pixels, dtype=torch.int32, device=dev)
    state = torch.empty(2, dtype=torch.int32, device=dev)
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)

    def kernels():
        _native.check(lib.exaspim_border_targets(labels.data_ptr(), dims, k, out_l.data_ptr(), out_v.data_ptr(), pixels,
                                                 state.data_ptr(), workspace.data_ptr(), need, None), "border_targets")

    report["border_targets_kernels_ms"] = median_ms(kernels)
    report["border_targets_ms"] = median_ms(lambda: inference._border_targets_on_device(labels, k))
    target_labels, target_voxels = inference._border_targets_on_device(labels, k)
    rows = torch.stack([target_labels, target_voxels], dim=1).cpu().numpy()
    host = labels.cpu().numpy()
    t0 = time.perf_counter()
    want = border_ref.by_component(host, k)
    report["host_oracle_s"] = round(time.perf_counter() - t0, 3)
    report["host_oracle"] = "tests/border_ref.py by_component: scipy label and distance_transform_edt per component"
    report["equal"] = bool(np.array_equal(rows, want))
    per_label = np.bincount(rows[:, 0], minlength=k + 1)
    report["targets"] = {"rows": int(len(rows)), "labels_with_a_target": int((per_label > 0).sum()),
                         "most_of_one_label": int(per_label.max()) if len(rows) else 0}
    del host, out_l, out_v, workspace
    torch.cuda.empty_cache()

    report["skeletonize"] = {}
    for fix_borders in (False, True):
        def chain(stats=None):
            return inference._skeleton_chain_on_device(labels, 1.25, 450.0, 4, 100000.0, False, None, True, stats,
                                                       fix_borders=fix_borders)

        stats = {}
        out = chain(stats)      # the warm-up, and the counts
        entry = {key: stats[key] for key in ("rounds", "reads", "updates", "given_rounds", "empty_rounds")
                 if key in stats}
        entry.update(vertices=int(out["voxels"].numel()), branches=int(out["branch_label"].numel()))
        del out
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chain()
        torch.cuda.synchronize()
        entry["chain_wall_s"] = round(time.perf_counter() - t0, 3)
        report["skeletonize"]["fix_borders" if fix_borders else "plain"] = entry
        print(json.dumps(entry), flush=True)
    text = json.dumps(report, indent=1)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", f"border_targets_{n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
