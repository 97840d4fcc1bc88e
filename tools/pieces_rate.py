"""
label_pieces and skeletonize_pieces' chain on the device (run on the MI355X box):
    python tools/pieces_rate.py [--size 512] [--reps 5] [--out FILE]

Labels as in tools/border_rate.py: the neurite-like size^3 affinities,
agglomerate_affinities(fragments="watershed", premerge_size=100), fill_holes. Recorded:
  label_pieces_kernels_ms  exaspim_label_pieces through the C ABI into buffers made once (HIP events, the median of
                           --reps runs after one warm-up), at dust thresholds 0 and 1000, with P and the dust count;
  label_pieces_ms          the Python entry point with its allocations, the read of P and the three tables;
  host_oracle_s            tests/pieces_ref.py's by_label (scipy.ndimage.label per label) on the same labels,
                           downloaded, with "equal": the device's volume is the oracle's;
  skeletonize              the chain (inference._skeleton_chain_on_device, the reference's teasar_params,
                           fix_branching=True, fix_borders=True) on the labels, which is skeletonize_fix_borders,
                           and on their pieces at dust 1000, which is skeletonize_pieces: rounds, vertices, and
                           the border targets kept that the old form dropped (targets of the labels that lie in a
                           kept piece and are no vertex of the old form's skeletons).
The C ABI has one entry for the eight launches, so the passes are timed one by one with a kernel trace of
    rocprofv3 --kernel-trace --stats -- python tools/pieces_rate.py --kernels-only
(1 + --reps calls at dust 0 and nothing else of the above). Nothing here is a pass criterion. Writes one JSON
object to --out (default profiles/label_pieces_<size>.json) and prints it.
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
    ap.add_argument("--kernels-only", action="store_true",
                    help="only the C-ABI calls at dust 0, for a kernel trace: no oracle, no chain, no file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import pieces_ref
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
    report = {
        "tool": f"tools/pieces_rate.py --size {n} --reps {args.reps}",
        "device": torch.cuda.get_device_name(0), "shape": list(shape), "labels": k,
        "foreground_voxels": int((labels > 0).sum()),
        "timing": f"HIP events, median of {args.reps} after a warm-up",
    }

    need = lib.exaspim_label_pieces_workspace_bytes(dims)
    pieces = torch.empty(shape, dtype=torch.int32, device=dev)
    state = torch.empty(2, dtype=torch.int32, device=dev)
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    host = labels.cpu().numpy()
    report["thresholds"] = {}
    for dust in (0, 1000):
        def kernels():
            _native.check(lib.exaspim_label_pieces(labels.data_ptr(), dims, k, dust, pieces.data_ptr(),
                                                   state.data_ptr(), workspace.data_ptr(), need, None), "label_pieces")

        entry = {"label_pieces_kernels_ms": median_ms(kernels)}
        if args.kernels_only:
            print(json.dumps(entry), flush=True)
            return
        entry["label_pieces_ms"] = median_ms(
            lambda: inference.label_pieces(labels, n_labels=k, dust_threshold=dust, return_device_tensors=True))
        entry["pieces"], entry["dust_pieces"] = (int(v) for v in state.cpu())
        t0 = time.perf_counter()
        want = pieces_ref.by_label(host, k, dust)
        entry["host_oracle_s"] = round(time.perf_counter() - t0, 3)
        entry["equal"] = bool(np.array_equal(pieces.cpu().numpy(), want[0])) and entry["pieces"] == len(want[1])
        report["thresholds"][str(dust)] = entry
        print(json.dumps(entry), flush=True)
    report["host_oracle"] = "tests/pieces_ref.py by_label: scipy.ndimage.label per label, 3x3x3 structure"
    del workspace, want
    torch.cuda.empty_cache()

    # the chain on the labels (skeletonize_fix_borders) and on their pieces at dust 1000 (skeletonize_pieces)
    pieces, state = inference._label_pieces_on_device(labels, k, 1000)
    n_pieces = int(state.cpu()[0])
    report["skeletonize"] = {}
    vertex_sets = {}
    for name, volume in (("labels", labels), ("pieces", pieces)):
        def chain(stats=None):
            return inference._skeleton_chain_on_device(volume, 1.25, 450.0, 4, 100000.0, False, None, True, stats,
                                                       fix_borders=True)

        stats = {}
        out = chain(stats)      # the warm-up, and the counts
        entry = {key: stats[key] for key in ("rounds", "reads", "updates", "given_rounds", "empty_rounds")
                 if key in stats}
        entry.update(vertices=int(out["voxels"].numel()), branches=int(out["branch_label"].numel()),
                     border_targets=int(out["border_targets"][0].numel()))
        vertex_sets[name] = set(out["voxels"].cpu().tolist())
        targets = out["border_targets"][1].cpu().numpy()
        entry["border_targets_on_the_skeleton"] = int(sum(int(v) in vertex_sets[name] for v in targets))
        if name == "labels":
            label_targets = targets
        del out
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chain()
        torch.cuda.synchronize()
        entry["chain_wall_s"] = round(time.perf_counter() - t0, 3)
        report["skeletonize"][name] = entry
        print(json.dumps(entry), flush=True)
    in_kept = pieces.reshape(-1)[torch.from_numpy(label_targets.astype(np.int64)).to(dev)].cpu().numpy() > 0
    report["skeletonize"]["kept_pieces"] = n_pieces
    report["skeletonize"]["label_targets_in_kept_pieces"] = int(in_kept.sum())
    report["skeletonize"]["kept_that_the_old_form_dropped"] = int(sum(
        int(v) not in vertex_sets["labels"] and int(v) in vertex_sets["pieces"] for v in label_targets[in_kept]))
    text = json.dumps(report, indent=1)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", f"label_pieces_{n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
