"""
Round counts and pass times of TEASAR's loop on the device (run on the MI355X box):
    python tools/teasar_rate.py [--size 512] [--reps 5] [--check-budget-s 30] [--out FILE]

Labels as in tools/parents_rate.py: the neurite-like size^3 affinities,
agglomerate_affinities(fragments="watershed", premerge_size=100), fill_holes. Then skeletonize_labels' chain on
the device (inference._skeleton_chain_on_device): DBF, segment_table, find-root, DAF, the penalty, its field,
parents and hops. On those tensors, once with const = 450 (the reference's: few rounds, every cube clipped to its
label's box) and once with const = 4 (many rounds), scale = 1.25 both times:
  loop     inference._teasar_on_device, begin to the last read, the whole loop as teasar_branches runs it;
  target   per round exaspim_teasar_round: the keys cleared, the target pass over the state bytes, the walks
           that measure the branches;
  apply    per round exaspim_teasar_apply: the walks that write the branches, and the invalidation;
  daf      inference._geodesic_on_device from the roots without the farthest table: the pass of the parent
           commit that 6m used as its yardstick, timed in the same run.
With HIP events, the median of --reps runs after one warm-up; the per-round figures are medians over the runs
of each round's own time (the first 32 rounds are listed, all of them summed). The read of the state between
the two calls of a round is not inside either figure but is inside "loop".
Check: on the labels whose bounding box is smallest, as many as fit into --check-budget-s, the branches are
compared with tests/teasar_ref.py incremental on the label's crop.
Writes one JSON object to --out (default profiles/teasar_<size>.json) and prints it.
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

LISTED = 32      # rounds whose own times are written out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-budget-s", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import teasar_ref
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
    chain = inference._skeleton_chain_on_device(labels, 1.25, 450.0, 4, 100000.0, False, 1)
    labels, dbf, boxes, roots, daf, parents, hops = (chain[name] for name in ("labels", "dbf", "boxes", "roots", "daf",
                                                                              "parents", "hops"))
    del chain
    torch.cuda.empty_cache()
    k = int(roots.numel()) - 1
    shape = tuple(labels.shape)
    dims = _native.int3(shape)
    report = {
        "tool": f"tools/teasar_rate.py --size {n} --reps {args.reps}", "device": torch.cuda.get_device_name(0),
        "shape": list(shape), "labels": k, "foreground_voxels": int((labels > 0).sum()),
        "timing": f"HIP events, median of {args.reps} after a warm-up", "scale": 1.25,
        "form": "single parental field (kimimaro's fix_branching=False), not the reference's fix_branching=True",
        "daf": {"ms": median_ms(lambda: inference._geodesic_on_device(labels, roots))},
    }
    print(json.dumps({"daf": report["daf"]}), flush=True)

    need = lib.exaspim_teasar_workspace_bytes(dims, k)
    mask = torch.empty(shape, dtype=torch.uint8, device=dev)
    state = torch.empty(5, dtype=torch.int32, device=dev)
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    targets = torch.empty(k + 1, dtype=torch.int32, device=dev)
    lengths = torch.empty(k + 1, dtype=torch.int64, device=dev)
    junction = torch.empty(k + 1, dtype=torch.int32, device=dev)
    offsets = torch.zeros(k + 2, dtype=torch.int64, device=dev)

    def rounds_apart(const):
        """One run through the C ABI with an event pair around either call of every round: (target ms, apply ms)."""
        _native.check(lib.exaspim_teasar_begin(labels.data_ptr(), roots.data_ptr(), hops.data_ptr(), daf.data_ptr(), dims,
                                               k, mask.data_ptr(), state.data_ptr(), workspace.data_ptr(), need, None),
                      "exaspim_teasar_begin")
        events = []
        while True:
            pair = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            pair[0].record()
            _native.check(lib.exaspim_teasar_round(labels.data_ptr(), daf.data_ptr(), parents.data_ptr(), hops.data_ptr(),
                                                   dims, k, mask.data_ptr(), targets.data_ptr(), lengths.data_ptr(),
                                                   junction.data_ptr(), state.data_ptr(), workspace.data_ptr(), need,
                                                   None), "exaspim_teasar_round")
            pair[1].record()
            live, broken, n_new, n_roots, refused = state.cpu().tolist()
            assert broken == 0 and refused == 0
            if live == 0:
                break
            torch.cumsum(lengths, 0, out=offsets[1:])
            voxels = torch.empty((3, n_new), dtype=torch.int32, device=dev)
            pair[2].record()
            _native.check(lib.exaspim_teasar_apply(labels.data_ptr(), parents.data_ptr(), dbf.data_ptr(), boxes.data_ptr(),
                                                   dims, k, 1.25, const, mask.data_ptr(), targets.data_ptr(),
                                                   lengths.data_ptr(), junction.data_ptr(), offsets.data_ptr(),
                                                   voxels[0].data_ptr(), voxels[1].data_ptr(), voxels[2].data_ptr(), n_new,
                                                   n_new, n_roots, state.data_ptr(), None), "exaspim_teasar_apply")
            pair[3].record()
            events.append(pair)
        torch.cuda.synchronize()
        return [p[0].elapsed_time(p[1]) for p in events], [p[2].elapsed_time(p[3]) for p in events]

    def per_round(runs):
        """Per round the median over the runs; the first LISTED of them, their sum, the largest."""
        med = [statistics.median(r[i] for r in runs) for i in range(len(runs[0]))]
        return {"ms_first_rounds": [round(v, 3) for v in med[:LISTED]], "ms_sum": round(sum(med), 3),
                "ms_largest": round(max(med), 3), "ms_median_round": round(statistics.median(med), 3)}

    results = {}
    for const in (450.0, 4.0):
        stats = {}
        out = inference._teasar_on_device(labels, roots, dbf, daf, parents, hops, boxes, 1.25, const, stats=stats)
        results[const] = out
        rounds_apart(const)      # warm-up
        runs = [rounds_apart(const) for _ in range(args.reps)]
        assert all(len(r[0]) == stats["rounds"] for r in runs)
        sizes = out[3][1:] - out[3][:-1]
        entry = {
            "const": const, "rounds": stats["rounds"], "reads": stats["reads"], "vertices": int(out[0].numel()),
            "branches": int(out[4].numel()), "longest_branch": int(sizes.max()) if sizes.numel() else 0,
            "largest_radius": int(out[1].max()) if out[1].numel() else 0,
            "vertices_first_rounds": stats["vertices"][:LISTED], "live_labels_first_rounds": stats["live_labels"][:LISTED],
            "valid_voxels_left": int((mask & 1).sum()), "skeleton_voxels": int(((mask >> 1) & 1).sum()),
            "target": per_round([r[0] for r in runs]), "apply": per_round([r[1] for r in runs]),
            "loop_ms": median_ms(lambda: inference._teasar_on_device(labels, roots, dbf, daf, parents, hops, boxes, 1.25,
                                                                     const)),
        }
        entry["loop_over_daf"] = round(entry["loop_ms"] / report["daf"]["ms"], 3)
        report[f"const_{int(const)}"] = entry
        print(json.dumps({f"const_{int(const)}": entry}), flush=True)

    # the branches of the labels with the smallest boxes against the oracle, with const = 4
    voxels, _, _, out_offsets, branch_label, _, _ = (t.cpu().numpy() for t in results[4.0])
    vertex_label = np.repeat(branch_label, np.diff(out_offsets))
    boxes_host, roots_host = boxes.cpu().numpy(), roots.cpu().numpy()
    volume = np.prod(boxes_host[:, 3:] - boxes_host[:, :3], axis=1)
    order = [int(row) for row in np.argsort(volume) if 0 < volume[row] <= 200_000 and roots_host[row] >= 0]
    t0 = time.perf_counter()
    checked, equal = 0, True
    for row in order:
        if time.perf_counter() - t0 > args.check_budget_s:
            break
        z0, y0, x0, z1, y1, x1 = (int(v) for v in boxes_host[row])
        box = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        crop = labels[box].cpu().numpy()
        crop = np.where(crop == row, 1, 0).astype(np.int32)

        def to_local(index):
            z, y, x = np.unravel_index(np.maximum(index, 0), shape)
            return np.where(index >= 0, ((z - z0) * crop.shape[1] + (y - y0)) * crop.shape[2] + (x - x0), -1)

        local_parents = np.where(crop == 1, to_local(parents[box].cpu().numpy()), -1).astype(np.int32)
        local_hops = np.where(crop == 1, hops[box].cpu().numpy(), -1).astype(np.int32)
        sources = np.array([-1, to_local(np.array(roots_host[row]))], dtype=np.int32)
        want = teasar_ref.incremental(crop, sources, dbf[box].cpu().numpy(), daf[box].cpu().numpy(), local_parents,
                                      local_hops, 1.25, 4.0)
        # the oracle caps a radius at the crop's longest side, the device at the volume's: after the clip to the
        # box, which is the crop, either cube covers the same voxels
        got = to_local(voxels[vertex_label == row]).tolist()
        equal = equal and got == want.voxels and want.broken == 0
        checked += 1
    report["check"] = {
        "comparator": "tests/teasar_ref.py incremental (numpy) on each label's crop, const = 4: the vertices in order",
        "labels_checked": checked, "labels_with_a_box_of_at_most_2e5_voxels": len(order), "all_equal": equal,
        "host_wall_s": round(time.perf_counter() - t0, 1),
    }
    text = json.dumps(report, indent=1)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", f"teasar_{n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
