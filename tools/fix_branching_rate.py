"""
Pass times of TEASAR's fix_branching loop on the device (run on the MI355X box):
    python tools/fix_branching_rate.py [--size 512] [--reps 5] [--consts 64 4] [--max-rounds 32]
                                       [--check-budget-s 20] [--out FILE]

Labels and the chain as in tools/teasar_rate.py: the neurite-like size^3 affinities,
agglomerate_affinities(fragments="watershed", premerge_size=100), fill_holes, then skeletonize_labels' chain on
the device up to the penalty field, its parents and hops. scale = 1.25 throughout. For every const of --consts
the loop runs for at most --max-rounds rounds (const = 4 has thousands: teasar_branches' own count is recorded
next to the cap), and per update, that is per round t >= 2, an event pair surrounds
  field          the incremental pass: exaspim_geodesic_reseed with the vertices of round t - 1 and the sweeps,
                 with the reads of the state that end it (ms and sweeps launched);
  hops           exaspim_geodesic_parents_begin_seeds with every vertex so far and the sweeps (ms and sweeps);
  parents        exaspim_geodesic_parents_finish and the read of the orphans;
  scratch_field, scratch_parents
                 the yardstick, in the same run: the parent commit's kernels doing the same update from scratch,
                 inference._geodesic_on_device(labels, roots, cost zeroed along the skeleton) and
                 inference._geodesic_parents_on_device on it. Its field must have the bits of the incremental one
                 ("fields_equal").
The whole loop (inference._fix_branching_on_device) is timed against inference._teasar_on_device at the same
const and cap, and at const = 450, where every label has one path, to show that the one-round case pays nothing.
HIP events, the median of --reps runs after one warm-up; per-round figures are medians over the runs.
Check: on the labels whose bounding box is smallest, as many as fit into --check-budget-s, the vertices at the
last const are compared with tests/fix_branching_ref.py's loop on the label's crop.
Writes one JSON object to --out (default profiles/fix_branching_<size>.json) and prints it.
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
    ap.add_argument("--consts", type=float, nargs="+", default=[64.0, 4.0])
    ap.add_argument("--max-rounds", type=int, default=32)
    ap.add_argument("--check-budget-s", type=float, default=20.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import fix_branching_ref
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
    labels, dbf, boxes, roots, daf, cost, parents, hops = (
        chain[name] for name in ("labels", "dbf", "boxes", "roots", "daf", "cost", "parents", "hops"))
    del chain
    field, _, _ = inference._geodesic_on_device(labels, roots, cost)
    torch.cuda.empty_cache()
    k = int(roots.numel()) - 1
    shape = tuple(labels.shape)
    dims = _native.int3(shape)
    cost_ptr = cost.data_ptr()
    need = lib.exaspim_geodesic_workspace_bytes(dims)
    report = {
        "tool": f"tools/fix_branching_rate.py --size {n} --reps {args.reps} --max-rounds {args.max_rounds} --consts "
                + " ".join(f"{c:g}" for c in args.consts),
        "device": torch.cuda.get_device_name(0), "shape": list(shape), "labels": k,
        "foreground_voxels": int((labels > 0).sum()),
        "timing": f"HIP events, median of {args.reps} after a warm-up", "scale": 1.25,
        "form": "fields re-seeded from the skeleton before every round after the first (fix_branching=True)",
        "yardstick": "the parent commit's kernels from scratch: the field of the cost zeroed along the skeleton from "
                     "the root, and its parental field",
    }

    own = {"field": torch.empty(shape, dtype=torch.float32, device=dev),
           "hops": torch.empty(shape, dtype=torch.int32, device=dev),
           "parents": torch.empty(shape, dtype=torch.int32, device=dev),
           "zeroed": torch.empty(shape, dtype=torch.float32, device=dev),
           "state": torch.empty(3, dtype=torch.int32, device=dev),
           "workspace": torch.empty(need, dtype=torch.uint8, device=dev)}

    def one_run(const, rounds_cap):
        """One run of the loop with its updates taken apart; per update a dict of ms, sweeps and the check."""
        own["field"].copy_(field)
        own["zeroed"].copy_(cost)
        vertices, rows = [], []

        def update(t, fresh):
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            vertices.append(fresh)
            every = torch.cat(vertices)
            field_stats = {}
            marks[0].record()
            inference._geodesic_seeded_on_device("fix_branching_rate", labels, k, fresh, cost, own["field"],
                                                 inference.FIX_BRANCHING_FIELD_SWEEPS, None, field_stats)
            marks[1].record()
            state, workspace = own["state"], own["workspace"]
            _native.check(lib.exaspim_geodesic_parents_begin_seeds(
                labels.data_ptr(), dims, k, every.data_ptr(), int(every.numel()), own["field"].data_ptr(),
                own["hops"].data_ptr(), state.data_ptr(), workspace.data_ptr(), need, None), "begin_seeds")
            flagged, invalid, _ = state.cpu().tolist()
            assert invalid == 0
            hops_sweeps = 0
            while flagged:
                _native.check(lib.exaspim_geodesic_parents_sweeps(
                    labels.data_ptr(), cost_ptr, own["field"].data_ptr(), dims, k, own["hops"].data_ptr(), 32,
                    state.data_ptr(), workspace.data_ptr(), need, None), "parents_sweeps")
                hops_sweeps += 32
                flagged = int(state.cpu()[0])
            marks[2].record()
            _native.check(lib.exaspim_geodesic_parents_finish(
                labels.data_ptr(), cost_ptr, own["field"].data_ptr(), own["hops"].data_ptr(), dims, k,
                own["parents"].data_ptr(), state.data_ptr(), None), "parents_finish")
            orphans = int(state.cpu()[2])
            assert orphans == 0
            marks[3].record()
            # the yardstick: the same update from scratch with the parent commit's kernels
            own["zeroed"].reshape(-1)[fresh.to(torch.int64)] = 0
            scratch, _, _ = inference._geodesic_on_device(labels, roots, own["zeroed"])
            marks[4].record()
            inference._geodesic_parents_on_device(labels, roots, scratch, own["zeroed"])
            marks[5].record()
            marks[5].synchronize()
            rows.append({
                "field_ms": marks[0].elapsed_time(marks[1]), "field_sweeps": field_stats["sweeps"],
                "hops_ms": marks[1].elapsed_time(marks[2]), "hops_sweeps": hops_sweeps,
                "parents_ms": marks[2].elapsed_time(marks[3]),
                "scratch_field_ms": marks[3].elapsed_time(marks[4]),
                "scratch_parents_ms": marks[4].elapsed_time(marks[5]),
                "fields_equal": bool(torch.equal(scratch.view(torch.int32), own["field"].view(torch.int32))),
                "seeds": int(every.numel()), "new_seeds": int(fresh.numel()),
            })
            return own["parents"], own["hops"]

        stats = {}
        out = inference._teasar_on_device(labels, roots, dbf, daf, parents, hops, boxes, 1.25, const, rounds_cap, stats,
                                          None, update, "fix_branching_rate")
        return rows, stats, out

    def medians(runs, key):
        return [statistics.median(r[i][key] for r in runs) for i in range(len(runs[0]))]

    last = None
    for const in [450.0] + list(args.consts):
        plain = {}
        inference._teasar_on_device(labels, roots, dbf, daf, parents, hops, boxes, 1.25, const, stats=plain)
        cap = args.max_rounds
        entry = {"const": const, "teasar_branches_rounds": plain["rounds"], "max_rounds": cap}
        stats = {}
        out = inference._fix_branching_on_device(labels, roots, dbf, daf, cost, field, parents, hops, boxes, 1.25, const,
                                                 cap, stats)
        entry.update(rounds=stats["rounds"], updates=stats["updates"], vertices=int(out[0].numel()),
                     branches=int(out[4].numel()), field_sweeps_launched=stats["field_sweeps"],
                     hops_sweeps_launched=stats["hops_sweeps"])
        entry["loop_ms"] = median_ms(lambda: inference._fix_branching_on_device(
            labels, roots, dbf, daf, cost, field, parents, hops, boxes, 1.25, const, cap))
        entry["teasar_branches_loop_ms"] = median_ms(lambda: inference._teasar_on_device(
            labels, roots, dbf, daf, parents, hops, boxes, 1.25, const, cap))
        entry["loop_over_teasar_branches"] = round(entry["loop_ms"] / entry["teasar_branches_loop_ms"], 3)
        if stats["updates"]:
            one_run(const, cap)      # warm-up
            runs = [one_run(const, cap)[0] for _ in range(args.reps)]
            assert all(len(r) == stats["updates"] for r in runs)
            per_update = {}
            for key in ("field_ms", "hops_ms", "parents_ms", "scratch_field_ms", "scratch_parents_ms"):
                med = medians(runs, key)
                per_update[key] = {"per_update": [round(v, 3) for v in med], "sum": round(sum(med), 3),
                                   "median": round(statistics.median(med), 3)}
            for key in ("field_sweeps", "hops_sweeps", "seeds", "new_seeds"):
                per_update[key] = [int(v) for v in medians(runs, key)]
            per_update["fields_equal"] = all(row["fields_equal"] for r in runs for row in r)
            update_ms = sum(per_update[key]["sum"] for key in ("field_ms", "hops_ms", "parents_ms"))
            scratch_ms = per_update["scratch_field_ms"]["sum"] + per_update["scratch_parents_ms"]["sum"]
            per_update["update_ms_sum"] = round(update_ms, 3)
            per_update["scratch_ms_sum"] = round(scratch_ms, 3)
            per_update["scratch_over_update"] = round(scratch_ms / update_ms, 3)
            entry["updates_apart"] = per_update
            last = (const, cap, out)
        report[f"const_{const:g}"] = entry
        print(json.dumps({f"const_{const:g}": entry}), flush=True)

    # the vertices of the labels with the smallest boxes against the oracle, at the last const
    if last is not None:
        const, cap, out = last
        voxels, _, _, out_offsets, branch_label, _, _ = (t.cpu().numpy() for t in out)
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

            sources = np.array([-1, to_local(np.array(roots_host[row]))], dtype=np.int32)
            # the oracle caps a radius at the crop's longest side, the device at the volume's: after the clip to the
            # box, which is the crop, either cube covers the same voxels
            want = fix_branching_ref.loop(crop, sources, dbf[box].cpu().numpy(), daf[box].cpu().numpy(),
                                          cost[box].cpu().numpy(), 1.25, const, max_paths=cap)
            got = to_local(voxels[vertex_label == row]).tolist()
            equal = equal and got == want.voxels
            checked += 1
        report["check"] = {
            "comparator": f"tests/fix_branching_ref.py loop (a heap Dijkstra per round) on each label's crop, const = "
                          f"{const:g}, at most {cap} rounds: the vertices in order",
            "labels_checked": checked, "labels_with_a_box_of_at_most_2e5_voxels": len(order), "all_equal": equal,
            "host_wall_s": round(time.perf_counter() - t0, 1),
        }
    text = json.dumps(report, indent=1)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", f"fix_branching_{n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
