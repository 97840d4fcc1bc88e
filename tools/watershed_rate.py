"""
Rate of the watershed fragments (run on the MI355X box):
    python tools/watershed_rate.py [--size 512] [--reps 5] [--slow-s 20] [--max-fragments 4000000]
                                   [--no-whole | --premerge-only] [--premerge-floors 100,25,400] [--out FILE]

On one size^3 float32 volume per case, with HIP events, the median of --reps runs after one warm-up of
each leg, all legs of a case on the same tensors in the same run:
  watershed         exaspim_watershed_fragments at (0.1, 0.9999), min_size 0;
  components        exaspim_components at 0.5, min_size 0: the yardstick, the same passes after another
                    edge mask;
  whole_components  inference.agglomerate_affinities(..., return_device_tensor=True) with the default
  whole_watershed   fragments and with fragments="watershed": fragments, region graph, the download of
                    the graph, exaspim_agglomerate on the host (timed separately, host_ms), the table's
                    upload and apply_table;
  whole_watershed_premerge
                    the same call with premerge_size = the first of --premerge-floors (100, the default
                    min_segment_size); whole_watershed_premerge_<floor> for the other floors. For
                    each floor one more call outside the timed ones gives "premerge": fragments and contacts
                    after each round, the device time of each round by HIP events, the host merging time,
                    the segment count, and the agreement with whole_watershed's labels of this run: over the
                    voxels that are foreground in either, the sum over exact segments of the largest overlap
                    with one pre-merged segment, divided by the voxel count. Where whole_watershed is skipped
                    for its fragment count the pre-merged call still runs if its rounds leave no more than
                    --max-fragments (no agreement then: there is nothing to agree with);
  download          .cpu() of the 12-byte-per-voxel affinities;
  labels            .cpu() of the 4-byte-per-voxel int32 labels.
A leg whose warm-up takes longer than --slow-s seconds is not repeated (reps_used 1). A whole_* leg is
not run at all when its fragments number more than --max-fragments: the host merging then takes minutes
(DESIGN 6e measured 203 s for 1.2e7 fragments), and the entry says so ("skipped").
--no-whole leaves the whole_* legs out: the form to run under a kernel trace for per-pass times.
--premerge-only runs, per case, the watershed, the region graph and the pre-merge rounds of the first
floor on the device --reps times and nothing else: the form to trace the pre-merge's passes.
Cases: the neurite-like and the uniform random tensors of tools/region_graph_rate.py.
Prints one JSON line; --out also writes it to a file, after every case.
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOW, HIGH, COMPONENTS_THRESHOLD = 0.1, 0.9999, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow-s", type=float, default=20.0)
    ap.add_argument("--max-fragments", type=int, default=4000000)
    ap.add_argument("--no-whole", action="store_true")
    ap.add_argument("--premerge-only", action="store_true")
    ap.add_argument("--premerge-floors", default="100,25,400")
    ap.add_argument("--cases", default="neurite,random")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from aind_exaspim_neuron_segmentation_amd import _native, inference
    # agglomerate_affinities resolves agglomerate in segmentation's globals: that is the name to rebind
    from aind_exaspim_neuron_segmentation_amd import segmentation as seg_module
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    dev = torch.device("cuda:0")
    n = args.size
    vox = float(n) ** 3
    lib = _native.lib()
    dims = _native.int3((n, n, n))
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)

    def neurite():
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

    def random():
        return torch.rand((3, n, n, n), dtype=torch.float32, device=dev, generator=gen)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def log(*what):
        print(*what, file=sys.stderr, flush=True)

    def write(res):
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")

    thresholds, min_size = [0.6, 0.8, 0.9], 100
    floors = [int(v) for v in args.premerge_floors.split(",") if v]

    def premerge_leg(floor):
        return "whole_watershed_premerge" + ("" if floor == floors[0] else f"_{floor}")

    def agreement(exact, merged):
        """Largest-overlap agreement of two label volumes over the voxels either calls foreground: the overlap
        table on the device. The packed-torch.unique form this used to be is tools/overlaps_rate.py's
        baseline."""
        return inference.compare_segmentations(exact, merged)["largest_overlap_agreement"]

    res = {"size": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "low": LOW, "high": HIGH,
           "components_threshold": COMPONENTS_THRESHOLD, "thresholds": thresholds, "min_segment_size": min_size,
           "cases": {}}
    makers = {"neurite": neurite, "random": random}
    for kind in args.cases.split(","):
        aff = makers[kind]()
        torch.cuda.synchronize()
        entry = {"legs": {}, "fragments": {}, "edges": {}, "edge_capacity": {}, "segments": {}, "skipped": {}}
        fragment_legs = {
            "watershed": lambda: inference._watershed_on_device(aff, LOW, HIGH, 0),
            "components": lambda: inference._components_on_device(aff, COMPONENTS_THRESHOLD, 0),
        }
        host = []

        def edge_capacity_for(name):
            """Twice the edges of a sizing run, so that the table's load stays under a half."""
            labels, count = fragment_legs[name]()
            k = int(count.cpu()[0])
            entry["fragments"][name] = k
            entry["background_voxels_" + name] = int((labels == 0).sum())
            if k > args.max_fragments:
                entry["skipped"]["whole_" + name] = (f"{k} fragments, more than --max-fragments "
                                                     f"{args.max_fragments}: the host merging would take minutes")
                if name != "watershed":
                    return None
            capacity = min(1 << 30, 1 << (3 * n ** 3 - 1).bit_length())
            while capacity > (1 << 16) and lib.exaspim_region_graph_workspace_bytes(dims, k, capacity) * 2 > \
                    torch.cuda.mem_get_info(dev)[0] // 2:
                capacity >>= 1
            n_edges = inference._region_graph_device(labels, aff, k, capacity)[4]
            entry["edges"][name] = n_edges
            capacity = max(1 << 16, 1 << (2 * n_edges - 1).bit_length())
            entry["edge_capacity"][name] = capacity
            del labels
            torch.cuda.empty_cache()
            return capacity

        def premerge_rounds(capacity, floor, timings=None):
            """The watershed, its graph and the pre-merge rounds, all on the device: (K', E') per round."""
            labels, count = fragment_legs["watershed"]()
            k = int(count.cpu()[0])
            graph = inference._region_graph_device(labels, aff, k, capacity)
            return inference._premerge_on_device(*graph[:5], thresholds[-1], floor, 4, capacity, timings)[6]

        def premerge_detail(capacity, floor, exact):
            labels, count = fragment_legs["watershed"]()
            stats = {}
            table = inference._premerged_table(labels, aff, int(count.cpu()[0]), thresholds, min_size, capacity,
                                               floor, 4, stats)
            _native.check(lib.exaspim_apply_label_table(labels.data_ptr(), labels.numel(), table.data_ptr(),
                                                        table.numel(), None), "apply_label_table")
            torch.cuda.synchronize()
            if exact is not None:
                stats["agreement"] = agreement(exact, labels)
            return stats

        def whole(name, capacity, floor=0):
            def call():
                real = seg_module.agglomerate

                def clocked(*a, **kw):
                    t0 = time.perf_counter()
                    out = real(*a, **kw)
                    host.append((time.perf_counter() - t0) * 1e3)
                    return out

                seg_module.agglomerate = clocked
                try:
                    return inference.agglomerate_affinities(
                        aff, thresholds, min_size, fragment_threshold=COMPONENTS_THRESHOLD, edge_capacity=capacity,
                        return_device_tensor=True, fragments=name, aff_threshold_low=LOW, aff_threshold_high=HIGH,
                        premerge_size=floor)
                finally:
                    seg_module.agglomerate = real
            return call

        if args.premerge_only:
            capacity = edge_capacity_for("watershed")
            entry["premerge_only"] = {"floor": floors[0], "round_ms": [], "history": None}
            for _ in range(1 + args.reps):      # the first one is the warm-up
                timings = []
                entry["premerge_only"]["history"] = premerge_rounds(capacity, floors[0], timings)
                entry["premerge_only"]["round_ms"].append(timings)
            res["cases"][kind] = entry
            del aff
            torch.cuda.empty_cache()
            write(res)
            continue

        legs = dict(fragment_legs)
        details = {}      # leg -> (capacity, floor)
        for name in () if args.no_whole else ("components", "watershed"):
            capacity = edge_capacity_for(name)
            log(f"{kind}: {name}: {entry['fragments'][name]} fragments, {entry['edges'].get(name)} edges")
            if capacity is None:
                continue
            if "whole_" + name not in entry["skipped"]:
                legs["whole_" + name] = whole(name, capacity)
            if name == "watershed":
                for floor in floors:
                    left = premerge_rounds(capacity, floor)[-1][0]
                    if left > args.max_fragments:
                        entry["skipped"][premerge_leg(floor)] = (
                            f"{left} fragments after the rounds, more than --max-fragments {args.max_fragments}")
                        continue
                    legs[premerge_leg(floor)] = whole(name, capacity, floor)
                    details[premerge_leg(floor)] = (capacity, floor)
        legs["download"] = lambda: aff.cpu()

        reps = {}
        segmentation = exact = None
        for name, fn in legs.items():      # warm-up
            host.clear()
            ms, out = timed(fn)
            reps[name] = 1 if ms > args.slow_s * 1e3 else args.reps
            entry["legs"][name] = {"warmup_ms": ms}
            if name.startswith("whole_"):
                segmentation = out
                if name == "whole_watershed":
                    exact = out
                entry["segments"][name[6:]] = int(out.max())
                entry["legs"][name]["warmup_host_ms"] = host[-1]
            del out
            log(f"{kind}: warm-up of {name} {ms:.1f} ms")
        if segmentation is None:
            segmentation = fragment_legs["watershed"]()[0]
        legs["labels"] = lambda: segmentation.cpu()
        reps["labels"] = args.reps
        entry["legs"]["labels"] = {"warmup_ms": timed(legs["labels"])[0]}
        for name, fn in legs.items():
            leg = entry["legs"][name]
            host.clear()
            if reps[name] == 1 and name != "labels":
                ts = [leg["warmup_ms"]]
                if name.startswith("whole_"):
                    leg["host_ms"] = leg["warmup_host_ms"]
            else:
                ts = []
                for _ in range(reps[name]):
                    ms, out = timed(fn)
                    del out
                    ts.append(ms)
                if name.startswith("whole_"):
                    leg["host_ms"] = statistics.median(host)
            med = statistics.median(ts)
            leg.update({"median_ms": med, "ms": ts, "reps_used": len(ts), "voxels_per_s": vox / (med * 1e-3)})
            log(f"{kind}: {name} median {med:.2f} ms of {len(ts)}")
        entry["premerge"] = {}
        for name, (capacity, floor) in details.items():
            stats = premerge_detail(capacity, floor, exact)
            stats["floor"] = floor
            entry["premerge"][name] = stats
            log(f"{kind}: {name}: {stats}")
        res["cases"][kind] = entry
        del aff, segmentation, exact
        torch.cuda.empty_cache()
        write(res)      # after every case: a later one may be cut short
    print(json.dumps(res))


if __name__ == "__main__":
    main()
