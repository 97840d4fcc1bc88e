"""
Rate of the overlap table of two label volumes (run on the MI355X box):
    python tools/overlaps_rate.py [--size 512] [--reps 7] [--premerge-size 100] [--out FILE]

On the neurite-like size^3 tensor of tools/watershed_rate.py, two pairs of int32 volumes made in this run:
  premerge     the exact segments (agglomerate_affinities, fragments="watershed") against the segments with
               premerge_size = --premerge-size: about 1e2 labels each and long runs;
  fragments    the watershed fragments against the exact segments: about 1e6 distinct pairs, the workgroups'
               LDS tables overflow in most chunks that hold foreground.
Per pair, with HIP events, the median of --reps runs after one warm-up, both legs on the same tensors in the
same process:
  call         exaspim_label_overlaps (reset + add + finish) into buffers allocated before the clock starts;
  add          exaspim_label_overlaps_add alone, after a reset outside the clock;
  baseline     the packed-torch.unique formulation that tools/watershed_rate.py's agreement() used to be:
               both volumes clamped at 0 and packed into one int64 key per voxel, torch.unique with counts.
Reported per leg: median_ms, ms, and for call / add the achieved bytes per second against the floor of 8 bytes
per voxel. The call's table is compared with the baseline's, row for row after sorting, and for the premerge pair
the largest-overlap agreement is computed both through compare_segmentations and by the old helper's rule.
Prints one JSON line; --out also writes it to a file.
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOW, HIGH, COMPONENTS_THRESHOLD = 0.1, 0.9999, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--premerge-size", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from aind_exaspim_neuron_segmentation_amd import _native, inference
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    dev = torch.device("cuda:0")
    n = args.size
    vox = n ** 3
    lib = _native.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)

    def log(*what):
        print(*what, file=sys.stderr, flush=True)

    def neurite():      # tools/watershed_rate.py's tensor
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
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def median_of(fn):
        timed(fn)      # warm-up
        ts = [timed(fn)[0] for _ in range(args.reps)]
        return {"median_ms": statistics.median(ts), "ms": ts}

    def packed_unique(a, b):
        keys = a.clamp_min(0).to(torch.int64) << 32 | b.clamp_min(0).to(torch.int64)
        return torch.unique(keys, return_counts=True)

    def old_agreement(exact, merged):
        """tools/watershed_rate.py's former helper: the largest-overlap agreement over the voxels either calls
        foreground, by one packed torch.unique."""
        either = (exact > 0) | (merged > 0)
        total = int(either.sum())
        if total == 0:
            return 1.0
        a, b = exact[either].to(torch.int64), merged[either].to(torch.int64)
        pairs, counts = torch.unique(a * (int(b.max()) + 1) + b, return_counts=True)
        seg = pairs // (int(b.max()) + 1)
        best = torch.zeros(int(seg.max()) + 1, dtype=torch.int64, device=dev)
        best.scatter_reduce_(0, seg, counts, "amax")
        return float(best[1:].sum()) / total

    aff = neurite()
    thresholds, min_size = [0.6, 0.8, 0.9], 100
    frags, count = inference._watershed_on_device(aff, LOW, HIGH, 0)
    k = int(count.cpu()[0])
    capacity = 1 << 24
    n_edges = inference._region_graph_device(frags, aff, k, capacity)[4]
    edge_capacity = max(1 << 16, 1 << (2 * n_edges - 1).bit_length())
    log(f"{k} fragments, {n_edges} edges")

    def segments(floor):
        return inference.agglomerate_affinities(
            aff, thresholds, min_size, fragment_threshold=COMPONENTS_THRESHOLD, edge_capacity=edge_capacity,
            return_device_tensor=True, fragments="watershed", aff_threshold_low=LOW, aff_threshold_high=HIGH,
            premerge_size=floor)

    exact = segments(0)
    merged = segments(args.premerge_size)
    del aff
    torch.cuda.empty_cache()
    res = {"size": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "fragments": k,
           "premerge_size": args.premerge_size, "floor_bytes_per_voxel": 8, "pairs": {}}

    for name, (a, b) in {"premerge": (exact, merged), "fragments": (frags, exact)}.items():
        keys, key_counts = packed_unique(a, b)
        distinct = int(keys.numel())
        pair_capacity = max(1 << 12, 1 << (2 * distinct - 1).bit_length())
        need = lib.exaspim_label_overlaps_workspace_bytes(pair_capacity)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        pairs = torch.empty((pair_capacity, 2), dtype=torch.int32, device=dev)
        counts = torch.empty(pair_capacity, dtype=torch.int64, device=dev)
        state = torch.empty(2, dtype=torch.int32, device=dev)

        def call():
            _native.check(lib.exaspim_label_overlaps(a.data_ptr(), b.data_ptr(), vox, pair_capacity, pairs.data_ptr(),
                                                     counts.data_ptr(), state.data_ptr(), ws.data_ptr(), need, None),
                          "exaspim_label_overlaps")

        def add():
            _native.check(lib.exaspim_label_overlaps_add(a.data_ptr(), b.data_ptr(), vox, pair_capacity,
                                                         ws.data_ptr(), need, None), "exaspim_label_overlaps_add")

        entry = {"distinct_pairs": distinct, "pair_capacity": pair_capacity,
                 "labels_a": int(torch.unique(a).numel()), "labels_b": int(torch.unique(b).numel()),
                 "background_pair_voxels": int(((a <= 0) & (b <= 0)).sum()), "legs": {}}
        entry["legs"]["call"] = median_of(call)
        _native.check(lib.exaspim_label_overlaps_reset(pair_capacity, ws.data_ptr(), need, None), "reset")
        entry["legs"]["add"] = median_of(add)      # the table goes on growing: the same keys, larger counts
        entry["legs"]["baseline"] = median_of(lambda: packed_unique(a, b))
        for leg in ("call", "add"):
            entry["legs"][leg]["bytes_per_s"] = 8.0 * vox / (entry["legs"][leg]["median_ms"] * 1e-3)
        entry["speedup_over_baseline"] = entry["legs"]["baseline"]["median_ms"] / entry["legs"]["call"]["median_ms"]

        call()
        torch.cuda.synchronize()
        found, overflow = (int(v) for v in state.cpu())
        got_keys = pairs[:found, 0].to(torch.int64) << 32 | pairs[:found, 1].to(torch.int64)
        order = torch.argsort(got_keys)
        entry["equals_baseline"] = bool(overflow == 0 and found == distinct and torch.equal(got_keys[order], keys)
                                        and torch.equal(counts[:found][order], key_counts))
        assert entry["equals_baseline"], name
        if name == "premerge":
            scores = inference.compare_segmentations(a, b, pair_capacity=pair_capacity)
            entry["scores"] = scores
            entry["agreement_old_helper"] = old_agreement(a, b)
            entry["agreement_same"] = scores["largest_overlap_agreement"] == entry["agreement_old_helper"]
        log(name, json.dumps(entry))
        res["pairs"][name] = entry
        del ws, pairs, counts, state, keys, key_counts
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
