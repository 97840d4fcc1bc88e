"""
What the dominant-edge contraction buys (run on the MI355X box):
    python tools/dominant_rate.py [--size 512] [--reps 5] [--rounds 64] [--premerge-size 0]
                                  [--cutoff-divisor 64] [--out FILE]

On the neurite-like size^3 float32 tensor of tools/watershed_rate.py and its watershed fragments at
(0.1, 0.9999), all in one run on the same tensor:
  rounds        the watershed, the region graph and the dominant rounds on the device, one warm-up and
                --reps repetitions: K and E after every round, and per round the median of the HIP-event
                milliseconds;
  whole_rounds  agglomerate_affinities(fragments="watershed", device_merge_rounds=--rounds,
                return_device_tensor=True): the whole call by HIP events around it and the host merging
                (exaspim_agglomerate) by the clock, one warm-up and, if that took less than --slow-s
                seconds, the median of --reps more;
  whole_zero    the same call with device_merge_rounds=0, the path without the rounds: the comparator,
                measured here and now;
  equal         whether the two label volumes are equal, voxel for voxel.
--premerge-size S > 0 runs both whole calls with premerge_size=S (the rounds then start from the
pre-merged graph) and leaves the "rounds" leg on the full graph.
--cutoff-divisor D other than 64 is an experiment, not the library's behaviour: for this run a round
that removes fewer than max(1, K // D) fragments is the last (segmentation._dominant_round_is_last is
rebound), to see what the rounds beyond the library's cut-off would cost and save.
Prints one JSON line; --out also writes it to a file.
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOW, HIGH = 0.1, 0.9999


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--premerge-size", type=int, default=0)
    ap.add_argument("--cutoff-divisor", type=int, default=64)
    ap.add_argument("--slow-s", type=float, default=5.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from aind_exaspim_neuron_segmentation_amd import _native, inference
    # agglomerate_affinities resolves agglomerate in segmentation's globals: that is the name to rebind
    from aind_exaspim_neuron_segmentation_amd import segmentation as seg_module
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    if args.cutoff_divisor != 64:
        seg_module._dominant_round_is_last = lambda k, k_new: k - k_new < max(1, k // args.cutoff_divisor)
    dev = torch.device("cuda:0")
    n = args.size
    lib = _native.lib()
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    thresholds, min_size = [0.6, 0.8, 0.9], 100

    def log(*what):
        print(*what, file=sys.stderr, flush=True)

    # the neurite-like tensor of tools/watershed_rate.py
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
    del p
    torch.cuda.synchronize()

    # a sizing run: twice the edges, so that the table's load stays under a half
    labels, count = inference._watershed_on_device(aff, LOW, HIGH, 0)
    k = int(count.cpu()[0])
    capacity = min(1 << 30, 1 << (3 * n ** 3 - 1).bit_length())
    n_edges = inference._region_graph_device(labels, aff, k, capacity)[4]
    capacity = max(1 << 16, 1 << (2 * n_edges - 1).bit_length())
    del labels
    torch.cuda.empty_cache()
    res = {"size": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "low": LOW, "high": HIGH,
           "thresholds": thresholds, "min_segment_size": min_size, "rounds_limit": args.rounds,
           "cutoff_divisor": args.cutoff_divisor, "premerge_size": args.premerge_size, "fragments": k,
           "edges": n_edges, "edge_capacity": capacity}
    log(f"{k} fragments, {n_edges} edges, capacity {capacity}")

    per_run, history = [], None
    for _ in range(1 + args.reps):      # the first one is the warm-up
        labels, count = inference._watershed_on_device(aff, LOW, HIGH, 0)
        graph = inference._region_graph_device(labels, aff, int(count.cpu()[0]), capacity)
        timings = []
        history = inference._contract_dominant_on_device(*graph[:5], thresholds[-1], args.rounds, capacity, timings)[6]
        per_run.append(timings)
        del labels, graph
    res["rounds"] = {"history": history, "round_ms": per_run,
                     "median_ms": [statistics.median(run[i] for run in per_run[1:]) for i in range(len(history))]}
    res["rounds"]["median_ms_total"] = sum(res["rounds"]["median_ms"])
    log(f"rounds: {history}, {res['rounds']['median_ms_total']:.2f} ms in all")

    host = []

    def whole(rounds):
        real = seg_module.agglomerate

        def clocked(*a, **kw):
            t0 = time.perf_counter()
            out = real(*a, **kw)
            host.append((time.perf_counter() - t0) * 1e3)
            return out

        seg_module.agglomerate = clocked
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        try:
            a.record()
            out = inference.agglomerate_affinities(aff, thresholds, min_size, edge_capacity=capacity,
                                                   return_device_tensor=True, fragments="watershed",
                                                   aff_threshold_low=LOW, aff_threshold_high=HIGH,
                                                   premerge_size=args.premerge_size, device_merge_rounds=rounds)
            b.record()
            b.synchronize()
        finally:
            seg_module.agglomerate = real
        return a.elapsed_time(b), host[-1], out

    volumes = {}
    for name, rounds in (("whole_rounds", args.rounds), ("whole_zero", 0)):
        ms, host_ms, volumes[name] = whole(rounds)
        leg = {"warmup_ms": ms, "warmup_host_ms": host_ms, "segments": int(volumes[name].max())}
        runs = [(ms, host_ms)]
        if ms <= args.slow_s * 1e3:
            runs = [whole(rounds)[:2] for _ in range(args.reps)]
        leg.update(ms=[r[0] for r in runs], host_ms_all=[r[1] for r in runs], reps_used=len(runs),
                   median_ms=statistics.median(r[0] for r in runs), host_ms=statistics.median(r[1] for r in runs))
        res[name] = leg
        log(f"{name}: {leg['median_ms']:.1f} ms, of which the host merging {leg['host_ms']:.1f} ms")
    res["equal"] = bool(torch.equal(volumes["whole_rounds"], volumes["whole_zero"]))
    log(f"equal: {res['equal']}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
