"""
Rate of the streamed watershed fragments (run on the MI355X box):
    python tools/watershed_stream_rate.py [--size 512] [--slab-depth 64] [--reps 5] [--slow-s 10]
                                          [--edge-capacity 16777216] [--fragments-only] [--out FILE]

On DESIGN 6g's neurite-like size^3 float32 tensor (tools/watershed_rate.py's), with HIP events, the median of
--reps runs after one warm-up of each leg, the two legs of a pair alternating in one process:
  streamed / whole      WatershedStream at --slab-depth (push of every slab, finish, apply on the resident
                        labels) against exaspim_watershed_fragments, both at (0.1, 0.9999), min_size 0, on the
                        same device tensor; torch.equal of the labels; ids used next to the fragment count,
                        which is the cost of the conservative marks;
  agglomerate_<r>_<p>   agglomerate_affinities_streaming(fragments="watershed", device_merge_rounds=r,
                        premerge_size=p) from a host array against agglomerate_affinities with the same options
                        on the device tensor, r in (0, 64), p in (0, 100); the labels compared for equality. The
                        streamed call includes the upload of the slabs and the download of the labels, the whole
                        call the download of the labels. A leg whose warm-up takes longer than --slow-s seconds
                        is not repeated (reps_used 1), as in tools/watershed_rate.py. Both calls get
                        --edge-capacity slots: the default of 2^22 is too few for this tensor's contacts.
--fragments-only runs the first pair alone: the form to run under a kernel trace for the mask kernels' times.
Prints one JSON line; --out also writes it to a file, after every pair.
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
    ap.add_argument("--slab-depth", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow-s", type=float, default=10.0)
    ap.add_argument("--edge-capacity", type=int, default=1 << 24)
    ap.add_argument("--fragments-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from aind_exaspim_neuron_segmentation_amd import _native, inference
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    dev = torch.device("cuda:0")
    n, depth = args.size, args.slab_depth
    lib = _native.lib()
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
    del p
    torch.cuda.synchronize()

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

    def pair(name, legs, same):
        """Warm-up of both legs, then --reps alternating rounds; same(a, b) compares the warm-ups' outputs."""
        entry = {}
        outs = {}
        for leg, fn in legs.items():
            ms, outs[leg] = timed(fn)
            entry[leg] = {"warmup_ms": ms, "ms": []}
            log(f"{name}: warm-up of {leg} {ms:.1f} ms")
        a, b = outs.values()
        entry["equal"] = bool(same(a, b))
        del outs, a, b
        repeat = {leg: entry[leg]["warmup_ms"] <= args.slow_s * 1e3 for leg in legs}
        for _ in range(args.reps):
            for leg, fn in legs.items():
                if repeat[leg]:
                    ms, out = timed(fn)
                    del out
                    entry[leg]["ms"].append(ms)
        for leg in legs:
            ts = entry[leg]["ms"] or [entry[leg]["warmup_ms"]]
            entry[leg].update(median_ms=statistics.median(ts), reps_used=len(ts))
            log(f"{name}: {leg} median {entry[leg]['median_ms']:.2f} ms of {len(ts)}")
        return entry

    res = {"size": n, "slab_depth": depth, "reps": args.reps, "device": torch.cuda.get_device_name(0), "low": LOW,
           "high": HIGH, "pairs": {}}
    resident = torch.empty((n, n, n), dtype=torch.int32, device=dev)
    used = {}

    def streamed():
        ws = inference.WatershedStream((n, n, n), LOW, HIGH, 0, device=dev, id_capacity=min(n ** 3, 2 ** 31 - 2) // 2)
        for z0 in range(0, n, depth):
            ws.push(aff[:, z0:z0 + depth], z0, resident[z0:z0 + depth])
        _, used["fragments"] = ws.finish()
        used["ids"] = ws.ids_used
        return ws.apply(resident)

    def whole():
        return inference._watershed_on_device(aff, LOW, HIGH, 0)[0]

    res["pairs"]["fragments"] = pair("fragments", {"streamed": streamed, "whole": whole}, torch.equal)
    res["pairs"]["fragments"].update(ids_used=used["ids"], fragments=used["fragments"])
    write(res)
    if not args.fragments_only:
        del resident
        torch.cuda.empty_cache()
        host = aff.cpu().numpy()
        thresholds, min_size = [0.6, 0.8, 0.9], 100
        for rounds in (0, 64):
            for floor in (0, 100):
                options = dict(fragments="watershed", aff_threshold_low=LOW, aff_threshold_high=HIGH,
                               premerge_size=floor, device_merge_rounds=rounds)
                t0 = time.perf_counter()
                res["pairs"][f"agglomerate_{rounds}_{floor}"] = pair(
                    f"agglomerate_{rounds}_{floor}",
                    {"streamed": lambda: inference.agglomerate_affinities_streaming(
                        host, thresholds, min_size, slab_depth=depth, id_capacity=n ** 3 // 2,
                        edge_capacity=args.edge_capacity, **options),
                     "whole": lambda: inference.agglomerate_affinities(aff, thresholds, min_size,
                                                                       edge_capacity=args.edge_capacity, **options)},
                    np.array_equal)
                res["pairs"][f"agglomerate_{rounds}_{floor}"]["wall_s"] = time.perf_counter() - t0
                write(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
