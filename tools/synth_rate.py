"""
Time of the two device-side volume generators (run on the MI355X box):
    python tools/synth_rate.py [--size 1024] [--reps 10] [--out FILE]

Times exaspim_synth_volume_u16 (uniform) and exaspim_synth_volume_neurite_u16 on one size^3 uint16
volume with HIP events, alternating launch by launch after one warm-up of each. Prints one JSON
line: per generator the median milliseconds, every repeat, and the bytes written per second.
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from aind_exaspim_neuron_segmentation_amd import _native

    dev = torch.device("cuda:0")
    n = args.size
    lib = _native.lib()
    gens = {"uniform": lib.exaspim_synth_volume_u16, "neurite": lib.exaspim_synth_volume_neurite_u16}
    raw = torch.empty((n, n, n), dtype=torch.int16, device=dev)
    blk = _native.Block.make((n, n, n))

    def run(kind):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _native.check(gens[kind](raw.data_ptr(), blk, 0, None), kind)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for kind in gens:
        run(kind)
    times = {kind: [] for kind in gens}
    for _ in range(args.reps):
        for kind in gens:
            times[kind].append(run(kind))
    res = {"size": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "generators": {}}
    for kind, ts in times.items():
        med = statistics.median(ts)
        res["generators"][kind] = {"median_ms": med, "ms": ts, "bytes_per_s": 2.0 * n ** 3 / (med * 1e-3)}
    res["neurite_over_uniform_time"] = res["generators"]["neurite"]["median_ms"] / res["generators"]["uniform"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
