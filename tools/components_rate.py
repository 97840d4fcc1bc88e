"""
Rate of the device connected-components front-end (run on the MI355X box):
    python tools/components_rate.py [--size 512] [--reps 5] [--check] [--out FILE]

On one size^3 volume, with HIP events, the median of --reps runs after one warm-up of each:
  neurite   affinities_to_components(..., return_device_tensor=True) on float32 binary affinities in
            get_affinity_channels' convention of the thresholded neurite-like volume
            (exaspim_synth_volume_neurite_u16 > NEURITE_FLOOR_MAX): aff_c[v] = on(v) & on(v + e_c);
  random    the same on uniform random float32 affinities at threshold 0.75, just at the bond
            percolation threshold of the cubic lattice: the adversarial case;
  download  what the front-end replaces: .cpu() of the same 12-byte-per-voxel float32 tensor;
  labels    .cpu() of the 4-byte-per-voxel int32 labels that leave the device instead.
--check also labels the neurite mask in foreground mode and compares it with scipy.ndimage.label,
array for array (both number components in raster order), which exercises the grid-stride paths of a
volume with more voxels than one launch has threads.
Prints one JSON line: per leg the median milliseconds, every repeat and voxels per second.
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
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from aind_exaspim_neuron_segmentation_amd import _native, inference
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    dev = torch.device("cuda:0")
    n = args.size
    vox = float(n) ** 3
    lib = _native.lib()

    raw = torch.empty((n, n, n), dtype=torch.int16, device=dev)
    _native.check(lib.exaspim_synth_volume_neurite_u16(raw.data_ptr(), _native.Block.make((n, n, n)), 0, None),
                  "synth_neurite")
    on = (raw.to(torch.int32) & 0xFFFF) > synthetic.NEURITE_FLOOR_MAX
    del raw
    neurite = torch.zeros((3, n, n, n), dtype=torch.float32, device=dev)
    neurite[0, :-1] = (on[:-1] & on[1:]).float()
    neurite[1, :, :-1] = (on[:, :-1] & on[:, 1:]).float()
    neurite[2, :, :, :-1] = (on[:, :, :-1] & on[:, :, 1:]).float()
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    random = torch.rand((3, n, n, n), dtype=torch.float32, device=dev, generator=gen)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    legs = {
        "neurite": lambda: inference.affinities_to_components(neurite, 0.5, 100, return_device_tensor=True),
        "random": lambda: inference.affinities_to_components(random, 0.75, 100, return_device_tensor=True),
        "download": lambda: neurite.cpu(),
    }
    res = {"size": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "legs": {}, "segments": {}}
    labels = None
    for kind, fn in legs.items():      # warm-up
        _, out = timed(fn)
        if kind != "download":
            res["segments"][kind] = int(out.max())
        if kind == "neurite":
            labels = out
        del out
    legs["labels"] = lambda: labels.cpu()
    timed(legs["labels"])
    times = {kind: [] for kind in legs}
    for _ in range(args.reps):
        for kind, fn in legs.items():
            ms, out = timed(fn)
            del out
            times[kind].append(ms)
    for kind, ts in times.items():
        med = statistics.median(ts)
        res["legs"][kind] = {"median_ms": med, "ms": ts, "voxels_per_s": vox / (med * 1e-3)}
    med = {k: v["median_ms"] for k, v in res["legs"].items()}
    res["components_plus_labels_ms"] = med["neurite"] + med["labels"]
    res["beats_download"] = res["components_plus_labels_ms"] < med["download"]

    if args.check:
        from scipy import ndimage

        got = inference.affinities_to_components(on.float(), 0.5, 0)
        want, count = ndimage.label(on.cpu().numpy())
        res["check"] = {"foreground_equals_ndimage_label": bool(np.array_equal(got, want)), "segments": int(count)}
        # binary affinities of that mask: the same components without the one-voxel ones
        sizes = np.bincount(want.ravel())
        res["check"]["segments_above_100"] = int((sizes[1:] > 100).sum())
        res["check"]["affinity_count_agrees"] = res["check"]["segments_above_100"] == res["segments"]["neurite"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.check and not (res["check"]["foreground_equals_ndimage_label"] and res["check"]["affinity_count_agrees"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
