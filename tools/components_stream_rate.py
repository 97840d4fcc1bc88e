"""
What labelling a volume slab by slab costs over labelling it whole (run on the MI355X box):
    python tools/components_stream_rate.py [--size 512] [--slab 64] [--reps 5] [--predict] [--out FILE]

On one size^3 volume that still fits the device, with HIP events, the median of --reps runs after one
warm-up of each, on the two tensors of tools/components_rate.py (binary affinities of the thresholded
neurite-like volume at 0.5; uniform random affinities at 0.75, the bond percolation threshold):
  whole     exaspim_components on the whole tensor (affinities_to_components, labels stay on the device);
  streamed  ComponentsStream over z slabs of --slab planes of the same tensor, labels staying on the
            device: the sum of its three parts, which are timed in the same run --
  slabs     every push() (the slab-local passes, the id compaction, the seam pass),
  finish    finish() (the id table; includes the one read of the device's id count and overflow flag),
  apply     apply() over the whole volume of provisional ids.
The streamed labels are compared with the whole-volume ones (torch.equal) and the ids used are reported.
--predict adds, host array to host array with the default model (fp16, batch 16, one warm-up, one run):
  predict_streaming             float32 affinities leave the device, 12 B/voxel;
  predict_components_streaming  int32 labels leave it, 4 B/voxel (threshold 0.5, min size 100).
Prints one JSON line.
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--slab", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--predict", action="store_true")
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
    del on
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    random = torch.rand((3, n, n, n), dtype=torch.float32, device=dev, generator=gen)

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def whole(aff, thr):
        a = event()
        labels = inference.affinities_to_components(aff, thr, 100, return_device_tensor=True)
        b = event()
        b.synchronize()
        return {"whole": a.elapsed_time(b)}, labels

    def streamed(aff, thr):
        labels = torch.empty((n, n, n), dtype=torch.int32, device=dev)
        # slabs are contiguous (3, d, H, W) tensors when they arrive; cutting them out of the whole
        # tensor is not part of the labelling
        parts = [(z0, min(z0 + args.slab, n)) for z0 in range(0, n, args.slab)]
        slabs = [aff[:, z0:z1].contiguous() for z0, z1 in parts]
        cs = inference.ComponentsStream((n, n, n), thr, 100, device=dev)
        a = event()
        for (z0, z1), slab in zip(parts, slabs):
            cs.push(slab, z0, labels[z0:z1])
        b = event()
        _, count = cs.finish()
        c = event()
        cs.apply(labels)
        d = event()
        d.synchronize()
        t = {"slabs": a.elapsed_time(b), "finish": b.elapsed_time(c), "apply": c.elapsed_time(d)}
        t["streamed"] = t["slabs"] + t["finish"] + t["apply"]
        return t, labels, count, cs.ids_used

    res = {"size": n, "slab_depth": args.slab, "reps": args.reps, "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, aff, thr in (("neurite", neurite, 0.5), ("random", random, 0.75)):
        _, want = whole(aff, thr)
        _, got, count, used = streamed(aff, thr)
        case = {"segments": count, "ids_used": used, "equals_whole_volume": bool(torch.equal(got, want)),
                "segments_whole": int(want.max())}
        del want, got
        times = {}
        for _ in range(args.reps):
            for t in (whole(aff, thr)[0], streamed(aff, thr)[0]):
                for k, v in t.items():
                    times.setdefault(k, []).append(v)
        case["legs"] = {k: {"median_ms": statistics.median(v), "ms": v} for k, v in times.items()}
        med = {k: v["median_ms"] for k, v in case["legs"].items()}
        case["streamed_over_whole"] = med["streamed"] / med["whole"]
        case["voxels_per_s_streamed"] = vox / (med["streamed"] * 1e-3)
        res["cases"][name] = case

    if args.predict:
        from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

        del neurite, random
        torch.cuda.empty_cache()
        sd = synthetic.synth_state_dict(3, 1, seed=1)
        model = UNet3D(output_channels=3, compute_dtype="fp16")
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        model.to(dev).eval()
        raw = torch.empty((n, n, n), dtype=torch.int16, device=dev)
        _native.check(lib.exaspim_synth_volume_neurite_u16(raw.data_ptr(), _native.Block.make((n, n, n)), 0, None),
                      "synth_neurite")
        vol = raw.cpu().numpy().view(np.uint16)
        del raw
        legs = {
            "predict_streaming": lambda: inference.predict_streaming(vol, model, verbose=False),
            "predict_components_streaming": lambda: inference.predict_components_streaming(vol, model, verbose=False),
        }
        pred = {}
        for kind, fn in legs.items():
            fn()
            t0 = time.perf_counter()
            out = fn()
            pred[kind] = {"seconds": time.perf_counter() - t0, "dtype": str(out.dtype), "bytes": int(out.nbytes)}
            if kind == "predict_components_streaming":
                pred[kind]["segments"] = int(out.max())
            del out
        pred["labels_over_affinities"] = (pred["predict_components_streaming"]["seconds"]
                                          / pred["predict_streaming"]["seconds"])
        res["predict"] = pred

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(c["equals_whole_volume"] for c in res["cases"].values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
