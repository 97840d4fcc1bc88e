"""
Throughput of compute_dtype="bf16x3" against the float32 mode in ONE process on one device
(run on the MI355X box):  python tools/dtype_rate.py [--size 512] [--batch 8] [--steps 5] [--out FILE]
                          [--modes fp16,bf16x3] [--volume uniform,neurite]

Times device-resident predict steps (sharding.predict_shard over the whole volume, as bench.py does) (BASELINE configs[1]: 512^3, batch 8, synthetic uint16
volume on the device, result left on the device) for both modes, alternating mode by mode so
that clock and temperature drift hit both alike, after a warm-up of each. Prints one JSON line:
voxels/s per mode (median of the timed steps), every step's seconds, the spread between repeats
((max - min) / median) and the ratio of the medians. The comparison base is the float32 mode in
the same run, never a number from another run or box. --volume picks the input (default uniform,
the behaviour above); "uniform,neurite" times every mode on both inputs in the same alternation,
which is how the data dependence of the step time is measured.
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="fp32,bf16x3")
    ap.add_argument("--volume", default="uniform",
                    help="comma-separated inputs: uniform (splitmix64 %% 2000) and/or neurite (sparse tubes on a dim floor); "
                         "with more than one, the legs alternate volume by volume and mode by mode")
    ap.add_argument("--out", default=None)
    ap.add_argument("--options", type=lambda s: int(s, 0), default=0, help="engine option bits (_native.OPT_*)")
    args = ap.parse_args()

    import torch

    from aind_exaspim_neuron_segmentation_amd import _native, inference
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    dev = torch.device("cuda:0")
    sd = synthetic.synth_state_dict(3, 1, seed=1)
    models = {}
    for mode in args.modes.split(","):
        m = UNet3D(output_channels=3, compute_dtype=mode)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        m.engine_options = args.options
        models[mode] = m.to(dev).eval()

    import numpy as np

    from aind_exaspim_neuron_segmentation_amd import sharding

    n = args.size
    gshape = (n, n, n)
    generators = {"uniform": _native.lib().exaspim_synth_volume_u16,
                  "neurite": _native.lib().exaspim_synth_volume_neurite_u16}
    kinds = args.volume.split(",")
    volumes = {}
    for kind in kinds:
        if kind not in generators:
            ap.error(f"--volume: unknown input {kind!r} (uniform, neurite)")
        raw = torch.empty(gshape, dtype=torch.int16, device=dev)
        _native.check(generators[kind](raw.data_ptr(), _native.Block.make(gshape), 0, None), "synth")
        volumes[kind] = inference.DeviceVolume(raw, np.uint16, (0, 0, 0), gshape)
    torch.cuda.synchronize()
    plan = inference.SlidingWindow(gshape, (96, 96, 96), (32, 32, 32), 8)
    shard = sharding.Shard(plan, (1, 1), 0)

    def step(mode, kind):
        # the device-resident step bench.py times: predict over one shard that is the whole volume
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sharding.predict_shard(volumes[kind], models[mode], plan, shard, n_channels=3, batch_size=args.batch,
                                     brightness_clip=1000, normalization_percentiles=(1, 99.9), n_streams=1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        del out
        return dt

    # one leg per (mode, volume); with the default single volume a leg is named by its mode alone
    legs = [(mode if len(kinds) == 1 else f"{mode}/{kind}", mode, kind) for mode in models for kind in kinds]
    for _, mode, kind in legs:
        for _ in range(args.warmup):
            step(mode, kind)
    times = {name: [] for name, _, _ in legs}
    for _ in range(args.steps):
        for name, mode, kind in legs:    # alternating
            times[name].append(step(mode, kind))

    vox = float(n) ** 3
    res = {"size": n, "batch": args.batch, "steps": args.steps, "device": torch.cuda.get_device_name(0),
           "options": args.options, "volume": args.volume, "library": os.environ.get("EXASPIM_LIB", "in-tree"), "modes": {}}
    for mode, ts in times.items():
        med = statistics.median(ts)
        res["modes"][mode] = {"voxels_per_s": vox / med, "median_s": med, "step_s": ts,
                              "spread": (max(ts) - min(ts)) / med}
    if "fp32" in times and "bf16x3" in times:
        res["bf16x3_over_fp32"] = res["modes"]["bf16x3"]["voxels_per_s"] / res["modes"]["fp32"]["voxels_per_s"]
    if len(kinds) > 1 and "uniform" in kinds and "neurite" in kinds:
        res["neurite_over_uniform"] = {
            mode: res["modes"][f"{mode}/neurite"]["voxels_per_s"] / res["modes"][f"{mode}/uniform"]["voxels_per_s"]
            for mode in models}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
