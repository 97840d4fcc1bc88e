"""
Per-layer activation ranges on the neurite-like volume (run on the MI355X box):
    python tools/neurite_ranges.py [--out FILE]

Runs UNet3D.fp16_report (synthetic weights, seed 1) on two batches of normalised 32^3 patches cut
from the 160^3 neurite volume (seed 0, clip 1000, percentiles (1, 99.9)): four patches centred on
the brightest tube voxels, and four patches that hold no tube voxel at all. Prints one JSON line
with both reports and, per layer, the ratio of the float32 ranges.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EDGE, P = 160, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D
    from aind_exaspim_neuron_segmentation_amd.utils import synthetic

    vol = synthetic.synth_neurite_volume((EDGE,) * 3, seed=0)
    clipped = np.minimum(vol, 1000)
    mn, mx = np.percentile(clipped, (1, 99.9))
    norm = np.clip((clipped - mn) / (mx - mn + 1e-8), 0, 1).astype(np.float32)
    tube = vol > synthetic.NEURITE_FLOOR_MAX

    def cut(o):
        return norm[o[0]:o[0] + P, o[1]:o[1] + P, o[2]:o[2] + P]

    bright, work = [], vol.astype(np.int64)
    while len(bright) < 4:
        c = np.unravel_index(int(np.argmax(work)), work.shape)
        o = tuple(min(max(int(v) - P // 2, 0), EDGE - P) for v in c)
        bright.append(o)
        work[o[0]:o[0] + P, o[1]:o[1] + P, o[2]:o[2] + P] = 0
    empty = []
    for z in range(0, EDGE - P + 1, 8):
        for y in range(0, EDGE - P + 1, 8):
            for x in range(0, EDGE - P + 1, 8):
                if len(empty) < 4 and not tube[z:z + P, y:y + P, x:x + P].any():
                    empty.append((z, y, x))
    assert len(empty) == 4, "no tube-free 32^3 windows found"

    dev = torch.device("cuda:0")
    sd = synthetic.synth_state_dict(3, 1, seed=1)
    model = UNet3D(output_channels=3, compute_dtype="fp16")
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model.to(dev).eval()
    res = {"patch": P, "percentiles": [float(mn), float(mx)]}
    for name, origins in (("tube", bright), ("background", empty)):
        x = torch.from_numpy(np.stack([cut(o) for o in origins])[:, None].copy()).to(dev)
        rep = model.fp16_report(x)
        rep["origins"] = [list(o) for o in origins]
        rep["input_max"] = float(x.max().item())
        rep["input_mean"] = float(x.mean().item())
        res[name] = rep
    res["tube_over_background_fp32_absmax"] = [
        (a / b if b else None) for a, b in zip(res["tube"]["fp32_absmax"], res["background"]["fp32_absmax"])]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
