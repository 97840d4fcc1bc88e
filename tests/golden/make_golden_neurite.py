"""
Generates tests/golden/g9_neurite_160.npz: the REFERENCE implementation's
predict() (CPU, float32, its defaults: patch 96, overlap 32, trim 8, batch 16,
clip 1000, percentiles (1, 99.9)) on the 160^3 neurite-like synthetic volume
(utils.synthetic.synth_neurite_volume, seed 0) with the synthetic weights
synth_state_dict(output_channels=3, seed=1).

Run once, in the build container, where the reference is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_neurite.py

Same approach as make_golden.py: the reference's predict() and UNet3D are
imported at run time, its absent third-party imports are replaced by empty stub
modules. Only the .npz travels; no test reads the reference. The archive is
written with fixed zip timestamps, so a second run gives the same bytes.

Fields
    pred_sub, pred_line, zero_fraction, zero_z, zero_y, zero_x   as in g6_default_160.npz
    percentiles   float64 (2,): the (mn, mx) the reference's normalize() got from np.percentile
    tube_origin   int64 (3,): corner of a 24^3 block centred on the brightest voxel
                  (first in C order), moved inside the region predict() writes
    pred_tube     float32 (3, 24, 24, 24): the prediction on that block
"""

import io
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

for _name in [
    "kimimaro", "waterz", "gcsfs", "s3fs", "tifffile", "zarr",
    "google", "google.cloud", "google.cloud.storage",
]:
    sys.modules[_name] = types.ModuleType(_name)
_fr = types.ModuleType("fastremap")
for _n in ("mask_except", "renumber", "unique"):
    setattr(_fr, _n, None)
sys.modules["fastremap"] = _fr
sys.path.insert(0, "/root/reference/src")

import torch  # noqa: E402

from aind_exaspim_neuron_segmentation import inference as ref_inf  # noqa: E402
from aind_exaspim_neuron_segmentation.machine_learning.unet3d import (  # noqa: E402
    UNet3D as RefUNet3D,
)
from aind_exaspim_neuron_segmentation.utils import img_util as ref_img  # noqa: E402

from aind_exaspim_neuron_segmentation_amd.utils import synthetic  # noqa: E402

NAME = "g9_neurite_160.npz"
EDGE = 160
TUBE = 24
TRIM = 8


def save_deterministic(path, **arrays):
    """np.savez_compressed with fixed member timestamps (same input, same bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    torch.manual_seed(0)
    sd = synthetic.synth_state_dict(output_channels=3, seed=1)
    model = RefUNet3D(output_channels=3)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model.eval()
    vol = synthetic.synth_neurite_volume((EDGE, EDGE, EDGE), seed=0)

    seen = []
    np_percentile = np.percentile

    def recording_percentile(img, q, *args, **kwargs):
        res = np_percentile(img, q, *args, **kwargs)
        seen.append(np.array(res, dtype=np.float64))
        return res

    ref_img.np.percentile = recording_percentile
    try:
        pred = ref_inf.predict(vol, model, verbose=False)
    finally:
        ref_img.np.percentile = np_percentile
    assert len(seen) == 1 and seen[0].shape == (2,), seen
    assert pred.dtype == np.float32 and pred.shape == (3, EDGE, EDGE, EDGE)

    peak = np.unravel_index(int(np.argmax(vol)), vol.shape)
    origin = np.array(
        [min(max(int(p) - TUBE // 2, TRIM), EDGE - TRIM - TUBE) for p in peak], dtype=np.int64
    )
    sl = tuple(slice(int(o), int(o) + TUBE) for o in origin)
    assert vol[sl].max() == vol.max()
    zero = (pred == 0).all(axis=0)
    path = os.path.join(HERE, NAME)
    save_deterministic(
        path,
        pred_sub=pred[:, ::5, ::5, ::5].copy(),
        pred_line=pred[:, 80, 81, :].copy(),
        zero_fraction=np.array(zero.mean()),
        zero_z=zero.all(axis=(1, 2)), zero_y=zero.all(axis=(0, 2)),
        zero_x=zero.all(axis=(0, 1)),
        percentiles=seen[0],
        tube_origin=origin,
        pred_tube=pred[(slice(None),) + sl].copy(),
    )
    print(f"wrote {NAME}: {os.path.getsize(path) / 1024:.1f} KiB, percentiles {seen[0]}, "
          f"tube block at {origin.tolist()}, brightest voxel {int(vol.max())}")


if __name__ == "__main__":
    main()
