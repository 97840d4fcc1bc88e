"""
Generates tests/golden/g10_components.npz: the REFERENCE implementation's
img_util.get_affinity_channels on a label mask of the 40 x 70 x 100 neurite-like
synthetic volume (utils.synthetic.synth_neurite_volume, seed 0):

    labels = scipy.ndimage.label(volume > NEURITE_FLOOR_MAX)      (6-connectivity)
    aff    = img_util.get_affinity_channels(labels)               (img_util.py:159-216)

Run once, in the build container, where the reference is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_components.py

Same approach as make_golden_neurite.py: the reference's module is imported at run
time, its absent third-party imports are replaced by empty stub modules. Only the
.npz travels; no test reads the reference. The archive is written with fixed zip
timestamps, so a second run gives the same bytes.

Fields
    aff      uint8 (3, 40, 70, 100): the reference's binary affinities (0 / 1)
    labels   int32 (40, 70, 100): the label mask they were made from
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

from scipy import ndimage  # noqa: E402

from aind_exaspim_neuron_segmentation.utils import img_util as ref_img  # noqa: E402

from aind_exaspim_neuron_segmentation_amd.utils import synthetic  # noqa: E402

NAME = "g10_components.npz"
SHAPE = (40, 70, 100)


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
    vol = synthetic.synth_neurite_volume(SHAPE, seed=0)
    labels, n = ndimage.label(vol > synthetic.NEURITE_FLOOR_MAX)
    labels = labels.astype(np.int32)
    aff = ref_img.get_affinity_channels(labels)
    assert aff.shape == (3,) + SHAPE and set(np.unique(aff).tolist()) <= {0.0, 1.0}
    sizes = np.bincount(labels.ravel())[1:]
    path = os.path.join(HERE, NAME)
    save_deterministic(path, aff=aff.astype(np.uint8), labels=labels)
    print(f"wrote {NAME}: {os.path.getsize(path) / 1024:.1f} KiB, {n} segments of "
          f"{int(sizes.min())} to {int(sizes.max())} voxels, {int((sizes > 100).sum())} above 100")


if __name__ == "__main__":
    main()
