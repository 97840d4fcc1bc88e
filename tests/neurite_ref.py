"""
Shared by test_neurite_cpu.py and test_gpu_neurite.py: the 160^3 neurite-like volume of golden g9
and the bounds the two files hold against it.

g9 (tests/golden/g9_neurite_160.npz, made by tests/golden/make_golden_neurite.py) is the
reference implementation's predict() with its defaults on synth_neurite_volume((160,) * 3, seed=0).

Bounds on |probability - g9|:
    fp32     5e-6, what the g6 tests hold (test_oracle_golden.py, test_gpu_parity.py)
    bf16x3   four times the deviation of the CPU emulation bf16x3_ref.emulate_unet on this volume,
             1.788e-6 (pred_sub; pred_tube 1.580e-6, pred_line 9.54e-7), the way
             test_gpu_bf16x3.py derives its g6 bound; test_neurite_cpu.py recomputes the figure
    fp16     1e-3 and bf16 4e-3: the bounds test_predict_16bit_default_config_vs_reference_golden
             holds on g6
"""

import functools

import numpy as np

from aind_exaspim_neuron_segmentation_amd.utils import synthetic

EDGE = 160
GOLDEN = "g9_neurite_160.npz"
CLIP = 1000
PERCENTILES = (1, 99.9)

FP32_TOL = 5e-6
BF16X3_EMULATION_DEVIATION = 1.788e-6
BF16X3_TOL = 4 * BF16X3_EMULATION_DEVIATION
TOL_16BIT = {"fp16": 1e-3, "bf16": 4e-3}


@functools.lru_cache(maxsize=1)
def volume():
    """The g9 input; read-only so that every test sees the same array."""
    vol = synthetic.synth_neurite_volume((EDGE, EDGE, EDGE), seed=0)
    vol.setflags(write=False)
    return vol


def deviations(pred, g):
    """|pred - g9| on the three fields of g9: (pred_sub, pred_line, pred_tube) error arrays."""
    o = [int(v) for v in g["tube_origin"]]
    n = g["pred_tube"].shape[1]
    tube = pred[:, o[0]:o[0] + n, o[1]:o[1] + n, o[2]:o[2] + n]
    return (np.abs(pred[:, ::5, ::5, ::5] - g["pred_sub"]),
            np.abs(pred[:, 80, 81, :] - g["pred_line"]),
            np.abs(tube - g["pred_tube"]))


def check_zero_masks(pred, g):
    zero = (pred == 0).all(axis=0)
    assert abs(zero.mean() - float(g["zero_fraction"])) < 1e-12
    np.testing.assert_array_equal(zero.all(axis=(1, 2)), g["zero_z"])
    np.testing.assert_array_equal(zero.all(axis=(0, 2)), g["zero_y"])
    np.testing.assert_array_equal(zero.all(axis=(0, 1)), g["zero_x"])
