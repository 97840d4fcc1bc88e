"""The network variants the plan tests run next to the base network (test_gpu_variant_plans.py,
test_gpu_variant_window.py, test_variant_window_cases_cpu.py, the variant cases of test_gpu_workspace.py and
test_gpu_clipped_forward.py). Plain data and helpers, no fixtures, no device.

What the engine decides from padded channel counts (pad to 32: conv_row_mode_ok, conv_can_fuse_head,
conv_carry_t14_tile_depth):
  row mode of inc.3, the fused head and everything trimmed, clipped or carried at the first level need a level 0
  whose padded width c0p is no multiple of 64; the second level carries only on 64-cout slices, c1p % 64 == 0.
"""

from carry_ref import _RowModel

# name -> output channels, trilinear, width multiplier, synth_state_dict seed, and what the engine is expected to
# answer: row mode (hence a first-level carry) and a second-level carry at a geometry that offers both
VARIANTS = {
    "foreground":    dict(out=1, trilinear=True, wm=1, seed=4, row=True, level1=True),      # the reference's own non-affinity model
    "convt":         dict(out=3, trilinear=False, wm=1, seed=8, row=True, level1=True),     # ConvTranspose3d decoder, level 4 is 512 wide
    "three_quarter": dict(out=4, trilinear=True, wm=0.75, seed=3, row=True, level1=True),   # 24 of 32 and 48 of 64: padding on both carried levels
    "half":          dict(out=2, trilinear=True, wm=0.5, seed=3, row=True, level1=False),   # 16 of 32; level 1 is 32-cout: pairs, no triples
    "double":        dict(out=3, trilinear=True, wm=2, seed=3, row=False, level1=False),    # 64-cout level 0: the plain plan whatever is asked
}
NAMES = list(VARIANTS)
ROW_NAMES = [n for n in NAMES if VARIANTS[n]["row"]]
LEVEL1_NAMES = [n for n in NAMES if VARIANTS[n]["level1"]]


def window_cases():
    """The two window_fuzz_cases.HAND cases the predict() ladder runs on every variant (with the seeds
    test_gpu_window_fuzz.py gives them): the smallest one, and the one whose chain is cut at every second batch."""
    import window_fuzz_cases as W

    return {"smallest": dict(W.HAND[3], seed=403), "cut": dict(W.HAND[2], seed=402)}


def channels(name):
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import unet_channels

    return [int(c) for c in unet_channels(VARIANTS[name]["wm"])]


def padded(name):
    """(c0p, c1p): the stored widths of the first two levels."""
    c = channels(name)
    return tuple(-(-v // 32) * 32 for v in c[:2])


def host_model(name, level1=True):
    """carry_ref's stand-in for the engine of this variant (level1=False: CARRY_Z1 off or no room for triples)."""
    c0p, c1p = padded(name)
    return _RowModel(level1=level1, c0p=c0p, c1p=c1p)


def make(make_model, dev, name, dtype):
    """(model, state dict) through test_gpu_bf16x3.make_model."""
    v = VARIANTS[name]
    return make_model(dev, out_channels=v["out"], seed=v["seed"], trilinear=v["trilinear"], wm=v["wm"],
                      compute_dtype=dtype)
