"""
The engine (csrc/engine.hip, forward()) chains about 30 launches through one caller-owned workspace
that it never clears, and several plans leave parts of it unwritten on purpose: the trimmed forward
(up4.3 writes [trim, size - trim), up4.0 one voxel more, the upsample before it margin trim - 2, thin
launches for the remainders of the z-column tiles), the row mode of inc.3, split-K partial sums in the
padded-input area, padded channels of narrow networks. Each is right only if no launch reads what no
earlier launch of the SAME forward wrote.

Here every forward entry runs, through the C ABI, on a workspace this file owns and fills first:
0x00 bytes (what a fresh process usually sees), 0xFF bytes (NaN in float32, IEEE half and bfloat16 and in
both halves of a split word), 0x7F bytes (3.39e38 in float32 and bfloat16, NaN in half: survives max,
clamps and a saturating sigmoid) and the workspace a forward of another input at a larger batch left
behind. The kept voxels -- everything, or [trim, size - trim)^3 of a trimmed plan -- must have the same
bits under all four and hold no NaN; the margin of a trimmed plan keeps the output's sentinel; 256 guard
bytes behind the workspace and behind the output stay as they were. The 0xFF run is also held to the
reference (golden g4 at 96^3, the oracle's unet_forward otherwise) at the tolerance the dtype's own tests use.
A NaN or a changed bit means that a kept output depends on memory this forward did not write.
"""

import numpy as np
import pytest
import torch

import layer_ref as R
import variant_models as V
from aind_exaspim_neuron_segmentation_amd import _native, inference
from aind_exaspim_neuron_segmentation_amd.utils import synthetic
from test_gpu_bf16x3 import PROB_TOL as PROB_TOL_BF16X3
from test_gpu_bf16x3 import dev, make_model, oracle  # noqa: F401  (fixtures)
from test_gpu_parity import PROB_TOL_16BIT, PROB_TOL_FP32

pytestmark = pytest.mark.gpu

PROB_TOL = dict(PROB_TOL_16BIT, fp32=PROB_TOL_FP32, bf16x3=PROB_TOL_BF16X3)   # max abs on the probabilities
DTYPES = ["fp32", "fp16", "bf16", "bf16x3"]
FILLS = ["0x00", "0xFF", "0x7F", "stale"]
GUARD = 256              # bytes behind the workspace and behind the output
SENTINEL = 0x5A          # byte the output and its guard are filled with (0x5A5A5A5A: a finite float32)
SENTINEL_WORD = 0x5A5A5A5A

# model variants: (synth_state_dict seed, trilinear, width multiplier, output channels); "base" is the model of
# golden g4; "foreground", "three_quarter" and "half2" (width 0.5 with 2 outputs) are variant_models.py's
VARIANTS = {"base": (1, True, 1, 3), "convt": (8, False, 1, 3), "half": (3, True, 0.5, 3), "double": (3, True, 2, 3)}
VARIANTS.update({{"half": "half2"}.get(k, k): (v["seed"], v["trilinear"], v["wm"], v["out"]) for k, v in V.VARIANTS.items()
                 if k not in ("convt", "double")})
assert all(VARIANTS[k] == tuple(V.VARIANTS[k][f] for f in ("seed", "trilinear", "wm", "out")) for k in ("convt", "double"))
ROW_VARIANTS = ["foreground", "convt", "three_quarter", "half2"]     # variant_models.ROW_NAMES under this file's names

# case -> (patch, n, row_stride): the smallest shapes at which each mechanism is live
CASES = {
    1: ((96, 96, 96), 1, 0),   # production geometry: up4.0 extent 82 = 80 + 2 on y and x, split-K at 12^3 / 6^3, strip upsample
    2: ((32, 32, 48), 2, 0),   # thin remainders on both axes: up4.0 extent 18 = 2 * 8 + 2 on y, 34 = 2 * 16 + 2 on x (trim 8)
    3: ((32, 32, 64), 2, 0),   # remainder on y only (trim 4: 26 = 24 + 2; 58 has none)
    4: ((16, 16, 16), 3, 0),   # smallest patch, level 4 is 1^3
    5: ((16, 32, 32), 2, 0),   # trims 1, 2, 3: upsample margin 0, 0, 1 against up4.0 margin 0, 1, 2
    6: ((16, 16, 64), 3, 32),  # row mode, overlap 32 = stride
    7: ((16, 16, 96), 2, 64),  # row mode at the default x geometry
}
SEED = {1: 0, 2: 110, 3: 120, 4: 130, 5: 140, 6: 150, 7: 160}   # case 1: the volume of golden g4
REFERENCE = {1: "golden", 2: "oracle", 4: "oracle"}


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- shared state: one model per (dtype, variant), one input per (case, seed, n), one reference ----------
@pytest.fixture(scope="module")
def state(dev):  # noqa: F811
    s = {"models": {}, "inputs": {}, "refs": {}}
    yield s
    s.clear()


def _model(state, dev, dtype, variant):  # noqa: F811
    key = (dtype, variant)
    if key not in state["models"]:
        seed, trilinear, wm, out = VARIANTS[variant]
        state["models"][key] = make_model(dev, out_channels=out, seed=seed, trilinear=trilinear, wm=wm,
                                          compute_dtype=dtype)
    return state["models"][key]


def _inputs(state, dev, case, n, seed):  # noqa: F811
    """The n patches of `case` cut from one seeded volume along x (side by side, or row_stride apart):
    the device volume, the patch starts and the float32 batch of the reference-shaped gather."""
    key = (case, n, seed)
    if key not in state["inputs"]:
        patch, _, stride = CASES[case]
        step = stride or patch[2]
        vol = synthetic.synth_volume(patch[:2] + (step * (n - 1) + patch[2],), seed=seed)
        mn, mx = np.percentile(np.minimum(vol, 1000), (1, 99.9))
        dvol = inference.DeviceVolume.from_array(vol, dev)
        starts = torch.tensor([(0, 0, step * i) for i in range(n)], dtype=torch.int32, device=dev)
        kw = dict(clip=np.uint16(1000), mn=mn, mx=mx)
        x = inference._get_batch_inputs(dvol, starts, patch, dev, **kw)
        state["inputs"][key] = {"vol": dvol, "starts": starts, "kw": kw, "x": x, "prepared": {}}
    return state["inputs"][key]


def _prepared(inp, layout, patch, dev):  # noqa: F811
    """The batch in the first convolution's operand layout, gathered into a 0xFF-filled buffer: the gather
    has to write its own zero border."""
    if layout not in inp["prepared"]:
        n = int(inp["starts"].shape[0])
        buf = torch.empty((n,) + tuple(p + 2 for p in patch), dtype=torch.float32, device=dev)
        buf.view(torch.uint8).fill_(0xFF)
        inp["prepared"][layout] = inference._get_batch_inputs(inp["vol"], inp["starts"], patch, dev, layout=layout,
                                                              out=buf, **inp["kw"])
    return inp["prepared"][layout]


def _reference(state, oracle, golden, case, variant, x, sd):  # noqa: F811
    """Probabilities of the reference: ("golden", g4's subsampled sigmoid) or ("oracle", the whole batch)."""
    kind = REFERENCE.get(case)
    if kind is None:
        return None
    key = (case, variant)
    if key not in state["refs"]:
        if kind == "golden":
            assert variant == "base"
            want = torch.from_numpy(golden("g4_single_patch.npz")["sigmoid_sub"].copy())[None]
        else:
            want = torch.sigmoid(oracle.unet_forward(x.cpu(), oracle.OracleModel(sd).sd))
        state["refs"][key] = (kind, want)
    return state["refs"][key]


# ---- one forward on buffers this file owns -----------------------------------------------------------------
def _call(lib, entry, handle, inp, layout, out, n, patch, trim, row_stride, ws, ws_bytes, dev):  # noqa: F811
    d, h, w = patch
    stream = torch.cuda.current_stream(dev).cuda_stream
    keep = None   # (alive until the synchronize below)
    if entry == "forward":
        rc = lib.exaspim_unet_forward(handle, inp["x"].data_ptr(), out.data_ptr(), n, d, h, w, 1, ws.data_ptr(),
                                      ws_bytes, stream)
    elif entry == "absmax":
        keep = torch.zeros(22, dtype=torch.float32, device=dev)
        rc = lib.exaspim_unet_forward_absmax(handle, inp["x"].data_ptr(), out.data_ptr(), n, d, h, w, 1,
                                             keep.data_ptr(), ws.data_ptr(), ws_bytes, stream)
    elif entry == "trimmed":
        rc = lib.exaspim_unet_forward_trimmed(handle, inp["x"].data_ptr(), out.data_ptr(), n, d, h, w, 1, trim,
                                              ws.data_ptr(), ws_bytes, stream)
    elif entry == "prepared":
        rc = lib.exaspim_unet_forward_prepared(handle, _prepared(inp, layout, patch, dev).data_ptr(), out.data_ptr(),
                                               n, d, h, w, 1, trim, ws.data_ptr(), ws_bytes, stream)
    else:
        assert entry == "row" and row_stride > 0
        rc = lib.exaspim_unet_forward_prepared_row(handle, _prepared(inp, layout, patch, dev).data_ptr(),
                                                   out.data_ptr(), n, d, h, w, 1, trim, row_stride, ws.data_ptr(),
                                                   ws_bytes, stream)
    _native.check(rc, entry)
    torch.cuda.synchronize()
    del keep


def _run(state, dev, model, entry, case, trim, fill):  # noqa: F811
    """One forward of `case` through `entry` on a workspace filled with `fill` -> float32 output on the CPU.
    Asserts that the guards behind the workspace and behind the output are intact."""
    lib = _native.lib()
    patch, n, row_stride = CASES[case]
    d, h, w = patch
    handle = model._ensure_engine(dev)
    layout = model.input_layout(dev)
    need = lib.exaspim_unet_workspace_bytes(handle, n, d, h, w)
    assert need, _native.last_error()
    if fill == "stale":
        # another input, one patch more, the same entry: its activations are what this forward finds
        big = lib.exaspim_unet_workspace_bytes(handle, n + 1, d, h, w)
        assert big >= need + GUARD
        ws = torch.empty(big, dtype=torch.uint8, device=dev)
        ws.fill_(0xA5)
        other = _inputs(state, dev, case, n + 1, SEED[case] + 1000)
        scratch = torch.empty((n + 1, model.output_channels, d, h, w), dtype=torch.float32, device=dev)
        _call(lib, entry, handle, other, layout, scratch, n + 1, patch, trim, row_stride, ws, big, dev)
        del scratch
    else:
        ws = torch.empty(need + GUARD, dtype=torch.uint8, device=dev)
        ws.fill_(int(fill, 16))
    ws_guard = ws[need: need + GUARD].clone()
    numel = n * model.output_channels * d * h * w
    out = torch.empty(numel + GUARD // 4, dtype=torch.float32, device=dev)
    out.view(torch.uint8).fill_(SENTINEL)
    inp = _inputs(state, dev, case, n, SEED[case])
    _call(lib, entry, handle, inp, layout, out, n, patch, trim, row_stride, ws, need, dev)
    assert torch.equal(ws[need: need + GUARD], ws_guard), f"{fill}: bytes behind workspace_bytes were written"
    assert bool((_bits(out[numel:]) == SENTINEL_WORD).all()), f"{fill}: bytes behind the output were written"
    return out[:numel].view(n, model.output_channels, d, h, w).cpu()


def _check(state, dev, oracle, golden, dtype, variant, entry, case, trim, options=0):  # noqa: F811
    model, sd = _model(state, dev, dtype, variant)
    patch, n, _ = CASES[case]
    # the plan trims only with the head fused into up4.3 (engine.hip): a 32-channel level 0, no separate head,
    # not the range probe; every other plan writes the whole patch
    trimmed = (trim > 0 and all(2 * trim < s for s in patch) and model.channels[0] <= 32 and entry != "absmax"
               and not options & _native.OPT_SEPARATE_HEAD)
    kept = torch.zeros((n, model.output_channels) + patch, dtype=torch.bool)
    kept[(Ellipsis,) + tuple(slice(trim, s - trim) if trimmed else slice(None) for s in patch)] = True
    model.engine_options = options
    try:
        outs = {fill: _run(state, dev, model, entry, case, trim, fill) for fill in FILLS}
    finally:
        model.engine_options = 0
    what = f"case {case} {dtype} {variant} {entry} trim {trim} options {options}"
    first = _bits(outs[FILLS[0]])[kept]
    for fill, out in outs.items():
        nans = int(torch.isnan(out[kept]).sum())
        assert nans == 0, f"{what}, fill {fill}: {nans} of {int(kept.sum())} kept voxels are NaN"
        if trimmed:
            written = int((_bits(out)[~kept] != SENTINEL_WORD).sum())
            assert written == 0, f"{what}, fill {fill}: {written} of {int((~kept).sum())} margin voxels were written"
        differ = _bits(out)[kept] != first
        if differ.any():
            where = kept.nonzero()[differ][:4].tolist()
            raise AssertionError(f"{what}: {int(differ.sum())} of {int(kept.sum())} kept voxels differ between the "
                                 f"fills {FILLS[0]} and {fill}, first at {where}")
    ref = _reference(state, oracle, golden, case, variant, _inputs(state, dev, case, n, SEED[case])["x"], sd)
    if ref is not None:
        kind, want = ref
        got, k = outs["0xFF"], kept
        if kind == "golden":
            got, k = got[..., ::8, ::8, ::8], kept[..., ::8, ::8, ::8]
        err = float((got - want).abs()[k].max())
        print(f"{what}: 0xFF-filled workspace vs {kind}: {err:.3e} over {int(k.sum())} voxels (tolerance {PROB_TOL[dtype]:.1e})")
        assert err < PROB_TOL[dtype], f"{what}: {err:.3e} from the reference ({kind})"


# ---- the cases -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ["trimmed", "prepared"])
@pytest.mark.parametrize("case,trim", [(1, 8), (2, 8), (3, 4)])
def test_trimmed_plans(state, dev, oracle, golden, case, trim, entry, dtype):  # noqa: F811
    _check(state, dev, oracle, golden, dtype, "base", entry, case, trim)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ["forward", "absmax"])
def test_smallest_patch_full_forward(state, dev, oracle, golden, entry, dtype):  # noqa: F811
    _check(state, dev, oracle, golden, dtype, "base", entry, 4, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("trim", [1, 2, 3])
def test_small_trims(state, dev, oracle, golden, trim, dtype):  # noqa: F811
    _check(state, dev, oracle, golden, dtype, "base", "trimmed", 5, trim)


def _assert_row_mode(case, dtype, channels=(32, 64, 128, 256, 512)):
    """conv_row_mode_ok, the engine's own predicate, says yes to inc.3 of this case."""
    probe = R.load_probe()
    (_, _, w), n, stride = CASES[case]
    dt = {"fp16": "f16", "bf16": "bf16"}[dtype]
    cout = R.plan_conv(probe, list(channels), 3, dt, 0)[5]
    assert probe.probe_conv_row_mode_ok(R.DTYPES[dt], cout, n, w, stride, 1) == 1


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case,trim", [(6, 0), (6, 4), (7, 4)])
def test_row_mode(state, dev, oracle, golden, case, trim, dtype):  # noqa: F811
    _assert_row_mode(case, dtype)
    _check(state, dev, oracle, golden, dtype, "base", "row", case, trim)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("variant", ROW_VARIANTS)
def test_row_mode_on_model_variants(state, dev, oracle, golden, variant, dtype):  # noqa: F811
    """The row entry at the default x geometry on 1, 2 and 4 outputs, ConvTranspose3d up blocks and widths 0.75 and
    0.5: inc.3's row and border launches write the padded channels of x1 and its max-pool themselves (the `stale`
    fill leaves another forward's activations there)."""
    model, _ = _model(state, dev, dtype, variant)
    _assert_row_mode(7, dtype, model.channels)
    _check(state, dev, oracle, golden, dtype, variant, "row", 7, 4)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("trim", [0, 4])
def test_row_entry_on_the_per_patch_encoder(state, dev, oracle, golden, trim, dtype):  # noqa: F811
    _check(state, dev, oracle, golden, dtype, "base", "row", 6, trim, options=_native.OPT_PER_PATCH_ENCODER)


OPTIONS = {"separate_pool": _native.OPT_SEPARATE_POOL, "separate_head": _native.OPT_SEPARATE_HEAD,
           "plain_upsample": _native.OPT_PLAIN_UPSAMPLE, "upsample_per_thread": _native.OPT_UPSAMPLE_PER_THREAD,
           "first_per_group": _native.OPT_FIRST_PER_GROUP}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ["trimmed", "prepared"])
@pytest.mark.parametrize("option", list(OPTIONS))
def test_engine_options(state, dev, oracle, golden, option, entry, dtype):  # noqa: F811
    _check(state, dev, oracle, golden, dtype, "base", entry, 2, 8, options=OPTIONS[option])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ["trimmed", "prepared"])
@pytest.mark.parametrize("variant", ["convt", "half", "double"])
def test_model_variants(state, dev, oracle, golden, variant, entry, dtype):  # noqa: F811
    """ConvTranspose3d up blocks; width 0.5 (16 real of 32 channels: the padded ones must be written as zeros,
    0 x stale NaN is NaN); width 2 (64-cout level 0: no thin remainders, no fused head, nothing trimmed)."""
    _check(state, dev, oracle, golden, dtype, variant, entry, 2, 8)
