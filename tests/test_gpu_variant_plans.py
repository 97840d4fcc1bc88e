"""
Row mode, the forward clipped to the volume and the planes of both levels carried along z, through the C ABI,
on the network variants of variant_models.py: 1, 2 and 4 outputs under the fused head, ConvTranspose3d up blocks,
widths 0.75 and 0.5 (padded channels in the caller's carry buffers, which hold stale bytes and not zeros; at
width 0.5 a 32-cout second level that cannot carry) and width 2 (a 64-cout level 0: no row mode, no fused head,
nothing trimmed, clipped or carried, whatever the caller asks for).

One geometry, the smallest at which both levels carry: n = 2 patches of (48, 16, 64), 32 apart along x, forward A
at z = 0 and forward B at z = 16 of one seeded volume, trim 4 (test_gpu_carry1_forward.GEOMETRIES). Per variant
and 16-bit storage type (width 2 in float32 as well):

  table    the engine's own answers -- conv_row_mode_ok, exaspim_unet_carry_planes, exaspim_unet_carry1_planes --
           are variant_models.py's row of the table.
  anchor   exaspim_unet_forward on batch B with the sigmoid against the CPU oracle's unet_forward, within
           test_gpu_parity's PROB_TOL_16BIT / PROB_TOL_FP32, set on the base network and held here as they are
           (measured on MI355X, fp16 / bf16 against 1e-3 / 4e-3: foreground 2.9e-4 / 1.8e-3, convt 9.0e-5 / 6.6e-4,
           three_quarter 3.5e-4 / 2.5e-3, half 1.8e-4 / 1.6e-3, double 3.6e-4 / 2.7e-3; double fp32 1.1e-6 against
           5e-6). Every step below is bit for bit and inherits this reference.
  row      exaspim_unet_forward_prepared_row with engine options 0 = the same entry under
           EXASPIM_OPT_PER_PATCH_ENCODER = the anchor on the kept voxels; the trimmed margin keeps its sentinel.
  clipped  keep_hi = (39, 9, 42): odd on z and y, x cut inside the second patch. The row entry's bits inside the
           box, the sentinel outside, under the workspace fills 0x00, 0xFF and 0x7F.
  carry    A carries out, B carries in, every caller buffer and the workspace filled with 0x00, 0xFF or 0x7F (and
           the workspace again between A and B): B has the clipped entry's bits, no NaN, sentinels outside, all
           guards intact. First level alone (options 0: the border launch carries and inc.0 skips planes; and
           EXASPIM_OPT_CARRY_MAIN_ONLY), then both levels; once on logits.
  refusals width 0.5: the second level's range is (0, 0) and a request to take level-1 planes over is refused; width
           2: the first level's is (0, 0) and any carry is refused. Nothing is launched: every buffer keeps its
           sentinel.

Width 2 runs the full pass everywhere: its row and clipped entries write every voxel and equal the anchor on all.
"""

import ctypes

import pytest
import torch

import layer_ref as R
import test_gpu_carry1_forward as C1
import variant_models as V
from aind_exaspim_neuron_segmentation_amd import _native, inference
from test_gpu_bf16x3 import dev, make_model, oracle  # noqa: F401  (fixtures)
from test_gpu_parity import PROB_TOL_16BIT, PROB_TOL_FP32

pytestmark = pytest.mark.gpu

PROB_TOL = dict(PROB_TOL_16BIT, fp32=PROB_TOL_FP32)
GEOMETRY = "48x16x64 shift 16"
PATCH, STRIDE, SHIFT, SPAN1 = C1.GEOMETRIES[GEOMETRY]
N, TRIM = 2, C1.TRIM
KEEP_HI = (PATCH[0] - TRIM - 5, PATCH[1] - TRIM - 3, PATCH[2] - TRIM - 18)
FILLS = C1.FILLS
SENTINEL, SENTINEL_WORD = C1.SENTINEL, C1.SENTINEL_WORD
CASES = [(name, dtype) for name in V.NAMES for dtype in ("fp16", "bf16")] + [("double", "fp32")]
ROW_CASES = [c for c in CASES if V.VARIANTS[c[0]]["row"]]
LEVEL1_CASES = [c for c in CASES if V.VARIANTS[c[0]]["level1"]]
ids = lambda c: f"{c[0]}-{c[1]}"     # noqa: E731


@pytest.fixture(scope="module")
def state(dev):  # noqa: F811
    s = {}
    yield s
    s.clear()


# ---- shared state: one model per (variant, dtype), its prepared batches, one reference per variant -------------
def _variant(state, dev, name, dtype):  # noqa: F811
    if ("variant", name, dtype) not in state:
        state[("variant", name, dtype)] = V.make(make_model, dev, name, dtype)
    return state[("variant", name, dtype)]


def _setup(state, dev, name, dtype, keep_hi=None, sigmoid=1):  # noqa: F811
    model, _ = _variant(state, dev, name, dtype)
    return C1._setup(state, dev, dtype, GEOMETRY, model=model, tag=name, keep_hi=keep_hi, sigmoid=sigmoid)


def _kept(model, hi=None):
    """The voxels a trimmed (and clipped to hi) forward writes. The engine trims only with the head fused into
    up4.3, a 32-channel level 0 (engine.hip): a wider network writes every voxel."""
    kept = torch.zeros((N, model.output_channels) + PATCH, dtype=torch.bool)
    if model.channels[0] > 32:
        kept[:] = True
    else:
        hi = hi or tuple(p - TRIM for p in PATCH)
        kept[(Ellipsis,) + tuple(slice(TRIM, k) for k in hi)] = True
    return kept


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want, kept, what):
    differ = _bits(got)[kept] != _bits(want)[kept]
    assert not differ.any(), (f"{what}: {int(differ.sum())} of {int(kept.sum())} kept voxels differ, first at "
                              f"{kept.nonzero()[differ][:4].tolist()}, max |diff| "
                              f"{float((got - want).abs()[kept].max()):.3e}")
    assert not bool(torch.isnan(got[kept]).any()), f"{what}: NaN among the kept voxels"


def _only_kept_written(got, kept, what):
    written = int((_bits(got)[~kept] != SENTINEL_WORD).sum())
    assert written == 0, f"{what}: {written} of {int((~kept).sum())} voxels outside the kept box were written"


def _entry(S, dev, entry, fill=0x00, options=0, keep_hi=None):  # noqa: F811
    """One forward of batch B through `entry` on a guarded workspace filled with `fill` and a guarded output filled
    with the sentinel -> float32 output on the CPU. Asserts the guards."""
    model, lib = S["model"], _native.lib()
    d, h, w = PATCH
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws_raw, ws = C1._guarded(S["need"], fill, dev)
    numel = N * model.output_channels * d * h * w
    out_raw, out = C1._guarded(4 * numel, SENTINEL, dev)
    model.engine_options = options
    try:
        handle = model._ensure_engine(dev)
        if entry == "forward":
            g = S["gather"][1]
            x = inference._get_batch_inputs(*g[:4], **g[4])
            rc = lib.exaspim_unet_forward(handle, x.data_ptr(), out.data_ptr(), N, d, h, w, S["sigmoid"], ws.data_ptr(),
                                          S["need"], stream)
        elif entry == "row":
            rc = lib.exaspim_unet_forward_prepared_row(handle, S["prepared"][1].data_ptr(), out.data_ptr(), N, d, h, w,
                                                       S["sigmoid"], TRIM, STRIDE, ws.data_ptr(), S["need"], stream)
        else:
            assert entry == "clipped"
            rc = lib.exaspim_unet_forward_prepared_clipped(handle, S["prepared"][1].data_ptr(), out.data_ptr(), N, d, h,
                                                           w, S["sigmoid"], TRIM, STRIDE, _native.int3(keep_hi),
                                                           ws.data_ptr(), S["need"], stream)
        torch.cuda.synchronize()
    finally:
        model.engine_options = 0
        model._ensure_engine(dev)
    _native.check(rc, entry)
    assert C1._intact(ws_raw, fill), f"{entry}, fill {fill:#x}: bytes around the workspace were written"
    assert C1._intact(out_raw, SENTINEL), f"{entry}: bytes around the output were written"
    return out.view(torch.float32).view(N, model.output_channels, d, h, w).cpu()


def _anchor(state, dev, name, dtype):  # noqa: F811
    """exaspim_unet_forward on batch B with the sigmoid: every voxel."""
    key = ("anchor", name, dtype)
    if key not in state:
        state[key] = _entry(_setup(state, dev, name, dtype), dev, "forward", 0xFF)
    return state[key]


def _row(state, dev, name, dtype):  # noqa: F811
    key = ("row", name, dtype)
    if key not in state:
        state[key] = _entry(_setup(state, dev, name, dtype), dev, "row", 0xFF)
    return state[key]


def _reference(state, dev, oracle, name):  # noqa: F811
    """The CPU oracle's probabilities of batch B, once per variant for every storage type."""
    key = ("reference", name)
    if key not in state:
        _, sd = _variant(state, dev, name, "fp16")
        g = _setup(state, dev, name, "fp16")["gather"][1]
        x = inference._get_batch_inputs(*g[:4], **g[4]).cpu()
        state[key] = torch.sigmoid(oracle.unet_forward(x, oracle.OracleModel(sd).sd))
    return state[key]


# ---- the table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_engine_answers_as_the_table_says(state, dev, case):  # noqa: F811
    name, dtype = case
    v = V.VARIANTS[name]
    model, _ = _variant(state, dev, name, dtype)
    shape = (N,) + PATCH
    span = model.carry_planes(shape, STRIDE, SHIFT, dev)
    span1 = model.carry1_planes(shape, STRIDE, SHIFT, dev)
    row = None
    if dtype != "fp32":
        probe = R.load_probe()
        dt = {"fp16": "f16", "bf16": "bf16"}[dtype]
        cout = R.plan_conv(probe, model.channels, model.output_channels, dt, 0)[5]
        assert cout == V.padded(name)[0]
        row = probe.probe_conv_row_mode_ok(R.DTYPES[dt], cout, N, PATCH[2], STRIDE, 1)
    print(f"{name} {dtype}: row mode {row}, first-level range {span}, second-level range {span1}, "
          f"padded widths {V.padded(name)}, pair {model.carry_pair_elems(shape)}, triple {model.carry_triple_elems(shape)}")
    host = V.host_model(name)
    if dtype == "fp32":     # (width 2 only: float32 has no row mode either)
        assert (span, span1) == ((0, 0), (0, 0))
        return
    assert row == int(v["row"])
    assert (span[1] > span[0]) == v["row"] and span == host.carry_planes(shape, STRIDE, SHIFT)
    assert span1 == (SPAN1 if v["level1"] else (0, 0)) == host.carry1_planes(shape, STRIDE, SHIFT)
    assert model.carry_pair_elems(shape) == host.carry_pair_elems(shape)
    assert model.carry_triple_elems(shape) == host.carry_triple_elems(shape)


# ---- anchor, row, clipped -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_anchor_plain_forward_against_the_cpu_oracle(state, dev, oracle, case):  # noqa: F811
    name, dtype = case
    got = _anchor(state, dev, name, dtype)
    want = _reference(state, dev, oracle, name)
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    err = float((got - want).abs().max())
    print(f"anchor {name} {dtype}: exaspim_unet_forward vs the CPU oracle: max |diff| = {err:.3e} "
          f"(bound {PROB_TOL[dtype]:.1e}), probabilities in [{float(want.min()):.3f}, {float(want.max()):.3f}]")
    assert err < PROB_TOL[dtype], f"{name} {dtype}: {err:.3e} from the CPU oracle"


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_row_entry_equals_the_per_patch_encoder_and_the_anchor(state, dev, case):  # noqa: F811
    name, dtype = case
    S = _setup(state, dev, name, dtype)
    kept = _kept(S["model"])
    row = _row(state, dev, name, dtype)
    per_patch = _entry(S, dev, "row", 0xFF, options=_native.OPT_PER_PATCH_ENCODER)
    _same_bits(row, per_patch, kept, f"{name} {dtype}: row entry, options 0 against the per-patch encoder")
    _same_bits(row, _anchor(state, dev, name, dtype), kept, f"{name} {dtype}: row entry against exaspim_unet_forward")
    for out in (row, per_patch):
        _only_kept_written(out, kept, f"{name} {dtype}: row entry")
    assert bool(kept.all()) == (name == "double")


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_clipped_entry_equals_the_row_entry_inside_the_box(state, dev, case):  # noqa: F811
    name, dtype = case
    S = _setup(state, dev, name, dtype)
    kept = _kept(S["model"], KEEP_HI)
    row = _row(state, dev, name, dtype)
    for fill in FILLS:
        got = _entry(S, dev, "clipped", fill, keep_hi=KEEP_HI)
        what = f"{name} {dtype}: clipped entry, keep_hi {KEEP_HI}, fill {fill:#x}"
        _same_bits(got, row, kept, what)
        _only_kept_written(got, kept, what)


# ---- carried planes -------------------------------------------------------------------------------------------------
def _carried(S, dev, level1, options, what):  # noqa: F811
    """test_gpu_carry1_forward's scheme: A carries out, B carries in; B against the clipped entry alone."""
    model = S["model"]
    shape = (N,) + PATCH
    d, h, w = PATCH
    span = model.carry_planes(shape, STRIDE, SHIFT, dev)
    assert span[1] > span[0]
    span1 = model.carry1_planes(shape, STRIDE, SHIFT, dev) if level1 else None
    assert span1 in (None, SPAN1)
    kept = _kept(model, tuple(S["keep_hi"]))
    numel = N * model.output_channels * d * h * w
    model.engine_options = options
    try:
        model._ensure_engine(dev)
        for fill in FILLS:
            bufs = C1._buffers(model, PATCH, fill, dev)
            t = [b[1] for b in bufs]
            a_pair, a_triple, b_pair, b_triple = t[:2], t[2:5], t[5:7], t[7:]
            ws_raw, ws = C1._guarded(S["need"], fill, dev)
            out_raw, out = C1._guarded(4 * numel, SENTINEL, dev)
            out_a = torch.empty(numel, dtype=torch.float32, device=dev)
            ca = C1._carry(a_pair, out=b_pair, out_z=(span[0] + SHIFT, span[1] + SHIFT), out_shift=SHIFT)
            cb = C1._carry(b_pair, in_z=span)
            ca1 = cb1 = None
            if level1:
                ca1 = C1._carry1(a_triple, out=b_triple, out_z=(span1[0] + SHIFT // 2, span1[1] + SHIFT // 2),
                                 out_shift=SHIFT // 2)
                cb1 = C1._carry1(b_triple, in_z=span1)
            assert C1._forward(S, dev, 0, out_a, ca, ca1, ws, PATCH, STRIDE) == 0, _native.last_error()
            ws.fill_(fill)     # (B must not depend on what A left in the workspace either)
            assert C1._forward(S, dev, 1, out, cb, cb1, ws, PATCH, STRIDE) == 0, _native.last_error()
            got = out.view(torch.float32).view(N, model.output_channels, d, h, w).cpu()
            _same_bits(got, S["want"], kept, f"{what}, fill {fill:#x}: B after A against the clipped entry alone")
            _only_kept_written(got, kept, f"{what}, fill {fill:#x}")
            used = bufs if level1 else bufs[:2] + bufs[5:7]
            for raw, _ in used:
                assert C1._intact(raw, fill), f"{what}, fill {fill:#x}: guard of a carry buffer"
            if not level1:      # the triples were not handed to the engine at all
                for raw, _ in bufs[2:5] + bufs[7:]:
                    assert bool((raw == fill).all())
            assert C1._intact(ws_raw, fill) and C1._intact(out_raw, SENTINEL), f"{what}, fill {fill:#x}: guards"
    finally:
        model.engine_options = 0
        model._ensure_engine(dev)


@pytest.mark.parametrize("options", [0, _native.OPT_CARRY_MAIN_ONLY], ids=["borders_carry", "main_only"])
@pytest.mark.parametrize("case", ROW_CASES, ids=ids)
def test_first_level_carry_equals_the_clipped_forward_alone(state, dev, case, options):  # noqa: F811
    name, dtype = case
    S = _setup(state, dev, name, dtype, keep_hi=KEEP_HI)
    _carried(S, dev, False, options, f"{name} {dtype}, first level, options {options}")


@pytest.mark.parametrize("case", LEVEL1_CASES, ids=ids)
def test_both_levels_carried_equal_the_clipped_forward_alone(state, dev, case):  # noqa: F811
    name, dtype = case
    S = _setup(state, dev, name, dtype, keep_hi=KEEP_HI)
    _carried(S, dev, True, 0, f"{name} {dtype}, both levels")


def test_carried_logits_of_the_foreground_model(state, dev):  # noqa: F811
    S = _setup(state, dev, "foreground", "fp16", keep_hi=KEEP_HI, sigmoid=0)
    probs = _setup(state, dev, "foreground", "fp16", keep_hi=KEEP_HI)["want"]
    kept = _kept(S["model"], KEEP_HI)
    # (the reference run gave logits: not the probabilities, but their sigmoid is -- up to float32 rounding of
    # two implementations of exp, a few units of 6e-8 on values below 1)
    assert not torch.equal(S["want"][kept], probs[kept])
    assert float((torch.sigmoid(S["want"][kept]) - probs[kept]).abs().max()) < 1e-6
    _carried(S, dev, True, 0, "foreground fp16, both levels, logits")


# ---- refusals -------------------------------------------------------------------------------------------------------
def _refused(S, dev, carry, carry1, bufs, entry="carry1"):  # noqa: F811
    """The call returns EXASPIM_E_INVALID and launches nothing: every buffer keeps its sentinel."""
    model, lib = S["model"], _native.lib()
    d, h, w = PATCH
    ws_raw, ws = C1._guarded(S["need"], SENTINEL, dev)
    out_raw, out = C1._guarded(4 * N * model.output_channels * d * h * w, SENTINEL, dev)
    if entry == "carry1":
        rc = C1._forward(S, dev, 1, out, carry, carry1, ws, PATCH, STRIDE)
    else:
        rc = lib.exaspim_unet_forward_prepared_carry(
            S["handle"], S["prepared"][1].data_ptr(), out.data_ptr(), N, d, h, w, 1, TRIM, STRIDE, S["keep_hi"],
            ctypes.byref(carry), ws.data_ptr(), S["need"], torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
    assert rc == -1, (rc, _native.last_error())      # EXASPIM_E_INVALID
    for raw, _ in bufs + [(ws_raw, ws), (out_raw, out)]:
        assert bool((raw == SENTINEL).all()), "a refused call wrote something"
    return _native.last_error()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_half_width_has_no_second_level_and_refuses_one(state, dev, dtype):  # noqa: F811
    S = _setup(state, dev, "half", dtype, keep_hi=KEEP_HI)
    model = S["model"]
    shape = (N,) + PATCH
    span = model.carry_planes(shape, STRIDE, SHIFT, dev)
    assert span[1] > span[0]
    assert model.carry1_planes(shape, STRIDE, SHIFT, dev) == (0, 0)
    bufs = C1._buffers(model, PATCH, SENTINEL, dev)
    t = [b[1] for b in bufs]
    msg = _refused(S, dev, C1._carry(t[:2], in_z=span), C1._carry1(t[2:5], in_z=SPAN1), bufs)
    assert "down1" in msg
    # ... and one to keep the second level in own buffers with nothing carried
    _refused(S, dev, C1._carry(t[:2], in_z=span), C1._carry1(t[2:5]), bufs)


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
def test_double_width_carries_nothing_and_refuses_a_carry(state, dev, dtype):  # noqa: F811
    S = _setup(state, dev, "double", dtype, keep_hi=KEEP_HI)
    model = S["model"]
    shape = (N,) + PATCH
    assert model.carry_planes(shape, STRIDE, SHIFT, dev) == (0, 0)
    assert model.carry1_planes(shape, STRIDE, SHIFT, dev) == (0, 0)
    bufs = C1._buffers(model, PATCH, SENTINEL, dev)
    t = [b[1] for b in bufs]
    host = V.host_model("foreground")      # the ranges a network with row mode takes at this geometry
    span = host.carry_planes(shape, STRIDE, SHIFT)
    assert span[1] > span[0]
    msg = _refused(S, dev, C1._carry(t[:2]), None, bufs, entry="carry")      # well-formed own buffers, nothing carried
    assert "row mode" in msg
    _refused(S, dev, C1._carry(t[:2], in_z=span), None, bufs, entry="carry")
    _refused(S, dev, C1._carry(t[:2], out=t[5:7], out_z=(span[0] + SHIFT, span[1] + SHIFT), out_shift=SHIFT), None, bufs,
             entry="carry")
    _refused(S, dev, C1._carry(t[:2], in_z=span), C1._carry1(t[2:5], in_z=SPAN1), bufs)
