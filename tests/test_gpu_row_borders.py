"""
Row mode of inc.3, the border launch (conv3d.hip: launch_conv3x3x3_row, kRowStageBorders = 8): one launch
computes x in [0, 2) of patches 1 .. n-1 and x in [w - 2, w) of patches 0 .. n-2, each in the patch's own
frame, and writes the pooled column each 2-wide tile holds. It replaces the two thin-tile launches and the
column max-pool (stages 2 and 4), which stay as they are and are the reference here: after Main | Borders
dst and the pool tensor have the bits of Main | Thin | Pool, NaN and saturated values included. Driven
through the layer probe on layer_ref.row_inputs operands, like test_gpu_row_layers.
"""

import pytest
import torch

import layer_ref as R
from test_gpu_layers import _uniform_pm, probe  # noqa: F401  (module-scoped fixture)
from test_gpu_row_layers import (ALL, DTS, MAIN, POOL, THIN, RowLayer, _check_pool, _same_bits, _untouched,
                                 _window)

pytestmark = pytest.mark.gpu

BORDERS = 8

# (ca, cout, cout_real, n, d, h, w, stride)
GEOMETRIES = [(32, 32, 32, n, d, h, 96, 64) for n in (2, 3, 16) for d, h in ((8, 16), (6, 12))]   # 6 x 12: masked z and y tiles
GEOMETRIES += [
    (32, 32, 32, 3, 8, 16, 64, 32),     # overlap == stride
    (96, 96, 96, 2, 4, 8, 64, 32),      # three 32-cout slices, the 4-plane tile
]
_ids = lambda g: "x".join(map(str, g))   # noqa: E731


def _both(probe, dt, g, seed, **kw):  # noqa: F811
    want = RowLayer(dt, g, seed=seed, **kw).run_row(probe, stages=ALL)
    got = RowLayer(dt, g, seed=seed, **kw).run_row(probe, stages=MAIN | BORDERS)
    _same_bits(got.dst, want.dst, "dst")
    _same_bits(got.pool, want.pool, "pool")
    return got, want


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=_ids)
def test_main_and_borders_equal_main_thin_pool(probe, dt, geometry):  # noqa: F811
    got, _ = _both(probe, dt, geometry, seed=sum(geometry))
    got.check()
    _check_pool(got)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("geometry", [GEOMETRIES[2], GEOMETRIES[3], GEOMETRIES[6]], ids=_ids)
def test_borders_alone_write_the_border_columns_only(probe, dt, geometry):  # noqa: F811
    L = RowLayer(dt, geometry, seed=5).run_row(probe, stages=BORDERS)
    config = probe.probe_last_config().decode()
    assert "launch_row_borders_cfg" in config, config
    assert probe.probe_last_row() == 0
    m, pm = L.border_masks()
    assert _untouched(L.dst, ~m), "the border launch wrote outside the border columns"
    assert _untouched(L.pool, ~pm), "the border launch wrote outside the pooled border columns"
    # every border value is written, with the bits of the thin launches and of the column max-pool
    W = RowLayer(dt, geometry, seed=5).run_row(probe, stages=THIN | POOL)
    k = L.dst.shape[-1]
    mb = m.reshape(m.shape[0], m.shape[1] // k, k, *m.shape[2:]).permute(0, 1, 3, 4, 5, 2)
    pb = pm.reshape(pm.shape[0], pm.shape[1] // k, k, *pm.shape[2:]).permute(0, 1, 3, 4, 5, 2)
    assert torch.equal(R.bits(L.dst)[mb], R.bits(W.dst)[mb])
    assert torch.equal(R.bits(L.pool)[pb], R.bits(W.pool)[pb])
    L.check(mask=m)


def test_launch_record_names_the_border_configuration(probe):  # noqa: F811
    seen = set()
    for dt in DTS:
        for g in (GEOMETRIES[0], GEOMETRIES[7]):
            RowLayer(dt, g).run_row(probe, stages=BORDERS)
            seen.add(probe.probe_last_config().decode())
    assert len(seen) == 4 and all("launch_row_borders_cfg" in c for c in seen), sorted(seen)
    assert {("8" in c.split("TZ = ")[1][:2], "F16Tag" in c and "BF16Tag" not in c) for c in seen} == {
        (True, True), (True, False), (False, True), (False, False)}, sorted(seen)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("where", ["own_x0", "own_xlast"])
def test_nan_in_an_own_border_column(probe, dt, where):  # noqa: F811
    g = (32, 32, 32, 3, 4, 8, 64, 32)
    ca, cout, _, n, d, h, w, stride = g
    x = R.row_inputs(n, ca, d, h, w, stride, torch.Generator().manual_seed(7))
    shape = (n, cout, d, h, w)
    z, y, nan = 2, 3, float("nan")
    if where == "own_x0":
        x[1, 5, z, y, 0] = nan
        win = _window(shape, 1, z, y, 0)
    else:
        x[0, 5, z, y, w - 1] = nan
        win = _window(shape, 0, z, y, w - 1)
    got, _ = _both(probe, dt, g, seed=11, x=x)
    assert torch.equal(torch.isnan(R.unpack_blocked(got.dst)), win)
    got.check(nan_ok=win)
    _check_pool(got)
    assert torch.equal(torch.isnan(R.unpack_blocked(got.pool)), R.maxpool_ref(win.to(torch.float64)) > 0)


def test_saturated_fp16_values_in_the_border_columns(probe):  # noqa: F811
    dt, g = "f16", (32, 32, 32, 3, 4, 8, 64, 32)
    ca, cout, _, n, d, h, w, stride = g
    gen = torch.Generator().manual_seed(2)
    x = 45000 * R.row_inputs(n, ca, d, h, w, stride, gen).abs()
    wt = _uniform_pm((cout, ca, 27), gen)
    wt[0] = wt[0].abs()
    wt[1] = -wt[1].abs()
    got, _ = _both(probe, dt, g, seed=0, x=x, weights=wt)
    got.check()
    v = R.unpack_blocked(got.dst)
    m, pm = got.border_masks()
    inner = torch.zeros_like(m)
    inner[:, :, 1:-1, 1:-1, 1:-1] = True      # all 27 taps: |acc| > 65504 / slope
    for c, val in ((0, 65504.0), (1, -65504.0)):
        sel = (m & inner)[:, c]
        assert sel.any() and (v[:, c][sel] == val).all()
    assert not torch.isinf(v).any() and not torch.isinf(R.unpack_blocked(got.pool)).any()
    _check_pool(got)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case,trim", [(6, 0), (7, 4)])
def test_engine_with_separate_borders_gives_the_same_bits(dtype, case, trim):
    """The whole forward in row mode: the border launch (the engine's plan) against
    EXASPIM_OPT_ROW_SEPARATE_BORDERS (two thin-tile launches and the column max-pool)."""
    import test_gpu_workspace as W
    from aind_exaspim_neuron_segmentation_amd import _native

    dev = torch.device("cuda:0")
    state = {"models": {}, "inputs": {}, "refs": {}}
    W._assert_row_mode(case, dtype)
    model, _ = W._model(state, dev, dtype, "base")
    got = W._run(state, dev, model, "row", case, trim, "0xFF")
    model.engine_options = _native.OPT_ROW_SEPARATE_BORDERS
    try:
        want = W._run(state, dev, model, "row", case, trim, "0xFF")
    finally:
        model.engine_options = 0
    assert torch.equal(W._bits(got), W._bits(want))
