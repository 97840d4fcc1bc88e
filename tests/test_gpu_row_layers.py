"""
Per-layer tests of inc.3's row mode (ConvArgs::row_stride) against float64 references.

The engine's own sequence (conv3d.hip: launch_conv3x3x3_row) -- the conv3x3x3_zpipe_row launch
over a row of overlapping patches, the two thin-tile launches on the patch faces that border a
neighbour and the column max-pool -- is driven stage by stage through the layer probe. Operands
come from layer_ref.row_inputs: neighbours agree on their shared columns except each patch's own
outermost x, whose fresh draws of twice the magnitude put an output computed in the wrong
patch's frame far outside the bound. The reference is layer_ref.conv_ref per patch on the very
operands the kernel reads and the checker layer_ref.check_conv with its own bound, as for every
other convolution path (test_gpu_layers.py).
"""

import copy

import pytest
import torch

import layer_ref as R
from test_gpu_layers import (E_INVALID, SENTINEL, Layer, _ptr, _record, _uniform_pm, encode_conv_weights,
                             probe)  # noqa: F401  (module-scoped fixture)

pytestmark = pytest.mark.gpu

DTS = ["bf16", "f16"]
MAIN, THIN, POOL = 1, 2, 4   # stages of launch_conv3x3x3_row
ALL = MAIN | THIN | POOL

# (ca, cout, cout_real, n, d, h, w, stride) -> tile depth of the row launch
GEOMETRIES = [
    ((32, 32, 32, 2, 6, 8, 64, 32), 6),      # overlap == stride, two patches (no interior patch)
    ((32, 32, 32, 3, 4, 8, 64, 32), 4),
    ((32, 32, 30, 3, 6, 16, 96, 64), 6),     # the default 96 / 64 geometry, padded couts
    ((32, 32, 32, 4, 10, 12, 80, 48), 4),    # stride 16 mod 32, masked last z tile (10 of 12 planes) and y tile
    ((32, 32, 32, 2, 6, 8, 128, 64), 6),     # overlap 64
    ((32, 32, 32, 3, 12, 8, 160, 96), 6),    # overlap 64 below the stride, two z tiles
    ((96, 96, 96, 2, 6, 8, 64, 32), 6),      # three 32-cout slices (width multiplier 3)
    ((32, 32, 16, 5, 8, 4, 64, 32), 4),      # h below the tile height, half-width model
]
GEOMETRY_2 = GEOMETRIES[1][0]
_ids = lambda g: "x".join(map(str, g[0]))   # noqa: E731


class RowLayer(Layer):
    """A Layer whose n patches are one row along x, `stride` voxels apart."""

    def __init__(self, dt, geometry, seed=0, x=None, weights=None):
        ca, cout, cout_real, n, d, h, w, stride = geometry
        self.stride = stride
        # (inc.3 maps c0 channels to c0: the padded input channels are the padded output channels)
        ca_real = min(ca, cout_real)
        if x is None:
            x = R.row_inputs(n, ca, d, h, w, stride, torch.Generator().manual_seed(1000 + seed))
            x[:, ca_real:] = 0
        super().__init__(dt, ca, 0, cout, n, d, h, w, seed=seed, ca_real=ca_real, cout_real=cout_real, x=x,
                         weights=weights)

    def run_row(self, probe, stages=ALL, expect_rc=0, dt_arg=None, pool=True, n_arg=None, stride_arg=None):
        """The row sequence on dst and the pool tensor pre-filled with the sentinel byte."""
        dt, (n, d, h, w) = self.dt, self.shape
        k = R.kc(dt)
        xa = R.pack_blocked(self.x, dt).cuda()
        wt = encode_conv_weights(self.w.numpy(), dt).cuda()
        bt = self.b.to(torch.float32).cuda()
        dst = torch.empty((n, self.cout // k, d, h, w, k), dtype=R.STORAGE[dt], device="cuda")
        pdst = torch.empty((n, self.cout // k, d // 2, h // 2, w // 2, k), dtype=R.STORAGE[dt], device="cuda")
        for t in (dst, pdst):
            R.bits(t).view(torch.uint8).fill_(SENTINEL)
        probe.probe_reset_config()
        torch.cuda.synchronize()
        rc = probe.probe_conv3x3x3_row(R.DTYPES[dt_arg or dt], _ptr(xa), self.ca, _ptr(wt), _ptr(bt), _ptr(dst),
                                       self.cout, n if n_arg is None else n_arg, d, h, w, R.SLOPE,
                                       self.stride if stride_arg is None else stride_arg,
                                       _ptr(pdst if pool else None), stages, None)
        if expect_rc:
            assert rc == expect_rc, rc
            return probe.probe_last_error().decode()
        assert rc == 0, probe.probe_last_error().decode()
        torch.cuda.synchronize()
        if stages == MAIN:   # (a later stage's launch replaces the record)
            self.row = probe.probe_last_row()
            self.launcher, self.params, self.config = _record(probe, dt)
        self.ksplit = 1
        self.dst, self.pool = dst.cpu(), pdst.cpu()
        return self

    def border_masks(self):
        """bool (n, cout, d, h, w) of the voxels the row launch leaves to the thin launches -- the two
        outermost x of every patch face that borders a neighbour -- and (n, cout, d/2, h/2, w/2) of the
        pooled voxels it leaves to the column max-pool."""
        n, d, h, w = self.shape
        m = torch.zeros((n, self.cout, d, h, w), dtype=torch.bool)
        pm = torch.zeros((n, self.cout, d // 2, h // 2, w // 2), dtype=torch.bool)
        m[1:, ..., :2] = True
        m[:-1, ..., w - 2:] = True
        pm[1:, ..., 0] = True
        pm[:-1, ..., w // 2 - 1] = True
        return m, pm


def _blocked(mask, k):
    """(n, c, d, h, w) mask -> the blocked layout (n, c / k, d, h, w, k)."""
    n, c, d, h, w = mask.shape
    return mask.reshape(n, c // k, k, d, h, w).permute(0, 1, 3, 4, 5, 2)


def _untouched(t, mask):
    """All bytes of the masked values of storage tensor t are still the sentinel."""
    raw = R.bits(t).view(torch.uint8).reshape(t.shape + (-1,))
    return bool((raw[_blocked(mask, t.shape[-1])] == SENTINEL).all())


def _check_pool(L, mask=None):
    """The pool tensor equals maxpool_ref of the stored dst, NaN pattern included (masked voxels)."""
    got = R.unpack_blocked(L.pool)
    want = R.maxpool_ref(R.unpack_blocked(L.dst))
    m = torch.ones_like(got, dtype=torch.bool) if mask is None else mask
    assert torch.equal(torch.isnan(got) & m, torch.isnan(want) & m)
    ok = m & ~torch.isnan(want)
    assert torch.equal(got[ok], want[ok]), (ok & (got != want)).nonzero()[:4]


def _same_bits(a, b, what):
    diff = R.bits(a) != R.bits(b)
    assert not diff.any(), f"{what}: {int(diff.sum())} values differ, first at {diff.nonzero()[0].tolist()}"


def _check_against_per_patch(L, probe):
    """dst and the pool of the row sequence have the bits of the per-patch fused-pool launch."""
    P = copy.copy(L)   # the same operands
    Layer.run(P, probe, pool=True)
    assert probe.probe_last_row() == 0 and P.params["POOL"] == "true", P.params
    _same_bits(L.dst, P.dst, "dst")
    _same_bits(L.pool, P.pool, "pool")
    return P


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=_ids)
def test_row_launch_alone(probe, dt, geometry):
    g, tz = geometry
    L = RowLayer(dt, g, seed=sum(g)).run_row(probe, stages=MAIN)
    assert L.row == 1
    assert (L.launcher, int(L.params["TZ"]), L.params["POOL"]) == ("launch_zpipe", tz, "true"), L.params
    m, pm = L.border_masks()
    assert _untouched(L.dst, m), "the row launch wrote a neighbour-facing outermost x"
    assert _untouched(L.pool, pm), "the row launch wrote a neighbour-facing pooled border column"
    L.check(mask=~m)
    _check_pool(L, mask=~pm)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=_ids)
def test_row_sequence(probe, dt, geometry):
    g, _ = geometry
    L = RowLayer(dt, g, seed=sum(g) + 1).run_row(probe)
    L.check()
    _check_pool(L)
    _check_against_per_patch(L, probe)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("tiles", ["wgs", "wgs+2", "2.5wgs"])
def test_row_tile_walk(probe, dt, tiles):
    # launch_zpipe: 32-cout slices, MINW = 2 -> max(8, 2 * CUs // 8 * 8) persistent workgroups; a row of
    # n 4 x 8 x 64 patches 32 apart is 2n + 2 tiles. Beyond one tile per workgroup the row walk prefetches
    # the next tile's operands across tiles (and across patches).
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    wgs = max(8, 2 * cus // 8 * 8)
    n = {"wgs": wgs // 2 - 1, "wgs+2": wgs // 2, "2.5wgs": (5 * wgs // 2) // 2 - 1}[tiles]
    L = RowLayer(dt, (32, 32, 32, n, 4, 8, 64, 32), seed=n).run_row(probe)
    P = _check_against_per_patch(L, probe)
    assert int(P.params["TZ"]) == 4
    keep = [0, n // 2, n - 2, n - 1]
    acc, s = R.conv_ref(L.x[keep], L.w, L.b)
    R.check_conv(R.unpack_blocked(L.dst[keep]), acc, s, 32, dt)


def _window(shape, nb, z, y, x):
    win = torch.zeros(shape, dtype=torch.bool)
    win[nb, :, max(0, z - 1): z + 2, max(0, y - 1): y + 2, max(0, x - 1): x + 2] = True
    return win


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("where", ["own_x0", "shared", "own_xlast"])
def test_row_nan(probe, dt, where):
    g = GEOMETRY_2
    ca, cout, _, n, d, h, w, stride = g
    x = R.row_inputs(n, ca, d, h, w, stride, torch.Generator().manual_seed(7))
    shape = (n, cout, d, h, w)
    z, y, nan = 2, 3, float("nan")
    if where == "own_x0":        # patch 1's own outermost x: patch 0 holds another value in that column
        x[1, 5, z, y, 0] = nan
        win = _window(shape, 1, z, y, 0)
    elif where == "shared":      # strip x = stride + 10 is x = stride + 10 of patch 0 and x = 10 of patch 1
        x[0, 5, z, y, stride + 10] = nan
        x[1, 5, z, y, 10] = nan
        win = _window(shape, 0, z, y, stride + 10) | _window(shape, 1, z, y, 10)
    else:                        # patch 0's own outermost x
        x[0, 5, z, y, w - 1] = nan
        win = _window(shape, 0, z, y, w - 1)
    L = RowLayer(dt, g, seed=11, x=x).run_row(probe)
    got = R.unpack_blocked(L.dst)
    assert torch.equal(torch.isnan(got), win), "NaN outputs are not the NaN voxels' 3x3x3 windows"
    L.check(nan_ok=win)
    _check_pool(L)
    assert torch.equal(torch.isnan(R.unpack_blocked(L.pool)), R.maxpool_ref(win.to(torch.float64)) > 0)
    _check_against_per_patch(L, probe)


def test_row_saturation(probe):
    dt, g = "f16", GEOMETRY_2
    ca, cout, _, n, d, h, w, stride = g
    gen = torch.Generator().manual_seed(2)
    x = 45000 * R.row_inputs(n, ca, d, h, w, stride, gen).abs()   # (a patch's own outermost x saturates on its way in)
    wt = _uniform_pm((cout, ca, 27), gen)
    wt[0] = wt[0].abs()
    wt[1] = -wt[1].abs()
    L = RowLayer(dt, g, x=x, weights=wt).run_row(probe)
    L.check()
    got = R.unpack_blocked(L.dst)
    inner = got[:, :, 1:-1, 1:-1, 1:-1]    # all 27 taps: |acc| > 65504 / slope
    assert (inner[:, 0] == 65504).all() and (inner[:, 1] == -65504).all()
    o = w - stride
    for shared in (got[:-1, :, 1:-1, 1:-1, stride: w - 1], got[1:, :, 1:-1, 1:-1, 1: o]):
        assert (shared[:, 0] == 65504).all() and (shared[:, 1] == -65504).all()
    assert not torch.isinf(got).any() and not torch.isinf(R.unpack_blocked(L.pool)).any()
    _check_pool(L)
    _check_against_per_patch(L, probe)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("w,cols", [(10, (0, 4)), (10, (1, 1)), (2, (0, 0))])
def test_maxpool2_xcols(probe, dt, w, cols):
    gen = torch.Generator().manual_seed(6)   # the input of test_maxpool2_nan_exact and a NaN in pooled column 1
    k = R.kc(dt)
    x = R.quantize(_uniform_pm((2, 2 * k, 6, 8, 10), gen), dt)
    x[0, 1, 0, 0, 0] = float("nan")
    x[1, 3, 3, 5, 7] = -float("nan")
    x[1, k, 5, 7, 9] = float("nan")
    x[0, 2, 2, 2, 3] = float("nan")
    x = x[..., :w].contiguous()
    src = R.pack_blocked(x, dt).cuda()
    if dt != "f32" and w == 10:   # a negative NaN's sign bit as well
        R.bits(src)[1, 0, 3, 5, 7, 3] |= -0x8000
    want = R.maxpool_ref(x)
    sel = torch.zeros_like(want, dtype=torch.bool)
    sel[..., list(cols)] = True
    assert torch.isnan(want[sel]).any() and (w == 2 or torch.isnan(want[~sel]).any())
    dst = torch.empty((2, 2, 3, 4, w // 2, k), dtype=R.STORAGE[dt], device="cuda")
    R.bits(dst).view(torch.uint8).fill_(SENTINEL)
    rc = probe.probe_maxpool2_xcols(R.DTYPES[dt], _ptr(src), _ptr(dst), 2, 6, 8, w, 2 * k, cols[0], cols[1], None)
    assert rc == 0, probe.probe_last_error()
    torch.cuda.synchronize()
    dst = dst.cpu()
    assert _untouched(dst, ~sel), "a column that was not selected was written"
    got = R.unpack_blocked(dst)
    assert torch.equal(torch.isnan(got) & sel, torch.isnan(want) & sel)
    ok = sel & ~torch.isnan(want)
    assert torch.equal(got[ok], want[ok])
    # rejected on the host, before any launch: columns outside [0, w / 2) and odd sizes
    for d_, h_, w_, c0, c1 in [(6, 8, w, -1, 0), (6, 8, w, 0, w // 2), (6, 8, w, w // 2, 0), (5, 8, w, 0, 0),
                               (6, 7, w, 0, 0), (6, 8, w + 1, 0, 0)]:
        before = dst.clone()
        rc = probe.probe_maxpool2_xcols(R.DTYPES[dt], _ptr(src), _ptr(dst), 2, d_, h_, w_, 2 * k, c0, c1, None)
        assert rc == E_INVALID, (d_, h_, w_, c0, c1)
        assert "maxpool" in probe.probe_last_error().decode()
        assert torch.equal(R.bits(dst), R.bits(before))


REJECTED = {
    # name: (dt of the tensors, geometry, run_row arguments, probe_conv_row_mode_ok arguments
    #        (dtype, cout, n, w, row_stride, fused_pool_whole_patch))
    "f32": ("f32", (32, 32, 32, 2, 6, 8, 64, 32), {}, ("f32", 32, 2, 64, 32, 1)),
    "no_pool_dst": ("f16", (32, 32, 32, 2, 6, 8, 64, 32), {"pool": False}, ("f16", 32, 2, 64, 32, 0)),
    "n1": ("f16", (32, 32, 32, 2, 6, 8, 64, 32), {"n_arg": 1}, ("f16", 32, 1, 64, 32, 1)),
    "cout64": ("f16", (32, 64, 64, 2, 6, 8, 64, 32), {}, ("f16", 64, 2, 64, 32, 1)),
    "overlap16": ("f16", (32, 32, 32, 2, 6, 8, 96, 80), {}, ("f16", 32, 2, 96, 80, 1)),
    "stride_below_overlap": ("f16", (32, 32, 32, 2, 6, 8, 96, 32), {}, ("f16", 32, 2, 96, 32, 1)),
    "w72": ("f16", (32, 32, 32, 2, 6, 8, 72, 40), {}, ("f16", 32, 2, 72, 40, 1)),
}


@pytest.mark.parametrize("case", list(REJECTED))
def test_row_rejected(probe, case):
    # every case returns from the host-side argument check: nothing is launched, nothing is written
    dt, g, kw, ok_args = REJECTED[case]
    L = RowLayer(dt, g)
    for stages in (ALL, MAIN, THIN | POOL):
        assert "row mode" in L.run_row(probe, stages=stages, expect_rc=E_INVALID, **kw)
    assert probe.probe_conv_row_mode_ok(R.DTYPES[ok_args[0]], *ok_args[1:]) == 0
    # (the predicate itself says yes to the first geometry of the table in both 16-bit types)
    for dt16 in DTS:
        assert probe.probe_conv_row_mode_ok(R.DTYPES[dt16], 32, 2, 64, 32, 1) == 1


def test_row_instantiations_covered(probe):
    """The table reaches the four instantiations of conv3x3x3_zpipe_row, {bf16, f16} x {6, 4}-plane
    tiles, under the configuration string of the per-patch fused-pool launch (which is why
    test_dispatch_coverage cannot tell them apart: ConvLaunchRecord::row does)."""
    hit, configs = set(), set()
    for dt in DTS:
        for g, _ in GEOMETRIES:
            L = RowLayer(dt, g).run_row(probe, stages=MAIN)
            if L.row:
                hit.add((dt, int(L.params["TZ"])))
                configs.add(L.config)
        for g in ((32, 32, 32, 2, 6, 8, 64, 32), (32, 32, 32, 2, 4, 8, 64, 32)):
            P = Layer(dt, 32, 0, 32, *g[3:7]).run(probe, pool=True)
            assert probe.probe_last_row() == 0
            assert P.config in configs, P.config
    assert hit == {(dt, tz) for dt in DTS for tz in (6, 4)}, sorted(hit)
    assert len(configs) == 4, sorted(configs)
