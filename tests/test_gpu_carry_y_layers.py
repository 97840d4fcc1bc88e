"""
Per-layer tests of inc.3's rows carried along y on top of the planes carried along z (ConvCarryY,
conv3x3x3_zpipe_rowzy).

Four row batches (k, j) -- z slab k, y row j -- run in plan order (0, 0), (0, 1), (1, 0), (1, 1), each in its own
poison-filled buffers, each storing what the rule names into its successors' buffers: the z successor gets planes
Zo x the rows the batch computes, the y successor rows Yo x the planes it computes, the diagonal successor Zo x Yo.
Every batch is held bit for bit to the uncarried row sequence on the same operands. A batch's operands agree with a
predecessor's only where the range taken over from it reads, so a block carried beyond its range, left out beyond
it, or never written (the diagonal) shows as different bits or as poison.
"""

import ctypes

import pytest
import torch

import layer_ref as R
from test_gpu_layers import E_INVALID, SENTINEL, _ptr, encode_conv_weights, probe as _base_probe  # noqa: F401
from test_gpu_row_layers import RowLayer, _blocked, _same_bits
from test_gpu_carry_layers import GUARD, POISON, Guarded, _raw, _shapes  # noqa: F401

pytestmark = pytest.mark.gpu

DTS = ["bf16", "f16"]
MAIN, BORDERS, BORDERS_CARRY = 1, 8, 16
# (ca, cout, cout_real, n, d, h, w, stride), (shift_z, Zc), (shift_y, Yc): Zc = the whole z tiles inside
# [2, d - shift_z - 2), Yc = the whole 8-row tiles inside [2, h - shift_y - 2) of the later frame
CUBE64 = ((32, 32, 32, 2, 64, 64, 64, 32), (32, (4, 28)), (32, (8, 24)))       # patch 64^3, overlap 32: 4-plane tiles
DEEP96 = ((32, 32, 32, 2, 96, 48, 64, 32), (64, (6, 30)), (16, (8, 24)))       # 6-plane tiles
SMALL = ((32, 32, 32, 2, 32, 48, 64, 32), (16, (4, 12)), (16, (8, 24)))


@pytest.fixture(scope="module")
def probe(_base_probe):  # noqa: F811
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    fn = _base_probe.probe_conv3x3x3_row_carry_y
    fn.restype = i32
    fn.argtypes = [i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp, ctypes.POINTER(i32), vp, vp,
                   ctypes.POINTER(i32), ctypes.POINTER(vp), i32, vp]
    for name in ("probe_last_carry", "probe_last_carry_y"):
        getattr(_base_probe, name).restype = i32
        getattr(_base_probe, name).argtypes = []
    return _base_probe


def _launch(probe, L, own, z=(0, 0, 0, 0, 0), ztgt=None, y=(0, 0, 0, 0, 0), ytgt=None, dtgt=None, stages=MAIN,
            expect_rc=0, stride=None):
    """launch_conv3x3x3_row with the z and y carry fields; own / ztgt / ytgt / dtgt: (dst, pool) Guarded pairs."""
    n, d, h, w = L.shape
    xa = R.pack_blocked(L.x, L.dt).cuda()
    wt = encode_conv_weights(L.w.numpy(), L.dt).cuda()
    bt = L.b.to(torch.float32).cuda()
    ptr = lambda pair, i: _ptr(pair[i].t) if pair is not None else None  # noqa: E731
    targets = (ctypes.c_void_p * 4)(ptr(ytgt, 0), ptr(ytgt, 1), ptr(dtgt, 0), ptr(dtgt, 1))
    probe.probe_reset_config()
    torch.cuda.synchronize()
    rc = probe.probe_conv3x3x3_row_carry_y(
        R.DTYPES[L.dt], _ptr(xa), L.ca, _ptr(wt), _ptr(bt), _ptr(own[0].t), L.cout, n, d, h, w, R.SLOPE,
        L.stride if stride is None else stride, _ptr(own[1].t), (ctypes.c_int32 * 5)(*z), ptr(ztgt, 0), ptr(ztgt, 1),
        (ctypes.c_int32 * 5)(*y), targets, stages, None)
    if expect_rc:
        assert rc == expect_rc, rc
        return probe.probe_last_error().decode()
    assert rc == 0, probe.probe_last_error().decode()
    torch.cuda.synchronize()
    return probe.probe_last_carry_y() if stages == MAIN else None


def _four(case, dt, seed, n=None, special=False):
    """The operands of batches (0, 0), (0, 1), (1, 0), (1, 1): fresh draws, equal to a predecessor's only on the
    planes and rows the range taken over from it reads (one voxel beyond the range on either side)."""
    g, (sz, (zl, zh)), (sy, (yl, yh)) = case
    if n is not None:
        g = g[:3] + (n,) + g[4:]
    ca, cout, _, n, d, h, w, stride = g
    x = {kj: R.row_inputs(n, ca, d, h, w, stride, torch.Generator().manual_seed(seed + i))
         for i, kj in enumerate(((1, 1), (1, 0), (0, 1), (0, 0)))}
    zr, zo = slice(zl - 1, zh + 1), slice(zl - 1 + sz, zh + 1 + sz)
    yr, yo = slice(yl - 1, yh + 1), slice(yl - 1 + sy, yh + 1 + sy)
    bias = None
    if special:
        # NaN in rows and planes that are carried (the diagonal block among them), a saturating half in channel 0
        x[1, 1][0, 3, zl + 2, yl + 3, stride + 7] = float("nan")
        x[1, 1][1, 2, zh + 3, yl + 5, 20] = float("nan")      # (an own column of patch 1)
        x[1, 1][0, 5, zl + 5, yh + 4, 20] = float("nan")
        bias = torch.zeros(cout, dtype=torch.float64)
        bias[0], bias[1] = 70000.0, -0.25
    x[1, 0][:, :, :, yo] = x[1, 1][:, :, :, yr]       # the y predecessor of (1, 1): rows, every plane
    x[0, 1][:, :, zo] = x[1, 1][:, :, zr]             # its z predecessor: planes, every row
    x[0, 0][:, :, zo] = x[1, 0][:, :, zr]             # (0, 0) is the z predecessor of (1, 0) ...
    x[0, 0][:, :, :, yo] = x[0, 1][:, :, :, yr]       # ... and the y predecessor of (0, 1): the diagonal block agrees
    assert torch.equal(x[0, 0][:, :, zo, yo].nan_to_num(7.0), x[1, 1][:, :, zr, yr].nan_to_num(7.0))
    first = RowLayer(dt, g, seed=seed, x=x[0, 0])
    if bias is not None:
        first.b = bias
    layers = {(0, 0): first}
    for kj in ((0, 1), (1, 0), (1, 1)):
        L = RowLayer(dt, g, seed=seed, x=x[kj], weights=first.w)
        L.w, L.b = first.w, first.b
        layers[kj] = L
    return layers


def _run_four(probe, layers, case, fill=POISON, borders=BORDERS_CARRY):
    """The four batches in plan order with every carry of the rule -> {(k, j): (own pair, uncarried pair)}."""
    _, (sz, (zl, zh)), (sy, (yl, yh)) = case
    dt = layers[0, 0].dt
    s, ps = _shapes(layers[0, 0])
    own = {kj: [Guarded(s, dt, fill), Guarded(ps, dt, fill)] for kj in layers}
    z_out, y_out = (zl + sz, zh + sz, sz), (yl + sy, yh + sy, sy)
    for k, j in ((0, 0), (0, 1), (1, 0), (1, 1)):
        z = ((zl, zh) if k == 1 else (0, 0)) + (z_out if k == 0 else (0, 0, 0))
        y = ((yl, yh) if j == 1 else (0, 0)) + (y_out if j == 0 else (0, 0, 0))
        was = _launch(probe, layers[k, j], own[k, j], z, own[1, j] if k == 0 else None, y,
                      own[k, 1] if j == 0 else None, own[1, 1] if (k, j) == (0, 0) else None, stages=MAIN)
        assert was == 1, "the launch with a y field did not run conv3x3x3_zpipe_rowzy"
        # (the border launch carries along z only and computes every row of its columns)
        _launch(probe, layers[k, j], own[k, j], z, own[1, j] if k == 0 else None, stages=borders)
    out = {}
    for kj, L in layers.items():
        ref = [Guarded(s, dt), Guarded(ps, dt)]
        _launch(probe, L, ref, stages=MAIN | BORDERS)
        out[kj] = (own[kj], ref)
    return out


def _check_four(out):
    for kj, (own, ref) in out.items():
        _same_bits(own[0].t.cpu(), ref[0].t.cpu(), f"batch {kj} dst")
        _same_bits(own[1].t.cpu(), ref[1].t.cpu(), f"batch {kj} pool")
        for gbuf in own + ref:
            assert gbuf.guards_intact(), kj


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [2, 3])
def test_four_batches_have_the_uncarried_bits(probe, dt, n):
    # poison in everything a batch leaves out: a block nobody wrote -- the diagonal -- stays poison
    _check_four(_run_four(probe, _four(CUBE64, dt, seed=100 + n, n=n), CUBE64))


@pytest.mark.parametrize("dt", DTS)
def test_six_plane_tiles(probe, dt):
    _check_four(_run_four(probe, _four(DEEP96, dt, seed=7), DEEP96))


@pytest.mark.parametrize("dt", DTS)
def test_main_only_borders(probe, dt):
    # the border launch that writes every plane (kRowStageBorders) goes with the y carry as well
    _check_four(_run_four(probe, _four(SMALL, dt, seed=9), SMALL, borders=BORDERS))


@pytest.mark.parametrize("dt", DTS)
def test_nan_and_saturation_in_carried_rows(probe, dt):
    layers = _four(SMALL, dt, seed=31, special=True)
    out = _run_four(probe, layers, SMALL)
    _, (sz, (zl, zh)), (sy, (yl, yh)) = SMALL
    got = R.unpack_blocked(out[1, 1][0][0].t.cpu())
    assert bool(torch.isnan(got[:, :, zl:zh, yl:yh]).any()), "no NaN reached the diagonal block"
    assert bool(torch.isnan(got[:, :, zh:, yl:yh]).any()), "no NaN reached the rows carried along y"
    if dt == "f16":
        v = got[:, 0, :, yl:yh]
        assert bool(((v == 65504.0) | torch.isnan(v)).all()) and bool((v == 65504.0).any())
    _check_four(out)


@pytest.mark.parametrize("dt", DTS)
def test_more_tiles_than_workgroups(probe, dt):
    # 32-cout slices, MINW = 2 -> max(8, 2 * CUs // 8 * 8) persistent workgroups; batch (1, 1) of n patches walks
    # (8 - 2) x (6 - 2) x (2 n + 2) tiles
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    wgs = max(8, 2 * cus // 8 * 8)
    n = -(-(wgs // 24 + 1 - 2) // 2) + 1
    assert 6 * 4 * (2 * n + 2) > wgs
    _check_four(_run_four(probe, _four(SMALL, dt, seed=41, n=n), SMALL))


def _region(L, planes, rows, shift_z, shift_y):
    """Masks of what a carry out of `planes` x `rows` (source frame) writes in the target frame: the row launch's
    own voxels (not the neighbour-facing outermost x, not their pooled column) at plane - shift_z, row - shift_y."""
    m, pm = L.border_masks()
    keep, pkeep = ~m, ~pm
    for mask, f in ((keep, 1), (pkeep, 2)):
        zsel = torch.zeros(mask.shape[2], dtype=torch.bool)
        ysel = torch.zeros(mask.shape[3], dtype=torch.bool)
        zsel[(planes[0] - shift_z) // f:(planes[1] - shift_z) // f] = True
        ysel[(rows[0] - shift_y) // f:(rows[1] - shift_y) // f] = True
        mask &= zsel[None, None, :, None, None] & ysel[None, None, None, :, None]
    return keep, pkeep


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("with_in", [False, True])
def test_carry_out_writes_exactly_what_the_rule_names(probe, dt, with_in):
    """Batch (0, 0) -- or, with_in, a batch that itself took Zc and Yc over -- stores to sentinel-filled targets."""
    case = SMALL
    g, (sz, (zl, zh)), (sy, (yl, yh)) = case
    L = _four(case, dt, seed=13)[0, 0]
    n, d, h, w = L.shape
    s, ps = _shapes(L)
    ref = [Guarded(s, dt), Guarded(ps, dt)]
    _launch(probe, L, ref, stages=MAIN)
    own, zt, yt, dg = ([Guarded(s, dt), Guarded(ps, dt)] for _ in range(4))
    z = ((zl, zh) if with_in else (0, 0)) + (zl + sz, zh + sz, sz)
    y = ((yl, yh) if with_in else (0, 0)) + (yl + sy, yh + sy, sy)
    assert _launch(probe, L, own, z, zt, y, yt, dg, stages=MAIN) == 1
    k = R.kc(dt)
    # the rows and planes the launch computes
    rows = [(0, yl), (yh, h)] if with_in else [(0, h)]
    planes = [(0, zl), (zh, d)] if with_in else [(0, d)]
    want = {"z": (zt, [((zl + sz, zh + sz), r) for r in rows], sz, 0),
            "y": (yt, [(p, (yl + sy, yh + sy)) for p in planes], 0, sy),
            "diagonal": (dg, [((zl + sz, zh + sz), (yl + sy, yh + sy))], sz, sy)}
    for what, (tgt, blocks, shz, shy) in want.items():
        keep = pkeep = None
        for p, r in blocks:
            kk, pk = _region(L, p, r, shz, shy)
            keep, pkeep = (kk, pk) if keep is None else (keep | kk, pkeep | pk)
        for i, (mask, f) in enumerate(((keep, 1), (pkeep, 2))):
            got, src = tgt[i].t.cpu(), ref[i].t.cpu()
            mb = _blocked(mask, k)
            assert bool((_raw(got)[~mb] == SENTINEL).all()), f"{what} carry out wrote outside its range ({i})"
            moved = torch.roll(R.bits(src), (-(shz // f), -(shy // f)), dims=(2, 3))
            assert torch.equal(R.bits(got)[mb], moved[mb]), f"{what} carry out differs from the batch's own output ({i})"
            assert not bool((_raw(got)[mb] == SENTINEL).all(dim=-1).all()), what
            assert tgt[i].guards_intact()
    # the batch's own buffers hold their own bits where it computes, and nothing where it took over
    mine, pmine = _region(L, (0, d), (0, h), 0, 0)
    if with_in:
        for mask, f in ((mine, 1), (pmine, 2)):
            mask[:, :, zl // f:zh // f] = False
            mask[:, :, :, yl // f:yh // f] = False
    for i, mask in enumerate((mine, pmine)):
        mb = _blocked(mask, k)
        assert torch.equal(R.bits(own[i].t.cpu())[mb], R.bits(ref[i].t.cpu())[mb])
        assert bool((_raw(own[i].t.cpu())[~mb] == SENTINEL).all()), "the launch wrote a block it took over"
        assert own[i].guards_intact()


BAD = [
    ("odd in", dict(y=(9, 24, 0, 0, 0))),
    ("partial tile in", dict(y=(8, 20, 0, 0, 0))),
    ("in below 2", dict(y=(0, 8, 0, 0, 0))),
    ("in beyond h - 2", dict(y=(40, 48, 0, 0, 0))),
    ("in reversed", dict(y=(24, 8, 0, 0, 0))),
    ("odd out", dict(y=(0, 0, 25, 40, 16), yt=True)),
    ("out beyond h - 2", dict(y=(0, 0, 24, 48, 16), yt=True)),
    ("target below 2", dict(y=(0, 0, 16, 32, 16), yt=True)),
    ("odd shift", dict(y=(0, 0, 24, 40, 15), yt=True)),
    ("out without targets", dict(y=(0, 0, 24, 40, 16))),
    ("targets without a range", dict(y=(0, 0, 0, 0, 0), yt=True)),
    ("out overlaps in", dict(y=(8, 32, 24, 40, 16), yt=True)),
    ("diagonal without the z carry out", dict(y=(0, 0, 24, 40, 16), yt=True, dg=True)),
    ("diagonal without the y carry out", dict(y=(8, 24, 0, 0, 0), z=(0, 0, 20, 28, 16), zt=True, dg=True)),
    ("z out overlaps z in, diagonal", dict(y=(0, 0, 24, 40, 16), yt=True, dg=True, z=(4, 24, 20, 28, 16), zt=True)),
    ("no row mode", dict(y=(8, 24, 0, 0, 0), stride=0)),
]


@pytest.mark.parametrize("what,kw", BAD, ids=[b[0] for b in BAD])
def test_argument_checks(probe, what, kw):
    L = _four(SMALL, "bf16", seed=5)[1, 1]
    s, ps = _shapes(L)
    own, zt, yt, dg = ([Guarded(s, "bf16"), Guarded(ps, "bf16")] for _ in range(4))
    msg = _launch(probe, L, own, kw.get("z", (0, 0, 0, 0, 0)), zt if kw.get("zt") else None, kw["y"],
                  yt if kw.get("yt") else None, dg if kw.get("dg") else None, stages=MAIN, expect_rc=E_INVALID,
                  stride=kw.get("stride"))
    assert "carry" in msg or "row mode" in msg, msg
    torch.cuda.synchronize()
    for pair in (own, zt, yt, dg):       # refused before anything was launched
        for gbuf in pair:
            assert bool((gbuf.raw == SENTINEL).all())
