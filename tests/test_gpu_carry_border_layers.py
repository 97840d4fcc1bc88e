"""
Per-layer tests of inc.3's border launch with carried planes (launch_conv3x3x3_row, kRowStageBordersCarry = 16,
conv3x3x3_t14_borders_carry).

The sequence Main | BordersCarry of a row A stores a plane range of its output a second time, shifted, at EVERY x
into the buffers of the row B that lies `shift` planes further down z; B's two launches then compute and store no
plane of the range, and nothing that reaches a stored value reads planes [lo + 1, hi - 1) of B's source. Everything
is held bit for bit to the uncarried sequence Main | Borders (which test_gpu_row_borders.py and
test_gpu_row_layers.py hold to float64 references). The helpers, geometries and the refusal table are
test_gpu_carry_layers.py's.
"""

import ctypes

import pytest
import torch

import layer_ref as R
from test_gpu_carry_layers import (BAD, BIG, BORDERS, MAIN, POISON, SMALL, Guarded, _launch, _pair, _raw, _shapes,
                                   probe as _carry_probe)  # noqa: F401
from test_gpu_layers import E_INVALID, SENTINEL, probe as _base_probe  # noqa: F401  (module-scoped fixture)
from test_gpu_row_layers import _blocked, _same_bits

pytestmark = pytest.mark.gpu

DTS = ["bf16", "f16"]
BORDERS_CARRY = 16
CARRY = MAIN | BORDERS_CARRY
# the geometries of test_gpu_carry_layers.py, and each with n = 3: the middle patch has both jobs
CASES = {"32x16x64": (SMALL, None), "96x16x96": (BIG, None), "32x16x64 n3": (SMALL, 3), "96x16x96 n3": (BIG, 3)}
# 12 planes: the one depth with room for a carry out at which the border launch picks its 4-plane tile
# (target-frame planes [2, 8) are A's planes [4, 10))
TINY = ((32, 32, 32, 3, 12, 16, 64, 32), 2, (2, 8), 6)
OUT_CASES = dict(CASES, **{"12x16x64 n3": (TINY, None)})


@pytest.fixture(scope="module")
def probe(_carry_probe):  # noqa: F811
    i32 = ctypes.c_int32
    _carry_probe.probe_conv_first_skip_planes.restype = None
    _carry_probe.probe_conv_first_skip_planes.argtypes = [i32, i32, i32, ctypes.POINTER(i32)]
    return _carry_probe


def _plane_masks(L, lo, hi):
    """Planes [lo, hi) at every x, and pooled planes [lo / 2, hi / 2) at every pooled x."""
    n, d, h, w = L.shape
    m = torch.zeros((n, L.cout, d, h, w), dtype=torch.bool)
    pm = torch.zeros((n, L.cout, d // 2, h // 2, w // 2), dtype=torch.bool)
    m[:, :, lo:hi] = True
    pm[:, :, lo // 2:hi // 2] = True
    return m, pm


def _uncarried(probe, L):
    s, ps = _shapes(L)
    ref = [Guarded(s, L.dt), Guarded(ps, L.dt)]
    _launch(probe, L, ref[0].t, ref[1].t, stages=MAIN | BORDERS)
    assert ref[0].guards_intact() and ref[1].guards_intact()
    return [ref[0].t.cpu().clone(), ref[1].t.cpu().clone()]


def _carry_out(probe, A, case):
    """A with Main | BordersCarry and a carry out into sentinel-filled targets: own buffers and targets."""
    _, shift, (lo, hi), _ = case
    s, ps = _shapes(A)
    own = [Guarded(s, A.dt), Guarded(ps, A.dt)]
    tgt = [Guarded(s, A.dt), Guarded(ps, A.dt)]
    _launch(probe, A, own[0].t, own[1].t, (0, 0, lo + shift, hi + shift, shift), tgt[0].t, tgt[1].t, stages=CARRY)
    return own, tgt


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(OUT_CASES))
def test_carry_out_holds_every_x_of_the_carried_planes(probe, dt, name):
    case, n = OUT_CASES[name]
    _, shift, (lo, hi), _ = case
    A, _ = _pair(case, dt, seed=13, n=n)
    ref_a = _uncarried(probe, A)
    own, tgt = _carry_out(probe, A, case)
    # A's own output is the uncarried sequence's
    _same_bits(own[0].t.cpu(), ref_a[0], "A dst")
    _same_bits(own[1].t.cpu(), ref_a[1], "A pool")
    k = R.kc(dt)
    m, pm = _plane_masks(A, lo, hi)
    for got, ref, mask, sh, what in ((tgt[0].t.cpu(), ref_a[0], m, shift, "dst"),
                                     (tgt[1].t.cpu(), ref_a[1], pm, shift // 2, "pool")):
        mb = _blocked(mask, k)
        assert bool((_raw(got)[~mb] == SENTINEL).all()), f"carry out wrote {what} outside its planes"
        want = torch.roll(R.bits(ref), -sh, dims=2)     # plane z of the target frame is A's plane z + shift
        diff = (R.bits(got) != want) & mb
        assert not diff.any(), f"carried {what}: {int(diff.sum())} values differ, first at {diff.nonzero()[0].tolist()}"
    for g in own + tgt:
        assert g.guards_intact()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(CASES))
def test_carry_in_leaves_the_carried_planes_alone(probe, dt, name):
    case, n = CASES[name]
    _, shift, (lo, hi), _ = case
    _, B = _pair(case, dt, seed=29, n=n)
    ref = _uncarried(probe, B)
    s, ps = _shapes(B)
    dst, pdst = Guarded(s, dt, POISON), Guarded(ps, dt, POISON)
    _launch(probe, B, dst.t, pdst.t, (lo, hi, 0, 0, 0), stages=CARRY)
    got, pgot = dst.t.cpu(), pdst.t.cpu()
    assert bool((_raw(got)[:, :, lo:hi] == POISON).all()), "a plane carried in was rewritten"
    assert bool((_raw(pgot)[:, :, lo // 2:hi // 2] == POISON).all()), "a pooled plane carried in was rewritten"
    keep = torch.ones(s[2], dtype=torch.bool)
    keep[lo:hi] = False
    pkeep = torch.ones(ps[2], dtype=torch.bool)
    pkeep[lo // 2:hi // 2] = False
    assert torch.equal(R.bits(got)[:, :, keep], R.bits(ref[0])[:, :, keep]), "a computed plane differs"
    assert torch.equal(R.bits(pgot)[:, :, pkeep], R.bits(ref[1])[:, :, pkeep]), "a computed pooled plane differs"
    assert dst.guards_intact() and pdst.guards_intact()


def _a_then_b(probe, A, B, case):
    """A carries out into B's buffers; B runs with the carry in on a source that is NaN on exactly the planes
    conv_first_skip_planes names. Returns B's buffers and the uncarried B."""
    _, shift, (lo, hi), _ = case
    ref_b = _uncarried(probe, B)        # (on the whole source)
    own, tgt = _carry_out(probe, A, case)
    skip = (ctypes.c_int32 * 2)()
    probe.probe_conv_first_skip_planes(B.shape[1], lo, hi, skip)
    assert tuple(skip) == (lo + 1, hi - 1)
    B.x = B.x.clone()
    B.x[:, :, skip[0]:skip[1]] = float("nan")
    _launch(probe, B, tgt[0].t, tgt[1].t, (lo, hi, 0, 0, 0), stages=CARRY)
    for g in own + tgt:
        assert g.guards_intact()
    return tgt, ref_b, own


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(CASES))
def test_a_then_b_on_a_source_without_the_skipped_planes(probe, dt, name):
    case, n = CASES[name]
    A, B = _pair(case, dt, seed=17, n=n)
    tgt, ref_b, _ = _a_then_b(probe, A, B, case)
    # a read of a skipped plane that reaches a stored value shows as NaN
    _same_bits(tgt[0].t.cpu(), ref_b[0], "B dst")
    _same_bits(tgt[1].t.cpu(), ref_b[1], "B pool")


@pytest.mark.parametrize("dt", DTS)
def test_nan_and_saturation_in_an_own_border_column(probe, dt):
    _, shift, (lo, hi), _ = SMALL
    A, B = _pair(SMALL, dt, seed=37, n=3, special=True)     # channel 0 saturates a half everywhere
    w = A.shape[3]
    # a NaN in patch 1's own x = 0 and in its own x = w - 1 (it has both jobs), on a carried plane
    for L, z in ((A, lo + 2 + shift), (B, lo + 2)):
        L.x = L.x.clone()
        L.x[1, 2, z, 5, 0] = float("nan")
        L.x[1, 6, z + 2, 9, w - 1] = float("nan")
    ref_a = _uncarried(probe, A)
    own, tgt = _carry_out(probe, A, SMALL)
    got = R.unpack_blocked(tgt[0].t.cpu())
    assert bool(torch.isnan(got[1, :, lo + 1:lo + 4, 4:7, :2]).all()), "the NaN of x = 0 did not reach the target"
    assert bool(torch.isnan(got[1, :, lo + 3:lo + 6, 8:11, w - 2:]).all()), "the NaN of x = w - 1 did not reach the target"
    pooled = R.unpack_blocked(tgt[1].t.cpu())
    assert bool(torch.isnan(pooled[1, :, (lo + 2) // 2, 2, 0]).all()) and bool(torch.isnan(pooled[1, :, (lo + 4) // 2, 4, w // 2 - 1]).all())
    if dt == "f16":
        v = got[:, 0, lo:hi]
        border = torch.cat([v[1:, ..., :2].reshape(-1), v[:-1, ..., w - 2:].reshape(-1)])
        assert bool(((border == 65504.0) | torch.isnan(border)).all()) and bool((border == 65504.0).any()), \
            "channel 0 of the carried border columns does not saturate"
    _same_bits(own[0].t.cpu(), ref_a[0], "A dst")
    _same_bits(own[1].t.cpu(), ref_a[1], "A pool")
    # ... and B on what A left has the uncarried bits, NaN included
    ref_b = _uncarried(probe, B)
    _launch(probe, B, tgt[0].t, tgt[1].t, (lo, hi, 0, 0, 0), stages=CARRY)
    _same_bits(tgt[0].t.cpu(), ref_b[0], "B dst")
    _same_bits(tgt[1].t.cpu(), ref_b[1], "B pool")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["32x16x64", "96x16x96", "12x16x64 n3"])
def test_launch_record_names_the_carrying_symbol(probe, dt, name):
    case, _ = OUT_CASES[name]
    _, shift, (lo, hi), _ = case
    _, B = _pair(case, dt, seed=3)
    s, ps = _shapes(B)
    dst, pdst, cd, cpd = Guarded(s, dt), Guarded(ps, dt), Guarded(s, dt), Guarded(ps, dt)
    if case is TINY:    # (no room for a range carried in at 12 planes)
        _launch(probe, B, dst.t, pdst.t, (0, 0, lo + shift, hi + shift, shift), cd.t, cpd.t, stages=BORDERS_CARRY)
    else:
        _launch(probe, B, dst.t, pdst.t, (lo, hi, 0, 0, 0), stages=BORDERS_CARRY)
    config = probe.probe_last_config().decode()
    assert probe.probe_last_carry() == 1 and "launch_row_borders_carry_cfg" in config, config
    assert f"TZ = {4 if case is TINY else 8}" in config and ("BF16Tag" in config) == (dt == "bf16"), config
    # with no carry field set stage 16 is stage 8
    _launch(probe, B, dst.t, pdst.t, stages=BORDERS_CARRY)
    config = probe.probe_last_config().decode()
    assert probe.probe_last_carry() == 0 and "launch_row_borders_cfg" in config, config
    ref, pref = Guarded(s, dt), Guarded(ps, dt)
    _launch(probe, B, ref.t, pref.t, stages=BORDERS)
    fresh, pfresh = Guarded(s, dt), Guarded(ps, dt)
    _launch(probe, B, fresh.t, pfresh.t, stages=BORDERS_CARRY)
    assert torch.equal(fresh.raw, ref.raw) and torch.equal(pfresh.raw, pref.raw)


@pytest.mark.parametrize("dt", DTS)
def test_stage_8_ignores_the_carry_fields(probe, dt):
    _, shift, (lo, hi), _ = SMALL
    _, B = _pair(SMALL, dt, seed=43, n=3)
    s, ps = _shapes(B)
    ref, pref = Guarded(s, dt, POISON), Guarded(ps, dt, POISON)
    _launch(probe, B, ref.t, pref.t, stages=BORDERS)
    for carry, targets in (((lo, hi, 0, 0, 0), False), ((0, 0, lo + shift, hi + shift, shift), True)):
        dst, pdst = Guarded(s, dt, POISON), Guarded(ps, dt, POISON)
        cd, cpd = Guarded(s, dt), Guarded(ps, dt)
        _launch(probe, B, dst.t, pdst.t, carry, cd.t if targets else None, cpd.t if targets else None, stages=BORDERS)
        assert probe.probe_last_carry() == 0
        assert "launch_row_borders_cfg" in probe.probe_last_config().decode()
        assert torch.equal(dst.raw, ref.raw) and torch.equal(pdst.raw, pref.raw), "stage 8 did not write every plane"
        assert bool((cd.raw == SENTINEL).all()) and bool((cpd.raw == SENTINEL).all()), "stage 8 carried out"
    m, pm = B.border_masks()
    got = _raw(ref.t.cpu())
    mb = _blocked(m, R.kc(dt))
    assert torch.equal(R.bits(ref.t.cpu())[mb], R.bits(_uncarried(probe, B)[0])[mb]), "a border value was left unwritten"
    assert bool((got[~_blocked(m, R.kc(dt))] == POISON).all())
    assert ref.guards_intact() and pref.guards_intact()


OVERLAP = [("out inside the planes carried in", (20, 28, 20, 28, 16), True, None),
           ("out across the end of the planes carried in", (16, 24, 20, 28, 16), True, None)]


@pytest.mark.parametrize("stages", [BORDERS_CARRY, CARRY])
@pytest.mark.parametrize("what,carry,targets,stride", BAD + OVERLAP, ids=[b[0] for b in BAD + OVERLAP])
def test_carry_argument_checks(probe, what, carry, targets, stride, stages):
    _, B = _pair(SMALL, "bf16", seed=5)
    s, ps = _shapes(B)
    dst, pdst, cd, cpd = (Guarded(x, "bf16") for x in (s, ps, s, ps))
    msg = _launch(probe, B, dst.t, pdst.t, carry, cd.t if targets else None, cpd.t if targets else None,
                  stages=stages, expect_rc=E_INVALID, stride=stride)
    assert "carry" in msg or "row mode" in msg, msg
    torch.cuda.synchronize()
    for gbuf in (dst, pdst, cd, cpd):       # refused before anything was launched
        assert bool((gbuf.raw == SENTINEL).all())
