"""
Per-layer tests of inc.3's carried planes (ConvArgs::in_z0 .. out_shift, conv3x3x3_zpipe_rowz).

A row launch A stores a plane range of its output a second time, shifted, into the buffers of the row
B that lies `shift` planes further down z; B's launch leaves those z tiles out. Everything is held bit
for bit to the uncarried row sequence (which test_gpu_row_layers.py holds to float64 references). B's
operands agree with A's only on the planes the carried range reads, [lo - 1, hi + 1) of B's frame: a
plane carried beyond the range, or left out beyond it, shows as different bits.
"""

import ctypes

import pytest
import torch

import layer_ref as R
from test_gpu_layers import E_INVALID, SENTINEL, _ptr, encode_conv_weights, probe as _base_probe  # noqa: F401
from test_gpu_row_layers import RowLayer, _blocked, _same_bits

pytestmark = pytest.mark.gpu

DTS = ["bf16", "f16"]
MAIN, BORDERS = 1, 8
POISON = 0xA5
GUARD = 256
# (ca, cout, cout_real, n, d, h, w, stride), shift, carried range of the later frame, tile depth
BIG = ((32, 32, 32, 2, 96, 16, 96, 64), 64, (6, 30), 6)
SMALL = ((32, 32, 32, 2, 32, 16, 64, 32), 16, (4, 12), 4)
CASES = {"96x16x96": BIG, "32x16x64": SMALL}


@pytest.fixture(scope="module")
def probe(_base_probe):  # noqa: F811
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    fn = _base_probe.probe_conv3x3x3_row_carry
    fn.restype = i32
    fn.argtypes = [i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp, ctypes.POINTER(i32), vp, vp,
                   i32, vp]
    _base_probe.probe_last_carry.restype = i32
    _base_probe.probe_last_carry.argtypes = []
    return _base_probe


class Guarded:
    """A storage tensor between two guard bands, every byte pre-filled."""

    def __init__(self, shape, dt, fill=SENTINEL):
        nbytes = 2 * int(torch.tensor(shape).prod())
        self.raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
        self.t = self.raw[GUARD:GUARD + nbytes].view(R.STORAGE[dt]).view(shape)
        self.fill = fill

    def guards_intact(self):
        return bool((self.raw[:GUARD] == self.fill).all() and (self.raw[-GUARD:] == self.fill).all())


def _shapes(L):
    n, d, h, w = L.shape
    k = R.kc(L.dt)
    return (n, L.cout // k, d, h, w, k), (n, L.cout // k, d // 2, h // 2, w // 2, k)


def _launch(probe, L, dst, pdst, carry=(0, 0, 0, 0, 0), cdst=None, cpdst=None, stages=MAIN | BORDERS, expect_rc=0,
            stride=None):
    """launch_conv3x3x3_row with carry fields on device tensors the caller owns."""
    n, d, h, w = L.shape
    xa = R.pack_blocked(L.x, L.dt).cuda()
    wt = encode_conv_weights(L.w.numpy(), L.dt).cuda()
    bt = L.b.to(torch.float32).cuda()
    probe.probe_reset_config()
    torch.cuda.synchronize()
    rc = probe.probe_conv3x3x3_row_carry(R.DTYPES[L.dt], _ptr(xa), L.ca, _ptr(wt), _ptr(bt), _ptr(dst), L.cout, n, d,
                                         h, w, R.SLOPE, L.stride if stride is None else stride, _ptr(pdst),
                                         (ctypes.c_int32 * 5)(*carry), _ptr(cdst), _ptr(cpdst), stages, None)
    if expect_rc:
        assert rc == expect_rc, rc
        return probe.probe_last_error().decode()
    assert rc == 0, probe.probe_last_error().decode()
    torch.cuda.synchronize()
    return probe.probe_last_carry() if stages == MAIN else None


def _pair(case, dt, seed, n=None, special=False):
    """Row A and the row B `shift` planes below it: B's operands are fresh except on the planes the carried
    range reads, where they are A's."""
    g, shift, (lo, hi), _ = case
    if n is not None:
        g = g[:3] + (n,) + g[4:]
    ca, cout, _, n, d, h, w, stride = g
    xa = R.row_inputs(n, ca, d, h, w, stride, torch.Generator().manual_seed(seed))
    xb = R.row_inputs(n, ca, d, h, w, stride, torch.Generator().manual_seed(seed + 1))
    bias = None
    if special:
        # a NaN that reaches carried planes lo + 1 .. lo + 3 of every channel, in a shared column and in an
        # own one; channel 0 saturates a half everywhere (bias beyond 65504)
        xa[0, 3, lo + 2 + shift, 5, stride + 7] = float("nan")
        xa[1, 3, lo + 2 + shift, 5, 7] = float("nan")
        xa[0, 4, hi - 2 + shift, 9, 20] = float("nan")
        bias = torch.zeros(cout, dtype=torch.float64)
        bias[0], bias[1] = 70000.0, -0.25
    xb[:, :, lo - 1:hi + 1] = xa[:, :, lo - 1 + shift:hi + 1 + shift]
    A = RowLayer(dt, g, seed=seed, x=xa)
    if bias is not None:
        A.b = bias
    B = RowLayer(dt, g, seed=seed, x=xb, weights=A.w)
    B.w, B.b = A.w, A.b
    return A, B


def _main_masks(L, lo, hi):
    """What a carry out of planes [lo, hi) (target frame) writes: those planes but the neighbour-facing
    outermost x, and their pooled planes but the neighbour-facing pooled border column."""
    m, pm = L.border_masks()
    keep, pkeep = ~m, ~pm
    keep[:, :, :lo], keep[:, :, hi:] = False, False
    pkeep[:, :, :lo // 2], pkeep[:, :, hi // 2:] = False, False
    return keep, pkeep


def _raw(t):
    return R.bits(t).view(torch.uint8).reshape(t.shape + (-1,))


def _carried_run(probe, A, B, case):
    """A uncarried and with carry out; B uncarried and with carry in on what A left. Returns everything."""
    _, shift, (lo, hi), tz = case
    dt = A.dt
    s, ps = _shapes(A)
    ref_a = [Guarded(s, dt), Guarded(ps, dt)]
    _launch(probe, A, ref_a[0].t, ref_a[1].t)
    own_a = [Guarded(s, dt), Guarded(ps, dt)]
    tgt = [Guarded(s, dt), Guarded(ps, dt)]
    _launch(probe, A, own_a[0].t, own_a[1].t, (0, 0, lo + shift, hi + shift, shift), tgt[0].t, tgt[1].t, stages=MAIN)
    after_a = [tgt[0].t.cpu().clone(), tgt[1].t.cpu().clone()]
    _launch(probe, A, own_a[0].t, own_a[1].t, stages=BORDERS)
    ref_b = [Guarded(s, dt), Guarded(ps, dt)]
    _launch(probe, B, ref_b[0].t, ref_b[1].t)
    was_carry = _launch(probe, B, tgt[0].t, tgt[1].t, (lo, hi, 0, 0, 0), stages=MAIN)
    _launch(probe, B, tgt[0].t, tgt[1].t, stages=BORDERS)
    return ref_a, own_a, tgt, after_a, ref_b, was_carry


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(CASES))
def test_carry_out_then_in(probe, dt, name):
    case = CASES[name]
    _, shift, (lo, hi), tz = case
    A, B = _pair(case, dt, seed=11)
    ref_a, own_a, tgt, after_a, ref_b, was_carry = _carried_run(probe, A, B, case)
    assert was_carry == 1
    # A's own output does not change
    _same_bits(own_a[0].t.cpu(), ref_a[0].t.cpu(), "A dst")
    _same_bits(own_a[1].t.cpu(), ref_a[1].t.cpu(), "A pool")
    # the carry out wrote exactly the planes, columns and pooled planes named, with A's own bits
    keep, pkeep = _main_masks(A, lo, hi)
    k = R.kc(dt)
    for got, ref, mask, sh, what in ((after_a[0], ref_a[0].t.cpu(), keep, shift, "dst"),
                                     (after_a[1], ref_a[1].t.cpu(), pkeep, shift // 2, "pool")):
        mb = _blocked(mask, k)
        assert bool((_raw(got)[~mb] == SENTINEL).all()), f"carry out wrote {what} outside its range"
        want = torch.roll(R.bits(ref), -sh, dims=2)     # plane z of the target frame is A's plane z + shift
        assert torch.equal(R.bits(got)[mb], want[mb]), f"carried {what} differs from A's own output"
        assert not bool((_raw(got)[mb] == SENTINEL).all(dim=-1).all()), what
    # B on the carried planes: the whole output and pool have the uncarried bits
    _same_bits(tgt[0].t.cpu(), ref_b[0].t.cpu(), "B dst")
    _same_bits(tgt[1].t.cpu(), ref_b[1].t.cpu(), "B pool")
    for gbuf in ref_a + own_a + tgt + ref_b:
        assert gbuf.guards_intact()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(CASES))
def test_carry_in_leaves_the_carried_planes_alone(probe, dt, name):
    case = CASES[name]
    _, shift, (lo, hi), tz = case
    _, B = _pair(case, dt, seed=23)
    s, ps = _shapes(B)
    dst, pdst = Guarded(s, dt, POISON), Guarded(ps, dt, POISON)
    assert _launch(probe, B, dst.t, pdst.t, (lo, hi, 0, 0, 0), stages=MAIN) == 1
    assert bool((_raw(dst.t.cpu())[:, :, lo:hi] == POISON).all()), "a left-out plane was rewritten"
    assert bool((_raw(pdst.t.cpu())[:, :, lo // 2:hi // 2] == POISON).all()), "a left-out pooled plane was rewritten"
    # ... and every other plane the row launch owns was written
    keep, pkeep = _main_masks(B, 0, s[2])
    keep[:, :, lo:hi], pkeep[:, :, lo // 2:hi // 2] = False, False
    k = R.kc(dt)
    ref, pref = Guarded(s, dt), Guarded(ps, dt)
    _launch(probe, B, ref.t, pref.t, stages=MAIN)
    assert torch.equal(R.bits(dst.t.cpu())[_blocked(keep, k)], R.bits(ref.t.cpu())[_blocked(keep, k)])
    assert torch.equal(R.bits(pdst.t.cpu())[_blocked(pkeep, k)], R.bits(pref.t.cpu())[_blocked(pkeep, k)])
    assert dst.guards_intact() and pdst.guards_intact()


@pytest.mark.parametrize("dt", DTS)
def test_carry_nan_and_saturation(probe, dt):
    A, B = _pair(SMALL, dt, seed=31, special=True)
    ref_a, own_a, tgt, after_a, ref_b, _ = _carried_run(probe, A, B, SMALL)
    _, shift, (lo, hi), _ = SMALL
    got = R.unpack_blocked(after_a[0])
    assert bool(torch.isnan(got[:, :, lo + 1:lo + 4]).any()), "no NaN reached the carried planes"
    if dt == "f16":
        keep, _ = _main_masks(A, lo, hi)
        v = got[:, 0][keep[:, 0]]
        assert bool(((v == 65504.0) | torch.isnan(v)).all()) and bool((v == 65504.0).any()), \
            "channel 0 of the carried planes does not saturate"
    _same_bits(tgt[0].t.cpu(), ref_b[0].t.cpu(), "B dst")
    _same_bits(tgt[1].t.cpu(), ref_b[1].t.cpu(), "B pool")
    _same_bits(own_a[0].t.cpu(), ref_a[0].t.cpu(), "A dst")


@pytest.mark.parametrize("dt", DTS)
def test_carry_more_tiles_than_workgroups(probe, dt):
    # 32-cout slices, MINW = 2 -> max(8, 2 * CUs // 8 * 8) persistent workgroups; n 32 x 16 x 64 patches 32 apart
    # are 8 (carry in: 6) x 2 x (2n + 2) tiles
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    wgs = max(8, 2 * cus // 8 * 8)
    n = -(-(wgs + 8) // (6 * 2 * 2))
    assert 6 * 2 * (2 * n + 2) > wgs
    A, B = _pair(SMALL, dt, seed=41, n=n)
    ref_a, own_a, tgt, after_a, ref_b, was_carry = _carried_run(probe, A, B, SMALL)
    assert was_carry == 1
    _same_bits(own_a[0].t.cpu(), ref_a[0].t.cpu(), "A dst")
    _same_bits(own_a[1].t.cpu(), ref_a[1].t.cpu(), "A pool")
    _same_bits(tgt[0].t.cpu(), ref_b[0].t.cpu(), "B dst")
    _same_bits(tgt[1].t.cpu(), ref_b[1].t.cpu(), "B pool")
    for gbuf in tgt + own_a:
        assert gbuf.guards_intact()


BAD = [
    ("odd in", (5, 12, 0, 0, 0), False, None),
    ("misaligned in", (6, 12, 0, 0, 0), False, None),          # even, but not 4-plane tiles
    ("in below 2", (0, 8, 0, 0, 0), False, None),
    ("in beyond d - 2", (24, 32, 0, 0, 0), False, None),
    ("in reversed", (12, 4, 0, 0, 0), False, None),
    ("odd out", (0, 0, 21, 28, 16), True, None),
    ("out beyond d - 2", (0, 0, 20, 32, 16), True, None),
    ("target below 2", (0, 0, 16, 28, 16), True, None),
    ("odd shift", (0, 0, 20, 28, 15), True, None),
    ("out without targets", (0, 0, 20, 28, 16), False, None),
    ("targets without a range", (0, 0, 0, 0, 0), True, None),
    ("no row mode", (4, 12, 0, 0, 0), False, 0),
]


@pytest.mark.parametrize("what,carry,targets,stride", BAD, ids=[b[0] for b in BAD])
def test_carry_argument_checks(probe, what, carry, targets, stride):
    _, B = _pair(SMALL, "bf16", seed=5)
    s, ps = _shapes(B)
    dst, pdst, cd, cpd = (Guarded(x, "bf16") for x in (s, ps, s, ps))
    msg = _launch(probe, B, dst.t, pdst.t, carry, cd.t if targets else None, cpd.t if targets else None,
                  stages=MAIN, expect_rc=E_INVALID, stride=stride)
    assert "carry" in msg or "row mode" in msg, msg
    torch.cuda.synchronize()
    for gbuf in (dst, pdst, cd, cpd):       # refused before anything was launched
        assert bool((gbuf.raw == SENTINEL).all())
