"""
Per-layer tests of the second level's carried planes (ConvArgs::in_z0 .. out_shift outside row mode,
conv3x3x3_t14_carry with and without the fused max-pool: down1.3 and down1.0).

A launch A stores a plane range of its output a second time, shifted, into the buffers of the launch B whose
patches lie `shift` level-1 planes further down z; B's launch leaves those z tiles out. Everything is held bit
for bit to the uncarried launch, and that to the float64 per-patch convolution with check_conv's bound. B's
operands agree with A's only on the planes the carried range reads, [lo - 1, hi + 1) of B's frame: a plane
carried beyond the range, or left out beyond it, shows as different bits.

The shapes are level 1 of the patches 48 x 16 x 64 (z shift 16 and 24) and 64 x 32 x 96 (z shift 32), n = 2.
"""

import ctypes

import pytest
import torch

import layer_ref as R
from test_gpu_layers import E_INVALID, SENTINEL, Layer, _ptr, encode_conv_weights, probe as _base_probe  # noqa: F401
from test_gpu_row_layers import _same_bits

pytestmark = pytest.mark.gpu

DTS = ["bf16", "f16"]
POISON = 0xA5
GUARD = 256
# (n, d, h, w) of the level-1 tensors, level-1 shift, carried range of the later frame
CASES = {
    "24x8x32 shift 8": ((2, 24, 8, 32), 8, (4, 12)),
    "24x8x32 shift 12": ((2, 24, 8, 32), 12, (4, 8)),
    "32x16x48 shift 16": ((2, 32, 16, 48), 16, (4, 12)),
}
SMALL = CASES["24x8x32 shift 8"]
# pool: down1.3 (64 -> 64, fused max-pool); plain: down1.0 (32 -> 64)
KINDS = {"pool": (64, True), "plain": (32, False)}


@pytest.fixture(scope="module")
def probe(_base_probe):  # noqa: F811
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    fn = _base_probe.probe_conv3x3x3_carry
    fn.restype = i32
    fn.argtypes = [i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, ctypes.c_size_t,
                   ctypes.POINTER(i32), vp, vp, vp]
    _base_probe.probe_last_carry.restype = i32
    _base_probe.probe_last_carry.argtypes = []
    return _base_probe


class Guarded:
    """A storage tensor between two guard bands, every byte pre-filled."""

    def __init__(self, shape, dt, fill=SENTINEL):
        nbytes = R.es(dt) * int(torch.tensor(shape).prod())
        self.raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
        self.t = self.raw[GUARD:GUARD + nbytes].view(R.STORAGE[dt]).view(shape)
        self.fill = fill

    def guards_intact(self):
        return bool((self.raw[:GUARD] == self.fill).all() and (self.raw[-GUARD:] == self.fill).all())


def _shapes(L):
    n, d, h, w = L.shape
    k = R.kc(L.dt)
    return (n, L.cout // k, d, h, w, k), (n, L.cout // k, d // 2, h // 2, w // 2, k)


def _launch(probe, L, dst, pdst, carry=(0, 0, 0, 0, 0), cdst=None, cpdst=None, expect_rc=0, partial=False,
            dt_arg=None):
    """launch_conv3x3x3 with carry fields on device tensors the caller owns; returns (carry flag, split-K)."""
    n, d, h, w = L.shape
    xa = R.pack_blocked(L.x, L.dt).cuda()
    wt = encode_conv_weights(L.w.numpy(), L.dt).cuda()
    bt = L.b.to(torch.float32).cuda()
    part, part_bytes = None, 0
    if partial:
        part_bytes = 4 * d * h * w * L.cout * 4
        part = torch.empty(n * part_bytes // 4, dtype=torch.float32, device="cuda")
    probe.probe_reset_config()
    torch.cuda.synchronize()
    rc = probe.probe_conv3x3x3_carry(R.DTYPES[dt_arg or L.dt], _ptr(xa), L.ca, _ptr(wt), _ptr(bt), _ptr(dst), L.cout, n,
                                     d, h, w, R.SLOPE, _ptr(pdst), _ptr(part), part_bytes,
                                     (ctypes.c_int32 * 5)(*carry), _ptr(cdst), _ptr(cpdst), None)
    if expect_rc:
        assert rc == expect_rc, rc
        return probe.probe_last_error().decode()
    assert rc == 0, probe.probe_last_error().decode()
    torch.cuda.synchronize()
    return probe.probe_last_carry(), probe.probe_last_ksplit()


def _pair(case, dt, kind, seed, cout=64, special=False):
    """Launch A and the launch B `shift` planes below it: B's operands are fresh except on the planes the
    carried range reads, where they are A's."""
    (n, d, h, w), shift, (lo, hi) = case
    ca, _ = KINDS[kind]
    A = Layer(dt, ca, 0, cout, n, d, h, w, seed=seed)
    xa = A.x.clone()
    bias = None
    if special:
        # a NaN that reaches carried planes lo + 1 .. lo + 3 of every channel and one that reaches the last
        # one; channel 0 saturates a half everywhere (bias beyond 65504)
        xa[0, 3, lo + 2 + shift, 5, 7] = float("nan")
        xa[1, 4, hi - 1 + shift, 2, 20] = float("nan")
        bias = A.b.clone()
        bias[0], bias[1] = 70000.0, -0.25
        A = Layer(dt, ca, 0, cout, n, d, h, w, seed=seed, x=xa, weights=A.w, bias=bias)
    xb = Layer(dt, ca, 0, cout, n, d, h, w, seed=seed + 1).x.clone()
    xb[:, :, lo - 1:hi + 1] = xa[:, :, lo - 1 + shift:hi + 1 + shift]
    B = Layer(dt, ca, 0, cout, n, d, h, w, seed=seed, x=xb, weights=A.w, bias=A.b)
    return A, B


def _raw(t):
    return R.bits(t).view(torch.uint8).reshape(t.shape + (-1,))


def _pooled(kind, shape, dt):
    return Guarded(shape, dt) if KINDS[kind][1] else None


def _t(g):
    return g.t if g is not None else None


def _carried_run(probe, A, B, case, kind):
    """A uncarried and with carry out; B uncarried and with carry in on what A left. Returns everything."""
    _, shift, (lo, hi) = case
    dt = A.dt
    s, ps = _shapes(A)
    ref_a = [Guarded(s, dt), _pooled(kind, ps, dt)]
    assert _launch(probe, A, ref_a[0].t, _t(ref_a[1])) == (0, 1)
    own_a = [Guarded(s, dt), _pooled(kind, ps, dt)]
    tgt = [Guarded(s, dt), _pooled(kind, ps, dt)]
    rec_a = _launch(probe, A, own_a[0].t, _t(own_a[1]), (0, 0, lo + shift, hi + shift, shift), tgt[0].t, _t(tgt[1]))
    after_a = [tgt[0].t.cpu().clone(), tgt[1].t.cpu().clone() if tgt[1] is not None else None]
    ref_b = [Guarded(s, dt), _pooled(kind, ps, dt)]
    _launch(probe, B, ref_b[0].t, _t(ref_b[1]))
    rec_b = _launch(probe, B, tgt[0].t, _t(tgt[1]), (lo, hi, 0, 0, 0))
    assert rec_a == (1, 1) and rec_b == (1, 1), "the launch record does not name the carry symbol"
    return ref_a, own_a, tgt, after_a, ref_b


def _check_float64(L, dst, mask=None, nan_ok=None):
    acc, s = L.ref()
    R.check_conv(R.unpack_blocked(dst), acc, s, L.ca, L.dt, cout_real=L.cout_real, mask=mask, nan_ok=nan_ok)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(CASES))
def test_carry_out_then_in(probe, dt, kind, name):
    case = CASES[name]
    _, shift, (lo, hi) = case
    A, B = _pair(case, dt, kind, seed=11)
    ref_a, own_a, tgt, after_a, ref_b = _carried_run(probe, A, B, case, kind)
    # A's own output does not change, and is the float64 convolution within check_conv's bound
    _same_bits(own_a[0].t.cpu(), ref_a[0].t.cpu(), "A dst")
    _check_float64(A, own_a[0].t.cpu())
    # the carry out wrote exactly the planes and pooled planes named, with A's own bits
    pairs = [(after_a[0], ref_a[0].t.cpu(), lo, hi, shift, "dst")]
    if KINDS[kind][1]:
        _same_bits(own_a[1].t.cpu(), ref_a[1].t.cpu(), "A pool")
        pairs.append((after_a[1], ref_a[1].t.cpu(), lo // 2, hi // 2, shift // 2, "pool"))
    for got, ref, p0, p1, sh, what in pairs:
        raw = _raw(got)
        assert bool((raw[:, :, :p0] == SENTINEL).all()) and bool((raw[:, :, p1:] == SENTINEL).all()), \
            f"carry out wrote {what} outside its range"
        # plane z of the target frame is A's plane z + shift
        assert torch.equal(R.bits(got)[:, :, p0:p1], R.bits(ref)[:, :, p0 + sh:p1 + sh]), \
            f"carried {what} differs from A's own output"
        assert not bool((raw[:, :, p0:p1] == SENTINEL).all(dim=-1).any()), f"a carried {what} record is missing"
    # B on the carried planes: the whole output and pool have the uncarried bits
    _same_bits(tgt[0].t.cpu(), ref_b[0].t.cpu(), "B dst")
    _check_float64(B, tgt[0].t.cpu())
    if KINDS[kind][1]:
        _same_bits(tgt[1].t.cpu(), ref_b[1].t.cpu(), "B pool")
    for gbuf in ref_a + own_a + tgt + ref_b:
        assert gbuf is None or gbuf.guards_intact()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(CASES))
def test_carry_in_leaves_the_carried_planes_alone(probe, dt, kind, name):
    case = CASES[name]
    _, shift, (lo, hi) = case
    _, B = _pair(case, dt, kind, seed=23)
    pool = KINDS[kind][1]
    s, ps = _shapes(B)
    dst, pdst = Guarded(s, dt, POISON), Guarded(ps, dt, POISON) if pool else None
    assert _launch(probe, B, dst.t, _t(pdst), (lo, hi, 0, 0, 0)) == (1, 1)
    ref, pref = Guarded(s, dt), Guarded(ps, dt) if pool else None
    _launch(probe, B, ref.t, _t(pref))
    got, want = dst.t.cpu(), ref.t.cpu()
    assert bool((_raw(got)[:, :, lo:hi] == POISON).all()), "a left-out plane was rewritten"
    # ... and every other plane was written, with the uncarried bits
    assert torch.equal(R.bits(got)[:, :, :lo], R.bits(want)[:, :, :lo])
    assert torch.equal(R.bits(got)[:, :, hi:], R.bits(want)[:, :, hi:])
    keep = torch.ones(R.unpack_blocked(got).shape, dtype=torch.bool)
    keep[:, :, lo:hi] = False
    _check_float64(B, got, mask=keep)
    if pool:
        got, want = pdst.t.cpu(), pref.t.cpu()
        assert bool((_raw(got)[:, :, lo // 2:hi // 2] == POISON).all()), "a left-out pooled plane was rewritten"
        assert torch.equal(R.bits(got)[:, :, :lo // 2], R.bits(want)[:, :, :lo // 2])
        assert torch.equal(R.bits(got)[:, :, hi // 2:], R.bits(want)[:, :, hi // 2:])
        assert pdst.guards_intact()
    assert dst.guards_intact()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_carry_nan_and_saturation(probe, dt, kind):
    A, B = _pair(SMALL, dt, kind, seed=31, special=True)
    ref_a, own_a, tgt, after_a, ref_b = _carried_run(probe, A, B, SMALL, kind)
    _, shift, (lo, hi) = SMALL
    got = R.unpack_blocked(after_a[0])
    assert bool(torch.isnan(got[:, :, lo + 1:lo + 4]).any()), "no NaN reached the carried planes"
    assert bool(torch.isnan(got[:, :, hi - 1]).any()), "no NaN reached the last carried plane"
    if dt == "f16":
        v = got[:, 0, lo:hi]
        assert bool(((v == 65504.0) | torch.isnan(v)).all()) and bool((v == 65504.0).any()), \
            "channel 0 of the carried planes does not saturate"
    _same_bits(own_a[0].t.cpu(), ref_a[0].t.cpu(), "A dst")
    assert torch.equal(R.bits(after_a[0])[:, :, lo:hi], R.bits(ref_a[0].t.cpu())[:, :, lo + shift:hi + shift])
    _same_bits(tgt[0].t.cpu(), ref_b[0].t.cpu(), "B dst")
    if KINDS[kind][1]:
        assert torch.equal(R.bits(after_a[1])[:, :, lo // 2:hi // 2],
                           R.bits(ref_a[1].t.cpu())[:, :, (lo + shift) // 2:(hi + shift) // 2])
        _same_bits(tgt[1].t.cpu(), ref_b[1].t.cpu(), "B pool")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_carry_two_cout_slices(probe, dt, kind):
    # 128 couts: two 64-cout slices (blockIdx.y), each with its own chunk planes of every target
    A, B = _pair(SMALL, dt, kind, seed=41, cout=128)
    ref_a, own_a, tgt, after_a, ref_b = _carried_run(probe, A, B, SMALL, kind)
    _, shift, (lo, hi) = SMALL
    _same_bits(own_a[0].t.cpu(), ref_a[0].t.cpu(), "A dst")
    assert torch.equal(R.bits(after_a[0])[:, :, lo:hi], R.bits(ref_a[0].t.cpu())[:, :, lo + shift:hi + shift])
    assert bool((_raw(after_a[0])[:, :, :lo] == SENTINEL).all()) and bool((_raw(after_a[0])[:, :, hi:] == SENTINEL).all())
    _same_bits(tgt[0].t.cpu(), ref_b[0].t.cpu(), "B dst")
    _check_float64(B, tgt[0].t.cpu())
    if KINDS[kind][1]:
        _same_bits(own_a[1].t.cpu(), ref_a[1].t.cpu(), "A pool")
        _same_bits(tgt[1].t.cpu(), ref_b[1].t.cpu(), "B pool")
    for gbuf in tgt + own_a:
        assert gbuf is None or gbuf.guards_intact()


# (carry, targets given, split-K scratch, dtype argument)
BAD = [
    ("odd in", (5, 12, 0, 0, 0), False, False, None),
    ("misaligned in", (6, 12, 0, 0, 0), False, False, None),          # even, but not 4-plane tiles
    ("in below 2", (0, 8, 0, 0, 0), False, False, None),
    ("in beyond d - 2", (20, 24, 0, 0, 0), False, False, None),
    ("in reversed", (12, 4, 0, 0, 0), False, False, None),
    ("odd out", (0, 0, 13, 20, 8), True, False, None),
    ("out beyond d - 2", (0, 0, 12, 24, 8), True, False, None),
    ("target below 2", (0, 0, 8, 20, 8), True, False, None),
    ("odd shift", (0, 0, 12, 20, 7), True, False, None),
    ("out without targets", (0, 0, 12, 20, 8), False, False, None),
    ("targets without a range", (0, 0, 0, 0, 0), True, False, None),
    ("split-K", (4, 12, 0, 0, 0), False, True, None),
    ("float32", (4, 12, 0, 0, 0), False, False, "f32"),
]


@pytest.mark.parametrize("what,carry,targets,partial,dt_arg", BAD, ids=[b[0] for b in BAD])
def test_carry_argument_checks(probe, what, carry, targets, partial, dt_arg):
    # (float32 has no fused max-pool on 64-cout slices: the plain layer, so that the carry is what gets refused)
    pool = dt_arg is None
    _, B = _pair(SMALL, "bf16", "pool" if pool else "plain", seed=5)
    s, ps = _shapes(B)
    dst, pdst, cd, cpd = (Guarded(x, "bf16") for x in (s, ps, s, ps))
    if partial:     # the layer is one the launcher splits when it has scratch: that is what gets refused
        plain = Layer("bf16", B.ca, 0, B.cout, *B.shape, seed=5).run(probe, pool=True, partial=True)
        assert plain.ksplit > 1
    msg = _launch(probe, B, dst.t, pdst.t if pool else None, carry, cd.t if targets else None,
                  cpd.t if targets else None, expect_rc=E_INVALID, partial=partial, dt_arg=dt_arg)
    assert "carr" in msg, msg
    torch.cuda.synchronize()
    for gbuf in (dst, pdst, cd, cpd):       # refused before anything was launched
        assert bool((gbuf.raw == SENTINEL).all())


def test_pooled_target_goes_with_the_fused_pool(probe):
    _, B = _pair(SMALL, "bf16", "plain", seed=5)
    s, ps = _shapes(B)
    dst, cd, cpd = (Guarded(x, "bf16") for x in (s, s, ps))
    msg = _launch(probe, B, dst.t, None, (0, 0, 12, 20, 8), cd.t, cpd.t, expect_rc=E_INVALID)
    assert "pooled" in msg, msg
    _, B = _pair(SMALL, "bf16", "pool", seed=5)
    pdst = Guarded(ps, "bf16")
    msg = _launch(probe, B, dst.t, pdst.t, (0, 0, 12, 20, 8), cd.t, None, expect_rc=E_INVALID)
    assert "pooled" in msg, msg
