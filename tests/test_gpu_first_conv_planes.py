"""
inc.0 with output planes nobody reads (launch_conv_first's [skip_z0, skip_z1), conv_first16_strip_kernel).

The row-strip kernel walks the strips of the planes that are left and stores nothing to the skipped ones; every
plane it does write has the bits of the full launch (which test_gpu_layers.py holds to a float64 reference).
The per-group kernels and float32 ignore the range and write everything. Destinations are pre-filled with 0xA5
between guard bands.
"""

import ctypes

import pytest
import torch

import layer_ref as R
from test_gpu_carry_layers import GUARD, POISON, Guarded
from test_gpu_layers import E_INVALID, _ptr, _uniform_pm, probe as _base_probe  # noqa: F401

pytestmark = pytest.mark.gpu

DTS = ["f16", "bf16"]
# (n, d, h, w): widths 32 .. 128 are 1 .. 4 groups per wave; the last has more strips than the 1024 workgroups
SHAPES = [(2, 12, hh, ww) for ww in (32, 64, 96, 128) for hh in (8, 16)] + [(2, 40, 64, 32)]
PRODUCTION = (1, 96, 8, 96)


class Guarded32(Guarded):
    """Guarded for float32 storage (Guarded sizes its band for the 16-bit types)."""

    def __init__(self, shape, dt, fill):
        nbytes = 4 * int(torch.tensor(shape).prod())
        self.raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
        self.t = self.raw[GUARD:GUARD + nbytes].view(torch.float32).view(shape)
        self.fill = fill


def _ranges(d):
    return [(3, 9), (1, d - 1), (5, 6), (0, 0)]


@pytest.fixture(scope="module")
def probe(_base_probe):  # noqa: F811
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    fn = _base_probe.probe_conv_first_planes
    fn.restype = i32
    fn.argtypes = [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, i32, i32, vp]
    return _base_probe


@pytest.fixture(scope="module")
def full(probe):
    """Operands and the full launch's output per (dt, shape, c0p), computed once."""
    cache = {}

    def get(dt, shape, c0p):
        key = (dt, shape, c0p)
        if key not in cache:
            n, d, h, w = shape
            gen = torch.Generator().manual_seed(n * d * h * w + c0p)
            c0 = c0p - 2
            x = (4 * _uniform_pm(shape, gen, lo=0.0)).to(torch.float32)
            wt = torch.zeros((27, c0p), dtype=torch.float32)
            wt[:, :c0] = (_uniform_pm((27, c0), gen, lo=0.0) / 3).to(torch.float32)
            b = torch.zeros(c0p, dtype=torch.float32)
            b[:c0] = (0.5 * _uniform_pm((c0,), gen, lo=0.0)).to(torch.float32)
            ops = (x.cuda(), wt.cuda(), b.cuda())
            ref, kernel = _run(probe, dt, shape, c0p, ops, (0, 0))
            assert ref.guards_intact()
            # every row of every plane was written (a single value may well have the poison's bits)
            assert not bool((_raw(ref.t) == POISON).all(dim=-1).all(dim=-1).all(dim=-1).any())
            cache[key] = (ops, ref.t.cpu().clone(), kernel)
        return cache[key]

    yield get
    cache.clear()


def _raw(t):
    return R.bits(t).view(torch.uint8).reshape(t.shape + (-1,))


def _run(probe, dt, shape, c0p, ops, skip, per_group=0, expect_rc=0):
    n, d, h, w = shape
    k = R.kc(dt)
    xpad = torch.zeros(n * (d + 2) * (h + 2) * (w + 2), dtype=torch.float32, device="cuda")
    dst = (Guarded32 if dt == "f32" else Guarded)((n, c0p // k, d, h, w, k), dt, POISON)
    probe.probe_reset_config()
    torch.cuda.synchronize()
    rc = probe.probe_conv_first_planes(R.DTYPES[dt], _ptr(ops[0]), _ptr(xpad), _ptr(ops[1]), _ptr(ops[2]), _ptr(dst.t),
                                       n, d, h, w, c0p, R.SLOPE, per_group, skip[0], skip[1], None)
    torch.cuda.synchronize()
    if expect_rc:
        assert rc == expect_rc, rc
        return dst, probe.probe_last_error().decode()
    assert rc == 0, probe.probe_last_error().decode()
    return dst, probe.probe_last_layer_kernel().decode()


def _check_skipped(dst, ref, skip, what):
    lo, hi = skip
    got = dst.t.cpu()
    assert dst.guards_intact(), what
    assert bool((_raw(got)[:, :, lo:hi] == POISON).all()), f"{what}: a skipped plane was written"
    keep = torch.ones(got.shape[2], dtype=torch.bool)
    keep[lo:hi] = False
    diff = R.bits(got)[:, :, keep] != R.bits(ref)[:, :, keep]
    assert not diff.any(), f"{what}: {int(diff.sum())} values of the written planes differ from the full launch"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c0p", [32, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_strip_kernel_leaves_the_skipped_planes_alone(probe, full, dt, c0p, shape):
    ops, ref, kernel = full(dt, shape, c0p)
    assert kernel == "conv_first16_strip"
    for skip in _ranges(shape[1]):
        dst, kernel = _run(probe, dt, shape, c0p, ops, skip)
        assert kernel == "conv_first16_strip", kernel
        _check_skipped(dst, ref, skip, f"skip {skip}")


@pytest.mark.parametrize("dt", DTS)
def test_production_range(probe, full, dt):
    ops, ref, _ = full(dt, PRODUCTION, 32)
    dst, kernel = _run(probe, dt, PRODUCTION, 32, ops, (7, 29))
    assert kernel == "conv_first16_strip", kernel
    _check_skipped(dst, ref, (7, 29), "d 96, skip [7, 29)")


@pytest.mark.parametrize("dt,per_group,kernel", [("f16", 1, "conv_first16_rows"), ("bf16", 1, "conv_first16_rows"),
                                                 ("f32", 0, "conv_first")])
def test_other_variants_write_every_plane(probe, full, dt, per_group, kernel):
    shape = (2, 12, 8, 64)
    if dt == "f32":
        ops = full("f16", shape, 32)[0]
        ref, name = _run(probe, dt, shape, 32, ops, (0, 0))
        ref = ref.t.cpu().clone()
    else:
        ops, ref, _ = full(dt, shape, 32)      # (the per-group kernel has the strip kernel's bits)
    dst, name = _run(probe, dt, shape, 32, ops, (3, 9), per_group=per_group)
    assert name == kernel, name
    assert dst.guards_intact()
    assert torch.equal(R.bits(dst.t.cpu()), R.bits(ref))


@pytest.mark.parametrize("skip", [(-1, 4), (4, 13), (9, 3), (13, 13)])
def test_ranges_outside_the_patch_are_refused(probe, full, skip):
    shape = (2, 12, 8, 64)
    ops, _, _ = full("f16", shape, 32)
    dst, msg = _run(probe, "f16", shape, 32, ops, skip, expect_rc=E_INVALID)
    assert "skipped planes" in msg, msg
    assert bool((dst.raw == POISON).all())      # refused before anything was launched
