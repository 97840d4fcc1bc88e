"""
conv_first_skip_planes (engine.hip): the planes of inc.3's source that inc.0 need not write when inc.3 takes
planes [in_z0, in_z1) over from the forward one z slab up. Held to a brute-force walk over the tiles of the two
launches of the row sequence Main | BordersCarry: the main launch computes the whole tiles outside the range,
the border launch the tiles over [0, in_z0) and [in_z1, d) with the first segment's last tile masked at in_z0,
and a computed plane reads itself and its two neighbours. The ranges are the ones exaspim_unet_carry_planes gives
(engine.hip: carry_span, restated here) for every even shift.
"""

import ctypes

import pytest

import layer_ref as R


@pytest.fixture(scope="module")
def probe():
    import __graft_entry__

    __graft_entry__.build()
    lib = ctypes.CDLL(R.PROBE_PATH)
    i32 = ctypes.c_int32
    lib.probe_conv_first_skip_planes.restype = None
    lib.probe_conv_first_skip_planes.argtypes = [i32, i32, i32, ctypes.POINTER(i32)]
    lib.probe_row_tile_depths.restype = None
    lib.probe_row_tile_depths.argtypes = [i32, ctypes.POINTER(i32)]
    return lib


def _carry_span(d, shift, tz):
    """The whole main-launch tiles inside [2, d - shift - 2), even bounds."""
    step = tz if tz % 2 == 0 else 2 * tz
    lo, hi = -(-2 // step) * step, (d - shift - 2) // step * step
    return (lo, hi) if lo < hi and hi + shift <= 254 else (0, 0)


def _planes_read(d, lo, hi, tz_main, tz_border):
    """Planes that reach a stored value of either launch."""
    computed = set()
    for t in range(-(-d // tz_main)):                       # main launch: whole tiles outside [lo, hi)
        if not (lo <= t * tz_main and (t + 1) * tz_main <= hi):
            computed.update(range(t * tz_main, min((t + 1) * tz_main, d)))
    for seg_lo, seg_hi in ((0, lo), (hi, d)):               # border launch: tiles laid over the two segments
        z = seg_lo
        while z < seg_hi:
            computed.update(range(z, min(z + tz_border, seg_hi)))
            z += tz_border
    read = set()
    for z in computed:
        read.update(p for p in (z - 1, z, z + 1) if 0 <= p < d)
    return computed, read


@pytest.mark.parametrize("d", [32, 48, 96])
def test_skip_range_is_what_no_computed_tile_reads(probe, d):
    depths, out = (ctypes.c_int32 * 2)(), (ctypes.c_int32 * 2)()
    probe.probe_row_tile_depths(d, depths)
    tz_main, tz_border = depths
    assert tz_main == (6 if d % 6 == 0 else 4) and tz_border in (4, 8)
    nonempty = 0
    for shift in range(2, d, 2):
        lo, hi = _carry_span(d, shift, tz_main)
        probe.probe_conv_first_skip_planes(d, lo, hi, out)
        if lo == hi:
            assert tuple(out) == (0, 0), (d, shift)
            continue
        computed, read = _planes_read(d, lo, hi, tz_main, tz_border)
        assert computed == set(range(d)) - set(range(lo, hi)), (d, shift)     # both launches leave the range out
        unread = sorted(set(range(d)) - read)
        if not unread:
            assert tuple(out) == (0, 0), (d, shift)
            continue
        assert unread == list(range(unread[0], unread[-1] + 1)), (d, shift, unread)
        assert tuple(out) == (unread[0], unread[-1] + 1) == (lo + 1, hi - 1), (d, shift, tuple(out), unread)
        nonempty += 1
    assert nonempty >= 3


def test_production_pair_and_empty_ranges(probe):
    out = (ctypes.c_int32 * 2)()
    for (d, lo, hi), want in {(96, 6, 30): (7, 29), (32, 4, 12): (5, 11), (96, 0, 0): (0, 0), (96, 6, 8): (0, 0),
                              (96, 6, 10): (7, 9), (32, 30, 34): (0, 0), (32, -2, 8): (0, 0)}.items():
        probe.probe_conv_first_skip_planes(d, lo, hi, out)
        assert tuple(out) == want, (d, lo, hi)
