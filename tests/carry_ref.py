"""Host model of the planes carried along z: the engine's plane-range rules restated by brute
force, and a stand-in for the model with what inference._carry_schedule asks of one. Plain helpers, no device
(test_carry1_plan_cpu.py, test_window_fuzz_cases_cpu.py, test_gpu_window_fuzz.py)."""


def _level0_span(d, shift):
    """exaspim_unet_carry_planes' rule: whole inc.3 tiles (6 planes where they divide d, else 4) with even bounds
    inside [2, d - shift - 2)."""
    if shift <= 0 or shift % 2 or shift >= d:
        return []
    tz = 6 if d % 6 == 0 else 4
    tiles = [t for t in range(0, d, tz) if t >= 2 and t + tz <= d - shift - 2 and t % 2 == 0 and (t + tz) % 2 == 0]
    return tiles if tiles and tiles[-1] + tz + shift <= 254 else []


def _brute_force(tz, d, shift):
    """The level-1 planes of the later frame that are whole tz-plane tiles inside [3, d/2 - shift/2 - 3): down1.3
    is clear of both frames' zero padding there. None unless the first level carries, the shift is even and so
    is the level-1 shift (a pooled plane of one frame is a pooled plane of the other)."""
    if not _level0_span(d, shift) or shift % 2 or (shift // 2) % 2:
        return (0, 0)
    d1, s1 = d // 2, shift // 2
    tiles = [t for t in range(0, d1, tz) if all(3 <= z < d1 - s1 - 3 for z in range(t, t + tz))]
    if not tiles:
        return (0, 0)
    assert tiles == list(range(tiles[0], tiles[-1] + tz, tz))
    return (tiles[0], tiles[-1] + tz)


class _Model:
    """What _carry_schedule asks of a model, with the engine's plane ranges for 16-bit row batches. c0p, c1p: the
    stored (padded to 32) widths of the first two levels, by default the full-width network's. A level 0 of whole
    64-cout slices has no row mode, hence nothing to carry; the second level carries only on 64-cout slices."""

    def __init__(self, level1=True, c0p=32, c1p=64):
        assert c0p % 32 == 0 and c1p % 32 == 0
        self.level1, self.c0p, self.c1p = level1, c0p, c1p

    def carry_planes(self, shape, row_stride, shift_z, device=None):
        tiles = _level0_span(shape[1], shift_z) if row_stride > 0 and self.c0p % 64 != 0 else []
        tz = 6 if shape[1] % 6 == 0 else 4
        return (tiles[0], tiles[-1] + tz) if tiles else (0, 0)

    def carry1_planes(self, shape, row_stride, shift_z, device=None):
        if not self.level1 or self.c1p % 64 != 0 or self.carry_planes(shape, row_stride, shift_z) == (0, 0):
            return (0, 0)
        return _brute_force(4, shape[1], shift_z)

    def carry_pair_elems(self, shape):
        n, d, h, w = shape
        return n * d * h * w * self.c0p, n * (d // 2) * (h // 2) * (w // 2) * self.c0p

    def carry_triple_elems(self, shape):
        n, d, h, w = shape
        full = n * (d // 2) * (h // 2) * (w // 2) * self.c1p
        return full, full, full // 8


def row_mode(n, w, row_stride):
    """Does a 16-bit engine whose level 0 is no whole 64-cout slice (the full-width network's 32) run a batch of n
    patches, w wide and row_stride apart along x, in row mode (conv_row_mode_ok for inc.3): at least two patches
    whose overlap is a positive multiple of 32 and at most the stride."""
    o = w - row_stride
    return n >= 2 and row_stride > 0 and o > 0 and o % 32 == 0 and row_stride >= o and w % 16 == 0


class _RowModel(_Model):
    """_Model that also says no where the engine runs no row mode (any geometry, not only row batches whose
    overlap is 32)."""

    def row_mode(self, n, w, row_stride):
        """row_mode for this model's level 0."""
        return self.c0p % 64 != 0 and row_mode(n, w, row_stride)

    def carry_planes(self, shape, row_stride, shift_z, device=None):
        if not self.row_mode(shape[0], shape[3], row_stride):
            return (0, 0)
        return super().carry_planes(shape, row_stride, shift_z)
