"""
Poisoned allocations for the Python layer (a plain module, no conftest): poisoned(monkeypatch, fill) replaces
torch.empty and numpy.empty, through pytest's monkeypatch, by wrappers that call the real function with the
caller's arguments unchanged and then overwrite every byte of the result with `fill`. The package reaches both
functions through the module attribute (tests/test_alloc_sites_cpu.py holds it to that), so every workspace,
output, state word, pool buffer and piecewise-filled host result of the wrappers starts as poison, the way the
C ABI's tests start their own buffers.

    with poisoned(monkeypatch, 0xFF) as counts:
        out = inference.fill_holes(labels)
    assert counts.calls["device"] >= 1

A device tensor is filled with fill_ on the current stream, the one the code under test then launches on. The
fills: 0x00 (what fresh pages hold: the baseline), 0xFF (-1 in every integer type, NaN in float32 and half),
0x7F (large positive integers, 3.39e38 in float32, NaN in half) and 0x01 (16843009 in int32: small positive
words that pass for counts, ids and set flags).
"""

import contextlib

import numpy
import torch

FILLS = (0x00, 0xFF, 0x7F, 0x01)
KINDS = ("device", "pinned", "host", "numpy")


class Counts:
    """Calls and bytes per kind of allocation since the context was entered."""

    def __init__(self):
        self.calls = dict.fromkeys(KINDS, 0)
        self.bytes = dict.fromkeys(KINDS, 0)

    def add(self, kind, nbytes):
        self.calls[kind] += 1
        self.bytes[kind] += int(nbytes)

    def __str__(self):
        return ", ".join(f"{kind} {self.calls[kind]} calls / {self.bytes[kind]} B" for kind in KINDS)


def _poison_tensor(t, fill):
    if t.numel():
        t.reshape(-1).view(torch.uint8).fill_(fill)      # torch.empty is contiguous: reshape is a view, 0-dim too


def _poison_array(a, fill):
    if a.size and not a.dtype.hasobject:
        flat = a.reshape(-1, order="A")      # a view for C and for Fortran order
        assert numpy.shares_memory(flat, a)
        flat.view(numpy.uint8)[...] = fill


@contextlib.contextmanager
def poisoned(monkeypatch, fill):
    """torch.empty and numpy.empty return memory whose every byte is `fill`; yields the Counts."""
    if not (isinstance(fill, int) and 0 <= fill <= 0xFF):
        raise ValueError(f"fill must be a byte, got {fill!r}")
    real_torch, real_numpy = torch.empty, numpy.empty
    counts = Counts()

    def torch_empty(*args, **kwargs):
        t = real_torch(*args, **kwargs)
        if isinstance(t, torch.Tensor) and t.layout == torch.strided and not t.is_meta:
            kind = "device" if t.device.type != "cpu" else "pinned" if kwargs.get("pin_memory") else "host"
            _poison_tensor(t, fill)
            counts.add(kind, t.numel() * t.element_size())
        return t

    def numpy_empty(*args, **kwargs):
        a = real_numpy(*args, **kwargs)
        if isinstance(a, numpy.ndarray):
            _poison_array(a, fill)
            counts.add("numpy", a.nbytes)
        return a

    with monkeypatch.context() as patch:
        patch.setattr(torch, "empty", torch_empty)
        patch.setattr(numpy, "empty", numpy_empty)
        yield counts
    assert torch.empty is real_torch and numpy.empty is real_numpy
