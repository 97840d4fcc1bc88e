"""
The two helpers that both inference.py (prediction) and segmentation.py
(labels from affinities) need; this module imports neither of them.
"""

import numpy as np
import torch


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _carrier(block):
    """numpy block -> torch CPU tensor (uint16 rides as int16 bits)."""
    block = np.ascontiguousarray(block)
    if not block.flags.writeable:      # read-only memmap / zarr chunk: torch wants a writable buffer
        block = block.copy()
    if block.dtype == np.uint16:
        block = block.view(np.int16)
    return torch.from_numpy(block)
