"""
Deterministic synthetic data for tests, golden fixtures and the benchmark.

Nothing here depends on torch's or numpy's RNG streams: every value is a pure
function of (seed, key, index) through the splitmix64 finaliser, so the build
container, the GPU box and the device-side generator
(``exaspim_synth_volume_u16`` in ``csrc/prepost.hip``) all produce identical
data.

* Volumes: ``uint16`` voxel = ``splitmix64(seed + global_linear_index) % 2000``
  (SURVEY.md section 8(d) "Synthetic input"); after the reference's brightness
  clip at 1000 this gives p1 = 19, p99.9 = 1000.
* Weights: one value stream per ``state_dict`` key (SURVEY.md section 8(d)
  "Synthetic weights"): conv W, b ~ U(+-1/sqrt(fan_in)); BatchNorm gamma ~
  U(0.5, 1.5), beta, running_mean ~ U(-0.2, 0.2), running_var ~ U(0.05, 0.55).
  Non-trivial running statistics matter: a freshly initialised BatchNorm is
  the identity and would hide BN-folding bugs.
"""

import zlib

import numpy as np

from aind_exaspim_neuron_segmentation_amd.machine_learning.spec import (
    unet_layer_specs,
)

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def splitmix64(x):
    """
    Applies the splitmix64 output function to an array of uint64 counters.

    Parameters
    ----------
    x : numpy.ndarray
        Array of dtype uint64.

    Returns
    -------
    numpy.ndarray
        Hashed values, dtype uint64.
    """
    with np.errstate(over="ignore"):
        z = x + _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def synth_volume(shape, seed=0, origin=(0, 0, 0), global_shape=None):
    """
    Generates (a sub-block of) the synthetic uint16 volume.

    Parameters
    ----------
    shape : Tuple[int]
        Shape (D, H, W) of the block to generate.
    seed : int, optional
        Seed added to the global linear voxel index. Default is 0.
    origin : Tuple[int], optional
        Global coordinate of the block's first voxel. Default is (0, 0, 0).
    global_shape : Tuple[int], optional
        Shape of the whole volume the block is cut from. Default is "shape".

    Returns
    -------
    numpy.ndarray
        Block of dtype uint16 with values in [0, 2000).
    """
    gshape = tuple(global_shape) if global_shape is not None else tuple(shape)
    z = np.arange(origin[0], origin[0] + shape[0], dtype=np.uint64)
    y = np.arange(origin[1], origin[1] + shape[1], dtype=np.uint64)
    x = np.arange(origin[2], origin[2] + shape[2], dtype=np.uint64)
    lin = (
        z[:, None, None] * np.uint64(gshape[1]) + y[None, :, None]
    ) * np.uint64(gshape[2]) + x[None, None, :]
    h = splitmix64(lin + np.uint64(seed))
    return (h % np.uint64(2000)).astype(np.uint16)


_MASK64 = (1 << 64) - 1

# ---- neurite-like volume: frozen constants (golden g9 depends on every one of them) ----
NEURITE_FLOOR_BASE = 8        # noise floor = base + splitmix64(seed + linear index) % mod
NEURITE_FLOOR_MOD = 32
NEURITE_FLOOR_MAX = NEURITE_FLOOR_BASE + NEURITE_FLOOR_MOD - 1
NEURITE_CELL_SHIFT = 5        # 32^3 cells
NEURITE_NODE_MARGIN = 4       # node offset inside its cell: 4 + (byte % 24), per axis
NEURITE_NODE_SPAN = 24
NEURITE_SALT = 0x6E65757269746573
NEURITE_PEAK_BASE = 100       # peak = base + (b^3 >> 14), b = a byte of splitmix64(h): 100 .. 1112


def _splitmix64_int(x):
    """splitmix64 of one Python int (the scalar twin of "splitmix64")."""
    z = (x + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def _neurite_cell(cz, cy, cx, seed):
    """
    Node and outgoing edges of one cell: (node, edges) with node = global
    (z, y, x) and edges[a] = (radius, peak) or None for the edge towards the
    next cell along axis a.
    """
    key = (cz << 42) | (cy << 21) | cx
    h = _splitmix64_int(key ^ _splitmix64_int((seed & _MASK64) ^ NEURITE_SALT))
    node = tuple(
        (c << NEURITE_CELL_SHIFT) + NEURITE_NODE_MARGIN
        + ((h >> (8 * a)) & 0xFF) % NEURITE_NODE_SPAN
        for a, c in enumerate((cz, cy, cx))
    )
    h2 = _splitmix64_int(h)
    edges = []
    for a in range(3):
        e = (h >> (24 + 8 * a)) & 0xFF
        if (e & 7) < 3:
            radius = 1 + (e >> 3) % 3
            b = (h2 >> (8 * a)) & 0xFF
            peak = NEURITE_PEAK_BASE + ((b * b * b) >> 14)
            edges.append((radius, peak))
        else:
            edges.append(None)
    return node, edges


def synth_neurite_volume(shape, seed=0, origin=(0, 0, 0), global_shape=None):
    """
    Generates (a sub-block of) the neurite-like synthetic uint16 volume: sparse
    bright tubes on a dim noise floor. Integer arithmetic only; the device twin
    is ``exaspim_synth_volume_neurite_u16`` (``csrc/prepost.hip``), same bits.

    Definition (frozen: golden g9 is made from it). With g = global (z, y, x):

    * floor(g) = 8 + splitmix64(seed + global linear index) % 32      (8 .. 39)
    * cells: c = g >> 5 per axis. h(c) = splitmix64(key ^ splitmix64(seed ^
      0x6E65757269746573)), key = cz << 42 | cy << 21 | cx. It does not depend
      on the volume's shape.
    * node(c)[a] = 32 * c[a] + 4 + (byte a of h) % 24, a = 0 (z), 1 (y), 2 (x).
    * edge of c towards c + e_a: e = byte 3 + a of h; present iff (e & 7) < 3;
      radius r = 1 + (e >> 3) % 3; peak = 100 + (b^3 >> 14) with b = byte a of
      splitmix64(h): 100 .. 1112, most tubes dim, about 4 % above the default clip.
      It is the segment A = node(c), B = node(c + e_a).
    * a voxel p tests the three edges leaving its cell and the three arriving
      from the cell before it on each axis (none from index -1). With
      d = B - A, w = p - A, dd = d.d, t = clamp(w.d, 0, dd),
      n = |w * dd - d * t|^2: core iff n <= r^2 dd^2 (value peak), halo iff
      n <= (r + 1)^2 dd^2 (value peak // 2), else 0. Every quantity < 2^40.
    * voxel = min(65535, floor + max over the edges).

    Nodes keep 4 voxels from the cell faces, so a tube with its halo lies
    inside the two cells it joins and no other cell's edge can reach a voxel.

    Parameters
    ----------
    shape : Tuple[int]
        Shape (D, H, W) of the block to generate.
    seed : int, optional
        Seed of the floor and of the cell hashes. Default is 0.
    origin : Tuple[int], optional
        Global coordinate of the block's first voxel. Default is (0, 0, 0).
    global_shape : Tuple[int], optional
        Shape of the whole volume the block is cut from. Default is "shape".

    Returns
    -------
    numpy.ndarray
        Block of dtype uint16.
    """
    gshape = tuple(global_shape) if global_shape is not None else tuple(shape)
    lo = [int(o) for o in origin]
    hi = [int(o) + int(s) for o, s in zip(origin, shape)]
    ax = [np.arange(lo[a], hi[a], dtype=np.uint64) for a in range(3)]
    lin = (
        ax[0][:, None, None] * np.uint64(gshape[1]) + ax[1][None, :, None]
    ) * np.uint64(gshape[2]) + ax[2][None, None, :]
    with np.errstate(over="ignore"):
        h = splitmix64(lin + np.uint64(seed & _MASK64))
    out = (h % np.uint64(NEURITE_FLOOR_MOD)).astype(np.int64) + NEURITE_FLOOR_BASE

    cells = {}

    def cell(c):
        if c not in cells:
            cells[c] = _neurite_cell(c[0], c[1], c[2], seed)
        return cells[c]

    sh = NEURITE_CELL_SHIFT
    for cz in range(lo[0] >> sh, ((hi[0] - 1) >> sh) + 1):
        for cy in range(lo[1] >> sh, ((hi[1] - 1) >> sh) + 1):
            for cx in range(lo[2] >> sh, ((hi[2] - 1) >> sh) + 1):
                c = (cz, cy, cx)
                segments = []
                node, edges = cell(c)
                for a in range(3):
                    nxt = tuple(c[i] + (i == a) for i in range(3))
                    if edges[a] is not None:
                        segments.append((node, cell(nxt)[0]) + edges[a])
                    if c[a] > 0:
                        prv = tuple(c[i] - (i == a) for i in range(3))
                        pnode, pedges = cell(prv)
                        if pedges[a] is not None:
                            segments.append((pnode, node) + pedges[a])
                if not segments:
                    continue
                g0 = [max(lo[a], c[a] << sh) for a in range(3)]
                g1 = [min(hi[a], (c[a] + 1) << sh) for a in range(3)]
                p = [np.arange(g0[a], g1[a], dtype=np.int64) for a in range(3)]
                p = [p[0][:, None, None], p[1][None, :, None], p[2][None, None, :]]
                tube = np.zeros([g1[a] - g0[a] for a in range(3)], dtype=np.int64)
                for A, B, radius, peak in segments:
                    d = [B[a] - A[a] for a in range(3)]
                    w = [p[a] - A[a] for a in range(3)]
                    dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                    t = np.clip(w[0] * d[0] + w[1] * d[1] + w[2] * d[2], 0, dd)
                    n = sum((w[a] * dd - d[a] * t) ** 2 for a in range(3))
                    val = np.where(
                        n <= radius * radius * dd * dd, peak,
                        np.where(n <= (radius + 1) * (radius + 1) * dd * dd, peak // 2, 0),
                    )
                    np.maximum(tube, val, out=tube)
                sl = tuple(slice(g0[a] - lo[a], g1[a] - lo[a]) for a in range(3))
                out[sl] += tube
    return np.minimum(out, 65535).astype(np.uint16)


def _uniform01(key, n, seed):
    """
    Returns n float64 values in [0, 1) from the stream named by (seed, key).
    """
    base = np.uint64(zlib.crc32(key.encode("utf-8"))) << np.uint64(32)
    with np.errstate(over="ignore"):
        offset = base + np.uint64(seed) * _GOLDEN
        h = splitmix64(np.arange(n, dtype=np.uint64) + offset)
    return (h >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def synth_state_dict(output_channels=3, width_multiplier=1, seed=1, trilinear=True):
    """
    Builds a synthetic UNet3D state_dict (numpy arrays) with the reference's
    keys in the reference's order (128 keys; 136 with "trilinear=False").

    Parameters
    ----------
    output_channels : int, optional
        Number of output channels of the head. Default is 3.
    width_multiplier : float, optional
        Channel width factor. Default is 1.
    seed : int, optional
        Seed of the value streams. Default is 1.
    trilinear : bool, optional
        False selects the ConvTranspose3d variant of the Up blocks. Default is
        True.

    Returns
    -------
    Dict[str, numpy.ndarray]
        float32 arrays (int64 scalars for "num_batches_tracked").
    """
    layers, (head_in, head_out) = unet_layer_specs(
        output_channels, trilinear, width_multiplier
    )
    sd = {}

    def uni(key, shape, lo, hi):
        n = int(np.prod(shape))
        u = _uniform01(key, n, seed)
        return (lo + (hi - lo) * u).astype(np.float32).reshape(shape)

    for layer in layers:
        if layer[0] == "conv_transpose":
            _, prefix, cin, cout = layer
            bound = 1.0 / np.sqrt(float(cin))
            sd[f"{prefix}.weight"] = uni(f"{prefix}.weight", (cin, cout, 2, 2, 2), -bound, bound)
            sd[f"{prefix}.bias"] = uni(f"{prefix}.bias", (cout,), -bound, bound)
            continue
        _, prefix, cin, cmid, cout = layer
        for conv_idx, bn_idx, ci, co in ((0, 1, cin, cmid), (3, 4, cmid, cout)):
            bound = 1.0 / np.sqrt(27.0 * ci)
            k = f"{prefix}.{conv_idx}"
            sd[f"{k}.weight"] = uni(f"{k}.weight", (co, ci, 3, 3, 3), -bound, bound)
            sd[f"{k}.bias"] = uni(f"{k}.bias", (co,), -bound, bound)
            k = f"{prefix}.{bn_idx}"
            sd[f"{k}.weight"] = uni(f"{k}.weight", (co,), 0.5, 1.5)
            sd[f"{k}.bias"] = uni(f"{k}.bias", (co,), -0.2, 0.2)
            sd[f"{k}.running_mean"] = uni(f"{k}.running_mean", (co,), -0.2, 0.2)
            sd[f"{k}.running_var"] = uni(f"{k}.running_var", (co,), 0.05, 0.55)
            sd[f"{k}.num_batches_tracked"] = np.array(100, dtype=np.int64)
    bound = 1.0 / np.sqrt(float(head_in))
    sd["outc.conv.weight"] = uni(
        "outc.conv.weight", (head_out, head_in, 1, 1, 1), -bound, bound
    )
    sd["outc.conv.bias"] = uni("outc.conv.bias", (head_out,), -bound, bound)
    return sd
