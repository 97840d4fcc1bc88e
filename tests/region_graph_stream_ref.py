"""
numpy model of the slab-by-slab region graph (exaspim_region_graph_stream_*), step for step
what the device does, on top of region_graph_ref and components_stream_ref:

  1. per slab [z0, z1): region_graph_ref.region_graph of the slab's ids under the slab's affinities,
     with id_capacity as the largest id that counts -- the z entries of the slab's last plane form no
     edge inside the slab -- added to an accumulator keyed by pairs of PROVISIONAL ids, and its voxel
     counts added to sizes_by_id;
  2. per seam: for every (y, x) the carried id of plane z0 - 1, the id of plane z0 and the carried
     q(channel 0) of plane z0 - 1, under the same rule;
  3. carried from slab to slab: one plane of ids and one plane of q, nothing after the last plane;
  4. finish(table, n_labels): every key through the table, keys with an id beyond the table, an end
     outside 1 .. n_labels or equal ends dropped, equal keys pooled; sizes through the table, what it
     does not hold or maps outside 0 .. n_labels into sizes[0].

    accumulate(labels, aff, cuts, id_capacity)      -> Accumulated
    finish(acc, table, n_labels)                    -> (edges, counts, sums, sizes), dropped, pooled
    fragments_streamed(aff, fragment_threshold, cuts)
        -> (graph of the final fragments, K, Accumulated, dropped, pooled, final labels)
    agglomerate_affinities_streamed(aff, thresholds, min_size, fragment_threshold, slab_depth)
        -> (labels int32, composed table, S, K)
"""

from dataclasses import dataclass

import numpy as np

import components_stream_ref
import region_graph_ref


@dataclass
class Accumulated:
    keys: np.ndarray             # uint64, sorted: (lo << 32) | hi of provisional ids
    counts: np.ndarray           # int64
    sums: np.ndarray             # uint64
    sizes_by_id: np.ndarray      # int64 (id_capacity + 1,)
    seam_contributions: int      # voxel edges across seams that contributed


def _pool(keys, counts, sums):
    uniq, inverse = np.unique(keys, return_inverse=True)
    c = np.zeros(uniq.size, np.int64)
    s = np.zeros(uniq.size, np.uint64)
    np.add.at(c, inverse, counts)
    np.add.at(s, inverse, sums)
    return uniq, c, s


def accumulate(labels, aff, cuts, id_capacity):
    labels = np.asarray(labels)
    aff = np.asarray(aff)
    depth = labels.shape[0]
    assert labels.ndim == 3 and aff.shape == (3,) + labels.shape
    bounds = [0] + [int(c) for c in cuts] + [depth]
    assert all(a < b for a, b in zip(bounds, bounds[1:])), bounds
    keys, counts, sums = [], [], []
    sizes_by_id = np.zeros(id_capacity + 1, np.int64)
    carry_ids = carry_q = None
    seam_contributions = 0
    for z0, z1 in zip(bounds, bounds[1:]):
        ids = labels[z0:z1]
        # the seam above this slab
        if carry_ids is not None:
            a, b = carry_ids.astype(np.int64), ids[0].astype(np.int64)
            m = (a > 0) & (b > 0) & (a != b) & (a <= id_capacity) & (b <= id_capacity)
            keys.append(((np.minimum(a, b)[m] << 32) | np.maximum(a, b)[m]).astype(np.uint64))
            counts.append(np.ones(int(m.sum()), np.int64))
            sums.append(carry_q[m])
            seam_contributions += int(m.sum())
        # the slab on its own
        edges, c, s, sizes = region_graph_ref.region_graph(ids, aff[:, z0:z1], id_capacity)
        keys.append(((edges[:, 0].astype(np.int64) << 32) | edges[:, 1].astype(np.int64)).astype(np.uint64))
        counts.append(c)
        sums.append(s)
        sizes_by_id += sizes
        # what the next seam needs; the volume's last plane carries nothing
        if z1 < depth:
            carry_ids, carry_q = ids[-1].copy(), region_graph_ref.quantise(aff[0, z1 - 1])
        else:
            carry_ids = carry_q = None
    k, c, s = _pool(np.concatenate(keys), np.concatenate(counts), np.concatenate(sums))
    return Accumulated(k, c, s, sizes_by_id, seam_contributions)


def finish(acc, table, n_labels):
    table = np.asarray(table).astype(np.int64)
    a, b = (acc.keys >> np.uint64(32)).astype(np.int64), (acc.keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    inside = (a < table.size) & (b < table.size)
    la = np.where(inside, table[np.minimum(a, table.size - 1)], 0)
    lb = np.where(inside, table[np.minimum(b, table.size - 1)], 0)
    keep = inside & (la >= 1) & (lb >= 1) & (la <= n_labels) & (lb <= n_labels) & (la != lb)
    final = ((np.minimum(la, lb)[keep] << 32) | np.maximum(la, lb)[keep]).astype(np.uint64)
    uniq, counts, sums = _pool(final, acc.counts[keep], acc.sums[keep])
    edges = np.stack([uniq >> np.uint64(32), uniq & np.uint64(0xFFFFFFFF)], axis=1).astype(np.int32).reshape(-1, 2)
    sizes = np.zeros(n_labels + 1, np.int64)
    ids = np.arange(acc.sizes_by_id.size)
    to = np.where(ids < table.size, table[np.minimum(ids, table.size - 1)], 0)
    to = np.where((to < 0) | (to > n_labels), 0, to)
    np.add.at(sizes, to, acc.sizes_by_id)
    dropped = int((~keep).sum())
    pooled = int(keep.sum()) - uniq.size
    return (edges, counts, sums, sizes), dropped, pooled


def fragments_streamed(aff, fragment_threshold, cuts):
    final, k, provisional, table = components_stream_ref.components_streamed(aff, fragment_threshold, 0, cuts)
    acc = accumulate(provisional, aff, cuts, table.size - 1)
    graph, dropped, pooled = finish(acc, table, k)
    return graph, k, acc, dropped, pooled, final


def agglomerate_affinities_streamed(aff, agglomeration_thresholds=(0.6, 0.8, 0.9), min_segment_size=100,
                                    fragment_threshold=0.5, slab_depth=8):
    thresholds = list(agglomeration_thresholds)
    cuts = list(range(slab_depth, aff.shape[1], slab_depth))
    _, k, provisional, fragment_table = components_stream_ref.components_streamed(aff, fragment_threshold, 0, cuts)
    acc = accumulate(provisional, aff, cuts, fragment_table.size - 1)
    (edges, counts, sums, sizes), _, _ = finish(acc, fragment_table, k)
    segment_table, s = region_graph_ref.agglomerate(edges, counts, sums, sizes, thresholds[-1], min_segment_size)
    composed = segment_table[fragment_table]
    return composed[provisional], composed, s, k
