"""
Host oracles for label_pieces_open, skeletonize_blocks and join_block_skeletons (no GPU), written from the
definitions in include/exaspim_affinity.h and DESIGN 6r:

grid          the blocks of a volume: along an axis of n voxels with block length b, block i starts at i (b - 1)
              while that is below n - 1 (one block for n = 1) and ends at min(start + b, n); a low face is open iff
              the block is not the first, a high face iff it is not the last; raster order of (iz, iy, ix).
open_pieces   the open rule applied to pieces_ref.flood_fill(..., dust 0): a piece is kept iff it has a voxel on an
              open face or at least dust_threshold voxels; kept pieces renumbered in order of first voxel.
owned_sizes   a piece's voxels outside the block's open high planes.
join          the join of the blocks' trees by graph search, with no union-find: an identified vertex's edges are
              moved to the anchor's, "already in the anchor's component" is a search for the anchor from the vertex.
"""

import collections

import numpy as np

import pieces_ref


def spans(n, b):
    """(start, end) of every block along one axis, from the closed form: ceil((n - 1) / (b - 1)) blocks."""
    assert n >= 1 and b >= 2
    count = max(1, -(-(n - 1) // (b - 1)))
    return [(i * (b - 1), min(i * (b - 1) + b, n)) for i in range(count)]


def grid(shape, block_shape):
    """The blocks in block order: dicts with "lo", "hi" (exclusive) and "open", six bools in face order."""
    axes = [spans(n, b) for n, b in zip(shape, block_shape)]
    blocks = []
    for iz, z in enumerate(axes[0]):
        for iy, y in enumerate(axes[1]):
            for ix, x in enumerate(axes[2]):
                where = ((iz, len(axes[0])), (iy, len(axes[1])), (ix, len(axes[2])))
                faces = []
                for i, count in where:
                    faces += [i > 0, i < count - 1]
                blocks.append(dict(lo=(z[0], y[0], x[0]), hi=(z[1], y[1], x[1]), open=faces))
    return blocks


def face_mask(shape, open_faces):
    """bool volume: the voxels that lie on a face whose entry of open_faces is set."""
    on = np.zeros(shape, dtype=bool)
    for axis in range(3):
        index = [slice(None)] * 3
        if open_faces[2 * axis]:
            index[axis] = 0
            on[tuple(index)] = True
        if open_faces[2 * axis + 1]:
            index[axis] = shape[axis] - 1
            on[tuple(index)] = True
    return on


def faces_of(mask):
    """The six bools of the C call's mask: bit f for face f."""
    return [bool(mask >> f & 1) for f in range(6)]


def open_pieces(labels, k, dust_threshold, open_faces, oracle=pieces_ref.flood_fill):
    """(pieces, piece_label, piece_size, piece_first, piece_open, dust pieces, pieces kept although small)."""
    pieces, piece_label, piece_size, piece_first, _ = oracle(labels, k, 0)
    touched = np.zeros(len(piece_label) + 1, dtype=bool)
    touched[pieces[face_mask(pieces.shape, open_faces)]] = True
    is_open = touched[1:]
    keep = is_open | (piece_size >= dust_threshold)
    number = np.concatenate([[0], np.where(keep, np.cumsum(keep), 0)]).astype(np.int32)
    small = int(np.count_nonzero(is_open & (piece_size < dust_threshold)))
    return (number[pieces], piece_label[keep], piece_size[keep], piece_first[keep], is_open[keep],
            int(np.count_nonzero(~keep)), small)


def owned_sizes(pieces, n_pieces, open_faces):
    high = [False, open_faces[1], False, open_faces[3], False, open_faces[5]]
    mine = np.where(face_mask(pieces.shape, high), 0, pieces)
    return np.bincount(mine.reshape(-1), minlength=n_pieces + 1)[1:].astype(np.int64)


def path_tree(block, piece, label, voxels, owned_size, border_rows, radius=None):
    """A hand-made record: a chain of voxels, row 0 the root, every other row's parent the row before it."""
    n = len(voxels)
    return dict(block=block, piece=piece, label=label, owned_size=owned_size,
                vertices=np.array(voxels, dtype=np.int32).reshape(n, 3),
                parent=np.arange(-1, n - 1, dtype=np.int32),
                radius=np.array(radius if radius is not None else np.ones(n), dtype=np.float32),
                border_rows=np.array(border_rows, dtype=np.int64))


def _reaches(adjacent, start, goal):
    seen, stack = {start}, [start]
    while stack:
        for other in adjacent[stack.pop()]:
            if other == goal:
                return True
            if other not in seen:
                seen.add(other)
                stack.append(other)
    return start == goal


def join(trees, dust_threshold=0):
    """(dict label -> (vertices, parent, radius), joints, skipped joints, dust components)."""
    trees = sorted(trees, key=lambda t: (t["block"], t["piece"]))
    adjacent = collections.defaultdict(set)
    radius = {}
    moved = {}      # an identified vertex -> its anchor
    meeting = collections.defaultdict(list)
    for t, tree in enumerate(trees):
        for row, up in enumerate(tree["parent"]):
            adjacent[(t, row)]      # a lone root is a vertex too
            radius[(t, row)] = float(tree["radius"][row])
            if up >= 0:
                adjacent[(t, row)].add((t, int(up)))
                adjacent[(t, int(up))].add((t, row))
        for row in tree["border_rows"]:
            meeting[(tree["label"],) + tuple(int(c) for c in tree["vertices"][row])].append((t, int(row)))
    joints = skipped = 0
    for where in sorted(meeting):
        nodes = sorted(meeting[where])
        if len({t for t, _ in nodes}) < 2:
            continue
        joints += 1
        anchor = nodes[0]
        for node in nodes[1:]:
            if _reaches(adjacent, node, anchor):
                skipped += 1
                continue
            for other in adjacent.pop(node):
                adjacent[other].discard(node)
                adjacent[other].add(anchor)
                adjacent[anchor].add(other)
            moved[node] = anchor
            radius[anchor] = min(radius[anchor], radius.pop(node))
    out, dust = {}, 0
    towards = {}
    for t, tree in enumerate(trees):
        root = (t, int(np.nonzero(np.asarray(tree["parent"]) == -1)[0][0]))
        if root in moved or root in towards:
            continue
        towards[root] = None
        stack, members = [root], set()
        while stack:
            node = stack.pop()
            members.add(node)
            for other in adjacent[node]:
                if other not in towards:
                    towards[other] = node
                    stack.append(other)
        member_trees = sorted({m for m, _ in members} | {m for (m, _), a in moved.items() if a in members})
        if sum(trees[m]["owned_size"] for m in member_trees) < dust_threshold:
            dust += 1
            continue
        rows = [(m, row) for m in member_trees for row in range(len(trees[m]["parent"])) if (m, row) in members]
        assert len(rows) == len(members)
        at = {node: i for i, node in enumerate(rows)}
        before = out.get(tree["label"])
        start = 0 if before is None else len(before[1])
        part = (np.array([trees[m]["vertices"][row] for m, row in rows], dtype=np.int32).reshape(-1, 3),
                np.array([-1 if towards[node] is None else at[towards[node]] + start for node in rows],
                         dtype=np.int32),
                np.array([radius[node] for node in rows], dtype=np.float32))
        out[tree["label"]] = part if before is None else tuple(np.concatenate(pair) for pair in zip(before, part))
    return out, joints, skipped, dust
