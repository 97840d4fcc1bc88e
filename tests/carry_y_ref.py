"""Host model of the plane-and-row rule: which (plane, row) of a batch's first-level skip tensor is
written by which batch when planes are carried along z and rows along y, replayed by brute force over a whole
plan. Plain helpers, no device (test_carry_y_rule_cpu.py).

A batch is z slab k, y row j of the window. With planes Zc carried in along z and rows Yc along y it computes
exactly {z not in Zc} x {y not in Yc} in inc.3's row launch (the interior columns) and {z not in Zc} x every row in
the border launch (the four border columns: only the row launch takes rows over). It stores again only what it
computes:
  * z successor: planes Zo x the rows it computes, both launches, at plane - shift_z;
  * y successor: rows Yo x the planes it computes, row launch only, at row - shift_y;
  * diagonal successor: Zo x Yo, row launch only, at both shifts.
inc.0 leaves planes [Zc0 + 1, Zc1 - 1) of inc.3's source unwritten."""

import numpy as np

from aind_exaspim_neuron_segmentation_amd import inference
from carry_ref import _RowModel


def rows_span(h, shift):
    """exaspim_unet_carry_rows by brute force: the 8-row tiles of the later frame whose rows all lie inside
    [2, h - shift - 2)."""
    if shift <= 0 or shift % 2 or shift >= h:
        return (0, 0)
    tiles = [t for t in range(0, h, 8) if all(2 <= y < h - shift - 2 for y in range(t, t + 8))]
    if not tiles:
        return (0, 0)
    assert tiles == list(range(tiles[0], tiles[-1] + 8, 8))
    return (tiles[0], tiles[-1] + 8)


def plan(shape, patch, overlap, batch, model=None, n_streams=1):
    model = _RowModel() if model is None else model
    starts = list(inference.generate_patch_starts((1, 1) + tuple(shape), patch, overlap))
    succ = inference.carry_plan(starts, batch, patch, overlap)
    links, peak, level1 = inference._carry_schedule(model, succ, starts, batch, patch, overlap, n_streams, None,
                                                    free=1 << 60)
    n = -(-len(starts) // batch)
    links = links or [None] * n
    ylinks, need = inference._carry_rows_schedule(links, starts, batch, patch, overlap)
    budgeted, more = (None, 0)
    if any(links):
        budgeted, more = inference._carry_rows_budget(model, links, peak, level1, starts, batch, patch, overlap,
                                                      n_streams, None, free=1 << 60)
    return dict(starts=starts, links=links, ylinks=ylinks, peak=peak, need=need, n=n, level1=level1, more=more,
                budgeted=budgeted)


def _sel(size, lo, hi):
    s = np.zeros(size, dtype=bool)
    s[lo:hi] = True
    return s


def walk(p, patch):
    """Replays a plan. Returns (written, problems): per batch and launch ("main": the row launch's columns,
    "border": the border launch's) a (d, h) array counting the batches that wrote each (plane, row) of the batch's
    skip tensor, and a list of everything that breaks the rule."""
    d, h = int(patch[0]), int(patch[1])
    n, links, ylinks = p["n"], p["links"], p["ylinks"]
    in_z, in_y = {}, {}
    for bi in range(n):
        if links[bi] is not None:
            in_z[links[bi][0]] = links[bi][2]
        if ylinks[bi] is not None:
            in_y[ylinks[bi][0]] = ylinks[bi][2]
    written = {b: {"main": np.zeros((d, h), dtype=np.int32), "border": np.zeros((d, h), dtype=np.int32)} for b in range(n)}
    problems = []

    def computed(b, launch):
        z0, z1 = in_z.get(b, (0, 0))
        y0, y1 = in_y.get(b, (0, 0)) if launch == "main" else (0, 0)
        return (~_sel(d, z0, z1))[:, None] & (~_sel(h, y0, y1))[None, :]

    def store(src, dst, launch, planes, rows, sz, sy, what):
        """src stores (planes x rows) of what it computes in `launch` into dst's buffers at the shifts."""
        if dst <= src:
            problems.append(f"batch {src} stores into batch {dst}, which does not run later ({what})")
        block = _sel(d, *planes)[:, None] & _sel(h, *rows)[None, :]
        # the range along a shifted axis must be planes (rows) the launch computes: it stores nothing else again
        own = computed(src, launch)
        if (sz and not own.any(axis=1)[planes[0]:planes[1]].all()) or (sy and not own.any(axis=0)[rows[0]:rows[1]].all()):
            problems.append(f"batch {src} is asked to pass on ({what}) planes {planes} x rows {rows} it does not compute")
        block &= own
        zs, ys = np.nonzero(block)
        # away from either frame's zero padding, or the bits would not be the successor's own
        ok = (zs >= 2) & (zs < d - 2) & (zs - sz >= 2) if sz else np.ones(len(zs), dtype=bool)
        ok &= (ys >= 2) & (ys < h - 2) & (ys - sy >= 2) if sy else True
        if not ok.all():
            problems.append(f"batch {src} passes on ({what}) voxels that see a zero padding")
        if ((zs - sz) < 0).any() or ((ys - sy) < 0).any():
            problems.append(f"batch {src} stores ({what}) before the start of the target")
            return
        np.add.at(written[dst][launch], (zs - sz, ys - sy), 1)

    for b in range(n):
        takes_part = links[b] is not None or b in in_z
        if not takes_part:
            if b in in_y or ylinks[b] is not None:
                problems.append(f"batch {b} carries rows without a buffer set")
            continue
        for launch in ("main", "border"):
            written[b][launch] += computed(b, launch)
        if links[b] is not None:
            t, sz, span, _ = links[b]
            zo = (span[0] + sz, span[1] + sz)
            for launch in ("main", "border"):
                store(b, t, launch, zo, (0, h), sz, 0, "z")
        if ylinks[b] is not None:
            t, sy, rows, diag = ylinks[b]
            if rows != rows_span(h, sy):
                problems.append(f"batch {b}: rows {rows} are not exaspim_unet_carry_rows' {rows_span(h, sy)}")
            yo = (rows[0] + sy, rows[1] + sy)
            store(b, t, "main", (0, d), yo, 0, sy, "y")
            if diag is not None:
                if links[b] is None:
                    problems.append(f"batch {b}: a diagonal successor without a z successor")
                    continue
                _, sz, span, _ = links[b]
                store(b, diag, "main", (span[0] + sz, span[1] + sz), yo, sz, sy, "diagonal")
    for b in range(n):
        if links[b] is None and b not in in_z:
            continue
        for launch in ("main", "border"):
            w = written[b][launch]
            if (w == 0).any():
                zs, ys = np.nonzero(w == 0)
                problems.append(f"batch {b} ({launch}): {len(zs)} (plane, row) nobody wrote, first ({zs[0]}, {ys[0]})")
            # a block the batch computes is its own alone; one it takes over has one writer, or two where a
            # predecessor that computes every plane or row covers the diagonal block as well
            if (w[computed(b, launch)] != 1).any():
                problems.append(f"batch {b} ({launch}): a predecessor wrote into what the batch computes itself")
            if (w > 2).any():
                problems.append(f"batch {b} ({launch}): a (plane, row) written by three batches")
        # inc.0: nothing that reaches a stored value reads a plane it skipped
        z0, z1 = in_z.get(b, (0, 0))
        skipped = _sel(d, z0 + 1, z1 - 1) if z1 - z0 > 2 else _sel(d, 0, 0)
        for launch in ("main", "border"):
            zs = np.nonzero(computed(b, launch).any(axis=1))[0]
            reads = np.unique(np.clip(np.concatenate([zs - 1, zs, zs + 1]), 0, d - 1))
            if skipped[reads].any():
                problems.append(f"batch {b} ({launch}) reads a plane of its source that inc.0 skipped")
    return written, problems
