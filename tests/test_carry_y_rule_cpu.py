"""The plane-and-row rule of the y carry on the host: inference._carry_rows_schedule's links replayed by
carry_y_ref.walk over whole plans -- every (plane, row) of every batch's first-level skip tensor is written, by the
batch itself where it computes it and else by a predecessor that computes it, away from any zero padding, and
nothing that reaches a stored value reads a plane inc.0 skipped -- and carry_plan's y successors against brute
force."""
import pytest

from aind_exaspim_neuron_segmentation_amd import inference
import carry_y_ref as Y
import window_fuzz_cases as W

# (volume, patch, overlap, batch size)
PLANS = {
    "bench": ((1024, 1024, 1024), (96, 96, 96), (32, 32, 32), 16),
    "64^3, 2 x 2 x 2": ((96, 96, 96), (64, 64, 64), (32, 32, 32), 2),
    "64^3, 3 x 3 x 3 rows of 3": ((128, 128, 128), (64, 64, 64), (32, 32, 32), 3),
    "ragged high faces": ((150, 141, 170), (64, 64, 64), (32, 32, 32), 5),
    "y chain cut": ((128, 112, 96), (64, 64, 64), (32, 48, 32), 2),         # y stride 16: takes [8, 40), would pass on [24, 56)
    "z chain cut": ((112, 128, 96), (48, 64, 64), (32, 32, 32), 2),         # z stride 16 under a depth of 48
    "both cut": ((112, 112, 96), (48, 64, 64), (32, 48, 32), 2),
    "links that skip batches": ((128, 160, 160), (64, 64, 64), (32, 32, 32), 2),     # rows of 4 in batches of 2
    "two rows per batch": ((128, 128, 96), (64, 64, 64), (32, 32, 32), 4),           # no row batches: nothing carried
    "no whole y tile": ((128, 72, 96), (64, 32, 64), (32, 8, 32), 2),
}


@pytest.mark.parametrize("name", list(PLANS))
def test_every_plane_and_row_is_written_by_a_batch_that_computes_it(name):
    shape, patch, overlap, batch = PLANS[name]
    p = Y.plan(shape, patch, overlap, batch)
    written, problems = Y.walk(p, patch)
    assert not problems, problems[:5]
    n_y = sum(l is not None for l in p["ylinks"])
    n_d = sum(l is not None and l[3] is not None for l in p["ylinks"])
    print(name, "batches", p["n"], "z links", sum(l is not None for l in p["links"]), "y links", n_y, "diagonal", n_d,
          "sets", p["peak"], "+", p["more"])
    if name == "bench":
        assert (n_y, n_d) == (240, 225) and (p["peak"], p["more"]) == (17, 1)      # (20 + 1 on three streams)
        assert Y.plan(shape, patch, overlap, batch, n_streams=3)["more"] == 1
        assert all(l is None or l[1:3] == (64, (8, 24)) for l in p["ylinks"])
    if name in ("64^3, 2 x 2 x 2", "64^3, 3 x 3 x 3 rows of 3", "ragged high faces", "links that skip batches"):
        assert n_y > 0 and n_d > 0
        assert all(l is None or l[2] == (8, 24) for l in p["ylinks"])
    if name in ("y chain cut", "both cut"):
        # every second batch along y computes everything and starts a new chain
        assert n_y > 0 and all(l is None or l[2] == (8, 40) for l in p["ylinks"])
        taken = {l[0] for l in p["ylinks"] if l is not None}
        assert not any(l is not None and bi in taken for bi, l in enumerate(p["ylinks"]))
    if name in ("two rows per batch", "no whole y tile"):
        assert n_y == 0
    # the sets that live longer for the rows are counted on top of the z links' and budgeted apart from them
    if n_y:
        assert p["need"] == p["peak"] + p["more"] and p["budgeted"] == p["ylinks"] and 0 <= p["more"] <= 2
    else:
        assert p["need"] is None and p["budgeted"] is None and p["more"] == 0


def test_the_walk_sees_a_missing_diagonal():
    shape, patch, overlap, batch = PLANS["64^3, 2 x 2 x 2"]
    p = Y.plan(shape, patch, overlap, batch)
    assert not Y.walk(p, patch)[1]
    p["ylinks"] = [l and l[:3] + (None,) for l in p["ylinks"]]
    problems = Y.walk(p, patch)[1]
    assert any("nobody wrote" in s for s in problems), problems


@pytest.mark.parametrize("case", W.cases(), ids=W.case_id)
def test_the_window_fuzz_cases_obey_the_rule(case):
    p = Y.plan(case["shape"], case["patch"], case["overlap"], case["batch"])
    assert not Y.walk(p, case["patch"])[1]


def test_switch_and_budget(monkeypatch):
    shape, patch, overlap, batch = PLANS["64^3, 3 x 3 x 3 rows of 3"]
    on = Y.plan(shape, patch, overlap, batch)
    assert on["level1"] and 0 < on["more"] <= 2        # the pool grows by at most two sets
    monkeypatch.setattr(inference, "ROWS_CARRY_Y", False)
    off = Y.plan(shape, patch, overlap, batch)
    # the z links, their sets and the second level do not depend on the switch
    assert (off["links"], off["peak"], off["level1"]) == (on["links"], on["peak"], on["level1"])
    assert not any(off["ylinks"]) and off["need"] is None and off["budgeted"] is None and off["more"] == 0
    monkeypatch.undo()
    starts = on["starts"]
    model = Y._RowModel()
    pair = 2 * sum(model.carry_pair_elems((batch,) + patch))
    triple = 2 * sum(model.carry_triple_elems((batch,) + patch))
    args = (model, on["links"], on["peak"], True, starts, batch, patch, overlap, 1, None)
    total = on["peak"] + on["more"]
    # a pool that holds the z links' sets and not one more: the rows go, exactly at the bound they stay
    monkeypatch.setattr(inference, "CARRY_POOL_BYTES", total * (pair + triple) - 1)
    assert inference._carry_rows_budget(*args, free=1 << 60) == (None, 0)
    monkeypatch.setattr(inference, "CARRY_POOL_BYTES", total * (pair + triple))
    assert inference._carry_rows_budget(*args, free=1 << 60) == (on["ylinks"], on["more"])
    assert inference._carry_rows_budget(*args, free=2 * total * (pair + triple) - 2) == (None, 0)     # half of the free memory
    # without the second level a set is a pair
    monkeypatch.setattr(inference, "CARRY_POOL_BYTES", total * pair)
    assert inference._carry_rows_budget(*args[:3], False, *args[4:], free=1 << 60) == (on["ylinks"], on["more"])
    monkeypatch.undo()
    # three streams: the spares are in peak already
    p3 = Y.plan(shape, patch, overlap, batch, n_streams=3)
    assert (p3["peak"], p3["more"]) == (on["peak"] + 3, on["more"])


def _brute_force_y(starts, batch, patch, overlap):
    batches = [starts[i:i + batch] for i in range(0, len(starts), batch)]
    succ = []
    for bi, b in enumerate(batches):
        stride = inference.batch_row_stride(b, patch, overlap)
        best = None
        for bj in range(bi + 1, len(batches)):
            c = batches[bj]
            if stride <= 0 or len(c) != len(b) or inference.batch_row_stride(c, patch, overlap) != stride:
                continue
            dy = int(c[0][1]) - int(b[0][1])
            same = all(int(s[0]) == int(t[0]) and int(s[2]) == int(t[2]) and int(t[1]) - int(s[1]) == dy
                       for s, t in zip(b, c))
            if same and 0 < dy < patch[1] and (best is None or dy < best[0]):
                best = (dy, bj)
        succ.append(best and best[1])
    return succ


@pytest.mark.parametrize("name", list(PLANS))
def test_y_successors_against_brute_force(name):
    shape, patch, overlap, batch = PLANS[name]
    starts = list(inference.generate_patch_starts((1, 1) + tuple(shape), patch, overlap))
    assert inference.carry_plan(starts, batch, patch, overlap, axis=1) == _brute_force_y(starts, batch, patch, overlap)
    # (the z successors are test_carry_plan_cpu.py's)
    assert inference.carry_plan(starts, batch, patch, overlap, axis=0) == inference.carry_plan(starts, batch, patch, overlap)


def test_rows_span_is_the_brute_force_rule():
    for h in range(16, 161, 16):
        for shift in range(0, h + 4, 2):
            assert inference._carry_rows_span(h, shift) == Y.rows_span(h, shift), (h, shift)
    assert inference._carry_rows_span(96, 64) == (8, 24)
