"""
Every refusal of the label post-processing functions, without a GPU, held to a record.

For every public function of segmentation.py from fill_holes to skeletonize_pieces the case list below
holds a call whose arguments are all valid (volumes are (3, 4, 5)) and, for every argument, every way it
can be wrong: a wrong Python type, a wrong dtype as an array and as a CPU tensor, a wrong rank, a wrong
shape, empty, a bool where an integer is wanted, negative, zero where one is the least, non-finite, None
where it is not allowed. Each such violation is a case of its own; every pair of violations on two
different arguments of one call is a case; and so is the all-valid call, once with arrays and once with
CPU tensors. Where an optional argument may be None, or a list may be empty, that form is a case as well
("ok:" in its tag), so that the messages that depend on it ("K + 1" without n_labels) are reached.

Each case runs with torch.cuda.is_available and _native.lib patched to raise, so a call that passes every
check ends in that AssertionError, which is an outcome like any other. The outcome of a case is the
exception's type and its whole message.

tests/refusals_cpu.json is the record: the outcomes of all cases, written by

    python tests/test_refusals_cpu.py --record

on the commit before the argument checks were unified, committed unchanged, and compared byte for byte
here. A pair's outcome is stored as "a" or "b" where it is that of its first or second violation alone, and
as an index into the messages otherwise (a message that quotes the other wrong argument, such as the
labels' shape, or the "K + 1" that sources get without n_labels).
"""

import itertools
import json
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aind_exaspim_neuron_segmentation_amd import _native, segmentation  # noqa: E402

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "refusals_cpu.json")
SHAPE = (3, 4, 5)
ROWS = 3            # K + 1 with n_labels = 2


def _both(array):
    """A value as a numpy array and as a CPU tensor."""
    return array, torch.from_numpy(array.copy())


def _array_cases(valid, other_dtypes, shapes):
    """The violations of an array argument: (tag, value) with arrays and CPU tensors of wrong dtype and shape."""
    out = [("type", valid.tolist()), ("none", None)]
    for dtype in other_dtypes:
        a, t = _both(valid.astype(dtype))
        out += [(f"dtype-{np.dtype(dtype)}", a), (f"dtype-{np.dtype(dtype)}-tensor", t)]
    for tag, shape in shapes:
        a, t = _both(np.ones(shape, dtype=valid.dtype))
        out += [(tag, a), (tag + "-tensor", t)]
    return out


def _volume(dtype):
    valid = np.ones(SHAPE, dtype=dtype)
    other = (np.int64, np.float32) if dtype == np.int32 else (np.float64, np.int32)
    return valid, _array_cases(valid, other, (("rank-2", SHAPE[1:]), ("rank-4", (1,) + SHAPE), ("shape", (3, 4, 6)),
                                              ("empty", (3, 0, 5))))


def _labels():
    valid, cases = _volume(np.int32)
    cases = [c for c in cases if not c[0].startswith("shape")]      # any (D, H, W) is a valid labels volume
    return valid, cases + [("cpu-tensor", torch.from_numpy(valid.copy()))]


def _table():
    valid = np.array([-1, 0, 1], dtype=np.int32)
    return valid, _array_cases(valid, (np.int64, np.float32), (("rank-2", (1, ROWS)), ("rank-0", ()),
                                                               ("shape", (ROWS + 1,)), ("empty", (0,))))


def _boxes():
    valid = np.zeros((ROWS, 6), dtype=np.int32)
    cases = _array_cases(valid, (np.int64, np.float32), (("rank-1", (6,)), ("shape-rows", (ROWS + 1, 6)),
                                                         ("shape-columns", (ROWS, 5)), ("empty", (0, 6))))
    return valid, [c for c in cases if c[0] != "none"] + [("ok:none", None)]


def _list():
    """seeds and targets: (S,) with S >= 0."""
    valid = np.array([0, 7], dtype=np.int32)
    cases = _array_cases(valid, (np.int64, np.float32), (("rank-2", (1, 2)), ("rank-0", ())))
    return valid, cases + [("ok:empty", np.zeros(0, dtype=np.int32)),
                           ("ok:empty-tensor", torch.zeros(0, dtype=torch.int32))]


def _pair(none_ok):
    a = np.array([1, 2], dtype=np.int32)
    t = torch.from_numpy(a.copy())
    cases = [("type", a), ("length", (a, a, a)), ("list", [a, a]), ("element-type", (a, a.tolist())),
             ("element-none", (None, a)), ("element-dtype", (a.astype(np.int64), a)),
             ("element-dtype-tensor", (a, t.to(torch.int64))), ("element-float", (a, a.astype(np.float32))),
             ("element-rank", (a[None], a)), ("element-rank-tensor", (t, t[None])), ("lengths", (a, a[:1])),
             ("ok:empty", (a[:0], a[:0])), ("ok:tensors", (t, t)), ("ok:none" if none_ok else "none", None)]
    return (a, a.copy()), cases


def _integer(valid, least, none_ok, most=None):
    cases = [("type-float", 2.5), ("type-str", "2"), ("bool", True), ("numpy-bool", np.bool_(True)),
             ("negative", -1), ("ok:numpy", np.int64(valid))]
    if least >= 1:
        cases.append(("zero", 0))
    if most is not None:
        cases.append(("most", most + 1))
    return valid, cases + [("ok:none" if none_ok else "none", None)]


def _real(valid):
    return valid, [("type-str", "1"), ("bool", True), ("none", None), ("negative", -1.0), ("nan", float("nan")),
                   ("inf", float("inf")), ("numpy-nan", np.float32("nan")), ("ok:int", 2)]


def _flag():
    return True, [("type-int", 1), ("type-str", "yes"), ("none", None), ("ok:numpy", np.bool_(False))]


def _swc_vertices():
    valid = np.arange(6, dtype=np.int32).reshape(2, 3)
    return valid, [("none", None), ("rank-1", valid[0]), ("columns", valid[:, :2]), ("rows", valid[:1]),
                   ("ok:float", valid.astype(np.float32)), ("ok:list", valid.tolist())]


def _swc_parent():
    valid = np.array([-1, 0], dtype=np.int32)
    return valid, [("none", None), ("rank-2", valid[None]), ("rows", valid[:1]), ("float", valid.astype(np.float32)),
                   ("below", np.array([-2, 0])), ("above", np.array([-1, 2])), ("ok:list", [-1, 0])]


def _swc_radius():
    valid = np.array([1.0, 2.0], dtype=np.float32)
    return valid, [("none", None), ("rank-2", valid[None]), ("rows", valid[:1]), ("ok:int", np.array([1, 2]))]


LABELS, I32, F32, TABLE, BOXES, LIST = _labels, lambda: _volume(np.int32), lambda: _volume(np.float32), _table, \
    _boxes, _list


def _optional(kind):
    """An array argument that may be None."""
    def build():
        valid, cases = kind()
        return valid, [c for c in cases if c[0] != "none"] + [("ok:none", None)]
    return build


N_LABELS = lambda: _integer(2, 0, True)                              # noqa: E731
N_LABELS_PIECES = lambda: _integer(2, 0, True, most=2**31 - 1)       # noqa: E731
SWEEPS_PER_READ = lambda: _integer(4, 1, False)                      # noqa: E731
MAX_SWEEPS = lambda: _integer(9, 0, True)                            # noqa: E731
MAX_PATHS = lambda: _integer(3, 1, True)                             # noqa: E731
DUST = lambda: _integer(5, 0, False)                                 # noqa: E731
EXPONENT = lambda: _integer(4, 0, False)                             # noqa: E731
REAL = lambda: _real(1.5)                                            # noqa: E731

_GEODESIC = [("cost", _optional(F32)), ("n_labels", N_LABELS), ("sweeps_per_read", SWEEPS_PER_READ),
             ("max_sweeps", MAX_SWEEPS)]
_TEASAR = [("scale", REAL), ("const", REAL), ("boxes", BOXES), ("n_labels", N_LABELS), ("max_paths", MAX_PATHS)]
_FIX_BRANCHING = [("scale", REAL), ("const", REAL), ("field", _optional(F32)), ("parents", _optional(I32)),
                  ("hops", _optional(I32)), ("boxes", BOXES), ("n_labels", N_LABELS), ("max_paths", MAX_PATHS)]
_CHAIN = [("scale", REAL), ("const", REAL), ("pdrf_exponent", EXPONENT), ("pdrf_scale", REAL),
          ("max_paths", MAX_PATHS)]

# name -> (positional arguments, keyword arguments), each a list of (argument, kind)
FUNCTIONS = {
    "fill_holes": ([("labels", LABELS)], []),
    "distance_to_boundary": ([("labels", LABELS)], []),
    "segment_table": ([("labels", LABELS), ("dbf", _optional(I32))], [("n_labels", N_LABELS)]),
    "border_targets": ([("labels", LABELS)], [("n_labels", N_LABELS)]),
    "label_pieces": ([("labels", LABELS)], [("n_labels", N_LABELS_PIECES), ("dust_threshold", DUST)]),
    "geodesic_field": ([("labels", LABELS), ("sources", TABLE)], _GEODESIC),
    "geodesic_parents": ([("labels", LABELS), ("sources", TABLE)], [("field", _optional(F32))] + _GEODESIC),
    "trace_paths": ([("parents", LABELS), ("hops", I32), ("targets", LIST)], []),
    "teasar_branches": ([("labels", LABELS), ("sources", TABLE), ("dbf", I32), ("daf", F32), ("parents", I32),
                         ("hops", I32)], _TEASAR),
    "teasar_branches_given": ([("labels", LABELS), ("sources", TABLE), ("dbf", I32), ("daf", F32), ("parents", I32),
                               ("hops", I32), ("targets_before", lambda: _pair(True))], _TEASAR),
    "skeletonize_labels": ([("labels", LABELS)], _CHAIN),
    "skeleton_to_swc": ([("vertices", _swc_vertices), ("parent", _swc_parent), ("radius", _swc_radius)], []),
    "geodesic_field_seeded": ([("labels", LABELS), ("seeds", LIST)], [("field", _optional(F32))] + _GEODESIC),
    "geodesic_parents_seeded": ([("labels", LABELS), ("seeds", LIST), ("field", F32)], _GEODESIC),
    "teasar_branches_fix_branching": ([("labels", LABELS), ("sources", TABLE), ("dbf", I32), ("daf", F32),
                                       ("cost", _optional(F32))], _FIX_BRANCHING),
    "teasar_branches_fix_branching_given": ([("labels", LABELS), ("sources", TABLE), ("dbf", I32), ("daf", F32),
                                             ("cost", _optional(F32)), ("targets_before", lambda: _pair(True))],
                                            _FIX_BRANCHING),
    "skeletonize": ([("segmentation", LABELS)], [("fix_branching", _flag)] + _CHAIN),
    "skeletonize_fix_borders": ([("segmentation", LABELS)],
                                [("fix_borders", _flag), ("fix_branching", _flag)] + _CHAIN),
    "skeletonize_pieces": ([("segmentation", LABELS)],
                           [("dust_threshold", DUST), ("fix_borders", _flag), ("fix_branching", _flag)] + _CHAIN),
}

def _as_tensor(value):
    if isinstance(value, np.ndarray):
        return torch.from_numpy(value.copy())
    if isinstance(value, tuple):
        return tuple(_as_tensor(v) for v in value)
    return value


def _cases(name):
    """(valid arguments, singles): singles is a list of (tag, argument index, value)."""
    positional, keywords = FUNCTIONS[name]
    valid, singles = [], []
    for at, (argument, kind) in enumerate(positional + keywords):
        good, bad = kind()
        valid.append(good)
        singles += [(f"{argument}:{tag}", at, value) for tag, value in bad]
    return valid, singles


def _outcome(name, arguments):
    positional, keywords = FUNCTIONS[name]
    n = len(positional)
    try:
        getattr(segmentation, name)(*arguments[:n], **{k: v for (k, _), v in zip(keywords, arguments[n:])})
    except Exception as e:      # noqa: BLE001 - the AssertionError of the patched device is an outcome too
        return f"{type(e).__name__}: {e}"
    return "returned"


def _asked(*a, **kw):
    raise AssertionError("a device was asked for")


def _no_device():
    """Any question to the device fails: what tests/test_geodesic_surface_cpu.py's fixture patches."""
    stack = mock.patch.object(torch.cuda, "is_available", _asked)
    return stack, mock.patch.object(_native, "lib", _asked)


def outcomes(name):
    """(the two all-valid outcomes, the singles' tags and outcomes, the pairs' outcomes in itertools' order)."""
    valid, singles = _cases(name)
    a, b = _no_device()
    with a, b:
        whole = [_outcome(name, valid), _outcome(name, [_as_tensor(v) for v in valid])]
        alone = []
        for tag, at, value in singles:
            arguments = list(valid)
            arguments[at] = value
            alone.append((tag, _outcome(name, arguments)))
        pairs = []
        for (_, at_a, value_a), (_, at_b, value_b) in itertools.combinations(singles, 2):
            if at_a == at_b:
                continue
            arguments = list(valid)
            arguments[at_a], arguments[at_b] = value_a, value_b
            pairs.append(_outcome(name, arguments))
    return whole, alone, pairs


def _pair_indices(name):
    _, singles = _cases(name)
    return [(i, j) for (i, a), (j, b) in itertools.combinations(enumerate(singles), 2) if a[1] != b[1]]


def record():
    """Writes the record."""
    messages, index, functions = [], {}, {}

    def number(message):
        if message not in index:
            index[message] = len(messages)
            messages.append(message)
        return index[message]

    for name in FUNCTIONS:
        whole, alone, pairs = outcomes(name)
        entry = {"valid": [number(m) for m in whole], "singles": [[tag, number(m)] for tag, m in alone]}
        coded = ["a" if message == alone[i][1] else "b" if message == alone[j][1] else number(message)
                 for (i, j), message in zip(_pair_indices(name), pairs)]
        # runs of letters as strings, other messages as lists of numbers between them
        entry["pairs"] = [("".join(g) if letters else list(g)) for letters, g in
                          itertools.groupby(coded, lambda c: isinstance(c, str))]
        functions[name] = entry
    with open(RECORD, "w") as f:
        json.dump({"messages": messages, "functions": functions}, f, separators=(",", ":"))
        f.write("\n")


def _decoded(pairs):
    out = []
    for run in pairs:
        out += list(run)
    return out


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(RECORD))


def test_the_record_covers_every_function(recorded):
    public = [n for n, f in vars(segmentation).items()
              if callable(f) and not n.startswith("_") and getattr(f, "__module__", "").endswith(".segmentation")
              and not isinstance(f, type)]
    first, last = public.index("fill_holes"), public.index("skeletonize_pieces")
    assert set(public[first:last + 1]) == set(FUNCTIONS) == set(recorded["functions"])
    assert os.path.getsize(RECORD) < 1 << 20


@pytest.mark.parametrize("name", list(FUNCTIONS))
def test_every_refusal_is_the_recorded_one(name, recorded):
    messages, entry = recorded["messages"], recorded["functions"][name]
    whole, alone, pairs = outcomes(name)
    assert whole == [messages[i] for i in entry["valid"]]
    assert [tag for tag, _ in alone] == [tag for tag, _ in entry["singles"]], "the case list and the record differ"
    wrong = [(tag, got, messages[i]) for (tag, got), (_, i) in zip(alone, entry["singles"]) if got != messages[i]]
    assert not wrong, f"{len(wrong)} single violation(s) differ from the record, the first: {wrong[0]}"
    indices, coded = _pair_indices(name), _decoded(entry["pairs"])
    assert len(indices) == len(pairs) == len(coded)
    wrong = []
    for (i, j), got, code in zip(indices, pairs, coded):
        want = alone[i][1] if code == "a" else alone[j][1] if code == "b" else messages[code]
        if got != want:
            wrong.append((alone[i][0], alone[j][0], got, want))
    assert not wrong, f"{len(wrong)} pair(s) of violations differ from the record, the first: {wrong[0]}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_refusals_cpu.py --record")
    record()
