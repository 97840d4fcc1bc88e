"""
The surface of the seeded fields, teasar_branches_fix_branching, skeletonize and the reference's archive and
voxel helpers, without a GPU, in the manner of test_teasar_surface_cpu.py: the names under inference and
segmentation are the same objects, the signatures, the two entry points declared in the header and bound in
_native with matching argument counts, the ABI version stays 5, header, README and docstrings say what this is
and is not, every argument check fires before any device or library is asked for, and the host-only helpers on a
hand-made dict.
"""

import inspect
import os
import re
import zipfile

import numpy as np
import pytest
import torch

from aind_exaspim_neuron_segmentation_amd import _native, inference, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["exaspim_geodesic_reseed", "exaspim_geodesic_parents_begin_seeds"]
NAMES = ["geodesic_field_seeded", "geodesic_parents_seeded", "teasar_branches_fix_branching", "skeletonize",
         "skeletons_to_zipped_swcs", "segmentation_to_zipped_swcs", "voxelize_skeletons",
         "_geodesic_seeded_on_device", "_fix_branching_on_device"]


def header():
    return open(os.path.join(ROOT, "include", "exaspim_affinity.h")).read()


@pytest.mark.parametrize("name", NAMES)
def test_name_is_the_same_object_under_inference(name):
    assert getattr(inference, name) is getattr(segmentation, name)
    assert getattr(segmentation, name).__module__.endswith(".segmentation")


def test_the_signatures():
    keyword, empty = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty

    def check(fn, positional, keywords):
        parameters = inspect.signature(fn).parameters
        assert list(parameters) == positional + list(keywords)
        for name in positional:
            assert parameters[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
            assert parameters[name].default is empty
        for name, default in keywords.items():
            assert parameters[name].kind is keyword, name
            assert parameters[name].default is default or parameters[name].default == default, name

    check(segmentation.geodesic_field_seeded, ["labels", "seeds"],
          dict(cost=None, field=None, n_labels=None, sweeps_per_read=32, max_sweeps=None, return_device_tensor=False,
               stats=None))
    check(segmentation.geodesic_parents_seeded, ["labels", "seeds", "field"],
          dict(cost=None, n_labels=None, sweeps_per_read=32, max_sweeps=None, return_hops=False,
               return_device_tensors=False, stats=None))
    check(segmentation.teasar_branches_fix_branching, ["labels", "sources", "dbf", "daf", "cost"],
          dict(scale=empty, const=empty, field=None, parents=None, hops=None, boxes=None, n_labels=None,
               max_paths=None, return_device_tensors=False, stats=None))
    check(segmentation.skeletonize, ["segmentation"],
          dict(fix_branching=True, scale=1.25, const=450.0, pdrf_exponent=4, pdrf_scale=100000.0, fill_holes=True,
               max_paths=None))
    check(segmentation.skeletons_to_zipped_swcs, ["skeleton_dict", "zip_path"], {})
    check(segmentation.segmentation_to_zipped_swcs, ["segmentation", "zip_path"], {})
    check(segmentation.voxelize_skeletons, ["skeleton_dict", "img_shape"], {})


def test_the_older_signatures_stay():
    assert list(inspect.signature(segmentation.geodesic_field).parameters) == [
        "labels", "sources", "cost", "n_labels", "sweeps_per_read", "max_sweeps", "return_farthest",
        "return_device_tensors", "stats"]
    assert list(inspect.signature(segmentation.geodesic_parents).parameters) == [
        "labels", "sources", "field", "cost", "n_labels", "sweeps_per_read", "max_sweeps", "return_hops",
        "return_device_tensors", "stats"]


@pytest.mark.parametrize("name", ["geodesic_field_seeded", "geodesic_parents_seeded", "teasar_branches_fix_branching",
                                  "skeletonize"])
def test_the_docstrings_say_not_kimimaro(name):
    doc = " ".join(getattr(segmentation, name).__doc__.split())
    for phrase in ("inference.py:257-291", "What this is not", "kimimaro", "not claimed"):
        assert phrase in doc, phrase
    if name == "skeletonize":
        assert "not osteoid" in doc and "fix_borders" in doc and "soma_*" in doc


def test_the_older_docstrings_point_to_the_new_functions():
    assert "teasar_branches_fix_branching" in segmentation.teasar_branches.__doc__
    assert "teasar_branches_fix_branching" in segmentation.skeletonize_labels.__doc__


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_and_bound(name):
    text = header()
    assert re.search(r"^int " + name + r"\(", text, re.M), name
    assert name in _native.SIGNATURES
    restype, argtypes = _native.SIGNATURES[name]
    declaration = re.search(r"^int " + name + r"\((.*?)\);", text, re.M | re.S).group(1)
    declaration = re.sub(r"/\*.*?\*/", "", declaration, flags=re.S)
    assert len(argtypes) == len(declaration.split(",")), (name, declaration)
    assert restype is _native._i32
    assert getattr(_native.lib(), name) is not None


def test_the_abi_version_stays():
    assert int(re.search(r"#define\s+EXASPIM_ABI_VERSION\s+(\d+)", header()).group(1)) == 5
    assert _native.lib().exaspim_abi_version() == 5


def test_the_header_states_the_definition():
    text = header()
    section = text[text.index("fields and hops seeded from a list"):text.index("TEASAR's loop: targets, branches")]
    section = " ".join(section.replace("\n *", " ").split())
    for phrase in ("inference.py:257-291", "fix_branching", "duplicates allowed", "multi-source float32 heap Dijkstra",
                   "own cost is never read", "bit for bit", "upper bound", "monotonicity", "not claimed",
                   "nothing allocated, nothing synchronised", "no output is touched", "may be NULL if n_seeds is 0"):
        assert phrase in section, phrase


def test_the_readme_no_longer_lists_them_as_out_of_scope():
    text = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    for name in ("teasar_branches_fix_branching", "geodesic_field_seeded", "skeletons_to_zipped_swcs",
                 "voxelize_skeletons"):
        assert name in text, name


@pytest.fixture
def no_device(monkeypatch):
    """Any question to the device fails the test: the refusals below come first."""

    def asked(*a, **kw):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(torch.cuda, "is_available", asked)
    monkeypatch.setattr(_native, "lib", asked)


SHAPE = (3, 4, 5)


def test_the_seeded_fields_refuse_before_any_device_is_asked_for(no_device):
    labels = np.ones(SHAPE, dtype=np.int32)
    seeds = np.array([0, 7, 7], dtype=np.int32)
    volume = np.ones(SHAPE, dtype=np.float32)
    field_fn = segmentation.geodesic_field_seeded

    def parents_fn(labels, seeds, **kw):
        kw.setdefault("field", volume)
        return segmentation.geodesic_parents_seeded(labels, seeds, kw.pop("field"), **kw)

    for fn in (field_fn, parents_fn):
        for dtype in (np.int64, np.uint32, np.float32, bool):
            with pytest.raises(TypeError, match="labels must be int32"):
                fn(labels.astype(dtype), seeds)
            with pytest.raises(TypeError, match="seeds must be int32"):
                fn(labels, seeds.astype(dtype))
        for name in ("cost", "field"):
            with pytest.raises(TypeError, match=f"{name} must be float32"):
                fn(labels, seeds, **{name: volume.astype(np.float64)})
            for bad in (volume[0], volume[:, :3], volume.reshape(5, 4, 3)):
                with pytest.raises(ValueError, match=f"{name} must have the labels' shape"):
                    fn(labels, seeds, **{name: bad})
        for bad in (seeds[None], np.int32(3)):
            with pytest.raises(ValueError, match=r"seeds must be \(S,\)"):
                fn(labels, np.asarray(bad))
        for bad in (labels[0], labels[None]):
            with pytest.raises(ValueError, match=r"\(D, H, W\)"):
                fn(bad, seeds, field=np.ones(bad.shape, dtype=np.float32))
        with pytest.raises(ValueError, match="empty"):
            fn(labels[:, :0], seeds, field=volume[:, :0])
        for bad in (1.0, "3", True):
            with pytest.raises(TypeError, match="sweeps_per_read must be an integer"):
                fn(labels, seeds, sweeps_per_read=bad)
            with pytest.raises(TypeError, match="n_labels must be an integer"):
                fn(labels, seeds, n_labels=bad)
        with pytest.raises(ValueError, match="sweeps_per_read must be at least 1"):
            fn(labels, seeds, sweeps_per_read=0)
        with pytest.raises(ValueError, match="max_sweeps must not be negative"):
            fn(labels, seeds, max_sweeps=-1)
        with pytest.raises(ValueError, match="n_labels"):
            fn(labels, seeds, n_labels=-1)
        # tensors: refused before the library is loaded
        with pytest.raises(TypeError, match="seeds must be int32"):
            fn(torch.from_numpy(labels), torch.from_numpy(seeds).long())
        with pytest.raises(ValueError, match="cost must have the labels' shape"):
            fn(torch.from_numpy(labels), torch.from_numpy(seeds), cost=torch.from_numpy(volume)[:, :, :4])
    with pytest.raises(TypeError, match="field must be a torch tensor or a numpy array"):
        segmentation.geodesic_parents_seeded(labels, seeds, None)
    with pytest.raises(RuntimeError, match="geodesic_field_seeded .* no CPU path"):
        field_fn(torch.from_numpy(labels), torch.from_numpy(seeds))
    with pytest.raises(RuntimeError, match="geodesic_parents_seeded .* no CPU path"):
        parents_fn(torch.from_numpy(labels), torch.from_numpy(seeds), field=torch.from_numpy(volume))


def loop_arguments(make=np.asarray):
    return dict(labels=make(np.ones(SHAPE, dtype=np.int32)), sources=make(np.array([-1, 0], dtype=np.int32)),
                dbf=make(np.ones(SHAPE, dtype=np.int32)), daf=make(np.ones(SHAPE, dtype=np.float32)),
                cost=make(np.ones(SHAPE, dtype=np.float32)))


def loop_call(args, **kw):
    keywords = dict(scale=1.25, const=2.0)
    keywords.update(kw)
    return segmentation.teasar_branches_fix_branching(
        *(args[k] for k in ("labels", "sources", "dbf", "daf", "cost")), **keywords)


def test_the_loop_refuses_before_any_device_is_asked_for(no_device):
    good = loop_arguments()
    ints, floats = np.zeros(SHAPE, dtype=np.int32), np.zeros(SHAPE, dtype=np.float32)
    for name in ("labels", "sources", "dbf"):
        with pytest.raises(TypeError, match=f"{name} must be int32"):
            loop_call(dict(good, **{name: good[name].astype(np.int64)}))
    for name in ("daf", "cost"):
        with pytest.raises(TypeError, match=f"{name} must be float32"):
            loop_call(dict(good, **{name: good[name].astype(np.float64)}))
        with pytest.raises(ValueError, match=f"{name} must have the labels' shape"):
            loop_call(dict(good, **{name: good[name][:, :3]}))
    for name in ("parents", "hops"):
        with pytest.raises(TypeError, match=f"{name} must be int32"):
            loop_call(good, **{name: floats})
        with pytest.raises(ValueError, match=f"{name} must have the labels' shape"):
            loop_call(good, **{name: ints[0]})
    with pytest.raises(TypeError, match="field must be float32"):
        loop_call(good, field=ints)
    with pytest.raises(ValueError, match="field must have the labels' shape"):
        loop_call(good, field=floats[:, :, :2])
    with pytest.raises(ValueError, match=r"sources must be \(K \+ 1,\)"):
        loop_call(dict(good, sources=good["sources"][:0]))
    with pytest.raises(ValueError, match=r"boxes must be \(2, 6\)"):
        loop_call(good, boxes=np.zeros((3, 6), dtype=np.int32))
    for name in ("scale", "const"):
        with pytest.raises(TypeError, match=f"{name} must be a real number"):
            loop_call(good, **{name: "1"})
        for bad in (-1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match=f"{name} must be finite and not negative"):
                loop_call(good, **{name: bad})
    with pytest.raises(TypeError):      # scale and const have no defaults here
        segmentation.teasar_branches_fix_branching(*good.values())
    with pytest.raises(TypeError, match="max_paths must be an integer"):
        loop_call(good, max_paths=1.0)
    with pytest.raises(ValueError, match="max_paths must be at least 1"):
        loop_call(good, max_paths=0)
    with pytest.raises(ValueError, match=r"n_labels \+ 1 = 3"):
        loop_call(good, n_labels=2)
    tensors = loop_arguments(torch.from_numpy)
    with pytest.raises(TypeError, match="cost must be float32"):
        loop_call(dict(tensors, cost=tensors["cost"].double()))
    with pytest.raises(ValueError, match="field must have the labels' shape"):
        loop_call(tensors, field=torch.from_numpy(floats)[:, :, :4])
    with pytest.raises(RuntimeError, match="teasar_branches_fix_branching .* no CPU path"):
        loop_call(tensors)


def test_skeletonize_refuses_before_any_device_is_asked_for(no_device, tmp_path):
    fn = segmentation.skeletonize
    good = np.ones(SHAPE, dtype=np.int32)
    for bad in (1, 0, "True", None):
        with pytest.raises(TypeError, match="fix_branching must be a bool"):
            fn(good, fix_branching=bad)
    for fix in (True, False):
        with pytest.raises(TypeError, match="labels must be int32"):
            fn(good.astype(np.int64), fix_branching=fix)
        with pytest.raises(ValueError, match=r"\(D, H, W\)"):
            fn(good[0], fix_branching=fix)
        with pytest.raises(TypeError, match="pdrf_exponent must be an integer"):
            fn(good, fix_branching=fix, pdrf_exponent=4.0)
        with pytest.raises(ValueError, match="const must be finite and not negative"):
            fn(good, fix_branching=fix, const=-1.0)
        with pytest.raises(ValueError, match="max_paths must be at least 1"):
            fn(good, fix_branching=fix, max_paths=0)
        with pytest.raises(RuntimeError, match="skeletonize .* no CPU path"):
            fn(torch.from_numpy(good), fix_branching=fix)
    path = tmp_path / "never.zip"
    with pytest.raises(TypeError, match="labels must be int32"):
        segmentation.segmentation_to_zipped_swcs(good.astype(np.int64), path)
    assert not path.exists()


def test_without_a_hip_device_the_upload_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    labels, seeds = np.ones(SHAPE, dtype=np.int32), np.zeros(1, dtype=np.int32)
    with pytest.raises(RuntimeError, match="geodesic_field_seeded .* no HIP device"):
        segmentation.geodesic_field_seeded(labels, seeds)
    with pytest.raises(RuntimeError, match="geodesic_parents_seeded .* no HIP device"):
        segmentation.geodesic_parents_seeded(labels, seeds, np.zeros(SHAPE, dtype=np.float32))
    with pytest.raises(RuntimeError, match="teasar_branches_fix_branching .* no HIP device"):
        loop_call(loop_arguments())
    with pytest.raises(RuntimeError, match="skeletonize .* no HIP device"):
        segmentation.skeletonize(labels)


def hand_made():
    #  label 3:  0 -- 1 -- 2        label 12: one vertex
    #                 |
    #                 3
    tree = (np.array([[1, 2, 3], [1, 2, 4], [1, 2, 5], [2, 2, 4]], dtype=np.int32),
            np.array([-1, 0, 1, 1], dtype=np.int32), np.array([1.0, 1.5, 2.0, 0.0], dtype=np.float32))
    dot = (np.array([[0, 0, 0]], dtype=np.int32), np.array([-1], dtype=np.int32), np.array([3.0], dtype=np.float32))
    return {3: tree, 12: dot}


def test_the_zip_writer_on_a_hand_made_dict(tmp_path):
    path = tmp_path / "skeletons.zip"
    path.write_bytes(b"something that is no archive and is overwritten")
    skeletons = hand_made()
    segmentation.skeletons_to_zipped_swcs(skeletons, str(path))
    with zipfile.ZipFile(path) as archive:
        assert archive.namelist() == ["3.swc", "12.swc"]
        for label, skeleton in skeletons.items():
            assert archive.read(f"{label}.swc").decode() == segmentation.skeleton_to_swc(*skeleton)
        assert archive.read("3.swc").decode().splitlines()[3] == "4 0 2 2 4 0 2"
    segmentation.skeletons_to_zipped_swcs({12: skeletons[12]}, path)      # a path object, and overwritten again
    with zipfile.ZipFile(path) as archive:
        assert archive.namelist() == ["12.swc"]
    segmentation.skeletons_to_zipped_swcs({}, path)
    with zipfile.ZipFile(path) as archive:
        assert archive.namelist() == []
    # a skeleton that cannot be written leaves the archive as it was
    broken = {3: (skeletons[3][0], np.array([-1, 0, 1, 9], dtype=np.int32), skeletons[3][2])}
    segmentation.skeletons_to_zipped_swcs({12: skeletons[12]}, path)
    with pytest.raises(ValueError, match="neither -1 nor a row"):
        segmentation.skeletons_to_zipped_swcs(broken, path)
    with zipfile.ZipFile(path) as archive:
        assert archive.namelist() == ["12.swc"]


def test_voxelize_skeletons_on_a_hand_made_dict():
    skeletons = hand_made()
    img = segmentation.voxelize_skeletons(skeletons, (3, 4, 6))
    assert img.shape == (3, 4, 6) and img.dtype == np.zeros(1, dtype=int).dtype
    want = np.zeros((3, 4, 6), dtype=int)
    for z, y, x in skeletons[3][0]:
        want[z, y, x] = 3
    want[0, 0, 0] = 12
    np.testing.assert_array_equal(img, want)

    class WithVertices:      # what the reference's dict holds: objects with a "vertices" attribute
        vertices = np.array([[2.0, 3.0, 5.0]])

    img = segmentation.voxelize_skeletons({7: WithVertices()}, [3, 4, 6])
    assert img[2, 3, 5] == 7 and img.sum() == 7
    assert not segmentation.voxelize_skeletons({}, (1, 1, 1)).any()
    for bad in ([[3, 0, 0]], [[0, 4, 0]], [[0, 0, 6]], [[-1, 0, 0]], [[0, 0, -6]]):
        with pytest.raises(ValueError, match="outside the volume"):
            segmentation.voxelize_skeletons({1: (np.array(bad), None, None)}, (3, 4, 6))
    with pytest.raises(ValueError, match=r"must be \(n, 3\)"):
        segmentation.voxelize_skeletons({1: (np.zeros((2, 2), dtype=int), None, None)}, (3, 4, 6))
    for bad in ((3, 4), (3, 0, 6), (3, 4, 6, 1)):
        with pytest.raises(ValueError, match="img_shape"):
            segmentation.voxelize_skeletons(skeletons, bad)
