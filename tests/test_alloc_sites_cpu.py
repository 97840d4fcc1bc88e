"""
tests/poisoned_alloc.py on CPU tensors and arrays, and a scan of the package's source that keeps
tests/test_gpu_poisoned_python.py honest: the poisoned runs see an uninitialised allocation only if it is the
attribute call torch.empty(...) or np.empty(...) / numpy.empty(...), so every other spelling is refused here.
No GPU.
"""

import ast
import pathlib

import numpy as np
import pytest
import torch

import poisoned_alloc
from poisoned_alloc import FILLS, poisoned

PACKAGE = pathlib.Path(__file__).resolve().parent.parent / "aind_exaspim_neuron_segmentation_amd"

TORCH_DTYPES = [torch.uint8, torch.int16, torch.int32, torch.int64, torch.float16, torch.float32]
NUMPY_DTYPES = [np.uint8, np.int16, np.int32, np.int64, np.float16, np.float32]


def all_bytes(t, fill):
    if isinstance(t, torch.Tensor):
        t = t.contiguous().reshape(-1).view(torch.uint8).numpy()
    else:
        t = np.ascontiguousarray(t).reshape(-1).view(np.uint8)
    return bool((t == fill).all())


# ---- 1. the helper ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("dtype", TORCH_DTYPES, ids=str)
def test_torch_empty_is_filled_in_every_call_form(monkeypatch, fill, dtype):
    size = dtype.itemsize
    with poisoned(monkeypatch, fill) as counts:
        made = [
            (torch.empty(7, dtype=dtype), (7,)),                                     # one positional int
            (torch.empty(3, 5, dtype=dtype), (3, 5)),                                # varargs
            (torch.empty((2, 3, 5), dtype=dtype), (2, 3, 5)),                        # a tuple
            (torch.empty([4, 3], dtype=dtype, device="cpu"), (4, 3)),                # a list and a device
            (torch.empty(size=(6,), dtype=dtype, device=torch.device("cpu")), (6,)),  # the keyword
            (torch.empty(torch.Size((2, 2)), dtype=dtype, pin_memory=False), (2, 2)),
        ]
        target = torch.zeros(9, dtype=dtype)
        returned = torch.empty((9,), dtype=dtype, out=target)
        assert returned is target
        made.append((target, (9,)))
        for t, shape in made:
            assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == "cpu" and t.is_contiguous()
            assert all_bytes(t, fill), (shape, dtype)
        assert counts.calls == {"device": 0, "pinned": 0, "host": len(made), "numpy": 0}
        assert counts.bytes["host"] == size * sum(int(np.prod(shape)) for _, shape in made)
        assert counts.bytes["device"] == counts.bytes["pinned"] == counts.bytes["numpy"] == 0
    if fill == 0xFF and dtype.is_floating_point:
        assert torch.isnan(made[0][0]).all()
    if fill == 0x01 and dtype == torch.int32:
        assert (made[0][0] == 16843009).all()
    if fill == 0x7F and dtype == torch.float32:
        assert ((made[0][0] > 3.39e38) & torch.isfinite(made[0][0])).all()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("dtype", NUMPY_DTYPES, ids=lambda d: np.dtype(d).name)
def test_numpy_empty_is_filled_in_every_call_form(monkeypatch, fill, dtype):
    size = np.dtype(dtype).itemsize
    with poisoned(monkeypatch, fill) as counts:
        made = [
            (np.empty(7, dtype), (7,)),                                  # positional dtype
            (np.empty((3, 5), dtype=dtype), (3, 5)),
            (np.empty(shape=(2, 3, 5), dtype=np.dtype(dtype).name), (2, 3, 5)),
            (np.empty([4, 3], dtype=dtype, order="F"), (4, 3)),          # Fortran order: still every byte
            (np.empty((3,) + (2, 2), dtype=dtype, order="C"), (3, 2, 2)),
        ]
        for a, shape in made:
            assert a.shape == shape and a.dtype == np.dtype(dtype) and all_bytes(a, fill), (shape, dtype)
        assert made[3][0].flags.f_contiguous
        assert counts.calls == {"device": 0, "pinned": 0, "host": 0, "numpy": len(made)}
        assert counts.bytes["numpy"] == size * sum(int(np.prod(shape)) for _, shape in made)
        default = np.empty(3)
        assert default.dtype == np.float64 and all_bytes(default, fill) and counts.calls["numpy"] == len(made) + 1


def test_zero_size_and_zero_dim_results_do_not_raise(monkeypatch):
    with poisoned(monkeypatch, 0xFF) as counts:
        assert torch.empty(0, dtype=torch.int32).numel() == 0
        assert tuple(torch.empty((0, 4), dtype=torch.float32).shape) == (0, 4)
        scalar = torch.empty((), dtype=torch.int32)
        assert scalar.dim() == 0 and int(scalar) == -1
        assert torch.empty((), dtype=torch.float16).element_size() == 2
        assert np.empty(0, dtype=np.int32).size == 0 and np.empty((3, 0), dtype=np.float32).shape == (3, 0)
        word = np.empty((), dtype=np.int64)
        assert word.shape == () and int(word) == -1
        assert counts.calls == {"device": 0, "pinned": 0, "host": 4, "numpy": 3}
        assert counts.bytes == {"device": 0, "pinned": 0, "host": 4 + 2, "numpy": 8}
    assert str(counts).startswith("device 0 calls / 0 B, pinned 0 calls")


def test_the_originals_are_back_afterwards_and_a_bad_fill_is_refused(monkeypatch):
    real_torch, real_numpy = torch.empty, np.empty
    with poisoned(monkeypatch, 0x7F):
        assert torch.empty is not real_torch and np.empty is not real_numpy
        with poisoned(monkeypatch, 0x01) as inner:      # nested: the inner fill wins, then the outer one is back
            assert all_bytes(torch.empty(5, dtype=torch.int16), 0x01) and inner.calls["host"] == 1
        assert all_bytes(torch.empty(5, dtype=torch.int16), 0x7F)
    assert torch.empty is real_torch and np.empty is real_numpy
    with pytest.raises(RuntimeError, match="boom"):
        with poisoned(monkeypatch, 0x00):
            raise RuntimeError("boom")
    assert torch.empty is real_torch and np.empty is real_numpy
    for bad in (-1, 256, 1.0, "0xFF"):
        with pytest.raises(ValueError, match="fill must be a byte"):
            with poisoned(monkeypatch, bad):
                pass
    assert poisoned_alloc.FILLS == (0x00, 0xFF, 0x7F, 0x01)


def test_the_package_modules_reach_the_wrappers(monkeypatch):
    """The modules hold `torch` and `np`, not the functions: patching the attribute reaches their sites."""
    from aind_exaspim_neuron_segmentation_amd import inference, segmentation, sharding
    from aind_exaspim_neuron_segmentation_amd.machine_learning import unet3d

    with poisoned(monkeypatch, 0x01) as counts:
        for module in (inference, segmentation, sharding, unet3d):
            assert module.torch.empty is torch.empty and module.np.empty is np.empty
            assert all_bytes(module.torch.empty(3, dtype=torch.int32), 0x01)
            assert all_bytes(module.np.empty(3, dtype=np.int32), 0x01)
        assert counts.calls["host"] == 4 and counts.calls["numpy"] == 4


# ---- 2. the scan -----------------------------------------------------------------------------------------------
TORCH_NAMES = {"torch"}
NUMPY_NAMES = {"np", "numpy"}
# uninitialised memory under any other name than <module>.empty: the wrappers do not see these
FORBIDDEN_ATTRIBUTES = {"empty_like", "new_empty", "empty_strided", "new_empty_strided", "empty_permuted",
                        "empty_quantized", "resize_", "ndarray"}
TENSOR_CONSTRUCTORS = {"Tensor", "FloatTensor", "DoubleTensor", "HalfTensor", "BFloat16Tensor", "ByteTensor",
                       "CharTensor", "ShortTensor", "IntTensor", "LongTensor", "BoolTensor"}


def dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    if isinstance(node, ast.Name):
        parts.append(node.id)
        return ".".join(reversed(parts))
    return None


def scan(source, filename):
    """(line, what) of every allocation of uninitialised memory that the poisoned tests cannot see, and the
    number of torch.empty / np.empty call sites that they can."""
    tree = ast.parse(source, filename)
    found, seen = [], 0
    called = {id(node.func) for node in ast.walk(tree) if isinstance(node, ast.Call)}
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] in ("torch", "numpy"):
            for alias in node.names:
                if alias.name in FORBIDDEN_ATTRIBUTES | TENSOR_CONSTRUCTORS | {"empty", "*"}:
                    found.append((node.lineno, f"from {node.module} import {alias.name}"))
        elif isinstance(node, ast.Import):
            for alias in node.names:
                if alias.name == "torch" and (alias.asname or "torch") not in TORCH_NAMES:      # not torch.nn as nn
                    found.append((node.lineno, f"import {alias.name} as {alias.asname}"))
                if alias.name == "numpy" and (alias.asname or "numpy") not in NUMPY_NAMES:
                    found.append((node.lineno, f"import {alias.name} as {alias.asname}"))
        elif isinstance(node, ast.Attribute):
            name = dotted(node)
            if node.attr in FORBIDDEN_ATTRIBUTES and (node.attr != "ndarray" or id(node) in called):
                found.append((node.lineno, f"{name or '<expression>.' + node.attr}"))      # x.new_empty, np.ndarray(...)
            elif node.attr in TENSOR_CONSTRUCTORS and id(node) in called:
                found.append((node.lineno, f"{name}(...)"))
            elif node.attr == "empty" and name and name.split(".")[0] in TORCH_NAMES | NUMPY_NAMES:
                if id(node) in called and name in ("torch.empty", "np.empty", "numpy.empty"):
                    seen += 1
                else:      # an alias (f = torch.empty), getattr-free partials, torch.cuda.empty...: not a plain call
                    found.append((node.lineno, f"{name} used other than as the call {name}(...)"))
        elif isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "getattr":
            if len(node.args) >= 2 and isinstance(node.args[1], ast.Constant) and node.args[1].value in (
                    FORBIDDEN_ATTRIBUTES | {"empty"}):
                found.append((node.lineno, f"getattr(..., {node.args[1].value!r})"))
    return sorted(found), seen


def test_every_uninitialised_allocation_of_the_package_is_a_plain_empty_call():
    files = sorted(PACKAGE.rglob("*.py"))
    assert len(files) >= 5
    problems, seen = [], {}
    for path in files:
        found, count = scan(path.read_text(), str(path))
        seen[path.name] = count
        problems += [f"{path.relative_to(PACKAGE.parent)}:{line}: {what}" for line, what in found]
    assert not problems, (
        "uninitialised memory that tests/test_gpu_poisoned_python.py cannot see (poisoned_alloc patches the "
        "attributes torch.empty and numpy.empty only; write the allocation as torch.empty(...) or np.empty(...)):\n  "
        + "\n  ".join(problems))
    print(f"plain empty() call sites: {seen}")
    for name in ("segmentation.py", "inference.py", "sharding.py", "unet3d.py"):
        assert seen[name] >= 1, name      # the scan reads the files it is meant to read; the count is not pinned


@pytest.mark.parametrize("line,what", [
    ("x = torch.empty_like(y)", "torch.empty_like"),
    ("x = y.new_empty((3,))", "y.new_empty"),
    ("x = torch.empty_strided((2, 2), (2, 1))", "torch.empty_strided"),
    ("x = torch.Tensor(3, 4)", "torch.Tensor(...)"),
    ("x = torch.FloatTensor(3)", "torch.FloatTensor(...)"),
    ("x = torch.cuda.IntTensor(3)", "torch.cuda.IntTensor(...)"),
    ("x = np.ndarray((3,), dtype=np.int32)", "np.ndarray"),
    ("x = numpy.ndarray((3,))", "numpy.ndarray"),
    ("from torch import empty", "from torch import empty"),
    ("from numpy import empty as e", "from numpy import empty"),
    ("make = torch.empty", "torch.empty used other than as the call"),
    ("make = functools.partial(np.empty, dtype=np.int32)", "np.empty used other than as the call"),
    ("import torch as t", "import torch as t"),
    ("import numpy as xp", "import numpy as xp"),
    ("x = getattr(torch, 'empty')(3)", "getattr(..., 'empty')"),
    ("y.resize_(9)", "y.resize_"),
])
def test_the_scan_refuses(line, what):
    found, seen = scan("import torch\nimport numpy as np\nimport numpy\n" + line + "\n", "<case>")
    assert [w for _, w in found if what in w] and found[0][0] == 4, found
    assert seen == 0


def test_the_scan_accepts_what_the_wrappers_see():
    source = ("import numpy\nimport numpy as np\nimport torch\n"
              "a = torch.empty(3, dtype=torch.int32, device=d)\nb = np.empty((2, 2), dtype=np.int32)\n"
              "c = numpy.empty(shape)\nd = torch.zeros(3)\ne = isinstance(x, np.ndarray)\nf = x.is_empty\n"
              "def g(a: np.ndarray) -> torch.Tensor:\n    return torch.zeros_like(a)\n")
    assert scan(source, "<case>") == ([], 3)
