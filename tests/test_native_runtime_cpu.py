"""One HIP runtime per process, whatever is imported first. torch's wheel ships its own libamdhip64 and the
extension links the system's under the same soname: with the extension loaded before torch the process used to map
both, torch's tensors lived in one runtime and the extension's kernels were launched in the other, which reports
"no ROCm-capable device is detected" (build() followed by smoke() in one process did just that). _native.lib()
imports torch first. Needs no device: the loader's choice shows in /proc/self/maps."""

import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = """
import sys
sys.path.insert(0, {root!r})
{first}
{second}
import torch
maps = sorted({{line.split()[-1] for line in open('/proc/self/maps') if 'libamdhip64' in line}})
print('\\n'.join(maps))
"""
EXTENSION = "from aind_exaspim_neuron_segmentation_amd import _native; _native.lib()"


@pytest.mark.parametrize("first,second", [(EXTENSION, "import torch"), ("import torch", EXTENSION),
                                          ("import __graft_entry__ as g; g.build()", "import torch")],
                         ids=["extension first", "torch first", "build() first"])
def test_one_hip_runtime_whatever_is_imported_first(first, second):
    out = subprocess.run([sys.executable, "-c", CODE.format(root=ROOT, first=first, second=second)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    maps = [line for line in out.stdout.splitlines() if "libamdhip64" in line]
    assert len(maps) == 1, f"{len(maps)} HIP runtimes mapped: {maps}"
