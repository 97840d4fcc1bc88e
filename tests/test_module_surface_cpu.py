"""
The module surface after the label post-processing moved out of inference.py into segmentation.py:
every moved name is still reachable as inference.NAME and is the same object, what the tests rebind
on inference is still defined there, and segmentation does not pull inference in.
"""

import os
import subprocess
import sys

import pytest

from aind_exaspim_neuron_segmentation_amd import inference, segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MOVED = [
    # functions
    "affinities_to_components", "_components_on_device",
    "watershed_fragments", "_watershed_on_device",
    "region_graph", "_region_graph_device", "_default_edge_capacity",
    "agglomerate",
    "premerge_region_graph", "_premerge_on_device", "_premerged_table",
    "agglomerate_affinities",
    "affinities_to_components_streaming", "agglomerate_affinities_streaming",
    # classes
    "ComponentsStream", "RegionGraphStream",
    # constants
    "DEFAULT_EDGE_CAPACITY", "DEFAULT_ID_CAPACITY", "MAX_TOTAL_COUNT",
]
STAYED_FUNCTIONS = ["predict_components_streaming", "predict_agglomerate_streaming", "export_half"]
STAYED_SWITCHES = ["PINNED_SLOT_BYTES", "CARRY_Z", "CARRY_Z1", "CARRY_POOL_BYTES", "CLIP_TO_VOLUME", "PLAIN_GATHER",
                   "FULL_PATCHES"]


@pytest.mark.parametrize("name", MOVED)
def test_moved_name_is_the_same_object_under_inference(name):
    assert getattr(inference, name) is getattr(segmentation, name)
    moved = getattr(segmentation, name)
    if callable(moved):
        assert moved.__module__.endswith(".segmentation"), moved.__module__


@pytest.mark.parametrize("name", STAYED_FUNCTIONS)
def test_function_is_still_defined_in_inference(name):
    fn = getattr(inference, name)
    assert fn.__module__.endswith(".inference"), fn.__module__
    assert not hasattr(segmentation, name)


def test_switches_are_still_inference_globals():
    carry = sorted(n for n in vars(inference) if n.startswith("CARRY_"))
    assert carry == ["CARRY_POOL_BYTES", "CARRY_Z", "CARRY_Z1"]
    for name in STAYED_SWITCHES:
        assert name in vars(inference), name
        assert not hasattr(segmentation, name), name      # moved code reads none of them
    # the drivers that stayed read PINNED_SLOT_BYTES from inference's own globals, which a test rebinds
    assert inference._label_predicted_slabs.__globals__ is vars(inference)
    assert "PINNED_SLOT_BYTES" in inference._label_predicted_slabs.__code__.co_names


def test_segmentation_does_not_import_inference():
    code = ("import sys; import aind_exaspim_neuron_segmentation_amd.segmentation as s; "
            "assert callable(s.agglomerate_affinities); "
            "print(int('aind_exaspim_neuron_segmentation_amd.inference' in sys.modules))")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip() == "0", run.stdout
