"""
test_gpu_window_fuzz.py's ladder of plan switches through predict() on the network variants of variant_models.py,
fp16 and bf16, on two of its hand-written cases: the smallest one, (64, 24, 96) under patches of (32, 16, 64), and
(112, 56, 96) under patches of (48, 32, 64) with a z overlap of 32, whose chain is cut at every second batch.

Rung 0, the plain plan, is held to the variant's fp32 engine within test_gpu_parity.PROB_TOL_16BIT; on the smallest
case that fp32 engine is held once per variant to the CPU oracle's predict() within PROB_TOL_FP32. Every later rung
has rung 0's bits. The ledger of run_prepared calls is held to the host model with the variant's padded level widths
(carry_ref.py; test_variant_window_cases_cpu.py holds the two cases to the traits this needs): width 0.5 has the
first level's links and no call is handed second-level buffers, width 2 carries nothing and every rung is the plain
plan.

predict() stitches 3 channels, or 1 with affinity_mode=False, like the reference, and refuses a network with any
other number (asserted below). The ladder therefore runs "three_quarter" and "half" -- whose 4 and 2 outputs
test_gpu_variant_plans.py covers through the C ABI -- with 3 outputs and otherwise as the table has them: the
planner and the carry buffers depend on the level widths, not on the head.
"""

import numpy as np
import pytest

import test_gpu_window_fuzz as F
import variant_models as V
from aind_exaspim_neuron_segmentation_amd import inference
from aind_exaspim_neuron_segmentation_amd.utils import synthetic
from test_gpu_bf16x3 import dev, make_model, oracle  # noqa: F401  (fixtures)
from test_gpu_parity import PROB_TOL_FP32

pytestmark = pytest.mark.gpu

CASES = V.window_cases()


@pytest.fixture(scope="module")
def state(dev):  # noqa: F811
    s = {}
    yield s
    s.clear()


def _outputs(name):
    """Output channels predict() can stitch: 1 for the foreground model, else 3."""
    return 1 if V.VARIANTS[name]["out"] == 1 else 3


def _model(state, dev, name, dtype):  # noqa: F811
    if ("model", name, dtype) not in state:
        v = V.VARIANTS[name]
        state[("model", name, dtype)] = make_model(dev, out_channels=_outputs(name), seed=v["seed"],
                                                   trilinear=v["trilinear"], wm=v["wm"], compute_dtype=dtype)
    return state[("model", name, dtype)]


def _fp32_reference(state, dev, name, case):  # noqa: F811
    """predict() of the variant's fp32 engine, once per case for both storage types."""
    key = ("fp32", name, case)
    if key not in state:
        c = CASES[case]
        vol = inference.DeviceVolume.from_array(F._volume(c), dev)
        state[key] = inference.predict(vol, _model(state, dev, name, "fp32")[0], n_streams=1,
                                       affinity_mode=_outputs(name) == 3, **F._kw(c))
    return state[key]


@pytest.mark.parametrize("name", V.NAMES)
def test_fp32_engine_against_the_cpu_oracle_on_the_smallest_case(state, dev, oracle, name):  # noqa: F811
    c = CASES["smallest"]
    got = _fp32_reference(state, dev, name, "smallest")
    _, sd = _model(state, dev, name, "fp32")
    kw = {k: v for k, v in F._kw(c).items() if k != "verbose"}
    want = oracle.predict(F._volume(c), oracle.OracleModel(sd), affinity_mode=_outputs(name) == 3, **kw)
    assert got.shape == want.shape and got.dtype == np.float32
    err = float(np.abs(got - want).max())
    print(f"{name}: fp32 engine's predict() vs the CPU oracle's on {c['shape']}: max |diff| = {err:.3e} "
          f"(bound {PROB_TOL_FP32:.0e})")
    assert err < PROB_TOL_FP32, f"{name}: {err:.3e}"


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", V.NAMES)
def test_every_plan_switch_keeps_the_bits_of_the_plain_plan(state, dev, name, case, dtype, monkeypatch):  # noqa: F811
    v = V.VARIANTS[name]
    c = CASES[case]
    model, _ = _model(state, dev, name, dtype)
    reference = _fp32_reference(state, dev, name, case)     # (before any switch is flipped)
    print(name, dtype, c)
    _, ledgers = F._ladder(model, reference, c, dtype, dev, monkeypatch,
                           host_model=lambda level1: V.host_model(name, level1=level1),
                           affinity_mode=_outputs(name) == 3)
    # what the ledger check has already held to the host model, said once more in the variant's own terms
    carried = {rung: [call for call in calls if call is not None] for rung, calls in ledgers.items()}
    if not v["row"]:
        assert set(ledgers) == {5, 6, 7} and not any(carried.values()), "width 2 carried something"
        return
    assert all(any(call["out"] is not None for call in calls) for calls in carried.values()), "no link"
    second = {rung: any(call["own1"] is not None for call in calls) for rung, calls in carried.items()}
    if v["level1"] and case == "cut":
        assert second == {5: False, 6: True, 7: True, 8: False}       # rung 8 ran: a pool for the pairs only
    else:       # no second level (width 0.5), or no whole level-1 tile at a depth of 32
        assert set(ledgers) == {5, 6, 7} and not any(second.values())


@pytest.mark.parametrize("name", ["three_quarter", "half"])
def test_predict_refuses_an_output_count_it_cannot_stitch(state, dev, name):  # noqa: F811
    """2 or 4 outputs: run_sliding_window says so at the first batch, before anything is stitched."""
    model, _ = V.make(make_model, dev, name, "fp16")
    c = CASES["smallest"]
    vol = inference.DeviceVolume.from_array(synthetic.synth_volume(c["shape"], seed=c["seed"]), dev)
    for affinity_mode in (True, False):
        with pytest.raises(RuntimeError, match=f"model produced {model.output_channels} channels"):
            inference.predict(vol, model, affinity_mode=affinity_mode, **F._kw(c))
