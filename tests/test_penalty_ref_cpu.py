"""
tests/penalty_ref.py held to a second formulation of its own, and the float32 torch expression of stage 6 of
skeletonize_labels (segmentation._skeleton_chain_on_device), evaluated on the CPU, held to the oracle within
penalty_ref.bound. tests/test_gpu_penalty.py holds the device's field to the same oracle and bound. No GPU.
"""

import numpy as np
import pytest
import torch

import geodesic_ref as ref
import penalty_ref as pen
import teasar_ref as tref

EXPONENTS = (0, 1, 2, 4, 7)
SCALES = (0.0, 1.0, 1e5, 3e7)


def torch_expression(labels, dbf, daf, k, pdrf_exponent, pdrf_scale, device="cpu"):
    """Stage 6 as segmentation.py writes it, fed with the per-label maxima of the oracle's maxima()."""
    peak, far_value = pen.maxima(labels, dbf, daf, k)
    labels, dbf, daf = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (labels, dbf, daf))
    peak = torch.from_numpy(peak.astype(np.int32)).to(device)
    far_value = torch.from_numpy(far_value.astype(np.float32)).to(device)      # a maximum of float32 words: exact
    rows = labels.clamp(0, k).to(torch.int64)
    root_peak = peak.to(torch.float32).sqrt()[rows]
    far = far_value[rows]
    zero = torch.zeros((), dtype=torch.float32, device=device)
    depth = torch.where(root_peak > 0, (1 - dbf.to(torch.float32).sqrt() / root_peak) ** pdrf_exponent * pdrf_scale,
                        zero)
    return (depth + torch.where(far > 0, daf / far, zero)).to(torch.float32).cpu().numpy()


def random_fields(seed):
    """Labels in -3 .. k + 2 with absent ids, any dbf >= 0 (DBF_INF among them), daf with +inf pieces."""
    rng = np.random.default_rng(3100 + seed)
    shape = tuple(int(rng.integers(1, m + 1)) for m in (9, 11, 40))
    k = int(rng.integers(1, 7))
    labels = rng.integers(-3, k + 3, size=shape).astype(np.int32)
    labels[labels == int(rng.integers(1, k + 1))] = 0 if seed % 2 else labels[labels > 0].min(initial=1)
    dbf = rng.choice(np.array([0, 1, 2, 3, 4, 9, 50, 1000, 2**24 + 1, pen.DBF_INF], dtype=np.int32), size=shape)
    dbf = np.where(rng.random(shape) < 0.5, rng.integers(0, 400, size=shape), dbf).astype(np.int32)
    daf = (rng.random(shape) * rng.choice([1.0, 40.0, 1e4], size=shape)).astype(np.float32)
    daf[rng.random(shape) < 0.1] = np.inf
    daf[rng.random(shape) < 0.1] = 0.0
    if seed % 3 == 0:      # a label whose daf is +inf or 0 throughout: far = 0
        daf[labels == k] = np.where(rng.random(shape) < 0.5, np.inf, 0.0).astype(np.float32)[labels == k]
    if seed % 4 == 0:      # a label whose dbf is 0 throughout: peak = 0
        dbf[labels == 1] = 0
    return labels, dbf, daf, k


def shaped_fields(name):
    """A shared volume with the dbf and daf the chain computes for it (holes left open: a CPU test)."""
    labels = pen.VOLUMES[name]()
    k = int(labels.max())
    roots = ref.first_voxels(labels, k)
    return labels, tref.dbf_of(labels), ref.relaxation(labels, roots), k


@pytest.mark.parametrize("seed", range(6))
def test_the_oracle_equals_its_loop_form_on_seeded_fields(seed):
    labels, dbf, daf, k = random_fields(seed)
    for e in EXPONENTS:
        for scale in SCALES:
            want, loop = pen.cost(labels, dbf, daf, k, e, scale), pen.by_label(labels, dbf, daf, k, e, scale)
            inside = pen.inside_of(labels, k)
            assert np.isnan(want[~inside]).all() and np.isnan(loop[~inside]).all()
            assert not np.isnan(want[inside]).any() and inside.any()
            np.testing.assert_array_equal(np.isinf(want), np.isinf(loop))
            finite = inside & np.isfinite(want)
            np.testing.assert_allclose(want[finite], loop[finite], rtol=1e-13, atol=0)      # pow against repeated *


def test_the_oracle_by_hand():
    labels = np.array([[[1, 1, 1, 0, 2, 2, 5, -1, 3]]], dtype=np.int32)
    dbf = np.array([[[1, 4, 16, 9, 0, 0, 7, 7, 9]]], dtype=np.int32)
    daf = np.array([[[0.0, 1.0, 4.0, 0.0, 0.0, np.inf, 1.0, 1.0, 0.0]]], dtype=np.float32)
    got = pen.cost(labels, dbf, daf, 3, 2, 10.0)[0, 0]
    # label 1: peak 16, far 4; label 2: peak 0 (first term 0), far 0 (second term 0, also for the +inf word);
    # label 3: one voxel, dbf = peak: 10 * 0^2 + 0 (far = 0)
    np.testing.assert_allclose(got[:3], [10 * 0.75 ** 2 + 0.0, 10 * 0.5 ** 2 + 0.25, 1.0], rtol=1e-15)
    assert np.isnan(got[3]) and got[4] == 0 and got[5] == 0 and np.isnan(got[6]) and np.isnan(got[7]) and got[8] == 0
    assert pen.cost(labels, dbf, daf, 3, 0, 10.0)[0, 0, 8] == 10.0      # 0 ** 0 = 1
    assert pen.cost(labels, dbf, daf, 3, 0, 10.0)[0, 0, 4] == 0.0       # peak = 0: no first term at all
    daf[0, 0, 5] = 2.0
    daf[0, 0, 4] = np.inf
    assert pen.cost(labels, dbf, daf, 3, 2, 10.0)[0, 0, 4] == np.inf and pen.by_label(labels, dbf, daf, 3, 2, 10.0)[0, 0, 4] == np.inf
    assert pen.bound(4, 1e5) == 32 * 2.0 ** -24 * 100001.0


@pytest.mark.parametrize("name", sorted(pen.VOLUMES))
def test_the_float32_expression_is_within_the_bound_on_the_shared_volumes(name):
    labels, dbf, daf, k = shaped_fields(name)
    assert labels.size <= 30000
    worst = 0.0
    for e in EXPONENTS:
        for scale in SCALES:
            got = torch_expression(labels, dbf, daf, k, e, scale)
            ratio = pen.worst_ratio(got, pen.cost(labels, dbf, daf, k, e, scale), labels, k, e, scale)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, e, scale, ratio)
    print(f"volume {name}: worst |cost - ref| / bound = {worst:.3f}")
    if name == "e":
        assert (dbf == pen.DBF_INF).all()
        assert (torch_expression(labels, dbf, daf, k, 4, 1e5) <= 1.0).all()      # the first term is 0 everywhere
    if name == "d":
        assert np.isinf(daf[labels == 1]).any() and np.isfinite(daf[labels == 2]).all()


@pytest.mark.parametrize("seed", range(6))
def test_the_float32_expression_is_within_the_bound_on_seeded_fields(seed):
    labels, dbf, daf, k = random_fields(seed)
    for e in EXPONENTS:
        for scale in SCALES:
            got = torch_expression(labels, dbf, daf, k, e, scale)
            ratio = pen.worst_ratio(got, pen.cost(labels, dbf, daf, k, e, scale), labels, k, e, scale)
            assert ratio <= 1.0, (seed, e, scale, ratio)


@pytest.mark.parametrize("wrong", ["dbf for sqrt(dbf)", "no daf / far", "swapped exponent", "another label's peak"])
def test_a_wrong_formula_leaves_the_bound(wrong):
    """The bound is tight enough to tell the formula from its neighbours (a check of the test, not of the code)."""
    labels, dbf, daf, k = shaped_fields("a")
    e, scale = 4, 1e5
    want = pen.cost(labels, dbf, daf, k, e, scale)
    if wrong == "dbf for sqrt(dbf)":
        got = pen.cost(labels, dbf.astype(np.int64) ** 2, daf, k, e, scale)      # sqrt of the square: dbf / peak
    elif wrong == "no daf / far":
        got = pen.cost(labels, dbf, np.zeros_like(daf), k, e, scale)
    elif wrong == "swapped exponent":
        got = pen.cost(labels, dbf, daf, k, 1, scale * 4)
    else:
        peak, far = pen.maxima(labels, dbf, daf, k)
        assert len(set(peak[1:].tolist())) > 1
        rows = np.where(pen.inside_of(labels, k), labels, 0)
        other = np.concatenate([[0], np.roll(peak[1:], 1)])[rows].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            got = scale * (1 - np.sqrt(dbf) / np.sqrt(other)) ** e + np.where(far[rows] > 0, daf / far[rows], 0)
    inside = pen.inside_of(labels, k) & np.isfinite(want)
    assert np.abs(got[inside] - want[inside]).max() > 4 * pen.bound(e, scale)      # daf / far <= 1 is 5.2 bounds at (4, 1e5)
