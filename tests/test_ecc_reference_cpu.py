"""CPU: the float64 restatement of one ECC iteration (tests/ecc_reference.py: ecc_step64) and the oracle (orc_ecc_translation) are
two independent implementations; what the GPU probes (test_gpu_registration_probe.py) rest on is checked here without a GPU:
they fail on the same cases, agree within 1e-6 px / 1e-7 where both succeed (measured: 4.8e-7 px, 1.1e-8), the probe cases are
well conditioned (step <= 8 px, largest 7.69; the three starts that take a longer step - 22.6, 9.3 and 8.3 px - are named in
ecc_reference.OVER_CAP, and the two references agree on them to the last digit), the oracle finds known off-diagonal translations
with their signs (worst error 0.066 px), and the reference notices a wrong pixel, a dropped border column and swapped axes."""
import numpy as np
import pytest

import ecc_reference as E


@pytest.fixture(scope="module")
def grid(oracle):
    return E.reference_grid(oracle)


def test_both_references_fail_on_the_same_cases(grid):
    for (shape, start, masked), (o, r) in grid.items():
        assert (o is None) == (r is None), (shape, start, masked, o, r)
        if E.listed_failure(shape, start):
            assert o is None and r is None, (shape, start, masked)
    # (the listed failures are in the grid, and the probe shapes do succeed elsewhere)
    assert sum(E.listed_failure(s, t) for s, t, _ in grid) >= 3 * len(E.STARTS) + 2 + 2 * len(E.PROBE_SHAPES)
    assert grid[(E.ILL_CONDITIONED_SHAPE, (0.0, 0.0), False)][0] is not None
    for shape in E.PROBE_SHAPES:
        # (at 3 columns the starts of 3 px and more leave no overlap: both references fail there too)
        assert grid[(shape, (0.0, 0.0), False)][0] is not None and sum(grid[(shape, s, False)][0] is not None for s in E.STARTS) >= len(E.STARTS) // 2, shape


def test_references_agree_within_the_floors_and_no_probe_case_is_ill_conditioned(grid):
    worst_t = worst_cc = worst_step = 0.0
    for (shape, start, masked), (o, r) in grid.items():
        if o is None or shape == E.ILL_CONDITIONED_SHAPE:
            continue
        d_t, d_cc = max(abs(o[0] - r[0]), abs(o[1] - r[1])), abs(o[2] - r[2])
        step = max(abs(v[0] - np.float32(start[0])) for v in (o, r)), max(abs(v[1] - np.float32(start[1])) for v in (o, r))
        worst_t, worst_cc, worst_step = max(worst_t, d_t), max(worst_cc, d_cc), max(worst_step, *step)
        assert d_t <= E.FLOOR_T and d_cc <= E.FLOOR_CC, (shape, start, masked, d_t, d_cc)
        # a condition of the inputs, not a tolerance; the three (shape, start) that do not meet it are named, and do exceed it
        assert (max(step) <= E.STEP_CAP) != ((shape, start) in E.OVER_CAP), (shape, start, masked, step)
    print("oracle vs float64 reference: %.3g px, %.3g on rho; largest step %.3g px" % (worst_t, worst_cc, worst_step))


@pytest.mark.parametrize("shape", E.TRUTH_SHAPES)
@pytest.mark.parametrize("truth", E.TRUTHS)
def test_oracle_finds_off_diagonal_translations_with_their_signs(oracle, shape, truth):
    t, i = E.truth_pair(shape, truth)
    tx = ty = 0.0
    for it in range(E.TRUTH_ITERATIONS):
        tx, ty, _ = E.oracle_step(oracle, t, i, tx, ty)
        # no rint tie can flip between implementations that differ in the last digits
        for v in (tx, ty):
            assert abs((v % 1.0) - 0.5) > 1e-3, (it, tx, ty)
    whole = oracle.ecc_translation(t, i, (0.0, 0.0), max_iter=E.TRUTH_ITERATIONS, eps=0.0)
    assert (whole[0], whole[1]) == (tx, ty) and whole[3] == E.TRUTH_ITERATIONS  # (the chain of single iterations is the 12-iteration run)
    print("truth %s at %s: oracle (%.5f, %.5f)" % (truth, shape, tx, ty))
    assert abs(tx - truth[0]) <= 0.1 and abs(ty - truth[1]) <= 0.1, (tx, ty)


@pytest.mark.parametrize("shape", [(67, 83), (300, 701)])
def test_reference_notices_a_wrong_pixel_a_dropped_column_and_swapped_axes(shape):
    h, w = shape
    t, i = E.probe_inputs(shape)
    moved = {"pixel": 0.0, "column": 0.0, "axes": 0.0}
    wrong = t.copy()
    wrong[h // 2, w // 3] = 3.0  # one template pixel replaced
    last_column = np.ones(shape, np.uint8)
    last_column[:, w - 1] = 0
    for start in E.STARTS:
        base = E.ecc_step64(t, i, start[0], start[1])
        for name, got in (("pixel", E.ecc_step64(wrong, i, start[0], start[1])),
                          ("column", E.ecc_step64(t, i, start[0], start[1], last_column)),
                          ("axes", E.ecc_step64(t, i, start[1], start[0]))):
            d = np.inf if got is None else max(abs(got[0] - base[0]), abs(got[1] - base[1]))
            moved[name] = max(moved[name], d)
    print(shape, moved)
    assert all(v > 1e-4 for v in moved.values()), moved
