"""tests/ro_reference.py -- the numpy restatement of add_to_mixed_opac for any number of Gauss points -- against the oracle's
port of the kernel where that exists (ny = 20: bit for bit), and held to what the rule implies where it does not."""
import numpy as np
import pytest

import ro_reference as rr
from helios_amd import phys_const as pc
from helios_amd import synthetic as syn

NYS = (2, 3, 7, 8, 10, 16, 19)


def test_equals_the_oracle_bit_for_bit_at_20_points(port):
    ny = 20
    gy, gw = syn.gauss_points(ny)
    for name, (mix0, spec) in rr.cases(ny, nbin=24, nlev=2).items():
        got, want = rr.call(rr, ny, mix0, spec, gw, gy), rr.call(port, ny, mix0, spec, gw, gy)
        assert np.abs(want - mix0).max() > 0, name
        np.testing.assert_array_equal(got, want, err_msg=name)


def test_equals_the_oracle_bit_for_bit_at_every_crossing_index(port):
    ny = 20
    gy, gw = syn.gauss_points(ny)
    mix0, spec = rr.crossing_rows(ny)
    np.testing.assert_array_equal(rr.call(rr, ny, mix0, spec, gw, gy), rr.call(port, ny, mix0, spec, gw, gy))


@pytest.mark.parametrize("ny", NYS)
def test_results_ascend_between_the_first_and_the_last_sum(ny):
    """two k-distributions in, one k-distribution out: ascending, inside [smallest sum, largest sum] -- wherever every Gauss
    point is interpolated inside an interval of its own (the walk's other case extrapolates)"""
    gy, gw = syn.gauss_points(ny)
    problems = {k: v for k, v in rr.cases(ny, nbin=24, nlev=2).items() if k != "unsorted"}
    problems["crossings"] = rr.crossing_rows(ny)
    regular = 0
    for name, (mix0, spec) in problems.items():
        mixed, new = mix0.reshape(-1, ny), (spec * rr.FAC).reshape(-1, ny)
        got, skipped = rr.mix_problems(mixed, new, gw, gy, with_skipped=True)
        assert np.all(np.isfinite(got)), name
        got, mixed, new = got[~skipped], mixed[~skipped], new[~skipped]
        regular += len(got)
        lo, hi = mixed[:, :1] + new[:, :1], mixed[:, -1:] + new[:, -1:]
        # (the interpolation between two EQUAL sums returns them within its own rounding, two products, a sum and a quotient)
        assert np.all(np.diff(got, axis=1) >= -1e-15 * got[:, 1:]), name
        assert np.all(got >= lo * (1 - 1e-12)) and np.all(got <= hi * (1 + 1e-12)), name
    assert regular > 100


@pytest.mark.parametrize("ny", NYS)
def test_a_negligible_absorber_is_added_point_by_point(ny):
    gy, gw = syn.gauss_points(ny)
    rng = np.random.default_rng(ny)
    mix0 = np.sort(10.0 ** rng.uniform(-2, 0, (2, 5, ny)), axis=2)
    add = np.sort(10.0 ** rng.uniform(-2, 0, (2, 5, ny)), axis=2) * 0.0099 * mix0[..., :1] / 1.0     # max(add) < 1 % of min(mix)
    fac = 1e-3 * (18.0 * pc.AMU) / (2.3 * pc.AMU)          # as the call forms it
    np.testing.assert_array_equal(rr.call(rr, ny, mix0, add / rr.FAC, gw, gy), mix0 + fac * (add / rr.FAC))
    # ... and the other way round
    np.testing.assert_array_equal(rr.call(rr, ny, add, mix0 / rr.FAC, gw, gy), add + fac * (mix0 / rr.FAC))


def test_one_gauss_point_is_correlated_k():
    mix0, spec = np.full((2, 3, 1), 0.5), np.full((2, 3, 1), 0.25) / rr.FAC
    fac = 1e-3 * (18.0 * pc.AMU) / (2.3 * pc.AMU)
    np.testing.assert_array_equal(rr.call(rr, 1, mix0, spec, np.array([2.0]), np.array([0.5])), mix0 + fac * spec)


def test_fill_order_is_a_permutation_of_the_tableau():
    for ny in NYS:
        for yx in range(1, ny + 1):
            for first in (False, True):
                y1, y2 = rr.fill_order(ny, yx, first)
                assert sorted(zip(y1.tolist(), y2.tolist())) == [(a, b) for a in range(ny) for b in range(ny)]
