"""The ensemble's risk measure as numpy states it (judo_amd.ensemble.aggregate_costs_host: the mean of the `worst` largest member costs, fp32, added in descending
order) and the admission rule of the members' descriptions.  No GPU."""

import copy

import numpy as np
import pytest


def _costs(M, N, seed):
    return np.random.default_rng(seed).uniform(0.5, 40.0, size=(M, N)).astype(np.float32)


def test_worst_one_is_the_maximum():
    from judo_amd.ensemble import aggregate_costs_host

    c = _costs(5, 300, 1)
    got = aggregate_costs_host(c, 1)
    assert got.dtype == np.float32 and got.shape == (300,)
    np.testing.assert_array_equal(got.view(np.uint32), c.max(axis=0).view(np.uint32))


def test_worst_m_is_the_mean_where_the_sum_is_exact():
    """Small integers times 2^-3: every partial sum is exactly representable, so the sequential fp32 sum is the exact sum and the quotient the correctly rounded mean."""
    from judo_amd.ensemble import aggregate_costs_host

    rng = np.random.default_rng(2)
    for M in (1, 2, 3, 7, 32):
        c = (rng.integers(0, 4096, size=(M, 257)) * 0.125).astype(np.float32)
        sums = c.astype(np.float64).sum(axis=0)  # exact, and below 2^24 eighths: every fp32 partial sum is exact too, in any order
        assert (sums.astype(np.float32).astype(np.float64) == sums).all()
        mean = (sums.astype(np.float32) / np.float32(M)).astype(np.float32)  # numpy's fp32 division is correctly rounded
        np.testing.assert_array_equal(aggregate_costs_host(c, M).view(np.uint32), mean.view(np.uint32))


def test_invariant_under_a_permutation_of_the_members():
    from judo_amd.ensemble import aggregate_costs_host

    c = _costs(6, 300, 3)
    c[4] = c[1]  # (ties)
    perm = np.random.default_rng(4).permutation(6)
    for j in (1, 2, 3, 6):
        np.testing.assert_array_equal(aggregate_costs_host(c, j).view(np.uint32), aggregate_costs_host(c[perm], j).view(np.uint32))


def test_non_increasing_in_worst():
    """The mean of the j largest cannot grow with j (each added value is no larger than those before it).  fp32 rounding of the sum and of the quotient moves either side
    by at most (j + 1) half-ulps: that is the slack."""
    from judo_amd.ensemble import aggregate_costs_host

    c = _costs(8, 300, 5)
    prev = aggregate_costs_host(c, 1)
    for j in range(2, 9):
        cur = aggregate_costs_host(c, j)
        assert (cur <= prev + (j + 1) * np.spacing(prev)).all(), j
        prev = cur
    assert (aggregate_costs_host(c, 8) < aggregate_costs_host(c, 1)).all()


def test_inf_and_the_sentinel_propagate():
    from judo_amd.ensemble import aggregate_costs_host

    c = _costs(4, 6, 6)
    c[2, 0] = np.inf
    c[1, 1] = c[3, 1] = np.float32(3.0e38)
    c[0, 2] = np.float32(3.0e38)
    for j in (1, 2, 4):
        got = aggregate_costs_host(c, j)
        assert got[0] == np.inf, j  # +inf is among the j largest for every j
        assert np.isfinite(got[3:]).all()
    assert aggregate_costs_host(c, 1)[1] == np.float32(3.0e38)
    assert aggregate_costs_host(c, 2)[1] == np.inf  # 3.0e38 + 3.0e38 overflows, as IEEE arithmetic has it
    assert aggregate_costs_host(c, 1)[2] == np.float32(3.0e38) and np.isfinite(aggregate_costs_host(c, 2)[2])


def test_bad_arguments():
    from judo_amd.ensemble import aggregate_costs_host

    c = _costs(3, 4, 7)
    for j in (0, 4):
        with pytest.raises(ValueError, match="worst"):
            aggregate_costs_host(c, j)
    with pytest.raises(ValueError, match=r"\(M, N\)"):
        aggregate_costs_host(c[0], 1)


def test_descriptions_are_admitted_by_their_sections():
    """Perturbed masses, friction and gains move the float section alone and are admitted; another <exclude> pair moves the int section and is refused with the section
    named, as a fleet refuses it."""
    from judo_amd.ensemble import MAX_ENSEMBLE, check_descriptions
    from judo_amd.models import load_description, scaled_description

    desc = load_description("leap_cube")
    ok = [desc, scaled_description(desc, body_mass={"cube": 1.5}, geom_friction={"cube": 0.6}), scaled_description(desc, actuator_kp={None: 1.2})]
    blobs = check_descriptions(ok)
    assert len(blobs) == 3 and len({len(b) for b in blobs}) == 1 and blobs[0] != blobs[1]
    edited = copy.deepcopy(desc)
    edited["excludes"][0] = [6, 10]  # (same lengths, other pair lists)
    with pytest.raises(ValueError, match="member 2.*int section"):
        check_descriptions([desc, ok[1], edited])
    with pytest.raises(ValueError, match="member 1"):
        check_descriptions([load_description("cartpole"), load_description("cylinder_push")])
    with pytest.raises(ValueError, match="at least one"):
        check_descriptions([])
    cart = load_description("cartpole")
    with pytest.raises(ValueError, match=str(MAX_ENSEMBLE)):
        check_descriptions([cart] * (MAX_ENSEMBLE + 1))
    assert MAX_ENSEMBLE == 32
