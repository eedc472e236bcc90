"""Horizon slices of unequal length on the leap kernel's group queue (jh_model_set_rollout_slice_bounds, and the automatic taper of jh_rollout_slice_schedule): a queue
unit's step range comes from a table of bounds instead of an even division of the horizon, so that the slices drawn last -- over which the launch drains -- can be the
short ones.  Where the horizon is cut may not change a bit: every case below is compared word for word with the static grid (set_rollout_schedule(1)) -- costs, candidate
knots, trace rows and the solver counters of jh_rollout_cost_traced, and the nominal of a whole plan step.

The shapes are those of tests/test_gpu_leap_slices.py: 94 rollouts (24 groups, the last ragged), H = 10, JUDO_AMD_LATENCY_SHIFT=0, the queue forced and its grid capped at
one or two workgroups, so that 4 or 8 waves draw 24 x S tickets and most units start from a parked state.  The launch's own count of recomputed units tells a resumed
unit from a recomputed one: all (S - 1) x 24 units behind a first slice with the hook set (flags bit 0), fewer than half of them without it.  Only the two launches of the
automatic rule's device test are of some size (H = 32, two and four groups per wave slot: about 10 ms each)."""

import numpy as np
import pytest

from tests.test_gpu_leap_schedule import _controller, _Direct, _plan_step
from tests.test_gpu_leap_slices import _check, _DirectFrom, _jammed_state, _leap

gpu_test = pytest.mark.gpu

N, H, LD, GROUPS = 94, 10, 97, 24


@pytest.fixture(autouse=True)
def _four_rollouts_per_wave(monkeypatch):
    monkeypatch.setenv("JUDO_AMD_LATENCY_SHIFT", "0")


def _bounded(d, noise, bounds, max_workgroups=0, flags=0, n=N):
    """One launch of `d` under the forced queue with the explicit schedule `bounds`: (outputs, counters), the slices and the bounds it ran; the model is left on the defaults."""
    m = d.ctrl.model
    m.set_rollout_slices(0, max_workgroups, flags)
    m.set_rollout_slice_bounds(bounds)
    try:
        out = d.run(2, noise, n)
        ran, ran_bounds = m.last_rollout_slices(), m.last_rollout_slice_bounds()
    finally:
        m.set_rollout_slice_bounds(())
        m.set_rollout_slices(0, 0, 0)
    return out, ran, ran_bounds


@gpu_test
@pytest.mark.parametrize("state", ["home", "tangled"])
def test_explicit_bounds_give_the_static_grid_bits(gpu, state):
    """Slices of 6 / 3 / 1 steps, two slices of 5, and ten slices of one step, on 4 and on 8 waves, handed off and with every hand-off missed."""
    d = _leap(state)
    assert d.K == 4 and d.H == H and d.nfl == 15
    noise = d.noise(LD, seed=71)
    ref = d.run(1, noise, N)
    assert d.ctrl.model.last_rollout_slices() == 0 and d.ctrl.model.last_rollout_slice_bounds() == ()
    for bounds in ((6, 9), (5,), tuple(range(1, 10))):
        for max_wg in (1, 2):
            for flags in (0, 1):
                got, ran, ran_bounds = _bounded(d, noise, bounds, max_wg, flags)
                assert ran == len(bounds) + 1 and ran_bounds == bounds
                _check((state, bounds, max_wg, flags), ref, got)
                behind = len(bounds) * GROUPS  # units behind a first slice
                assert d.recomputed == behind if flags else 2 * d.recomputed < behind, (state, bounds, max_wg, flags, d.recomputed)


@gpu_test
def test_bounds_behind_the_horizon_are_dropped(gpu):
    """(6, 9, 12, 40) at H = 10 runs as (6, 9): one schedule serves any horizon."""
    d = _leap("home")
    noise = d.noise(LD, seed=72)
    ref = d.run(1, noise, N)
    for flags in (0, 1):
        got, ran, ran_bounds = _bounded(d, noise, (6, 9, 12, 40), 2, flags)
        assert ran == 3 and ran_bounds == (6, 9)
        _check(("dropped bounds", flags), ref, got)
        assert d.recomputed == 2 * GROUPS if flags else 2 * d.recomputed < 2 * GROUPS


@gpu_test
def test_recomputed_steps_count_no_dropped_contacts_under_bounds(gpu):
    """The 48-contact build from a state with more than 48 contacts: contacts are dropped, and the units that recompute seven and nine steps in front of their slices
    count none of them a second time."""
    d = _DirectFrom(_controller("leap_cube", 64, H), _jammed_state())
    noise = d.noise(LD, seed=73)
    ref = d.run(1, noise, N)
    assert ref[1]["contact_overflow"] > 0, ref[1]
    got, ran, ran_bounds = _bounded(d, noise, (7, 9), 2, 1)
    assert ran == 3 and ran_bounds == (7, 9) and d.recomputed == 2 * GROUPS
    _check("dropped contacts", ref, got)


@gpu_test
def test_recomputing_pass_has_its_own_overflow_rows_under_bounds(gpu):
    """The same state on the 64-contact build, 24 waves for 24 groups, every hand-off missed: the recomputing passes keep their contacts above the LDS pool in rows of their own."""
    ctrl = _controller("leap_cube", 64, H)
    ctrl.model.set_contact_capacity(64)
    assert ctrl.model.build()["contact_capacity"] == 64
    d = _DirectFrom(ctrl, _jammed_state())
    noise = d.noise(LD, seed=74)
    ref = d.run(1, noise, N)
    got, ran, ran_bounds = _bounded(d, noise, (7, 9), 0, 1)
    assert ran == 3 and ran_bounds == (7, 9) and d.recomputed == 2 * GROUPS
    _check("overflow rows", ref, got)


@gpu_test
def test_the_64_contact_build_under_bounds(gpu):
    """caltech_leap_cube runs the 64-contact build of the kernel (jh_engine_v5_cap64.hip): the same table there."""
    from judo_amd.controller import make_controller

    ctrl = make_controller("caltech_leap_cube", "mppi")
    ctrl.optimizer.config.num_rollouts = 64
    ctrl.controller_cfg.horizon = H * ctrl.task.dt
    ctrl.reset()
    ctrl.current_state = ctrl.task.default_state()
    build = ctrl.model.build()
    assert build["kernel_generation"] == 3 and build["contact_capacity"] == 64 and not build["cylinder_build"], build
    d = _DirectFrom(ctrl)
    assert d.H == H
    noise = d.noise(LD, seed=75)
    ref = d.run(1, noise, N)
    got, ran, ran_bounds = _bounded(d, noise, (4, 8, 9), 2, 0)
    assert ran == 4 and ran_bounds == (4, 8, 9)
    _check("caltech_leap_cube", ref, got)


@gpu_test
def test_plan_step_nominal_under_bounds(gpu):
    """A whole plan step (nominal, rewards, candidates, traces) from the same noise: static grid against the queue under bounds (6, 9)."""
    ctrl = _controller("leap_cube", N, H)
    noise = np.random.default_rng(19).standard_normal((N - 1, ctrl.optimizer.num_nodes, ctrl.nu)).astype(np.float32)
    ref = _plan_step(ctrl, 1, noise)
    assert np.isfinite(ref[0]["nominal"]).all() and ref[1]["steps"] == N * ctrl.num_timesteps
    try:
        ctrl.model.set_rollout_slices(0, 2, 0)
        ctrl.model.set_rollout_slice_bounds((6, 9))
        got = _plan_step(ctrl, 2, noise)
        assert ctrl.model.last_rollout_slices() == 3 and ctrl.model.last_rollout_slice_bounds() == (6, 9)
        _check("plan step", ref, got)
    finally:
        ctrl.model.set_rollout_slices(0, 0, 0)


@gpu_test
def test_bounds_setter_checks_its_arguments_and_the_later_call_decides(gpu):
    d = _leap("home")
    m = d.ctrl.model
    noise = d.noise(LD, seed=76)
    for bad in ((3, 3), (5, 2), (0,), (-1,), tuple(range(1, 17))):
        with pytest.raises(ValueError):
            m.set_rollout_slice_bounds(bad)
    m.set_rollout_slice_bounds(tuple(range(1, 16)))  # fifteen first steps: sixteen slices, the most
    try:
        # a schedule, then a number: the number
        m.set_rollout_slice_bounds((6, 9))
        m.set_rollout_slices(2, 2, 0)
        d.run(2, noise, N)
        assert m.last_rollout_slices() == 2 and m.last_rollout_slice_bounds() == (5,)
        # a number, then a schedule: the schedule (the grid's cap stays)
        m.set_rollout_slice_bounds((6, 9))
        d.run(2, noise, N)
        assert m.last_rollout_slices() == 3 and m.last_rollout_slice_bounds() == (6, 9)
        # cleared: the automatic rule, which keeps whole groups at 24 of them
        m.set_rollout_slice_bounds(())
        d.run(2, noise, N)
        assert m.last_rollout_slices() == 1 and m.last_rollout_slice_bounds() == ()
    finally:
        m.set_rollout_slice_bounds(())
        m.set_rollout_slices(0, 0, 0)


@gpu_test
def test_automatic_rule_tapers_only_deep_queues(gpu):
    """H = 32 under the automatic schedule: four groups per resident wave run the rule's schedule for that shape -- the taper if one is shipped: bounds strictly increasing, the
    last slice shorter than the first --, two groups per wave run four equal slices; both give the static grid's words."""
    import torch

    from judo_amd.device import rollout_slice_schedule

    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 4  # waves of the kernel the GPU holds
    d = _Direct("leap_cube", 32)
    for groups in (4 * slots + 3, 2 * slots + 3):
        n = 4 * groups - 3  # (the last group ragged)
        noise = d.noise(n, seed=groups)
        ref = d.run(1, noise, n)
        assert d.ctrl.model.last_rollout_slices() == 0
        got = d.run(0, noise, n)
        bounds = d.ctrl.model.last_rollout_slice_bounds()
        assert bounds == rollout_slice_schedule(32, groups, slots) and d.ctrl.model.last_rollout_slices() == len(bounds) + 1
        if groups < 4 * slots:
            assert bounds == (8, 16, 24)
        else:
            assert bounds == SHIPPED_32 and all(b > a for a, b in zip((0,) + bounds, bounds)) and 32 - bounds[-1] < bounds[0]
        _check(("automatic", groups), ref, got)


SHIPPED_64 = (24, 40, 52, 60)  # the automatic schedule of the headline launch (profiles/leap_tapered_slices.md): 24 / 16 / 12 / 8 / 4 steps
SHIPPED_32 = (12, 20, 26, 30)


def test_the_automatic_rule_is_a_pure_function():
    """No device: horizon, groups and wave slots in, the slices' first steps out."""
    from judo_amd.device import rollout_slice_schedule

    assert rollout_slice_schedule(64, 16384, 2048) == SHIPPED_64  # the headline: 65 536 rollouts x 64 steps on 256 CUs
    assert rollout_slice_schedule(32, 4 * 2048 + 3, 2048) == SHIPPED_32
    assert rollout_slice_schedule(8, 2 * 2048 + 3, 2048) == (2, 4, 6)  # a short horizon: four equal slices
    assert rollout_slice_schedule(8, 16384, 2048) == (2, 4, 6)  # however deep the queue
    assert rollout_slice_schedule(64, 4 * 2048 - 1, 2048) == (16, 32, 48)  # below four groups per slot: equal slices
    assert rollout_slice_schedule(31, 16384, 2048) == (7, 15, 23)  # below 32 steps: equal slices
    assert rollout_slice_schedule(64, 2 * 2048 - 1, 2048) == ()  # fewer than two groups per slot: whole groups
    assert rollout_slice_schedule(64, 24, 2048) == () and rollout_slice_schedule(64, 0, 2048) == () and rollout_slice_schedule(64, 16384, 0) == ()
    assert rollout_slice_schedule(1, 16384, 2048) == () and rollout_slice_schedule(2, 16384, 2048) == (1,) and rollout_slice_schedule(3, 16384, 2048) == (1, 2)
    for h in range(1, 200):
        for groups, slots in ((16384, 2048), (5000, 2048), (4096, 2048), (12, 1), (4, 1), (2, 1)):
            b = rollout_slice_schedule(h, groups, slots)
            assert all(0 < x < h for x in b) and all(y > x for x, y in zip(b, b[1:])), (h, groups, slots, b)
