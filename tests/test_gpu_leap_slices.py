"""Horizon slices on the leap kernel's group queue (jh_model_set_rollout_slices): a queue unit is (group of four rollouts, slice of the horizon), a slice parks the
rollouts' state for the next one behind a flag that is read once, and a wave that finds the flag unset recomputes the group's steps up to its slice.  None of it may
change a bit: every case below is compared word for word with the static grid (set_rollout_schedule(1)) -- costs, candidate knots, trace rows and the solver counters
of jh_rollout_cost_traced, and the nominal of a whole plan step.

The launches are small (94 rollouts = 24 groups, the last ragged; H = 10, which 3 and 4 do not divide), so the tests leave the latency mode (JUDO_AMD_LATENCY_SHIFT=0:
four rollouts per wave under both schedules, hence the same wave-level counters), force the queue, and cap its grid at one or two workgroups: 4 or 8 waves then draw
24 x S tickets, and most units start from a parked state.  The bits cannot tell a resumed unit from a recomputed one, so the cases also read the launch's count of
recomputed units (jh_model_recomputed_units): every unit behind the first slice with the hook set, and few without it -- dependent units are 24 tickets apart and
at most 8 are in flight, so a producer would have to outlast three units in a row on every other wave; "fewer than half" is asserted."""

import numpy as np
import pytest

from tests.test_gpu_leap_schedule import _bits, _controller, _counters, _Direct, _plan_step, _same_bits  # noqa: F401  (the helpers of the schedule tests)
from tests.test_gpu_leap_self import _contact_kinds, _tangled_states

pytestmark = pytest.mark.gpu

N, H, LD = 94, 10, 97


@pytest.fixture(autouse=True)
def _four_rollouts_per_wave(monkeypatch):
    monkeypatch.setenv("JUDO_AMD_LATENCY_SHIFT", "0")


class _DirectFrom(_Direct):
    """_Direct with a start state of the test's choice (None: the home state) on a controller of the test's choice."""

    def __init__(self, ctrl, state=None):
        import torch

        self.ctrl = ctrl
        if state is not None:
            ctrl.current_state = np.asarray(state, dtype=np.float64)
        ctrl.update_action()
        torch.cuda.synchronize()
        self.b = ctrl._last_fused["b"]
        self.K, self.nu, self.H = ctrl.optimizer.num_nodes, ctrl.nu, ctrl.num_timesteps
        self.W = ctrl._weights(self.K, self.H)
        self.nfl = ctrl._fused_trace_floats()

    def run(self, mode, noise, n, n_offset=0):
        """_Direct.run, which also keeps the launch's count of recomputed units (read in front of the counters' reset) in `self.recomputed`."""
        import tests.test_gpu_leap_schedule as sched

        orig = sched._counters

        def counters(model):
            self.recomputed = model.recomputed_units()
            return orig(model)

        sched._counters = counters
        try:
            return super().run(mode, noise, n, n_offset)
        finally:
            sched._counters = orig

    def sliced(self, noise, slices, max_workgroups=0, flags=0, n=N):
        """One launch under the forced queue with these slices; the model is left on the defaults."""
        m = self.ctrl.model
        m.set_rollout_slices(slices, max_workgroups, flags)
        try:
            out = self.run(2, noise, n)
            ran = m.last_rollout_slices()
        finally:
            m.set_rollout_slices(0, 0, 0)
        return out, ran


def _leap(state):
    ctrl = _controller("leap_cube", 64, H)
    if state == "tangled":  # the hand's own contacts and their warm start cross the slice boundaries
        return _DirectFrom(ctrl, _tangled_state())
    return _DirectFrom(ctrl)


def _jammed_state():
    """The first of the jammed-cube configurations of tests/test_gpu_leap_self.py (the cube inside a tangled hand at a random attitude) with 50 to 62 contacts, some of
    them between two finger chains, by the oracle's count: above the 48 contacts of the LDS pool, within the 64 of the larger build."""
    n = 1200
    rng = np.random.default_rng(123)
    om, xs, q = _tangled_states(n, seed=99, frac=0.5)
    home = xs[0, :3].copy()
    home[2] -= 0.3
    xs[:, :3] = home + rng.uniform(-0.03, 0.03, (n, 3))
    quat = rng.standard_normal((n, 4))
    xs[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    xs[:, 23:29] = rng.standard_normal((n, 6)) * np.array([0.2, 0.2, 0.2, 2, 2, 2])
    for x, u in zip(xs, q):
        k = _contact_kinds(om, x, u)
        if 50 <= sum(k[:3]) <= 62 and k[2] > 0:
            return x
    raise AssertionError("no jammed state with 50 to 62 contacts")


def _tangled_state():
    """The first of the tangled hand configurations of tests/test_gpu_leap_self.py in which two finger chains touch each other (the oracle's forward pass says so)."""
    om, xs, q = _tangled_states(32, seed=17)
    for x, u in zip(xs, q):
        if _contact_kinds(om, x, u)[2] > 0:
            return x
    raise AssertionError("no tangled state with a contact between two finger chains")


def _check(what, ref, got):
    (oref, cref), (ogot, cgot) = ref, got
    assert set(oref) == set(ogot)
    for k in oref:
        _same_bits((what, k), oref[k], ogot[k])
    assert cref == cgot, (what, cref, cgot)


@pytest.mark.parametrize("state", ["home", "tangled"])
def test_sliced_queue_gives_the_static_grid_bits(gpu, state):
    """Tickets and hand-offs, and the recomputation (flags = 1: every hand-off counts as missed): S = 2, 3, 4 on 4 and on 8 waves."""
    d = _leap(state)
    assert d.K == 4 and d.H == H and d.nfl == 15
    noise = d.noise(LD, seed=41)
    ref = d.run(1, noise, N)
    assert d.ctrl.model.last_rollout_slices() == 0
    for slices in (2, 3, 4):
        for max_wg in (1, 2):
            for flags in (0, 1):
                got, ran = d.sliced(noise, slices, max_wg, flags)
                assert ran == slices
                _check((state, slices, max_wg, flags), ref, got)
                behind = (slices - 1) * 24  # units behind a first slice
                assert d.recomputed == behind if flags else 2 * d.recomputed < behind, (state, slices, max_wg, flags, d.recomputed)


def test_recomputed_steps_count_no_dropped_contacts(gpu):
    """The 48-contact build from a state with more than 48 contacts: the launch drops contacts (contact_overflow > 0), and a unit that recomputes the steps in front of
    its slice must not count theirs a second time -- the counters are the static grid's with every hand-off missed as well."""
    d = _DirectFrom(_controller("leap_cube", 64, H), _jammed_state())
    noise = d.noise(LD, seed=44)
    ref = d.run(1, noise, N)
    assert ref[1]["contact_overflow"] > 0, ref[1]
    for slices, max_wg, flags in ((3, 2, 1), (4, 1, 1), (3, 2, 0)):
        got, ran = d.sliced(noise, slices, max_wg, flags)
        assert ran == slices and (d.recomputed == (slices - 1) * 24 if flags else True)
        _check(("dropped contacts", slices, max_wg, flags), ref, got)


def test_recomputing_beside_the_running_producer_keeps_the_overflow_rows_apart(gpu):
    """The 64-contact build keeps contacts 49 .. 64 of a rollout in a row of global memory.  24 waves for 24 groups and one step per unit (S = H): the first waves to
    finish draw second slices whose producers are still running, so units recompute WHILE the producer runs the same rollouts, from a state with more than 48
    contacts -- both then use overflow rows in the same steps, and the recomputing pass has rows of its own."""
    ctrl = _controller("leap_cube", 64, H)
    ctrl.model.set_contact_capacity(64)
    assert ctrl.model.build()["contact_capacity"] == 64
    d = _DirectFrom(ctrl, _jammed_state())
    noise = d.noise(LD, seed=45)
    ref = d.run(1, noise, N)
    missed = 0
    for slices in (H, 5, H):
        got, ran = d.sliced(noise, slices, 0, 0)
        assert ran == slices
        missed += d.recomputed
        _check(("overflow rows", slices), ref, got)
    assert missed > 0  # (hand-offs were missed with the producer under way: that is the case under test)
    got, _ = d.sliced(noise, H, 0, 1)
    assert d.recomputed == (H - 1) * 24
    _check(("overflow rows", "every hand-off missed"), ref, got)


def test_slices_are_clipped_to_the_horizon(gpu):
    """S = H (one step per unit) and S > H (clipped to it) agree with each other and with the static grid, handed off and recomputed."""
    d = _leap("tangled")
    noise = d.noise(LD, seed=42)
    ref = d.run(1, noise, N)
    for flags in (0, 1):
        a, ran_a = d.sliced(noise, H, 2, flags)
        b, ran_b = d.sliced(noise, 64, 2, flags)
        assert ran_a == H and ran_b == H
        _check(("S = H", flags), ref, a)
        _check(("S > H", flags), ref, b)


def test_one_slice_is_the_queue_of_whole_groups(gpu):
    d = _leap("home")
    noise = d.noise(LD, seed=43)
    ref = d.run(1, noise, N)
    queue = d.run(2, noise, N)
    assert d.ctrl.model.last_rollout_slices() == 1  # (24 groups: far from two per resident wave, the automatic rule keeps whole groups)
    one, ran = d.sliced(noise, 1, 2, 0)
    assert ran == 1
    _check("queue", ref, queue)
    _check("S = 1", ref, one)


def test_plan_step_nominal_under_slices(gpu):
    """A whole plan step (nominal, rewards, candidates, traces) from the same noise: static grid against the sliced queue, handed off and recomputed."""
    ctrl = _controller("leap_cube", N, H)
    noise = np.random.default_rng(9).standard_normal((N - 1, ctrl.optimizer.num_nodes, ctrl.nu)).astype(np.float32)
    ref = _plan_step(ctrl, 1, noise)
    assert np.isfinite(ref[0]["nominal"]).all() and ref[1]["steps"] == N * ctrl.num_timesteps
    try:
        for slices, flags in ((3, 0), (4, 1)):
            ctrl.model.set_rollout_slices(slices, 2, flags)
            got = _plan_step(ctrl, 2, noise)
            assert ctrl.model.last_rollout_slices() == slices
            _check(("plan step", slices, flags), ref, got)
    finally:
        ctrl.model.set_rollout_slices(0, 0, 0)


def test_two_streams_share_one_model(gpu):
    """Two sliced launches of one model in flight on two streams: flags and parked rows are per launch, so both give the static grid's words."""
    import torch

    from judo_amd import _lib
    from judo_amd.device import current_stream_ptr

    d = _leap("tangled")
    noises = [d.noise(LD, seed=51), d.noise(LD, seed=52)]
    refs = [d.run(1, nz, N) for nz in noises]
    ctrl, b, m = d.ctrl, d.b, d.ctrl.model
    m.set_rollout_schedule(2)
    m.set_rollout_slices(4, 1, 0)
    m.stats()
    outs = []
    try:
        torch.cuda.synchronize()
        for nz in noises:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                costs = torch.full((N,), float("nan"), dtype=torch.float32, device="cuda")
                knots = torch.full((d.K, d.nu, LD), float("nan"), dtype=torch.float32, device="cuda")
                trace = torch.full((N * d.H * d.nfl,), float("nan"), dtype=torch.float32, device="cuda")
                st = _lib.lib().jh_rollout_cost_traced(m.handle, _lib.ptr(b.x0), _lib.ptr(b.nominal), nz.data_ptr(), LD, _lib.ptr(b.sigma), _lib.ptr(d.W), _lib.ptr(b.lohi), _lib.ptr(b.tp),
                                                       int(ctrl.task.phase), N, 0, d.H, d.K, _lib.ptr(costs), _lib.ptr(knots), _lib.ptr(trace), current_stream_ptr())
                _lib.check(st, "jh_rollout_cost_traced")
            outs.append((s, costs, knots, trace))
        torch.cuda.synchronize()
        assert m.last_rollout_slices() == 4
    finally:
        m.set_rollout_slices(0, 0, 0)
        m.set_rollout_schedule(0)
    both = _counters(m)
    for (oref, _), (_, costs, knots, trace) in zip(refs, outs):
        _same_bits("costs", oref["costs"], costs.cpu().numpy())
        _same_bits("knots", oref["knots"], knots[:, :, :N].cpu().numpy())
        _same_bits("trace", oref["trace"], trace.cpu().numpy())
    assert both == {k: refs[0][1][k] + refs[1][1][k] for k in both}


def test_the_64_contact_build_under_slices(gpu):
    """caltech_leap_cube runs the 64-contact build of the kernel (jh_engine_v5_cap64.hip): the same rule there."""
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
    noise = d.noise(LD, seed=61)
    ref = d.run(1, noise, N)
    for flags in (0, 1):
        got, ran = d.sliced(noise, 3, 2, flags)
        assert ran == 3
        _check(("caltech_leap_cube", flags), ref, got)


def test_slices_setter_checks_its_arguments(gpu):
    ctrl = _controller("leap_cube", 8)
    for good in ((0, 0, 0), (1, 0, 0), (64, 3, 1), (4, 512, 0)):
        ctrl.model.set_rollout_slices(*good)
    for bad in ((-1, 0, 0), (65, 0, 0), (2, -1, 0), (2, 0, 2), (2, 0, -1)):
        with pytest.raises(ValueError):
            ctrl.model.set_rollout_slices(*bad)
    ctrl.model.set_rollout_slices(0, 0, 0)
    ctrl.model.set_rollout_slices()


def test_automatic_rule_slices_only_launches_of_two_groups_per_wave(gpu):
    """Under the automatic schedule a launch that takes the queue with fewer than two groups per resident wave keeps whole groups, one with more is sliced; both
    give the static grid's words (H = 8: four slices of two steps)."""
    import torch

    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 4  # waves of the kernel the GPU holds
    d = _Direct("leap_cube")
    for groups, want in ((slots + slots // 2 + 1, 1), (2 * slots + 3, 4)):
        n = 4 * groups - 3  # (the last group ragged)
        noise = d.noise(n, seed=groups)
        ref = d.run(1, noise, n)
        assert d.ctrl.model.last_rollout_slices() == 0
        got = d.run(0, noise, n)
        assert d.ctrl.model.last_rollout_slices() == want, (groups, slots)
        _check(("automatic", groups), ref, got)
