"""The launch shape of the fused leap kernel (jh_model_set_rollout_schedule): a launch with more groups of four rollouts than the GPU holds waves runs persistent waves
that draw their groups from a per-launch queue; 1 forces the static grid, 2 the queue wherever the kernel has it.  The schedule changes where and when a rollout runs
and nothing else: every output and every solver counter is the same under both, bit for bit -- for the 48-contact build with and without the hand's own contacts, the
64-contact build (leap_cube_down) and the cylinder build, through jh_rollout_cost_traced and through whole plan steps, the sharded entry with a rollout offset included."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H_SHORT = 8
N_QUEUE = 3 * 8192 + 5  # above 2 x CUs x 16 rollouts (8 192 on 256 CUs) and not a multiple of 16: the queue is used, the last group and the last workgroup are ragged
COUNTERS = ("contact_overflow", "newton_cap_hits", "newton_iters", "steps", "wave_newton_iters", "wave_steps")

VARIANTS = ["leap_cube", "leap_cube_noself", "leap_cube_down", "caltech_cylinder"]


def _controller(variant, N, H=H_SHORT):
    from judo_amd.controller import make_controller, make_controller_for

    if variant == "caltech_cylinder":
        from judo_amd.tasks import CaltechLeapCube

        ctrl = make_controller_for(CaltechLeapCube(fingertips="cylinder"), "mppi")
    else:
        ctrl = make_controller("leap_cube_down" if variant == "leap_cube_down" else "leap_cube", "mppi")
    ctrl.optimizer.config.num_rollouts = N
    ctrl.controller_cfg.horizon = H * ctrl.task.dt
    ctrl.reset()
    ctrl.current_state = ctrl.task.default_state()
    if variant == "leap_cube_noself":
        ctrl.model.set_self_collision(False)
    build = ctrl.model.build()
    assert build["kernel_generation"] == 3
    assert build["contact_capacity"] == (48 if variant.startswith("leap_cube") and variant != "leap_cube_down" else 64), build
    assert build["cylinder_build"] == (variant == "caltech_cylinder")
    return ctrl


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same_bits(what, a, b):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()), a.size)


def _counters(model):
    st = model.stats()
    assert st["overflow_pool_fallbacks"] == 0
    return {k: st[k] for k in COUNTERS}


def _plan_step(ctrl, mode, noise):
    """One plan step from the home state on `noise` under rollout schedule `mode`: everything it produces, and the solver counters."""
    import torch

    ctrl.model.set_rollout_schedule(mode)
    ctrl.reset()
    ctrl.current_state = ctrl.task.default_state()
    ctrl.optimizer.injected_noise = noise
    ctrl.keep_candidates = True
    ctrl.model.stats()
    ctrl.update_action()
    torch.cuda.synchronize()
    out = {"nominal": np.array(ctrl.nominal_knots, dtype=np.float32), "rewards": np.array(ctrl.rewards_local, dtype=np.float32),
           "candidates": ctrl.candidate_knots_device.cpu().numpy()}
    tr = ctrl.traces
    if tr is not None:
        out["traces"] = np.array(tr, dtype=np.float32)
    return out, _counters(ctrl.model)


class _Direct:
    """jh_rollout_cost_traced on the device block of a controller that has run one (small) plan step: x0, nominal, sigma, bounds and task parameters as the plan step
    uploaded them, noise and outputs of this test's own."""

    def __init__(self, variant, H=H_SHORT):
        import torch

        self.ctrl = ctrl = _controller(variant, 64, H)
        ctrl.update_action()
        torch.cuda.synchronize()
        self.b = ctrl._last_fused["b"]
        self.K, self.nu, self.H = ctrl.optimizer.num_nodes, ctrl.nu, ctrl.num_timesteps
        assert self.H == H
        self.W = ctrl._weights(self.K, self.H)
        self.nfl = ctrl._fused_trace_floats()

    def noise(self, ld, seed):
        import torch

        g = torch.Generator(device="cuda").manual_seed(seed)
        return torch.randn((self.K, self.nu, ld), device="cuda", generator=g, dtype=torch.float32).contiguous()

    def run(self, mode, noise, N, n_offset=0):
        import torch

        from judo_amd import _lib
        from judo_amd.device import current_stream_ptr

        ctrl, b, ld = self.ctrl, self.b, int(noise.shape[2])
        assert N <= ld
        ctrl.model.set_rollout_schedule(mode)
        costs = torch.full((N,), float("nan"), dtype=torch.float32, device="cuda")
        knots = torch.full((self.K, self.nu, ld), float("nan"), dtype=torch.float32, device="cuda")
        trace = torch.full((N * self.H * self.nfl,), float("nan"), dtype=torch.float32, device="cuda") if self.nfl else None
        ctrl.model.stats()
        st = _lib.lib().jh_rollout_cost_traced(ctrl.model.handle, _lib.ptr(b.x0), _lib.ptr(b.nominal), noise.data_ptr(), ld, _lib.ptr(b.sigma), _lib.ptr(self.W), _lib.ptr(b.lohi),
                                               _lib.ptr(b.tp), int(ctrl.task.phase), N, n_offset, self.H, self.K, _lib.ptr(costs), _lib.ptr(knots), _lib.ptr(trace), current_stream_ptr())
        _lib.check(st, "jh_rollout_cost_traced")
        torch.cuda.synchronize()
        out = {"costs": costs.cpu().numpy(), "knots": knots[:, :, :N].cpu().numpy(), "untouched_knots": knots[:, :, N:].cpu().numpy()}
        if trace is not None:
            out["trace"] = trace.cpu().numpy()
        counters = _counters(ctrl.model)
        assert np.isfinite(out["costs"]).all() and np.isfinite(out["knots"]).all() and np.isnan(out["untouched_knots"]).all()  # every rollout written, nothing beyond them
        assert counters["steps"] == N * self.H  # every rollout ran once
        if N > 4096:  # (outside the latency mode a wave holds four rollouts)
            assert counters["wave_steps"] == ((N + 3) // 4) * self.H  # every group ran once
        return out, counters


@pytest.mark.parametrize("variant", VARIANTS)
def test_rollout_cost_is_the_same_bits_under_both_schedules(gpu, variant):
    """jh_rollout_cost_traced (costs, candidate knots, trace rows where the model has them) and the solver counters: static grid against the queue, N = 24 581 at H = 8, with and
    without a rollout offset (global sample 0, which keeps the nominal, is in the launch only without)."""
    d = _Direct(variant)
    noise = d.noise(N_QUEUE + 3, seed=21)
    for n_offset in (0, 7):
        ref, cref = d.run(1, noise, N_QUEUE, n_offset)
        got, cgot = d.run(2, noise, N_QUEUE, n_offset)
        for k in ref:
            _same_bits((variant, n_offset, k), ref[k], got[k])
        assert cref == cgot, (variant, n_offset, cref, cgot)
        auto, cauto = d.run(0, noise, N_QUEUE, n_offset)  # the default takes the queue at this size: the same bits again
        for k in ref:
            _same_bits((variant, n_offset, k, "automatic"), ref[k], auto[k])
        assert cref == cauto


@pytest.mark.parametrize("variant", VARIANTS)
def test_plan_step_is_the_same_bits_under_both_schedules(gpu, variant):
    """One whole plan step (nominal, rewards, candidates, traces) from the same noise under the static grid and under the queue."""
    ctrl = _controller(variant, N_QUEUE)
    noise = np.random.default_rng(5).standard_normal((N_QUEUE - 1, ctrl.optimizer.num_nodes, ctrl.nu)).astype(np.float32)
    ref, cref = _plan_step(ctrl, 1, noise)
    got, cgot = _plan_step(ctrl, 2, noise)
    assert ctrl.uses_fused_cost and set(ref) == set(got)
    assert np.isfinite(ref["nominal"]).all() and cref["steps"] == N_QUEUE * ctrl.num_timesteps
    for k in ref:
        _same_bits((variant, k), ref[k], got[k])
    assert cref == cgot, (variant, cref, cgot)


def test_sharded_plan_step_with_a_rollout_offset_is_the_same_bits_under_both_schedules(gpu, monkeypatch):
    """The shard entry (jh_plan_step_shard -> records -> jh_plan_merge) of a rank whose shard starts at global rollout 11: the noise column and the 'sample 0 keeps the
    nominal' rule follow the group drawn from the queue exactly as they follow the place in the grid."""
    import judo_amd.controller as C
    from judo_amd.distributed import Shard

    off = 11
    ctrl = _controller("leap_cube", N_QUEUE + off)
    ctrl.force_shard_path = True
    monkeypatch.setattr(C, "shard_rollouts", lambda total, world, rank: Shard(world, rank, total, total - off, off))
    noise = np.random.default_rng(6).standard_normal((N_QUEUE + off - 1, ctrl.optimizer.num_nodes, ctrl.nu)).astype(np.float32)
    ref, cref = _plan_step(ctrl, 1, noise)
    got, cgot = _plan_step(ctrl, 2, noise)
    assert ctrl.last_shard.offset == off and ctrl.last_shard.count == N_QUEUE and ref["rewards"].shape == (N_QUEUE,)
    for k in ref:
        _same_bits(k, ref[k], got[k])
    assert cref == cgot and cref["steps"] == N_QUEUE * ctrl.num_timesteps


def test_a_rollout_does_not_depend_on_what_else_is_in_the_queue(gpu):
    """Under the queue a rollout lands on whichever wave draws its group, next to whatever that wave ran before: the same rollouts in a launch of N and in a launch of 2N
    (other rollouts added behind them) cost the same bits."""
    d = _Direct("leap_cube")
    noise = d.noise(2 * N_QUEUE, seed=33)
    one, _ = d.run(2, noise, N_QUEUE)
    two, _ = d.run(2, noise, 2 * N_QUEUE)
    _same_bits("costs", one["costs"], two["costs"][:N_QUEUE])
    _same_bits("knots", one["knots"], two["knots"][:, :, :N_QUEUE])
    _same_bits("trace", one["trace"], two["trace"][: one["trace"].size])


@pytest.mark.parametrize("N", [32, 37, 4100])
def test_launches_that_fit_the_gpu_keep_the_static_grid_and_its_bits(gpu, N):
    """The latency mode (32 and 37 rollouts: rows of a wave compute copies) and a launch of one group per resident wave slot or fewer (4 100 rollouts) take the static grid under
    the automatic schedule: the bits of schedule 1.  Schedule 2 runs the queue at 4 100 (every wave finds it empty after its own group) and the static grid in latency mode."""
    d = _Direct("leap_cube", H=16)
    noise = d.noise(N, seed=N)
    ref, cref = d.run(1, noise, N)
    for mode in (0, 2):
        got, cgot = d.run(mode, noise, N)
        for k in ref:
            _same_bits((N, mode, k), ref[k], got[k])
        assert cref == cgot


def test_schedule_setter_checks_its_argument(gpu):
    ctrl = _controller("leap_cube", 8)
    for mode in (0, 1, 2):
        ctrl.model.set_rollout_schedule(mode)
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            ctrl.model.set_rollout_schedule(bad)
    ctrl.model.set_rollout_schedule(0)
