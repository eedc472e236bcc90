"""The plan step across its path switches: `Controller.update_action` at the knot counts where one way through hands over to the next.

The closed-form models (cartpole, cylinder_push) run a plan step as one launch (rollout + cost + update tail, k_plan_step) up to
jh_model_one_launch_max_knots(H), as the fused rollout kernel followed by the update tail up to jh_model_max_fused_knots(H), and through the materialise path
(jh_spline_controls -> jh_rollout_materialize -> jh_task_reward -> the update) above, up to K * nu = JH_MAX_KNOT_DIM.  Each side of each hand-over is compared
with the fp64 oracle on the same injected noise; the two launch forms are compared with each other bit for bit (jh_model_set_plan_step_launches); and MPPI at
the small N smoke() runs, where the cost round-off does not average out."""

import numpy as np
import pytest

from tests.conftest import bounded

pytestmark = pytest.mark.gpu


def _controller(task, opt, N, K, H, seed, traces=3):
    from judo_amd.controller import make_controller

    ctrl = make_controller(task, opt)
    ctrl.optimizer.config.num_rollouts = N
    ctrl.optimizer.config.num_nodes = K
    ctrl.controller_cfg.horizon = H * ctrl.task.dt
    ctrl.controller_cfg.max_num_traces = traces
    if opt == "cem":
        ctrl.optimizer.sigma = ((ctrl.optimizer.sigma_min + ctrl.optimizer.sigma_max) / 2) * np.ones((K, ctrl.nu))
    ctrl.reset()
    assert ctrl.num_timesteps == H and ctrl.optimizer.num_nodes == K
    ctrl.current_state = ctrl.task.default_state()
    ctrl.system_metadata = {"goal_quat": np.array([0.0, 1.0, 0.0, 0.0])} if task == "leap_cube" else {}
    rng = np.random.default_rng(seed)
    if ctrl.model.closed_form:
        ctrl.nominal_knots = 0.3 * rng.standard_normal((K, ctrl.nu))
        ctrl.update_spline(ctrl.times, ctrl.nominal_knots)
    return ctrl, rng


def _plan_and_oracle(ctrl, opt, rng):
    """One plan step on injected noise and the oracle's restatement of it (tests/harness.py)."""
    import torch

    from oracle import oracle as O
    from tests.harness import oracle_plan_step

    N, K, nu = ctrl.optimizer.num_rollouts, ctrl.optimizer.num_nodes, ctrl.nu
    noise = rng.standard_normal((max(N - 1, 0), K, nu)).astype(np.float32)
    ctrl.optimizer.injected_noise = noise
    nominal0 = np.atleast_2d(ctrl.spline(ctrl.time + ctrl.spline_timesteps))
    sigma0 = ctrl.optimizer.sigma.copy() if opt == "cem" else None
    ctrl.model.stats(reset=True)
    ctrl.update_action()
    torch.cuda.synchronize()
    return oracle_plan_step(O.Model(ctrl.task.name), ctrl, nominal0, noise, opt, sigma0)


def _check_against_oracle(ctrl, opt, ref, what, cost_tol):
    """Candidates, per-rollout costs, the update (on the GPU's own costs and against the oracle's) and the trace segments."""
    from oracle import oracle as O

    cand = ctrl.candidate_knots
    np.testing.assert_allclose(cand, ref["knots"], rtol=4e-7, atol=4e-7)  # fp32 fma(sigma, noise, nominal) and clip vs fp64
    costs = -ctrl.rewards_local
    assert np.isfinite(costs).all()
    np.testing.assert_allclose(costs, -ref["rewards"], **cost_tol)
    dc = float(np.abs(costs + ref["rewards"]).max())
    if opt == "mppi":
        lam = ctrl.optimizer.temperature
        # the update alone: the fp64 MPPI average of the GPU's own candidates with the GPU's own costs (fp32 weights, sums of N terms)
        exp = O.mppi_update(cand, -costs.astype(np.float64), lam)
        np.testing.assert_allclose(ctrl.nominal_knots, exp, rtol=0, atol=1e-6)
        # against the oracle's whole plan step: a cost error dc moves every log-weight by at most 2 dc / lambda, so the average moves by at most
        # 2 dc / lambda * max |x - nominal| to first order (x 1.5 for the second order at 2 dc / lambda <= 0.3), plus the update's own 1e-6
        spread = float(np.abs(ref["knots"] - ref["nominal"][None]).max())
        bound = 1.5 * 2 * dc / lam * spread + 1e-6
        assert 2 * dc / lam <= 0.3, (what, dc)
        assert bounded(f"{what}: MPPI |nominal - oracle|, derived bound {bound:.2e}", np.abs(ctrl.nominal_knots - ref["nominal"]).max(), bound)
    elif opt == "ps":
        win = int(np.argmax(-costs))
        np.testing.assert_allclose(ctrl.nominal_knots, cand[win], rtol=0, atol=1e-12)  # the candidate itself, copied (through the normaliser's affine map and back)
        # the oracle's argmax, unless two rewards lie within the cost error of each other
        assert ref["rewards"][win] >= ref["rewards"].max() - 2 * dc, what
    else:
        exp_nom, exp_sig, idx_gpu = O.cem_update(cand, -costs.astype(np.float64), ctrl.optimizer.num_elites, ctrl.optimizer.sigma_min, ctrl.optimizer.sigma_max)
        np.testing.assert_allclose(ctrl.nominal_knots, exp_nom, rtol=5e-7, atol=5e-8)
        np.testing.assert_allclose(ctrl.optimizer.sigma, exp_sig, rtol=5e-7, atol=5e-9)
        _, _, idx_ref = O.cem_update(ref["knots"], ref["rewards"], ctrl.optimizer.num_elites, ctrl.optimizer.sigma_min, ctrl.optimizer.sigma_max)
        cut = np.sort(ref["rewards"])[::-1][len(idx_ref) - 1]
        for i in set(idx_gpu) ^ set(idx_ref):  # elites may differ only where the oracle's rewards sit within the cost error of the elite cut
            assert abs(ref["rewards"][i] - cut) <= 2 * dc, (what, i)
    adrs = [s["adr"] for s in ctrl.trace_sensors]
    if adrs:
        exp = O.trace_segments(ref["sensors"], ctrl.rewards, adrs, ctrl.max_num_traces)
        assert ctrl.traces.shape == exp.shape
        np.testing.assert_allclose(ctrl.traces, exp, rtol=0, atol=1e-5)  # fp32 sensors of the elites after up to 64 steps (observed <= 8.7e-7)


CLOSED_TOL = dict(rtol=3e-6, atol=3e-5)  # per-rollout cost: fp32 accumulation over H steps of O(1..100) terms (tests/test_gpu_simple.py)


@pytest.mark.parametrize("where", ["one_launch_last", "one_launch_next", "fused_last", "fused_next", "knot_dim_max"])
@pytest.mark.parametrize("H", [16, 64])
@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
@pytest.mark.parametrize("task", ["cartpole", "cylinder_push"])
def test_closed_form_plan_step_at_every_hand_over(gpu, task, opt, H, where):
    """The last K of each path and the first of the next, read from the library's own limits: one launch -> two launches -> materialise, and
    K * nu = JH_MAX_KNOT_DIM.  The path taken is checked too (jh_model_stats counts the one-launch plan steps)."""
    from judo_amd import _lib
    from judo_amd.controller import make_controller

    probe = make_controller(task, opt)
    nu = probe.nu
    one, fused = probe.model.one_launch_max_knots_at(H), probe.model.max_fused_knots_at(H)
    assert 1 <= one < fused < _lib.MAX_KNOT_DIM // nu
    K = {"one_launch_last": one, "one_launch_next": one + 1, "fused_last": fused, "fused_next": fused + 1, "knot_dim_max": _lib.MAX_KNOT_DIM // nu}[where]
    ctrl, rng = _controller(task, opt, 257, K, H, seed=K * 31 + H)
    ref = _plan_and_oracle(ctrl, opt, rng)
    assert ctrl.uses_fused_cost == (K <= fused)
    assert ctrl.model.stats()["one_launch_plan_steps"] == (ctrl.max_opt_iters if K <= one else 0)
    _check_against_oracle(ctrl, opt, ref, f"{task} {opt} H={H} K={K} ({where})", CLOSED_TOL)


@pytest.mark.parametrize("task,opt,materialize", [("leap_cube", "mppi", False), ("leap_cube", "mppi", True), ("leap_cube", "cem", True), ("fr3_pick", "mppi", False),
                                                  ("fr3_pick", "cem", False)])
@pytest.mark.parametrize("KU", [256, 512])
def test_articulated_plan_step_at_large_knot_dims(gpu, task, opt, materialize, KU):
    """K * nu = 256 and 512: the leap_cube kernel takes them fused (it reads the knots from memory), fr3_pick and `force_materialize` through the materialise
    path, whose spline kernel stages 64 rollouts' K * nu knots in LDS only where they fit."""
    ctrl, rng = _controller(task, opt, 16, KU // {"leap_cube": 16, "fr3_pick": 8}[task], 4, seed=KU)
    ctrl.force_materialize = materialize
    ref = _plan_and_oracle(ctrl, opt, rng)
    assert ctrl.uses_fused_cost == (task == "leap_cube" and not materialize)
    _check_against_oracle(ctrl, opt, ref, f"{task} {opt} K*nu={KU} materialize={materialize}", dict(rtol=2e-6, atol=2e-5))  # (tests/test_gpu_edges.py: four steps, fp32 vs fp64 engine)


@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
@pytest.mark.parametrize("task", ["cartpole", "cylinder_push"])
def test_one_and_two_launch_plan_steps_are_bit_identical(gpu, task, opt):
    """jh_plan_step forced to one launch and forced to two (jh_model_set_plan_step_launches), host block read in place as the controller does, trace elites on,
    ragged N, three consecutive plan steps: the same nominal, sigma, costs and trace records to the bit."""
    import torch

    for N in (1, 255, 257, 4097):
        runs = []
        for launches in (1, 2):
            ctrl, _ = _controller(task, opt, N, 4, 25, seed=0)
            ctrl.model.set_plan_step_launches(launches)
            ctrl.optimizer.seed(1234)
            ctrl.model.stats(reset=True)
            steps = []
            for step in range(3):
                ctrl.time = 0.05 * step
                ctrl.update_action()
                torch.cuda.synchronize()
                assert ctrl.uses_fused_cost and ctrl._trace_stage["kind"] == "sensors"
                steps.append((ctrl.nominal_knots.copy(), np.atleast_1d(getattr(ctrl.optimizer, "sigma", 0.0)).copy(), ctrl.costs_device.cpu().numpy(), ctrl._trace_stage["recs"].copy(),
                              ctrl.traces.copy()))
            assert ctrl.model.stats()["one_launch_plan_steps"] == (3 * ctrl.max_opt_iters if launches == 1 else 0)
            runs.append(steps)
        for step, (a, b) in enumerate(zip(*runs)):
            for name, x, y in zip(("nominal", "sigma", "costs", "trace records", "traces"), a, b):
                np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"{task} {opt} N={N} step {step}: {name}")


def test_forced_one_launch_refuses_what_it_cannot_hold(gpu):
    from judo_amd.device import GpuModel

    ctrl, _ = _controller("cartpole", "mppi", 64, 4, 64, seed=0)
    K = ctrl.model.one_launch_max_knots_at(64) + 1
    ctrl.model.set_plan_step_launches(1)
    ctrl.optimizer.config.num_nodes = K
    with pytest.raises(ValueError, match="one launch is forced"):
        ctrl.update_action()
    ctrl.model.set_plan_step_launches(0)  # automatic: the same plan step takes two launches
    ctrl.update_action()
    assert np.isfinite(ctrl.nominal_knots).all() and ctrl.nominal_knots.shape == (K, 1)
    leap = GpuModel("leap_cube", gpu)
    assert leap.one_launch_max_knots_at(16) == 0
    with pytest.raises(ValueError):
        leap.set_plan_step_launches(1)
    leap.set_plan_step_launches(2)
    with pytest.raises(ValueError):
        leap.set_plan_step_launches(3)


@pytest.mark.parametrize("H", [16, 64])
@pytest.mark.parametrize("N", [32, 64])
@pytest.mark.parametrize("task", ["cartpole", "cylinder_push"])
def test_small_n_mppi_on_the_closed_form_models(gpu, task, N, H):
    """smoke()'s case as a test: MPPI at a few tens of rollouts, where one cost's round-off moves the plan (lambda = 0.0025).  Three separate checks: the costs
    against the oracle's, the update against the fp64 update of the GPU's own costs, the plan against the oracle's plan."""
    from oracle import oracle as O

    ctrl, rng = _controller(task, "mppi", N, 4, H, seed=N + H)
    ref = _plan_and_oracle(ctrl, "mppi", rng)
    costs = -ctrl.rewards_local
    rel = np.abs(costs + ref["rewards"]) / np.maximum(np.abs(ref["rewards"]), 1e-30)
    # a cost is a sum of H positive fp32 terms: (H - 1) u relative for the additions, a few u per term for its own arithmetic (v_sqrt_f32 / v_rcp_f32, 1 ulp
    # each) -- (H + 8) u in all (observed on the MI355X: 0.1 .. 0.3 of it; the state's own fp32 drift over H steps stays below it at these horizons)
    assert bounded(f"small-N MPPI {task} N={N} H={H}: costs, max relative error", rel.max(), (H + 8) * 2.0**-24)
    exp = O.mppi_update(ref["knots"], -costs.astype(np.float64), ctrl.optimizer.temperature)
    assert bounded(f"small-N MPPI {task} N={N} H={H}: |nominal - fp64 update of the GPU's costs|", np.abs(ctrl.nominal_knots - exp).max(), 1.5e-6)
    # 5 x the largest error observed on the MI355X for this model and horizon (N = 32 and 64): cartpole 2.65e-5 / 4.8e-8, cylinder_push 2.2e-6 / 1.2e-7 at H = 16 / 64
    # (at H = 64 the costs spread over many lambda and the best rollout alone carries the plan; at H = 16 a few weights share it and the cost round-off moves them)
    tol = {("cartpole", 16): 1.35e-4, ("cartpole", 64): 2.4e-7, ("cylinder_push", 16): 1.1e-5, ("cylinder_push", 64): 6e-7}[task, H]
    assert bounded(f"small-N MPPI {task} N={N} H={H}: |nominal - oracle|", np.abs(ctrl.nominal_knots - ref["nominal"]).max(), tol)
