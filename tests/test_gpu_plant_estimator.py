"""judo_amd.identify.PlantEstimator on the device: W recorded windows rolled out on the M plants of a set in one launch and scored by jh_plant_residuals.

The observed states of a case are jh_rollout_materialize on the true plant's OWN handle -- the reference, not the code under test.  The plants launch is bit for bit
that rollout (tests/test_gpu_materialize_plants.py, test_gpu_materialize_plants_fr3.py), so the true plant's error is exactly 0.0 in every window and needs no tolerance;
the other plants' errors are the numpy restatement's on the single-handle rollouts, bit for bit.  The plants, start states and controls are those tests'."""

import functools

import numpy as np
import pytest

from tests import test_gpu_materialize_plants as closed
from tests import test_gpu_materialize_plants_fr3 as arm

pytestmark = pytest.mark.gpu

TASKS = ["cartpole", "cylinder_push", "leap_cube", "fr3_pick"]
W, M = 4, 3
HORIZON = {"cartpole": 4, "cylinder_push": 4, "leap_cube": 4, "fr3_pick": 4}  # (a larger one, up to 8, only where `_reference`'s "plants differ" assertion needs it)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The case of a task, computed once and left unchanged: the three plants and their set, W start states and control windows, and every plant's own single-handle
    rollout of them, (W, H, nx) fp32 each.  Every two plants roll out differently: the evidence tells them apart."""
    import torch

    dev, H = torch.device("cuda", 0), HORIZON[name]
    if name == "fr3_pick":
        models, mset = list(arm._models(dev)[:M]), arm._set(dev, False, M)
        x0, controls = arm._x0(W, 3), arm._controls(W, H, 4)
    else:
        models, mset = closed._plants(name, True) if name == "leap_cube" else closed._plants(name)  # (the calls of that file: its cached plants)
        x0, controls = closed._x0(name, W, 3), closed._controls(name, W, H, 4)
    x0_d, controls_d = torch.from_numpy(x0).to(dev), torch.from_numpy(controls).to(dev)
    obs = [closed._single(m, x0_d, 1, controls_d, want_sensors=False)[0].cpu().numpy() for m in models]
    for a in range(M):
        assert np.isfinite(obs[a]).all()
        for b in range(a + 1, M):
            assert not np.array_equal(obs[a], obs[b]), f"{name}: plants {a} and {b} roll out alike at H = {H}: the case shows nothing"
    return dict(models=models, mset=mset, x0=x0, controls=controls, obs=obs, H=H)


def _estimator(ref, observed, **kw):
    from judo_amd.identify import PlantEstimator

    est = PlantEstimator(ref["mset"], horizon=ref["H"], windows=W, **kw)
    for w in range(W):
        est.observe(ref["x0"][w], ref["controls"][w], observed[w])
    assert len(est) == W
    return est


@pytest.mark.parametrize("name", TASKS)
def test_the_true_plant_has_error_zero_and_is_the_map(gpu, name):
    from judo_amd.identify import plant_residuals_host

    ref = _reference(name)
    nx, nq = ref["models"][0].nx, ref["models"][0].nq
    for j in range(M):
        est = _estimator(ref, ref["obs"][j])
        post = est.update()
        assert est.errors.shape == (M, W) and est.errors.dtype == np.float32
        assert np.array_equal(est.errors[j], np.zeros(W, dtype=np.float32)), f"{name}: true plant {j}: errors {est.errors[j]}"
        for m in range(M):
            assert m == j or est.errors[m].sum() > 0, f"{name}: plant {m} is told from true plant {j} by nothing"
        assert est.map == j and post.argmax() == j and not est.degenerate and abs(post.sum() - 1) < 1e-12
        want = plant_residuals_host(np.concatenate(ref["obs"]), ref["obs"][j], np.ones(nx, dtype=np.float32), est.quat_adr, nq=nq)
        np.testing.assert_array_equal(est.errors.view(np.uint32), want.view(np.uint32), err_msg=f"{name}: true plant {j}")
    assert est.quat_adr == ([] if name in ("cartpole", "cylinder_push") else [3])


@pytest.mark.parametrize("name", ["cartpole", "leap_cube"])
def test_the_map_survives_observation_noise(gpu, name):
    """Gaussian noise of standard deviation sigma, a tenth of the smallest root-mean-square state difference between any two plants on these windows, and
    state_sigma = sigma.  With d the difference between a wrong plant's prediction and the true one over the n = W * H * nx scalar samples, rms(d) >= 10 sigma, the
    log-likelihood gap is 0.5 * sum(d^2 - 2 d noise) / sigma^2: its mean is 0.5 * sum(d^2) / sigma^2 >= 50 n, its standard deviation sqrt(sum(d^2)) / sigma, which
    is 10 sqrt(n) at rms(d) = 10 sigma: 50 n against 10 sqrt(n) is decided by construction, not by luck."""
    ref = _reference(name)
    obs = ref["obs"]
    rms = min(float(np.sqrt(np.mean((obs[a].astype(np.float64) - obs[b]) ** 2))) for a in range(M) for b in range(a + 1, M))
    sigma = 0.1 * rms
    assert sigma > 0
    n = obs[0].size
    for j in range(M):
        noise = np.random.default_rng(100 + j).standard_normal(obs[j].shape)
        est = _estimator(ref, (obs[j] + sigma * noise).astype(np.float32), state_sigma=sigma)
        est.update()
        ll = est.log_likelihood
        gap = ll[j] - max(ll[m] for m in range(M) if m != j)
        print(f"{name}: true plant {j}: sigma = {sigma:.3e}, log-likelihood gap {gap:.1f} over n = {n} samples ({gap / n:.1f} per sample; expected at least about 50)")
        assert est.map == j and gap > 0 and np.isfinite(ll).all()


def _configure(c, n=32, steps=8):
    c.optimizer.config.num_rollouts = n
    c.controller_cfg.horizon = steps * c.task.dt
    c.controller_cfg.max_opt_iters = 1
    c.reset()
    c.current_state = c.task.default_state()


def _cartpole_descriptions():
    from judo_amd.models import scaled_description

    desc = closed._task("cartpole").desc
    return [desc] + [scaled_description(desc, **kw) for kw in closed.PLANTS["cartpole"]]


def test_for_controller_follows_set_member(gpu):
    """An estimator made with `for_controller` reads the controller's set on every update: after set_member(1, plant 2's description) plants 1 and 2 score alike."""
    from judo_amd.identify import PlantEstimator
    from judo_amd.randomized import make_randomized_controller

    ref = _reference("cartpole")
    descs = _cartpole_descriptions()
    ctrl = make_randomized_controller("cartpole", "mppi", descs)
    est = PlantEstimator.for_controller(ctrl, horizon=ref["H"], windows=W)
    for w in range(W):
        est.observe(ref["x0"][w], ref["controls"][w], ref["obs"][2][w])
    est.update()
    assert np.array_equal(est.errors[2], np.zeros(W, dtype=np.float32)) and (est.errors[1] > 0).all() and est.map == 2
    ctrl.set_member(1, descs[2])
    post = est.update()
    assert np.array_equal(est.errors[1], est.errors[2]) and np.array_equal(est.errors[1], np.zeros(W, dtype=np.float32)) and post[1] == post[2] and est.errors[0].sum() > 0


def test_non_finite_errors(gpu):
    """A non-finite error counts as +inf.  A window observed as NaN, through the public `observe`, is non-finite for EVERY plant: no member keeps a finite
    log-probability, the posterior is the prior and `degenerate` says so.  A prediction poisoned to NaN -- one plant's block of what the launch wrote -- gives that
    plant posterior exactly 0 and leaves the others their shares."""
    ref = _reference("cartpole")
    prior = [0.2, 0.3, 0.5]
    observed = [o.copy() for o in ref["obs"][0]]
    observed[2][:] = np.nan
    est = _estimator(ref, observed, prior=prior)
    post = est.update()
    assert est.degenerate and np.allclose(post, prior, rtol=1e-15, atol=0) and np.isnan(est.errors[:, 2]).all() and np.isfinite(np.delete(est.errors, 2, axis=1)).all()

    est = _estimator(ref, ref["obs"][0], prior=prior, state_sigma=1e-3)
    clean = est.update()
    predict = est._predict

    def poisoned():
        pred, obs = predict()
        pred[W + 1, 0, 0] = float("nan")  # plant 1's block, its window 1
        return pred, obs

    est._predict = poisoned
    post = est.update()
    assert np.isnan(est.errors[1, 1]) and np.isfinite(np.delete(est.errors, 1, axis=0)).all()
    assert post[1] == 0.0 and not est.degenerate and est.log_likelihood[1] == -np.inf
    np.testing.assert_allclose(post[[0, 2]], clean[[0, 2]] / clean[[0, 2]].sum(), rtol=1e-12)


def test_closed_loop_on_cartpole(gpu):
    """The truth is plant 2: 2 * horizon model steps on its own handle, one launch per step, fed through `observe_step`; the belief goes to a RandomizedController of
    8 blocks and 32 rollouts, whose next plan step runs on the new assignment.  The truth is noise-free, so state_sigma is small."""
    import torch

    from judo_amd.identify import PlantEstimator
    from judo_amd.randomized import make_randomized_controller

    ref = _reference("cartpole")
    H = ref["H"]
    ctrl = make_randomized_controller("cartpole", "mppi", _cartpole_descriptions(), blocks=8)
    _configure(ctrl)
    assert ctrl.assignment == [0, 1, 2, 0, 1, 2, 0, 1]
    ctrl.update_action()
    est = PlantEstimator.for_controller(ctrl, horizon=H, windows=W, state_sigma=1e-4)
    truth = ref["models"][2]
    x = torch.from_numpy(closed._x0("cartpole", 1, 9)[0]).to(gpu)
    us = torch.from_numpy(closed._controls("cartpole", 1, 2 * H, 10)).to(gpu)
    for t in range(2 * H):
        u = us[:, t : t + 1].contiguous()
        x_next = closed._single(truth, x, 0, u, want_sensors=False)[0][0, 0].clone()
        est.observe_step(x, u[0, 0], x_next)
        x = x_next
    assert len(est) == 2 and est.pending_steps == 0
    w = est.apply(ctrl, floor=0.25)
    assert est.map == 2 and est.posterior[2] > 0.99, (est.posterior, est.errors)
    np.testing.assert_allclose(w, [1 / 12, 1 / 12, 10 / 12], atol=0.01)
    assert ctrl.assignment == [0, 1, 2, 2, 2, 2, 2, 2]
    ctrl.update_action()
    torch.cuda.synchronize()
    assert np.isfinite(ctrl.nominal_knots).all() and list(ctrl.plant_of_rollout) == [0] * 4 + [1] * 4 + [2] * 24
