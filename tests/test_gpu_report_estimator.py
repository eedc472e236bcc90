"""judo_amd.reports.ReportEstimator on the device: W recorded windows rolled out on the M plants of a set in one launch and scored by jh_plant_residuals_reports over
the entries a robot reported.

The plants, start states, controls and single-handle rollouts are those of tests/test_gpu_plant_estimator.py (`_reference`: jh_rollout_materialize on every plant's OWN
handle -- the reference, not the code under test), thinned here: (a) every second step, no velocities; (b) on fr3_pick no state at all, the sensors the only evidence.
The plants launch is bit for bit the single-handle rollout, so the true plant's error is exactly 0.0 in every window and needs no tolerance; the other plants' errors are
the numpy restatement's, bit for bit."""

import functools

import numpy as np
import pytest

from tests import test_gpu_materialize_plants as closed
from tests.test_gpu_plant_estimator import M, W, _reference

pytestmark = pytest.mark.gpu

TASKS = ["cartpole", "leap_cube", "fr3_pick"]


def _thinned(ref, j):
    """Plant j's rollouts as a robot would report them: steps 1 and 3 (every second step), positions only."""
    nq = ref["models"][0].nq
    obs = ref["obs"][j].copy()
    obs[:, 0::2] = np.nan
    obs[..., nq:] = np.nan
    return obs


@functools.lru_cache(maxsize=None)
def _sensors(name):
    """Every plant's own single-handle sensor rows for the case's windows, (W, H, ns) fp32 each: computed once, left unchanged."""
    import torch

    ref = _reference(name)
    dev = ref["models"][0].device
    x0_d, controls_d = torch.from_numpy(ref["x0"]).to(dev), torch.from_numpy(ref["controls"]).to(dev)
    return [closed._single(m, x0_d, 1, controls_d, want_states=False)[1].cpu().numpy() for m in ref["models"]]


def _estimator(ref, observed, sensors=None, **kw):
    from judo_amd.reports import ReportEstimator

    est = ReportEstimator(ref["mset"], horizon=ref["H"], windows=W, **kw)
    for w in range(W):
        est.observe(ref["x0"][w], ref["controls"][w], observed[w], None if sensors is None else sensors[w])
    assert len(est) == W
    return est


def _assert_identified(est, j, want, what):
    post = est.update()
    assert est.errors.shape == (M, W) and est.errors.dtype == np.float32
    assert np.array_equal(est.errors[j], np.zeros(W, dtype=np.float32)), f"{what}: true plant {j}: errors {est.errors[j]}"
    for m in range(M):
        assert m == j or est.errors[m].sum() > 0, f"{what}: plant {m} is told from true plant {j} by nothing"
    assert est.map == j and post.argmax() == j and not est.degenerate and abs(post.sum() - 1) < 1e-12
    np.testing.assert_array_equal(est.errors.view(np.uint32), want.view(np.uint32), err_msg=f"{what}: true plant {j}")


@pytest.mark.parametrize("name", TASKS)
def test_the_true_plant_is_identified_from_every_second_step_without_velocities(gpu, name):
    from judo_amd.reports import plant_residuals_reports_host

    ref = _reference(name)
    nx, nq, H = ref["models"][0].nx, ref["models"][0].nq, ref["H"]
    thin = [_thinned(ref, j) for j in range(M)]
    for a in range(M):  # the condition of the test: every two plants differ in the reported entries
        for b in range(a + 1, M):
            assert not np.array_equal(thin[a], thin[b], equal_nan=True), f"{name}: plants {a} and {b} report alike at steps 1 and 3: the case shows nothing"
    for j in range(M):
        est = _estimator(ref, thin[j])
        assert est.reported.tolist() == [(H // 2) * nq] * W
        want = plant_residuals_reports_host(np.concatenate(ref["obs"]), thin[j], np.ones(nx, dtype=np.float32), est.quat_adr, nq=nq)
        _assert_identified(est, j, want, name)


def test_sensors_alone_identify_the_arm(gpu):
    """fr3_pick with no state reported at all: the 14 sensor readings of every step are the evidence."""
    from judo_amd.reports import plant_residuals_reports_host

    ref, sens = _reference("fr3_pick"), _sensors("fr3_pick")
    nx, nq, H = ref["models"][0].nx, ref["models"][0].nq, ref["H"]
    ns = sens[0].shape[-1]
    for a in range(M):
        assert np.isfinite(sens[a]).all()
        for b in range(a + 1, M):
            assert not np.array_equal(sens[a], sens[b]), f"plants {a} and {b} read alike: the case shows nothing"
    nothing = np.full((W, H, nx), np.nan, dtype=np.float32)
    for j in range(M):
        est = _estimator(ref, nothing, sens[j], sensor_sigma=0.5)
        assert est.reported.tolist() == [H * ns] * W
        want = plant_residuals_reports_host(np.concatenate(ref["obs"]), nothing, np.ones(nx, dtype=np.float32), est.quat_adr, nq=nq, pred_sens=np.concatenate(sens),
                                            obs_sens=sens[j], weight_sens=np.full(ns, 4.0, dtype=np.float32))
        _assert_identified(est, j, want, "fr3_pick, sensors alone")
    # states and sensors together, the sensors dropped on every second step: the sum continues behind the state's terms
    y = sens[1].copy()
    y[:, 1::2] = np.nan
    est = _estimator(ref, _thinned(ref, 1), y, sensor_sigma=0.5)
    want = plant_residuals_reports_host(np.concatenate(ref["obs"]), _thinned(ref, 1), np.ones(nx, dtype=np.float32), est.quat_adr, nq=nq, pred_sens=np.concatenate(sens),
                                        obs_sens=y, weight_sens=np.full(ns, 4.0, dtype=np.float32))
    _assert_identified(est, 1, want, "fr3_pick, states and sensors")
    # a window with nothing reported is no evidence: exactly 0.0 for every plant
    est = _estimator(ref, nothing, sensor_sigma=0.5)
    est.update()
    assert np.array_equal(est.errors, np.zeros((M, W), dtype=np.float32)) and est.reported.tolist() == [0] * W and np.allclose(est.posterior, 1 / M, rtol=1e-15)


@pytest.mark.parametrize("name", TASKS)
def test_nothing_thinned_is_the_plant_estimator(gpu, name):
    from judo_amd.identify import PlantEstimator

    ref = _reference(name)
    for j in (0, M - 1):
        new = _estimator(ref, ref["obs"][j], state_sigma=0.5, prior=[0.2, 0.3, 0.5])
        old = PlantEstimator(ref["mset"], horizon=ref["H"], windows=W, state_sigma=0.5, prior=[0.2, 0.3, 0.5])
        for w in range(W):
            old.observe(ref["x0"][w], ref["controls"][w], ref["obs"][j][w])
        p_new, p_old = new.update(), old.update()
        assert new.errors.tobytes() == old.errors.tobytes() and p_new.tobytes() == p_old.tobytes() and new.log_likelihood.tobytes() == old.log_likelihood.tobytes()
        assert new.map == old.map and np.array_equal(old.errors[j], np.zeros(W, dtype=np.float32)) and (np.delete(old.errors, j, axis=0).sum(axis=1) > 0).all()


def test_start_and_step_record_what_observe_records(gpu):
    """Two windows of cartpole fed a model step at a time -- a report on every second step, positions only, the window's last a full state -- against `observe`."""
    ref = _reference("cartpole")
    H, nq = ref["H"], ref["models"][0].nq
    truth = ref["obs"][2]
    from judo_amd.reports import ReportEstimator

    est = ReportEstimator(ref["mset"], horizon=H, windows=W)
    for w in range(2):
        est.start(ref["x0"][w])
        for t in range(H):
            report = truth[w, t].copy()
            if t < H - 1:
                report[nq:] = np.nan
            est.step(ref["controls"][w, t], report if t % 2 else None)
        assert not est.needs_start and len(est) == w + 1
    obs = truth[:2].copy()
    obs[:, 0::2] = np.nan
    obs[:, :-1, nq:] = np.nan
    other = ReportEstimator(ref["mset"], horizon=H, windows=W)
    for w in range(2):
        other.observe(ref["x0"][w], ref["controls"][w], obs[w])
    for a, b in zip(est.recorded(), other.recorded()):
        assert a.tobytes() == b.tobytes()
    assert est.reported.tolist() == other.reported.tolist() == [nq + 2 * nq] * 2
    assert est.update().tobytes() == other.update().tobytes() and est.errors.tobytes() == other.errors.tobytes()
    assert est.map == 2 and np.array_equal(est.errors[2], np.zeros(2, dtype=np.float32)) and (est.errors[:2].sum(axis=1) > 0).all()


def test_for_controller_and_the_hand_over(gpu):
    """`for_controller` reads the controller's set on every update, and `apply` hands a randomised controller the posterior of thinned reports."""
    from judo_amd.randomized import make_randomized_controller
    from judo_amd.reports import ReportEstimator
    from tests.test_gpu_plant_estimator import _cartpole_descriptions

    ref = _reference("cartpole")
    descs = _cartpole_descriptions()
    ctrl = make_randomized_controller("cartpole", "mppi", descs, blocks=8)
    est = ReportEstimator.for_controller(ctrl, horizon=ref["H"], windows=W, state_sigma=1e-4)
    thin = _thinned(ref, 2)
    for w in range(W):
        est.observe(ref["x0"][w], ref["controls"][w], thin[w])
    w8 = est.apply(ctrl, floor=0.25)
    assert est.map == 2 and np.array_equal(est.errors[2], np.zeros(W, dtype=np.float32)) and (est.errors[1] > 0).all()
    np.testing.assert_allclose(w8, [1 / 12, 1 / 12, 10 / 12], atol=0.01)
    assert ctrl.assignment == [0, 1, 2, 2, 2, 2, 2, 2]
    ctrl.set_member(1, descs[2])
    post = est.update()
    assert np.array_equal(est.errors[1], est.errors[2]) and post[1] == post[2] and est.errors[0].sum() > 0
