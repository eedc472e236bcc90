"""jh_plants_advance through judo_amd.simulation.PlantFleet and through the C ABI: B plants of a model set advance S steps on their splines in one call.

The reference is jh_rollout_materialize on every plant's OWN handle (tests/test_gpu_materialize_plants.py `_single`) with the controls of the numpy restatement
`plant_controls_host` -- not the code under test.  Sets of three plants as tests/test_gpu_plant_estimator.py builds them; truth = [2, 0, 2] repeats a plant and is out
of order; S = 1 and S = 5; every comparison is bit for bit."""

import ctypes as C
import functools

import numpy as np
import pytest

from tests import test_gpu_materialize_plants as closed
from tests import test_gpu_materialize_plants_fr3 as arm

pytestmark = pytest.mark.gpu

INVALID = -1
POISON = -7.0
TASKS = ["cartpole", "leap_cube", "fr3_pick"]
TRUTH = [2, 0, 2]
K = 4


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The three plants and their set (the estimator tests' cached ones), a start state per plant of the fleet -- leap_cube's with the cube resting on the fingers -- and K = 4
    knots per plant near the task's home controls.  Computed once, left unchanged."""
    from tests.test_gpu_plant_estimator import _reference

    ref = _reference(name)
    B = len(TRUTH)
    if name == "fr3_pick":
        x0, knots = arm._x0(B, 5), arm._controls(B, K, 6)
    else:
        x0, knots = closed._x0(name, B, 5), closed._controls(name, B, K, 6)
    return dict(models=ref["models"], mset=ref["mset"], x0=x0, knots=knots)


def _splines(case, t0, kind="cubic"):
    """Plant b's spline: its knot grid starts 0.3 dt after plant b - 1's, the knots the case's."""
    from judo_amd.structs import SplineData

    dt = case["models"][0].dt
    return [SplineData(t0 + 0.3 * dt * b + np.linspace(0.0, 6 * dt, K), case["knots"][b].astype(np.float64), kind) for b in range(len(TRUTH))]


def _own_handle(case, x, controls, want_sensors=True):
    """(states (B, S, nx), sensors (B, S, ns)) fp32 on the host: plant TRUTH[b]'s own jh_rollout_materialize from x[b] with controls[b], one launch per plant."""
    import torch

    dev = case["models"][0].device
    out = [closed._single(case["models"][p], torch.from_numpy(np.ascontiguousarray(x[b])).to(dev), 0, torch.from_numpy(np.ascontiguousarray(controls[b : b + 1])).to(dev))
           for b, p in enumerate(TRUTH)]
    return np.concatenate([s.cpu().numpy() for s, _ in out]), np.concatenate([y.cpu().numpy() for _, y in out])


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("name", TASKS)
def test_two_advances_equal_the_plants_own_launches(gpu, name, S):
    """Controls bit for bit the restatement; states and sensors bit for bit the own-handle launches; a second advance continues from the carried state and the advanced
    clocks, as two own-handle launches chained through that state do."""
    from judo_amd.simulation import PlantFleet, plant_controls_host, spline_rows

    case = _case(name)
    fleet = PlantFleet(case["mset"], TRUTH, case["x0"])
    splines = _splines(case, 0.0)
    x, count, seen = case["x0"], 0, []
    for seg in range(2):
        assert fleet.steps_taken.tolist() == [count] * 3 and np.array_equal(fleet.time, count * fleet.dt * np.ones(3))
        fleet.advance(splines, S)
        controls = plant_controls_host(*spline_rows(splines, np.full(3, count * fleet.dt), fleet.dt, 0, S))
        states, sensors = _own_handle(case, x, controls)
        assert np.isfinite(states).all() and np.isfinite(sensors).all()
        for got, want, what in ((fleet.controls, controls, "controls"), (fleet.states, states, "states"), (fleet.sensors, sensors, "sensors")):
            np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want), err_msg=f"{name} S={S} segment {seg}: {what}")
        x = states[:, -1]
        np.testing.assert_array_equal(_bits(fleet.x_host()), _bits(x), err_msg="the carried state")
        assert fleet.reported_states is None
        seen.append(states)
        count += S
    assert not np.array_equal(seen[0][0], seen[0][2]) or not np.array_equal(case["x0"][0], case["x0"][2])
    assert not np.array_equal(seen[0], seen[1])  # the second segment went on
    if S == 5:  # plants 0 and 2 are the same member from different states; plant 1 is another member: the table matters
        other = _own_handle(dict(case, models=[case["models"][0]] * 3), case["x0"], plant_controls_host(*spline_rows(splines, np.zeros(3), fleet.dt, 0, S)))[0]
        assert not np.array_equal(other[0], seen[0][0]), f"{name}: plants 2 and 0 roll out alike: the case shows nothing"


@pytest.mark.parametrize("name", TASKS)
def test_reports_equal_the_restatement(gpu, name):
    """every = 1, 2, 3 with S = 5 over two segments (the stride carries), with and without velocities, sigma zero and nonzero, the sensors too: bit for bit
    `plant_reports_host` on the segment's own states and the noise the call drew; with everything reported and no noise the reports are the states bit for bit."""
    from judo_amd.simulation import PlantFleet, plant_reports_host

    case = _case(name)
    nq, nx, ns = case["models"][0].nq, case["models"][0].nx, case["models"][0].ns
    S = 5
    for every in (1, 2, 3):
        for velocities in (True, False):
            for sigma in (None, 0.0, 0.01):
                fleet = PlantFleet(case["mset"], TRUTH, case["x0"])
                cols = None if velocities else range(nq)
                ssig = None if sigma is None else np.linspace(sigma, 2 * sigma, ns)
                fleet.reports(every=every, columns=cols, state_sigma=sigma, sensor_sigma=ssig, seed=11, sensor_columns=None if velocities else range(0, ns, 2))
                for seg in range(2):
                    count = fleet.steps_taken.copy()
                    fleet.advance(_splines(case, 0.0, "linear"), S)
                    states, sensors = fleet.states.cpu().numpy(), fleet.sensors.cpu().numpy()
                    what = f"{name} every={every} velocities={velocities} sigma={sigma} segment {seg}"
                    noise = None if sigma is None else fleet.last_noise.cpu().numpy()
                    want, carry = plant_reports_host(states, count, every, None if cols is None else np.arange(nx) < nq, None if sigma is None else np.full(nx, sigma), noise)
                    got = fleet.reported_states.cpu().numpy()
                    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)
                    np.testing.assert_array_equal(_bits(fleet.x_host()), _bits(carry), err_msg=what + ": the carry is the exact state")
                    noise_s = None if sigma is None else fleet.last_sensor_noise.cpu().numpy()
                    want_s, _ = plant_reports_host(sensors, count, every, None if velocities else np.arange(ns) % 2 == 0, ssig, noise_s)
                    np.testing.assert_array_equal(_bits(fleet.reported_sensors.cpu().numpy()), _bits(want_s), err_msg=what + ": sensors")
                    if every == 1 and velocities and sigma is None:
                        assert _bits(got).tobytes() == _bits(states).tobytes() and _bits(fleet.reported_sensors.cpu().numpy()).tobytes() == _bits(sensors).tobytes()
                    elif sigma:
                        shown = ~np.isnan(got)
                        assert shown.any() and (got[shown] != states[shown]).any(), what + ": the noise changed nothing"
                    assert np.isnan(got).sum() == got.size - int(((count[:, None] + np.arange(S) + 1) % every == 0).sum()) * (nx if velocities else nq)
                assert fleet.report_settings["draws"] == (0 if sigma is None else 4)  # a fresh draw per segment, states and sensors


def _raw(case, **change):
    """One raw jh_plants_advance call on poisoned outputs with `change` applied to otherwise valid arguments; returns (status, message, outputs)."""
    import torch

    from judo_amd import _lib
    from judo_amd.device import current_stream_ptr

    dev, m = case["models"][0].device, case["models"][0]
    B, S = 3, 5
    a = dict(set=case["mset"].handle, truth=TRUTH, B=B, x=torch.from_numpy(case["x0"]).to(dev), W=torch.zeros((B, S, K), device=dev), knots=torch.from_numpy(case["knots"]).to(dev),
             knot_stride=K * m.nu, K=K, lohi=None, step0=0, S=S, controls=torch.full((B, S, m.nu), POISON, device=dev), states=torch.full((B, S, m.nx), POISON, device=dev),
             sensors=torch.full((B, S, m.ns), POISON, device=dev), count=[0] * B, every=1, reports=None, reports_sens=None)
    a.update(change)
    ints = lambda v: None if v is None else (C.c_int * max(len(v), 1))(*v)
    st = _lib.lib().jh_plants_advance(a["set"], ints(a["truth"]), a["B"], _lib.ptr(a["x"]), _lib.ptr(a["W"]), _lib.ptr(a["knots"]), a["knot_stride"], a["K"], _lib.ptr(a["lohi"]),
                                      a["step0"], a["S"], _lib.ptr(a["controls"]), _lib.ptr(a["states"]), _lib.ptr(a["sensors"]), ints(a["count"]), a["every"], None, None, None,
                                      _lib.ptr(a["reports"]), None, None, None, _lib.ptr(a["reports_sens"]), current_stream_ptr())
    return st, _lib.lib().jh_last_error().decode(), a


@pytest.mark.parametrize("name", ["cartpole", "fr3_pick"])
def test_every_refusal_stands_in_front_of_the_first_enqueue(gpu, name):
    import torch

    case = _case(name)
    nu = case["models"][0].nu
    st, _, a = _raw(case)
    assert st == 0 and not (a["states"] == POISON).any()  # the arguments the refusals start from are valid
    for change, word in ((dict(set=None), "set is a null pointer"), (dict(truth=None), "truth is a null pointer"), (dict(x=None), "x is a null pointer"), (dict(W=None), "W is a null pointer"),
                         (dict(knots=None), "knots is a null pointer"), (dict(controls=None), "controls is a null pointer"), (dict(states=None), "states is a null pointer"),
                         (dict(count=None), "count is a null pointer"), (dict(B=0), "B = 0"), (dict(B=257, truth=[0] * 257, count=[0] * 257), "JH_MAX_FLEET_PLANT_BLOCKS"),
                         (dict(S=0), "S = 0"), (dict(K=0), "K = 0"), (dict(K=512 // nu + 1), "JH_MAX_KNOT_DIM"), (dict(knot_stride=K * nu - 1), "knot_stride"),
                         (dict(truth=[2, 3, 0]), "truth[1] = 3"), (dict(truth=[-1, 0, 0]), "truth[0] = -1"), (dict(every=0), "every = 0"), (dict(step0=5), "step0 = 5"),
                         (dict(step0=-1), "step0 = -1"), (dict(count=[0, -2, 0]), "count[1] = -2"),
                         (dict(sensors=None, reports_sens=torch.zeros(1, device=case["models"][0].device)), "reports_sens")):
        st, msg, a = _raw(case, **change)
        assert st == INVALID and word in msg and msg.startswith("plants_advance:"), (change, st, msg)
        torch.cuda.synchronize()
        for out in ("controls", "states", "sensors"):
            assert a[out] is None or (a[out] == POISON).all(), f"{change}: {out} was written: something was enqueued before the refusal"
    # sensors may be NULL: states alone, still the own-handle bits
    st, _, a = _raw(case, sensors=None, W=torch.ones((3, 5, K), device=case["models"][0].device) / K)
    assert st == 0
    want = _own_handle(case, case["x0"], a["controls"].cpu().numpy())[0]
    np.testing.assert_array_equal(_bits(a["states"].cpu().numpy()), _bits(want))
