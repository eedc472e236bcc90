"""FR3Fleet: B fr3_pick controllers, each in its own phase, planned in one launch leave every member bit for bit where its own update_action() would have left it."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, H, TRACES = 32, 8, 3
CUBES = ([0.7, 0.0, 0.02], [0.7, 0.0, 0.05], [0.6, 0.4, 0.05], [0.6, 0.4, 0.02])  # the four phase states: LIFT, MOVE, PLACE, HOMING


def _configure(c, i, n=N, iters=1):
    """Member i of a fleet, or the lone controller it is compared with: the same configuration from the same numbers."""
    c.optimizer.config.num_rollouts = n
    c.controller_cfg.horizon = H * c.task.dt
    c.controller_cfg.max_num_traces = TRACES
    c.controller_cfg.max_opt_iters = iters
    c.solver_warnings = False
    c.reset()
    assert c.num_timesteps == H and c.max_opt_iters == iters
    c.optimizer.seed(i)


def _set_state(c, i, step, cube=None):
    """The state the plant reports to member i before plan step `step`, and its time: phase state i % 4, the arm a little off the home pose."""
    rng = np.random.default_rng(1000 * i + step)
    x = c.task.default_state()
    x[7:14] += 0.02 * rng.standard_normal(7)
    x[0:3] = CUBES[i % 4] if cube is None else cube
    c.update_states(x[: c.task.nq], x[c.task.nq :], 0.03 * step + 0.001 * i, {})


def _snapshot(c):
    t = c.time + 0.5 * c.task.dt
    return dict(nominal=c.nominal_knots.copy(), times=np.array(c.times), traces=c.traces.copy(), rewards=np.array(c.rewards), sigma=np.atleast_1d(np.asarray(getattr(c.optimizer, "sigma", 0.0))).copy(),
                action=np.array(c.action(t)), phase=np.array([c.task.phase]))


def _assert_same(a, b, what):
    for key in a:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, key)
        assert x.tobytes() == y.tobytes(), f"{what}: {key} differs (max |d| = {np.abs(x - y).max():.3e})"


def _lone(opt, self_collision=False):
    from judo_amd.controller import make_controller_for
    from judo_amd.tasks import FR3Pick

    return make_controller_for(FR3Pick(self_collision=self_collision), opt)


def _run(fleet, alone, steps, what, lifted=None):
    """`steps` plan steps with time advancing, the fleet against the lone controllers; before step 1 the cube of member `lifted` is raised to z = 0.05."""
    B = len(fleet)
    for step in range(steps):
        for i in range(B):
            cube = [0.7, 0.0, 0.05] if (i == lifted and step >= 1) else None
            _set_state(fleet[i], i, step, cube)
            _set_state(alone[i], i, step, cube)
        fleet.update_action()
        for i in range(B):
            alone[i].update_action()
            _assert_same(_snapshot(fleet[i]), _snapshot(alone[i]), f"{what} member {i} step {step}")
        yield step


@pytest.mark.parametrize("opt", ["cem", "mppi"])
def test_fleet_equals_lone_controllers_in_four_phases(gpu, opt):
    """Four members in the four phase states, seeds 0..3; two plan steps, and between them member 0's cube is lifted: its phase goes from LIFT to MOVE."""
    from judo_amd.fr3_fleet import FR3Fleet, make_fr3_fleet

    fleet = make_fr3_fleet(opt, 4)
    assert isinstance(fleet, FR3Fleet) and len(fleet) == 4 and all(c.model is fleet.model for c in fleet)
    alone = [_lone(opt) for _ in range(4)]
    for i in range(4):
        _configure(fleet[i], i)
        _configure(alone[i], i)
    for step in _run(fleet, alone, 2, opt, lifted=0):
        assert [c.task.phase for c in fleet] == ([0, 1, 2, 3] if step == 0 else [1, 1, 2, 3])
        assert fleet[0].traces.shape[0] == TRACES * len(fleet[0].trace_sensors) * (H - 1)
    assert len({np.asarray(c.rewards).tobytes() for c in fleet}) == 4  # the members planned different problems


def test_two_optimizer_iterations_per_plan_step(gpu):
    from judo_amd.fr3_fleet import make_fr3_fleet

    fleet = make_fr3_fleet("cem", 4)
    alone = [_lone("cem") for _ in range(4)]
    for i in range(4):
        _configure(fleet[i], i, iters=2)
        _configure(alone[i], i, iters=2)
    for _ in _run(fleet, alone, 2, "max_opt_iters=2", lifted=0):
        pass


def test_self_collision_fleet(gpu):
    from judo_amd.fr3_fleet import make_fr3_fleet

    fleet = make_fr3_fleet("cem", 2, self_collision=True)
    assert fleet.model.fr3_build()["self_collision_build"] and fleet.model.build()["kernel_generation"] == 3
    alone = [_lone("cem", self_collision=True) for _ in range(2)]
    for i in range(2):
        _configure(fleet[i], i)
        _configure(alone[i], i)
    for _ in _run(fleet, alone, 2, "self-collision"):
        pass


def test_fleet_of_one_and_a_member_that_goes_on_alone(gpu):
    from judo_amd.fr3_fleet import make_fr3_fleet

    fleet = make_fr3_fleet("mppi", 1)
    alone = [_lone("mppi")]
    _configure(fleet[0], 2)
    _configure(alone[0], 2)
    for i, step in ((2, 0), (2, 1)):
        _set_state(fleet[0], i, step)
        _set_state(alone[0], i, step)
        fleet.update_action()
        alone[0].update_action()
        _assert_same(_snapshot(fleet[0]), _snapshot(alone[0]), f"fleet of one step {step}")
    member = fleet[0]
    _set_state(member, 2, 2)
    _set_state(alone[0], 2, 2)
    member.update_action()  # (the member on its own: jh_plan_step with its phase as the argument)
    alone[0].update_action()
    _assert_same(_snapshot(member), _snapshot(alone[0]), "the member on its own")


def test_refusals(gpu):
    from judo_amd.controller import make_controller, make_controller_for
    from judo_amd.fleet import ControllerFleet
    from judo_amd.fr3_fleet import FR3Fleet
    from judo_amd.models import layout, scaled_description
    from judo_amd.tasks import FR3Pick

    a = _lone("mppi")
    with pytest.raises(ValueError, match="self_collision"):
        FR3Fleet([a, _lone("mppi", self_collision=True)])
    with pytest.raises(ValueError, match="fr3_pick"):
        FR3Fleet([a, make_controller("leap_cube", "mppi")])
    t = FR3Pick()
    t.desc = scaled_description(t.desc, actuator_kp={None: 1.1})
    t._layout, t._ctrlrange, t._jadr = layout(t.desc), None, None
    with pytest.raises(ValueError, match="model set per problem.*not available for fr3_pick"):
        FR3Fleet([a, make_controller_for(t, "mppi")])
    b = _lone("mppi")
    b.optimizer.config.num_rollouts = a.optimizer.num_rollouts + 1
    with pytest.raises(ValueError, match="num_rollouts"):
        FR3Fleet([a, b])
    c = _lone("mppi")
    c.keep_candidates = True
    with pytest.raises(ValueError, match="keep_candidates"):
        FR3Fleet([a, c])
    with pytest.raises(ValueError, match="fr3_pick"):
        ControllerFleet([a, _lone("mppi")])
    with pytest.raises(ValueError):
        FR3Fleet([])
    assert len(FR3Fleet([a, _lone("mppi")])) == 2
