"""fr3_pick on a model set through the public classes: an FR3PlantFleet (B arms on B plants, one launch) leaves every member bit for bit where its own update_action()
on its own plant would have left it, and an FR3RandomizedController (one arm, its candidates spread over M plants) rolls block g out as a plain controller on plant
assignment[g] does.  No tolerance anywhere.  The plants are D0..D3 of tests/test_fr3_plants_host.py."""

import copy

import numpy as np
import pytest

from tests.test_fr3_plants_host import plants
from tests.test_gpu_fr3_fleet import H, TRACES, _assert_same, _configure, _set_state, _snapshot
from tests.test_gpu_randomized_controller import _update_fused

pytestmark = pytest.mark.gpu

N_RND = 64


def _lone_on(desc, opt):
    """A plain controller on the plant `desc`."""
    from judo_amd.controller import make_controller_for
    from judo_amd.models import layout
    from judo_amd.tasks import FR3Pick

    t = FR3Pick()
    t.desc = desc
    t._layout, t._ctrlrange, t._jadr = layout(desc), None, None
    return make_controller_for(t, opt)


def _snap(c):
    s = _snapshot(c)
    g = c.optimizer._generator
    # the position of the noise stream: the draws a plan step has used (a lone controller may hold the next one already, drawn behind its last download)
    ahead = getattr(c, "_noise_ahead", None)
    s["noise stream"] = np.array([-1 if g is None else g.draws - (ahead is not None and ahead[1] is g)])
    return s


# ------------------------------------------------------------------------------------------------ 1. the plant fleet
def test_plant_fleet_equals_lone_controllers_on_their_plants(gpu):
    """make_fr3_fleet("cem", 3, descriptions=[D1, D2, D3]); two plan steps, the members in the phases LIFT, MOVE, PLACE and member 0's cube lifted between them (LIFT ->
    MOVE); then member 1 leaves the fleet and goes on alone."""
    from judo_amd.fr3_fleet import FR3Fleet, FR3PlantFleet, make_fr3_fleet

    descs = list(plants()[1:])
    fleet = make_fr3_fleet("cem", 3, descriptions=descs)
    assert isinstance(fleet, FR3PlantFleet) and len(fleet) == 3 and len({id(c.model) for c in fleet}) == 3
    assert all(c.model.desc is d for c, d in zip(fleet, descs))
    alone = [_lone_on(d, "cem") for d in descs]
    nominal_plant = _lone_on(plants()[0], "cem")  # member 0's twin on D0: the plant must matter
    for i in range(3):
        _configure(fleet[i], i)
        _configure(alone[i], i)
    _configure(nominal_plant, 0)
    for step in range(2):
        for i in range(3):
            cube = [0.7, 0.0, 0.05] if (i == 0 and step >= 1) else None
            _set_state(fleet[i], i, step, cube)
            _set_state(alone[i], i, step, cube)
        fleet.update_action()
        assert fleet._model_set is not None and fleet._model_set.fr3 and fleet._model_set.info()["distinct_from_first"] == 2
        for i in range(3):
            alone[i].update_action()
            _assert_same(_snap(fleet[i]), _snap(alone[i]), f"member {i} step {step}")
        assert [c.task.phase for c in fleet] == ([0, 1, 2] if step == 0 else [1, 1, 2])
        if step == 0:
            _set_state(nominal_plant, 0, 0)
            nominal_plant.update_action()
            assert (np.asarray(nominal_plant.rewards) != np.asarray(fleet[0].rewards)).any()
    member = fleet[1]
    _set_state(member, 1, 2)
    _set_state(alone[1], 1, 2)
    member.update_action()  # (the member on its own: jh_plan_step on its own model with its phase as the argument)
    alone[1].update_action()
    _assert_same(_snap(member), _snap(alone[1]), "the member on its own")
    # without descriptions the fleet is the one-image FR3Fleet it was
    plain = make_fr3_fleet("cem", 2)
    assert type(plain) is FR3Fleet and plain[1].model is plain[0].model


def test_plant_fleet_refusals(gpu):
    from judo_amd.fr3_fleet import FR3Fleet, FR3PlantFleet
    from judo_amd.models import scaled_description

    d = plants()
    a, b = _lone_on(d[0], "mppi"), _lone_on(d[1], "mppi")
    with pytest.raises(ValueError, match="model set per problem.*not available for fr3_pick.*FR3PlantFleet"):
        FR3Fleet([a, b])
    assert len(FR3PlantFleet([a, b])) == 2
    other = _lone_on(dict(scaled_description(d[0]), geoms=d[0]["geoms"][:-1]), "mppi")  # a geom less: another int section
    with pytest.raises(ValueError, match="fleet member 1 has another model image or kernel build"):
        FR3PlantFleet([a, other])
    from judo_amd.controller import make_controller_for
    from judo_amd.tasks import FR3Pick

    with pytest.raises(ValueError, match="self_collision"):
        FR3PlantFleet([a, make_controller_for(FR3Pick(self_collision=True), "mppi")])


# ------------------------------------------------------------------------------------------------ 2. the randomised controller
def _inject(cs, seed=3):
    """The same injected noise for every controller of `cs` (reference layout (N - 1, K, nu))."""
    c = cs[0]
    noise = np.random.default_rng(seed).standard_normal((N_RND - 1, c.optimizer.num_nodes, c.nu)).astype(np.float32)
    for c in cs:
        c.optimizer.injected_noise = noise


def _stitch(plains, a):
    nb = N_RND // len(a)
    return np.concatenate([np.asarray(plains[p].rewards)[g * nb : (g + 1) * nb] for g, p in enumerate(a)])


def test_randomized_controller_blocks_equal_lone_controllers(gpu):
    """make_fr3_randomized_controller("mppi", [D0, D1, D2], blocks=4, weights=[2, 1, 1]), 64 rollouts, H = 8: the assignment is [0, 0, 1, 2]; block g of the rewards is that
    block of a lone controller on plant assignment[g] with the same injected noise, in the phase the state selects; an assignment set between the steps takes effect at
    the next; a plant without a block has a NaN mean."""
    from judo_amd.fr3_randomized import FR3RandomizedController, make_fr3_randomized_controller

    descs = list(plants()[:3])
    rn = make_fr3_randomized_controller("mppi", descs, blocks=4, weights=[2, 1, 1])
    assert isinstance(rn, FR3RandomizedController) and rn.assignment == [0, 0, 1, 2] and rn.num_members == 3 and rn.model_set.fr3
    plains = [_lone_on(d, "mppi") for d in descs]
    cs = [rn] + plains
    for c in cs:
        _configure(c, 5, n=N_RND)
    _inject(cs)
    for c in cs:
        _set_state(c, 2, 0)  # the cube above the goal: PLACE
        c.update_action()
    assert rn.task.phase == 2 and all(p.task.phase == 2 for p in plains)
    assert len({np.asarray(p.rewards).tobytes() for p in plains}) == 3  # the plants matter
    want = _stitch(plains, [0, 0, 1, 2])
    _assert_same(dict(rewards=np.asarray(rn.rewards)), dict(rewards=want), "step 0: rewards against the lone controllers' blocks")
    assert rn.rewards[0] == plains[0].rewards[0] and rn.rewards[32] != plains[1].rewards[0]  # only global rollout 0 drops its noise
    _assert_same(dict(nominal=rn.nominal_knots), dict(nominal=_update_fused(rn, want)), "step 0: nominal_knots against jh_update_fused on the stitched rewards")
    assert rn.plant_of_rollout.tolist() == [0] * 32 + [1] * 16 + [2] * 16
    assert rn.traces.shape[0] == TRACES * len(rn.trace_sensors) * (H - 1) and np.isfinite(rn.traces).all()
    # an assignment re-drawn between the steps; the lone controllers follow the randomised one's nominal and stay comparable through the shared noise
    rn.assignment = [2, 1, 0, 2]
    for p in plains:
        p.nominal_knots, p.times = rn.nominal_knots.copy(), rn.times.copy()
        p.update_spline(p.times, p.nominal_knots)
    for c in cs:
        _set_state(c, 1, 1)  # the cube lifted: MOVE
        c.update_action()
    assert rn.task.phase == 1
    _assert_same(dict(rewards=np.asarray(rn.rewards)), dict(rewards=_stitch(plains, [2, 1, 0, 2])), "step 1: the assignment set between the steps")
    assert rn.plant_of_rollout.tolist() == [2] * 16 + [1] * 16 + [0] * 16 + [2] * 16
    rn.set_weights([1, 0, 1])
    assert rn.assignment == [0, 0, 2, 2]
    _set_state(rn, 1, 2)
    rn.update_action()
    pr = rn.plant_rewards()
    assert np.isnan(pr[1]) and pr[0] == np.asarray(rn.rewards, dtype=np.float64)[:32].mean() and pr[2] == np.asarray(rn.rewards, dtype=np.float64)[32:].mean()


def test_randomized_controller_on_identical_plants_is_a_plain_controller(gpu):
    """Three copies of D0: two plan steps in closed sequence, the phase changing between them, leave nominal, rewards, traces and the phase where a plain controller that
    re-rolls its trace elites leaves them."""
    from judo_amd.controller import make_controller_for
    from judo_amd.fr3_randomized import make_fr3_randomized_controller
    from judo_amd.tasks import FR3Pick

    d0 = plants()[0]
    rn = make_fr3_randomized_controller("mppi", [copy.deepcopy(d0) for _ in range(3)])
    assert rn.assignment == [0, 1, 2]
    plain = make_controller_for(FR3Pick(), "mppi")
    plain.fused_traces = False
    for c in (rn, plain):
        _configure(c, 7, n=48)
    for step in range(2):
        for c in (rn, plain):
            _set_state(c, 0, step, [0.7, 0.0, 0.05] if step else None)
            c.update_action()
        _assert_same(_snap(rn), _snap(plain), f"identical plants step {step}")
    assert rn.task.phase == 1


def test_no_fleet_takes_a_randomized_fr3_controller(gpu):
    from judo_amd.ensemble_fleet import EnsembleFleet
    from judo_amd.fleet import ControllerFleet
    from judo_amd.fr3_fleet import FR3Fleet, FR3PlantFleet
    from judo_amd.fr3_randomized import make_fr3_randomized_controller
    from judo_amd.randomized_fleet import RandomizedFleet

    rn = make_fr3_randomized_controller("mppi", list(plants()[:2]))
    lone = _lone_on(plants()[0], "mppi")
    for fleet, members in ((ControllerFleet, [rn]), (EnsembleFleet, [rn]), (RandomizedFleet, [rn, rn]), (FR3Fleet, [lone, rn]), (FR3PlantFleet, [lone, rn])):
        with pytest.raises(ValueError, match="is an FR3RandomizedController.*no controller axis"):
            fleet(members)
