"""The plant axis of the tree kernel through the C ABI (judo_amd/csrc/jh_engine_v4.hip, PLANTS; include/judo_amd.h jh_tree_set_*, jh_tree_substeps_plants,
jh_policy_rollout_plants): every rollout block of a launch on a jh_tree_set is bit for bit what the single call computes on that plant's own jh_tree -- states, sensors,
policy outputs and warm start -- in latency mode and with two rollouts to a wave, with an odd block size, with several problems, after a plant was replaced; and every
refusal comes before anything is enqueued.

Shapes: P = 2 plants, G = 3 blocks on plants [1, 0, 1], n = 3 rollouts to a block (odd: the last wave of a block has a dead row when two rollouts share a wave), T = 2
command rows of 2 substeps.  No deadline (cutoff < 0): timing cannot enter the results."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G, N_BLOCK, T, SUBSTEPS = 3, 3, 2, 2
TABLE = [1, 0, 1]
# the model, its task (for a start state), the scaling of plant 1, where the free object is put: the box 4 mm into the plane within the arm's reach, the tire likewise
KINDS = {
    "spot_box": ("spot_box_push", dict(body_mass={"box_body": 1.7}, geom_friction={"box_collision": 0.6}, actuator_kp={None: 1.2}), (0.95, 0.0, 0.25)),
    "spot_tire": ("spot_tire_roll", dict(body_mass={"tire": 1.7}, geom_friction={"object_primitive_approx": 0.6}, actuator_kp={None: 1.2}), (0.95, 0.0, 0.326)),
    "spot": ("spot_navigate", dict(body_mass={"body": 1.7}, geom_friction={"body_collision": 0.6}, actuator_kp={None: 1.2}), None),
}
CASES = [("spot_box", True), ("spot_tire", False), ("spot", True)]  # self-collision on and off, one object kind each

_cache: dict = {}


def _L():
    from judo_amd import _lib

    return _lib.lib()


def _err():
    return _L().jh_last_error().decode()


def _task(kind):
    from judo_amd.tasks import get_registered_tasks

    if ("task", kind) not in _cache:
        _cache[("task", kind)] = get_registered_tasks()[KINDS[kind][0]][0]()
    return _cache[("task", kind)]


def _plants(kind, self_collision):
    """The set of P = 2 plants of the kind (the task's description and its scaled copy), once per module."""
    from judo_amd.models import scaled_description
    from judo_amd.policy import SpotPlantSet

    key = ("set", kind, self_collision)
    if key not in _cache:
        base = _task(kind).desc
        _cache[key] = SpotPlantSet([base, scaled_description(base, **KINDS[kind][1])], self_collision=self_collision)
    return _cache[key]


def _policy():
    from judo_amd.policy import SpotLocomotionPolicy

    if "policy" not in _cache:
        _cache["policy"] = SpotLocomotionPolicy()
    return _cache["policy"]


def _states(kind, rows, seed):
    """(rows, nx) fp32 start states: the task's standing state with other leg angles and base offsets per row, the free object on the plane where the robot touches it."""
    import torch

    task, rng = _task(kind), np.random.default_rng(seed)
    x = np.tile(np.array(task.default_state(), dtype=np.float64), (rows, 1))
    x[:, 7:19] += 0.05 * rng.standard_normal((rows, 12))
    x[:, :2] += 0.02 * rng.standard_normal((rows, 2))
    if KINDS[kind][2] is not None:
        x[:, 26:29] = KINDS[kind][2]
        x[:, 26:28] += 0.01 * rng.standard_normal((rows, 2))
    return torch.as_tensor(x, dtype=torch.float32, device="cuda").contiguous()


def _commands(rows, seed):
    import torch

    rng = np.random.default_rng(seed)
    cmd = np.tile(np.asarray(_task("spot").default_policy_command, dtype=np.float64), (rows, T, 1))
    assert cmd.shape[2] == 25
    cmd[:, :, :3] = rng.uniform(-0.5, 0.5, (rows, 1, 3))
    cmd[:, :, 3:10] += 0.2 * rng.standard_normal((rows, 1, 7))
    return torch.as_tensor(cmd, dtype=torch.float32, device="cuda").contiguous()


def _ints(values):
    return (C.c_int * len(values))(*values)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _substeps_plants(ps, table, states, ctrl, warm, n):
    import torch

    out, sens = torch.full_like(states, 7.0), torch.full((states.shape[0], ps.nsensordata), 7.0, dtype=torch.float32, device="cuda")
    rc = _L().jh_tree_substeps_plants(ps.handle, _ints(table), len(table), n, _ptr(states), _ptr(ctrl), _ptr(warm), SUBSTEPS, _ptr(out), _ptr(sens), None)
    assert rc == 0, _err()
    torch.cuda.synchronize()
    return out, sens


def _substeps_single(ps, table, states, ctrl, warm, n):
    """The reference: block g's rows through jh_tree_substeps on plant table[g]'s own handle."""
    import torch

    out, sens = torch.empty_like(states), torch.empty((states.shape[0], ps.nsensordata), dtype=torch.float32, device="cuda")
    for g, p in enumerate(table):
        r = slice(g * n, (g + 1) * n)
        ps.engines[p].substeps(states[r], ctrl[r], warm[r], SUBSTEPS, out=out[r], sensors=sens[r])
    torch.cuda.synchronize()
    return out, sens


def _rollout_plants(ps, B, table, x0, commands, policy_out, warm, n, over=None):
    """jh_policy_rollout_plants with the arguments of the valid call, `over` replacing some; returns (status, states, sensors, steps done)."""
    import torch

    rows, nx = commands.shape[0], ps.nq + ps.nv
    states = torch.full((rows, T, nx), 7.0, dtype=torch.float32, device="cuda")
    sensors = torch.full((rows, T, ps.nsensordata), 7.0, dtype=torch.float32, device="cuda")
    scratch = torch.empty(int(_L().jh_policy_rollout_scratch_floats(rows)), dtype=torch.float32, device="cuda")
    done = C.c_int(-5)
    a = dict(policy=_policy().handle, set=ps.handle, B=B, G=len(table) // B, plant_of_block=_ints(table), x0=_ptr(x0), x0_stride=nx, commands=_ptr(commands), policy_out=_ptr(policy_out),
             warm=_ptr(warm), reset_warm=0, n=n, T=T, substeps=SUBSTEPS, cutoff=-1.0, states=_ptr(states), sensors=_ptr(sensors), scratch=_ptr(scratch))
    a.update(over or {})
    rc = _L().jh_policy_rollout_plants(a["policy"], a["set"], a["B"], a["G"], a["plant_of_block"], a["x0"], a["x0_stride"], a["commands"], a["policy_out"], a["warm"], a["reset_warm"], a["n"],
                                       a["T"], a["substeps"], a["cutoff"], a["states"], a["sensors"], a["scratch"], C.byref(done), None)
    torch.cuda.synchronize()
    return rc, states, sensors, done.value


def _rollout_single(ps, B, table, x0, commands, policy_out, warm, n):
    """The reference: block (b, g) through jh_policy_rollout with N = n on plant table[b * G + g]'s own handle, from problem b's state; policy_out and warm in place."""
    import torch

    rows, nx, Gb = commands.shape[0], ps.nq + ps.nv, len(table) // B
    states = torch.empty((rows, T, nx), dtype=torch.float32, device="cuda")
    sensors = torch.empty((rows, T, ps.nsensordata), dtype=torch.float32, device="cuda")
    scratch = torch.empty(int(_L().jh_policy_rollout_scratch_floats(n)), dtype=torch.float32, device="cuda")
    for e, p in enumerate(table):
        r, done = slice(e * n, (e + 1) * n), C.c_int(0)
        rc = _L().jh_policy_rollout(_policy().handle, ps.engines[p].handle, _ptr(x0[e // Gb]), 0, _ptr(commands[r]), _ptr(policy_out[r]), _ptr(warm[r]), 0, n, T, SUBSTEPS, -1.0,
                                    _ptr(states[r]), _ptr(sensors[r]), _ptr(scratch), C.byref(done), None)
        assert rc == 0 and done.value == T, _err()
    torch.cuda.synchronize()
    return states, sensors


def _carried(rows, nv, seed):
    """Policy outputs to carry in (small, not zero) and a zero warm start."""
    import torch

    out = torch.as_tensor(0.1 * np.random.default_rng(seed).standard_normal((rows, 12)), dtype=torch.float32, device="cuda").contiguous()
    return out, torch.zeros((rows, nv), dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("kind,self_collision", CASES)
def test_substeps_on_a_set_equal_the_plants_own_handles(gpu, monkeypatch, kind, self_collision):
    """jh_tree_substeps_plants, blocks [1, 0, 1] of 3 rows: states, sensors and warm start equal the per-block single calls, in latency mode and with two rollouts to a
    wave (the dead row of an odd block), and the two plants do compute different results."""
    import torch

    ps = _plants(kind, self_collision)
    rows = G * N_BLOCK
    states = _states(kind, rows, seed=1)
    ctrl = (states[:, 7:26] + torch.as_tensor(0.05 * np.random.default_rng(2).standard_normal((rows, 19)), dtype=torch.float32, device="cuda")).contiguous()
    warm_ref = torch.zeros((rows, ps.nv), dtype=torch.float32, device="cuda")
    ref, sref = _substeps_single(ps, TABLE, states, ctrl, warm_ref, N_BLOCK)
    other, _ = _substeps_single(ps, [0, 0, 0], states, ctrl, torch.zeros_like(warm_ref), N_BLOCK)
    assert torch.isfinite(ref).all() and not torch.equal(other[:N_BLOCK], ref[:N_BLOCK]), "the two plants give the same states: the test would show nothing"
    assert torch.equal(other[N_BLOCK : 2 * N_BLOCK], ref[N_BLOCK : 2 * N_BLOCK])
    for shift in (None, "0"):
        if shift is not None:
            monkeypatch.setenv("JUDO_AMD_LATENCY_SHIFT", shift)
        warm = torch.zeros_like(warm_ref)
        got, sgot = _substeps_plants(ps, TABLE, states, ctrl, warm, N_BLOCK)
        assert torch.equal(got, ref), (kind, shift, "states")
        assert torch.equal(sgot, sref), (kind, shift, "sensors")
        assert torch.equal(warm, warm_ref), (kind, shift, "warm start")


@pytest.mark.parametrize("kind,self_collision", CASES)
def test_policy_rollout_on_a_set_equals_the_plants_own_handles(gpu, monkeypatch, kind, self_collision):
    """jh_policy_rollout_plants, B = 1: states, sensors, policy outputs and warm start of every block equal jh_policy_rollout on the block's plant; the same bits in
    latency mode and with two rollouts to a wave; the set counts G * n * T * substeps steps."""
    import torch

    ps = _plants(kind, self_collision)
    rows = G * N_BLOCK
    x0, commands = _states(kind, 1, seed=3), _commands(rows, seed=4)
    out_ref, warm_ref = _carried(rows, ps.nv, seed=5)
    ref, sref = _rollout_single(ps, 1, TABLE, x0, commands, out_ref, warm_ref, N_BLOCK)
    out0, warm0 = _carried(rows, ps.nv, seed=5)
    on0, _ = _rollout_single(ps, 1, [0, 0, 0], x0, commands, out0, warm0, N_BLOCK)
    assert torch.isfinite(ref).all() and not torch.equal(on0[:N_BLOCK], ref[:N_BLOCK]), "the two plants give the same states: the test would show nothing"
    for shift in (None, "0"):
        if shift is not None:
            monkeypatch.setenv("JUDO_AMD_LATENCY_SHIFT", shift)
        ps.stats()
        out, warm = _carried(rows, ps.nv, seed=5)
        rc, got, sgot, done = _rollout_plants(ps, 1, TABLE, x0, commands, out, warm, N_BLOCK)
        assert rc == 0 and done == T, _err()
        assert torch.equal(got, ref), (kind, shift, "states")
        assert torch.equal(sgot, sref), (kind, shift, "sensors")
        assert torch.equal(out, out_ref), (kind, shift, "policy outputs")
        assert torch.equal(warm, warm_ref), (kind, shift, "warm start")
        assert ps.stats()["steps"] == G * N_BLOCK * T * SUBSTEPS


def test_two_problems_with_their_own_states_and_a_two_by_three_table(gpu, monkeypatch):
    """B = 2 problems, start states 80 floats apart, table [[1, 0, 1], [0, 1, 1]]: block (b, g) from problem b's state on plant table[b][g]."""
    import torch

    ps = _plants("spot_box", True)
    B, table, nx = 2, [1, 0, 1, 0, 1, 1], ps.nq + ps.nv
    rows = B * G * N_BLOCK
    x0 = _states("spot_box", B, seed=6)
    assert not torch.equal(x0[0], x0[1])
    padded = torch.full((B, 80), 3.0, dtype=torch.float32, device="cuda")
    padded[:, :nx] = x0
    commands = _commands(rows, seed=7)
    out_ref, warm_ref = _carried(rows, ps.nv, seed=8)
    ref, sref = _rollout_single(ps, B, table, x0, commands, out_ref, warm_ref, N_BLOCK)
    assert not torch.equal(ref[: G * N_BLOCK], ref[G * N_BLOCK :])
    for shift in (None, "0"):
        if shift is not None:
            monkeypatch.setenv("JUDO_AMD_LATENCY_SHIFT", shift)
        out, warm = _carried(rows, ps.nv, seed=8)
        rc, got, sgot, done = _rollout_plants(ps, B, table, padded, commands, out, warm, N_BLOCK, over=dict(x0_stride=80))
        assert rc == 0 and done == T, _err()
        assert torch.equal(got, ref) and torch.equal(sgot, sref) and torch.equal(out, out_ref) and torch.equal(warm, warm_ref), shift


def test_a_replaced_plant_is_the_one_that_runs(gpu):
    """jh_tree_set_update: after plant 0 is replaced, its blocks equal the new plant's own handle; plant 1's blocks are what they were."""
    import torch

    from judo_amd.models import scaled_description
    from judo_amd.policy import SpotPlantSet

    base = _task("spot").desc
    ps = SpotPlantSet([base, scaled_description(base, **KINDS["spot"][1])])
    info = (C.c_int * 4)()
    assert _L().jh_tree_set_info(ps.handle, info) == 0
    assert list(info)[0] == 2 and info[1] % 4 == 0 and (info[2], info[3]) == (26, 25)
    rows = G * N_BLOCK
    states = _states("spot", rows, seed=9)
    ctrl = states[:, 7:26].contiguous()
    before, _ = _substeps_plants(ps, TABLE, states, ctrl, torch.zeros((rows, ps.nv), dtype=torch.float32, device="cuda"), N_BLOCK)
    ps.set_member(0, scaled_description(base, actuator_kp={None: 0.8}, body_mass={"body": 0.9}))
    warm_ref = torch.zeros((rows, ps.nv), dtype=torch.float32, device="cuda")
    ref, sref = _substeps_single(ps, TABLE, states, ctrl, warm_ref, N_BLOCK)  # (ps.engines[0] is the new plant's own handle)
    warm = torch.zeros_like(warm_ref)
    got, sgot = _substeps_plants(ps, TABLE, states, ctrl, warm, N_BLOCK)
    assert torch.equal(got, ref) and torch.equal(sgot, sref) and torch.equal(warm, warm_ref)
    mid = slice(N_BLOCK, 2 * N_BLOCK)
    assert not torch.equal(got[mid], before[mid]) and torch.equal(got[:N_BLOCK], before[:N_BLOCK])
    # the checks of the update are those of the creation: another model's tree is refused, naming the member and the section
    other = _plants("spot_box", True).engines[0]
    assert _L().jh_tree_set_update(ps.handle, 1, other.handle) == -1 and "member 1" in _err() and ("float section" in _err() or "int section" in _err())
    assert _L().jh_tree_set_update(ps.handle, 2, ps.engines[0].handle) == -1 and "p = 2" in _err()


def test_the_set_refuses_members_that_differ_beyond_the_float_section(gpu):
    from judo_amd.policy import SpotTreeEngine

    spot, box = _plants("spot", True).engines[0], _plants("spot_box", True).engines[0]
    handle = C.c_void_p()

    def create(engines, P=None):
        arr = (C.c_void_p * len(engines))(*[e.handle if e is not None else None for e in engines])
        return _L().jh_tree_set_create(arr, len(engines) if P is None else P, C.byref(handle))

    assert create([spot, box]) == -1 and "member 1" in _err() and ("float section" in _err() or "int section" in _err())
    off = SpotTreeEngine(_task("spot").desc, self_collision=False)
    assert create([spot, off]) == -1 and "member 1" in _err() and "self-collision" in _err()
    assert create([spot, None]) == -1 and "member 1" in _err()
    assert create([spot], P=0) == -1 and "P = 0" in _err()
    assert create([spot] * 33) == -1 and "P = 33" in _err() and "JH_MAX_ENSEMBLE" in _err()
    assert handle.value is None


def test_refusals_come_before_anything_is_enqueued(gpu):
    """Every JH_ERR_INVALID case of the two launches returns -1, names its argument, and leaves states, sensors, policy outputs and warm start as they were."""
    import torch

    ps = _plants("spot", True)
    rows, nx = G * N_BLOCK, ps.nq + ps.nv
    x0, commands = _states("spot", 2, seed=10), _commands(rows, seed=11)
    out0, warm0 = _carried(rows, ps.nv, seed=12)

    def refused(what, **over):
        out, warm = out0.clone(), warm0.clone()
        rc, states, sensors, done = _rollout_plants(ps, 1, TABLE, x0, commands, out, warm, N_BLOCK, over=over)
        assert rc == -1 and what in _err(), (over, rc, _err())
        assert bool((states == 7.0).all()) and bool((sensors == 7.0).all()) and torch.equal(out, out0) and torch.equal(warm, warm0) and done == -5, over

    for name in ("policy", "set", "plant_of_block", "x0", "commands", "policy_out", "states", "scratch"):
        refused("null pointer", **{name: None})
    for name in ("B", "G", "n", "T", "substeps"):
        refused(f"{name} = 0", **{name: 0})
    refused("B * G = 2 * 129 = 258 exceeds JH_MAX_FLEET_PLANT_BLOCKS = 256", B=2, G=129, plant_of_block=_ints([0] * 258))
    refused("plant_of_block[1] = 2 outside [0, P = 2)", plant_of_block=_ints([1, 2, 1]))
    refused("plant_of_block[2] = -1 outside", plant_of_block=_ints([1, 0, -1]))
    refused(f"x0_stride_floats = {nx - 1} is smaller than a state", x0_stride=nx - 1)
    refused("reset_warmstart needs a warmstart buffer", reset_warm=1, warm=None)

    states = _states("spot", rows, seed=13)
    ctrl = states[:, 7:26].contiguous()

    def refused_substeps(what, set_=ps.handle, table=TABLE, g=G, n=N_BLOCK, x=states, u=ctrl, substeps=SUBSTEPS, null_out=False):
        out, sens = torch.full_like(states, 7.0), torch.full((rows, ps.nsensordata), 7.0, dtype=torch.float32, device="cuda")
        warm = warm0.clone()
        rc = _L().jh_tree_substeps_plants(set_, _ints(table) if table is not None else None, g, n, _ptr(x), _ptr(u), _ptr(warm), substeps, None if null_out else _ptr(out), _ptr(sens), None)
        torch.cuda.synchronize()
        assert rc == -1 and what in _err(), (what, rc, _err())
        assert bool((out == 7.0).all()) and bool((sens == 7.0).all()) and torch.equal(warm, warm0), what

    refused_substeps("null pointer", set_=None)
    refused_substeps("null pointer", table=None)
    refused_substeps("null pointer", x=None)
    refused_substeps("null pointer", u=None)
    refused_substeps("null pointer", null_out=True)
    refused_substeps("G = 0", g=0)
    refused_substeps("n = 0", n=0)
    refused_substeps("substeps = 0", substeps=0)
    refused_substeps("G = 257 exceeds JH_MAX_FLEET_PLANT_BLOCKS = 256", table=[0] * 257, g=257)
    refused_substeps("plant_of_block[0] = 2 outside [0, P = 2)", table=[2, 0, 1])
    buf = (C.c_int * 4)()
    assert _L().jh_tree_set_stats(None, buf, 0) == -1 and _L().jh_tree_set_info(ps.handle, None) == -1
