"""jh_rollout_materialize_plants through the C ABI: G blocks of n rollouts in one launch, block g on plant plant_of_block[g] of a model set, against
jh_rollout_materialize on that plant's own model handle for the block's n rows.

Every comparison is bit for bit (`torch.equal`), states and sensors of every block: the kernels offset their pointers by blockIdx.y and run the single launch's code.
So that a kernel that ignored the table could not pass, the M = 3 plants are required to give different single-launch outputs from the same inputs."""

import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_gpu_model_set import _settled, _task

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3
POISON = -7.0
# the perturbed members (keyword arguments of models.scaled_description); member 0 is the shipped description
PLANTS = {
    "cartpole": [dict(body_mass={"pole": 1.5}), dict(body_mass={"cart": 0.7, "pole": 1.2})],
    "cylinder_push": [dict(body_mass={"pusher": 1.5}, geom_friction={None: 0.8}), dict(body_mass={"cart": 0.6}, geom_friction={None: 1.3})],
    "leap": [dict(body_mass={"cube": 1.5}, geom_friction={"cube": 0.6}), dict(body_mass={"cube": 0.7}, geom_friction={"cube": 1.3})],
}
# the variants of a closed-form case: (x0_batched, controls_shared, states, sensors)
VARIANTS = [(0, False, True, True), (1, False, True, True), (0, True, True, True), (1, True, True, False), (0, False, False, True)]


@functools.lru_cache(maxsize=None)
def _plants(name, self_collision=None):
    """(models, set): the shipped model of `name` and its two perturbed plants, each with a handle of its own, and the set of the three (made once per session)."""
    import torch

    from judo_amd.device import GpuModel, GpuModelSet
    from judo_amd.models import scaled_description

    dev = torch.device("cuda", 0)
    desc = _task(name).desc
    models = [GpuModel(desc, dev)] + [GpuModel(scaled_description(desc, **kw), dev) for kw in PLANTS.get(name, PLANTS["leap"])]
    if self_collision is not None:
        for m in models:
            m.set_self_collision(self_collision)
    return models, GpuModelSet(models)


def _x0(name, rows, seed):
    """(rows, nx) fp32 start states: the closed-form tasks' default state, the leap family's settled state (the cube rests in the hand), each row moved a little."""
    task = _task(name)
    rng = np.random.default_rng(seed)
    if name in ("cartpole", "cylinder_push"):
        x = np.tile(np.asarray(task.default_state(), dtype=np.float64), (rows, 1)) + 0.2 * rng.standard_normal((rows, task.nq + task.nv))
    else:
        x = np.tile(_settled(name, 5 if name == "leap_cube_down" else 60), (rows, 1))
        x[:, 7:23] += 0.01 * rng.standard_normal((rows, 16))  # the finger joints alone: the cube stays where it rests
    return x.astype(np.float32)


def _controls(name, rows, H, seed):
    task = _task(name)
    rng = np.random.default_rng(seed)
    if name == "cartpole":
        return (0.8 * rng.standard_normal((rows, H, 1))).astype(np.float32)
    if name == "cylinder_push":
        return (np.asarray(task.default_state())[:2] + 0.3 * rng.standard_normal((rows, H, 2))).astype(np.float32)
    home = _settled(name, 5 if name == "leap_cube_down" else 60)[7:23]
    return (home + 0.15 * rng.standard_normal((rows, H, 16))).astype(np.float32)


def _single(model, x0, batched, controls, want_states=True, want_sensors=True):
    """jh_rollout_materialize on `model`'s own handle."""
    import torch

    from judo_amd import _lib
    from judo_amd.device import current_stream_ptr

    n, H, _ = controls.shape
    states = torch.empty((n, H, model.nx), dtype=torch.float32, device=model.device) if want_states else None
    sensors = torch.empty((n, H, model.ns), dtype=torch.float32, device=model.device) if want_sensors else None
    st = _lib.lib().jh_rollout_materialize(model.handle, x0.data_ptr(), batched, controls.data_ptr(), n, H, _lib.ptr(states), _lib.ptr(sensors), current_stream_ptr())
    _lib.check(st, "jh_rollout_materialize")
    return states, sensors


def _call(mset, table, n, x0, batched, controls, shared, H, states, sensors):
    """The raw entry: its status.  `table` may hold anything an int array holds; None passes a null pointer."""
    from judo_amd import _lib
    from judo_amd.device import current_stream_ptr

    arr = (C.c_int * max(len(table), 1))(*table) if table is not None else None
    return _lib.lib().jh_rollout_materialize_plants(mset.handle if mset is not None else None, arr, len(table) if table is not None else 1, n, _lib.ptr(x0), batched, _lib.ptr(controls),
                                                    int(shared), H, _lib.ptr(states), _lib.ptr(sensors), current_stream_ptr())


def _check(name, models, mset, table, n, H, batched, shared, want_states, want_sensors, seed):
    """One launch on the set against one single launch per block; returns the per-block references (states, sensors)."""
    import torch

    dev, G = models[0].device, len(table)
    x0 = torch.from_numpy(_x0(name, G * n if batched else 1, seed)).to(dev)
    x0 = x0 if batched else x0[0].contiguous()
    controls = torch.from_numpy(_controls(name, n if shared else G * n, H, seed + 1)).to(dev)
    nx, ns = models[0].nx, models[0].ns
    states = torch.full((G * n, H, nx), POISON, dtype=torch.float32, device=dev) if want_states else None
    sensors = torch.full((G * n, H, ns), POISON, dtype=torch.float32, device=dev) if want_sensors else None
    assert _call(mset, table, n, x0, batched, controls, shared, H, states, sensors) == 0
    refs = []
    for g, p in enumerate(table):
        rows = slice(g * n, (g + 1) * n)
        ref = _single(models[p], x0[rows].contiguous() if batched else x0, batched, controls if shared else controls[rows].contiguous(), want_states, want_sensors)
        for got, want, what in ((states, ref[0], "states"), (sensors, ref[1], "sensors")):
            if want is not None:
                assert torch.isfinite(want).all()
                assert torch.equal(got[rows], want), f"{name}: block {g} on plant {p}: {what} differ from the plant's own launch (G={G} n={n} H={H} x0_batched={batched} shared={shared})"
        refs.append(ref)
    return refs


def _plants_differ(name, models, n, H, seed):
    """The same inputs give different outputs on every two plants: the table matters."""
    import torch

    dev = models[0].device
    x0 = torch.from_numpy(_x0(name, 1, seed)).to(dev)[0].contiguous()
    controls = torch.from_numpy(_controls(name, n, H, seed + 1)).to(dev)
    outs = [_single(m, x0, 0, controls)[0] for m in models]
    for a in range(len(outs)):
        for b in range(a + 1, len(outs)):
            assert not torch.equal(outs[a], outs[b]), f"{name}: plants {a} and {b} roll out alike: the case shows nothing"


@pytest.mark.parametrize("name", ["cartpole", "cylinder_push"])
@pytest.mark.parametrize("table,n,H", [([2, 0, 2], 5, 3), ([2, 0, 2], 129, 8), ([1], 1, 3)], ids=["odd_offset", "ragged_last_workgroup", "one_rollout"])
def test_closed_form_blocks_equal_the_plants_own_launches(gpu, name, table, n, H):
    """cartpole and cylinder_push.  n = 5, H = 3: a block offset of 15 (30) control floats, no multiple of 4 -- the scalar tile path.  n = 129 = 2 * 64 + 1, H = 8: two
    full workgroups on the 16-byte tile path and a ragged third one per block.  G = 1, n = 1.  Each with one x0 and one per row, own and shared controls, both outputs,
    states alone and sensors alone."""
    models, mset = _plants(name)
    _plants_differ(name, models, 5, 8, seed=3)
    for i, (batched, shared, want_states, want_sensors) in enumerate(VARIANTS):
        _check(name, models, mset, table, n, H, batched, shared, want_states, want_sensors, seed=10 * i + n)


@pytest.mark.parametrize("name,self_collision", [("leap_cube", False), ("leap_cube", True), ("leap_cube_down", None), ("caltech_cylinder", None)],
                         ids=["leap_cube_cube_contacts", "leap_cube_hand_contacts", "leap_cube_down_64_contacts", "caltech_cylinders"])
def test_leap_blocks_equal_the_plants_own_launches(gpu, name, self_collision):
    """The three builds of the leap kernel, the hand's own contacts off and on: G = 3, n = 5, H = 4 from a state with the cube in contact; own controls with one x0,
    shared controls with an x0 per row."""
    models, mset = _plants(name, self_collision)
    build = models[0].build()
    assert build["cylinder_build"] == (name == "caltech_cylinder") and build["contact_capacity"] == (48 if name == "leap_cube" else 64)
    assert models[0].self_collision == (True if self_collision is None else self_collision)
    _plants_differ(name, models, 5, 4, seed=5)
    _check(name, models, mset, [2, 0, 2], 5, 4, 0, False, True, True, seed=21)
    _check(name, models, mset, [1, 2, 0], 5, 4, 1, True, True, True, seed=22)


def test_leap_latency_shifts_of_the_whole_launch(gpu):
    """The latency shift is taken from G * n, the launch's rollouts: G = 4 blocks of n just above CUs, then just above 2 * CUs, put the launch into each of the two
    shallower shifts while every single-launch reference stays in the deepest.  On 256 CUs: n = 259 (1036 rollouts: shift 1) and n = 515 (2060: shift 0); a single
    launch keeps shift 2 up to 1024 rollouts.  n is no multiple of 4, so every block ends in a wave with idle rows.  The bits do not depend on the shift."""
    import torch

    models, mset = _plants("leap_cube", True)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    G, rpw = 4, 4
    for want_shift, base in ((1, cus), (0, 2 * cus)):
        n = base + 3 if (base + 3) % 4 else base + 1
        shift = lambda rollouts: next((s for s in (2, 1) if (rollouts << s) <= cus * 4 * rpw), 0)  # jh_latency_shift (judo_amd/csrc/jh_api.hip)
        assert n % 4 != 0 and shift(G * n) == want_shift and shift(n) == 2, (cus, n)
        _check("leap_cube", models, mset, [0, 1, 2, 1], n, 2, 0, want_shift == 1, True, True, seed=30 + want_shift)


def test_a_replaced_member_is_followed(gpu):
    """jh_model_set_update between two calls: the second call's blocks on that member follow the new plant."""
    import torch

    from judo_amd.device import GpuModel, GpuModelSet
    from judo_amd.models import scaled_description

    for name, kw in (("cartpole", dict(body_mass={"pole": 2.0})), ("leap_cube", dict(body_mass={"cube": 2.0}, geom_friction={"cube": 0.5}))):
        models, _ = _plants(name, True if name == "leap_cube" else None)
        models = list(models)
        mset = GpuModelSet(models)  # (a set of this test's own: the shared one stays as it is)
        before = _check(name, models, mset, [1, 0, 1], 5, 4, 0, True, True, True, seed=41)
        new = GpuModel(scaled_description(_task(name).desc, **kw), models[0].device)
        mset.update(1, new)
        models[1] = new
        after = _check(name, models, mset, [1, 0, 1], 5, 4, 0, True, True, True, seed=41)
        assert not torch.equal(before[0][0], after[0][0]) and torch.equal(before[1][0], after[1][0])  # member 1 moved, member 0 did not
        mset.close()


def test_refusals_name_the_argument_and_touch_nothing(gpu):
    import torch

    from judo_amd import _lib
    from judo_amd.device import GpuModel, GpuModelSet

    models, mset = _plants("cartpole")
    dev, n, H = models[0].device, 4, 3
    x0 = torch.from_numpy(_x0("cartpole", 1, 0)).to(dev)[0].contiguous()
    controls = torch.from_numpy(_controls("cartpole", 3 * n, H, 1)).to(dev)
    states = torch.full((3 * n, H, models[0].nx), POISON, dtype=torch.float32, device=dev)
    sensors = torch.full((3 * n, H, models[0].ns), POISON, dtype=torch.float32, device=dev)
    ok = dict(mset=mset, table=[2, 0, 1], n=n, x0=x0, batched=0, controls=controls, shared=0, H=H, states=states, sensors=sensors)
    cases = [
        (dict(mset=None), INVALID, "set is a null pointer"),
        (dict(table=None), INVALID, "plant_of_block is a null pointer"),
        (dict(x0=None), INVALID, "x0 is a null pointer"),
        (dict(controls=None), INVALID, "controls is a null pointer"),
        (dict(states=None, sensors=None), INVALID, "states and sensors are both null"),
        (dict(table=[]), INVALID, "G = 0"),
        (dict(table=[0] * (_lib.MAX_FLEET_PLANT_BLOCKS + 1)), INVALID, f"G = {_lib.MAX_FLEET_PLANT_BLOCKS + 1}"),
        (dict(n=0), INVALID, "n = 0"),
        (dict(H=0), INVALID, "H = 0"),
        (dict(table=[2, 3, 1]), INVALID, "plant_of_block[1] = 3"),
        (dict(table=[2, 0, -1]), INVALID, "plant_of_block[2] = -1"),
        (dict(table=[0] * 256, n=1 << 23), INVALID, "G * n = 256 * 8388608"),
    ]
    for change, status, text in cases:
        got = _call(**{**ok, **change})  # (an empty table: G = 0 with a table pointer that is not null)
        msg = _lib.lib().jh_last_error().decode()
        assert got == status and text in msg and "rollout_materialize_plants" in msg, (change, got, msg)
    fr3 = GpuModelSet([GpuModel("fr3_pick", dev)])
    assert fr3.fr3
    got = _call(fr3, [0], n, x0, 0, controls, 0, H, states, sensors)
    msg = _lib.lib().jh_last_error().decode()
    assert got == UNSUPPORTED and "fr3_pick" in msg and "arm kernel has no materialise launch on plants yet" in msg, (got, msg)
    torch.cuda.synchronize()
    assert bool((states == POISON).all()) and bool((sensors == POISON).all())
    assert _call(**ok) == 0  # ... and the arguments they were varied from are accepted
    torch.cuda.synchronize()
    assert bool((states != POISON).any()) and bool((sensors != POISON).any())


def test_the_backend_rolls_out_on_plants(gpu):
    """`GpuRolloutBackend.rollout_plants_device` and its numpy twin: the rows of the C entry, shapes checked on the host."""
    import torch

    from judo_amd.rollout_backend import GpuRolloutBackend

    models, mset = _plants("cylinder_push")
    be = GpuRolloutBackend(models[0], 10)
    x0, controls = _x0("cylinder_push", 1, 7)[0], _controls("cylinder_push", 5, 4, 8)
    s, y = be.rollout_plants_device(mset, [1, 2], torch.from_numpy(x0).to(gpu), torch.from_numpy(controls).to(gpu), shared_controls=True)
    assert tuple(s.shape) == (10, 4, models[0].nx) and tuple(y.shape) == (10, 4, models[0].ns)
    for g, p in enumerate([1, 2]):
        ref = GpuRolloutBackend(models[p], 5).rollout_device(torch.from_numpy(x0).to(gpu), torch.from_numpy(controls).to(gpu))
        assert torch.equal(s[5 * g : 5 * g + 5], ref[0]) and torch.equal(y[5 * g : 5 * g + 5], ref[1])
    s_np, y_np, none = be.rollout_plants(mset, [1, 2], x0, controls, shared_controls=True)
    assert none is None and s_np.dtype == np.float64 and np.array_equal(s_np, s.cpu().numpy().astype(np.float64)) and np.array_equal(y_np, y.cpu().numpy().astype(np.float64))
    with pytest.raises(ValueError, match=r"plant_of_block\[1\] = 3"):
        be.rollout_plants_device(mset, [0, 3], torch.from_numpy(x0).to(gpu), torch.from_numpy(controls).to(gpu), shared_controls=True)
    with pytest.raises(ValueError, match="do not split into G = 2 equal blocks"):
        be.rollout_plants_device(mset, [0, 1], torch.from_numpy(x0).to(gpu), torch.from_numpy(controls).to(gpu))
