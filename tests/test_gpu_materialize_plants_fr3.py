"""jh_fr3_rollout_materialize_plants through the C ABI: G blocks of n fr3_pick rollouts in one launch of the cooperative arm kernel, block g on plant plant_of_block[g] of
an fr3 model set, against jh_rollout_materialize on that plant's own model handle for the block's n rows.

Every comparison is bit for bit (`torch.equal`), states and sensors of every block: the batched materialise instantiation offsets its pointers by blockIdx.y and runs the
single launch's code.  No tolerance appears in this file.  So that a kernel that ignored the table or the image stride could not pass, the plants used are required to
give different single-launch states from the same inputs.  The plants are D0..D3 of tests/test_fr3_plants_host.py; the start states are the phase states and the pressed
states of tests/test_gpu_plan_batch_fr3.py; the controls are the home joint targets plus small noise."""

import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_fr3_plants_host import plants
from tests.test_gpu_materialize_plants import INVALID, POISON, UNSUPPORTED, _single
from tests.test_gpu_plan_batch_fr3 import _phase_states, _pressed_states

pytestmark = pytest.mark.gpu

# (x0_batched, controls_shared, states, sensors)
VARIANTS = [(0, False, True, True), (1, False, True, True), (0, True, True, True), (1, True, True, False), (0, False, False, True)]


@functools.lru_cache(maxsize=None)
def _models(dev, self_collision=False):
    """GpuModels of D0..D3, made once per build."""
    from judo_amd.device import GpuModel

    return tuple(GpuModel(d, dev) for d in plants(self_collision))


@functools.lru_cache(maxsize=None)
def _set(dev, self_collision=False, members=3):
    from judo_amd.device import GpuModelSet

    s = GpuModelSet(list(_models(dev, self_collision)[:members]))
    assert s.fr3 and s.info()["B"] == members
    return s


def _x0(rows, seed, base=None):
    """(rows, nx) fp32 start states: the phase states in turn (or `base`'s), the arm joints of each row moved a little."""
    xs = _phase_states() if base is None else base
    rng = np.random.default_rng(seed)
    x = np.stack([np.asarray(xs[(seed + i) % len(xs)], dtype=np.float64) for i in range(rows)])
    if rows > 1:
        x[:, 7:14] += 0.01 * rng.standard_normal((rows, 7))
    return x.astype(np.float32)


def _controls(rows, H, seed, sigma=0.05):
    from judo_amd.tasks import FR3Pick

    t = FR3Pick()
    r = t.actuator_ctrlrange
    u = t.reset_command[None, None] + sigma * np.random.default_rng(seed).standard_normal((rows, H, t.nu))
    return np.clip(u, r[:, 0], r[:, 1]).astype(np.float32)


def _call(mset, table, n, x0, batched, controls, shared, H, states, sensors):
    """The raw entry: its status.  `table` may hold anything an int array holds; None passes a null pointer."""
    from judo_amd import _lib
    from judo_amd.device import current_stream_ptr

    arr = (C.c_int * max(len(table), 1))(*table) if table is not None else None
    return _lib.lib().jh_fr3_rollout_materialize_plants(mset.handle if mset is not None else None, arr, len(table) if table is not None else 1, n, _lib.ptr(x0), batched,
                                                        _lib.ptr(controls), int(shared), H, _lib.ptr(states), _lib.ptr(sensors), current_stream_ptr())


def _check(models, mset, table, n, H, batched, shared, want_states, want_sensors, seed, base=None):
    """One launch on the set against one single launch per block, outputs poisoned beforehand; returns the per-block references (states, sensors)."""
    import torch

    from judo_amd import _lib

    dev, G = models[0].device, len(table)
    x0 = torch.from_numpy(_x0(G * n if batched else 1, seed, base)).to(dev)
    x0 = x0 if batched else x0[0].contiguous()
    controls = torch.from_numpy(_controls(n if shared else G * n, H, seed + 1)).to(dev)
    nx, ns = models[0].nx, models[0].ns
    states = torch.full((G * n, H, nx), POISON, dtype=torch.float32, device=dev) if want_states else None
    sensors = torch.full((G * n, H, ns), POISON, dtype=torch.float32, device=dev) if want_sensors else None
    got = _call(mset, table, n, x0, batched, controls, shared, H, states, sensors)
    assert got == 0, _lib.lib().jh_last_error().decode()
    refs = []
    for g, p in enumerate(table):
        rows = slice(g * n, (g + 1) * n)
        ref = _single(models[p], x0[rows].contiguous() if batched else x0, batched, controls if shared else controls[rows].contiguous(), want_states, want_sensors)
        for out, want, what in ((states, ref[0], "states"), (sensors, ref[1], "sensors")):
            if want is not None:
                assert torch.isfinite(want).all()
                assert torch.equal(out[rows], want), f"block {g} on plant {p}: {what} differ from the plant's own launch (G={G} n={n} H={H} x0_batched={batched} shared={shared})"
        refs.append(ref)
    return refs


def _plants_differ(models, n, H, seed, base=None):
    """From the same x0 and controls the single launches on every two of the plants give different states: the table and the image stride matter."""
    import torch

    dev = models[0].device
    x0 = torch.from_numpy(_x0(1, seed, base)).to(dev)[0].contiguous()
    controls = torch.from_numpy(_controls(n, H, seed + 1)).to(dev)
    outs = [_single(m, x0, 0, controls)[0] for m in models]
    for a in range(len(outs)):
        for b in range(a + 1, len(outs)):
            assert not torch.equal(outs[a], outs[b]), f"plants {a} and {b} roll out alike: the case shows nothing"


@pytest.mark.parametrize("self_collision", [False, True], ids=["default_build", "self_collision_build"])
def test_blocks_equal_the_plants_own_launches(gpu, self_collision):
    """Both builds.  Table [2, 0, 1, 2] on the set of D0..D2, n = 6 (two waves per block in the launch, the second ragged) and n = 1, H = 8; one x0 and one per row, own
    and shared controls, both outputs, states alone and sensors alone.  Then the odd tables [1] and [3, 3] on the set of D0..D3."""
    ms = _models(gpu, self_collision)
    assert all(m.fr3_build()["self_collision_build"] == self_collision for m in ms)
    _plants_differ(ms, 6, 8, seed=3)
    three, four = _set(gpu, self_collision, 3), _set(gpu, self_collision, 4)
    for i, (batched, shared, want_states, want_sensors) in enumerate(VARIANTS):
        _check(ms, three, [2, 0, 1, 2], 6, 8, batched, shared, want_states, want_sensors, seed=10 * i + 6)
    for i, (batched, shared, want_states, want_sensors) in enumerate(VARIANTS[:3]):
        _check(ms, three, [2, 0, 1, 2], 1, 8, batched, shared, want_states, want_sensors, seed=10 * i + 1)
    _check(ms, four, [1], 6, 8, 0, False, True, True, seed=61)
    _check(ms, four, [3, 3], 6, 8, 1, False, True, True, seed=62)


def test_overflow_rows_of_the_second_block(gpu):
    """G = 2 on D0 and D2 from the pressed states (more than 32 general contacts: the contacts above the LDS pool live in a row of global memory per rollout, and block 1's
    rows lie n behind block 0's), n = 6, H = 4.  Block 1's rows equal D2's own launch; nothing is dropped and the fallback is not taken, on member 0's counters."""
    import torch

    from judo_amd.device import GpuModelSet

    xs, gen = _pressed_states()
    assert all(32 < n <= 96 for n in gen), gen
    ms = _models(gpu)
    mset = GpuModelSet([ms[0], ms[2]])
    _plants_differ([ms[0], ms[2]], 6, 4, seed=1, base=xs)
    x0 = torch.from_numpy(np.repeat(np.asarray(xs, dtype=np.float32), 6, axis=0)).to(gpu)  # block 0 from the first pressed state, block 1 from the second
    controls = torch.from_numpy(_controls(12, 4, 5, sigma=0.02)).to(gpu)
    states = torch.full((12, 4, ms[0].nx), POISON, dtype=torch.float32, device=gpu)
    sensors = torch.full((12, 4, ms[0].ns), POISON, dtype=torch.float32, device=gpu)
    ms[0].stats(reset=True)
    assert _call(mset, [0, 1], 6, x0, 1, controls, False, 4, states, sensors) == 0
    torch.cuda.synchronize()
    st = ms[0].stats(reset=True)
    assert st["overflow_pool_fallbacks"] == 0 and st["contact_overflow"] == 0, st
    for g, m in enumerate((ms[0], ms[2])):
        ref = _single(m, x0[6 * g : 6 * g + 6].contiguous(), 1, controls[6 * g : 6 * g + 6].contiguous())
        assert torch.isfinite(ref[0]).all()
        assert torch.equal(states[6 * g : 6 * g + 6], ref[0]) and torch.equal(sensors[6 * g : 6 * g + 6], ref[1]), f"block {g}"
    mset.close()


def test_latency_shifts_of_the_whole_launch(gpu):
    """The latency shift is taken from G * n, the launch's rollouts: G = 4 blocks of n just above CUs, then just above 2 * CUs, put the launch into each of the two
    shallower shifts while every single-launch reference stays in the deepest.  n is no multiple of 4, so every block ends in a wave with idle rows.  The bits do not
    depend on the shift."""
    import torch

    ms = _models(gpu)
    four = _set(gpu, False, 4)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    G, rpw = 4, 4
    for want_shift, base in ((1, cus), (0, 2 * cus)):
        n = base + 3 if (base + 3) % 4 else base + 1
        shift = lambda rollouts: next((s for s in (2, 1) if (rollouts << s) <= cus * 4 * rpw), 0)  # jh_latency_shift (judo_amd/csrc/jh_api.hip)
        assert n % 4 != 0 and shift(G * n) == want_shift and shift(n) == 2, (cus, n)
        _check(ms, four, [0, 3, 2, 1], n, 2, 0, want_shift == 1, True, True, seed=30 + want_shift)


def test_a_replaced_member_is_followed(gpu):
    """jh_model_set_update between two calls: the second call's blocks on that member follow the new plant."""
    import torch

    from judo_amd.device import GpuModel, GpuModelSet
    from judo_amd.models import scaled_description

    models = list(_models(gpu)[:2])
    mset = GpuModelSet(models)  # (a set of this test's own: the shared ones stay as they are)
    before = _check(models, mset, [1, 0, 1], 5, 4, 0, True, True, True, seed=41)
    new = GpuModel(scaled_description(plants()[0], body_mass={"object": 2.0}, actuator_kp={None: 0.8}), gpu)
    mset.update(1, new)
    models[1] = new
    after = _check(models, mset, [1, 0, 1], 5, 4, 0, True, True, True, seed=41)
    assert not torch.equal(before[0][0], after[0][0]) and torch.equal(before[1][0], after[1][0])  # member 1 moved, member 0 did not
    mset.close()


def test_refusals_name_the_argument_and_touch_nothing(gpu):
    import torch

    from judo_amd import _lib
    from judo_amd.device import GpuModel, GpuModelSet

    ms, mset = _models(gpu), _set(gpu, False, 3)
    n, H = 4, 3
    x0 = torch.from_numpy(_x0(1, 0)).to(gpu)[0].contiguous()
    controls = torch.from_numpy(_controls(3 * n, H, 1)).to(gpu)
    states = torch.full((3 * n, H, ms[0].nx), POISON, dtype=torch.float32, device=gpu)
    sensors = torch.full((3 * n, H, ms[0].ns), POISON, dtype=torch.float32, device=gpu)
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
        assert got == status and text in msg and "fr3_rollout_materialize_plants" in msg, (change, got, msg)
    leap = GpuModelSet([GpuModel("leap_cube", gpu)])
    assert not leap.fr3
    got = _call(leap, [0], n, x0, 0, controls, 0, H, states, sensors)
    msg = _lib.lib().jh_last_error().decode()
    assert got == UNSUPPORTED and "fr3_rollout_materialize_plants: not an fr3_pick set" in msg and "jh_rollout_materialize_plants" in msg, (got, msg)
    torch.cuda.synchronize()
    assert bool((states == POISON).all()) and bool((sensors == POISON).all())
    assert _call(**ok) == 0  # ... and the arguments they were varied from are accepted
    torch.cuda.synchronize()
    assert bool((states != POISON).any()) and bool((sensors != POISON).any())


def test_the_backend_rolls_out_on_an_fr3_set(gpu):
    """`GpuRolloutBackend.rollout_plants` on an fr3 set: fp64 arrays whose blocks equal `rollout` on the plants' own backends."""
    from judo_amd.rollout_backend import GpuRolloutBackend

    ms, mset = _models(gpu), _set(gpu, False, 3)
    be = GpuRolloutBackend(ms[0], 10)
    x0, controls = _x0(1, 7)[0], _controls(10, 4, 8)
    s, y, none = be.rollout_plants(mset, [2, 1], x0, controls)
    assert none is None and s.dtype == np.float64 and y.dtype == np.float64 and s.shape == (10, 4, ms[0].nx) and y.shape == (10, 4, ms[0].ns)
    for g, p in enumerate([2, 1]):
        rs, ry, _ = GpuRolloutBackend(ms[p], 5).rollout(x0, controls[5 * g : 5 * g + 5])
        assert np.array_equal(s[5 * g : 5 * g + 5], rs) and np.array_equal(y[5 * g : 5 * g + 5], ry), (g, p)
    assert not np.array_equal(s[:5], GpuRolloutBackend(ms[0], 5).rollout(x0, controls[:5])[0])  # (the plant matters)
