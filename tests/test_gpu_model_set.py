"""jh_model_set_* and jh_plan_step_batch_models through the C ABI: B plan steps in one launch, every problem on its own image of the model's float section, against
jh_plan_step on each member's own model handle and sub-block.

Every comparison of the batched call is bit for bit (costs, nominal, sigma, trace records): the kernels offset the base of the float section by blockIdx.y * stride
and run the single call's code.  So that a kernel that ignored the stride could not pass, the problems of a case share ONE packed block and ONE noise slice and differ in
the model alone, and the single-call costs of every two members are required to differ in every rollout.  The one tolerance in this file is the oracle parity of a
perturbed image, at the bounds of tests/test_gpu_leap.py::test_leap_rollouts_and_costs_match_oracle."""

import copy
import ctypes as C
import functools

import numpy as np
import pytest

from tests.conftest import bounded
from tests.test_gpu_plan_batch import OPTS, PAD_BLK, PAD_NOISE, PAD_OUT, _err

pytestmark = pytest.mark.gpu

# the perturbed members (keyword arguments of models.scaled_description); member 0 of every case is the shipped description
CARTPOLE = [dict(body_mass={"pole": 1.5}), dict(body_mass={"pole": 0.7}, actuator_kp={None: 1.2})]
CYLINDER = [dict(body_mass={"pusher": 1.5}), dict(body_mass={"cart": 0.6}, actuator_kp={None: 1.2})]
LEAP_A, LEAP_B, LEAP_C = dict(body_mass={"cube": 1.5}, geom_friction={"cube": 0.6}), dict(actuator_kp={None: 1.2}), dict(body_mass={"cube": 0.7}, geom_friction={"cube": 1.3}, actuator_kp={None: 0.85})


def _task(name):
    from judo_amd.tasks import CaltechLeapCube, get_registered_tasks

    return CaltechLeapCube(fingertips="cylinder") if name == "caltech_cylinder" else get_registered_tasks()[name][0]()


def _models(dev, name, perturbations):
    """The shipped model of `name` and one model per perturbation, each with a handle of its own."""
    from judo_amd.device import GpuModel
    from judo_amd.models import scaled_description

    desc = _task(name).desc
    return [GpuModel(copy.deepcopy(desc), dev)] + [GpuModel(scaled_description(desc, **kw), dev) for kw in perturbations]


@functools.lru_cache(maxsize=None)
def _settled(name, steps):
    """The state after `steps` oracle steps from the task's home state under its home control (computed once, on the CPU).  From the home state itself the cube is in free
    fall over a short horizon, and neither its mass nor its friction nor the cost would notice the image: leap_cube and caltech_leap_cube take 60 steps, after which
    the cube rests in the hand; leap_cube_down 5 -- its hand faces down and the cube slides off the fingers within a dozen steps."""
    from oracle import oracle as O

    task = _task(name)
    x0 = task.default_state()
    om = O.Model("caltech_leap_cube" if name == "caltech_cylinder" else name)
    rs, _ = om.rollout(x0, np.tile(x0[7:23], (1, steps, 1)))
    return rs[0, -1].copy()


class SetProblems:
    """B problems of one task that share ONE packed block (x0 | nominal | sigma | task params | bounds) and ONE noise slice, each repeated at the strides of
    tests/test_gpu_plan_batch.py, and differ in the model: problem b belongs to models[b].  `single(b)` is jh_plan_step on models[b]'s handle and problem b's sub-block.
    A model whose kernel writes no trace rows (caltech_leap_cube) is planned without trace records."""

    def __init__(self, dev, task_name, models, N, K, H, E, seed, x0, sigma=None, distinct_problems=False):
        import torch

        from judo_amd import _lib
        from judo_amd.device import GpuModelSet
        from judo_amd.spline import spline_weights

        self.lib, self.dev, self.B, self.N, self.K, self.H = _lib.lib(), dev, len(models), N, K, H
        self.models, self.model = list(models), models[0]
        B = self.B
        task = _task(task_name)
        nu, nx = task.nu, task.nq + task.nv
        self.nu, self.KU = nu, K * nu
        rng = np.random.default_rng(seed)
        tp = np.asarray(task.task_params({}), dtype=np.float32)
        self.sizes = [nx, self.KU, self.KU, len(tp), 2 * nu]
        self.off = [int(v) for v in np.cumsum([0] + self.sizes)]
        self.nblk, self.blk_stride = self.off[-1], self.off[-1] + PAD_BLK
        r = task.actuator_ctrlrange
        lohi = np.nan_to_num(np.concatenate([r[:, 0], r[:, 1]]).astype(np.float32), posinf=3.0e38, neginf=-3.0e38)
        blocks = np.full((B, self.blk_stride), np.nan, dtype=np.float32)  # (NaN between the blocks: a kernel that reads past a block's end shows)
        self.ldn = N + 4
        self.noise_stride = self.KU * self.ldn + PAD_NOISE
        noise = np.zeros((B, self.noise_stride), dtype=np.float32)
        for b in range(B):
            if b == 0 or distinct_problems:
                warm = np.tile(np.asarray(task.optimizer_warm_start(), dtype=np.float64), (K, 1))
                nominal = (warm + 0.1 * rng.standard_normal((K, nu))).astype(np.float32).reshape(-1)
                sig = (0.05 + 0.2 * rng.random((K, nu))).astype(np.float32).reshape(-1) if sigma is None else np.full(self.KU, sigma, dtype=np.float32)
                blocks[b, : self.nblk] = np.concatenate([np.asarray(x0, dtype=np.float32), nominal, sig, tp, lohi])
                noise[b] = rng.standard_normal(self.noise_stride).astype(np.float32)
            else:
                blocks[b], noise[b] = blocks[0], noise[0]
        self.blocks, self.noise = torch.from_numpy(blocks).to(dev), torch.from_numpy(noise).to(dev)
        dt = task.dt
        self.W = torch.from_numpy(spline_weights("linear", np.linspace(0, H * dt, K), dt * np.arange(H)).astype(np.float32)).to(dev)
        _, nfl, cm = self.model.trace_layout()
        self.traced = nfl > 0
        self.E = E if self.traced else 0
        self.row, self.colmajor = H * nfl, int(cm)
        self.rec = 2 * self.KU + self.E * (2 + self.row)
        self.out_stride = self.rec + PAD_OUT
        self.per_scratch = int(self.lib.jh_update_fused_scratch_floats(N, K, nu))
        self.batch_scratch = torch.zeros(B * self.per_scratch, dtype=torch.float32, device=dev)
        self.mark = torch.zeros(4, dtype=torch.int32).pin_memory()
        self.set = GpuModelSet(models)

    def _batch(self, opt, use_mark, shared_model):
        import torch

        from judo_amd import _lib

        B = self.B
        mode, lam, k, tie = OPTS[opt]
        costs = torch.full((B, self.N), -7.0, dtype=torch.float32, device=self.dev)
        trace = torch.zeros(B * self.N * self.row, dtype=torch.float32, device=self.dev) if self.traced else None
        out = torch.zeros((B, self.out_stride), dtype=torch.float32, device=self.dev)
        p = self.blocks.data_ptr()
        tail = (p, p, 4 * self.nblk, 4 * self.blk_stride, self.off[1], self.off[2], self.off[3], self.off[4], self.noise.data_ptr(), self.ldn, self.noise_stride, self.W.data_ptr(), self.N, self.H,
                self.K, costs.data_ptr(), _lib.ptr(trace), mode, lam, k, tie, self.E, self.row, self.colmajor, self.batch_scratch.data_ptr(), out.data_ptr(), self.out_stride,
                self.mark.data_ptr() if use_mark else out.data_ptr(), None, 0)
        if shared_model is None:
            _lib.check(self.lib.jh_plan_step_batch_models(self.set.handle, *tail), "jh_plan_step_batch_models")
        else:
            _lib.check(self.lib.jh_plan_step_batch(shared_model.handle, B, *tail), "jh_plan_step_batch")
        _lib.check(self.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[:, self.rec :] == 0).all(), "the batch wrote between the output records"
        return costs.cpu().numpy(), o[:, : self.rec].copy()

    def batch_models(self, opt, use_mark=False):
        """One jh_plan_step_batch_models on the set; returns (costs (B, N), out (B, rec)) as numpy."""
        return self._batch(opt, use_mark, None)

    def batch_shared(self, opt, model):
        """One jh_plan_step_batch of the same B problems on one model."""
        return self._batch(opt, False, model)

    def single(self, opt, b):
        import torch

        from judo_amd import _lib

        mode, lam, k, tie = OPTS[opt]
        costs = torch.full((self.N,), -7.0, dtype=torch.float32, device=self.dev)
        trace = torch.zeros(self.N * self.row, dtype=torch.float32, device=self.dev) if self.traced else None
        out = torch.zeros(self.rec, dtype=torch.float32, device=self.dev)
        scratch = torch.zeros(self.per_scratch, dtype=torch.float32, device=self.dev)
        p = self.blocks.data_ptr() + 4 * b * self.blk_stride
        st = self.lib.jh_plan_step(self.models[b].handle, p, p, 4 * self.nblk, self.off[1], self.off[2], self.off[3], self.off[4], self.noise.data_ptr() + 4 * b * self.noise_stride, self.ldn,
                                   self.W.data_ptr(), 0, self.N, 0, self.H, self.K, costs.data_ptr(), None, _lib.ptr(trace), mode, lam, k, tie, self.E, self.row, self.colmajor,
                                   scratch.data_ptr(), out.data_ptr(), out.data_ptr(), None, 0)
        _lib.check(st, "jh_plan_step")
        _lib.check(self.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        return costs.cpu().numpy(), out.cpu().numpy()

    def check(self, opt, got, what=""):
        """Problem b of the batched call against jh_plan_step on member b: costs, nominal, sigma and the E trace records, bit for bit."""
        costs, out = got
        KU = self.KU
        for b in range(self.B):
            c1, o1 = self.single(opt, b)
            assert np.isfinite(c1).all()
            for name, x, y in (("costs", costs[b], c1), ("nominal", out[b, :KU], o1[:KU]), ("sigma", out[b, KU : 2 * KU], o1[KU : 2 * KU]), ("trace records", out[b, 2 * KU :], o1[2 * KU :])):
                np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"{what} {opt} problem {b}: {name}")

    def teeth(self, opt):
        """The members are different plants: the single-call costs of every two of them differ in EVERY rollout (same block, same noise)."""
        costs = [self.single(opt, b)[0] for b in range(self.B)]
        for a in range(self.B):
            for b in range(a + 1, self.B):
                same = int((costs[a] == costs[b]).sum())
                rel = np.abs(costs[a] - costs[b]) / np.abs(costs[a])
                print(f"teeth: members {a} / {b}: {same} of {self.N} rollouts with equal costs, smallest relative difference {rel.min():.3e}")
                assert same == 0, f"members {a} and {b} give the same cost in {same} of {self.N} rollouts: the case cannot tell their images apart"

    def tickets(self):
        return self.batch_scratch.cpu().numpy().view(np.uint32).reshape(self.B, -1)[:, :4]


# ------------------------------------------------------------------------------------------------ 1. closed-form models
@pytest.mark.parametrize("launches", [1, 2])
@pytest.mark.parametrize("task,opt", [("cartpole", "mppi"), ("cartpole", "cem"), ("cylinder_push", "mppi")])
def test_closed_form_set_equals_single_calls(gpu, task, opt, launches):
    """B = 3 (a distinct image at problem 0, in the middle and last), N = 300 (two workgroups of the one-launch form, the second ragged), H = 8, K = 4, E = 3, as one
    launch and as two.  A second call on the same scratch gives the same bytes and leaves the B + 1 tickets at zero; the completion word counts both."""
    models = _models(gpu, task, CARTPOLE if task == "cartpole" else CYLINDER)
    for m in models:
        m.set_plan_step_launches(launches)
    if task == "cartpole":
        pr = SetProblems(gpu, task, models, 300, 4, 8, 3, seed=3, x0=[0.1, 0.3, 0.0, 0.0])
    else:
        pr = SetProblems(gpu, task, models, 300, 4, 8, 3, seed=4, x0=[0.0, 0.0, -0.5, 0.0, 0.0, 0.0, 0.0, 0.0], sigma=3.0)
    info = pr.set.info()
    assert info == {"B": 3, "image_floats": len(models[0]._blob[64:]) // 4, "stride_floats": 64, "distinct_from_first": 2}, info
    pr.teeth(opt)
    models[0].stats(reset=True)
    old = 0xFFFFFFFF
    pr.mark.numpy().view(np.uint32)[0] = old
    first = pr.batch_models(opt, use_mark=True)
    assert int(pr.mark.numpy().view(np.uint32)[0]) == 0
    assert models[0].stats(reset=True)["one_launch_plan_steps"] == (1 if launches == 1 else 0)  # (a set's counters are member 0's)
    pr.check(opt, first, what=f"{task} set launches={launches}")
    second = pr.batch_models(opt, use_mark=True)
    assert int(pr.mark.numpy().view(np.uint32)[0]) == 1
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()
    assert (pr.tickets() == 0).all()


def test_update_replaces_one_member(gpu):
    """jh_model_set_update of member 1: problem 1 then has the new model's single-call bits, problems 0 and 2 the bits they had."""
    from judo_amd.device import GpuModel
    from judo_amd.models import scaled_description

    models = _models(gpu, "cartpole", CARTPOLE)
    pr = SetProblems(gpu, "cartpole", models, 300, 4, 8, 3, seed=5, x0=[0.1, 0.3, 0.0, 0.0])
    before = pr.batch_models("mppi")
    new = GpuModel(scaled_description(_task("cartpole").desc, body_mass={"pole": 2.0, "cart": 0.8}), gpu)
    pr.set.update(1, new)
    pr.models[1] = new
    assert pr.set.info()["distinct_from_first"] == 2
    after = pr.batch_models("mppi")
    pr.check("mppi", after, what="cartpole after update")
    for x, y in zip(before, after):
        assert x[0].tobytes() == y[0].tobytes() and x[2].tobytes() == y[2].tobytes()
        assert (x[1] != y[1]).any()
    assert (before[0][1] != after[0][1]).all()  # every rollout of problem 1 ran on another plant
    pr.set.update(1, models[0])  # ... and member 0's own image in place 1: one member left that differs
    assert pr.set.info()["distinct_from_first"] == 1
    with pytest.raises(ValueError, match="member 3"):
        pr.set.update(3, new)
    pr.set.close()
    pr.set.close()  # (idempotent)


@pytest.mark.parametrize("task", ["cartpole", "leap_cube"])
def test_set_of_identical_handles_equals_plan_step_batch(gpu, task):
    """B times the same handle: the set call gives bit for bit what jh_plan_step_batch gives on the same buffers (B distinct blocks and noise slices here)."""
    from judo_amd.device import GpuModel

    model = GpuModel(task, gpu)
    if task == "cartpole":
        pr = SetProblems(gpu, task, [model] * 3, 300, 4, 8, 3, seed=8, x0=[0.1, 0.3, 0.0, 0.0], distinct_problems=True)
    else:
        pr = SetProblems(gpu, task, [model] * 3, 6, 4, 8, 1, seed=8, x0=_settled("leap_cube", 60), distinct_problems=True)
    assert pr.set.info()["distinct_from_first"] == 0
    want = pr.batch_shared("mppi", model)
    assert len({want[0][b].tobytes() for b in range(3)}) == 3
    got = pr.batch_models("mppi")
    for x, y in zip(want, got):
        assert x.tobytes() == y.tobytes()
    assert (pr.tickets() == 0).all()


# ------------------------------------------------------------------------------------------------ 2. the leap family
def test_leap_set_in_latency_mode(gpu):
    """leap_cube from the settled state, B = 3 (base, A, B), N = 6 (one full group of four rollouts, one ragged), H = 8, K = 4, E = 1, MPPI; then member 1 is replaced
    by the third perturbation."""
    from judo_amd.device import GpuModel
    from judo_amd.models import scaled_description

    models = _models(gpu, "leap_cube", [LEAP_A, LEAP_B])
    pr = SetProblems(gpu, "leap_cube", models, 6, 4, 8, 1, seed=22, x0=_settled("leap_cube", 60))
    assert pr.set.info()["B"] == 3 and pr.set.info()["stride_floats"] % 64 == 0 and pr.set.info()["distinct_from_first"] == 2
    pr.teeth("mppi")
    first = pr.batch_models("mppi")
    pr.check("mppi", first, what="leap_cube set, latency mode")
    second = pr.batch_models("mppi")
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()
    assert (pr.tickets() == 0).all()
    new = GpuModel(scaled_description(_task("leap_cube").desc, **LEAP_C), gpu)
    pr.set.update(1, new)
    pr.models[1] = new
    pr.teeth("mppi")
    after = pr.batch_models("mppi")
    pr.check("mppi", after, what="leap_cube set after update")
    assert after[0][0].tobytes() == first[0][0].tobytes() and after[0][2].tobytes() == first[0][2].tobytes()


def test_leap_set_outside_latency_mode(gpu):
    """B = 3, N = 352, H = 4: 1 056 rollouts in the launch, every row of a wave its own rollout (the latency mode is chosen from B * N), while each single call of 352
    still runs it."""
    models = _models(gpu, "leap_cube", [LEAP_A, LEAP_B])
    pr = SetProblems(gpu, "leap_cube", models, 352, 4, 4, 1, seed=32, x0=_settled("leap_cube", 60))
    pr.teeth("mppi")
    pr.check("mppi", pr.batch_models("mppi"), what="leap_cube set B*N=1056")


@pytest.mark.parametrize("task,steps,build", [("leap_cube_down", 5, dict(contact_capacity=64, cylinder_build=False)), ("caltech_cylinder", 60, dict(contact_capacity=64, cylinder_build=True))])
def test_leap_set_on_the_other_builds(gpu, task, steps, build):
    """The 64-contact build (leap_cube_down) and the cylinder build (caltech_leap_cube with its fingertip cylinders): B = 2 (base, A), N = 4, H = 4."""
    models = _models(gpu, task, [LEAP_A])
    got = models[0].build()
    assert {k: got[k] for k in build} == build
    pr = SetProblems(gpu, task, models, 4, 4, 4, 1, seed=42, x0=_settled(task, steps))
    pr.teeth("mppi")
    models[0].stats(reset=True)
    res = pr.batch_models("mppi")
    assert models[0].stats(reset=True)["overflow_pool_fallbacks"] == 0
    pr.check("mppi", res, what=f"{task} set")


# ------------------------------------------------------------------------------------------------ 3. refusals
def _create(models, B=None):
    from judo_amd import _lib

    hs = (C.c_void_p * len(models))(*[m.handle.value for m in models])
    out = C.c_void_p()
    st = _lib.lib().jh_model_set_create(hs, len(models) if B is None else B, C.byref(out))
    if st == 0:
        _lib.lib().jh_model_set_destroy(out)
    return st


def test_set_refusals(gpu):
    from judo_amd.device import GpuModel, GpuModelSet
    from judo_amd.models import scaled_description

    desc = _task("leap_cube").desc
    leap, leap64 = GpuModel(desc, gpu), GpuModel(scaled_description(desc, **LEAP_A), gpu)
    assert _create([leap, leap64]) == 0
    leap64.set_contact_capacity(64)  # a mixed contact capacity
    assert _create([leap, leap64]) == -1 and "member 1" in _err() and "contact_capacity" in _err()
    leap64.set_contact_capacity(48)
    leap64.set_self_collision(False)
    assert _create([leap, leap64]) == -1 and "member 1" in _err() and "self_collision" in _err()
    leap64.set_self_collision(True)
    leap64.set_rollout_schedule(1)
    assert _create([leap, leap, leap64]) == -1 and "member 2" in _err() and "rollout_schedule" in _err()
    leap64.set_rollout_schedule(0)
    assert _create([leap, leap64]) == 0
    edited = copy.deepcopy(desc)  # a hand-edited description whose int section differs: another <exclude> pair (palm / if_bs collide, if_px / mf_px do not) -- same lengths, other pair lists
    edited["excludes"][0] = [6, 10]
    assert _create([leap, GpuModel(edited, gpu)]) == -1 and "member 1" in _err() and "h_i" in _err()
    edited["excludes"] = desc["excludes"][1:]  # ... and one pair less: a longer int section
    assert _create([leap, leap, GpuModel(edited, gpu)]) == -1 and "member 2" in _err() and "ni" in _err()
    skew = copy.deepcopy(desc)  # an anisotropic cube inertia: the leap kernel's own acceptance test, which reads the image's floats
    cube = next(b for b in skew["bodies"] if b["name"] == "cube")
    cube["inertia"] = [cube["inertia"][0], cube["inertia"][1], 1.25 * cube["inertia"][2]]
    assert _create([leap, GpuModel(skew, gpu)]) == -3 and "member 1" in _err() and "inertia" in _err() and "h_f" in _err()
    assert _create([GpuModel(skew, gpu)]) == -3 and "member 0" in _err()
    assert _create([GpuModel("fr3_pick", gpu)]) == -3 and "member 0" in _err() and "fr3_pick" in _err()
    old = GpuModel(desc, gpu)
    old.set_kernel(2)  # (a cross-check generation of the test build)
    assert _create([old]) == -3 and "member 0" in _err() and "kernel_gen" in _err()
    cart, cyl = GpuModel("cartpole", gpu), GpuModel("cylinder_push", gpu)
    assert _create([cart, cyl]) == -1 and "member 1" in _err() and "kind" in _err()
    two = GpuModel("cartpole", gpu)
    two.set_plan_step_launches(2)
    assert _create([cart, two]) == -1 and "member 1" in _err() and "plan_step_launches" in _err()
    assert _create([cart], B=0) == -1 and "B must be" in _err()
    assert _create([cart], B=65536) == -1 and "65535" in _err()
    with pytest.raises(ValueError, match="contact_capacity|member"):
        leap64.set_contact_capacity(64)
        GpuModelSet([leap, leap64])
    s = GpuModelSet([cart, cart])
    with pytest.raises(ValueError, match="kind"):
        s.update(1, cyl)
    assert s.info()["distinct_from_first"] == 0  # (a refused update changes nothing)


# ------------------------------------------------------------------------------------------------ 4. the packer carries the perturbation as the oracle reads it
def test_perturbed_leap_image_matches_the_oracle_on_the_same_description(gpu):
    """leap member A (cube mass x 1.5, cube friction x 0.6) from the settled state, N = 64, H = 16: `GpuRolloutBackend` on the packed perturbed description against
    `O.Model("leap_cube", desc=<the same description>)`, with the assertions and bounds of test_leap_rollouts_and_costs_match_oracle.  The controls are that test's
    (seed 3, chosen on the oracle alone: its own costs for member A and for the base model then differ by more than 8e-5 on every rollout, 160 times the median bound,
    so an ignored perturbation cannot pass)."""
    from judo_amd.device import GpuModel
    from judo_amd.models import scaled_description
    from judo_amd.rollout_backend import GpuRolloutBackend
    from judo_amd.tasks import LeapCube
    from oracle import oracle as O
    from tests.test_gpu_leap import GOAL, _mppi_controls

    N = 64
    om, _, U, _ = _mppi_controls(N, H=16, seed=3)
    desc_a = scaled_description(om.desc, **LEAP_A)
    x0 = _settled("leap_cube", 60)
    rs, _ = O.Model("leap_cube", desc=desc_a).rollout(x0, U)
    cr = -O.reward_leap(rs, GOAL["goal_quat"])
    cr_base = -O.reward_leap(om.rollout(x0, U)[0], GOAL["goal_quat"])
    print(f"oracle, member A against the base model: smallest cost difference over the rollouts {np.abs(cr - cr_base).min():.3e}")
    assert np.abs(cr - cr_base).min() >= 8e-5
    gs, gsens, _ = GpuRolloutBackend(GpuModel(desc_a, gpu), N).rollout(x0, U)
    assert gs.shape == rs.shape and np.isfinite(gs).all()
    err = np.abs(gs - rs)
    cg = -LeapCube().reward(gs, gsens, U, GOAL)
    d = np.abs(cr - cg)
    print(f"perturbed image against the oracle: cost error median {np.median(d):.3e}, 95th percentile {np.percentile(d, 95):.3e}; cube position at the horizon median "
          f"{np.median(err[:, -1, :3]):.3e}, 95th percentile {np.percentile(err[:, -1, :3], 95):.3e}")
    assert bounded("np.median(err[:, -1, :3])", np.median(err[:, -1, :3]), 3e-8) and bounded("np.percentile(err[:, -1, :3], 95)", np.percentile(err[:, -1, :3], 95), 5e-7)
    assert bounded("np.median(np.abs(cr - cg))", np.median(d), 5e-7) and bounded("np.percentile(np.abs(cr - cg), 95)", np.percentile(d, 95), 1.5e-6)
