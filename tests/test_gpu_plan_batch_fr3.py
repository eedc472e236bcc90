"""jh_plan_step_batch_phases through the C ABI: B fr3_pick plan steps, each in its own phase, in one launch against B calls of jh_plan_step(..., phase_b, ...) on the
same sub-blocks.

Every comparison is on raw 32-bit words: the batched instantiation of the fr3 kernel runs the single call's code on pointers offset by the problem's strides and reads
the phase, the single call's argument, from a word of the problem's block; the single path is the one held to the oracle (tests/test_gpu_fr3.py,
tests/test_gpu_fr3_self_collision.py).  No tolerance appears in this file."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = {"mppi": (0, 0.05, 0, 0), "cem": (1, 0.0, 3, 1), "ps": (1, 0.0, 1, 0)}  # (mode, lambda, k, tie_high) of jh_update_fused
PAD_BLK, PAD_NOISE, PAD_OUT = 3, 8, 5  # the strides are larger than a block / a noise slice / an output record: what lies between must be skipped, not assumed away
K, E = 4, 2
# the two states of the overflow test (found with the oracle on the CPU, _pressed_states below): arm joints of a gripper pressed flat onto the table
# (the hand vertical, joint 6 = joint 2 - joint 4, and lowered until the twelve finger boxes lie on the table: 48 contacts each, up to 2.5 cm deep)
PRESSED_ARM = ((0.0, 0.6, 0.0, -2.3, 0.0, 2.9, 0.7854), (0.3, 0.8, 0.0, -1.85, 0.0, 2.65, 0.7854))


def _err():
    from judo_amd import _lib

    return _lib.lib().jh_last_error().decode()


def _home():
    from judo_amd.tasks import FR3Pick

    return FR3Pick().default_state()


def _phase_states():
    """The four phase states of test_fr3_plan_step_cem_matches_oracle: the cube at home (LIFT), at z = 0.05 (MOVE), above the goal (PLACE), on the goal (HOMING)."""
    xs = [_home() for _ in range(4)]
    xs[1][2] = 0.05
    xs[2][0:3] = [0.6, 0.4, 0.05]
    xs[3][0:3] = [0.6, 0.4, 0.02]
    return xs


class Problems:
    """B fr3_pick problems laid out for jh_plan_step_batch_phases -- x0 | nominal | sigma | task parameters | bounds | phase word, NaN between the blocks -- in a pinned host
    buffer with a device copy behind it; `single(b)` runs jh_plan_step with problem b's phase as its argument on problem b's sub-block, with buffers of its own.
    `shared`: every problem has problem 0's x0, nominal, sigma, task parameters and noise."""

    def __init__(self, dev, B, N, H, seed, x0s, phases, model=None, shared=False, sigma=None, plain=False):
        import torch

        from judo_amd import _lib
        from judo_amd.device import GpuModel
        from judo_amd.spline import spline_weights
        from judo_amd.tasks import FR3Pick

        self.lib, self.dev, self.B, self.N, self.H = _lib.lib(), dev, B, N, H
        task = FR3Pick()
        self.model = model if model is not None else GpuModel("fr3_pick", dev)
        nu, nx = task.nu, task.nq + task.nv
        self.nu, self.KU = nu, K * nu
        rng = np.random.default_rng(seed)
        tp0 = np.asarray(task.task_params({}), dtype=np.float32)
        self.sizes = [nx, self.KU, self.KU, len(tp0), 2 * nu, 1]
        self.off = [int(v) for v in np.cumsum([0] + self.sizes)]
        self.o_phase = self.off[5]
        self.nblk, self.blk_stride = self.off[-1], self.off[-1] + PAD_BLK
        r = task.actuator_ctrlrange
        lohi = np.nan_to_num(np.concatenate([r[:, 0], r[:, 1]]).astype(np.float32), posinf=3.0e38, neginf=-3.0e38)
        self.phases = [int(p) for p in phases]
        self.host = torch.full((B, self.blk_stride), float("nan"), dtype=torch.float32).pin_memory()  # (NaN between the blocks: a kernel that reads past a block's end shows)
        blocks = self.host.numpy()
        for b in range(B):
            x0 = np.asarray(x0s[b], dtype=np.float32)
            warm = np.tile(np.asarray(task.optimizer_warm_start(), dtype=np.float64), (K, 1))
            nominal = (warm + (0.0 if plain else 0.1) * rng.standard_normal((K, nu))).astype(np.float32).reshape(-1)
            sig = (0.05 + 0.2 * rng.random((K, nu))).astype(np.float32).reshape(-1) if sigma is None else np.asarray(sigma, dtype=np.float32).reshape(-1)
            tp = tp0 if plain else tp0 * (1.0 + 0.2 * rng.random(len(tp0))).astype(np.float32)
            blocks[b, : self.nblk] = np.concatenate([x0, nominal, sig, tp, lohi, [float(self.phases[b])]])
            if shared:
                blocks[b, : self.o_phase] = blocks[0, : self.o_phase]
        self.blocks_dev = torch.full((B * self.blk_stride,), float("nan"), dtype=torch.float32, device=dev)
        self.ldn = N + 4
        self.noise_stride = self.KU * self.ldn + PAD_NOISE
        noise = rng.standard_normal((B, self.noise_stride)).astype(np.float32)
        if shared:
            noise[:] = noise[0]
        self.noise = torch.from_numpy(noise).to(dev)
        dt = task.dt
        self.W = torch.from_numpy(spline_weights("linear", np.linspace(0, H * dt, K), dt * np.arange(H)).astype(np.float32)).to(dev)
        adr, nfl, cm = self.model.trace_layout()
        assert nfl == 6
        self.row, self.colmajor = H * nfl, int(cm)
        self.rec = 2 * self.KU + E * (2 + self.row)
        self.out_stride = self.rec + PAD_OUT
        self.per_scratch = int(self.lib.jh_update_fused_scratch_floats(N, K, nu))
        assert int(self.lib.jh_plan_batch_scratch_floats(B, N, K, nu)) == B * self.per_scratch
        self.batch_scratch = torch.zeros(B * self.per_scratch, dtype=torch.float32, device=dev)
        self.mark = torch.zeros(4, dtype=torch.int32).pin_memory()

    def call(self, costs, trace, out, opt="mppi", use_mark=False, B=None, model=None, o_phase=None, k=K):
        """The status of one jh_plan_step_batch_phases on the given outputs."""
        mode, lam, kk, tie = OPTS[opt]
        return self.lib.jh_plan_step_batch_phases((model or self.model).handle, self.B if B is None else B, self.blocks_dev.data_ptr(), self.host.data_ptr(), 4 * self.nblk, 4 * self.blk_stride,
                                                  self.off[1], self.off[2], self.off[3], self.off[4], self.o_phase if o_phase is None else o_phase, self.noise.data_ptr(), self.ldn,
                                                  self.noise_stride, self.W.data_ptr(), self.N, self.H, k, costs.data_ptr(), trace.data_ptr(), mode, lam, kk, tie, E, self.row, self.colmajor,
                                                  self.batch_scratch.data_ptr(), out.data_ptr(), self.out_stride, self.mark.data_ptr() if use_mark else out.data_ptr(), None, 0)

    def outputs(self, B=None):
        import torch

        B = self.B if B is None else B
        costs = torch.full((B, self.N), -7.0, dtype=torch.float32, device=self.dev)
        trace = torch.zeros(B * self.N * self.row, dtype=torch.float32, device=self.dev)
        out = torch.zeros((B, self.out_stride), dtype=torch.float32, device=self.dev)
        return costs, trace, out

    def batch(self, opt, use_mark=False):
        """One jh_plan_step_batch_phases over the B problems; returns (costs (B, N), out (B, rec)) as numpy."""
        import torch

        from judo_amd import _lib

        costs, trace, out = self.outputs()
        _lib.check(self.call(costs, trace, out, opt, use_mark), "jh_plan_step_batch_phases")
        _lib.check(self.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[:, self.rec :] == 0).all(), "the batch wrote between the output records"
        return costs.cpu().numpy(), o[:, : self.rec].copy()

    def single(self, opt, b, model=None):
        import torch

        from judo_amd import _lib

        mode, lam, k, tie = OPTS[opt]
        costs = torch.full((self.N,), -7.0, dtype=torch.float32, device=self.dev)
        trace = torch.zeros(self.N * self.row, dtype=torch.float32, device=self.dev)
        out = torch.zeros(self.rec, dtype=torch.float32, device=self.dev)
        scratch = torch.zeros(self.per_scratch, dtype=torch.float32, device=self.dev)
        blk = torch.full((self.nblk,), float("nan"), dtype=torch.float32, device=self.dev)
        st = self.lib.jh_plan_step((model or self.model).handle, blk.data_ptr(), self.host.data_ptr() + 4 * b * self.blk_stride, 4 * self.nblk, self.off[1], self.off[2], self.off[3], self.off[4],
                                   self.noise.data_ptr() + 4 * b * self.noise_stride, self.ldn, self.W.data_ptr(), self.phases[b], self.N, 0, self.H, K, costs.data_ptr(), None,
                                   trace.data_ptr(), mode, lam, k, tie, E, self.row, self.colmajor, scratch.data_ptr(), out.data_ptr(), out.data_ptr(), None, 0)
        _lib.check(st, "jh_plan_step")
        _lib.check(self.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        return costs.cpu().numpy(), out.cpu().numpy()

    def check(self, opt, got, which=None, what=""):
        costs, out = got
        for b in (range(self.B) if which is None else which):
            c1, o1 = self.single(opt, b)
            assert np.isfinite(c1).all()
            KU = self.KU
            for name, x, y in (("costs", costs[b], c1), ("nominal", out[b, :KU], o1[:KU]), ("sigma", out[b, KU : 2 * KU], o1[KU : 2 * KU]), ("trace records", out[b, 2 * KU :], o1[2 * KU :])):
                np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"{what} {opt} problem {b} (phase {self.phases[b]}): {name}")


# ------------------------------------------------------------------------------------------------ 1. the phase alone
@pytest.mark.parametrize("opt", ["mppi", "cem"])
def test_problems_that_differ_in_the_phase_word_only(gpu, opt):
    """B = 4, N = 6 (two groups of four rows, the second ragged), H = 8: one x0 -- the home pose with the cube above the goal, where the PLACE term and its object-table
    distance are live --, one nominal, sigma, task parameters and noise, and the phase word 0..3.  The four cost vectors differ pairwise and equal the single calls'."""
    x = _phase_states()[2]
    pr = Problems(gpu, 4, 6, 8, seed=3, x0s=[x] * 4, phases=range(4), shared=True)
    got = pr.batch(opt)
    assert len({got[0][b].tobytes() for b in range(4)}) == 4
    pr.check(opt, got, what="phase alone")


# ------------------------------------------------------------------------------------------------ 2. latency mode, distinct problems
@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
def test_four_problems_in_four_phases_in_latency_mode(gpu, opt):
    """B = 4, N = 6, H = 8: 24 rollouts select the latency mode, as each single call does; every problem has its phase state, nominal, sigma, noise and task parameters."""
    pr = Problems(gpu, 4, 6, 8, seed=4, x0s=_phase_states(), phases=range(4))
    pr.check(opt, pr.batch(opt), what="four phases")


# ------------------------------------------------------------------------------------------------ 3. the two other launch shapes
@pytest.mark.parametrize("B", [5, 9])
def test_launch_shapes_outside_the_full_latency_mode(gpu, B):
    """N = 256, H = 4.  B = 5: 1 280 rollouts, two rows of a wave per rollout; B = 9: 2 304 rollouts, every row its own rollout -- while a single call of 256 runs four
    rows per rollout.  Phases cycling; problems 0, 3 and B - 1."""
    xs = _phase_states()
    pr = Problems(gpu, B, 256, 4, seed=5 + B, x0s=[xs[b % 4] for b in range(B)], phases=[b % 4 for b in range(B)])
    pr.check("mppi", pr.batch("mppi"), which=(0, 3, B - 1), what=f"B*N={B * 256}")


# ------------------------------------------------------------------------------------------------ 4. overflow rows
@functools.lru_cache(maxsize=None)
def _pressed_states():
    """Two states with the gripper's pads pressed flat onto the table, and their numbers of general (non finger-finger) contacts by the oracle's forward pass on the
    CPU (the classification of test_fr3_general_contacts_beyond_the_lds_pool)."""
    from oracle import oracle as O

    om = O.Model("fr3_pick")
    gbody = [g["body"] for g in om.desc["geoms"]]
    fing = {i for i, b in enumerate(om.desc["bodies"]) if "finger" in b["name"]}
    xs, gen = [], []
    for arm in PRESSED_ARM:
        x = _home()
        x[7:14] = arm
        n = 0
        for r in om.forward(x[:16], x[16:], x[7:15])["contacts"]:
            n += not (gbody[int(r[13])] in fing and gbody[int(r[14])] in fing)
        xs.append(x)
        gen.append(n)
    return xs, gen


def test_overflow_rows_of_the_second_problem(gpu):
    """B = 2, N = 6, H = 4 from states with more than 32 general contacts: the contacts above the LDS pool live in a row of global memory per rollout, and problem 1's rows
    lie N behind problem 0's.  Nothing is dropped and the fallback is not taken."""
    xs, gen = _pressed_states()
    assert all(32 < n <= 96 for n in gen), gen
    pr = Problems(gpu, 2, 6, 4, seed=6, x0s=xs, phases=(0, 1), plain=True)
    pr.model.stats(reset=True)
    got = pr.batch("mppi")
    st = pr.model.stats(reset=True)
    assert st["overflow_pool_fallbacks"] == 0 and st["contact_overflow"] == 0, st
    pr.check("mppi", got, what="overflow rows")


# ------------------------------------------------------------------------------------------------ 5. the self-collision build
def test_self_collision_build(gpu):
    """The model of FR3Pick(self_collision=True).  B = 2, N = 24, H = 250 from the home pose with four times the CEM's sigma ramp (the workload of
    tests/test_gpu_fr3_self_collision.py).  Precondition: the same problems cost differently on the default build in at least one rollout, so a left-out pair touched."""
    from judo_amd.device import GpuModel
    from judo_amd.tasks import FR3Pick

    sigma = np.repeat(4.0 * np.clip(0.155 * np.linspace(1, 4, K), 0.01, 0.3), 8)
    model = GpuModel(FR3Pick(self_collision=True).desc, gpu)
    assert model.fr3_build()["self_collision_build"]
    pr = Problems(gpu, 2, 24, 250, seed=7, x0s=[_home()] * 2, phases=(0, 1), model=model, sigma=sigma, plain=True)
    default = GpuModel("fr3_pick", gpu)
    assert not default.fr3_build()["self_collision_build"]
    assert any((pr.single("mppi", b)[0] != pr.single("mppi", b, model=default)[0]).any() for b in range(2))
    pr.check("mppi", pr.batch("mppi"), what="self-collision build")


# ------------------------------------------------------------------------------------------------ 6. B = 1, the counters, the two completion marks
@pytest.mark.parametrize("use_mark", [True, False])
def test_batch_of_one_and_a_second_batch_on_the_same_scratch(gpu, use_mark):
    xs = _phase_states()
    one = Problems(gpu, 1, 6, 8, seed=8, x0s=xs[2:3], phases=(2,))
    one.check("cem", one.batch("cem", use_mark=use_mark), what="B=1")
    pr = Problems(gpu, 3, 6, 8, seed=9, x0s=xs[1:], phases=(1, 2, 3))
    old = 0xDEADBEEF
    pr.mark.numpy().view(np.uint32)[0] = old
    first = pr.batch("cem", use_mark=use_mark)
    second = pr.batch("cem", use_mark=use_mark)
    assert int(pr.mark.numpy().view(np.uint32)[0]) == ((old + 2) & 0xFFFFFFFF if use_mark else old)
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()
    assert (pr.batch_scratch.cpu().numpy().view(np.uint32).reshape(3, -1)[:, :4] == 0).all()  # every problem's ticket and the batch's are back at zero
    pr.check("cem", first, what="B=3")


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(gpu):
    import torch

    from judo_amd.device import GpuModel

    pr = Problems(gpu, 2, 6, 8, seed=10, x0s=_phase_states()[:2], phases=(0, 1))
    costs, trace, out = pr.outputs()
    word = pr.host.numpy()[:, pr.o_phase]
    for name in ("cartpole", "leap_cube"):
        assert pr.call(costs, trace, out, model=GpuModel(name, gpu)) == -3 and "jh_plan_step_batch" in _err()
    for bad in (4.0, 1.5, float("nan")):
        word[1] = bad
        assert pr.call(costs, trace, out) == -1 and "problem 1" in _err()
    word[1] = 1.0
    assert pr.call(costs, trace, out, o_phase=pr.nblk) == -1 and "o_phase" in _err()
    assert pr.call(costs, trace, out, o_phase=-1) == -1 and "o_phase" in _err()
    assert pr.call(costs, trace, out, k=9) == -1 and "at most 8 knots" in _err()
    assert pr.call(costs, trace, out, B=0) == -1 and "B must be" in _err()
    assert pr.call(costs, trace, out, B=65536) == -1 and "65535" in _err()
    torch.cuda.synchronize()
    assert (costs.cpu().numpy() == -7.0).all() and (trace.cpu().numpy() == 0).all() and (out.cpu().numpy() == 0).all()  # nothing ran
    pr.check("mppi", pr.batch("mppi"), what="after the refusals")
