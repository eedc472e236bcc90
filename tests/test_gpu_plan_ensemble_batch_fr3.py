"""jh_plan_step_ensemble_batch_phases through the C ABI: B fr3_pick ensemble plan steps, each in its own phase, in one launch of the fr3 kernel on the grid
(workgroups, M, B) against B calls of jh_plan_step_ensemble_phase on the same sub-blocks.

Every comparison is on raw 32-bit words: the controller axis offsets the kernel's pointers once, at its top, and the code below is the single launch's; the single entry
is held to jh_plan_step by tests/test_gpu_plan_ensemble_fr3.py.  No tolerance appears in this file.  `Blocks` lays B controllers out as tests/test_gpu_plan_batch_fr3.py
does (x0 | nominal | sigma | task parameters | bounds | phase word, NaN between the blocks, padded strides) for any K, and carries the calls of both batched entries."""

import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_plan_batch_fr3 import OPTS, PAD_BLK, PAD_NOISE, PAD_OUT, _err, _phase_states, _pressed_states
from tests.test_gpu_plan_batch_fr3_models import _models

pytestmark = pytest.mark.gpu


class Blocks:
    """B fr3_pick controllers' packed blocks with a phase word each, in a pinned host buffer with a device copy behind it, their noise, and buffers for the outputs of a
    batched call.  `shared`: every controller has controller 0's x0, nominal, sigma, task parameters and noise, so that only the phase word differs."""

    def __init__(self, dev, B, N, H, K, seed, x0s, phases, shared=False, plain=False):
        import torch

        from judo_amd import _lib
        from judo_amd.spline import spline_weights
        from judo_amd.tasks import FR3Pick

        self.lib, self.dev, self.B, self.N, self.H, self.K = _lib.lib(), dev, B, N, H, K
        task = FR3Pick()
        nu, nx = task.nu, task.nq + task.nv
        self.nu, self.KU = nu, K * nu
        rng = np.random.default_rng(seed)
        tp0 = np.asarray(task.task_params({}), dtype=np.float32)
        self.off = [int(v) for v in np.cumsum([0, nx, self.KU, self.KU, len(tp0), 2 * nu, 1])]
        self.o_phase = self.off[5]
        self.nblk, self.blk_stride = self.off[-1], self.off[-1] + PAD_BLK
        r = task.actuator_ctrlrange
        lohi = np.nan_to_num(np.concatenate([r[:, 0], r[:, 1]]).astype(np.float32), posinf=3.0e38, neginf=-3.0e38)
        self.phases = [int(p) for p in phases]
        self.host = torch.full((B, self.blk_stride), float("nan"), dtype=torch.float32).pin_memory()  # (NaN between the blocks: a kernel that reads past a block's end shows)
        blocks = self.host.numpy()
        for b in range(B):
            warm = np.tile(np.asarray(task.optimizer_warm_start(), dtype=np.float64), (K, 1))
            nominal = (warm + (0.0 if plain else 0.1) * rng.standard_normal((K, nu))).astype(np.float32).reshape(-1)
            sig = (0.05 + 0.2 * rng.random((K, nu))).astype(np.float32).reshape(-1)
            tp = tp0 if plain else tp0 * (1.0 + 0.2 * rng.random(len(tp0))).astype(np.float32)
            blocks[b, : self.nblk] = np.concatenate([np.asarray(x0s[b], dtype=np.float32), nominal, sig, tp, lohi, [float(self.phases[b])]])
            if shared:
                blocks[b, : self.o_phase] = blocks[0, : self.o_phase]
        self.blocks_dev = torch.full((B * self.blk_stride,), float("nan"), dtype=torch.float32, device=dev)
        self.ldn = N + 4
        self.noise_stride = self.KU * self.ldn + PAD_NOISE
        noise = rng.standard_normal((B, self.noise_stride)).astype(np.float32)
        if shared:
            noise[:] = noise[0]
        self.noise = torch.from_numpy(noise).to(dev)
        self.W = torch.from_numpy(spline_weights("linear", np.linspace(0, H * task.dt, K), task.dt * np.arange(H)).astype(np.float32)).to(dev)
        self.rec = 2 * self.KU
        self.out_stride = self.rec + PAD_OUT
        self.per_scratch = int(self.lib.jh_update_fused_scratch_floats(N, K, nu))
        self.batch_scratch = torch.zeros(int(self.lib.jh_plan_batch_scratch_floats(B, N, K, nu)), dtype=torch.float32, device=dev)
        self.mark = torch.zeros(4, dtype=torch.int32).pin_memory()

    def outputs(self, M=1):
        import torch

        mc = torch.full((self.B, M, self.N), -7.0, dtype=torch.float32, device=self.dev)
        costs = torch.full((self.B, self.N), -7.0, dtype=torch.float32, device=self.dev)
        out = torch.zeros((self.B, self.out_stride), dtype=torch.float32, device=self.dev)
        return mc, costs, out

    def _finish(self, st, what, out):
        import torch

        from judo_amd import _lib

        _lib.check(st, what)
        _lib.check(self.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[:, self.rec :] == 0).all(), "the batch wrote between the output records"
        return o[:, : self.rec].copy()

    # ---- the ensemble entries
    def ens_raw(self, set_, M, worst, bufs, opt="mppi", use_mark=False, B=None, o_phase=None):
        """The status of one jh_plan_step_ensemble_batch_phases on the given outputs."""
        mode, lam, k, tie = OPTS[opt]
        mc, costs, out = bufs
        B = self.B if B is None else B
        return self.lib.jh_plan_step_ensemble_batch_phases(set_.handle, B, M, self.blocks_dev.data_ptr(), self.host.data_ptr(), 4 * self.nblk, 4 * self.blk_stride, self.off[1], self.off[2],
                                                           self.off[3], self.off[4], self.o_phase if o_phase is None else o_phase, self.noise.data_ptr(), self.ldn, self.noise_stride,
                                                           self.W.data_ptr(), self.N, self.H, self.K, mc.data_ptr(), costs.data_ptr(), (C.c_int * len(worst))(*worst), mode, lam, k, tie,
                                                           self.batch_scratch.data_ptr(), out.data_ptr(), self.out_stride, self.mark.data_ptr() if use_mark else out.data_ptr(), None, 0)

    def ens_batch(self, set_, M, worst, opt="mppi", use_mark=False):
        """(member_costs (B, M, N), costs (B, N), out (B, 2 KU)) of one batched call."""
        bufs = self.outputs(M)
        o = self._finish(self.ens_raw(set_, M, worst, bufs, opt, use_mark), "jh_plan_step_ensemble_batch_phases", bufs[2])
        return bufs[0].cpu().numpy(), bufs[1].cpu().numpy(), o

    def ens_single(self, set_, opt, b, worst):
        """(member_costs (M, N), costs (N,), out (2 KU,)) of jh_plan_step_ensemble_phase on controller b's sub-block and noise, in its phase, with buffers of its own."""
        import torch

        from judo_amd import _lib

        mode, lam, k, tie = OPTS[opt]
        M = set_.info()["B"]
        mc = torch.full((M, self.N), -7.0, dtype=torch.float32, device=self.dev)
        costs = torch.full((self.N,), -7.0, dtype=torch.float32, device=self.dev)
        out = torch.zeros(self.rec, dtype=torch.float32, device=self.dev)
        scratch = torch.zeros(self.per_scratch, dtype=torch.float32, device=self.dev)
        blk = torch.full((self.nblk,), float("nan"), dtype=torch.float32, device=self.dev)
        st = self.lib.jh_plan_step_ensemble_phase(set_.handle, blk.data_ptr(), self.host.data_ptr() + 4 * b * self.blk_stride, 4 * self.nblk, self.off[1], self.off[2], self.off[3], self.off[4],
                                                  self.noise.data_ptr() + 4 * b * self.noise_stride, self.ldn, self.W.data_ptr(), self.phases[b], self.N, self.H, self.K, mc.data_ptr(),
                                                  costs.data_ptr(), worst, mode, lam, k, tie, scratch.data_ptr(), out.data_ptr(), out.data_ptr(), None, 0)
        _lib.check(st, "jh_plan_step_ensemble_phase")
        _lib.check(self.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        c = costs.cpu().numpy()
        assert np.isfinite(c).all()
        return mc.cpu().numpy(), c, out.cpu().numpy()

    def ens_check(self, sets, opt, worst, got, what=""):
        """`sets[b]`: the set of controller b's M plants."""
        for b in range(self.B):
            for name, x, y in zip(("member_costs", "costs", "nominal | sigma"), (g[b] for g in got), self.ens_single(sets[b], opt, b, worst[b])):
                np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"{what} {opt} controller {b} (phase {self.phases[b]}, worst {worst[b]}): {name}")

    # ---- the randomised entries
    def rnd_raw(self, set_, M, tables, bufs, opt="mppi", use_mark=False, B=None, o_phase=None):
        """The status of one jh_plan_step_randomized_batch_phases on the given outputs; `tables`: B lists of G plants."""
        mode, lam, k, tie = OPTS[opt]
        _, costs, out = bufs
        B = self.B if B is None else B
        flat = [p for a in tables for p in a]
        return self.lib.jh_plan_step_randomized_batch_phases(set_.handle, B, M, self.blocks_dev.data_ptr(), self.host.data_ptr(), 4 * self.nblk, 4 * self.blk_stride, self.off[1], self.off[2],
                                                             self.off[3], self.off[4], self.o_phase if o_phase is None else o_phase, self.noise.data_ptr(), self.ldn, self.noise_stride,
                                                             self.W.data_ptr(), self.N, self.H, self.K, (C.c_ubyte * len(flat))(*flat), len(tables[0]), costs.data_ptr(), mode, lam, k, tie,
                                                             self.batch_scratch.data_ptr(), out.data_ptr(), self.out_stride, self.mark.data_ptr() if use_mark else out.data_ptr(), None, 0)

    def rnd_batch(self, set_, M, tables, opt="mppi", use_mark=False):
        """(costs (B, N), out (B, 2 KU)) of one batched call."""
        bufs = self.outputs()
        o = self._finish(self.rnd_raw(set_, M, tables, bufs, opt, use_mark), "jh_plan_step_randomized_batch_phases", bufs[2])
        return bufs[1].cpu().numpy(), o

    def rnd_single(self, set_, opt, b, table):
        """(costs (N,), out (2 KU,)) of jh_plan_step_randomized_phase on controller b's sub-block and noise, in its phase, with buffers of its own."""
        import torch

        from judo_amd import _lib

        mode, lam, k, tie = OPTS[opt]
        costs = torch.full((self.N,), -7.0, dtype=torch.float32, device=self.dev)
        out = torch.zeros(self.rec, dtype=torch.float32, device=self.dev)
        scratch = torch.zeros(self.per_scratch, dtype=torch.float32, device=self.dev)
        blk = torch.full((self.nblk,), float("nan"), dtype=torch.float32, device=self.dev)
        st = self.lib.jh_plan_step_randomized_phase(set_.handle, blk.data_ptr(), self.host.data_ptr() + 4 * b * self.blk_stride, 4 * self.nblk, self.off[1], self.off[2], self.off[3], self.off[4],
                                                    self.noise.data_ptr() + 4 * b * self.noise_stride, self.ldn, self.W.data_ptr(), self.phases[b], self.N, self.H, self.K,
                                                    (C.c_ubyte * len(table))(*table), len(table), costs.data_ptr(), mode, lam, k, tie, scratch.data_ptr(), out.data_ptr(), out.data_ptr(), None, 0)
        _lib.check(st, "jh_plan_step_randomized_phase")
        _lib.check(self.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        c = costs.cpu().numpy()
        assert np.isfinite(c).all()
        return c, out.cpu().numpy()

    def rnd_check(self, sets, opt, tables, got, what=""):
        for b in range(self.B):
            for name, x, y in zip(("costs", "nominal | sigma"), (g[b] for g in got), self.rnd_single(sets[b], opt, b, tables[b])):
                np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"{what} {opt} controller {b} (phase {self.phases[b]}, table {tables[b]}): {name}")

    def tickets_at_zero(self):
        return (self.batch_scratch.cpu().numpy().view(np.uint32).reshape(self.B, -1)[:, :4] == 0).all()


def _sets(gpu, B, M, per_controller):
    """(the launch's set, the B sets of a controller's own M plants): D0..D3 cycling.  Shared: M plants for everybody; per controller: controller b plans on plants
    b, b + 1, ... so that no two controllers have the same list."""
    from judo_amd.device import GpuModelSet

    ms = _models(gpu)
    if not per_controller:
        s = GpuModelSet([ms[(m + 1) % 4] for m in range(M)])
        return s, [s] * B
    lists = [[ms[(b + m) % 4] for m in range(M)] for b in range(B)]
    return GpuModelSet([m for plants in lists for m in plants]), [GpuModelSet(plants) for plants in lists]


# ------------------------------------------------------------------------------------------------ 1. three controllers, three phases, a risk level each
@pytest.mark.parametrize("per_controller", [False, True])
@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
def test_three_controllers_in_three_phases(gpu, opt, per_controller):
    """B = 3, M = 2, N = 12, H = 8, K = 4, phases (0, 2, 3) from their phase states, worst (1, 2, 1); the shared set of 2 and the set of B * M = 6.  With the set of 6 the
    same controllers on controller 0's plants give other bytes: the controller's image stride is read."""
    xs = _phase_states()
    bl = Blocks(gpu, 3, 12, 8, 4, seed=101, x0s=[xs[0], xs[2], xs[3]], phases=(0, 2, 3))
    worst = [1, 2, 1]
    launch, own = _sets(gpu, 3, 2, per_controller)
    assert launch.info()["B"] == (6 if per_controller else 2)
    got = bl.ens_batch(launch, 2, worst, opt)
    bl.ens_check(own, opt, worst, got, what="set of 6" if per_controller else "shared set")
    assert bl.tickets_at_zero()
    if per_controller:
        on_first = bl.ens_batch(own[0], 2, worst, opt)
        assert on_first[0][0].tobytes() == got[0][0].tobytes()
        assert all((on_first[0][b] != got[0][b]).any() for b in (1, 2))


def test_controllers_that_differ_in_the_phase_word_only(gpu):
    """B = 4, one x0 (the cube above the goal, where the PLACE term is live), nominal, sigma, task parameters and noise, the phase word 0..3: four different cost rows, each
    the single entry's."""
    bl = Blocks(gpu, 4, 12, 8, 4, seed=102, x0s=[_phase_states()[2]] * 4, phases=range(4), shared=True)
    launch, own = _sets(gpu, 4, 2, False)
    got = bl.ens_batch(launch, 2, [1] * 4)
    assert len({got[1][b].tobytes() for b in range(4)}) == 4
    bl.ens_check(own, "mppi", [1] * 4, got, what="phase alone")


# ------------------------------------------------------------------------------------------------ 2. larger launch shapes
@pytest.mark.parametrize("N", [257, 513])
def test_launch_shapes_outside_the_full_latency_mode(gpu, N):
    """B = 2, M = 2, H = 4, K = 2.  N = 257: 1 028 rollouts, two rows of a wave per rollout; N = 513: 2 052 rollouts, every row its own rollout -- while a single ensemble
    call of 2 N rollouts runs in another mode.  The set of B * M = 4."""
    xs = _phase_states()
    bl = Blocks(gpu, 2, N, 4, 2, seed=103 + N, x0s=[xs[1], xs[3]], phases=(1, 3))
    launch, own = _sets(gpu, 2, 2, True)
    bl.ens_check(own, "cem", [1, 2], bl.ens_batch(launch, 2, [1, 2], "cem"), what=f"B*M*N={4 * N}")


# ------------------------------------------------------------------------------------------------ 3. overflow rows
def test_overflow_rows_of_the_last_pair(gpu):
    """B = 2, M = 2, N = 6, H = 4 from states with more than 32 general contacts: pair (c, m)'s overflow rows lie (c * M + m) * N behind the first pair's.  Nothing is dropped
    and the fallback is not taken."""
    xs, gen = _pressed_states()
    assert all(32 < n <= 96 for n in gen), gen
    bl = Blocks(gpu, 2, 6, 4, 4, seed=106, x0s=xs, phases=(0, 1), plain=True)
    launch, own = _sets(gpu, 2, 2, True)
    m0 = launch.models[0]
    m0.stats(reset=True)
    got = bl.ens_batch(launch, 2, [1, 1])
    st = m0.stats(reset=True)
    assert st["overflow_pool_fallbacks"] == 0 and st["contact_overflow"] == 0, st
    assert (got[0][1][1] != got[0][1][0]).any()  # (the plant matters in the last controller's state)
    bl.ens_check(own, "mppi", [1, 1], got, what="overflow rows")


# ------------------------------------------------------------------------------------------------ 4. B = 1, a second batch, the two completion marks
@pytest.mark.parametrize("use_mark", [True, False])
def test_batch_of_one_and_a_second_batch_on_the_same_scratch(gpu, use_mark):
    xs = _phase_states()
    one = Blocks(gpu, 1, 12, 8, 4, seed=107, x0s=xs[2:3], phases=(2,))
    launch, own = _sets(gpu, 1, 4, False)
    one.ens_check(own, "cem", [2], one.ens_batch(launch, 4, [2], "cem", use_mark=use_mark), what="B=1")
    bl = Blocks(gpu, 3, 12, 8, 4, seed=108, x0s=xs[1:], phases=(1, 2, 3))
    launch, own = _sets(gpu, 3, 2, False)
    old = 0xDEADBEEF
    bl.mark.numpy().view(np.uint32)[0] = old
    first = bl.ens_batch(launch, 2, [2, 1, 2], "cem", use_mark=use_mark)
    second = bl.ens_batch(launch, 2, [2, 1, 2], "cem", use_mark=use_mark)
    assert int(bl.mark.numpy().view(np.uint32)[0]) == ((old + 2) & 0xFFFFFFFF if use_mark else old)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, second)) and bl.tickets_at_zero()
    bl.ens_check(own, "cem", [2, 1, 2], first, what="B=3")


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(gpu):
    import torch

    from judo_amd.device import GpuModel, GpuModelSet

    xs = _phase_states()
    bl = Blocks(gpu, 3, 12, 8, 4, seed=109, x0s=xs[:3], phases=(0, 1, 2))
    launch, own = _sets(gpu, 3, 2, False)
    bufs = bl.outputs(2)
    word = bl.host.numpy()[:, bl.o_phase]
    for bad in (1.5, 4.0, float("nan")):
        word[2] = bad
        assert bl.ens_raw(launch, 2, [1, 1, 1], bufs) == -1 and "controller 2" in _err() and "phase word" in _err()
    word[2] = 2.0
    assert bl.ens_raw(launch, 2, [1, 1, 1], bufs, o_phase=bl.nblk) == -1 and "o_phase" in _err()
    assert bl.ens_raw(launch, 2, [1, 1, 1], bufs, o_phase=-1) == -1 and "o_phase" in _err()
    five = GpuModelSet([_models(gpu)[m % 4] for m in range(5)])
    assert bl.ens_raw(five, 2, [1, 1, 1], bufs) == -1 and "set of 5" in _err()
    assert bl.ens_raw(launch, 2, [1, 3, 1], bufs) == -1 and "controller 1" in _err() and "worst" in _err()
    leap = GpuModel("leap_cube", gpu)
    assert bl.ens_raw(GpuModelSet([leap, leap]), 2, [1, 1, 1], bufs) == -3 and "jh_plan_step_ensemble_batch plans" in _err()
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == v).all() for t, v in zip(bufs, (-7.0, -7.0, 0.0)))  # nothing ran
    bl.ens_check(own, "mppi", [1, 2, 1], bl.ens_batch(launch, 2, [1, 2, 1]), what="after the refusals")
