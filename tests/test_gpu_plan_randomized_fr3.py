"""jh_plan_step_randomized_phase through the C ABI: ONE fr3_pick plan step in one phase whose N candidates form G contiguous blocks of Nb = N / G rollouts, block g
rolled out on plant plant_of_block[g] of an fr3 model set (M = 4: D0..D3 of tests/test_fr3_plants_host.py), and updated on the N costs as they are.

Everything is compared bit for bit (`view(np.uint32)`), no tolerance anywhere, against what the tree already had:
  costs   block g of the costs of jh_plan_step(plant plant_of_block[g]'s own handle, ..., phase, ...) with the same block, noise and N, stitched by block;
  out     nominal | sigma of jh_update_fused on those stitched costs with the same block, noise and scratch size."""

import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_plan_batch_fr3 import OPTS, _err, _phase_states
from tests.test_gpu_plan_batch_fr3_models import _models
from tests.test_gpu_plan_randomized import nominal_rule, stitch

pytestmark = pytest.mark.gpu

PAD_OUT = 5  # floats behind nominal | sigma that the call must leave alone


class OneBlock:
    """One fr3_pick problem -- x0 | nominal | sigma | task parameters | bounds on the device, one noise slice of pitch N + 4 -- and the calls on it."""

    def __init__(self, dev, models, N, H, K, seed, x0):
        import torch

        from judo_amd import _lib
        from judo_amd.device import GpuModelSet
        from judo_amd.spline import spline_weights
        from judo_amd.tasks import FR3Pick

        self.lib, self.dev, self.models, self.N, self.H, self.K = _lib.lib(), dev, list(models), N, H, K
        self.set = GpuModelSet(self.models)
        assert self.set.fr3
        task = FR3Pick()
        nu, nx = task.nu, task.nq + task.nv
        self.nu, self.KU = nu, K * nu
        rng = np.random.default_rng(seed)
        tp = np.asarray(task.task_params({}), dtype=np.float32)
        tp = tp * (1.0 + 0.2 * rng.random(len(tp))).astype(np.float32)
        self.off = [int(v) for v in np.cumsum([0, nx, self.KU, self.KU, len(tp), 2 * nu])]
        self.nblk = self.off[-1]
        r = task.actuator_ctrlrange
        lohi = np.nan_to_num(np.concatenate([r[:, 0], r[:, 1]]).astype(np.float32), posinf=3.0e38, neginf=-3.0e38)
        warm = np.tile(np.asarray(task.optimizer_warm_start(), dtype=np.float64), (K, 1))
        nominal = (warm + 0.1 * rng.standard_normal((K, nu))).astype(np.float32).reshape(-1)
        sigma = (0.05 + 0.2 * rng.random((K, nu))).astype(np.float32).reshape(-1)
        self.host = torch.from_numpy(np.concatenate([np.asarray(x0, dtype=np.float32), nominal, sigma, tp, lohi])).pin_memory()
        self.blk = self.host.to(dev)
        self.ldn = N + 4
        self.noise = torch.from_numpy(rng.standard_normal((self.KU, self.ldn)).astype(np.float32)).to(dev)
        self.W = torch.from_numpy(spline_weights("linear", np.linspace(0, H * task.dt, K), task.dt * np.arange(H)).astype(np.float32)).to(dev)
        self.per_scratch = int(self.lib.jh_update_fused_scratch_floats(N, K, nu))
        self.scratch = torch.zeros(self.per_scratch, dtype=torch.float32, device=dev)
        self.mark = torch.zeros(4, dtype=torch.int32).pin_memory()
        self.costs = torch.full((N,), -7.0, dtype=torch.float32, device=dev)
        self.out = torch.zeros(2 * self.KU + PAD_OUT, dtype=torch.float32, device=dev)

    def raw(self, opt, a, phase, handle=None, N=None, table="from a", use_mark=False):
        """The status of one jh_plan_step_randomized_phase into the object's cost and output buffers."""
        mode, lam, k, tie = OPTS[opt]
        o = self.off
        t = (C.c_ubyte * len(a))(*a) if table == "from a" else table
        return self.lib.jh_plan_step_randomized_phase(handle or self.set.handle, self.blk.data_ptr(), self.host.data_ptr(), 4 * self.nblk, o[1], o[2], o[3], o[4], self.noise.data_ptr(), self.ldn,
                                                      self.W.data_ptr(), phase, self.N if N is None else N, self.H, self.K, t, len(a), self.costs.data_ptr(), mode, lam, k, tie,
                                                      self.scratch.data_ptr(), self.out.data_ptr(), self.mark.data_ptr() if use_mark else self.out.data_ptr(), None, 0)

    def call(self, opt, a, phase, use_mark=False):
        """(costs (N,), nominal | sigma (2 KU,)) as numpy; the buffers are filled with sentinels in front of the call."""
        import torch

        from judo_amd import _lib

        self.costs.fill_(-7.0)
        self.out.zero_()
        _lib.check(self.raw(opt, a, phase, use_mark=use_mark), "jh_plan_step_randomized_phase")
        _lib.check(self.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        out = self.out.cpu().numpy()
        assert (out[2 * self.KU :] == 0).all(), "the call wrote behind nominal | sigma"
        return self.costs.cpu().numpy(), out[: 2 * self.KU].copy()

    def single(self, opt, p, phase):
        """(costs, nominal | sigma) of jh_plan_step on plant p's own handle with the same block, noise and N, buffers of its own."""
        import torch

        from judo_amd import _lib

        mode, lam, k, tie = OPTS[opt]
        o = self.off
        costs = torch.full((self.N,), -7.0, dtype=torch.float32, device=self.dev)
        out = torch.zeros(2 * self.KU, dtype=torch.float32, device=self.dev)
        scratch = torch.zeros(self.per_scratch, dtype=torch.float32, device=self.dev)
        blk = torch.full((self.nblk,), float("nan"), dtype=torch.float32, device=self.dev)
        st = self.lib.jh_plan_step(self.models[p].handle, blk.data_ptr(), self.host.data_ptr(), 4 * self.nblk, o[1], o[2], o[3], o[4], self.noise.data_ptr(), self.ldn, self.W.data_ptr(), phase, self.N,
                                   0, self.H, self.K, costs.data_ptr(), None, None, mode, lam, k, tie, 0, 0, 0, scratch.data_ptr(), out.data_ptr(), out.data_ptr(), None, 0)
        _lib.check(st, "jh_plan_step")
        _lib.check(self.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        c = costs.cpu().numpy()
        assert np.isfinite(c).all()
        return c, out.cpu().numpy()

    def update_fused(self, opt, costs):
        """nominal | sigma of jh_update_fused on `costs` with the block and noise of the randomised call and a fresh scratch block of the same size."""
        import torch

        from judo_amd import _lib

        mode, lam, k, tie = OPTS[opt]
        o, p = self.off, self.blk.data_ptr()
        d_c = torch.from_numpy(np.ascontiguousarray(costs, dtype=np.float32)).to(self.dev)
        out = torch.zeros(2 * self.KU, dtype=torch.float32, device=self.dev)
        scratch = torch.zeros(self.per_scratch, dtype=torch.float32, device=self.dev)
        st = self.lib.jh_update_fused(d_c.data_ptr(), None, p + 4 * o[1], self.noise.data_ptr(), self.ldn, p + 4 * o[2], p + 4 * o[4], self.N, 0, self.K, self.nu, mode, lam, k, tie, 0, None, 0, 0,
                                      scratch.data_ptr(), out.data_ptr(), out.data_ptr() + 4 * self.KU, None, 0)
        _lib.check(st, "jh_update_fused")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def check(self, opt, a, got, singles, what=""):
        costs, out = got
        want = stitch(singles, a)
        np.testing.assert_array_equal(costs.view(np.uint32), want.view(np.uint32), err_msg=f"{what} {opt} {a}: costs")
        ref = self.update_fused(opt, want)
        np.testing.assert_array_equal(out.view(np.uint32), ref.view(np.uint32), err_msg=f"{what} {opt} {a}: nominal | sigma")
        assert (self.scratch.cpu().numpy().view(np.uint32)[:4] == 0).all()  # the ticket is back at zero


# ------------------------------------------------------------------------------------------------ 1. stitched costs, latency mode
@pytest.mark.parametrize("phase", [0, 1, 2, 3])
@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
def test_stitched_costs_in_every_phase(gpu, opt, phase):
    """N = 12, G = 4, table [2, 0, 1, 2]: Nb = 3 gives ragged waves, block 0 is not on plant 0 and plant 2 is named by non-adjacent blocks; from the phase's own state.
    Rollout 0 runs on plant 2 and is the only noise-free one: rollout Nb, the first of the block on plant 0, does not cost what plant 0's nominal costs."""
    a = [2, 0, 1, 2]
    ob = OneBlock(gpu, _models(gpu), 12, 8, 4, seed=40 + phase, x0=_phase_states()[phase])
    singles = [ob.single(opt, p, phase)[0] for p in range(4)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert (singles[i] != singles[j]).any(), (i, j)  # the plants matter
    got = ob.call(opt, a, phase)
    ob.check(opt, a, got, singles, what=f"phase {phase}")
    nominal_rule(got[0], singles, a)
    assert got[0][3:4].tobytes() != singles[0][:1].tobytes()
    again = ob.call(opt, a, phase, use_mark=True)  # the polled completion word, on the same scratch
    assert int(ob.mark.numpy().view(np.uint32)[0]) == 1 and all(x.tobytes() == y.tobytes() for x, y in zip(got, again))


def test_the_phase_matters(gpu):
    """One block (the cube above the goal, where the PLACE term is live), one table, the four phases: four different cost vectors."""
    ob = OneBlock(gpu, _models(gpu), 12, 8, 4, seed=44, x0=_phase_states()[2])
    assert len({ob.call("mppi", [2, 0, 1, 2], ph)[0].tobytes() for ph in range(4)}) == 4


# ------------------------------------------------------------------------------------------------ 2. larger launch shapes
@pytest.mark.parametrize("N,a", [(1030, [1, 3]), (2052, [3, 0, 2, 1])])
def test_launch_shapes_outside_the_full_latency_mode(gpu, N, a):
    """H = 4, K = 2.  N = 1 030, G = 2: two rows of a wave per rollout, Nb = 515 ragged; N = 2 052, G = 4: every row its own rollout, Nb = 513 ragged."""
    ob = OneBlock(gpu, _models(gpu), N, 4, 2, seed=50 + len(a), x0=_phase_states()[1])
    singles = [ob.single("cem", p, 1)[0] for p in range(4)]
    got = ob.call("cem", a, 1)
    ob.check("cem", a, got, singles, what=f"N={N}")
    nominal_rule(got[0], singles, a)


# ------------------------------------------------------------------------------------------------ 3. degenerate tables
def test_degenerate_tables(gpu):
    ob = OneBlock(gpu, _models(gpu), 12, 8, 4, seed=60, x0=_phase_states()[0])
    full = [ob.single("cem", p, 0) for p in range(4)]
    singles = [c for c, _ in full]
    for a in ([0], [0, 0, 0, 0]):  # a plain plan step on plant 0
        got = ob.call("cem", a, 0)
        assert got[0].tobytes() == full[0][0].tobytes() and got[1].tobytes() == full[0][1].tobytes(), a
    got = ob.call("cem", [3], 0)
    assert got[0].tobytes() == full[3][0].tobytes() and got[1].tobytes() == full[3][1].tobytes()
    for a in ([0, 1, 2, 3], [1, 0, 1, 3], [3, 3, 0, 3, 1, 3]):  # G = M with the identity; one plant named by non-adjacent blocks; G > M
        ob.check("cem", a, ob.call("cem", a, 0), singles, what="degenerate")


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals(gpu):
    import torch

    from judo_amd.device import GpuModel, GpuModelSet

    ob = OneBlock(gpu, _models(gpu), 12, 8, 4, seed=70, x0=_phase_states()[0])
    ob.costs.fill_(-7.0)
    ob.out.zero_()
    assert ob.raw("mppi", [0, 1, 2, 3, 0], 0) == -1 and "no multiple of G" in _err()  # N % G != 0
    assert ob.raw("mppi", [0, 1, 4, 3], 0) == -1 and "plant_of_block[2]" in _err() and "block 2" in _err()
    for bad in (4, -1):
        assert ob.raw("mppi", [0, 1], bad) == -1 and "phase" in _err()
    leap = GpuModel("leap_cube", gpu)
    leaps = GpuModelSet([leap, leap])
    assert ob.raw("mppi", [0, 1], 0, handle=leaps.handle) == -3 and "jh_plan_step_randomized" in _err()
    assert ob.raw("mppi", [0, 1], 0, table=None) == -1 and "plant_of_block" in _err()
    assert ob.raw("mppi", [0] * 65, 0, N=65) == -1 and "JH_MAX_PLANT_BLOCKS" in _err()
    torch.cuda.synchronize()
    assert (ob.costs.cpu().numpy() == -7.0).all() and (ob.out.cpu().numpy() == 0).all()  # nothing ran
    a = [2, 0, 1, 2]
    ob.check("mppi", a, ob.call("mppi", a, 0), [ob.single("mppi", p, 0)[0] for p in range(4)], what="after the refusals")
