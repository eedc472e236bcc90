"""jh_plan_step_ensemble_phase through the C ABI: ONE fr3_pick plan step in one phase whose N candidates are rolled out on every plant of an fr3 model set (D0..D3 of
tests/test_fr3_plants_host.py) in one launch of the fr3 kernel on the grid (workgroups, M), aggregated with `worst` and updated in the tail.

Everything is compared bit for bit (`view(np.uint32)`), no tolerance anywhere, against what the tree already had:
  member_costs   row m is the costs of jh_plan_step(plant m's own handle, ..., phase, ...) with the same block, noise and N;
  costs          judo_amd.ensemble.aggregate_costs_host of those rows;
  out            nominal | sigma of jh_update_fused on those costs with the same block, noise and scratch size."""

import numpy as np
import pytest

from tests.test_gpu_plan_batch_fr3 import OPTS, _err, _phase_states, _pressed_states
from tests.test_gpu_plan_batch_fr3_models import _models
from tests.test_gpu_plan_randomized_fr3 import OneBlock

pytestmark = pytest.mark.gpu


class EnsembleBlock(OneBlock):
    """`OneBlock` with the (M, N) member costs and the ensemble call on it."""

    def __init__(self, dev, models, N, H, K, seed, x0):
        import torch

        super().__init__(dev, models, N, H, K, seed, x0)
        self.M = len(self.models)
        self.mc = torch.full((self.M, N), -7.0, dtype=torch.float32, device=dev)

    def raw_ens(self, opt, phase, worst, handle=None, mc="own", use_mark=False):
        """The status of one jh_plan_step_ensemble_phase into the object's buffers."""
        mode, lam, k, tie = OPTS[opt]
        o = self.off
        return self.lib.jh_plan_step_ensemble_phase(handle or self.set.handle, self.blk.data_ptr(), self.host.data_ptr(), 4 * self.nblk, o[1], o[2], o[3], o[4], self.noise.data_ptr(), self.ldn,
                                                    self.W.data_ptr(), phase, self.N, self.H, self.K, self.mc.data_ptr() if mc == "own" else mc, self.costs.data_ptr(), worst, mode, lam, k, tie,
                                                    self.scratch.data_ptr(), self.out.data_ptr(), self.mark.data_ptr() if use_mark else self.out.data_ptr(), None, 0)

    def untouched(self):
        import torch

        torch.cuda.synchronize()
        return (self.costs.cpu().numpy() == -7.0).all() and (self.mc.cpu().numpy() == -7.0).all() and (self.out.cpu().numpy() == 0).all()

    def call_ens(self, opt, phase, worst, use_mark=False):
        """(member_costs (M, N), costs (N,), nominal | sigma (2 KU,)) as numpy; the buffers are filled with sentinels in front of the call."""
        import torch

        from judo_amd import _lib

        self.costs.fill_(-7.0)
        self.mc.fill_(-7.0)
        self.out.zero_()
        _lib.check(self.raw_ens(opt, phase, worst, use_mark=use_mark), "jh_plan_step_ensemble_phase")
        _lib.check(self.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        out = self.out.cpu().numpy()
        assert (out[2 * self.KU :] == 0).all(), "the call wrote behind nominal | sigma"
        return self.mc.cpu().numpy(), self.costs.cpu().numpy(), out[: 2 * self.KU].copy()

    def check_ens(self, opt, worst, got, singles, what=""):
        from judo_amd.ensemble import aggregate_costs_host

        mc, costs, out = got
        for m, want in enumerate(singles):
            np.testing.assert_array_equal(mc[m].view(np.uint32), want.view(np.uint32), err_msg=f"{what} {opt}: member_costs row {m}")
        agg = aggregate_costs_host(np.stack(singles), worst)
        np.testing.assert_array_equal(costs.view(np.uint32), agg.view(np.uint32), err_msg=f"{what} {opt} worst={worst}: costs")
        ref = self.update_fused(opt, agg)
        np.testing.assert_array_equal(out.view(np.uint32), ref.view(np.uint32), err_msg=f"{what} {opt} worst={worst}: nominal | sigma")
        assert (self.scratch.cpu().numpy().view(np.uint32)[:4] == 0).all()  # the ticket is back at zero


# ------------------------------------------------------------------------------------------------ 1. four plants, every phase, every optimizer, three risk levels
@pytest.mark.parametrize("phase", [0, 1, 2, 3])
@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
def test_member_costs_aggregate_and_update_in_every_phase(gpu, opt, phase):
    """M = 4, N = 12 (three groups of four rows), H = 8, K = 4, from the phase's own state; `worst` = 1 (the maximum), 2 (a tail mean) and 4 (the mean)."""
    eb = EnsembleBlock(gpu, _models(gpu), 12, 8, 4, seed=80 + phase, x0=_phase_states()[phase])
    singles = [eb.single(opt, p, phase)[0] for p in range(4)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert (singles[i] != singles[j]).any(), (i, j)  # the plants matter
    for worst in (1, 2, 4):
        got = eb.call_ens(opt, phase, worst)
        eb.check_ens(opt, worst, got, singles, what=f"phase {phase}")
        before = int(eb.mark.numpy().view(np.uint32)[0])
        again = eb.call_ens(opt, phase, worst, use_mark=True)  # the polled completion word, on the same scratch
        assert int(eb.mark.numpy().view(np.uint32)[0]) == before + 1 and all(x.tobytes() == y.tobytes() for x, y in zip(got, again))


def test_the_phase_matters(gpu):
    """One block (the cube above the goal, where the PLACE term is live), one set, the four phases: four different cost vectors."""
    eb = EnsembleBlock(gpu, _models(gpu), 12, 8, 4, seed=84, x0=_phase_states()[2])
    assert len({eb.call_ens("mppi", ph, 1)[1].tobytes() for ph in range(4)}) == 4


# ------------------------------------------------------------------------------------------------ 2. larger launch shapes
@pytest.mark.parametrize("M,N", [(2, 515), (4, 513)])
def test_launch_shapes_outside_the_full_latency_mode(gpu, M, N):
    """H = 4, K = 2.  M = 2, N = 515: 1 030 rollouts, two rows of a wave per rollout; M = 4, N = 513: 2 052 rollouts, every row its own rollout -- while a single call of N
    runs four rows per rollout.  N is no multiple of the rows of a wave in either mode."""
    eb = EnsembleBlock(gpu, _models(gpu)[4 - M :], N, 4, 2, seed=90 + M, x0=_phase_states()[1])
    singles = [eb.single("cem", p, 1)[0] for p in range(M)]
    eb.check_ens("cem", 1, eb.call_ens("cem", 1, 1), singles, what=f"M*N={M * N}")


# ------------------------------------------------------------------------------------------------ 3. overflow rows
def test_overflow_rows_of_the_later_members(gpu):
    """M = 3 (D0, D2, D3), N = 6, H = 4 from a state with more than 32 general contacts: the contacts above the LDS pool live in a row of global memory per rollout, and
    member m's rows lie m * N behind member 0's.  Nothing is dropped and the fallback is not taken."""
    xs, gen = _pressed_states()
    assert all(32 < n <= 96 for n in gen), gen
    ms = _models(gpu)
    eb = EnsembleBlock(gpu, [ms[0], ms[2], ms[3]], 6, 4, 4, seed=95, x0=xs[1])
    singles = [eb.single("mppi", p, 0)[0] for p in range(3)]
    assert (singles[1] != singles[0]).any() and (singles[2] != singles[0]).any()  # (the plant matters in this state)
    ms[0].stats(reset=True)
    got = eb.call_ens("mppi", 0, 1)
    st = ms[0].stats(reset=True)
    assert st["overflow_pool_fallbacks"] == 0 and st["contact_overflow"] == 0, st
    eb.check_ens("mppi", 1, got, singles, what="overflow rows")


# ------------------------------------------------------------------------------------------------ 4. the self-collision build
def test_self_collision_build(gpu):
    ms = _models(gpu, True)
    assert all(m.fr3_build()["self_collision_build"] for m in ms)
    eb = EnsembleBlock(gpu, ms[1:3], 12, 8, 4, seed=97, x0=_phase_states()[0])
    singles = [eb.single("mppi", p, 0)[0] for p in range(2)]
    eb.check_ens("mppi", 2, eb.call_ens("mppi", 0, 2), singles, what="self-collision build")


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(gpu):
    from judo_amd.device import GpuModel, GpuModelSet

    eb = EnsembleBlock(gpu, _models(gpu), 12, 8, 4, seed=99, x0=_phase_states()[0])
    eb.costs.fill_(-7.0)
    eb.out.zero_()
    for bad in (4, -1):
        assert eb.raw_ens("mppi", bad, 1) == -1 and "phase" in _err()
    leap = GpuModel("leap_cube", gpu)
    leaps = GpuModelSet([leap, leap])
    assert eb.raw_ens("mppi", 0, 1, handle=leaps.handle) == -3 and "jh_plan_step_ensemble plans" in _err()
    for bad in (0, 5):
        assert eb.raw_ens("mppi", 0, bad) == -1 and "worst" in _err()
    assert eb.raw_ens("mppi", 0, 1, mc=None) == -1 and "member_costs" in _err()
    assert eb.untouched()  # nothing ran
    singles = [eb.single("mppi", p, 0)[0] for p in range(4)]
    eb.check_ens("mppi", 1, eb.call_ens("mppi", 0, 1), singles, what="after the refusals")
