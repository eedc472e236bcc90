"""jh_plan_step_randomized through the C ABI: ONE plan step whose N candidates form G contiguous blocks of Nb = N / G rollouts, block g rolled out on plant
plant_of_block[g] of a model set, and updated on the N costs as they are.

Everything is compared bit for bit (`view(np.uint32)`), no tolerance anywhere, against what the tree already had:
  costs   block g of the costs of jh_plan_step on plant plant_of_block[g]'s own handle (SetProblems.single: same block, same noise, same N), stitched by block;
  out     nominal | sigma of jh_update_fused on those stitched costs with the same block, noise and scratch size.
SetProblems (tests/test_gpu_model_set.py) builds M problems that share one block and one noise slice and differ in the model alone; the randomised call takes problem
0's block and noise pointers.  The members' single-call costs differ in every rollout (tests/test_gpu_plan_ensemble.py::test_the_members_and_the_risk_measure_matter
on the same cases), so a block that ran on another plant than its table names cannot pass the stitch."""

import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_plan_batch import OPTS, _err
from tests.test_gpu_plan_ensemble import _members, _problems  # (SetProblems, _models and _settled of tests/test_gpu_model_set.py behind them: one set of handles for both modules)

pytestmark = pytest.mark.gpu

PAD_OUT = 5  # floats behind nominal | sigma that the call must leave alone


def _table(a):
    return (C.c_ubyte * len(a))(*a)


class Randomized:
    """jh_plan_step_randomized on a SetProblems' set, block 0 and noise slice 0, with scratch, cost and output buffers of its own that live across calls."""

    def __init__(self, pr):
        import torch

        self.pr = pr
        self.scratch = torch.zeros(pr.per_scratch, dtype=torch.float32, device=pr.dev)
        self.mark = torch.zeros(4, dtype=torch.int32).pin_memory()
        self.costs = torch.full((pr.N,), -7.0, dtype=torch.float32, device=pr.dev)
        self.out = torch.zeros(2 * pr.KU + PAD_OUT, dtype=torch.float32, device=pr.dev)

    def args(self, opt, table, G, costs, out, mark):
        pr = self.pr
        mode, lam, k, tie = OPTS[opt]
        p = pr.blocks.data_ptr()
        return [pr.set.handle, p, p, 4 * pr.nblk, pr.off[1], pr.off[2], pr.off[3], pr.off[4], pr.noise.data_ptr(), pr.ldn, pr.W.data_ptr(), pr.N, pr.H, pr.K, table, G, costs,
                mode, lam, k, tie, self.scratch.data_ptr(), out, mark, None, 0]

    def call(self, opt, a, use_mark=False):
        """Returns (costs (N,), nominal | sigma (2 KU,)) as numpy; the device buffers are the object's, filled with sentinels in front of the call."""
        import torch

        from judo_amd import _lib

        pr = self.pr
        self.costs.fill_(-7.0)
        self.out.zero_()
        args = self.args(opt, _table(a), len(a), self.costs.data_ptr(), self.out.data_ptr(), self.mark.data_ptr() if use_mark else self.out.data_ptr())
        _lib.check(pr.lib.jh_plan_step_randomized(*args), "jh_plan_step_randomized")
        _lib.check(pr.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        o = self.out.cpu().numpy()
        assert (o[2 * pr.KU :] == 0).all(), "the call wrote behind nominal | sigma"
        return self.costs.cpu().numpy(), o[: 2 * pr.KU].copy()

    def update_fused(self, opt, costs):
        """nominal | sigma of jh_update_fused on `costs` (numpy, (N,)) with the block and noise of the randomised call and a fresh scratch block of the same size."""
        import torch

        from judo_amd import _lib

        pr = self.pr
        mode, lam, k, tie = OPTS[opt]
        d_c = torch.from_numpy(np.ascontiguousarray(costs, dtype=np.float32)).to(pr.dev)
        out = torch.zeros(2 * pr.KU, dtype=torch.float32, device=pr.dev)
        scratch = torch.zeros(pr.per_scratch, dtype=torch.float32, device=pr.dev)
        p = pr.blocks.data_ptr()
        st = pr.lib.jh_update_fused(d_c.data_ptr(), None, p + 4 * pr.off[1], pr.noise.data_ptr(), pr.ldn, p + 4 * pr.off[2], p + 4 * pr.off[4], pr.N, 0, pr.K, pr.nu, mode, lam, k, tie, 0, None,
                                    0, 0, scratch.data_ptr(), out.data_ptr(), out.data_ptr() + 4 * pr.KU, None, 0)
        _lib.check(st, "jh_update_fused")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def tickets(self):
        return self.scratch.cpu().numpy().view(np.uint32)[:4]

    def check(self, opt, a, got, singles, what=""):
        """The two comparisons of the module's docstring; `singles`: [SetProblems.single(opt, b)[0] for every member].  Returns the stitched costs."""
        costs, out = got
        want = stitch(singles, a)
        np.testing.assert_array_equal(costs.view(np.uint32), want.view(np.uint32), err_msg=f"{what} {opt} {a}: costs")
        ref = self.update_fused(opt, want)
        np.testing.assert_array_equal(out.view(np.uint32), ref.view(np.uint32), err_msg=f"{what} {opt} {a}: nominal | sigma")
        return want


def stitch(singles, a):
    """Block g of plant a[g]'s single-call costs, for every g."""
    N = len(singles[0])
    assert N % len(a) == 0
    Nb = N // len(a)
    return np.concatenate([singles[p][g * Nb : (g + 1) * Nb] for g, p in enumerate(a)])


def nominal_rule(costs, singles, a):
    """Global rollout 0 is the noise-free nominal on plant a[0]; the first rollout of block 1 carries its noise (rollout 0 of a single call is that plant's noise-free
    cost).  Implied by the stitch, asserted on its own: a launch that let every block drop its first rollout's noise fails the second line."""
    Nb = len(costs) // len(a)
    assert costs[:1].tobytes() == singles[a[0]][:1].tobytes()
    if len(a) > 1:
        assert costs[Nb : Nb + 1].tobytes() != singles[a[1]][:1].tobytes()
        assert costs[Nb : Nb + 1].tobytes() == singles[a[1]][Nb : Nb + 1].tobytes()


# ------------------------------------------------------------------------------------------------ 1. closed-form models
@pytest.mark.parametrize("task,opt", [("cartpole", "mppi"), ("cartpole", "cem"), ("cartpole", "ps"), ("cylinder_push", "mppi")])
def test_closed_form_randomized(gpu, task, opt):
    """M = 3, N = 300, H = 8, K = 4: G = 3 with [2, 0, 1] (Nb = 100: ragged waves, block 0 not on plant 0), G = 6 with [1, 1, 0, 2, 2, 2] (Nb = 50: G > M, repeats)
    and G = 1 with [2]; with the stream's event and with the polled word.  A second call on the same scratch gives the same bytes and leaves the ticket words at zero;
    the completion word counts the calls."""
    pr = _problems(gpu, task, list(_members(gpu, task)), 300, 4, 8, seed=3)
    rn = Randomized(pr)
    singles = [pr.single(opt, b)[0] for b in range(pr.B)]
    rn.mark.numpy().view(np.uint32)[0] = 0xFFFFFFFF
    marks = 0
    for a in ([2, 0, 1], [1, 1, 0, 2, 2, 2], [2]):
        by_event = rn.call(opt, a)
        rn.check(opt, a, by_event, singles, what=task)
        nominal_rule(by_event[0], singles, a)
        assert (rn.tickets() == 0).all()
        by_word = rn.call(opt, a, use_mark=True)
        marks += 1
        assert int(rn.mark.numpy().view(np.uint32)[0]) == marks - 1  # (0xFFFFFFFF + 1 wraps to 0)
        for x, y in zip(by_event, by_word):
            assert x.tobytes() == y.tobytes()
        assert (rn.tickets() == 0).all()
    c1, o1 = pr.single(opt, 2)  # G = 1: a plain plan step on that plant
    assert by_word[0].tobytes() == c1.tobytes() and by_word[1].tobytes() == o1[: 2 * pr.KU].tobytes()


# ------------------------------------------------------------------------------------------------ 2. the leap family
@pytest.mark.parametrize("opt", ["mppi", "cem"])
@pytest.mark.parametrize("N,H,a", [(24, 8, [3, 0, 2, 0]), (1408, 4, [3, 0, 2, 1])])
def test_leap_randomized(gpu, opt, N, H, a):
    """leap_cube from the settled state, M = 4 (shipped, A, B, C), K = 4, G = 4: N = 24 (Nb = 6: one full group of four rollouts and a ragged one per block, the block
    starts off any wave boundary, the launch of 24 rollouts in the latency mode -- as the single calls of 24 are) and N = 1 408 (Nb = 352: outside the latency mode)."""
    pr = _problems(gpu, "leap_cube", list(_members(gpu, "leap_cube")), N, 4, H, seed=22)
    rn = Randomized(pr)
    singles = [pr.single(opt, b)[0] for b in range(pr.B)]
    got = rn.call(opt, a)
    rn.check(opt, a, got, singles, what=f"leap_cube N={N}")
    nominal_rule(got[0], singles, a)
    assert (rn.tickets() == 0).all()
    again = rn.call(opt, a)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes() and (rn.tickets() == 0).all()


@pytest.mark.parametrize("task,build", [("leap_cube_down", dict(contact_capacity=64, cylinder_build=False)), ("caltech_cylinder", dict(contact_capacity=64, cylinder_build=True))])
def test_leap_randomized_on_the_other_builds(gpu, task, build):
    """The 64-contact build (leap_cube_down) and the cylinder build (caltech_leap_cube with its fingertip cylinders): M = 2 (shipped, A), N = 24, G = 4 with [1, 0, 0, 1],
    H = 4, MPPI."""
    models = list(_members(gpu, task))
    got = models[0].build()
    assert {k: got[k] for k in build} == build
    pr = _problems(gpu, task, models, 24, 4, 4, seed=42)
    rn = Randomized(pr)
    singles = [pr.single("mppi", b)[0] for b in range(pr.B)]
    models[0].stats(reset=True)
    a = [1, 0, 0, 1]
    res = rn.call("mppi", a)
    rn.check("mppi", a, res, singles, what=task)
    nominal_rule(res[0], singles, a)
    assert models[0].stats(reset=True)["overflow_pool_fallbacks"] == 0


# ------------------------------------------------------------------------------------------------ 3. the assignment travels with the call
@pytest.mark.parametrize("task,N,H", [("cartpole", 300, 8), ("leap_cube", 24, 8)])
def test_assignment_changed_between_calls(gpu, task, N, H):
    """Two calls on the same buffers with two tables: the second result follows the second table (and differs from the first: the members are different plants)."""
    pr = _problems(gpu, task, list(_members(gpu, task)), N, 4, H, seed=7)
    rn = Randomized(pr)
    singles = [pr.single("mppi", b)[0] for b in range(pr.B)]
    first, second = [2, 0, 1], [0, 1, 2]
    got1 = rn.call("mppi", first)
    got2 = rn.call("mppi", second)
    rn.check("mppi", first, got1, singles, what=task)
    rn.check("mppi", second, got2, singles, what=task)
    assert (got1[0] != got2[0]).any() and (got1[1] != got2[1]).any()
    assert (rn.tickets() == 0).all()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_randomized_refusals(gpu):
    import torch

    from judo_amd.device import GpuModel, GpuModelSet

    models = list(_members(gpu, "cartpole"))
    pr = _problems(gpu, "cartpole", models, 8, 4, 8, seed=11)
    rn = Randomized(pr)
    L = pr.lib
    costs = torch.full((8,), -7.0, dtype=torch.float32, device=gpu)
    out = torch.full((2 * pr.KU,), -7.0, dtype=torch.float32, device=gpu)
    base = rn.args("mppi", _table([2, 0]), 2, costs.data_ptr(), out.data_ptr(), out.data_ptr())
    names = ["set", "blk_dev", "blk_host", "blk_bytes", "o_nominal", "o_sigma", "o_tp", "o_lohi", "noise", "ldn", "W", "N", "H", "K", "plant_of_block", "G", "costs", "mode", "lambda", "k",
             "tie_high", "scratch", "out", "out_host_mark", "timing", "stream"]
    assert len(names) == len(base)

    def call(**kw):
        a = list(base)
        for key, v in kw.items():
            a[names.index(key)] = v
        return L.jh_plan_step_randomized(*a)

    for ptr in ("set", "blk_dev", "blk_host", "noise", "W", "plant_of_block", "costs", "scratch", "out"):
        assert call(**{ptr: None}) == -1 and f"{ptr} is a null pointer" in _err(), ptr
    assert call(G=0) == -1 and "G = 0" in _err() and "JH_MAX_PLANT_BLOCKS = 64" in _err()
    assert call(G=65, plant_of_block=_table([0] * 65)) == -1 and "G = 65" in _err()
    assert call(G=3, plant_of_block=_table([0, 1, 2])) == -1 and "N = 8 is no multiple of G = 3" in _err()
    assert call(plant_of_block=_table([0, 3])) == -1 and "plant_of_block[1] = 3" in _err() and "M = 3" in _err() and "block 1" in _err()
    assert call(plant_of_block=_table([255, 0])) == -1 and "plant_of_block[0] = 255" in _err()
    assert call(N=0) == -1 and "N, H, K must be positive" in _err()
    assert call(ldn=7) == -1 and "ldn (7) < N (8)" in _err()
    assert call(K=513) == -1 and "K*nu = 513 exceeds 512" in _err()
    assert call(o_sigma=-1) == -1 and "negative block offset" in _err()
    assert call(blk_bytes=4 * pr.nblk - 4) == -1 and "does not hold" in _err()
    assert call(mode=2) == -1 and "mode must be" in _err()
    assert call(mode=0, **{"lambda": 0.0}) == -1 and "temperature" in _err()
    assert call(mode=1, k=0) == -1 and "k = 0" in _err()
    big = GpuModelSet([models[0]] * 33)
    assert call(set=big.handle) == -1 and "33 members" in _err() and "JH_MAX_ENSEMBLE" in _err()
    big.close()
    forced = GpuModel("cartpole", gpu)
    forced.set_plan_step_launches(1)
    one = GpuModelSet([forced])
    assert call(set=one.handle, plant_of_block=_table([0, 0])) == -1 and "one launch is forced" in _err()
    one.close()
    leap = GpuModel("leap_cube", gpu)  # JH_ERR_UNSUPPORTED, as the ensemble call: a set is made of generation 3 alone; a later change of member 0's generation is caught by the call
    held = GpuModelSet([leap])
    leap.set_kernel(2)
    assert call(set=held.handle, plant_of_block=_table([0, 0])) == -3 and "only kernel generation 3" in _err()
    held.close()
    torch.cuda.synchronize()
    assert (costs.cpu().numpy() == -7.0).all() and (out.cpu().numpy() == -7.0).all()  # nothing ran
    assert call() == 0 and L.jh_download_end() == 0
    torch.cuda.synchronize()
    assert (costs.cpu().numpy() != -7.0).all() and (out.cpu().numpy()[: pr.KU] != -7.0).all()  # (MPPI writes the nominal alone)
