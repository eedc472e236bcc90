"""jh_plan_step_ensemble through the C ABI: ONE plan step whose N candidates are rolled out on the M members of a model set and updated on the aggregated costs.

Everything is compared bit for bit (`view(np.uint32)`), no tolerance anywhere, against what the tree already had:
  member_costs[b]   the costs of jh_plan_step on member b's own handle (SetProblems.single: same block, same noise);
  costs             judo_amd.ensemble.aggregate_costs_host(member_costs, worst), the numpy restatement of the risk measure;
  out               nominal | sigma of jh_update_fused on those aggregated costs with the same block, noise and scratch size.
SetProblems (tests/test_gpu_model_set.py) builds M problems that share one block and one noise slice and differ in the model alone; the ensemble call takes problem 0's
block and noise pointers."""

import functools

import numpy as np
import pytest

from tests.test_gpu_model_set import CARTPOLE, CYLINDER, LEAP_A, LEAP_B, LEAP_C, SetProblems, _models, _settled
from tests.test_gpu_plan_batch import OPTS, _err

pytestmark = pytest.mark.gpu

PAD_OUT = 5  # floats behind nominal | sigma that the call must leave alone


@functools.lru_cache(maxsize=None)
def _members(gpu, task):
    """The shipped model of `task` and its perturbed members, made once for the module (no test changes a handle's settings)."""
    pert = {"cartpole": CARTPOLE, "cylinder_push": CYLINDER, "leap_cube": [LEAP_A, LEAP_B, LEAP_C]}.get(task, [LEAP_A])
    return tuple(_models(gpu, task, pert))


class Ensemble:
    """jh_plan_step_ensemble on a SetProblems' set, block 0 and noise slice 0, with a scratch block of its own that lives across calls."""

    def __init__(self, pr):
        import torch

        self.pr = pr
        self.scratch = torch.zeros(pr.per_scratch, dtype=torch.float32, device=pr.dev)
        self.mark = torch.zeros(4, dtype=torch.int32).pin_memory()

    def args(self, opt, worst, member, costs, out, mark):
        pr = self.pr
        mode, lam, k, tie = OPTS[opt]
        p = pr.blocks.data_ptr()
        return [pr.set.handle, p, p, 4 * pr.nblk, pr.off[1], pr.off[2], pr.off[3], pr.off[4], pr.noise.data_ptr(), pr.ldn, pr.W.data_ptr(), pr.N, pr.H, pr.K, member, costs, worst,
                mode, lam, k, tie, self.scratch.data_ptr(), out, mark, None, 0]

    def call(self, opt, worst, use_mark=False):
        """Returns (member_costs (M, N), costs (N,), nominal | sigma (2 KU,)) as numpy."""
        import torch

        from judo_amd import _lib

        pr = self.pr
        member = torch.full((pr.B, pr.N), -7.0, dtype=torch.float32, device=pr.dev)
        costs = torch.full((pr.N,), -7.0, dtype=torch.float32, device=pr.dev)
        out = torch.zeros(2 * pr.KU + PAD_OUT, dtype=torch.float32, device=pr.dev)
        a = self.args(opt, worst, member.data_ptr(), costs.data_ptr(), out.data_ptr(), self.mark.data_ptr() if use_mark else out.data_ptr())
        _lib.check(pr.lib.jh_plan_step_ensemble(*a), "jh_plan_step_ensemble")
        _lib.check(pr.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[2 * pr.KU :] == 0).all(), "the call wrote behind nominal | sigma"
        return member.cpu().numpy(), costs.cpu().numpy(), o[: 2 * pr.KU].copy()

    def update_fused(self, opt, costs):
        """nominal | sigma of jh_update_fused on `costs` (numpy, (N,)) with the block and noise of the ensemble call and a fresh scratch block of the same size."""
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

    def check(self, opt, worst, got, singles, what=""):
        """The three comparisons of the module's docstring; `singles`: [SetProblems.single(opt, b)[0] for every member]."""
        from judo_amd.ensemble import aggregate_costs_host

        member, costs, out = got
        for b, c1 in enumerate(singles):
            np.testing.assert_array_equal(member[b].view(np.uint32), c1.view(np.uint32), err_msg=f"{what} {opt} worst={worst}: member {b}'s costs")
        want = aggregate_costs_host(member, worst)
        np.testing.assert_array_equal(costs.view(np.uint32), want.view(np.uint32), err_msg=f"{what} {opt} worst={worst}: aggregated costs")
        ref = self.update_fused(opt, want)
        np.testing.assert_array_equal(out.view(np.uint32), ref.view(np.uint32), err_msg=f"{what} {opt} worst={worst}: nominal | sigma")


def _problems(gpu, task, models, N, K, H, seed):
    if task == "cartpole":
        return SetProblems(gpu, task, models, N, K, H, 0, seed=seed, x0=[0.1, 0.3, 0.0, 0.0])
    if task == "cylinder_push":
        return SetProblems(gpu, task, models, N, K, H, 0, seed=seed, x0=[0.0, 0.0, -0.5, 0.0, 0.0, 0.0, 0.0, 0.0], sigma=3.0)
    steps = 5 if task == "leap_cube_down" else 60
    return SetProblems(gpu, task, models, N, K, H, 0, seed=seed, x0=_settled(task, steps))


# ------------------------------------------------------------------------------------------------ 1. closed-form models
@pytest.mark.parametrize("task,opt", [("cartpole", "mppi"), ("cartpole", "cem"), ("cartpole", "ps"), ("cylinder_push", "mppi")])
def test_closed_form_ensemble(gpu, task, opt):
    """M = 3, N = 300 (two tail workgroups, the second ragged), H = 8, K = 4, worst = 1, 2, 3, with the stream's event and with the polled word.  A second call on the
    same scratch gives the same bytes and leaves the ticket words at zero; the completion word counts the calls."""
    pr = _problems(gpu, task, list(_members(gpu, task)), 300, 4, 8, seed=3)
    en = Ensemble(pr)
    singles = [pr.single(opt, b)[0] for b in range(pr.B)]
    en.mark.numpy().view(np.uint32)[0] = 0xFFFFFFFF
    marks = 0
    for worst in (1, 2, 3):
        by_event = en.call(opt, worst)
        en.check(opt, worst, by_event, singles, what=task)
        assert (en.tickets() == 0).all()
        by_word = en.call(opt, worst, use_mark=True)
        marks += 1
        assert int(en.mark.numpy().view(np.uint32)[0]) == marks - 1  # (0xFFFFFFFF + 1 wraps to 0)
        for x, y in zip(by_event, by_word):
            assert x.tobytes() == y.tobytes()
        assert (en.tickets() == 0).all()


# ------------------------------------------------------------------------------------------------ 2. the leap family
@pytest.mark.parametrize("opt", ["mppi", "cem"])
@pytest.mark.parametrize("N,H", [(6, 8), (352, 4)])
def test_leap_ensemble(gpu, opt, N, H):
    """leap_cube from the settled state, M = 4 (shipped, A, B, C), K = 4: N = 6 (one full group of four rollouts, one ragged; the launch of 24 rollouts runs the latency
    mode) and N = 352 (1 408 rollouts in the launch: outside it, while each single call of 352 still runs it)."""
    pr = _problems(gpu, "leap_cube", list(_members(gpu, "leap_cube")), N, 4, H, seed=22)
    en = Ensemble(pr)
    singles = [pr.single(opt, b)[0] for b in range(pr.B)]
    for worst in (1, 2, 4):
        en.check(opt, worst, en.call(opt, worst), singles, what=f"leap_cube N={N}")
    assert (en.tickets() == 0).all()


@pytest.mark.parametrize("opt", ["mppi", "cem"])
@pytest.mark.parametrize("task,build", [("leap_cube_down", dict(contact_capacity=64, cylinder_build=False)), ("caltech_cylinder", dict(contact_capacity=64, cylinder_build=True))])
def test_leap_ensemble_on_the_other_builds(gpu, task, build, opt):
    """The 64-contact build (leap_cube_down) and the cylinder build (caltech_leap_cube with its fingertip cylinders): M = 2 (shipped, A), N = 4, H = 4."""
    models = list(_members(gpu, task))
    got = models[0].build()
    assert {k: got[k] for k in build} == build
    pr = _problems(gpu, task, models, 4, 4, 4, seed=42)
    en = Ensemble(pr)
    singles = [pr.single(opt, b)[0] for b in range(pr.B)]
    models[0].stats(reset=True)
    for worst in (1, 2):
        en.check(opt, worst, en.call(opt, worst), singles, what=task)
    assert models[0].stats(reset=True)["overflow_pool_fallbacks"] == 0


# ------------------------------------------------------------------------------------------------ 3. teeth
@pytest.mark.parametrize("task,N,H", [("cartpole", 300, 8), ("leap_cube", 6, 8)])
def test_the_members_and_the_risk_measure_matter(gpu, task, N, H):
    """The members are different plants (their costs differ in every rollout), so the nominal of the worst case differs from the nominal of the mean, and both differ from
    the nominal every member would plan alone.  A kernel that ignored the image stride, read another member's row, or a tail that read unaggregated costs fails here
    or in the bit comparisons above."""
    pr = _problems(gpu, task, list(_members(gpu, task)), N, 4, H, seed=7)
    pr.teeth("mppi")
    en = Ensemble(pr)
    KU = pr.KU
    worst_case, mean = en.call("mppi", 1), en.call("mppi", pr.B)
    assert (worst_case[1] != mean[1]).any() and (worst_case[1] >= mean[1]).all()
    assert (worst_case[2][:KU] != mean[2][:KU]).any()
    for b in range(pr.B):
        own = pr.single("mppi", b)[1][:KU]
        assert (own != worst_case[2][:KU]).any() and (own != mean[2][:KU]).any(), b
        assert (mean[0][b] != mean[1]).any(), b  # the tail did not read a member's own costs


# ------------------------------------------------------------------------------------------------ 4. M = 1 and identical members
@pytest.mark.parametrize("task,opt,N,H", [("cartpole", "mppi", 300, 8), ("cartpole", "cem", 300, 8), ("leap_cube", "mppi", 6, 8)])
def test_one_member_equals_plan_step(gpu, task, opt, N, H):
    """M = 1, worst = 1: costs, nominal and sigma are those of jh_plan_step on the member."""
    model = _members(gpu, task)[0]
    pr = _problems(gpu, task, [model], N, 4, H, seed=9)
    member, costs, out = Ensemble(pr).call(opt, 1)
    c1, o1 = pr.single(opt, 0)
    assert member[0].tobytes() == c1.tobytes() and costs.tobytes() == c1.tobytes()
    assert out.tobytes() == o1[: 2 * pr.KU].tobytes()


@pytest.mark.parametrize("M,worst", [(3, 1), (2, 2)])
@pytest.mark.parametrize("task,N,H", [("cartpole", 300, 8), ("leap_cube", 6, 8)])
def test_identical_members_equal_plan_step(gpu, task, N, H, M, worst):
    """M times the same handle: the maximum of equal values is the value, and (c + c) / 2 is exact, so the result is the single call's.  (Not a mean over 3: fl(3c) / 3
    need not give back c.)"""
    model = _members(gpu, task)[0]
    pr = _problems(gpu, task, [model] * M, N, 4, H, seed=10)
    member, costs, out = Ensemble(pr).call("mppi", worst)
    c1, o1 = pr.single("mppi", 0)
    for b in range(M):
        assert member[b].tobytes() == c1.tobytes()
    assert costs.tobytes() == c1.tobytes() and out.tobytes() == o1[: 2 * pr.KU].tobytes()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_ensemble_refusals(gpu):
    import torch

    from judo_amd.device import GpuModel, GpuModelSet

    models = list(_members(gpu, "cartpole"))
    pr = _problems(gpu, "cartpole", models, 8, 4, 8, seed=11)
    en = Ensemble(pr)
    L = pr.lib
    member = torch.full((3, 8), -7.0, dtype=torch.float32, device=gpu)
    costs = torch.full((8,), -7.0, dtype=torch.float32, device=gpu)
    out = torch.zeros(2 * pr.KU, dtype=torch.float32, device=gpu)
    base = en.args("mppi", 2, member.data_ptr(), costs.data_ptr(), out.data_ptr(), out.data_ptr())
    names = ["set", "blk_dev", "blk_host", "blk_bytes", "o_nominal", "o_sigma", "o_tp", "o_lohi", "noise", "ldn", "W", "N", "H", "K", "member_costs", "costs", "worst", "mode", "lambda", "k",
             "tie_high", "scratch", "out", "out_host_mark", "timing", "stream"]
    assert len(names) == len(base)

    def call(**kw):
        a = list(base)
        for key, v in kw.items():
            a[names.index(key)] = v
        return L.jh_plan_step_ensemble(*a)

    for ptr in ("set", "blk_dev", "blk_host", "noise", "W", "member_costs", "costs", "scratch", "out"):
        assert call(**{ptr: None}) == -1 and f"{ptr} is a null pointer" in _err(), ptr
    assert call(worst=0) == -1 and "worst = 0" in _err() and "M = 3" in _err()
    assert call(worst=4) == -1 and "worst = 4" in _err()
    assert call(N=0) == -1 and "N, H, K must be positive" in _err()
    assert call(ldn=7) == -1 and "ldn (7) < N (8)" in _err()
    assert call(K=513) == -1 and "K*nu = 513 exceeds 512" in _err()
    assert call(o_sigma=-1) == -1 and "negative block offset" in _err()
    assert call(blk_bytes=4 * pr.nblk - 4) == -1 and "does not hold" in _err()
    assert call(mode=2) == -1 and "mode must be" in _err()
    assert call(mode=0, **{"lambda": 0.0}) == -1 and "temperature" in _err()
    assert call(mode=1, k=0) == -1 and "k = 0" in _err()
    big = GpuModelSet([models[0]] * 33)
    assert call(set=big.handle, worst=33) == -1 and "33 members" in _err() and "JH_MAX_ENSEMBLE" in _err()
    big.close()
    forced = GpuModel("cartpole", gpu)
    forced.set_plan_step_launches(1)
    one = GpuModelSet([forced])
    assert call(set=one.handle, worst=1) == -1 and "one launch is forced" in _err()
    one.close()
    torch.cuda.synchronize()
    assert (member.cpu().numpy() == -7.0).all() and (costs.cpu().numpy() == -7.0).all() and (out.cpu().numpy() == 0).all()  # nothing ran
    assert call() == 0 and L.jh_download_end() == 0
    torch.cuda.synchronize()
    assert (member.cpu().numpy() != -7.0).all()
