"""jh_plan_step_ensemble_batch through the C ABI: B ensemble plan steps -- each controller's N candidates on its M plants, its own `worst`, its own nominal -- in ONE
call, against B calls of jh_plan_step_ensemble on the same blocks, noise slices and plants.

Every comparison is bit for bit (`view(np.uint32)`), no tolerance anywhere: the batched kernels run the ensemble call's code on pointers offset by the controller's and
the member's strides.  The problems are laid out by SetProblems (tests/test_gpu_model_set.py) with `distinct_problems`: B blocks and B noise slices at the padded
strides of tests/test_gpu_plan_batch.py; the controllers' x0 are made to differ here.  The plants come as a set of M, shared by all controllers, or as a set of B * M,
controller-major."""

import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_gpu_model_set import CARTPOLE, CYLINDER, LEAP_A, LEAP_B, LEAP_C, SetProblems, _models, _settled
from tests.test_gpu_plan_batch import OPTS, _err

pytestmark = pytest.mark.gpu

PAD_MEMBER = 7  # floats behind member_costs that the call must leave alone
# two more cartpole ensembles, so that a set of B * M = 9 holds nine different plants (controller 0's are tests/test_gpu_model_set.py's: shipped, CARTPOLE[0], CARTPOLE[1])
CARTPOLE_1 = [dict(body_mass={"pole": 1.2}), dict(body_mass={"pole": 1.7}), dict(body_mass={"pole": 0.85}, actuator_kp={None: 1.1})]
CARTPOLE_2 = [dict(body_mass={"pole": 0.9}), dict(body_mass={"pole": 1.35}), dict(body_mass={"pole": 0.6}, actuator_kp={None: 1.3})]


@functools.lru_cache(maxsize=None)
def _plants(gpu, task):
    """The shipped model of `task` and its perturbed members, made once for the module (no test changes a handle's settings).  cartpole: nine, three controllers' worth."""
    if task == "cartpole":
        return tuple(_models(gpu, task, CARTPOLE + CARTPOLE_1 + CARTPOLE_2))
    pert = {"cylinder_push": CYLINDER, "leap_cube": [LEAP_A, LEAP_B, LEAP_C]}.get(task, [LEAP_A])
    return tuple(_models(gpu, task, pert))


class FleetProblems:
    """B controllers x M plants.  `plants`: M models (every controller plans against them) or B * M, controller-major.  `call` is one jh_plan_step_ensemble_batch,
    `single(b)` jh_plan_step_ensemble on controller b's block, noise and plants with buffers of its own."""

    def __init__(self, gpu, task, plants, B, M, N, K, H, seed):
        import torch

        from judo_amd.device import GpuModelSet

        assert len(plants) in (M, B * M)
        self.B, self.M, self.N, self.plants = B, M, N, list(plants)
        lead = [plants[0]] * B
        if task == "cartpole":
            pr = SetProblems(gpu, task, lead, N, K, H, 0, seed=seed, x0=[0.1, 0.3, 0.0, 0.0], distinct_problems=True)
        elif task == "cylinder_push":
            pr = SetProblems(gpu, task, lead, N, K, H, 0, seed=seed, x0=[0.0, 0.0, -0.5, 0.0, 0.0, 0.0, 0.0, 0.0], sigma=3.0, distinct_problems=True)
        else:
            pr = SetProblems(gpu, task, lead, N, K, H, 0, seed=seed, x0=_settled(task, 5 if task == "leap_cube_down" else 60), distinct_problems=True)
        self.pr = pr
        # the controllers' states differ too: the cart / the pusher a little further along per controller; the leap hand's joints (q[7:23]) a little more closed
        blocks = pr.blocks.cpu().numpy()
        for b in range(B):
            if task in ("cartpole", "cylinder_push"):
                blocks[b, 0] += 0.05 * b
            else:
                blocks[b, 7:23] += 0.01 * b
        pr.blocks = torch.from_numpy(blocks).to(gpu)
        assert all((blocks[a, : pr.sizes[0]] != blocks[b, : pr.sizes[0]]).any() for a in range(B) for b in range(a + 1, B))
        self.set = GpuModelSet(self.plants)
        self.sets = [self.set if len(plants) == M else GpuModelSet(self.plants[b * M : (b + 1) * M]) for b in range(B)]
        self.scratch = torch.zeros(B * pr.per_scratch, dtype=torch.float32, device=gpu)
        self.mark = torch.zeros(4, dtype=torch.int32).pin_memory()

    def args(self, opt, worst, member, costs, out, mark, B=None):
        pr = self.pr
        mode, lam, k, tie = OPTS[opt]
        p = pr.blocks.data_ptr()
        B = self.B if B is None else B
        return [self.set.handle, B, self.M, p, p, 4 * pr.nblk, 4 * pr.blk_stride, pr.off[1], pr.off[2], pr.off[3], pr.off[4], pr.noise.data_ptr(), pr.ldn, pr.noise_stride, pr.W.data_ptr(),
                pr.N, pr.H, pr.K, member, costs, (C.c_int * len(worst))(*worst), mode, lam, k, tie, self.scratch.data_ptr(), out, pr.out_stride, mark, None, 0]

    def call(self, opt, worst, use_mark=False):
        """Returns (member_costs (B, M, N), costs (B, N), nominal | sigma (B, 2 KU)) as numpy; checks the pads behind member_costs and behind every output record."""
        import torch

        from judo_amd import _lib

        pr, B, M, N = self.pr, self.B, self.M, self.N
        member = torch.full((B * M * N + PAD_MEMBER,), -7.0, dtype=torch.float32, device=pr.dev)
        costs = torch.full((B, N), -7.0, dtype=torch.float32, device=pr.dev)
        out = torch.zeros((B, pr.out_stride), dtype=torch.float32, device=pr.dev)
        a = self.args(opt, worst, member.data_ptr(), costs.data_ptr(), out.data_ptr(), self.mark.data_ptr() if use_mark else out.data_ptr())
        _lib.check(pr.lib.jh_plan_step_ensemble_batch(*a), "jh_plan_step_ensemble_batch")
        _lib.check(pr.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        o, mc = out.cpu().numpy(), member.cpu().numpy()
        assert (o[:, 2 * pr.KU :] == 0).all(), "the call wrote between the output records"
        assert (mc[B * M * N :] == -7.0).all(), "the call wrote behind member_costs"
        return mc[: B * M * N].reshape(B, M, N).copy(), costs.cpu().numpy(), o[:, : 2 * pr.KU].copy()

    def single(self, opt, b, worst):
        """jh_plan_step_ensemble of controller b alone: (member_costs (M, N), costs (N,), nominal | sigma (2 KU,))."""
        import torch

        from judo_amd import _lib

        pr, M, N = self.pr, self.M, self.N
        mode, lam, k, tie = OPTS[opt]
        member = torch.full((M, N), -7.0, dtype=torch.float32, device=pr.dev)
        costs = torch.full((N,), -7.0, dtype=torch.float32, device=pr.dev)
        out = torch.zeros(2 * pr.KU, dtype=torch.float32, device=pr.dev)
        scratch = torch.zeros(pr.per_scratch, dtype=torch.float32, device=pr.dev)
        p = pr.blocks.data_ptr() + 4 * b * pr.blk_stride
        st = pr.lib.jh_plan_step_ensemble(self.sets[b].handle, p, p, 4 * pr.nblk, pr.off[1], pr.off[2], pr.off[3], pr.off[4], pr.noise.data_ptr() + 4 * b * pr.noise_stride, pr.ldn,
                                          pr.W.data_ptr(), N, pr.H, pr.K, member.data_ptr(), costs.data_ptr(), worst, mode, lam, k, tie, scratch.data_ptr(), out.data_ptr(), out.data_ptr(), None, 0)
        _lib.check(st, "jh_plan_step_ensemble")
        _lib.check(pr.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        return member.cpu().numpy(), costs.cpu().numpy(), out.cpu().numpy()

    def tickets(self):
        """The B + 1 ticket words: word 0 of every controller's scratch block and word 1 of controller 0's (with the rest of the four-word heads)."""
        return self.scratch.cpu().numpy().view(np.uint32).reshape(self.B, -1)[:, :4]

    def check(self, opt, worst, got, what=""):
        """Controller b of the batched call against jh_plan_step_ensemble on b alone with worst[b], and its costs against the numpy restatement of the risk measure."""
        from judo_amd.ensemble import aggregate_costs_host

        member, costs, out = got
        for b in range(self.B):
            m1, c1, o1 = self.single(opt, b, worst[b])
            assert np.isfinite(m1).all()
            for name, x, y in (("member costs", member[b], m1), ("costs", costs[b], c1), ("nominal | sigma", out[b], o1), ("costs against aggregate_costs_host", costs[b], aggregate_costs_host(member[b], worst[b]))):
                np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"{what} {opt} controller {b} worst={worst[b]}: {name}")

    def teeth(self, member):
        """An index mix-up cannot pass: any two controllers' member costs differ in every rollout, and so do any two members' costs of a controller."""
        B, M = self.B, self.M
        rows = member.reshape(B * M, -1)
        for a in range(B * M):
            for b in range(a + 1, B * M):
                same = int((rows[a] == rows[b]).sum())
                assert same == 0, f"(controller, member) {divmod(a, M)} and {divmod(b, M)} give the same cost in {same} of {self.N} rollouts: the case cannot tell them apart"


# ------------------------------------------------------------------------------------------------ 1. closed-form models
@pytest.mark.parametrize("task,opt", [("cartpole", "mppi"), ("cartpole", "cem"), ("cartpole", "ps"), ("cylinder_push", "mppi")])
def test_closed_form_ensemble_batch(gpu, task, opt):
    """B = 3, M = 3, N = 300 (two tail workgroups, the second ragged), H = 8, K = 4, worst = [1, 2, 3], with the stream's event and with the polled word (which starts
    at 0xFFFFFFFF: its wrap).  A second call on the same scratch gives the same bytes; the B + 1 ticket words are zero afterwards; the word counts the calls."""
    fp = FleetProblems(gpu, task, _plants(gpu, task)[:3], 3, 3, 300, 4, 8, seed=3)
    worst = [1, 2, 3]
    by_event = fp.call(opt, worst)
    fp.check(opt, worst, by_event, what=task)
    assert (fp.tickets() == 0).all()
    fp.mark.numpy().view(np.uint32)[0] = 0xFFFFFFFF
    for calls in (1, 2):
        by_word = fp.call(opt, worst, use_mark=True)
        assert int(fp.mark.numpy().view(np.uint32)[0]) == calls - 1  # (0xFFFFFFFF + 1 wraps to 0)
        for x, y in zip(by_event, by_word):
            assert x.tobytes() == y.tobytes()
        assert (fp.tickets() == 0).all()


@pytest.mark.parametrize("form", ["shared", "per_controller"])
def test_both_set_forms(gpu, form):
    """cartpole, B = 3, M = 3: a set of M that every controller shares, and a set of B * M = 9 in which every controller has plants of its own.  With its teeth."""
    plants = _plants(gpu, "cartpole")
    fp = FleetProblems(gpu, "cartpole", plants[:3] if form == "shared" else plants, 3, 3, 300, 4, 8, seed=5)
    assert fp.set.info()["B"] == (3 if form == "shared" else 9)
    if form == "per_controller":
        for m in range(3):
            assert plants[3 + m]._blob != plants[m]._blob and plants[6 + m]._blob != plants[m]._blob and plants[6 + m]._blob != plants[3 + m]._blob
    got = fp.call("mppi", [1, 2, 3])
    fp.teeth(got[0])
    fp.check("mppi", [1, 2, 3], got, what=f"cartpole {form}")
    if form == "per_controller":  # the same controllers on controller 0's plants plan something else: the controller axis of the images is read
        shared = FleetProblems(gpu, "cartpole", plants[:3], 3, 3, 300, 4, 8, seed=5).call("mppi", [1, 2, 3])
        assert shared[0][0].tobytes() == got[0][0].tobytes()
        assert (shared[0][1] != got[0][1]).all() and (shared[0][2] != got[0][2]).all()


# ------------------------------------------------------------------------------------------------ 2. the leap family
@pytest.mark.parametrize("opt", ["mppi", "cem"])
@pytest.mark.parametrize("B,M,N,H", [(2, 3, 6, 8), (2, 2, 352, 4)])
def test_leap_ensemble_batch(gpu, opt, B, M, N, H):
    """leap_cube (48 contacts) from the settled state, K = 4.  B = 2, M = 3, N = 6: one full group of four rollouts and one ragged, 36 rollouts in the launch -- the latency
    mode -- on a shared set.  B = 2, M = 2, N = 352: 1 408 rollouts in the launch, outside the latency mode, while each single ensemble call of 704 is still inside
    it; on a set of B * M = 4 (shipped, A | B, C)."""
    plants = _plants(gpu, "leap_cube")
    fp = FleetProblems(gpu, "leap_cube", plants[:3] if M == 3 else plants, B, M, N, 4, H, seed=22)
    worst = [1, M]
    got = fp.call(opt, worst)
    fp.teeth(got[0])
    fp.check(opt, worst, got, what=f"leap_cube B={B} M={M} N={N}")
    assert (fp.tickets() == 0).all()


def test_leap_ensemble_batch_on_the_64_contact_build(gpu):
    """leap_cube_down: B = 2, M = 2 (shipped, A), N = 6, H = 4."""
    plants = _plants(gpu, "leap_cube_down")
    got_build = plants[0].build()
    assert got_build["contact_capacity"] == 64 and not got_build["cylinder_build"]
    fp = FleetProblems(gpu, "leap_cube_down", plants, 2, 2, 6, 4, 4, seed=42)
    plants[0].stats(reset=True)
    fp.check("mppi", [2, 1], fp.call("mppi", [2, 1]), what="leap_cube_down")
    assert plants[0].stats(reset=True)["overflow_pool_fallbacks"] == 0
    assert (fp.tickets() == 0).all()


# ------------------------------------------------------------------------------------------------ 3. degenerate axes
@pytest.mark.parametrize("task,opt,N,H", [("cartpole", "cem", 300, 8), ("leap_cube", "mppi", 6, 8)])
def test_one_controller_equals_the_ensemble_call(gpu, task, opt, N, H):
    fp = FleetProblems(gpu, task, _plants(gpu, task)[:3], 1, 3, N, 4, H, seed=9)
    fp.check(opt, [2], fp.call(opt, [2]), what=f"{task} B=1")


@pytest.mark.parametrize("task,opt,N,H", [("cartpole", "mppi", 300, 8), ("cartpole", "cem", 300, 8), ("leap_cube", "mppi", 6, 8)])
def test_one_member_equals_plan_step_batch_models(gpu, task, opt, N, H):
    """M = 1, worst = 1: a controller's costs are its member's, and nominal | sigma are jh_plan_step_batch_models' on the same blocks, noise and plant."""
    fp = FleetProblems(gpu, task, _plants(gpu, task)[:1], 3, 1, N, 4, H, seed=10)
    member, costs, out = fp.call(opt, [1, 1, 1])
    assert member[:, 0].tobytes() == costs.tobytes()
    c_b, o_b = fp.pr.batch_models(opt)  # (fp.pr's own set: B times the plant)
    assert costs.tobytes() == c_b.tobytes() and out.tobytes() == o_b[:, : 2 * fp.pr.KU].tobytes()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_ensemble_batch_refusals(gpu):
    """Every refusal comes before anything is enqueued: the buffers, the ticket words and the mark stay as they were."""
    import torch

    from judo_amd.device import GpuModel, GpuModelSet

    plants = _plants(gpu, "cartpole")
    fp = FleetProblems(gpu, "cartpole", plants[:3], 3, 3, 8, 4, 8, seed=11)
    pr, L = fp.pr, fp.pr.lib
    member = torch.full((3, 3, 8), -7.0, dtype=torch.float32, device=gpu)
    costs = torch.full((3, 8), -7.0, dtype=torch.float32, device=gpu)
    out = torch.zeros((3, pr.out_stride), dtype=torch.float32, device=gpu)
    fp.mark.numpy().view(np.uint32)[0] = 41
    base = fp.args("mppi", [1, 2, 3], member.data_ptr(), costs.data_ptr(), out.data_ptr(), fp.mark.data_ptr())
    names = ["set", "B", "M", "blk_dev", "blk_host", "blk_bytes", "blk_stride_bytes", "o_nominal", "o_sigma", "o_tp", "o_lohi", "noise", "ldn", "noise_stride_floats", "W", "N", "H", "K",
             "member_costs", "costs", "worst", "mode", "lambda", "k", "tie_high", "scratch", "out", "out_stride_floats", "out_host_mark", "timing", "stream"]
    assert len(names) == len(base)

    def call(**kw):
        a = list(base)
        for key, v in kw.items():
            a[names.index(key)] = v
        return L.jh_plan_step_ensemble_batch(*a)

    def ints(*v):
        return (C.c_int * len(v))(*v)

    for ptr in ("set", "blk_dev", "blk_host", "noise", "W", "member_costs", "costs", "worst", "scratch", "out"):
        assert call(**{ptr: None}) == -1 and f"{ptr} is a null pointer" in _err(), ptr
    assert call(B=257, worst=ints(*([1] * 257))) == -1 and "B = 257" in _err() and "JH_MAX_ENSEMBLE_FLEET = 256" in _err()
    assert call(B=0) == -1 and "B = 0" in _err()
    assert call(worst=ints(1, 0, 3)) == -1 and "controller 1" in _err() and "worst = 0" in _err() and "M = 3" in _err()
    assert call(worst=ints(1, 4, 3)) == -1 and "controller 1" in _err() and "worst = 4" in _err()
    four = GpuModelSet(list(plants[:4]))
    assert call(set=four.handle) == -1 and "a set of 4 members" in _err() and "M = 3" in _err() and "B * M = 9" in _err()
    four.close()
    big = GpuModelSet([plants[0]] * 33)
    assert call(set=big.handle, M=33) == -1 and "M = 33" in _err() and "JH_MAX_ENSEMBLE = 32" in _err()
    big.close()
    assert call(N=0) == -1 and "N, H, K must be positive" in _err()
    assert call(ldn=7) == -1 and "ldn (7) < N (8)" in _err()
    assert call(o_sigma=-1) == -1 and "negative block offset" in _err()
    assert call(blk_bytes=4 * pr.nblk - 4) == -1 and "does not hold" in _err()
    assert call(blk_stride_bytes=4 * pr.nblk - 4) == -1 and "blk_stride_bytes" in _err()
    assert call(noise_stride_floats=pr.KU * pr.ldn - 1) == -1 and "noise_stride_floats" in _err()
    assert call(out_stride_floats=2 * pr.KU - 1) == -1 and "out_stride_floats" in _err()
    assert call(mode=2) == -1 and "mode must be" in _err()
    assert call(mode=0, **{"lambda": 0.0}) == -1 and "temperature" in _err()
    assert call(mode=1, k=0) == -1 and "k = 0" in _err()
    forced = GpuModel("cartpole", gpu)
    forced.set_plan_step_launches(1)
    one = GpuModelSet([forced])
    assert call(set=one.handle, M=1, worst=ints(1, 1, 1)) == -1 and "one launch is forced" in _err()
    one.close()
    # fr3_pick: the call takes its plants as a model set, and no set holds an fr3_pick model -- the refusal a caller meets is the set's, with the status and the name
    fr3 = GpuModel("fr3_pick", gpu)
    handles = (C.c_void_p * 1)(fr3.handle)
    made = C.c_void_p()
    assert L.jh_model_set_create(handles, 1, C.byref(made)) == -3 and "fr3_pick" in _err()
    torch.cuda.synchronize()
    assert (member.cpu().numpy() == -7.0).all() and (costs.cpu().numpy() == -7.0).all() and (out.cpu().numpy() == 0).all()  # nothing ran
    assert (fp.tickets() == 0).all() and int(fp.mark.numpy().view(np.uint32)[0]) == 41
    assert call() == 0 and L.jh_download_end() == 0
    torch.cuda.synchronize()
    assert (member.cpu().numpy() != -7.0).all() and int(fp.mark.numpy().view(np.uint32)[0]) == 42 and (fp.tickets() == 0).all()
