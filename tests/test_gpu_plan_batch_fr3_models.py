"""jh_plan_step_batch_phases_models through the C ABI: B fr3_pick plan steps, each on its own plant of an fr3 model set and in its own phase, in one launch against B
calls of jh_plan_step(member b's own handle, ..., phase_b, ...) on the same sub-blocks.

Every comparison is on raw 32-bit words: the batched instantiation of the fr3 kernel offsets the base of the model's float section by the problem's image and runs the
single call's code, which is the path held to the oracle (tests/test_gpu_fr3.py).  No tolerance appears in this file.  The problems are laid out by the builder of
tests/test_gpu_plan_batch_fr3.py; the plants are D0..D3 of tests/test_fr3_plants_host.py."""

import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_fr3_plants_host import plants
from tests.test_gpu_plan_batch_fr3 import OPTS, E, K, Problems, _err, _phase_states, _pressed_states

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _models(dev, self_collision=False):
    """GpuModels of D0..D3, made once per build."""
    from judo_amd.device import GpuModel

    return tuple(GpuModel(d, dev) for d in plants(self_collision))


class PlantProblems(Problems):
    """`Problems` whose problem b runs on `models[b]`: the batch is one jh_plan_step_batch_phases_models on the set of the models, `single(opt, b)` one jh_plan_step on
    models[b]'s own handle."""

    def __init__(self, dev, models, N, H, seed, x0s, phases, **kw):
        from judo_amd.device import GpuModelSet

        self.models = list(models)
        super().__init__(dev, len(self.models), N, H, seed, x0s, phases, model=self.models[0], **kw)
        self.set = GpuModelSet(self.models)
        assert self.set.fr3 and self.set.info()["B"] == self.B

    def call(self, costs, trace, out, opt="mppi", use_mark=False, B=None, handle=None, o_phase=None, k=K):
        mode, lam, kk, tie = OPTS[opt]
        return self.lib.jh_plan_step_batch_phases_models(handle or self.set.handle, self.B if B is None else B, self.blocks_dev.data_ptr(), self.host.data_ptr(), 4 * self.nblk,
                                                         4 * self.blk_stride, self.off[1], self.off[2], self.off[3], self.off[4], self.o_phase if o_phase is None else o_phase,
                                                         self.noise.data_ptr(), self.ldn, self.noise_stride, self.W.data_ptr(), self.N, self.H, k, costs.data_ptr(), trace.data_ptr(), mode,
                                                         lam, kk, tie, E, self.row, self.colmajor, self.batch_scratch.data_ptr(), out.data_ptr(), self.out_stride,
                                                         self.mark.data_ptr() if use_mark else out.data_ptr(), None, 0)

    def single(self, opt, b, model=None):
        return super().single(opt, b, model=model or self.models[b])


# ------------------------------------------------------------------------------------------------ 1. three plants, three phases, both builds
@pytest.mark.parametrize("self_collision", [False, True])
@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
def test_three_plants_in_three_phases(gpu, opt, self_collision):
    """B = 3 on D1, D2, D3, N = 6 (two groups of four rows, the second ragged), H = 8, phases (0, 2, 3), each from its phase state.  Precondition: on ONE block (problem 0's)
    the three plants cost differently in every rollout, so a launch that ignored the image stride cannot pass."""
    ms = _models(gpu, self_collision)
    assert all(m.fr3_build()["self_collision_build"] == self_collision for m in ms)
    xs = _phase_states()
    pr = PlantProblems(gpu, ms[1:], 6, 8, seed=21, x0s=[xs[0], xs[2], xs[3]], phases=(0, 2, 3))
    assert pr.set.info()["distinct_from_first"] == 2
    common = [pr.single(opt, 0, model=m)[0] for m in pr.models]
    for i in range(3):
        for j in range(i + 1, 3):
            assert (common[i].view(np.uint32) != common[j].view(np.uint32)).all(), (i, j, common[i], common[j])
    pr.check(opt, pr.batch(opt), what="three plants")


# ------------------------------------------------------------------------------------------------ 2. the two other launch shapes
@pytest.mark.parametrize("B", [5, 9])
def test_launch_shapes_outside_the_full_latency_mode(gpu, B):
    """N = 256, H = 4.  B = 5: 1 280 rollouts, two rows of a wave per rollout; B = 9: 2 304 rollouts, every row its own rollout.  Members cycle over D0..D3, phases over 0..3
    one step out of phase with them."""
    ms, xs = _models(gpu), _phase_states()
    phases = [(b + b // 4) % 4 for b in range(B)]
    pr = PlantProblems(gpu, [ms[b % 4] for b in range(B)], 256, 4, seed=30 + B, x0s=[xs[p] for p in phases], phases=phases)
    pr.check("mppi", pr.batch("mppi"), what=f"B*N={B * 256}")


# ------------------------------------------------------------------------------------------------ 3. overflow rows
def test_overflow_rows_of_the_second_problem_on_its_own_plant(gpu):
    """B = 2, N = 6, H = 4 from states with more than 32 general contacts; problem 1 runs on D2 (a heavier cube, less pad friction, a weaker gripper).  Nothing is dropped
    and the fallback is not taken; the counters are member 0's."""
    xs, gen = _pressed_states()
    assert all(32 < n <= 96 for n in gen), gen
    ms = _models(gpu)
    pr = PlantProblems(gpu, [ms[0], ms[2]], 6, 4, seed=6, x0s=xs, phases=(0, 1), plain=True)
    ms[0].stats(reset=True)
    got = pr.batch("mppi")
    st = ms[0].stats(reset=True)
    assert st["overflow_pool_fallbacks"] == 0 and st["contact_overflow"] == 0, st
    assert (pr.single("mppi", 1)[0] != pr.single("mppi", 1, model=ms[0])[0]).any()  # (the plant matters in these states)
    pr.check("mppi", got, what="overflow rows")


# ------------------------------------------------------------------------------------------------ 4. set update, back-to-back calls
@pytest.mark.parametrize("use_mark", [True, False])
def test_set_update_and_a_second_call_on_the_same_scratch(gpu, use_mark):
    ms, xs = _models(gpu), _phase_states()
    pr = PlantProblems(gpu, ms[1:], 6, 8, seed=9, x0s=xs[1:], phases=(1, 2, 3))
    old = 0xDEADBEEF
    pr.mark.numpy().view(np.uint32)[0] = old
    first = pr.batch("cem", use_mark=use_mark)
    second = pr.batch("cem", use_mark=use_mark)
    assert int(pr.mark.numpy().view(np.uint32)[0]) == ((old + 2) & 0xFFFFFFFF if use_mark else old)
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()
    assert (pr.batch_scratch.cpu().numpy().view(np.uint32).reshape(3, -1)[:, :4] == 0).all()  # every problem's ticket and the batch's are back at zero
    pr.check("cem", first, what="before the update")
    pr.set.update(1, ms[0])  # member 1: D2 -> D0
    pr.models[1] = ms[0]
    third = pr.batch("cem", use_mark=use_mark)
    assert (third[0][1] != first[0][1]).any() and third[0][0].tobytes() == first[0][0].tobytes() and third[0][2].tobytes() == first[0][2].tobytes()
    pr.check("cem", third, what="after the update")
    assert pr.set.info()["distinct_from_first"] == 2  # (D0 and D3 against D1)


# ------------------------------------------------------------------------------------------------ 5. refusals
def _create(fn, models):
    from judo_amd import _lib

    hs = (C.c_void_p * len(models))(*[m.handle.value for m in models])
    out = C.c_void_p()
    st = getattr(_lib.lib(), fn)(hs, len(models), C.byref(out))
    if st == 0:
        _lib.lib().jh_model_set_destroy(out)
    return st


def test_refusals(gpu):
    import torch

    from judo_amd.device import GpuModel, GpuModelSet

    ms, xs = _models(gpu), _phase_states()
    leap, cart = GpuModel("leap_cube", gpu), GpuModel("cartpole", gpu)
    # the constructors
    assert _create("jh_model_set_create", [ms[0]]) == -3 and "member 0" in _err() and "fr3_pick" in _err() and "jh_fr3_model_set_create" in _err()
    assert _create("jh_fr3_model_set_create", [ms[0], leap]) == -3 and "member 1" in _err() and "no fr3_pick model" in _err()
    assert _create("jh_fr3_model_set_create", [leap]) == -3 and "member 0" in _err()
    assert _create("jh_fr3_model_set_create", [ms[0], _models(gpu, True)[1]]) == -1 and "member 1" in _err()  # the default and the self-collision build do not mix
    assert _create("jh_fr3_model_set_create", list(ms)) == 0
    pr = PlantProblems(gpu, ms[1:], 6, 8, seed=10, x0s=xs[:3], phases=(0, 1, 2))
    # jh_model_set_update: an fr3 member on another set and the reverse
    carts = GpuModelSet([cart, cart])
    assert not carts.fr3
    assert pr.lib.jh_model_set_update(carts.handle, 1, ms[0].handle) == -3 and "fr3_pick" in _err()
    assert pr.lib.jh_model_set_update(pr.set.handle, 1, leap.handle) == -3 and "no fr3_pick model" in _err()
    assert pr.set.info()["distinct_from_first"] == 2 and carts.info()["distinct_from_first"] == 0  # (a refused update changes nothing)
    costs, trace, out = pr.outputs()
    # the five set-taking entries without a phase
    h, blk, host, nb, st_b = pr.set.handle, pr.blocks_dev.data_ptr(), pr.host.data_ptr(), 4 * pr.nblk, 4 * pr.blk_stride
    o, noise, W, N, H = pr.off, pr.noise.data_ptr(), pr.W.data_ptr(), pr.N, pr.H
    mc = torch.full((3, N), -7.0, dtype=torch.float32, device=gpu)
    tail = (pr.batch_scratch.data_ptr(), out.data_ptr())
    table, worst = (C.c_ubyte * 3)(0, 1, 2), (C.c_int * 1)(1)
    L = pr.lib
    st = L.jh_plan_step_ensemble(h, blk, host, nb, o[1], o[2], o[3], o[4], noise, pr.ldn, W, N, H, K, mc.data_ptr(), costs.data_ptr(), 1, 0, 0.05, 0, 0, *tail, out.data_ptr(), None, 0)
    assert st == -3 and "fr3_pick" in _err() and "jh_plan_step_randomized_phase" in _err()
    st = L.jh_plan_step_ensemble_batch(h, 1, 3, blk, host, nb, st_b, o[1], o[2], o[3], o[4], noise, pr.ldn, pr.noise_stride, W, N, H, K, mc.data_ptr(), costs.data_ptr(), worst, 0, 0.05, 0, 0, *tail,
                                       pr.out_stride, out.data_ptr(), None, 0)
    assert st == -3 and "fr3_pick" in _err() and "jh_plan_step_batch_phases_models" in _err()
    st = L.jh_plan_step_randomized_batch(h, 1, 3, blk, host, nb, st_b, o[1], o[2], o[3], o[4], noise, pr.ldn, pr.noise_stride, W, N, H, K, table, 3, costs.data_ptr(), 0, 0.05, 0, 0, *tail,
                                         pr.out_stride, out.data_ptr(), None, 0)
    assert st == -3 and "fr3_pick" in _err() and "jh_plan_step_randomized_phase" in _err()
    st = L.jh_plan_step_randomized(h, blk, host, nb, o[1], o[2], o[3], o[4], noise, pr.ldn, W, N, H, K, table, 3, costs.data_ptr(), 0, 0.05, 0, 0, *tail, out.data_ptr(), None, 0)
    assert st == -3 and "jh_plan_step_randomized_phase" in _err()
    st = L.jh_plan_step_batch_models(h, blk, host, nb, st_b, o[1], o[2], o[3], o[4], noise, pr.ldn, pr.noise_stride, W, N, H, K, costs.data_ptr(), trace.data_ptr(), 0, 0.05, 0, 0, E, pr.row,
                                     pr.colmajor, *tail, pr.out_stride, out.data_ptr(), None, 0)
    assert st == -3 and "jh_plan_step_batch_phases_models" in _err()
    # the new entry's own
    leaps = GpuModelSet([leap, leap])
    assert pr.call(costs, trace, out, handle=leaps.handle, B=2) == -3 and "jh_plan_step_batch_models" in _err()
    word = pr.host.numpy()[:, pr.o_phase]
    for bad in (4.0, 1.5, float("nan")):
        word[1] = bad
        assert pr.call(costs, trace, out) == -1 and "problem 1" in _err()
    word[1] = 1.0
    assert pr.call(costs, trace, out, B=2) == -1 and "set of 3" in _err()
    assert pr.call(costs, trace, out, B=4) == -1 and "set of 3" in _err()
    assert pr.call(costs, trace, out, o_phase=pr.nblk) == -1 and "o_phase" in _err()
    assert pr.call(costs, trace, out, o_phase=-1) == -1 and "o_phase" in _err()
    assert pr.call(costs, trace, out, k=9) == -1 and "at most 8 knots" in _err()
    torch.cuda.synchronize()
    assert (costs.cpu().numpy() == -7.0).all() and (mc.cpu().numpy() == -7.0).all() and (trace.cpu().numpy() == 0).all() and (out.cpu().numpy() == 0).all()  # nothing ran
    pr.check("mppi", pr.batch("mppi"), what="after the refusals")
