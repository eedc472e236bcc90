"""jh_plan_step_randomized_batch through the C ABI: B domain-randomised plan steps -- each controller's N candidates in G blocks, block g on the plant its own table
names -- in ONE call, against B calls of jh_plan_step_randomized on the same blocks, noise slices, plants and tables.

Every comparison is bit for bit (`view(np.uint32)` / `tobytes()`), no tolerance anywhere: the batched kernels run the randomised call's code on pointers offset by
the controller's and the block's strides, and read the plant from entry (controller, block) of a table that travels in the kernel arguments.  The single call is itself
held to jh_plan_step and jh_update_fused by tests/test_gpu_plan_randomized.py.  The problems are FleetProblems' (tests/test_gpu_plan_ensemble_batch.py): B blocks
and B noise slices at padded strides, every controller with its own state; the plants come as a set of M, shared by all controllers, or as a set of B * M,
controller-major."""

import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_plan_batch import OPTS, _err
from tests.test_gpu_plan_ensemble_batch import FleetProblems, _plants

pytestmark = pytest.mark.gpu

PAD_COSTS = 7  # floats behind `costs` that the call must leave alone


def _table(rows):
    flat = [p for r in rows for p in r]
    return (C.c_ubyte * len(flat))(*flat)


class RandomizedProblems(FleetProblems):
    """FleetProblems with `call` = one jh_plan_step_randomized_batch and `single(b)` = jh_plan_step_randomized on controller b's block, noise, plants and table."""

    def rargs(self, opt, tables, costs, out, mark, B=None, G=None):
        pr = self.pr
        mode, lam, k, tie = OPTS[opt]
        p = pr.blocks.data_ptr()
        return [self.set.handle, self.B if B is None else B, self.M, p, p, 4 * pr.nblk, 4 * pr.blk_stride, pr.off[1], pr.off[2], pr.off[3], pr.off[4], pr.noise.data_ptr(), pr.ldn, pr.noise_stride,
                pr.W.data_ptr(), pr.N, pr.H, pr.K, _table(tables), len(tables[0]) if G is None else G, costs, mode, lam, k, tie, self.scratch.data_ptr(), out, pr.out_stride, mark, None, 0]

    def call(self, opt, tables, use_mark=False):
        """Returns (costs (B, N), nominal | sigma (B, 2 KU)) as numpy; checks the pads behind `costs` and behind every output record."""
        import torch

        from judo_amd import _lib

        pr, B, N = self.pr, self.B, self.N
        assert len(tables) == B
        costs = torch.full((B * N + PAD_COSTS,), -7.0, dtype=torch.float32, device=pr.dev)
        out = torch.zeros((B, pr.out_stride), dtype=torch.float32, device=pr.dev)
        a = self.rargs(opt, tables, costs.data_ptr(), out.data_ptr(), self.mark.data_ptr() if use_mark else out.data_ptr())
        _lib.check(pr.lib.jh_plan_step_randomized_batch(*a), "jh_plan_step_randomized_batch")
        _lib.check(pr.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        o, c = out.cpu().numpy(), costs.cpu().numpy()
        assert (o[:, 2 * pr.KU :] == 0).all(), "the call wrote between the output records"
        assert (c[B * N :] == -7.0).all(), "the call wrote behind costs"
        return c[: B * N].reshape(B, N).copy(), o[:, : 2 * pr.KU].copy()

    def single(self, opt, b, table):
        """jh_plan_step_randomized of controller b alone: (costs (N,), nominal | sigma (2 KU,))."""
        import torch

        from judo_amd import _lib

        pr, N = self.pr, self.N
        mode, lam, k, tie = OPTS[opt]
        costs = torch.full((N,), -7.0, dtype=torch.float32, device=pr.dev)
        out = torch.zeros(2 * pr.KU, dtype=torch.float32, device=pr.dev)
        scratch = torch.zeros(pr.per_scratch, dtype=torch.float32, device=pr.dev)
        p = pr.blocks.data_ptr() + 4 * b * pr.blk_stride
        st = pr.lib.jh_plan_step_randomized(self.sets[b].handle, p, p, 4 * pr.nblk, pr.off[1], pr.off[2], pr.off[3], pr.off[4], pr.noise.data_ptr() + 4 * b * pr.noise_stride, pr.ldn,
                                            pr.W.data_ptr(), N, pr.H, pr.K, _table([table]), len(table), costs.data_ptr(), mode, lam, k, tie, scratch.data_ptr(), out.data_ptr(), out.data_ptr(),
                                            None, 0)
        _lib.check(st, "jh_plan_step_randomized")
        _lib.check(pr.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        return costs.cpu().numpy(), out.cpu().numpy()

    def plain(self, opt, b, plant):
        """jh_plan_step on the handle of controller b's plant `plant`, with b's block and noise: (costs (N,), nominal | sigma (2 KU,)).  Its rollout 0 is noise-free."""
        pr = self.pr
        model = self.plants[plant] if len(self.plants) == self.M else self.plants[b * self.M + plant]
        keep = pr.models[b]
        pr.models[b] = model
        try:
            c, o = pr.single(opt, b)
        finally:
            pr.models[b] = keep
        return c, o[: 2 * pr.KU]

    def check(self, opt, tables, got, what=""):
        """Controller b of the batched call against jh_plan_step_randomized on b alone with tables[b]."""
        costs, out = got
        for b in range(self.B):
            c1, o1 = self.single(opt, b, tables[b])
            assert np.isfinite(c1).all()
            for name, x, y in (("costs", costs[b], c1), ("nominal | sigma", out[b], o1)):
                np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"{what} {opt} controller {b} table {tables[b]}: {name}")


def _same_problem(fp, src, dst):
    """Controller `dst` takes controller `src`'s block and noise slice."""
    fp.pr.blocks[dst] = fp.pr.blocks[src]
    fp.pr.noise[dst] = fp.pr.noise[src]


# ------------------------------------------------------------------------------------------------ 1. closed-form models
@pytest.mark.parametrize("task,opt", [("cartpole", "mppi"), ("cartpole", "cem"), ("cartpole", "ps"), ("cylinder_push", "mppi")])
def test_closed_form_randomized_batch(gpu, task, opt):
    """B = 3, M = 3, N = 300, H = 8, K = 4: G = 3 (Nb = 100: ragged waves) and G = 6 (Nb = 50: G > M, repeats), each with the stream's event and with the polled word,
    which starts at a non-zero value -- and with that twice on one scratch.  The B + 1 ticket words are zero after every call; the word counts the calls."""
    fp = RandomizedProblems(gpu, task, _plants(gpu, task)[:3], 3, 3, 300, 4, 8, seed=3)
    fp.mark.numpy().view(np.uint32)[0] = 0xFFFFFFFE
    marks = 0xFFFFFFFE
    for tables in ([[2, 0, 1], [0, 0, 2], [1, 2, 2]], [[1, 1, 0, 2, 2, 2], [0, 2, 1, 0, 2, 1], [2, 2, 2, 0, 0, 1]]):
        by_event = fp.call(opt, tables)
        fp.check(opt, tables, by_event, what=task)
        assert (fp.tickets() == 0).all()
        for _ in range(2):
            by_word = fp.call(opt, tables, use_mark=True)
            marks = (marks + 1) & 0xFFFFFFFF
            assert int(fp.mark.numpy().view(np.uint32)[0]) == marks
            for x, y in zip(by_event, by_word):
                assert x.tobytes() == y.tobytes()
            assert (fp.tickets() == 0).all()


def test_a_table_per_controller_and_one_nominal_per_controller(gpu):
    """The teeth.  cartpole, B = 3, M = 3, G = 3, N = 300: controllers 0 and 1 have the same block and the same noise slice, and tables that differ in block 1 alone.
    Their costs are bit-equal in blocks 0 and 2 and differ in every rollout of block 1: each controller reads its own row of the table.  Rollout g * Nb, g >= 1, of
    every controller differs from the noise-free rollout on that block's plant, and rollout 0 of every controller -- 1 and 2 included -- is that noise-free rollout:
    only a controller's global rollout 0 dropped its noise."""
    fp = RandomizedProblems(gpu, "cartpole", _plants(gpu, "cartpole")[:3], 3, 3, 300, 4, 8, seed=13)
    _same_problem(fp, 0, 1)
    tables = [[2, 0, 1], [2, 1, 1], [1, 2, 0]]
    costs, out = fp.call("mppi", tables)
    fp.check("mppi", tables, (costs, out), what="teeth")
    Nb = 100
    assert costs[0, :Nb].tobytes() == costs[1, :Nb].tobytes() and costs[0, 2 * Nb :].tobytes() == costs[1, 2 * Nb :].tobytes()
    assert (costs[0, Nb : 2 * Nb] != costs[1, Nb : 2 * Nb]).all()
    for b in range(3):
        for g in range(3):
            free = fp.plain("mppi", b, tables[b][g])[0][0]  # the noise-free rollout of controller b on block g's plant
            got = costs[b, g * Nb]
            assert (got.tobytes() == free.tobytes()) == (g == 0), (b, g)


def test_a_table_past_64_bytes(gpu):
    """cartpole, B = 5, G = 16, N = 320 (Nb = 20): B * G = 80 entries, so controller 4's row lies behind byte 64 of the table, word 16 and later.  Its table is unlike
    the others', and the others differ among themselves."""
    from judo_amd import _lib

    assert 5 * 16 > _lib.MAX_PLANT_BLOCKS
    fp = RandomizedProblems(gpu, "cartpole", _plants(gpu, "cartpole")[:3], 5, 3, 320, 4, 8, seed=17)
    tables = [[(g + b) % 3 for g in range(16)] for b in range(4)] + [[2, 2, 1, 0, 0, 0, 1, 2, 1, 1, 0, 2, 2, 0, 1, 0]]
    assert all(tables[4] != t for t in tables[:4])
    got = fp.call("mppi", tables)
    fp.check("mppi", tables, got, what="B * G = 80")
    assert (fp.tickets() == 0).all()
    # controller 4 with controller 0's problem and its own table differs from controller 0 exactly in the blocks whose plants differ
    _same_problem(fp, 0, 4)
    costs, _ = fp.call("mppi", tables)
    for g in range(16):
        same = costs[0, g * 20 : (g + 1) * 20] == costs[4, g * 20 : (g + 1) * 20]
        assert same.all() if tables[0][g] == tables[4][g] else not same.any(), g


@pytest.mark.parametrize("form", ["shared", "per_controller"])
def test_both_set_forms(gpu, form):
    """cartpole, B = 3, M = 3, G = 3: a set of M that every controller shares, and a set of B * M = 9 in which controller b's plant m differs from controller 0's plant
    m.  Rows follow their own plants: on the set of 9 controllers 1 and 2 plan something else than on controller 0's plants."""
    plants = _plants(gpu, "cartpole")
    fp = RandomizedProblems(gpu, "cartpole", plants[:3] if form == "shared" else plants, 3, 3, 300, 4, 8, seed=5)
    assert fp.set.info()["B"] == (3 if form == "shared" else 9)
    tables = [[2, 0, 1], [0, 0, 2], [1, 2, 2]]
    got = fp.call("mppi", tables)
    fp.check("mppi", tables, got, what=f"cartpole {form}")
    if form == "per_controller":
        for m in range(3):
            assert plants[3 + m]._blob != plants[m]._blob and plants[6 + m]._blob != plants[m]._blob
        shared = RandomizedProblems(gpu, "cartpole", plants[:3], 3, 3, 300, 4, 8, seed=5).call("mppi", tables)
        assert shared[0][0].tobytes() == got[0][0].tobytes()
        assert (shared[0][1] != got[0][1]).all() and (shared[0][2] != got[0][2]).all()


# ------------------------------------------------------------------------------------------------ 2. the leap family
def _shift(rollouts, cus):
    """jh_latency_shift's rule for the leap kernel (four rollout rows per wave; jh_api.hip): the largest shift that leaves every wave of the launch a SIMD of its own."""
    return next((s for s in (2, 1) if (rollouts << s) <= cus * 4 * 4), 0)


@pytest.mark.parametrize("opt", ["mppi", "cem"])
@pytest.mark.parametrize("N,H,tables", [(24, 8, [[3, 0, 2, 0], [1, 1, 0, 2]]), (704, 4, [[3, 0, 2, 1], [0, 2, 2, 3]])])
def test_leap_randomized_batch(gpu, opt, N, H, tables):
    """leap_cube (48 contacts) from the settled state, B = 2, M = 4, K = 4, G = 4.  N = 24 (Nb = 6: one full group of four rollouts and a ragged one per block): the
    launch of 48 rollouts in the latency mode, as the single calls are.  N = 704 (Nb = 176): the launch's latency shift is chosen from B * N = 1 408 rollouts and is
    another than the single call's, chosen from 704 (asserted from the launcher's rule on this GPU's compute units) -- and the bits are the same."""
    import torch

    if N == 704:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert _shift(2 * N, cus) != _shift(N, cus), (cus, _shift(2 * N, cus), _shift(N, cus))
    fp = RandomizedProblems(gpu, "leap_cube", _plants(gpu, "leap_cube"), 2, 4, N, 4, H, seed=22)
    got = fp.call(opt, tables)
    fp.check(opt, tables, got, what=f"leap_cube N={N}")
    assert (fp.tickets() == 0).all()
    again = fp.call(opt, tables)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes() and (fp.tickets() == 0).all()


@pytest.mark.parametrize("task,build", [("leap_cube_down", dict(contact_capacity=64, cylinder_build=False)), ("caltech_cylinder", dict(contact_capacity=64, cylinder_build=True))])
def test_leap_randomized_batch_on_the_other_builds(gpu, task, build):
    """The 64-contact build (leap_cube_down) and the cylinder build (caltech_leap_cube with its fingertip cylinders): B = 2, M = 2 (shipped, A), N = 24, G = 4, H = 4."""
    plants = _plants(gpu, task)
    got_build = plants[0].build()
    assert {k: got_build[k] for k in build} == build
    fp = RandomizedProblems(gpu, task, plants, 2, 2, 24, 4, 4, seed=42)
    plants[0].stats(reset=True)
    tables = [[1, 0, 0, 1], [0, 0, 1, 1]]
    fp.check("mppi", tables, fp.call("mppi", tables), what=task)
    assert plants[0].stats(reset=True)["overflow_pool_fallbacks"] == 0
    assert (fp.tickets() == 0).all()


# ------------------------------------------------------------------------------------------------ 3. degenerate axes
@pytest.mark.parametrize("task,opt,N,H,table", [("cartpole", "cem", 300, 8, [2, 0, 1]), ("leap_cube", "mppi", 24, 8, [1, 2, 0, 1])])
def test_one_controller_equals_the_randomized_call(gpu, task, opt, N, H, table):
    fp = RandomizedProblems(gpu, task, _plants(gpu, task)[:3], 1, 3, N, 4, H, seed=9)
    fp.check(opt, [table], fp.call(opt, [table]), what=f"{task} B=1")
    assert (fp.tickets() == 0).all()


@pytest.mark.parametrize("task,opt,N,H", [("cartpole", "mppi", 300, 8), ("cartpole", "cem", 300, 8), ("leap_cube", "mppi", 24, 8)])
def test_one_block_equals_plan_step(gpu, task, opt, N, H):
    """G = 1 with the tables [p_b]: controller b's results are jh_plan_step's on plant p_b with b's block and noise."""
    fp = RandomizedProblems(gpu, task, _plants(gpu, task)[:3], 3, 3, N, 4, H, seed=10)
    tables = [[2], [0], [1]]
    costs, out = fp.call(opt, tables)
    for b in range(3):
        c1, o1 = fp.plain(opt, b, tables[b][0])
        assert costs[b].tobytes() == c1.tobytes() and out[b].tobytes() == o1.tobytes(), b


# ------------------------------------------------------------------------------------------------ 4. the assignment travels with the call
@pytest.mark.parametrize("task,N,H", [("cartpole", 300, 8), ("leap_cube", 24, 8)])
def test_assignment_redrawn_between_calls(gpu, task, N, H):
    """Two calls on the same buffers with two sets of tables: the second result follows the second tables, and differs from the first."""
    fp = RandomizedProblems(gpu, task, _plants(gpu, task)[:3], 2, 3, N, 4, H, seed=7)
    first, second = [[2, 0, 1], [1, 1, 0]], [[0, 1, 2], [2, 0, 0]]
    got1 = fp.call("mppi", first)
    got2 = fp.call("mppi", second)
    fp.check("mppi", first, got1, what=task)
    fp.check("mppi", second, got2, what=task)
    assert (got1[0] != got2[0]).any(axis=1).all() and (got1[1] != got2[1]).any(axis=1).all()
    assert (fp.tickets() == 0).all()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_randomized_batch_refusals(gpu):
    """Every refusal comes before anything is enqueued: the buffers, the ticket words and the mark stay as they were."""
    import torch

    from judo_amd import _lib
    from judo_amd.device import GpuModel, GpuModelSet

    plants = _plants(gpu, "cartpole")
    fp = RandomizedProblems(gpu, "cartpole", plants[:3], 3, 3, 8, 4, 8, seed=11)
    pr, L = fp.pr, fp.pr.lib
    costs = torch.full((3, 8), -7.0, dtype=torch.float32, device=gpu)
    out = torch.zeros((3, pr.out_stride), dtype=torch.float32, device=gpu)
    fp.mark.numpy().view(np.uint32)[0] = 41
    tables = [[2, 0], [0, 1], [1, 1]]
    base = fp.rargs("mppi", tables, costs.data_ptr(), out.data_ptr(), fp.mark.data_ptr())
    names = ["set", "B", "M", "blk_dev", "blk_host", "blk_bytes", "blk_stride_bytes", "o_nominal", "o_sigma", "o_tp", "o_lohi", "noise", "ldn", "noise_stride_floats", "W", "N", "H", "K",
             "plant_of_block", "G", "costs", "mode", "lambda", "k", "tie_high", "scratch", "out", "out_stride_floats", "out_host_mark", "timing", "stream"]
    assert len(names) == len(base)

    def call(**kw):
        a = list(base)
        for key, v in kw.items():
            a[names.index(key)] = v
        return L.jh_plan_step_randomized_batch(*a)

    for ptr in ("set", "blk_dev", "blk_host", "noise", "W", "plant_of_block", "costs", "scratch", "out"):
        assert call(**{ptr: None}) == -1 and f"{ptr} is a null pointer" in _err(), ptr
    zeros = _table([[0] * 4096])
    assert call(B=257, plant_of_block=zeros) == -1 and "B = 257" in _err() and "JH_MAX_ENSEMBLE_FLEET = 256" in _err()
    assert call(B=0) == -1 and "B = 0" in _err()
    assert call(G=0) == -1 and "G = 0" in _err() and "JH_MAX_PLANT_BLOCKS = 64" in _err()
    assert call(G=65, plant_of_block=zeros) == -1 and "G = 65" in _err()
    assert call(M=0) == -1 and "M = 0" in _err()
    limit = _lib.MAX_FLEET_PLANT_BLOCKS
    B_over = limit // 64 + 1  # with G = 64: the first B whose B * G exceeds the limit
    assert B_over <= _lib.MAX_ENSEMBLE_FLEET
    assert call(B=B_over, G=64, N=64, ldn=64, plant_of_block=zeros) == -1 and f"B * G = {B_over} * 64 = {B_over * 64}" in _err() and f"JH_MAX_FLEET_PLANT_BLOCKS = {limit}" in _err()
    assert call(G=3, plant_of_block=_table([[0, 1, 2]] * 3)) == -1 and "N = 8 is no multiple of G = 3" in _err()
    assert call(plant_of_block=_table([[2, 0], [0, 3], [1, 1]])) == -1 and "plant_of_block[3] = 3" in _err() and "M = 3" in _err() and "controller 1, block 1" in _err()
    assert call(plant_of_block=_table([[2, 0], [0, 1], [255, 1]])) == -1 and "plant_of_block[4] = 255" in _err() and "controller 2, block 0" in _err()
    four = GpuModelSet(list(plants[:4]))
    assert call(set=four.handle) == -1 and "a set of 4 members" in _err() and "M = 3" in _err() and "B * M = 9" in _err()
    four.close()
    big = GpuModelSet([plants[0]] * 33)
    assert call(set=big.handle, M=33) == -1 and "M = 33" in _err() and "JH_MAX_ENSEMBLE = 32" in _err()
    big.close()
    assert call(N=0) == -1 and "N, H, K must be positive" in _err()
    assert call(ldn=7) == -1 and "ldn (7) < N (8)" in _err()
    assert call(K=513) == -1 and "K*nu = 513 exceeds 512" in _err()
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
    assert call(set=one.handle, M=1, plant_of_block=zeros) == -1 and "one launch is forced" in _err()
    one.close()
    leap = GpuModel("leap_cube", gpu)  # JH_ERR_UNSUPPORTED with the single call's text: a set is made of generation 3 alone; a later change of member 0's generation is caught by the call
    held = GpuModelSet([leap])
    leap.set_kernel(2)
    assert call(set=held.handle, M=1, plant_of_block=zeros) == -3 and "only kernel generation 3" in _err()
    held.close()
    # fr3_pick: the call takes its plants as a model set, and no set holds an fr3_pick model -- the refusal a caller meets is the set's, with the status and the name
    fr3 = GpuModel("fr3_pick", gpu)
    handles = (C.c_void_p * 1)(fr3.handle)
    made = C.c_void_p()
    assert L.jh_model_set_create(handles, 1, C.byref(made)) == -3 and "fr3_pick" in _err()
    torch.cuda.synchronize()
    assert (costs.cpu().numpy() == -7.0).all() and (out.cpu().numpy() == 0).all()  # nothing ran
    assert (fp.tickets() == 0).all() and int(fp.mark.numpy().view(np.uint32)[0]) == 41
    assert call() == 0 and L.jh_download_end() == 0
    torch.cuda.synchronize()
    assert (costs.cpu().numpy() != -7.0).all() and int(fp.mark.numpy().view(np.uint32)[0]) == 42 and (fp.tickets() == 0).all()
