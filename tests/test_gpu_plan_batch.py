"""jh_plan_step_batch and jh_noise_normal_batch through the C ABI: B plan steps in one launch against B calls of jh_plan_step on the same sub-blocks.

Every comparison is bit for bit: the batched kernels run the single call's code on pointers offset by the problem's strides, and the single path is the one held
to the oracle (tests/test_gpu_simple.py, test_gpu_leap.py, test_gpu_plan_edges.py).  No tolerance appears in this file."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = {"mppi": (0, 0.05, 0, 0), "cem": (1, 0.0, 5, 1), "ps": (1, 0.0, 1, 0)}  # (mode, lambda, k, tie_high) of jh_update_fused
PAD_BLK, PAD_NOISE, PAD_OUT = 3, 8, 5  # the strides are larger than a block / a noise slice / an output record: what lies between must be skipped, not assumed away


def _err():
    from judo_amd import _lib

    return _lib.lib().jh_last_error().decode()


class Problems:
    """B problems of one model with distinct x0, nominal, sigma, task parameters and noise, laid out for jh_plan_step_batch; `single(b)` runs jh_plan_step on
    problem b's sub-block with buffers of its own."""

    def __init__(self, dev, task_name, B, N, K, H, E, seed, x0s=None, tps=None, model=None):
        import torch

        from judo_amd import _lib
        from judo_amd.device import GpuModel
        from judo_amd.spline import spline_weights
        from judo_amd.tasks import get_registered_tasks

        self.lib, self.dev, self.B, self.N, self.K, self.H, self.E = _lib.lib(), dev, B, N, K, H, E
        task = get_registered_tasks()[task_name][0]()
        self.model = model if model is not None else GpuModel(task_name, dev)
        nu, nx = task.nu, task.nq + task.nv
        self.nu, self.KU = nu, K * nu
        rng = np.random.default_rng(seed)
        tp0 = np.asarray(task.task_params({}), dtype=np.float32)
        self.sizes = [nx, self.KU, self.KU, len(tp0), 2 * nu]
        self.off = [int(v) for v in np.cumsum([0] + self.sizes)]
        self.nblk, self.blk_stride = self.off[-1], self.off[-1] + PAD_BLK
        r = task.actuator_ctrlrange
        lohi = np.nan_to_num(np.concatenate([r[:, 0], r[:, 1]]).astype(np.float32), posinf=3.0e38, neginf=-3.0e38)
        blocks = np.full((B, self.blk_stride), np.nan, dtype=np.float32)  # (NaN between the blocks: a kernel that reads past a block's end shows)
        for b in range(B):
            x0 = np.asarray(x0s[b] if x0s is not None else task.default_state() + 0.05 * rng.standard_normal(nx), dtype=np.float32)
            warm = np.tile(np.asarray(task.optimizer_warm_start(), dtype=np.float64), (K, 1))
            nominal = (warm + 0.1 * rng.standard_normal((K, nu))).astype(np.float32).reshape(-1)
            sigma = (0.05 + 0.2 * rng.random((K, nu))).astype(np.float32).reshape(-1)
            tp = np.asarray(tps[b], dtype=np.float32) if tps is not None else tp0 * (1.0 + 0.2 * rng.random(len(tp0))).astype(np.float32)
            blocks[b, : self.nblk] = np.concatenate([x0, nominal, sigma, tp, lohi])
        self.blocks = torch.from_numpy(blocks).to(dev)
        self.ldn = N + 4
        self.noise_stride = self.KU * self.ldn + PAD_NOISE
        noise = rng.standard_normal((B, self.noise_stride)).astype(np.float32)
        self.noise = torch.from_numpy(noise).to(dev)
        dt = task.dt
        self.W = torch.from_numpy(spline_weights("linear", np.linspace(0, H * dt, K), dt * np.arange(H)).astype(np.float32)).to(dev)
        adr, nfl, cm = self.model.trace_layout()
        assert nfl > 0
        self.row, self.colmajor = H * nfl, int(cm)
        self.rec = 2 * self.KU + E * (2 + self.row)
        self.out_stride = self.rec + PAD_OUT
        self.per_scratch = int(self.lib.jh_update_fused_scratch_floats(N, K, nu))
        assert int(self.lib.jh_plan_batch_scratch_floats(B, N, K, nu)) == B * self.per_scratch
        self.batch_scratch = torch.zeros(B * self.per_scratch, dtype=torch.float32, device=dev)
        self.mark = torch.zeros(4, dtype=torch.int32).pin_memory()

    def batch(self, opt, use_mark=False, B=None):
        """One jh_plan_step_batch over the first B problems; returns (costs (B, N), out (B, rec)) as numpy."""
        import torch

        from judo_amd import _lib

        B = self.B if B is None else B
        mode, lam, k, tie = OPTS[opt]
        costs = torch.full((B, self.N), -7.0, dtype=torch.float32, device=self.dev)
        trace = torch.zeros(B * self.N * self.row, dtype=torch.float32, device=self.dev)
        out = torch.zeros((B, self.out_stride), dtype=torch.float32, device=self.dev)
        p = self.blocks.data_ptr()
        st = self.lib.jh_plan_step_batch(self.model.handle, B, p, p, 4 * self.nblk, 4 * self.blk_stride, self.off[1], self.off[2], self.off[3], self.off[4], self.noise.data_ptr(), self.ldn,
                                         self.noise_stride, self.W.data_ptr(), self.N, self.H, self.K, costs.data_ptr(), trace.data_ptr(), mode, lam, k, tie, self.E, self.row, self.colmajor,
                                         self.batch_scratch.data_ptr(), out.data_ptr(), self.out_stride, self.mark.data_ptr() if use_mark else out.data_ptr(), None, 0)
        _lib.check(st, "jh_plan_step_batch")
        _lib.check(self.lib.jh_download_end(), "jh_download_end")
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[:, self.rec :] == 0).all(), "the batch wrote between the output records"
        return costs.cpu().numpy(), o[:, : self.rec].copy()

    def single(self, opt, b):
        import torch

        from judo_amd import _lib

        mode, lam, k, tie = OPTS[opt]
        costs = torch.full((self.N,), -7.0, dtype=torch.float32, device=self.dev)
        trace = torch.zeros(self.N * self.row, dtype=torch.float32, device=self.dev)
        out = torch.zeros(self.rec, dtype=torch.float32, device=self.dev)
        scratch = torch.zeros(self.per_scratch, dtype=torch.float32, device=self.dev)
        p = self.blocks.data_ptr() + 4 * b * self.blk_stride
        st = self.lib.jh_plan_step(self.model.handle, p, p, 4 * self.nblk, self.off[1], self.off[2], self.off[3], self.off[4], self.noise.data_ptr() + 4 * b * self.noise_stride, self.ldn,
                                   self.W.data_ptr(), 0, self.N, 0, self.H, self.K, costs.data_ptr(), None, trace.data_ptr(), mode, lam, k, tie, self.E, self.row, self.colmajor,
                                   scratch.data_ptr(), out.data_ptr(), out.data_ptr(), None, 0)
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
                np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"{what} {opt} problem {b}: {name}")


# ------------------------------------------------------------------------------------------------ 1. closed-form models
@pytest.mark.parametrize("launches", [1, 2])
@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
@pytest.mark.parametrize("task", ["cartpole", "cylinder_push"])
def test_closed_form_batch_equals_single_calls(gpu, task, opt, launches):
    """B = 3, N = 300 (two workgroups of the one-launch form, the second ragged), K = 4, H = 16, E = 3: costs, nominal, sigma and trace records of the batch are those
    of three jh_plan_step calls, as one launch and as two; a second batch on the same scratch gives the same bytes (the tickets were reset); the completion word,
    garbage beforehand, holds its old value + 1."""
    pr = Problems(gpu, task, 3, 300, 4, 16, 3, seed=11)
    pr.model.set_plan_step_launches(launches)
    pr.model.stats(reset=True)
    old = 0xDEADBEEF
    pr.mark.numpy().view(np.uint32)[0] = old
    first = pr.batch(opt, use_mark=True)
    assert int(pr.mark.numpy().view(np.uint32)[0]) == (old + 1) & 0xFFFFFFFF
    assert pr.model.stats(reset=True)["one_launch_plan_steps"] == (1 if launches == 1 else 0)
    pr.check(opt, first, what=f"{task} launches={launches}")
    second = pr.batch(opt, use_mark=True)
    assert int(pr.mark.numpy().view(np.uint32)[0]) == (old + 2) & 0xFFFFFFFF
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()
    assert (pr.batch_scratch.cpu().numpy().view(np.uint32).reshape(3, -1)[:, :4] == 0).all()  # every problem's ticket and the batch's are back at zero


# ------------------------------------------------------------------------------------------------ 2. edges
@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
def test_batch_of_one_equals_plan_step(gpu, opt):
    pr = Problems(gpu, "cartpole", 1, 300, 4, 16, 3, seed=5)
    pr.check(opt, pr.batch(opt), what="cartpole B=1")


def test_fewer_rollouts_than_trace_elites(gpu):
    """N = 2 with E = 3: the third trace record of every problem is empty as documented (cost +inf, index -1, zero row)."""
    pr = Problems(gpu, "cartpole", 3, 2, 4, 16, 3, seed=6)
    costs, out = got = pr.batch("mppi")
    pr.check("mppi", got, what="cartpole N=2 E=3")
    recs = out[:, 2 * pr.KU :].reshape(3, 3, 2 + pr.row)
    assert np.isposinf(recs[:, 2, 0]).all() and (recs[:, 2, 1].view(np.int32) == -1).all() and (recs[:, 2, 2:] == 0).all()
    assert (recs[:, :2, 1].view(np.int32) >= 0).all()


@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
def test_five_problems_of_one_rollout(gpu, opt):
    pr = Problems(gpu, "cylinder_push", 5, 1, 4, 16, 1, seed=7)
    pr.check(opt, pr.batch(opt), what="cylinder_push B=5 N=1")


# ------------------------------------------------------------------------------------------------ 3. noise
def test_noise_batch_equals_single_draws(gpu):
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    B, rows, n_local, ldn = 3, 8, 301, 320
    seeds, draws = [1234, 0xFEDCBA9876543210, 7], [0, 41, 0xFFFFFFFF]
    got = torch.full((B, rows, ldn), 9.0, dtype=torch.float32, device=gpu)
    _lib.check(L.jh_noise_normal_batch(B, (C.c_ulonglong * B)(*seeds), (C.c_uint * B)(*draws), rows, n_local, got.data_ptr(), ldn, 0), "jh_noise_normal_batch")
    want = torch.full((B, rows, ldn), 9.0, dtype=torch.float32, device=gpu)
    for b in range(B):
        _lib.check(L.jh_noise_normal(seeds[b], draws[b], rows, 0, n_local, want[b].data_ptr(), ldn, 0), "jh_noise_normal")
    torch.cuda.synchronize()
    g, w = got.cpu().numpy(), want.cpu().numpy()
    np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32))
    assert (g[:, :, n_local:] == 9.0).all()  # the padding columns are untouched
    assert np.isfinite(g[:, :, :n_local]).all() and len({g[b, :, :n_local].tobytes() for b in range(B)}) == B
    assert L.jh_noise_normal_batch(0, (C.c_ulonglong * 1)(1), (C.c_uint * 1)(0), rows, n_local, got.data_ptr(), ldn, 0) == -1 and _err()


# ------------------------------------------------------------------------------------------------ 4. - 6. the leap family
def _leap_states(task_name, B, seed):
    """Per problem: the cube displaced differently and another goal quaternion; the last problem has the cube pushed down into half-closed fingers, where the hand's
    own contacts (finger against finger, finger against palm) are live next to the cube's."""
    from judo_amd.tasks import get_registered_tasks

    task = get_registered_tasks()[task_name][0]()
    rng = np.random.default_rng(seed)
    x0s, tps = [], []
    for b in range(B):
        x = task.default_state().copy()
        x[:3] += 0.01 * rng.standard_normal(3)
        if b == B - 1:
            x[2] -= 0.015
            x[7:23] += 0.25
        q = rng.standard_normal(4)
        tp = np.asarray(task.task_params({"goal_quat": q / np.linalg.norm(q)}), dtype=np.float32)
        x0s.append(x)
        tps.append(tp)
    return x0s, tps


def test_leap_batch_in_latency_mode(gpu):
    """leap_cube, B = 3, N = 6 (two groups of four rollouts, the second ragged), H = 8, K = 4, E = 2: B * N = 18 rollouts select the latency mode, as each single call does."""
    x0s, tps = _leap_states("leap_cube", 3, 21)
    pr = Problems(gpu, "leap_cube", 3, 6, 4, 8, 2, seed=22, x0s=x0s, tps=tps)
    got = pr.batch("mppi")
    assert len({got[0][b].tobytes() for b in range(3)}) == 3  # the problems are different problems
    pr.check("mppi", got, what="leap_cube latency mode")
    pr.check("cem", pr.batch("cem"), what="leap_cube latency mode")


def test_leap_batch_outside_latency_mode(gpu):
    """B = 9, N = 256, H = 4: 2 304 rollouts in the launch, every row of a wave its own rollout, while a single call of 256 still runs the latency mode; four sampled problems."""
    x0s, tps = _leap_states("leap_cube", 9, 31)
    pr = Problems(gpu, "leap_cube", 9, 256, 4, 4, 2, seed=32, x0s=x0s, tps=tps)
    pr.check("mppi", pr.batch("mppi"), which=(0, 3, 5, 8), what="leap_cube B*N=2304")


def test_leap_cube_down_batch_on_the_64_contact_build(gpu):
    """leap_cube_down runs the 64-contact build, whose contacts above the LDS pool live in one row of global memory per rollout: a problem's rows lie N behind the one before's."""
    x0s, tps = _leap_states("leap_cube_down", 2, 41)
    pr = Problems(gpu, "leap_cube_down", 2, 6, 4, 8, 2, seed=42, x0s=x0s, tps=tps)
    assert pr.model.build()["contact_capacity"] == 64
    pr.model.stats(reset=True)
    got = pr.batch("mppi")
    assert pr.model.stats(reset=True)["overflow_pool_fallbacks"] == 0
    pr.check("mppi", got, what="leap_cube_down")


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_batch_refusals(gpu):
    import torch

    from judo_amd.device import GpuModel

    pr = Problems(gpu, "cartpole", 2, 8, 4, 16, 1, seed=1)
    L, p = pr.lib, pr.blocks.data_ptr()
    costs = torch.zeros((2, 8), dtype=torch.float32, device=gpu)
    trace = torch.zeros(2 * 8 * pr.row, dtype=torch.float32, device=gpu)
    out = torch.zeros((2, pr.out_stride), dtype=torch.float32, device=gpu)

    def call(model=pr.model, B=2, blk_stride=4 * pr.blk_stride, out_stride=pr.out_stride):
        return L.jh_plan_step_batch(model.handle, B, p, p, 4 * pr.nblk, blk_stride, pr.off[1], pr.off[2], pr.off[3], pr.off[4], pr.noise.data_ptr(), pr.ldn, pr.noise_stride, pr.W.data_ptr(),
                                    8, 16, 4, costs.data_ptr(), trace.data_ptr(), 0, 0.05, 0, 0, 1, pr.row, pr.colmajor, pr.batch_scratch.data_ptr(), out.data_ptr(), out_stride, out.data_ptr(),
                                    None, 0)

    assert call(model=GpuModel("fr3_pick", gpu)) == -3 and "fr3_pick" in _err()
    assert call(blk_stride=4 * pr.nblk - 4) == -1 and "blk_stride_bytes" in _err()
    assert call(out_stride=pr.rec - 1) == -1 and "out_stride_floats" in _err()
    assert call(B=0) == -1 and "B must be" in _err()
    assert call(B=65536) == -1 and "65535" in _err()
    pr.model.set_plan_step_launches(1)
    pr.K = K = pr.model.one_launch_max_knots_at(16) + 1  # a forced one-launch plan step that does not fit (the arguments are checked before any pointer is followed)
    assert L.jh_plan_step_batch(pr.model.handle, 2, p, p, 4 * (4 + 2 * K + 6 + 2), 4 * (4 + 2 * K + 6 + 2), 4, 4 + K, 4 + 2 * K, 4 + 2 * K + 6, pr.noise.data_ptr(), 8, K * 8, pr.W.data_ptr(),
                                8, 16, K, costs.data_ptr(), None, 0, 0.05, 0, 0, 0, 0, 0, pr.batch_scratch.data_ptr(), out.data_ptr(), 2 * K, out.data_ptr(), None, 0) == -1
    assert "one launch is forced" in _err()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0).all()  # nothing ran
