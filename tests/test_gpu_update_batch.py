"""jh_spline_controls_batch, jh_update_fused_batch and jh_policy_rollout_batch through the C ABI: B problems in one launch (chain) against B calls of the single entry
on the same sub-blocks.

Every comparison is on bit patterns: the batched kernels run the single calls' statements on pointers offset by the problem's strides, and a Spot rollout's bits depend
neither on its wave-mates nor on the latency mode nor on the policy launch shape (tests/test_gpu_spot.py).  No tolerance appears in this file."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = {"mppi": (0, 0.05, 0, 0), "cem": (1, 0.0, 3, 1), "ps": (1, 0.0, 1, 0)}  # (mode, lambda, k, tie_high) of jh_update_fused
PAD_BLK, PAD_NOISE, PAD_OUT = 3, 8, 5  # the strides are larger than a block / a noise slice / an output record: what lies between must be skipped, not assumed away


def _err():
    from judo_amd import _lib

    return _lib.lib().jh_last_error().decode()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


class Blocks:
    """B packed blocks [x0 (nx) | nominal | sigma | bounds] with NaN between them, and B noise slices with NaN between them."""

    def __init__(self, dev, B, n, K, nu, seed, nx=4):
        import torch

        rng = np.random.default_rng(seed)
        self.B, self.n, self.K, self.nu, self.KU = B, n, K, nu, K * nu
        self.off = [nx, nx + self.KU, nx + 2 * self.KU]  # nominal, sigma, bounds
        self.nblk, self.stride = nx + 2 * self.KU + 2 * nu, nx + 2 * self.KU + 2 * nu + PAD_BLK
        blocks = np.full((B, self.stride), np.nan, dtype=np.float32)
        for b in range(B):
            nominal, sigma = rng.standard_normal(self.KU), 0.05 + rng.random(self.KU)
            lo = -0.8 - rng.random(nu)  # (tight enough that some candidates are clipped)
            blocks[b, : self.nblk] = np.concatenate([rng.standard_normal(nx), nominal, sigma, lo, -lo + 0.1])
        self.blocks = torch.from_numpy(blocks).to(dev)
        self.ldn = n + 3
        self.noise_stride = self.KU * self.ldn + PAD_NOISE
        noise = np.full((B, self.noise_stride), np.nan, dtype=np.float32)
        noise[:, : self.KU * self.ldn] = rng.standard_normal((B, self.KU * self.ldn))
        self.noise = torch.from_numpy(noise).to(dev)

    def blk(self, b):
        return self.blocks.data_ptr() + 4 * b * self.stride

    def nz(self, b):
        return self.noise.data_ptr() + 4 * b * self.noise_stride


# ------------------------------------------------------------------------------------------------ 1. jh_spline_controls_batch
@pytest.mark.parametrize("nu,H", [(3, 7), (10, 7), (3, 5400)])
def test_spline_controls_batch_equals_single_calls(gpu, nu, H):
    """B = 3, n = 5, K = 3; H = 5 400 puts W (H x K floats) past the 64 KiB of LDS staging, so both the single call and the batch take the global-memory form."""
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    B, n, K = 3, 5, 3
    assert (4 * (H * K + 64 * ((K * nu) | 1)) > 64 * 1024) == (H == 5400)
    pb = Blocks(gpu, B, n, K, nu, seed=3 + nu)
    W = torch.from_numpy(np.random.default_rng(1).standard_normal((H, K)).astype(np.float32)).to(gpu)
    got = torch.full((B * n, H, nu), 9.0, dtype=torch.float32, device=gpu)
    st = L.jh_spline_controls_batch(W.data_ptr(), B, pb.blk(0), pb.stride, pb.off[0], pb.off[1], pb.off[2], pb.nz(0), pb.ldn, pb.noise_stride, n, H, K, nu, got.data_ptr(), 0)
    _lib.check(st, "jh_spline_controls_batch")
    want = torch.full((B, n, H, nu), 9.0, dtype=torch.float32, device=gpu)
    for b in range(B):
        p = pb.blk(b)
        st = L.jh_spline_controls(W.data_ptr(), None, p + 4 * pb.off[0], pb.nz(b), pb.ldn, p + 4 * pb.off[1], p + 4 * pb.off[2], n, 0, H, K, nu, want[b].data_ptr(), 0)
        _lib.check(st, "jh_spline_controls")
    torch.cuda.synchronize()
    g, w = got.cpu().numpy().reshape(B, n, H, nu), want.cpu().numpy()
    assert np.isfinite(w).all() and len({w[b].tobytes() for b in range(B)}) == B
    np.testing.assert_array_equal(_bits(g), _bits(w))


def test_spline_controls_batch_refusals(gpu):
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    pb = Blocks(gpu, 2, 5, 3, 3, seed=1)
    W = torch.zeros((7, 3), dtype=torch.float32, device=gpu)
    out = torch.zeros((10, 7, 3), dtype=torch.float32, device=gpu)

    def call(B=2, stride=pb.stride, noise_stride=pb.noise_stride):
        return L.jh_spline_controls_batch(W.data_ptr(), B, pb.blk(0), stride, pb.off[0], pb.off[1], pb.off[2], pb.nz(0), pb.ldn, noise_stride, 5, 7, 3, 3, out.data_ptr(), 0)

    assert call(B=0) == -1 and "B must be" in _err()
    assert call(B=65536) == -1 and "65535" in _err()
    assert call(stride=pb.nblk - 1) == -1 and "blk_stride_floats" in _err()
    assert call(noise_stride=pb.KU * pb.ldn - 1) == -1 and "noise_stride_floats" in _err()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0).all()  # nothing ran


# ------------------------------------------------------------------------------------------------ 2. jh_update_fused_batch
def _update_case(dev, B, n, K, nu, E, seed):
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    pb = Blocks(dev, B, n, K, nu, seed)
    rng = np.random.default_rng(seed + 100)
    costs = rng.standard_normal((B, n)).astype(np.float32)
    costs[:, n // 2] = costs[:, 0]  # a tie
    costs[:, -1] = costs.min(axis=1)  # a tie for the best
    costs[0, 1] = np.nan  # a diverged rollout
    row = 6
    trace = rng.standard_normal((B, n * row)).astype(np.float32)
    per = int(L.jh_update_fused_scratch_floats(n, K, nu))
    assert int(L.jh_plan_batch_scratch_floats(B, n, K, nu)) == B * per
    return dict(L=L, pb=pb, costs=torch.from_numpy(costs).to(dev), trace=torch.from_numpy(trace).to(dev), row=row, E=E, per=per, rec=2 * pb.KU + E * (2 + row),
                scratch=torch.zeros(B * per, dtype=torch.float32, device=dev), mark=torch.zeros(4, dtype=torch.int32).pin_memory())


def _update_batch(c, opt, use_mark, pinned):
    """One jh_update_fused_batch; returns the B records (numpy) after checking that nothing was written between them."""
    import torch

    from judo_amd import _lib

    pb, L = c["pb"], c["L"]
    mode, lam, k, tie = OPTS[opt]
    stride = c["rec"] + PAD_OUT
    out = torch.full((pb.B, stride), 7.0, dtype=torch.float32)
    out = out.pin_memory() if pinned else out.to(c["costs"].device)
    E = c["E"]
    st = L.jh_update_fused_batch(pb.B, c["costs"].data_ptr(), pb.blk(0), pb.stride, pb.off[0], pb.off[1], pb.off[2], pb.nz(0), pb.ldn, pb.noise_stride, pb.n, pb.K, pb.nu, mode, lam, k, tie,
                                 E, c["trace"].data_ptr() if E else None, c["row"] if E else 0, 0, c["scratch"].data_ptr(), out.data_ptr(), stride,
                                 c["mark"].data_ptr() if use_mark else out.data_ptr(), 0)
    _lib.check(st, "jh_update_fused_batch")
    _lib.check(L.jh_download_end(), "jh_download_end")
    o = out.numpy().copy() if pinned else out.cpu().numpy()  # (pinned: read right behind the completion mark, with no other synchronisation)
    torch.cuda.synchronize()
    written = np.ones(c["rec"], dtype=bool)
    if mode == 0:
        written[pb.KU : 2 * pb.KU] = False  # (MPPI has no sigma)
    assert (o[:, c["rec"] :] == 7.0).all() and (o[:, : c["rec"]][:, ~written] == 7.0).all(), "the batch wrote outside its records"
    return o[:, : c["rec"]], written


def _update_single(c, opt, b):
    import torch

    from judo_amd import _lib

    pb, L = c["pb"], c["L"]
    mode, lam, k, tie = OPTS[opt]
    dev = c["costs"].device
    out = torch.full((c["rec"],), 7.0, dtype=torch.float32, device=dev)
    scratch = torch.zeros(c["per"], dtype=torch.float32, device=dev)
    p, o, E, KU = pb.blk(b), out.data_ptr(), c["E"], pb.KU
    st = L.jh_update_fused(c["costs"][b].data_ptr(), None, p + 4 * pb.off[0], pb.nz(b), pb.ldn, p + 4 * pb.off[1], p + 4 * pb.off[2], pb.n, 0, pb.K, pb.nu, mode, lam, k, tie, E,
                           c["trace"][b].data_ptr() if E else None, c["row"] if E else 0, 0, scratch.data_ptr(), o, o + 4 * KU, (o + 8 * KU) if E else None, 0)
    _lib.check(st, "jh_update_fused")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [5, 300])
@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
def test_update_fused_batch_equals_single_calls(gpu, opt, n):
    """B = 3, K = 3, nu = 3, E = 2 trace records; n = 300 is two workgroups per problem, the second ragged.  Costs with a NaN and ties.  Run twice on one scratch, once per
    completion convention: into device-visible pinned host memory behind the polled word (garbage beforehand: it holds its old value + 1), then behind the stream's event."""
    c = _update_case(gpu, 3, n, 3, 3, 2, seed=7 + n)
    old = 0xDEADBEEF
    c["mark"].numpy().view(np.uint32)[0] = old
    first, written = _update_batch(c, opt, use_mark=True, pinned=True)
    assert int(c["mark"].numpy().view(np.uint32)[0]) == (old + 1) & 0xFFFFFFFF
    tickets = c["scratch"].cpu().numpy().view(np.uint32).reshape(3, -1)[:, :4]
    assert (tickets == 0).all()  # every problem's ticket and the batch's are back at zero
    for b in range(3):
        want = _update_single(c, opt, b)
        np.testing.assert_array_equal(_bits(first[b][written]), _bits(want[written]), err_msg=f"{opt} n={n} problem {b}")
    assert len({first[b].tobytes() for b in range(3)}) == 3
    second, _ = _update_batch(c, opt, use_mark=False, pinned=True)
    assert first.tobytes() == second.tobytes()
    assert (c["scratch"].cpu().numpy().view(np.uint32).reshape(3, -1)[:, :4] == 0).all()
    third, _ = _update_batch(c, opt, use_mark=False, pinned=False)  # (device memory as the output block)
    assert first.tobytes() == third.tobytes()


@pytest.mark.parametrize("opt", ["mppi", "cem", "ps"])
def test_update_fused_batch_of_one_without_traces(gpu, opt):
    """B = 1, and trace NULL with E > 0: E is ignored (the Spot case: its traces come from the materialised sensors), the record is nominal | sigma alone."""
    c = _update_case(gpu, 1, 5, 3, 10, 0, seed=2)
    import torch

    from judo_amd import _lib

    pb, L = c["pb"], c["L"]
    mode, lam, k, tie = OPTS[opt]
    out = torch.full((2 * pb.KU + PAD_OUT,), 7.0, dtype=torch.float32, device=gpu)
    st = L.jh_update_fused_batch(1, c["costs"].data_ptr(), pb.blk(0), pb.stride, pb.off[0], pb.off[1], pb.off[2], pb.nz(0), pb.ldn, pb.noise_stride, pb.n, pb.K, pb.nu, mode, lam, k, tie, 4, None,
                                 0, 0, c["scratch"].data_ptr(), out.data_ptr(), 2 * pb.KU, out.data_ptr(), 0)
    _lib.check(st, "jh_update_fused_batch")
    _lib.check(L.jh_download_end(), "jh_download_end")
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), _update_single(c, opt, 0)
    n_res = pb.KU if mode == 0 else 2 * pb.KU
    np.testing.assert_array_equal(_bits(got[:n_res]), _bits(want[:n_res]))
    assert (got[n_res:] == 7.0).all() and np.isfinite(got[:n_res]).all()


def test_update_fused_batch_refusals(gpu):
    import torch

    c = _update_case(gpu, 2, 5, 3, 3, 2, seed=1)
    pb, L = c["pb"], c["L"]
    out = torch.zeros((2, c["rec"]), dtype=torch.float32, device=gpu)

    def call(B=2, stride=pb.stride, noise_stride=pb.noise_stride, out_stride=c["rec"]):
        return L.jh_update_fused_batch(B, c["costs"].data_ptr(), pb.blk(0), stride, pb.off[0], pb.off[1], pb.off[2], pb.nz(0), pb.ldn, noise_stride, pb.n, pb.K, pb.nu, 0, 0.05, 0, 0, 2,
                                       c["trace"].data_ptr(), c["row"], 0, c["scratch"].data_ptr(), out.data_ptr(), out_stride, out.data_ptr(), 0)

    assert call(B=0) == -1 and "B must be" in _err()
    assert call(B=65536) == -1 and "65535" in _err()
    assert call(stride=pb.nblk - 1) == -1 and "blk_stride_floats" in _err()
    assert call(noise_stride=pb.KU * pb.ldn - 1) == -1 and "noise_stride_floats" in _err()
    assert call(out_stride=c["rec"] - 1) == -1 and "out_stride_floats" in _err()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0).all()  # nothing ran, and no completion mark is pending
    assert L.jh_download_end() != 0


# ------------------------------------------------------------------------------------------------ 3. jh_policy_rollout_batch
PAD_X0 = 5


@pytest.fixture(scope="module")
def plant(gpu):
    """(engine, policy) per model image, made once: "spot" (the robot alone) and "spot_box" (with the free box)."""
    from judo_amd.models import load_description
    from judo_amd.policy import SpotLocomotionPolicy, SpotTreeEngine

    policy = SpotLocomotionPolicy(device=gpu)
    return {name: (SpotTreeEngine(load_description(name), gpu), policy) for name in ("spot", "spot_box")}


def _start_states(name, B, seed):
    """B distinct standing states: other leg angles, base positions and (spot_box) box positions."""
    from judo_amd.spot_tasks import SpotBoxPush, SpotNavigate

    rng = np.random.default_rng(seed)
    if name == "spot_box":
        x = SpotBoxPush().default_state()
    else:
        task = SpotNavigate()
        x = np.concatenate([task.reset_pose, np.zeros(task.nv)])
    X = np.tile(x, (B, 1))
    X[:, 7:19] += 0.05 * rng.standard_normal((B, 12))
    X[:, :2] += 0.1 * rng.standard_normal((B, 2))
    if name == "spot_box":
        X[:, 26:28] += 0.2 * rng.standard_normal((B, 2))
    return X.astype(np.float32)


def _rollout_inputs(dev, eng, name, B, n, T, seed):
    import torch

    from judo_amd.spot_tasks import SpotNavigate

    rng = np.random.default_rng(seed)
    nx = eng.nq + eng.nv
    x0 = np.full((B, nx + PAD_X0), np.nan, dtype=np.float32)  # (NaN between the states)
    x0[:, :nx] = _start_states(name, B, seed)
    cmds = np.tile(SpotNavigate().default_policy_command, (B * n, T, 1)).astype(np.float32)
    cmds[:, :, :3] = rng.uniform(-0.5, 0.5, (B * n, 1, 3))
    out0 = (0.3 * rng.standard_normal((B * n, 12))).astype(np.float32)   # non-zero incoming policy outputs
    warm0 = (0.5 * rng.standard_normal((B * n, eng.nv))).astype(np.float32)  # and warm start
    return tuple(torch.from_numpy(a).to(dev) for a in (x0, cmds, out0, warm0))


def _rollout(L, eng, policy, x0_ptr, B, x0_stride, cmds, out0, warm0, reset_warm, n, T, single):
    """jh_policy_rollout_batch over B problems, or (single) jh_policy_rollout on one problem's rows; returns (states, sensors, policy_out, warm) as numpy."""
    import torch

    from judo_amd import _lib

    N, nx, dev = int(cmds.shape[0]), eng.nq + eng.nv, cmds.device
    states = torch.full((N, T, nx), 9.0, dtype=torch.float32, device=dev)
    sensors = torch.full((N, T, eng.nsensordata), 9.0, dtype=torch.float32, device=dev)
    out, warm = out0.clone(), warm0.clone()
    scratch = torch.empty(int(L.jh_policy_rollout_scratch_floats(N)), dtype=torch.float32, device=dev)
    done = C.c_int(0)
    if single:
        st = L.jh_policy_rollout(policy.handle, eng.handle, x0_ptr, 0, cmds.data_ptr(), out.data_ptr(), warm.data_ptr(), int(reset_warm), N, T, 2, -1.0, states.data_ptr(), sensors.data_ptr(),
                                 scratch.data_ptr(), C.byref(done), 0)
        _lib.check(st, "jh_policy_rollout")
    else:
        st = L.jh_policy_rollout_batch(policy.handle, eng.handle, B, x0_ptr, x0_stride, cmds.data_ptr(), out.data_ptr(), warm.data_ptr(), int(reset_warm), n, T, 2, -1.0, states.data_ptr(),
                                       sensors.data_ptr(), scratch.data_ptr(), C.byref(done), 0)
        _lib.check(st, "jh_policy_rollout_batch")
    torch.cuda.synchronize()
    assert done.value == T
    return tuple(a.cpu().numpy() for a in (states, sensors, out, warm))


def _compare_rollouts(L, eng, policy, inputs, B, n, T, reset_warm, which, what):
    x0, cmds, out0, warm0 = inputs
    stride = int(x0.shape[1])
    got = _rollout(L, eng, policy, x0.data_ptr(), B, stride, cmds, out0, warm0, reset_warm, n, T, single=False)
    assert all(np.isfinite(a).all() for a in got)
    for b in which:
        r = slice(b * n, (b + 1) * n)
        want = _rollout(L, eng, policy, x0.data_ptr() + 4 * b * stride, 1, stride, cmds[r].contiguous(), out0[r].contiguous(), warm0[r].contiguous(), reset_warm, n, T, single=True)
        for name, g, w in zip(("states", "sensors", "policy outputs", "warm start"), got, want):
            np.testing.assert_array_equal(_bits(g[r]), _bits(w), err_msg=f"{what} problem {b}: {name}")
    return got


@pytest.mark.parametrize("reset_warm", [0, 1])
@pytest.mark.parametrize("latency", ["auto", "off"])
@pytest.mark.parametrize("name", ["spot", "spot_box"])
def test_policy_rollout_batch_equals_single_calls(gpu, plant, monkeypatch, name, latency, reset_warm):
    """B = 3, n = 5, T = 3, distinct states, non-zero incoming policy outputs and warm start.  n is odd: with the latency mode off a wave holds two rollouts, so one wave
    holds the last rollout of a problem and the first of the next one."""
    from judo_amd import _lib

    if latency == "off":
        monkeypatch.setenv("JUDO_AMD_LATENCY_SHIFT", "0")
    else:
        monkeypatch.delenv("JUDO_AMD_LATENCY_SHIFT", raising=False)
    eng, policy = plant[name]
    B, n, T = 3, 5, 3
    inputs = _rollout_inputs(gpu, eng, name, B, n, T, seed=11)
    states, _, outs, _ = _compare_rollouts(_lib.lib(), eng, policy, inputs, B, n, T, reset_warm, range(B), f"{name} latency={latency} reset_warmstart={reset_warm}")
    assert len({states[b * n : (b + 1) * n, 0, :7].tobytes() for b in range(B)}) == B  # the problems started from different states
    assert (outs != inputs[2].cpu().numpy()).any()


def test_policy_rollout_batch_across_policy_launch_shapes(gpu, plant, monkeypatch):
    """B * n = 22 * 24 = 528 > 512 rollouts: the batch's policy step is the four per-layer launches, a single call of 24 the workgroup-per-rollout launch.  T = 2; three problems compared."""
    from judo_amd import _lib

    monkeypatch.delenv("JUDO_AMD_LATENCY_SHIFT", raising=False)
    monkeypatch.delenv("JUDO_AMD_POLICY_ROWS_MAX", raising=False)
    eng, policy = plant["spot"]
    B, n, T = 22, 24, 2
    inputs = _rollout_inputs(gpu, eng, "spot", B, n, T, seed=13)
    _compare_rollouts(_lib.lib(), eng, policy, inputs, B, n, T, 0, (0, 10, 21), "spot B*n=528")


@pytest.mark.parametrize("name", ["spot", "spot_box"])
def test_policy_rollout_batch_with_one_command_row(gpu, plant, monkeypatch, name):
    """T = 1: the start states are expanded into row 0 of `states`, which the one control step reads and writes in place."""
    from judo_amd import _lib

    monkeypatch.delenv("JUDO_AMD_LATENCY_SHIFT", raising=False)
    eng, policy = plant[name]
    inputs = _rollout_inputs(gpu, eng, name, 3, 5, 1, seed=17)
    _compare_rollouts(_lib.lib(), eng, policy, inputs, 3, 5, 1, 0, range(3), f"{name} T=1")


def test_policy_rollout_batch_refusals(gpu, plant):
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    eng, policy = plant["spot"]
    x0, cmds, out0, warm0 = _rollout_inputs(gpu, eng, "spot", 2, 5, 2, seed=1)
    nx = eng.nq + eng.nv
    states = torch.zeros((10, 2, nx), dtype=torch.float32, device=gpu)
    scratch = torch.empty(int(L.jh_policy_rollout_scratch_floats(10)), dtype=torch.float32, device=gpu)

    def call(B=2, n=5, stride=int(x0.shape[1])):
        return L.jh_policy_rollout_batch(policy.handle, eng.handle, B, x0.data_ptr(), stride, cmds.data_ptr(), out0.data_ptr(), warm0.data_ptr(), 0, n, 2, 2, -1.0, states.data_ptr(), None,
                                         scratch.data_ptr(), None, 0)

    assert call(B=0) == -1 and "at least one problem" in _err()
    assert call(n=0) == -1 and "at least one problem" in _err()
    assert call(stride=nx - 1) == -1 and "x0_stride_floats" in _err()
    torch.cuda.synchronize()
    assert (states.cpu().numpy() == 0).all()  # nothing ran
