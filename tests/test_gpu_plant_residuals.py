"""jh_plant_residuals through the C ABI: the weighted squared prediction error of M plants on W recorded windows, bit for bit against its numpy restatement
(judo_amd.identify.plant_residuals_host), at the smallest shapes at which the kernel can go wrong; and its refusals.

`err` is a poisoned buffer with ld > W: a write outside row m's W entries shows.  No tolerance appears in this file."""

import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_plan_batch import _err

pytestmark = pytest.mark.gpu

POISON = -7.0
# (M, W, H, nx, nq, quaternion offsets)
CASES = {
    "no_quaternion": (3, 5, 3, 4, 2, ()),  # the plain path
    "leap_sized_row": (2, 3, 7, 45, 23, (3,)),  # H no power of two; one quaternion at offset 3; one observed row sign-flipped
    "single_item": (1, 1, 1, 4, 2, ()),  # one wave, one live lane
    "full_wave": (2, 3, 64, 6, 6, ()),  # every lane live
    "many_windows": (3, 65, 3, 4, 2, ()),  # 195 (m, w) pairs: more than one workgroup holds, whatever its size (at most 1024 threads: 16 waves)
    "four_quaternions": (2, 2, 5, 19, 17, (0, 4, 9, 13)),  # JH_MAX_ID_QUATS of them, the last ending at nq
}


def _inputs(M, W, H, nx, nq, quats, seed):
    """(pred (M * W, H, nx), obs (W, H, nx), weight (nx)) in fp32: predictions around the observations, unit quaternions at the offsets -- plant 0's near the observed
    one, the last plant's near its antipode."""
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((W, H, nx))
    pred = obs[None] + 0.3 * rng.standard_normal((M, W, H, nx))
    for a in quats:
        q = rng.standard_normal((W, H, 4))
        obs[..., a : a + 4] = q / np.linalg.norm(q, axis=-1, keepdims=True)
        sign = np.ones((M, 1, 1, 1))
        sign[-1] = -1.0
        p = sign * obs[None, ..., a : a + 4] + 0.05 * rng.standard_normal((M, W, H, 4))
        pred[..., a : a + 4] = p / np.linalg.norm(p, axis=-1, keepdims=True)
    return pred.reshape(M * W, H, nx).astype(np.float32), obs.astype(np.float32), rng.uniform(0.25, 4.0, nx).astype(np.float32)


def _call(gpu, pred, obs, weight, quats, M, W, H, nx, nq, ld):
    """The raw entry on host arrays: (M, ld) fp32, poisoned beforehand."""
    import torch

    from judo_amd import _lib

    d = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (pred, obs, weight)]
    err = torch.full((M, ld), POISON, dtype=torch.float32, device=gpu)
    arr = (C.c_int * len(quats))(*quats) if quats else None
    _lib.check(_lib.lib().jh_plant_residuals(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), arr, len(quats), M, W, H, nx, nq, err.data_ptr(), ld, 0), "jh_plant_residuals")
    torch.cuda.synchronize()
    for t, a in zip(d, (pred, obs, weight)):
        assert t.cpu().numpy().tobytes() == a.tobytes()  # the inputs are read only
    return err.cpu().numpy()


@pytest.mark.parametrize("case", list(CASES))
def test_residuals_equal_the_numpy_restatement(gpu, case):
    from judo_amd.identify import plant_residuals_host

    M, W, H, nx, nq, quats = CASES[case]
    pred, obs, weight = _inputs(M, W, H, nx, nq, quats, seed=len(case) + 7 * M + W)
    ld = W + 3
    got = _call(gpu, pred, obs, weight, quats, M, W, H, nx, nq, ld)
    want = plant_residuals_host(pred, obs, weight, quats, nq=nq)
    np.testing.assert_array_equal(got[:, :W].view(np.uint32), want.view(np.uint32), err_msg=case)
    assert (got[:, W:] == POISON).all(), "the floats between W and ld were written"
    assert np.isfinite(want).all() and (want > 0).all()
    if quats:
        # the antipodal plant was aligned: unaligned, |p + o|^2 is near 4 per quaternion and step, at a weight of 0.25 or more
        assert (plant_residuals_host(pred, obs, weight, (), nq=nq)[-1] - want[-1] > 0.5 * H).all()
        # one observed row sign-flipped: the same pose, the same bits
        flipped = obs.copy()
        a = quats[0]
        flipped[W - 1, H // 2, a : a + 4] *= -1
        again = _call(gpu, pred, flipped, weight, quats, M, W, H, nx, nq, ld)
        np.testing.assert_array_equal(again.view(np.uint32), got.view(np.uint32), err_msg=f"{case}: a sign-flipped observed quaternion")


def test_exact_zeros_and_nan(gpu):
    """pred == obs and an antipodal quaternion give exactly 0.0; NaN in gives NaN out, in that (plant, window) alone."""
    rng = np.random.default_rng(3)
    M, W, H, nx, nq, quats = 3, 2, 7, 13, 7, (3,)
    _, obs, weight = _inputs(1, W, H, nx, nq, quats, seed=11)
    pred = np.tile(obs, (M, 1, 1))
    pred[W : 2 * W, :, 3:7] *= -1  # plant 1: the antipodal quaternions
    pred[2 * W + 1, H - 1, rng.integers(nx)] = np.nan  # plant 2, window 1
    got = _call(gpu, pred, obs, weight, quats, M, W, H, nx, nq, W)
    assert np.array_equal(got[:2], np.zeros((2, W), dtype=np.float32)) and not np.signbit(got[:2]).any()
    assert got[2, 0] == 0.0 and np.isnan(got[2, 1])


def test_residuals_refusals(gpu):
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    M, W, H, nx, nq = 3, 4, 5, 9, 7
    pred = torch.ones((33 * W, H, nx), dtype=torch.float32, device=gpu)
    obs = torch.ones((W, H, nx), dtype=torch.float32, device=gpu)
    weight = torch.ones(nx, dtype=torch.float32, device=gpu)
    err = torch.full((33, W + 2), POISON, dtype=torch.float32, device=gpu)

    def call(quats=(3,), nquat=None, null_quats=False, **kw):
        a = {**dict(pred=pred.data_ptr(), obs=obs.data_ptr(), weight=weight.data_ptr(), M=M, W=W, H=H, nx=nx, nq=nq, err=err.data_ptr(), ld=W + 2), **kw}
        arr = None if null_quats else (C.c_int * max(len(quats), 1))(*quats)
        return L.jh_plant_residuals(a["pred"], a["obs"], a["weight"], arr, len(quats) if nquat is None else nquat, a["M"], a["W"], a["H"], a["nx"], a["nq"], a["err"], a["ld"], 0)

    cases = [
        (dict(pred=None), "pred is a null pointer"),
        (dict(obs=None), "obs is a null pointer"),
        (dict(weight=None), "weight is a null pointer"),
        (dict(err=None), "err is a null pointer"),
        (dict(M=0), "M = 0"),
        (dict(M=33), "M = 33"),
        (dict(W=0), "W = 0"),
        (dict(H=0), "H = 0"),
        (dict(H=65), "H = 65"),
        (dict(nx=0, nq=0, quats=()), "nx = 0"),
        (dict(nq=-1), "nq = -1"),
        (dict(nq=10), "nq = 10"),
        (dict(ld=3), "ld (3) < W (4)"),
        (dict(nquat=-1), "nquat = -1"),
        (dict(quats=(0, 0, 0, 0, 0)), "nquat = 5"),
        (dict(null_quats=True, nquat=1), "quat_adr is a null pointer"),
        (dict(quats=(-1,)), "quat_adr[0] = -1"),
        (dict(quats=(4,)), "quat_adr[0] = 4"),  # reaches past nq = 7 with its fourth coordinate
        (dict(quats=(3,), nq=6), "quat_adr[0] = 3"),
        (dict(quats=(0, 3)), "quat_adr[1] = 3 overlaps quat_adr[0] = 0"),
        (dict(quats=(3, 0)), "quat_adr[1] = 0 overlaps quat_adr[0] = 3"),
    ]
    for change, text in cases:
        got = call(**change)
        assert got == -1 and text in _err() and "plant_residuals" in _err(), (change, got, _err())
    assert "JH_MAX_ENSEMBLE" in (call(M=33), _err())[1] and "JH_MAX_ID_HORIZON" in (call(H=65), _err())[1] and "JH_MAX_ID_QUATS" in (call(quats=(0,) * 5), _err())[1]
    torch.cuda.synchronize()
    assert bool((err == POISON).all())
    assert call() == 0 and call(quats=(), null_quats=True) == 0 and call(M=32, H=1, ld=W) == 0  # ... and the arguments they were varied from are accepted
    torch.cuda.synchronize()
    assert bool((err[:3, :W] == 0).all())
