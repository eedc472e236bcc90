"""jh_plant_residuals_reports through the C ABI: the weighted squared prediction error of M plants on W recorded windows over the REPORTED entries, bit for bit against
its numpy restatement (judo_amd.reports.plant_residuals_reports_host), in both layouts, with and without sensors, under the NaN patterns a robot's reports produce; bit
for bit jh_plant_residuals where the two coincide; and its refusals.

M = 3 plants on W = 5 windows are 15 (plant, window) pairs: the last workgroup of four waves is ragged, and M differs from W, so a swapped stride shows.  `err` is a
poisoned buffer with ld > W: a write outside row m's W entries shows.  No tolerance appears in this file."""

import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_plan_batch import _err
from tests.test_plant_reports_host import _inputs

pytestmark = pytest.mark.gpu

POISON = -7.0
M, W = 3, 5
SHAPES = {"nx9": (9, 9, (0, 4)), "nx1": (1, 1, ())}  # (nx, nq, quaternion offsets)
PATTERNS = ["full", "rows", "columns", "quaternion", "window", "scattered"]


def _thinned(obs, obs_sens, quats, pattern, seed):
    """The NaN patterns, on copies: every second step row; the last state column and every second sensor column; the first quaternion whole, everywhere; window 1 whole,
    sensors included; scattered readings outside the quaternions and a whole quaternion in some rows."""
    rng = np.random.default_rng(seed)
    o, s = obs.copy(), None if obs_sens is None else obs_sens.copy()
    nx = o.shape[-1]
    if pattern == "rows":
        o[:, 1::2] = np.nan
        if s is not None:
            s[:, ::2] = np.nan  # the sensors arrive on the other steps
    elif pattern == "columns":
        o[..., nx - 1] = np.nan
        if s is not None:
            s[..., ::2] = np.nan
    elif pattern == "quaternion":
        for a in quats[:1]:
            o[..., a : a + 4] = np.nan
    elif pattern == "window":
        o[1] = np.nan
        if s is not None:
            s[1] = np.nan
    elif pattern == "scattered":
        inq = np.zeros(nx, dtype=bool)
        for a in quats:
            inq[a : a + 4] = True
        drop = (rng.random(o.shape) < 0.3) & ~inq
        o[drop] = np.nan
        for a in quats[1:]:
            o[:, ::2, a : a + 4] = np.nan
        if s is not None:
            s[rng.random(s.shape) < 0.3] = np.nan
    return o, s


def _window_major(a, H):
    """Row m * W + w -> row w * M + m."""
    return None if a is None else np.ascontiguousarray(a.reshape(M, W, H, -1).transpose(1, 0, 2, 3)).reshape(M * W, H, -1)


def _call(gpu, pred, obs, weight, quats, nq, sens=(None, None, None), window_major=False, ld=W + 3):
    """The raw entry on host arrays: (M, ld) fp32, poisoned beforehand."""
    import torch

    from judo_amd import _lib

    H, nx = obs.shape[1:]
    host = [pred, obs, weight] + [a for a in sens if a is not None]
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in host]
    ns = 0 if sens[0] is None else sens[1].shape[-1]
    sp = [t.data_ptr() for t in d[3:]] if ns else [None, None, None]
    err = torch.full((M, ld), POISON, dtype=torch.float32, device=gpu)
    arr = (C.c_int * len(quats))(*quats) if quats else None
    ps, ws_ = (1, M) if window_major else (W, 1)
    _lib.check(_lib.lib().jh_plant_residuals_reports(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), arr, len(quats), sp[0], sp[1], sp[2], ns, ps, ws_, M, W, H, nx, nq,
                                                     err.data_ptr(), ld, 0), "jh_plant_residuals_reports")
    torch.cuda.synchronize()
    for t, a in zip(d, host):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()  # the inputs are read only
    return err.cpu().numpy()


@pytest.mark.parametrize("H", [1, 3, 33, 64])
@pytest.mark.parametrize("ns", [0, 1, 5])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_reports_equal_the_numpy_restatement(gpu, shape, ns, H):
    """Every NaN pattern in both layouts: one case per (shape, ns, H), twelve launches of 15 waves."""
    from judo_amd.reports import plant_residuals_reports_host

    nx, nq, quats = SHAPES[shape]
    pred, obs, weight, ps, os_, ws = _inputs(M, W, H, nx, ns, quats, seed=1000 * nx + 10 * ns + H)
    for pattern in PATTERNS:
        o, s = _thinned(obs, os_, quats, pattern, seed=H)
        want = plant_residuals_reports_host(pred, o, weight, quats, nq=nq, pred_sens=ps, obs_sens=s, weight_sens=ws)
        assert np.isfinite(want).all()
        if pattern == "window":
            assert np.array_equal(want[:, 1], np.zeros(M, dtype=np.float32)) and (np.delete(want, 1, axis=1) > 0).all()
        for window_major in (False, True):
            p, q = (_window_major(pred, H), _window_major(ps, H)) if window_major else (pred, ps)
            got = _call(gpu, p, o, weight, quats, nq, (q, s, ws), window_major)
            what = f"{shape} ns={ns} H={H} {pattern} {'window' if window_major else 'plant'}-major"
            np.testing.assert_array_equal(got[:, :W].view(np.uint32), want.view(np.uint32), err_msg=what)
            assert (got[:, W:] == POISON).all(), f"{what}: the floats between W and ld were written"
    # a swapped stride reads other pairs' rows: the case tells the layouts apart
    swapped = plant_residuals_reports_host(pred, obs, weight, quats, nq=nq, pred_sens=ps, obs_sens=os_, weight_sens=ws, window_major=True)
    assert not np.array_equal(swapped, plant_residuals_reports_host(pred, obs, weight, quats, nq=nq, pred_sens=ps, obs_sens=os_, weight_sens=ws))


@pytest.mark.parametrize("H", [1, 3, 33, 64])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_reports_equal_jh_plant_residuals_where_the_two_coincide(gpu, shape, H):
    """Nothing NaN, no sensors, plant-major strides: the bits of jh_plant_residuals, one observed quaternion sign-flipped included."""
    from tests.test_gpu_plant_residuals import _call as old_call

    nx, nq, quats = SHAPES[shape]
    pred, obs, weight, *_ = _inputs(M, W, H, nx, 0, quats, seed=7 * nx + H)
    if quats:
        obs[W - 1, H // 2, quats[0] : quats[0] + 4] *= -1
    got = _call(gpu, pred, obs, weight, quats, nq)
    old = old_call(gpu, pred, obs, weight, quats, M, W, H, nx, nq, W + 3)
    np.testing.assert_array_equal(got.view(np.uint32), old.view(np.uint32))
    assert (old[:, :W] > 0).all()


def test_nan_predictions(gpu):
    """A NaN prediction under an unreported entry is not read into the sum; under a reported one it gives NaN, in that (plant, window) alone.  pred == obs and an
    antipodal quaternion give exactly +0.0."""
    from judo_amd.reports import plant_residuals_reports_host

    H, ns = 7, 5
    nx, nq, quats = SHAPES["nx9"]
    pred, obs, weight, ps, os_, ws = _inputs(M, W, H, nx, ns, quats, seed=3)
    obs[3, 1, 8], obs[2, :, 0:4], os_[0, 2, 1] = np.nan, np.nan, np.nan
    clean = _call(gpu, pred, obs, weight, quats, nq, (ps, os_, ws))
    p4, s4 = pred.copy().reshape(M, W, H, nx), ps.copy().reshape(M, W, H, ns)
    p4[1, 3, 1, 8], p4[0, 2, 4, 2], s4[2, 0, 2, 1] = np.nan, np.nan, np.nan  # all three under unreported entries
    got = _call(gpu, p4.reshape(M * W, H, nx), obs, weight, quats, nq, (s4.reshape(M * W, H, ns), os_, ws))
    np.testing.assert_array_equal(got.view(np.uint32), clean.view(np.uint32))
    assert np.isfinite(clean[:, :W]).all()
    p4[1, 3, 1, 7], s4[2, 4, 0, 0] = np.nan, np.nan  # under reported ones
    got = _call(gpu, p4.reshape(M * W, H, nx), obs, weight, quats, nq, (s4.reshape(M * W, H, ns), os_, ws))[:, :W]
    want = plant_residuals_reports_host(p4.reshape(M * W, H, nx), obs, weight, quats, nq=nq, pred_sens=s4.reshape(M * W, H, ns), obs_sens=os_, weight_sens=ws)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    nan = np.zeros((M, W), dtype=bool)
    nan[1, 3] = nan[2, 4] = True
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], clean[:, :W][~nan])

    same, same_s = np.tile(np.nan_to_num(obs), (M, 1, 1)), np.tile(np.nan_to_num(os_), (M, 1, 1))
    same[W : 2 * W, :, 4:8] *= -1  # plant 1: the antipodal quaternions
    got = _call(gpu, same, obs, weight, quats, nq, (same_s, os_, ws))[:, :W]
    assert np.array_equal(got, np.zeros((M, W), dtype=np.float32)) and not np.signbit(got).any()


def test_reports_refusals(gpu):
    import torch

    from judo_amd import _lib

    L = _lib.lib()
    M, W, H, nx, nq, ns = 3, 4, 5, 9, 7, 2
    pred = torch.ones((33 * W, H, nx), dtype=torch.float32, device=gpu)
    obs = torch.ones((W, H, nx), dtype=torch.float32, device=gpu)
    weight = torch.ones(nx, dtype=torch.float32, device=gpu)
    pred_sens = torch.ones((33 * W, H, ns), dtype=torch.float32, device=gpu)
    obs_sens = torch.ones((W, H, ns), dtype=torch.float32, device=gpu)
    weight_sens = torch.ones(ns, dtype=torch.float32, device=gpu)
    err = torch.full((33, W + 2), POISON, dtype=torch.float32, device=gpu)

    def call(quats=(3,), nquat=None, null_quats=False, **kw):
        a = {**dict(pred=pred.data_ptr(), obs=obs.data_ptr(), weight=weight.data_ptr(), pred_sens=pred_sens.data_ptr(), obs_sens=obs_sens.data_ptr(),
                    weight_sens=weight_sens.data_ptr(), ns=ns, plant_stride=W, window_stride=1, M=M, W=W, H=H, nx=nx, nq=nq, err=err.data_ptr(), ld=W + 2), **kw}
        arr = None if null_quats else (C.c_int * max(len(quats), 1))(*quats)
        return L.jh_plant_residuals_reports(a["pred"], a["obs"], a["weight"], arr, len(quats) if nquat is None else nquat, a["pred_sens"], a["obs_sens"], a["weight_sens"], a["ns"],
                                            a["plant_stride"], a["window_stride"], a["M"], a["W"], a["H"], a["nx"], a["nq"], a["err"], a["ld"], 0)

    none = dict(pred_sens=None, obs_sens=None, weight_sens=None, ns=0)
    cases = [
        # everything jh_plant_residuals refuses
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
        # the sensors and the strides
        (dict(ns=-1), "ns = -1"),
        (dict(pred_sens=None), "pred_sens is a null pointer with ns = 2"),
        (dict(obs_sens=None), "obs_sens is a null pointer with ns = 2"),
        (dict(weight_sens=None), "weight_sens is a null pointer with ns = 2"),
        ({**none, "pred_sens": pred_sens.data_ptr()}, "pred_sens is not a null pointer with ns = 0"),
        ({**none, "obs_sens": obs_sens.data_ptr()}, "obs_sens is not a null pointer with ns = 0"),
        ({**none, "weight_sens": weight_sens.data_ptr()}, "weight_sens is not a null pointer with ns = 0"),
        (dict(plant_stride=0), "plant_stride = 0"),
        (dict(window_stride=0), "window_stride = 0"),
    ]
    for change, text in cases:
        got = call(**change)
        assert got == -1 and text in _err() and "plant_residuals_reports" in _err(), (change, got, _err())
    assert "JH_MAX_ENSEMBLE" in (call(M=33), _err())[1] and "JH_MAX_ID_HORIZON" in (call(H=65), _err())[1] and "JH_MAX_ID_QUATS" in (call(quats=(0,) * 5), _err())[1]
    torch.cuda.synchronize()
    assert bool((err == POISON).all())
    # ... and the arguments they were varied from are accepted
    assert call() == 0 and call(quats=(), null_quats=True, **none) == 0 and call(M=32, H=1, ld=W) == 0 and call(plant_stride=1, window_stride=M) == 0
    torch.cuda.synchronize()
    assert bool((err[:3, :W] == 0).all())
