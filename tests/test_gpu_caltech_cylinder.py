"""The cylinder build of the leap kernel (jh_engine_v5_cyl.hip) against the fp64 oracle on the MJCF's geometry: caltech_leap_cube with its four fingertip cylinders
(r = 14 mm, half length 7 mm) as cylinders on both sides -- `CaltechLeapCube(fingertips="cylinder")` here, `oracle.Model("caltech_leap_cube")` there, nothing shared.

Sphere against cylinder is MuJoCo's primitive on both sides and agrees like the box / sphere pairs.  Box and cylinder against cylinder go through GJK + EPA: fp64 with
an unbounded polytope in the oracle, fp32 with at most 40 vertices and a stop within 1e-6 m of the surface in the kernel (jh_coop.h).  That stop leaves the normal of a
curved contact within about sqrt(2e-6 / 0.014) = 12 mrad of the oracle's (a host build of the routine on these poses' 1 691 GJK + EPA contacts: 99 % within 10 mrad), so the
one-step error of those pairs sits orders of magnitude above the closed-form pairs'.
Every bound below is 5 x the value observed on an MI355X (the comment beside it; profiles/caltech_cylinder.md has the table)."""

import numpy as np
import pytest

from tests.conftest import bounded

pytestmark = pytest.mark.gpu

KINDS = ("box-cylinder", "cylinder-sphere", "cylinder-cylinder")
# one step, per pair kind: (median, 90th percentile, maximum) over the poses of the largest velocity error of a pose, relative to max(1, largest |velocity| of the pose),
# and the maximum position error (rad / m).  5 x observed.  The poses span the whole joint ranges: 200 per kind, 5 to 64 contacts each, cylinder contacts 0.2 to 19 mm deep
# (the fingertip's radius is 14 mm), and most poses of one kind hold contacts of the other two as well: the cylinder-sphere row's errors are those of the GJK + EPA pairs in
# the same poses, the primitive itself being the oracle's closed form.  The tire's largest observed one-step velocity error is 1.4e-2 (tests/test_gpu_spot_tire.py).
# With the stop at 1e-7 m instead of 1e-6 the medians are 1.4e-4 / 1.8e-4 / 2.4e-4 and the 90th percentiles 2.1e-3 / 1.8e-3 / 1.9e-3, the maxima 7.5e-2 / 4.6e-2 / 1.9e-1 --
# no better at the top -- for 22 % more time at 65 536 x 48 (profiles/caltech_cylinder.md), so the build keeps 1e-6.
TOL_STEP = {
    "box-cylinder": (1.8e-3, 1.7e-2, 6.9e-2, 2.0e-2),       # observed 3.482e-4, 3.234e-3, 1.362e-2, 3.825e-3; the worst pose's deepest contact of the kind: rim, 3.6 mm deep
    "cylinder-sphere": (2.9e-3, 2.0e-2, 1.9e-1, 4.5e-3),    # observed 5.640e-4, 3.887e-3, 3.753e-2, 8.867e-4; rim, 10 mm deep
    "cylinder-cylinder": (3.4e-3, 2.5e-2, 6.8e-1, 1.9e-2),  # observed 6.660e-4, 4.931e-3, 1.357e-1, 3.615e-3; cap, 1 mm deep (two caps nearly parallel: the contact point on a non-unique feature)
}
# trajectories (256 x 48 from the home state), cylinder build against the MJCF oracle: median state error, per knot noise.  5 x observed (5.947e-8, 6.918e-8, 8.388e-8).
TOL_TRAJ_MEDIAN = {0.2: 3.0e-7, 0.4: 3.5e-7, 0.8: 4.2e-7}
# fused cost against the cost of the materialised rollout of the same controls, relative.  Observed 7.451e-9; 5 x that is below one unit in the last place of an fp32
# cost (2^-23 = 1.19e-7), which is the bound: the two instantiations of the kernel may round the last bit differently.
TOL_FUSED_VS_MATERIALISED = 1.19e-7
# Controller, MPPI: nominal knots against the oracle's plan step, and against the fp64 update of the oracle's candidates with the GPU's own rewards.  5 x observed
# (N = 32: 4.896e-3, 1.442e-7; N = 4096: 1.061e-2, 1.422e-7).  Against the oracle's plan step the temperature 0.0025 multiplies a reward difference by 400 in the exponent,
# and over the shipped 100-step horizon a contact-rich rollout diverges from the oracle's (reward difference: median 8e-6 / 6e-6, largest 2.2e-3 / 1.3e-1; a cylinder
# touches in 53 % / 38 % of the rollouts).
TOL_NOMINAL = {32: (2.5e-2, 7.2e-7), 4096: (5.3e-2, 7.1e-7)}

def _task():
    from judo_amd.tasks import CaltechLeapCube

    return CaltechLeapCube(fingertips="cylinder")


def _pair_kinds(om):
    gt = [g["type"] for g in om.desc["geoms"]]
    code = {("box", "cylinder"): 0, ("cylinder", "sphere"): 1, ("cylinder", "cylinder"): 2}
    return np.array([code.get(tuple(sorted((gt[a], gt[b]))), 3) for a, b in om.pairs])


def test_task_model_backend_and_controller_run_the_cylinder_build(gpu):
    from judo_amd.controller import Controller, make_controller, make_controller_for
    from judo_amd.rollout_backend import GpuRolloutBackend
    from judo_amd.tasks import CaltechLeapCube

    t = _task()
    gm = t.gpu_model()
    assert gm.fingertips == "cylinder" and gm.build() == {"kernel_generation": 3, "contact_capacity": 64, "cylinder_build": True, "cylinders": 4}
    assert gm.contact_capacity == 64 and gm.limits()[3] == 64
    assert GpuRolloutBackend(gm, 8).model.build()["cylinder_build"]
    ctrl = make_controller_for(t, "mppi")
    assert isinstance(ctrl, Controller) and ctrl.model.build()["cylinder_build"] and ctrl.optimizer.config.num_rollouts == 32
    for c in (make_controller("caltech_leap_cube", "mppi"), make_controller_for(CaltechLeapCube(), "mppi")):  # the default stays the sphere build
        assert c.model.fingertips == "sphere" and c.model.build() == {"kernel_generation": 3, "contact_capacity": 64, "cylinder_build": False, "cylinders": 0}
    lc = make_controller("leap_cube", "mppi")
    assert lc.model.build() == {"kernel_generation": 3, "contact_capacity": 48, "cylinder_build": False, "cylinders": 0}


def _feature(om, x, u, k):
    """(depth, side / rim / cap): where on its cylinder the deepest contact of pair kind k sits in this state (the normal against the cylinder's axis)."""
    from judo_amd.models import quat_to_mat

    d = om.desc
    code = {("box", "cylinder"): 0, ("cylinder", "sphere"): 1, ("cylinder", "cylinder"): 2}
    best = None
    for row in om.forward(x[:23], x[23:], u)["contacts"]:
        g1, g2 = int(row[13]), int(row[14])
        if code.get(tuple(sorted((d["geoms"][g1]["type"], d["geoms"][g2]["type"])))) != k or (best is not None and row[0] >= best[0]):
            continue
        g = d["geoms"][g1 if d["geoms"][g1]["type"] == "cylinder" else g2]
        _, Rb = om.body_pose(x[:23], g["body"])
        c = abs(float((Rb @ quat_to_mat(np.array(g["quat"]))[:, 2]) @ row[4:7]))
        best = (float(row[0]), "cap" if c > 0.999 else ("side" if c < 0.045 else "rim"))
    return best


def _one_step_cases():
    """Hand poses drawn uniformly inside the joint ranges (4 000 draws, default_rng(0)), the cube moved away to (0.5, 0.5, 0.5) and the cube at home, zero velocity,
    controls = the pose.  Per pair kind: the poses whose oracle contacts fit the build's 64 and that hold a contact of the kind -- the first 100 of either cube position,
    in the order drawn; none is left out for any other reason.  Returns the oracle, the states, the controls and per kind the rows."""
    from judo_amd.tasks import CALTECH_LEAP_QPOS_HOME as HOME
    from oracle import oracle as O

    om = O.Model("caltech_leap_cube")
    kind = _pair_kinds(om)
    assert [int((kind == k).sum()) for k in range(3)] == [233, 12, 6]
    cap = 64
    rngs = np.array([j["range"] for j in om.desc["joints"] if j["type"] != "free"])
    rng = np.random.default_rng(0)
    ND = 4000
    q = rngs[:, 0] + (rngs[:, 1] - rngs[:, 0]) * rng.uniform(0.0, 1.0, (ND, 16))
    sel = {k: [] for k in range(3)}
    xs_all = []
    for cube in ("away", "home"):
        xs = np.zeros((ND, 45))
        xs[:, :7] = HOME[:7]
        if cube == "away":
            xs[:, :3] = 0.5
        xs[:, 7:23] = q
        cnt = np.array([om.pair_contact_counts(xs[i, :23]) for i in range(ND)])
        tot = cnt.sum(axis=1)
        for k in range(3):
            has = (tot <= cap) & (cnt[:, kind == k].sum(axis=1) > 0)
            print(f"cube {cube}: {int(has.sum())} poses within {cap} contacts hold a {KINDS[k]} contact")
            sel[k] += (len(xs_all) * ND + np.flatnonzero(has)[:100]).tolist()
        xs_all.append(xs)
    xs_all = np.concatenate(xs_all)
    rows = np.unique(np.concatenate([sel[k] for k in range(3)]))
    where = {int(r): i for i, r in enumerate(rows)}
    return om, xs_all[rows], xs_all[rows, None, 7:23], {k: np.array([where[r] for r in sel[k]]) for k in range(3)}


def test_each_pair_kind_one_step(gpu):
    """The state after one step from the poses of `_one_step_cases`, per pair kind."""
    from judo_amd.rollout_backend import GpuRolloutBackend

    om, xs, U, sel = _one_step_cases()
    ref, _ = om.rollout(xs, U)
    t = _task()
    assert t.gpu_model().limits()[3] == 64
    be = GpuRolloutBackend(t.gpu_model(), len(xs))
    assert be.model.build()["cylinder_build"]
    be.model.stats()
    g, _, _ = be.rollout(xs, U)
    st = be.model.stats()
    assert np.isfinite(g).all() and st["contact_overflow"] == 0 and st["newton_cap_hits"] == 0, st
    scale = np.maximum(1.0, np.abs(ref[:, 0, 23:]).max(axis=1))
    ev = np.abs(g[:, 0, 23:] - ref[:, 0, 23:]).max(axis=1) / scale
    ep = np.abs(g[:, 0, :23] - ref[:, 0, :23]).max(axis=1)
    failed = []
    for k in range(3):
        idx = sel[k]
        assert len(idx) >= 50, (KINDS[k], len(idx))
        worst = idx[np.argmax(ev[idx])]
        print(f"{KINDS[k]}: {len(idx)} poses, velocity error median {np.median(ev[idx]):.3e} p90 {np.percentile(ev[idx], 90):.3e} max {ev[idx].max():.3e}, "
              f"position error max {ep[idx].max():.3e}; worst pose's deepest {KINDS[k]} contact: {_feature(om, xs[worst], U[worst, 0], k)}")
        tm, t90, tx, tp = TOL_STEP[KINDS[k]]
        ok = bounded(f"{KINDS[k]}: one-step velocity error, median", np.median(ev[idx]), tm)
        ok &= bounded(f"{KINDS[k]}: one-step velocity error, 90th percentile", np.percentile(ev[idx], 90), t90)
        ok &= bounded(f"{KINDS[k]}: one-step velocity error, max", ev[idx].max(), tx)
        ok &= bounded(f"{KINDS[k]}: one-step position error, max", ep[idx].max(), tp)
        if not ok:
            failed.append(KINDS[k])
    assert not failed, failed


def test_trajectories_follow_the_mjcf_oracle_closer_than_the_sphere_build(gpu):
    """The inputs of test_gpu_leap.py::test_caltech_fingertip_cylinder_stand_in_is_a_measured_deviation (256 x 48 from the home state, knot noise 0.2 and 0.4) and the
    same construction at 0.8, where a cylinder touches in half of the rollouts.  Both builds against the oracle on the MJCF's geometry, over ALL rollouts."""
    from judo_amd.rollout_backend import GpuRolloutBackend
    from judo_amd.tasks import CaltechLeapCube
    from oracle import oracle as O

    t = _task()
    x0 = t.default_state()
    N, H = 256, 48
    om = O.Model("caltech_leap_cube")
    kind = _pair_kinds(om)
    bc = GpuRolloutBackend(t.gpu_model(), N)
    bs = GpuRolloutBackend(CaltechLeapCube().gpu_model(), N)
    assert bc.model.build()["cylinder_build"] and not bs.model.build()["cylinder_build"] and bs.model.contact_capacity == 64
    failed = []
    for amp in (0.2, 0.4, 0.8):
        rng = np.random.default_rng(4)
        U = t.reset_command[None, None] + amp * np.repeat(rng.standard_normal((N, 4, 16)), H // 4, axis=1)
        rc, _ = om.rollout(x0, U)
        assert np.isfinite(rc).all()
        touched = np.array([om.pair_contact_counts(np.concatenate([x0[None, :23], rc[i, :-1, :23]]))[kind < 3].sum() > 0 for i in range(N)])
        share = touched.mean()
        bc.model.stats()
        gc, _, _ = bc.rollout(x0, U)
        stc = bc.model.stats()
        gs, _, _ = bs.rollout(x0, U)
        assert np.isfinite(gc).all() and np.isfinite(gs).all()
        ec, es = np.abs(gc - rc), np.abs(gs - rc)
        p90c, p90s = np.percentile(ec[:, -1, :3], 90), np.percentile(es[:, -1, :3], 90)
        print(f"noise {amp}: a cylinder touches in {share:.3f} of the rollouts; cylinder build: median state error {np.median(ec):.3e}, cube position at the horizon p90 {p90c:.3e}; "
              f"sphere build: {np.median(es):.3e}, {p90s:.3e}; dropped contacts {stc['contact_overflow']}, Newton cap hits {stc['newton_cap_hits']}")
        if amp == 0.8:
            assert share >= 1.0 / 3.0, share  # (observed on the CPU: 0.52 of the first 128) -- the cylinders are not idle
        assert stc["contact_overflow"] == 0
        if not bounded(f"cylinder build, noise {amp}: median state error", np.median(ec), TOL_TRAJ_MEDIAN[amp]):
            failed.append((amp, "median", np.median(ec)))
        if amp >= 0.4 and not p90c < p90s:
            failed.append((amp, "p90 cylinder build >= sphere build", p90c, p90s))
    assert not failed, failed


def test_same_answers_on_every_path(gpu, monkeypatch):
    """Launch shapes of the cylinder build agree as the sphere builds' do (tests/test_gpu_edges.py, tests/test_gpu_leap.py): a rollout's bits do not depend on the launch it
    is in, on its position in a wave, or on the latency mode of small launches; the fused cost is the cost of the materialised rollout up to the two instantiations'
    rounding; the model has no trace sensors, so a traced launch is refused as the sphere build refuses it."""
    import torch

    from judo_amd import _lib
    from judo_amd.controller import make_controller_for
    from judo_amd.rollout_backend import GpuRolloutBackend

    t = _task()
    N, H = 130, 48
    x0 = torch.as_tensor(np.asarray(t.default_state(), dtype=np.float32)).cuda()
    g = torch.Generator(device="cuda").manual_seed(5)
    U = (0.6 * torch.randn((N, 4, t.nu), device="cuda", generator=g).repeat_interleave(H // 4, dim=1) + torch.as_tensor(np.asarray(t.reset_command, dtype=np.float32)).cuda()).contiguous()
    be = GpuRolloutBackend(t.gpu_model(), N)
    s0, y0 = be.rollout_device(x0, U)
    s1, y1 = be.rollout_device(x0, U)
    assert torch.equal(s0, s1) and torch.equal(y0, y1)
    for sh in (1, 3):  # another row of the wave, other wave-mates
        Us = torch.cat([U[:1].expand(sh, -1, -1), U[:-sh]]).contiguous()
        s2, y2 = be.rollout_device(x0, Us)
        assert torch.equal(s2[sh:], s0[:-sh]) and torch.equal(y2[sh:], y0[:-sh])
    # latency mode (below 1 024 rollouts several rows of a wave compute the same rollout) against the full mapping: materialised ...
    out = {}
    for mode in ("0", "1", "2", None):
        monkeypatch.delenv("JUDO_AMD_LATENCY_SHIFT", raising=False) if mode is None else monkeypatch.setenv("JUDO_AMD_LATENCY_SHIFT", mode)
        be.model.stats()
        s, y = be.rollout_device(x0, U[:37].contiguous())
        out[mode] = (s.clone(), y.clone(), be.model.stats())
    for mode in ("1", "2", None):
        assert torch.equal(out[mode][0], out["0"][0]) and torch.equal(out[mode][1], out["0"][1])
        assert out[mode][2]["steps"] == out["0"][2]["steps"] == 37 * H and out[mode][2]["newton_iters"] == out["0"][2]["newton_iters"]
    assert torch.equal(out["0"][0], s0[:37])
    # ... and fused (the plan step of a Controller on injected noise)
    costs = {}
    noise = np.random.default_rng(3).standard_normal((36, 4, 16)).astype(np.float32) * 3.0  # (sigma 0.2 with the ramp: up to 0.6 rad on the last knot)
    for mode in ("0", None):
        monkeypatch.delenv("JUDO_AMD_LATENCY_SHIFT", raising=False) if mode is None else monkeypatch.setenv("JUDO_AMD_LATENCY_SHIFT", mode)
        for mat in (False, True):
            ctrl = make_controller_for(_task(), "mppi")
            assert ctrl.model.build()["cylinder_build"]
            ctrl.optimizer.config.num_rollouts = 37
            ctrl.controller_cfg.horizon = 0.48
            ctrl.force_materialize = mat
            ctrl.reset()
            ctrl.current_state = ctrl.task.default_state()
            ctrl.optimizer.injected_noise = noise
            ctrl.update_action()
            torch.cuda.synchronize()
            assert ctrl.uses_fused_cost or mat
            costs[(mode, mat)] = (-np.asarray(ctrl.rewards_local, dtype=np.float64), ctrl.nominal_knots.copy())
            assert ctrl.traces is None or ctrl.traces.size == 0
    for mat in (False, True):
        np.testing.assert_array_equal(costs[(None, mat)][0], costs[("0", mat)][0])
        np.testing.assert_array_equal(costs[(None, mat)][1], costs[("0", mat)][1])
    d = np.abs(costs[("0", False)][0] - costs[("0", True)][0]) / np.maximum(1.0, np.abs(costs[("0", True)][0]))
    print(f"fused cost against the materialised rollout's: max relative difference {d.max():.3e} (costs up to {np.abs(costs[('0', True)][0]).max():.3e})")
    assert bounded("cylinder build: fused cost against the materialised rollout's cost", d.max(), TOL_FUSED_VS_MATERIALISED)
    # no trace sensors in caltech_leap_cube: the traced launch is an error, not a silent no-op
    gm = t.gpu_model()
    assert gm.trace_layout()[1] == 0
    z = torch.zeros(64, device="cuda")
    st = _lib.lib().jh_rollout_cost_traced(gm.handle, _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), 1, _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), 0, 1, 0, 4, 1, _lib.ptr(z), None,
                                           _lib.ptr(z), torch.cuda.current_stream().cuda_stream)
    with pytest.raises(ValueError, match="no trace sensors"):
        _lib.check(st, "jh_rollout_cost_traced")


@pytest.mark.parametrize("N", [32, 4096])
def test_controller_plan_step_matches_the_mjcf_oracle(gpu, N):
    """MPPI on `CaltechLeapCube(fingertips="cylinder")` at the shipped 32 rollouts (latency mode) and at 4 096: one plan step from the home state on injected noise against
    the same step built from oracle primitives on the MJCF's geometry."""
    import torch

    from judo_amd.controller import make_controller_for
    from oracle import oracle as O

    ctrl = make_controller_for(_task(), "mppi")
    cfg = ctrl.optimizer.config
    assert cfg.num_rollouts == 32 and ctrl.model.build()["cylinder_build"]
    cfg.num_rollouts = N
    ctrl.reset()
    ctrl.current_state = ctrl.task.default_state()
    noise = np.random.default_rng(11).standard_normal((N - 1, cfg.num_nodes, 16)).astype(np.float32)
    ctrl.optimizer.injected_noise = noise
    nominal0 = ctrl.nominal_knots.copy()
    ctrl.model.stats()
    ctrl.update_action()
    torch.cuda.synchronize()
    assert ctrl.uses_fused_cost
    st = ctrl.model.stats()
    om = O.Model("caltech_leap_cube")
    sigma = O.mppi_sigma(cfg.sigma, cfg.use_noise_ramp, cfg.noise_ramp, cfg.num_nodes, 16)
    r = ctrl.task.actuator_ctrlrange
    knots = O.clip_knots(O.sample_knots(nominal0, noise.astype(np.float64), sigma), r[:, 0], r[:, 1])
    U = O.spline_eval(O.spline_weights(ctrl.spline_order, ctrl.spline_timesteps, ctrl.rollout_times), knots)
    states, _ = om.rollout(ctrl.current_state, U)
    gq = np.array([1.0, 0.0, 0.0, 0.0])
    rewards = O.reward_leap(states, gq, ctrl.task.config.w_pos, ctrl.task.config.w_rot, ctrl.task.goal_pos)
    ref = O.mppi_update(knots, rewards, cfg.temperature)
    kind = _pair_kinds(om)
    sample = range(0, N, max(1, N // 128))
    share = np.mean([om.pair_contact_counts(states[i, :, :23])[kind < 3].sum() > 0 for i in sample])
    err = float(np.abs(ctrl.nominal_knots - ref).max())
    err_update = float(np.abs(ctrl.nominal_knots - O.mppi_update(knots, np.asarray(ctrl.rewards_local, dtype=np.float64), cfg.temperature)).max())
    dc = np.abs(np.asarray(ctrl.rewards_local, dtype=np.float64) - rewards)
    print(f"N = {N}, H = {ctrl.num_timesteps}: a cylinder touches in {share:.3f} of the sampled rollouts; |nominal - oracle| = {err:.3e}, |nominal - update of the GPU's rewards| = {err_update:.3e}, "
          f"reward difference median {np.median(dc):.3e} max {dc.max():.3e}; dropped contacts {st['contact_overflow']}, Newton cap hits {st['newton_cap_hits']}")
    assert np.isfinite(ctrl.nominal_knots).all() and st["contact_overflow"] == 0
    ok = bounded(f"cylinder build, MPPI N = {N}: nominal knots against the oracle's plan step", err, TOL_NOMINAL[N][0])
    ok &= bounded(f"cylinder build, MPPI N = {N}: nominal knots against the fp64 update of the GPU's rewards", err_update, TOL_NOMINAL[N][1])
    assert ok, (err, err_update)


def test_refusals(gpu):
    """An image with a cylinder runs on the cylinder build and nowhere else: kernel generations 1 and 2, the 48-contact setting, another model family and a malformed
    cylinder record are refused with a message."""
    import ctypes as C
    import struct

    from judo_amd import _lib
    from judo_amd.device import GpuModel
    from judo_amd.engine_model import pack_engine_model
    from judo_amd.models import load_description

    gm = _task().gpu_model()
    for gen in (1, 2):
        with pytest.raises(RuntimeError, match="cylinder"):
            gm.set_kernel(gen)
        assert gm.build()["kernel_generation"] == 3
    with pytest.raises(ValueError, match="cylinder build"):
        gm.set_contact_capacity(48)
    assert gm.build()["contact_capacity"] == 64
    gm.set_self_collision(False)  # the cube's contacts alone: the same build without the hand's own pairs
    gm.set_self_collision(True)

    def create(blob):
        h = C.c_void_p()
        buf = C.create_string_buffer(blob, len(blob))
        st = _lib.lib().jh_model_create(buf, len(blob), 0, C.byref(h))
        if st == 0:
            _lib.lib().jh_model_destroy(h)
        _lib.check(st, "jh_model_create")

    desc = load_description("caltech_leap_cube")
    good = pack_engine_model(desc, fingertips="cylinder")
    create(good)
    nf = struct.unpack_from("<I", good, 32)[0]
    F = np.frombuffer(good, dtype="<f4", count=nf, offset=64).copy()
    I = np.frombuffer(good, dtype="<i4", offset=64 + 4 * nf)
    oI = 24 + int(I[0]) * 6 + int(I[1]) * 4 + int(I[4]) * 2
    oF = 24 + int(I[0]) * 32 + int(I[2]) * 20 + int(I[4]) * 8
    gcyl = next(g for g in range(int(I[5])) if I[oI + 2 * g + 1] == 5)
    for field, value, msg in ((1, 0.0, "half length"), (0, -0.014, "radius"), (15, 0.014, "bounding radius")):
        Fb = F.copy()
        Fb[oF + 20 * gcyl + field] = value
        with pytest.raises(RuntimeError, match=msg):
            create(good[:64] + Fb.tobytes() + good[64 + 4 * nf:])
    # a cylinder in the other articulated family: type code 5 planted in an fr3_pick image
    fr3 = pack_engine_model(load_description("fr3_pick"))
    nf3 = struct.unpack_from("<I", fr3, 32)[0]
    I3 = np.frombuffer(fr3, dtype="<i4", offset=64 + 4 * nf3).copy()
    F3 = np.frombuffer(fr3, dtype="<f4", count=nf3, offset=64).copy()
    oI3 = 24 + int(I3[0]) * 6 + int(I3[1]) * 4 + int(I3[4]) * 2
    oF3 = 24 + int(I3[0]) * 32 + int(I3[2]) * 20 + int(I3[4]) * 8
    I3[oI3 + 1] = 5
    F3[oF3:oF3 + 3] = (0.014, 0.007, 0.0)
    F3[oF3 + 15] = np.float32(np.hypot(0.014, 0.007))
    with pytest.raises(RuntimeError, match="only the leap kernel"):
        create(fr3[:64] + F3.tobytes() + I3.tobytes())
    # the default image still creates a sphere-build model, and GpuModel reports it
    assert GpuModel("caltech_leap_cube").fingertips == "sphere"
