"""The self-collision build of the fr3 kernel (jh_engine_v6_self.hip, `FR3Pick(self_collision=True)`: all 190 pairs the MJCF leaves) against the fp64 oracle's default
model, `oracle.Model("fr3_pick")`, which has had those pairs all along.

Every input comes from one oracle workload (tests/test_oracle.py::test_fr3_link_pairs_never_touch_on_the_baseline_workload at the shipped horizon and four times the
noise): 96 rollouts from the home pose, knots = reset command + 4 x the CEM's first sigma ramp (clip(0.155 * (1, 2, 3, 4), 0.01, 0.3)) x default_rng(7) normals, clipped to
the control ranges, linear spline, K = 4, dt = 0.004, H = 250.  There 26 of the 96 rollouts get a contact on a pair the default build leaves out, in 564 rollout-states:
hand box - link capsule 342, finger box - link capsule 128, hand / finger box - static fr3_link0 capsule 69, link capsule - link capsule 25.

Bounds: the single-step bounds are those of test_fr3_arm_links_collide_with_table_and_cube (the parent kernel's recorded error on link contacts); the plan-step tolerances
those of test_fr3_plan_step_cem_matches_oracle; the full-size tolerances those of test_fr3_full_size_sampled_rollouts_match_oracle.  profiles/fr3_self_collision.md has
the figures observed on an MI355X."""

import functools

import numpy as np
import pytest

from tests.conftest import bounded

pytestmark = pytest.mark.gpu

CLASSES = ("hand box - link capsule", "finger box - link capsule", "box - static fr3_link0 capsule", "link capsule - link capsule")
K, H, N = 4, 250, 96
# one step, per class of left-out contact: (median, maximum) of a state's largest velocity error relative to max(1, largest |velocity| of the step), and the maximum position
# error.  The bounds of test_fr3_arm_links_collide_with_table_and_cube (7e-6, 1e-3, 2e-5) where the class meets them, else 5 x the value observed on an MI355X (the comment
# beside it).  Every excess sits in the 67 of the 407 kept states whose two finger stacks overlap (the closed empty gripper at 4 x the noise: 86-96 contacts, the stiff regime
# of test_fr3_plan_step_cem_matches_oracle): there the fp64 oracle's own one-step answer moves by up to 3.7e-3 (positions 5.3e-5) when its inputs are rounded to fp32, and by at
# most 1.3e-6 on the other 340 states -- which the test holds to the three bounds as they stand, class by class present (243 / 70 / 14 / 13 states).
TOL_CLASS = (
    (7e-6, 2.9e-2, 2.4e-4),    # observed 2.579e-07, 5.757e-03, 4.630e-05
    (7e-6, 8.2e-3, 2.3e-4),    # observed 5.539e-07, 1.627e-03, 4.417e-05
    (1.5e-4, 2.0e-2, 1.7e-4),  # observed 2.955e-05, 3.993e-03, 3.397e-05 (15 of its 29 states have the stacks overlapped)
    (7e-6, 9.8e-3, 1.7e-4),    # observed 1.573e-06, 1.941e-03, 3.203e-05
)
MULT = 4.0


def _task():
    from judo_amd.tasks import FR3Pick

    return FR3Pick(self_collision=True)


def _pair_class(names, types, p):
    a, b = p
    if types[a] == types[b] == "capsule":
        return 3
    box, cap = (names[a], names[b]) if types[a] == "box" else (names[b], names[a])
    if "link0" in cap:
        return 2
    return 0 if "hand" in box else 1


@functools.lru_cache(maxsize=None)
def _workload():
    """The oracle side, computed once per session: both oracle models, the controls, the all-pairs and the kernel-subset rollouts, and per rollout-state (the state a step
    STARTS from) whether a left-out pair is in contact there and of which classes."""
    from judo_amd.tasks import FR3Pick
    from oracle import oracle as O

    t = FR3Pick()
    desc = O.load_description("fr3_pick")
    full, sub = O.Model("fr3_pick"), O.Model("fr3_pick", scope="kernel")
    kept = set(sub.pairs)
    extra = np.array([i for i, p in enumerate(full.pairs) if p not in kept])
    assert len(full.pairs) == 190 and len(extra) == 112
    names, types = [g["name"] for g in desc["geoms"]], [g["type"] for g in desc["geoms"]]
    cls = np.array([_pair_class(names, types, full.pairs[i]) for i in extra])
    assert [int((cls == c).sum()) for c in range(4)] == [5, 72, 13, 22]
    x0 = t.default_state()
    lo, hi = np.array([a["ctrlrange"] for a in desc["actuators"]]).T
    sigma_k = np.clip(0.155 * np.linspace(1, 4, K), 0.01, 0.3)
    W = O.spline_weights("linear", np.linspace(0, 1.0, K), 0.004 * np.arange(H))
    rng = np.random.default_rng(7)
    z = rng.standard_normal((N, K, 8))
    knots = np.clip(t.reset_command[None, None] + MULT * sigma_k[None, :, None] * z, lo, hi)
    U = O.spline_eval(W, knots)
    rf, _ = full.rollout(x0, U)
    rk, _ = sub.rollout(x0, U)
    X = np.concatenate([np.broadcast_to(x0, (N, 1, 31)), rf[:, :-1]], axis=1)  # the state step h starts from
    kcls = np.zeros((N, H, 4), dtype=bool)
    for n in range(N):
        for h in range(H):
            ce = full.pair_contact_counts(X[n, h, :16][None])[extra]
            for c in np.unique(cls[ce > 0]):
                kcls[n, h, c] = True
    return dict(full=full, sub=sub, x0=x0, U=U, z=z, rf=rf, rk=rk, X=X, kcls=kcls, hit=kcls.any(axis=2), extra=extra)


def test_precondition_the_left_out_pairs_touch_on_this_workload(gpu):
    w = _workload()
    hit_rollouts = int(w["hit"].any(axis=1).sum())
    per_class = w["kcls"].sum(axis=(0, 1))
    print(f"rollouts with a contact on a left-out pair: {hit_rollouts} of {N}; rollout-states {int(w['hit'].sum())}; per class {dict(zip(CLASSES, per_class.tolist()))}")
    assert hit_rollouts >= 20  # measured: 26
    assert (per_class > 0).all()  # measured: 342, 128, 69, 25
    d = np.abs(w["rf"][:, -1, 7:14] - w["rk"][:, -1, 7:14]).max(axis=1)[w["hit"].any(axis=1)]
    print(f"arm joints at the horizon, all pairs against the kernel's subset, on the hit rollouts: median {np.median(d):.3f} rad, min {d.min():.3f} rad")
    assert d.min() >= 0.1  # measured: 0.11 (median 0.49): the two pair sets are different physics on these rollouts


def test_single_steps_on_the_left_out_contacts(gpu):
    """One step of the new build against one step of the all-pairs oracle from every state of the oracle's rollouts at which a left-out pair is in contact, the oracle's solve
    converged below its iteration cap (100) and the state holds at most 96 general contacts (the kernel's capacity)."""
    from judo_amd.rollout_backend import GpuRolloutBackend

    w = _workload()
    full, sub = w["full"], w["sub"]
    idx = np.argwhere(w["hit"])
    S = w["X"][idx[:, 0], idx[:, 1]]
    U1 = w["U"][idx[:, 0], idx[:, 1]][:, None, :]
    kc = w["kcls"][idx[:, 0], idx[:, 1]]
    fw = [full.forward(x[:16], x[16:], u[0]) for x, u in zip(S, U1)]
    it, nc = np.array([f["solver_iter"] for f in fw]), np.array([f["ncon"] for f in fw])
    gripper = np.array([sum(1 for r in f["contacts"] if "finger" in full.desc["geoms"][int(r[13])]["name"] and "finger" in full.desc["geoms"][int(r[14])]["name"]) for f in fw])
    general = nc - gripper  # (finger against finger sits in the kernel's own 96 slots)
    keep = (it < 100) & (general <= 96)
    print(f"states {len(S)}: at the iteration cap {np.mean(it >= 100):.3f}, above 96 general contacts {np.mean(general > 96):.3f}, kept {keep.mean():.3f} = {int(keep.sum())}; "
          f"per class before {kc.sum(axis=0).tolist()} after {kc[keep].sum(axis=0).tolist()}")
    assert (~keep).mean() <= 0.35  # measured: 27.8 % at the cap (the finger-slam regime, the same share over all states of this workload), 0.7 % above 96 contacts
    assert keep.sum() >= 300 and (kc[keep].sum(axis=0) >= 10).all()
    S, U1, kc = S[keep], U1[keep], kc[keep]
    rs, _ = full.rollout(S, U1)
    rsub, _ = sub.rollout(S, U1)
    be = GpuRolloutBackend(_task().gpu_model(), len(S))
    assert be.model.fr3_build()["self_collision_build"]
    be.model.stats()
    gs, _, _ = be.rollout(S, U1)
    st = be.model.stats()
    assert np.isfinite(gs).all() and st["contact_overflow"] == 0
    sc = np.maximum(1.0, np.abs(rs[:, 0, 16:]).max(axis=1, keepdims=True))
    e1 = (np.abs(gs[:, 0, 16:] - rs[:, 0, 16:]) / sc).max(axis=1)
    sep = (np.abs(rsub[:, 0, 16:] - rs[:, 0, 16:]) / sc).max(axis=1)
    ep = np.abs(gs[:, 0, :16] - rs[:, 0, :16]).max(axis=1)
    # the reference's own error on these states: the oracle's answer when its inputs are rounded to fp32 (what the kernel is handed)
    r32, _ = full.rollout(S.astype(np.float32).astype(np.float64), U1.astype(np.float32).astype(np.float64))
    o1 = (np.abs(r32[:, 0, 16:] - rs[:, 0, 16:]) / sc).max(axis=1)
    op = np.abs(r32[:, 0, :16] - rs[:, 0, :16]).max(axis=1)
    shut = (S[:, 14] + S[:, 15]) < -5e-4  # the two finger stacks overlap by more than 0.5 mm in the state the step starts from (test_fr3_plan_step_cem_matches_oracle's split)
    ok = True
    for c in range(4):
        m = kc[:, c]
        print(f"  {CLASSES[c]:34s} states {int(m.sum()):4d} ({int((m & ~shut).sum())} with the finger stacks apart): velocity error median {np.median(e1[m]):.3e} max {e1[m].max():.3e}, position "
              f"error max {ep[m].max():.3e}; oracle all pairs against oracle subset: median {np.median(sep[m]):.3e}")
        ok &= bounded(f"self-collision build, one step, {CLASSES[c]}: velocity error median", np.median(e1[m]), TOL_CLASS[c][0])
        ok &= bounded(f"self-collision build, one step, {CLASSES[c]}: velocity error max", e1[m].max(), TOL_CLASS[c][1])
        ok &= bounded(f"self-collision build, one step, {CLASSES[c]}: position error max", ep[m].max(), TOL_CLASS[c][2])
    for nm, m in (("finger stacks apart", ~shut), ("finger stacks overlapped", shut)):
        print(f"  {nm:24s} states {int(m.sum()):4d} per class {kc[m].sum(axis=0).tolist()}: velocity error median {np.median(e1[m]):.3e} p90 {np.percentile(e1[m], 90):.3e} max {e1[m].max():.3e}, "
              f"position error max {ep[m].max():.3e} | the oracle on fp32 inputs: median {np.median(o1[m]):.3e} p90 {np.percentile(o1[m], 90):.3e} max {o1[m].max():.3e}, position max {op[m].max():.3e}")
    print(f"  all: velocity error median {np.median(e1):.3e} p90 {np.percentile(e1, 90):.3e} max {e1.max():.3e}; position error max {ep.max():.3e}; separation median "
          f"{np.median(sep):.3e} p10 {np.percentile(sep, 10):.3e}; Newton cap hits {st['newton_cap_hits']}")
    # (a) the finger stacks apart -- every class still has its ten states and 300 remain: the bounds of test_fr3_arm_links_collide_with_table_and_cube as they stand
    apart = ~shut
    assert apart.sum() >= 300 and (kc[apart].sum(axis=0) >= 10).all()
    ok &= bounded("self-collision build, one step, finger stacks apart: velocity error median", np.median(e1[apart]), 7e-6)
    ok &= bounded("self-collision build, one step, finger stacks apart: velocity error max", e1[apart].max(), 1e-3)
    ok &= bounded("self-collision build, one step, finger stacks apart: position error max", ep[apart].max(), 2e-5)
    # (b) the finger stacks overlapped: 5 x the oracle's own movement under fp32 rounding of its inputs on the same states
    ok &= bounded("self-collision build, one step, finger stacks overlapped: velocity error max against 5 x the oracle's own on fp32 inputs", e1[shut].max(), 5 * o1[shut].max())
    ok &= bounded("self-collision build, one step, finger stacks overlapped: position error max against 5 x the oracle's own on fp32 inputs", ep[shut].max(), 5 * op[shut].max())
    # (c) all kept states: the median, and the median against 1/100 of what the left-out pairs change
    ok &= bounded("self-collision build, one step: velocity error median", np.median(e1), 7e-6)
    ok &= bounded("self-collision build, one step: median error against 1/100 of the separation of the two pair sets", np.median(e1), np.median(sep) / 100)
    assert ok
    np.testing.assert_allclose(gs[apart, 0, :16], rs[apart, 0, :16], atol=2e-5)


def test_trajectories_follow_the_all_pairs_oracle(gpu):
    """The same controls through the new build and through the default build.  Where a left-out pair touches, the new build ends closer to the all-pairs oracle than the
    default build does (the two oracles are at least 0.11 rad apart there).  Elsewhere both builds meet the same bound: the default build's own error on those rollouts is
    the yardstick, at the project's factor of 5."""
    from judo_amd.rollout_backend import GpuRolloutBackend
    from judo_amd.tasks import FR3Pick

    w = _workload()
    bn = GpuRolloutBackend(_task().gpu_model(), N)
    bd = GpuRolloutBackend(FR3Pick().gpu_model(), N)
    assert bn.model.fr3_build()["self_collision_build"] and not bd.model.fr3_build()["self_collision_build"]
    gn, _, _ = bn.rollout(w["x0"], w["U"])
    gd, _, _ = bd.rollout(w["x0"], w["U"])
    stn, std = bn.model.stats(), bd.model.stats()
    assert np.isfinite(gn).all() and np.isfinite(gd).all()
    en = np.abs(gn[:, -1, 7:14] - w["rf"][:, -1, 7:14]).max(axis=1)
    ed = np.abs(gd[:, -1, 7:14] - w["rf"][:, -1, 7:14]).max(axis=1)
    hit = w["hit"].any(axis=1)
    ratio = en[hit] / ed[hit]
    print(f"hit rollouts {int(hit.sum())}: new build against the all-pairs oracle median {np.median(en[hit]):.3e} max {en[hit].max():.3e} rad; default build median "
          f"{np.median(ed[hit]):.3e} min {ed[hit].min():.3e} rad; ratio new / default median {np.median(ratio):.3e} max {ratio.max():.3e}")
    print(f"other rollouts {int((~hit).sum())}: new build median {np.median(en[~hit]):.3e} max {en[~hit].max():.3e}; default build median {np.median(ed[~hit]):.3e} max "
          f"{ed[~hit].max():.3e}; bit-identical states: {int((gn[~hit] == gd[~hit]).all(axis=(1, 2)).sum())} of {int((~hit).sum())}; dropped contacts new {stn['contact_overflow']} "
          f"default {std['contact_overflow']}")
    worse = np.flatnonzero(hit)[en[hit] >= ed[hit]]
    assert worse.size == 0, [(int(i), float(en[i]), float(ed[i])) for i in worse]
    ok = bounded("rollouts without a left-out contact: new build, median error at the horizon", np.median(en[~hit]), 5 * np.median(ed[~hit]))
    ok &= bounded("rollouts without a left-out contact: new build, max error at the horizon", en[~hit].max(), 5 * ed[~hit].max())
    assert ok


def _cem_controller(task, n, horizon_steps=H, mult=MULT):
    from judo_amd.controller import make_controller_for

    ctrl = make_controller_for(task, "cem")
    cfg = ctrl.optimizer.config
    cfg.num_rollouts = n
    cfg.sigma_min, cfg.sigma_max = mult * cfg.sigma_min, mult * cfg.sigma_max  # sigma scaled: the ramp's clip with it, so the first iteration samples mult x the shipped ramp
    ctrl.controller_cfg.horizon = horizon_steps * ctrl.task.dt
    ctrl.reset()
    ctrl.optimizer.sigma = mult * ctrl.optimizer.sigma
    ctrl.current_state = ctrl.task.default_state()
    return ctrl


def test_plan_step_cem_matches_the_all_pairs_oracle(gpu):
    """One CEM plan step in the shape of test_fr3_plan_step_cem_matches_oracle at the shipped H = 250 with sigma scaled 4 x: N = 64 (the shipped count; the oracle's leg is
    64 x 250 steps), noise default_rng(32) -- chosen on the oracle alone as the seed in 30..35 with the widest gap between the third and the fourth best reward (23.4; the
    slammed-gripper cost bound is 0.25).  The oracle must see a left-out pair touch in at least 10 % of the sampled rollouts (20 %)."""
    import torch

    from judo_amd.tasks import Phase
    from oracle import oracle as O
    from tests.harness import oracle_plan_step

    n = 64
    ctrl = _cem_controller(_task(), n)
    assert ctrl.model.fr3_build()["self_collision_build"] and ctrl.num_timesteps == H
    noise = np.random.default_rng(32).standard_normal((n - 1, K, 8)).astype(np.float32)
    ctrl.optimizer.injected_noise = noise
    ctrl.keep_candidates = True
    nominal0 = ctrl.nominal_knots.copy()
    sigma0 = ctrl.optimizer.sigma.copy()
    ctrl.model.stats()
    ctrl.update_action()
    torch.cuda.synchronize()
    st = ctrl.model.stats()
    assert ctrl.uses_fused_cost and ctrl.task.phase == Phase.LIFT.value
    om = O.Model("fr3_pick")
    ref = oracle_plan_step(om, ctrl, nominal0, noise, "cem", sigma0)
    np.testing.assert_allclose(ref["sigma_used"][:, 0], MULT * np.clip(0.155 * np.linspace(1, 4, K), 0.01, 0.3))
    w = _workload()
    x0 = ctrl.current_state
    touched = np.array([om.pair_contact_counts(np.concatenate([x0[None, :16], ref["states"][i, :-1, :16]]))[w["extra"]].sum() > 0 for i in range(n)])
    print(f"a left-out pair touches in {touched.mean():.3f} of the {n} sampled rollouts; dropped contacts {st['contact_overflow']}, Newton cap hits {st['newton_cap_hits']} of {st['steps']} steps")
    assert touched.mean() >= 0.10
    cand = ctrl.candidate_knots_device.permute(2, 0, 1).cpu().numpy()
    np.testing.assert_allclose(cand, ref["knots"], rtol=4e-7, atol=4e-7)
    costs = -ctrl.rewards_local
    d = np.abs(costs + ref["rewards"])
    slam = (ref["states"][:, :, 14] + ref["states"][:, :, 15]).min(axis=1) < -5e-4
    print(f"cost error: finger stacks apart ({int((~slam).sum())}) " + (f"median {np.median(d[~slam]):.3e} max {d[~slam].max():.3e}" if (~slam).any() else "-") +
          f"; slammed ({int(slam.sum())}) p95 {np.percentile(d[slam], 95):.3e} max {d[slam].max():.3e}; touched rollouts max {d[touched].max():.3e}")
    order = np.argsort(-ref["rewards"])
    gap = ref["rewards"][order[2]] - ref["rewards"][order[3]]
    print(f"elite gap {gap:.3f} against 20 x the elites' cost error {20 * d[order[:4]].max():.3e}")
    assert gap > 20 * d[order[:4]].max(), (gap, d[order[:4]].max())
    assert set(np.argsort(costs)[:3]) == set(order[:3])
    exp_nom, exp_sig, _ = O.cem_update(ref["knots"], -costs.astype(np.float64), 3, ctrl.optimizer.sigma_min, ctrl.optimizer.sigma_max)
    np.testing.assert_allclose(ctrl.nominal_knots, exp_nom, rtol=7e-7, atol=7e-8)
    np.testing.assert_allclose(ctrl.optimizer.sigma, exp_sig, rtol=5e-6, atol=5e-8)
    np.testing.assert_allclose(ctrl.nominal_knots, ref["nominal"], atol=7e-7)
    np.testing.assert_allclose(ctrl.optimizer.sigma, ref["sigma"], rtol=5e-6, atol=5e-8)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def test_same_answers_on_every_path(gpu, monkeypatch):
    """The launch shapes of the new build relate as the cylinder build's do (tests/test_gpu_caltech_cylinder.py::test_same_answers_on_every_path): a rollout's bits do not
    depend on the launch it is in, on its row in a wave or on the latency mode of small launches; the one-call plan step, the shard record path with one rank, the
    separate rollout + update launches, traced and untraced, give the same costs and the same nominal to the bit; the fused cost is the cost jh_task_reward gives the
    materialised rollout of the same knots up to the summation of 250 fp32 terms on either side (2 x 250 x 2^-24 = 3e-5 relative)."""
    import torch

    w = _workload()
    from judo_amd.rollout_backend import GpuRolloutBackend

    t = _task()
    x0 = torch.as_tensor(np.asarray(w["x0"], dtype=np.float32)).cuda()
    U = torch.as_tensor(np.asarray(w["U"], dtype=np.float32)).cuda().contiguous()
    be = GpuRolloutBackend(t.gpu_model(), N)
    s0, y0 = be.rollout_device(x0, U)
    s1, y1 = be.rollout_device(x0, U)
    assert torch.equal(s0, s1) and torch.equal(y0, y1)
    for sh in (1, 3):  # another row of the wave, other wave-mates
        Us = torch.cat([U[:1].expand(sh, -1, -1), U[:-sh]]).contiguous()
        s2, y2 = be.rollout_device(x0, Us)
        assert torch.equal(s2[sh:], s0[:-sh]) and torch.equal(y2[sh:], y0[:-sh])
    out = {}
    for mode in ("0", "1", "2", None):  # latency mode: N = 64 is below 1 024 rollouts
        monkeypatch.delenv("JUDO_AMD_LATENCY_SHIFT", raising=False) if mode is None else monkeypatch.setenv("JUDO_AMD_LATENCY_SHIFT", mode)
        be.model.stats()
        s, y = be.rollout_device(x0, U[:64].contiguous())
        out[mode] = (s.clone(), y.clone(), be.model.stats())
    for mode in ("1", "2", None):
        assert torch.equal(out[mode][0], out["0"][0]) and torch.equal(out[mode][1], out["0"][1])
        assert out[mode][2]["steps"] == out["0"][2]["steps"] == 64 * H and out[mode][2]["newton_iters"] == out["0"][2]["newton_iters"]
    assert torch.equal(out["0"][0], s0[:64])
    # the plan step of a Controller on the workload's own normals: candidate i + 1 has the knots of the workload's rollout i
    noise = w["z"][:63].astype(np.float32)
    res = {}
    shapes = {"plan_step": {}, "plan_step untraced": dict(fused_traces=False), "plan_step_shard": dict(force_shard_path=True), "separate": dict(fused_update=False),
              "separate untraced": dict(fused_update=False, fused_traces=False), "materialise": dict(force_materialize=True)}
    for mode in ("0", None):
        monkeypatch.delenv("JUDO_AMD_LATENCY_SHIFT", raising=False) if mode is None else monkeypatch.setenv("JUDO_AMD_LATENCY_SHIFT", mode)
        for name, knobs in shapes.items():
            ctrl = _cem_controller(_task(), 64)
            assert ctrl.model.fr3_build()["self_collision_build"]
            for k, v in knobs.items():
                setattr(ctrl, k, v)
            ctrl.optimizer.injected_noise = noise
            ctrl.update_action()
            torch.cuda.synchronize()
            assert ctrl.uses_fused_cost == (name != "materialise")
            tr = ctrl.traces
            res[(mode, name)] = (np.asarray(ctrl.rewards_local, dtype=np.float64).copy(), ctrl.nominal_knots.copy(), np.asarray(ctrl.optimizer.sigma).copy(), None if tr is None else np.array(tr))
    for name in shapes:
        for q in range(3):
            assert np.array_equal(_bits(res[(None, name)][q]), _bits(res[("0", name)][q])), (name, q)
    ref = res[("0", "plan_step")]
    for name in shapes:
        if name == "materialise":
            continue
        for q in range(3):
            assert np.array_equal(_bits(res[("0", name)][q]), _bits(ref[q])), (name, q)
        # the trace segments: the same bits wherever the same kernel wrote them (the fused kernel's trace rows; the elites re-rolled in materialise mode)
        same_source = res[("0", "plan_step untraced" if "untraced" in name else "plan_step")][3]
        assert res[("0", name)][3] is not None and np.array_equal(_bits(res[("0", name)][3]), _bits(same_source)), name
    dt = np.abs(res[("0", "plan_step untraced")][3] - ref[3]).max()
    print(f"trace segments, fused kernel's rows against the re-rolled elites: max difference {dt:.3e} m")
    cm, cf = -res[("0", "materialise")][0], -ref[0]
    d = np.abs(cf - cm) / np.maximum(1.0, np.abs(cm))
    print(f"fused cost against jh_task_reward on the materialised rollout: max relative difference {d.max():.3e} (costs up to {np.abs(cm).max():.3e})")
    assert bounded("self-collision build: fused cost against the materialised rollout's cost", d.max(), 2 * H * 2.0 ** -24)


def test_no_capacity_loss_on_the_baseline_sample(gpu):
    """BASELINE size (32 768 x 40, CEM, device noise; no left-out pair touches there): test_fr3_full_size_sampled_rollouts_match_oracle on the new build, at its tolerances,
    with the dropped contacts below 1e-4 per step -- 190 candidate pairs go through the same MAXHIT list and the same 32 + 64 contact capacity.  Whether the costs equal the
    default build's bit for bit is recorded."""
    import torch

    from judo_amd.controller import make_controller_for
    from judo_amd.tasks import FR3Pick
    from oracle import oracle as O
    from tests.harness import oracle_plan_step

    NB, M = 32768, 256
    runs = {}
    for name, task in (("self", _task()), ("default", FR3Pick())):
        ctrl = make_controller_for(task, "cem")
        ctrl.optimizer.config.num_rollouts = NB
        ctrl.controller_cfg.horizon = 40 * ctrl.task.dt
        ctrl.reset()
        ctrl.current_state = ctrl.task.default_state()
        ctrl.optimizer.seed(12)
        ctrl.prefetch_noise = False
        ctrl.keep_candidates = True
        nominal0 = ctrl.nominal_knots.copy()
        sigma0 = ctrl.optimizer.sigma.copy()
        assert ctrl.model.fr3_build()["self_collision_build"] == (name == "self")
        ctrl.update_action()
        torch.cuda.synchronize()
        runs[name] = (ctrl, nominal0, sigma0, ctrl.costs_device.cpu().numpy().astype(np.float64), ctrl.solver_stats())
    ctrl, nominal0, sigma0, costs, st = runs["self"]
    same = np.array_equal(_bits(costs), _bits(runs["default"][3]))
    print(f"costs of the 32 768 rollouts equal the default build's bit for bit: {same} ({int((_bits(costs) != _bits(runs['default'][3])).sum())} differ); dropped contacts per step "
          f"{st['contact_overflow'] / st['steps']:.3e} (default build {runs['default'][4]['contact_overflow'] / runs['default'][4]['steps']:.3e})")
    noise = ctrl.optimizer.last_noise
    cand = ctrl.candidate_knots_device.permute(2, 0, 1).cpu().numpy().astype(np.float64)
    assert costs.shape == (NB,) and np.isfinite(costs).all() and cand.shape == (NB, 4, 8)
    idx = np.concatenate([[0], np.sort(np.random.default_rng(6).choice(np.arange(1, NB), M - 1, replace=False))])
    inj = noise[:, :, torch.as_tensor(idx[1:], device=noise.device)].permute(2, 0, 1).cpu().numpy()
    ref = oracle_plan_step(O.Model("fr3_pick"), ctrl, nominal0, inj, "cem", sigma0)
    np.testing.assert_allclose(cand[idx], ref["knots"], rtol=4e-7, atol=4e-7)
    d = np.abs(costs[idx] + ref["rewards"])
    slam = (ref["states"][:, :, 14] + ref["states"][:, :, 15]).min(axis=1) < -5e-4
    print(f"cost error: apart median {np.median(d[~slam]):.3e} p95 {np.percentile(d[~slam], 95):.3e}; slammed p95 {np.percentile(d[slam], 95):.3e} max {d[slam].max():.3e}")
    assert bounded("self-collision build, full size, finger stacks apart: median", np.median(d[~slam]), 2e-4) and bounded("self-collision build, full size, finger stacks apart: p95", np.percentile(d[~slam], 95), 5e-4)
    assert bounded("self-collision build, full size, finger stacks slammed together: p95", np.percentile(d[slam], 95), 0.05) and bounded("self-collision build, full size, finger stacks slammed together: max", d[slam].max(), 0.25)
    exp_nom, exp_sig, _ = O.cem_update(cand, -costs, 3, ctrl.optimizer.sigma_min, ctrl.optimizer.sigma_max)
    np.testing.assert_allclose(ctrl.nominal_knots, exp_nom, rtol=3e-7, atol=3e-8)
    np.testing.assert_allclose(ctrl.optimizer.sigma, exp_sig, rtol=5e-7, atol=5e-9)
    assert st["contact_overflow"] < 1e-4 * st["steps"], st


def test_task_model_backend_controller_and_benchmark_run_the_new_build(gpu):
    from judo_amd.benchmark import plan_times
    from judo_amd.controller import Controller, make_controller, make_controller_for
    from judo_amd.device import GpuModel
    from judo_amd.rollout_backend import GpuRolloutBackend
    from judo_amd.tasks import FR3Pick

    t = _task()
    gm = t.gpu_model()
    assert gm.arm_self_collision and gm.fr3_build() == {"self_collision_build": True, "arm_pairs": 112, "default_build_accepts": False, "self_collision_build_accepts": True}
    assert gm.build() == {"kernel_generation": 3, "contact_capacity": 0, "cylinder_build": False, "cylinders": 0} and gm.limits()[3] == 96
    assert GpuRolloutBackend(gm, 8).model.fr3_build()["self_collision_build"] and GpuModel(t.desc).arm_self_collision
    ctrl = make_controller_for(t, "cem")
    assert isinstance(ctrl, Controller) and ctrl.model.arm_self_collision and ctrl.optimizer.config.num_rollouts == 64
    for c in (make_controller("fr3_pick", "cem"), make_controller_for(FR3Pick(), "cem")):  # the default stays the default build
        assert not c.model.arm_self_collision
        assert c.model.fr3_build() == {"self_collision_build": False, "arm_pairs": 0, "default_build_accepts": True, "self_collision_build_accepts": True}
    assert GpuModel("leap_cube").fr3_build() == {"self_collision_build": False, "arm_pairs": 0, "default_build_accepts": False, "self_collision_build_accepts": False}
    times = plan_times(_task(), "cem", 2, 1, None)
    assert times.shape == (2,) and (times > 0).all()


def test_refusals(gpu):
    """The full image runs on the self-collision build and nowhere else: kernel generations 1 and 2 refuse it, the default build refuses it, and a malformed pair between
    arm bodies is refused at jh_model_create, each with a message."""
    import ctypes as C
    import struct

    import torch

    from judo_amd import _lib
    from judo_amd.engine_model import pack_engine_model

    gm = _task().gpu_model()
    for gen in (1, 2):
        with pytest.raises(RuntimeError, match="pairs between arm bodies"):
            gm.set_kernel(gen)
        assert gm.build()["kernel_generation"] == 3
    assert not gm.fr3_build()["default_build_accepts"]
    # the default build's launchers themselves (C++ symbols of the library): handed the full image, they refuse it
    lib = C.CDLL(_lib.LIB_PATH)
    z = torch.zeros(4096, device="cuda")
    p = C.c_void_p(z.data_ptr())
    sym = "_Z22jh_engine6_materializePK8jh_modelPKfiS3_iiPfS4_P12ihipStream_t"
    fn = getattr(lib, sym)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    st = fn(gm.handle, p, 0, p, 1, 1, p, p, None)
    with pytest.raises(RuntimeError, match="self-collision build"):
        _lib.check(st, "jh_engine6_materialize")

    def create(blob):
        h = C.c_void_p()
        buf = C.create_string_buffer(blob, len(blob))
        st = _lib.lib().jh_model_create(buf, len(blob), 0, C.byref(h))
        if st == 0:
            _lib.lib().jh_model_destroy(h)
        _lib.check(st, "jh_model_create")

    good = pack_engine_model(_task().desc)
    create(good)
    nf = struct.unpack_from("<I", good, 32)[0]
    I = np.frombuffer(good, dtype="<i4", offset=64 + 4 * nf).copy()
    gi = int(I[13])
    nag, npair = int(I[gi]), int(I[gi + 1])
    op = gi + 8 + 2 * nag
    body = lambda g: int(I[gi + 8 + 2 * g])  # noqa: E731
    kind = lambda g: int(I[gi + 8 + 2 * g + 1])  # noqa: E731
    bc = next(p_ for p_ in range(78, npair) if kind(I[op + 2 * p_]) == 6 and kind(I[op + 2 * p_ + 1]) == 3 and body(I[op + 2 * p_ + 1]) >= 1)  # a box on the arm against a link capsule
    cases = []
    Ib = I.copy()
    Ib[op + 2 * bc], Ib[op + 2 * bc + 1] = I[op + 2 * bc + 1], I[op + 2 * bc]
    cases.append((Ib, "capsule first"))
    Ib = I.copy()
    Ib[op + 2 * bc + 1] = nag + 3
    cases.append((Ib, "names geoms"))
    Ib = I.copy()
    other = next(g for g in range(nag) if g != int(I[op + 2 * bc]) and body(g) == body(int(I[op + 2 * bc])))
    Ib[op + 2 * bc + 1] = other
    cases.append((Ib, "with each other"))
    for Ib, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            create(good[:64 + 4 * nf] + Ib.tobytes())
    # the default image still creates a default-build model
    from judo_amd.device import GpuModel

    assert not GpuModel("fr3_pick").arm_self_collision
