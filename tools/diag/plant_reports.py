"""What identifying the plant from a robot's reports costs (judo_amd/reports.py, `jh_plant_residuals_reports`); profiles/plant_reports.md is written from it.

    python tools/diag/plant_reports.py [--plants 4] [--windows 16] [--horizon 8] [--spot-horizon 4] [--reps 20] [--runs 5]

One JSON line per case, times in ms from device events around `reps` calls in a row after a warm-up call, `runs` measurements each, the old and the new alternating
within a run; the median and all runs are printed.
    leap_cube, fr3_pick   `PlantEstimator.update()` on fully observed windows against `ReportEstimator.update()` on the same windows (the two give the same bits, which
                          the tool checks first), and against `ReportEstimator.update()` on the windows thinned to every second step without velocities.
    spot_box_push         one plan step of the plain controller at 24 rollouts against one `SpotReportEstimator.update()` over `plants` boxes of other mass and
                          friction, `windows` windows of `spot-horizon` control steps, the object's pose and the robot's joint angles reported."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from materialize_plants_bench import descriptions  # noqa: E402


def events(fn, reps: int) -> float:
    import torch

    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(runs: dict) -> dict:
    out = {}
    for k, v in runs.items():
        out[k + "_ms"], out[k + "_runs"] = round(float(np.median(v)), 4), [round(x, 4) for x in v]
    return out


def model_set_case(task_name: str, M: int, W: int, H: int, reps: int, runs: int, sigma: float) -> dict:
    import torch

    from judo_amd.device import GpuModel, GpuModelSet
    from judo_amd.identify import PlantEstimator
    from judo_amd.reports import ReportEstimator
    from judo_amd.rollout_backend import GpuRolloutBackend
    from judo_amd.tasks import get_registered_tasks

    dev = torch.device("cuda", 0)
    task = get_registered_tasks()[task_name][0]()
    models = [GpuModel(d, dev) for d in descriptions(task_name, M)]
    mset, gm = GpuModelSet(models), models[0]
    rng = np.random.default_rng(0)
    x0 = np.tile(np.asarray(task.default_state(), dtype=np.float32), (W, 1))
    hold, spread = (np.asarray(task.reset_command, dtype=np.float32), 0.05) if task_name == "fr3_pick" else (x0[0, 7:23], 0.2)
    controls = (hold + spread * rng.standard_normal((W, H, gm.nu))).astype(np.float32)
    if task_name != "fr3_pick":  # let the cube come to rest in the hand first, as tools/diag/plant_identification.py does
        held = torch.from_numpy(np.tile(hold, (1, 100, 1)).astype(np.float32)).to(dev)
        x0 = np.tile(GpuRolloutBackend(gm, 1).rollout_device(torch.from_numpy(x0[0]).to(dev), held, want_sensors=False)[0][0, -1].cpu().numpy(), (W, 1))
    truth = GpuRolloutBackend(models[-1], W).rollout_device(torch.from_numpy(x0).to(dev), torch.from_numpy(controls).to(dev), want_sensors=False)[0].cpu().numpy()
    thin = truth.copy()
    thin[:, 0::2] = np.nan
    thin[..., gm.nq :] = np.nan
    old = PlantEstimator(mset, horizon=H, windows=W, state_sigma=sigma)
    new, sparse = ReportEstimator(mset, horizon=H, windows=W, state_sigma=sigma), ReportEstimator(mset, horizon=H, windows=W, state_sigma=sigma)
    for w in range(W):
        old.observe(x0[w], controls[w], truth[w])
        new.observe(x0[w], controls[w], truth[w])
        sparse.observe(x0[w], controls[w], thin[w])
    same = bool(old.update().tobytes() == new.update().tobytes() and old.errors.tobytes() == new.errors.tobytes())
    sparse.update()
    t = dict(plant_estimator=[], report_estimator=[], report_estimator_thinned=[])
    for _ in range(runs):
        t["plant_estimator"].append(events(old.update, reps))
        t["report_estimator"].append(events(new.update, reps))
        t["report_estimator_thinned"].append(events(sparse.update, reps))
    return dict(case=f"{task_name} M {M} x W {W} x H {H}", same_bits_when_nothing_is_thinned=same, truth=M - 1, map=int(new.map), map_thinned=int(sparse.map),
                reported_per_window_thinned=int(sparse.reported[0]), **summary(t))


def spot_case(M: int, W: int, T: int, reps: int, runs: int, sigma: float, rollouts: int = 24) -> dict:
    import torch

    from judo_amd.controller import make_controller
    from judo_amd.models import scaled_description
    from judo_amd.policy import PolicyRolloutBackend, SpotPlantSet
    from judo_amd.reports import SpotReportEstimator

    ctrl = make_controller("spot_box_push", "mppi")
    ctrl.optimizer.config.num_rollouts = rollouts
    ctrl.rollout_cutoff_time = None
    ctrl.reset()
    own = ctrl.rollout_backend
    base = ctrl.task.desc
    descs = [base] + [scaled_description(base, body_mass={"box_body": float(m)}, geom_friction={"box_collision": float(f)})
                      for m, f in zip(np.linspace(0.6, 1.7, M - 1), np.linspace(1.3, 0.6, M - 1))]
    plants = SpotPlantSet(descs, own.device, self_collision=own.engine.self_collision)
    nq = plants.nq
    rng = np.random.default_rng(0)
    x = np.tile(np.asarray(ctrl.task.default_state(), dtype=np.float64), (W, 1))
    x[:, 7:19] += 0.05 * rng.standard_normal((W, 12))
    x[:, 26:29] = (0.95, 0.0, 0.25)  # the box on the plane within the arm's reach: its mass and friction matter
    x[:, 26:28] += 0.01 * rng.standard_normal((W, 2))
    cmd = np.tile(np.asarray(ctrl.task.default_policy_command, dtype=np.float64), (W, T, 1))
    cmd[:, :, :3] = rng.uniform(-0.5, 0.5, (W, 1, 3))
    x0, cmd = torch.as_tensor(x, dtype=torch.float32, device=own.device), torch.as_tensor(cmd, dtype=torch.float32, device=own.device)
    out = torch.zeros((W, 12), dtype=torch.float32, device=own.device)
    truth = PolicyRolloutBackend(1, physics_substeps=own.physics_substeps, carry_warmstart=False,
                                 share=SimpleNamespace(device=own.device, engine=plants.engines[-1], policy=own.policy))
    est = SpotReportEstimator(plants, horizon=T, windows=W, physics_substeps=own.physics_substeps, policy=own.policy, state_sigma=sigma)
    for w in range(W):
        states = truth.rollout(x0[w], cmd[w : w + 1], out[w : w + 1])[0][0].cpu().numpy()
        states[:, nq:] = np.nan  # joint angles and poses, no velocities
        est.observe(x0[w], cmd[w], out[w], states)
    est.update()
    ctrl.current_state = ctrl.task.default_state()
    for _ in range(3):
        ctrl.update_action()
    t = dict(plan_step=[], spot_report_estimator=[])
    for _ in range(runs):
        t["plan_step"].append(events(ctrl.update_action, reps))
        t["spot_report_estimator"].append(events(est.update, reps))
    return dict(case=f"spot_box_push M {M} x W {W} x T {T}", plan_step=f"{type(ctrl).__name__} {rollouts} x H {int(ctrl.num_timesteps)}", truth=M - 1, map=int(est.map),
                posterior=[round(float(p), 6) for p in est.posterior], chains=len(est.chunks()), **summary(t))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--plants", type=int, default=4)
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--spot-horizon", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--state-sigma", type=float, default=1e-3, help="the estimators' state_sigma: the recorded states are noise-free")
    ap.add_argument("--tasks", default="leap_cube,fr3_pick,spot_box_push")
    a = ap.parse_args()
    for task_name in a.tasks.split(","):
        if task_name == "spot_box_push":
            print(json.dumps(spot_case(a.plants, a.windows, a.spot_horizon, a.reps, a.runs, a.state_sigma)), flush=True)
        else:
            print(json.dumps(model_set_case(task_name, a.plants, a.windows, a.horizon, a.reps, a.runs, a.state_sigma)), flush=True)


if __name__ == "__main__":
    main()
