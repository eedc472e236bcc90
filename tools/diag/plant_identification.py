"""What identifying the plant costs (judo_amd/identify.py, `jh_plant_residuals`); profiles/plant_identification.md is written from it.

    python tools/diag/plant_identification.py [--plants 4] [--windows 16] [--horizon 8] [--state-sigma 1e-3] [--reps 20] [--runs 5]

For leap_cube and fr3_pick, a set of `plants` perturbed plants and `windows` recorded windows of `horizon` model steps (rolled out on the last plant's own handle, so that
plant is the truth), one JSON line each with, in ms, the median of `runs` measurements (all of them listed beside it):
    update_ms      one `PlantEstimator.update()`: the one materialise launch on the set, one `jh_plant_residuals` call, the (M, W) errors to the host, the posterior.
                   Wall clock of `reps` calls in a row (each ends with the download, which waits for the device).
    singles_ms     what it replaces: M single launches (`jh_rollout_materialize` on every plant's own handle), the M * W * H states to the host, the errors there
                   (`plant_residuals_host`) and the posterior.  Wall clock likewise; the tool first checks that both give the same errors bit for bit.
    plan_step_ms   one plan step of the randomised controller over the same plants at the task's shipped rollout count and horizon (`update_action()` closed by a
                   device synchronisation), the mean of `reps` steps after 3 warm-up steps.
    launch_ms, residuals_ms   the two stages of the update alone, HIP events around `reps` repetitions on one stream: the materialise launch on the set, and the
                   `jh_plant_residuals` call with the download of the (M, W) errors behind it."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from materialize_plants_bench import descriptions  # noqa: E402  (the plants of profiles/materialize_plants.md and fr3_materialize_plants.md)


def case(task_name: str, M: int, W: int, H: int, reps: int, runs: int, sigma: float) -> dict:
    import torch

    from judo_amd.device import GpuModel, GpuModelSet
    from judo_amd.identify import PlantEstimator, plant_residuals_host, posterior_from_errors
    from judo_amd.rollout_backend import GpuRolloutBackend
    from judo_amd.tasks import get_registered_tasks

    dev = torch.device("cuda", 0)
    task = get_registered_tasks()[task_name][0]()
    descs = descriptions(task_name, M)
    models = [GpuModel(d, dev) for d in descs]
    mset = GpuModelSet(models)
    gm = models[0]
    rng = np.random.default_rng(0)
    x0 = np.tile(np.asarray(task.default_state(), dtype=np.float32), (W, 1))
    hold, spread = (np.asarray(task.reset_command, dtype=np.float32), 0.05) if task_name == "fr3_pick" else (x0[0, 7:23], 0.2)
    controls = (hold + spread * rng.standard_normal((W, H, gm.nu))).astype(np.float32)
    backends = [GpuRolloutBackend(m, W) for m in models]
    if task_name != "fr3_pick":  # let the cube come to rest in the hand first (100 steps on the nominal plant, the fingers held): in free fall its mass and friction tell nothing
        held = torch.from_numpy(np.tile(hold, (1, 100, 1)).astype(np.float32)).to(dev)
        x0 = np.tile(backends[0].rollout_device(torch.from_numpy(x0[0]).to(dev), held, want_sensors=False)[0][0, -1].cpu().numpy(), (W, 1))
    x0_d, controls_d = torch.from_numpy(x0).to(dev), torch.from_numpy(controls).to(dev)
    truth = backends[-1].rollout_device(x0_d, controls_d, want_sensors=False)[0].cpu().numpy()
    est = PlantEstimator(mset, horizon=H, windows=W, state_sigma=sigma)
    for w in range(W):
        est.observe(x0[w], controls[w], truth[w])

    def singles():
        pred = np.concatenate([b.rollout_device(x0_d, controls_d, want_sensors=False)[0].cpu().numpy() for b in backends])
        err = plant_residuals_host(pred, truth, est.weight, est.quat_adr, nq=est.nq)
        return err, posterior_from_errors(err, est.prior, est.temperature, est.discount)[0]

    def wall(fn, n=reps) -> float:
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    def events(fn) -> float:
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    post = est.update()
    err_host, post_host = singles()
    same = bool(np.array_equal(est.errors.view(np.uint32), err_host.view(np.uint32)) and np.array_equal(post, post_host))
    pred, obs = est._predict()
    update = [wall(est.update) for _ in range(runs)]
    single = [wall(singles) for _ in range(runs)]
    launch = [events(est._predict) for _ in range(runs)]
    resid = [events(lambda: est._residuals(pred, obs)) for _ in range(runs)]

    if task_name == "fr3_pick":
        from judo_amd.fr3_randomized import make_fr3_randomized_controller

        ctrl = make_fr3_randomized_controller("cem", descs)
    else:
        from judo_amd.randomized import make_randomized_controller

        ctrl = make_randomized_controller(task_name, "mppi", descs)
    ctrl.reset()
    ctrl.current_state = ctrl.task.default_state()
    for _ in range(3):
        ctrl.update_action()
    plan = [wall(ctrl.update_action) for _ in range(runs)]
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    return dict(case=f"{task_name} M {M} x W {W} x H {H}", errors_bit_identical=same, map=int(est.map), truth=M - 1, posterior=[round(float(p), 6) for p in post],
                update_ms=med(update), update_runs=[round(v, 4) for v in update], singles_ms=med(single), singles_runs=[round(v, 4) for v in single],
                launch_ms=med(launch), launch_runs=[round(v, 4) for v in launch], residuals_ms=med(resid), residuals_runs=[round(v, 4) for v in resid],
                plan_step=f"{type(ctrl).__name__} {int(ctrl.optimizer.num_rollouts)} x H {int(ctrl.num_timesteps)}", plan_step_ms=med(plan), plan_step_runs=[round(v, 4) for v in plan])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--plants", type=int, default=4)
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--state-sigma", type=float, default=1e-3, help="the estimator's state_sigma: the recorded states are noise-free")
    ap.add_argument("--tasks", default="leap_cube,fr3_pick")
    a = ap.parse_args()
    for task_name in a.tasks.split(","):
        print(json.dumps(case(task_name, a.plants, a.windows, a.horizon, a.reps, a.runs, a.state_sigma)), flush=True)


if __name__ == "__main__":
    main()
