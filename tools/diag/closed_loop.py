"""What the closed loop costs and what it shows (judo_amd/simulation.py, `jh_plants_advance`); writes profiles/closed_loop.md.

    python tools/diag/closed_loop.py [--plants 8] [--runs 7] [--reps 10] [--seeds 3] [--periods 150] [--out profiles/closed_loop.md]

  period     one control period of `plants` leap_cube and fr3_pick plants at their shipped steps_per_plan = round(1 / (control_freq * dt)): one `PlantFleet.advance`
             (host spline weights, two uploads, one jh_plants_advance call) against the same steps as plants * steps single-step jh_rollout_materialize launches on the
             plants' own handles, chained on the device, and against those launches with the host round trip per step that a hand-written loop makes.  Wall-clock ms
             around `reps` periods behind a warm-up, `runs` measurements, the forms alternating within a run.
  cold start one advance(2 S) against two advance(S) on leap_cube in contact: the largest state difference, per seed -- the solver starts cold at the top of a launch.
  returns    closed-loop returns of a plain, a randomised and a worst-case ensemble controller on a true plant at the edge of the set (cartpole, the heaviest pole),
             per seed."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from materialize_plants_bench import descriptions  # noqa: E402


def _start(task_name, task, gm, dev):
    """(x0 (nx,), hold (nu,)): leap_cube after the cube has come to rest in the hand, fr3_pick at its home state."""
    import torch

    from judo_amd.rollout_backend import GpuRolloutBackend

    x0 = np.asarray(task.default_state(), dtype=np.float32)
    if task_name == "fr3_pick":
        return x0, np.asarray(task.reset_command, dtype=np.float32)
    hold = x0[7:23].copy()
    held = torch.from_numpy(np.tile(hold, (1, 100, 1)).astype(np.float32)).to(dev)
    return GpuRolloutBackend(gm, 1).rollout_device(torch.from_numpy(x0).to(dev), held, want_sensors=False)[0][0, -1].cpu().numpy(), hold


def _splines(hold, spread, B, dt, S, seed, kind="cubic"):
    from judo_amd.structs import SplineData

    rng = np.random.default_rng(seed)
    return [SplineData(np.linspace(0.0, 4 * S * dt, 4), hold + spread * rng.standard_normal((4, hold.size)), kind) for _ in range(B)]


def period_case(task_name: str, B: int, runs: int, reps: int) -> dict:
    import torch

    from judo_amd import _lib
    from judo_amd.config import ControllerConfig
    from judo_amd.device import GpuModel, GpuModelSet, current_stream_ptr
    from judo_amd.simulation import PlantFleet, plant_controls_host, spline_rows
    from judo_amd.tasks import get_registered_tasks

    dev = torch.device("cuda", 0)
    task = get_registered_tasks()[task_name][0]()
    M = 4
    models = [GpuModel(d, dev) for d in descriptions(task_name, M)]
    mset, gm = GpuModelSet(models), models[0]
    cfg = ControllerConfig()
    cfg.set_override(task_name)
    S = max(1, int(round(1.0 / (cfg.control_freq * gm.dt))))
    x0, hold = _start(task_name, task, gm, dev)
    truth = [b % M for b in range(B)]
    splines = _splines(hold, 0.05, B, gm.dt, S, 0)
    fleet = PlantFleet(mset, truth, x0)
    controls = torch.from_numpy(plant_controls_host(*spline_rows(splines, np.zeros(B), gm.dt, 0, S))).to(dev)
    x_start = torch.from_numpy(np.tile(x0, (B, 1))).to(dev)
    nxt = [torch.empty((1, 1, gm.nx), dtype=torch.float32, device=dev) for _ in range(B)]
    lib = _lib.lib()

    def one_call():
        fleet.set_state(x0, time=0.0)
        fleet.advance(splines, S)

    def single_steps(round_trip: bool):
        for b in range(B):
            x = x_start[b]
            for s in range(S):
                _lib.check(lib.jh_rollout_materialize(models[truth[b]].handle, x.data_ptr(), 0, controls[b, s].data_ptr(), 1, 1, nxt[b].data_ptr(), None, current_stream_ptr()), "step")
                x = torch.from_numpy(nxt[b].cpu().numpy()[0, 0]).to(dev) if round_trip else nxt[b][0, 0].clone()

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / reps

    # the one call against each plant's own launch of the whole segment: the same bits.  Against the single steps it differs where there are contacts, because every
    # launch starts the solver cold: the largest difference is reported
    one_call()
    single_steps(False)
    whole = torch.empty((1, S, gm.nx), dtype=torch.float32, device=dev)
    same = True
    for b in range(B):
        _lib.check(lib.jh_rollout_materialize(models[truth[b]].handle, x_start[b].data_ptr(), 0, controls[b].data_ptr(), 1, S, whole.data_ptr(), None, current_stream_ptr()), "segment")
        same = same and torch.equal(fleet.states[b], whole[0])
    step_diff = max(float((fleet.states[b, -1] - nxt[b][0, 0]).abs().max()) for b in range(B))
    out = {"advance": [], "single_steps_device_chained": [], "single_steps_host_round_trip": []}
    for _ in range(runs):
        out["advance"].append(wall(one_call))
        out["single_steps_device_chained"].append(wall(lambda: single_steps(False)))
        out["single_steps_host_round_trip"].append(wall(lambda: single_steps(True)))
    res = {"case": "period", "task": task_name, "plants": B, "steps_per_plan": S, "same_bits_as_own_handle_segments": bool(same), "max_abs_difference_to_single_steps": step_diff}
    for k, v in out.items():
        res[k + "_ms"], res[k + "_runs"] = round(float(np.median(v)), 4), [round(x, 4) for x in v]
    return res


def cold_start_case(seeds: int) -> dict:
    import torch

    from judo_amd.device import GpuModel, GpuModelSet
    from judo_amd.simulation import PlantFleet
    from judo_amd.tasks import get_registered_tasks

    dev = torch.device("cuda", 0)
    task = get_registered_tasks()["leap_cube"][0]()
    gm = GpuModel(task.desc, dev)
    mset = GpuModelSet([gm])
    x0, hold = _start("leap_cube", task, gm, dev)
    S, B = 5, 8
    diffs = []
    for seed in range(seeds):
        splines = _splines(hold, 0.15, B, gm.dt, 2 * S, 100 + seed)
        whole, halves = PlantFleet(mset, [0] * B, x0), PlantFleet(mset, [0] * B, x0)
        whole.advance(splines, 2 * S)
        halves.advance(splines, S)
        first = halves.states.cpu().numpy()
        halves.advance(splines, S)
        a, b = whole.states.cpu().numpy(), np.concatenate([first, halves.states.cpu().numpy()], axis=1)
        diffs.append({"seed": 100 + seed, "first_half_equal": bool(np.array_equal(a[:, :S], b[:, :S])), "max_abs_qpos": float(np.abs(a[..., : gm.nq] - b[..., : gm.nq]).max()),
                      "max_abs_qvel": float(np.abs(a[..., gm.nq :] - b[..., gm.nq :]).max())})
    return {"case": "cold_start", "task": "leap_cube", "plants": B, "steps": S, "per_seed": diffs}


def returns_case(seeds: int, periods: int) -> dict:
    import torch

    from judo_amd.controller import make_controller
    from judo_amd.device import GpuModel, GpuModelSet
    from judo_amd.ensemble import make_ensemble_controller
    from judo_amd.randomized import make_randomized_controller
    from judo_amd.simulation import ClosedLoop, PlantFleet

    dev = torch.device("cuda", 0)
    M = 4
    descs = descriptions("cartpole", M)
    mset = GpuModelSet([GpuModel(d, dev) for d in descs])
    makers = {"plain": lambda: make_controller("cartpole", "mppi"), "randomized": lambda: make_randomized_controller("cartpole", "mppi", descs, blocks=M),
              "worst_case": lambda: make_ensemble_controller("cartpole", "mppi", descs, worst=1)}
    rows = {k: [] for k in makers}
    for seed in range(seeds):
        for kind, make in makers.items():
            c = make()
            c.optimizer.config.num_rollouts = 256
            np.random.seed(seed)
            c.reset()
            c.optimizer.seed(seed)
            loop = ClosedLoop([c], PlantFleet(mset, [M - 1], np.concatenate([c.task.data.qpos, c.task.data.qvel])), record=False)
            rows[kind].append(round(float(loop.run(periods)[0]), 3))
    return {"case": "returns", "task": "cartpole", "true_plant": M - 1, "pole_mass_scale": 1.7, "periods": periods, "rollouts": 256, "returns_per_seed": rows,
            "mean": {k: round(float(np.mean(v)), 3) for k, v in rows.items()}, "std": {k: round(float(np.std(v)), 3) for k, v in rows.items()}}


def markdown(results: list) -> str:
    lines = ["# The closed loop: one `advance` against single-step launches, the cold start, and returns on an edge plant", "",
             "Written by `tools/diag/closed_loop.py` on an MI355X; the JSON lines below are its output, the tables restate them.", ""]
    per = [r for r in results if r["case"] == "period"]
    if per:
        lines += ["## One control period", "", "Wall-clock ms per period, median of the runs (all runs in the JSON).", "",
                  "| task | plants | steps | one `advance` | B x S launches, device-chained | B x S launches, host round trip | ratio (chained / advance) | same bits as own-handle segments | max abs difference to single steps |", "|---|---|---|---|---|---|---|---|---|"]
        for r in per:
            lines.append(f"| {r['task']} | {r['plants']} | {r['steps_per_plan']} | {r['advance_ms']} | {r['single_steps_device_chained_ms']} | {r['single_steps_host_round_trip_ms']} | "
                         f"{r['single_steps_device_chained_ms'] / r['advance_ms']:.2f} | {r['same_bits_as_own_handle_segments']} | {r['max_abs_difference_to_single_steps']:.3e} |")
        lines.append("")
    for r in results:
        if r["case"] == "cold_start":
            lines += ["## The cold-start deviation", "", f"leap_cube in contact, {r['plants']} plants: one `advance({2 * r['steps']})` against two `advance({r['steps']})`.", "",
                      "| seed | first half equal | max abs qpos difference | max abs qvel difference |", "|---|---|---|---|"]
            lines += [f"| {d['seed']} | {d['first_half_equal']} | {d['max_abs_qpos']:.3e} | {d['max_abs_qvel']:.3e} |" for d in r["per_seed"]] + [""]
        if r["case"] == "returns":
            lines += ["## Returns on a plant at the edge of the set", "",
                      f"cartpole, the true plant is member {r['true_plant']} (pole mass x {r['pole_mass_scale']}), {r['periods']} control periods, {r['rollouts']} rollouts, MPPI.", "",
                      "| controller | returns per seed | mean | std |", "|---|---|---|---|"]
            lines += [f"| {k} | {v} | {r['mean'][k]} | {r['std'][k]} |" for k, v in r["returns_per_seed"].items()] + [""]
    lines += ["## JSON", "", "```"] + [json.dumps(r) for r in results] + ["```", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--plants", type=int, default=8)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--periods", type=int, default=150)
    ap.add_argument("--out", default=os.path.join("profiles", "closed_loop.md"))
    a = ap.parse_args()
    results = []
    for name in ("leap_cube", "fr3_pick"):
        results.append(period_case(name, a.plants, a.runs, a.reps))
        print(json.dumps(results[-1]), flush=True)
    results.append(cold_start_case(a.seeds))
    print(json.dumps(results[-1]), flush=True)
    results.append(returns_case(a.seeds, a.periods))
    print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(markdown(results))
