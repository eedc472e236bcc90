"""B plan steps in one launch against B plan steps back to back: `ControllerFleet.update_action()` (one jh_plan_step_batch) timed against update_action() of the
same B controllers one after the other, in one process, on the shipped rollout counts (32) and the BASELINE horizons (64 steps).

    python tools/diag/plan_batch_sweep.py [--tasks cartpole,cylinder_push,leap_cube] [--batches 1,8,64] [--out plan_batch_sweep.md]

Wall clock of the whole call, host work included: that is what a user with B robots waits for.  Both forms run in every rep, in alternating order, so that clock and thermal drift
hit both alike; medians over the reps.  For leap_cube the table also gives the waves the batched rollout launch keeps resident (the latency mode is chosen from B * N
rollouts; the GPU holds two waves of the kernel per SIMD)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from judo_amd.fleet import make_controller_fleet  # noqa: E402

N, H = 32, 64


def leap_waves(B: int, n: int, cus: int) -> tuple[int, int, int]:
    """(latency shift, waves of the batched leap launch, waves the GPU holds at once) -- the launcher's rule (jh_latency_shift, rollout_cost_batch of jh_engine_v5.hip)."""
    shift = next((s for s in (2, 1) if ((B * n) << s) <= cus * 4 * 4), 0)
    per_block = (4 >> shift) * 4
    return shift, B * ((n + per_block - 1) // per_block) * 4, 8 * cus


def configure(fleet, task: str) -> None:
    for i, c in enumerate(fleet):
        c.optimizer.config.num_rollouts = N
        c.controller_cfg.horizon = H * c.task.dt
        np.random.seed(i)
        c.reset()
        c.optimizer.seed(100 + i)
        rng = np.random.default_rng(i)
        c.current_state = c.task.default_state() + 0.02 * rng.standard_normal(c.task.nq + c.task.nv)
        if task == "leap_cube":
            q = rng.standard_normal(4)
            c.system_metadata = {"goal_quat": q / np.linalg.norm(q)}


def measure(task: str, B: int, reps: int, warmup: int) -> dict:
    fleet = make_controller_fleet(task, "mppi", B)
    configure(fleet, task)
    t, batch, seq = 0.0, [], []
    for r in range(warmup + reps):
        for c in fleet:
            c.time = t
        for first in ((0, 1) if r % 2 == 0 else (1, 0)):  # (the order alternates: whichever form runs second finds the clocks already up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if first == 0:
                fleet.update_action()
            else:
                for c in fleet:
                    c.update_action()
            dt = time.perf_counter() - t0
            if r >= warmup:
                (batch if first == 0 else seq).append(dt)
        t += 0.02
    assert all(np.isfinite(c.nominal_knots).all() for c in fleet)
    out = dict(task=task, B=B, N=N, H=H, reps=reps, batch_ms=1e3 * float(np.median(batch)), sequential_ms=1e3 * float(np.median(seq)), batch_min_ms=1e3 * float(np.min(batch)),
               sequential_min_ms=1e3 * float(np.min(seq)))
    out["speedup"] = out["sequential_ms"] / out["batch_ms"]
    if task == "leap_cube":
        out["latency_shift"], out["launch_waves"], out["resident_wave_slots"] = leap_waves(B, N, torch.cuda.get_device_properties(0).multi_processor_count)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", default="cartpole,cylinder_push,leap_cube")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for task in args.tasks.split(","):
        for B in (int(b) for b in args.batches.split(",")):
            slow = task == "leap_cube"
            row = measure(task, B, reps=(7 if B >= 64 else 15) if slow else 100, warmup=2 if slow else 10)
            print(json.dumps(row), flush=True)
            rows.append(row)
    lines = ["| task | B | batch, median ms | B sequential steps, median ms | sequential / batch | per problem in the batch, ms | leap launch: shift, waves / resident slots |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        leap = f"{r['latency_shift']}, {r['launch_waves']} / {r['resident_wave_slots']}" if "launch_waves" in r else ""
        lines.append(f"| {r['task']} | {r['B']} | {r['batch_ms']:.3f} | {r['sequential_ms']:.3f} | {r['speedup']:.2f} | {r['batch_ms'] / r['B']:.4f} | {leap} |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
