"""B Spot plan steps as one launch chain against B plan steps back to back: `ControllerFleet.update_action()` on a Spot policy task (one jh_spline_controls_batch, one
jh_policy_rollout_batch, one jh_update_fused_batch, one wait) timed against update_action() of the same B controllers one after the other, in one process, MPPI on the
shipped 24 rollouts and 100 control steps, no rollout deadline (a deadline would cut both forms to the same 125 ms and hide the difference).

    python tools/diag/spot_fleet_sweep.py [--tasks spot_navigate,spot_box_push] [--batches 1,4,8,16] [--reps 7] [--split 8] [--sequential-only] [--out spot_fleet_sweep.md]

Wall clock of the whole call, host work included: that is what a user with B robots waits for.  Both forms run in every rep, in alternating order, so that clock and thermal
drift hit both alike; medians over the reps.  `--sequential-only` times the B back-to-back steps alone and needs no fleet: it runs on a commit that has none for Spot, to show
that the standalone path did not move.  `--split B`: one more fleet of B members per task whose iteration is bracketed with HIP events on the launch stream -- spline
(+ upload, noise) / command mapping + rollout / rewards (B x Task.reward in torch) / update -- by wrapping the bound library entries; medians over the reps, in ms.
A batch of more than 512 rollouts (B * 24 > 512, i.e. B >= 22) would move the policy step from one workgroup per rollout to the four per-layer launches (jh_policy.hip)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from judo_amd import _lib  # noqa: E402
from judo_amd.controller import make_controller  # noqa: E402

N, H = 24, 100


def configure(cs) -> None:
    for i, c in enumerate(cs):
        c.optimizer.config.num_rollouts = N
        c.controller_cfg.horizon = H * c.task.dt
        c.controller_cfg.max_opt_iters = 1
        c.rollout_cutoff_time = None
        np.random.seed(i)
        c.reset()
        c.optimizer.seed(100 + i)
        rng = np.random.default_rng(i)
        x = np.array(c.task.default_state(), dtype=np.float64)
        x[7:19] += 0.03 * rng.standard_normal(12)
        c.current_state = x
        goal = np.array(c.task.config.goal_position, dtype=np.float64)
        goal[:2] += rng.uniform(-2, 2, 2)
        c.task.config.goal_position = goal
        assert c.num_timesteps == H


def measure(task: str, B: int, reps: int, warmup: int, sequential_only: bool) -> dict:
    if sequential_only:
        fleet, cs = None, [make_controller(task, "mppi") for _ in range(B)]
    else:
        from judo_amd.fleet import make_controller_fleet

        fleet = make_controller_fleet(task, "mppi", B)
        cs = list(fleet)
    configure(cs)
    t, batch, seq = 0.0, [], []
    for r in range(warmup + reps):
        for c in cs:
            c.time = t
        forms = (1,) if sequential_only else ((0, 1) if r % 2 == 0 else (1, 0))  # (the order alternates: whichever form runs second finds the clocks already up)
        for form in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if form == 0:
                fleet.update_action()
            else:
                for c in cs:
                    c.update_action()
            dt = time.perf_counter() - t0
            if r >= warmup:
                (batch if form == 0 else seq).append(dt)
        t += 0.02
    assert all(np.isfinite(c.nominal_knots).all() for c in cs)
    out = dict(task=task, B=B, N=N, H=H, reps=reps, sequential_ms=1e3 * float(np.median(seq)), sequential_min_ms=1e3 * float(np.min(seq)))
    if batch:
        out.update(batch_ms=1e3 * float(np.median(batch)), batch_min_ms=1e3 * float(np.min(batch)), policy_launch="row" if B * N <= 512 else "layers")
        out["speedup"] = out["sequential_ms"] / out["batch_ms"]
    return out


def stage_split(task: str, B: int, reps: int, warmup: int) -> dict:
    """HIP events on the launch stream around the fleet iteration's stages: recorded in front of each of the three batched library calls and behind the last."""
    from judo_amd.fleet import make_controller_fleet

    fleet = make_controller_fleet(task, "mppi", B)
    configure(list(fleet))
    L = _lib.lib()
    marks: list = []

    def bracket(name, after=False):
        fn = getattr(L, name)

        def wrapper(*a):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append(ev)
            st = fn(*a)
            if after:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                marks.append(ev)
            return st

        setattr(L, name, wrapper)
        return fn

    saved = {name: bracket(name, after=(name != "jh_upload_async")) for name in ("jh_upload_async", "jh_spline_controls_batch", "jh_policy_rollout_batch", "jh_update_fused_batch")}
    rows, t = [], 0.0
    try:
        for r in range(warmup + reps):
            for c in fleet:
                c.time = t
            marks.clear()
            fleet.update_action()
            torch.cuda.synchronize()
            # marks: upload | spline in, out | rollout in, out | update in, out
            up, s0, s1, r0, r1, u0, u1 = marks
            if r >= warmup:
                rows.append([up.elapsed_time(s1), s1.elapsed_time(r1), r1.elapsed_time(u0), u0.elapsed_time(u1)])
            t += 0.02
    finally:
        for name, fn in saved.items():
            setattr(L, name, fn)
    med = np.median(np.array(rows), axis=0)
    return dict(task=task, B=B, spline_ms=float(med[0]), rollout_ms=float(med[1]), rewards_ms=float(med[2]), update_ms=float(med[3]))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", default="spot_navigate,spot_box_push")
    ap.add_argument("--batches", default="1,4,8,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--split", type=int, default=8)
    ap.add_argument("--sequential-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows, splits = [], []
    for task in args.tasks.split(","):
        for B in (int(b) for b in args.batches.split(",")):
            row = measure(task, B, reps=args.reps, warmup=2, sequential_only=args.sequential_only)
            print(json.dumps(row), flush=True)
            rows.append(row)
        if args.split > 0 and not args.sequential_only:
            sp = stage_split(task, args.split, reps=args.reps, warmup=2)
            print(json.dumps(sp), flush=True)
            splits.append(sp)
    if args.sequential_only:
        lines = ["| task | B | B sequential steps, median ms | min ms | per step, ms |", "|---|---|---|---|---|"]
        lines += [f"| {r['task']} | {r['B']} | {r['sequential_ms']:.2f} | {r['sequential_min_ms']:.2f} | {r['sequential_ms'] / r['B']:.2f} |" for r in rows]
    else:
        lines = ["| task | B | rollouts in the chain | policy launch | fleet, median ms | B sequential steps, median ms | sequential / fleet | per member in the fleet, ms |", "|---|---|---|---|---|---|---|---|"]
        lines += [f"| {r['task']} | {r['B']} | {r['B'] * N} | {r['policy_launch']} | {r['batch_ms']:.2f} | {r['sequential_ms']:.2f} | {r['speedup']:.2f} | {r['batch_ms'] / r['B']:.2f} |" for r in rows]
        if splits:
            lines += ["", "| task | B | upload + noise + spline, ms | command mapping + rollout, ms | rewards (B x Task.reward), ms | update, ms |", "|---|---|---|---|---|---|"]
            lines += [f"| {s['task']} | {s['B']} | {s['spline_ms']:.3f} | {s['rollout_ms']:.3f} | {s['rewards_ms']:.3f} | {s['update_ms']:.3f} |" for s in splits]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
