"""B fr3_pick plan steps in one launch against B plan steps back to back: `FR3Fleet.update_action()` (one jh_plan_step_batch_phases) timed against update_action() of
the same B controllers one after the other, in one process, on the reference's shipped configuration (CEM, 64 rollouts x 250 steps) and on the BASELINE one
(CEM, 32 768 rollouts x 40 steps, where one controller already fills the GPU).

    python tools/diag/fr3_fleet_sweep.py [--configs shipped,baseline] [--batches 1,2,4,8,16] [--reps 50] [--out profiles/fr3_fleet.md]

Wall clock of the whole call, host work included, around calls that end in the library's own wait (jh_download_end): that is what a user with B arms waits for.  Every
shape is warmed up first; then both forms run in every rep, in alternating order, so that clock and thermal drift hit both alike.  Median and the 10th / 90th
percentile over the reps.  The members stand in the four phase states (LIFT, MOVE, PLACE, HOMING), cycling, so the launch carries every phase.

`--out`: a document with the lines `<!-- sweep:begin -->` / `<!-- sweep:end -->` gets the table between them replaced; any other path receives the table alone."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from judo_amd.fr3_fleet import make_fr3_fleet  # noqa: E402

CONFIGS = {"shipped": (64, 250), "baseline": (32768, 40)}  # rollouts, horizon steps
CUBES = ([0.7, 0.0, 0.02], [0.7, 0.0, 0.05], [0.6, 0.4, 0.05], [0.6, 0.4, 0.02])
BEGIN, END = "<!-- sweep:begin -->", "<!-- sweep:end -->"


def launch_shape(B: int, n: int, cus: int) -> tuple[int, int, int]:
    """(latency shift, one-wave workgroups of the batched launch, wave slots of the GPU at two waves per SIMD) -- the launcher's rule (jh_latency_shift, rollout_cost_batch of jh_engine_v6.hip)."""
    shift = next((s for s in (2, 1) if ((B * n) << s) <= cus * 4 * 4), 0)
    per_wave = 4 >> shift
    return shift, B * ((n + per_wave - 1) // per_wave), 8 * cus


def configure(fleet, n: int, h: int) -> None:
    for i, c in enumerate(fleet):
        c.optimizer.config.num_rollouts = n
        c.controller_cfg.horizon = h * c.task.dt
        c.solver_warnings = False
        c.reset()
        c.optimizer.seed(100 + i)
        x = c.task.default_state()
        x[7:14] += 0.02 * np.random.default_rng(i).standard_normal(7)
        x[0:3] = CUBES[i % 4]
        c.current_state = x


def measure(config: str, B: int, reps: int, warmup: int) -> dict:
    n, h = CONFIGS[config]
    fleet = make_fr3_fleet("cem", B)
    configure(fleet, n, h)
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
    ms = lambda v, f: 1e3 * float(f(v))  # noqa: E731
    out = dict(config=config, B=B, N=n, H=h, reps=reps, fleet_ms=ms(batch, np.median), fleet_p10_ms=ms(batch, lambda v: np.percentile(v, 10)), fleet_p90_ms=ms(batch, lambda v: np.percentile(v, 90)),
               sequential_ms=ms(seq, np.median), sequential_p10_ms=ms(seq, lambda v: np.percentile(v, 10)), sequential_p90_ms=ms(seq, lambda v: np.percentile(v, 90)))
    out["speedup"] = out["sequential_ms"] / out["fleet_ms"]
    out["latency_shift"], out["launch_waves"], out["resident_wave_slots"] = launch_shape(B, n, torch.cuda.get_device_properties(0).multi_processor_count)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="shipped,baseline")
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for config in args.configs.split(","):
        for B in (int(b) for b in args.batches.split(",")):
            row = measure(config, B, reps=args.reps, warmup=3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    lines = [f"`python tools/diag/fr3_fleet_sweep.py --configs {args.configs} --batches {args.batches} --reps {args.reps}` on {torch.cuda.get_device_name(0)}; CEM, wall clock in ms, "
             "median (10th - 90th percentile) over the reps.", "",
             "| configuration | B | one FR3Fleet.update_action() | B Controller.update_action() back to back | back to back / fleet | per arm in the fleet | launch: shift, waves / resident slots |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['config']} {r['N']} x {r['H']} | {r['B']} | {r['fleet_ms']:.2f} ({r['fleet_p10_ms']:.2f} - {r['fleet_p90_ms']:.2f}) | "
                     f"{r['sequential_ms']:.2f} ({r['sequential_p10_ms']:.2f} - {r['sequential_p90_ms']:.2f}) | {r['speedup']:.2f} | {r['fleet_ms'] / r['B']:.2f} | "
                     f"{r['latency_shift']}, {r['launch_waves']} / {r['resident_wave_slots']} |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        doc = open(args.out).read() if os.path.exists(args.out) else ""
        if BEGIN in doc and END in doc:
            text = doc[: doc.index(BEGIN) + len(BEGIN)] + "\n" + text + "\n" + doc[doc.index(END) :]
        else:
            text += "\n"
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
