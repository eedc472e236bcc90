"""The plan step of spot_box_push (MPPI, the shipped 24 rollouts) as a plain `Controller`, as a `SpotRandomizedController` on M plants in M blocks and as a
`SpotEnsembleController` over M plants: the mean of `--steps` plan steps after `--warmup`, `--runs` times each, in one process.

    python tools/diag/spot_plants_bench.py [--forms plain,randomized,ensemble] [--members 4] [--steps 100] [--warmup 10] [--runs 5] [--cutoff shipped|none]

Wall clock of the whole `update_action()` call, host work included, closed by a device synchronisation.  Every plan step starts from the task's default state with the
box 0.95 m in front of the robot, moved by a few millimetres per step so that no two steps are alike, and advances the controller's time by one control period.  One JSON
line per form: the runs' means in milliseconds, their mean, and the spread (max - min) over the runs.  A tree without judo_amd/spot_plants.py measures the plain form alone,
so the same file measures the parent commit.  `--cutoff none` switches the 125 ms device-time deadline of the Spot rollout off; it never strikes at these sizes."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.getcwd())  # (the tree the command is run from: this file also times a checkout of another commit)
from judo_amd.controller import make_controller  # noqa: E402

TASK, OPT = "spot_box_push", "mppi"


def descriptions(M: int) -> list[dict]:
    from judo_amd.models import scaled_description
    from judo_amd.tasks import get_registered_tasks

    base = get_registered_tasks()[TASK][0]().desc
    # an unknown box: mass 0.6 .. 1.7 of the nominal, friction 1.0 .. 0.6, plant 0 nominal
    return [base] + [scaled_description(base, body_mass={"box_body": m}, geom_friction={"box_collision": f})
                     for m, f in zip(np.linspace(0.6, 1.7, max(M - 1, 1))[: M - 1], np.linspace(1.0, 0.6, max(M - 1, 1))[: M - 1])]


def make(form: str, M: int):
    if form == "plain":
        return make_controller(TASK, OPT)
    from judo_amd.spot_plants import make_spot_ensemble_controller, make_spot_randomized_controller

    if form == "randomized":
        return make_spot_randomized_controller(TASK, OPT, descriptions(M), blocks=M)
    return make_spot_ensemble_controller(TASK, OPT, descriptions(M))


def run(c, steps: int, warmup: int, seed: int) -> float:
    rng = np.random.default_rng(seed)
    c.reset()
    c.optimizer.seed(seed)
    x0 = np.array(c.task.default_state(), dtype=np.float64)
    x0[26:28] = [0.95, 0.0]
    total = 0.0
    for i in range(warmup + steps):
        x = x0.copy()
        x[26:28] += 0.005 * rng.standard_normal(2)
        c.update_states(x[: c.task.nq], x[c.task.nq :], i * c.task.dt, {})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.update_action()
        torch.cuda.synchronize()
        if i >= warmup:
            total += time.perf_counter() - t0
    return 1e3 * total / steps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default="plain,randomized,ensemble")
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cutoff", default="shipped", choices=["shipped", "none"])
    a = ap.parse_args()
    have_plants = os.path.exists(os.path.join(os.getcwd(), "judo_amd", "spot_plants.py"))
    for form in a.forms.split(","):
        if form != "plain" and not have_plants:
            continue
        c = make(form, a.members)
        c.solver_warnings = False
        if a.cutoff == "none":
            c.rollout_cutoff_time = None
        means = [run(c, a.steps, a.warmup, seed=r) for r in range(a.runs)]
        st = c.solver_stats()
        print(json.dumps(dict(form=form, members=1 if form == "plain" else a.members, rollouts=c.optimizer.num_rollouts, horizon_steps=c.num_timesteps, steps=a.steps,
                              run_means_ms=[round(m, 3) for m in means], mean_ms=round(float(np.mean(means)), 3), spread_ms=round(max(means) - min(means), 3),
                              contact_overflow=st["contact_overflow"], newton_cap_hits=st["newton_cap_hits"])), flush=True)


if __name__ == "__main__":
    main()
