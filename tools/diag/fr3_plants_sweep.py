"""fr3_pick on a model set, timed: what a plant per problem and a plant per rollout block cost against the forms the tree already had.

    python tools/diag/fr3_plants_sweep.py [--configs shipped,baseline] [--batches 1,2,4,8,16] [--blocks 1,4,16] [--reps 30] [--out profiles/fr3_plants.md]

Two comparisons, each in one process on the reference's shipped configuration (CEM, 64 rollouts x 250 steps) and on the BASELINE one (CEM, 32 768 x 40):
  fleet        one `FR3PlantFleet.update_action()` (jh_plan_step_batch_phases_models, B arms on B plants cycling over D0..D3) against `update_action()` of B lone
               controllers on the same plants back to back, and against one `FR3Fleet.update_action()` of B arms on ONE image (jh_plan_step_batch_phases, stride 0);
  randomized   one `FR3RandomizedController.update_action()` with G rollout blocks over D0..D3 against one plain `Controller.update_action()`.
Wall clock of the whole call, host work included, around calls that end in the library's own wait (jh_download_end).  Every shape is warmed up first; then all forms run
in every rep, in rotating order, so that clock and thermal drift hit them alike.  Median and the 10th / 90th percentile over the reps: every figure stands beside its
own run-to-run spread.  The arms stand in the four phase states, cycling.

`--out`: a document with the lines `<!-- sweep:begin -->` / `<!-- sweep:end -->` gets the tables between them replaced; any other path receives the tables alone."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from judo_amd.controller import make_controller_for  # noqa: E402
from judo_amd.fr3_fleet import make_fr3_fleet  # noqa: E402
from judo_amd.fr3_randomized import make_fr3_randomized_controller  # noqa: E402
from judo_amd.models import layout, scaled_description  # noqa: E402
from judo_amd.tasks import FR3Pick  # noqa: E402

CONFIGS = {"shipped": (64, 250), "baseline": (32768, 40)}  # rollouts, horizon steps
CUBES = ([0.7, 0.0, 0.02], [0.7, 0.0, 0.05], [0.6, 0.4, 0.05], [0.6, 0.4, 0.02])
BEGIN, END = "<!-- sweep:begin -->", "<!-- sweep:end -->"


def plants() -> list[dict]:
    d0 = FR3Pick().desc
    return [d0, scaled_description(d0, body_mass={"object": 0.7}, actuator_kp={None: 1.1}),
            scaled_description(d0, body_mass={"object": 1.4}, geom_friction={"box": 0.6}, actuator_kp={None: 0.9}),
            scaled_description(d0, body_mass={"fr3_link7": 1.2, "hand": 1.2}, geom_friction={"table": 0.5})]


def lone_on(desc: dict):
    t = FR3Pick()
    t.desc = desc
    t._layout, t._ctrlrange, t._jadr = layout(desc), None, None
    return make_controller_for(t, "cem")


def configure(cs, n: int, h: int) -> None:
    for i, c in enumerate(cs):
        c.optimizer.config.num_rollouts = n
        c.controller_cfg.horizon = h * c.task.dt
        c.solver_warnings = False
        c.reset()
        c.optimizer.seed(100 + i)
        x = c.task.default_state()
        x[7:14] += 0.02 * np.random.default_rng(i).standard_normal(7)
        x[0:3] = CUBES[i % 4]
        c.current_state = x


def timed(forms: dict, clocks, reps: int, warmup: int) -> dict:
    """`forms`: name -> callable; every form runs in every rep, the order rotating.  `clocks`: the controllers whose time advances between the reps."""
    names = list(forms)
    got = {k: [] for k in names}
    t = 0.0
    for r in range(warmup + reps):
        for c in clocks:
            c.time = t
        for j in range(len(names)):
            name = names[(r + j) % len(names)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            forms[name]()
            dt = time.perf_counter() - t0
            if r >= warmup:
                got[name].append(dt)
        t += 0.02
    return {k: [1e3 * float(np.median(v)), 1e3 * float(np.percentile(v, 10)), 1e3 * float(np.percentile(v, 90))] for k, v in got.items()}


def measure_fleet(config: str, B: int, reps: int) -> dict:
    n, h = CONFIGS[config]
    d = plants()
    descs = [d[b % 4] for b in range(B)]
    plant_fleet, one_image = make_fr3_fleet("cem", B, descriptions=descs), make_fr3_fleet("cem", B)
    alone = [lone_on(x) for x in descs]
    for cs in (plant_fleet, one_image, alone):
        configure(cs, n, h)

    def back_to_back():
        for c in alone:
            c.update_action()

    ms = timed({"plant_fleet": plant_fleet.update_action, "back_to_back": back_to_back, "one_image_fleet": one_image.update_action}, list(plant_fleet) + list(one_image) + alone, reps, 3)
    assert all(np.isfinite(c.nominal_knots).all() for c in list(plant_fleet) + list(one_image) + alone)
    return dict(kind="fleet", config=config, B=B, N=n, H=h, reps=reps, **ms)


def measure_randomized(config: str, G: int, reps: int) -> dict:
    n, h = CONFIGS[config]
    rn, plain = make_fr3_randomized_controller("cem", plants(), blocks=G), make_controller_for(FR3Pick(), "cem")
    configure([rn], n, h)
    configure([plain], n, h)
    ms = timed({"randomized": rn.update_action, "plain": plain.update_action}, [rn, plain], reps, 3)
    assert np.isfinite(rn.nominal_knots).all() and np.isfinite(plain.nominal_knots).all()
    return dict(kind="randomized", config=config, G=G, N=n, H=h, reps=reps, **ms)


def cell(v) -> str:
    return f"{v[0]:.2f} ({v[1]:.2f} - {v[2]:.2f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="shipped,baseline")
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--blocks", default="1,4,16")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for config in args.configs.split(","):
        for B in (int(b) for b in args.batches.split(",") if b):
            rows.append(measure_fleet(config, B, args.reps))
            print(json.dumps(rows[-1]), flush=True)
        for G in (int(g) for g in args.blocks.split(",") if g):
            rows.append(measure_randomized(config, G, args.reps))
            print(json.dumps(rows[-1]), flush=True)
    lines = [f"`python tools/diag/fr3_plants_sweep.py --configs {args.configs} --batches {args.batches} --blocks {args.blocks} --reps {args.reps}` on {torch.cuda.get_device_name(0)}; CEM, "
             "wall clock in ms, median (10th - 90th percentile) over the reps.", "",
             "| configuration | B | one FR3PlantFleet.update_action() | one-image FR3Fleet.update_action() | B lone controllers back to back | plant fleet / one-image fleet | back to back / plant fleet |",
             "|---|---|---|---|---|---|---|"]
    for r in (r for r in rows if r["kind"] == "fleet"):
        lines.append(f"| {r['config']} {r['N']} x {r['H']} | {r['B']} | {cell(r['plant_fleet'])} | {cell(r['one_image_fleet'])} | {cell(r['back_to_back'])} | "
                     f"{r['plant_fleet'][0] / r['one_image_fleet'][0]:.3f} | {r['back_to_back'][0] / r['plant_fleet'][0]:.2f} |")
    lines += ["", "| configuration | G | one FR3RandomizedController.update_action() | one Controller.update_action() | randomised / plain |", "|---|---|---|---|---|"]
    for r in (r for r in rows if r["kind"] == "randomized"):
        lines.append(f"| {r['config']} {r['N']} x {r['H']} | {r['G']} | {cell(r['randomized'])} | {cell(r['plain'])} | {r['randomized'][0] / r['plain'][0]:.3f} |")
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
