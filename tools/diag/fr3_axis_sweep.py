"""The fr3 launch's controller axis, timed: what B fr3_pick ensemble or randomised controllers in one launch cost against the same controllers back to back, and what one
ensemble controller over M plants costs against M plain plan steps.

    python tools/diag/fr3_axis_sweep.py [--configs shipped,baseline] [--batches 1,2,4,8] [--members 1,2,4] [--reps 20] [--out profiles/fr3_controller_axis.md]

Three comparisons, each in one process on the reference's shipped configuration (CEM, 64 rollouts x 250 steps) and on the BASELINE one (CEM, 32 768 x 40):
  ensemble fleet     one `FR3EnsembleFleet.update_action()` (jh_plan_step_ensemble_batch_phases: B arms, each against the M = 2 plants D0, D1, worst = 1) against
                     `update_action()` of B lone `FR3EnsembleController`s back to back;
  randomised fleet   one `FR3RandomizedFleet.update_action()` (jh_plan_step_randomized_batch_phases: B arms, each with G = 4 rollout blocks over D0..D3) against B lone
                     `FR3RandomizedController`s back to back;
  ensemble           one `FR3EnsembleController.update_action()` over M plants (jh_plan_step_ensemble_phase, worst = 1) against M plain `Controller.update_action()`, one
                     per plant, back to back.
Wall clock of the whole call, host work included, around calls that end in the library's own wait (jh_download_end).  Every shape is warmed up first; then all forms run
in every rep, in rotating order, so that clock and thermal drift hit them alike.  Median and the 10th / 90th percentile over the reps: every figure stands beside its
own run-to-run spread.  The arms stand in the four phase states, cycling.

`--out`: a document with the lines `<!-- sweep:begin -->` / `<!-- sweep:end -->` gets the tables between them replaced; any other path receives the tables alone."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from fr3_plants_sweep import BEGIN, CONFIGS, END, cell, configure, lone_on, plants, timed  # noqa: E402
from judo_amd.fr3_ensemble import make_fr3_ensemble_controller, make_fr3_ensemble_fleet  # noqa: E402
from judo_amd.fr3_randomized import make_fr3_randomized_controller  # noqa: E402
from judo_amd.fr3_randomized_fleet import make_fr3_randomized_fleet  # noqa: E402

FLEET_M, FLEET_G = 2, 4  # plants of an ensemble fleet's members; rollout blocks of a randomised fleet's members


def measure_pair(kind: str, config: str, B: int, reps: int) -> dict:
    n, h = CONFIGS[config]
    d = plants()
    if kind == "ensemble_fleet":
        fleet = make_fr3_ensemble_fleet("cem", B, d[:FLEET_M], worst=1)
        alone = [make_fr3_ensemble_controller("cem", d[:FLEET_M], worst=1) for _ in range(B)]
    else:
        fleet = make_fr3_randomized_fleet("cem", B, d, blocks=FLEET_G)
        alone = [make_fr3_randomized_controller("cem", d, blocks=FLEET_G) for _ in range(B)]
    for cs in (fleet, alone):
        configure(cs, n, h)

    def back_to_back():
        for c in alone:
            c.update_action()

    ms = timed({"fleet": fleet.update_action, "back_to_back": back_to_back}, list(fleet) + alone, reps, 3)
    assert all(np.isfinite(c.nominal_knots).all() for c in list(fleet) + alone)
    return dict(kind=kind, config=config, B=B, N=n, H=h, reps=reps, **ms)


def measure_ensemble(config: str, M: int, reps: int) -> dict:
    n, h = CONFIGS[config]
    d = plants()[:M]
    en, plain = make_fr3_ensemble_controller("cem", d, worst=1), [lone_on(x) for x in d]
    configure([en], n, h)
    configure(plain, n, h)

    def back_to_back():
        for c in plain:
            c.update_action()

    ms = timed({"ensemble": en.update_action, "plain": back_to_back}, [en] + plain, reps, 3)
    assert np.isfinite(en.nominal_knots).all() and all(np.isfinite(c.nominal_knots).all() for c in plain)
    return dict(kind="ensemble", config=config, M=M, N=n, H=h, reps=reps, **ms)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="shipped,baseline")
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--members", default="1,2,4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for config in args.configs.split(","):
        for kind in ("ensemble_fleet", "randomized_fleet"):
            for B in (int(b) for b in args.batches.split(",") if b):
                rows.append(measure_pair(kind, config, B, args.reps))
                print(json.dumps(rows[-1]), flush=True)
        for M in (int(m) for m in args.members.split(",") if m):
            rows.append(measure_ensemble(config, M, args.reps))
            print(json.dumps(rows[-1]), flush=True)
    lines = [f"`python tools/diag/fr3_axis_sweep.py --configs {args.configs} --batches {args.batches} --members {args.members} --reps {args.reps}` on {torch.cuda.get_device_name(0)}; CEM, "
             "wall clock in ms, median (10th - 90th percentile) over the reps."]
    for kind, fleet, lone in (("ensemble_fleet", f"one FR3EnsembleFleet.update_action() (M = {FLEET_M})", "B lone FR3EnsembleControllers back to back"),
                              ("randomized_fleet", f"one FR3RandomizedFleet.update_action() (G = {FLEET_G})", "B lone FR3RandomizedControllers back to back")):
        lines += ["", f"| configuration | B | {fleet} | {lone} | back to back / fleet | fleet / fleet of one |", "|---|---|---|---|---|---|"]
        for r in (r for r in rows if r["kind"] == kind):
            one = [q for q in rows if q["kind"] == kind and q["config"] == r["config"] and q["B"] == 1]
            lines.append(f"| {r['config']} {r['N']} x {r['H']} | {r['B']} | {cell(r['fleet'])} | {cell(r['back_to_back'])} | {r['back_to_back'][0] / r['fleet'][0]:.2f} | "
                         + (f"{r['fleet'][0] / one[0]['fleet'][0]:.2f} |" if one else "- |"))
    lines += ["", "| configuration | M | one FR3EnsembleController.update_action() | M plain Controller.update_action() back to back | plain / ensemble |", "|---|---|---|---|---|"]
    for r in (r for r in rows if r["kind"] == "ensemble"):
        lines.append(f"| {r['config']} {r['N']} x {r['H']} | {r['M']} | {cell(r['ensemble'])} | {cell(r['plain'])} | {r['plain'][0] / r['ensemble'][0]:.2f} |")
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
