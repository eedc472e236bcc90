"""Recorder of tests/golden/leap_broadphase_bits.npz: what the leap kernel (jh_engine_v5.hip and its 64-contact and cylinder builds) computes, word for word, from tangled
hand configurations -- the states in which the hand's broad phase has work on every level.  tests/test_gpu_leap_broadphase.py replays the recorded inputs and compares
uint32 views: a change of the broad phase's lane mapping must keep every candidate pair and its place in the list, and with them every bit of every output.

The fixture is the kernel's OWN output at a stated commit, recorded on an MI355X before the broad phase was touched; re-record only for a change that is meant to move bits.

  1. selection (a -DJH_V5_COUNT build of the library, selected with JUDO_AMD_LIB): candidate states are run in chunks of eight, and chunks are chosen so that the
     recorded rollout-steps meet the coverage conditions of the test (more than 16 box survivors at level 1, a body pair with more than 16 geom combinations, one near
     geom on either side, a step without a sphere survivor) with no contact dropped:
         JUDO_AMD_LIB=<count build> python tools/record_leap_broadphase_bits.py select --out selection.json
  2. recording (the product build):
         python tools/record_leap_broadphase_bits.py record --selection selection.json --commit <hash> --out tests/golden/leap_broadphase_bits.npz

This module is also the test's runner: `gpu_model`, `run_materialize`, `run_cost_traced` (the test imports them from here, so that recorder and test cannot drift apart).
"""

from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H = 8
CHUNK = 8
# name -> task, fingertips, rollouts, JUDO_AMD_LATENCY_SHIFT ("0": one rollout per row of a wave; None: the launcher's choice, rows computing copies at these sizes)
CASES = {
    "leap_cube": dict(task="leap_cube", fingertips="sphere", N=64, shift="0"),
    "leap_cube_down": dict(task="leap_cube_down", fingertips="sphere", N=32, shift="0"),
    "caltech_sphere": dict(task="caltech_leap_cube", fingertips="sphere", N=32, shift="0"),
    "caltech_cylinder": dict(task="caltech_leap_cube", fingertips="cylinder", N=32, shift="0"),
    "leap_cube_latency": dict(task="leap_cube", fingertips="sphere", N=8, shift=None),
}
COUNTERS = ("contact_overflow", "newton_cap_hits", "newton_iters", "steps", "wave_newton_iters", "wave_steps")
# stats[34..53] of a -DJH_V5_COUNT build (jh_engine_v5.hip)
CB = ("sph", "sph_wavemax", "box_wavemax", "l1_pair_passes", "l1_list_passes", "l2_trips", "bpairs", "T", "combo_passes", "cube_box_regions", "cube_box_lanes", "max_sph", "max_box",
      "max_T", "steps_no_sph", "pairs_one_A", "pairs_one_B", "own_trips", "steps_sph_over_cap", "fewest_sph_inv")
CONDITIONS = {"box_survivors_above_16": lambda c: c["max_box"] > 16, "combinations_above_16": lambda c: c["max_T"] > 16, "one_near_geom_A": lambda c: c["pairs_one_A"] > 0,
              "one_near_geom_B": lambda c: c["pairs_one_B"] > 0, "step_without_sphere_survivor": lambda c: c["steps_no_sph"] > 0}


@contextlib.contextmanager
def latency_shift(shift):
    old = os.environ.get("JUDO_AMD_LATENCY_SHIFT")
    if shift is None:
        os.environ.pop("JUDO_AMD_LATENCY_SHIFT", None)
    else:
        os.environ["JUDO_AMD_LATENCY_SHIFT"] = shift
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("JUDO_AMD_LATENCY_SHIFT", None)
        else:
            os.environ["JUDO_AMD_LATENCY_SHIFT"] = old


def gpu_model(case: dict):
    from judo_amd.device import GpuModel
    from judo_amd.models import load_description

    desc = load_description(case["task"])
    if case["fingertips"] == "cylinder":
        desc = dict(desc, fingertips="cylinder")
    gm = GpuModel(desc)
    assert gm.build()["cylinder_build"] == (case["fingertips"] == "cylinder") and gm.build()["contact_capacity"] == (48 if case["task"] == "leap_cube" else 64)
    return gm


def _counters(gm) -> np.ndarray:
    st = gm.stats()
    return np.array([st[k] for k in COUNTERS], dtype=np.int64)


def run_materialize(gm, x0: np.ndarray, U: np.ndarray, shift):
    """jh_rollout_materialize from per-rollout start states: (states, sensors, solver counters)."""
    import torch

    from judo_amd.rollout_backend import GpuRolloutBackend

    with latency_shift(shift):
        gm.stats()
        s, y = GpuRolloutBackend(gm, len(U)).rollout_device(torch.as_tensor(x0).cuda(), torch.as_tensor(U).cuda())
        torch.cuda.synchronize()
        return s.cpu().numpy(), y.cpu().numpy(), _counters(gm)


def run_cost_traced(gm, blk: dict, noise: np.ndarray, N: int, shift):
    """jh_rollout_cost_traced on a recorded device block (x0, nominal, sigma, W, lohi, tp as a plan step uploads them): (costs, trace rows, solver counters)."""
    import torch

    from judo_amd import _lib
    from judo_amd.device import current_stream_ptr

    t = {k: torch.as_tensor(np.ascontiguousarray(blk[k], dtype=np.float32)).cuda() for k in ("x0", "nominal", "sigma", "W", "lohi", "tp")}
    nz = torch.as_tensor(np.ascontiguousarray(noise, dtype=np.float32)).cuda()
    K, nu, ld = (int(v) for v in noise.shape)
    Hs = int(blk["W"].shape[0])
    nfl = gm.trace_layout()[1]
    costs = torch.full((N,), float("nan"), dtype=torch.float32, device="cuda")
    trace = torch.full((N * Hs * nfl,), float("nan"), dtype=torch.float32, device="cuda") if nfl else None
    with latency_shift(shift):
        gm.stats()
        st = _lib.lib().jh_rollout_cost_traced(gm.handle, _lib.ptr(t["x0"]), _lib.ptr(t["nominal"]), nz.data_ptr(), ld, _lib.ptr(t["sigma"]), _lib.ptr(t["W"]), _lib.ptr(t["lohi"]),
                                               _lib.ptr(t["tp"]), int(blk["phase"]), N, 0, Hs, K, _lib.ptr(costs), None, _lib.ptr(trace), current_stream_ptr())
        _lib.check(st, "jh_rollout_cost_traced")
        torch.cuda.synchronize()
        return costs.cpu().numpy(), (trace.cpu().numpy() if trace is not None else np.zeros(0, np.float32)), _counters(gm)


# ------------------------------------------------------------------------------------------------------------------------------ recorder only
def candidates(name: str):
    """Candidate start states and controls of a case, in chunks of CHUNK rows: tangled hands (tests/test_gpu_leap_self.py) from the home pose (frac 0) to uniformly random joint
    angles (frac 1), fingers clenched to either end of their ranges, joint angles anywhere on the circle, the cube parked away from the hand in every other chunk and at its home pose in the rest."""
    from judo_amd.tasks import get_registered_tasks
    from tests.test_gpu_leap_self import _tangled_states

    case = CASES[name]
    task = case["task"]
    home = np.asarray(get_registered_tasks()[task][0]().default_state(), dtype=np.float64)
    seed0 = 7000 + 100 * sorted(CASES).index(name if name != "leap_cube_latency" else "leap_cube")  # (the latency case draws from leap_cube's candidates)
    xs_all, q_all = [], []
    for fi, frac in enumerate((0.0, 0.3, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0)):
        om, xs, q = _tangled_states(6 * CHUNK, seed=seed0 + fi, frac=frac, task=task)
        xs_all.append(xs)
        q_all.append(q)
    rng = np.random.default_rng(seed0 + 50)
    r = np.array([a["ctrlrange"] for a in om.desc["actuators"]])
    for end in (0.02, 0.98, None):  # every joint near its lower / upper limit; each finger at one end or the other
        w = np.full((CHUNK, 16), end) if end is not None else np.repeat(rng.integers(0, 2, (CHUNK, 4)).astype(float), 4, axis=1) * 0.96 + 0.02
        q = r[:, 0] + (r[:, 1] - r[:, 0]) * np.clip(w + 0.02 * rng.uniform(-1, 1, (CHUNK, 16)), 0.0, 1.0)
        xs = np.zeros((CHUNK, 45))
        xs[:, 7:23] = q
        xs[:, 23:] = 0.2 * rng.standard_normal((CHUNK, 22))
        xs_all.append(xs)
        q_all.append(q)
    for _ in range(6):  # joint angles anywhere on the circle, far outside the joints' ranges (finite, not reachable), at rest: the search for a step in which no two bounding spheres overlap
        q = rng.uniform(-np.pi, np.pi, (CHUNK, 16))
        xs = np.zeros((CHUNK, 45))
        xs[:, 7:23] = q
        xs_all.append(xs)
        q_all.append(q)
    xs, q = np.concatenate(xs_all), np.concatenate(q_all)
    xs[:, :7] = home[:7]
    parked = (np.arange(len(xs)) // CHUNK) % 2 == 0
    xs[parked, 0 if task == "leap_cube_down" else 2] += 0.3
    U = q[:, None, :] + 0.3 * rng.standard_normal((len(xs), H, 16))
    return xs.astype(np.float32), U.astype(np.float32), q.astype(np.float32)


def _raw_counters(gm) -> dict:
    from judo_amd import _lib

    L = _lib.lib()
    L.jh_model_counters.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int]
    raw = (C.c_int * len(CB))()
    assert L.jh_model_counters(gm.handle, raw, 34, len(CB)) == 0
    return {k: int(v) for k, v in zip(CB, raw)}


def select(out: str) -> None:
    """Needs a -DJH_V5_COUNT build.  Chooses the chunks of every case and writes them, with the counters of every candidate chunk, to `out`."""
    sel = {}
    for name, case in CASES.items():
        gm = gpu_model(case)
        xs, U, _ = candidates(name)
        chunks = []
        for ci in range(len(xs) // CHUNK):
            rows = slice(ci * CHUNK, (ci + 1) * CHUNK)
            with latency_shift("0"):
                import torch
                from judo_amd.rollout_backend import GpuRolloutBackend

                gm.stats()
                s, y = GpuRolloutBackend(gm, CHUNK).rollout_device(torch.as_tensor(xs[rows]).cuda(), torch.as_tensor(U[rows]).cuda())
                torch.cuda.synchronize()
                c = _raw_counters(gm)
                st = gm.stats()
            c.update(chunk=ci, contact_overflow=int(st["contact_overflow"]), finite=bool(torch.isfinite(s).all() and torch.isfinite(y).all()), newton_cap_hits=int(st["newton_cap_hits"]))
            chunks.append(c)
        assert any(c["sph"] > 0 for c in chunks), "no counters: this is not a -DJH_V5_COUNT build"
        ok = [c for c in chunks if c["contact_overflow"] == 0 and c["finite"]]
        want = case["N"] // CHUNK
        chosen = []
        for cond, f in CONDITIONS.items():  # one chunk per condition first ...
            if not any(f(c) for c in chosen):
                hit = next((c for c in ok if f(c) and c not in chosen), None)
                if hit is not None and len(chosen) < want:
                    chosen.append(hit)
        for c in sorted(ok, key=lambda c: -c["T"]):  # ... then the chunks with the most level-2 work
            if len(chosen) < want and c not in chosen:
                chosen.append(c)
        assert len(chosen) == want, (name, len(ok))
        chosen.sort(key=lambda c: c["chunk"])
        sel[name] = {"chunks": [c["chunk"] for c in chosen], "coverage": {k: bool(any(f(c) for c in chosen)) for k, f in CONDITIONS.items()},
                     "max_box_survivors_any_candidate": max(c["max_box"] for c in chunks), "max_sphere_survivors_any_candidate": max(c["max_sph"] for c in chunks), "fewest_sphere_survivors_any_candidate": min(128 - c["fewest_sph_inv"] for c in chunks),
                     "candidate_chunks": chunks}
        print(name, sel[name]["chunks"], sel[name]["coverage"], "largest level-1 lists among all candidates: sphere", sel[name]["max_sphere_survivors_any_candidate"], "box",
              sel[name]["max_box_survivors_any_candidate"], "fewest sphere survivors", sel[name]["fewest_sphere_survivors_any_candidate"], "; chunks without dropped contacts:", len(ok), "of", len(chunks), flush=True)
    with open(out, "w") as f:
        json.dump(sel, f, indent=1)


def _plan_block(case: dict) -> tuple[dict, int, int]:
    """The device block of one small plan step of the case's controller (sigma, control bounds, task parameters, spline weights as the plan step uploads them)."""
    import torch

    from judo_amd.controller import make_controller, make_controller_for

    if case["fingertips"] == "cylinder":
        from judo_amd.tasks import CaltechLeapCube

        ctrl = make_controller_for(CaltechLeapCube(fingertips="cylinder"), "mppi")
    else:
        ctrl = make_controller(case["task"], "mppi")
    ctrl.optimizer.config.num_rollouts = 64
    ctrl.controller_cfg.horizon = H * ctrl.task.dt
    ctrl.reset()
    ctrl.current_state = ctrl.task.default_state()
    ctrl.update_action()
    torch.cuda.synchronize()
    b = ctrl._last_fused["b"]
    K, nu = ctrl.optimizer.num_nodes, ctrl.nu
    assert ctrl.num_timesteps == H
    blk = {k: getattr(b, k).detach().cpu().numpy().astype(np.float32).copy() for k in ("x0", "nominal", "sigma", "lohi", "tp")}
    blk["W"] = ctrl._weights(K, H).detach().cpu().numpy().astype(np.float32).reshape(H, K)
    blk["phase"] = int(ctrl.task.phase)
    return blk, K, nu


def record(selection: str, commit: str, out: str) -> None:
    sel = json.load(open(selection))
    import shutil

    hipcc = subprocess.run([shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.strip()
    data = {}
    meta = {"commit": commit, "hipcc": hipcc, "H": H, "counters": list(COUNTERS), "cases": {}}
    for name, case in CASES.items():
        gm = gpu_model(case)
        xs, U, q = candidates(name)
        rows = np.concatenate([np.arange(ci * CHUNK, (ci + 1) * CHUNK) for ci in sel[name]["chunks"]])
        x0, Us, qs = xs[rows], U[rows], q[rows]
        s, y, cm = run_materialize(gm, x0, Us, case["shift"])
        assert np.isfinite(s).all() and np.isfinite(y).all() and cm[0] == 0, (name, cm)
        blk, K, nu = _plan_block(case)
        noise = np.random.default_rng(17).standard_normal((K, nu, case["N"])).astype(np.float32)
        tangled = np.argsort(-np.abs(qs - qs.mean(0)).sum(1))  # start of the fused launch: the first of the recorded states (most unusual pose first) that drops no contact
        for j in tangled:
            blk["x0"] = x0[j].reshape(blk["x0"].shape).copy()
            blk["nominal"] = np.tile(qs[j], (K, 1)).reshape(blk["nominal"].shape).astype(np.float32)
            costs, trace, cc = run_cost_traced(gm, blk, noise, case["N"], case["shift"])
            if cc[0] == 0 and np.isfinite(costs).all():
                break
        else:
            raise AssertionError((name, "no start state of the fused launch without dropped contacts"))
        for k, v in (("x0", x0), ("U", Us), ("states", s.view(np.uint32)), ("sensors", y.view(np.uint32)), ("materialize_counters", cm), ("noise", noise), ("costs", costs.view(np.uint32)),
                     ("trace", trace.view(np.uint32)), ("cost_counters", cc)):
            data[f"{name}/{k}"] = v
        for k in ("x0", "nominal", "sigma", "lohi", "tp", "W"):
            data[f"{name}/blk_{k}"] = blk[k]
        meta["cases"][name] = {"phase": blk["phase"], "chunks": sel[name]["chunks"], "coverage": sel[name]["coverage"], "fused_start_row": int(j),
                               "materialize_counters": [int(v) for v in cm], "cost_counters": [int(v) for v in cc]}
        print(name, "materialize", dict(zip(COUNTERS, cm.tolist())), "fused", dict(zip(COUNTERS, cc.tolist())), "start row", int(j), flush=True)
    meta["coverage"] = {k: bool(any(m["coverage"][k] for m in meta["cases"].values())) for k in CONDITIONS}
    data["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **data)
    print("coverage", meta["coverage"], "->", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["select", "record"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--selection")
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    if a.what == "select":
        select(a.out)
    else:
        record(a.selection, a.commit, a.out)
