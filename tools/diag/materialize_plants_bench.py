"""What the materialise launch on a plant axis costs (`jh_rollout_materialize_plants`, judo_amd/materialized.py; `jh_fr3_rollout_materialize_plants`,
judo_amd/fr3_materialized.py); profiles/materialize_plants.md and profiles/fr3_materialize_plants.md are written from it.

    python tools/diag/materialize_plants_bench.py launch [--family leap|fr3] [--plants 4] [--reps 20] [--runs 5]
        One plants launch of G blocks against G single-image launches back to back, the same rollouts: leap_cube and cartpole at their shipped rollout counts and
        horizons (MPPI's overrides), and leap_cube at 4 x 8192 x H 64.  HIP events around `reps` repetitions on one stream; one JSON line per case.
        `--family fr3`: fr3_pick at its shipped 64 x 250 (CEM's overrides) and at 4 x 8192 x H 40, through the arm's entry.
    python tools/diag/materialize_plants_bench.py plan [--family leap|fr3] [--forms plain,randomized,ensemble] [--plants 4] [--steps 100] [--warmup 10] [--runs 3]
        The plan step of a plugin-reward leap_cube task (a torch reward of its own: the materialise path) as a plain `Controller`, as a
        `MaterializedRandomizedController` over the plants in as many blocks and as a `MaterializedEnsembleController`: wall clock of `update_action()` closed by a device
        synchronisation, the mean of `steps` plan steps after `warmup`, `runs` times each.  A tree without judo_amd/materialized.py measures the plain form alone, so
        the same file measures the parent commit (run it from that tree's root).
        `--family fr3`: the same of a plugin-reward fr3_pick task with CEM and the makers of judo_amd/fr3_materialized.py (a tree without that module: plain alone).
    python tools/diag/materialize_plants_bench.py resources [BUILD_DIR]
        Registers, spills, scratch, LDS and argument bytes of every instantiation of k_leap_v5, k_materialize and k_fr3_v6 in BUILD_DIR's object files (no GPU)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())  # (the tree the command is run from: `plan` also times a checkout of another commit)


def descriptions(task_name: str, M: int) -> list[dict]:
    from judo_amd.models import scaled_description
    from judo_amd.tasks import get_registered_tasks

    base = get_registered_tasks()[task_name][0]().desc
    if task_name == "fr3_pick":  # an unknown cube and gripper: mass 0.6 .. 1.7 of the nominal, pad friction 1.3 .. 0.6, gain 1.1 .. 0.9, plant 0 nominal
        return [base] + [scaled_description(base, body_mass={"object": float(m)}, geom_friction={"box": float(f)}, actuator_kp={None: float(k)})
                         for m, f, k in zip(np.linspace(0.6, 1.7, max(M - 1, 1))[: M - 1], np.linspace(1.3, 0.6, max(M - 1, 1))[: M - 1], np.linspace(1.1, 0.9, max(M - 1, 1))[: M - 1])]
    if task_name == "cartpole":  # an unknown pole: 0.6 .. 1.7 of the nominal mass
        return [base] + [scaled_description(base, body_mass={"pole": float(m)}) for m in np.linspace(0.6, 1.7, max(M - 1, 1))[: M - 1]]
    # an unknown cube: mass 0.6 .. 1.7 of the nominal, friction 1.3 .. 0.6, plant 0 nominal
    return [base] + [scaled_description(base, body_mass={"cube": float(m)}, geom_friction={"cube": float(f)})
                     for m, f in zip(np.linspace(0.6, 1.7, max(M - 1, 1))[: M - 1], np.linspace(1.3, 0.6, max(M - 1, 1))[: M - 1])]


# ---------------------------------------------------------------------------------------------------------------------------------------- launch cost
def launch_case(task_name: str, M: int, n: int, H: int, reps: int, runs: int) -> dict:
    import ctypes as C

    import torch

    from judo_amd import _lib
    from judo_amd.device import GpuModel, GpuModelSet, current_stream_ptr
    from judo_amd.tasks import get_registered_tasks

    dev = torch.device("cuda", 0)
    task = get_registered_tasks()[task_name][0]()
    models = [GpuModel(d, dev) for d in descriptions(task_name, M)]
    mset = GpuModelSet(models)
    L, gm = _lib.lib(), models[0]
    rng = np.random.default_rng(0)
    x0 = torch.from_numpy(np.asarray(task.default_state(), dtype=np.float32)).to(dev)
    hold = np.asarray(task.default_state(), dtype=np.float32)[7:23] if gm.nu == 16 else np.zeros(gm.nu, dtype=np.float32)
    spread = 0.2
    if task_name == "fr3_pick":  # the home joint targets, the spread of the task's CEM override
        hold, spread = np.asarray(task.reset_command, dtype=np.float32), 0.05
    controls = torch.from_numpy((hold + spread * rng.standard_normal((M * n, H, gm.nu))).astype(np.float32)).to(dev)
    states = torch.empty((M * n, H, gm.nx), dtype=torch.float32, device=dev)
    sensors = torch.empty((M * n, H, gm.ns), dtype=torch.float32, device=dev)
    table = (C.c_int * M)(*range(M))

    entry = "jh_fr3_rollout_materialize_plants" if mset.fr3 else "jh_rollout_materialize_plants"

    def plants():
        _lib.check(getattr(L, entry)(mset.handle, table, M, n, x0.data_ptr(), 0, controls.data_ptr(), 0, H, states.data_ptr(), sensors.data_ptr(), current_stream_ptr()),
                   entry)

    def singles():
        for g in range(M):
            r = slice(g * n, (g + 1) * n)
            _lib.check(L.jh_rollout_materialize(models[g].handle, x0.data_ptr(), 0, controls[r].data_ptr(), n, H, states[r].data_ptr(), sensors[r].data_ptr(), current_stream_ptr()),
                       "jh_rollout_materialize")

    def timed(fn) -> float:
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    singles()
    ref = (states.clone(), sensors.clone())
    plants()
    torch.cuda.synchronize()
    same = bool(torch.equal(states, ref[0]) and torch.equal(sensors, ref[1]))
    p, s = [timed(plants) for _ in range(runs)], [timed(singles) for _ in range(runs)]
    return dict(case=f"{task_name} {M} x {n} x H {H}", plants_ms=[round(v, 4) for v in p], singles_ms=[round(v, 4) for v in s], plants_median_ms=round(float(np.median(p)), 4),
                singles_median_ms=round(float(np.median(s)), 4), ratio=round(float(np.median(p) / np.median(s)), 3), bit_identical=same)


def launch(a) -> None:
    from judo_amd.controller import make_controller

    if a.family == "fr3":
        c = make_controller("fr3_pick", "cem")
        print(json.dumps(launch_case("fr3_pick", a.plants, int(c.optimizer.num_rollouts), int(c.num_timesteps), a.reps, a.runs)), flush=True)
        print(json.dumps(launch_case("fr3_pick", 4, 8192, 40, max(2, a.reps // 5), a.runs)), flush=True)
        return
    for task_name in ("leap_cube", "cartpole"):
        c = make_controller(task_name, "mppi")
        print(json.dumps(launch_case(task_name, a.plants, int(c.optimizer.num_rollouts), int(c.num_timesteps), a.reps, a.runs)), flush=True)
    print(json.dumps(launch_case("leap_cube", 4, 8192, 64, max(2, a.reps // 5), a.runs)), flush=True)


# ---------------------------------------------------------------------------------------------------------------------------------------- plan step
def plugin_task():
    """A third-party task on the leap_cube model with a torch reward of its own: keep the cube where it is, a small control penalty."""
    import torch

    from judo_amd.tasks import get_registered_tasks

    class CubeKeeper(get_registered_tasks()["leap_cube"][0]):
        def reward(self, states, sensors, controls, system_metadata=None):
            target = torch.tensor([0.0, 0.03, 0.1], dtype=states.dtype, device=states.device)
            d = states[..., :3] - target
            return -((d * d).sum(-1).sum(-1) + 1e-3 * (controls * controls).sum(-1).sum(-1))

    return CubeKeeper()


def plugin_fr3_task():
    """A third-party task on the fr3_pick model with a torch reward of its own: bring the cube over the goal, a small control penalty."""
    import torch

    from judo_amd.tasks import FR3Pick

    class CubeToGoal(FR3Pick):
        def reward(self, states, sensors, controls, system_metadata=None):
            goal = torch.tensor([0.6, 0.4, 0.3], dtype=states.dtype, device=states.device)
            d = states[..., :3] - goal
            return -((d * d).sum(-1).sum(-1) + 1e-3 * (controls * controls).sum(-1).sum(-1))

    return CubeToGoal()


def make(form: str, M: int, family: str = "leap"):
    from judo_amd.controller import make_controller_for

    if family == "fr3":
        if form == "plain":
            return make_controller_for(plugin_fr3_task(), "cem")
        from judo_amd.fr3_materialized import make_fr3_materialized_ensemble_controller, make_fr3_materialized_randomized_controller

        if form == "randomized":
            return make_fr3_materialized_randomized_controller(plugin_fr3_task(), "cem", descriptions("fr3_pick", M), blocks=M)
        return make_fr3_materialized_ensemble_controller(plugin_fr3_task(), "cem", descriptions("fr3_pick", M))
    if form == "plain":
        return make_controller_for(plugin_task(), "mppi")
    from judo_amd.materialized import make_materialized_ensemble_controller, make_materialized_randomized_controller

    if form == "randomized":
        return make_materialized_randomized_controller(plugin_task(), "mppi", descriptions("leap_cube", M), blocks=M)
    return make_materialized_ensemble_controller(plugin_task(), "mppi", descriptions("leap_cube", M))


def run(c, steps: int, warmup: int, seed: int) -> float:
    import torch

    rng = np.random.default_rng(seed)
    c.reset()
    c.optimizer.seed(seed)
    x0 = np.array(c.task.default_state(), dtype=np.float64)
    total = 0.0
    for i in range(warmup + steps):
        x = x0.copy()
        arm = slice(7, 14) if c.task.name == "fr3_pick" else slice(7, 23)
        x[arm] += 0.01 * rng.standard_normal(arm.stop - arm.start)  # no two steps alike
        c.update_states(x[: c.task.nq], x[c.task.nq :], i * c.task.dt, {} if c.task.name == "fr3_pick" else {"goal_quat": np.array([1.0, 0.0, 0.0, 0.0])})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.update_action()
        torch.cuda.synchronize()
        if i >= warmup:
            total += time.perf_counter() - t0
    return 1e3 * total / steps


def plan(a) -> None:
    have = os.path.exists(os.path.join(os.getcwd(), "judo_amd", "fr3_materialized.py" if a.family == "fr3" else "materialized.py"))
    for form in a.forms.split(","):
        if form != "plain" and not have:
            continue
        c = make(form, a.plants, a.family)
        c.solver_warnings = False
        assert not c.uses_fused_cost
        means = [run(c, a.steps, a.warmup, seed=r) for r in range(a.runs)]
        print(json.dumps(dict(family=a.family, form=form, members=1 if form == "plain" else a.plants, rollouts=int(c.optimizer.num_rollouts), horizon_steps=int(c.num_timesteps), steps=a.steps,
                              run_means_ms=[round(m, 3) for m in means], mean_ms=round(float(np.mean(means)), 3), spread_ms=round(max(means) - min(means), 3))), flush=True)


# ---------------------------------------------------------------------------------------------------------------------------------------- code objects
def resources(a) -> None:
    import tempfile

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import isa_compare as ic

    tmp = tempfile.mkdtemp()
    for f in ("jh_engine_v5.o", "jh_engine_v5_cap64.o", "jh_engine_v5_cyl.o", "jh_simple.o", "jh_engine_v6.o", "jh_engine_v6_self.o"):
        co = ic.code_object(os.path.join(a.build_dir, f), os.path.join(tmp, f))
        for sym, fig in ic.notes(co).items():
            name = ic.short(sym)
            if name.startswith("k_leap_v5<") or name.startswith("k_materialize<") or name.startswith("k_fr3_v6<"):
                print(json.dumps(dict(object=f, kernel=name, **fig)), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    p = sub.add_parser("launch"); p.add_argument("--family", choices=["leap", "fr3"], default="leap"); p.add_argument("--plants", type=int, default=4); p.add_argument("--reps", type=int, default=20); p.add_argument("--runs", type=int, default=5)
    p = sub.add_parser("plan"); p.add_argument("--family", choices=["leap", "fr3"], default="leap"); p.add_argument("--forms", default="plain,randomized,ensemble"); p.add_argument("--plants", type=int, default=4)
    p.add_argument("--steps", type=int, default=100); p.add_argument("--warmup", type=int, default=10); p.add_argument("--runs", type=int, default=3)
    p = sub.add_parser("resources"); p.add_argument("build_dir", nargs="?", default=os.path.join(os.getcwd(), "build"))
    a = ap.parse_args()
    {"launch": launch, "plan": plan, "resources": resources}[a.what](a)


if __name__ == "__main__":
    main()
