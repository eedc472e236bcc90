"""Times of B domain-randomised plan steps in one launch against the way the library already had to run them (profiles/randomized_fleet.md), through the C ABI alone:
  fleet        ONE jh_plan_step_randomized_batch: B blocks, B noise slices, a shared set of M images, B tables of G entries, grid (workgroups of N / G rollouts, G, B),
               one tail on (tail workgroups, B)
  singles_a/b  B back-to-back jh_plan_step_randomized calls on the same blocks, noise, set and tables, then their B completion marks -- twice per repetition: the A / A
               spread of the session, which is the margin the comparison has
  one_a/b      ONE jh_plan_step_randomized call (controller 0's): what a single plan step costs, twice per repetition likewise
All legs run in one process, alternating within every repetition; a time is the host clock around the call(s) and jh_download_end.  What the legs compute is compared
too: the fleet's costs and nominals are the singles', bit for bit.
Shapes: cartpole N = 32, 4096 and leap_cube N = 32, 1024; H = 64, K = 4, MPPI; B = 1, 2, 4, 8, 16; M = G = 4 (members: pole mass, or cube mass and friction, scaled per
member); controller b's table is [(g + b) % M for g in range(G)].
usage: python tools/diag/randomized_fleet_sweep.py [--reps N] [--tasks cartpole,leap_cube] [--out FILE]

    python tools/diag/randomized_fleet_sweep.py --arg-block [--lib PATH/libjudo_amd.so] [--reps N] [--out FILE]
The cost of the kernel-argument block of the batched rollout kernels, which carries the table by value: jh_plan_step_batch on cartpole (B = 8, N = 32) and
jh_plan_step_randomized on cartpole (N = 32, M = G = 4), both H = 64, each leg twice per repetition.  `--lib` times another build of the library (the parent commit's)
with the same script: run the two builds in alternating processes of one session and compare the medians beside each build's own a / b difference."""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = {"cartpole": (32, 4096), "leap_cube": (32, 1024)}
FLEET = (1, 2, 4, 8, 16)
M = G = 4
H, K = 64, 4
MPPI = (0, 0.05, 0, 0)


def load(path):
    """The library: the tree's own through the shim, or another build of it with the shim's signatures for the symbols it has."""
    from judo_amd import _lib

    if path is None:
        return _lib.lib()
    L = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib._SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


class Problems:
    """M model handles of `task_name` (member 0 shipped, the others scaled), and B packed blocks and noise slices for N rollouts."""

    def __init__(self, L, dev, task_name):
        import torch

        from judo_amd.models import pack_model, scaled_description
        from judo_amd.spline import spline_weights
        from judo_amd.tasks import get_registered_tasks

        self.L, self.dev, self.task = L, dev, get_registered_tasks()[task_name][0]()
        task = self.task
        self.nu, self.nx = task.nu, task.nq + task.nv
        self.KU = K * self.nu
        body, geom = ("pole", None) if task_name == "cartpole" else ("cube", "cube")
        self.handles = []
        for i, f in enumerate(np.linspace(0.7, 1.5, M)):
            desc = task.desc if i == 0 else scaled_description(task.desc, body_mass={body: f}, geom_friction={geom: 2.0 - f} if geom else None)
            blob = pack_model(desc)
            h = C.c_void_p()
            assert L.jh_model_create(C.create_string_buffer(blob, len(blob)), len(blob), 0, C.byref(h)) == 0, L.jh_last_error()
            if task_name == "leap_cube":
                assert L.jh_model_set_contact_capacity(h, 48) == 0
            self.handles.append(h)
        self.mset = C.c_void_p()
        assert L.jh_model_set_create((C.c_void_p * M)(*[h.value for h in self.handles]), M, C.byref(self.mset)) == 0, L.jh_last_error()
        self.tp = np.asarray(task.task_params({}), dtype=np.float32)
        sizes = [self.nx, self.KU, self.KU, len(self.tp), 2 * self.nu]
        self.off = [int(v) for v in np.cumsum([0] + sizes)]
        self.nblk = self.off[-1]
        r = task.actuator_ctrlrange
        self.lohi = np.nan_to_num(np.concatenate([r[:, 0], r[:, 1]]).astype(np.float32), posinf=3.0e38, neginf=-3.0e38)
        self.warm = np.tile(np.asarray(task.optimizer_warm_start(), dtype=np.float64), (K, 1)).reshape(-1)
        self.W = torch.from_numpy(spline_weights("linear", np.linspace(0, H * task.dt, K), task.dt * np.arange(H)).astype(np.float32)).to(dev)

    def buffers(self, B, N):
        import torch

        rng = np.random.default_rng(1)
        blocks = np.stack([np.concatenate([np.asarray(self.task.default_state(), dtype=np.float32), (self.warm + 0.05 * rng.standard_normal(self.KU)).astype(np.float32),
                                           np.full(self.KU, 0.1, dtype=np.float32), self.tp, self.lohi]) for _ in range(B)])
        self.blk = torch.from_numpy(blocks).to(self.dev)
        self.noise = torch.from_numpy(rng.standard_normal((B, self.KU, N)).astype(np.float32)).to(self.dev)
        self.per = int(self.L.jh_update_fused_scratch_floats(N, K, self.nu))
        self.costs = torch.zeros((B, N), dtype=torch.float32, device=self.dev)
        self.out = torch.zeros((B, 2 * self.KU), dtype=torch.float32, device=self.dev)
        self.scratch = torch.zeros(B * self.per, dtype=torch.float32, device=self.dev)
        self.tables = [[(g + b) % M for g in range(G)] for b in range(B)]
        self.table_c = (C.c_ubyte * (B * G))(*[p for t in self.tables for p in t])
        self.rows_c = [(C.c_ubyte * G)(*t) for t in self.tables]

    def randomized(self, b, N):
        """jh_plan_step_randomized of controller b on its slices of the buffers (no wait)."""
        L, p, o, off, KU = self.L, self.blk.data_ptr() + 4 * b * self.nblk, self.out.data_ptr() + 8 * b * self.KU, self.off, self.KU
        st = L.jh_plan_step_randomized(self.mset, p, p, 4 * self.nblk, off[1], off[2], off[3], off[4], self.noise.data_ptr() + 4 * b * KU * N, N, self.W.data_ptr(), N, H, K, self.rows_c[b], G,
                                       self.costs.data_ptr() + 4 * b * N, *MPPI, self.scratch.data_ptr() + 4 * b * self.per, o, o, None, 0)
        assert st == 0, L.jh_last_error()

    def fleet(self, B, N):
        L, p, o, off, KU = self.L, self.blk.data_ptr(), self.out.data_ptr(), self.off, self.KU
        st = L.jh_plan_step_randomized_batch(self.mset, B, M, p, p, 4 * self.nblk, 4 * self.nblk, off[1], off[2], off[3], off[4], self.noise.data_ptr(), N, KU * N, self.W.data_ptr(), N, H, K,
                                             self.table_c, G, self.costs.data_ptr(), *MPPI, self.scratch.data_ptr(), o, 2 * KU, o, None, 0)
        assert st == 0, L.jh_last_error()

    def plan_step_batch(self, B, N):
        """jh_plan_step_batch of the B problems on member 0's handle (no wait)."""
        L, p, o, off, KU = self.L, self.blk.data_ptr(), self.out.data_ptr(), self.off, self.KU
        st = L.jh_plan_step_batch(self.handles[0], B, p, p, 4 * self.nblk, 4 * self.nblk, off[1], off[2], off[3], off[4], self.noise.data_ptr(), N, KU * N, self.W.data_ptr(), N, H, K,
                                  self.costs.data_ptr(), None, *MPPI, 0, 0, 0, self.scratch.data_ptr(), o, 2 * KU, o, None, 0)
        assert st == 0, L.jh_last_error()

    def wait(self, ends):
        for _ in range(ends):
            assert self.L.jh_download_end() == 0, self.L.jh_last_error()


def stats(t):
    t = np.asarray(t)
    return {"median_ms": float(np.median(t)), "p25_ms": float(np.percentile(t, 25)), "p75_ms": float(np.percentile(t, 75)), "min_ms": float(t.min())}


def timed(legs, run, reps, warmup=3):
    """Every leg `reps` times, alternating within a repetition (forwards, then backwards); returns the legs' times in ms."""
    for name in legs:
        for _ in range(warmup):
            run(name)
    times = {name: [] for name in legs}
    for rep in range(reps):
        for name in (legs if rep % 2 == 0 else legs[::-1]):
            t0 = time.perf_counter()
            run(name)
            times[name].append(1e3 * (time.perf_counter() - t0))
    return times


def sweep(L, dev, args):
    import torch

    results = []
    for task_name in args.tasks.split(","):
        pr = Problems(L, dev, task_name)
        for N in SHAPES[task_name]:
            for B in FLEET:
                reps = max(6, min(args.reps, args.reps * 2048 // (B * N)))
                pr.buffers(B, N)

                def run(name):
                    if name == "fleet":
                        pr.fleet(B, N); pr.wait(1)
                    elif name.startswith("singles"):
                        for b in range(B):
                            pr.randomized(b, N)
                        pr.wait(B)
                    else:
                        pr.randomized(0, N); pr.wait(1)

                bits = {}
                for name in ("fleet", "singles_a"):  # what the two forms compute
                    pr.costs.zero_(); pr.out.zero_()
                    run(name)
                    torch.cuda.synchronize()
                    bits[name] = pr.costs.cpu().numpy().tobytes() + pr.out.cpu().numpy().tobytes()
                legs = ["fleet", "singles_a", "singles_b", "one_a", "one_b"]
                times = timed(legs, run, reps)
                torch.cuda.synchronize()
                row = {"task": task_name, "B": B, "M": M, "G": G, "N": N, "H": H, "K": K, "rollouts": B * N, "reps": reps}
                for name in legs:
                    row[name] = stats(times[name])
                singles = 0.5 * (row["singles_a"]["median_ms"] + row["singles_b"]["median_ms"])
                one = 0.5 * (row["one_a"]["median_ms"] + row["one_b"]["median_ms"])
                row["singles_a_vs_b_median_ms"] = abs(row["singles_a"]["median_ms"] - row["singles_b"]["median_ms"])
                row["one_a_vs_b_median_ms"] = abs(row["one_a"]["median_ms"] - row["one_b"]["median_ms"])
                row["fleet_over_singles"] = row["fleet"]["median_ms"] / singles
                row["fleet_over_one"] = row["fleet"]["median_ms"] / one
                row["fleet_equals_singles_bits"] = bool(bits["fleet"] == bits["singles_a"])
                results.append(row)
                print(json.dumps(row), flush=True)
    return results


def arg_block(L, dev, args):
    """The two calls whose rollout kernels take the plant axis by value, at the sizes where a launch costs most of the call."""
    import torch

    pr = Problems(L, dev, "cartpole")
    B, N = 8, 32
    pr.buffers(B, N)

    def run(name):
        if name.startswith("plan_step_batch"):
            pr.plan_step_batch(B, N)
        else:
            pr.randomized(0, N)
        pr.wait(1)

    legs = ["plan_step_batch_a", "randomized_a", "plan_step_batch_b", "randomized_b"]
    times = timed(legs, run, args.reps, warmup=50)
    torch.cuda.synchronize()
    row = {"lib": args.lib or "tree", "task": "cartpole", "B": B, "N": N, "H": H, "K": K, "M": M, "G": G, "reps": args.reps}
    for name in legs:
        row[name] = stats(times[name])
    print(json.dumps(row), flush=True)
    return [row]


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=None, help="repetitions at the smallest launch (default 100; larger launches run fewer, never below 6); --arg-block: of every leg (default 4000)")
    ap.add_argument("--tasks", default="cartpole,leap_cube")
    ap.add_argument("--arg-block", action="store_true")
    ap.add_argument("--lib", default=None, help="--arg-block: another build of libjudo_amd.so to time instead of the tree's")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.reps = args.reps or (4000 if args.arg_block else 100)
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    L = load(args.lib if args.arg_block else None)
    results = arg_block(L, dev, args) if args.arg_block else sweep(L, dev, args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
