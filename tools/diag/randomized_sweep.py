"""Times of the domain-randomised plan step against what the library already had for the same N rollouts (profiles/randomized.md), through the C ABI alone:
  randomized   jh_plan_step_randomized on a set of M images, G = M blocks of N / M rollouts, block g on plant g: grid (workgroups of a block, M), the single call's tail
  single_a/b   jh_plan_step on plant 0 at the same N -- the yardstick: for leap_cube the queue and the horizon slices where the launch is large enough for them, for
               cartpole the one-launch form -- twice per repetition: the A / A spread of the session, which is the margin any comparison with it has
  slices       what a user does today: M back-to-back jh_plan_step calls on N / M rollouts each (plant g, the block's columns of the noise, n_offset = g N / M), then
               their M completion marks; the host would still have to stitch the M updates
  ensemble1    cartpole only: jh_plan_step_ensemble on a set of one plant, the two-launch form of the same plan step
All legs run in one process on the same buffers, alternating within every repetition; a time is the host clock around the call(s) and jh_download_end.  What the legs
compute is compared too: the randomised call's costs are the slices' costs stitched, bit for bit, and at M = 1 the single call's.
Shapes: leap_cube N = 32, 1024, 4096, 65536 and cartpole N = 32, 4096; H = 64, K = 4, MPPI, M = G = 1, 2, 4, 8 (members: pole mass, or cube mass and friction, scaled).
usage: python tools/diag/randomized_sweep.py [--reps N] [--tasks cartpole,leap_cube] [--out FILE]"""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = {"cartpole": (32, 4096), "leap_cube": (32, 1024, 4096, 65536)}
MEMBERS = (1, 2, 4, 8)
H, K = 64, 4


def main():
    import torch

    from judo_amd import _lib
    from judo_amd.models import pack_model, scaled_description
    from judo_amd.spline import spline_weights
    from judo_amd.tasks import get_registered_tasks

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="repetitions at the smallest launch; larger launches run fewer (never below 10)")
    ap.add_argument("--tasks", default="cartpole,leap_cube")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    L = _lib.lib()
    results = []
    for task_name in args.tasks.split(","):
        task = get_registered_tasks()[task_name][0]()
        nu, nx = task.nu, task.nq + task.nv
        KU = K * nu
        factors = np.linspace(0.7, 1.5, max(MEMBERS))
        body, geom = ("pole", None) if task_name == "cartpole" else ("cube", "cube")
        handles = []
        for i, f in enumerate(factors):  # member 0 is the shipped description
            desc = task.desc if i == 0 else scaled_description(task.desc, body_mass={body: f}, geom_friction={geom: 2.0 - f} if geom else None)
            blob = pack_model(desc)
            h = C.c_void_p()
            assert L.jh_model_create(C.create_string_buffer(blob, len(blob)), len(blob), 0, C.byref(h)) == 0, L.jh_last_error()
            if task_name == "leap_cube":
                assert L.jh_model_set_contact_capacity(h, 48) == 0
            handles.append(h)
        tp = np.asarray(task.task_params({}), dtype=np.float32)
        sizes = [nx, KU, KU, len(tp), 2 * nu]
        off = [int(v) for v in np.cumsum([0] + sizes)]
        nblk = off[-1]
        r = task.actuator_ctrlrange
        lohi = np.nan_to_num(np.concatenate([r[:, 0], r[:, 1]]).astype(np.float32), posinf=3.0e38, neginf=-3.0e38)
        warm = np.tile(np.asarray(task.optimizer_warm_start(), dtype=np.float64), (K, 1)).reshape(-1)
        W = torch.from_numpy(spline_weights("linear", np.linspace(0, H * task.dt, K), task.dt * np.arange(H)).astype(np.float32)).to(dev)
        one = (C.c_void_p * 1)(handles[0].value)
        set1 = C.c_void_p()
        assert L.jh_model_set_create(one, 1, C.byref(set1)) == 0, L.jh_last_error()
        for N in SHAPES[task_name]:
            rng = np.random.default_rng(1)
            block = np.concatenate([np.asarray(task.default_state(), dtype=np.float32), (warm + 0.05 * rng.standard_normal(KU)).astype(np.float32), np.full(KU, 0.1, dtype=np.float32), tp, lohi])
            blk = torch.from_numpy(block).to(dev)
            noise = torch.from_numpy(rng.standard_normal((KU, N)).astype(np.float32)).to(dev)
            per = int(L.jh_update_fused_scratch_floats(N, K, nu))
            reps = max(10, min(args.reps, args.reps * 2048 // N))
            for M in MEMBERS:
                Nb = N // M
                hs = (C.c_void_p * M)(*[h.value for h in handles[:M]])
                mset = C.c_void_p()
                assert L.jh_model_set_create(hs, M, C.byref(mset)) == 0, L.jh_last_error()
                table = (C.c_ubyte * M)(*range(M))
                costs = torch.zeros(N, dtype=torch.float32, device=dev)
                member = torch.zeros(N, dtype=torch.float32, device=dev)
                out = torch.zeros((M, 2 * KU), dtype=torch.float32, device=dev)
                scratch = torch.zeros(M * per, dtype=torch.float32, device=dev)
                p, o = blk.data_ptr(), out.data_ptr()
                mppi = (0, 0.05, 0, 0)

                def leg(name):
                    t0 = time.perf_counter()
                    ends = 1
                    if name == "randomized":
                        st = L.jh_plan_step_randomized(mset, p, p, 4 * nblk, off[1], off[2], off[3], off[4], noise.data_ptr(), N, W.data_ptr(), N, H, K, table, M, costs.data_ptr(), *mppi,
                                                       scratch.data_ptr(), o, o, None, 0)
                    elif name == "slices":
                        for g in range(M):
                            st = L.jh_plan_step(handles[g], p, p, 4 * nblk, off[1], off[2], off[3], off[4], noise.data_ptr() + 4 * g * Nb, N, W.data_ptr(), 0, Nb, g * Nb, H, K,
                                                costs.data_ptr() + 4 * g * Nb, None, None, *mppi, 0, 0, 0, scratch.data_ptr() + 4 * g * per, o + 8 * g * KU, o + 8 * g * KU, None, 0)
                            assert st == 0, L.jh_last_error()
                        ends = M
                    elif name == "ensemble1":
                        st = L.jh_plan_step_ensemble(set1, p, p, 4 * nblk, off[1], off[2], off[3], off[4], noise.data_ptr(), N, W.data_ptr(), N, H, K, member.data_ptr(), costs.data_ptr(), 1, *mppi,
                                                     scratch.data_ptr(), o, o, None, 0)
                    else:
                        st = L.jh_plan_step(handles[0], p, p, 4 * nblk, off[1], off[2], off[3], off[4], noise.data_ptr(), N, W.data_ptr(), 0, N, 0, H, K, costs.data_ptr(), None, None, *mppi, 0, 0, 0,
                                            scratch.data_ptr(), o, o, None, 0)
                    assert st == 0, L.jh_last_error()
                    for _ in range(ends):
                        assert L.jh_download_end() == 0, L.jh_last_error()
                    return 1e3 * (time.perf_counter() - t0)

                legs = ["randomized", "single_a", "single_b", "slices"] + (["ensemble1"] if task_name == "cartpole" else [])
                bits = {}
                for name in legs:  # warm-up, and what each leg computes
                    for _ in range(3):
                        leg(name)
                    torch.cuda.synchronize()
                    bits[name] = costs.cpu().numpy().copy()
                times = {name: [] for name in legs}
                for rep in range(reps):
                    for name in (legs if rep % 2 == 0 else legs[::-1]):
                        times[name].append(leg(name))
                torch.cuda.synchronize()
                row = {"task": task_name, "M": M, "N": N, "H": H, "K": K, "reps": reps}
                for name in legs:
                    t = np.asarray(times[name])
                    row[name] = {"median_ms": float(np.median(t)), "p25_ms": float(np.percentile(t, 25)), "p75_ms": float(np.percentile(t, 75)), "min_ms": float(t.min())}
                single = 0.5 * (row["single_a"]["median_ms"] + row["single_b"]["median_ms"])
                row["single_a_vs_b_median_ms"] = abs(row["single_a"]["median_ms"] - row["single_b"]["median_ms"])
                row["randomized_over_single"] = row["randomized"]["median_ms"] / single
                row["randomized_over_slices"] = row["randomized"]["median_ms"] / row["slices"]["median_ms"]
                if "ensemble1" in row:
                    row["randomized_over_ensemble1"] = row["randomized"]["median_ms"] / row["ensemble1"]["median_ms"]
                row["costs_equal_slices_bits"] = bool(bits["randomized"].tobytes() == bits["slices"].tobytes())
                if M == 1:
                    row["costs_equal_single_bits"] = bool(bits["randomized"].tobytes() == bits["single_a"].tobytes())
                results.append(row)
                print(json.dumps(row), flush=True)
                L.jh_model_set_destroy(mset)
        L.jh_model_set_destroy(set1)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
