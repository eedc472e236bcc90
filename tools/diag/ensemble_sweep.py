"""Times of the ensemble plan step against the two ways the library already had to roll N candidates out on M plants (profiles/ensemble.md), through the C ABI alone:
  ensemble   jh_plan_step_ensemble on a set of M images: one block, one noise slice, grid (workgroups, M), one aggregating tail
  singles    M back-to-back jh_plan_step calls on the members' own handles (the same block and noise), then their M completion marks
  batch_a/b  jh_plan_step_batch_models of M problems at the same N -- M copies of the block and of the noise, M tails -- twice per repetition: the A / A spread of the
             session, which is the margin any comparison with it has
All legs run in one process on the same buffers, alternating within every repetition; a time is the host clock around the call(s) and jh_download_end.  What the legs
compute is compared too: the ensemble's member costs are the batch's costs, bit for bit (the problems of the batch are given the ensemble's block and noise).
Shapes: cartpole N = 32, 4096 and leap_cube N = 32, 1024, 4096, H = 64, K = 4, MPPI, M = 1, 2, 4, 8, 16 (members: pole mass, or cube mass and friction, scaled per member).
usage: python tools/diag/ensemble_sweep.py [--reps N] [--tasks cartpole,leap_cube] [--out FILE]"""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = {"cartpole": (32, 4096), "leap_cube": (32, 1024, 4096)}
MEMBERS = (1, 2, 4, 8, 16)
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
        for N in SHAPES[task_name]:
            rng = np.random.default_rng(1)
            block = np.concatenate([np.asarray(task.default_state(), dtype=np.float32), (warm + 0.05 * rng.standard_normal(KU)).astype(np.float32), np.full(KU, 0.1, dtype=np.float32), tp, lohi])
            noise1 = rng.standard_normal((KU, N)).astype(np.float32)
            per = int(L.jh_update_fused_scratch_floats(N, K, nu))
            for M in MEMBERS:
                reps = max(10, min(args.reps, args.reps * 2048 // (M * N)))
                hs = (C.c_void_p * M)(*[h.value for h in handles[:M]])
                mset = C.c_void_p()
                assert L.jh_model_set_create(hs, M, C.byref(mset)) == 0, L.jh_last_error()
                blk = torch.from_numpy(np.tile(block, (M, 1))).to(dev)  # (the batch's M blocks and noise slices: copies of the ensemble's one)
                noise = torch.from_numpy(np.tile(noise1, (M, 1, 1))).to(dev)
                member = torch.zeros((M, N), dtype=torch.float32, device=dev)
                costs = torch.zeros((M, N), dtype=torch.float32, device=dev)
                agg = torch.zeros(N, dtype=torch.float32, device=dev)
                out = torch.zeros((M, 2 * KU), dtype=torch.float32, device=dev)
                scratch = torch.zeros(M * per, dtype=torch.float32, device=dev)
                p, o = blk.data_ptr(), out.data_ptr()
                mppi = (0, 0.05, 0, 0)

                def leg(name):
                    t0 = time.perf_counter()
                    if name == "ensemble":
                        st = L.jh_plan_step_ensemble(mset, p, p, 4 * nblk, off[1], off[2], off[3], off[4], noise.data_ptr(), N, W.data_ptr(), N, H, K, member.data_ptr(), agg.data_ptr(), M, *mppi,
                                                     scratch.data_ptr(), o, o, None, 0)
                        assert st == 0, L.jh_last_error()
                        ends = 1
                    elif name == "singles":
                        for b in range(M):
                            st = L.jh_plan_step(handles[b], p, p, 4 * nblk, off[1], off[2], off[3], off[4], noise.data_ptr(), N, W.data_ptr(), 0, N, 0, H, K, costs.data_ptr() + 4 * b * N, None, None,
                                                *mppi, 0, 0, 0, scratch.data_ptr() + 4 * b * per, o + 8 * b * KU, o + 8 * b * KU, None, 0)
                            assert st == 0, L.jh_last_error()
                        ends = M
                    else:
                        st = L.jh_plan_step_batch_models(mset, p, p, 4 * nblk, 4 * nblk, off[1], off[2], off[3], off[4], noise.data_ptr(), N, KU * N, W.data_ptr(), N, H, K, costs.data_ptr(), None,
                                                         *mppi, 0, 0, 0, scratch.data_ptr(), o, 2 * KU, o, None, 0)
                        assert st == 0, L.jh_last_error()
                        ends = 1
                    for _ in range(ends):
                        assert L.jh_download_end() == 0, L.jh_last_error()
                    return 1e3 * (time.perf_counter() - t0)

                legs = ["ensemble", "singles", "batch_a", "batch_b"]
                bits = {}
                for name in legs:  # warm-up, and what each leg computes
                    for _ in range(3):
                        leg(name)
                    torch.cuda.synchronize()
                    bits[name] = (member if name == "ensemble" else costs).cpu().numpy().copy()
                times = {name: [] for name in legs}
                for rep in range(reps):
                    for name in (legs if rep % 2 == 0 else legs[::-1]):
                        times[name].append(leg(name))
                torch.cuda.synchronize()
                row = {"task": task_name, "M": M, "N": N, "H": H, "K": K, "reps": reps}
                for name in legs:
                    t = np.asarray(times[name])
                    row[name] = {"median_ms": float(np.median(t)), "p25_ms": float(np.percentile(t, 25)), "p75_ms": float(np.percentile(t, 75)), "min_ms": float(t.min())}
                batch = 0.5 * (row["batch_a"]["median_ms"] + row["batch_b"]["median_ms"])
                row["batch_a_vs_b_median_ms"] = abs(row["batch_a"]["median_ms"] - row["batch_b"]["median_ms"])
                row["ensemble_over_batch"] = row["ensemble"]["median_ms"] / batch
                row["ensemble_over_singles"] = row["ensemble"]["median_ms"] / row["singles"]["median_ms"]
                row["member_costs_equal_batch_bits"] = bool(bits["ensemble"].tobytes() == bits["batch_a"].tobytes())
                row["member_costs_equal_singles_bits"] = bool(bits["ensemble"].tobytes() == bits["singles"].tobytes())
                results.append(row)
                print(json.dumps(row), flush=True)
                L.jh_model_set_destroy(mset)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
