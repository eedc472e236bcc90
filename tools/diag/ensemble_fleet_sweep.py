"""Times of B ensemble plan steps in one launch against the two ways the library already had to run them (profiles/ensemble_fleet.md), through the C ABI alone:
  fleet        ONE jh_plan_step_ensemble_batch: B blocks, B noise slices, a shared set of M images, grid (workgroups, M, B), one aggregating tail on (tail workgroups, B)
  singles_a/b  B back-to-back jh_plan_step_ensemble calls on the same blocks, noise and set, then their B completion marks -- twice per repetition: the A / A spread of the
               session, which is the margin the comparison has
  batch_a/b    one jh_plan_step_batch_models of B * M problems at the same N (a set of B * M images, B * M blocks, noise slices and tails): the floor a launch of that many
               rollouts has without the aggregation -- twice per repetition likewise
All legs run in one process, alternating within every repetition; a time is the host clock around the call(s) and jh_download_end.  What the legs compute is compared
too: the fleet's member costs, costs and nominals are the singles', bit for bit.
Shapes: cartpole N = 32, 4096 and leap_cube N = 32, 1024; H = 64, K = 4, MPPI; B = 1, 2, 4, 8, 16; M = 2, 4, 8 (members: pole mass, or cube mass and friction, scaled per
member); controller b plans with worst = 1 + b % M.
usage: python tools/diag/ensemble_fleet_sweep.py [--reps N] [--tasks cartpole,leap_cube] [--out FILE]"""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = {"cartpole": (32, 4096), "leap_cube": (32, 1024)}
FLEET = (1, 2, 4, 8, 16)
MEMBERS = (2, 4, 8)
H, K = 64, 4


def main():
    import torch

    from judo_amd import _lib
    from judo_amd.models import pack_model, scaled_description
    from judo_amd.spline import spline_weights
    from judo_amd.tasks import get_registered_tasks

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100, help="repetitions at the smallest launch; larger launches run fewer (never below 6)")
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
            per = int(L.jh_update_fused_scratch_floats(N, K, nu))
            for M in MEMBERS:
                hs = (C.c_void_p * M)(*[h.value for h in handles[:M]])
                mset = C.c_void_p()
                assert L.jh_model_set_create(hs, M, C.byref(mset)) == 0, L.jh_last_error()
                for B in FLEET:
                    reps = max(6, min(args.reps, args.reps * 2048 // (B * M * N)))
                    rng = np.random.default_rng(1)
                    blocks = np.stack([np.concatenate([np.asarray(task.default_state(), dtype=np.float32), (warm + 0.05 * rng.standard_normal(KU)).astype(np.float32),
                                                       np.full(KU, 0.1, dtype=np.float32), tp, lohi]) for _ in range(B)])
                    blk = torch.from_numpy(blocks).to(dev)
                    noise = torch.from_numpy(rng.standard_normal((B, KU, N)).astype(np.float32)).to(dev)
                    worst = [1 + b % M for b in range(B)]
                    worst_c = (C.c_int * B)(*worst)
                    member = torch.zeros((B, M, N), dtype=torch.float32, device=dev)
                    agg = torch.zeros((B, N), dtype=torch.float32, device=dev)
                    out = torch.zeros((B, 2 * KU), dtype=torch.float32, device=dev)
                    scratch = torch.zeros(B * per, dtype=torch.float32, device=dev)
                    # the floor: B * M problems, controller-major -- problem b * M + m has controller b's block and noise and member m's image
                    hs_bm = (C.c_void_p * (B * M))(*[handles[m].value for _ in range(B) for m in range(M)])
                    set_bm = C.c_void_p()
                    assert L.jh_model_set_create(hs_bm, B * M, C.byref(set_bm)) == 0, L.jh_last_error()
                    blk_bm = blk.repeat_interleave(M, dim=0).contiguous()
                    noise_bm = noise.repeat_interleave(M, dim=0).contiguous()
                    costs_bm = torch.zeros((B * M, N), dtype=torch.float32, device=dev)
                    out_bm = torch.zeros((B * M, 2 * KU), dtype=torch.float32, device=dev)
                    scratch_bm = torch.zeros(B * M * per, dtype=torch.float32, device=dev)
                    p, o = blk.data_ptr(), out.data_ptr()
                    mppi = (0, 0.05, 0, 0)

                    def leg(name):
                        t0 = time.perf_counter()
                        if name == "fleet":
                            st = L.jh_plan_step_ensemble_batch(mset, B, M, p, p, 4 * nblk, 4 * nblk, off[1], off[2], off[3], off[4], noise.data_ptr(), N, KU * N, W.data_ptr(), N, H, K,
                                                               member.data_ptr(), agg.data_ptr(), worst_c, *mppi, scratch.data_ptr(), o, 2 * KU, o, None, 0)
                            assert st == 0, L.jh_last_error()
                            ends = 1
                        elif name.startswith("singles"):
                            for b in range(B):
                                st = L.jh_plan_step_ensemble(mset, p + 4 * b * nblk, p + 4 * b * nblk, 4 * nblk, off[1], off[2], off[3], off[4], noise.data_ptr() + 4 * b * KU * N, N, W.data_ptr(), N, H, K,
                                                             member.data_ptr() + 4 * b * M * N, agg.data_ptr() + 4 * b * N, worst[b], *mppi, scratch.data_ptr() + 4 * b * per, o + 8 * b * KU,
                                                             o + 8 * b * KU, None, 0)
                                assert st == 0, L.jh_last_error()
                            ends = B
                        else:
                            q = blk_bm.data_ptr()
                            st = L.jh_plan_step_batch_models(set_bm, q, q, 4 * nblk, 4 * nblk, off[1], off[2], off[3], off[4], noise_bm.data_ptr(), N, KU * N, W.data_ptr(), N, H, K, costs_bm.data_ptr(),
                                                             None, *mppi, 0, 0, 0, scratch_bm.data_ptr(), out_bm.data_ptr(), 2 * KU, out_bm.data_ptr(), None, 0)
                            assert st == 0, L.jh_last_error()
                            ends = 1
                        for _ in range(ends):
                            assert L.jh_download_end() == 0, L.jh_last_error()
                        return 1e3 * (time.perf_counter() - t0)

                    legs = ["fleet", "singles_a", "singles_b", "batch_a", "batch_b"]
                    bits = {}
                    for name in legs:  # warm-up, and what each leg computes
                        for _ in range(3):
                            leg(name)
                        torch.cuda.synchronize()
                        bits[name] = costs_bm.cpu().numpy().tobytes() if name.startswith("batch") else member.cpu().numpy().tobytes() + agg.cpu().numpy().tobytes() + out.cpu().numpy().tobytes()
                        if not name.startswith("batch"):
                            bits[name + "_member"] = member.cpu().numpy().tobytes()
                            member.zero_(); agg.zero_(); out.zero_()
                    times = {name: [] for name in legs}
                    for rep in range(reps):
                        for name in (legs if rep % 2 == 0 else legs[::-1]):
                            times[name].append(leg(name))
                    torch.cuda.synchronize()
                    row = {"task": task_name, "B": B, "M": M, "N": N, "H": H, "K": K, "rollouts": B * M * N, "reps": reps}
                    for name in legs:
                        t = np.asarray(times[name])
                        row[name] = {"median_ms": float(np.median(t)), "p25_ms": float(np.percentile(t, 25)), "p75_ms": float(np.percentile(t, 75)), "min_ms": float(t.min())}
                    singles = 0.5 * (row["singles_a"]["median_ms"] + row["singles_b"]["median_ms"])
                    batch = 0.5 * (row["batch_a"]["median_ms"] + row["batch_b"]["median_ms"])
                    row["singles_a_vs_b_median_ms"] = abs(row["singles_a"]["median_ms"] - row["singles_b"]["median_ms"])
                    row["batch_a_vs_b_median_ms"] = abs(row["batch_a"]["median_ms"] - row["batch_b"]["median_ms"])
                    row["fleet_over_singles"] = row["fleet"]["median_ms"] / singles
                    row["fleet_over_batch"] = row["fleet"]["median_ms"] / batch
                    row["fleet_equals_singles_bits"] = bool(bits["fleet"] == bits["singles_a"])
                    row["member_costs_equal_batch_bits"] = bool(bits["fleet_member"] == bits["batch_a"])
                    results.append(row)
                    print(json.dumps(row), flush=True)
                    L.jh_model_set_destroy(set_bm)
                L.jh_model_set_destroy(mset)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
