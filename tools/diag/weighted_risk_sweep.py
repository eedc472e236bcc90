"""Times of the ensemble plan step with the `worst` measure and with the plant-weighted one (profiles/weighted_risk.md), through the C ABI alone:
  ensemble_a/b  jh_plan_step_ensemble with `worst` = M, twice per repetition: the A / A spread of the session, which is the margin any comparison has
  weighted      jh_plan_step_ensemble_weighted with uniform weights and tail = 1 (every member is visited: the most passes), where the library has the entry
All legs run in one process on the same buffers, alternating within every repetition; a time is the host clock around the call and jh_download_end.  The member costs
of the legs are compared bit for bit.  `--lib` times another build of the library (the parent commit's, which lacks the weighted entry: the leg is left out).
Shapes: those of tools/diag/ensemble_sweep.py -- cartpole N = 32, 4096 and leap_cube N = 32, 1024, 4096, H = 64, K = 4, MPPI -- at M = 4 and M = 32.
usage: python tools/diag/weighted_risk_sweep.py [--reps N] [--tasks cartpole,leap_cube] [--lib PATH] [--out FILE]"""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = {"cartpole": (32, 4096), "leap_cube": (32, 1024, 4096)}
MEMBERS = (4, 32)
H, K = 64, 4
USED = ("jh_last_error", "jh_model_create", "jh_model_destroy", "jh_model_set_contact_capacity", "jh_model_set_create", "jh_model_set_destroy", "jh_update_fused_scratch_floats",
        "jh_plan_step_ensemble", "jh_plan_step_ensemble_weighted", "jh_download_end")


def load(path):
    """The library at `path` with the signatures of what this tool calls; an entry the build lacks is left out."""
    from judo_amd import _lib

    L = C.CDLL(path)
    for name in USED:
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return L


def main():
    import torch

    from judo_amd import _lib
    from judo_amd.models import pack_model, scaled_description
    from judo_amd.spline import spline_weights
    from judo_amd.tasks import get_registered_tasks

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="repetitions at the smallest launch; larger launches run fewer (never below 10)")
    ap.add_argument("--tasks", default="cartpole,leap_cube")
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    L = load(args.lib)
    has_weighted = hasattr(L, "jh_plan_step_ensemble_weighted")
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
            blk = torch.from_numpy(block).to(dev)
            noise = torch.from_numpy(rng.standard_normal((KU, N)).astype(np.float32)).to(dev)
            per = int(L.jh_update_fused_scratch_floats(N, K, nu))
            for M in MEMBERS:
                reps = max(10, min(args.reps, args.reps * 2048 // (M * N)))
                hs = (C.c_void_p * M)(*[h.value for h in handles[:M]])
                mset = C.c_void_p()
                assert L.jh_model_set_create(hs, M, C.byref(mset)) == 0, L.jh_last_error()
                member = torch.zeros((M, N), dtype=torch.float32, device=dev)
                agg = torch.zeros(N, dtype=torch.float32, device=dev)
                out = torch.zeros(2 * KU, dtype=torch.float32, device=dev)
                scratch = torch.zeros(per, dtype=torch.float32, device=dev)
                weights = (C.c_float * M)(*([1.0 / M] * M))
                p, o = blk.data_ptr(), out.data_ptr()
                mppi = (0, 0.05, 0, 0)
                head = (mset, p, p, 4 * nblk, off[1], off[2], off[3], off[4], noise.data_ptr(), N, W.data_ptr(), N, H, K, member.data_ptr(), agg.data_ptr())
                tail = (*mppi, scratch.data_ptr(), o, o, None, 0)

                def leg(name):
                    t0 = time.perf_counter()
                    st = L.jh_plan_step_ensemble_weighted(*head, weights, 1.0, *tail) if name == "weighted" else L.jh_plan_step_ensemble(*head, M, *tail)
                    assert st == 0, L.jh_last_error()
                    assert L.jh_download_end() == 0, L.jh_last_error()
                    return 1e3 * (time.perf_counter() - t0)

                legs = ["ensemble_a", "ensemble_b"] + (["weighted"] if has_weighted else [])
                bits = {}
                for name in legs:  # warm-up, and what each leg computes
                    for _ in range(3):
                        leg(name)
                    torch.cuda.synchronize()
                    bits[name] = (member.cpu().numpy().copy(), agg.cpu().numpy().copy())
                times = {name: [] for name in legs}
                for rep in range(reps):
                    for name in (legs if rep % 2 == 0 else legs[::-1]):
                        times[name].append(leg(name))
                torch.cuda.synchronize()
                row = {"task": task_name, "M": M, "N": N, "H": H, "K": K, "reps": reps}
                for name in legs:
                    t = np.asarray(times[name])
                    row[name] = {"median_ms": float(np.median(t)), "p25_ms": float(np.percentile(t, 25)), "p75_ms": float(np.percentile(t, 75)), "min_ms": float(t.min())}
                row["a_vs_b_median_ms"] = abs(row["ensemble_a"]["median_ms"] - row["ensemble_b"]["median_ms"])
                if has_weighted:
                    row["weighted_minus_ensemble_ms"] = row["weighted"]["median_ms"] - 0.5 * (row["ensemble_a"]["median_ms"] + row["ensemble_b"]["median_ms"])
                    row["member_costs_equal_bits"] = bool(bits["weighted"][0].tobytes() == bits["ensemble_a"][0].tobytes())
                    d = np.abs(bits["weighted"][1].astype(np.float64) - bits["ensemble_a"][1].astype(np.float64))
                    row["max_rel_diff_of_the_mean"] = float((d / np.maximum(np.abs(bits["ensemble_a"][1]), 1e-30)).max())  # (uniform weights, tail 1 against worst = M: the mean both ways)
                results.append(row)
                print(json.dumps(row), flush=True)
                L.jh_model_set_destroy(mset)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
