"""Times of the batched plan step with a shared model image and with one image per problem (profiles/model_set.md), through the C ABI alone:
  parent   jh_plan_step_batch of another build of the library (--parent-lib: the commit in front of the model sets), twice per repetition -- the A / A spread of the session
  shared   jh_plan_step_batch of this build, B problems on one image
  set_same jh_plan_step_batch_models of this build on a set of B copies of that one image: the per-problem addressing alone, the same rollouts
  set      jh_plan_step_batch_models of this build, B problems on B distinct images (cube mass / friction, or pole mass, scaled per problem): other plants, other rollouts
All legs run in one process on the same buffers, alternating within every repetition; a time is the host clock around the call and its jh_download_end (which waits
for the completion mark behind the last problem).  Shapes: leap_cube B = 8 x 32 rollouts x H 64, cartpole B = 64 x 32 rollouts x H 64, MPPI, K = 4.
  NAME     (--other-lib NAME=PATH, repeatable) jh_plan_step_batch of a further build, one image: variants of a kernel side by side
usage: python tools/diag/model_set_timing.py [--parent-lib PATH] [--other-lib NAME=PATH ...] [--reps N] [--out FILE]"""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def bind(path, names):
    from judo_amd import _lib

    L = C.CDLL(path)
    for n in names:
        fn = getattr(L, n)
        fn.restype, fn.argtypes = _lib._SIGNATURES[n]
    return L


COMMON = ["jh_last_error", "jh_model_create", "jh_model_set_contact_capacity", "jh_plan_step_batch", "jh_download_end", "jh_plan_batch_scratch_floats", "jh_model_trace_layout"]


def main():
    import torch

    from judo_amd import _lib
    from judo_amd.models import pack_model, scaled_description
    from judo_amd.spline import spline_weights
    from judo_amd.tasks import get_registered_tasks

    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--other-lib", action="append", default=[])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cur = bind(_lib.LIB_PATH, COMMON + ["jh_model_set_create", "jh_plan_step_batch_models"])
    par = bind(args.parent_lib, COMMON) if args.parent_lib else None
    others = {spec.split("=", 1)[0]: bind(spec.split("=", 1)[1], COMMON) for spec in args.other_lib}
    results = []
    for task_name, B, N, H, reps in (("cartpole", 64, 32, 64, args.reps), ("leap_cube", 8, 32, 64, max(10, args.reps // 2))):
        task = get_registered_tasks()[task_name][0]()
        K, nu, nx = 4, task.nu, task.nq + task.nv
        KU = K * nu
        rng = np.random.default_rng(1)
        factors = np.linspace(0.7, 1.5, B)
        body, geom = ("pole", None) if task_name == "cartpole" else ("cube", "cube")
        descs = [scaled_description(task.desc, body_mass={body: f}, geom_friction={geom: 2.0 - f} if geom else None) for f in factors]

        def model(L, desc):
            blob = pack_model(desc)
            h = C.c_void_p()
            assert L.jh_model_create(C.create_string_buffer(blob, len(blob)), len(blob), 0, C.byref(h)) == 0, L.jh_last_error()
            if task_name == "leap_cube":
                assert L.jh_model_set_contact_capacity(h, 48) == 0
            return h

        m_cur = [model(cur, d) for d in descs]
        m_shared = model(cur, task.desc)
        m_par = model(par, task.desc) if par else None
        m_other = {name: model(L, task.desc) for name, L in others.items()}
        sets = {}
        for name, handles in (("set", m_cur), ("set_same", [m_shared] * B)):
            hs = (C.c_void_p * B)(*[h.value for h in handles])
            sets[name] = C.c_void_p()
            assert cur.jh_model_set_create(hs, B, C.byref(sets[name])) == 0, cur.jh_last_error()
        tp = np.asarray(task.task_params({}), dtype=np.float32)
        sizes = [nx, KU, KU, len(tp), 2 * nu]
        off = [int(v) for v in np.cumsum([0] + sizes)]
        nblk = off[-1]
        r = task.actuator_ctrlrange
        lohi = np.nan_to_num(np.concatenate([r[:, 0], r[:, 1]]).astype(np.float32), posinf=3.0e38, neginf=-3.0e38)
        warm = np.tile(np.asarray(task.optimizer_warm_start(), dtype=np.float64), (K, 1)).reshape(-1)
        blocks = np.stack([np.concatenate([np.asarray(task.default_state(), dtype=np.float32), (warm + 0.05 * rng.standard_normal(KU)).astype(np.float32),
                                           np.full(KU, 0.1, dtype=np.float32), tp, lohi]) for _ in range(B)])
        blk = torch.from_numpy(blocks).to(dev)
        noise = torch.from_numpy(rng.standard_normal((B, KU, N)).astype(np.float32)).to(dev)
        W = torch.from_numpy(spline_weights("linear", np.linspace(0, H * task.dt, K), task.dt * np.arange(H)).astype(np.float32)).to(dev)
        costs = torch.zeros((B, N), dtype=torch.float32, device=dev)
        out = torch.zeros((B, 2 * KU), dtype=torch.float32, device=dev)
        scratch = torch.zeros(int(cur.jh_plan_batch_scratch_floats(B, N, K, nu)), dtype=torch.float32, device=dev)
        tail = (blk.data_ptr(), blk.data_ptr(), 4 * nblk, 4 * nblk, off[1], off[2], off[3], off[4], noise.data_ptr(), N, KU * N, W.data_ptr(), N, H, K, costs.data_ptr(), None, 0, 0.05, 0, 0,
                0, 0, 0, scratch.data_ptr(), out.data_ptr(), 2 * KU, out.data_ptr(), None, 0)

        def leg(name):
            L = par if name.startswith("parent") else others.get(name, cur)
            t0 = time.perf_counter()
            st = cur.jh_plan_step_batch_models(sets[name], *tail) if name in sets else L.jh_plan_step_batch(m_par if L is par else m_other.get(name, m_shared), B, *tail)
            assert st == 0, L.jh_last_error()
            assert L.jh_download_end() == 0, L.jh_last_error()
            return 1e3 * (time.perf_counter() - t0)

        legs = (["parent_a", "parent_b"] if par else []) + ["shared", "set_same", "set"] + list(others)
        bits = {}
        for name in legs:  # warm-up, and what each leg computes
            for _ in range(3):
                leg(name)
            torch.cuda.synchronize()
            bits[name] = costs.cpu().numpy().copy()
        times = {name: [] for name in legs}
        for rep in range(reps):
            order = legs if rep % 2 == 0 else legs[::-1]
            for name in order:
                times[name].append(leg(name))
        row = {"task": task_name, "B": B, "N": N, "H": H, "K": K, "reps": reps}
        for name in legs:
            t = np.asarray(times[name])
            row[name] = {"median_ms": float(np.median(t)), "p25_ms": float(np.percentile(t, 25)), "p75_ms": float(np.percentile(t, 75)), "min_ms": float(t.min())}
        if par:
            row["parent_a_vs_b_median_ms"] = abs(row["parent_a"]["median_ms"] - row["parent_b"]["median_ms"])
            row["shared_costs_equal_parent_bits"] = bool(bits["shared"].tobytes() == bits["parent_a"].tobytes())
        row["set_over_shared"] = row["set"]["median_ms"] / row["shared"]["median_ms"]
        row["set_same_over_shared"] = row["set_same"]["median_ms"] / row["shared"]["median_ms"]
        row["set_same_costs_equal_shared_bits"] = bool(bits["set_same"].tobytes() == bits["shared"].tobytes())
        row["set_problems_with_costs_unlike_shared"] = int((bits["set"] != bits["shared"]).any(axis=1).sum())
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
