"""Times of B ensemble plan steps with a risk record per controller in one launch (profiles/weighted_fleet.md), through the C ABI alone:
  risk          ONE jh_plan_step_ensemble_batch_risk, every controller weighted (general weights, tail 0.5)
  risk_counted  the same entry with every tail word 0.0: the counted measure through the new tail, worst[b] as in the legs below -- the scalar loads alone
  plain         ONE jh_plan_step_ensemble_batch of this build on the same blocks, noise and set
  parent_a/b    the same call in ANOTHER build of the library (--parent-lib: the parent commit's), with its own handles -- twice per repetition: the A / A spread of the
                session, which is the margin the comparison has.  Without --parent-lib the two legs run this build's unweighted entry.
  singles       B back-to-back jh_plan_step_ensemble_weighted calls with the controllers' weights and tails, then their B completion marks
All legs run in one process, alternating within every repetition; a time is the host clock around the call(s) and jh_download_end.  The tail launch alone is the time
between the entries' second and third timing event (jh_event_elapsed_ms), taken in repetitions of their own.  What the legs compute is compared too: the risk leg's
member costs are the plain leg's and its costs and nominals the singles', bit for bit.  The closed-form model's blocks are read in place with the polled completion
word, the leap model's uploaded, as the fleets do it.
Shapes: cartpole N = 32, 4096 and leap_cube N = 32, 1024; H = 64, K = 4, MPPI; B = 8, M = 4.
usage: python tools/diag/weighted_fleet_sweep.py [--reps N] [--tasks cartpole,leap_cube] [--parent-lib FILE] [--out FILE]"""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = {"cartpole": (32, 4096), "leap_cube": (32, 1024)}
B, M, H, K = 8, 4, 64, 4


def load(path, signatures):
    L = C.CDLL(path)
    for name, (res, args) in signatures.items():
        fn = getattr(L, name, None)  # (a parent build lacks the new entries)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return L


def main():
    import torch

    from judo_amd import _lib
    from judo_amd.models import pack_model, scaled_description
    from judo_amd.spline import spline_weights
    from judo_amd.tasks import get_registered_tasks

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100, help="repetitions at the small N; the large one runs a fifth (never below 10)")
    ap.add_argument("--tasks", default="cartpole,leap_cube")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    L = _lib.lib()
    P = load(args.parent_lib, _lib._SIGNATURES) if args.parent_lib else L
    results = []
    for task_name in args.tasks.split(","):
        task = get_registered_tasks()[task_name][0]()
        nu, nx = task.nu, task.nq + task.nv
        KU = K * nu
        closed = task_name == "cartpole"
        body, geom = ("pole", None) if closed else ("cube", "cube")
        sets = {}
        for lib in {id(L): L, id(P): P}.values():  # the M plants and their set, in each build
            hs = []
            for i, f in enumerate(np.linspace(0.7, 1.5, M)):  # member 0 is the shipped description
                desc = task.desc if i == 0 else scaled_description(task.desc, body_mass={body: f}, geom_friction={geom: 2.0 - f} if geom else None)
                blob = pack_model(desc)
                h = C.c_void_p()
                assert lib.jh_model_create(C.create_string_buffer(blob, len(blob)), len(blob), 0, C.byref(h)) == 0, lib.jh_last_error()
                if not closed:
                    assert lib.jh_model_set_contact_capacity(h, 48) == 0
                hs.append(h)
            mset = C.c_void_p()
            assert lib.jh_model_set_create((C.c_void_p * M)(*[h.value for h in hs]), M, C.byref(mset)) == 0, lib.jh_last_error()
            sets[id(lib)] = mset
        tp = np.asarray(task.task_params({}), dtype=np.float32)
        off = [int(v) for v in np.cumsum([0, nx, KU, KU, len(tp), 2 * nu])]
        nblk = off[-1]
        stride = nblk + 1 + M
        r = task.actuator_ctrlrange
        lohi = np.nan_to_num(np.concatenate([r[:, 0], r[:, 1]]).astype(np.float32), posinf=3.0e38, neginf=-3.0e38)
        warm = np.tile(np.asarray(task.optimizer_warm_start(), dtype=np.float64), (K, 1)).reshape(-1)
        W = torch.from_numpy(spline_weights("linear", np.linspace(0, H * task.dt, K), task.dt * np.arange(H)).astype(np.float32)).to(dev)
        for N in SHAPES[task_name]:
            per = int(L.jh_update_fused_scratch_floats(N, K, nu))
            reps = args.reps if N == SHAPES[task_name][0] else max(10, args.reps // 5)
            rng = np.random.default_rng(1)
            host = torch.zeros((B, stride), dtype=torch.float32).pin_memory()
            weights = rng.uniform(0.05, 1.0, (B, M))
            weights = (weights / weights.sum(axis=1, keepdims=True)).astype(np.float32)
            tails = np.full(B, 0.5, dtype=np.float32)
            for b in range(B):
                host.numpy()[b] = np.concatenate([np.asarray(task.default_state(), dtype=np.float32), (warm + 0.05 * rng.standard_normal(KU)).astype(np.float32),
                                                  np.full(KU, 0.1, dtype=np.float32), tp, lohi, [tails[b]], weights[b]])
            host0 = host.clone().pin_memory()  # the same blocks with every tail word 0.0
            host0.numpy()[:, nblk] = 0.0
            blk = torch.zeros((B, stride), dtype=torch.float32, device=dev)
            noise = torch.from_numpy(rng.standard_normal((B, KU, N)).astype(np.float32)).to(dev)
            worst = [1 + b % M for b in range(B)]
            worst_c = (C.c_int * B)(*worst)
            member = torch.zeros((B, M, N), dtype=torch.float32, device=dev)
            agg = torch.zeros((B, N), dtype=torch.float32, device=dev)
            out = torch.zeros((B, 2 * KU), dtype=torch.float32).pin_memory()
            done = torch.zeros(4, dtype=torch.int32).pin_memory()
            scratch = torch.zeros(B * per, dtype=torch.float32, device=dev)
            hp, o = host.data_ptr(), out.data_ptr()
            p = hp if closed else blk.data_ptr()
            mark = done.data_ptr() if closed else o
            mppi = (0, 0.05, 0, 0)
            events = {}
            for lib in {id(L): L, id(P): P}.values():
                evs = []
                for _ in range(3):
                    e = C.c_void_p()
                    assert lib.jh_event_create(C.byref(e)) == 0
                    evs.append(e)
                events[id(lib)] = evs

            def batched(lib, entry, extra, blk_floats, timing, hp=hp):
                p = hp if closed else blk.data_ptr()
                st = entry(sets[id(lib)], B, M, p, hp, 4 * blk_floats, 4 * stride, off[1], off[2], off[3], off[4], *extra, noise.data_ptr(), N, KU * N, W.data_ptr(), N, H, K, member.data_ptr(),
                           agg.data_ptr(), worst_c, *mppi, scratch.data_ptr(), o, 2 * KU, mark, timing, 0)
                assert st == 0, lib.jh_last_error()
                assert lib.jh_download_end() == 0, lib.jh_last_error()

            def leg(name, timed_tail=False):
                lib = P if name.startswith("parent") else L
                timing = (C.c_void_p * 3)(*[e.value for e in events[id(lib)]]) if timed_tail else None
                t0 = time.perf_counter()
                if name == "risk":
                    batched(L, L.jh_plan_step_ensemble_batch_risk, (nblk,), stride, timing)
                elif name == "risk_counted":
                    batched(L, L.jh_plan_step_ensemble_batch_risk, (nblk,), stride, timing, hp=host0.data_ptr())
                elif name == "singles":
                    for b in range(B):
                        q = p + 4 * b * stride
                        st = L.jh_plan_step_ensemble_weighted(sets[id(L)], q, hp + 4 * b * stride, 4 * nblk, off[1], off[2], off[3], off[4], noise.data_ptr() + 4 * b * KU * N, N, W.data_ptr(), N, H,
                                                              K, member.data_ptr() + 4 * b * M * N, agg.data_ptr() + 4 * b * N, (C.c_float * M)(*weights[b].tolist()), float(tails[b]), *mppi,
                                                              scratch.data_ptr() + 4 * b * per, o + 8 * b * KU, (mark + 0) if closed else o + 8 * b * KU, None, 0)
                        assert st == 0, L.jh_last_error()
                        if closed:  # (one polled word: a call's mark is read before the next call counts on it)
                            assert L.jh_download_end() == 0, L.jh_last_error()
                    if not closed:
                        for _ in range(B):
                            assert L.jh_download_end() == 0, L.jh_last_error()
                else:
                    batched(lib, lib.jh_plan_step_ensemble_batch, (), nblk, timing)
                ms = 1e3 * (time.perf_counter() - t0)
                if timed_tail:
                    torch.cuda.synchronize()
                    t = C.c_float()
                    assert lib.jh_event_elapsed_ms(events[id(lib)][1], events[id(lib)][2], C.byref(t)) == 0, lib.jh_last_error()
                    return t.value
                return ms

            legs = ["risk", "risk_counted", "plain", "parent_a", "parent_b", "singles"]
            bits = {}
            for name in legs:  # warm-up, and what each leg computes
                for _ in range(3):
                    leg(name)
                torch.cuda.synchronize()
                bits[name] = (member.cpu().numpy().tobytes(), agg.cpu().numpy().tobytes() + out.numpy().tobytes())
                member.zero_(); agg.zero_(); out.zero_()
            times = {name: [] for name in legs}
            for rep in range(reps):
                for name in (legs if rep % 2 == 0 else legs[::-1]):
                    times[name].append(leg(name))
            tails_ms = {name: [] for name in ("risk", "risk_counted", "parent_a", "parent_b")}
            for rep in range(max(10, reps // 2)):
                for name in (list(tails_ms) if rep % 2 == 0 else list(tails_ms)[::-1]):
                    tails_ms[name].append(leg(name, timed_tail=True))
            torch.cuda.synchronize()
            row = {"task": task_name, "B": B, "M": M, "N": N, "H": H, "K": K, "rollouts": B * M * N, "reps": reps, "parent_lib": bool(args.parent_lib)}
            for name in legs:
                t = np.asarray(times[name])
                row[name] = {"median_ms": float(np.median(t)), "p25_ms": float(np.percentile(t, 25)), "p75_ms": float(np.percentile(t, 75)), "min_ms": float(t.min())}
            for name, t in tails_ms.items():
                t = np.asarray(t)
                row["tail_" + name] = {"median_us": float(1e3 * np.median(t)), "p25_us": float(1e3 * np.percentile(t, 25)), "p75_us": float(1e3 * np.percentile(t, 75)), "min_us": float(1e3 * t.min())}
            parent = 0.5 * (row["parent_a"]["median_ms"] + row["parent_b"]["median_ms"])
            row["parent_a_vs_b_median_ms"] = abs(row["parent_a"]["median_ms"] - row["parent_b"]["median_ms"])
            row["risk_minus_parent_median_ms"] = row["risk"]["median_ms"] - parent
            row["risk_over_parent"] = row["risk"]["median_ms"] / parent
            row["risk_counted_minus_parent_median_ms"] = row["risk_counted"]["median_ms"] - parent
            row["risk_over_singles"] = row["risk"]["median_ms"] / row["singles"]["median_ms"]
            row["tail_parent_a_vs_b_median_us"] = abs(row["tail_parent_a"]["median_us"] - row["tail_parent_b"]["median_us"])
            row["tail_risk_minus_parent_median_us"] = row["tail_risk"]["median_us"] - 0.5 * (row["tail_parent_a"]["median_us"] + row["tail_parent_b"]["median_us"])
            row["tail_risk_counted_minus_parent_median_us"] = row["tail_risk_counted"]["median_us"] - 0.5 * (row["tail_parent_a"]["median_us"] + row["tail_parent_b"]["median_us"])
            row["member_costs_equal_bits"] = bool(bits["risk"][0] == bits["risk_counted"][0] == bits["plain"][0] == bits["parent_a"][0] == bits["singles"][0])
            row["risk_equals_singles_bits"] = bool(bits["risk"][1] == bits["singles"][1])
            row["plain_equals_parent_bits"] = bool(bits["plain"] == bits["parent_a"])
            row["risk_counted_equals_plain_bits"] = bool(bits["risk_counted"] == bits["plain"])
            results.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
