"""How the leap kernel's launch fills the GPU, measured: a -DJH_V5_WAVESTAMP build (selected with JUDO_AMD_LIB) stores, per group of four rollouts, the 100 MHz wall clock at
its wave's entry, after the staging barrier, at the group's start and at its end, with the workgroup and wave that ran it.  Plan steps of the recorded headline inputs
(tools/diag/ab_inputs_leap.npz, as ab_fixed_inputs.py replays them) run under the static grid and under the queue (jh_model_set_rollout_schedule 1 / 2); printed per launch:
the distribution of group durations, what a workgroup's waves wait for each other, the occupied wave slots over time, the drain at the end -- and what a greedy placement
of the MEASURED durations (constant speed per slot) predicts for the static grid, a per-wave queue, a queue of horizon slices and the ideal.
--slices S[,S..] (default 1,2,4): the replay's queue of (group, slice) units -- a group's S equal parts, each the group's measured duration / S, taken breadth-first
(all first slices, then all second ones; hand-offs not modelled).  S = 1 is the per-wave queue.
--kernel-slices S (default 0: the launcher's rule): what jh_model_set_rollout_slices is given for the launches themselves; the kernel stamps per UNIT, so the
durations printed for a sliced launch are a slice's, and the replay is printed for unsliced launches only.  --max-workgroups W caps the queue's grid (0: the resident slots).
--kernel-bounds a,b,... : the launches run that explicit schedule (jh_model_set_rollout_slice_bounds) instead of --kernel-slices.
--save FILE: the stamps of every launch read (per unit: wave, wave entry, start, end, in ticks from the first entry) go to FILE (.npz), for the replay below.
--replay-from FILE [--against FILE,FILE..] [--bounds a,b,c/a,b,..] [--handoff-us X]: NO GPU.  FILE holds the stamps of launches forced to S = 16 (4-step units at
H = 64); the replay composes any schedule whose cuts are multiples of four steps from them and places its units greedily, breadth-first, on the wave slots.  A unit's cost
is its SLOT time (from the end of the unit before it on its wave to its own end: the ticket and the prologue are in it); a unit composed of m stamped ones costs their sum
less (m - 1) hand-offs.  The cost of one hand-off comes from the sums of slot time of the stamped launches: (T16 - T4) / (12 G) with the S = 4 stamps among --against, or
--handoff-us.  A unit that starts before its producer ended has missed its hand-off and pays the group's prefix from step 0 as well.  Printed per schedule: launch, drain,
share of slot time occupied, missed hand-offs; the files of --against are printed as measured beside it (the S = 4 row must reproduce the S = 4 stamps).
build:  tools/diag/build_variant.sh wavestamp judo_amd/csrc/jh_engine_v5.hip -DJH_V5_WAVESTAMP
usage:  JUDO_AMD_LIB=variants/libjudo_amd_wavestamp.so python tools/diag/wave_schedule.py [plan steps, default 5,35] [schedules, default 1,2] [--slices 1,2,4] [--kernel-slices S]"""
import ctypes as C, heapq, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

N, H, WPB, TICK_US = 65536, 64, 4, 0.01


def _opt(name, default):
    """Takes `name VALUE` out of sys.argv."""
    if name in sys.argv:
        k = sys.argv.index(name); v = sys.argv[k + 1]; del sys.argv[k:k + 2]
        return v
    return default


SLICES = [int(a) for a in _opt("--slices", "1,2,4").split(",")]
KSLICES, MAXWG = int(_opt("--kernel-slices", "0")), int(_opt("--max-workgroups", "0"))
KBOUNDS = [int(a) for a in _opt("--kernel-bounds", "").split(",") if a]
SAVE, REPLAY_FROM, AGAINST = _opt("--save", ""), _opt("--replay-from", ""), [a for a in _opt("--against", "").split(",") if a]
BOUNDS = [[int(a) for a in b.split(",") if a] for b in _opt("--bounds", "16,32,48/24,40,52,60/20,36,48,56,60").split("/")]
HANDOFF_US = float(_opt("--handoff-us", "nan"))
G = (N + 3) // 4


def slot_times(u):
    """Stamps [units, 4] (wave, wave entry, start, end; ticks) -> per unit the slot time in microseconds: from the end of the unit before it on its wave (the wave's entry
    for its first) to its own end."""
    wave, entry, end = u[:, 0], u[:, 1], u[:, 3]
    o = np.lexsort((end, wave))
    prev = np.empty(len(u)); prev[o[1:]] = end[o[:-1]]
    firsts = np.concatenate([[True], wave[o][1:] != wave[o][:-1]])
    prev[o[firsts]] = entry[o[firsts]]
    return (end - prev) * TICK_US


def measured(u):
    """(launch, drain, share of slot time occupied) of stamped units, in microseconds, as the live report below takes them."""
    start, end = u[:, 2] * TICK_US, u[:, 3] * TICK_US
    launch = end.max()
    slots = len(np.unique(u[:, 0]))
    return launch, launch - end[end > start.max()].min(), slot_times(u).sum() / (slots * launch), slots


def replay(d16, bounds, c, slots):
    """Greedy breadth-first placement of the schedule `bounds` (first steps of slices 1.., multiples of 4) composed from d16[group, 4-step unit] slot times; hand-off cost c."""
    cuts = [0] + [b // 4 for b in bounds] + [d16.shape[1]]
    cum = np.concatenate([np.zeros((len(d16), 1)), np.cumsum(d16, axis=1)], axis=1)
    dur = [cum[:, b] - cum[:, a] - (b - a - 1) * c for a, b in zip(cuts[:-1], cuts[1:])]  # per slice, per group
    pre = [cum[:, a] - max(a - 1, 0) * c for a in cuts[:-1]]  # the group from step 0 up to the slice, as one unit
    free = [0.0] * slots; heapq.heapify(free)
    ends = np.zeros((len(dur), len(d16))); missed = 0; busy = 0.0; last_start = 0.0
    for k in range(len(dur)):
        for g in range(len(d16)):
            t = heapq.heappop(free); w = dur[k][g]
            if k > 0 and t < ends[k - 1][g]: w += pre[k][g]; missed += 1
            ends[k][g] = t + w; busy += w; last_start = t
            heapq.heappush(free, t + w)
    launch = ends.max()
    return launch, launch - min(free), busy / (slots * launch), missed


if REPLAY_FROM:
    z16 = np.load(REPLAY_FROM); others = [np.load(f) for f in AGAINST]
    for key in z16.files:
        u16 = z16[key]; assert len(u16) == 16 * G, "the replay composes from launches forced to S = 16"
        d16 = slot_times(u16).reshape(16, G).T  # (unit t is slice t // G of group t % G)
        l16, dr16, sh16, slots = measured(u16)
        print(f"\n{key}: S = 16 stamped: launch {l16 / 1e3:.2f} ms, drain {dr16 / 1e3:.2f} ms, occupied {sh16:.3f}, slot time {d16.sum() / 1e6:.3f} s on {slots} slots")
        sums = {16: d16.sum()}
        for z in others:
            if key not in z.files: continue
            u = z[key]; S = len(u) // G; sums[S] = slot_times(u).sum()
            l, dr, sh, _ = measured(u)
            print(f"{key}: S = {S} stamped: launch {l / 1e3:.2f} ms, drain {dr / 1e3:.2f} ms, occupied {sh:.3f}, slot time {sums[S] / 1e6:.3f} s")
        c = HANDOFF_US
        for a, b in ((16, 4), (4, 1), (16, 1)):
            if a in sums and b in sums:
                est = (sums[a] - sums[b]) / ((a - b) * G)
                print(f"  one hand-off from the sums of S = {a} and S = {b}: {est:.1f} us")
                if np.isnan(c): c = est
        assert not np.isnan(c), "--handoff-us, or the S = 4 stamps among --against"
        print(f"  replay with {c:.1f} us per hand-off:")
        for b in [[]] + BOUNDS:
            assert all(x % 4 == 0 and 0 < x < H for x in b) and sorted(set(b)) == b, b
            l, dr, sh, miss = replay(d16, b, c, slots)
            steps = [y - x for x, y in zip([0] + b, b + [H])]
            print(f"    {' / '.join(map(str, steps)):>28}: launch {l / 1e3:.2f} ms, drain {dr / 1e3:.2f} ms, occupied {sh:.3f}, missed hand-offs {miss}")
    sys.exit(0)

import torch
from judo_amd.controller import make_controller
from judo_amd import _lib
d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ab_inputs_leap.npz"))
c = make_controller("leap_cube", "mppi"); c.optimizer.config.num_rollouts = N; c.controller_cfg.horizon = H * c.task.dt
c.reset(); c.current_state = c.task.default_state(); c.system_metadata = {"goal_quat": np.array([0.0, 1.0, 0.0, 0.0])}
L = _lib.lib()
L.jh_v5_wavestamp_buffer.argtypes = [C.c_void_p, C.c_int]; L.jh_v5_wavestamp_buffer.restype = C.c_int  # AttributeError: not a -DJH_V5_WAVESTAMP build
ROWS = G * (len(KBOUNDS) + 1 if KBOUNDS else min(KSLICES, H) if KSLICES else 8)  # one stamp row per queue unit: unit t is slice t // G of group t % G (unsliced launches: the group); room for an automatic schedule of up to 8 slices
buf = torch.zeros((ROWS, 6), dtype=torch.int64, device="cuda")
assert L.jh_v5_wavestamp_buffer(buf.data_ptr(), ROWS) == 0
if KSLICES or MAXWG:
    c.model.set_rollout_slices(KSLICES, MAXWG, 0)  # (AttributeError: a library from before the slices)
if KBOUNDS:
    c.model.set_rollout_slice_bounds(KBOUNDS)  # (AttributeError: a library from before the explicit schedules)
saved = {}
SLOTS = 2 * torch.cuda.get_device_properties(0).multi_processor_count * WPB  # waves of this kernel the GPU holds: two workgroups of four per CU
steps = [int(a) for a in (sys.argv[1] if len(sys.argv) > 1 else "5,35").split(",")]
modes = [int(a) for a in (sys.argv[2] if len(sys.argv) > 2 else "1,2").split(",")]


def greedy(units, slots):
    """Launch length when `units` (durations, in ticket order) go one after the other to whichever of `slots` slots is free first."""
    free = [0.0] * min(slots, len(units)); heapq.heapify(free)
    end = 0.0
    for u in units:
        t = heapq.heappop(free) + u; end = max(end, t); heapq.heappush(free, t)
    return end


def model(dur):
    """The greedy model on measured group durations `dur` (launch order)."""
    pad = np.concatenate([dur, np.zeros(-len(dur) % WPB)]).reshape(-1, WPB)
    static = greedy(pad.max(axis=1), SLOTS // WPB)  # a workgroup's slots are held until its slowest wave ends
    sliced = [greedy(np.tile(dur / s, s), SLOTS) for s in SLICES]  # breadth-first tickets: all first slices before any second (hand-offs not modelled); S = 1: the per-wave queue
    ideal = dur.sum() / SLOTS
    return static, sliced, ideal


def pct(a, q): return float(np.percentile(a, q))


for i in steps:
    for mode in modes:
        c.model.set_rollout_schedule(mode)
        for rep in range(2):  # (the second launch is the one read: the first may carry one-off costs)
            buf.zero_()
            c.optimizer.seed(1000 + i); c.nominal_knots = d["knots"][i].copy(); c.times = d["times"][i].copy(); c.update_spline(c.times, c.nominal_knots); c.time = float(d["t"][i])
            c.update_action(); torch.cuda.synchronize()
        a = buf.cpu().numpy()
        a = a[a[:, 5] == 1]  # (a sliced launch stamps its units; a launch the rule leaves unsliced, and the static grid, the first G rows)
        assert len(a) == G * max(1, c.model.last_rollout_slices()), "units without a stamp"
        sliced_launch = len(a) > G
        if SAVE: saved[f"step{i}_schedule{mode}"] = np.stack([(a[:, 0] >> 32) * WPB + ((a[:, 0] >> 8) & 0xFF), a[:, 1] - a[:, 1].min(), a[:, 3] - a[:, 1].min(), a[:, 4] - a[:, 1].min()], axis=1).astype(np.int32)
        if sliced_launch and hasattr(c.model, "last_rollout_slice_bounds"): print(f"  slices' first steps {c.model.last_rollout_slice_bounds()}; recomputed units {c.model.recomputed_units()}")
        wg, wv = a[:, 0] >> 32, (a[:, 0] >> 8) & 0xFF
        t0 = a[:, 1].min()
        entry, staged, start, end = ((a[:, k] - t0) * TICK_US for k in (1, 2, 3, 4))  # microseconds from the first wave's entry
        dur = end - start
        kernel = end.max()
        print(f"\nplan step {i}, schedule {mode} ({'static grid' if mode == 1 else 'queue'}): {len(a)} {'units (group, slice)' if sliced_launch else 'groups'} on {int(wg.max()) + 1} workgroups, {SLOTS} wave slots; launch {kernel / 1e3:.2f} ms from first entry to last end")
        print(f"  {'unit' if sliced_launch else 'group'} duration [ms]: mean {dur.mean() / 1e3:.3f}  cv {dur.std() / dur.mean():.4f}  p50 {pct(dur, 50) / 1e3:.3f}  p90 {pct(dur, 90) / 1e3:.3f}  p99 {pct(dur, 99) / 1e3:.3f}  max {dur.max() / 1e3:.3f}")
        print(f"  staging (entry -> barrier passed) [us]: mean {(staged - entry).mean():.1f}  max {(staged - entry).max():.1f}")
        wave = wg * WPB + wv  # the wave (slot holder) that ran each group
        order = np.argsort(wave, kind="stable")
        first = np.concatenate([[True], wave[order][1:] != wave[order][:-1]])
        w_entry, w_end = np.minimum.reduceat(entry[order], np.flatnonzero(first)), np.maximum.reduceat(end[order], np.flatnonzero(first))
        w_wg = wg[order][first]
        per_wg = [(w_end[w_wg == g] - w_entry[w_wg == g]) for g in np.unique(w_wg)[:: max(1, len(np.unique(w_wg)) // 512)]]
        print(f"  waves: {len(w_end)}, lifetime mean {(w_end - w_entry).mean() / 1e3:.3f} ms; over (sampled) workgroups, mean of (max - mean) of their waves' lifetimes: {np.mean([p.max() - p.mean() for p in per_wg]) / 1e3:.3f} ms"
              f" ({100 * np.mean([(p.max() - p.mean()) / p.max() for p in per_wg]):.1f} % of the workgroup's lifetime)")
        # occupied slots over time: a slot is occupied from its wave's entry to the end of the wave's last group (static grid: the wave's only group)
        ts = np.concatenate([w_entry, w_end]); dv = np.concatenate([np.ones(len(w_entry)), -np.ones(len(w_end))])
        o = np.argsort(ts, kind="stable"); ts, occ = ts[o], np.cumsum(dv[o])
        grid_t = np.linspace(0, kernel, 21)[1:-1]
        print("  occupied wave slots at 5 % .. 95 % of the launch: " + " ".join(str(int(occ[np.searchsorted(ts, t, side='right') - 1])) for t in grid_t))
        share = float((occ[:-1] * np.diff(ts)).sum() / (SLOTS * kernel))
        # the drain: once the last group has started nothing is left to hand out, and the first slot that frees after that stays empty
        drain = kernel - end[end > start.max()].min()
        print(f"  resident-wave share from the stamps {share:.3f}; most waves at once {int(occ.max())}; from the first slot that stays empty to the end {drain / 1e3:.3f} ms ({100 * drain / kernel:.1f} % of the launch)")
        if not sliced_launch:  # (the replay wants whole groups' durations, in ticket order: under the queue the first SLOTS groups are the waves' own, the rest in the order drawn)
            s_, sl_, id_ = model(dur)
            ref_ = kernel if mode == 2 else s_
            print(f"  greedy model on these durations: static grid {s_ / 1e3:.2f} ms; " + "; ".join(f"queue, S = {s} {v / 1e3:.2f} ms ({100 * (1 - v / ref_):.1f} %)" for s, v in zip(SLICES, sl_))
                  + f"; ideal {id_ / 1e3:.2f} ms ({100 * (1 - id_ / ref_):.1f} %)  [per cent shorter than {'this measured launch' if mode == 2 else 'the replayed static grid'}, {ref_ / 1e3:.2f} ms]")
assert L.jh_v5_wavestamp_buffer(None, 0) == 0
if SAVE:
    os.makedirs(os.path.dirname(os.path.abspath(SAVE)), exist_ok=True)
    np.savez_compressed(SAVE, **saved)
