"""Lane use of the hand's broad phase in the leap kernel (a -DJH_V5_COUNT build selected with JUDO_AMD_LIB; counters stats[34..53] of jh_engine_v5.hip) on recorded plan steps
of the headline workload: level-1 sphere / box survivors per rollout-step and as the wave's maximum, how often the box region of level 1 runs in the per-pair and in the list
form, trips of the per-geom loop of level 2 (b) against passes of 16 combinations, and the cube sweep's box region.  profiles/leap_broad_phase.md has the table.
The pair tables (stats[54..55]; profiles/leap_pair_tables.md): table pairs that read safe per rollout-step, and those of them that the sphere test had passed (dropped
from the list).  The queue's horizon slices (stats[56]; profiles/leap_horizon_slices.md): the units whose hand-off was missed and which recomputed their group's steps up
to their slice, of the units the launch had.  `--no-pair-tables` packs the image without tables: the loops before the cut, every pair tested."""
import ctypes as C, sys
import numpy as np, torch
sys.path.insert(0, ".")
from judo_amd.controller import make_controller_for
from judo_amd.tasks import get_registered_tasks
from judo_amd import _lib
CB = ("sph", "sph_wavemax", "box_wavemax", "l1_pair_passes", "l1_list_passes", "l2_trips", "bpairs", "T", "combo_passes", "cube_box_regions", "cube_box_lanes", "max_sph", "max_box",
      "max_T", "steps_no_sph", "pairs_one_A", "pairs_one_B", "own_trips", "steps_sph_over_cap", "fewest_sph_inv")
d = np.load("tools/diag/ab_inputs_leap.npz")
L = _lib.lib(); L.jh_model_counters.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int]
task = get_registered_tasks()["leap_cube"][0]()
if "--no-pair-tables" in sys.argv[1:]: task.desc = dict(task.desc, pair_tables=False)
c = make_controller_for(task, "mppi"); c.optimizer.config.num_rollouts = 65536; c.controller_cfg.horizon = 0.64
c.reset(); c.current_state = c.task.default_state(); c.system_metadata = {"goal_quat": np.array([0.0, 1.0, 0.0, 0.0])}
for i in (2, 20, 35):
    c.model.stats()
    c.optimizer.seed(1000 + i); c.nominal_knots = d["knots"][i].copy(); c.times = d["times"][i].copy(); c.update_spline(c.times, c.nominal_knots); c.time = float(d["t"][i])
    c.update_action(); torch.cuda.synchronize()
    old = (C.c_int * 10)(); assert L.jh_model_counters(c.model.handle, old, 24, 10) == 0
    raw = (C.c_int * len(CB))(); assert L.jh_model_counters(c.model.handle, raw, 34, len(CB)) == 0
    pt = (C.c_int * 2)(); assert L.jh_model_counters(c.model.handle, pt, 34 + len(CB), 2) == 0
    rc = (C.c_int * 1)(); assert L.jh_model_counters(c.model.handle, rc, 36 + len(CB), 1) == 0
    k = {n: (v & 0xFFFFFFFF) for n, v in zip(CB, raw)}
    l2, bp = old[2] & 0xFFFFFFFF, old[3] & 0xFFFFFFFF
    nw = 65536 // 4 * 64; nr = 65536 * 64
    print(f"plan step {i:2d}")
    print(f"  level 1, per rollout-step: sphere survivors {k['sph'] / nr:.2f} (largest {k['max_sph']}, fewest {128 - k['fewest_sph_inv']}), box survivors {bp / nr:.2f} (largest {k['max_box']}); steps without a sphere survivor {k['steps_no_sph'] / nr:.4f}, above the list's cap {k['steps_sph_over_cap']}")
    print(f"  level 1, per wave-step: maximum of the sphere survivors {k['sph_wavemax'] / nw:.2f}, of the box survivors {k['box_wavemax'] / nw:.2f}; box region runs {k['l1_pair_passes'] / nw:.2f} (per pair pass) against {k['l1_list_passes'] / nw:.2f} (list form)")
    print(f"  level 2, per wave-step: passes (body pairs) {l2 / nw:.2f}, trips of the per-geom loop {k['l2_trips'] / nw:.2f} = {k['l2_trips'] / max(l2, 1):.2f} per pass, passes of 16 combinations {k['combo_passes'] / nw:.2f} = {k['combo_passes'] / max(l2, 1):.2f} per pass")
    print(f"  level 2, per rollout-step: body pairs that reach (b) {k['bpairs'] / nr:.2f}, combinations {k['T'] / max(k['bpairs'], 1):.2f} per such pair (largest {k['max_T']}), trips a rollout needs alone {k['own_trips'] / max(k['bpairs'], 1):.2f} per pair; one near geom on side A {k['pairs_one_A'] / max(k['bpairs'], 1):.2f}, on side B {k['pairs_one_B'] / max(k['bpairs'], 1):.2f} of the pairs")
    print(f"  pair tables, per rollout-step: table pairs that read safe {(pt[0] & 0xFFFFFFFF) / nr:.3f}, dropped behind the sphere test {(pt[1] & 0xFFFFFFFF) / nr:.3f}")
    sl = c.model.last_rollout_slices()
    print(f"  queue units: {sl} per group ({'the static grid' if sl == 0 else 'whole groups' if sl == 1 else 'horizon slices'}), {max(sl, 1) * (65536 // 4)} in the launch; recomputed after a missed hand-off {rc[0] & 0xFFFFFFFF}")
    print(f"  cube sweep, per wave-step: geom slots with a lane in the box region {k['cube_box_regions'] / nw:.2f}, lanes in it {k['cube_box_lanes'] / max(k['cube_box_regions'], 1):.1f} per run")
