"""ctypes binding of `libjudo_amd.so` (the C ABI declared in `include/judo_amd.h`).

There is no fallback: if the HIP library is missing the import of any compute entry point raises.
Build it with `python -c "import __graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).
"""

from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JUDO_AMD_LIB") or os.path.join(_HERE, "libjudo_amd.so")  # JUDO_AMD_LIB: alternative build of the same C ABI

_lib: C.CDLL | None = None

f32p = C.c_void_p  # device pointers travel as integers (tensor.data_ptr())

_SIGNATURES = {
    "jh_last_error": (C.c_char_p, []),
    "jh_version": (C.c_int, []),
    "jh_model_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "jh_model_destroy": (None, [C.c_void_p]),
    "jh_model_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "jh_model_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "jh_model_set_kernel": (C.c_int, [C.c_void_p, C.c_int]),
    "jh_model_limits": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "jh_register_xcheck": (C.c_int, [C.c_void_p]),
    "jh_model_max_fused_knots": (C.c_int, [C.c_void_p, C.c_int]),
    "jh_model_one_launch_max_knots": (C.c_int, [C.c_void_p, C.c_int]),
    "jh_model_set_plan_step_launches": (C.c_int, [C.c_void_p, C.c_int]),
    "jh_model_set_rollout_schedule": (C.c_int, [C.c_void_p, C.c_int]),
    "jh_model_set_rollout_slices": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "jh_model_last_rollout_slices": (C.c_int, [C.c_void_p]),
    "jh_model_set_rollout_slice_bounds": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "jh_model_last_rollout_slice_bounds": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "jh_rollout_slice_schedule": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "jh_model_recomputed_units": (C.c_int, [C.c_void_p]),
    "jh_model_set_self_collision": (C.c_int, [C.c_void_p, C.c_int]),
    "jh_model_set_contact_capacity": (C.c_int, [C.c_void_p, C.c_int]),
    "jh_model_build": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "jh_model_fr3_build": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "jh_model_trace_layout": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "jh_trace_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "jh_upload_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "jh_download_wait": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "jh_download_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "jh_download_end": (C.c_int, []),
    "jh_rollout_cost": (C.c_int, [C.c_void_p, f32p, f32p, f32p, C.c_int, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_void_p]),
    "jh_rollout_cost_traced": (C.c_int, [C.c_void_p, f32p, f32p, f32p, C.c_int, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, C.c_void_p]),
    "jh_rollout_materialize": (C.c_int, [C.c_void_p, f32p, C.c_int, f32p, C.c_int, C.c_int, f32p, f32p, C.c_void_p]),
    "jh_rollout_materialize_plants": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, f32p, C.c_int, f32p, C.c_int, C.c_int, f32p, f32p, C.c_void_p]),
    "jh_fr3_rollout_materialize_plants": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, f32p, C.c_int, f32p, C.c_int, C.c_int, f32p, f32p, C.c_void_p]),
    "jh_plant_residuals": (C.c_int, [f32p, f32p, f32p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_void_p]),
    "jh_plant_residuals_reports": (C.c_int, [f32p, f32p, f32p, C.POINTER(C.c_int), C.c_int, f32p, f32p, f32p, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p,
                                             C.c_int, C.c_void_p]),
    "jh_plant_controls": (C.c_int, [f32p, f32p, C.c_size_t, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p]),
    "jh_plant_reports": (C.c_int, [f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, f32p, f32p, C.c_void_p, f32p, f32p, f32p, C.c_void_p, f32p, f32p, C.c_void_p]),
    "jh_plants_advance": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, f32p, f32p, f32p, C.c_size_t, C.c_int, f32p, C.c_int, C.c_int, f32p, f32p, f32p, C.POINTER(C.c_int), C.c_int,
                                    f32p, f32p, C.c_void_p, f32p, f32p, f32p, C.c_void_p, f32p, C.c_void_p]),
    "jh_task_reward": (C.c_int, [C.c_void_p, f32p, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p]),
    "jh_noise_normal": (C.c_int, [C.c_ulonglong, C.c_uint, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_void_p]),
    "jh_sample_knots": (C.c_int, [f32p, f32p, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p]),
    "jh_spline_controls": (C.c_int, [f32p, f32p, f32p, f32p, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p]),
    "jh_spline_controls_batch": (C.c_int, [f32p, C.c_int, f32p, C.c_size_t, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p]),
    "jh_knot_moments": (C.c_int, [f32p, f32p, f32p, C.c_int, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p]),
    "jh_policy_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "jh_policy_destroy": (None, [C.c_void_p]),
    "jh_policy_scratch_floats": (C.c_size_t, [C.c_int]),
    "jh_policy_step": (C.c_int, [C.c_void_p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, f32p, C.c_int, C.c_void_p]),
    "jh_tree_create": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "jh_tree_destroy": (None, [C.c_void_p]),
    "jh_tree_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "jh_tree_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "jh_tree_set_self_collision": (C.c_int, [C.c_void_p, C.c_int]),
    "jh_tree_substeps": (C.c_int, [C.c_void_p, f32p, f32p, f32p, C.c_int, C.c_int, f32p, f32p, C.c_void_p]),
    "jh_policy_rollout_scratch_floats": (C.c_size_t, [C.c_int]),
    "jh_policy_rollout": (C.c_int, [C.c_void_p, C.c_void_p, f32p, C.c_int, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, f32p, f32p, f32p, C.POINTER(C.c_int), C.c_void_p]),
    "jh_policy_rollout_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, f32p, C.c_size_t, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, f32p, f32p, f32p, C.POINTER(C.c_int),
                                          C.c_void_p]),
    "jh_tree_set_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]),
    "jh_tree_set_update": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "jh_tree_set_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "jh_tree_set_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "jh_tree_set_destroy": (None, [C.c_void_p]),
    "jh_tree_substeps_plants": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, f32p, f32p, f32p, C.c_int, f32p, f32p, C.c_void_p]),
    "jh_policy_rollout_plants": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), f32p, C.c_size_t, f32p, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                           f32p, f32p, f32p, C.POINTER(C.c_int), C.c_void_p]),
    "jh_update_scratch_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "jh_mppi_partial": (C.c_int, [f32p, f32p, f32p, f32p, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, f32p, f32p, C.c_void_p]),
    "jh_mppi_merge": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_float, f32p, C.c_void_p]),
    "jh_topk_partial": (C.c_int, [f32p, f32p, f32p, f32p, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_void_p]),
    "jh_update_fused_scratch_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "jh_update_fused": (C.c_int, [f32p, f32p, f32p, f32p, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_int,
                                  f32p, f32p, f32p, f32p, C.c_void_p]),
    "jh_plan_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p,
                               C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_plan_batch_scratch_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "jh_plan_step_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_size_t, f32p, C.c_int, C.c_int, C.c_int,
                                     f32p, f32p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_plan_step_batch_phases": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_size_t, f32p, C.c_int, C.c_int,
                                            C.c_int, f32p, f32p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_model_set_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]),
    "jh_fr3_model_set_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]),
    "jh_plan_step_batch_phases_models": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_size_t, f32p, C.c_int,
                                                   C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_plan_step_randomized_phase": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.POINTER(C.c_ubyte), C.c_int, f32p, C.c_int, C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_model_set_update": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "jh_model_set_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "jh_model_set_destroy": (None, [C.c_void_p]),
    "jh_model_set_pair_tables": (C.c_int, [C.c_void_p]),
    "jh_pair_tables_shared": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "jh_plan_step_batch_models": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_size_t, f32p, C.c_int, C.c_int, C.c_int,
                                            f32p, f32p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_ensemble_costs": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p]),
    "jh_plan_step_ensemble": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_int,
                                        C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_plan_step_ensemble_phase": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int,
                                              C.c_int, C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_ensemble_costs_weighted": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float, f32p, C.c_void_p]),
    "jh_plan_step_ensemble_weighted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, f32p, f32p,
                                                 C.POINTER(C.c_float), C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_plan_step_ensemble_weighted_phase": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p,
                                                       f32p, C.POINTER(C.c_float), C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_plan_step_ensemble_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_size_t, f32p, C.c_int,
                                              C.c_int, C.c_int, f32p, f32p, C.POINTER(C.c_int), C.c_int, C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_plan_step_ensemble_batch_phases": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_size_t, f32p,
                                                     C.c_int, C.c_int, C.c_int, f32p, f32p, C.POINTER(C.c_int), C.c_int, C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]),
    "jh_ensemble_costs_risk_batch": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_size_t, C.POINTER(C.c_int), f32p, C.c_int, C.c_void_p]),
    "jh_plan_step_ensemble_batch_risk": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_size_t,
                                                   f32p, C.c_int, C.c_int, C.c_int, f32p, f32p, C.POINTER(C.c_int), C.c_int, C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_size_t, C.c_void_p,
                                                   C.c_void_p, C.c_void_p]),
    "jh_plan_step_ensemble_batch_phases_risk": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int,
                                                          C.c_size_t, f32p, C.c_int, C.c_int, C.c_int, f32p, f32p, C.POINTER(C.c_int), C.c_int, C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_size_t,
                                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_plan_step_randomized": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int,
                                          f32p, C.c_int, C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_plan_step_randomized_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_size_t, f32p, C.c_int,
                                                C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, f32p, C.c_int, C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_plan_step_randomized_batch_phases": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_size_t, f32p,
                                                       C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, f32p, C.c_int, C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]),
    "jh_update_fused_batch": (C.c_int, [C.c_int, f32p, f32p, C.c_size_t, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int,
                                        f32p, C.c_int, C.c_int, f32p, f32p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "jh_noise_normal_batch": (C.c_int, [C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint), C.c_int, C.c_int, f32p, C.c_int, C.c_void_p]),
    "jh_shard_record_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "jh_update_shard": (C.c_int, [f32p, f32p, f32p, f32p, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, f32p, C.c_int, C.c_int,
                                  f32p, f32p, C.c_void_p]),
    "jh_shard_merge": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, C.c_void_p]),
    "jh_plan_step_shard": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p,
                                     C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_void_p, C.c_void_p]),
    "jh_plan_merge": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jh_event_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "jh_event_destroy": (None, [C.c_void_p]),
    "jh_event_record": (C.c_int, [C.c_void_p, C.c_void_p]),
    "jh_stream_wait_event": (C.c_int, [C.c_void_p, C.c_void_p]),
    "jh_event_elapsed_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "jh_elite_merge": (C.c_int, [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, f32p, f32p, C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

# compile-time limits of the library (include/judo_amd.h; tests/test_host.py checks that the two agree)
MAX_KNOT_DIM = 512  # JH_MAX_KNOT_DIM: K * nu
MAX_ELITES = 32  # JH_MAX_ELITES: CEM elites / trace elites
MAX_TASK_PARAMS = 32  # JH_MAX_TASK_PARAMS
MAX_ENSEMBLE = 32  # JH_MAX_ENSEMBLE: members of a model set that jh_plan_step_ensemble plans against
MAX_ENSEMBLE_FLEET = 256  # JH_MAX_ENSEMBLE_FLEET: controllers of one jh_plan_step_ensemble_batch call
MAX_PLANT_BLOCKS = 64  # JH_MAX_PLANT_BLOCKS: rollout blocks of one jh_plan_step_randomized call
MAX_FLEET_PLANT_BLOCKS = 256  # JH_MAX_FLEET_PLANT_BLOCKS: B * G, the (controller, block) pairs of one jh_plan_step_randomized_batch call
MAX_ID_HORIZON = 64  # JH_MAX_ID_HORIZON: steps of a recorded window that jh_plant_residuals scores
MAX_ID_QUATS = 4  # JH_MAX_ID_QUATS: quaternions of a state row that jh_plant_residuals aligns


class JudoAmdError(RuntimeError):
    """A HIP/runtime failure reported by libjudo_amd.so."""


def lib() -> C.CDLL:
    """Load the shared library (once).  Raises ImportError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the MI355X engine has no CPU fallback. "
                "Build it with `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc)."
            )
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status: int, what: str) -> None:
    """Map a jh_status to the reference's error behaviour: shape/argument errors -> ValueError
    (the conditions judo/utils/mj_rollout_backend.py:78-82 asserts), runtime errors -> RuntimeError."""
    if status == 0:
        return
    msg = lib().jh_last_error().decode("utf-8", "replace")
    if status == -1:
        raise ValueError(f"{what}: {msg}")
    raise JudoAmdError(f"{what} failed (status {status}): {msg}")


def ptr(t) -> int | None:
    """data_ptr of a torch tensor (None passes a NULL pointer; an int is a raw device address and passes through)."""
    if t is None or isinstance(t, int):
        return t
    return t.data_ptr()
