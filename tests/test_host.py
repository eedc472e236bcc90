"""CPU tests of the product's host logic (no GPU, no compute calls through the C ABI)."""

import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT


def test_config_overrides_match_reference():
    from judo_amd import config as c

    g = json.load(open(os.path.join(GOLDEN, "configs.json")))
    for task, d in g["optimizer"].items():
        for name, cls in (("mppi", c.MPPIConfig), ("cem", c.CrossEntropyMethodConfig), ("ps", c.PredictiveSamplingConfig)):
            cfg = cls()
            if task != "default":
                cfg.set_override(task)
            assert c.as_plain_dict(cfg) == d[name], (task, name)
    for task, d in g["controller"].items():
        cfg = c.ControllerConfig()
        if task != "default":
            cfg.set_override(task)
        assert c.as_plain_dict(cfg) == d, task
    # switching override keys resets untouched fields to their defaults
    cfg = c.MPPIConfig()
    cfg.set_override("leap_cube")
    assert cfg.temperature == 0.0025
    cfg.set_override("cartpole")
    assert cfg.temperature == 0.05 and cfg.sigma == 0.1 and cfg.use_noise_ramp
    with pytest.warns(UserWarning, match="not found in class"):  # the reference warns and skips the name (judo/config.py:88-95)
        c.set_config_overrides("x", c.MPPIConfig, {"not_a_field": 1})


def test_spline_weights_numpy_match_reference():
    from judo_amd.spline import evaluate, spline_weights

    g = np.load(os.path.join(GOLDEN, "spline.npz"))
    for key in [k[: -len("_cfg")] for k in g.files if k.endswith("_cfg")]:
        kind, K, H, dt, hor, t0 = g[key + "_cfg"]
        kind = {0: "zero", 1: "linear", 3: "cubic"}[int(kind)]
        kt = t0 + np.linspace(0, hor, int(K))
        W = spline_weights(kind, kt, t0 + dt * np.arange(int(H)))
        np.testing.assert_allclose(W, g[key + "_W"], atol=1e-12)
        np.testing.assert_allclose(evaluate(kind, kt, g[key + "_knots"], t0 + dt * np.arange(int(H))), g[key + "_U"], atol=1e-12)
        np.testing.assert_allclose(evaluate(kind, kt, g[key + "_knots"][0], g[key + "_shift_times"]), g[key + "_shift_knots"], atol=1e-12)
        np.testing.assert_allclose(evaluate(kind, kt, g[key + "_knots"][0], np.array([t0 - 1.0, t0 + hor + 2.0])), g[key + "_far"], atol=1e-14)
    with pytest.raises(ValueError):
        spline_weights("cubic", np.linspace(0, 1, 3), np.zeros(2))
    with pytest.raises(ValueError):
        spline_weights("quintic", np.linspace(0, 1, 4), np.zeros(2))


def test_min_max_normaliser_is_an_affine_sigma_scale():
    """Sampling nominal_n + sigma*eps in MinMaxNormalizer units == nominal + sigma*(hi-lo)/2*eps in raw units."""
    g = np.load(os.path.join(GOLDEN, "normalizer.npz"))
    lo, hi, x = g["minmax_lo"], g["minmax_hi"], g["minmax_x"]
    finite = np.isfinite(lo) & np.isfinite(hi)
    lo_f, hi_f = np.where(finite, lo, -1.0), np.where(finite, hi, 1.0)  # (+inf) + (-inf) is a RuntimeWarning even under np.where: mask first
    scale = np.where(finite, (hi_f - lo_f) / 2, 1.0)
    off = np.where(finite, (hi_f + lo_f) / 2, 0.0)
    np.testing.assert_allclose((x - off) / scale, g["minmax_norm"], atol=1e-12)
    np.testing.assert_allclose(x * scale + off, g["minmax_denorm"], atol=1e-12)


@pytest.mark.parametrize("task", ["cartpole", "cylinder_push", "leap_cube", "fr3_pick"])
def test_model_constants_agree_with_oracle(task):
    """Two independent implementations (numpy here, C in the oracle) of the reference-pose inertia and inverse weights."""
    from judo_amd import models as M
    from oracle import oracle as O

    d = M.load_description(task)
    om = O.Model(task)
    dw, bw = M.inverse_weights(d)
    odw, obw = om.invweight0()
    np.testing.assert_allclose(dw, odw, rtol=1e-10)
    np.testing.assert_allclose(bw, obw, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(M.qpos0(d), om.qpos0())
    q = M.qpos0(d)
    q[-1] += 0.3
    Mm, _ = M.mass_matrix(d, q)
    np.testing.assert_allclose(Mm, om.mass_matrix(q), rtol=1e-10, atol=1e-14)
    lay = M.layout(d)
    assert (lay.nq, lay.nv, lay.nu, lay.ns) == (om.nq, om.nv, om.nu, om.ns)


def test_model_dimensions_match_survey_table():
    from judo_amd import models as M

    dims = {"cartpole": (2, 2, 1, 6, 0.04), "cylinder_push": (4, 4, 2, 6, 0.02), "fr3_pick": (16, 15, 8, 14, 0.004), "leap_cube": (23, 22, 16, 31, 0.01)}
    for task, (nq, nv, nu, ns, dt) in dims.items():
        d = M.load_description(task)
        lay = M.layout(d)
        assert (lay.nq, lay.nv, lay.nu, lay.ns) == (nq, nv, nu, ns)
        assert d["option"]["timestep"] == dt
    r = M.actuator_ctrlrange(M.load_description("fr3_pick"))
    np.testing.assert_allclose(r[-1], [-0.02, 0.06])  # inheritrange=2 about the finger joint range (0, 0.04)
    with pytest.raises(ValueError):
        M.load_description("no_such_task")


def test_blob_packing():
    import struct

    from judo_amd import models as M

    for task, kind in (("cartpole", 0), ("cylinder_push", 1), ("leap_cube", 2), ("fr3_pick", 3)):
        blob = M.pack_model(M.load_description(task))
        head = struct.unpack("<16I", blob[:64])
        assert head[0] == M.BLOB_MAGIC and head[2] == kind
        assert len(blob) == 64 + 4 * (head[8] + head[9])
    from judo_amd.engine_model import engine_structure

    st = engine_structure(M.load_description("leap_cube"))
    assert len(st["moving"]) == 17 and [len(b) for b in st["blocks"]] == [4, 4, 4, 4]


def test_fused_fixed_bodies_preserve_the_dynamics():
    """fr3_pick: `hand` (no joint, welded to link7) is merged into its parent for the engine; the joint-space inertia of the
    merged tree equals that of the original at arbitrary configurations, and the candidate contact pairs match the oracle's."""
    from judo_amd import models as M
    from judo_amd.engine_model import engine_structure, fuse_fixed_bodies, generic_pairs
    from oracle import oracle as O

    d = M.load_description("fr3_pick")
    f = fuse_fixed_bodies(d)
    assert f["fused"] == ["hand"] and len(f["bodies"]) == len(d["bodies"]) - 1
    rng = np.random.default_rng(0)
    for _ in range(3):
        q = M.qpos0(d)
        q[7:] = rng.uniform(-1.5, 1.5, 9)
        M1, _ = M.mass_matrix(d, q)
        M2, _ = M.mass_matrix(f, q)
        np.testing.assert_allclose(M1, M2, rtol=1e-12, atol=1e-14)
    st = engine_structure(f)
    assert len(st["moving"]) == 10 and [len(b) for b in st["blocks"]] == [9]
    allg = [g for g in f["geoms"] if g["type"] in ("box", "sphere", "capsule")]
    pairs = generic_pairs(d, dict(f, geoms=allg), st)
    names = {tuple(sorted((allg[a]["name"], allg[b]["name"]))) for a, b in pairs}
    om = O.Model("fr3_pick", scope="kernel")  # the subset k_fr3_v6 models
    onames = {tuple(sorted((om.desc["geoms"][a]["name"], om.desc["geoms"][b]["name"]))) for a, b in om.pairs}
    assert names == onames and len(names) == 78  # 63 box pairs + the arm links' capsules against table (7) and cube (8), round 3
    # the oracle's DEFAULT model is what the MJCF says (fr3_components/fr3.xml:11-99, no <exclude>): every pair MuJoCo's static filters leave -- 22 link-link capsule pairs
    # and 90 link-against-gripper-box pairs on top; the kernel's subset is a stated deviation, held to "never touches on the measured workloads" by
    # tests/test_oracle.py::test_fr3_link_pairs_never_touch_on_the_baseline_workload and tests/test_gpu_fr3.py::test_fr3_link_pairs_never_touch_where_the_kernel_goes
    full = O.Model("fr3_pick")
    fnames = {tuple(sorted((full.desc["geoms"][a]["name"], full.desc["geoms"][b]["name"]))) for a, b in full.pairs}
    extra = fnames - onames
    assert onames < fnames and len(fnames) == 190 and len(extra) == 112 and all("link" in a or "link" in b for a, b in extra)


def test_c_abi_library_exports_every_declared_symbol():
    """include/judo_amd.h <-> libjudo_amd.so <-> the ctypes table agree (loading needs no GPU)."""
    from judo_amd import _lib

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    xheader = open(os.path.join(ROOT, "include", "judo_amd_xcheck.h")).read()  # the test-build hooks (cross-check kernel generations): declared apart from the boundary
    declared = set(re.findall(r"\b(jh_[a-z_0-9]+)\s*\(", header))
    xdeclared = set(re.findall(r"\b(jh_[a-z_0-9]+)\s*\(", xheader))
    assert xdeclared == {"jh_model_set_kernel", "jh_register_xcheck"} and not (declared & xdeclared)
    declared |= xdeclared
    assert declared == set(_lib.EXPORTED_SYMBOLS), declared ^ set(_lib.EXPORTED_SYMBOLS)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
    assert _lib.lib().jh_version() >= 100
    assert _lib.lib().jh_update_scratch_floats(65536, 4, 16) >= 256 * 66


def test_library_limits_agree_with_the_header():
    from judo_amd import _lib

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    limits = (("JH_MAX_KNOT_DIM", _lib.MAX_KNOT_DIM), ("JH_MAX_ELITES", _lib.MAX_ELITES), ("JH_MAX_TASK_PARAMS", _lib.MAX_TASK_PARAMS), ("JH_MAX_ENSEMBLE", _lib.MAX_ENSEMBLE),
              ("JH_MAX_ENSEMBLE_FLEET", _lib.MAX_ENSEMBLE_FLEET), ("JH_MAX_PLANT_BLOCKS", _lib.MAX_PLANT_BLOCKS), ("JH_MAX_FLEET_PLANT_BLOCKS", _lib.MAX_FLEET_PLANT_BLOCKS),
              ("JH_MAX_ID_HORIZON", _lib.MAX_ID_HORIZON), ("JH_MAX_ID_QUATS", _lib.MAX_ID_QUATS))
    for name, val in limits:
        m = re.search(rf"#define\s+{name}\s+(\d+)", header)
        assert m and int(m.group(1)) == val and type(val) is int, name
    assert {name for name, _ in limits} == set(re.findall(r"#define\s+(JH_MAX_\w+)", header))  # every limit of the header has its name in the binding


HEADER_SAMPLE = r"""
/* thing.h -- a comment that holds a call, f(a, b); and a prototype, int jh_ghost(int n); neither is an entry */
#ifndef THING_H
#define THING_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define JH_MAX_THINGS 7 /* things (a, b) */
#define JH_MAX_WIDE 512
#define JH_BOTH(a, b) \
  ((a) + (b))
typedef struct jh_thing jh_thing;
enum jh_kind { JH_A = 0, JH_B = 1 };
const char* jh_name(void);
int jh_count();
void jh_thing_destroy(jh_thing* t);
size_t jh_thing_floats(int n, unsigned int draw, unsigned long long seed, float scale, double tol, size_t stride);
int jh_thing_create(const void* blob, jh_thing** out); // a line comment, g(a, b);
int jh_thing_run(const jh_thing* t, const float* x /* DEVICE, (n, 3) */, float* y, void* stream,
                 const int* plan /* HOST, (a, b) */, int* stats, const unsigned int* draws,
                 const unsigned long long *seeds, const unsigned char* plant_of_block);
int jh_thing_set(const jh_thing* const* members, const float* const* rows, void** outs, int lut[4]);
int jh_thing_weighted(const float* weights, float* ms, const unsigned char* column_mask, const unsigned char* column_mask_sens, void* const* timing);
typedef struct jh_hooks {
  int (*run)(const jh_thing* t, int n, float* y);
  int (*max)(const jh_thing* t);
} jh_hooks;
int jh_register(const jh_hooks* hooks);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_header_reader_maps_every_rule_and_exception():
    """The reader of judo_amd._lib on a header written here: one declaration per type rule and per named exception, in the shapes the real headers hold."""
    from judo_amd._lib import read_header

    P, void_p, i = ctypes.POINTER, ctypes.c_void_p, ctypes.c_int
    table, limits = read_header(HEADER_SAMPLE)
    assert limits == {"MAX_THINGS": 7, "MAX_WIDE": 512}
    assert table == {
        "jh_name": (ctypes.c_char_p, []),
        "jh_count": (i, []),
        "jh_thing_destroy": (None, [void_p]),
        "jh_thing_floats": (ctypes.c_size_t, [i, ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_float, ctypes.c_double, ctypes.c_size_t]),
        "jh_thing_create": (i, [void_p, P(void_p)]),
        "jh_thing_run": (i, [void_p, void_p, void_p, void_p, P(i), P(i), P(ctypes.c_uint), P(ctypes.c_ulonglong), P(ctypes.c_ubyte)]),
        "jh_thing_set": (i, [P(void_p), P(void_p), P(void_p), P(i)]),
        "jh_thing_weighted": (i, [P(ctypes.c_float), P(ctypes.c_float), void_p, void_p, void_p]),
        "jh_register": (i, [void_p]),
    }
    assert list(table) == ["jh_name", "jh_count", "jh_thing_destroy", "jh_thing_floats", "jh_thing_create", "jh_thing_run", "jh_thing_set", "jh_thing_weighted", "jh_register"]
    # an exception may name its entry: it holds there and nowhere else
    table, _ = read_header("int jh_a(const float* x);\nint jh_b(const float* x);", {("const float*", "x", "jh_b"): P(ctypes.c_float)})
    assert table == {"jh_a": (i, [void_p]), "jh_b": (i, [P(ctypes.c_float)])}
    # it refuses what it cannot map, and names the entry and the parameter
    with pytest.raises(TypeError, match=r"jh_bad.*short\* codes"):
        read_header("int jh_ok(int n);\nint jh_bad(int n,\n           const short* codes /* HOST */);")
    with pytest.raises(TypeError, match=r"jh_bad.*double\* tol"):
        read_header("int jh_bad(double* tol);")
    with pytest.raises(TypeError, match=r"jh_bad.*float\*\*\* rows"):
        read_header("int jh_bad(float*** rows);")
    with pytest.raises(TypeError, match=r"jh_bad.*cb"):
        read_header("int jh_bad(int (*cb)(int, int));")
    with pytest.raises(TypeError, match=r"jh_bad.*return type `float\*`"):
        read_header("float* jh_bad(int n);")
    with pytest.raises(TypeError, match=r"jh_twice"):
        read_header("int jh_twice(int n);\nint jh_twice(int n);")
    with pytest.raises(TypeError, match=r"cannot read the declaration `int jh_open\(int n`"):
        read_header("int jh_open(int n;")


def test_ctypes_table_is_the_headers():
    """Every prototype of the two headers, and nothing else, is bound: the loaded function carries the derived restype and argtypes, and as many parameters as an
    independent split of the prototype's text counts."""
    from judo_amd import _lib

    text = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("judo_amd.h", "judo_amd_xcheck.h"))
    protos = re.findall(r"\b(jh_\w+)\s*\(([^;()]*)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    counts = {name: 0 if params.strip() in ("", "void") else params.count(",") + 1 for name, params in protos}
    assert len(protos) == len(counts) == len(_lib.EXPORTED_SYMBOLS) and set(counts) == set(_lib.EXPORTED_SYMBOLS) == set(_lib._SIGNATURES), set(counts) ^ set(_lib.EXPORTED_SYMBOLS)
    L = _lib.lib()
    for name, (restype, argtypes) in _lib._SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and len(fn.argtypes) == len(argtypes) == counts[name], name
        assert all(a is b for a, b in zip(fn.argtypes, argtypes)), name
        assert restype in (None, ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p), name


def test_missing_header_is_an_import_error_with_its_path(monkeypatch, tmp_path):
    from judo_amd import _lib

    monkeypatch.setattr(_lib, "_INCLUDE", str(tmp_path))
    with pytest.raises(ImportError, match=re.escape(os.path.join(str(tmp_path), "judo_amd.h"))):
        _lib._read_headers()


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    """`--gpus 8` under a 1-rank environment must not run (and label) a 1-GPU job: non-zero exit, before any GPU work."""
    import subprocess
    import sys

    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "0"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--gpus 8 but WORLD_SIZE=1" in r.stderr
    assert not r.stdout.strip()  # no JSON line


def test_optimizer_host_state_and_registry():
    from judo_amd import config as c
    from judo_amd import optimizers as o

    assert set(o.get_registered_optimizers()) == {"cem", "mppi", "ps"}
    m = o.GpuMPPI(c.MPPIConfig(num_nodes=4, use_noise_ramp=True, noise_ramp=4.0, sigma=0.2), 16)
    np.testing.assert_allclose(m.knot_sigma()[:, 0], [0.2, 0.4, 0.6, 0.8])
    cem = o.GpuCEM(c.CrossEntropyMethodConfig(num_nodes=4, sigma_min=0.01, sigma_max=0.3, use_noise_ramp=True, noise_ramp=4.0), 2)
    np.testing.assert_allclose(cem.sigma, 0.155)
    s1 = cem.knot_sigma().copy()
    s2 = cem.knot_sigma().copy()
    np.testing.assert_allclose(s1[:, 0], np.clip(0.155 * np.array([1, 2, 3, 4.0]), 0.01, 0.3))
    np.testing.assert_allclose(s2[:, 0], np.clip(s1[:, 0] * np.array([1, 2, 3, 4.0]), 0.01, 0.3))  # cumulative
    o.register_optimizer("mine", o.GpuPS, c.PredictiveSamplingConfig)
    assert "mine" in o.get_registered_optimizers()
    o.get_registered_optimizers().pop("mine")


def test_tasks_host_side():
    from judo_amd import tasks as T

    assert set(T.get_registered_tasks()) >= {"cartpole", "cylinder_push", "leap_cube", "fr3_pick"}
    t = T.FR3Pick()
    x = t.default_state()
    t.pre_rollout(x)
    assert t.phase == T.Phase.LIFT.value
    x2 = x.copy(); x2[2] = 0.1
    t.pre_rollout(x2); assert t.phase == T.Phase.MOVE.value
    x3 = x2.copy(); x3[:2] = t.config.goal_pos
    t.pre_rollout(x3); assert t.phase == T.Phase.PLACE.value
    x4 = x3.copy(); x4[2] = 0.02
    t.pre_rollout(x4); assert t.phase == T.Phase.HOMING.value
    assert len(t.task_params()) == 22
    lc = T.LeapCube()
    np.testing.assert_allclose(lc.task_params({"goal_quat": np.array([0, 1, 0, 0.0])}), [100, 0.1, 0, 0.03, 0.1, 0, 1, 0, 0], rtol=1e-6)
    np.testing.assert_allclose(lc.optimizer_warm_start(), T.LEAP_QPOS_HOME[7:])
    assert lc.dt == 0.01 and lc.nu == 16 and np.isfinite(lc.actuator_ctrlrange).all()
    assert T.Cartpole().default_state().shape == (4,)


def test_sharding():
    from judo_amd.distributed import shard_rollouts

    for total, world in ((65536, 8), (65536, 1), (1000, 3), (7, 7)):
        shards = [shard_rollouts(total, world, r) for r in range(world)]
        assert sum(s.count for s in shards) == total and shards[0].offset == 0
        for a, b in zip(shards, shards[1:]):
            assert a.offset + a.count == b.offset
    with pytest.raises(ValueError):
        shard_rollouts(3, 4, 0)
    with pytest.raises(ValueError):
        shard_rollouts(8, 2, 2)


def test_compute_requires_gpu_and_never_falls_back():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from judo_amd import config as c
    from judo_amd import optimizers as o

    with pytest.raises(RuntimeError):
        o.GpuMPPI(c.MPPIConfig(), 1).sample_control_knots(np.zeros((4, 1)))


def test_product_never_imports_the_oracle():
    """No product source imports, includes, links or loads anything under oracle/ (comments may cite it)."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "judo_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                if f.endswith(".py"):
                    code = re.sub(r'"""[\s\S]*?"""', "", src)
                    code = re.sub(r"#.*", "", code)
                else:
                    code = re.sub(r"//.*", "", src)
                    code = re.sub(r"/\*[\s\S]*?\*/", "", code)
                assert not re.search(r"^\s*(from|import)\s+oracle", code, re.M), f
                assert "libjudo_oracle" not in code and "jo_engine" not in code and "jo_plan" not in code and "oracle/" not in code, f


def test_wire_records_round_trip_through_arrow():
    """SplineData / MujocoState (judo/app/structs.py:30-84): Arrow form and back; SplineData.spline() holds the end knots."""
    from judo_amd.structs import MujocoState, SplineData, from_arrow, to_arrow

    rng = np.random.default_rng(0)
    st = MujocoState(time=1.25, qpos=rng.standard_normal(23), qvel=rng.standard_normal(22), xpos=rng.standard_normal((5, 3)),
                     xquat=rng.standard_normal((5, 4)), sim_metadata={"goal_quat": np.array([0.0, 1.0, 0.0, 0.0]), "phase": 2})
    arr, meta = to_arrow(st)
    assert all(isinstance(v, str) for v in meta.values())
    back = from_arrow(arr, meta, MujocoState)
    assert back.time == 1.25 and back.sim_metadata == {"goal_quat": [0.0, 1.0, 0.0, 0.0], "phase": 2}
    for f in ("qpos", "qvel", "xpos", "xquat", "mocap_pos", "mocap_quat"):
        np.testing.assert_array_equal(getattr(back, f), getattr(st, f))
        assert getattr(back, f).shape == getattr(st, f).shape
    with pytest.raises(ValueError):
        from_arrow(arr, meta, SplineData)

    g = np.load(os.path.join(GOLDEN, "spline.npz"))
    for key in [k[: -len("_cfg")] for k in g.files if k.endswith("_cfg")]:
        kind, K, H, dt, hor, t0 = g[key + "_cfg"]
        kind = {0: "zero", 1: "linear", 3: "cubic"}[int(kind)]
        sp = SplineData(t0 + np.linspace(0, hor, int(K)), g[key + "_knots"], kind)  # batched knots (N, K, nu)
        f = sp.spline()
        np.testing.assert_allclose(f(t0 + dt * np.arange(int(H))), g[key + "_U"], atol=1e-12)  # the reference's make_spline(...)(q)
        np.testing.assert_allclose(f(np.array([t0 - 1.0, t0 + hor + 2.0]))[0], g[key + "_far"], atol=1e-14)  # held end values
        a2, m2 = to_arrow(sp)
        sp2 = from_arrow(a2, m2, SplineData)
        assert sp2.kind == kind and sp2.extrapolate is True
        np.testing.assert_array_equal(sp2.x, sp.x)
        np.testing.assert_array_equal(sp2.t, sp.t)
    with pytest.raises(ValueError):
        SplineData(np.arange(4.0), np.zeros((4, 2)), "quintic")
    with pytest.raises(ValueError):
        SplineData(np.arange(4.0), np.zeros((4, 2)), "linear", extrapolate=False).spline()(5.0)


def test_running_normaliser_loop_matches_reference_golden():
    """The optimiser loop of Controller.update_action with the "running" action normaliser (judo/controller/controller.py:222-296),
    restated the way the GPU path runs it: the kernels see raw knots (nominal_eff, sigma_eff, bounds_eff), the update returns the
    weighted mean of RAW candidates, the statistics are updated from two moments per actuator.  The golden sequence was produced by the
    reference's RunningMeanStdNormalizer + MPPI with a stand-in reward (tools/gen_golden.py::gen_normalizer)."""
    from judo_amd.normalization import RunningMeanStdNormalizer
    from oracle import oracle as O

    g = np.load(os.path.join(GOLDEN, "normalizer.npz"))
    N, K, nu, iters, sigma, lam, ramp = g["running_cfg"]
    N, K, nu, iters = int(N), int(K), int(nu), int(iters)
    lo, hi, target = g["running_lo"], g["running_hi"], g["running_target"]
    nrm = RunningMeanStdNormalizer(nu)
    sig_n = O.mppi_sigma(sigma, True, ramp, K, nu)
    nominal_n = nrm.normalize(g["running_nominal_in"])
    for it in range(iters):
        scale, center = nrm.noise_scale(), nrm.denormalize(np.zeros(nu))
        np.testing.assert_allclose(scale, nrm.std, rtol=1e-15)
        nominal_eff, sigma_eff = nrm.denormalize(nominal_n), sig_n * scale[None, :]
        lo_eff, hi_eff = nrm.denormalize(nrm.normalize(lo)), nrm.denormalize(nrm.normalize(hi))
        # what jh_rollout_cost / jh_knot_moments compute from the effective inputs
        cand = O.clip_knots(O.sample_knots(nominal_eff, g[f"running_it{it}_noise"], sigma_eff), lo_eff, hi_eff)
        np.testing.assert_allclose(cand, g[f"running_it{it}_candidates"], rtol=1e-12, atol=1e-12)
        rewards = -np.sum((cand - target) ** 2, axis=(1, 2))
        np.testing.assert_allclose(rewards, g[f"running_it{it}_rewards"], rtol=1e-12)
        wmean_raw = O.mppi_update(cand, rewards, lam)           # the device update acts on raw candidates ...
        nominal_n = (wmean_raw - center[None, :]) / scale[None, :]  # ... which is the update in normalised units
        np.testing.assert_allclose(nominal_n, g[f"running_it{it}_nominal_normalized"], rtol=1e-9, atol=1e-12)
        d = cand.reshape(-1, nu) - nrm.mean
        nrm.update_from_moments(N * K, d.sum(0), (d * d).sum(0))
        st = g[f"running_it{it}_state"]
        assert nrm.count == st[0]
        np.testing.assert_allclose(np.concatenate([nrm.mean, nrm.std, nrm.M2]), st[1:], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(nrm.denormalize(nominal_n), g["running_nominal_out"], rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ Spot task layer
def test_spot_task_layer_matches_reference_golden():
    """SpotBase command mapping for all 12 feature combinations, SpotNavigate.reward, overrides and constants (tools/gen_golden_spot.py)."""
    import torch
    from judo_amd import spot_tasks as ST
    from judo_amd.config import ControllerConfig, CrossEntropyMethodConfig, MPPIConfig, PredictiveSamplingConfig

    d = np.load(os.path.join(GOLDEN, "spot_tasks.npz"))
    for ci, combo in enumerate(d["combos"]):
        t = ST.SpotBase(*[bool(x) for x in combo])
        assert np.array_equal(t.default_command, d[f"c{ci}_default_command"]) and np.array_equal(t.command_mask, d[f"c{ci}_command_mask"])
        assert np.array_equal(t.actuator_ctrlrange, d[f"c{ci}_ctrlrange"]) and t.nu == len(t.default_command)
        ctl = d[f"c{ci}_controls"]
        assert np.array_equal(t.task_to_sim_ctrl(ctl), d[f"c{ci}_sim3"])
        assert np.array_equal(t.task_to_sim_ctrl(ctl[:, 0]), d[f"c{ci}_sim2"])
        assert np.array_equal(t.task_to_sim_ctrl(ctl[0, 0]), d[f"c{ci}_sim1"])
        assert np.array_equal(t.task_to_sim_ctrl(torch.as_tensor(ctl)).numpy(), d[f"c{ci}_sim3"])   # the device path runs the same code on tensors
        assert np.array_equal(ctl, d[f"c{ci}_controls"])                                             # inputs are not modified in place
        assert len(t.get_action_components()) == t.nu - (t.gripper_selection_index is not None)
    nav = ST.SpotNavigate()
    assert nav.nu == 3 and (nav.nq, nav.nv) == (26, 25) and nav.physics_substeps == 2 and abs(nav.dt - 0.02) < 1e-15 and nav.uses_locomotion_policy
    assert np.array_equal(nav.data.qpos[7:19], ST.LEGS_STANDING_POS) and np.array_equal(nav.data.qpos[19:], ST.ARM_STOWED_POS)
    nav.config.goal_position = d["nav_goal"]
    np.testing.assert_allclose(nav.reward(d["nav_states"], None, d["nav_controls"]), d["nav_reward"], rtol=1e-13)
    np.testing.assert_allclose(nav.reward(torch.as_tensor(d["nav_states"]), None, torch.as_tensor(d["nav_controls"])).numpy(), d["nav_reward"], rtol=1e-13)
    nav.config.w_controls = 0.25
    np.testing.assert_allclose(nav.reward(d["nav_states"], None, d["nav_controls"]), d["nav_reward_wc"], rtol=1e-13)
    assert not ST.SpotBase().reward(d["nav_states"], None, None).any()
    g = json.load(open(os.path.join(GOLDEN, "spot_configs.json")))
    for task in ("spot_base", "spot_navigate"):
        for nm, cls in (("mppi", MPPIConfig), ("cem", CrossEntropyMethodConfig), ("ps", PredictiveSamplingConfig)):
            c = cls()
            c.set_override(task)
            assert {k: getattr(c, k) for k in g["optimizer"][task][nm]} == g["optimizer"][task][nm]
        c = ControllerConfig()
        c.set_override(task)
        assert vars(c) == g["controller"][task]
    for k, v in g["constants"].items():
        np.testing.assert_allclose(np.asarray(getattr(ST, k), dtype=np.float64), np.asarray(v, dtype=np.float64), rtol=0, atol=0)
    cfg = ST.SpotNavigateConfig()
    assert {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in vars(cfg).items()} == g["task_defaults"]["spot_navigate"]


def test_tree_model_image():
    """Host-side packing for the floating-base tree kernel: structure checks, image layout, rejection of models outside its scope."""
    from judo_amd import models
    from judo_amd.tree_model import TD_F, TD_I, TG_F, TG_I, TH_F, TH_I, TS_F, TS_I, pack_tree_blob, pack_tree_model, tree_structure

    desc = models.load_description("spot")
    st = tree_structure(desc)
    chains = {}
    for k, i in enumerate(st["info"]):
        chains.setdefault(i["start"], []).append((k, i["depth"], i["parent"]))
    assert sorted(len(v) for v in chains.values()) == [3, 3, 3, 3, 7]           # four legs, one arm
    for start, links in chains.items():
        assert [d for _, d, _ in links] == list(range(len(links))) and links[0][2] == -1 and all(p == k - 1 for k, _, p in links[1:])
    F, I = pack_tree_model(desc)
    nj, ng = int(I[0]), int(I[1])
    assert (nj, ng, int(I[2]), int(I[3])) == (19, 27, 26, 25)
    nsen, nsd = int(I[4]), int(I[5])
    assert (nsen, nsd) == (16, 48)
    npair, opair = int(I[6]), int(I[7])
    assert F.size == TH_F + nj * TD_F + ng * TG_F + nsen * TS_F and I.size == TH_I + nj * TD_I + ng * TG_I + nsen * TS_I + npair and F.dtype == np.float32 and I.dtype == np.int32
    # the robot against itself: the 287 geom pairs MuJoCo's static filters and the 11 excludes of spot_primitive/contact.xml leave, g1 | g2 << 8 with g1 < g2, behind the sensor records
    assert npair == 287 and opair == TH_I + nj * TD_I + ng * TG_I + nsen * TS_I
    pk = I[opair : opair + npair]
    assert ((pk & 255) < (pk >> 8)).all() and (pk >> 8).max() < ng and len(set(pk.tolist())) == npair
    from oracle import oracle as O
    plane = next(i for i, g in enumerate(desc["geoms"]) if g["type"] == "plane")
    assert plane == ng  # (robot geom indices = the description's: the plane comes last)
    assert {(int(p) & 255, int(p) >> 8) for p in pk} == {p for p in O.collision_pairs(desc, scope="all") if plane not in p}
    srec = I[TH_I + nj * TD_I + ng * TG_I : opair].reshape(nsen, TS_I)
    assert list(srec[:, 2]) == list(range(0, 48, 3)) and set(srec[:, 0]) == {0, 1, 2, 3} and srec[0, 3] == 1 and (srec[2:4, 1] == -2).all()   # object axes sit on a world-fixed site
    assert abs(F[0] - 0.01) < 1e-9 and np.allclose(F[11:14], [0, 0, 1]) and np.allclose(F[5:8], [0, 0, -9.81])
    M, _ = models.mass_matrix(desc, models.qpos0(desc))
    assert abs(sum(F[TH_F + k * TD_F + 15] for k in range(nj)) + F[14] - M[0, 0]) < 1e-4   # link masses add up to the translational inertia
    owners = I[TH_I + nj * TD_I : TH_I + nj * TD_I + ng * TG_I : TG_I]
    assert owners.min() == -1 and owners.max() < nj
    blob = pack_tree_blob(desc)
    hd = np.frombuffer(blob[:16], dtype=np.uint32)
    assert hd[0] == 0x34564A54 and hd[1] == F.size and hd[2] == I.size and len(blob) == 16 + 4 * (F.size + I.size)
    for other in ("leap_cube", "fr3_pick", "cartpole"):
        with pytest.raises(NotImplementedError):
            pack_tree_model(models.load_description(other))


def test_tree_create_rejects_images_outside_the_kernel_instantiation():
    """jh_tree_create validates the image before it touches the device: these calls fail with a message on a box without a GPU too."""
    from judo_amd import _lib, models
    from judo_amd.tree_model import TD_I, TH_I, pack_tree_blob

    L = _lib.lib()
    L.jh_last_error.restype = ctypes.c_char_p
    blob = bytearray(pack_tree_blob(models.load_description("spot")))

    def create(b):
        buf = (ctypes.c_char * len(b)).from_buffer_copy(bytes(b))
        h = ctypes.c_void_p()
        rc = L.jh_tree_create(ctypes.cast(buf, ctypes.c_void_p), len(b), ctypes.byref(h))
        return rc, (L.jh_last_error() or b"").decode()

    bad = bytearray(blob); bad[0] ^= 0xFF
    rc, msg = create(bad)
    assert rc < 0 and "magic" in msg
    rc, msg = create(blob[:-4])
    assert rc < 0 and "size" in msg
    hd = np.frombuffer(bytes(blob[:16]), dtype=np.uint32)
    nf = int(hd[1])
    ints = np.frombuffer(bytes(blob[16 + 4 * nf :]), dtype=np.int32).copy()
    ints[TH_I + 3 * TD_I + 1 : TH_I + 3 * TD_I + 3] = [0, 3]       # the fourth joint claims to extend the first leg: not the {3,3,3,3,7} layout
    wrong = bytes(blob[: 16 + 4 * nf]) + ints.tobytes()
    rc, msg = create(wrong)
    assert rc < 0 and "chain" in msg


def test_caltech_leap_cube_model_and_oracle_sensors():
    """caltech_leap_cube: the packed image carries the reference frames of its two frame sensors and four groups of hand bodies for the
    self-collision tables; the oracle evaluates `framepos reftype=site` and `framequat reftype=body` as mj_sensorPos does."""
    import struct

    from judo_amd.models import load_description, pack_model
    from judo_amd.tasks import CaltechLeapCube, get_registered_tasks
    from oracle import oracle as O

    assert "caltech_leap_cube" in get_registered_tasks()
    d = load_description("caltech_leap_cube")
    assert d["option"]["impratio"] == 1.0 and d["nsensordata"] == 23
    assert sum(g["type"] == "sphere" for g in d["geoms"]) == 4 and sum(g["type"] == "cylinder" for g in d["geoms"]) == 4  # per fingertip: the MJCF's cylinder + sphere
    b = pack_model(d)
    h = struct.unpack("<16I", b[:64])
    nf, ni = h[8], h[9]
    F = np.frombuffer(b[64 : 64 + 4 * nf], dtype=np.float32)
    I = np.frombuffer(b[64 + 4 * nf : 64 + 4 * (nf + ni)], dtype=np.int32)
    assert h[6] == 23 and I[7] == 23 and 0 < I[17] <= 128 and I[18] > 0
    np.testing.assert_allclose(F[I[18] : I[18] + 16], [0.11, 0.005, 0.03, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0], atol=1e-7)  # grasp site, goal body
    om = O.Model("caltech_leap_cube")
    t = CaltechLeapCube()
    x = t.default_state()
    q = np.array([0.5, 0.5, -0.5, 0.5])
    x[3:7] = q
    x[0:3] = [0.13, -0.02, 0.08]
    y = om.forward(x[:23], x[23:], np.zeros(16))["sensordata"]
    np.testing.assert_allclose(y[:16], x[7:23], atol=1e-12)
    np.testing.assert_allclose(y[16:19], x[0:3] - np.array([0.11, 0.005, 0.03]), atol=1e-12)
    np.testing.assert_allclose(y[19:23], q, atol=1e-12)


def test_hand_self_collision_pair_tables():
    """MuJoCo's static collision filters on the leap models (same welded body, parent-child unless the parent is welded to the world, the <exclude> pairs, judo/models/xml/
    leap_components/params_and_default.xml:76-101): the oracle's geom pair list and the body-pair table of the packed image describe the same candidate set."""
    import struct

    from judo_amd.models import load_description, pack_model
    from oracle import oracle as O

    for task, n_all, n_cube, n_body_pairs, n_excl in (("leap_cube", 1950, 75, 106, 18), ("leap_cube_down", 1950, 75, 106, 18), ("caltech_leap_cube", 1955, 74, 122, 35)):
        d = load_description(task)
        assert len(d["excludes"]) == n_excl
        pa, pc = O.collision_pairs(d, scope="all"), O.collision_pairs(d, scope="cube")
        assert (len(pa), len(pc)) == (n_all, n_cube) and set(pc) <= set(pa)
        names = [b["name"] for b in d["bodies"]]
        cube = names.index("cube")
        body = [g["body"] for g in d["geoms"]]
        assert all(cube in (body[a], body[b]) for a, b in pc) and not any(cube in (body[a], body[b]) for a, b in set(pa) - set(pc))
        excl = {frozenset(e) for e in d["excludes"]}
        hand = set(pa) - set(pc)
        assert not any(frozenset((body[a], body[b])) in excl or body[a] == body[b] for a, b in hand)
        b = pack_model(d)
        h = struct.unpack("<16I", b[:64])
        I = np.frombuffer(b[64 + 4 * h[8] : 64 + 4 * (h[8] + h[9])], dtype=np.int32)
        assert I[17] == n_body_pairs
        # every body pair of the image expands to (geoms of A) x (geoms of B): the sum over the pairs is the oracle's hand pair count
        bp = I[I[15] : I[15] + 2 * I[17]].reshape(-1, 2)
        rng = I[I[15] + 2 * I[17] : I[15] + 2 * I[17] + 40].reshape(20, 2)
        assert int(sum(rng[a, 1] * rng[c, 1] for a, c in bp)) == len(hand)


def test_exported_mjcf_round_trips(tmp_path):
    """tools/export_mjcf.py writes the model descriptions back out as mesh-free MJCF (what `tools/gen_golden_mujoco.py` hands to MuJoCo to pin the physics
    oracle on ALL tasks the day the wheel is importable).  No MuJoCo here, so the exporter is checked by parsing its output with the MJCF compiler of this
    repository: every number must come back."""
    import json
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import compile_mjcf as CM
    import export_mjcf as EM

    def diff(x, y, path=""):
        if isinstance(y, dict):
            out = []
            for k in set(x) | set(y):
                out += [(path + "/" + k, x.get(k, "<missing>"), y.get(k, "<missing>"))] if (k not in x or k not in y) else diff(x[k], y[k], path + "/" + k)
            return out
        if isinstance(y, list):
            if not isinstance(x, list) or len(x) != len(y):
                return [(path, x, y)]
            return [d for i, (a, b) in enumerate(zip(x, y)) for d in diff(a, b, f"{path}[{i}]")]
        if isinstance(x, float) or isinstance(y, float):
            return [] if (x is not None and y is not None and abs(x - y) <= 1e-14 * max(1.0, abs(y))) else [(path, x, y)]
        return [] if x == y else [(path, x, y)]

    old = CM.REF_XML
    try:
        CM.REF_XML = str(tmp_path)
        for task in EM.TASKS:
            EM.write(task, str(tmp_path))
            got = CM.compile_model(task + ".xml", task)
            with open(os.path.join(ROOT, "judo_amd", "models", task + ".json")) as f:
                ref = json.load(f)
            for d in (got, ref):
                d.pop("source", None); d.pop("family", None)
                d["geoms"] = [{k: v for k, v in g.items() if not k.startswith("substitute")} for g in d["geoms"]]
            assert diff(got, ref) == [], (task, diff(got, ref)[:3])
    finally:
        CM.REF_XML = old


def test_task_index_getters_by_name():
    """judo/tasks/base.py:180-204 (the reference's tests/test_tasks/test_indexing.py: three slide joints -> positions 0, 1, 2, velocities nq + 0, 1, 2, a sensor's address):
    on the shipped models, where free joints (7 / 6 columns) come before hinges."""
    from judo_amd.tasks import get_registered_tasks

    cyl = get_registered_tasks()["cylinder_push"][0]()
    names = [j["name"] for j in cyl.desc["joints"]]
    assert [cyl.get_joint_position_start_index(n) for n in names] == [0, 1, 2, 3]
    assert [cyl.get_joint_velocity_start_index(n) for n in names] == [4, 5, 6, 7]
    assert cyl.get_sensor_start_index("trace_pusher") == 0 and cyl.get_sensor_start_index("trace_cart") == 3
    leap = get_registered_tasks()["leap_cube"][0]()
    jn = [j["name"] for j in leap.desc["joints"]]
    free = next(j["name"] for j in leap.desc["joints"] if j["type"] == "free")
    assert leap.get_joint_position_start_index(free) == 0 and leap.get_joint_velocity_start_index(free) == leap.nq
    first_hinge = next(j["name"] for j in leap.desc["joints"] if j["type"] == "hinge")
    assert leap.get_joint_position_start_index(first_hinge) == 7 and leap.get_joint_velocity_start_index(first_hinge) == leap.nq + 6
    last = jn[-1]
    assert leap.get_joint_position_start_index(last) == leap.nq - 1 and leap.get_joint_velocity_start_index(last) == leap.nq + leap.nv - 1
    assert leap.get_sensor_start_index("trace_cube") == 16
    with pytest.raises(KeyError):
        leap.get_sensor_start_index("no_such_sensor")
    with pytest.raises(KeyError):
        leap.get_joint_position_start_index("no_such_joint")


def test_controller_helper_properties_of_the_reference_exist():
    """judo/controller/controller.py:109-207: the accessors the app layer uses on a Controller (config swaps from the GUI, class lookups)."""
    import inspect

    from judo_amd.controller import Controller

    for name in ("horizon", "nu", "max_num_traces", "max_opt_iters", "spline_order", "spline_data", "action_normalizer_type", "num_timesteps", "rollout_times",
                 "spline_timesteps", "optimizer_cfg", "optimizer_cls", "optimizer_config_cls", "task_config", "time", "controller_cfg"):
        assert isinstance(inspect.getattr_static(Controller, name), property), name
    for name in ("optimizer_cfg", "task_config", "time", "controller_cfg"):
        assert inspect.getattr_static(Controller, name).fset is not None, name
    for name in ("update_action", "action", "update_spline", "reset", "update_traces", "update_states"):
        assert callable(getattr(Controller, name)), name


def test_bench_reads_a_committed_traffic_file():
    """`bench.py`'s `roofline.traffic` / `roofline.issue` come from the round's committed PMC passes (profiles/<TRAFFIC_FILE>, written by tools/collect_profiles.py): the file
    the bench names exists and holds the headline kernel's HBM bytes per launch and its issue-side counters."""
    import json
    import re

    src = open(os.path.join(ROOT, "bench.py")).read()
    name = re.search(r'^TRAFFIC_FILE = "([^"]+)"', src, re.M).group(1)
    t = json.load(open(os.path.join(ROOT, "profiles", name)))
    for case in ("leap_cube", "leap_cube_cube_only", "fr3_pick"):
        assert t[case]["hbm_bytes_per_launch"] > 0 and t[case]["issue"]["cycles_per_valu_instruction_per_simd"] > 2.0, case
