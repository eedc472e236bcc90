"""The packed image of an articulated model has one written layout, judo_amd/csrc/jh_image.h: its constants against the ones judo_amd/engine_model.py packs with, its
view (`EngineModel::init`, `fits`) and the host's readers against `engine_model.image_offsets` and under the address and undefined-behaviour sanitizers -- a plain g++
build of tests/image_view_check.cpp, nothing loaded into Python -- and, on the GPU, what the library does with an image whose view does not fit (no kernel runs)."""

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from judo_amd import engine_model as em
from judo_amd import models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "judo_amd", "csrc")
# the six shipped images: name -> (description, fingertips, self_collision), and what jh_model_build / jh_model_fr3_build report of them (tests/test_gpu_leap_cylinder.py,
# tests/test_gpu_fr3_self_collision.py): four fingertip cylinders, the 112 pairs of the arm with itself
IMAGES = {"leap_cube": ("leap_cube", None, False), "leap_cube_down": ("leap_cube_down", None, False), "caltech_box_tips": ("caltech_leap_cube", "sphere", False),
          "caltech_cylinder_tips": ("caltech_leap_cube", "cylinder", False), "fr3_pick": ("fr3_pick", None, False), "fr3_pick_self": ("fr3_pick", None, True)}
CYLINDERS = {"caltech_cylinder_tips": 4}
ARM_PAIRS = {"fr3_pick_self": 112}


def packed(name: str) -> bytes:
    task, tips, self_collision = IMAGES[name]
    d = models.load_description(task)
    return em.pack_engine_model(dict(d, self_collision=True) if self_collision else d, fingertips=tips)


def header_constants() -> dict:
    """Every `constexpr int A = 1, B = 2;` and every enumerator of jh_image.h, evaluated in order (a value may name an earlier constant)."""
    text = re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "jh_image.h")).read()), flags=re.S)
    out: dict = {}
    for m in re.finditer(r"constexpr\s+int\s+([^;]+);|enum\s*\{([^}]*)\}", text):
        nxt = 0
        for item in (m.group(1) or m.group(2)).split(","):
            name, _, val = (x.strip() for x in item.partition("="))
            if not name:
                continue
            assert m.group(2) is not None or val, item  # (a constexpr has its value)
            out[name] = nxt = int(eval(val, {"__builtins__": {}}, dict(out))) if val else nxt
            nxt += 1
    return out


def test_python_and_the_header_agree():
    """Every name both sides define has one value; the sides define the same header and generic-block slots; and every header slot that `pack_engine_model` writes on
    a shipped image has a name."""
    H = header_constants()
    P = {k: v for k, v in vars(em).items() if re.fullmatch(r"[A-Z][A-Z0-9_]*", k) and isinstance(v, int) and not isinstance(v, bool)}
    P.update(JH_PT_MAX=em.PT_MAX, JH_PT_I=em.PT_I, JH_PT_LEN=1 + em.PT_MAX * em.PT_I)  # (the pair tables' constants carry the library's prefix in the header)
    both = sorted(set(H) & set(P))
    assert [k for k in both if H[k] != P[k]] == [], {k: (H[k], P[k]) for k in both if H[k] != P[k]}
    slots = lambda D: {k: v for k, v in D.items() if k.startswith(("HI_", "GI_"))}  # noqa: E731
    assert slots(H) == slots(P) and sorted(v for k, v in H.items() if k.startswith("HI_")) == list(range(22))
    for k in ("HEADER_I", "HEADER_F", "BODY_I", "GEOM_I", "ACT_I", "BLOCK_I", "SENS_I", "EQ_I", "BODY_F", "DOF_F", "ACT_F", "GEOM_F", "SITE_F", "EQ_F", "FRAME_F", "GP_F", "LANES",
              "BODY_CODES", "BV_F", "REF_F", "GEN_I", "JFREE", "JSLIDE", "JHINGE", "GBOX", "GSPHERE", "GCAPSULE", "GCYLINDER", "BF_LPOS", "BF_LR", "BF_AXIS", "DF_LIMITED", "DF_LO",
              "DF_HI", "GF_SIZE", "GF_POS", "GF_R", "GF_RBOUND", "JH_PT_MAX", "JH_PT_I", "JH_PT_LEN"):
        assert k in both, k
    named = {v for k, v in H.items() if k.startswith("HI_")}
    for name in IMAGES:
        I = em.blob_sections(packed(name))[1]
        assert set(np.flatnonzero(I[: em.HEADER_I]).tolist()) <= named, name


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine: tests/image_view_check.cpp is built with the host compiler's sanitizers")
    exe = str(tmp_path_factory.mktemp("image_view") / "image_view_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "image_view_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


@pytest.mark.parametrize("name", list(IMAGES))
def test_the_view_and_the_readers_under_sanitizers(checker, tmp_path, name):
    """`fits` holds and every offset is `image_offsets`'; the readers count what the library reports today; `pair_tables_shared(x, x)`; then each named count and offset
    of the header and of the generic block set to -1, nint, nfloat and 0x7fffffff, and each section cut short by a word: the view does not fit or a reader says
    malformed, every time, and the sanitizers have nothing to report (a report ends the program with a status of its own)."""
    blob = packed(name)
    path = tmp_path / "image.bin"
    path.write_bytes(blob)
    r = subprocess.run([checker, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [ln for ln in lines if ln[0] == "undetected"] == []
    out = {k: int(v) for k, v in lines}
    assert out.pop("fits") == 1
    I = em.blob_sections(blob)[1]
    want = vars(em.image_offsets(I))
    assert len(want) == 47 and {k: out[k] for k in want} == want
    assert out["cylinders"] == CYLINDERS.get(name, 0) and out["arm_pairs"] == ARM_PAIRS.get(name, 0)
    assert out["pair_tables"] == (1 + em.PT_MAX * em.PT_I if name.startswith(("leap", "caltech")) else 0) and out["shared_with_itself"] == 1
    assert out["mutations"] == 4 * (18 + 6) + 2 and out["undetected_mutations"] == 0


@pytest.mark.gpu
def test_an_image_whose_view_does_not_fit_is_a_model_that_no_launcher_accepts(gpu):
    """A leap image whose body-pair offset is the int section's length (the kernel would read its pairs behind the section) and an fr3 image whose generic block starts
    four ints before the end (the acceptance test read its counts behind it): jh_model_create makes a model of each, as it always has; neither build of the fr3 kernel
    accepts the fr3 one, and a model set refuses the leap one with the launchers' message.  No kernel is launched."""
    from judo_amd import _lib

    L = _lib.lib()

    def create(name, slot, value):
        blob = packed(name)
        F, I = em.blob_sections(blob)
        J = I.copy()
        J[slot] = value(I)
        bad = blob[:64] + F.tobytes() + J.tobytes()
        h = C.c_void_p()
        assert L.jh_model_create(C.create_string_buffer(bad, len(bad)), len(bad), 0, C.byref(h)) == 0, L.jh_last_error()
        return h

    fr3 = create("fr3_pick", em.HI_GI, lambda I: len(I) - 4)
    leap = create("leap_cube", em.HI_BP, lambda I: len(I))
    try:
        out = (C.c_int * 4)()
        assert L.jh_model_fr3_build(fr3, out) == 0 and list(out) == [0, 0, 0, 0]  # the default build is selected, no arm pairs were counted, and neither build accepts
        s = C.c_void_p()
        assert L.jh_model_set_create((C.c_void_p * 1)(leap), 1, C.byref(s)) == -3  # JH_ERR_UNSUPPORTED
        assert "member 0: the leap kernel does not accept this image" in L.jh_last_error().decode()
    finally:
        L.jh_model_destroy(fr3)
        L.jh_model_destroy(leap)
