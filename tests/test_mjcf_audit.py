"""The model compiler may not silently drop a physics attribute of the reference's MJCF files (rounds 1-3 dropped `euler` on nine geoms of the Spot arm -- wrong in the
oracle AND in the kernel, every parity test green).  The MJCF files are not part of this repository: the audit reads their attribute census
(tests/golden/mjcf_attributes.json, tools/diag/mjcf_attribute_audit.py --write-census), the refusals are shown on a small model of our own (STAND_IN)."""
import importlib.util
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one body on a hinge with a sphere and a motor: it compiles as it stands, so every refusal below is the patched attribute's
STAND_IN = """<mujoco model="stand_in">
  <compiler angle="radian"/>
  <option timestep="0.01"/>
  <worldbody>
    <body name="pole" pos="0 0 1">
      <joint name="hinge" type="hinge" axis="0 1 0"/>
      <geom name="bob" type="sphere" size="0.1"/>
    </body>
  </worldbody>
  <actuator>
    <motor name="torque" joint="hinge"/>
  </actuator>
</mujoco>
"""


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    return mod


def test_every_non_visual_attribute_of_the_shipped_mjcf_is_read_by_the_compiler():
    audit = _load(os.path.join(ROOT, "tools", "diag", "mjcf_attribute_audit.py"), "mjcf_attribute_audit")
    with open(audit.CENSUS) as f:
        seen = json.load(f)
    assert set(seen) >= {"body", "geom", "joint", "option", "compiler", "position", "framepos"} and "euler" in seen["geom"]  # the census covers the seven models
    assert audit.unread_non_visual(seen) == {}, "tools/compile_mjcf.py never reads these attributes: implement them or raise on a non-default value"


@pytest.mark.parametrize("xml_name,tag,attr,value", [
    ("spot_primitive/robot.xml", "option", "solver", "CG"),
    ("spot_primitive/robot.xml", "compiler", "autolimits", "false"),
    ("spot_primitive/robot.xml", "option", "density", "1000"),
    ("spot_primitive/robot.xml", "body", "gravcomp", "1"),
    ("leap_cube.xml", "body", "zaxis", "0 0 1"),
    ("spot_primitive/robot.xml", "geom", "contype", "2"),  # mixed collision masks: the pair lists apply MuJoCo's body-level filters only
])
def test_a_value_the_engines_do_not_model_is_refused(monkeypatch, tmp_path, xml_name, tag, attr, value):
    C = _load(os.path.join(ROOT, "tools", "compile_mjcf.py"), "compile_mjcf_audit")
    (tmp_path / xml_name).parent.mkdir(parents=True, exist_ok=True)
    (tmp_path / xml_name).write_text(STAND_IN)
    monkeypatch.setattr(C, "REF_XML", str(tmp_path))
    assert C.compile_model(xml_name, "x")["joints"][0]["name"] == "hinge"
    load = C.load_xml

    def patched(path):
        root = load(path)
        el = root if root.tag == tag else next(root.iter(tag))
        el.set(attr, value)
        return root

    monkeypatch.setattr(C, "load_xml", patched)
    with pytest.raises(NotImplementedError):
        C.compile_model(xml_name, "x")
