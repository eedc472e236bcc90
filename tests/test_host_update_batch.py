"""The three batched entries of the Spot fleet (include/judo_amd.h) are declared in the header, exported by the built library and bound in judo_amd._lib.  No GPU."""

import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jh_spline_controls_batch", "jh_update_fused_batch", "jh_policy_rollout_batch")


def test_batched_entries_are_declared_exported_and_bound():
    from judo_amd import _lib

    header = open(os.path.join(ROOT, "include", "judo_amd.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)  # (loading needs no GPU)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", header), f"{name} is not declared in include/judo_amd.h"
        assert hasattr(L, name), f"{name} is not exported by {_lib.LIB_PATH}"
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(_lib.lib(), name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
    # the argument counts of the bindings are those of the declarations
    for name in NEW:
        decl = re.search(rf"\bint\s+{name}\s*\(([^;]*)\);", header).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(getattr(_lib.lib(), name).argtypes), name

