"""ctypes binding of `libjudo_amd.so` (the C ABI declared in `include/judo_amd.h`).

There is no fallback: if the HIP library is missing the import of any compute entry point raises.
Build it with `python -c "import __graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).
"""

from __future__ import annotations

import ctypes as C
import glob
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JUDO_AMD_LIB") or os.path.join(_HERE, "libjudo_amd.so")  # JUDO_AMD_LIB: alternative build of the same C ABI

_lib: C.CDLL | None = None

_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

# How a C type of the header travels through ctypes.  Scalars and return types map one to one.  Pointers: device memory (`float*`, `void*`) and opaque handles
# (`jh_*` `*`) travel as addresses (tensor.data_ptr(), a handle's value); integer arrays are host arrays and keep their type, so ctypes checks what is passed;
# a pointer to pointers (`jh_model**`, `const float* const*`) is a host array of addresses.
_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "unsigned int": C.c_uint, "unsigned long long": C.c_ulonglong}
_RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "void": None, "const char*": C.c_char_p}
_HOST_ARRAYS = {"int": C.c_int, "unsigned int": C.c_uint, "unsigned long long": C.c_ulonglong, "unsigned char": C.c_ubyte}
# The parameters the rule gets wrong, by (C type, parameter name) or (C type, parameter name, entry name).
_EXCEPTIONS = {
    ("const float*", "weights"): C.POINTER(C.c_float),  # host array read before the call returns (the plant weights of a risk measure)
    ("float*", "ms"): C.POINTER(C.c_float),  # host float that jh_event_elapsed_ms writes before it returns
    ("const unsigned char*", "column_mask"): C.c_void_p,  # device bytes
    ("const unsigned char*", "column_mask_sens"): C.c_void_p,  # device bytes
    ("void* const*", "timing"): C.c_void_p,  # host array of event handles or NULL: callers pass a ctypes array, which an address parameter accepts
}


def _spell(ctype: str) -> str:
    """One spelling per C type: single spaces, every `*` on the word before it (`const float*`, `void* const*`, `jh_model**`)."""
    return re.sub(r"\*(?=\w)", "* ", re.sub(r"\s*\*", "*", " ".join(ctype.split())))


def read_header(text: str, exceptions: dict = _EXCEPTIONS) -> tuple[dict, dict]:
    """The ctypes table {entry: (restype, [argtypes])} of every prototype `ret name(params);` of a C header, and its {"MAX_X": n} from the `#define JH_MAX_X n` lines.
    Raises TypeError for a declaration or a type it has no rule for, naming the entry and the parameter: it never skips an entry."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    limits = {name: int(n) for name, n in re.findall(r"^[ \t]*#[ \t]*define[ \t]+JH_(MAX_\w+)[ \t]+(\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"#\s*ifdef\s+__cplusplus.*?#\s*endif", " ", text, flags=re.S)  # `extern "C" {` and its `}`
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)
    while (stripped := re.sub(r"\{[^{}]*\}", " ", text)) != text:  # bodies of enums and structs (the launcher struct of function pointers is no entry)
        text = stripped
    table = {}
    for decl in map(str.strip, text.split(";")):
        if not decl or re.match(r"(typedef|enum|struct)\b", decl):
            continue
        m = re.fullmatch(r"(.+?)\b(\w+)\s*\((.*)\)", decl, re.S)
        if not m:
            raise TypeError(f"cannot read the declaration `{' '.join(decl.split())}`")
        ret, entry, params = _spell(m.group(1)), m.group(2), m.group(3).strip()
        if ret not in _RETURNS or entry in table:
            raise TypeError(f"{entry}: " + ("declared twice" if entry in table else f"no ctypes rule for the return type `{ret}`"))
        argtypes = []
        for param in [] if params in ("", "void") else params.split(","):
            m = re.fullmatch(r"(.+?)\b(\w+)\s*(\[.*\])?", param.strip(), re.S)  # type, name, `[n]` of an array parameter: `T x[n]` is `T* x`
            ctype, name = (_spell(m.group(1) + ("*" if m.group(3) else "")), m.group(2)) if m else (_spell(param), "")
            base, stars = " ".join(w for w in ctype.replace("*", " ").split() if w != "const"), ctype.count("*")
            address = base in ("float", "void") or base.startswith("jh_")
            named = exceptions.get((ctype, name, entry), exceptions.get((ctype, name)))
            if named is not None:
                argtypes.append(named)
            elif stars == 0 and base in _SCALARS:
                argtypes.append(_SCALARS[base])
            elif stars == 1 and (address or base in _HOST_ARRAYS):
                argtypes.append(C.c_void_p if address else C.POINTER(_HOST_ARRAYS[base]))
            elif stars == 2 and address:
                argtypes.append(C.POINTER(C.c_void_p))
            else:
                raise TypeError(f"{entry}: no ctypes rule for the parameter `{ctype} {name}`")
        table[entry] = (_RETURNS[ret], argtypes)
    return table, limits


def _read_headers() -> tuple[dict, dict]:
    """Every header of include/: judo_amd.h, the boundary, and beside it the hooks of the test build, which the library exports as well."""
    boundary = os.path.join(_INCLUDE, "judo_amd.h")
    if not os.path.exists(boundary):
        raise ImportError(f"{boundary} is missing: the ctypes table of libjudo_amd.so is derived from it")
    table, limits = {}, {}
    for path in sorted(glob.glob(os.path.join(_INCLUDE, "*.h"))):
        t, m = read_header(open(path).read())
        if set(t) & set(table):
            raise TypeError(f"{path} declares {sorted(set(t) & set(table))} again")
        table.update(t)
        limits.update(m)
    return table, limits


_SIGNATURES, _LIMITS = _read_headers()
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

# compile-time limits of the library, from the `#define JH_MAX_*` lines of include/judo_amd.h
MAX_KNOT_DIM = _LIMITS["MAX_KNOT_DIM"]  # K * nu
MAX_ELITES = _LIMITS["MAX_ELITES"]  # CEM elites / trace elites
MAX_TASK_PARAMS = _LIMITS["MAX_TASK_PARAMS"]
MAX_ENSEMBLE = _LIMITS["MAX_ENSEMBLE"]  # members of a model set that jh_plan_step_ensemble plans against
MAX_ENSEMBLE_FLEET = _LIMITS["MAX_ENSEMBLE_FLEET"]  # controllers of one jh_plan_step_ensemble_batch call
MAX_PLANT_BLOCKS = _LIMITS["MAX_PLANT_BLOCKS"]  # rollout blocks of one jh_plan_step_randomized call
MAX_FLEET_PLANT_BLOCKS = _LIMITS["MAX_FLEET_PLANT_BLOCKS"]  # B * G, the (controller, block) pairs of one jh_plan_step_randomized_batch call
MAX_ID_HORIZON = _LIMITS["MAX_ID_HORIZON"]  # steps of a recorded window that jh_plant_residuals scores
MAX_ID_QUATS = _LIMITS["MAX_ID_QUATS"]  # quaternions of a state row that jh_plant_residuals aligns


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
