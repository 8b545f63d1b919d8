"""Relation checks of the LatticeFold+ slice (lfplus_r1cs_check / lfplus_linb_check: R_ComR1CS and R_LinB on the resident (A, f)), the parts that need no GPU:
the two entry points exist in every layer (header, shared library, generated Rust binding, ctypes mirror) and the Python surface is in place."""
import os
import re
import subprocess

from latticefold_amd import plus

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("lfplus_r1cs_check", "lfplus_linb_check")


def test_entry_points_exist_in_every_layer():
    hdr = open(os.path.join(ROOT, "include", "lfplus.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    lib = plus._lib()
    dyn = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "latticefold_amd", "liblfhip.so")], check=True, capture_output=True, text=True).stdout
    for n in NAMES:
        assert re.search(r"\bint %s\(lfplus_ctx \*ctx" % n, hdr), f"{n} is not declared in include/lfplus.h"
        assert n in plus.exported_symbols()
        assert re.search(r"\bT %s$" % n, dyn, flags=re.M), f"liblfhip.so does not export {n}"
        assert hasattr(lib, n), f"liblfhip.so does not export {n}"
        assert re.search(r"pub fn %s\(" % n, rs), f"{n} is missing from the generated Rust binding"
        assert getattr(lib, n).argtypes is not None, f"{n} has no argtypes in plus.py"
    assert len(lib.lfplus_r1cs_check.argtypes) == 9 and len(lib.lfplus_linb_check.argtypes) == 12
    for bit in ("LFPLUS_REL_CM = 1", "LFPLUS_REL_R1CS = 2", "LFPLUS_REL_V = 4", "LFPLUS_REL_NORM = 8"):
        assert bit in hdr
        assert re.search(r"pub const %s: c_int = %s;" % tuple(bit.split(" = ")), rs), f"{bit} is missing from the generated Rust binding"
    assert (plus.REL_CM, plus.REL_R1CS, plus.REL_V, plus.REL_NORM) == (1, 2, 4, 8)


def test_python_surface():
    for meth in ("r1cs_check", "linb_check"):
        assert callable(getattr(plus.PlusContext, meth))
    assert callable(plus.ComR1CS.check_relation) and callable(plus.PlusProver.decide)
    import inspect
    sig = inspect.signature(plus.PlusContext.r1cs_check)
    assert isinstance(sig.parameters["M"].default, type(plus.RESIDENT(3))) and len(sig.parameters["M"].default) == 3 and sig.parameters["bound"].default == 0
    assert inspect.signature(plus.PlusContext.linb_check).parameters["M"].default == ()
