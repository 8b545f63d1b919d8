"""The chained NIFS prover object (lf_prover_*, include/lfhip_prover.h) without a GPU: every entry point is declared by the header lfhip.h includes, exported by
liblfhip.so, prototyped by latticefold_amd.api, bound by module `prover` of the -sys crate and the block of INTEGRATION.md generated from the header, and called by
the safe crate's HipChainProver; the NULL forms are harmless; the ABI version is the header's."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

from latticefold_amd import api

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NAMES = ("lf_prover_create", "lf_prover_destroy", "lf_prover_last_error", "lf_prover_init", "lf_prover_resume", "lf_prover_resume_dev", "lf_prover_ingest",
         "lf_prover_ingest_dev", "lf_prover_check_fresh", "lf_prover_prove", "lf_prover_accumulator", "lf_prover_accumulator_dev", "lf_prover_decide",
         "lf_prover_steps")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_rust_bindings", os.path.join(ROOT, "tools", "gen_rust_bindings.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_header_is_included_and_declares_the_object():
    main = open(os.path.join(ROOT, "include", "lfhip.h")).read()
    assert main.index('extern "C" {') < main.index('#include "lfhip_prover.h"') < main.rindex("#ifdef __cplusplus"), "included inside the extern C block"
    assert api.exported_symbols("lfhip_prover.h") == sorted(NAMES)
    for other in ("lfhip.h", "lfhip_parts.h", "lfhip_sumcheck.h"):
        assert not set(NAMES) & set(api.exported_symbols(other)), other
    hdr = open(os.path.join(ROOT, "include", "lfhip_prover.h")).read()
    assert re.search(r"typedef struct lf_prover lf_prover;", hdr) and re.search(r"enum \{ LF_PROVER_COMMIT_INLINE = 1 \};", hdr)


def test_library_exports_every_name():
    dyn = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "latticefold_amd", "liblfhip.so")], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(lf_prover_[a-z_]+)$", dyn, re.M))
    assert exported == set(NAMES)


def test_python_surface():
    lib = api._lib()
    for n in NAMES:
        assert getattr(lib, n).argtypes is not None, f"{n} has no ctypes prototype"
    for meth in ("create", "init", "resume", "ingest", "check_fresh", "prove", "accumulator", "decide", "steps", "close", "last_error"):
        assert callable(getattr(api.NIFSChainProver, meth)), meth
    assert api.NIFSChainProver.COMMIT_INLINE == 1
    assert issubclass(api.ChainProverError, api.LfError)


def test_rust_bindings_are_generated_from_the_header():
    gen = _gen()
    text, fns = gen.generate_prover()
    assert tuple(fns) == NAMES                                            # (header order)
    assert open(gen.PROVER_OUT).read() == text, "run tools/gen_rust_bindings.py --write"
    assert "pub const LF_PROVER_COMMIT_INLINE: c_uint = 1;" in text and "pub struct lf_prover" in text
    doc = open(gen.DOC).read()
    block = doc[doc.index(gen.PROVER_BEGIN) + len(gen.PROVER_BEGIN):doc.index(gen.PROVER_END)]
    assert block.strip() == ("```rust\n" + text + "```").strip(), "run tools/gen_rust_bindings.py --write"
    assert "pub mod prover;" in open(gen.OUT).read()
    root_rs = open(gen.OUT).read()
    for n in NAMES:
        assert len(re.findall(r"pub fn " + n + r"\(", text)) == 1 and not re.search(r"pub fn " + n + r"\(", root_rs), n


def test_safe_crate_owns_the_handle():
    lib_rs = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "lib.rs")).read()
    assert re.search(r"^pub mod chain;", lib_rs, re.M) and "pub use chain::HipChainProver;" in lib_rs
    safe = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "chain.rs")).read()
    assert "use sys::prover as raw;" in safe
    assert set(re.findall(r"raw::(lf_prover_[a-z_]+)\(", safe)) == set(NAMES)
    assert re.search(r"pub struct HipChainProver<'ctx, NTT, P> \{\s*ctx: &'ctx HipContext,", safe), "borrows the context with a lifetime"
    assert re.search(r"impl<'ctx, NTT, P> Drop for HipChainProver<'ctx, NTT, P>", safe) and "raw::lf_prover_destroy(self.raw)" in safe
    assert "HipError::Lib(format!(\"{what}: {msg}\"), rc)" in safe, "the error code is carried through"
    for meth in ("create", "init", "resume", "resume_dev", "ingest", "ingest_dev", "check_fresh", "prove", "accumulator", "accumulator_dev", "decide", "steps"):
        assert re.search(r"pub (unsafe )?fn " + meth + r"\(", safe), meth


def test_null_forms():
    lib = api._lib()
    h = C.c_void_p()
    assert lib.lf_prover_create(None, 0, C.byref(h)) == -1 and h.value is None       # LF_ERR_INVALID
    assert lib.lf_prover_create(None, 0, None) == -1
    lib.lf_prover_destroy(None)
    msg = lib.lf_prover_last_error(None)
    assert isinstance(msg, bytes) and msg
    assert lib.lf_prover_steps(None) == 0
    for call in (lambda: lib.lf_prover_init(None, None, None, None, None, None), lambda: lib.lf_prover_resume(None, None, None),
                 lambda: lib.lf_prover_resume_dev(None, None, None), lambda: lib.lf_prover_ingest(None, None, None), lambda: lib.lf_prover_ingest_dev(None, None, None),
                 lambda: lib.lf_prover_check_fresh(None, 0, None, None), lambda: lib.lf_prover_prove(None, None, None, None, None),
                 lambda: lib.lf_prover_accumulator(None, None, None), lambda: lib.lf_prover_accumulator_dev(None, None, None), lambda: lib.lf_prover_decide(None, 0, None)):
        assert call() == -1


def test_abi_version_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "lfhip.h")).read()
    assert api.abi_version() == int(re.search(r"#define LFHIP_ABI_VERSION (\d+)", hdr).group(1))
    sysrs = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    assert f"pub const LFHIP_ABI_VERSION: c_int = {api.abi_version()};" in sysrs
