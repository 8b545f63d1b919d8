#!/usr/bin/env python3
"""Generates the raw Rust binding of the C ABI (`latticefold-hip-sys/src/lib.rs`) from include/lfhip.h and include/lfplus.h, and its modules `parts`
(`src/parts.rs`) from include/lfhip_parts.h, the file lfhip.h includes for the entry points of the decomposed witnesses, and `sumcheck` (`src/sumcheck.rs`)
from include/lfhip_sumcheck.h, the one for the generic sumcheck, `prover` (`src/prover.rs`) from include/lfhip_prover.h, the one for the chained prover object,
and `tables` (`src/tables.rs`) from include/lfhip_tables.h, the one for the witness tables.

    python tools/gen_rust_bindings.py            print the binding
    python tools/gen_rust_bindings.py --write    rewrite bindings/latticefold-hip-sys/src/lib.rs and the block between the
                                                 GENERATED markers of INTEGRATION.md; the same for src/parts.rs, src/sumcheck.rs, src/prover.rs, src/tables.rs and their markers

The reference is safe Rust with `#![forbid(unsafe_code)]` (crates/latticefold/src/lib.rs:4): the `extern "C"` block lives in a new
`-sys` crate.  No Rust toolchain exists in the build image, so the text is derived mechanically from the headers (every prototype, the
error enums, `lf_params`, the exchange callback) and tests/test_abi_cpu.py checks that header, binding file and INTEGRATION.md agree
symbol by symbol and that the shared library exports each of them."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("include/lfhip.h", "include/lfplus.h")
OUT = os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")
DOC = os.path.join(ROOT, "INTEGRATION.md")
BEGIN, END = "<!-- BEGIN GENERATED BINDING (tools/gen_rust_bindings.py) -->", "<!-- END GENERATED BINDING -->"
PARTS_HEADER = "include/lfhip_parts.h"
PARTS_OUT = os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "parts.rs")
PARTS_BEGIN, PARTS_END = "<!-- BEGIN GENERATED BINDING: parts (tools/gen_rust_bindings.py) -->", "<!-- END GENERATED BINDING: parts -->"
SUMCHECK_HEADER = "include/lfhip_sumcheck.h"
SUMCHECK_OUT = os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "sumcheck.rs")
SUMCHECK_BEGIN, SUMCHECK_END = "<!-- BEGIN GENERATED BINDING: sumcheck (tools/gen_rust_bindings.py) -->", "<!-- END GENERATED BINDING: sumcheck -->"
PROVER_HEADER = "include/lfhip_prover.h"
PROVER_OUT = os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "prover.rs")
PROVER_BEGIN, PROVER_END = "<!-- BEGIN GENERATED BINDING: prover (tools/gen_rust_bindings.py) -->", "<!-- END GENERATED BINDING: prover -->"
TABLES_HEADER = "include/lfhip_tables.h"
TABLES_OUT = os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "tables.rs")
TABLES_BEGIN, TABLES_END = "<!-- BEGIN GENERATED BINDING: tables (tools/gen_rust_bindings.py) -->", "<!-- END GENERATED BINDING: tables -->"

SCALARS = {
    "int": "c_int", "unsigned": "c_uint", "unsigned int": "c_uint", "char": "c_char", "float": "f32", "double": "f64", "void": "c_void",
    "size_t": "usize", "uint64_t": "u64", "uint32_t": "u32", "uint8_t": "u8", "int8_t": "i8", "int32_t": "i32", "int64_t": "i64",
}
OPAQUE = ["lf_ctx", "lf_witness", "lf_witness_job", "lf_transcript", "lfplus_ctx", "lfplus_transcript", "lfplus_prover"]
PROVER_OPAQUE = ["lf_prover"]     # declared by module `prover`, not by the crate root
KEYWORDS = {"in": "inp", "type": "ty", "ref": "r", "fn": "f", "mod": "m", "box": "b", "use": "u", "loop": "lp", "match": "mt", "move": "mv", "self": "this"}


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def rust_type(ctype):
    """`const uint64_t *const *` -> `*const *const u64`"""
    toks = re.findall(r"\*|[A-Za-z_][A-Za-z_0-9]*", ctype)
    base, quals, ptrs = [], False, []          # ptrs: constness of the pointee at each level, innermost first
    pending_const = False
    for t in toks:
        if t == "const":
            pending_const = True
        elif t == "*":
            ptrs.append(pending_const)
            pending_const = False
        elif t == "struct":
            continue
        else:
            base.append(t)
    name = " ".join(base)
    if name in SCALARS:
        r = SCALARS[name]
    elif name in OPAQUE or name in PROVER_OPAQUE or name in ("lf_params", "lfplus_params", "lf_vpoly", "lfplus_vpoly", "lfplus_ccs"):
        r = name
    elif name in ("lf_exchange_fn", "lfplus_exchange_fn"):
        r = "lf_exchange_fn"
    else:
        raise ValueError(f"unknown C type {ctype!r}")
    # C reads inside-out: `const T *const *p`: first `*` points at const T, second `*` points at a const pointer.  The constness of level i's
    # pointee is the `const` seen before that `*` -- for the first level that is the base type's const.
    for is_const in ptrs:
        r = ("*const " if is_const else "*mut ") + r
    return r


def split_params(s):
    s = s.strip()
    if s in ("", "void"):
        return []
    out = []
    for i, p in enumerate(x.strip() for x in s.split(",")):
        m = re.match(r"^(.*?)([A-Za-z_][A-Za-z_0-9]*)?$", p)
        ctype, name = m.group(1).strip(), m.group(2)
        if name in SCALARS or name in OPAQUE or name in PROVER_OPAQUE or name in ("lf_params", "lfplus_params", "lf_vpoly", "lfplus_vpoly", "lfplus_ccs", "lf_exchange_fn", "lfplus_exchange_fn", "unsigned", "const") or not ctype:   # unnamed parameter
            ctype, name = p, None
        if name is None:
            base = re.findall(r"[A-Za-z_][A-Za-z_0-9]*", ctype)[-1]
            name = {"lf_ctx": "ctx", "lf_transcript": "t", "lf_witness": "w", "lf_params": "p", "lf_vpoly": "poly", "lfplus_ctx": "ctx", "lfplus_prover": "prover", "lf_prover": "prover"}.get(base, f"a{i}")
        out.append((KEYWORDS.get(name, name), rust_type(ctype)))
    return out


def parse(path):
    text = strip_comments(open(os.path.join(ROOT, path)).read())
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    text = text.replace('extern "C" {', "").replace("\n}\n", "\n")
    enums = []
    for body in re.findall(r"enum\s*\{(.*?)\}\s*;", text, flags=re.S):
        for name, val in re.findall(r"([A-Z_0-9]+)\s*=\s*(-?\d+)", body):
            enums.append((name, int(val)))
    text = re.sub(r"enum\s*\{.*?\}\s*;", "", text, flags=re.S)
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r"typedef[^;]*;", "", text)
    fns = []
    for m in re.finditer(r"([A-Za-z_][A-Za-z_0-9 \*]*?)\b(lf(?:plus)?_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        ret, name, params = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        fns.append((name, split_params(params), None if ret == "void" else rust_type(ret)))
    return enums, fns


def defines(path):
    text = strip_comments(open(os.path.join(ROOT, path)).read())
    out = []
    for name, val in re.findall(r"^\s*#define\s+(LF[A-Z_0-9]*)\s+\(?(-?\d+|0x[0-9A-Fa-f]+)(?:ULL)?\)?\s*$", text, flags=re.M):
        out.append((name, int(val, 0)))
    return out


def generate():
    L = ["// GENERATED by tools/gen_rust_bindings.py from include/lfhip.h and include/lfplus.h -- do not edit.",
         "// latticefold-hip-sys: raw binding of liblfhip.so (MI355X / gfx950).  Every pointer is a HOST pointer, except the array arguments of",
         "// the lf_*_dev / lfplus_*_dev entry points (the caller's device memory: \"device-resident callers\" in both headers); every `c_int` result is 0 or a",
         "// negative LF_ERR_* / LFPLUS_E_* code.  The comments of the headers are the documentation.",
         "#![allow(non_camel_case_types, non_upper_case_globals, non_snake_case)]",
         "use core::ffi::{c_char, c_int, c_uint, c_void};", ""]
    for o in OPAQUE:
        L.append(f"#[repr(C)] pub struct {o} {{ _p: [u8; 0] }}")
    L += ["",
          "/// DecompositionParams + CCS shape (decomposition_parameters.rs:11-20, arith.rs:50-74)",
          "#[repr(C)] #[derive(Clone, Copy, Debug)]",
          "pub struct lf_params { pub s: u32, pub wit_len: u32, pub l: u32, pub L: u32, pub K: u32, pub b: u32, pub B: u64, pub kappa: u32, pub t: u32, pub q: u32, pub d: u32 }",
          "/// PlusParameters with LinParameters / DecompParameters flattened (latticefold-plus plus.rs:43-47, lin.rs:24-28, rgchk.rs:20-24)",
          "#[repr(C)] #[derive(Clone, Copy, Debug)]",
          "pub struct lfplus_params { pub kappa: u32, pub k: u32, pub l: u32, pub b: u64, pub B: u64 }",
          "/// VirtualPolynomial over RqPoly as a flat product list (latticefold utils/sumcheck/utils.rs:24-75; lfplus_mlsumcheck_*): 16 words per coefficient",
          "#[repr(C)] #[derive(Clone, Copy, Debug)]",
          "pub struct lfplus_vpoly { pub nvars: u32, pub ntables: u32, pub nterms: u32, pub degree: u32, pub term_off: *const u32, pub term_idx: *const u32, pub coef: *const u64 }",
          "/// A CCS shape over t matrices (lfplus_ccs_*): sum_i c_i prod_{j in S_idx[S_off[i] .. S_off[i+1])} (M_j f), 16 words per coefficient",
          "#[repr(C)] #[derive(Clone, Copy, Debug)]",
          "pub struct lfplus_ccs { pub t: u32, pub q: u32, pub S_off: *const u32, pub S_idx: *const u32, pub c: *const u64 }",
          "/// all-gather `words` u64 from every rank into recv_all[world * words] in rank order; 0 on success (lf_set_sharding)",
          "pub type lf_exchange_fn = Option<unsafe extern \"C\" fn(user: *mut c_void, send: *const u64, recv_all: *mut u64, words: usize) -> c_int>;", ""]
    allfns = []
    for h in HEADERS:
        enums, fns = parse(h)
        L.append(f"// ---- {h} " + "-" * (100 - len(h)))
        for name, val in defines(h):
            ty = "u64" if val > 2 ** 31 else "c_int"
            L.append(f"pub const {name}: {ty} = {val};")
        for name, val in enums:
            L.append(f"pub const {name}: c_int = {val};")
        L.append('#[link(name = "lfhip")]')
        L.append('extern "C" {')
        for name, params, ret in fns:
            ps = ", ".join(f"{n}: {t}" for n, t in params)
            L.append(f"    pub fn {name}({ps})" + (f" -> {ret}" if ret else "") + ";")
            allfns.append(name)
        L += ["}", ""]
    L += ["/// include/lfhip_parts.h (included by lfhip.h): the decomposed witnesses as handles -- `parts::lf_witness_decompose`, ...", "pub mod parts;",
          "/// include/lfhip_sumcheck.h (included by lfhip.h): MLSumcheck over any sum of products of MLE tables -- `sumcheck::lf_mlsumcheck_prove`, ...",
          "pub mod sumcheck;",
          "/// include/lfhip_prover.h (included by lfhip.h): the chained NIFS prover object -- `prover::lf_prover_create`, `prover::lf_prover_prove`, ...",
          "pub mod prover;",
          "/// include/lfhip_tables.h (included by lfhip.h): f-hat, z, M z, M^T v and fix_variables from a witness handle -- `tables::lf_witness_get_fhat`, ...",
          "pub mod tables;", ""]
    return "\n".join(L), allfns


def generate_parts():
    """src/parts.rs: the entry points of include/lfhip_parts.h, over the types of the crate root"""
    _, fns = parse(PARTS_HEADER)
    L = [f"// GENERATED by tools/gen_rust_bindings.py from {PARTS_HEADER} -- do not edit.",
         "// Module `parts` of latticefold-hip-sys: the decomposed witnesses of LFDecompositionProver / LFFoldingProver as device handles.",
         "use core::ffi::{c_int, c_uint};", "",
         "use super::{lf_ctx, lf_transcript, lf_witness};", "",
         '#[link(name = "lfhip")]', 'extern "C" {']
    for name, params, ret in fns:
        ps = ", ".join(f"{n}: {t}" for n, t in params)
        L.append(f"    pub fn {name}({ps})" + (f" -> {ret}" if ret else "") + ";")
    L += ["}", ""]
    return "\n".join(L), [f[0] for f in fns]


def generate_sumcheck():
    """src/sumcheck.rs: the descriptor and the entry points of include/lfhip_sumcheck.h, over the types of the crate root"""
    _, fns = parse(SUMCHECK_HEADER)
    L = [f"// GENERATED by tools/gen_rust_bindings.py from {SUMCHECK_HEADER} -- do not edit.",
         "// Module `sumcheck` of latticefold-hip-sys: MLSumcheck::prove_as_subprotocol / verify_as_subprotocol over any sum of products of MLE tables.",
         "use core::ffi::c_int;", "",
         "use super::{lf_ctx, lf_transcript};", "",
         "/// VirtualPolynomial as a flat product list (utils/sumcheck/utils.rs:24-75): g = sum_i coef_i prod_{k in [term_off[i], term_off[i+1])} T_{term_idx[k]}",
         "#[repr(C)] #[derive(Clone, Copy, Debug)]",
         "pub struct lf_vpoly { pub nvars: u32, pub ntables: u32, pub nterms: u32, pub degree: u32, pub term_off: *const u32, pub term_idx: *const u32, pub coef: *const u64 }", "",
         '#[link(name = "lfhip")]', 'extern "C" {']
    for name, params, ret in fns:
        ps = ", ".join(f"{n}: {t}" for n, t in params)
        L.append(f"    pub fn {name}({ps})" + (f" -> {ret}" if ret else "") + ";")
    L += ["}", ""]
    return "\n".join(L), [f[0] for f in fns]


def generate_prover():
    """src/prover.rs: the handle, the flag and the entry points of include/lfhip_prover.h, over the types of the crate root"""
    enums, fns = parse(PROVER_HEADER)
    L = [f"// GENERATED by tools/gen_rust_bindings.py from {PROVER_HEADER} -- do not edit.",
         "// Module `prover` of latticefold-hip-sys: NIFSProver::prove chained -- an object that owns the accumulator on the device (lf_prover_*).",
         "use core::ffi::{c_char, c_int, c_uint};", "",
         "use super::{lf_ctx, lf_transcript};", ""]
    for o in PROVER_OPAQUE:
        L.append(f"#[repr(C)] pub struct {o} {{ _p: [u8; 0] }}")
    for name, val in enums:
        L.append(f"pub const {name}: c_uint = {val};")
    L += ["", '#[link(name = "lfhip")]', 'extern "C" {']
    for name, params, ret in fns:
        ps = ", ".join(f"{n}: {t}" for n, t in params)
        L.append(f"    pub fn {name}({ps})" + (f" -> {ret}" if ret else "") + ";")
    L += ["}", ""]
    return "\n".join(L), [f[0] for f in fns]


def generate_tables():
    """src/tables.rs: the entry points of include/lfhip_tables.h, over the types of the crate root"""
    _, fns = parse(TABLES_HEADER)
    L = [f"// GENERATED by tools/gen_rust_bindings.py from {TABLES_HEADER} -- do not edit.",
         "// Module `tables` of latticefold-hip-sys: the protocol's own tables from a witness handle (f-hat, z, M z), M^T v and fix_variables on tables; the",
         "// array arguments of the *_device functions are the caller's device memory.",
         "use core::ffi::{c_int, c_uint};", "",
         "use super::{lf_ctx, lf_witness};", "",
         '#[link(name = "lfhip")]', 'extern "C" {']
    for name, params, ret in fns:
        ps = ", ".join(f"{n}: {t}" for n, t in params)
        L.append(f"    pub fn {name}({ps})" + (f" -> {ret}" if ret else "") + ";")
    L += ["}", ""]
    return "\n".join(L), [f[0] for f in fns]


def main():
    text, fns = generate()
    if "--write" in sys.argv:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        open(OUT, "w").write(text)
        doc = open(DOC).read()
        if BEGIN in doc and END in doc:
            a, b = doc.index(BEGIN) + len(BEGIN), doc.index(END)
            doc = doc[:a] + "\n```rust\n" + text + "```\n" + doc[b:]
            open(DOC, "w").write(doc)
        ptext, pfns = generate_parts()
        open(PARTS_OUT, "w").write(ptext)
        doc = open(DOC).read()
        if PARTS_BEGIN in doc and PARTS_END in doc:
            a, b = doc.index(PARTS_BEGIN) + len(PARTS_BEGIN), doc.index(PARTS_END)
            open(DOC, "w").write(doc[:a] + "\n```rust\n" + ptext + "```\n" + doc[b:])
        print(f"{len(pfns)} functions -> {os.path.relpath(PARTS_OUT, ROOT)}")
        stext, sfns = generate_sumcheck()
        open(SUMCHECK_OUT, "w").write(stext)
        doc = open(DOC).read()
        if SUMCHECK_BEGIN in doc and SUMCHECK_END in doc:
            a, b = doc.index(SUMCHECK_BEGIN) + len(SUMCHECK_BEGIN), doc.index(SUMCHECK_END)
            open(DOC, "w").write(doc[:a] + "\n```rust\n" + stext + "```\n" + doc[b:])
        print(f"{len(sfns)} functions -> {os.path.relpath(SUMCHECK_OUT, ROOT)}")
        rtext, rfns = generate_prover()
        open(PROVER_OUT, "w").write(rtext)
        doc = open(DOC).read()
        if PROVER_BEGIN in doc and PROVER_END in doc:
            a, b = doc.index(PROVER_BEGIN) + len(PROVER_BEGIN), doc.index(PROVER_END)
            open(DOC, "w").write(doc[:a] + "\n```rust\n" + rtext + "```\n" + doc[b:])
        print(f"{len(rfns)} functions -> {os.path.relpath(PROVER_OUT, ROOT)}")
        ttext, tfns = generate_tables()
        open(TABLES_OUT, "w").write(ttext)
        doc = open(DOC).read()
        if TABLES_BEGIN in doc and TABLES_END in doc:
            a, b = doc.index(TABLES_BEGIN) + len(TABLES_BEGIN), doc.index(TABLES_END)
            open(DOC, "w").write(doc[:a] + "\n```rust\n" + ttext + "```\n" + doc[b:])
        print(f"{len(tfns)} functions -> {os.path.relpath(TABLES_OUT, ROOT)}")
        print(f"{len(fns)} functions -> {os.path.relpath(OUT, ROOT)}" + (", INTEGRATION.md" if BEGIN in doc else ""))
    else:
        sys.stdout.write(text)
        sys.stdout.write(generate_parts()[0])
        sys.stdout.write(generate_sumcheck()[0])
        sys.stdout.write(generate_prover()[0])
        sys.stdout.write(generate_tables()[0])


if __name__ == "__main__":
    main()
