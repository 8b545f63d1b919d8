"""The rest of the AjtaiCommitmentScheme surface without a GPU: commit_coeff, decompose_and_commit_coeff and decompose_and_commit_ntt
(commitment/commitment_scheme.rs:81-113) are declared by include/lfhip.h, exported by liblfhip.so, bound in api.AjtaiCommitmentScheme and wrapped by
HipAjtai in bindings/latticefold-hip with the reference's generics and parameter names; the digit-plane count the gadget commitments use per base."""
import ctypes as C
import inspect
import os
import re

import pytest

from latticefold_amd import api

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SYMS = ("lf_ajtai_commit_coeff", "lf_ajtai_decompose_and_commit_coeff", "lf_ajtai_decompose_and_commit_ntt")
# commitment_scheme.rs:81-113: method -> name of its one parameter (besides &self); all three are generic over P: DecompositionParams
REF_METHODS = {"commit_coeff": "f", "decompose_and_commit_coeff": "f", "decompose_and_commit_ntt": "w"}


def test_header_declares_and_library_exports_the_three_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfhip.h")).read(), flags=re.S)
    lib = api._lib()
    for s in SYMS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), s
        assert s in api.exported_symbols(), s
        assert hasattr(lib, s), s


def test_python_scheme_has_the_methods():
    for name, params in (("commit_coeff", ["self", "f_coeff"]), ("decompose_and_commit_coeff", ["self", "f_coeff", "B", "L"]),
                         ("decompose_and_commit_ntt", ["self", "w", "B", "L"])):
        m = getattr(api.AjtaiCommitmentScheme, name)
        assert list(inspect.signature(m).parameters) == params, name


def _impl_body(src, head):
    m = re.search(re.escape(head) + r"\s*\{", src)
    assert m, head
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
    return src[m.end():i - 1]


def _fn(body, name):
    """(generics, parameter text, body) of `fn name<..>(..) -> .. { .. }`"""
    m = re.search(r"\bfn " + name + r"\s*<([^>]*)>\s*\(", body)
    assert m, name
    depth, i = 1, m.end()
    while depth:
        depth += {"(": 1, ")": -1}.get(body[i], 0)
        i += 1
    params = body[m.end():i - 1]
    j = body.index("{", i)
    depth, k = 1, j + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(body[k], 0)
        k += 1
    return m.group(1), params, body[j + 1:k - 1]


def test_rust_wrapper_has_the_reference_signatures():
    src = open(os.path.join(ROOT, "bindings", "latticefold-hip", "src", "lib.rs")).read()
    body = _impl_body(src, "impl<NTT: SuitableRing> HipAjtai<NTT>")
    sysrs = open(os.path.join(ROOT, "bindings", "latticefold-hip-sys", "src", "lib.rs")).read()
    declared = set(re.findall(r"pub fn (lf_[a-z0-9_]+)\(", sysrs))
    types = {"commit_coeff": r"Vec<NTT::CoefficientRepresentation>", "decompose_and_commit_coeff": r"&\[NTT::CoefficientRepresentation\]",
             "decompose_and_commit_ntt": r"Vec<NTT>"}
    used = set()
    for name, pname in REF_METHODS.items():
        generics, params, fbody = _fn(body, name)
        assert re.fullmatch(r"\s*P\s*:\s*DecompositionParams\s*", generics), (name, generics)
        ps = [p.strip() for p in params.split(",") if p.strip()]
        assert ps[0] == "&self" and len(ps) == 2, (name, ps)
        pn, pt = (x.strip() for x in ps[1].split(":", 1))
        assert pn == pname and re.fullmatch(types[name], pt), (name, ps[1])
        calls = set(re.findall(r"sys::(lf_[a-z0-9_]+)", fbody))
        for helper in re.findall(r"self\.(\w+)::<P>\(", fbody):          # (a private generic helper of the same impl)
            calls |= set(re.findall(r"sys::(lf_[a-z0-9_]+)", _fn(body, helper)[2]))
        assert calls, name
        used |= calls
    assert set(SYMS) <= used, sorted(set(SYMS) - used)
    assert used - {"lf_ctx", "lf_witness"} <= declared, sorted(used - declared)


# commitment planes per base (the table of DESIGN.md, k_ajtai_i8g row): the smallest k with 63 (128^k - 1) / 127 >= min(B/2, (p-1)/2)
PLANES = {"goldilocks": {2: 1, 2**8: 2, 2**15: 3, 2**16: 3, 2**22: 4, 2**31: 5, 2**32: 5, 2**40: 6, 2**48: 7, 2**50: 8, 2**56: 9, 2**63: 10},
          "babybear": {2: 1, 2**8: 2, 2**15: 3, 2**16: 3, 2**22: 4, 2**31: 5, 2**32: 5}}


@pytest.mark.parametrize("ring", ["goldilocks", "babybear"])
def test_digit_planes_per_base(ring):
    f = api._lib().lfdbg_i8g_planes_base
    f.argtypes, f.restype = [C.c_int, C.c_uint64], C.c_uint
    p = {"goldilocks": api.P, "babybear": 15 * 2**27 + 1}[ring]
    for B, k in PLANES[ring].items():
        assert f(api.RING_IDS[ring], B) == k, (ring, B)
        bound = min(B // 2, (p - 1) // 2)
        cap = 63 * (128**k - 1) // 127
        assert cap >= bound and (k == 1 or 63 * (128**(k - 1) - 1) // 127 < bound), (ring, B)
