#!/usr/bin/env python3
"""Record the NAMES the safe Rust wrapper (bindings/latticefold-hip) has to match: the parameter names of each `prove` of the reference's three prover
traits and of NIFSProver, and the required methods of its transcript traits.

    python tests/tools/extract_reference_signatures.py <checkout of NethermindEth/latticefold>

Writes tests/golden/reference_signatures.json (names only; no reference source text is stored), which tests/test_rust_wrapper_cpu.py reads.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from test_rust_wrapper_cpu import _fn_sig  # noqa: E402  (the same signature parser the test applies to the wrapper)

OUT = os.path.join(HERE, "..", "golden", "reference_signatures.json")
# (file under crates/latticefold/src, pattern of the trait / impl whose `prove` is recorded)
CASES = [("nifs/linearization.rs", r"pub trait LinearizationProver<"),
         ("nifs/decomposition/structs.rs", r"pub trait DecompositionProver<"),
         ("nifs/folding/structs.rs", r"pub trait FoldingProver<"),
         ("nifs.rs", r"impl<NTT: SuitableRing, P: DecompositionParams, T: TranscriptWithShortChallenges<NTT>>\s*NIFSProver<NTT, P, T>\s*\{")]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src = os.path.join(sys.argv[1], "crates", "latticefold", "src")
    read = lambda rel: open(os.path.join(src, rel)).read()
    out = {"source": "crates/latticefold/src of NethermindEth/latticefold: parameter names of `prove` (nifs/linearization.rs:26-52, "
                     "nifs/decomposition/structs.rs:48-64, nifs/folding/structs.rs:43-70, nifs.rs:48-103) and the required methods of transcript.rs",
           "prove_params": {rel: _fn_sig(read(rel), pat) for rel, pat in CASES},
           "transcript_required_methods": re.findall(r"\n    fn (\w+)\([^)]*\)[^{;]*;", read("transcript.rs"))}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", os.path.normpath(OUT))


if __name__ == "__main__":
    main()
