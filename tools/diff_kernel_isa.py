#!/usr/bin/env python3
"""Diff the gfx950 machine code of kernels between two builds of one translation unit.

    hipcc --offload-arch=gfx950 $(CXXFLAGS) -x hip --cuda-device-only -S -o before.s lf_kernels.hip    (at the parent commit)
    hipcc ...                                                             -o after.s  lf_kernels.hip    (at the new one)
    tools/diff_kernel_isa.py before.s after.s pairs.txt [-v]

pairs.txt: one kernel per line, `old<TAB>new`, each a substring that selects exactly one demangled kernel name of its file (a kernel whose name did not
change needs one column).  Per pair the instruction stream between the kernel's label and its end marker is compared after the kernel's own mangled name
and the function number in local labels are rewritten, and with it the metadata: VGPRs, SGPRs, LDS bytes, scratch bytes.  The tool only diffs; it looks for
no instruction.  Output: a markdown table; -v prints the unified diff of the streams that differ.  Exit status 1 if any pair differs.
"""
import difflib, re, subprocess, sys

META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def kernels(path):
    """{demangled name: (stream lines, metadata dict)} of every kernel in an assembly file"""
    text = open(path).read()
    lines = text.split("\n")
    names = re.findall(r"^\t\.amdhsa_kernel (\S+)$", text, re.M)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    meta = {}
    for blk in text[text.index("amdhsa.kernels:"):].split("\n  - ")[1:]:
        kv = dict(re.findall(r"^\s+(\.\w+):\s+(\S+)$", blk, re.M))
        if ".name" in kv:
            meta[kv[".name"]] = {k: int(kv[k]) for k in META}
    out = {}
    for name, d in zip(names, dem):
        a = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        b = next(i for i in range(a, len(lines)) if lines[i].startswith((".Lfunc_end", "\t.section\t.rodata")))   # (the kernel descriptor follows the code)
        body = []
        for l in lines[a + 1:b]:
            l = l.split(";")[0].rstrip().replace(name, "KERNEL")
            l = re.sub(r"\.L(BB|tmp|JTI)\d+_", r".L\1_", l)
            if l.strip():
                body.append(l)
        out[d] = (body, meta[name])
    return out


def pick(ks, sub, path):
    hit = [k for k in ks if sub in k]
    if len(hit) != 1:
        sys.exit(f"{path}: '{sub}' selects {len(hit)} kernels: {hit}")
    return hit[0]


def main():
    verbose = "-v" in sys.argv
    before_s, after_s, pairs = [a for a in sys.argv[1:] if a != "-v"]
    kb, ka = kernels(before_s), kernels(after_s)
    differ = 0
    print("| kernel (before -> after) | stream identical | VGPR | SGPR | LDS | scratch |\n|---|---|---|---|---|---|")
    for line in open(pairs):
        if not line.strip() or line.startswith("#"):
            continue
        cols = line.rstrip("\n").split("\t")
        nb, na = pick(kb, cols[0], before_s), pick(ka, cols[-1], after_s)
        (sb, mb), (sa, ma) = kb[nb], ka[na]
        same = sb == sa
        differ += not same or mb != ma
        short = lambda n: n.split("(")[0].replace("void ", "")
        label = short(nb) if short(nb) == short(na) else f"{short(nb)} -> {short(na)}"
        print(f"| `{label}` | {'yes' if same else 'NO'} ({len(sb)} / {len(sa)}) | " + " | ".join(f"{mb[k]} / {ma[k]}" for k in META) + " |")
        if verbose and not same:
            sys.stderr.write("\n".join(difflib.unified_diff(sb, sa, nb, na, lineterm="", n=2)) + "\n")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
