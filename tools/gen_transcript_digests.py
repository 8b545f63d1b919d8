"""Digests of the host transcripts' squeeze_bytes output on a fixed script (no GPU needed):

    python tools/gen_transcript_digests.py            # prints the JSON of tests/golden/host_transcript_digests.json
    python tools/gen_transcript_digests.py --write    # rewrites that file

The library is latticefold_amd/liblfhip.so or $LFHIP_LIB (as tools/time_poseidon.py), so the file can be regenerated from any build.  The
oracle only squeezes challenge-sized amounts on the Goldilocks and BabyBear transcripts; this script pins what the library itself answers
for long absorbs and for squeezes around and beyond one block of the rate (20 words), which tests/test_abi_cpu.py replays.
"""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_transcript_digests.json")
RINGS = {"goldilocks": (0, 7), "babybear": (1, 3)}      # ABI ring id, usable bytes per squeezed field element
SQUEEZE_WORDS = (1, 19, 20, 21, 40, 41, 45)
M64 = (1 << 64) - 1


def splitmix64(seed):
    x = seed & M64
    while True:
        x = (x + 0x9E3779B97F4A7C15) & M64
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        yield z ^ (z >> 31)


def load(path=None):
    lib = C.CDLL(path or os.environ.get("LFHIP_LIB") or os.path.join(ROOT, "latticefold_amd", "liblfhip.so"))
    lib.lf_transcript_new_ring.restype = C.c_void_p
    lib.lf_transcript_new_ring.argtypes = [C.c_int]
    lib.lf_transcript_free.argtypes = [C.c_void_p]
    lib.lf_transcript_absorb_fq.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.lf_transcript_squeeze_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.lf_transcript_squeeze_bytes.restype = None
    return lib


def digest(lib, ring):
    """The script: absorbs of 1..70 full 64-bit words (NOT reduced mod p: 70 lengths in a seeded order), each followed by one to three squeezes
    of SQUEEZE_WORDS words' worth of bytes in a seeded order -- so squeezes follow absorbs and squeezes, with the rate index anywhere including
    exactly at the end of a block, and absorbs follow squeezes that stopped inside and at the end of a block."""
    ring_id, usable = RINGS[ring]
    rng = splitmix64(0x5EED0000 + ring_id)
    lengths = list(range(1, 71))
    for i in range(len(lengths) - 1, 0, -1):            # Fisher-Yates
        j = next(rng) % (i + 1)
        lengths[i], lengths[j] = lengths[j], lengths[i]
    t = lib.lf_transcript_new_ring(ring_id)
    h = hashlib.sha256()
    try:
        for n in lengths:
            x = (C.c_uint64 * n)(*[next(rng) for _ in range(n)])
            lib.lf_transcript_absorb_fq(t, x, n)
            for _ in range(1 + next(rng) % 3):
                nbytes = SQUEEZE_WORDS[next(rng) % len(SQUEEZE_WORDS)] * usable
                out = (C.c_uint8 * nbytes)()
                lib.lf_transcript_squeeze_bytes(t, out, nbytes)
                h.update(bytes(out))
    finally:
        lib.lf_transcript_free(t)
    return h.hexdigest()


def main():
    lib = load()
    doc = {"script": "tools/gen_transcript_digests.py", "sha256": {ring: digest(lib, ring) for ring in RINGS}}
    text = json.dumps(doc, indent=1) + "\n"
    if "--write" in sys.argv[1:]:
        with open(GOLDEN, "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
