"""Host-side mirror of the reference's interface for the prover hot path, over the C ABI of liblfhip.so.

Names follow crates/latticefold: `AjtaiCommitmentScheme` (commitment/commitment_scheme.rs:17-114),
`Witness` (arith.rs:213-362), `PoseidonTranscript` (transcript/poseidon.rs), `DecompositionParams`
(decomposition_parameters.rs:11-20), `NIFSProver.prove` (nifs.rs:48-103), `CCS` (arith.rs:50-74).
All bulk data are numpy uint64 arrays of canonical residues, shape (..., d) per ring element: d = 24 for
GoldilocksRingNTT (default), d = 72 for BabyBearRingNTT (`Context(device, ring="babybear")`, `PoseidonTranscript(ring=..)`).
Where an O(n) array crosses the ABI -- crt / icrt, the commitments, Witness.from_*, the `*_into` getters, check_relation -- a DEVICE array is
accepted next to numpy: any object with `data_ptr()` and a true `is_cuda` (a torch tensor), contiguous, 8-byte elements, same shape.  It goes to
the `_dev` entry point as it is, no copy; the context is first ordered behind the current torch stream (lf_ctx_wait_stream).

There is NO CPU fallback: if the HIP library is missing or no GPU is present every call raises.
"""
import ctypes as C
import os

import numpy as np

RE = 24
P = 2**64 - 2**32 + 1
RING_IDS = {"goldilocks": 0, "babybear": 1}   # LF_RING_* of include/lfhip.h
RING_WORDS = {"goldilocks": 24, "babybear": 72}
RING_TAU = {"goldilocks": 3, "babybear": 9}
FORMS = {"ntt": 0, "coeff": 1}                # LF_FORM_* of include/lfhip.h
_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "liblfhip.so")

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, u64p, u64p, C.c_size_t)   # lf_exchange_fn


class LfError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        msg = _lib().lf_strerror(code).decode() if _LIB is not None else str(code)
        super().__init__(f"liblfhip {where}: {msg} ({code})")


class CommitmentError(LfError):
    """CommitmentError::WrongWitnessLength (commitment.rs:14-27)"""


LF_ERR_REJECT = -8
# the components of a relation: the LF_REL_* bits of lf_cccs_check / lf_lcccs_check
REL_BITS = {"cm": 1, "ccs": 2, "u": 4, "v": 8, "norm": 16}


class NotSatisfied(LfError):
    """Error::NotSatisfied(row) of CCS::check_relation (arith.rs:76-110): `row` is the first row with a non-zero residual"""

    def __init__(self, row, where="lf_ccs_check"):
        super().__init__(LF_ERR_REJECT, where)
        self.row = row


class Params(C.Structure):
    """lf_params == DecompositionParams {B, L, B_SMALL=b, K} + CCS shape + kappa."""
    _fields_ = [("s", C.c_uint32), ("wit_len", C.c_uint32), ("l", C.c_uint32), ("L", C.c_uint32),
                ("K", C.c_uint32), ("b", C.c_uint32), ("B", C.c_uint64), ("kappa", C.c_uint32),
                ("t", C.c_uint32), ("q", C.c_uint32), ("d", C.c_uint32)]


class VPolyDesc(C.Structure):
    """lf_vpoly (include/lfhip_sumcheck.h)"""
    _fields_ = [("nvars", C.c_uint32), ("ntables", C.c_uint32), ("nterms", C.c_uint32), ("degree", C.c_uint32),
                ("term_off", u32p), ("term_idx", u32p), ("coef", u64p)]


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            raise RuntimeError(f"{_SO} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the HIP extension is required; there is no CPU fallback)")
        L = C.CDLL(_SO)
        vp = C.c_void_p
        L.lf_strerror.restype = C.c_char_p
        L.lf_strerror.argtypes = [C.c_int]
        L.lf_ctx_create.argtypes = [C.POINTER(vp), C.c_int]
        L.lf_ctx_create_ring.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
        L.lf_ctx_ring.argtypes = [vp]
        L.lf_ring_modulus.restype = C.c_uint64
        L.lf_ring_modulus.argtypes = [C.c_int]
        for f in ("lf_lcccs_len_ring", "lf_cccs_len_ring", "lf_proof_len_ring"):
            getattr(L, f).restype = C.c_size_t
            getattr(L, f).argtypes = [C.POINTER(Params), C.c_int]
        L.lf_transcript_new_ring.restype = vp
        L.lf_transcript_new_ring.argtypes = [C.c_int]
        L.lf_poseidon_params_ring.argtypes = [u64p, u64p, C.c_int]
        L.lf_poseidon_params_ring.restype = None
        L.lf_proof_wire_size.argtypes = [C.POINTER(Params), C.c_int]
        L.lf_proof_wire_size.restype = C.c_size_t
        L.lf_proof_serialize.argtypes = [C.POINTER(Params), C.c_int, u64p, C.c_void_p, C.c_size_t]
        L.lf_proof_deserialize.argtypes = [C.POINTER(Params), C.c_int, C.c_void_p, C.c_size_t, u64p]
        L.lf_poseidon_permute_ring.argtypes = [u64p, C.c_int, C.c_int]
        L.lf_poseidon_permute_ring.restype = None
        L.lf_ctx_destroy.argtypes = [vp]
        L.lf_ctx_destroy.restype = None
        L.lf_set_ring_tables.argtypes = [vp, C.c_uint64, u64p]
        L.lf_set_ext_basis.argtypes = [vp, u64p]
        L.lf_set_digit_mode.argtypes = [vp, C.c_int]
        L.lf_get_ring_tables.argtypes = [vp, u64p, u64p]
        L.lf_device_synchronize.argtypes = [vp]
        L.lf_mem_info.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.lf_selftest_field.argtypes = [vp, C.c_uint64, C.c_uint32, u64p]
        L.lf_ntt_fwd.argtypes = [vp, u64p, u64p, C.c_size_t]
        L.lf_ntt_inv.argtypes = [vp, u64p, u64p, C.c_size_t]
        L.lf_ring_mul.argtypes = [vp, u64p, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p]
        L.lf_decompose.argtypes = [vp, u64p, C.c_size_t, C.c_uint64, C.c_uint, C.c_int, u64p]
        L.lf_recompose.argtypes = [vp, u64p, C.c_size_t, C.c_uint64, C.c_uint, u64p]
        L.lf_linf_check.argtypes = [vp, u64p, C.c_size_t, C.c_uint64, C.c_int, C.POINTER(C.c_int), u64p]
        L.lf_ajtai_load.argtypes = [vp, u64p, C.c_size_t, C.c_size_t]
        L.lf_ajtai_generate.argtypes = [vp, C.c_uint64, C.c_size_t, C.c_size_t]
        L.lf_device_memory.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.lf_ajtai_commit.argtypes = [vp, u64p, C.c_size_t, C.c_size_t, u64p]
        L.lf_ajtai_commit_coeff.argtypes = [vp, u64p, C.c_size_t, C.c_size_t, u64p]
        L.lf_ajtai_decompose_and_commit_coeff.argtypes = [vp, u64p, C.c_size_t, C.c_uint64, C.c_uint, C.c_size_t, u64p]
        L.lf_ajtai_decompose_and_commit_ntt.argtypes = [vp, u64p, C.c_size_t, C.c_uint64, C.c_uint, C.c_size_t, u64p]
        L.lf_modsum.argtypes = [u64p, C.c_size_t, C.c_size_t, u64p]
        L.lf_modsum_ring.argtypes = [u64p, C.c_size_t, C.c_size_t, u64p, C.c_int]
        L.lf_set_sharding.argtypes = [vp, C.c_int, C.c_int, EXCHANGE_FN, vp]
        L.lf_set_sharding_lanes.argtypes = [vp, C.c_int, C.c_int, EXCHANGE_FN, vp, EXCHANGE_FN, vp]
        L.lf_dist_unique_id.argtypes = [C.c_void_p]
        L.lf_dist_init.argtypes = [vp, C.c_int, C.c_int, C.c_void_p]
        L.lf_dist_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
        L.lf_build_eq.argtypes = [vp, u64p, C.c_uint, u64p]
        L.lf_mle_eval_batch.argtypes = [vp, u64p, C.c_size_t, C.c_size_t, u64p, C.c_uint, u64p]
        L.lf_ccs_load.argtypes = [vp, C.POINTER(Params), C.POINTER(u32p), C.POINTER(u32p), C.POINTER(u64p), u32p, u32p, u64p]
        L.lf_spmv.argtypes = [vp, C.c_uint, u64p, u64p]
        for f in ("lf_lcccs_len", "lf_cccs_len", "lf_proof_len"):
            getattr(L, f).restype = C.c_size_t
            getattr(L, f).argtypes = [C.POINTER(Params)]
        L.lf_witness_from_w_ccs.argtypes = [vp, u64p, C.POINTER(vp)]
        L.lf_witness_from_f_coeff.argtypes = [vp, u64p, C.POINTER(vp)]
        L.lf_witness_from_f.argtypes = [vp, u64p, C.POINTER(vp)]
        L.lf_witness_get_f_coeff.argtypes = [vp, vp, u64p]
        L.lf_witness_get_f.argtypes = [vp, vp, u64p]
        L.lf_witness_get_w_ccs.argtypes = [vp, vp, u64p]
        L.lf_witness_commit.argtypes = [vp, vp, u64p]
        L.lf_witness_free.argtypes = [vp]
        L.lf_witness_free.restype = None
        L.lf_transcript_new.restype = vp
        L.lf_transcript_clone.restype = vp
        L.lf_transcript_clone.argtypes = [vp]
        L.lf_transcript_free.argtypes = [vp]
        L.lf_transcript_free.restype = None
        L.lf_transcript_absorb_fq.argtypes = [vp, u64p, C.c_size_t]
        L.lf_transcript_absorb_fq.restype = None
        L.lf_transcript_absorb_ring.argtypes = [vp, u64p, C.c_size_t]
        L.lf_transcript_absorb_ring.restype = None
        L.lf_transcript_get_challenge.argtypes = [vp, u64p]
        L.lf_transcript_get_challenge.restype = None
        L.lf_transcript_get_short_challenge.argtypes = [vp, u64p]
        L.lf_transcript_get_short_challenge.restype = None
        L.lf_poseidon_params.argtypes = [u64p, u64p]
        L.lf_poseidon_params.restype = None
        L.lf_poseidon_permute.argtypes = [u64p, C.c_int]
        L.lf_poseidon_permute.restype = None
        L.lf_sumcheck_lin_begin.argtypes = [vp, u64p, u64p]
        L.lf_sumcheck_lin_round.argtypes = [vp, u64p, u64p]
        L.lf_sumcheck_lin_end.argtypes = [vp]
        L.lf_linearize.argtypes = [vp, vp, u64p, vp, u64p, u64p]
        L.lf_fold_step.argtypes = [vp, vp, u64p, vp, u64p, vp, u64p, C.POINTER(vp), u64p]
        L.lf_device_sponge.argtypes = [vp, u32p, C.c_size_t, u64p, C.c_size_t, u64p, C.c_size_t, u64p]
        L.lf_sumcheck_fold_begin.argtypes = [vp, u64p, u64p]
        L.lf_sumcheck_fold_round.argtypes = [vp, u64p, u64p]
        L.lf_sumcheck_fold_end.argtypes = [vp]
        L.lf_lincomb.argtypes = [vp, u64p, u64p, C.c_size_t, C.c_size_t, u64p]
        L.lf_horner_combine.argtypes = [vp, u64p, C.c_size_t, C.c_size_t, C.c_size_t, u64p, u64p]
        L.lf_decomposition_prove.argtypes = [vp, vp, u64p, vp, u64p, u64p]
        L.lf_folding_prove.argtypes = [vp, vp, u64p, vp, vp, u64p, C.POINTER(vp), u64p]
        # decomposed witnesses: arrays of handles
        L.lf_witness_decompose.argtypes = [vp, vp, C.POINTER(vp)]
        L.lf_witness_recompose.argtypes = [vp, C.POINTER(vp), C.c_uint, C.POINTER(vp)]
        L.lf_decomposition_prove_parts.argtypes = [vp, vp, u64p, vp, u64p, u64p, C.POINTER(vp)]
        L.lf_folding_prove_parts.argtypes = [vp, vp, u64p, C.POINTER(vp), C.c_uint, u64p, C.POINTER(vp), u64p]
        L.lf_last_phase_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.lf_phase_name.restype = C.c_char_p
        L.lf_phase_name.argtypes = [C.c_int]
        L.lf_verify_host.argtypes = [C.c_int, C.POINTER(Params), u32p, u32p, u64p, vp, u64p, u64p, u64p, u64p, C.POINTER(C.c_int)]
        L.lf_last_fold_paths.argtypes = [vp, C.POINTER(C.c_uint)]
        L.lf_last_lin_split_rounds.argtypes = [vp, C.POINTER(C.c_uint)]
        L.lf_last_fold_split_rounds.argtypes = [vp, C.POINTER(C.c_uint)]
        L.lf_last_timeline.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.c_int]
        L.lf_last_kernel_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)]
        # device-resident callers: the device arrays are plain addresses
        L.lf_ctx_wait_stream.argtypes = [vp, vp]
        L.lf_ntt_fwd_dev.argtypes = [vp, vp, vp, C.c_size_t]
        L.lf_ntt_inv_dev.argtypes = [vp, vp, vp, C.c_size_t]
        L.lf_ring_mul_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp]
        L.lf_ajtai_commit_dev.argtypes = [vp, vp, C.c_size_t, C.c_size_t, u64p]
        L.lf_ajtai_commit_coeff_dev.argtypes = [vp, vp, C.c_size_t, C.c_size_t, u64p]
        L.lf_ajtai_decompose_and_commit_coeff_dev.argtypes = [vp, vp, C.c_size_t, C.c_uint64, C.c_uint, C.c_size_t, u64p]
        L.lf_ajtai_decompose_and_commit_ntt_dev.argtypes = [vp, vp, C.c_size_t, C.c_uint64, C.c_uint, C.c_size_t, u64p]
        for f in ("lf_witness_from_w_ccs_dev", "lf_witness_from_f_coeff_dev", "lf_witness_from_f_dev"):
            getattr(L, f).argtypes = [vp, vp, C.POINTER(vp)]
        for f in ("lf_witness_get_f_coeff_dev", "lf_witness_get_f_dev", "lf_witness_get_w_ccs_dev"):
            getattr(L, f).argtypes = [vp, vp, vp]
        L.lf_ccs_check_dev.argtypes = [vp, vp, u64p]
        L.lf_decompose_dev.argtypes = [vp, vp, C.c_size_t, C.c_uint64, C.c_uint, C.c_int, vp]
        L.lf_recompose_dev.argtypes = [vp, vp, C.c_size_t, C.c_uint64, C.c_uint, vp]
        L.lf_linf_check_dev.argtypes = [vp, vp, C.c_size_t, C.c_uint64, C.c_int, C.POINTER(C.c_int), u64p]
        L.lf_build_eq_dev.argtypes = [vp, u64p, C.c_uint, vp]
        L.lf_mle_eval_batch_dev.argtypes = [vp, vp, C.c_size_t, C.c_size_t, u64p, C.c_uint, u64p]
        L.lf_spmv_dev.argtypes = [vp, C.c_uint, vp, vp]
        L.lf_sumcheck_lin_begin_dev.argtypes = [vp, vp, u64p]
        L.lf_sumcheck_fold_begin_dev.argtypes = [vp, vp, u64p]
        L.lf_lincomb_dev.argtypes = [vp, u64p, vp, C.c_size_t, C.c_size_t, vp]
        L.lf_horner_combine_dev.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, u64p, vp]
        # the generic sumcheck (include/lfhip_sumcheck.h)
        vpp = C.POINTER(VPolyDesc)
        L.lf_mlsumcheck_begin.argtypes = [vp, vpp, u64p]
        L.lf_mlsumcheck_begin_device.argtypes = [vp, vpp, vp]
        L.lf_mlsumcheck_round.argtypes = [vp, u64p, u64p]
        L.lf_mlsumcheck_final.argtypes = [vp, u64p, u64p]
        L.lf_mlsumcheck_end.argtypes = [vp]
        L.lf_mlsumcheck_prove.argtypes = [vp, vp, vpp, u64p, u64p, u64p, u64p]
        L.lf_mlsumcheck_prove_device.argtypes = [vp, vp, vpp, vp, u64p, u64p, u64p]
        L.lf_mlsumcheck_verify.argtypes = [C.c_int, vp, C.c_uint32, C.c_uint32, u64p, u64p, u64p, u64p]
        # witness tables (include/lfhip_tables.h); the _device arrays are plain addresses
        hp = C.POINTER(vp)
        L.lf_witness_get_fhat.argtypes = [vp, hp, C.c_uint, u64p]
        L.lf_witness_get_fhat_device.argtypes = [vp, hp, C.c_uint, vp]
        L.lf_witness_get_z.argtypes = L.lf_witness_mz.argtypes = [vp, vp, u64p, u64p]
        L.lf_witness_get_z_device.argtypes = L.lf_witness_mz_device.argtypes = [vp, vp, u64p, vp]
        L.lf_spmv_t.argtypes = [vp, C.c_uint, u64p, u64p]
        L.lf_spmv_t_device.argtypes = [vp, C.c_uint, vp, vp]
        L.lf_mle_fix_variables.argtypes = [vp, u64p, C.c_size_t, C.c_size_t, u64p, C.c_uint, u64p]
        L.lf_mle_fix_variables_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, u64p, C.c_uint, vp]
        L.lfdbg_spmv_t_heavy_min.argtypes = [vp, C.c_uint]
        L.lfdbg_spmv_t_heavy_min.restype = C.c_uint
        # the chained prover object (include/lfhip_prover.h); the _dev arrays are plain addresses
        uip = C.POINTER(C.c_uint)
        L.lf_prover_create.argtypes = [vp, C.c_uint, C.POINTER(vp)]
        L.lf_prover_destroy.argtypes = [vp]
        L.lf_prover_destroy.restype = None
        L.lf_prover_last_error.argtypes = [vp]
        L.lf_prover_last_error.restype = C.c_char_p
        L.lf_prover_init.argtypes = [vp, vp, u64p, u64p, u64p, u64p]
        L.lf_prover_resume.argtypes = [vp, u64p, u64p]
        L.lf_prover_resume_dev.argtypes = [vp, u64p, vp]
        L.lf_prover_ingest.argtypes = [vp, u64p, u64p]
        L.lf_prover_ingest_dev.argtypes = [vp, vp, u64p]
        L.lf_prover_check_fresh.argtypes = [vp, C.c_uint64, uip, u64p]
        L.lf_prover_prove.argtypes = [vp, vp, u64p, u64p, u64p]
        L.lf_prover_accumulator.argtypes = [vp, u64p, u64p]
        L.lf_prover_accumulator_dev.argtypes = [vp, u64p, vp]
        L.lf_prover_decide.argtypes = [vp, C.c_uint64, uip]
        L.lf_prover_steps.argtypes = [vp]
        L.lf_prover_steps.restype = C.c_uint64
        _LIB = L
    return _LIB


def dist_unique_ids():
    """two ncclUniqueIds (256 bytes) for Context.dist_init: one RCCL communicator per lane of the fold step"""
    out = b""
    for _ in range(2):
        buf = (C.c_uint8 * 128)()
        _chk(_lib().lf_dist_unique_id(buf), "lf_dist_unique_id")
        out += bytes(buf)
    return out


def abi_version():
    """LFHIP_ABI_VERSION the library was built with (include/lfhip.h)"""
    L = _lib()
    L.lf_abi_version.restype = C.c_int
    return int(L.lf_abi_version())


def exported_symbols(header="lfhip.h"):
    """Every symbol include/lfhip.h declares (used by the CPU-side ABI test); header="lfhip_parts.h" / "lfhip_sumcheck.h" / "lfhip_prover.h": the ones of a
    file it includes ("lfhip_tables.h": the witness tables)."""
    import re
    hdr = open(os.path.join(_HERE, "..", "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(lf_[a-z0-9_]+)\s*\(", hdr)))


def _a64(x):
    a = np.ascontiguousarray(x, dtype=np.uint64)
    return a, a.ctypes.data_as(u64p)


def _chk(rc, where):
    if rc != 0:
        raise LfError(rc, where)


def is_device_array(x):
    """a device-resident array argument: anything with data_ptr() and a true is_cuda (a torch tensor)"""
    return hasattr(x, "data_ptr") and bool(getattr(x, "is_cuda", False))


def _dev(ctx, t, words=None):
    """device array -> its address for a _dev entry point, after ordering the context behind the stream the array was produced on (the current torch stream).
    words: the last dimension (default: a ring element; an eq table has TAU)"""
    words = ctx.RE if words is None else words
    if not t.is_contiguous() or t.element_size() != 8 or t.dim() < 2 or t.shape[-1] != words:
        raise ValueError(f"device arrays must be contiguous, 8-byte elements, shape (..., {words})")
    ctx.wait_stream()
    return C.c_void_p(t.data_ptr())


def _dev_out(like, shape, out):
    """where a _dev call writes: `out`, which must be a device array of that shape, or a fresh tensor next to `like`"""
    if out is None:
        import torch
        return torch.empty(shape, dtype=like.dtype, device=like.device)
    if not is_device_array(out) or tuple(out.shape) != tuple(shape):
        raise ValueError(f"out must be a device array of shape {tuple(shape)}")
    return out


class Context:
    """Owns the device memory (lf_ctx).  One per GPU / process."""

    def __init__(self, device=0, ring="goldilocks"):
        self.h = C.c_void_p()
        self.device = device
        self.ring = ring
        self.ring_id = RING_IDS[ring]
        self.RE = RING_WORDS[ring]
        self.TAU = RING_TAU[ring]
        _chk(_lib().lf_ctx_create_ring(C.byref(self.h), device, self.ring_id), "lf_ctx_create_ring")
        self.params = None

    def close(self):
        if getattr(self, "h", None):
            _lib().lf_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- ring tables -------------------------------------------------------------------
    def set_ring_tables(self, nonres, y):
        a, p = _a64(y)
        _chk(_lib().lf_set_ring_tables(self.h, nonres, p), "lf_set_ring_tables")

    def get_ring_tables(self):
        nr = C.c_uint64()
        y = np.zeros(8 * self.TAU, dtype=np.uint64)
        _chk(_lib().lf_get_ring_tables(self.h, C.cast(C.byref(nr), u64p), y.ctypes.data_as(u64p)), "lf_get_ring_tables")
        return nr.value, y

    def selftest_field(self, seed=1, n=1 << 20):
        m = C.c_uint64(1)
        _chk(_lib().lf_selftest_field(self.h, seed, n, C.cast(C.byref(m), u64p)), "lf_selftest_field")
        return m.value

    def set_digit_mode(self, mode):
        """lf_set_digit_mode: 0 = sign-magnitude truncation (default), 1 = floor rule (digits in [-base/2, base/2))"""
        _chk(_lib().lf_set_digit_mode(self.h, int(mode)), "lf_set_digit_mode")

    def set_ext_basis(self, T):
        """lf_set_ext_basis: T (tau x tau) maps the internal binomial-basis coordinates of F_{p^tau} to the caller's external ones"""
        a, p = _a64(np.ascontiguousarray(T, dtype=np.uint64).reshape(-1))
        assert a.size == self.TAU * self.TAU
        _chk(_lib().lf_set_ext_basis(self.h, p), "lf_set_ext_basis")

    def set_sharding(self, rank, world, allgather, allgather_lane1=None):
        """Intra-step sharding over a HOST transport (lf_set_sharding_lanes); call before creating the AjtaiCommitmentScheme.
        allgather(np.uint64[words]) -> np.uint64[world, words] in rank order (see latticefold_amd.dist.make_allgather).  The two lanes
        of a fold step exchange concurrently from two threads: pass a second callable with its own ordered channel (its own process
        group) as allgather_lane1."""
        def mk(fn):
            def _cb(user, send, recv, words):
                try:
                    mine = np.ctypeslib.as_array(send, shape=(words,)).copy()
                    out = np.ascontiguousarray(fn(mine), dtype=np.uint64).reshape(world * words)
                    C.memmove(recv, out.ctypes.data, world * words * 8)
                    return 0
                except Exception as e:  # never let an exception cross the C boundary
                    import sys
                    print("lf exchange callback failed:", repr(e), file=sys.stderr)
                    return -1
            return EXCHANGE_FN(_cb)
        self._exchange_cb = mk(allgather) if world > 1 else EXCHANGE_FN(0)
        self._exchange_cb1 = mk(allgather_lane1) if (world > 1 and allgather_lane1 is not None) else EXCHANGE_FN(0)
        _chk(_lib().lf_set_sharding_lanes(self.h, rank, world, self._exchange_cb, None, self._exchange_cb1, None), "lf_set_sharding_lanes")
        self.shard = (rank, world)

    def dist_init(self, rank, world, ids):
        """Intra-step sharding over RCCL (lf_dist_init): ids = bytes of TWO ncclUniqueIds (api.dist_unique_ids() on rank 0, broadcast by
        the launcher).  Exchanges then run on device buffers in the library's own streams (ncclAllGather + modular-sum kernel)."""
        ids = bytes(ids)
        assert len(ids) == 256
        buf = (C.c_uint8 * 256).from_buffer_copy(ids)
        _chk(_lib().lf_dist_init(self.h, rank, world, buf), "lf_dist_init")
        self.shard = (rank, world)

    def dist_two_lanes(self, set=-1):
        """lf_dist_two_lanes: 1 when sharded steps run the threaded two-lane schedule (the outcome of lf_dist_init's self-check); set = 0 / 1 overrides it --
        every rank must use the same value"""
        L = _lib()
        L.lf_dist_two_lanes.argtypes = [C.c_void_p, C.c_int]
        rc = L.lf_dist_two_lanes(self.h, int(set))
        if rc < 0:
            raise LfError(rc, "lf_dist_two_lanes")
        return rc

    def dist_stats(self, reset=False):
        """(number of exchanges, total us, max us) of the context's exchange log"""
        n, tot, mx = C.c_uint64(), C.c_double(), C.c_double()
        _chk(_lib().lf_dist_stats(self.h, C.byref(n), C.byref(tot), C.byref(mx), int(reset)), "lf_dist_stats")
        return n.value, tot.value, mx.value

    def set_sharding_model(self, rank, world):
        """lf_set_sharding_model: a TIMING model of rank `rank` of `world` with no peers (zeros stand in for their words).  What such a context returns is not
        a proof; tools/shard_model.py measures a rank's share of a sharded step with it on a one-GPU box."""
        L = _lib()
        L.lf_set_sharding_model.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _chk(L.lf_set_sharding_model(self.h, int(rank), int(world)), "lf_set_sharding_model")
        self.shard = (rank, world)

    def dist_stats_words(self, reset=False):
        """u64 words this rank contributed to its exchanges (lf_dist_stats_words)"""
        L = _lib()
        L.lf_dist_stats_words.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        w = C.c_uint64()
        _chk(L.lf_dist_stats_words(self.h, C.byref(w), int(reset)), "lf_dist_stats_words")
        return w.value

    def mem_info(self):
        f, t = C.c_size_t(), C.c_size_t()
        _chk(_lib().lf_mem_info(self.h, C.byref(f), C.byref(t)), "lf_mem_info")
        return f.value, t.value

    def synchronize(self):
        _chk(_lib().lf_device_synchronize(self.h), "lf_device_synchronize")

    def wait_stream(self, stream=None):
        """lf_ctx_wait_stream: the context's streams wait for what is enqueued so far on `stream` (a hipStream_t address; default: the current torch
        stream of the context's device); the host does not wait"""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        _chk(_lib().lf_ctx_wait_stream(self.h, C.c_void_p(stream)), "lf_ctx_wait_stream")

    # ---- element-wise ops ----------------------------------------------------------------
    def _ntt_dev(self, fn, name, x, out):
        import torch
        o = torch.empty_like(x) if out is None else out
        if o.shape != x.shape:
            raise ValueError("out must have the shape of the input")
        px, po = _dev(self, x), (_dev(self, o) if o is not x else None)
        _chk(fn(self.h, px, po or px, x.numel() // self.RE), name)
        return o

    def crt(self, coeff, out=None):  # CRT::elementwise_crt
        """numpy in, numpy out; a device array in, a device array out (`out`: where to, may be the input itself)"""
        if is_device_array(coeff):
            return self._ntt_dev(_lib().lf_ntt_fwd_dev, "lf_ntt_fwd_dev", coeff, out)
        a, p = _a64(coeff)
        o = np.empty_like(a)
        _chk(_lib().lf_ntt_fwd(self.h, p, o.ctypes.data_as(u64p), a.size // self.RE), "lf_ntt_fwd")
        return o

    def icrt(self, ntt, out=None):  # ICRT::elementwise_icrt
        if is_device_array(ntt):
            return self._ntt_dev(_lib().lf_ntt_inv_dev, "lf_ntt_inv_dev", ntt, out)
        a, p = _a64(ntt)
        o = np.empty_like(a)
        _chk(_lib().lf_ntt_inv(self.h, p, o.ctypes.data_as(u64p), a.size // self.RE), "lf_ntt_inv")
        return o

    ntt_fwd, ntt_inv = crt, icrt

    def ring_mul(self, a, b, form="ntt", out=None):
        """lf_ring_mul: out[x] = sum_i a_i[x] * b_i[x] in the context's ring.  a, b: (count, RE) or (n_terms, count, RE), both in `form` ("ntt": slot-wise
        products, in the external basis if one is set; "coeff": products mod the cyclotomic polynomial, transforms fused); the result has that form too.
        numpy in, numpy out; device arrays in, a device array out (`out`: where to; with one term it may be `a` or `b` itself)"""
        fid = FORMS[form]
        if is_device_array(a) != is_device_array(b) or tuple(a.shape) != tuple(b.shape) or len(a.shape) not in (2, 3) or a.shape[-1] != self.RE:
            raise ValueError(f"a and b: two numpy arrays or two device arrays of one shape, (count, {self.RE}) or (n_terms, count, {self.RE})")
        nt, cnt = (1, a.shape[0]) if len(a.shape) == 2 else (a.shape[0], a.shape[1])
        if is_device_array(a):
            o = _dev_out(a, (cnt, self.RE), out)
            _chk(_lib().lf_ring_mul_device(self.h, _dev(self, a), _dev(self, b), nt, cnt, fid, _dev(self, o)), "lf_ring_mul_device")
            return o
        (x, px), (y, py) = _a64(a), _a64(b)
        o = np.empty((cnt, self.RE), dtype=np.uint64)
        _chk(_lib().lf_ring_mul(self.h, px, py, nt, cnt, fid, o.ctypes.data_as(u64p)), "lf_ring_mul")
        return o

    def decompose(self, coeff, base, digits, layout, out=None):
        """numpy in, numpy out; a device array in, a device array out (`out`: where to; it may not overlap the input)"""
        if is_device_array(coeff):
            cnt = coeff.numel() // self.RE
            o = _dev_out(coeff, (cnt * digits, self.RE), out)
            _chk(_lib().lf_decompose_dev(self.h, _dev(self, coeff), cnt, base, digits, layout, _dev(self, o)), "lf_decompose_dev")
            return o
        a, p = _a64(coeff)
        cnt = a.size // self.RE
        o = np.zeros((cnt * digits, self.RE), dtype=np.uint64)
        _chk(_lib().lf_decompose(self.h, p, cnt, base, digits, layout, o.ctypes.data_as(u64p)), "lf_decompose")
        return o

    def recompose(self, x, base, digits, out=None):
        if is_device_array(x):
            cnt = x.numel() // self.RE // digits
            o = _dev_out(x, (cnt, self.RE), out)
            _chk(_lib().lf_recompose_dev(self.h, _dev(self, x), cnt, base, digits, _dev(self, o)), "lf_recompose_dev")
            return o
        a, p = _a64(x)
        cnt = a.size // self.RE // digits
        o = np.zeros((cnt, self.RE), dtype=np.uint64)
        _chk(_lib().lf_recompose(self.h, p, cnt, base, digits, o.ctypes.data_as(u64p)), "lf_recompose")
        return o

    def linf_check(self, f_ntt, bound, unsigned_variant=False):
        ok = C.c_int()
        mx = C.c_uint64()
        if is_device_array(f_ntt):
            _chk(_lib().lf_linf_check_dev(self.h, _dev(self, f_ntt), f_ntt.numel() // self.RE, bound, int(unsigned_variant), C.byref(ok),
                                          C.cast(C.byref(mx), u64p)), "lf_linf_check_dev")
            return bool(ok.value), mx.value
        a, p = _a64(f_ntt)
        _chk(_lib().lf_linf_check(self.h, p, a.size // self.RE, bound, int(unsigned_variant), C.byref(ok), C.cast(C.byref(mx), u64p)), "lf_linf_check")
        return bool(ok.value), mx.value

    def build_eq(self, point, out=None):
        """the eq table of `point` (host), (1 << nv, TAU): a numpy array, or written into the device array `out` (lf_build_eq_dev)"""
        a, p = _a64(point)
        nv = a.size // self.TAU
        if out is not None:
            o = _dev_out(None, (1 << nv, self.TAU), out)
            _chk(_lib().lf_build_eq_dev(self.h, p, nv, _dev(self, o, self.TAU)), "lf_build_eq_dev")
            return o
        o = np.zeros(((1 << nv), self.TAU), dtype=np.uint64)
        _chk(_lib().lf_build_eq(self.h, p, nv, o.ctypes.data_as(u64p)), "lf_build_eq")
        return o

    def evaluate_mles(self, tables, point):  # utils/mle_helpers.rs:65-88
        """tables (ntables, len, RE), numpy or a device array; the evaluations come back as numpy either way"""
        b, q = _a64(point)
        if is_device_array(tables):
            nt, ln = tables.shape[0], tables.shape[1]
            o = np.zeros((nt, self.RE), dtype=np.uint64)
            _chk(_lib().lf_mle_eval_batch_dev(self.h, _dev(self, tables), nt, ln, q, b.size // self.TAU, o.ctypes.data_as(u64p)), "lf_mle_eval_batch_dev")
            return o
        a, p = _a64(tables)
        nt, ln = a.shape[0], a.shape[1]
        o = np.zeros((nt, self.RE), dtype=np.uint64)
        _chk(_lib().lf_mle_eval_batch(self.h, p, nt, ln, q, b.size // self.TAU, o.ctypes.data_as(u64p)), "lf_mle_eval_batch")
        return o

    mle_eval_batch = evaluate_mles

    # ---- CCS -------------------------------------------------------------------------------
    def load_ccs(self, wl):
        """wl: latticefold_amd.workload.Workload (params + CSR matrices)."""
        self.params = Params(wl.s, wl.wit_len, wl.l, wl.L, wl.K, wl.b, wl.B, wl.kappa, wl.t, wl.q, wl.d)
        t = wl.t
        rp = [np.ascontiguousarray(a, dtype=np.uint32) for a in wl.rowptr]
        ci = [np.ascontiguousarray(a, dtype=np.uint32) for a in wl.col]
        va = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in wl.val]
        so = np.ascontiguousarray(wl.S_off, dtype=np.uint32)
        si = np.ascontiguousarray(wl.S_idx, dtype=np.uint32)
        cc = np.ascontiguousarray(wl.c, dtype=np.uint64).reshape(-1)
        rpp = (u32p * t)(*[a.ctypes.data_as(u32p) for a in rp])
        cip = (u32p * t)(*[a.ctypes.data_as(u32p) for a in ci])
        vap = (u64p * t)(*[a.ctypes.data_as(u64p) for a in va])
        _chk(_lib().lf_ccs_load(self.h, C.byref(self.params), C.cast(rpp, C.POINTER(u32p)), C.cast(cip, C.POINTER(u32p)),
                                C.cast(vap, C.POINTER(u64p)), so.ctypes.data_as(u32p), si.ctypes.data_as(u32p),
                                cc.ctypes.data_as(u64p)), "lf_ccs_load")
        self.lcccs_len = _lib().lf_lcccs_len_ring(C.byref(self.params), self.ring_id)
        self.cccs_len = _lib().lf_cccs_len_ring(C.byref(self.params), self.ring_id)
        self.proof_len = _lib().lf_proof_len_ring(C.byref(self.params), self.ring_id)
        self.N = wl.N
        self.m = wl.m
        self.n = wl.n

    def mat_vec_mul(self, j, z, out=None):  # arith/utils.rs:52-65
        if is_device_array(z):
            o = _dev_out(z, (self.m, self.RE), out)
            _chk(_lib().lf_spmv_dev(self.h, j, _dev(self, z), _dev(self, o)), "lf_spmv_dev")
            return o
        a, p = _a64(z)
        o = np.zeros((self.m, self.RE), dtype=np.uint64)
        _chk(_lib().lf_spmv(self.h, j, p, o.ctypes.data_as(u64p)), "lf_spmv")
        return o

    def mat_vec_mul_t(self, j, v, out=None, device=None):
        """lf_spmv_t: M_j^T v for v of m general ring elements (NTT form), (n, RE).  v a device array: lf_spmv_t_device, the result a device array (`out` or a
        fresh one); device=True with a numpy v uploads it first"""
        if device and not is_device_array(v):
            import torch
            v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint64).view(np.int64)).to(torch.device("cuda", self.device))
        if is_device_array(v):
            o = _dev_out(v, (self.n, self.RE), out)
            _chk(_lib().lf_spmv_t_device(self.h, j, _dev(self, v), _dev(self, o)), "lf_spmv_t_device")
            return o
        a, p = _a64(v)
        o = np.zeros((self.n, self.RE), dtype=np.uint64)
        _chk(_lib().lf_spmv_t(self.h, j, p, o.ctypes.data_as(u64p)), "lf_spmv_t")
        return o

    def spmv_t_heavy_min(self, next=0):
        """(tests, measurements; not part of the ABI) the heavy-column threshold of lf_spmv_t in force for the loaded system; next != 0: the one the next
        load_ccs builds its work lists with"""
        return int(_lib().lfdbg_spmv_t_heavy_min(self.h, next))

    # ---- relation checks (arith.rs:76-110, 193-206) ------------------------------------------------------------
    def check_relation(self, z):
        """CCS::check_relation (arith.rs:76-110) of the loaded CCS on z (n NTT-form elements): None, or raises NotSatisfied with .row = the first bad row"""
        L = _lib()
        L.lf_ccs_check.argtypes = [C.c_void_p, u64p, u64p]
        fb = C.c_uint64()
        if is_device_array(z):
            rc, name = L.lf_ccs_check_dev(self.h, _dev(self, z), C.cast(C.byref(fb), u64p)), "lf_ccs_check_dev"
        else:
            a, p = _a64(z)
            rc, name = L.lf_ccs_check(self.h, p, C.cast(C.byref(fb), u64p)), "lf_ccs_check"
        if rc == LF_ERR_REJECT:
            raise NotSatisfied(fb.value, name)
        _chk(rc, name)

    def check_cccs(self, cccs, wit, bound=0):
        """R_CCCS of (cccs, wit): the set of failing components among "cm", "ccs", "norm" (norm: max |centred coefficient| < bound, checked when
        bound != 0); empty when the relation holds.  The first bad row of the CCS (m when it holds) is left in .last_first_bad"""
        L = _lib()
        L.lf_cccs_check.argtypes = [C.c_void_p, u64p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint), u64p]
        a, p = _a64(cccs)
        f, fb = C.c_uint(), C.c_uint64()
        rc = L.lf_cccs_check(self.h, p, wit.h, int(bound), C.byref(f), C.cast(C.byref(fb), u64p))
        if rc != LF_ERR_REJECT:
            _chk(rc, "lf_cccs_check")
        self.last_first_bad = fb.value
        return {name for name, bit in REL_BITS.items() if f.value & bit}

    def check_lcccs(self, lcccs, wit, bound=0):
        """R_LCCCS of (lcccs, wit), the decider of an accumulator: the set of failing components among "cm", "u", "v", "norm"; empty when it holds"""
        L = _lib()
        L.lf_lcccs_check.argtypes = [C.c_void_p, u64p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint)]
        a, p = _a64(lcccs)
        f = C.c_uint()
        rc = L.lf_lcccs_check(self.h, p, wit.h, int(bound), C.byref(f))
        if rc != LF_ERR_REJECT:
            _chk(rc, "lf_lcccs_check")
        return {name for name, bit in REL_BITS.items() if f.value & bit}

    def phase_ms(self):
        out = (C.c_float * 8)()
        _chk(_lib().lf_last_phase_ms(self.h, out), "lf_last_phase_ms")
        return {_lib().lf_phase_name(i).decode(): float(out[i]) for i in range(8)}

    def fold_paths(self):
        m = C.c_uint()
        _chk(_lib().lf_last_fold_paths(self.h, C.byref(m)), "lf_last_fold_paths")
        return m.value

    def lin_split_rounds(self):
        """rounds of the last linearization sumcheck that ran in the split eq form -- test hook"""
        m = C.c_uint()
        _chk(_lib().lf_last_lin_split_rounds(self.h, C.byref(m)), "lf_last_lin_split_rounds")
        return m.value

    def live_rows(self):
        """1 + the last row with an entry in any matrix of the loaded CCS (the rows behind it are skipped) -- test hook, not part of the ABI"""
        f = _lib().lfdbg_live_rows
        f.argtypes, f.restype = [C.c_void_p], C.c_longlong
        return f(self.h)

    def lin_live_rounds(self):
        """rounds of the last linearization sumcheck that ran over a live prefix of their tables only -- test hook, not part of the ABI"""
        f = _lib().lfdbg_last_lin_live_rounds
        f.argtypes, f.restype = [C.c_void_p], C.c_int
        return f(self.h)

    def fold_split_rounds(self):
        """mask (bit i-1 = round i) of the table rounds of the last folding sumcheck that ran in the split eq form -- test hook"""
        m = C.c_uint()
        _chk(_lib().lf_last_fold_split_rounds(self.h, C.byref(m)), "lf_last_fold_split_rounds")
        return m.value

    def timeline(self):
        """[(mark, ms since the start of the step)] of the last fold step (wall clock of the calling thread)"""
        names, ms = C.create_string_buffer(32 * 64), (C.c_double * 64)()
        n = _lib().lf_last_timeline(self.h, names, ms, 64)
        if n < 0:
            raise LfError(n, "lf_last_timeline")
        return [(names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode(), float(ms[i])) for i in range(n)]

    def device_memory(self):
        """(free, total) bytes of the device (lf_device_memory)"""
        f, t = C.c_size_t(), C.c_size_t()
        _chk(_lib().lf_device_memory(self.h, C.byref(f), C.byref(t)), "lf_device_memory")
        return f.value, t.value

    def kernel_stats(self):
        f, a = C.c_float(), C.c_float()
        fn, an = C.c_int(), C.c_int()
        _chk(_lib().lf_last_kernel_stats(self.h, C.byref(f), C.byref(fn), C.byref(a), C.byref(an)), "lf_last_kernel_stats")
        return {"fold_round_ms": f.value, "fold_round_launches": fn.value, "ajtai_ms": a.value, "ajtai_launches": an.value}


class AjtaiCommitmentScheme:
    """commitment/commitment_scheme.rs:17-114.  The matrix lives on the device."""

    def __init__(self, ctx, matrix=None, kappa=None, n=None, seed=None):
        self.ctx = ctx
        if matrix is not None:  # AjtaiCommitmentScheme::new
            a, p = _a64(matrix)
            self._kappa, self._n = a.shape[0], a.shape[1]
            _chk(_lib().lf_ajtai_load(ctx.h, p, self._kappa, self._n), "lf_ajtai_load")
        else:                    # synthetic i.i.d. matrix generated on the device (bench)
            self._kappa, self._n = kappa, n
            _chk(_lib().lf_ajtai_generate(ctx.h, seed, kappa, n), "lf_ajtai_generate")

    def kappa(self):
        return self._kappa

    def width(self):
        return self._n

    def commit_ntt(self, f):
        """commit / commit_ntt: f is (n,d) or (batch,n,d), numpy or a device array; the commitment is numpy either way."""
        dev = is_device_array(f)
        a, p = (f, _dev(self.ctx, f)) if dev else _a64(f)
        batch = 1 if a.ndim == 2 else a.shape[0]
        n = a.shape[-2]
        o = np.zeros((batch, self._kappa, self.ctx.RE), dtype=np.uint64)
        rc = (_lib().lf_ajtai_commit_dev if dev else _lib().lf_ajtai_commit)(self.ctx.h, p, n, batch, o.ctypes.data_as(u64p))
        if rc == -1 and (not dev or n != self._n):   # (a device array may also be refused for what it is: LfError)
            raise CommitmentError(rc, f"WrongWitnessLength({n}, {self._n})")
        _chk(rc, "lf_ajtai_commit_dev" if dev else "lf_ajtai_commit")
        return o[0] if a.ndim == 2 else o

    commit = commit_ntt

    def _commit_with(self, fn, name, f, *args, digits=1):
        if is_device_array(f):
            fn, name = getattr(_lib(), name + "_dev"), name + "_dev"
            a, p = f, _dev(self.ctx, f)
        else:
            a, p = _a64(f)
        batch = 1 if a.ndim == 2 else a.shape[0]
        n = a.shape[-2]
        o = np.zeros((batch, self._kappa, self.ctx.RE), dtype=np.uint64)
        rc = fn(self.ctx.h, p, n, *args, batch, o.ctypes.data_as(u64p))
        if rc == -1 and n * digits != self._n:
            raise CommitmentError(rc, f"WrongWitnessLength({n * digits}, {self._n})")
        _chk(rc, name)
        return o[0] if a.ndim == 2 else o

    def commit_coeff(self, f_coeff):
        """commit_coeff (commitment_scheme.rs:81-87): commit_ntt of CRT(f_coeff); f_coeff (n,d) or (batch,n,d) in coefficient form"""
        return self._commit_with(_lib().lf_ajtai_commit_coeff, "lf_ajtai_commit_coeff", f_coeff)

    def decompose_and_commit_coeff(self, f_coeff, B, L):
        """decompose_and_commit_coeff (commitment_scheme.rs:90-101): the commitment of the count*L vector decompose_to_vec(B, L) (element i -> columns
        [i*L, (i+1)*L)), without building it; f_coeff (count,d) or (batch,count,d) in coefficient form"""
        return self._commit_with(_lib().lf_ajtai_decompose_and_commit_coeff, "lf_ajtai_decompose_and_commit_coeff", f_coeff, int(B), int(L), digits=int(L))

    def decompose_and_commit_ntt(self, w, B, L):
        """decompose_and_commit_ntt (commitment_scheme.rs:106-113): the same from NTT-form w"""
        return self._commit_with(_lib().lf_ajtai_decompose_and_commit_ntt, "lf_ajtai_decompose_and_commit_ntt", w, int(B), int(L), digits=int(L))


class PendingWitness:
    """a witness being ingested on the context's lowest-priority stream (lf_witness_from_w_ccs_begin / lf_witness_job_finish); keeps the host words alive until
    the job has finished"""

    def __init__(self, ctx, w_ccs):
        self.ctx = ctx
        self._keep, p = _a64(w_ccs)
        self._job = C.c_void_p()
        L = _lib()
        L.lf_witness_from_w_ccs_begin.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.lf_witness_job_finish.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        _chk(L.lf_witness_from_w_ccs_begin(ctx.h, p, C.byref(self._job)), "lf_witness_from_w_ccs_begin")

    def result(self):
        if not self._job:
            raise RuntimeError("the job was finished already")
        h = C.c_void_p()
        job, self._job = self._job, None
        rc = _lib().lf_witness_job_finish(job, C.byref(h))
        self._keep = None
        _chk(rc, "lf_witness_job_finish")
        return Witness(self.ctx, h)

    def abandon(self):
        if self._job:
            job, self._job = self._job, None
            _lib().lf_witness_job_finish(job, None)
            self._keep = None

    def __del__(self):
        try:
            self.abandon()
        except Exception:
            pass


class Witness:
    """arith.rs:213-362; device-resident (centred f_coeff planes)."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @classmethod
    def from_w_ccs(cls, ctx, w_ccs):
        h = C.c_void_p()
        if is_device_array(w_ccs):
            _chk(_lib().lf_witness_from_w_ccs_dev(ctx.h, _dev(ctx, w_ccs), C.byref(h)), "lf_witness_from_w_ccs_dev")
            return cls(ctx, h)
        a, p = _a64(w_ccs)
        _chk(_lib().lf_witness_from_w_ccs(ctx.h, p, C.byref(h)), "lf_witness_from_w_ccs")
        return cls(ctx, h)

    @classmethod
    def from_w_ccs_begin(cls, ctx, w_ccs):
        """lf_witness_from_w_ccs_begin: start building the witness next to whatever the context runs (a fold step); `.result()` waits and returns the Witness"""
        return PendingWitness(ctx, w_ccs)

    @classmethod
    def from_f_coeff(cls, ctx, f_coeff):
        h = C.c_void_p()
        if is_device_array(f_coeff):
            _chk(_lib().lf_witness_from_f_coeff_dev(ctx.h, _dev(ctx, f_coeff), C.byref(h)), "lf_witness_from_f_coeff_dev")
            return cls(ctx, h)
        a, p = _a64(f_coeff)
        _chk(_lib().lf_witness_from_f_coeff(ctx.h, p, C.byref(h)), "lf_witness_from_f_coeff")
        return cls(ctx, h)

    @classmethod
    def from_f(cls, ctx, f_ntt):
        h = C.c_void_p()
        if is_device_array(f_ntt):
            _chk(_lib().lf_witness_from_f_dev(ctx.h, _dev(ctx, f_ntt), C.byref(h)), "lf_witness_from_f_dev")
            return cls(ctx, h)
        a, p = _a64(f_ntt)
        _chk(_lib().lf_witness_from_f(ctx.h, p, C.byref(h)), "lf_witness_from_f")
        return cls(ctx, h)

    def _get(self, fn, count):
        o = np.zeros((count, self.ctx.RE), dtype=np.uint64)
        _chk(fn(self.ctx.h, self.h, o.ctypes.data_as(u64p)), "lf_witness_get")
        return o

    @property
    def f_coeff(self):
        return self._get(_lib().lf_witness_get_f_coeff, self.ctx.N)

    @property
    def f(self):
        return self._get(_lib().lf_witness_get_f, self.ctx.N)

    @property
    def w_ccs(self):
        return self._get(_lib().lf_witness_get_w_ccs, self.ctx.params.wit_len)

    def _get_into(self, fn, name, count, out):
        if not is_device_array(out) or tuple(out.shape) != (count, self.ctx.RE):
            raise ValueError(f"out must be a device array of shape ({count}, {self.ctx.RE})")
        _chk(fn(self.ctx.h, self.h, _dev(self.ctx, out)), name)
        return out

    def f_coeff_into(self, out):
        """f_coeff written into a device array (N, d)"""
        return self._get_into(_lib().lf_witness_get_f_coeff_dev, "lf_witness_get_f_coeff_dev", self.ctx.N, out)

    def f_into(self, out):
        return self._get_into(_lib().lf_witness_get_f_dev, "lf_witness_get_f_dev", self.ctx.N, out)

    def w_ccs_into(self, out):
        return self._get_into(_lib().lf_witness_get_w_ccs_dev, "lf_witness_get_w_ccs_dev", self.ctx.params.wit_len, out)

    def get_fhat(self, device=None):
        """Witness::get_fhat (arith.rs:273-297): the tau f-hat tables, (tau, m, RE); device: a device array to write into, or True for a fresh one"""
        return get_fhat(self.ctx, [self], device=device)

    def _xz(self, x, host_fn, dev_fn, name, shape, device):
        a, p = _a64(x)
        if a.size != self.ctx.params.l * self.ctx.RE:
            raise ValueError("x must hold l ring elements")
        if device is not None and device is not False:
            o = _new_dev(self.ctx, shape) if device is True else _dev_out(None, shape, device)
            _chk(dev_fn(self.ctx.h, self.h, p, _dev(self.ctx, o)), name + "_device")
            return o
        o = np.zeros(shape, dtype=np.uint64)
        _chk(host_fn(self.ctx.h, self.h, p, o.ctypes.data_as(u64p)), name)
        return o

    def get_z(self, x, device=None):
        """z = x || 1 || w_ccs (arith.rs:399-409), (n, RE); x: (l, RE) on the host"""
        L = _lib()
        return self._xz(x, L.lf_witness_get_z, L.lf_witness_get_z_device, "lf_witness_get_z", (self.ctx.n, self.ctx.RE), device)

    def mz(self, x, device=None):
        """calculate_Mz_mles (utils/mle_helpers.rs:137-146): the t tables M_j z, (t, m, RE)"""
        L = _lib()
        return self._xz(x, L.lf_witness_mz, L.lf_witness_mz_device, "lf_witness_mz", (self.ctx.params.t, self.ctx.m, self.ctx.RE), device)

    def commit(self, scheme):
        o = np.zeros((scheme.kappa(), self.ctx.RE), dtype=np.uint64)
        _chk(_lib().lf_witness_commit(self.ctx.h, self.h, o.ctypes.data_as(u64p)), "lf_witness_commit")
        return o

    def decompose(self, ctx):
        """decompose_witness (nifs/decomposition.rs:162-167): the K base-b parts of this witness under the context's digit rule, each a Witness of its own"""
        hs = (C.c_void_p * max(ctx.params.K if ctx.params else 0, 1))()
        _chk(_lib().lf_witness_decompose(ctx.h, self.h, hs), "lf_witness_decompose")
        return [Witness(ctx, C.c_void_p(h)) for h in hs[:ctx.params.K]]

    @classmethod
    def recompose(cls, ctx, parts):
        """the witness whose base-b parts are `parts` (K of them); LfError unless they are exactly the decomposition of their sum"""
        h = C.c_void_p()
        _chk(_lib().lf_witness_recompose(ctx.h, _handles(parts), len(parts), C.byref(h)), "lf_witness_recompose")
        return cls(ctx, h)

    def free(self):
        if self.h:
            _lib().lf_witness_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _handles(wits):
    """witnesses -> the array of handles an entry point with a `const lf_witness *const *` argument takes"""
    return (C.c_void_p * max(len(wits), 1))(*[w.h.value if isinstance(w.h, C.c_void_p) else w.h for w in wits])


def _new_dev(ctx, shape):
    """a fresh device array of canonical words on the context's device"""
    import torch
    return torch.empty(shape, dtype=torch.int64, device=torch.device("cuda", ctx.device))


def get_fhat(ctx, wits, device=None):
    """lf_witness_get_fhat for a batch: (len(wits) * tau, m, RE), table w * tau + j = f-hat_j of wits[w] -- the order MLSumcheckFold takes them from slot 5
    on.  device: a device array to write into (e.g. a view of the fold sumcheck's table array), or True for a fresh one: lf_witness_get_fhat_device"""
    shape = (len(wits) * ctx.TAU, ctx.m, ctx.RE)
    if device is not None and device is not False:
        o = _new_dev(ctx, shape) if device is True else _dev_out(None, shape, device)
        _chk(_lib().lf_witness_get_fhat_device(ctx.h, _handles(wits), len(wits), _dev(ctx, o)), "lf_witness_get_fhat_device")
        return o
    o = np.zeros(shape, dtype=np.uint64)
    _chk(_lib().lf_witness_get_fhat(ctx.h, _handles(wits), len(wits), o.ctypes.data_as(u64p)), "lf_witness_get_fhat")
    return o


def mle_fix_variables(ctx, tables, point, out=None):
    """DenseMultilinearExtension::fix_variables on tables (ntables, len, RE): the lowest nfix = len(point) / tau variables fixed at `point` (host) ->
    (ntables, len >> nfix, RE).  tables a device array: lf_mle_fix_variables_device, the result a device array (`out` or a fresh one)"""
    b, q = _a64(point)
    nfix = b.size // ctx.TAU
    nt, ln = int(tables.shape[0]), int(tables.shape[1])
    shape = (nt, ln >> nfix, ctx.RE)
    if is_device_array(tables):
        o = _dev_out(tables, shape, out)
        _chk(_lib().lf_mle_fix_variables_device(ctx.h, _dev(ctx, tables), nt, ln, q, nfix, _dev(ctx, o)), "lf_mle_fix_variables_device")
        return o
    a, p = _a64(tables)
    o = np.zeros(shape, dtype=np.uint64)
    _chk(_lib().lf_mle_fix_variables(ctx.h, p, nt, ln, q, nfix, o.ctypes.data_as(u64p)), "lf_mle_fix_variables")
    return o


class PoseidonTranscript:
    """transcript/poseidon.rs:17-75 (host)."""

    def __init__(self, handle=None, ring="goldilocks"):
        self.ring = ring
        self.RE, self.TAU = RING_WORDS[ring], RING_TAU[ring]
        self.h = handle or C.c_void_p(_lib().lf_transcript_new_ring(RING_IDS[ring]))

    def clone(self):
        return PoseidonTranscript(C.c_void_p(_lib().lf_transcript_clone(self.h)), ring=self.ring)

    def absorb_fq(self, xs):
        a, p = _a64(xs)
        _lib().lf_transcript_absorb_fq(self.h, p, a.size)

    def absorb_slice(self, elems):
        a, p = _a64(elems)
        _lib().lf_transcript_absorb_ring(self.h, p, a.size // self.RE)

    absorb = absorb_slice

    def get_challenge(self):
        o = np.zeros(self.TAU, dtype=np.uint64)
        _lib().lf_transcript_get_challenge(self.h, o.ctypes.data_as(u64p))
        return o

    def get_short_challenge(self):
        o = np.zeros(self.RE, dtype=np.uint64)
        _lib().lf_transcript_get_short_challenge(self.h, o.ctypes.data_as(u64p))
        return o

    def __del__(self):
        try:
            if self.h:
                _lib().lf_transcript_free(self.h)
                self.h = None
        except Exception:
            pass


def poseidon_params(ring="goldilocks"):
    ark = np.zeros(720, dtype=np.uint64)
    mds = np.zeros(576, dtype=np.uint64)
    _lib().lf_poseidon_params_ring(ark.ctypes.data_as(u64p), mds.ctypes.data_as(u64p), RING_IDS[ring])
    return ark, mds


def poseidon_permute(state, plain=False, ring="goldilocks"):
    a = np.ascontiguousarray(state, dtype=np.uint64).copy()
    _lib().lf_poseidon_permute_ring(a.ctypes.data_as(u64p), int(plain), RING_IDS[ring])
    return a


class LFLinearizationProver:
    @staticmethod
    def prove(ctx, cm_i, wit, transcript):
        """nifs/linearization.rs:145-189 -> (lcccs flat, linearization proof flat)."""
        a, p = _a64(cm_i)
        lc = np.zeros((ctx.lcccs_len, ctx.RE), dtype=np.uint64)
        prm = ctx.params
        pr = np.zeros((prm.s * (prm.d + 2) + ctx.TAU + prm.t, ctx.RE), dtype=np.uint64)
        _chk(_lib().lf_linearize(ctx.h, transcript.h, p, wit.h, lc.ctypes.data_as(u64p), pr.ctypes.data_as(u64p)), "lf_linearize")
        return lc, pr


class LFDecompositionProver:
    @staticmethod
    def prove(ctx, lcccs, wit, transcript):
        """nifs/decomposition.rs:33-88 -> (K decomposed LCCCS flat [K*lcccs_len], decomposition proof flat).  The K decomposed
        witnesses are the base-b parts of `wit` and stay virtual on the device."""
        a, p = _a64(lcccs)
        prm = ctx.params
        lcs = np.zeros((prm.K * ctx.lcccs_len, ctx.RE), dtype=np.uint64)
        pr = np.zeros((prm.K * (prm.t + ctx.TAU + prm.l + 1 + prm.kappa), ctx.RE), dtype=np.uint64)
        _chk(_lib().lf_decomposition_prove(ctx.h, transcript.h, p, wit.h, lcs.ctypes.data_as(u64p), pr.ctypes.data_as(u64p)),
             "lf_decomposition_prove")
        return lcs, pr

    @staticmethod
    def prove_parts(ctx, lcccs, wit, transcript):
        """LFDecompositionProver::prove with its wit_s -> (K decomposed LCCCS flat, decomposition proof flat, the K decomposed witnesses)"""
        a, p = _a64(lcccs)
        prm = ctx.params
        lcs = np.zeros((prm.K * ctx.lcccs_len, ctx.RE), dtype=np.uint64)
        pr = np.zeros((prm.K * (prm.t + ctx.TAU + prm.l + 1 + prm.kappa), ctx.RE), dtype=np.uint64)
        hs = (C.c_void_p * prm.K)()
        _chk(_lib().lf_decomposition_prove_parts(ctx.h, transcript.h, p, wit.h, lcs.ctypes.data_as(u64p), pr.ctypes.data_as(u64p), hs),
             "lf_decomposition_prove_parts")
        return lcs, pr, [Witness(ctx, C.c_void_p(h)) for h in hs]


class LFFoldingProver:
    @staticmethod
    def prove(ctx, lcccs_s, w_left, w_right, transcript):
        """nifs/folding.rs:42-130: lcccs_s = the 2K decomposed LCCCS, w_left / w_right the witnesses they are parts of
        -> (folded LCCCS flat, folded Witness, folding proof flat)."""
        a, p = _a64(lcccs_s)
        prm = ctx.params
        lc = np.zeros((ctx.lcccs_len, ctx.RE), dtype=np.uint64)
        pr = np.zeros((prm.s * (2 * prm.b + 1) + 2 * prm.K * (ctx.TAU + prm.t), ctx.RE), dtype=np.uint64)
        h = C.c_void_p()
        _chk(_lib().lf_folding_prove(ctx.h, transcript.h, p, w_left.h, w_right.h, lc.ctypes.data_as(u64p), C.byref(h),
                                     pr.ctypes.data_as(u64p)), "lf_folding_prove")
        return lc, Witness(ctx, h), pr

    @staticmethod
    def prove_parts(ctx, lcccs_s, w_s, transcript):
        """LFFoldingProver::prove with the reference's w_s: the 2K decomposed witnesses (K of the accumulator, then K of the fresh instance), which must be
        the decompositions of their sums -> (folded LCCCS flat, folded Witness, folding proof flat), those of `prove` on the two sums."""
        a, p = _a64(lcccs_s)
        prm = ctx.params
        lc = np.zeros((ctx.lcccs_len, ctx.RE), dtype=np.uint64)
        pr = np.zeros((prm.s * (2 * prm.b + 1) + 2 * prm.K * (ctx.TAU + prm.t), ctx.RE), dtype=np.uint64)
        h = C.c_void_p()
        _chk(_lib().lf_folding_prove_parts(ctx.h, transcript.h, p, _handles(w_s), len(w_s), lc.ctypes.data_as(u64p), C.byref(h),
                                           pr.ctypes.data_as(u64p)), "lf_folding_prove_parts")
        return lc, Witness(ctx, h), pr


class NIFSProver:
    @staticmethod
    def prove(ctx, acc, w_acc, cm_i, w_i, transcript):
        """nifs.rs:48-103 -> (folded LCCCS flat, folded Witness, LFProof flat).  `ccs` and `scheme` of the
        reference signature are the ones loaded into ctx (load_ccs / AjtaiCommitmentScheme)."""
        a, pa = _a64(acc)
        b, pb = _a64(cm_i)
        lc = np.zeros((ctx.lcccs_len, ctx.RE), dtype=np.uint64)
        pr = np.zeros((ctx.proof_len, ctx.RE), dtype=np.uint64)
        h = C.c_void_p()
        _chk(_lib().lf_fold_step(ctx.h, transcript.h, pa, w_acc.h, pb, w_i.h, lc.ctypes.data_as(u64p), C.byref(h),
                                 pr.ctypes.data_as(u64p)), "lf_fold_step")
        return lc, Witness(ctx, h), pr


class ChainProverError(LfError):
    """an lf_prover_* call failed: .code is the LF_ERR_* code, .detail the text of lf_prover_last_error"""

    def __init__(self, code, where, detail=""):
        super().__init__(code, where)
        self.detail = detail
        if detail:
            self.args = (f"{self.args[0]} -- {detail}",)


class NIFSChainProver:
    """The chained NIFS prover object (lf_prover_*, include/lfhip_prover.h): NIFSProver::prove made a chain that owns its accumulator on the device.
    create -> init | resume -> (ingest -> [check_fresh] -> prove)* ; accumulator / decide / steps at any point with an accumulator; close.
    w_ccs, f_ntt: numpy, or a device array (a torch tensor) for the `_dev` entry points.  The context is borrowed: close the prover before it."""
    COMMIT_INLINE = 1   # LF_PROVER_COMMIT_INLINE

    def __init__(self, ctx, flags=0):
        self.ctx = ctx
        self.h = C.c_void_p()
        self._keep = None
        self.last_first_bad = None
        rc = _lib().lf_prover_create(ctx.h, int(flags), C.byref(self.h))
        if rc != 0:
            self.h = None
            raise ChainProverError(rc, "lf_prover_create")

    create = classmethod(lambda cls, ctx, flags=0: cls(ctx, flags))

    def last_error(self):
        return _lib().lf_prover_last_error(self.h).decode()

    def _chk(self, rc, where, ok=()):
        if rc != 0 and rc not in ok:
            raise ChainProverError(rc, where, self.last_error())
        return rc

    def init(self, transcript, w_ccs, x_ccs):
        """first accumulator = the linearization of (x_ccs, w_ccs) on `transcript` -> (LCCCS flat, linearization proof flat)"""
        ctx, prm = self.ctx, self.ctx.params
        (a, pw), (b, px) = _a64(w_ccs), _a64(x_ccs)
        assert a.size == prm.wit_len * ctx.RE and b.size == prm.l * ctx.RE
        lc = np.zeros((ctx.lcccs_len, ctx.RE), dtype=np.uint64)
        pr = np.zeros((prm.s * (prm.d + 2) + ctx.TAU + prm.t, ctx.RE), dtype=np.uint64)
        self._chk(_lib().lf_prover_init(self.h, transcript.h, pw, px, lc.ctypes.data_as(u64p), pr.ctypes.data_as(u64p)), "lf_prover_init")
        return lc, pr

    def resume(self, lcccs, f_ntt):
        """take up a chain again from (LCCCS, folded witness f in NTT form: numpy or a device array)"""
        a, pl = _a64(lcccs)
        assert a.size == self.ctx.lcccs_len * self.ctx.RE
        if is_device_array(f_ntt):
            assert f_ntt.numel() == self.ctx.N * self.ctx.RE
            self._chk(_lib().lf_prover_resume_dev(self.h, pl, _dev(self.ctx, f_ntt)), "lf_prover_resume_dev")
            return
        f, pf = _a64(f_ntt)
        assert f.size == self.ctx.N * self.ctx.RE
        self._chk(_lib().lf_prover_resume(self.h, pl, pf), "lf_prover_resume")

    def ingest(self, w_ccs, x_ccs):
        """names the fresh instance of the next prove and returns at once (a device w_ccs: blocking).  The host words are kept alive until that prove"""
        b, px = _a64(x_ccs)
        assert b.size == self.ctx.params.l * self.ctx.RE
        if is_device_array(w_ccs):
            assert w_ccs.numel() == self.ctx.params.wit_len * self.ctx.RE
            self._chk(_lib().lf_prover_ingest_dev(self.h, _dev(self.ctx, w_ccs), px), "lf_prover_ingest_dev")
            return
        a, pw = _a64(w_ccs)
        assert a.size == self.ctx.params.wit_len * self.ctx.RE
        keep, self._keep = self._keep, a     # (a refused ingest drops the instance that was pending: its words may go once the call is back)
        try:
            self._chk(_lib().lf_prover_ingest(self.h, pw, px), "lf_prover_ingest")
        except ChainProverError:
            self._keep = None
            raise
        finally:
            del keep

    def check_fresh(self, bound=0):
        """R_CCCS of the pending instance: the set of failing components among "ccs", "norm" (the commitment is the prover's own); the first bad row of the CCS
        (m when it holds) is left in .last_first_bad"""
        f, fb = C.c_uint(), C.c_uint64()
        rc = _lib().lf_prover_check_fresh(self.h, int(bound), C.byref(f), C.cast(C.byref(fb), u64p))
        if rc not in (0, LF_ERR_REJECT):
            self._keep = None
        self._chk(rc, "lf_prover_check_fresh", ok=(LF_ERR_REJECT,))
        self.last_first_bad = fb.value
        return {name for name, bit in REL_BITS.items() if f.value & bit}

    def prove(self, transcript):
        """NIFSProver::prove of (accumulator, pending instance) -> (fresh CCCS cm || x_ccs, folded LCCCS flat, LFProof flat); the folded pair is the accumulator"""
        ctx = self.ctx
        cc = np.zeros((ctx.cccs_len, ctx.RE), dtype=np.uint64)
        lc = np.zeros((ctx.lcccs_len, ctx.RE), dtype=np.uint64)
        pr = np.zeros((ctx.proof_len, ctx.RE), dtype=np.uint64)
        rc = _lib().lf_prover_prove(self.h, transcript.h, cc.ctypes.data_as(u64p), lc.ctypes.data_as(u64p), pr.ctypes.data_as(u64p))
        self._keep = None
        self._chk(rc, "lf_prover_prove")
        return cc, lc, pr

    def accumulator(self, out=None):
        """(LCCCS flat, f in NTT form); out: a device array (N, d) to write f into (lf_prover_accumulator_dev)"""
        ctx = self.ctx
        lc = np.zeros((ctx.lcccs_len, ctx.RE), dtype=np.uint64)
        if out is not None:
            if not is_device_array(out) or tuple(out.shape) != (ctx.N, ctx.RE):
                raise ValueError(f"out must be a device array of shape ({ctx.N}, {ctx.RE})")
            self._chk(_lib().lf_prover_accumulator_dev(self.h, lc.ctypes.data_as(u64p), _dev(ctx, out)), "lf_prover_accumulator_dev")
            return lc, out
        f = np.zeros((ctx.N, ctx.RE), dtype=np.uint64)
        self._chk(_lib().lf_prover_accumulator(self.h, lc.ctypes.data_as(u64p), f.ctypes.data_as(u64p)), "lf_prover_accumulator")
        return lc, f

    def decide(self, bound=0):
        """R_LCCCS of the accumulator: the set of failing components among "cm", "u", "v", "norm"; empty when it holds"""
        f = C.c_uint()
        self._chk(_lib().lf_prover_decide(self.h, int(bound), C.byref(f)), "lf_prover_decide", ok=(LF_ERR_REJECT,))
        return {name for name, bit in REL_BITS.items() if f.value & bit}

    def steps(self):
        return int(_lib().lf_prover_steps(self.h))

    def close(self):
        if getattr(self, "h", None):
            _lib().lf_prover_destroy(self.h)
            self.h = None
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NIFSVerifier:
    @staticmethod
    def verify(wl, acc, cm_i, proof, transcript):
        """nifs.rs:117-163 on the host (no GPU): wl gives the CCS shape (params, S, c).  Returns (ok, folded LCCCS flat,
        failed_stage)."""
        ring = wl.ring
        rid, RE_ = RING_IDS[ring], RING_WORDS[ring]
        prm = Params(wl.s, wl.wit_len, wl.l, wl.L, wl.K, wl.b, wl.B, wl.kappa, wl.t, wl.q, wl.d)
        so = np.ascontiguousarray(wl.S_off, dtype=np.uint32)
        si = np.ascontiguousarray(wl.S_idx, dtype=np.uint32)
        cc, pc = _a64(np.ascontiguousarray(wl.c).reshape(-1))
        a, pa = _a64(acc)
        b, pb = _a64(cm_i)
        pr, pp = _a64(proof)
        lc = np.zeros((_lib().lf_lcccs_len_ring(C.byref(prm), rid), RE_), dtype=np.uint64)
        st = C.c_int(0)
        rc = _lib().lf_verify_host(rid, C.byref(prm), so.ctypes.data_as(u32p), si.ctypes.data_as(u32p), pc, transcript.h, pa, pb, pp,
                                   lc.ctypes.data_as(u64p), C.byref(st))
        if rc not in (0, -8):
            raise LfError(rc, "lf_verify_host")
        return rc == 0, lc, st.value


def _wl_params(wl):
    return Params(wl.s, wl.wit_len, wl.l, wl.L, wl.K, wl.b, wl.B, wl.kappa, wl.t, wl.q, wl.d)


def proof_to_bytes(wl, proof):
    """LFProof::serialize_with_mode(Compress::Yes) (nifs.rs:28-34) of a flat proof; layout notes in include/lfhip.h."""
    prm, rid = _wl_params(wl), RING_IDS[wl.ring]
    a, p = _a64(proof)
    n = _lib().lf_proof_wire_size(C.byref(prm), rid)
    if a.size != _lib().lf_proof_len_ring(C.byref(prm), rid) * RING_WORDS[wl.ring]:
        raise LfError(-1, "proof_to_bytes: wrong proof length")
    buf = (C.c_uint8 * n)()
    _chk(_lib().lf_proof_serialize(C.byref(prm), rid, p, buf, n), "lf_proof_serialize")
    return bytes(buf)


def proof_from_bytes(wl, data):
    """LFProof::deserialize_with_mode(Compress::Yes, Validate::Yes) -> flat proof (ring elements x words)."""
    prm, rid = _wl_params(wl), RING_IDS[wl.ring]
    out = np.zeros((_lib().lf_proof_len_ring(C.byref(prm), rid), RING_WORDS[wl.ring]), dtype=np.uint64)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data) if len(data) else (C.c_uint8 * 1)()
    _chk(_lib().lf_proof_deserialize(C.byref(prm), rid, buf, len(data), out.ctypes.data_as(u64p)), "lf_proof_deserialize")
    return out


class MLSumcheckLin:
    """utils/sumcheck.rs:53-80 split at the transcript, for the linearization-shaped polynomial (lf_sumcheck_lin_*)."""

    def __init__(self, ctx, tables, eq_point):
        self.ctx = ctx
        b, q = _a64(eq_point)
        if is_device_array(tables):   # (t, m, RE) on the device: read in place
            _chk(_lib().lf_sumcheck_lin_begin_dev(ctx.h, _dev(ctx, tables), q), "lf_sumcheck_lin_begin_dev")
            return
        a, p = _a64(tables)
        _chk(_lib().lf_sumcheck_lin_begin(ctx.h, p, q), "lf_sumcheck_lin_begin")

    def prove_round(self, r_prev=None):
        prm = self.ctx.params
        o = np.zeros((prm.d + 2, self.ctx.RE), dtype=np.uint64)
        if r_prev is None:
            rc = _lib().lf_sumcheck_lin_round(self.ctx.h, None, o.ctypes.data_as(u64p))
        else:
            a, p = _a64(r_prev)
            rc = _lib().lf_sumcheck_lin_round(self.ctx.h, p, o.ctypes.data_as(u64p))
        _chk(rc, "lf_sumcheck_lin_round")
        return o

    def end(self):
        _chk(_lib().lf_sumcheck_lin_end(self.ctx.h), "lf_sumcheck_lin_end")


class VPoly:
    """VirtualPolynomial (utils/sumcheck/utils.rs:24-75) over a flat list of MLE tables: g = sum_i coef_i * prod_{j in indices_i} T_j.
    terms: [(coef, [indices])], coef a ring element in NTT form (RE words) or a Python integer (the constant, the same in every slot); an index may repeat
    inside a term and across terms.  degree: what the prover sends degree + 1 evaluations for (default: the widest term)."""

    def __init__(self, terms, degree=None):
        self.terms = [(c, [int(j) for j in idx]) for c, idx in terms]
        self.degree = max((len(idx) for _, idx in self.terms), default=0) if degree is None else int(degree)

    def desc(self, ring, nvars, ntables):
        """the lf_vpoly of this polynomial on `ring` (the arrays it points to stay alive with the returned object)"""
        RE_, tau, p = RING_WORDS[ring], RING_TAU[ring], int(_lib().lf_ring_modulus(RING_IDS[ring]))
        off = np.zeros(len(self.terms) + 1, dtype=np.uint32)
        coef = np.zeros((max(len(self.terms), 1), RE_), dtype=np.uint64)
        idx = []
        for i, (c, ix) in enumerate(self.terms):
            idx += ix
            off[i + 1] = len(idx)
            if isinstance(c, (int, np.integer)):
                coef[i, ::tau] = int(c) % p
            else:
                coef[i] = np.asarray(c, dtype=np.uint64).reshape(RE_)
        idx = np.asarray(idx + [0], dtype=np.uint32)
        d = VPolyDesc(nvars, ntables, len(self.terms), self.degree, off.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), coef.ctypes.data_as(u64p))
        d._keep = (off, idx, coef)
        return d


class MLSumcheck:
    """MLSumcheck::prove_as_subprotocol / verify_as_subprotocol (utils/sumcheck.rs:53-104) over any VPoly (lf_mlsumcheck_*, include/lfhip_sumcheck.h), on a
    bare context.  tables: (T, 2^nvars, RE) ring elements in NTT form, a numpy array or a device array (read in place).  The object is the split form:
    prove_round / final / end with the caller's transcript in between; prove is the whole subprotocol in one call."""

    @staticmethod
    def _shape(ctx, tables):
        sh = tuple(tables.shape)
        if len(sh) != 3 or sh[2] != ctx.RE or sh[1] < 2 or sh[1] & (sh[1] - 1):
            raise ValueError(f"tables: (T, 2^nvars, {ctx.RE})")
        return sh[0], sh[1].bit_length() - 1

    def __init__(self, ctx, tables, vpoly):
        self.ctx = ctx
        self.ntables, self.nvars = self._shape(ctx, tables)
        self.degree = vpoly.degree
        d = vpoly.desc(ctx.ring, self.nvars, self.ntables)
        if is_device_array(tables):
            _chk(_lib().lf_mlsumcheck_begin_device(ctx.h, C.byref(d), _dev(ctx, tables)), "lf_mlsumcheck_begin_device")
            return
        a, p = _a64(tables)
        _chk(_lib().lf_mlsumcheck_begin(ctx.h, C.byref(d), p), "lf_mlsumcheck_begin")

    def prove_round(self, r_prev=None):
        o = np.zeros((self.degree + 1, self.ctx.RE), dtype=np.uint64)
        if r_prev is None:
            rc = _lib().lf_mlsumcheck_round(self.ctx.h, None, o.ctypes.data_as(u64p))
        else:
            a, p = _a64(r_prev)
            rc = _lib().lf_mlsumcheck_round(self.ctx.h, p, o.ctypes.data_as(u64p))
        _chk(rc, "lf_mlsumcheck_round")
        return o

    def final(self, r_last):
        """after the last round: every table's value at the whole point, (T, RE)"""
        o = np.zeros((self.ntables, self.ctx.RE), dtype=np.uint64)
        a, p = _a64(r_last)
        _chk(_lib().lf_mlsumcheck_final(self.ctx.h, p, o.ctypes.data_as(u64p)), "lf_mlsumcheck_final")
        return o

    def end(self):
        _chk(_lib().lf_mlsumcheck_end(self.ctx.h), "lf_mlsumcheck_end")

    @staticmethod
    def prove(ctx, transcript, tables, vpoly):
        """prove_as_subprotocol -> (msgs (nvars, degree + 1, RE), point (nvars, TAU), final (T, RE): the tables' values at the point)"""
        T, nv = MLSumcheck._shape(ctx, tables)
        d = vpoly.desc(ctx.ring, nv, T)
        msgs = np.zeros((nv, vpoly.degree + 1, ctx.RE), dtype=np.uint64)
        point = np.zeros((nv, ctx.TAU), dtype=np.uint64)
        fin = np.zeros((T, ctx.RE), dtype=np.uint64)
        outs = (msgs.ctypes.data_as(u64p), point.ctypes.data_as(u64p), fin.ctypes.data_as(u64p))
        if is_device_array(tables):
            _chk(_lib().lf_mlsumcheck_prove_device(ctx.h, transcript.h, C.byref(d), _dev(ctx, tables), *outs), "lf_mlsumcheck_prove_device")
        else:
            a, p = _a64(tables)
            _chk(_lib().lf_mlsumcheck_prove(ctx.h, transcript.h, C.byref(d), p, *outs), "lf_mlsumcheck_prove")
        return msgs, point, fin

    @staticmethod
    def verify(transcript, nvars, degree, claimed_sum, msgs, ring="goldilocks"):
        """verify_as_subprotocol on the host (no GPU, no context) -> (ok, point (nvars, TAU), expected): expected is the subclaim's ring element, or the index of
        the failing round when ok is False"""
        RE_, tau = RING_WORDS[ring], RING_TAU[ring]
        cs, pc = _a64(claimed_sum)
        m, pm = _a64(msgs)
        if cs.size != RE_ or m.size != nvars * (degree + 1) * RE_:
            raise ValueError("claimed_sum: one ring element; msgs: nvars x (degree + 1) ring elements")
        point = np.zeros((nvars, tau), dtype=np.uint64)
        exp = np.zeros(RE_, dtype=np.uint64)
        rc = _lib().lf_mlsumcheck_verify(RING_IDS[ring], transcript.h, nvars, degree, pc, pm, point.ctypes.data_as(u64p), exp.ctypes.data_as(u64p))
        if rc not in (0, LF_ERR_REJECT):
            raise LfError(rc, "lf_mlsumcheck_verify")
        return rc == 0, point, (exp if rc == 0 else int(exp[0]))

    @staticmethod
    def extract_sum(msgs):
        """MLSumcheck::extract_sum (utils/sumcheck.rs:46-48): the claimed sum a proof is about, p_1(0) + p_1(1)"""
        m = np.asarray(msgs, dtype=np.uint64)
        ring = {v: k for k, v in RING_WORDS.items()}[m.shape[-1]]
        p = int(_lib().lf_ring_modulus(RING_IDS[ring]))
        m = m.reshape(-1, m.shape[-1])
        return ((m[0].astype(object) + m[1].astype(object)) % p).astype(np.uint64)


class MLSumcheckFold:
    """utils/sumcheck.rs:53-80 split at the transcript, for the folding polynomial (nifs/folding/utils.rs:200-325):
    tables = [eq_L, G_L, eq_R, G_R, eq_beta, f-hat ...] ((5 + 2K*tau) x m ring elements), mu = 2K challenges (lf_sumcheck_fold_*)."""

    def __init__(self, ctx, tables, mu):
        self.ctx = ctx
        b, q = _a64(mu)
        if is_device_array(tables):
            _chk(_lib().lf_sumcheck_fold_begin_dev(ctx.h, _dev(ctx, tables), q), "lf_sumcheck_fold_begin_dev")
            return
        a, p = _a64(tables)
        _chk(_lib().lf_sumcheck_fold_begin(ctx.h, p, q), "lf_sumcheck_fold_begin")

    def prove_round(self, r_prev=None):
        prm = self.ctx.params
        o = np.zeros((2 * prm.b + 1, self.ctx.RE), dtype=np.uint64)
        if r_prev is None:
            rc = _lib().lf_sumcheck_fold_round(self.ctx.h, None, o.ctypes.data_as(u64p))
        else:
            a, p = _a64(r_prev)
            rc = _lib().lf_sumcheck_fold_round(self.ctx.h, p, o.ctypes.data_as(u64p))
        _chk(rc, "lf_sumcheck_fold_round")
        return o

    def end(self):
        _chk(_lib().lf_sumcheck_fold_end(self.ctx.h), "lf_sumcheck_fold_end")


def lincomb(ctx, coef, tables, out=None):
    """compute_f_0 (nifs/folding.rs:258-268): sum_i coef_i (.) tables_i; coef (n, RE), tables (n, len, RE).  Device tables: a device result (`out`: where to)"""
    a, p = _a64(coef)
    if is_device_array(tables):
        n, ln = tables.shape[0], tables.shape[1]
        o = _dev_out(tables, (ln, ctx.RE), out)
        _chk(_lib().lf_lincomb_dev(ctx.h, p, _dev(ctx, tables), n, ln, _dev(ctx, o)), "lf_lincomb_dev")
        return o
    t = np.ascontiguousarray(tables, dtype=np.uint64)
    n, ln = t.shape[0], t.shape[1]
    o = np.zeros((ln, ctx.RE), dtype=np.uint64)
    _chk(_lib().lf_lincomb(ctx.h, p, t.ctypes.data_as(u64p), n, ln, o.ctypes.data_as(u64p)), "lf_lincomb")
    return o


def horner_combine(ctx, tables, challenges, out=None):
    """calculate_challenged_mz_mle (nifs/folding.rs:208-226): tables (groups, per_group, len, RE), challenges (groups, TAU).  Device tables: a device result"""
    a, p = _a64(challenges)
    if is_device_array(tables):
        g, pg, ln = tables.shape[0], tables.shape[1], tables.shape[2]
        o = _dev_out(tables, (ln, ctx.RE), out)
        _chk(_lib().lf_horner_combine_dev(ctx.h, _dev(ctx, tables), g, pg, ln, p, _dev(ctx, o)), "lf_horner_combine_dev")
        return o
    t = np.ascontiguousarray(tables, dtype=np.uint64)
    g, pg, ln = t.shape[0], t.shape[1], t.shape[2]
    o = np.zeros((ln, ctx.RE), dtype=np.uint64)
    _chk(_lib().lf_horner_combine(ctx.h, t.ctypes.data_as(u64p), g, pg, ln, p, o.ctypes.data_as(u64p)), "lf_horner_combine")
    return o


def device_sponge(ctx, ops):
    """PoseidonSponge on the device (lf_device_sponge): ops = list of ("absorb", words) / ("squeeze", n) on a fresh sponge.
    Returns (list of squeezed arrays, state[26])."""
    codes, words, nout = [], [], 0
    for kind, arg in ops:
        if kind == "absorb":
            a = np.ascontiguousarray(arg, dtype=np.uint64).reshape(-1)
            codes.append(a.size)
            words.append(a)
        else:
            codes.append((1 << 24) | int(arg))
            nout += int(arg)
    cw = np.array(codes, dtype=np.uint32)
    w = np.concatenate(words) if words else np.zeros(0, dtype=np.uint64)
    out = np.zeros(max(nout, 1), dtype=np.uint64)
    st = np.zeros(26, dtype=np.uint64)
    _chk(_lib().lf_device_sponge(ctx.h, cw.ctypes.data_as(u32p), cw.size, w.ctypes.data_as(u64p), w.size, out.ctypes.data_as(u64p), nout,
                                 st.ctypes.data_as(u64p)), "lf_device_sponge")
    res, o = [], 0
    for kind, arg in ops:
        if kind != "absorb":
            res.append(out[o:o + int(arg)].copy())
            o += int(arg)
    return res, st
