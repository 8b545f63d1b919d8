"""LatticeFold+ slice: Python mirror of the reference interface over the C ABI include/lfplus.h (ctypes, liblfhip.so).

Reference (crates/latticefold-plus): `RgInstance::from_f(f, &A, &DecompParameters{b, k, l})` (src/rgchk.rs:260-331), the double
commitment benchmarked by benches/double_commitment.rs; `utils::tensor` / `tensor_product` (src/utils.rs:45-83).  Ring: FrogRing
RqPoly, Z_p[X]/(X^16 + 1) in coefficient form, 16 canonical u64 words per element.  GPU only: there is no CPU path."""
import ctypes as C
import math
import re
import os
from dataclasses import dataclass

import numpy as np

from . import api

P = 15912092521325583641
D = 16
u64p = C.POINTER(C.c_uint64)
i8p = C.POINTER(C.c_int8)
_READY = False


class LfPlusError(RuntimeError):
    def __init__(self, code, msg):
        self.code = code
        super().__init__(f"liblfhip (lfplus): {msg} ({code})")


E_ARG, E_NO_DEVICE, E_HIP, E_EXP_DOMAIN, E_SMALL_N, E_REJECT = -1, -2, -3, -4, -5, -6
REL_CM, REL_R1CS, REL_V, REL_NORM = 1, 2, 4, 8      # lfplus.h LFPLUS_REL_*: the components of a relation check (lfplus_r1cs_check / lfplus_linb_check)
REL_CCS = 2                                         # the row-wise residual of lfplus_ccs_check: the bit of REL_R1CS
ABSENT = -128     # exponent digit of a zero entry of a monomial set (lfplus.h LFPLUS_ABSENT)
MUL_ELEMENTWISE, MUL_BROADCAST = 0, 1      # lfplus.h LFPLUS_MUL_*: the modes of lfplus_ring_mul
DIGITS_GADGET, DIGITS_PLANES = 0, 1        # lfplus.h LFPLUS_DIGITS_*: the layouts of lfplus_balanced_decompose / lfplus_balanced_recompose


class VPolyDesc(C.Structure):
    """lfplus.h lfplus_vpoly"""
    _fields_ = [("nvars", C.c_uint32), ("ntables", C.c_uint32), ("nterms", C.c_uint32), ("degree", C.c_uint32), ("term_off", C.POINTER(C.c_uint32)),
                ("term_idx", C.POINTER(C.c_uint32)), ("coef", u64p)]


class CCSDesc(C.Structure):
    """lfplus.h lfplus_ccs"""
    _fields_ = [("t", C.c_uint32), ("q", C.c_uint32), ("S_off", C.POINTER(C.c_uint32)), ("S_idx", C.POINTER(C.c_uint32)), ("c", u64p)]


def exported_symbols():
    """every symbol include/lfplus.h declares"""
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "lfplus.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(lfplus_[a-z0-9_]+)\s*\(", hdr)))


def _lib():
    global _READY
    L = api._lib()
    if not _READY:
        vp = C.c_void_p
        L.lfplus_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.lfplus_ctx_destroy.argtypes = [vp]
        L.lfplus_ctx_destroy.restype = None
        L.lfplus_scratch_trim.argtypes = [C.c_int]
        L.lfplus_scratch_trim.restype = None
        L.lfplus_scratch_bytes.argtypes = [C.c_int]
        L.lfplus_scratch_bytes.restype = C.c_size_t
        L.lfplus_last_error.argtypes = [vp]
        L.lfplus_last_error.restype = C.c_char_p
        L.lfplus_set_matrix.argtypes = [vp, u64p, C.c_uint32, C.c_uint64]
        L.lfplus_set_witness.argtypes = [vp, u64p, C.c_uint64]
        L.lfplus_witness_from_z.argtypes = [vp, u64p, C.c_uint64, C.c_uint64, C.c_uint32, u64p]
        L.lfplus_witness_from_z_timed.argtypes = [vp, u64p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
        L.lfplus_commit_resident.argtypes = [vp, u64p]
        L.lfplus_rg_from_f.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32]
        L.lfplus_rg_from_f_async.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32]
        L.lfplus_join_async.argtypes = [vp]
        L.lfplus_rg_read.argtypes = [vp, i8p, u64p, u64p, i8p, u64p, u64p, u64p]
        L.lfplus_rg_from_f_timed.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
        L.lfplus_commit.argtypes = [vp, u64p, C.c_uint64, u64p]
        u32pp, u64pp = C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(u64p)
        L.lfplus_decompose.argtypes = [vp, C.c_uint64, u64p, u64p, C.c_uint32, u32pp, u32pp, u64pp, u64p, u64p, u64p, u64p, u64p, u64p]
        L.lfplus_decompose_resident.argtypes = [vp, C.c_uint64, u64p, u64p, C.c_uint32, u32pp, u32pp, u64pp, vp, vp, u64p, u64p, u64p, u64p]
        L.lfplus_get_witness.argtypes = [vp, u64p, C.c_uint64]
        uip = C.POINTER(C.c_uint)
        L.lfplus_r1cs_check.argtypes = [vp, u64p, u32pp, u32pp, u64pp, C.c_uint64, uip, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.lfplus_linb_check.argtypes = [vp, u64p, u64p, u64p, C.c_uint32, u32pp, u32pp, u64pp, u64p, C.c_uint64, uip, C.POINTER(C.c_uint64)]
        L.lfplus_tensor.argtypes = [vp, u64p, C.c_uint32, u64p]
        L.lfplus_tensor_product.argtypes = [vp, u64p, C.c_uint64, u64p, C.c_uint64, u64p]
        u8p, vpp, ip = C.POINTER(C.c_uint8), C.POINTER(vp), C.POINTER(C.c_int)
        L.lfplus_transcript_new.restype = vp
        L.lfplus_transcript_clone.restype = vp
        L.lfplus_transcript_clone.argtypes = [vp]
        L.lfplus_transcript_free.argtypes = [vp]
        L.lfplus_transcript_free.restype = None
        L.lfplus_transcript_absorb.argtypes = [vp, u64p, C.c_size_t]
        L.lfplus_transcript_challenge.argtypes = [vp, u64p]
        L.lfplus_transcript_squeeze_bytes.argtypes = [vp, C.c_size_t, u8p]
        L.lfplus_short_challenge.argtypes = [vp, u64p]
        L.lfplus_poseidon_params.argtypes = [u64p, u64p]
        L.lfplus_poseidon_permute.argtypes = [u64p, C.c_int]
        L.lfplus_set_check.argtypes = [vp, vp, C.c_uint32, i8p, C.c_uint32, C.c_uint32, i8p, C.c_uint32, C.c_uint32, u32pp, u32pp, u64pp, u64p, u64p, u64p, u64p]
        L.lfplus_set_check_verify.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p, u64p, u64p, u64p, ip]
        L.lfplus_range_check.argtypes = [vpp, C.c_uint32, vp, C.c_uint32, u32pp, u32pp, u64pp] + [u64p] * 8
        L.lfplus_range_check_verify.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32] + [u64p] * 8 + [ip]
        L.lfplus_cm_prove.argtypes = [vpp, C.c_uint32, vp, C.c_uint32, C.c_uint32, u32pp, u32pp, u64pp] + [u64p] * 17
        L.lfplus_cm_read_g.argtypes = [vp, u64p]
        L.lfplus_share_matrix.argtypes = [vp, vp]
        L.lfplus_set_matrices.argtypes = [vp, C.c_uint64, C.c_uint32, u32pp, u32pp, u64pp]
        L.lfplus_share_matrices.argtypes = [vp, vp]
        L.lfplus_r1cs_linearize.argtypes = [vp, vp, u32pp, u32pp, u64pp, u64p, u64p, u64p]
        L.lfplus_r1cs_verify.argtypes = [vp, C.c_uint32, u64p, u64p, u64p, ip]
        L.lfplus_decomp_verify.argtypes = [u64p, u64p, C.c_uint32, u64p, u64p, C.c_uint32, u64p, u64p, C.c_uint64, ip]
        L.lfplus_mlin.argtypes = [vpp, C.c_uint32, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, u32pp, u32pp, u64pp] + [u64p] * 19
        L.lfplus_cm_verify.argtypes = [vp] + [C.c_uint32] * 6 + [u64pp] + [u64p] * 15 + [ip]
        L.lfplus_set_sharding.argtypes = [vp, C.c_int, C.c_int, api.EXCHANGE_FN, vp]
        L.lfplus_dist_unique_id.argtypes = [u8p]
        L.lfplus_dist_init.argtypes = [vp, C.c_int, C.c_int, u8p]
        L.lfplus_dist_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
        # the _dev twins (lfplus.h "device-resident callers"): the O(n) arrays are device addresses
        L.lfplus_ctx_wait_stream.argtypes = [vp, vp]
        L.lfplus_set_witness_dev.argtypes = [vp, vp, C.c_uint64]
        L.lfplus_witness_from_z_dev.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, u64p]
        L.lfplus_commit_dev.argtypes = [vp, vp, C.c_uint64, u64p]
        L.lfplus_get_witness_dev.argtypes = [vp, vp, C.c_uint64]
        L.lfplus_decompose_dev.argtypes = [vp, C.c_uint64, u64p, u64p, C.c_uint32, u32pp, u32pp, u64pp, vp, vp, u64p, u64p, u64p, u64p]
        # the generic sumcheck (lfplus_mlsumcheck_*)
        dp = C.POINTER(VPolyDesc)
        L.lfplus_mlsumcheck_begin.argtypes = [vp, dp, u64p]
        L.lfplus_mlsumcheck_begin_device.argtypes = [vp, dp, vp]
        L.lfplus_mlsumcheck_round.argtypes = [vp, u64p, u64p]
        L.lfplus_mlsumcheck_final.argtypes = [vp, u64p, u64p]
        L.lfplus_mlsumcheck_end.argtypes = [vp]
        L.lfplus_mlsumcheck_prove.argtypes = [vp, vp, dp, u64p, u64p, u64p, u64p]
        L.lfplus_mlsumcheck_prove_device.argtypes = [vp, vp, dp, vp, u64p, u64p, u64p]
        L.lfplus_mlsumcheck_verify.argtypes = [vp, C.c_uint32, C.c_uint32, u64p, u64p, u64p, u64p, ip]
        # ring arithmetic on arrays (the _device forms: a, out, x, y -- and b of mode 0 -- are device addresses; b of mode 1 stays a host pointer, so it is
        # passed as an address in both modes)
        L.lfplus_ring_mul.argtypes = [vp, u64p, u64p, C.c_uint64, C.c_uint64, C.c_int, u64p]
        L.lfplus_ring_mul_device.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_int, vp]
        L.lfplus_spmv.argtypes = [vp, C.c_uint32, u64p, C.c_uint64, u64p]
        L.lfplus_spmv_device.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp]
        # MLE tables on arrays (the _device forms: tables, v and the O(n) outputs are device addresses; points and the results of an evaluation stay host pointers)
        L.lfplus_build_eq.argtypes = [vp, u64p, C.c_uint32, u64p]
        L.lfplus_build_eq_device.argtypes = [vp, u64p, C.c_uint32, vp]
        L.lfplus_mle_eval_batch.argtypes = [vp, u64p, C.c_uint32, C.c_uint64, u64p, C.c_uint32, u64p]
        L.lfplus_mle_eval_batch_device.argtypes = [vp, vp, C.c_uint32, C.c_uint64, u64p, C.c_uint32, u64p]
        L.lfplus_mle_fix_variables.argtypes = [vp, u64p, C.c_uint32, C.c_uint64, u64p, C.c_uint32, u64p]
        L.lfplus_mle_fix_variables_device.argtypes = [vp, vp, C.c_uint32, C.c_uint64, u64p, C.c_uint32, vp]
        L.lfplus_spmv_t.argtypes = [vp, C.c_uint32, u64p, C.c_uint64, u64p]
        L.lfplus_spmv_t_device.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp]
        # gadget maps on arrays (the _device forms: in, out and v are device addresses; absmax and the CSR arrays stay host pointers)
        L.lfplus_balanced_decompose.argtypes = [vp, u64p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, u64p]
        L.lfplus_balanced_decompose_device.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, vp]
        L.lfplus_balanced_recompose.argtypes = [vp, u64p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, u64p]
        L.lfplus_balanced_recompose_device.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, vp]
        L.lfplus_linf_norm.argtypes = [vp, u64p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.lfplus_linf_norm_device.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.lfplus_set_matrices_gadget.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, u32pp, u32pp, u64pp]
        # committed CCS instances (lfplus_ccs_*)
        cp = C.POINTER(CCSDesc)
        L.lfplus_ccs_linearize.argtypes = [vp, vp, cp, u32pp, u32pp, u64pp, u64p, u64p, u64p]
        L.lfplus_ccs_verify.argtypes = [vp, C.c_uint32, cp, u64p, u64p, u64p, ip]
        L.lfplus_ccs_check.argtypes = [vp, u64p, cp, u32pp, u32pp, u64pp, C.c_uint64, uip, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _READY = True
    return L


def _w(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(u64p)


def _dev(t, shape=None):
    """device array (api.is_device_array: a torch tensor) -> its address for a _dev entry point: contiguous, 8-byte elements, (rows, 16) -- `shape` when given"""
    if not t.is_contiguous() or t.element_size() != 8 or t.dim() != 2 or t.shape[1] != D or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise LfPlusError(E_ARG, f"device arrays must be contiguous, 8-byte elements, shape {tuple(shape) if shape is not None else '(rows, 16)'}")
    return C.c_void_p(t.data_ptr())


@dataclass
class DecompParameters:
    """rgchk.rs:20-24"""
    b: int
    k: int
    l: int

    @staticmethod
    def for_frog(k, b=D // 2):
        """l = ceil(log_{d/2} q) as every reference call site computes it (rgchk.rs:369-371, benches/double_commitment.rs:68-70)"""
        return DecompParameters(b, k, math.ceil(math.log(float(P)) / math.log(D / 2)))


def scratch_bytes(device=0):
    """Bytes of idle scratch the process-wide cache holds on `device` (lfplus_scratch_bytes)"""
    return int(_lib().lfplus_scratch_bytes(int(device)))


def scratch_trim(device=-1):
    """Frees the scratch blocks destroyed contexts left in the process-wide cache (lfplus_scratch_trim; device < 0: every device)"""
    _lib().lfplus_scratch_trim(int(device))


class _Resident(tuple):
    """M = RESIDENT(count): use the matrices lfplus_set_matrices left in the (first) context"""


def RESIDENT(count):
    return _Resident((None,) * count)


class PlusContext:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        rc = _lib().lfplus_ctx_create(device, C.byref(self.h))
        if rc:
            raise LfPlusError(rc, "lfplus_ctx_create: no usable HIP device (the library has no CPU path)")
        self.kappa = self.n = 0

    def _chk(self, rc):
        if rc:
            raise LfPlusError(rc, _lib().lfplus_last_error(self.h).decode())

    def close(self):
        if self.h:
            _lib().lfplus_ctx_destroy(self.h)
            self.h = C.c_void_p()

    shard = (0, 1)     # (rank, world) of a column-sharded prover

    def set_sharding_model(self, rank, world):
        """lfplus_set_sharding_model: a TIMING model of rank `rank` of `world` with no peers (tools/shard_model.py --lfplus); what such a prover returns is not a proof"""
        L = _lib()
        L.lfplus_set_sharding_model.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._chk(L.lfplus_set_sharding_model(self.h, int(rank), int(world)))
        self.shard = (rank, world)

    def dist_stats_words(self, reset=False):
        L = _lib()
        L.lfplus_dist_stats_words.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        w = C.c_uint64()
        self._chk(L.lfplus_dist_stats_words(self.h, C.byref(w), int(reset)))
        return w.value

    def set_sharding(self, rank, world, allgather):
        """Column sharding over a HOST transport (lfplus_set_sharding); call before set_matrix.  allgather(np.uint64[words]) -> np.uint64[world, words]
        in rank order (latticefold_amd.dist.make_allgather)."""
        def _cb(user, send, recv, words):
            try:
                mine = np.ctypeslib.as_array(send, shape=(words,)).copy()
                out = np.ascontiguousarray(allgather(mine), dtype=np.uint64).reshape(world * words)
                C.memmove(recv, out.ctypes.data, world * words * 8)
                return 0
            except Exception as e:  # never let an exception cross the C boundary
                import sys
                print("lfplus exchange callback failed:", repr(e), file=sys.stderr)
                return -1
        self._exchange_cb = api.EXCHANGE_FN(_cb) if world > 1 else api.EXCHANGE_FN(0)
        self._chk(_lib().lfplus_set_sharding(self.h, rank, world, self._exchange_cb, None))
        self.shard = (rank, world)

    def dist_init(self, rank, world, id128):
        """Column sharding over RCCL (lfplus_dist_init): id128 = the bytes of an ncclUniqueId (plus.dist_unique_id() on rank 0, broadcast by the launcher)"""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(id128))
        self._chk(_lib().lfplus_dist_init(self.h, rank, world, buf))
        self.shard = (rank, world)

    def dist_stats(self, reset=False):
        n, tot, mx = C.c_uint64(), C.c_double(), C.c_double()
        self._chk(_lib().lfplus_dist_stats(self.h, C.byref(n), C.byref(tot), C.byref(mx), int(reset)))
        return n.value, tot.value, mx.value

    def set_matrix(self, A):
        """A: (kappa, n, 16) canonical words (Matrix<R>, coefficient form); in a sharded context the rank's columns (kappa, n / world, 16)"""
        A, p = _w(A)
        assert A.ndim == 3 and A.shape[2] == D
        self._chk(_lib().lfplus_set_matrix(self.h, p, A.shape[0], A.shape[1]))
        self.kappa, self.n = A.shape[0], A.shape[1] * self.shard[1]

    def generate_matrix(self, seed, kappa, n, iters=0):
        """lfplus_matrix_generate: the (kappa, n, 16) commitment matrix filled on the device, word w = splitmix64(seed + (w + 1) G) mod p -- the words of
        PlusWorkload.ajtai_matrix for seed = PlusWorkload.ajtai_seed, with no host generation and no upload.  iters > 0: the fill alone that many times more
        between two HIP events -> average milliseconds (lfplus_matrix_generate_timed)"""
        ms = C.c_double()
        if iters:
            self._chk(_nlib().lfplus_matrix_generate_timed(self.h, int(seed) & (2**64 - 1), int(kappa), int(n), int(iters), C.byref(ms)))
        else:
            self._chk(_nlib().lfplus_matrix_generate(self.h, int(seed) & (2**64 - 1), int(kappa), int(n)))
        self.kappa, self.n = int(kappa), int(n)
        return ms.value if iters else None

    def share_matrix(self, other):
        """use `other`'s resident commitment matrix (no copy, reference-counted) -- and, for a sharded prover, its transport"""
        self._chk(_lib().lfplus_share_matrix(self.h, other.h))
        self.kappa, self.n, self.shard = other.kappa, other.n, other.shard

    def set_matrices(self, M, n=None):
        """make the constraint-system matrices resident (CSR triples); calls that get M = RESIDENT then use them without another upload"""
        keep, rp, cp, vp = _csr_args(M)
        self._chk(_lib().lfplus_set_matrices(self.h, n if n is not None else self.n, len(M), rp, cp, vp))
        self._nres = len(M)

    def share_matrices(self, other):
        self._chk(_lib().lfplus_share_matrices(self.h, other.h))

    def wait_stream(self, stream=None):
        """lfplus_ctx_wait_stream: both streams of the context wait for what is enqueued so far on `stream` (a hipStream_t address; default: the current torch
        stream); the host does not wait"""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        self._chk(_lib().lfplus_ctx_wait_stream(self.h, C.c_void_p(stream)))

    def _dev_in(self, t, shape=None):
        """a device input: its address, after ordering the context behind the stream it was produced on (the current torch stream)"""
        p = _dev(t, shape)
        self.wait_stream()
        return p

    def set_witness(self, f):
        """f: (n, 16) host array, or a device array (lfplus_set_witness_dev: copied and checked on the device, nothing crosses PCIe)"""
        if api.is_device_array(f):
            return self._chk(_lib().lfplus_set_witness_dev(self.h, self._dev_in(f), f.shape[0]))
        f, p = _w(f)
        assert f.ndim == 2 and f.shape[1] == D
        self._chk(_lib().lfplus_set_witness(self.h, p, f.shape[0]))

    def witness_from_z(self, z, b, k):
        """ComR1CS::new on the device (lfplus_witness_from_z): f = z.gadget_decompose(b, k) becomes the resident witness, only z is uploaded -> cm_f = A f.
        A device array z is read in place (lfplus_witness_from_z_dev)"""
        out = np.zeros((self.kappa, D), dtype=np.uint64)
        if api.is_device_array(z):
            self._chk(_lib().lfplus_witness_from_z_dev(self.h, self._dev_in(z), z.shape[0], int(b), int(k), out.ctypes.data_as(u64p)))
            return out
        z, p = _w(z)
        assert z.ndim == 2 and z.shape[1] == D
        self._chk(_lib().lfplus_witness_from_z(self.h, p, z.shape[0], int(b), int(k), out.ctypes.data_as(u64p)))
        return out

    def time_witness_from_z(self, z, b, k, iters):
        """lfplus_witness_from_z_timed: HIP-event milliseconds of the ingestion pass alone (z resident), averaged over `iters`"""
        z, p = _w(z)
        ms = C.c_double()
        self._chk(_lib().lfplus_witness_from_z_timed(self.h, p, z.shape[0], int(b), int(k), int(iters), C.byref(ms)))
        return ms.value

    def commit_resident(self):
        """Matrix::try_mul_vec on the resident witness (lfplus_commit_resident: no upload)"""
        out = np.zeros((self.kappa, D), dtype=np.uint64)
        self._chk(_lib().lfplus_commit_resident(self.h, out.ctypes.data_as(u64p)))
        return out

    def commit(self, v):
        """Matrix::try_mul_vec; a device array v is read in place (lfplus_commit_dev)"""
        out = np.zeros((self.kappa, D), dtype=np.uint64)
        if api.is_device_array(v):
            self._chk(_lib().lfplus_commit_dev(self.h, self._dev_in(v), v.shape[0], out.ctypes.data_as(u64p)))
            return out
        v, p = _w(v)
        self._chk(_lib().lfplus_commit(self.h, p, v.shape[0], out.ctypes.data_as(u64p)))
        return out

    def tensor(self, r):
        r, p = _w([int(x) % P for x in r])
        out = np.zeros(1 << r.size, dtype=np.uint64)
        self._chk(_lib().lfplus_tensor(self.h, p, r.size, out.ctypes.data_as(u64p)))
        return out

    def tensor_product(self, a, b):
        a, pa = _w([int(x) % P for x in a])
        b, pb = _w([int(x) % P for x in b])
        out = np.zeros(a.size * b.size if a.size and b.size else a.size + b.size, dtype=np.uint64)
        self._chk(_lib().lfplus_tensor_product(self.h, pa, a.size, pb, b.size, out.ctypes.data_as(u64p)))
        return out

    def get_witness(self, out=None):
        """the context's resident witness (n, 16), read back from the device; out = a device array (n, 16): copied there instead (lfplus_get_witness_dev) and
        returned"""
        if out is not None:
            if not api.is_device_array(out):
                raise LfPlusError(E_ARG, "get_witness: out must be a device array")
            self._chk(_lib().lfplus_get_witness_dev(self.h, self._dev_in(out, (self.n, D)), self.n))
            return out
        out = np.zeros((self.n, D), dtype=np.uint64)
        self._chk(_lib().lfplus_get_witness(self.h, out.ctypes.data_as(u64p), self.n))
        return out

    def ring_mul(self, a, b, broadcast=False, out=None):
        """lfplus_ring_mul: out[x] = sum_i a_i[x] * b_i[x] (negacyclic products).  a: (count, 16) or (n_terms, count, 16); b: the shape of a, or with
        broadcast=True one coefficient per term, (16,) or (n_terms, 16), always a host array.  a, b and out are numpy arrays, or device arrays
        (lfplus_ring_mul_device: read and written in place).  out (count, 16): default a new array; it may be a (or b, element-wise) when n_terms == 1"""
        dev = api.is_device_array(a)
        sh = tuple(a.shape)
        if len(sh) not in (2, 3) or sh[-1] != D:
            raise LfPlusError(E_ARG, "ring_mul: a is (count, 16) or (n_terms, count, 16)")
        n_terms, count = (1, sh[0]) if len(sh) == 2 else (sh[0], sh[1])
        if broadcast:
            if api.is_device_array(b):
                raise LfPlusError(E_ARG, "ring_mul: the coefficients of a broadcast are a host array")
            bk = np.ascontiguousarray(b, dtype=np.uint64)
            if bk.size != n_terms * D:
                raise LfPlusError(E_ARG, "ring_mul: b is one ring element per term")
        elif api.is_device_array(b) != dev or tuple(b.shape) != sh:
            raise LfPlusError(E_ARG, "ring_mul: b has the shape and the memory space of a")
        if out is not None and (api.is_device_array(out) != dev or tuple(out.shape) != (count, D)):
            raise LfPlusError(E_ARG, "ring_mul: out is (count, 16) in the memory space of a")
        mode = MUL_BROADCAST if broadcast else MUL_ELEMENTWISE
        if dev:
            if out is None:
                out = a.new_empty((count, D))
            for t in (a, out) if broadcast else (a, b, out):
                if not t.is_contiguous() or t.element_size() != 8:
                    raise LfPlusError(E_ARG, "device arrays must be contiguous with 8-byte elements")
            self.wait_stream()
            pb = C.c_void_p(bk.ctypes.data) if broadcast else C.c_void_p(b.data_ptr())
            self._chk(_lib().lfplus_ring_mul_device(self.h, C.c_void_p(a.data_ptr()), pb, n_terms, count, mode, C.c_void_p(out.data_ptr())))
            return out
        square = b is a
        a, pa = _w(a)
        bk, pb = (bk, bk.ctypes.data_as(u64p)) if broadcast else ((a, pa) if square else _w(b))
        if out is None:
            out = np.zeros((count, D), dtype=np.uint64)
        elif out.dtype != np.uint64 or not out.flags["C_CONTIGUOUS"]:
            raise LfPlusError(E_ARG, "ring_mul: out is a contiguous uint64 array")
        self._chk(_lib().lfplus_ring_mul(self.h, pa, pb, n_terms, count, mode, out.ctypes.data_as(u64p)))
        return out

    def spmv(self, j, x, out=None):
        """lfplus_spmv: M_j x for the j-th resident matrix (set_matrices / share_matrices); x (n, 16), a numpy array or a device array
        (lfplus_spmv_device) -> out (n, 16) in the memory space of x"""
        if len(tuple(x.shape)) != 2 or x.shape[1] != D:
            raise LfPlusError(E_ARG, "spmv: x is (n, 16)")
        n = x.shape[0]
        dev = api.is_device_array(x)
        if out is not None and (api.is_device_array(out) != dev or tuple(out.shape) != (n, D)):
            raise LfPlusError(E_ARG, "spmv: out is (n, 16) in the memory space of x")
        if dev:
            if out is None:
                out = x.new_empty((n, D))
            px, po = _dev(x), _dev(out)
            self.wait_stream()
            self._chk(_lib().lfplus_spmv_device(self.h, int(j), px, n, po))
            return out
        x, px = _w(x)
        if out is None:
            out = np.zeros((n, D), dtype=np.uint64)
        elif out.dtype != np.uint64 or not out.flags["C_CONTIGUOUS"]:
            raise LfPlusError(E_ARG, "spmv: out is a contiguous uint64 array")
        self._chk(_lib().lfplus_spmv(self.h, int(j), px, n, out.ctypes.data_as(u64p)))
        return out

    @staticmethod
    def _point(point, who):
        pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1)
        if pt.size < 1:
            raise LfPlusError(E_ARG, f"{who}: the point has at least one word")
        return pt

    @staticmethod
    def _tables(tables, who):
        """tables (len, 16) or (ntables, len, 16), numpy or device -> (is_device, ntables, len)"""
        sh = tuple(tables.shape)
        if len(sh) not in (2, 3) or sh[-1] != D:
            raise LfPlusError(E_ARG, f"{who}: tables are (len, 16) or (ntables, len, 16)")
        dev = api.is_device_array(tables)
        if dev and (not tables.is_contiguous() or tables.element_size() != 8):
            raise LfPlusError(E_ARG, "device arrays must be contiguous with 8-byte elements")
        return (dev, 1, sh[0]) if len(sh) == 2 else (dev, sh[0], sh[1])

    def build_eq(self, point, out=None):
        """lfplus_build_eq: the table eq(point, .) as constant polynomials, (2^nv, 16) -- the eq factor MLSumcheck takes.  Answers a numpy array, or writes the
        device array `out` (2^nv, 16) (lfplus_build_eq_device: nothing crosses PCIe) and returns it"""
        pt = self._point(point, "build_eq")
        nv = pt.size
        if out is not None and api.is_device_array(out):
            self._chk(_lib().lfplus_build_eq_device(self.h, pt.ctypes.data_as(u64p), nv, self._dev_in(out, (1 << nv, D))))
            return out
        if out is None:
            out = np.zeros((1 << nv, D), dtype=np.uint64)
        elif out.dtype != np.uint64 or not out.flags["C_CONTIGUOUS"] or out.shape != (1 << nv, D):
            raise LfPlusError(E_ARG, "build_eq: out is a contiguous uint64 array of (2^nv, 16)")
        self._chk(_lib().lfplus_build_eq(self.h, pt.ctypes.data_as(u64p), nv, out.ctypes.data_as(u64p)))
        return out

    def mle_eval_batch(self, tables, point):
        """lfplus_mle_eval_batch: out[j] = sum_{x < len} eq(point, x) T_j[x] for tables (len, 16) or (ntables, len, 16) of general ring elements, len <= 2^nv
        (entries from len on count as zero); a device array is read in place (lfplus_mle_eval_batch_device) -> a numpy array (16,) or (ntables, 16)"""
        pt = self._point(point, "mle_eval_batch")
        dev, nt, ln = self._tables(tables, "mle_eval_batch")
        out = np.zeros((nt, D), dtype=np.uint64)
        if dev:
            self.wait_stream()
            self._chk(_lib().lfplus_mle_eval_batch_device(self.h, C.c_void_p(tables.data_ptr()), nt, ln, pt.ctypes.data_as(u64p), pt.size, out.ctypes.data_as(u64p)))
        else:
            t, p = _w(tables)
            self._chk(_lib().lfplus_mle_eval_batch(self.h, p, nt, ln, pt.ctypes.data_as(u64p), pt.size, out.ctypes.data_as(u64p)))
        return out[0] if len(tuple(tables.shape)) == 2 else out

    def mle_fix_variables(self, tables, point, out=None):
        """lfplus_mle_fix_variables: the LOWEST len(point) variables of tables (len, 16) or (ntables, len, 16), len a power of two, fixed at the point ->
        (len >> nfix, 16) or (ntables, len >> nfix, 16) in the memory space of the tables (lfplus_mle_fix_variables_device reads and writes in place)"""
        pt = self._point(point, "mle_fix_variables")
        dev, nt, ln = self._tables(tables, "mle_fix_variables")
        if ln >> pt.size < 1 or ln & (ln - 1):
            raise LfPlusError(E_ARG, "mle_fix_variables: len is a power of two of at least 2^nfix entries")
        osh = (ln >> pt.size, D) if len(tuple(tables.shape)) == 2 else (nt, ln >> pt.size, D)
        if out is not None and (api.is_device_array(out) != dev or tuple(out.shape) != osh):
            raise LfPlusError(E_ARG, f"mle_fix_variables: out is {osh} in the memory space of the tables")
        if dev:
            if out is None:
                out = tables.new_empty(osh)
            if not out.is_contiguous() or out.element_size() != 8:
                raise LfPlusError(E_ARG, "device arrays must be contiguous with 8-byte elements")
            self.wait_stream()
            self._chk(_lib().lfplus_mle_fix_variables_device(self.h, C.c_void_p(tables.data_ptr()), nt, ln, pt.ctypes.data_as(u64p), pt.size,
                                                             C.c_void_p(out.data_ptr())))
            return out
        t, p = _w(tables)
        if out is None:
            out = np.zeros(osh, dtype=np.uint64)
        elif out.dtype != np.uint64 or not out.flags["C_CONTIGUOUS"]:
            raise LfPlusError(E_ARG, "mle_fix_variables: out is a contiguous uint64 array")
        self._chk(_lib().lfplus_mle_fix_variables(self.h, p, nt, ln, pt.ctypes.data_as(u64p), pt.size, out.ctypes.data_as(u64p)))
        return out

    def spmv_t(self, j, v, out=None):
        """lfplus_spmv_t: M_j^T v for the j-th resident matrix (set_matrices / share_matrices); v (n, 16) general ring elements, a numpy array or a device
        array (lfplus_spmv_t_device) -> out (n, 16) in the memory space of v"""
        if len(tuple(v.shape)) != 2 or v.shape[1] != D:
            raise LfPlusError(E_ARG, "spmv_t: v is (n, 16)")
        n = v.shape[0]
        dev = api.is_device_array(v)
        if out is not None and (api.is_device_array(out) != dev or tuple(out.shape) != (n, D)):
            raise LfPlusError(E_ARG, "spmv_t: out is (n, 16) in the memory space of v")
        if dev:
            if out is None:
                out = v.new_empty((n, D))
            pv, po = _dev(v), _dev(out)
            self.wait_stream()
            self._chk(_lib().lfplus_spmv_t_device(self.h, int(j), pv, n, po))
            return out
        v, pv = _w(v)
        if out is None:
            out = np.zeros((n, D), dtype=np.uint64)
        elif out.dtype != np.uint64 or not out.flags["C_CONTIGUOUS"]:
            raise LfPlusError(E_ARG, "spmv_t: out is a contiguous uint64 array")
        self._chk(_lib().lfplus_spmv_t(self.h, int(j), pv, n, out.ctypes.data_as(u64p)))
        return out

    def _digits(self, name, x, nin, nout, b, k, layout, out):
        """the body of balanced_decompose / balanced_recompose: x (nin, 16) -> out (nout, 16) in the memory space of x"""
        if len(tuple(x.shape)) != 2 or x.shape[1] != D or x.shape[0] != nin:
            raise LfPlusError(E_ARG, f"{name}: the input is ({nin}, 16)")
        dev = api.is_device_array(x)
        if out is not None and (api.is_device_array(out) != dev or tuple(out.shape) != (nout, D)):
            raise LfPlusError(E_ARG, f"{name}: out is ({nout}, 16) in the memory space of the input")
        count = min(nin, nout)
        if dev:
            if out is None:
                out = x.new_empty((nout, D))
            pi, po = _dev(x), _dev(out)
            self.wait_stream()
            self._chk(getattr(_lib(), f"lfplus_{name}_device")(self.h, pi, count, int(b), int(k), int(layout), po))
            return out
        x, pi = _w(x)
        if out is None:
            out = np.zeros((nout, D), dtype=np.uint64)
        elif out.dtype != np.uint64 or not out.flags["C_CONTIGUOUS"]:
            raise LfPlusError(E_ARG, f"{name}: out is a contiguous uint64 array")
        self._chk(getattr(_lib(), f"lfplus_{name}")(self.h, pi, count, int(b), int(k), int(layout), out.ctypes.data_as(u64p)))
        return out

    def balanced_decompose(self, x, b, k, layout=DIGITS_GADGET, out=None):
        """lfplus_balanced_decompose: the k balanced base-b digits of every coefficient of x (count, 16), as canonical residues -> (count k, 16): digit i of element
        j at row j k + i (DIGITS_GADGET: Vec<R>::gadget_decompose) or i count + j (DIGITS_PLANES: decompose_to_vec(b, k).transpose()); a numpy array or a device
        array (lfplus_balanced_decompose_device), out in the memory space of x"""
        return self._digits("balanced_decompose", x, x.shape[0], x.shape[0] * int(k), b, k, layout, out)

    def balanced_recompose(self, x, b, k, layout=DIGITS_GADGET, out=None):
        """lfplus_balanced_recompose: out[j] = sum_i b^i x[digit i of j] coefficient by coefficient mod p, x (count k, 16) GENERAL ring elements -> (count, 16)"""
        if int(k) < 1 or x.shape[0] % int(k):
            raise LfPlusError(E_ARG, "balanced_recompose: the input is (count k, 16)")
        return self._digits("balanced_recompose", x, x.shape[0], x.shape[0] // int(k), b, k, layout, out)

    def linf_norm(self, v):
        """lfplus_linf_norm: the largest |centred coefficient| of v (count, 16), a numpy array or a device array (lfplus_linf_norm_device) -> int"""
        if len(tuple(v.shape)) != 2 or v.shape[1] != D:
            raise LfPlusError(E_ARG, "linf_norm: v is (count, 16)")
        am = C.c_uint64()
        if api.is_device_array(v):
            pv = _dev(v)
            self.wait_stream()
            self._chk(_lib().lfplus_linf_norm_device(self.h, pv, v.shape[0], C.byref(am)))
        else:
            v, pv = _w(v)
            self._chk(_lib().lfplus_linf_norm(self.h, pv, v.shape[0], C.byref(am)))
        return am.value

    def set_matrices_gadget(self, M, m, b, k, n=None):
        """lfplus_set_matrices_gadget: the system as stated over z -- CSR triples of rows x m with ring coefficients -- made resident in its gadget form over
        f = gadget_decompose(z, b, k), n = m k: what set_matrices(r1cs_decomposed_square(M, n, b, k)) leaves, expanded on the device from the short arrays"""
        keep, rp, cp, vp = _csr_args(M)
        rows = keep[0][0].size - 1 if keep else 0
        if any(r.size - 1 != rows for r, _, _ in keep):
            raise LfPlusError(E_ARG, "set_matrices_gadget: the matrices have the same number of rows")
        self._chk(_lib().lfplus_set_matrices_gadget(self.h, rows, int(m), int(b), int(k), int(n) if n is not None else int(m) * int(k), len(M), rp, cp, vp))
        self._nres = len(M)

    def _cm_arg(self, cm_f):
        if cm_f is None:
            return None, None
        cm = np.ascontiguousarray(cm_f, dtype=np.uint64)
        if cm.shape != (self.kappa, D):
            raise LfPlusError(E_ARG, f"relation check: cm_f must be (kappa, 16) = ({self.kappa}, {D})")
        return cm, cm.ctypes.data_as(u64p)

    def r1cs_check(self, cm_f, M=RESIDENT(3), bound=0):
        """R_ComR1CS on the resident (A, f) (lfplus_r1cs_check; r1cs.rs:21-60): cm_f = A f (None: not checked), (M_A f) o (M_B f) = M_C f row by row, and
        ||f||_inf < bound (0: not checked) -> (ok, failed, first_bad, absmax): failed = OR of the REL_* bits of the failing components, first_bad = the smallest
        row with a non-zero residual (n when all hold), absmax = the largest |centred coefficient| of f.  Nothing but these words leaves the device."""
        if len(M) != 3:
            raise LfPlusError(E_ARG, "r1cs_check: an R1CS has three matrices")
        keep, rp, cp, vp = _csr_args(M)
        cm, cmp_ = self._cm_arg(cm_f)
        failed, fb, am = C.c_uint(), C.c_uint64(), C.c_uint64()
        rc = _lib().lfplus_r1cs_check(self.h, cmp_, rp, cp, vp, int(bound), C.byref(failed), C.byref(fb), C.byref(am))
        if rc not in (0, E_REJECT):
            self._chk(rc)
        return rc == 0, failed.value, fb.value, am.value

    def ccs_check(self, cm_f, shape, M=None, bound=0):
        """The committed CCS relation on the resident (A, f) (lfplus_ccs_check): cm_f = A f (None: not checked), sum_i c_i prod_{j in S_i} (M_j f)[row] = 0 row
        by row, ||f||_inf < bound (0: not checked) -> (ok, failed, first_bad, absmax) as r1cs_check; the residual's bit is REL_CCS.  M: the shape's t matrices
        (None: the resident ones)"""
        M = RESIDENT(shape.t) if M is None else M
        if len(M) != shape.t:
            raise LfPlusError(E_ARG, f"ccs_check: the shape has {shape.t} matrices")
        keep, rp, cp, vp = _csr_args(M)
        cm, cmp_ = self._cm_arg(cm_f)
        d = shape.desc()
        failed, fb, am = C.c_uint(), C.c_uint64(), C.c_uint64()
        rc = _lib().lfplus_ccs_check(self.h, cmp_, C.byref(d), rp, cp, vp, int(bound), C.byref(failed), C.byref(fb), C.byref(am))
        if rc not in (0, E_REJECT):
            self._chk(rc)
        return rc == 0, failed.value, fb.value, am.value

    def linb_check(self, cm_f, r, v, M=(), bound=0):
        """R_LinB on the resident (A, f) (lfplus_linb_check; lin.rs:29-40): cm_f = A f (None: not checked), v[0][pt] = mle(f)(r_pt) and v[1 + j][pt] =
        mle(M_j f)(r_pt) for both points, ||f||_inf < bound (0: not checked).  r: (nvars, 2, 16) pairs of ring elements and v: (1 + len(M), 2, 16), both as
        decompose takes / returns them -> (ok, failed, absmax)"""
        nvars, nm = self.n.bit_length() - 1, len(M)
        r, v = np.ascontiguousarray(r, dtype=np.uint64), np.ascontiguousarray(v, dtype=np.uint64)
        if r.shape != (nvars, 2, D) or v.shape != (1 + nm, 2, D):
            raise LfPlusError(E_ARG, f"linb_check: r must be ({nvars}, 2, 16) and v ({1 + nm}, 2, 16)")
        r_a, r_b = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
        keep, rp, cp, vp = _csr_args(M)
        cm, cmp_ = self._cm_arg(cm_f)
        failed, am = C.c_uint(), C.c_uint64()
        rc = _lib().lfplus_linb_check(self.h, cmp_, r_a.ctypes.data_as(u64p), r_b.ctypes.data_as(u64p), nm, rp, cp, vp, v.ctypes.data_as(u64p), int(bound),
                                      C.byref(failed), C.byref(am))
        if rc not in (0, E_REJECT):
            self._chk(rc)
        return rc == 0, failed.value, am.value

    def decompose(self, f, A, B, r, M=(), into=None, out_bufs=None, out=None):
        """Decomp{f, r, M}.decompose(&A, B) (decomp.rs:32-99).  r: (nvars, 2, 16) pairs of ring elements; M: CSR matrices (rowptr, col, val[nnz][16]).
        -> dict(F0, F1 (n,16); C0, C1 (kappa,16); v0, v1 (1+len(M), 2, 16)): ((LinB0, LinB1), DecompProof) of the reference, flat.
        into = (ctx0, ctx1): F0 / F1 stay on the device as the resident witnesses of those contexts (lfplus_decompose_resident) and are not returned;
        out_bufs = (F0, F1): host arrays to receive them (already touched: a download into fresh pages is page-fault-bound, 10 ms instead of 2.4 per 2^20 rows);
        out = (F0, F1): DEVICE arrays (n, 16), either may be None -- the halves are written there by the kernel that cuts them (lfplus_decompose_dev) and
        returned under "F0" / "F1" (None for a half not asked for)"""
        dev_out = out
        if A is not None:
            self.set_matrix(A)
        if f is not None:              # None: the resident witness (e.g. the folded g Mlin.mlin left there)
            self.set_witness(f)
        r = np.ascontiguousarray(r, dtype=np.uint64)
        r_a, r_b = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
        nm = len(M)
        keep, rp, cp, vp_ = _csr_args(M)
        n, kappa = self.n, self.kappa
        out = {"C0": np.zeros((kappa, D), dtype=np.uint64), "C1": np.zeros((kappa, D), dtype=np.uint64), "v0": np.zeros((1 + nm, 2, D), dtype=np.uint64),
               "v1": np.zeros((1 + nm, 2, D), dtype=np.uint64)}
        if into is not None:
            self._chk(_lib().lfplus_decompose_resident(self.h, B, r_a.ctypes.data_as(u64p), r_b.ctypes.data_as(u64p), nm, rp, cp, vp_, into[0].h, into[1].h,
                                                       *[out[k].ctypes.data_as(u64p) for k in ("C0", "C1", "v0", "v1")]))
            return out
        if dev_out is not None:
            F = tuple(dev_out)
            if len(F) != 2 or any(x is not None and not api.is_device_array(x) for x in F):
                raise LfPlusError(E_ARG, "decompose: out must be two device arrays (or None)")
            ptrs = [None if x is None else self._dev_in(x, (n, D)) for x in F]
            self._chk(_lib().lfplus_decompose_dev(self.h, B, r_a.ctypes.data_as(u64p), r_b.ctypes.data_as(u64p), nm, rp, cp, vp_, *ptrs,
                                                  *[out[k].ctypes.data_as(u64p) for k in ("C0", "C1", "v0", "v1")]))
            out["F0"], out["F1"] = F
            return out
        if out_bufs is not None and all(isinstance(b, np.ndarray) and b.shape == (n, D) and b.dtype == np.uint64 and b.flags.c_contiguous for b in out_bufs):
            out["F0"], out["F1"] = out_bufs
        else:
            out["F0"], out["F1"] = np.zeros((n, D), dtype=np.uint64), np.zeros((n, D), dtype=np.uint64)
        self._chk(_lib().lfplus_decompose(self.h, B, r_a.ctypes.data_as(u64p), r_b.ctypes.data_as(u64p), nm, rp, cp, vp_,
                                          *[out[k].ctypes.data_as(u64p) for k in ("F0", "F1", "C0", "C1", "v0", "v1")]))
        return out

    def rg_from_f_async(self, dparams):
        """lfplus_rg_from_f_async: RgInstance::from_f of the resident witness on the context's second stream (collected by rg_from_f / mlin with the same parameters)"""
        self._chk(_lib().lfplus_rg_from_f_async(self.h, dparams.b, dparams.k, dparams.l))

    def join_async(self):
        self._chk(_lib().lfplus_join_async(self.h))

    def time_rg_from_f(self, dparams, iters):
        ms = C.c_double()
        self._chk(_lib().lfplus_rg_from_f_timed(self.h, dparams.b, dparams.k, dparams.l, iters, C.byref(ms)))
        return ms.value


@dataclass
class FComs:
    """rgchk.rs:26-31"""
    cm_f: np.ndarray
    C_Mf: np.ndarray
    cm_mtau: np.ndarray


@dataclass
class RgInstance:
    """rgchk.rs:40-48.  M_f / m_tau are unit monomials, held as their exponent digits D_f / centred tau (exp(a) = X^a, X^(d+a) for a < 0)."""
    D_f: np.ndarray      # (k, n, 16) int8
    tau: np.ndarray      # (n,)
    m_tau_exp: np.ndarray  # (n,) int8
    f: np.ndarray
    comM_f: np.ndarray   # (k, kappa, 16, 16): comM_f[k_i] is a kappa x d matrix of ring elements
    fcoms: FComs

    @staticmethod
    def from_f(ctx, f, A, dparams):
        """RgInstance::from_f(f, &A, &decomp) (rgchk.rs:260-331).  A = None keeps the matrix already resident in ctx."""
        if A is not None:
            ctx.set_matrix(A)
        ctx.set_witness(f)
        ctx._chk(_lib().lfplus_rg_from_f(ctx.h, dparams.b, dparams.k, dparams.l))
        ctx._k = dparams.k
        k, n, kappa = dparams.k, ctx.n, ctx.kappa
        Df = np.zeros((k, n, D), dtype=np.int8)
        com = np.zeros((k, kappa, D, D), dtype=np.uint64)
        tau = np.zeros(n, dtype=np.uint64)
        mt = np.zeros(n, dtype=np.int8)
        c = [np.zeros((kappa, D), dtype=np.uint64) for _ in range(3)]
        ctx._chk(_lib().lfplus_rg_read(ctx.h, Df.ctypes.data_as(i8p), com.ctypes.data_as(u64p), tau.ctypes.data_as(u64p), mt.ctypes.data_as(i8p),
                                       *[x.ctypes.data_as(u64p) for x in c]))
        return RgInstance(Df, tau, mt, np.asarray(f), com, FComs(*c))

    def M_f(self, ki, rows=slice(None)):
        """dense monomial matrix exp(D_f[ki]) for the given rows: (rows, 16 columns, 16 words)"""
        return exp(self.D_f[ki, rows])


def dist_unique_id():
    """an ncclUniqueId (128 bytes) for PlusContext.dist_init"""
    buf = (C.c_uint8 * 128)()
    rc = _lib().lfplus_dist_unique_id(buf)
    if rc:
        raise LfPlusError(rc, "lfplus_dist_unique_id: RCCL not loadable")
    return bytes(buf)


def exp(digits):
    """stark_rings exp: digit a in (-d/2, d/2) -> the unit monomial X^a (a >= 0) / X^(d + a) (a < 0), as 16-word elements"""
    dg = np.asarray(digits, dtype=np.int64)
    if (np.abs(dg) >= D // 2).any():
        raise ValueError("exp: digit outside (-d/2, d/2)")
    out = np.zeros(dg.shape + (D,), dtype=np.uint64)
    np.put_along_axis(out, np.where(dg >= 0, dg, D + dg)[..., None], 1, axis=-1)
    return out


# ---- the transcript-driven part (src/transcript.rs, setchk.rs, rgchk.rs:81-258) ------------------------------------------------------------
def _csr_args(mats):
    """mats: list of (rowptr uint32 [n+1], col uint32 [nnz], val uint64 [nnz][16]), or RESIDENT(count)"""
    if isinstance(mats, _Resident):
        return [], None, None, None
    keep = [(np.ascontiguousarray(r, dtype=np.uint32), np.ascontiguousarray(c, dtype=np.uint32), np.ascontiguousarray(v, dtype=np.uint64)) for r, c, v in mats]
    u32p = C.POINTER(C.c_uint32)
    n = max(1, len(keep))
    return keep, (u32p * n)(*[k[0].ctypes.data_as(u32p) for k in keep]), (u32p * n)(*[k[1].ctypes.data_as(u32p) for k in keep]), \
        (u64p * n)(*[k[2].ctypes.data_as(u64p) for k in keep])


class PoseidonTranscript:
    """PoseidonTranscript::<RqPoly>::empty::<FrogPoseidonConfig>() (src/transcript.rs:20-78); host object, no GPU needed"""

    def __init__(self, h=None):
        self.h = h if h is not None else _lib().lfplus_transcript_new()

    def clone(self):
        return PoseidonTranscript(_lib().lfplus_transcript_clone(self.h))

    def absorb(self, ring):
        a = np.ascontiguousarray(ring, dtype=np.uint64).reshape(-1, D)
        _lib().lfplus_transcript_absorb(self.h, a.ctypes.data_as(u64p), a.shape[0])

    def get_challenge(self):
        o = C.c_uint64()
        _lib().lfplus_transcript_challenge(self.h, C.byref(o))
        return o.value

    def squeeze_bytes(self, n):
        o = np.zeros(n, dtype=np.uint8)
        _lib().lfplus_transcript_squeeze_bytes(self.h, n, o.ctypes.data_as(C.POINTER(C.c_uint8)))
        return o

    def short_challenge(self):
        """utils::short_challenge(128, transcript) (src/utils.rs:87-101)"""
        o = np.zeros(D, dtype=np.uint64)
        _lib().lfplus_short_challenge(self.h, o.ctypes.data_as(u64p))
        return o

    def __del__(self):
        try:
            _lib().lfplus_transcript_free(self.h)
        except Exception:
            pass


def poseidon_simd():
    """True when the transcript's permutation runs on the host's AVX-512 IFMA lanes (lfp_poseidon_simd.cc)"""
    L = _lib()
    L.lfplus_poseidon_simd.restype = C.c_int
    return bool(L.lfplus_poseidon_simd())


def poseidon_permute(state, plain=False):
    """one Poseidon permutation of 24 canonical words; plain = True / 1: the textbook definition, 2: the scalar sparse form, False / 0: the form the
    transcript runs (AVX-512 IFMA lanes when the CPU has them)"""
    st = np.ascontiguousarray(state, dtype=np.uint64).copy()
    assert st.shape == (24,)
    rc = _lib().lfplus_poseidon_permute(st.ctypes.data_as(u64p), int(plain))
    if rc:
        raise LfPlusError(rc, "lfplus_poseidon_permute")
    return st


def poseidon_params():
    ark, mds = np.zeros(720, dtype=np.uint64), np.zeros(576, dtype=np.uint64)
    _lib().lfplus_poseidon_params(ark.ctypes.data_as(u64p), mds.ctypes.data_as(u64p))
    return ark, mds


def set_check(ctx, transcript, nvars, mat_digits, vec_digits=None, M=()):
    """In::set_check (src/setchk.rs:65-262).  mat_digits (nmat, n, ncols) / vec_digits (nvec, n): exponent digits (int8; ABSENT = zero entry)
    -> dict(r, msgs (nvars, 4, 16), e (1 + len(M), nmat, ncols, 16), b (nvec, 16))"""
    md = np.ascontiguousarray(mat_digits, dtype=np.int8)
    nmat, n, ncols = md.shape
    vd = np.zeros((0, n), dtype=np.int8) if vec_digits is None else np.ascontiguousarray(vec_digits, dtype=np.int8)
    nvec, nM = vd.shape[0], len(M)
    keep, rp, cp, vp = _csr_args(M)
    r, msgs = np.zeros(nvars, dtype=np.uint64), np.zeros((nvars, 4, D), dtype=np.uint64)
    e, b = np.zeros((1 + nM, nmat, ncols, D), dtype=np.uint64), np.zeros((max(nvec, 1), D), dtype=np.uint64)
    ctx._chk(_lib().lfplus_set_check(ctx.h, transcript.h, nvars, md.ctypes.data_as(i8p), nmat, ncols, vd.ctypes.data_as(i8p) if nvec else None, nvec, nM, rp, cp, vp,
                                     r.ctypes.data_as(u64p), msgs.ctypes.data_as(u64p), e.ctypes.data_as(u64p), b.ctypes.data_as(u64p)))
    return {"r": r, "msgs": msgs, "e": e, "b": b[:nvec]}


def _shaped(proof, key, shape):
    """a proof array as contiguous u64 words of exactly `shape` -- the C verifiers index raw pointers with the VERIFIER's parameters, so a proof whose arrays
    are shorter than those parameters imply must be refused here (LFPLUS_E_ARG), never read"""
    try:
        a = np.ascontiguousarray(proof[key], dtype=np.uint64)
    except (KeyError, TypeError, ValueError, OverflowError) as ex:
        raise LfPlusError(E_ARG, f"malformed proof: field {key!r}: {ex}")
    if a.shape != tuple(shape):
        raise LfPlusError(E_ARG, f"malformed proof: field {key!r} has shape {a.shape}, the verifier's parameters require {tuple(shape)}")
    return a


def _nvars_ok(nvars):
    if not isinstance(nvars, (int, np.integer)) or not 1 <= int(nvars) <= 32:
        raise LfPlusError(E_ARG, "nvars outside [1, 32]")
    return int(nvars)


def set_check_verify(transcript, nvars, out, nM=0, nmat=None, ncols=None, nvec=None):
    """Out::verify (src/setchk.rs:266-340) on the host -> (accepted, stage, r).  nvars and nM are the VERIFIER's; nmat / ncols / nvec default to the shape of
    out["e"] / out["b"], and every array is checked against them before the C verifier sees a pointer"""
    nvars = _nvars_ok(nvars)
    e0, b0 = np.asarray(out["e"]), np.asarray(out["b"])
    if e0.ndim != 4 or b0.ndim != 2:
        raise LfPlusError(E_ARG, "malformed proof: e must be (1 + nM, nmat, ncols, 16), b (nvec, 16)")
    nmat, ncols, nvec = (e0.shape[1] if nmat is None else nmat), (e0.shape[2] if ncols is None else ncols), (b0.shape[0] if nvec is None else nvec)
    if nmat < 1 or ncols < 1:
        raise LfPlusError(E_ARG, "malformed proof: no matrix set")
    e, b, msgs = _shaped(out, "e", (1 + nM, nmat, ncols, D)), _shaped(out, "b", (nvec, D)), _shaped(out, "msgs", (nvars, 4, D))
    bb = b if nvec else np.zeros((1, D), dtype=np.uint64)
    r, st = np.zeros(nvars, dtype=np.uint64), C.c_int()
    rc = _lib().lfplus_set_check_verify(transcript.h, nvars, nmat, ncols, nvec, nM, msgs.ctypes.data_as(u64p), e.ctypes.data_as(u64p), bb.ctypes.data_as(u64p),
                                        r.ctypes.data_as(u64p), C.byref(st))
    if rc not in (0, E_REJECT):
        raise LfPlusError(rc, "lfplus_set_check_verify")
    return rc == 0, st.value, r


def range_check(ctxs, transcript, M=()):
    """Rg::range_check (src/rgchk.rs:81-186) over the resident RgInstances of `ctxs` (each after RgInstance.from_f) -> dict of the Dcom fields"""
    L, nM, c0 = len(ctxs), len(M), ctxs[0]
    if not c0.n or not getattr(c0, "_k", 0):
        raise LfPlusError(E_ARG, "range_check: no resident RgInstance (run RgInstance.from_f first)")
    n, k = c0.n, c0._k
    nvars = n.bit_length() - 1
    keep, rp, cp, vp = _csr_args(M)
    hs = (C.c_void_p * L)(*[c.h for c in ctxs])
    r, msgs = np.zeros(nvars, dtype=np.uint64), np.zeros((nvars, 4, D), dtype=np.uint64)
    e, b = np.zeros((1 + nM, L * k, D, D), dtype=np.uint64), np.zeros((L, D), dtype=np.uint64)
    v, a = np.zeros((L, D), dtype=np.uint64), np.zeros((L, 1 + nM), dtype=np.uint64)
    bb, c = np.zeros((L, 1 + nM, D), dtype=np.uint64), np.zeros((L, 1 + nM, D), dtype=np.uint64)
    c0._chk(_lib().lfplus_range_check(hs, L, transcript.h, nM, rp, cp, vp, *[x.ctypes.data_as(u64p) for x in (r, msgs, e, b, v, a, bb, c)]))
    return {"r": r, "msgs": msgs, "e": e, "b": b, "v": v, "a": a, "bb": bb, "c": c, "k": k, "nvars": nvars}


def _dcom_arrays(d, nvars, L, k, nM):
    """the Dcom fields (rgchk.rs:50-79) checked against the verifier's nvars, L, k, nM"""
    return {"msgs": _shaped(d, "msgs", (nvars, 4, D)), "e": _shaped(d, "e", (1 + nM, L * k, D, D)), "b": _shaped(d, "b", (L, D)), "v": _shaped(d, "v", (L, D)),
            "a": _shaped(d, "a", (L, 1 + nM)), "bb": _shaped(d, "bb", (L, 1 + nM, D)), "c": _shaped(d, "c", (L, 1 + nM, D))}


def range_check_verify(transcript, d, nvars=None, L=None, k=None, nM=None):
    """Dcom::verify (src/rgchk.rs:193-258) on the host -> (accepted, stage, r).  nvars / L / k / nM are the VERIFIER's parameters (a caller without its own
    takes them from the proof's metadata -- fine for a self-check, not for an untrusted proof); every array is checked against them"""
    nvars = _nvars_ok(d["nvars"] if nvars is None else nvars)
    k = int(d["k"] if k is None else k)
    L = int(np.asarray(d["b"]).shape[0] if L is None else L)
    nM = int(np.asarray(d["a"]).shape[-1] - 1 if nM is None else nM)
    if L < 1 or k < 1 or nM < 0:
        raise LfPlusError(E_ARG, "range_check_verify: bad parameters")
    arr = _dcom_arrays(d, nvars, L, k, nM)
    r, st = np.zeros(nvars, dtype=np.uint64), C.c_int()
    rc = _lib().lfplus_range_check_verify(transcript.h, nvars, L, k, nM, *[arr[key].ctypes.data_as(u64p) for key in ("msgs", "e", "b", "v", "a", "bb", "c")],
                                          r.ctypes.data_as(u64p), C.byref(st))
    if rc not in (0, E_REJECT):
        raise LfPlusError(rc, "lfplus_range_check_verify")
    return rc == 0, st.value, r


def cm_prove(ctxs, transcript, ell, M=(), want_g=False):
    """Cm::prove (src/cm.rs:56-347) over the resident RgInstances of `ctxs` -> dict of the CmProof fields (dcom = the range check's fields, comh,
    sumcheck proofs pa / pb, evals ea / eb) and of the folded instance x = (cm_g, ro, vo); `g` (L, n, 16) when want_g, else it stays on the device"""
    L, nM, c0 = len(ctxs), len(M), ctxs[0] if ctxs else None
    if not ctxs or not c0.n or not getattr(c0, "_k", 0):
        raise LfPlusError(E_ARG, "cm_prove: no resident RgInstance (run RgInstance.from_f first)")
    n, k, kappa = c0.n, c0._k, c0.kappa
    nvars = n.bit_length() - 1
    per = 4 + 4 * nM
    keep, rp, cp, vp = _csr_args(M)
    hs = (C.c_void_p * L)(*[c.h for c in ctxs])
    z = lambda *shape: np.zeros(shape, dtype=np.uint64)
    o = {"r": z(nvars), "msgs": z(nvars, 4, D), "e": z(1 + nM, L * k, D, D), "b": z(L, D), "v": z(L, D), "a": z(L, 1 + nM), "bb": z(L, 1 + nM, D),
         "c": z(L, 1 + nM, D), "comh": z(L, kappa, D), "pa": z(nvars, 3, D), "pb": z(nvars, 3, D), "ea": z(L, per, D), "eb": z(L, per, D),
         "cm_g": z(L, kappa, D), "ro": z(2, nvars), "vo": z(L, 1 + nM, 2, D)}
    g = z(L, n, D) if want_g else None
    keys = ("r", "msgs", "e", "b", "v", "a", "bb", "c", "comh", "pa", "pb", "ea", "eb", "cm_g", "ro", "vo")
    c0._chk(_lib().lfplus_cm_prove(hs, L, transcript.h, ell, nM, rp, cp, vp, *[o[key].ctypes.data_as(u64p) for key in keys],
                                   g.ctypes.data_as(u64p) if want_g else None))
    o.update(k=k, ell=ell, kappa=kappa, nvars=nvars)
    if want_g:
        o["g"] = g
    return o


def cm_read_g(ctx):
    """the folded witness g of the last cm_prove this context took part in: (n, 16) canonical words"""
    g = np.zeros((ctx.n, D), dtype=np.uint64)
    ctx._chk(_lib().lfplus_cm_read_g(ctx.h, g.ctypes.data_as(u64p)))
    return g


def cm_verify(transcript, proof, fcoms, nvars=None, L=None, k=None, ell=None, kappa=None, nM=None):
    """CmProof::verify (src/cm.rs:349-543) on the host.  fcoms[l] = (3, kappa, 16): cm_f | C_Mf | cm_mtau -> (accepted, stage, dict(cm_g, ro, vo)).
    nvars .. nM are the VERIFIER's parameters (CmProof::verify takes M.len() and the parameters from its own side, cm.rs:349-365); left None they come from
    the proof's metadata, which only a self-check should do.  Every array is checked against them before the C verifier sees a pointer"""
    nvars = _nvars_ok(proof["nvars"] if nvars is None else nvars)
    k, ell, kappa = (int(proof[key] if val is None else val) for key, val in (("k", k), ("ell", ell), ("kappa", kappa)))
    L = int(np.asarray(proof["b"]).shape[0] if L is None else L)
    nM = int(np.asarray(proof["a"]).shape[-1] - 1 if nM is None else nM)
    if L < 1 or not 1 <= k <= 16 or not 1 <= ell <= 64 or not 1 <= kappa <= 64 or not 0 <= nM <= 64:
        raise LfPlusError(E_ARG, "cm_verify: parameters outside the envelope")
    per = 4 + 4 * nM
    keys = ("msgs", "e", "b", "v", "a", "bb", "c", "comh", "pa", "pb", "ea", "eb")
    arr = _dcom_arrays(proof, nvars, L, k, nM)
    arr.update(comh=_shaped(proof, "comh", (L, kappa, D)), pa=_shaped(proof, "pa", (nvars, 3, D)), pb=_shaped(proof, "pb", (nvars, 3, D)),
               ea=_shaped(proof, "ea", (L, per, D)), eb=_shaped(proof, "eb", (L, per, D)))
    fc = [np.ascontiguousarray(x, dtype=np.uint64) for x in fcoms]
    if len(fc) != L or any(x.shape != (3, kappa, D) for x in fc):
        raise LfPlusError(E_ARG, f"cm_verify: fcoms must be {L} arrays of shape (3, {kappa}, 16)")
    fptr = (u64p * L)(*[x.ctypes.data_as(u64p) for x in fc])
    x = {"cm_g": np.zeros((L, kappa, D), dtype=np.uint64), "ro": np.zeros((2, nvars), dtype=np.uint64), "vo": np.zeros((L, 1 + nM, 2, D), dtype=np.uint64)}
    st = C.c_int()
    rc = _lib().lfplus_cm_verify(transcript.h, nvars, L, k, ell, kappa, nM, fptr, *[arr[key].ctypes.data_as(u64p) for key in keys],
                                 *[x[key].ctypes.data_as(u64p) for key in ("cm_g", "ro", "vo")], C.byref(st))
    if rc not in (0, E_REJECT):
        raise LfPlusError(rc, "lfplus_cm_verify")
    return rc == 0, st.value, x



# ---- ComR1CS / Mlin / PlusProver / PlusVerifier (src/r1cs.rs, lin.rs, mlin.rs, plus.rs) ------------------------------------------------------
@dataclass
class LinParameters:
    """lin.rs:24-28"""
    kappa: int
    decomp: DecompParameters


@dataclass
class PlusParameters:
    """plus.rs:43-47"""
    lin: LinParameters
    B: int


def _centre(x):
    x = np.asarray(x, dtype=np.uint64)
    neg = x > np.uint64(P // 2)
    return np.where(neg, -((np.uint64(P) - x) * neg).astype(np.int64), (x * ~neg).astype(np.int64))


def gadget_decompose(z, b, k):
    """Vec<R>::gadget_decompose(b, k): element j -> its k balanced base-b digits (coefficient-wise, least significant first) at positions [j k, (j + 1) k)"""
    cur = _centre(np.asarray(z, dtype=np.uint64).reshape(-1, D))
    out = np.zeros((cur.shape[0], k, D), dtype=np.int64)
    half = b // 2
    for i in range(k):
        q, rem = np.divmod(cur, b)                       # floor division: rem in [0, b)
        hi = rem > half
        rem, q = np.where(hi, rem - b, rem), np.where(hi, q + 1, q)
        if b % 2 == 0:                                    # |rem| == b / 2 keeps the sign of the value (truncating division in the reference)
            flip = (rem == half) & (cur < 0)
            rem, q = np.where(flip, rem - b, rem), np.where(flip, q + 1, q)
        out[:, i], cur = rem, q
    out = out.reshape(-1, D)
    return np.where(out < 0, np.uint64(P) - np.abs(out).astype(np.uint64), out.astype(np.uint64))


def identity_csr(m):
    """SparseMatrix::identity(m) as (rowptr, col, val[nnz][16])"""
    val = np.zeros((m, D), dtype=np.uint64)
    val[:, 0] = 1
    return np.arange(m + 1, dtype=np.uint32), np.arange(m, dtype=np.uint32), val


def gadget_decompose_csr(mat, b, k):
    """SparseMatrix::gadget_decompose(b, k): rows x m -> rows x (m k) with (M G) gadget_decompose(z) = M z: coefficient c at column j becomes
    c b^i at columns j k + i"""
    rowptr, col, val = (np.asarray(x) for x in mat)
    pw = [pow(b, i, P) for i in range(k)]
    v = np.asarray(val, dtype=np.uint64).astype(object)
    nv = np.stack([(v * pw[i]) % P for i in range(k)], axis=1).astype(np.uint64).reshape(-1, D)
    ncol = (np.asarray(col, dtype=np.uint32)[:, None] * np.uint32(k) + np.arange(k, dtype=np.uint32)[None, :]).reshape(-1)
    return (np.asarray(rowptr, dtype=np.uint32) * np.uint32(k)).astype(np.uint32), ncol.astype(np.uint32), nv


def pad_rows(mat, n):
    rowptr, col, val = mat
    rowptr = np.asarray(rowptr, dtype=np.uint32)
    return np.concatenate([rowptr, np.full(n + 1 - rowptr.size, rowptr[-1], dtype=np.uint32)]), col, val


def r1cs_decomposed_square(r1cs, n, b, k):
    """r1cs.rs:170-184: the three matrices gadget-decomposed (m -> m k columns) and padded to n rows"""
    return tuple(pad_rows(gadget_decompose_csr(m, b, k), n) for m in r1cs)


@dataclass
class ComR1CS:
    """r1cs.rs:21-58: r1cs = (A, B, C) CSR matrices (n x n), z the short witness, f = z.gadget_decompose(b, k), cm_f = A f.
    A RESIDENT instance (new_resident) has f = None: the witness was cut on the device and lives in `ctx`, until that context gets another witness"""
    r1cs: tuple
    z: np.ndarray
    f: np.ndarray
    cm_f: np.ndarray
    l_in: int = 1
    ctx: object = None

    @staticmethod
    def new(ctx, r1cs, z, l_in, b, k, A=None):
        if A is not None:
            ctx.set_matrix(A)
        f = gadget_decompose(z, b, k)
        return ComR1CS(tuple(r1cs), np.asarray(z, dtype=np.uint64), f, ctx.commit(f), l_in)

    @staticmethod
    def new_resident(ctx, r1cs, z, l_in, b, k):
        """ComR1CS::new with f cut and committed on the device (PlusContext.witness_from_z): only z crosses PCIe, f stays in `ctx` and is not downloaded
        (fetch_f reads it back)"""
        if not api.is_device_array(z):      # (a device z goes through as it is: lfplus_witness_from_z_dev reads it in place)
            z = np.ascontiguousarray(z, dtype=np.uint64)
        return ComR1CS(tuple(r1cs), z, None, ctx.witness_from_z(z, b, k), l_in, ctx)

    def fetch_f(self):
        """f as a host array: of a resident instance, read back from its context (which must still hold it)"""
        return self.f if self.f is not None else self.ctx.get_witness()

    def matrices(self):
        return list(self.r1cs)

    def check_relation(self, ctx, bound=0, resident=False):
        """Is this instance in R_ComR1CS (r1cs.rs:21-60)?  cm_f = A f for the matrix resident in `ctx`, (M_A f) o (M_B f) = M_C f, ||f||_inf < bound (0: not
        checked), all on the device (PlusContext.r1cs_check) -> (ok, failed, first_bad, absmax).  A host instance uploads its f into `ctx` (it becomes the
        resident witness there); a resident instance is checked in the context that holds its witness, which is not touched.  resident: the three matrices are
        the ones ctx.set_matrices / share_matrices left on the device"""
        if self.f is None:
            if ctx is not self.ctx:
                raise LfPlusError(E_ARG, "ComR1CS.check_relation: a resident instance is checked in the context that holds its witness")
        else:
            ctx.set_witness(self.f)
        return ctx.r1cs_check(self.cm_f, RESIDENT(3) if resident else self.r1cs, bound)

    def linearize(self, ctx, transcript, resident=False, preloaded=False, from_f_hint=None):
        """Linearize::linearize (r1cs.rs:76-139) on `ctx` (the witness becomes resident there) -> (LinB fields, ComR1CSProof fields); resident: the three
        matrices are the ones ctx.set_matrices / share_matrices left on the device; preloaded: ctx.set_witness(self.f) was already called (PlusProver.preload);
        from_f_hint: DecompParameters of the Mlin::mlin that follows -- the double commitment of this witness is enqueued on the context's second stream now
        (lfplus_rg_from_f_async) and runs next to the sumcheck rounds"""
        if self.f is None:
            if ctx is not self.ctx:
                raise LfPlusError(E_ARG, "ComR1CS.linearize: a resident instance is linearized in the context that holds its witness")
        elif not preloaded:
            ctx.set_witness(self.f)
        if from_f_hint is not None:
            ctx.rg_from_f_async(from_f_hint)
        n = ctx.n if self.f is None else self.f.shape[0]
        nvars = n.bit_length() - 1
        keep, rp, cp, vp = _csr_args(RESIDENT(3) if resident else self.r1cs)
        msgs, ro, ev = np.zeros((nvars, 4, D), dtype=np.uint64), np.zeros(nvars, dtype=np.uint64), np.zeros((4, D), dtype=np.uint64)
        ctx._chk(_lib().lfplus_r1cs_linearize(ctx.h, transcript.h, rp, cp, vp, *[x.ctypes.data_as(u64p) for x in (msgs, ro, ev)]))
        proof = {"msgs": msgs, "nvars": nvars, "r": ro, "evals": ev}
        linb = {"f": self.f, "cm_f": self.cm_f, "r": ro, "v": ev}
        return linb, proof


def r1cs_verify(transcript, proof, nvars=None):
    """ComR1CSProof::verify (r1cs.rs:141-162), host -> (accepted, stage, ro).  nvars: the VERIFIER's log2 n (None: the proof's own field, as the reference reads
    `self.nvars` -- the arrays are checked against it either way)"""
    nvars = _nvars_ok(proof["nvars"] if nvars is None else nvars)
    msgs, ev = _shaped(proof, "msgs", (nvars, 4, D)), _shaped(proof, "evals", (4, D))
    ro, st = np.zeros(nvars, dtype=np.uint64), C.c_int()
    rc = _lib().lfplus_r1cs_verify(transcript.h, nvars, msgs.ctypes.data_as(u64p), ev.ctypes.data_as(u64p), ro.ctypes.data_as(u64p), C.byref(st))
    if rc not in (0, E_REJECT):
        raise LfPlusError(rc, "lfplus_r1cs_verify")
    return rc == 0, st.value, ro


# ---- committed CCS instances (lfplus_ccs_*; the reference has none: self-consistent, pinned to the reference at the R1CS shape) ---------------------------
class CCSShape:
    """A CCS shape over t matrices: sum_i c_i * prod_{j in S_i} (M_j f) = 0 row by row.  multisets: q sequences of matrix indices (an index may repeat inside
    one and across them); coeffs: q ring elements (16 canonical words) or Python integers (constant polynomials, reduced mod p).  The envelope (1 <= t, q <= 8,
    1 <= |S_i| <= 7, at most 16 indices in all, indices < t) is the library's to refuse: desc() passes anything that can be written down."""

    def __init__(self, t, multisets, coeffs):
        self.t = int(t)
        self.multisets = [[int(j) for j in S] for S in multisets]
        if len(coeffs) != len(self.multisets):
            raise LfPlusError(E_ARG, "CCSShape: one coefficient per multiset")
        self.coeffs = np.zeros((max(len(self.multisets), 1), D), dtype=np.uint64)
        for i, c in enumerate(coeffs):
            if isinstance(c, (int, np.integer)):
                self.coeffs[i, 0] = int(c) % P
            else:
                self.coeffs[i] = np.asarray(c, dtype=np.uint64).reshape(D)

    @staticmethod
    def r1cs():
        """(M_0 f) o (M_1 f) - M_2 f: the shape lfplus_r1cs_linearize hard-wires"""
        return CCSShape(3, [[0, 1], [2]], [1, -1])

    @property
    def q(self):
        return len(self.multisets)

    @property
    def degree(self):
        """d = max |S_i| (the sumcheck runs at degree d + 1 and sends d + 2 evaluations per round)"""
        return max((len(S) for S in self.multisets), default=0)

    def desc(self):
        """the lfplus_ccs of this shape (the arrays it points to stay alive with the returned object)"""
        off = np.zeros(self.q + 1, dtype=np.uint32)
        idx = []
        for i, S in enumerate(self.multisets):
            idx += S
            off[i + 1] = len(idx)
        idx = np.asarray(idx + [0], dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        d = CCSDesc(self.t, self.q, off.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), self.coeffs.ctypes.data_as(u64p))
        d._keep = (off, idx, self.coeffs)
        return d


@dataclass
class ComCCS:
    """A committed CCS instance, mirroring ComR1CS: shape, its t CSR matrices (n x n), the witness f (n ring elements; None: resident in `ctx`) and cm_f = A f"""
    shape: CCSShape
    mats: tuple
    f: np.ndarray
    cm_f: np.ndarray
    ctx: object = None

    @staticmethod
    def new(ctx, shape, mats, f, A=None):
        if A is not None:
            ctx.set_matrix(A)
        if len(mats) != shape.t:
            raise LfPlusError(E_ARG, f"ComCCS: the shape has {shape.t} matrices")
        f = np.ascontiguousarray(f, dtype=np.uint64)
        return ComCCS(shape, tuple(mats), f, ctx.commit(f))

    @staticmethod
    def new_resident(ctx, shape, mats, z, b, k):
        """ComCCS.new with f = z.gadget_decompose(b, k) cut and committed on the device (PlusContext.witness_from_z), as ComR1CS.new_resident: f stays in `ctx`"""
        if len(mats) != shape.t:
            raise LfPlusError(E_ARG, f"ComCCS: the shape has {shape.t} matrices")
        if not api.is_device_array(z):
            z = np.ascontiguousarray(z, dtype=np.uint64)
        return ComCCS(shape, tuple(mats), None, ctx.witness_from_z(z, b, k), ctx)

    def fetch_f(self):
        """f as a host array: of a resident instance, read back from its context (which must still hold it)"""
        return self.f if self.f is not None else self.ctx.get_witness()

    def matrices(self):
        return list(self.mats)

    def check_relation(self, ctx, bound=0, resident=False):
        """Is the instance satisfied?  PlusContext.ccs_check on `ctx` -> (ok, failed, first_bad, absmax).  A host instance uploads its f into `ctx`; a resident
        one is checked in the context that holds its witness.  resident: the matrices are the ones ctx.set_matrices / share_matrices left on the device"""
        if self.f is None:
            if ctx is not self.ctx:
                raise LfPlusError(E_ARG, "ComCCS.check_relation: a resident instance is checked in the context that holds its witness")
        else:
            ctx.set_witness(self.f)
        return ctx.ccs_check(self.cm_f, self.shape, None if resident else self.mats, bound)

    def linearize(self, ctx, transcript, resident=False, preloaded=False, from_f_hint=None):
        """lfplus_ccs_linearize on `ctx` (the witness becomes resident there) -> (LinB fields, proof fields): msgs (nvars, d + 2, 16), r = ro (nvars), evals
        (1 + t, 16).  The LinB goes into mlin / decompose with the shape's t matrices.  resident / preloaded / from_f_hint as ComR1CS.linearize"""
        if self.f is None:
            if ctx is not self.ctx:
                raise LfPlusError(E_ARG, "ComCCS.linearize: a resident instance is linearized in the context that holds its witness")
        elif not preloaded:
            ctx.set_witness(self.f)
        if from_f_hint is not None:
            ctx.rg_from_f_async(from_f_hint)
        n = ctx.n if self.f is None else self.f.shape[0]
        nvars = max(int(n).bit_length() - 1, 0)
        t, d = self.shape.t, self.shape.degree
        keep, rp, cp, vp = _csr_args(RESIDENT(t) if resident else self.mats)
        if not resident and len(self.mats) != t:
            raise LfPlusError(E_ARG, f"ComCCS.linearize: the shape has {t} matrices")
        msgs, ro, ev = np.zeros((nvars, d + 2, D), dtype=np.uint64), np.zeros(max(nvars, 1), dtype=np.uint64), np.zeros((1 + max(t, 0), D), dtype=np.uint64)
        desc = self.shape.desc()
        ctx._chk(_lib().lfplus_ccs_linearize(ctx.h, transcript.h, C.byref(desc), rp, cp, vp, *[x.ctypes.data_as(u64p) for x in (msgs, ro, ev)]))
        ro = ro[:nvars]
        proof = {"msgs": msgs, "nvars": nvars, "r": ro, "evals": ev}
        linb = {"f": self.f, "cm_f": self.cm_f, "r": ro, "v": ev}
        return linb, proof


def ccs_verify(transcript, shape, proof, nvars=None):
    """The verifier of ComCCS.linearize's proofs (lfplus_ccs_verify), host -> (accepted, stage, ro): stage 1 = a sumcheck round, 2 = the final identity.  nvars:
    the VERIFIER's log2 n (None: the proof's own field); the arrays are checked against it and against the shape either way"""
    if not isinstance(shape, CCSShape):
        raise LfPlusError(E_ARG, "ccs_verify: shape must be a CCSShape")
    nvars = _nvars_ok(proof["nvars"] if nvars is None else nvars)
    if not 1 <= shape.t <= 8 or not 1 <= shape.q <= 8 or not 1 <= shape.degree <= 7:      # (the arrays' shapes follow from these: nothing to check them against)
        raise LfPlusError(E_ARG, "ccs_verify: shape outside the envelope (1 <= t, q <= 8, 1 <= |S_i| <= 7)")
    msgs, ev = _shaped(proof, "msgs", (nvars, shape.degree + 2, D)), _shaped(proof, "evals", (1 + shape.t, D))
    ro, st = np.zeros(nvars, dtype=np.uint64), C.c_int()
    d = shape.desc()
    rc = _lib().lfplus_ccs_verify(transcript.h, nvars, C.byref(d), msgs.ctypes.data_as(u64p), ev.ctypes.data_as(u64p), ro.ctypes.data_as(u64p), C.byref(st))
    if rc not in (0, E_REJECT):
        raise LfPlusError(rc, "lfplus_ccs_verify")
    return rc == 0, st.value, ro


def decomp_verify(dproof, cm_f, v, B, kappa=None, nM=None):
    """DecompProof::verify (decomp.rs:101-123), host -> (accepted, stage).  kappa / nM: the verifier's (None: the shape of cm_f / v); all six arrays must agree"""
    cm_f, v = np.ascontiguousarray(cm_f, dtype=np.uint64), np.ascontiguousarray(v, dtype=np.uint64)
    kappa = int(cm_f.shape[0] if kappa is None and cm_f.ndim == 2 else (kappa or 0))
    count = int(v.shape[0] if nM is None and v.ndim == 3 else 1 + (nM or 0))
    if kappa < 1 or cm_f.shape != (kappa, D) or v.shape != (count, 2, D):
        raise LfPlusError(E_ARG, "decomp_verify: cm_f must be (kappa, 16) and v (1 + nM, 2, 16)")
    arr = [_shaped(dproof, "C0", (kappa, D)), _shaped(dproof, "C1", (kappa, D)), _shaped(dproof, "v0", (count, 2, D)), _shaped(dproof, "v1", (count, 2, D)), cm_f, v]
    st = C.c_int()
    rc = _lib().lfplus_decomp_verify(arr[0].ctypes.data_as(u64p), arr[1].ctypes.data_as(u64p), arr[0].shape[0], arr[2].ctypes.data_as(u64p),
                                     arr[3].ctypes.data_as(u64p), arr[2].shape[0], arr[4].ctypes.data_as(u64p), arr[5].ctypes.data_as(u64p), B, C.byref(st))
    if rc not in (0, E_REJECT):
        raise LfPlusError(rc, "lfplus_decomp_verify")
    return rc == 0, st.value


# ---- MLSumcheck over any sum of products of MLE tables (latticefold utils/sumcheck.rs:53-104; lfplus_mlsumcheck_*) --------------------------------------
class VPoly:
    """VirtualPolynomial (utils/sumcheck/utils.rs:24-75) over a flat list of MLE tables: g = sum_i coef_i * prod_{j in indices_i} T_j.
    terms: [(coef, [indices])], coef a ring element (16 canonical words) or a Python integer (the constant polynomial); an index may repeat inside a term and
    across terms.  degree: what the prover sends degree + 1 evaluations for (default: the widest term)."""

    def __init__(self, terms, degree=None):
        self.terms = [(c, [int(j) for j in idx]) for c, idx in terms]
        self.degree = max((len(idx) for _, idx in self.terms), default=0) if degree is None else int(degree)

    def desc(self, nvars, ntables):
        """the lfplus_vpoly of this polynomial (the arrays it points to stay alive with the returned object)"""
        off = np.zeros(len(self.terms) + 1, dtype=np.uint32)
        coef = np.zeros((max(len(self.terms), 1), D), dtype=np.uint64)
        idx = []
        for i, (c, ix) in enumerate(self.terms):
            idx += ix
            off[i + 1] = len(idx)
            if isinstance(c, (int, np.integer)):
                coef[i, 0] = int(c) % P
            else:
                coef[i] = np.asarray(c, dtype=np.uint64).reshape(D)
        idx = np.asarray(idx + [0], dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        d = VPolyDesc(int(nvars), int(ntables), len(self.terms), self.degree, off.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), coef.ctypes.data_as(u64p))
        d._keep = (off, idx, coef)
        return d


def _mls_tables(ctx, tables):
    """tables (T, 2^nvars, 16): a host array, or a device array on the context's device (read by the _dev calls) -> (T, nvars, pointer, is_device, keep-alive)"""
    sh = tuple(tables.shape)
    if len(sh) != 3 or sh[2] != D or sh[1] < 2 or sh[1] & (sh[1] - 1):
        raise LfPlusError(E_ARG, "tables: (T, 2^nvars, 16)")
    if api.is_device_array(tables):
        if not tables.is_contiguous() or tables.element_size() != 8:
            raise LfPlusError(E_ARG, "device tables must be contiguous with 8-byte elements")
        ctx.wait_stream()
        return sh[0], sh[1].bit_length() - 1, C.c_void_p(tables.data_ptr()), True, tables
    a, p = _w(tables)
    return sh[0], sh[1].bit_length() - 1, p, False, a


class MLSumcheck:
    """The split form of MLSumcheck::prove_as_subprotocol over any VPoly (lfplus_mlsumcheck_begin / _round / _final / _end), on a bare context or a loaded one:
    prove_round / final / end with the caller's transcript in between.  tables: (T, 2^nvars, 16) canonical words, a numpy array or a device array"""

    def __init__(self, ctx, tables, vpoly):
        self.ctx, self.degree = ctx, vpoly.degree
        self.ntables, self.nvars, p, dev, keep = _mls_tables(ctx, tables)
        d = vpoly.desc(self.nvars, self.ntables)
        ctx._chk((_lib().lfplus_mlsumcheck_begin_device if dev else _lib().lfplus_mlsumcheck_begin)(ctx.h, C.byref(d), p))

    def prove_round(self, r_prev=None):
        """round messages in order: r_prev = None in round 1, the previous challenge (one word) afterwards -> (degree + 1, 16)"""
        o = np.zeros((self.degree + 1, D), dtype=np.uint64)
        r = None if r_prev is None else C.byref(C.c_uint64(int(r_prev)))
        self.ctx._chk(_lib().lfplus_mlsumcheck_round(self.ctx.h, r, o.ctypes.data_as(u64p)))
        return o

    def final(self, r_last):
        """after the last round: every table's value at the whole point, (T, 16)"""
        o = np.zeros((self.ntables, D), dtype=np.uint64)
        r = C.c_uint64(int(r_last))
        self.ctx._chk(_lib().lfplus_mlsumcheck_final(self.ctx.h, C.byref(r), o.ctypes.data_as(u64p)))
        return o

    def end(self):
        self.ctx._chk(_lib().lfplus_mlsumcheck_end(self.ctx.h))


def mlsumcheck_prove(ctx, transcript, tables, vpoly):
    """prove_as_subprotocol in one call (lfplus_mlsumcheck_prove; a device array is read in place by lfplus_mlsumcheck_prove_device) ->
    (msgs (nvars, degree + 1, 16), point (nvars,), final (T, 16): the tables' values at the point)"""
    T, nv, p, dev, keep = _mls_tables(ctx, tables)
    d = vpoly.desc(nv, T)
    msgs, point, fin = np.zeros((nv, vpoly.degree + 1, D), dtype=np.uint64), np.zeros(nv, dtype=np.uint64), np.zeros((T, D), dtype=np.uint64)
    f = _lib().lfplus_mlsumcheck_prove_device if dev else _lib().lfplus_mlsumcheck_prove
    ctx._chk(f(ctx.h, transcript.h, C.byref(d), p, msgs.ctypes.data_as(u64p), point.ctypes.data_as(u64p), fin.ctypes.data_as(u64p)))
    return msgs, point, fin


def mlsumcheck_verify(transcript, nvars, degree, claimed_sum, msgs):
    """verify_as_subprotocol on the host (lfplus_mlsumcheck_verify: no GPU, no context) -> (ok, point (nvars,), expected): expected is the subclaim's ring
    element g(point), or the index of the first failing round when ok is False"""
    if not isinstance(nvars, (int, np.integer)) or not isinstance(degree, (int, np.integer)) or not 1 <= int(nvars) <= 28 or not 1 <= int(degree) <= 8:
        raise LfPlusError(E_ARG, "mlsumcheck_verify: nvars outside [1, 28] or degree outside [1, 8]")
    cs, pc = _w(claimed_sum)
    m = _shaped({"msgs": msgs}, "msgs", (int(nvars), int(degree) + 1, D))
    if cs.shape != (D,):
        raise LfPlusError(E_ARG, "mlsumcheck_verify: claimed_sum is one ring element")
    point, exp, rnd = np.zeros(int(nvars), dtype=np.uint64), np.zeros(D, dtype=np.uint64), C.c_int(-1)
    rc = _lib().lfplus_mlsumcheck_verify(transcript.h, int(nvars), int(degree), pc, m.ctypes.data_as(u64p), point.ctypes.data_as(u64p), exp.ctypes.data_as(u64p),
                                         C.byref(rnd))
    if rc not in (0, E_REJECT):
        raise LfPlusError(rc, "lfplus_mlsumcheck_verify")
    return rc == 0, point, (exp if rc == 0 else rnd.value)


def mlsumcheck_extract_sum(msgs):
    """MLSumcheck::extract_sum (utils/sumcheck.rs:46-48): the claimed sum a proof is about, p_1(0) + p_1(1)"""
    m = np.asarray(msgs, dtype=np.uint64).reshape(-1, D)
    return ((m[0].astype(object) + m[1].astype(object)) % P).astype(np.uint64)


def mlin(ctxs, transcript, params, M=()):
    """Mlin{lins, params}.mlin(&A, &M, transcript) (mlin.rs:42-107) over the resident witnesses of ctxs -> (LinB2X fields, CmProof fields).  The folded
    witness g stays on the device as ctxs[0]'s resident witness."""
    L, nM, c0 = len(ctxs), len(M), ctxs[0]
    n, k, kappa, dp = c0.n, params.decomp.k, c0.kappa, params.decomp
    nvars = n.bit_length() - 1
    per = 4 + 4 * nM
    keep, rp, cp, vp = _csr_args(M)
    hs = (C.c_void_p * L)(*[c.h for c in ctxs])
    z = lambda *shape: np.zeros(shape, dtype=np.uint64)
    o = {"r": z(nvars), "msgs": z(nvars, 4, D), "e": z(1 + nM, L * k, D, D), "b": z(L, D), "v": z(L, D), "a": z(L, 1 + nM), "bb": z(L, 1 + nM, D),
         "c": z(L, 1 + nM, D), "comh": z(L, kappa, D), "pa": z(nvars, 3, D), "pb": z(nvars, 3, D), "ea": z(L, per, D), "eb": z(L, per, D),
         "cm_g": z(L, kappa, D), "ro": z(2, nvars), "vo": z(L, 1 + nM, 2, D), "fcoms": z(L, 3, kappa, D)}
    x = {"cm_g": z(kappa, D), "vo": z(1 + nM, 2, D)}
    keys = ("r", "msgs", "e", "b", "v", "a", "bb", "c", "comh", "pa", "pb", "ea", "eb", "cm_g", "ro", "vo", "fcoms")
    c0._chk(_lib().lfplus_mlin(hs, L, transcript.h, dp.b, dp.k, dp.l, nM, rp, cp, vp, *[o[key].ctypes.data_as(u64p) for key in keys],
                               x["cm_g"].ctypes.data_as(u64p), x["vo"].ctypes.data_as(u64p)))
    for c in ctxs:
        c._k = k
    o.update(k=k, ell=dp.l, kappa=kappa, nvars=nvars)
    x["ro"] = o["ro"]
    return x, o


def _ro_pairs(ro):
    """ComX.ro: Vec<(R, R)> -- the two sumcheck points as pairs of ring constants, (nvars, 2, 16)"""
    out = np.zeros((ro.shape[1], 2, D), dtype=np.uint64)
    out[:, 0, 0], out[:, 1, 0] = ro[0], ro[1]
    return out


class PlusProver:
    """plus.rs:15-108.  One context per instance (2 accumulated + ncomp fresh); all share the Ajtai matrix of the first."""

    def __init__(self, A, M, ncomp, params, transcript, device=0, shard=None, shape=None):
        """shape: a CCSShape over the t = len(M) matrices -- the prover folds ComCCS instances (lfplus_ccs_linearize in place of lfplus_r1cs_linearize; unsharded
        only).  shard = (rank, world, transport): a prover column-sharded over `world` ranks, one GPU each -- A is then the rank's column slice (kappa, n / world,
        16); transport is an allgather callable (host transport: PlusContext.set_sharding) or the bytes of an ncclUniqueId (RCCL: PlusContext.dist_init).
        Every rank makes the same calls with the same (whole) witnesses and gets the same proof."""
        self.M, self.params, self.transcript, self.shape = list(M), params, transcript, shape
        if shape is not None:      # (before a context exists)
            if not isinstance(shape, CCSShape) or shape.t != len(self.M):
                raise LfPlusError(E_ARG, "PlusProver: shape must be a CCSShape over len(M) matrices")
            if shard is not None:
                raise LfPlusError(E_ARG, "PlusProver: a CCS prover is unsharded only (lfplus_ccs_linearize refuses sharded contexts)")
        self.device = device
        self.ctxs = [PlusContext(device) for _ in range(2 + ncomp)]
        if shard is not None:
            rank, world, transport = shard
            if transport == "model":
                self.ctxs[0].set_sharding_model(rank, world)
            elif callable(transport):
                self.ctxs[0].set_sharding(rank, world, transport)
            else:
                self.ctxs[0].dist_init(rank, world, transport)
        self.ctxs[0].set_matrix(A)
        self.ctxs[0].set_matrices(self.M)
        for c in self.ctxs[1:]:
            c.share_matrix(self.ctxs[0])
            c.share_matrices(self.ctxs[0])
        self.res = RESIDENT(len(self.M))
        self.acc = []          # the accumulated LinB witnesses: host copies of F0, F1 -- or, with device_acc, the markers "ctx0" / "ctx1" (they live in ctxs[0] / ctxs[1])
        self.device_acc = False   # True: the accumulator never leaves the device between proves (lfplus_decompose_resident); accumulator() reads it back
        self._preloaded = None
        self.failed = None     # set when a prove() raised half way: the Fiat-Shamir transcript has advanced and the contexts hold a half-folded state

    @staticmethod
    def init(A, M, ncomp, params, transcript, device=0, shard=None, shape=None):
        return PlusProver(A, M, ncomp, params, transcript, device, shard, shape)

    def close(self):
        for c in reversed(self.ctxs):
            c.close()
        self.ctxs = []

    def preload(self, comp):
        """upload the witnesses of the instances the next prove(comp) will fold into their contexts now (a pipeline has them on the device already: the timed region
        of bench.py starts after this, as the contract's "inputs resident in HBM" asks)"""
        nacc = len(self.acc)
        if nacc + len(comp) > len(self.ctxs):
            raise LfPlusError(E_ARG, "PlusProver.preload: more instances than contexts (ncomp)")
        for i, ci in enumerate(comp):
            self.ctxs[nacc + i].set_witness(ci.f)
        self._preloaded = [ci.f for ci in comp]

    def ingest(self, zs, r1cs=None, l_in=1):
        """The fresh instances of the next prove, built in the contexts that prove will use (ComR1CS.new_resident in ctxs[nacc + i]: z is uploaded, cut into
        f = z.gadget_decompose(B, k) and committed on the device) -> the ComR1CS list; prove(comps) then neither uploads nor reads a host f.  Not for a sharded
        prover.  A CCS prover (shape=) builds resident ComCCS over its own matrices (r1cs: not used).  A prover whose ingest raised is failed, as one whose prove raised (a context may be left without its witness)."""
        if self.failed is not None:
            raise LfPlusError(E_ARG, f"PlusProver.ingest: this prover failed earlier ({self.failed}) -- build a new prover")
        nacc = len(self.acc)
        if nacc + len(zs) > len(self.ctxs):
            raise LfPlusError(E_ARG, "PlusProver.ingest: more instances than contexts (ncomp)")
        try:
            if self.shape is not None:
                comps = [ComCCS.new_resident(self.ctxs[nacc + i], self.shape, self.M, z, self.params.B, self.params.lin.decomp.k) for i, z in enumerate(zs)]
            else:
                comps = [ComR1CS.new_resident(self.ctxs[nacc + i], r1cs, z, l_in, self.params.B, self.params.lin.decomp.k) for i, z in enumerate(zs)]
        except Exception as ex:
            self.failed = repr(ex)
            raise
        self._preloaded = list(comps)
        return comps

    def accumulator(self):
        """(F0, F1) of the last prove as host arrays"""
        if self.device_acc and self.acc:
            return self.ctxs[0].get_witness(), self.ctxs[1].get_witness()
        return tuple(self.acc)

    def decide(self, proof, bound=0):
        """Are the two halves of the accumulator this prover holds after prove() -> proof valid LinB instances (lin.rs:29-40)?  Half i = (F_i, C_i, v_i) at the
        points linb2x.ro: C_i = A F_i, v_i = the evaluations of F_i and M_j F_i at both points, ||F_i||_inf < bound (0: not checked) -- PlusContext.linb_check
        on the device.  With device_acc the halves are checked where they live (ctxs[0] / ctxs[1]) and nothing moves; a host accumulator is uploaded into
        scratch contexts.  -> [(ok, failed, absmax)] per half.  Read-only: the prover, its transcript and its accumulator are as before the call."""
        if self.failed is not None or len(self.acc) != 2:
            raise LfPlusError(E_ARG, "PlusProver.decide: no accumulator (call it after a successful prove)")
        r, dproof, out = _ro_pairs(np.asarray(proof["linb2x"]["ro"], dtype=np.uint64)), proof["dproof"], []
        for i in range(2):
            if self.device_acc:
                out.append(self.ctxs[i].linb_check(dproof[f"C{i}"], r, dproof[f"v{i}"], self.res, bound))
                continue
            cx = PlusContext(self.device)
            try:
                cx.share_matrix(self.ctxs[0])
                cx.share_matrices(self.ctxs[0])
                cx.set_witness(self.acc[i])
                out.append(cx.linb_check(dproof[f"C{i}"], r, dproof[f"v{i}"], self.res, bound))
            finally:
                cx.close()
        return out

    def prove(self, comp):
        """PlusProver::prove (plus.rs:77-108) -> PlusProof fields: linb2x, lproof, cmproof, dproof"""
        if self.failed is not None:
            raise LfPlusError(E_ARG, f"PlusProver.prove: this prover failed in an earlier prove() ({self.failed}); its transcript and accumulator are half-advanced -- "
                                     "build a new prover")
        nacc = len(self.acc)
        if nacc + len(comp) > len(self.ctxs):
            raise LfPlusError(E_ARG, "PlusProver.prove: more instances than contexts (ncomp)")
        if any((self.shape is not None) != isinstance(ci, ComCCS) for ci in comp):      # (a shape error: nothing is touched)
            raise LfPlusError(E_ARG, "PlusProver.prove: a CCS prover (shape=) folds ComCCS instances, any other prover ComR1CS")
        try:
            return self._prove(comp, nacc)
        except Exception as ex:      # the reference's prove() panics on these paths; here the object survives, so it must refuse to continue from this state
            self.failed = repr(ex)
            raise

    def _prove(self, comp, nacc):
        ctxs = self.ctxs[:nacc + len(comp)]
        lproof = []
        # preloaded: by preload (the same host arrays) or by ingest (the same resident instances, each in the context it is folded from)
        pre = self._preloaded is not None and len(self._preloaded) == len(comp) and all(
            (a is ci and ci.ctx is self.ctxs[nacc + i]) if ci.f is None else a is ci.f for i, (a, ci) in enumerate(zip(self._preloaded, comp)))
        self._preloaded = None
        if not pre and any(ci.f is None for ci in comp):
            raise LfPlusError(E_ARG, "PlusProver.prove: resident instances must come from this prover's last ingest, in its order")
        # RgInstance::from_f of every instance (Mlin::mlin, mlin.rs:52-60) needs no challenge: each is enqueued on its context's second stream as soon as the
        # witness is resident and runs next to the linearizations' latency-bound rounds; lfplus_mlin collects the results
        dp = self.params.lin.decomp
        # Witnesses that are still on the host (the accumulator of a prover without device_acc, fresh instances that were not preloaded) cross PCIe on a worker
        # thread, one after the other, while this thread linearizes the instances that have arrived (an upload is 2.4 ms per 2^20-row witness, a linearization
        # 2.3 ms): only the first upload is exposed.  Sharded provers upload in line (their contexts exchange from this thread).
        ups = [(ctxs[i], f) for i, f in enumerate(self.acc) if not isinstance(f, str)]      # (device_acc: F0 / F1 of the last prove are resident in ctxs[0] / ctxs[1] already)
        if not pre:
            ups += [(ctxs[nacc + i], ci.f) for i, ci in enumerate(comp)]
        arrived, up_err, outs = {}, [], []
        want_outs = not self.device_acc      # (F0, F1) come back to the host: their buffers are allocated AND touched by the worker while the GPU works
        if (ups or want_outs) and self.ctxs[0].shard[1] == 1 and not os.environ.get("LFPLUS_SERIAL_UPLOADS"):
            import threading
            for cx, _ in ups:
                arrived[id(cx)] = threading.Event()

            def _upload():
                try:
                    for cx, f in ups:
                        cx.set_witness(f)
                        arrived[id(cx)].set()
                    if want_outs:
                        outs.extend(np.zeros((ctxs[0].n, D), dtype=np.uint64) for _ in range(2))
                        for b in outs:
                            b[::32, 0] = 0           # one word per 4 KiB page (32 rows of 128 bytes): the pages exist before the download needs them
                        outs_ready.set()
                except Exception as ex:      # (reported by the thread that waits for the witness)
                    up_err.append(ex)
                    for ev in arrived.values():
                        ev.set()
            outs_ready = threading.Event()
            th = threading.Thread(target=_upload, daemon=True)
            th.start()
        else:
            th = None
            for cx, f in ups:
                cx.set_witness(f)

        def _wait(cx):
            ev = arrived.get(id(cx))
            if ev is not None:
                ev.wait()
                if up_err:
                    raise up_err[0]
        try:
            for i in range(nacc):
                _wait(ctxs[i])
                ctxs[i].rg_from_f_async(dp)
            for i, ci in enumerate(comp):
                mats = ci.mats if self.shape is not None else ci.r1cs
                same = len(self.M) == (3 if self.shape is None else self.shape.t) and all(a is b for x, y in zip(mats, self.M) for a, b in zip(x, y))   # (M = cr1cs.x.matrices() in every reference use)
                _wait(ctxs[nacc + i])
                _, lp = ci.linearize(ctxs[nacc + i], self.transcript, resident=same, preloaded=True, from_f_hint=dp)
                lproof.append(lp)
        except Exception:
            if th is not None:               # (never leave the worker writing into contexts the caller is about to close)
                th.join()
            raise
        linb2x, cmproof = mlin(ctxs, self.transcript, self.params.lin, self.res)
        if self.device_acc:
            dec = ctxs[0].decompose(None, None, self.params.B, _ro_pairs(linb2x["ro"]), self.res, into=(self.ctxs[0], self.ctxs[1]))
            self.acc = ["ctx0", "ctx1"]
        else:
            if th is not None:
                th.join()
                if up_err:
                    raise up_err[0]
            dec = ctxs[0].decompose(None, None, self.params.B, _ro_pairs(linb2x["ro"]), self.res, out_bufs=tuple(outs) if len(outs) == 2 else None)
            self.acc = [dec["F0"], dec["F1"]]
        dproof = {key: dec[key] for key in ("C0", "C1", "v0", "v1")}
        return {"linb2x": linb2x, "lproof": lproof, "cmproof": cmproof, "dproof": dproof}


class PlusVerifier:
    """plus.rs:25-33, 110-146 (host only).  verify returns True, or False with .stage = (which proof, stage) -- the reference panics there"""

    def __init__(self, A, M, params, transcript, shape=None):
        self.M, self.params, self.transcript, self.shape = list(M), params, transcript, shape
        if shape is not None and (not isinstance(shape, CCSShape) or shape.t != len(self.M)):
            raise LfPlusError(E_ARG, "PlusVerifier: shape must be a CCSShape over len(M) matrices")
        self.stage = None
        # the verifier's OWN shape parameters (plus.rs:110-146 passes &self.A, &self.M down; CmProof::verify sizes everything from them, cm.rs:349-365):
        # nothing below is taken from the proof
        A = np.asarray(A)
        if A.ndim != 3 or A.shape[2] != D or A.shape[0] != params.lin.kappa or A.shape[1] < 2 or A.shape[1] & (A.shape[1] - 1):
            raise LfPlusError(E_ARG, "PlusVerifier: A must be (kappa, n = 2^nvars, 16) with kappa = params.lin.kappa")
        self.kappa, self.n = int(A.shape[0]), int(A.shape[1])
        self.nvars = self.n.bit_length() - 1

    @staticmethod
    def init(A, M, params, transcript, shape=None):
        return PlusVerifier(A, M, params, transcript, shape)

    def verify(self, proof):
        """False with .stage = (which proof, stage); a proof whose arrays do not have the shapes this verifier's parameters imply is rejected as
        ("malformed", message) before any C verifier reads it"""
        dp, nM = self.params.lin.decomp, len(self.M)
        try:
            for i, lp in enumerate(proof["lproof"]):
                if self.shape is not None:
                    ok, st, _ = ccs_verify(self.transcript, self.shape, lp, nvars=self.nvars)
                else:
                    ok, st, _ = r1cs_verify(self.transcript, lp, nvars=self.nvars)
                if not ok:
                    self.stage = (f"lproof[{i}]", st)
                    return False
            cm = proof["cmproof"]
            L = int(np.asarray(cm["b"]).shape[0])      # the number of folded instances is the statement's (the reference: self.lins.len()); every array must agree with it
            fcoms = np.ascontiguousarray(cm["fcoms"], dtype=np.uint64)
            if fcoms.shape != (L, 3, self.kappa, D):
                raise LfPlusError(E_ARG, "malformed proof: fcoms")
            ok, st, _ = cm_verify(self.transcript, cm, list(fcoms), nvars=self.nvars, L=L, k=dp.k, ell=dp.l, kappa=self.kappa, nM=nM)
            if not ok:
                self.stage = ("cmproof", st)
                return False
            ok, st = decomp_verify(proof["dproof"], proof["linb2x"]["cm_g"], proof["linb2x"]["vo"], self.params.B, kappa=self.kappa, nM=nM)
            if not ok:
                self.stage = ("dproof", st)
                return False
        except LfPlusError as ex:
            if ex.code != E_ARG:
                raise
            self.stage = ("malformed", str(ex))
            return False
        except (KeyError, TypeError, IndexError) as ex:
            self.stage = ("malformed", repr(ex))
            return False
        self.stage = None
        return True


# ---- deterministic synthetic workloads (numpy only: no oracle, no GPU) -----------------------------------------------------------------------
# The shape of the reference's end-to-end bench (benches/e2e.rs:57-100: `setup_input(n, L, k, kappa)`: decomposed-square R1CS over identity matrices,
# BinaryChoice witness, L fresh instances folded by one PlusProver::prove, B = estimate_bound(d * 128, L, d, k) / 2, l = ceil(log_{d/2} q)).
# Differences, deliberate: the L instances are distinct (the bench clones one), the Ajtai matrix is i.i.d. from an indexable SplitMix64 stream.
PLUS_CONFIGS = {
    # name: (nvars, L, k, kappa)
    "P12": (12, 2, 2, 1),        # tiny: unit tests of the sharded path (kappa k d l d = 11264 > n: from_f refuses it -- used with k = 1 shapes only)
    "P15": (15, 3, 4, 1),        # kappa 1 keeps tau inside n = 2^15 (kappa k d l d = 22528)
    "P16": (16, 3, 4, 2),        # benches/utils/mod.rs:282-301 PROTOCOL_SCALING[1] = (65536, 3, 4, 2)
    "P17": (17, 3, 4, 2),        # PROTOCOL_SCALING[2] = (131072, 3, 4, 2): the reference's largest e2e row
    "P20": (20, 3, 4, 2),        # BASELINE configs[4]: 2^20 rows (the same row extrapolated)
}


def estimate_bound(sop, L, d, k):
    """utils::estimate_bound (utils.rs:102-112)"""
    a, c = sop * L, d // 2 + d * k + 1
    return math.ceil((a + math.sqrt(float(a * a + 4 * a * c))) / 2.0)


def _splitmix_words(seed, start, count):
    from .workload import _G, _M1, _M2
    with np.errstate(over="ignore"):
        idx = np.arange(start + 1, start + count + 1, dtype=np.uint64)
        z = np.uint64(seed & (2**64 - 1)) + idx * _G
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


@dataclass
class PlusWorkload:
    name: str
    nvars: int
    L: int
    k: int
    kappa: int
    B: int
    l: int

    @property
    def n(self):
        return 1 << self.nvars

    def params(self):
        return PlusParameters(LinParameters(self.kappa, DecompParameters(D // 2, self.k, self.l)), self.B)

    @property
    def ajtai_seed(self):
        """the seed of ajtai_matrix's stream: PlusContext.generate_matrix(ajtai_seed, kappa, n) fills the same words on the device"""
        return 0xA17A2 + self.nvars

    def ajtai_matrix(self, cols=None):
        """(kappa, n, 16) canonical words, or the column range cols = (c0, c1) of it (what a rank of a sharded prover uploads)"""
        c0, c1 = cols if cols is not None else (0, self.n)
        rows = [_splitmix_words(0xA17A2 + self.nvars, (i * self.n + c0) * D, (c1 - c0) * D) % np.uint64(P) for i in range(self.kappa)]
        return np.stack(rows).reshape(self.kappa, c1 - c0, D)

    def r1cs(self):
        return r1cs_decomposed_square((identity_csr(self.n // self.k),) * 3, self.n, self.B, self.k)

    def z(self, i):
        """WitnessPattern::BinaryChoice: constant coefficient 0 / 1 (so z o z = z holds for the square system)"""
        z = np.zeros((self.n // self.k, D), dtype=np.uint64)
        z[:, 0] = _splitmix_words(0x2B1A0 + 977 * i + self.nvars, 0, self.n // self.k) >> np.uint64(63)
        return z


def make_plus_workload(name):
    nvars, L, k, kappa = PLUS_CONFIGS[name]
    B = estimate_bound(D * 128, L, D, k) // 2                                    # benches/e2e.rs:71
    return PlusWorkload(name, nvars, L, k, kappa, B, math.ceil(math.log(float(P)) / math.log(D / 2)))


# ---- PlusProver / PlusVerifier behind the C ABI (lfplus_prover_*, lfplus_verify: csrc/lfp_prover.cpp) and the flat PlusProof ------------------------------
PROOF_HEADER = 8                                  # lfplus.h LFPLUS_PROOF_HEADER
PROOF_MAGIC = 0x4C46504C55533031                  # lfplus.h LFPLUS_PROOF_MAGIC
PROOF_HEADER_CCS = 12                             # lfplus.h LFPLUS_PROOF_HEADER_CCS
PROOF_MAGIC_CCS = 0x4C46504C55533032              # lfplus.h LFPLUS_PROOF_MAGIC_CCS
PROOF_CM_KEYS = ("r", "msgs", "e", "b", "v", "a", "bb", "c", "comh", "pa", "pb", "ea", "eb", "cm_g", "ro", "vo", "fcoms")    # the order lfplus_mlin takes them
_NATIVE_READY = False


class _CParams(C.Structure):
    """lfplus.h lfplus_params"""
    _fields_ = [("kappa", C.c_uint32), ("k", C.c_uint32), ("l", C.c_uint32), ("b", C.c_uint64), ("B", C.c_uint64)]


def _cparams(params):
    dp = params.lin.decomp
    return _CParams(int(params.lin.kappa), int(dp.k), int(dp.l), int(dp.b), int(params.B))


def _nlib():
    global _NATIVE_READY
    L = _lib()
    if not _NATIVE_READY:
        vp, pp, u32pp, u64pp, ip = C.c_void_p, C.POINTER(_CParams), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(u64p), C.POINTER(C.c_int)
        L.lfplus_matrix_generate.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint64]
        L.lfplus_matrix_generate_timed.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]
        L.lfplus_proof_fields.argtypes = [C.c_uint32]
        L.lfplus_proof_fields.restype = C.c_uint32
        L.lfplus_proof_len.argtypes = [pp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
        L.lfplus_proof_len.restype = C.c_uint64
        L.lfplus_proof_layout.argtypes = [pp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, u64p, u64p, C.c_uint32]
        L.lfplus_prover_create.argtypes = [C.c_int, pp, u64p, C.c_uint64, C.c_uint64, C.c_uint32, u32pp, u32pp, u64pp, C.c_uint32, vp, C.POINTER(vp)]
        L.lfplus_prover_destroy.argtypes = [vp]
        L.lfplus_prover_destroy.restype = None
        L.lfplus_prover_last_error.argtypes = [vp]
        L.lfplus_prover_last_error.restype = C.c_char_p
        L.lfplus_prover_ingest.argtypes = [vp, u64pp, C.c_uint32, C.c_uint64, C.c_uint32, u64p]
        L.lfplus_prover_set_instances.argtypes = [vp, u64pp, u64pp, C.c_uint32]
        L.lfplus_prover_prove.argtypes = [vp, u64p, C.c_uint64]
        L.lfplus_prover_accumulator.argtypes = [vp, u64p, u64p]
        L.lfplus_prover_decide.argtypes = [vp, u64p, C.c_uint64, C.c_uint64, ip, C.POINTER(C.c_uint), u64p]
        L.lfplus_verify.argtypes = [pp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, u64p, C.c_uint64, ip, ip]
        vpp = C.POINTER(vp)              # host arrays of device addresses
        L.lfplus_prover_wait_stream.argtypes = [vp, vp]
        L.lfplus_prover_ingest_dev.argtypes = [vp, vpp, C.c_uint32, C.c_uint64, C.c_uint32, u64p]
        L.lfplus_prover_set_instances_dev.argtypes = [vp, vpp, u64pp, C.c_uint32]
        L.lfplus_prover_accumulator_dev.argtypes = [vp, vp, vp]
        # the same objects for committed CCS instances (the shape in place of nM) and the relation check of the fresh instances
        cp = C.POINTER(CCSDesc)
        L.lfplus_prover_create_ccs.argtypes = [C.c_int, pp, u64p, C.c_uint64, C.c_uint64, cp, u32pp, u32pp, u64pp, C.c_uint32, vp, C.POINTER(vp)]
        L.lfplus_proof_len_ccs.argtypes = [pp, C.c_uint64, cp, C.c_uint32, C.c_uint32]
        L.lfplus_proof_len_ccs.restype = C.c_uint64
        L.lfplus_proof_layout_ccs.argtypes = [pp, C.c_uint64, cp, C.c_uint32, C.c_uint32, u64p, u64p, C.c_uint32]
        L.lfplus_verify_ccs.argtypes = [pp, C.c_uint64, cp, C.c_uint32, C.c_uint32, vp, u64p, C.c_uint64, ip, ip]
        L.lfplus_prover_check_fresh.argtypes = [vp, C.c_uint64, ip, C.POINTER(C.c_uint), u64p, u64p]
        _NATIVE_READY = True
    return L


def _shape_nM(shape, nM, who):
    """the number of matrices of a flat proof: the shape's t when a CCSShape is given in place of nM (nM is then None, or agrees)"""
    if shape is None:
        return int(nM)
    if not isinstance(shape, CCSShape):
        raise LfPlusError(E_ARG, f"{who}: shape must be a CCSShape")
    if nM is not None and int(nM) != shape.t:
        raise LfPlusError(E_ARG, f"{who}: nM differs from the shape's t")
    return shape.t


def proof_len(params, n, nM, L, nfresh, shape=None):
    """lfplus_proof_len: words of the flat PlusProof of a prove that folds L instances, nfresh of them fresh (0: outside the envelope).  shape: a CCSShape in
    place of nM -- the flat proof of a CCS prover (lfplus_proof_len_ccs)"""
    if shape is not None:
        _shape_nM(shape, nM, "proof_len")
        return int(_nlib().lfplus_proof_len_ccs(C.byref(_cparams(params)), int(n), C.byref(shape.desc()), int(L), int(nfresh)))
    return int(_nlib().lfplus_proof_len(C.byref(_cparams(params)), int(n), int(nM), int(L), int(nfresh)))


def proof_fields(params, n, nM, L, nfresh, shape=None):
    """The fields of the flat PlusProof in their fixed order (lfplus.h): [(path, shape)], path = ("lproof", i, key) or (part, key).  shape: a CCSShape in place
    of nM (msgs (nvars, d + 2, 16) and evals (1 + t, 16) per fresh instance, the tail with nM = t)"""
    nM = _shape_nM(shape, nM, "proof_fields")
    np_, nev = (4, 4) if shape is None else (shape.degree + 2, 1 + shape.t)
    nvars, kappa, k, q, per = int(n).bit_length() - 1, params.lin.kappa, params.lin.decomp.k, 1 + nM, 4 + 4 * nM
    out = []
    for i in range(nfresh):
        out += [(("lproof", i, "msgs"), (nvars, np_, D)), (("lproof", i, "r"), (nvars,)), (("lproof", i, "evals"), (nev, D))]
    cm = {"r": (nvars,), "msgs": (nvars, 4, D), "e": (q, L * k, D, D), "b": (L, D), "v": (L, D), "a": (L, q), "bb": (L, q, D), "c": (L, q, D), "comh": (L, kappa, D),
          "pa": (nvars, 3, D), "pb": (nvars, 3, D), "ea": (L, per, D), "eb": (L, per, D), "cm_g": (L, kappa, D), "ro": (2, nvars), "vo": (L, q, 2, D),
          "fcoms": (L, 3, kappa, D)}
    out += [(("cmproof", key), cm[key]) for key in PROOF_CM_KEYS]
    out += [(("linb2x", "cm_g"), (kappa, D)), (("linb2x", "ro"), (2, nvars)), (("linb2x", "vo"), (q, 2, D))]
    out += [(("dproof", "C0"), (kappa, D)), (("dproof", "C1"), (kappa, D)), (("dproof", "v0"), (q, 2, D)), (("dproof", "v1"), (q, 2, D))]
    return out


def proof_layout(params, n, nM, L, nfresh, shape=None):
    """lfplus_proof_layout -> (offsets, lengths) in words, one entry per field of proof_fields; LfPlusError(E_ARG) outside the envelope.  shape: a CCSShape in
    place of nM (lfplus_proof_layout_ccs)"""
    lib = _nlib()
    nf = int(lib.lfplus_proof_fields(int(nfresh)))
    off, ln = np.zeros(nf, dtype=np.uint64), np.zeros(nf, dtype=np.uint64)
    if shape is not None:
        _shape_nM(shape, nM, "proof_layout")
        rc = lib.lfplus_proof_layout_ccs(C.byref(_cparams(params)), int(n), C.byref(shape.desc()), int(L), int(nfresh), off.ctypes.data_as(u64p), ln.ctypes.data_as(u64p), nf)
    else:
        rc = lib.lfplus_proof_layout(C.byref(_cparams(params)), int(n), int(nM), int(L), int(nfresh), off.ctypes.data_as(u64p), ln.ctypes.data_as(u64p), nf)
    if rc:
        raise LfPlusError(rc, "lfplus_proof_layout: parameters outside the envelope")
    return [int(x) for x in off], [int(x) for x in ln]


def _proof_header(params, n, nM, L, nfresh, shape=None):
    dp = params.lin.decomp
    h = [PROOF_MAGIC, L, nfresh, int(n).bit_length() - 1, dp.k, dp.l, params.lin.kappa, nM]
    if shape is not None:
        h = [PROOF_MAGIC_CCS] + h[1:7] + [shape.t, shape.q, shape.degree, sum(len(S) for S in shape.multisets), 0]
    return np.array(h, dtype=np.uint64)


def proof_to_flat(proof, params, n, nM, shape=None):
    """A PlusProof dict (PlusProver.prove, the oracle's) as the flat words of lfplus.h; L = the instances the Cm proof folds, nfresh = len(lproof).  A field
    whose shape is not the one (params, n, nM, L) imply raises LfPlusError(E_ARG).  shape: a CCSShape in place of nM (the CCS layout and header)"""
    nM = _shape_nM(shape, nM, "proof_to_flat")
    try:
        L, nfresh = int(np.asarray(proof["cmproof"]["b"]).shape[0]), len(proof["lproof"])
    except (KeyError, TypeError, IndexError) as ex:
        raise LfPlusError(E_ARG, f"malformed proof: {ex!r}")
    off, ln = proof_layout(params, n, nM, L, nfresh, shape=shape)
    hdr = _proof_header(params, n, nM, L, nfresh, shape)
    out = np.zeros(off[-1] + ln[-1], dtype=np.uint64)
    out[:hdr.size] = hdr
    for (path, shp), o, w in zip(proof_fields(params, n, nM, L, nfresh, shape=shape), off, ln):
        try:
            src = proof["lproof"][path[1]] if path[0] == "lproof" else proof[path[0]]
        except (KeyError, TypeError, IndexError) as ex:
            raise LfPlusError(E_ARG, f"malformed proof: {ex!r}")
        out[o:o + w] = _shaped(src, path[-1], shp).reshape(-1)
    return out


def proof_from_flat(words, params, n, nM, L, nfresh, shape=None):
    """The flat words as a PlusProof dict of the shapes PlusProver.prove returns (copies; the metadata k / ell / kappa / nvars is the CALLER's).  A buffer whose
    length or header disagrees with (params, n, nM, L, nfresh) raises LfPlusError(E_ARG).  shape: a CCSShape in place of nM"""
    nM = _shape_nM(shape, nM, "proof_from_flat")
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    off, ln = proof_layout(params, n, nM, L, nfresh, shape=shape)
    hdr = _proof_header(params, n, nM, L, nfresh, shape)
    if words.size != off[-1] + ln[-1] or (words[:hdr.size] != hdr).any():
        raise LfPlusError(E_ARG, "malformed proof: length or header differs from the parameters")
    nvars, dp = int(n).bit_length() - 1, params.lin.decomp
    proof = {"lproof": [{"nvars": nvars} for _ in range(nfresh)], "cmproof": {"k": dp.k, "ell": dp.l, "kappa": params.lin.kappa, "nvars": nvars}, "linb2x": {}, "dproof": {}}
    for (path, shp), o, w in zip(proof_fields(params, n, nM, L, nfresh, shape=shape), off, ln):
        dst = proof["lproof"][path[1]] if path[0] == "lproof" else proof[path[0]]
        dst[path[-1]] = words[o:o + w].reshape(shp).copy()
    return proof


class NativePlusProver:
    """PlusProver (plus.rs:15-108) as the C object lfplus_prover: the schedule PlusProver runs in Python (contexts, upload thread, from_f hints, device-resident
    accumulator, failed state) lives below the ABI; this class only marshals.  Unsharded, the accumulator always stays on the device (PlusProver.device_acc).
    A = None: the commitment matrix is generated on the device from `seed` (PlusContext.generate_matrix).  prove() returns the FLAT proof (proof_from_flat).
    shape: a CCSShape -- the prover folds committed CCS instances over the shape's t matrices M (lfplus_prover_create_ccs) and its proofs have the CCS layout."""

    def __init__(self, A, M, ncomp, params, transcript, device=0, seed=0, shape=None):
        if shape is not None and not isinstance(shape, CCSShape):
            raise LfPlusError(E_ARG, "NativePlusProver: shape must be a CCSShape")
        self.params, self.transcript, self.nM, self.ncomp, self.shape = params, transcript, len(M), int(ncomp), shape
        self.h = C.c_void_p()
        self.nacc = self.nfresh = 0
        self.last = None         # (L, nfresh) of the last proof
        self._keep = None        # host witnesses the upload thread still reads
        keep, rp, cp, vp = _csr_args(M)
        if A is not None:
            A, ap = _w(A)
            if A.ndim != 3 or A.shape[2] != D or A.shape[0] != params.lin.kappa:
                raise LfPlusError(E_ARG, "NativePlusProver: A must be (kappa, n, 16) with kappa = params.lin.kappa")
            self.n = int(A.shape[1])
        else:
            ap, self.n = None, int(keep[0][0].size - 1) if keep else 0
        self.kappa = int(params.lin.kappa)
        if shape is not None:
            if self.nM != shape.t:
                raise LfPlusError(E_ARG, f"NativePlusProver: the shape has {shape.t} matrices")
            rc = _nlib().lfplus_prover_create_ccs(int(device), C.byref(_cparams(params)), ap, int(seed) & (2**64 - 1), self.n, C.byref(shape.desc()), rp, cp, vp, self.ncomp,
                                                  transcript.h, C.byref(self.h))
        else:
            rc = _nlib().lfplus_prover_create(int(device), C.byref(_cparams(params)), ap, int(seed) & (2**64 - 1), self.n, self.nM, rp, cp, vp, self.ncomp, transcript.h,
                                              C.byref(self.h))
        if rc:
            self.h = C.c_void_p()
            raise LfPlusError(rc, "lfplus_prover_create: no usable HIP device, parameters outside the envelope (three R1CS matrices or a CCS shape, n = 2^nvars), or the "
                                  "upload failed")

    @staticmethod
    def init(A, M, ncomp, params, transcript, device=0, seed=0, shape=None):
        return NativePlusProver(A, M, ncomp, params, transcript, device, seed, shape)

    def last_error(self):
        return _nlib().lfplus_prover_last_error(self.h).decode() if self.h else ""

    def _chk(self, rc):
        if rc:
            raise LfPlusError(rc, self.last_error())

    def close(self):
        if self.h:
            _nlib().lfplus_prover_destroy(self.h)
            self.h = C.c_void_p()
        self._keep = None

    def wait_stream(self, stream=None):
        """lfplus_prover_wait_stream: the streams of every context of the prover wait for what is enqueued so far on `stream` (a hipStream_t address; default:
        the current torch stream); the host does not wait for the device"""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        self._chk(_nlib().lfplus_prover_wait_stream(self.h, C.c_void_p(stream)))

    def _dev_ptrs(self, ts, shape, who):
        if not all(api.is_device_array(t) for t in ts):
            raise LfPlusError(E_ARG, f"NativePlusProver.{who}: device and host arrays cannot be mixed")
        ptrs = (C.c_void_p * len(ts))(*[_dev(t, shape) for t in ts])
        self.wait_stream()
        return ptrs

    def ingest(self, zs, r1cs=None, l_in=1):
        """lfplus_prover_ingest: the fresh instances of the next prove from their short witnesses -> cm_f (count, kappa, 16).  Device arrays z are read in place
        (lfplus_prover_ingest_dev)"""
        zs = list(zs)
        if zs and any(api.is_device_array(z) for z in zs):
            ptrs = self._dev_ptrs(zs, tuple(zs[0].shape), "ingest")
            out = np.zeros((len(zs), self.kappa, D), dtype=np.uint64)
            self._chk(_nlib().lfplus_prover_ingest_dev(self.h, ptrs, len(zs), zs[0].shape[0], int(l_in), out.ctypes.data_as(u64p)))
            self.nfresh = len(zs)
            return out
        zs = [np.ascontiguousarray(z, dtype=np.uint64) for z in zs]
        if not zs or any(z.ndim != 2 or z.shape != zs[0].shape or z.shape[1] != D for z in zs):
            raise LfPlusError(E_ARG, "NativePlusProver.ingest: z must be equal (m, 16) arrays")
        ptrs = (u64p * len(zs))(*[z.ctypes.data_as(u64p) for z in zs])
        out = np.zeros((len(zs), self.kappa, D), dtype=np.uint64)
        self._chk(_nlib().lfplus_prover_ingest(self.h, ptrs, len(zs), zs[0].shape[0], int(l_in), out.ctypes.data_as(u64p)))
        self.nfresh = len(zs)
        return out

    def set_instances(self, fs, cm_fs=None):
        """lfplus_prover_set_instances: the fresh instances of the next prove from host witnesses (n, 16); they go up on the library's worker thread.  Device
        arrays f (cm_f stays host) are copied and checked at once, without a worker, and are free again on return (lfplus_prover_set_instances_dev)"""
        fs = list(fs)
        dev = bool(fs) and any(api.is_device_array(f) for f in fs)
        if not dev:
            fs = [np.ascontiguousarray(f, dtype=np.uint64) for f in fs]
        if not fs or any(tuple(f.shape) != (self.n, D) for f in fs):
            raise LfPlusError(E_ARG, "NativePlusProver.set_instances: f must be (n, 16) arrays")
        cms = None if cm_fs is None else [np.ascontiguousarray(c, dtype=np.uint64) for c in cm_fs]
        if cms is not None and (len(cms) != len(fs) or any(c.shape != (self.kappa, D) for c in cms)):
            raise LfPlusError(E_ARG, "NativePlusProver.set_instances: cm_f must be (kappa, 16) arrays, one per instance")
        if dev:
            fp = self._dev_ptrs(fs, (self.n, D), "set_instances")
            cp = None if cms is None else (u64p * len(fs))(*[c.ctypes.data_as(u64p) for c in cms])
            self._chk(_nlib().lfplus_prover_set_instances_dev(self.h, fp, cp, len(fs)))
            self.nfresh = len(fs)
            return
        fp = (u64p * len(fs))(*[f.ctypes.data_as(u64p) for f in fs])
        cp = None if cms is None else (u64p * len(fs))(*[c.ctypes.data_as(u64p) for c in cms])
        self._keep = fs          # borrowed by the worker until the prove returns
        self._chk(_nlib().lfplus_prover_set_instances(self.h, fp, cp, len(fs)))
        self.nfresh = len(fs)

    def prove(self, comp=None):
        """lfplus_prover_prove -> the flat proof.  comp: host ComR1CS instances (set_instances is called with their f and cm_f); None: the instances named by
        the last ingest / set_instances"""
        if comp is not None:
            self.set_instances([ci.f for ci in comp], [ci.cm_f for ci in comp])
        L, nfresh = self.nacc + self.nfresh, self.nfresh
        words = proof_len(self.params, self.n, self.nM, L, nfresh, shape=self.shape) if L else 0
        out = np.zeros(max(words, 1), dtype=np.uint64)
        try:
            self._chk(_nlib().lfplus_prover_prove(self.h, out.ctypes.data_as(u64p), words))
        finally:
            self._keep = None
        self.nacc, self.nfresh, self.last = 2, 0, (L, nfresh)
        return out

    def check_fresh(self, bound=0):
        """lfplus_prover_check_fresh: is every instance named by the last ingest / set_instances in its relation (ccs_check for a CCS prover, r1cs_check otherwise,
        where the instance lives; cm_f when set_instances gave it; ||f||_inf < bound, 0: not checked) -> [(ok, failed, first_bad, absmax)] per instance.  Valid
        between naming the instances and prove(); read-only"""
        cnt = max(self.nfresh, 1)
        ok, failed, fb, am = (C.c_int * cnt)(), (C.c_uint * cnt)(), (C.c_uint64 * cnt)(), (C.c_uint64 * cnt)()
        rc = _nlib().lfplus_prover_check_fresh(self.h, int(bound), ok, failed, fb, am)
        if rc not in (0, E_REJECT):
            self._chk(rc)
        return [(bool(ok[i]), int(failed[i]), int(fb[i]), int(am[i])) for i in range(self.nfresh)]

    def accumulator(self, out=None):
        """(F0, F1) of the last prove, read back from the device; out = (F0, F1) device arrays (n, 16), either may be None: copied there, device to device
        (lfplus_prover_accumulator_dev), and returned"""
        if out is not None:
            F = tuple(out)
            if len(F) != 2 or any(x is not None and not api.is_device_array(x) for x in F):
                raise LfPlusError(E_ARG, "NativePlusProver.accumulator: out must be two device arrays (or None)")
            ptrs = [None if x is None else _dev(x, (self.n, D)) for x in F]
            self.wait_stream()
            self._chk(_nlib().lfplus_prover_accumulator_dev(self.h, *ptrs))
            return F
        F = [np.zeros((self.n, D), dtype=np.uint64) for _ in range(2)]
        self._chk(_nlib().lfplus_prover_accumulator(self.h, F[0].ctypes.data_as(u64p), F[1].ctypes.data_as(u64p)))
        return tuple(F)

    def decide(self, proof, bound=0):
        """lfplus_prover_decide on the flat proof of the last prove -> [(ok, failed, absmax)] per accumulator half (as PlusProver.decide)"""
        w = np.ascontiguousarray(proof, dtype=np.uint64).reshape(-1)
        ok, failed, am = (C.c_int * 2)(), (C.c_uint * 2)(), (C.c_uint64 * 2)()
        rc = _nlib().lfplus_prover_decide(self.h, w.ctypes.data_as(u64p), w.size, int(bound), ok, failed, am)
        if rc not in (0, E_REJECT):
            self._chk(rc)
        return [(bool(ok[i]), int(failed[i]), int(am[i])) for i in range(2)]


class NativePlusVerifier:
    """PlusVerifier (plus.rs:25-33, 110-146) through lfplus_verify: host only, on the flat proof.  The statement -- params, n, nM and per proof (L, nfresh) --
    is the verifier's own.  verify returns True, or False with .stage = (which proof, stage) named as PlusVerifier names them, ("malformed", message) for a
    buffer that does not fit the statement; .which is the C index (i < nfresh, nfresh: cmproof, nfresh + 1: dproof, -1: malformed).  shape: a CCSShape -- the
    statement is about committed CCS instances over the shape's t matrices and the proofs have the CCS layout (lfplus_verify_ccs)"""

    def __init__(self, A, M, params, transcript, shape=None):
        if shape is not None and (not isinstance(shape, CCSShape) or shape.t != len(M)):
            raise LfPlusError(E_ARG, "NativePlusVerifier: shape must be a CCSShape over len(M) matrices")
        self.params, self.transcript, self.nM, self.shape = params, transcript, len(M), shape
        shape = tuple(A) if isinstance(A, tuple) else np.asarray(A).shape          # (kappa, n, 16): the matrix or just its shape
        if len(shape) != 3 or shape[2] != D or shape[0] != params.lin.kappa or shape[1] < 2 or shape[1] & (shape[1] - 1):
            raise LfPlusError(E_ARG, "NativePlusVerifier: A must be (kappa, n = 2^nvars, 16) with kappa = params.lin.kappa")
        self.n = int(shape[1])
        self.stage, self.which, self.code = None, None, 0

    @staticmethod
    def init(A, M, params, transcript, shape=None):
        return NativePlusVerifier(A, M, params, transcript, shape)

    def verify(self, proof, L, nfresh):
        w, p = (None, None) if proof is None else _w(np.asarray(proof).reshape(-1))
        which, st = C.c_int(), C.c_int()
        if self.shape is not None:
            rc = _nlib().lfplus_verify_ccs(C.byref(_cparams(self.params)), self.n, C.byref(self.shape.desc()), int(L), int(nfresh), self.transcript.h, p,
                                           0 if w is None else w.size, C.byref(which), C.byref(st))
        else:
            rc = _nlib().lfplus_verify(C.byref(_cparams(self.params)), self.n, self.nM, int(L), int(nfresh), self.transcript.h, p, 0 if w is None else w.size,
                                       C.byref(which), C.byref(st))
        self.code, self.which = rc, which.value
        if rc == 0:
            self.stage = None
            return True
        if rc == E_REJECT:
            name = f"lproof[{which.value}]" if which.value < nfresh else ("cmproof", "dproof")[which.value - nfresh]
            self.stage = (name, st.value)
            return False
        if rc == E_ARG:
            self.stage = ("malformed", "length or header differs from the verifier's parameters")
            return False
        raise LfPlusError(rc, "lfplus_verify")
