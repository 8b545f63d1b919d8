//! LatticeFold+ behind the reference's `PlusProver` / `PlusVerifier` surface (`crates/latticefold-plus/src/plus.rs:15-146`) over the prover and verifier
//! objects of `include/lfplus.h` (`lfplus_prover_*`, `lfplus_verify`).
//!
//! | reference (file:line)                                   | here                                           |
//! |---------------------------------------------------------|------------------------------------------------|
//! | `PlusProver::{init, prove}` `plus.rs:55-108`            | [`HipPlusProver::init`], [`HipPlusProver::prove`] |
//! | `PlusVerifier::{init, verify}` `plus.rs:118-143`        | [`HipPlusVerifier::init`], [`HipPlusVerifier::verify`] (host only) |
//! | `PlusProof` `plus.rs:34-40`                             | [`PlusProof`]: the flat words of `lfplus.h`    |
//! | `PlusParameters` `plus.rs:42-47`                        | [`PlusParameters`] (`sys::lfplus_params`)      |
//! | `PoseidonTranscript<RqPoly>` `transcript.rs:20-78`      | [`HipPlusTranscript`]                          |
//! | `MLSumcheck::{prove, verify}_as_subprotocol` `latticefold/src/utils/sumcheck.rs:53-104` | [`HipPlusMLSumcheck`] over a [`HipPlusVPoly`] |
//! | (none: "Support CCS" is the reference README's next step) committed CCS instances, `ComR1CS::linearize` / `ComR1CSProof::verify` `r1cs.rs:72-163` generalised | [`HipComCCS`] over a [`HipPlusCCS`]: `linearize`, `verify`, `check_relation` |
//! | `RqPoly` products and `SparseMatrix` x vector on arrays (the `g_q = M_q f`, `g_A o g_B - g_C` of `r1cs.rs:76-95`) | [`HipPlusContext::ring_mul`], [`HipPlusContext::spmv`] and their `_device` forms |
//!
//! The ring is the one the reference runs latticefold-plus on (FrogRing `RqPoly`, coefficient form, 16 canonical words per element); `R: RingWords` with
//! `WORDS == 16` marshals it.  The schedule of a prove -- which context holds which accumulator half, the upload thread, the refusal to continue after a
//! half-advanced transcript -- is the library's; this module only marshals.  NOT COMPILED in the build image, as the rest of the crate;
//! `tests/test_lfplus_native_cpu.py` checks names and arities against the reference.
#![allow(non_snake_case)]

use core::marker::PhantomData;

use latticefold_hip_sys as sys;
use stark_rings_linalg::{Matrix, SparseMatrix};

use crate::{flatten, RingWords};

/// A failure of the LatticeFold+ ABI: `code` is the library's `LFPLUS_E_*` value (`sys::LFPLUS_E_ARG`, `sys::LFPLUS_E_REJECT`, ...)
#[derive(Debug, Clone, thiserror::Error)]
#[error("liblfhip (lfplus): {what}: {msg} ({code})")]
pub struct HipPlusError {
    pub code: i32,
    pub what: &'static str,
    pub msg: String,
}

impl HipPlusError {
    fn new(code: i32, what: &'static str, msg: impl Into<String>) -> Self {
        HipPlusError { code, what, msg: msg.into() }
    }
    /// `LFPLUS_E_ARG`: a shape, a length or the object's state refuses the call
    pub fn is_arg(&self) -> bool {
        self.code == sys::LFPLUS_E_ARG
    }
    /// `LFPLUS_E_REJECT`: a verifier rejected the proof
    pub fn is_reject(&self) -> bool {
        self.code == sys::LFPLUS_E_REJECT
    }
}

/// `PlusParameters { lin: LinParameters { kappa, decomp: DecompParameters { b, k, l } }, B }`, flat
pub type PlusParameters = sys::lfplus_params;

/// `PlusProof` as the flat canonical words `lfplus.h` documents (header, per fresh instance `msgs | r | evals`, the `CmProof` fields, `linb2x`, `dproof`)
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct PlusProof(pub Vec<u64>);

impl PlusProof {
    /// `lfplus_proof_len`: the words of a proof that folds `L` instances, `nfresh` of them fresh
    pub fn len_for(params: &PlusParameters, n: usize, nM: usize, L: usize, nfresh: usize) -> usize {
        // SAFETY: params is a valid reference; the call reads nothing else
        unsafe { sys::lfplus_proof_len(params, n as u64, nM as u32, L as u32, nfresh as u32) as usize }
    }
    /// `lfplus_proof_len_ccs`: the same for a prover of committed CCS instances (0: a shape or parameters the library refuses)
    pub fn len_for_ccs(params: &PlusParameters, n: usize, shape: &HipPlusCCS, L: usize, nfresh: usize) -> usize {
        let (off, idx, coef) = shape.flat();
        let d = sys::lfplus_ccs { t: shape.t as u32, q: shape.terms.len() as u32, S_off: off.as_ptr(), S_idx: idx.as_ptr(), c: coef.as_ptr() };
        // SAFETY: params is a valid reference; d points into off / idx / coef, which outlive the call
        unsafe { sys::lfplus_proof_len_ccs(params, n as u64, &d, L as u32, nfresh as u32) as usize }
    }
    /// `lfplus_proof_layout_ccs`: (offset, length) in words of every field of such a proof, in the order `lfplus.h` documents; `None` where `len_for_ccs` is 0
    pub fn layout_for_ccs(params: &PlusParameters, n: usize, shape: &HipPlusCCS, L: usize, nfresh: usize) -> Option<Vec<(usize, usize)>> {
        let (off, idx, coef) = shape.flat();
        let d = sys::lfplus_ccs { t: shape.t as u32, q: shape.terms.len() as u32, S_off: off.as_ptr(), S_idx: idx.as_ptr(), c: coef.as_ptr() };
        // SAFETY: no pointer is passed
        let nf = unsafe { sys::lfplus_proof_fields(nfresh as u32) } as usize;
        let (mut o, mut l) = (vec![0u64; nf], vec![0u64; nf]);
        // SAFETY: d points into off / idx / coef; o and l hold the nf entries the call is told of
        let rc = unsafe { sys::lfplus_proof_layout_ccs(params, n as u64, &d, L as u32, nfresh as u32, o.as_mut_ptr(), l.as_mut_ptr(), nf as u32) };
        if rc != sys::LFPLUS_OK {
            return None;
        }
        Some(o.iter().zip(&l).map(|(a, b)| (*a as usize, *b as usize)).collect())
    }
}

/// `PoseidonTranscript::<RqPoly>::empty::<FrogPoseidonConfig>()`: the host sponge the library advances
pub struct HipPlusTranscript {
    raw: *mut sys::lfplus_transcript,
}
// SAFETY: a transcript is a plain host object with no thread affinity; `&mut self` serialises its users
unsafe impl Send for HipPlusTranscript {}

impl Default for HipPlusTranscript {
    fn default() -> Self {
        // SAFETY: returns an owned handle (never null: the allocation aborts on failure)
        HipPlusTranscript { raw: unsafe { sys::lfplus_transcript_new() } }
    }
}
impl Clone for HipPlusTranscript {
    fn clone(&self) -> Self {
        // SAFETY: self.raw is a live handle
        HipPlusTranscript { raw: unsafe { sys::lfplus_transcript_clone(self.raw) } }
    }
}
impl Drop for HipPlusTranscript {
    fn drop(&mut self) {
        // SAFETY: the handle is owned and freed exactly once
        unsafe { sys::lfplus_transcript_free(self.raw) }
    }
}
impl HipPlusTranscript {
    pub fn absorb<R: RingWords>(&mut self, v: &[R]) {
        let w = flatten(v);
        // SAFETY: w holds v.len() ring elements of 16 words
        unsafe { sys::lfplus_transcript_absorb(self.raw, w.as_ptr(), v.len()) };
    }
    pub fn get_challenge(&mut self) -> u64 {
        let mut out = 0u64;
        // SAFETY: out is one word
        unsafe { sys::lfplus_transcript_challenge(self.raw, &mut out) };
        out
    }
}

/// CSR triples (`rowptr`, `col`, `val[nnz][16]`) of a `SparseMatrix<R>` padded to `n` rows
fn csr<R: RingWords + Clone>(m: &SparseMatrix<R>, n: usize) -> (Vec<u32>, Vec<u32>, Vec<u64>) {
    let (mut rowptr, mut col, mut val) = (vec![0u32], Vec::new(), Vec::new());
    for row in &m.coeffs {
        for (c, j) in row {
            col.push(*j as u32);
            c.to_words(&mut val);
        }
        rowptr.push(col.len() as u32);
    }
    rowptr.resize(n + 1, col.len() as u32);
    (rowptr, col, val)
}

/// A fresh `ComR1CS` instance in host form: the witness `f` (n ring elements) and its commitment `cm_f` (kappa ring elements), flat
pub struct HipComR1CS {
    pub f: Vec<u64>,
    pub cm_f: Vec<u64>,
}

impl HipComR1CS {
    pub fn new<R: RingWords>(f: &[R], cm_f: &[R]) -> Self {
        HipComR1CS { f: flatten(f), cm_f: flatten(cm_f) }
    }
}

/// `PlusProver<R, TS>`: 2 + ncomp device contexts sharing A and M, the accumulator resident between proves
pub struct HipPlusProver<R> {
    raw: *mut sys::lfplus_prover,
    // private: the C object holds this handle's raw pointer for its whole life, so the field must never be replaced (see `transcript`)
    transcript: HipPlusTranscript,
    pub params: PlusParameters,
    n: usize,
    nM: usize,
    nacc: usize,
    nfresh: usize,
    // Some: a prover of committed CCS instances (`init_ccs`); its proofs have the CCS layout
    shape: Option<HipPlusCCS>,
    _r: PhantomData<R>,
}
// SAFETY: the object has no thread affinity (every entry point selects its device); `&mut self` gives the one-thread-at-a-time the header asks for
unsafe impl<R> Send for HipPlusProver<R> {}

impl<R: RingWords + Clone> HipPlusProver<R> {
    /// Initialize (plus.rs:55-74) on device 0
    pub fn init(A: Matrix<R>, M: Vec<SparseMatrix<R>>, ncomp: usize, params: PlusParameters, transcript: HipPlusTranscript) -> Result<Self, HipPlusError> {
        assert_eq!(R::WORDS, 16, "the LatticeFold+ ABI is the Frog ring: 16 words per element");
        let n = A.ncols;
        let a_words: Vec<u64> = A.vals.iter().flat_map(|row| flatten(row)).collect();
        let mats: Vec<_> = M.iter().map(|m| csr(m, n)).collect();
        let rp: Vec<*const u32> = mats.iter().map(|m| m.0.as_ptr()).collect();
        let cp: Vec<*const u32> = mats.iter().map(|m| m.1.as_ptr()).collect();
        let vp: Vec<*const u64> = mats.iter().map(|m| m.2.as_ptr()).collect();
        let mut raw = core::ptr::null_mut();
        // SAFETY: every pointer outlives the call (the library copies A and M to the device); the transcript handle outlives the prover, which owns it
        let rc = unsafe {
            sys::lfplus_prover_create(0, &params, a_words.as_ptr(), 0, n as u64, M.len() as u32, rp.as_ptr(), cp.as_ptr(), vp.as_ptr(), ncomp as u32, transcript.raw, &mut raw)
        };
        if rc != sys::LFPLUS_OK {
            return Err(HipPlusError::new(rc, "lfplus_prover_create", "no usable device, or parameters outside the envelope"));
        }
        Ok(HipPlusProver { raw, transcript, params, n, nM: M.len(), nacc: 0, nfresh: 0, shape: None, _r: PhantomData })
    }

    /// The same for committed CCS instances over the `shape.t` matrices `M` (`lfplus_prover_create_ccs`): `prove` linearizes with `lfplus_ccs_linearize` and
    /// writes the CCS layout; the instances are `HipComR1CS` values (a witness and its commitment: nothing in them is R1CS-specific)
    pub fn init_ccs(A: Matrix<R>, M: Vec<SparseMatrix<R>>, shape: HipPlusCCS, ncomp: usize, params: PlusParameters, transcript: HipPlusTranscript) -> Result<Self, HipPlusError> {
        assert_eq!(R::WORDS, 16, "the LatticeFold+ ABI is the Frog ring: 16 words per element");
        if M.len() != shape.t {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "lfplus_prover_create_ccs", "the shape names t matrices"));
        }
        let n = A.ncols;
        let a_words: Vec<u64> = A.vals.iter().flat_map(|row| flatten(row)).collect();
        let mats: Vec<_> = M.iter().map(|m| csr(m, n)).collect();
        let rp: Vec<*const u32> = mats.iter().map(|m| m.0.as_ptr()).collect();
        let cp: Vec<*const u32> = mats.iter().map(|m| m.1.as_ptr()).collect();
        let vp: Vec<*const u64> = mats.iter().map(|m| m.2.as_ptr()).collect();
        let (off, idx, coef) = shape.flat();
        let d = sys::lfplus_ccs { t: shape.t as u32, q: shape.terms.len() as u32, S_off: off.as_ptr(), S_idx: idx.as_ptr(), c: coef.as_ptr() };
        let mut raw = core::ptr::null_mut();
        // SAFETY: every pointer outlives the call (the library copies A, M and the shape); the transcript handle outlives the prover, which owns it
        let rc = unsafe {
            sys::lfplus_prover_create_ccs(0, &params, a_words.as_ptr(), 0, n as u64, &d, rp.as_ptr(), cp.as_ptr(), vp.as_ptr(), ncomp as u32, transcript.raw, &mut raw)
        };
        if rc != sys::LFPLUS_OK {
            return Err(HipPlusError::new(rc, "lfplus_prover_create_ccs", "no usable device, a refused shape, or parameters outside the envelope"));
        }
        Ok(HipPlusProver { raw, transcript, params, n, nM: M.len(), nacc: 0, nfresh: 0, shape: Some(shape), _r: PhantomData })
    }

    /// `lfplus_prover_set_instances`: names the fresh instances of the next prove (their upload starts on the library's worker thread).  With
    /// [`HipPlusProver::check_fresh`] and [`HipPlusProver::prove_named`] this is `prove` in steps.
    /// # Safety
    /// every `comp[i].f` stays alive and unmoved until `prove_named` (or the drop of the prover) returns: the library borrows it
    pub unsafe fn set_instances(&mut self, comp: &[HipComR1CS]) -> Result<(), HipPlusError> {
        let fp: Vec<*const u64> = comp.iter().map(|c| c.f.as_ptr()).collect();
        let cp: Vec<*const u64> = comp.iter().map(|c| c.cm_f.as_ptr()).collect();
        // SAFETY: the caller's contract
        let rc = unsafe { sys::lfplus_prover_set_instances(self.raw, fp.as_ptr(), cp.as_ptr(), comp.len() as u32) };
        if rc != sys::LFPLUS_OK {
            return Err(self.err(rc, "lfplus_prover_set_instances"));
        }
        self.nfresh = comp.len();
        Ok(())
    }

    /// `lfplus_prover_check_fresh`: is every instance named for the next prove in its relation (`lfplus_ccs_check` for a CCS prover, `lfplus_r1cs_check`
    /// otherwise), where it lives -> per instance (failed: the `LFPLUS_REL_*` bits, first_bad, absmax); `Ok` also when one is not satisfied.  Read-only
    pub fn check_fresh(&mut self, bound: u64) -> Result<Vec<(u32, u64, u64)>, HipPlusError> {
        let cnt = self.nfresh.max(1);
        let (mut ok, mut failed, mut first_bad, mut absmax) = (vec![0i32; cnt], vec![0u32; cnt], vec![0u64; cnt], vec![0u64; cnt]);
        // SAFETY: the four arrays hold at least nfresh entries, the number of instances the library has been given
        let rc = unsafe { sys::lfplus_prover_check_fresh(self.raw, bound, ok.as_mut_ptr(), failed.as_mut_ptr(), first_bad.as_mut_ptr(), absmax.as_mut_ptr()) };
        if rc != sys::LFPLUS_OK && rc != sys::LFPLUS_E_REJECT {
            return Err(self.err(rc, "lfplus_prover_check_fresh"));
        }
        Ok((0..self.nfresh).map(|i| (failed[i], first_bad[i], absmax[i])).collect())
    }

    fn proof_words(&self, L: usize, nfresh: usize) -> usize {
        match &self.shape {
            Some(shape) => PlusProof::len_for_ccs(&self.params, self.n, shape, L, nfresh),
            None => PlusProof::len_for(&self.params, self.n, self.nM, L, nfresh),
        }
    }

    /// `lfplus_prover_prove` on the instances named by `set_instances` / `ingest_dev` / `set_instances_dev`
    pub fn prove_named(&mut self) -> Result<PlusProof, HipPlusError> {
        let words = self.proof_words(self.nacc + self.nfresh, self.nfresh);
        let mut proof = vec![0u64; words];
        // SAFETY: proof holds exactly the words the library checks the length against
        let rc = unsafe { sys::lfplus_prover_prove(self.raw, proof.as_mut_ptr(), words as u64) };
        if rc != sys::LFPLUS_OK {
            return Err(self.err(rc, "lfplus_prover_prove"));
        }
        self.nacc = 2;
        self.nfresh = 0;
        Ok(PlusProof(proof))
    }

    /// The transcript the prover advances (`PlusProver::transcript` of the reference, read-only here: the library borrows the handle until the prover is
    /// dropped).  Clone it to continue the Fiat-Shamir schedule elsewhere.
    pub fn transcript(&self) -> &HipPlusTranscript {
        &self.transcript
    }

    fn err(&self, rc: i32, what: &'static str) -> HipPlusError {
        // SAFETY: returns a NUL-terminated string owned by the prover, valid until its next call
        let msg = unsafe { std::ffi::CStr::from_ptr(sys::lfplus_prover_last_error(self.raw)) }.to_string_lossy().into_owned();
        HipPlusError::new(rc, what, msg)
    }

    /// Prove (plus.rs:77-108): the fresh instances go up on the library's worker thread while the ones that have arrived are linearized
    pub fn prove(&mut self, comp: &[HipComR1CS]) -> Result<PlusProof, HipPlusError> {
        let fp: Vec<*const u64> = comp.iter().map(|c| c.f.as_ptr()).collect();
        let cp: Vec<*const u64> = comp.iter().map(|c| c.cm_f.as_ptr()).collect();
        // SAFETY: `comp` is borrowed for the whole call, which covers the span the library borrows f for (until lfplus_prover_prove returns)
        let rc = unsafe { sys::lfplus_prover_set_instances(self.raw, fp.as_ptr(), cp.as_ptr(), comp.len() as u32) };
        if rc != sys::LFPLUS_OK {
            return Err(self.err(rc, "lfplus_prover_set_instances"));
        }
        let words = self.proof_words(self.nacc + comp.len(), comp.len());
        let mut proof = vec![0u64; words];
        // SAFETY: proof holds exactly the words the library checks the length against
        let rc = unsafe { sys::lfplus_prover_prove(self.raw, proof.as_mut_ptr(), words as u64) };
        if rc != sys::LFPLUS_OK {
            return Err(self.err(rc, "lfplus_prover_prove"));
        }
        self.nacc = 2;
        Ok(PlusProof(proof))
    }

    // ---- device-resident callers (`lfplus.h` "device-resident callers"): raw device pointers, as `HipContext::*_dev` of lib.rs.  NOT COMPILED, like the rest.

    /// `lfplus_prover_wait_stream`: every context of the prover waits for what `hip_stream` holds now (null: the default stream)
    /// # Safety
    /// `hip_stream` is a live `hipStream_t` of the prover's device, or null
    pub unsafe fn wait_stream(&mut self, hip_stream: *mut core::ffi::c_void) -> Result<(), HipPlusError> {
        // SAFETY: the caller's contract
        let rc = unsafe { sys::lfplus_prover_wait_stream(self.raw, hip_stream) };
        if rc != sys::LFPLUS_OK { Err(self.err(rc, "lfplus_prover_wait_stream")) } else { Ok(()) }
    }

    /// `lfplus_prover_ingest_dev`: the fresh instances of the next prove from short witnesses `z[i]` (m ring elements each) in DEVICE memory, read in
    /// place -> their commitments (count x kappa x 16 words)
    /// # Safety
    /// every `z[i]` is 16-byte aligned device memory of the prover's device holding m x 16 canonical words, complete on the stream last passed to `wait_stream`
    pub unsafe fn ingest_dev(&mut self, z: &[*const u64], m: usize, l_in: usize) -> Result<Vec<u64>, HipPlusError> {
        let mut cm = vec![0u64; z.len() * self.params.kappa as usize * 16];
        // SAFETY: the caller's contract; cm holds count x kappa ring elements
        let rc = unsafe { sys::lfplus_prover_ingest_dev(self.raw, z.as_ptr(), z.len() as u32, m as u64, l_in as u32, cm.as_mut_ptr()) };
        if rc != sys::LFPLUS_OK {
            return Err(self.err(rc, "lfplus_prover_ingest_dev"));
        }
        self.nfresh = z.len();
        Ok(cm)
    }

    /// `lfplus_prover_set_instances_dev`: the same from witnesses `f[i]` (n ring elements each) in DEVICE memory; copied and checked before the call returns
    /// (no upload thread, nothing is borrowed afterwards).  `cm_f[i]`: host words (kappa x 16) or null
    /// # Safety
    /// every `f[i]` is 16-byte aligned device memory of the prover's device holding n x 16 words; every non-null `cm_f[i]` is kappa x 16 host words
    pub unsafe fn set_instances_dev(&mut self, f: &[*const u64], cm_f: &[*const u64]) -> Result<(), HipPlusError> {
        assert_eq!(f.len(), cm_f.len());
        // SAFETY: the caller's contract
        let rc = unsafe { sys::lfplus_prover_set_instances_dev(self.raw, f.as_ptr(), cm_f.as_ptr(), f.len() as u32) };
        if rc != sys::LFPLUS_OK {
            return Err(self.err(rc, "lfplus_prover_set_instances_dev"));
        }
        self.nfresh = f.len();
        Ok(())
    }

    /// `lfplus_prover_accumulator_dev`: the accumulator halves copied, device to device, into `F0` / `F1` (n x 16 words each; either may be null)
    /// # Safety
    /// non-null pointers are 16-byte aligned device memory of the prover's device with room for n x 16 words, and do not overlap
    pub unsafe fn accumulator_dev(&mut self, F0: *mut u64, F1: *mut u64) -> Result<(), HipPlusError> {
        // SAFETY: the caller's contract
        let rc = unsafe { sys::lfplus_prover_accumulator_dev(self.raw, F0, F1) };
        if rc != sys::LFPLUS_OK { Err(self.err(rc, "lfplus_prover_accumulator_dev")) } else { Ok(()) }
    }
}

/// One `lfplus_ctx` for the component calls on DEVICE memory (`lfplus_*_dev`): the commitment matrix generated on the device, witnesses and vectors as raw
/// device pointers.  NOT COMPILED, like the rest of the crate.
pub struct HipPlusContext {
    raw: *mut sys::lfplus_ctx,
    kappa: usize,
}
// SAFETY: no thread affinity (every entry point selects its device); `&mut self` serialises the users
unsafe impl Send for HipPlusContext {}

impl HipPlusContext {
    /// `lfplus_ctx_create` + `lfplus_matrix_generate(seed, kappa, n)`
    pub fn generate(device: i32, seed: u64, kappa: usize, n: usize) -> Result<Self, HipPlusError> {
        let mut raw = core::ptr::null_mut();
        // SAFETY: raw receives an owned handle
        let rc = unsafe { sys::lfplus_ctx_create(device, &mut raw) };
        if rc != sys::LFPLUS_OK {
            return Err(HipPlusError::new(rc, "lfplus_ctx_create", "no usable device"));
        }
        let ctx = HipPlusContext { raw, kappa };
        // SAFETY: live handle
        ctx.chk(unsafe { sys::lfplus_matrix_generate(raw, seed, kappa as u32, n as u64) }, "lfplus_matrix_generate")?;
        Ok(ctx)
    }
    fn chk(&self, rc: i32, what: &'static str) -> Result<(), HipPlusError> {
        if rc == sys::LFPLUS_OK {
            return Ok(());
        }
        // SAFETY: a NUL-terminated string owned by the context, valid until its next call
        let msg = unsafe { std::ffi::CStr::from_ptr(sys::lfplus_last_error(self.raw)) }.to_string_lossy().into_owned();
        Err(HipPlusError::new(rc, what, msg))
    }
    /// `lfplus_ctx_wait_stream`
    /// # Safety
    /// `hip_stream` is a live `hipStream_t` of the context's device, or null
    pub unsafe fn wait_stream(&mut self, hip_stream: *mut core::ffi::c_void) -> Result<(), HipPlusError> {
        // SAFETY: the caller's contract
        self.chk(unsafe { sys::lfplus_ctx_wait_stream(self.raw, hip_stream) }, "lfplus_ctx_wait_stream")
    }
    /// `lfplus_set_witness_dev`
    /// # Safety
    /// `f`: n x 16 words of 16-byte aligned device memory of the context's device
    pub unsafe fn set_witness_dev(&mut self, f: *const u64, n: usize) -> Result<(), HipPlusError> {
        // SAFETY: the caller's contract
        self.chk(unsafe { sys::lfplus_set_witness_dev(self.raw, f, n as u64) }, "lfplus_set_witness_dev")
    }
    /// `lfplus_witness_from_z_dev` -> cm_f
    /// # Safety
    /// `z`: m x 16 words of 16-byte aligned device memory of the context's device
    pub unsafe fn witness_from_z_dev(&mut self, z: *const u64, m: usize, b: u64, k: u32) -> Result<Vec<u64>, HipPlusError> {
        let mut cm = vec![0u64; self.kappa * 16];
        // SAFETY: the caller's contract; cm holds kappa ring elements
        self.chk(unsafe { sys::lfplus_witness_from_z_dev(self.raw, z, m as u64, b, k, cm.as_mut_ptr()) }, "lfplus_witness_from_z_dev")?;
        Ok(cm)
    }
    /// `lfplus_commit_dev` -> A v
    /// # Safety
    /// `v`: n x 16 words of 16-byte aligned device memory of the context's device
    pub unsafe fn commit_dev(&mut self, v: *const u64, n: usize) -> Result<Vec<u64>, HipPlusError> {
        let mut out = vec![0u64; self.kappa * 16];
        // SAFETY: the caller's contract; out holds kappa ring elements
        self.chk(unsafe { sys::lfplus_commit_dev(self.raw, v, n as u64, out.as_mut_ptr()) }, "lfplus_commit_dev")?;
        Ok(out)
    }
    /// `lfplus_get_witness_dev`
    /// # Safety
    /// `f_out`: room for n x 16 words of 16-byte aligned device memory of the context's device
    pub unsafe fn get_witness_dev(&mut self, f_out: *mut u64, n: usize) -> Result<(), HipPlusError> {
        // SAFETY: the caller's contract
        self.chk(unsafe { sys::lfplus_get_witness_dev(self.raw, f_out, n as u64) }, "lfplus_get_witness_dev")
    }
    /// `lfplus_decompose_dev` on the resident constraint matrices (`nm` of them; 0: none) -> (C0, C1, v0, v1); `F0` / `F1` (either may be null) receive the halves
    /// # Safety
    /// non-null `F0` / `F1`: room for n x 16 words of 16-byte aligned device memory of the context's device each, not overlapping; `r_a` / `r_b`: log2(n) ring elements
    pub unsafe fn decompose_dev(&mut self, B: u64, r_a: &[u64], r_b: &[u64], nm: usize, F0: *mut u64, F1: *mut u64) -> Result<[Vec<u64>; 4], HipPlusError> {
        let (mut c0, mut c1) = (vec![0u64; self.kappa * 16], vec![0u64; self.kappa * 16]);
        let (mut v0, mut v1) = (vec![0u64; (1 + nm) * 32], vec![0u64; (1 + nm) * 32]);
        // SAFETY: the caller's contract; the host outputs have the sizes lfplus.h documents; null CSR pointers select the resident matrices
        self.chk(
            unsafe {
                sys::lfplus_decompose_dev(self.raw, B, r_a.as_ptr(), r_b.as_ptr(), nm as u32, core::ptr::null(), core::ptr::null(), core::ptr::null(), F0, F1, c0.as_mut_ptr(),
                                          c1.as_mut_ptr(), v0.as_mut_ptr(), v1.as_mut_ptr())
            },
            "lfplus_decompose_dev",
        )?;
        Ok([c0, c1, v0, v1])
    }
    /// `lfplus_ring_mul`: out[x] = sum_i a_i[x] * b_i[x] over `n_terms` tables of `count` ring elements (16 canonical words each; table i of `a` at
    /// `i * count * 16`).  `broadcast`: `b` holds one ring element per term instead of a table
    pub fn ring_mul(&mut self, a: &[u64], b: &[u64], n_terms: usize, count: usize, broadcast: bool) -> Result<Vec<u64>, HipPlusError> {
        if n_terms == 0 || count == 0 || a.len() != n_terms * count * 16 || b.len() != if broadcast { n_terms * 16 } else { a.len() } {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "ring_mul", "a: n_terms x count x 16 words; b: the same, or n_terms x 16 words with broadcast"));
        }
        let mode = if broadcast { sys::LFPLUS_MUL_BROADCAST } else { sys::LFPLUS_MUL_ELEMENTWISE };
        let mut out = vec![0u64; count * 16];
        // SAFETY: live handle; the arrays have the sizes checked above
        self.chk(unsafe { sys::lfplus_ring_mul(self.raw, a.as_ptr(), b.as_ptr(), n_terms as u64, count as u64, mode as i32, out.as_mut_ptr()) }, "lfplus_ring_mul")?;
        Ok(out)
    }
    /// `lfplus_ring_mul_device`: the same on the caller's device arrays, in place; `b` is a HOST pointer with `broadcast`
    /// # Safety
    /// `a` (and `b` without `broadcast`): n_terms x count x 16 words, `out`: count x 16 words of 16-byte aligned device memory of the context's device; `b` with
    /// `broadcast`: n_terms x 16 words of host memory; `out` overlaps an input only as lfplus.h allows
    pub unsafe fn ring_mul_device(&mut self, a: *const u64, b: *const u64, n_terms: usize, count: usize, broadcast: bool, out: *mut u64) -> Result<(), HipPlusError> {
        let mode = if broadcast { sys::LFPLUS_MUL_BROADCAST } else { sys::LFPLUS_MUL_ELEMENTWISE };
        // SAFETY: the caller's contract
        self.chk(unsafe { sys::lfplus_ring_mul_device(self.raw, a, b, n_terms as u64, count as u64, mode as i32, out) }, "lfplus_ring_mul_device")
    }
    /// `lfplus_spmv`: M_j x for the j-th resident constraint matrix; `x` = n ring elements
    pub fn spmv(&mut self, j: usize, x: &[u64]) -> Result<Vec<u64>, HipPlusError> {
        if x.is_empty() || x.len() % 16 != 0 {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "spmv", "x: n x 16 words"));
        }
        let mut y = vec![0u64; x.len()];
        // SAFETY: live handle; y has the size of x
        self.chk(unsafe { sys::lfplus_spmv(self.raw, j as u32, x.as_ptr(), (x.len() / 16) as u64, y.as_mut_ptr()) }, "lfplus_spmv")?;
        Ok(y)
    }
    /// `lfplus_spmv_device`
    /// # Safety
    /// `x`, `y`: n x 16 words of 16-byte aligned device memory of the context's device each, not overlapping
    pub unsafe fn spmv_device(&mut self, j: usize, x: *const u64, n: usize, y: *mut u64) -> Result<(), HipPlusError> {
        // SAFETY: the caller's contract
        self.chk(unsafe { sys::lfplus_spmv_device(self.raw, j as u32, x, n as u64, y) }, "lfplus_spmv_device")
    }
    /// `lfplus_build_eq`: the table eq(point, .) as 2^nv constant polynomials (nv = `point.len()` words, 1..=28) -- the eq factor of a generic sumcheck
    pub fn build_eq(&mut self, point: &[u64]) -> Result<Vec<u64>, HipPlusError> {
        if point.is_empty() || point.len() > 28 {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "build_eq", "point: 1 ..= 28 words"));
        }
        let mut out = vec![0u64; 16usize << point.len()];
        // SAFETY: live handle; out holds 2^nv ring elements
        self.chk(unsafe { sys::lfplus_build_eq(self.raw, point.as_ptr(), point.len() as u32, out.as_mut_ptr()) }, "lfplus_build_eq")?;
        Ok(out)
    }
    /// `lfplus_build_eq_device`
    /// # Safety
    /// `out`: room for 2^nv x 16 words of 16-byte aligned device memory of the context's device
    pub unsafe fn build_eq_device(&mut self, point: &[u64], out: *mut u64) -> Result<(), HipPlusError> {
        // SAFETY: the caller's contract
        self.chk(unsafe { sys::lfplus_build_eq_device(self.raw, point.as_ptr(), point.len() as u32, out) }, "lfplus_build_eq_device")
    }
    /// `lfplus_mle_eval_batch`: out[j] = sum_{x < len} eq(point, x) T_j[x] for `ntables` tables of `len` <= 2^nv general ring elements -> ntables x 16 words
    pub fn mle_eval_batch(&mut self, tables: &[u64], ntables: usize, len: usize, point: &[u64]) -> Result<Vec<u64>, HipPlusError> {
        if ntables == 0 || len == 0 || tables.len() != ntables * len * 16 || point.is_empty() {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "mle_eval_batch", "tables: ntables x len x 16 words; point: nv words"));
        }
        let mut out = vec![0u64; ntables * 16];
        // SAFETY: live handle; the arrays have the sizes checked above
        self.chk(
            unsafe { sys::lfplus_mle_eval_batch(self.raw, tables.as_ptr(), ntables as u32, len as u64, point.as_ptr(), point.len() as u32, out.as_mut_ptr()) },
            "lfplus_mle_eval_batch",
        )?;
        Ok(out)
    }
    /// `lfplus_mle_eval_batch_device`: the tables are read in place; the point and the result stay on the host
    /// # Safety
    /// `tables`: ntables x len x 16 words of 16-byte aligned device memory of the context's device
    pub unsafe fn mle_eval_batch_device(&mut self, tables: *const u64, ntables: usize, len: usize, point: &[u64]) -> Result<Vec<u64>, HipPlusError> {
        let mut out = vec![0u64; ntables * 16];
        // SAFETY: the caller's contract; out holds ntables ring elements
        self.chk(
            unsafe { sys::lfplus_mle_eval_batch_device(self.raw, tables, ntables as u32, len as u64, point.as_ptr(), point.len() as u32, out.as_mut_ptr()) },
            "lfplus_mle_eval_batch_device",
        )?;
        Ok(out)
    }
    /// `lfplus_mle_fix_variables`: the lowest `point.len()` variables of `ntables` tables of `len` = 2^nv ring elements fixed at `point` -> ntables x (len >> nfix) x 16 words
    pub fn mle_fix_variables(&mut self, tables: &[u64], ntables: usize, len: usize, point: &[u64]) -> Result<Vec<u64>, HipPlusError> {
        if ntables == 0 || !len.is_power_of_two() || tables.len() != ntables * len * 16 || point.is_empty() || point.len() > 28 || len >> point.len() == 0 {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "mle_fix_variables", "tables: ntables x 2^nv x 16 words; point: 1 ..= nv words"));
        }
        let mut out = vec![0u64; ntables * (len >> point.len()) * 16];
        // SAFETY: live handle; the arrays have the sizes checked above
        self.chk(
            unsafe { sys::lfplus_mle_fix_variables(self.raw, tables.as_ptr(), ntables as u32, len as u64, point.as_ptr(), point.len() as u32, out.as_mut_ptr()) },
            "lfplus_mle_fix_variables",
        )?;
        Ok(out)
    }
    /// `lfplus_mle_fix_variables_device`
    /// # Safety
    /// `tables`: ntables x len x 16 words, `out`: room for ntables x (len >> nfix) x 16 words of 16-byte aligned device memory of the context's device, not overlapping
    pub unsafe fn mle_fix_variables_device(&mut self, tables: *const u64, ntables: usize, len: usize, point: &[u64], out: *mut u64) -> Result<(), HipPlusError> {
        // SAFETY: the caller's contract
        self.chk(
            unsafe { sys::lfplus_mle_fix_variables_device(self.raw, tables, ntables as u32, len as u64, point.as_ptr(), point.len() as u32, out) },
            "lfplus_mle_fix_variables_device",
        )
    }
    /// `lfplus_spmv_t`: M_j^T v for the j-th resident constraint matrix; `v` = n general ring elements
    pub fn spmv_t(&mut self, j: usize, v: &[u64]) -> Result<Vec<u64>, HipPlusError> {
        if v.is_empty() || v.len() % 16 != 0 {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "spmv_t", "v: n x 16 words"));
        }
        let mut out = vec![0u64; v.len()];
        // SAFETY: live handle; out has the size of v
        self.chk(unsafe { sys::lfplus_spmv_t(self.raw, j as u32, v.as_ptr(), (v.len() / 16) as u64, out.as_mut_ptr()) }, "lfplus_spmv_t")?;
        Ok(out)
    }
    /// `lfplus_spmv_t_device`
    /// # Safety
    /// `v`, `out`: n x 16 words of 16-byte aligned device memory of the context's device each, not overlapping
    pub unsafe fn spmv_t_device(&mut self, j: usize, v: *const u64, n: usize, out: *mut u64) -> Result<(), HipPlusError> {
        // SAFETY: the caller's contract
        self.chk(unsafe { sys::lfplus_spmv_t_device(self.raw, j as u32, v, n as u64, out) }, "lfplus_spmv_t_device")
    }
    /// `lfplus_balanced_decompose`: the `k` balanced base-`b` digits of every coefficient of `x` (count x 16 words), as canonical residues.  `planes`: digit i of
    /// element j at `i * count + j` (`decompose_to_vec(b, k).transpose()`); otherwise at `j * k + i` (`Vec<R>::gadget_decompose(b, k)`)
    pub fn balanced_decompose(&mut self, x: &[u64], b: u64, k: usize, planes: bool) -> Result<Vec<u64>, HipPlusError> {
        if x.is_empty() || x.len() % 16 != 0 || k == 0 || k > 64 {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "balanced_decompose", "x: count x 16 words; 1 <= k <= 64"));
        }
        let layout = if planes { sys::LFPLUS_DIGITS_PLANES } else { sys::LFPLUS_DIGITS_GADGET };
        let mut out = vec![0u64; x.len() * k];
        // SAFETY: live handle; out has k times the size of x
        self.chk(unsafe { sys::lfplus_balanced_decompose(self.raw, x.as_ptr(), (x.len() / 16) as u64, b, k as u32, layout as i32, out.as_mut_ptr()) }, "lfplus_balanced_decompose")?;
        Ok(out)
    }
    /// `lfplus_balanced_decompose_device`
    /// # Safety
    /// `x`: count x 16 words, `out`: count x k x 16 words of 16-byte aligned device memory of the context's device, not overlapping
    pub unsafe fn balanced_decompose_device(&mut self, x: *const u64, count: usize, b: u64, k: usize, planes: bool, out: *mut u64) -> Result<(), HipPlusError> {
        let layout = if planes { sys::LFPLUS_DIGITS_PLANES } else { sys::LFPLUS_DIGITS_GADGET };
        // SAFETY: the caller's contract
        self.chk(unsafe { sys::lfplus_balanced_decompose_device(self.raw, x, count as u64, b, k as u32, layout as i32, out) }, "lfplus_balanced_decompose_device")
    }
    /// `lfplus_balanced_recompose`: out[j] = sum_i b^i x[digit i of j], coefficient by coefficient mod p; `x` = count x k GENERAL ring elements in the layout
    /// `balanced_decompose` writes
    pub fn balanced_recompose(&mut self, x: &[u64], b: u64, k: usize, planes: bool) -> Result<Vec<u64>, HipPlusError> {
        if x.is_empty() || k == 0 || k > 64 || x.len() % (16 * k) != 0 {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "balanced_recompose", "x: count x k x 16 words; 1 <= k <= 64"));
        }
        let layout = if planes { sys::LFPLUS_DIGITS_PLANES } else { sys::LFPLUS_DIGITS_GADGET };
        let mut out = vec![0u64; x.len() / k];
        // SAFETY: live handle; out has a k-th of the size of x
        self.chk(unsafe { sys::lfplus_balanced_recompose(self.raw, x.as_ptr(), (x.len() / (16 * k)) as u64, b, k as u32, layout as i32, out.as_mut_ptr()) }, "lfplus_balanced_recompose")?;
        Ok(out)
    }
    /// `lfplus_balanced_recompose_device`
    /// # Safety
    /// `x`: count x k x 16 words, `out`: count x 16 words of 16-byte aligned device memory of the context's device, not overlapping
    pub unsafe fn balanced_recompose_device(&mut self, x: *const u64, count: usize, b: u64, k: usize, planes: bool, out: *mut u64) -> Result<(), HipPlusError> {
        let layout = if planes { sys::LFPLUS_DIGITS_PLANES } else { sys::LFPLUS_DIGITS_GADGET };
        // SAFETY: the caller's contract
        self.chk(unsafe { sys::lfplus_balanced_recompose_device(self.raw, x, count as u64, b, k as u32, layout as i32, out) }, "lfplus_balanced_recompose_device")
    }
    /// `lfplus_linf_norm`: the largest |centred coefficient| of `v` (count x 16 words)
    pub fn linf_norm(&mut self, v: &[u64]) -> Result<u64, HipPlusError> {
        if v.is_empty() || v.len() % 16 != 0 {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "linf_norm", "v: count x 16 words"));
        }
        let mut absmax = 0u64;
        // SAFETY: live handle; absmax is one word
        self.chk(unsafe { sys::lfplus_linf_norm(self.raw, v.as_ptr(), (v.len() / 16) as u64, &mut absmax) }, "lfplus_linf_norm")?;
        Ok(absmax)
    }
    /// `lfplus_linf_norm_device`
    /// # Safety
    /// `v`: count x 16 words of 16-byte aligned device memory of the context's device
    pub unsafe fn linf_norm_device(&mut self, v: *const u64, count: usize) -> Result<u64, HipPlusError> {
        let mut absmax = 0u64;
        // SAFETY: the caller's contract; absmax is one word of host memory
        self.chk(unsafe { sys::lfplus_linf_norm_device(self.raw, v, count as u64, &mut absmax) }, "lfplus_linf_norm_device")?;
        Ok(absmax)
    }
    /// `lfplus_set_matrices_gadget`: the system as stated over z (`M`: matrices of `rows` x `m`) made resident in its gadget form over
    /// f = z.gadget_decompose(b, k), n = m k -- what `r1cs_decomposed_square` builds on the host, expanded on the device from the short arrays
    pub fn set_matrices_gadget<R: RingWords + Clone>(&mut self, M: &[SparseMatrix<R>], rows: usize, m: usize, b: u64, k: usize) -> Result<(), HipPlusError> {
        let flat: Vec<(Vec<u32>, Vec<u32>, Vec<u64>)> = M.iter().map(|x| csr(x, rows)).collect();
        let rp: Vec<*const u32> = flat.iter().map(|x| x.0.as_ptr()).collect();
        let cp: Vec<*const u32> = flat.iter().map(|x| x.1.as_ptr()).collect();
        let vp: Vec<*const u64> = flat.iter().map(|x| x.2.as_ptr()).collect();
        // SAFETY: live handle; the pointer arrays name M.len() CSR triples of rows + 1 / nnz / nnz x 16 entries that outlive the call
        self.chk(
            unsafe { sys::lfplus_set_matrices_gadget(self.raw, rows as u64, m as u64, b, k as u32, (m * k) as u64, M.len() as u32, rp.as_ptr(), cp.as_ptr(), vp.as_ptr()) },
            "lfplus_set_matrices_gadget",
        )
    }
    /// `lfplus_ctx_create` alone: a BARE context (no matrix, no witness) -- all the generic sumcheck needs
    pub fn bare(device: i32) -> Result<Self, HipPlusError> {
        let mut raw = core::ptr::null_mut();
        // SAFETY: raw receives an owned handle
        let rc = unsafe { sys::lfplus_ctx_create(device, &mut raw) };
        if rc != sys::LFPLUS_OK {
            return Err(HipPlusError::new(rc, "lfplus_ctx_create", "no usable device"));
        }
        Ok(HipPlusContext { raw, kappa: 0 })
    }
}

/// `VirtualPolynomial<RqPoly>` as the flat product list of `lfplus_vpoly` (`latticefold/src/utils/sumcheck/utils.rs:24-75`):
/// g = sum_i coef_i prod_{k in terms[i]} T_k; `coef[i]` is one ring element (16 canonical words)
#[derive(Debug, Clone)]
pub struct HipPlusVPoly {
    pub nvars: usize,
    pub ntables: usize,
    pub degree: usize,
    pub terms: Vec<([u64; 16], Vec<u32>)>,
}

/// `MLSumcheck<RqPoly, _>` over any product list on the GPU (`lfplus_mlsumcheck_*`), under the reference's names (`latticefold/src/utils/sumcheck.rs:53-104`)
pub struct HipPlusMLSumcheck;

impl HipPlusMLSumcheck {
    /// `MLSumcheck::prove_as_subprotocol`: `tables` = T x 2^nvars x 16 canonical words (table j first entry at `j * 2^nvars * 16`; variable 1 in bit 0 of the
    /// entry index) -> (msgs: nvars x (degree + 1) x 16 words, point: nvars challenges, the T table values at the point)
    pub fn prove_as_subprotocol(ctx: &mut HipPlusContext, transcript: &mut HipPlusTranscript, poly: &HipPlusVPoly, tables: &[u64])
                                -> Result<(Vec<u64>, Vec<u64>, Vec<u64>), HipPlusError> {
        if poly.nvars == 0 || poly.nvars > 28 || tables.len() != (poly.ntables << poly.nvars) * 16 {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "prove_as_subprotocol", "tables: ntables x 2^nvars x 16 words, 1 <= nvars <= 28"));
        }
        let (mut off, mut idx, mut coef) = (vec![0u32], Vec::new(), Vec::new());
        for (c, ix) in &poly.terms {
            idx.extend_from_slice(ix);
            off.push(idx.len() as u32);
            coef.extend_from_slice(c);
        }
        idx.push(0);
        let d = sys::lfplus_vpoly { nvars: poly.nvars as u32, ntables: poly.ntables as u32, nterms: poly.terms.len() as u32, degree: poly.degree as u32,
                                    term_off: off.as_ptr(), term_idx: idx.as_ptr(), coef: coef.as_ptr() };
        let mut msgs = vec![0u64; poly.nvars * (poly.degree + 1) * 16];
        let (mut point, mut fin) = (vec![0u64; poly.nvars], vec![0u64; poly.ntables * 16]);
        // SAFETY: live handles; d points into off / idx / coef, which outlive the call; tables and the outputs have the sizes lfplus.h documents (the library
        // refuses a descriptor outside its envelope before it reads a table)
        ctx.chk(unsafe { sys::lfplus_mlsumcheck_prove(ctx.raw, transcript.raw, &d, tables.as_ptr(), msgs.as_mut_ptr(), point.as_mut_ptr(), fin.as_mut_ptr()) },
                "lfplus_mlsumcheck_prove")?;
        Ok((msgs, point, fin))
    }
    /// `MLSumcheck::verify_as_subprotocol`, host only -> the subclaim (point, expected evaluation); `Err` with `is_reject()` and the failing round in `msg`
    pub fn verify_as_subprotocol(transcript: &mut HipPlusTranscript, nvars: usize, degree: usize, claimed_sum: &[u64; 16], msgs: &[u64])
                                 -> Result<(Vec<u64>, [u64; 16]), HipPlusError> {
        if nvars == 0 || nvars > 28 || degree == 0 || degree > 8 || msgs.len() != nvars * (degree + 1) * 16 {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "verify_as_subprotocol", "msgs: nvars x (degree + 1) x 16 words, 1 <= nvars <= 28, 1 <= degree <= 8"));
        }
        let (mut point, mut expected, mut round) = (vec![0u64; nvars], [0u64; 16], -1i32);
        // SAFETY: live handle; the arrays have the sizes checked above
        let rc = unsafe {
            sys::lfplus_mlsumcheck_verify(transcript.raw, nvars as u32, degree as u32, claimed_sum.as_ptr(), msgs.as_ptr(), point.as_mut_ptr(), expected.as_mut_ptr(), &mut round)
        };
        if rc != sys::LFPLUS_OK {
            return Err(HipPlusError::new(rc, "lfplus_mlsumcheck_verify", if rc == sys::LFPLUS_E_REJECT { format!("round {round}") } else { "bad arguments".into() }));
        }
        Ok((point, expected))
    }
}
/// A CCS shape over `t` resident constraint matrices (`lfplus_ccs`): sum_i coef_i prod_{j in multisets[i]} (M_j f) = 0 row by row; `coef` is one ring element
/// (16 canonical words) per multiset.  Envelope (refused by the library with `LFPLUS_E_ARG`): 1 <= t, q <= 8, 1 <= |S_i| <= 7, at most 16 indices in all.
#[derive(Debug, Clone)]
pub struct HipPlusCCS {
    pub t: usize,
    pub terms: Vec<([u64; 16], Vec<u32>)>,
}

impl HipPlusCCS {
    /// (M_0 f) o (M_1 f) - M_2 f: the shape `lfplus_r1cs_linearize` hard-wires (word-identical proofs)
    pub fn r1cs() -> Self {
        let (mut one, mut minus) = ([0u64; 16], [0u64; 16]);
        one[0] = 1;
        minus[0] = sys::LFPLUS_P - 1;
        HipPlusCCS { t: 3, terms: vec![(one, vec![0, 1]), (minus, vec![2])] }
    }
    /// d = max |S_i|: the sumcheck runs at degree d + 1
    pub fn degree(&self) -> usize {
        self.terms.iter().map(|(_, s)| s.len()).max().unwrap_or(0)
    }
    fn flat(&self) -> (Vec<u32>, Vec<u32>, Vec<u64>) {
        let (mut off, mut idx, mut coef) = (vec![0u32], Vec::new(), Vec::new());
        for (c, s) in &self.terms {
            idx.extend_from_slice(s);
            off.push(idx.len() as u32);
            coef.extend_from_slice(c);
        }
        idx.push(0);
        (off, idx, coef)
    }
}

/// The linearization of a committed CCS instance (`lfplus_ccs_*`; self-consistent, pinned to the reference at the R1CS shape), on a context whose resident
/// witness is the instance's `f` and whose resident matrices (`lfplus_set_matrices`) are the shape's `t`
pub struct HipComCCS;

impl HipComCCS {
    /// `lfplus_ccs_linearize` -> (msgs: nvars x (d + 2) x 16 words, ro: nvars words, evals: (1 + t) x 16 words); `nvars` = log2 of the resident witness's length
    pub fn linearize(ctx: &mut HipPlusContext, transcript: &mut HipPlusTranscript, shape: &HipPlusCCS, nvars: usize) -> Result<(Vec<u64>, Vec<u64>, Vec<u64>), HipPlusError> {
        let (off, idx, coef) = shape.flat();
        let d = sys::lfplus_ccs { t: shape.t as u32, q: shape.terms.len() as u32, S_off: off.as_ptr(), S_idx: idx.as_ptr(), c: coef.as_ptr() };
        let mut msgs = vec![0u64; nvars * (shape.degree() + 2) * 16];
        let (mut ro, mut evals) = (vec![0u64; nvars.max(1)], vec![0u64; (1 + shape.t) * 16]);
        // SAFETY: live handles; d points into off / idx / coef, which outlive the call; the outputs have the sizes lfplus.h documents for a witness of 2^nvars
        // elements (the library refuses a shape outside its envelope before it writes); null CSR pointers select the resident matrices
        ctx.chk(
            unsafe {
                sys::lfplus_ccs_linearize(ctx.raw, transcript.raw, &d, core::ptr::null(), core::ptr::null(), core::ptr::null(), msgs.as_mut_ptr(), ro.as_mut_ptr(),
                                          evals.as_mut_ptr())
            },
            "lfplus_ccs_linearize",
        )?;
        ro.truncate(nvars);
        Ok((msgs, ro, evals))
    }
    /// `lfplus_ccs_verify`, host only -> ro; `Err` with `is_reject()` and the stage (1 = a sumcheck round, 2 = the final identity) in `msg`
    pub fn verify(transcript: &mut HipPlusTranscript, nvars: usize, shape: &HipPlusCCS, msgs: &[u64], evals: &[u64]) -> Result<Vec<u64>, HipPlusError> {
        let dg = shape.degree();
        if nvars == 0 || nvars > 32 || dg == 0 || dg > 7 || shape.t == 0 || shape.t > 8 || msgs.len() != nvars * (dg + 2) * 16 || evals.len() != (1 + shape.t) * 16 {
            return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "ccs_verify", "msgs: nvars x (d + 2) x 16 words, evals: (1 + t) x 16 words, 1 <= nvars <= 32, 1 <= d <= 7, 1 <= t <= 8"));
        }
        let (off, idx, coef) = shape.flat();
        let d = sys::lfplus_ccs { t: shape.t as u32, q: shape.terms.len() as u32, S_off: off.as_ptr(), S_idx: idx.as_ptr(), c: coef.as_ptr() };
        let (mut ro, mut stage) = (vec![0u64; nvars], 0i32);
        // SAFETY: live handle; d points into off / idx / coef; the arrays have the sizes checked above
        let rc = unsafe { sys::lfplus_ccs_verify(transcript.raw, nvars as u32, &d, msgs.as_ptr(), evals.as_ptr(), ro.as_mut_ptr(), &mut stage) };
        if rc != sys::LFPLUS_OK {
            return Err(HipPlusError::new(rc, "lfplus_ccs_verify", if rc == sys::LFPLUS_E_REJECT { format!("stage {stage}") } else { "bad arguments".into() }));
        }
        Ok(ro)
    }
    /// `lfplus_ccs_check` on the resident (A, f) and the resident matrices -> (failed: the `LFPLUS_REL_*` bits, first_bad, absmax); `Ok` also when the instance
    /// is not satisfied (`failed != 0`).  `cm_f`: kappa x 16 words, or `None` (not checked); `bound` 0: the norm is not checked
    pub fn check_relation(ctx: &mut HipPlusContext, shape: &HipPlusCCS, cm_f: Option<&[u64]>, bound: u64) -> Result<(u32, u64, u64), HipPlusError> {
        if let Some(cm) = cm_f {
            if cm.len() != ctx.kappa * 16 {
                return Err(HipPlusError::new(sys::LFPLUS_E_ARG, "ccs_check", "cm_f: kappa x 16 words"));
            }
        }
        let (off, idx, coef) = shape.flat();
        let d = sys::lfplus_ccs { t: shape.t as u32, q: shape.terms.len() as u32, S_off: off.as_ptr(), S_idx: idx.as_ptr(), c: coef.as_ptr() };
        let (mut failed, mut first_bad, mut absmax) = (0u32, 0u64, 0u64);
        // SAFETY: live handle; d points into off / idx / coef; cm_f has the size checked above; null CSR pointers select the resident matrices
        let rc = unsafe {
            sys::lfplus_ccs_check(ctx.raw, cm_f.map_or(core::ptr::null(), |c| c.as_ptr()), &d, core::ptr::null(), core::ptr::null(), core::ptr::null(), bound, &mut failed,
                                  &mut first_bad, &mut absmax)
        };
        if rc != sys::LFPLUS_OK && rc != sys::LFPLUS_E_REJECT {
            ctx.chk(rc, "lfplus_ccs_check")?;
        }
        Ok((failed, first_bad, absmax))
    }
}
impl Drop for HipPlusContext {
    fn drop(&mut self) {
        // SAFETY: owned handle, destroyed once
        unsafe { sys::lfplus_ctx_destroy(self.raw) }
    }
}

impl<R> Drop for HipPlusProver<R> {
    fn drop(&mut self) {
        // SAFETY: owned handle, destroyed once, before the transcript field it borrows is dropped
        unsafe { sys::lfplus_prover_destroy(self.raw) }
    }
}

/// `PlusVerifier<R, TS>` (host only: no GPU, no context)
pub struct HipPlusVerifier<R> {
    pub transcript: HipPlusTranscript,
    pub params: PlusParameters,
    n: usize,
    nM: usize,
    nacc: usize,
    // Some: the statement is about committed CCS instances (`init_ccs`); proofs have the CCS layout
    shape: Option<HipPlusCCS>,
    _r: PhantomData<R>,
}

impl<R: RingWords> HipPlusVerifier<R> {
    /// Initialize (plus.rs:118-130): only the shapes of A and M enter the verification
    pub fn init(A: Matrix<R>, M: Vec<SparseMatrix<R>>, params: PlusParameters, transcript: HipPlusTranscript) -> Self {
        HipPlusVerifier { transcript, params, n: A.ncols, nM: M.len(), nacc: 0, shape: None, _r: PhantomData }
    }
    /// The verifier of a [`HipPlusProver::init_ccs`] prover (`lfplus_verify_ccs`; host only)
    pub fn init_ccs(A: Matrix<R>, M: Vec<SparseMatrix<R>>, shape: HipPlusCCS, params: PlusParameters, transcript: HipPlusTranscript) -> Self {
        HipPlusVerifier { transcript, params, n: A.ncols, nM: M.len(), nacc: 0, shape: Some(shape), _r: PhantomData }
    }

    /// Verify (plus.rs:133-143) a proof that folds `nfresh` fresh instances into this verifier's accumulator.  `Err` with `LFPLUS_E_REJECT` and the
    /// `(which, stage)` of the sub-verifier in the message where the reference panics; `LFPLUS_E_ARG` for a buffer that does not fit the statement
    pub fn verify_fresh(&mut self, proof: &PlusProof, nfresh: usize) -> Result<bool, HipPlusError> {
        let (mut which, mut stage) = (0i32, 0i32);
        let L = self.nacc + nfresh;
        let rc = match &self.shape {
            Some(shape) => {
                let (off, idx, coef) = shape.flat();
                let d = sys::lfplus_ccs { t: shape.t as u32, q: shape.terms.len() as u32, S_off: off.as_ptr(), S_idx: idx.as_ptr(), c: coef.as_ptr() };
                // SAFETY: d points into off / idx / coef; the library checks proof.0.len() against its own layout before it reads a field
                unsafe {
                    sys::lfplus_verify_ccs(&self.params, self.n as u64, &d, L as u32, nfresh as u32, self.transcript.raw, proof.0.as_ptr(), proof.0.len() as u64, &mut which, &mut stage)
                }
            }
            // SAFETY: the library checks proof.0.len() against its own layout before it reads a field
            None => unsafe {
                sys::lfplus_verify(&self.params, self.n as u64, self.nM as u32, L as u32, nfresh as u32, self.transcript.raw, proof.0.as_ptr(), proof.0.len() as u64, &mut which, &mut stage)
            },
        };
        if rc != sys::LFPLUS_OK {
            return Err(HipPlusError::new(rc, if self.shape.is_some() { "lfplus_verify_ccs" } else { "lfplus_verify" }, format!("which = {which}, stage = {stage}")));
        }
        self.nacc = 2;
        Ok(true)
    }

    /// Verify with the reference's signature.  The reference takes the number of fresh instances from the proof it is handed (`proof.lproof.len()`,
    /// plus.rs:134-136); this mirrors it deliberately by reading the header's nfresh word and passing it on as the statement.  Nothing is SIZED from that
    /// word: the library derives the one admissible length from (params, n, nM, L, nfresh) and refuses any other buffer before it reads a field.  A caller
    /// that knows how many instances it expects calls [`HipPlusVerifier::verify_fresh`] with its own count.
    pub fn verify(&mut self, proof: &PlusProof) -> bool {
        let nfresh = proof.0.get(2).copied().unwrap_or(0) as usize;
        self.verify_fresh(proof, nfresh).unwrap_or(false)
    }
}
