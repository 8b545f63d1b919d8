//! `HipChainProver`: the chained NIFS prover object of include/lfhip_prover.h (`lf_prover_*`) behind a safe owner.
//!
//! `NIFSProver::prove` in a loop (nifs/tests.rs:58-117, examples/e2e.rs): every step ingests a new `w_ccs`, commits it and folds it into an accumulator that the
//! object keeps on the device.  The prover BORROWS its context: `HipChainProver<'ctx, ..>` holds `&'ctx HipContext`, so the borrow checker enforces the library's
//! rule that provers are destroyed before their context; `Drop` abandons a pending ingest job and frees the accumulator.  Every error carries the library's code
//! and the text of `lf_prover_last_error` (`HipError::Lib(text, code)`): `LF_ERR_STATE` for call-sequence misuse and for a context whose CCS or matrix was
//! loaded again, `LF_ERR_REJECT` never (the two checks return the failing components instead).
//!
//! NOT COMPILED in the build image, as the rest of this crate (see lib.rs).
use core::marker::PhantomData;

use cyclotomic_rings::rings::SuitableRing;
use latticefold::{
    arith::{CCCS, LCCCS},
    commitment::Commitment,
    decomposition_parameters::DecompositionParams,
    nifs::{linearization::LinearizationProof, LFProof},
    transcript::TranscriptWithShortChallenges,
};
use latticefold_hip_sys as sys;
use sys::prover as raw;

use super::{as_hip, dec_proof_from, flatten, fold_proof_from, lcccs_from, lcccs_words, lin_proof_from, ring_id, section_lens, unflatten, HipContext, HipError, RingWords};

/// `LF_PROVER_COMMIT_INLINE`: commit the fresh witness at the head of `prove` on the main lane (the one placement the library has; accepted for callers that
/// name it)
pub const COMMIT_INLINE: u32 = raw::LF_PROVER_COMMIT_INLINE;

/// Owner of an `lf_prover`.  One thread at a time (`&mut self` on everything that changes the chain).
pub struct HipChainProver<'ctx, NTT, P> {
    ctx: &'ctx HipContext,
    raw: *mut raw::lf_prover,
    /// the host words of the pending instance: the library borrows them from `ingest` until the `prove` that consumes them (or `Drop`) returns
    pending_words: Option<Box<[u64]>>,
    _m: PhantomData<(NTT, P)>,
}
// SAFETY: the handle is plain host state plus device handles of a context that is Sync; the object is used from one thread at a time (&mut self)
unsafe impl<'ctx, NTT, P> Send for HipChainProver<'ctx, NTT, P> {}

impl<'ctx, NTT: SuitableRing, P: DecompositionParams> HipChainProver<'ctx, NTT, P> {
    fn err(&self, rc: i32, what: &str) -> HipError {
        // SAFETY: lf_prover_last_error never returns null and the text lives until the next call on this prover
        let msg = unsafe { std::ffi::CStr::from_ptr(raw::lf_prover_last_error(self.raw)) }.to_string_lossy().into_owned();
        HipError::Lib(format!("{what}: {msg}"), rc)
    }
    fn chk(&self, rc: i32, what: &str) -> Result<(), HipError> {
        if rc == sys::LF_OK { Ok(()) } else { Err(self.err(rc, what)) }
    }

    /// `lf_prover_create`: the context must have a CCS loaded and an Ajtai matrix resident (`LF_ERR_STATE`) and must not be sharded (`LF_ERR_UNSUPPORTED`)
    pub fn create(ctx: &'ctx HipContext, flags: u32) -> Result<Self, HipError> {
        ring_id::<NTT>()?;
        let mut h = core::ptr::null_mut();
        // SAFETY: out-pointer to a local; the library fills it on success only
        super::chk(unsafe { raw::lf_prover_create(ctx.raw, flags, &mut h) }, "lf_prover_create")?;
        Ok(Self { ctx, raw: h, pending_words: None, _m: PhantomData })
    }

    /// first accumulator = the linearization of `(x_ccs, w_ccs)` on `transcript` (`Witness::from_w_ccs` + `Witness::commit` + `LFLinearizationProver::prove`)
    pub fn init(&mut self, transcript: &mut impl TranscriptWithShortChallenges<NTT>, w_ccs: &[NTT], x_ccs: &[NTT]) -> Result<(LCCCS<NTT>, LinearizationProof<NTT>), HipError> {
        let p = self.ctx.params()?;
        assert_eq!(w_ccs.len(), p.wit_len as usize);
        assert_eq!(x_ccs.len(), p.l as usize);
        let tr = as_hip::<NTT, _>(transcript)?;
        let (lin, _, _) = section_lens::<NTT>(&p);
        // SAFETY: p is a live parameter block
        let ll = unsafe { sys::lf_lcccs_len_ring(&p, ring_id::<NTT>()?) };
        let (w, x) = (flatten(w_ccs), flatten(x_ccs));
        let (mut lc, mut pr) = (vec![0u64; ll * NTT::WORDS], vec![0u64; lin * NTT::WORDS]);
        // SAFETY: input lengths checked above, output lengths per include/lfhip.h (lf_lcccs_len_ring, the linearization proof of lf_linearize)
        let rc = unsafe { raw::lf_prover_init(self.raw, tr, w.as_ptr(), x.as_ptr(), lc.as_mut_ptr(), pr.as_mut_ptr()) };
        self.chk(rc, "lf_prover_init")?;
        Ok((lcccs_from(&lc, &p), lin_proof_from(&unflatten::<NTT>(&pr), &p)))
    }

    /// take up a chain again from `(acc, f)`: the folded witness `f` in NTT form, N elements
    pub fn resume(&mut self, acc: &LCCCS<NTT>, f: &[NTT]) -> Result<(), HipError> {
        let p = self.ctx.params()?;
        assert_eq!(f.len(), (p.wit_len * p.L) as usize);
        let (a, w) = (lcccs_words(acc), flatten(f));
        // SAFETY: a holds lf_lcccs_len_ring elements, w holds N
        let rc = unsafe { raw::lf_prover_resume(self.raw, a.as_ptr(), w.as_ptr()) };
        self.chk(rc, "lf_prover_resume")
    }

    /// the same from device memory of the context's device (N elements, NTT form, the layout of the host ABI)
    ///
    /// # Safety
    /// `f_dev` must stay allocated and unwritten until the call returns.
    pub unsafe fn resume_dev(&mut self, acc: &LCCCS<NTT>, f_dev: *const u64) -> Result<(), HipError> {
        let a = lcccs_words(acc);
        // SAFETY: the caller vouches for the device range; the library checks the pointer before it launches anything
        let rc = unsafe { raw::lf_prover_resume_dev(self.raw, a.as_ptr(), f_dev) };
        self.chk(rc, "lf_prover_resume_dev")
    }

    /// names the fresh instance of the NEXT `prove` and returns at once: the upload, the ICRT and the gadget decomposition run on a worker thread
    pub fn ingest(&mut self, w_ccs: &[NTT], x_ccs: &[NTT]) -> Result<(), HipError> {
        let p = self.ctx.params()?;
        assert_eq!(w_ccs.len(), p.wit_len as usize);
        assert_eq!(x_ccs.len(), p.l as usize);
        let (words, x) = (flatten(w_ccs).into_boxed_slice(), flatten(x_ccs));
        // SAFETY: `words` lives in self until the prove that consumes it (or Drop) has returned; x is copied by the call
        let rc = unsafe { raw::lf_prover_ingest(self.raw, words.as_ptr(), x.as_ptr()) };
        // (a refused ingest has dropped the instance that was pending: the library holds none of the older words any more)
        self.pending_words = if rc == sys::LF_OK { Some(words) } else { None };
        self.chk(rc, "lf_prover_ingest")
    }

    /// the same from device memory (blocking, as `lf_witness_from_w_ccs_dev`)
    ///
    /// # Safety
    /// `w_ccs_dev` (wit_len elements) must stay allocated and unwritten until the call returns.
    pub unsafe fn ingest_dev(&mut self, w_ccs_dev: *const u64, x_ccs: &[NTT]) -> Result<(), HipError> {
        assert_eq!(x_ccs.len(), self.ctx.params()?.l as usize);
        let x = flatten(x_ccs);
        // SAFETY: the caller vouches for the device range
        let rc = unsafe { raw::lf_prover_ingest_dev(self.raw, w_ccs_dev, x.as_ptr()) };
        self.pending_words = None;
        self.chk(rc, "lf_prover_ingest_dev")
    }

    /// R_CCCS of the pending instance: `(failing components: OR of LF_REL_{CCS,NORM}, first bad row)`; `(0, m)` when it holds
    pub fn check_fresh(&mut self, bound: u64) -> Result<(u32, u64), HipError> {
        let (mut failed, mut first_bad) = (0u32, 0u64);
        // SAFETY: plain out-parameters
        let rc = unsafe { raw::lf_prover_check_fresh(self.raw, bound, &mut failed, &mut first_bad) };
        if rc != sys::LF_ERR_REJECT {
            if rc != sys::LF_OK { self.pending_words = None; }
            self.chk(rc, "lf_prover_check_fresh")?;
        }
        Ok((failed, first_bad))
    }

    /// `NIFSProver::prove` of (accumulator, pending instance): `(fresh CCCS, folded LCCCS, proof)`; the folded pair becomes the accumulator
    pub fn prove(&mut self, transcript: &mut impl TranscriptWithShortChallenges<NTT>) -> Result<(CCCS<NTT>, LCCCS<NTT>, LFProof<NTT>), HipError> {
        let p = self.ctx.params()?;
        let tr = as_hip::<NTT, _>(transcript)?;
        let (lin, dec, fold) = section_lens::<NTT>(&p);
        // SAFETY: p is a live parameter block
        let (ll, cl) = unsafe { (sys::lf_lcccs_len_ring(&p, ring_id::<NTT>()?), sys::lf_cccs_len_ring(&p, ring_id::<NTT>()?)) };
        let (mut cc, mut lc, mut pr) = (vec![0u64; cl * NTT::WORDS], vec![0u64; ll * NTT::WORDS], vec![0u64; (lin + 2 * dec + fold) * NTT::WORDS]);
        // SAFETY: output lengths per include/lfhip.h (lf_cccs_len_ring / lf_lcccs_len_ring / lf_proof_len_ring)
        let rc = unsafe { raw::lf_prover_prove(self.raw, tr, cc.as_mut_ptr(), lc.as_mut_ptr(), pr.as_mut_ptr()) };
        self.pending_words = None;   // consumed, or dropped by the refusal
        self.chk(rc, "lf_prover_prove")?;
        let e: Vec<NTT> = unflatten(&pr);
        let proof = LFProof {
            linearization_proof: lin_proof_from(&e[..lin], &p),
            decomposition_proof_l: dec_proof_from(&e[lin..lin + dec], &p),
            decomposition_proof_r: dec_proof_from(&e[lin + dec..lin + 2 * dec], &p),
            folding_proof: fold_proof_from(&e[lin + 2 * dec..], &p),
        };
        let c: Vec<NTT> = unflatten(&cc);
        let k = p.kappa as usize;
        Ok((CCCS { cm: Commitment::from(c[..k].to_vec()), x_ccs: c[k..].to_vec() }, lcccs_from(&lc, &p), proof))
    }

    /// the accumulator: `(LCCCS, f in NTT form)`
    pub fn accumulator(&mut self) -> Result<(LCCCS<NTT>, Vec<NTT>), HipError> {
        let p = self.ctx.params()?;
        // SAFETY: p is a live parameter block
        let ll = unsafe { sys::lf_lcccs_len_ring(&p, ring_id::<NTT>()?) };
        let (mut lc, mut f) = (vec![0u64; ll * NTT::WORDS], vec![0u64; (p.wit_len * p.L) as usize * NTT::WORDS]);
        // SAFETY: output lengths per include/lfhip_prover.h
        let rc = unsafe { raw::lf_prover_accumulator(self.raw, lc.as_mut_ptr(), f.as_mut_ptr()) };
        self.chk(rc, "lf_prover_accumulator")?;
        Ok((lcccs_from(&lc, &p), unflatten(&f)))
    }

    /// the same with f written into device memory (N elements)
    ///
    /// # Safety
    /// `f_dev_out` must be N elements of device memory of the context's device that nobody else touches until the call returns.
    pub unsafe fn accumulator_dev(&mut self, f_dev_out: *mut u64) -> Result<LCCCS<NTT>, HipError> {
        let p = self.ctx.params()?;
        // SAFETY: p is a live parameter block
        let ll = unsafe { sys::lf_lcccs_len_ring(&p, ring_id::<NTT>()?) };
        let mut lc = vec![0u64; ll * NTT::WORDS];
        // SAFETY: the caller vouches for the device range
        let rc = unsafe { raw::lf_prover_accumulator_dev(self.raw, lc.as_mut_ptr(), f_dev_out) };
        self.chk(rc, "lf_prover_accumulator_dev")?;
        Ok(lcccs_from(&lc, &p))
    }

    /// the decider: R_LCCCS of the accumulator -> failing components (OR of LF_REL_{CM,U,V,NORM}); 0 when it holds.  Read-only
    pub fn decide(&mut self, bound: u64) -> Result<u32, HipError> {
        let mut failed = 0u32;
        // SAFETY: plain out-parameter
        let rc = unsafe { raw::lf_prover_decide(self.raw, bound, &mut failed) };
        if rc != sys::LF_ERR_REJECT {
            self.chk(rc, "lf_prover_decide")?;
        }
        Ok(failed)
    }

    /// proves since `init` / `resume`
    pub fn steps(&self) -> u64 {
        // SAFETY: raw is a live handle
        unsafe { raw::lf_prover_steps(self.raw) }
    }
}

impl<'ctx, NTT, P> Drop for HipChainProver<'ctx, NTT, P> {
    fn drop(&mut self) {
        // SAFETY: raw came from lf_prover_create and is destroyed exactly once; the call joins a pending job before `pending_words` goes
        unsafe { raw::lf_prover_destroy(self.raw) }
    }
}
