//! `GpuVerifier`: `kimchi::verifier::batch_verify` (kimchi/src/verifier.rs:1275-1373) as ONE call into `libkimchi_hip.so` (`kh_batch_verify`, the host
//! loop in C++ over the library's own entry points: Fiat-Shamir replay, public commitment, the linearisation's constant term on the device, the scalars
//! of `SRS::verify`, one MSM for the whole batch).  The verifier index is the one the library built with the prover index (`kh_verifier_index_of`), so a
//! `GpuVerifier` is made from a `GpuProver`; the proofs go in as the reference's `ProverProof` values, laid out as the sections `kh_proof_section` gives.
//!
//! STATUS: EXPERIMENTAL, NEVER COMPILED, like `prover.rs`: the image this repository is built in has no Rust toolchain.  Every `sys::` call is in the C
//! header (tests/test_verify_abi.py checks the generated `-sys` crate); treat the rest as the shim a maintainer starts from, with `cargo check` against
//! the proof-systems workspace as the first step.
use crate::{limbs, pack, prover::GpuProver, HipCurve};
use ark_ff::PrimeField;
use kimchi::proof::{PointEvaluations, ProverProof};
use kimchi_hip_sys as sys;
use poly_commitment::{commitment::PolyComm, ipa::OpeningProof};
use std::ffi::CStr;

pub struct GpuVerifier<G: HipCurve> {
    index: *mut sys::kh_verifier_index_t,
    _marker: core::marker::PhantomData<G>,
}
unsafe impl<G: HipCurve> Send for GpuVerifier<G> {}
unsafe impl<G: HipCurve> Sync for GpuVerifier<G> {}
impl<G: HipCurve> Drop for GpuVerifier<G> {
    fn drop(&mut self) {
        unsafe { sys::kh_verifier_index_free(self.index) }
    }
}

/// Owns a `kh_proof_t` made by `kh_proof_from_sections` until the batch has been verified.
struct ProofGuard(*mut sys::kh_proof_t);
impl Drop for ProofGuard {
    fn drop(&mut self) {
        unsafe { sys::kh_proof_free(self.0) }
    }
}

fn last_error() -> String {
    unsafe { CStr::from_ptr(sys::kh_last_error()) }.to_string_lossy().into_owned()
}

/// One proof's data in the wire format, alive while its `kh_section_t` records point into it.
struct Sections {
    points: Vec<(i32, Vec<u64>, Vec<u8>)>,
    elems: Vec<(i32, Vec<u64>)>,
}

impl<G: HipCurve> GpuVerifier<G>
where
    G::BaseField: PrimeField,
{
    /// The verifier index of the circuit `prover` was made for (a copy: it outlives the prover, not the SRS handle).  The index must come from
    /// `GpuProver::from_gates` (`kh_prover_index_create(_lookup)`); one built from the caller's columns carries no commitments.
    pub fn from_prover(prover: &GpuProver<G>) -> Result<Self, String> {
        let mut index = core::ptr::null_mut();
        let rc = unsafe { sys::kh_verifier_index_of(prover.index_handle(), &mut index) };
        if rc != sys::KH_OK {
            return Err(last_error());
        }
        Ok(GpuVerifier { index, _marker: core::marker::PhantomData })
    }

    fn sections(proof: &ProverProof<G, OpeningProof<G>>) -> Sections {
        let comm = |c: &PolyComm<G>| c.chunks.clone();
        let scalars = |v: &[G::ScalarField]| unsafe { core::slice::from_raw_parts(limbs(v), 4 * v.len()) }.to_vec();
        let mut points = Vec::new();
        let mut put = |s: i32, pts: Vec<G>| {
            let (xy, inf) = pack::<G>(&pts);
            points.push((s, xy, inf));
        };
        let c = &proof.commitments;
        put(sys::KH_PROOF_W_COMM, c.w_comm.iter().flat_map(comm).collect());
        put(sys::KH_PROOF_Z_COMM, comm(&c.z_comm));
        put(sys::KH_PROOF_T_COMM, comm(&c.t_comm));
        if let Some(l) = &c.lookup {
            put(sys::KH_PROOF_LOOKUP_SORTED_COMM, l.sorted.iter().flat_map(comm).collect());
            put(sys::KH_PROOF_LOOKUP_AGGREG_COMM, comm(&l.aggreg));
            if let Some(r) = &l.runtime {
                put(sys::KH_PROOF_LOOKUP_RUNTIME_COMM, comm(r));
            }
        }
        put(sys::KH_PROOF_LR, proof.proof.lr.iter().flat_map(|(l, r)| [*l, *r]).collect());
        put(sys::KH_PROOF_DELTA, vec![proof.proof.delta]);
        put(sys::KH_PROOF_SG, vec![proof.proof.sg]);
        // KH_PROOF_EVALS: the opening order (kimchi_hip.h): z, the six selectors, w, coefficients, s, the optional selectors present, then the lookup
        // polynomials: sorted ..., aggregation, table, [runtime table, runtime selector], the pattern selectors present
        let e = &proof.evals;
        let mut cols: Vec<&PointEvaluations<Vec<G::ScalarField>>> =
            vec![&e.z, &e.generic_selector, &e.poseidon_selector, &e.complete_add_selector, &e.mul_selector, &e.emul_selector, &e.endomul_scalar_selector];
        cols.extend(e.w.iter());
        cols.extend(e.coefficients.iter());
        cols.extend(e.s.iter());
        let optional = [&e.range_check0_selector, &e.range_check1_selector, &e.foreign_field_add_selector, &e.foreign_field_mul_selector, &e.xor_selector, &e.rot_selector];
        cols.extend(optional.into_iter().flatten());
        cols.extend(e.lookup_sorted.iter().flatten());
        let lookups = [&e.lookup_aggregation, &e.lookup_table, &e.runtime_lookup_table, &e.runtime_lookup_table_selector, &e.xor_lookup_selector,
                       &e.lookup_gate_lookup_selector, &e.range_check_lookup_selector, &e.foreign_field_mul_lookup_selector];
        cols.extend(lookups.into_iter().flatten());
        let mut flat = Vec::new();
        for c in cols {
            flat.extend(scalars(&c.zeta));
            flat.extend(scalars(&c.zeta_omega));
        }
        let mut elems = vec![(sys::KH_PROOF_EVALS, flat), (sys::KH_PROOF_FT_EVAL1, scalars(&[proof.ft_eval1])), (sys::KH_PROOF_Z1_Z2, scalars(&[proof.proof.z1, proof.proof.z2]))];
        if let Some(p) = &e.public {
            let mut v = scalars(&p.zeta);
            v.extend(scalars(&p.zeta_omega));
            elems.push((sys::KH_PROOF_PUBLIC_EVALS, v));
        }
        Sections { points, elems }
    }

    /// `batch_verify` for proofs of this index: `Ok(true)` if all are accepted, `Ok(false)` if one is rejected, `Err` with the library's text (it names
    /// the item and the check) for a malformed proof -- the reference's `VerifyError` cases that are about shape, not validity.
    pub fn verify(&self, proofs: &[(&ProverProof<G, OpeningProof<G>>, &[G::ScalarField])]) -> Result<bool, String> {
        const NSEC: usize = sys::KH_PROOF_LOOKUP_RUNTIME_COMM as usize + 1;
        let data: Vec<Sections> = proofs.iter().map(|(p, _)| Self::sections(p)).collect();
        let mut handles = Vec::with_capacity(proofs.len());
        for d in &data {
            let mut secs = [sys::kh_section_t { limbs: core::ptr::null(), flags: core::ptr::null(), count: 0 }; NSEC];
            for (s, xy, inf) in &d.points {
                secs[*s as usize] = sys::kh_section_t { limbs: xy.as_ptr(), flags: inf.as_ptr(), count: inf.len() };
            }
            for (s, v) in &d.elems {
                secs[*s as usize] = sys::kh_section_t { limbs: v.as_ptr(), flags: core::ptr::null(), count: v.len() / 4 };
            }
            let mut h = core::ptr::null_mut();
            if unsafe { sys::kh_proof_from_sections(secs.as_ptr(), NSEC, &mut h) } != sys::KH_OK {
                return Err(last_error());
            }
            handles.push(ProofGuard(h));
        }
        // the previous challenges of each proof, as for kh_prove_recursive: challenges concatenated, rounds, commitment chunks concatenated
        let prev: Vec<(Vec<u64>, Vec<u32>, Vec<u64>, Vec<u8>, Vec<usize>)> = proofs
            .iter()
            .map(|(p, _)| {
                let (mut chals, mut rounds, mut pts, mut chunks) = (Vec::new(), Vec::new(), Vec::new(), Vec::new());
                for rc in &p.prev_challenges {
                    chals.extend(unsafe { core::slice::from_raw_parts(limbs(&rc.chals), 4 * rc.chals.len()) });
                    rounds.push(rc.chals.len() as u32);
                    pts.extend(rc.comm.chunks.iter().copied());
                    chunks.push(rc.comm.chunks.len());
                }
                let (xy, inf) = pack::<G>(&pts);
                (chals, rounds, xy, inf, chunks)
            })
            .collect();
        let items: Vec<sys::kh_verify_item_t> = proofs
            .iter()
            .zip(&handles)
            .zip(&prev)
            .map(|(((_, public), h), (chals, rounds, xy, inf, chunks))| sys::kh_verify_item_t {
                index: self.index,
                proof: h.0,
                public_inputs: limbs(public),
                n_public: public.len(),
                prev_chals: chals.as_ptr(),
                prev_rounds: rounds.as_ptr(),
                prev_comm_xy: xy.as_ptr(),
                prev_comm_inf: inf.as_ptr(),
                prev_comm_chunks: chunks.as_ptr(),
                n_prev: chunks.len(),
            })
            .collect();
        let mut accepted = 0i32;
        let rc = unsafe { sys::kh_batch_verify(items.as_ptr(), items.len(), core::ptr::null(), &mut accepted, core::ptr::null_mut()) };
        if rc != sys::KH_OK {
            return Err(last_error());
        }
        Ok(accepted == 1)
    }
}
