//! One-call form of the integration: `create_proof` hands the whole proof to `zk_plonk_prove_phased` (include/zkmi355.h; csrc/prover.hip) — every circuit of its slice,
//! every advice phase: for a circuit with `advice_column_in(SecondPhase)` / `challenge_usable_after` the library calls back (`next_phase`) once the challenges of a
//! phase exist and the closure re-runs synthesis with the challenge map, exactly where halo2's own phase loop does.  A single-phase key takes zk_plonk_prove_phased's path.
//! `mod create_proof_native;` next to `mod mi355x;` and `mod pk_desc;` — hooked into plonk/prover.rs by prover_native.patch, INSIDE create_proof right after
//! witness synthesis of EVERY circuit (`batch_invert_assigned`), because that is where the advice columns exist and nothing random has been drawn yet:
//!
//!     if let Some(done) = crate::create_proof_native::try_create_proof::<Scheme, E, R, T, _>(params, pk, instances, &native_advice, &mut resynthesize, &mut rng, transcript) {
//!         return done;          // Ok(()) with the proof written into `transcript`, or the Err the CPU body would have returned
//!     }
//!
//! Guards (any failing -> None -> the original body continues, draw for draw, as if the hook were absent):
//!   * the scheme is KZG over bn256 (TypeId of the params type) and HALO2_MI355X != 0 and a gfx950 context exists;
//!   * any number of circuit instances (the reference passes `&[circuit]`, circuits/src/sgx_dcap_verifier.rs:814-822; m circuits become ONE proof, as on the CPU)
//!     with advice in up to three phases and the Challenge API (pk_desc::key_for builds a phased key for those);
//!   * the transcript is `Blake2bWrite<_, G1Affine, Challenge255<_>>` (by type name: the library hashes with Blake2b / Challenge255 itself) and NOTHING has been
//!     absorbed since `init` except what create_proof absorbed (vk, instances) — the library re-absorbs those, then every commitment and evaluation;
//!   * n >= 2^12.
//! The proof comes back as bytes; `replay` feeds them through the caller's transcript (write_point / write_scalar, and a squeeze wherever create_proof squeezes),
//! so the writer holds the same bytes AND the same hash state as after the CPU body — for any `W: Write`, without touching Blake2bWrite's private fields.  Every
//! challenge the replay squeezes is compared with what the library squeezed (zk_plonk_last_challenges): the first mismatch is Error::Transcript.
//! `R: Send`: zk_plonk_prove_phased calls the draw callback from a helper thread of the library (so that the draws of phase p + 1 overlap the kernels of phase p) while the
//! calling thread blocks — the exclusive borrow travels to that thread and back, which is exactly what `Send` licenses.  OsRng (what the reference passes,
//! sgx_dcap_verifier.rs:819) and every seedable rng are Send; create_proof's own bound becomes `R: RngCore + Send` in prover_native.patch (a ThreadRng caller
//! wraps it or keeps the CPU prover).
//! Witness synthesis (`WitnessCollection`, plonk/prover.rs) stays the CPU code it is.  Uncompiled in the build image (no rustc there).
use std::any::{type_name, TypeId};
use std::ffi::c_void;
use std::os::raw::c_int;

use ff::{Field, PrimeField};
use group::GroupEncoding;
use halo2curves::bn256::{Bn256, Fr, G1Affine};
use halo2curves::CurveAffine;
use rand_core::RngCore;

use crate::mi355x::{gpu, ZkCtx, MIN_LEN};
use crate::plonk::{Error, ProvingKey};
use crate::poly::commitment::{CommitmentScheme, Params};
use crate::poly::kzg::commitment::ParamsKZG;
use crate::poly::{LagrangeCoeff, Polynomial};
use crate::transcript::{EncodedChallenge, TranscriptWrite};

use crate::mi355x::{zk_plonk_last_challenges, zk_plonk_prove_phased};

/// What the library's callback needs: the caller's re-synthesis, the columns it returned (alive until the proof is done) and the first error it reported.
struct PhaseState<'a, S> {
    synthesize: &'a mut S,
    n_circuits: usize, n_advice: usize,
    advice_phase: Vec<u8>, challenge_phase: Vec<u8>,
    kept: Vec<Polynomial<Fr, LagrangeCoeff>>,
    error: Option<Error>,
}

/// zk_phase_fn: `challenges` holds n_challenges Montgomery values (Fr's memory layout), zero where not yet squeezed; the closure gets halo2's challenge map (index ->
/// value, the challenges of phases before `phase`) and returns circuit c's columns of `phase` as (column index, values) after batch_invert_assigned, blinding rows
/// not yet filled.  Runs on the thread that called zk_plonk_prove_phased, no library lock held.  Non-zero = the proof ends with ZK_ERR_ARG.
unsafe extern "C" fn next_phase<S>(user: *mut c_void, phase: u32, challenges: *const c_void, n_challenges: u32, advice: *mut *const c_void) -> c_int
where S: FnMut(usize, u8, &std::collections::HashMap<usize, Fr>) -> Result<Vec<(usize, Polynomial<Fr, LagrangeCoeff>)>, Error> {
    let st = &mut *(user as *mut PhaseState<S>);
    let all = std::slice::from_raw_parts(challenges as *const Fr, n_challenges as usize);
    let map: std::collections::HashMap<usize, Fr> = all.iter().enumerate().filter(|(i, _)| (st.challenge_phase[*i] as u32) < phase).map(|(i, v)| (i, *v)).collect();
    for c in 0..st.n_circuits {
        match (st.synthesize)(c, phase as u8, &map) {
            Ok(columns) => for (index, values) in columns {
                if index >= st.n_advice || st.advice_phase[index] as u32 != phase { return 2; }
                *advice.add(c * st.n_advice + index) = values.as_ptr() as *const c_void;
                st.kept.push(values);                                 // (a Polynomial's buffer does not move when the Polynomial does)
            },
            Err(e) => { st.error = Some(e); return 1; }
        }
    }
    0
}

/// `Fr::random(&mut rng)` n times, written as the 4 x u64 Montgomery limbs Fr is in memory (layout asserted by mi355x::gpu()).  The library calls this from
/// ONE helper thread, block by block, in halo2's own order (zk_plonk_pk_desc.draw_schedule = 1: blinding rows, the Blind of every commitment, the random
/// polynomial, the h-piece Blinds) and has made every draw when zk_plonk_prove_phased returns: `rng` is left exactly where the CPU body would leave it.
extern "C" fn draw<R: RngCore + Send>(user: *mut c_void, n: usize, out_fr: *mut c_void) {
    let rng = unsafe { &mut *(user as *mut R) };
    let out = unsafe { std::slice::from_raw_parts_mut(out_fr as *mut Fr, n) };
    for v in out.iter_mut() {
        *v = Fr::random(&mut *rng);
    }
}

/// Proof layout of create_proof + ProverSHPLONK: commitments per phase, then the evaluations, then SHPLONK's two points.  Over m circuits every
/// per-circuit count is m times the circuit's (the points of a phase and the evaluations come circuit by circuit; replay only needs the counts).
struct Layout { advice: usize, lookups: usize, sets: usize, pieces: usize, evals: usize,
                /// per advice phase: the commitments of the phase (all circuits) and the user challenges squeezed after them; their sum over the phases is `advice`
                phases: Vec<(usize, usize)>, n_challenges: usize }

/// Feed `proof` through the caller's transcript exactly as the CPU body would have: write the phase's points, squeeze where create_proof squeezes.
/// Generic over the curve (only trait methods are used), so no reinterpretation of the transcript is needed: C is G1Affine by the caller's TypeId guard.
/// `squeezed`: zk_plonk_last_challenges of the proof — the user challenges in index order, then theta, beta, gamma, y, x, SHPLONK's y, v, u — as canonical bytes;
/// `user_order`: the indices of the user challenges in the order the transcript squeezes them (phase by phase, ascending index within a phase).
fn replay<C: CurveAffine, E: EncodedChallenge<C>, T: TranscriptWrite<C, E>>(t: &mut T, proof: &[u8], l: &Layout, squeezed: &[[u8; 32]], user_order: &[usize]) -> Result<(), Error> {
    let bad = |what: &str| Error::Transcript(std::io::Error::new(std::io::ErrorKind::Other, format!("mi355x: bad {what} in the returned proof")));
    // a challenge of the caller's transcript against the library's: the two hashed the same bytes, so a difference means the transcripts diverged (another
    // personalisation, something absorbed before the hook): the proof would not verify — refuse it here
    let mut check = |t: &mut T, slot: usize, what: &str| -> Result<(), Error> {
        let c: C::Scalar = *t.squeeze_challenge_scalar::<()>();
        if squeezed.get(slot).map(|b| &b[..]) != Some(c.to_repr().as_ref()) {
            return Err(Error::Transcript(std::io::Error::new(std::io::ErrorKind::Other, format!("mi355x: challenge {what} differs from the library's"))));
        }
        Ok(())
    };
    let fixed_at = l.n_challenges;                                   // theta's slot
    let mut at = 0usize;
    let mut point = |t: &mut T| -> Result<(), Error> {
        let mut repr = <C as GroupEncoding>::Repr::default();
        repr.as_mut().copy_from_slice(&proof[at..at + 32]);
        at += 32;
        let p: C = Option::from(C::from_bytes(&repr)).ok_or_else(|| bad("point"))?;
        t.write_point(p).map_err(Error::from)
    };
    let mut next_user = user_order.iter();
    for (points, challenges) in l.phases.iter() {                    // advice, phase by phase: the phase's commitments, then its challenges
        for _ in 0..*points { point(t)?; }
        for _ in 0..*challenges { check(t, *next_user.next().ok_or_else(|| bad("phase list"))?, "of an advice phase")?; }
    }
    check(t, fixed_at, "theta")?;
    for _ in 0..2 * l.lookups { point(t)?; }
    check(t, fixed_at + 1, "beta")?;
    check(t, fixed_at + 2, "gamma")?;
    for _ in 0..l.sets + l.lookups + 1 { point(t)?; }            // permutation products, lookup products, the vanishing argument's random polynomial
    check(t, fixed_at + 3, "y")?;
    for _ in 0..l.pieces { point(t)?; }
    check(t, fixed_at + 4, "x")?;
    drop(point);
    for _ in 0..l.evals {
        let mut repr = <C::Scalar as PrimeField>::Repr::default();
        repr.as_mut().copy_from_slice(&proof[at..at + 32]);
        at += 32;
        let s: C::Scalar = Option::from(C::Scalar::from_repr(repr)).ok_or_else(|| bad("scalar"))?;
        t.write_scalar(s).map_err(Error::from)?;
    }
    check(t, fixed_at + 5, "y of SHPLONK")?;
    check(t, fixed_at + 6, "v of SHPLONK")?;
    for _ in 0..2 {                                               // SHPLONK: h(X), squeeze u, the linearisation quotient
        let mut repr = <C as GroupEncoding>::Repr::default();
        repr.as_mut().copy_from_slice(&proof[at..at + 32]);
        at += 32;
        let p: C = Option::from(C::from_bytes(&repr)).ok_or_else(|| bad("point"))?;
        t.write_point(p).map_err(Error::from)?;
        if at + 32 == proof.len() { check(t, fixed_at + 7, "u of SHPLONK")?; }
    }
    debug_assert_eq!(at, proof.len());
    Ok(())
}

/// See the module comment.  `advice_values[c]`: circuit c's advice columns (all num_advice_columns of them) after the FIRST phase's synthesis and
/// batch_invert_assigned, blinding rows NOT yet filled — one entry per circuit of create_proof's `circuits` (one proof over all of them); the columns of later phases
/// are whatever synthesis left there and are not read.  `synthesize(circuit, phase, challenges)`: halo2's re-run of Circuit::synthesize for a later phase.
pub fn try_create_proof<Scheme, E, R, T, S>(params: &Scheme::ParamsProver, pk: &ProvingKey<Scheme::Curve>, instances: &[&[&[Scheme::Scalar]]],
                                            advice_values: &[Vec<Polynomial<Scheme::Scalar, LagrangeCoeff>>], synthesize: &mut S, rng: &mut R, transcript: &mut T) -> Option<Result<(), Error>>
where
    S: FnMut(usize, u8, &std::collections::HashMap<usize, Fr>) -> Result<Vec<(usize, Polynomial<Fr, LagrangeCoeff>)>, Error>,
    Scheme: CommitmentScheme + 'static,
    Scheme::ParamsProver: 'static,
    E: EncodedChallenge<Scheme::Curve>,
    R: RngCore + Send, // the library draws through `&mut R` on ITS helper thread while this thread blocks in zk_plonk_prove_phased: moving a `&mut R` across threads needs R: Send
    T: TranscriptWrite<Scheme::Curve, E>,
{
    if TypeId::of::<Scheme::ParamsProver>() != TypeId::of::<ParamsKZG<Bn256>>() || instances.is_empty() || advice_values.len() != instances.len() {
        return None;
    }
    let tn = type_name::<T>();
    if !(tn.contains("Blake2bWrite") && tn.contains("Challenge255")) {
        return None;
    }
    // Scheme::Curve == G1Affine and Scheme::Scalar == Fr from here on (the TypeId check): reinterpret the generic references
    let params: &ParamsKZG<Bn256> = unsafe { &*(params as *const _ as *const ParamsKZG<Bn256>) };
    let pk: &ProvingKey<G1Affine> = unsafe { &*(pk as *const _ as *const ProvingKey<G1Affine>) };
    let n = params.n() as usize;
    if n < MIN_LEN {
        return None;
    }
    let g = gpu()?;
    let key = crate::pk_desc::key_for(g, params, pk)?;
    let cs = &pk.vk.cs;
    if advice_values.iter().any(|a| a.len() != cs.num_advice_columns) || instances.iter().any(|i| i.len() != cs.num_instance_columns) {
        return None;
    }
    let m = instances.len();

    // every circuit's columns, circuit-major (halo2's own order of the circuits)
    let mut adv: Vec<*const c_void> = advice_values.iter().flat_map(|a| a.iter().map(|c| c.as_ptr() as *const c_void)).collect();
    // [3P-MEM] sealed::Phase(u8)
    let advice_phase: Vec<u8> = cs.advice_column_phase.iter().map(|p| p.0).collect();
    let challenge_phase: Vec<u8> = cs.challenge_phase.iter().map(|p| p.0).collect();
    let n_phases = advice_phase.iter().copied().max().unwrap_or(0) as usize + 1;
    let phases: Vec<(usize, usize)> = (0..n_phases).map(|p| (m * advice_phase.iter().filter(|q| **q as usize == p).count(), challenge_phase.iter().filter(|q| **q as usize == p).count())).collect();
    let mut user_order: Vec<usize> = (0..challenge_phase.len()).collect();
    user_order.sort_by_key(|i| (challenge_phase[*i], *i));
    let canon: Vec<Vec<[u8; 32]>> = instances.iter().flat_map(|i| i.iter())
        .map(|c| c.iter().map(|v| { let mut b = [0u8; 32]; b.copy_from_slice(v.to_repr().as_ref()); b }).collect()).collect();
    let inst: Vec<*const c_void> = canon.iter().map(|c| c.as_ptr() as *const c_void).collect();
    let lens: Vec<u32> = canon.iter().map(|c| c.len() as u32).collect();
    let chunk = cs.degree() - 2;
    let p = cs.permutation.get_columns().len();
    let layout = Layout {
        advice: m * cs.num_advice_columns, lookups: m * cs.lookups.len(), sets: m * ((p + chunk - 1) / chunk), pieces: cs.degree() - 1,
        evals: m * (cs.advice_queries.len() + (if p > 0 { 3 * ((p + chunk - 1) / chunk) - 1 } else { 0 }) + 5 * cs.lookups.len()) + cs.fixed_queries.len() + 1 + p,
        phases, n_challenges: challenge_phase.len(),
    };
    let mut state = PhaseState { synthesize, n_circuits: m, n_advice: cs.num_advice_columns, advice_phase, challenge_phase, kept: Vec::new(), error: None };
    let cap = 32 * (layout.advice + 2 * layout.lookups + layout.sets + layout.lookups + 1 + layout.pieces + layout.evals + 2);
    let mut proof = vec![0u8; cap];
    let mut len = 0usize;
    let rc = unsafe {
        zk_plonk_prove_phased(g.ctx, key, m as u32, adv.as_mut_ptr(), 0, inst.as_ptr(), lens.as_ptr(), Some(next_phase::<S>), &mut state as *mut _ as *mut c_void,
                              draw::<R>, rng as *mut R as *mut c_void, proof.as_mut_ptr() as *mut c_void, proof.len(), &mut len)
    };
    if let Some(e) = state.error.take() {
        return Some(Err(e));                                          // the caller's own synthesis error of a later phase, as the CPU body would have returned it
    }
    if rc != 0 {
        g.complain("zk_plonk_prove_phased");
        // ZK_ERR_ARG from the lookup phase = an input outside its table: the CPU body reports exactly that (Error::ConstraintSystemFailure) — but part of
        // `rng` has been consumed, so re-running the CPU body here would not reproduce a seeded proof.  Surface the error instead.
        return Some(Err(Error::ConstraintSystemFailure));
    }
    debug_assert_eq!(len, cap);
    proof.truncate(len);
    // (vk and the instance scalars were absorbed by create_proof before the hook; the library absorbed the same values on its side)
    // the challenges the library squeezed (this thread's last proof): replay compares every one of them with the caller's transcript
    let mut squeezed = vec![[0u8; 32]; layout.n_challenges + 8];
    let mut n_squeezed = 0usize;
    if unsafe { zk_plonk_last_challenges(squeezed.as_mut_ptr() as *mut c_void, squeezed.len() * 32, &mut n_squeezed) } != 0 || n_squeezed != squeezed.len() {
        g.complain("zk_plonk_last_challenges");
        return Some(Err(Error::Transcript(std::io::Error::new(std::io::ErrorKind::Other, "mi355x: the library reported no challenges for the proof"))));
    }
    Some(replay::<Scheme::Curve, E, T>(transcript, &proof, &layout, &squeezed, &user_order))
}
