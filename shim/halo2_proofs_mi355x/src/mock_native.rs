//! MockProver on the GPU: the declarations of `zk_mock_prover_verify` (include/zkmi355.h; csrc/mockprover.hip) and the translation of its records into
//! halo2's `VerifyFailure`s.  `mod mock_native;` next to `mod mi355x;`, hooked into dev.rs by dev_native.patch.  Uncompiled in the build image (no rustc there).
//!
//! Guards (any failing -> None -> the CPU body of MockProver::verify runs as before): HALO2_MI355X != 0 and a gfx950 context exists (mi355x::gpu());
//! n >= 2^12 (mi355x::MIN_LEN).  A circuit with user challenges passes the values halo2's MockProver derived (`MockInput::challenges`, zk_mock_prover_verify_phased).  Gate, lookup and permutation failures then come from the device; CellNotAssigned and the other checks of
//! the regions' metadata stay on the CPU body, which the patch runs with those three loops skipped.
use std::ffi::c_void;
use std::os::raw::c_int;

use crate::mi355x::{gpu, ZkCtx, MIN_LEN};

/// field-for-field `zk_mock_desc`
#[repr(C)]
#[derive(Debug)]
pub struct ZkMockDesc {
    pub struct_size: u32, // size_of::<ZkMockDesc>()
    pub k: u32,
    pub blinding_factors: u32,
    pub n_fixed: u32,
    pub n_advice: u32,
    pub n_instance: u32,
    pub n_lookups: u32,
    pub n_perm_columns: u32,
    pub perm_columns: *const u32,
    pub evaluator_zkq1: *const c_void,
    pub evaluator_zkq1_len: usize,
    pub lookup_input_zkq1: *const *const c_void,
    pub lookup_input_zkq1_len: *const usize,
    pub lookup_table_zkq1: *const *const c_void,
    pub lookup_table_zkq1_len: *const usize,
    pub fixed_values: *const *const c_void,
    pub advice_values: *const *const c_void,
    pub instances: *const *const c_void,
    pub instance_lens: *const u32,
    pub perm_map_column: *const u32,
    pub perm_map_row: *const u32,
    pub values_on_device: u32,
}

/// field-for-field `zk_mock_failure` (kind 0 gate, 1 lookup, 2 copy)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ZkMockFailure {
    pub kind: u32,
    pub index: u32,
    pub row: u32,
    pub other_column: u32,
    pub other_row: u32,
}

extern "C" {
    pub fn zk_mock_prover_verify(ctx: *mut ZkCtx, desc: *const ZkMockDesc, out: *mut ZkMockFailure, cap: usize, counts: *mut u64, n_written: *mut usize) -> c_int;
    pub fn zk_mock_prover_verify_phased(ctx: *mut ZkCtx, desc: *const ZkMockDesc, challenges: *const c_void, n_challenges: u32, out: *mut ZkMockFailure, cap: usize,
                                        counts: *mut u64, n_written: *mut usize) -> c_int;
}

/// What MockProver::verify owns, flattened for the call: the Evaluator / lookup blobs of the circuit's ConstraintSystem (evaluation_zkq1.rs), the columns as
/// assigned (Fr is its Montgomery limbs in memory), the instance values as canonical bytes and the permutation Assembly's mapping as two u32 planes.
pub struct MockInput<'a> {
    pub k: u32,
    pub blinding_factors: u32,
    pub perm_columns: &'a [u32],
    pub evaluator_zkq1: &'a [u8],
    pub lookup_inputs: &'a [Vec<u8>],
    pub lookup_tables: &'a [Vec<u8>],
    pub fixed: &'a [*const c_void],
    pub advice: &'a [*const c_void],
    pub instances: &'a [Vec<[u8; 32]>],
    pub map_column: &'a [u32],
    pub map_row: &'a [u32],
    /// MockProver's `challenges: Vec<F>` (Fr is its Montgomery limbs in memory); empty for a circuit without the Challenge API
    pub challenges: &'a [halo2curves::bn256::Fr],
}

/// All failures in MockProver's order (gates by (row, polynomial), lookups by (lookup, row), copies by (column, row)) and the exact counts, or None when a
/// guard fails or the library reports an error (the CPU body then runs).
pub fn verify(inp: &MockInput) -> Option<(Vec<ZkMockFailure>, [u64; 3])> {
    let g = gpu()?;
    if (1usize << inp.k) < MIN_LEN {
        return None;
    }
    let in_ptrs: Vec<*const c_void> = inp.lookup_inputs.iter().map(|b| b.as_ptr() as *const c_void).collect();
    let in_lens: Vec<usize> = inp.lookup_inputs.iter().map(|b| b.len()).collect();
    let tab_ptrs: Vec<*const c_void> = inp.lookup_tables.iter().map(|b| b.as_ptr() as *const c_void).collect();
    let tab_lens: Vec<usize> = inp.lookup_tables.iter().map(|b| b.len()).collect();
    let inst_ptrs: Vec<*const c_void> = inp.instances.iter().map(|c| c.as_ptr() as *const c_void).collect();
    let inst_lens: Vec<u32> = inp.instances.iter().map(|c| c.len() as u32).collect();
    let d = ZkMockDesc {
        struct_size: std::mem::size_of::<ZkMockDesc>() as u32,
        k: inp.k,
        blinding_factors: inp.blinding_factors,
        n_fixed: inp.fixed.len() as u32,
        n_advice: inp.advice.len() as u32,
        n_instance: inp.instances.len() as u32,
        n_lookups: inp.lookup_inputs.len() as u32,
        n_perm_columns: (inp.perm_columns.len() / 2) as u32,
        perm_columns: inp.perm_columns.as_ptr(),
        evaluator_zkq1: inp.evaluator_zkq1.as_ptr() as *const c_void,
        evaluator_zkq1_len: inp.evaluator_zkq1.len(),
        lookup_input_zkq1: in_ptrs.as_ptr(),
        lookup_input_zkq1_len: in_lens.as_ptr(),
        lookup_table_zkq1: tab_ptrs.as_ptr(),
        lookup_table_zkq1_len: tab_lens.as_ptr(),
        fixed_values: inp.fixed.as_ptr(),
        advice_values: inp.advice.as_ptr(),
        instances: inst_ptrs.as_ptr(),
        instance_lens: inst_lens.as_ptr(),
        perm_map_column: inp.map_column.as_ptr(),
        perm_map_row: inp.map_row.as_ptr(),
        values_on_device: 0,
    };
    let mut counts = [0u64; 3];
    let mut written = 0usize;
    let (ch, n_ch) = (inp.challenges.as_ptr() as *const c_void, inp.challenges.len() as u32);
    // first call: the counts (cap 0); second: every record
    if unsafe { zk_mock_prover_verify_phased(g.ctx, &d, ch, n_ch, std::ptr::null_mut(), 0, counts.as_mut_ptr(), &mut written) } != 0 {
        g.complain("zk_mock_prover_verify_phased");
        return None;
    }
    let total = (counts[0] + counts[1] + counts[2]) as usize;
    let mut out = vec![ZkMockFailure::default(); total];
    if total > 0 && unsafe { zk_mock_prover_verify_phased(g.ctx, &d, ch, n_ch, out.as_mut_ptr(), total, counts.as_mut_ptr(), &mut written) } != 0 {
        g.complain("zk_mock_prover_verify_phased");
        return None;
    }
    out.truncate(written);
    Some((out, counts))
}
