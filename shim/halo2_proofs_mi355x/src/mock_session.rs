//! MockProver session: one circuit resident on the GPU, many witnesses checked against it - the declarations of `zk_mock_prover_open` / `_check` / `_info` /
//! `_close` (include/zkmi355.h, ZK_ABI_VERSION 8; csrc/mockprover.hip) and a safe wrapper.  `mod mock_session;` next to `mod mock_native;`; dev_native.patch files
//! one session per key, the way keygen_native.patch files its handle.  Uncompiled in the build image (no rustc there).
//!
//! Guards as mock_native::verify: HALO2_MI355X != 0 and a gfx950 context, n >= 2^12; any failing -> None -> the caller falls back to mock_native::verify or the CPU body.
use std::ffi::c_void;
use std::os::raw::c_int;

use crate::mi355x::{gpu, ZkCtx, MIN_LEN};
use crate::mock_native::{MockInput, ZkMockDesc, ZkMockFailure};

/// field-for-field `zk_mock_witness`: what changes from one check of a session to the next
#[repr(C)]
#[derive(Debug)]
pub struct ZkMockWitness {
    pub struct_size: u32, // size_of::<ZkMockWitness>()
    pub advice_values: *const *const c_void,
    pub instances: *const *const c_void,
    pub instance_lens: *const u32,
    pub values_on_device: u32,
    pub challenges: *const c_void,
    pub n_challenges: u32,
}

/// field-for-field `zk_mock_info`
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ZkMockInfo {
    pub struct_size: u32, // size_of::<ZkMockInfo>()
    pub n_tables: u32,
    pub n_resident_tables: u32,
    pub n_programs: u32,
    pub n_edges: u64,
    pub n_cells: u64,
    pub device_bytes: u64,
}

extern "C" {
    pub fn zk_mock_prover_open(ctx: *mut ZkCtx, desc: *const ZkMockDesc, mp: *mut u64) -> c_int;
    pub fn zk_mock_prover_check(ctx: *mut ZkCtx, mp: u64, w: *const ZkMockWitness, out: *mut ZkMockFailure, cap: usize, counts: *mut u64, n_written: *mut usize) -> c_int;
    pub fn zk_mock_prover_info(ctx: *mut ZkCtx, mp: u64, info: *mut ZkMockInfo) -> c_int;
    pub fn zk_mock_prover_close(ctx: *mut ZkCtx, mp: u64) -> c_int;
}

/// The circuit half of a `ZkMockDesc` (advice and instances NULL: zk_mock_prover_open ignores them).  The Vecs of pointers live as long as the returned closure's
/// borrow: build, call, drop.
fn with_desc<R>(inp: &MockInput, with_witness: bool, f: impl FnOnce(&ZkMockDesc) -> R) -> R {
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
        advice_values: if with_witness { inp.advice.as_ptr() } else { std::ptr::null() },
        instances: if with_witness { inst_ptrs.as_ptr() } else { std::ptr::null() },
        instance_lens: if with_witness { inst_lens.as_ptr() } else { std::ptr::null() },
        perm_map_column: inp.map_column.as_ptr(),
        perm_map_row: inp.map_row.as_ptr(),
        values_on_device: 0,
    };
    f(&d)
}

/// A circuit resident on the GPU (zk_mock_prover_open): its fixed columns, copy edges, compiled programs and sorted fixed-only tables.  dev_native.patch files one
/// per key - the way keygen_native files its handle - so that every later `MockProver::verify` of a circuit with that key pays for its kernels only.
pub struct MockSession {
    handle: u64,
    n_advice: usize,
    n_instance: usize,
}

impl MockSession {
    /// None when a guard fails or the library refuses the circuit (the CPU body then runs); `inp.advice` / `inp.instances` are not read
    pub fn open(inp: &MockInput) -> Option<MockSession> {
        let g = gpu()?;
        if (1usize << inp.k) < MIN_LEN {
            return None;
        }
        let mut handle = 0u64;
        if with_desc(inp, false, |d| unsafe { zk_mock_prover_open(g.ctx, d, &mut handle) }) != 0 {
            g.complain("zk_mock_prover_open");
            return None;
        }
        Some(MockSession { handle, n_advice: inp.advice.len(), n_instance: inp.instances.len() })
    }

    /// one witness: the records in MockProver's order and the exact counts, as `verify` returns them
    pub fn check(&self, advice: &[*const c_void], instances: &[Vec<[u8; 32]>], challenges: &[halo2curves::bn256::Fr]) -> Option<(Vec<ZkMockFailure>, [u64; 3])> {
        let g = gpu()?;
        if advice.len() != self.n_advice || instances.len() != self.n_instance {
            return None;
        }
        let inst_ptrs: Vec<*const c_void> = instances.iter().map(|c| c.as_ptr() as *const c_void).collect();
        let inst_lens: Vec<u32> = instances.iter().map(|c| c.len() as u32).collect();
        let w = ZkMockWitness {
            struct_size: std::mem::size_of::<ZkMockWitness>() as u32,
            advice_values: advice.as_ptr(),
            instances: inst_ptrs.as_ptr(),
            instance_lens: inst_lens.as_ptr(),
            values_on_device: 0,
            challenges: challenges.as_ptr() as *const c_void,
            n_challenges: challenges.len() as u32,
        };
        let mut counts = [0u64; 3];
        let mut written = 0usize;
        // first call: the counts (cap 0); second, only for a witness that fails: every record
        if unsafe { zk_mock_prover_check(g.ctx, self.handle, &w, std::ptr::null_mut(), 0, counts.as_mut_ptr(), &mut written) } != 0 {
            g.complain("zk_mock_prover_check");
            return None;
        }
        let total = (counts[0] + counts[1] + counts[2]) as usize;
        let mut out = vec![ZkMockFailure::default(); total];
        if total > 0 && unsafe { zk_mock_prover_check(g.ctx, self.handle, &w, out.as_mut_ptr(), total, counts.as_mut_ptr(), &mut written) } != 0 {
            g.complain("zk_mock_prover_check");
            return None;
        }
        out.truncate(written);
        Some((out, counts))
    }

    pub fn info(&self) -> Option<ZkMockInfo> {
        let g = gpu()?;
        let mut info = ZkMockInfo { struct_size: std::mem::size_of::<ZkMockInfo>() as u32, ..Default::default() };
        if unsafe { zk_mock_prover_info(g.ctx, self.handle, &mut info) } != 0 {
            return None;
        }
        Some(info)
    }
}

/// Sessions filed under their key, (params.g_lagrange address, vk.transcript_repr) - what keygen_native::remember files its handle under: the first
/// `MockProver::verify_with_session` of a key opens the session from its circuit, every later one finds it here.  `forget` closes it (Drop).
static SESSIONS: std::sync::Mutex<Vec<((usize, [u8; 32]), std::sync::Arc<MockSession>)>> = std::sync::Mutex::new(Vec::new());

pub fn session_for<'a>(key: (usize, [u8; 32]), circuit: impl FnOnce() -> MockInput<'a>) -> Option<std::sync::Arc<MockSession>> {
    let mut filed = SESSIONS.lock().ok()?;
    if let Some((_, s)) = filed.iter().find(|(k, _)| *k == key) {
        return Some(s.clone());
    }
    let s = std::sync::Arc::new(MockSession::open(&circuit())?);
    filed.push((key, s.clone()));
    Some(s)
}

pub fn forget(key: (usize, [u8; 32])) {
    if let Ok(mut filed) = SESSIONS.lock() {
        filed.retain(|(k, _)| *k != key);
    }
}

impl Drop for MockSession {
    fn drop(&mut self) {
        if let Some(g) = gpu() {
            unsafe { zk_mock_prover_close(g.ctx, self.handle) };
        }
    }
}
