//! keygen_vk / keygen_pk on the GPU: the declarations of `zk_plonk_keygen_vk` / `_columns` / `_pk` / `_release` (include/zkmi355.h; csrc/pk.hip) and the two calls
//! keygen_native.patch hooks into plonk/keygen.rs.  `mod keygen_native;` next to `mod mi355x;`.  Uncompiled in the build image (no rustc there).
//!
//! What crosses the FFI: the fixed columns as keygen holds them after synthesis and selector compression (`Vec<Polynomial<Fr, LagrangeCoeff>>`: Fr is its Montgomery
//! limbs in memory) and the permutation Assembly's mapping as two u32 planes — the same planes mock_native.rs passes.  The library builds the sigma columns from the
//! mapping on the device (no `omega_powers` table, no host gather over n_perm_columns x 2^k cells), commits all columns in one batch and keeps them in HBM;
//! the key object of the first proof (pk_desc::key_for) is then built on those resident columns, so the Lagrange columns never cross the link a second time.
//!
//! Guards (any failing -> None -> the CPU body of keygen_vk / keygen_pk runs as before): HALO2_MI355X != 0 and a gfx950 context exists (mi355x::gpu());
//! n >= 2^12 (mi355x::MIN_LEN).  A library error is reported through Gpu::complain and also ends in None.
use std::collections::HashMap;
use std::ffi::c_void;
use std::os::raw::c_int;
use std::sync::Mutex;

use halo2curves::bn256::G1;

use crate::mi355x::{gpu, Gpu, ZkCtx, MIN_LEN};
use crate::pk_desc::{ZkPlonkPhases, ZkPlonkPkHost};

/// field-for-field `zk_plonk_keygen_desc`
#[repr(C)]
#[derive(Debug)]
pub struct ZkPlonkKeygenDesc {
    pub struct_size: u32, // size_of::<ZkPlonkKeygenDesc>()
    pub k: u32,
    pub n_fixed: u32,
    pub n_perm_columns: u32,
    pub fixed_values: *const *const c_void,
    pub perm_map_column: *const u32,
    pub perm_map_row: *const u32,
    pub values_on_device: u32,
}

extern "C" {
    pub fn zk_plonk_keygen_vk(ctx: *mut ZkCtx, desc: *const ZkPlonkKeygenDesc, srs_g_lagrange: u64, fixed_commitments: *mut c_void,
                              permutation_commitments: *mut c_void, kg: *mut u64) -> c_int;
    pub fn zk_plonk_keygen_columns(ctx: *mut ZkCtx, kg: u64, fixed_dev: *mut *const c_void, sigma_dev: *mut *const c_void) -> c_int;
    pub fn zk_plonk_keygen_pk(ctx: *mut ZkCtx, kg: u64, host: *const ZkPlonkPkHost, phases: *const ZkPlonkPhases, srs_g: u64, srs_g_lagrange: u64,
                              pk: *mut u64) -> c_int;
    pub fn zk_plonk_keygen_release(ctx: *mut ZkCtx, kg: u64) -> c_int;
}

/// What keygen_vk owns after synthesis, flattened for the call.
pub struct KeygenInput<'a> {
    pub k: u32,
    /// the fixed columns, selectors already compressed into them: 2^k Fr each
    pub fixed: &'a [*const c_void],
    /// `permutation::keygen::Assembly::mapping` as two planes, column-major: n_perm_columns x 2^k (mock_native.rs passes the same)
    pub map_column: &'a [u32],
    pub map_row: &'a [u32],
}

/// The commitments of keygen_vk — `fixed_commitments`, `permutation.commitments` as halo2curves G1 values (normalised: z = 1, or the identity) — and the handle
/// that keeps the Lagrange columns in HBM for `keygen_pk`.
pub struct KeygenVk {
    pub fixed_commitments: Vec<G1>,
    pub permutation_commitments: Vec<G1>,
    pub handle: u64,
}

/// (address of params.g_lagrange, transcript_repr bytes) -> keygen handle, from keygen_vk until the first proof with a ProvingKey of that vk: pk_desc::key_for takes
/// it out and builds the key on it.  Filed by VALUE of the vk, not by the address of any ProvingKey: keygen_pk returns its key by move and callers move it again, so no
/// address is stable before create_proof borrows it.  The columns stay in HBM meanwhile (the fixed and sigma columns once: 32 B x 2^k each); a circuit that is
/// keygen'd and never proved keeps them until pk_desc::forget, the next keygen_vk of the same (params, vk), or the end of the process.
static PENDING: Mutex<Option<HashMap<(usize, [u8; 32]), u64>>> = Mutex::new(None);

pub fn keygen_vk(g: &'static Gpu, srs_g_lagrange: u64, inp: &KeygenInput) -> Option<KeygenVk> {
    let n = 1usize << inp.k;
    if n < MIN_LEN {
        return None;
    }
    let m = inp.map_column.len() / n;
    debug_assert!(inp.map_column.len() == m * n && inp.map_row.len() == m * n);
    let d = ZkPlonkKeygenDesc {
        struct_size: std::mem::size_of::<ZkPlonkKeygenDesc>() as u32,
        k: inp.k,
        n_fixed: inp.fixed.len() as u32,
        n_perm_columns: m as u32,
        fixed_values: inp.fixed.as_ptr(),
        perm_map_column: inp.map_column.as_ptr(),
        perm_map_row: inp.map_row.as_ptr(),
        values_on_device: 0,
    };
    // G1 is {x, y, z} of 32-byte Montgomery limbs: the library's 96-byte normalised form (mi355x::gpu() asserts size_of::<G1>() == 96)
    let mut fixed_commitments = vec![G1::default(); inp.fixed.len()];
    let mut permutation_commitments = vec![G1::default(); m];
    let mut handle = 0u64;
    let rc = unsafe {
        zk_plonk_keygen_vk(g.ctx, &d, srs_g_lagrange, fixed_commitments.as_mut_ptr() as *mut c_void, permutation_commitments.as_mut_ptr() as *mut c_void, &mut handle)
    };
    if rc != 0 {
        g.complain("zk_plonk_keygen_vk");
        return None;
    }
    Some(KeygenVk { fixed_commitments, permutation_commitments, handle })
}

/// keygen_vk's hook remembers the handle under the vk it produced; key_for (same params, a ProvingKey whose vk has the same transcript_repr) takes it out again.
pub fn remember(params_g_lagrange: usize, transcript_repr: [u8; 32], handle: u64) {
    let mut guard = PENDING.lock().unwrap();
    if let Some(old) = guard.get_or_insert_with(HashMap::new).insert((params_g_lagrange, transcript_repr), handle) {
        if let Some(g) = gpu() {
            unsafe { zk_plonk_keygen_release(g.ctx, old) };
        }
    }
}
pub fn take(params_g_lagrange: usize, transcript_repr: [u8; 32]) -> Option<u64> {
    PENDING.lock().unwrap().as_mut()?.remove(&(params_g_lagrange, transcript_repr))
}

/// Release every pending handle of this vk, whatever params it was made with (pk_desc::forget).
pub fn forget(transcript_repr: [u8; 32]) {
    let (Some(g), Ok(mut guard)) = (gpu(), PENDING.lock()) else { return };
    if let Some(map) = guard.as_mut() {
        map.retain(|(_, repr), h| {
            if *repr == transcript_repr {
                unsafe { zk_plonk_keygen_release(g.ctx, *h) };
                false
            } else {
                true
            }
        });
    }
}

/// zk_plonk_keygen_pk on a remembered handle: `host` as pk_desc.rs fills it for zk_plonk_pk_build, with fixed_values / sigma_values null (the columns are the
/// handle's); `phases` None for a single-phase circuit.  The handle is released either way: the key shares the columns and keeps them alive.
pub fn keygen_pk(g: &'static Gpu, handle: u64, host: &ZkPlonkPkHost, phases: Option<&ZkPlonkPhases>, srs_g: u64, srs_g_lagrange: u64) -> Option<u64> {
    debug_assert!(host.fixed_values.is_null() && host.sigma_values.is_null());
    let mut key = 0u64;
    let rc = unsafe {
        zk_plonk_keygen_pk(g.ctx, handle, host, phases.map_or(std::ptr::null(), |p| p as *const ZkPlonkPhases), srs_g, srs_g_lagrange, &mut key)
    };
    unsafe { zk_plonk_keygen_release(g.ctx, handle) };
    if rc != 0 {
        g.complain("zk_plonk_keygen_pk");
        return None;
    }
    Some(key)
}
