"""The ABI of the MockProver session (ZK_ABI_VERSION 8): the four entry points are exported, zk_abi_struct_size knows zk_mock_witness and zk_mock_info, and their ctypes
and Rust mirrors (zk_dcap_verifier_amd._lib, shim/halo2_proofs_mi355x/src/mock_session.rs) follow include/zkmi355.h field for field.  The two structs are declared
apart from their typedefs, like zk_mock_desc, so they are brought into the form tests/test_shim_abi.py's parser reads first (tests/test_mock_prover_native.py does
the same for the one-shot structs)."""
import ctypes as C
import os
import re

import pytest

import test_shim_abi as sa
from conftest import EMU_SO, ROOT
from zk_dcap_verifier_amd import _lib

FUNCTIONS = ("zk_mock_prover_open", "zk_mock_prover_check", "zk_mock_prover_info", "zk_mock_prover_close")
STRUCTS = {"zk_mock_witness": _lib.MockWitness, "zk_mock_info": _lib.MockInfo}


def _header():
    hdr = open(sa.HEADER).read()
    for name in STRUCTS:
        assert f"typedef struct {name} {name};" in hdr
        hdr = hdr.replace(f"typedef struct {name} {name};", "")
        hdr = re.sub(r"\bstruct %s \{(.*?)\};" % name, lambda m: "typedef struct %s {%s} %s;" % (name, m.group(1), name), hdr, flags=re.S)
    return hdr


def _sysv_size(fields):
    off, align = 0, 1
    for _, (base, ptrs) in fields:
        sz = 8 if ptrs or base in ("u64", "usize", "f64") else 4
        off = (off + sz - 1) // sz * sz + sz
        align = max(align, sz)
    return (off + align - 1) // align * align


def test_header_declares_version_8_and_the_session():
    hdr = open(sa.HEADER).read()
    assert int(re.search(r"#define\s+ZK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8 == _lib.ABI_VERSION
    structs, _, protos = sa.parse_header(_header())
    assert set(FUNCTIONS) <= set(protos)
    for name, mirror in STRUCTS.items():
        assert structs[name][0] == ("struct_size", ("u32", [])), name
        assert [n for n, _ in structs[name]] == [n for n, _ in mirror._fields_]
        assert _sysv_size(structs[name]) == C.sizeof(mirror)
    # open takes the one-shot descriptor; check returns the one-shot records
    assert protos["zk_mock_prover_open"][1][1] == ("zk_mock_desc", ["const"])
    assert protos["zk_mock_prover_check"][1][3] == ("zk_mock_failure", ["mut"])


@pytest.mark.parametrize("which", ["product", "emulator"])
def test_library_exports_the_session(built, which):
    import zk_dcap_verifier_amd as z
    lib = C.CDLL(z.LIB_PATH if which == "product" else EMU_SO)
    lib.zk_abi_version.restype = C.c_uint32
    lib.zk_abi_struct_size.restype = C.c_uint32
    assert lib.zk_abi_version() == 8
    for fn in FUNCTIONS:
        assert hasattr(lib, fn), fn
    for name, mirror in STRUCTS.items():
        assert lib.zk_abi_struct_size(name.encode()) == C.sizeof(mirror), name


def test_rust_session_bindings_match_the_header():
    rs = open(os.path.join(ROOT, "shim", "halo2_proofs_mi355x", "src", "mock_session.rs")).read()
    rs_plain = re.sub(r"#\[repr\(C\)\]\s*#\[derive\([^\]]*\)\]", "#[repr(C)]", rs)
    structs, externs, _, _ = sa.parse_rust(rs_plain)
    assert {"ZkMockWitness", "ZkMockInfo"} <= set(structs) and set(FUNCTIONS) <= set(externs)
    hdr = _header()
    for name in ("zk_mock_desc", "zk_mock_failure"):
        hdr = hdr.replace(f"typedef struct {name} {name};", "")
        hdr = re.sub(r"\bstruct %s \{(.*?)\};" % name, lambda m: "typedef struct %s {%s} %s;" % (name, m.group(1), name), hdr, flags=re.S)
    bad = sa.diff_against_header(rs_plain, "mock_session.rs", header_text=hdr + "\n" + open(sa.RCCL_HEADER).read())
    assert not bad, "\n".join(bad)
    # a field dropped from the Rust struct, or an argument from a prototype, is reported
    assert any("ZkMockWitness fields" in b for b in sa.diff_against_header(rs_plain.replace("    pub values_on_device: u32,\n    pub challenges", "    pub challenges", 1), "cut", header_text=hdr))
    assert any("zk_mock_prover_check" in b for b in sa.diff_against_header(rs_plain.replace("mp: u64, w: *const ZkMockWitness, ", "w: *const ZkMockWitness, ", 1), "cut", header_text=hdr))
    # the binding asserts both sizes at start-up, against the version it was written for
    mi = open(os.path.join(ROOT, "shim", "halo2_proofs_mi355x", "src", "mi355x.rs")).read()
    assert "zk_mock_witness\\0" in mi and "zk_mock_info\\0" in mi and "ZK_ABI_VERSION: u32 = 8;" in mi


@pytest.mark.gpu
def test_product_library_reports_the_session_structs_gpu(gpu):
    assert gpu.lib.zk_abi_version() == 8
    for name, mirror in STRUCTS.items():
        assert gpu.lib.zk_abi_struct_size(name.encode()) == C.sizeof(mirror)
