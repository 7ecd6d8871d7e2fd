"""CPU: the C-ABI library loads and exports every symbol include/srganst.h declares, and the ctypes
signature table agrees with the header (names and argument counts).  No compute calls (no GPU here)."""
import ctypes
import os
import re

from conftest import ROOT


def header_decls():
    src = open(os.path.join(ROOT, "include", "srganst.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(sst_\w+)\s*\(([^)]*)\)\s*;", src):
        args = m.group(2).strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        decls[m.group(1)] = n
    return decls


def test_header_matches_ctypes_table_and_exports():
    from srganst import _abi
    decls = header_decls()
    assert len(decls) >= 35
    assert set(decls) == set(_abi.SIGNATURES), set(decls) ^ set(_abi.SIGNATURES)
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name, nargs in decls.items():
        assert hasattr(lib, name), f"{name} not exported by libsrganst.so"
        assert len(_abi.SIGNATURES[name][1]) == nargs, name


def test_library_identity_and_error_channel():
    from srganst import _abi
    lib = _abi.lib()
    assert lib.sst_arch() == b"gfx950" and lib.sst_version() >= 100
    # argument validation happens on the host before any launch: safe to exercise without a GPU
    rc = lib.sst_conv_fwd(None, None, None, None, None, None, None, None, 0.0, 0, None, None, None, 0, 1, 8, 8, 8, 8, 3, 1, None)
    assert rc != 0 and b"null pointer" in lib.sst_last_error()
    n = ctypes.c_int64()
    assert lib.sst_st_loss_workspace(16, 96, 96, ctypes.byref(n)) == 0 and n.value == 16 * 9
    assert lib.sst_conv_mtiles(16, 24, 24) == 288
    assert lib.sst_conv_packed_floats(64, 64, 3) == 2 * 1 * 9 * 8 * 256 + 2048 + 64 * 64 * 9   # + band-kernel copy
    assert lib.sst_conv_packed_floats(128, 128, 3) == 4 * 2 * 9 * 8 * 256 + 2048
    assert lib.sst_conv_stat_tiles(16, 24, 24, 64, 64, 3, 1) == 192 and lib.sst_conv_stat_tiles(16, 24, 24, 64, 64, 3, 2) == 96


# No kernel of the library may use scratch (private segment) memory.  A kernel with spilled registers returned wrong, run-to-run
# different results next to a concurrently running branch of the training iteration's two-branch hipGraph on ROCm 7.2 (an
# experimental BatchNorm finalize with 38 spilled registers) while being exact in eager launches - so spills are
# a correctness matter here, not a performance note.  There is no allow-list: every criterion, the best-buddy patch losses included,
# can run inside the captured iteration (engine._criterion_total).


def test_no_kernel_of_the_library_uses_scratch_memory(tmp_path):
    import shutil
    import subprocess
    import pytest
    from srganst import _abi
    llvm = "/opt/rocm/lib/llvm/bin"
    objdump, readelf = os.path.join(llvm, "llvm-objdump"), os.path.join(llvm, "llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm LLVM binutils not found")
    so = shutil.copy(_abi.LIB_PATH, tmp_path / "libsrganst.so")
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)     # extracts the code objects
    objs = [f for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert objs, "no gfx950 code object found in libsrganst.so"
    seen, bad = 0, []
    for f in objs:
        notes = subprocess.run([readelf, "--notes", str(tmp_path / f)], check=True, capture_output=True, text=True).stdout
        name = None
        for line in notes.splitlines():
            line = line.strip()
            if line.startswith(".name:"):
                name = line.split(":", 1)[1].strip()
            elif line.startswith(".private_segment_fixed_size:") and name is not None:
                seen += 1
                if int(line.split(":", 1)[1]) > 0:
                    bad.append((name, int(line.split(":", 1)[1])))
                name = None
    assert seen > 100, f"only {seen} kernels found"
    assert not bad, f"kernels with scratch memory (spilled registers): {bad}"
