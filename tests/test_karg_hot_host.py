"""The hot argument header of the batch-1 decode kernels (csrc/common.h PG_KARG_HOT) is filled inside the library from
the structs the launchers always built: the C boundary -- PgFusedArgs, the entry points, the ABI number -- is what it
was, and so is the kernels' own EpiArgs.  Host-side checks of that, no device needed."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paligemma-multimodal-system_amd", "csrc")

# the parent's values (include/pghip.h compiled as C, and csrc's EpiArgs: 64 bytes in front of its PgFusedArgs, the
# PG_SLOT_ROWS word behind it)
FUSED_SIZE, EPI_SIZE, ABI = 336, 408, 13
FUSED_OFFSETS = {"pro_mode": 0, "resid_in": 8, "norm_w": 40, "part_o": 56, "part_ml": 64, "pos": 112, "slot_dev": 128,
                 "ss_in": 192,"fx": 304, "status": 328}


def test_fused_args_layout_and_abi_number_are_the_parents():
    from pghip import _lib
    assert ctypes.sizeof(_lib.PgFusedArgs) == FUSED_SIZE
    for name, off in FUSED_OFFSETS.items():
        assert getattr(_lib.PgFusedArgs, name).offset == off, name
    assert _lib.ABI_VERSION == ABI and _lib.load().pg_abi_version() == ABI


def test_header_struct_compiles_to_the_same_size():
    """include/pghip.h's PgFusedArgs as a C compiler lays it out (the binding above mirrors it by hand)."""
    import shutil
    import subprocess
    import tempfile
    import pytest
    if shutil.which("gcc") is None:
        pytest.skip("gcc not installed")
    src = ('#include "pghip.h"\n_Static_assert(sizeof(PgFusedArgs) == %d, "size");\nint main(void) { return 0; }\n'
           % FUSED_SIZE)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "t.c")
        open(f, "w").write(src)
        r = subprocess.run(["gcc", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I",
                            "/opt/rocm/include", f], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_sources_assert_both_struct_sizes_at_compile_time():
    """The library that loaded was compiled with the static_assert on csrc's PgFusedArgs mirror and EpiArgs."""
    text = open(os.path.join(CSRC, "gemm.hip")).read()
    m = re.search(r"static_assert\(sizeof\(PgFusedArgs\) == (\d+) && sizeof\(EpiArgs\) == (\d+)", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (FUSED_SIZE, EPI_SIZE)


def test_entry_points_keep_their_signatures():
    """The launchers changed, the entry points did not: every argument list the binding declares is still the header's
    (count of parameters per function)."""
    from pghip import _lib
    hdr = open(os.path.join(ROOT, "include", "pghip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("pg_gemm_fused", "pg_gemm", "pg_attention", "pg_attention_rows", "pg_argmax", "pg_argmax_embed"):
        m = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name


def test_switch_defaults_on_and_the_build_asks_for_the_preload_where_it_gained():
    from pghip import build
    text = open(os.path.join(CSRC, "common.h")).read()
    assert re.search(r"#ifndef PG_KARG_HOT\n#define PG_KARG_HOT 1\n#endif", text)
    assert build.PRELOAD_FLAGS == ["-mllvm", "-amdgpu-kernarg-preload-count=16"]
    assert set(build.PRELOAD_SOURCES) == {"gemm_gemv.hip", "misc.hip"}
    for name in build.PRELOAD_SOURCES:
        assert os.path.exists(os.path.join(CSRC, name)), name
    # the preload is part of the configuration the library's source hash covers
    assert "-amdgpu-kernarg-preload-count=16" in build._config() and "misc.hip" in build._config()
