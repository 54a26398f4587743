"""The host side of the batched rotate-and-sum (fhs_inner_sum_many) without a GPU: the symbols the header, the
library and the binding export, and the argument validation / step list (fhs_tables.h inner_sum_steps) checked by
the stand-alone program tools/debug/inner_sum_check.cpp under the address and undefined-behaviour sanitizers."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]


def test_header_library_and_binding_export_inner_sum_many():
    import pyPhantom as ph
    header = re.sub(r"\s+", " ", (REPO / "include" / "fhespear.h").read_text())
    assert ("fhs_status fhs_inner_sum_many(fhs_context* ctx, const fhs_ciphertext* const* in, int n, int dim, "
            "int stride, const fhs_galois_keys* gk, fhs_ciphertext** out_array);") in header
    res, args = ph._SIGS["fhs_inner_sum_many"]
    vp, pvp = C.c_void_p, C.POINTER(C.c_void_p)
    assert res is C.c_int and args == [vp, pvp, C.c_int, C.c_int, C.c_int, vp, pvp]
    fn = ph._lib.fhs_inner_sum_many                 # the built library has it
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    assert list(inspect.signature(ph.inner_sum_many).parameters) == ["ctx", "cts", "dim", "gk", "stride"]
    assert list(inspect.signature(ph.inner_sum).parameters) == ["ctx", "ct", "dim", "gk", "stride"]
    assert inspect.signature(ph.inner_sum_many).parameters["stride"].default == 1
    assert inspect.signature(ph.inner_sum).parameters["stride"].default == 1
    assert list(inspect.signature(ph.ct_pt_dot_many).parameters) == ["ctx", "ct", "pts", "dim", "gk"]
    # a null context is rejected before the device is touched
    assert fn(None, None, 1, 2, 1, None, None) == 1 and b"null context" in ph._lib.fhs_last_error()


def test_step_list_and_rejections_under_sanitizers(tmp_path):
    """For every N = 256..32768, every dim up to 64 (and N/2, N/2 + 1, N) and strides from 1 to N/2: an accepted call
    gives exactly the reference loop's steps (step = 1; while step < dim: stride * step; step *= 2), each a rotation
    fhs_rotate accepts; a call is rejected exactly when the loop's largest step is none; n, dim, stride < 1 and the
    extremes of int are rejected with their own messages and leave no steps."""
    exe = tmp_path / "inner_sum_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'tools/debug/shim'}", f"-I{REPO / 'fhe-spear_amd/csrc'}",
                    str(REPO / "tools/debug/inner_sum_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("N=")]
    assert [int(ln.split()[0][2:]) for ln in lines] == [256 << k for k in range(8)]
    assert all(" ok: " in ln for ln in lines)
