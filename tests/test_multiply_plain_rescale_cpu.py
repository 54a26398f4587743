"""The host side of the fused batched CT x PT multiply and rescale (fhs_multiply_plain_rescale_many) without a GPU:
the symbols the header, the library and the binding export, and the argument validation / chunk plan (fhs_tables.h
mulp_rescale_many_error, mulp_rescale_chunks) checked by the stand-alone program tools/debug/mulp_rescale_check.cpp
under the address and undefined-behaviour sanitizers."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def test_header_library_and_binding_export_multiply_plain_rescale_many():
    import pyPhantom as ph
    header = re.sub(r"\s+", " ", (REPO / "include" / "fhespear.h").read_text())
    assert ("fhs_status fhs_multiply_plain_rescale_many(fhs_context* ctx, const fhs_ciphertext* const* a, "
            "const fhs_plaintext* const* p, int n, fhs_ciphertext** out_array);") in header
    res, args = ph._SIGS["fhs_multiply_plain_rescale_many"]
    vp, pvp = C.c_void_p, C.POINTER(C.c_void_p)
    assert res is C.c_int and args == [vp, pvp, pvp, C.c_int, pvp]
    fn = ph._lib.fhs_multiply_plain_rescale_many    # the built library has it
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    assert list(inspect.signature(ph.multiply_plain_rescale_many).parameters) == ["ctx", "cts", "pts"]
    assert list(inspect.signature(ph.rescale_many).parameters) == ["ctx", "cts"]
    assert list(inspect.signature(ph.ct_pt_dot_columns).parameters) == ["ctx", "ct", "W", "dim", "scale", "gk"]
    assert list(inspect.signature(ph.ct_pt_dot_many).parameters) == ["ctx", "ct", "pts", "dim", "gk"]


def test_null_context_is_rejected_before_the_device_is_touched():
    import pyPhantom as ph
    assert ph._lib.fhs_multiply_plain_rescale_many(None, None, None, 1, None) == 1
    assert b"null context" in ph._lib.fhs_last_error()


def test_lists_of_different_length_are_rejected_in_the_binding():
    """The one rejection the C call cannot make (it takes a single n): before any handle is read.  The single
    ciphertext form takes its length from the plaintexts and cannot be ragged."""
    import pyPhantom as ph
    with pytest.raises(ValueError, match="different length"):
        ph.multiply_plain_rescale_many(None, [], [object()])
    with pytest.raises(ValueError, match="different length"):
        ph.multiply_plain_rescale_many(None, [object(), object()], [object()])
    with pytest.raises(ValueError, match=r"\(dim, F\) array"):
        ph.ct_pt_dot_columns(None, None, [[1.0, 2.0]], 2, 2.0 ** 40, None)


def test_validation_and_chunk_plan_under_sanitizers(tmp_path):
    """For every N = 256..32768, level 1..12 and n = 1..5000, with the per-item costs the host layer charges: the
    chunks cover [0, n) exactly once, their sizes differ by at most one, none is over the item, pointer-buffer or grid
    bound, none exceeds the byte cap unless it is a single item, and no fewer chunks would fit; the null, n, component,
    chain-index (ciphertexts, plaintexts) and last-level rejections each carry their own message and status class."""
    exe = tmp_path / "mulp_rescale_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'tools/debug/shim'}", f"-I{REPO / 'fhe-spear_amd/csrc'}",
                    str(REPO / "tools/debug/mulp_rescale_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("N=")]
    assert [int(ln.split()[0][2:]) for ln in lines] == [256 << k for k in range(8)]
    assert all(" ok: " in ln for ln in lines)
