"""The host side of the batched multiply / relinearize / rescale (fhs_multiply_relin_many) without a GPU: the symbols
the header, the library and the binding export, and the argument validation / chunk plan (fhs_tables.h
multiply_many_error, batch_chunks) checked by the stand-alone program tools/debug/multiply_many_check.cpp under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]


def test_header_library_and_binding_export_multiply_relin_many():
    import pyPhantom as ph
    header = re.sub(r"\s+", " ", (REPO / "include" / "fhespear.h").read_text())
    assert ("fhs_status fhs_multiply_relin_many(fhs_context* ctx, const fhs_ciphertext* const* a, "
            "const fhs_ciphertext* const* b, int n, const fhs_relin_key* rk, int rescale, "
            "fhs_ciphertext** out_array);") in header
    res, args = ph._SIGS["fhs_multiply_relin_many"]
    vp, pvp = C.c_void_p, C.POINTER(C.c_void_p)
    assert res is C.c_int and args == [vp, pvp, pvp, C.c_int, vp, C.c_int, pvp]
    fn = ph._lib.fhs_multiply_relin_many            # the built library has it
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    assert list(inspect.signature(ph.multiply_relin_many).parameters) == ["ctx", "a", "b", "rk", "rescale"]
    assert list(inspect.signature(ph.square_many).parameters) == ["ctx", "cts", "rk", "rescale"]
    assert inspect.signature(ph.multiply_relin_many).parameters["rescale"].default is True
    assert inspect.signature(ph.square_many).parameters["rescale"].default is True


def test_null_context_is_rejected_before_the_device_is_touched():
    import pyPhantom as ph
    assert ph._lib.fhs_multiply_relin_many(None, None, None, 1, None, 1, None) == 1
    assert b"null context" in ph._lib.fhs_last_error()


def test_lists_of_different_length_are_rejected_in_the_binding():
    """The one rejection the C call cannot make (it takes a single n): before any handle is read."""
    import pyPhantom as ph
    import pytest
    with pytest.raises(ValueError, match="different length"):
        ph.multiply_relin_many(None, [], [object()], None)


def test_validation_and_chunk_plan_under_sanitizers(tmp_path):
    """For every N = 256..32768, level 1..12, P = 1 and 3 and n = 1..5000, with the per-item scratch the host layer
    charges: the chunks cover [0, n) exactly once, their sizes differ by at most one, none exceeds the item buffer,
    none exceeds the byte cap unless it is a single item, and no fewer chunks would fit; batch_chunks keeps the chunk
    count and the largest chunk of the plan fhs_inner_sum_many used to make by hand (n = 1..1100); the null, n, component,
    chain-index and last-level rejections each carry their own message and status class."""
    exe = tmp_path / "multiply_many_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'tools/debug/shim'}", f"-I{REPO / 'fhe-spear_amd/csrc'}",
                    str(REPO / "tools/debug/multiply_many_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("N=")]
    assert [int(ln.split()[0][2:]) for ln in lines] == [256 << k for k in range(8)]
    assert all(" ok: " in ln for ln in lines)
    assert "inner_sum_many ok: 7700 plans" in r.stdout
