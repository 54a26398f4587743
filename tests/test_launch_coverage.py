"""Launch coverage: every kernel compiled into libfhespear_hip.so is launched by an oracle-checked case.

The library keeps a launch ledger (fhs_debug_launch_ledger, pyPhantom.debug_launch_ledger): while armed it records
which kernels were launched.  tests/golden/kernel_manifest.json lists every kernel of the built library (CPU test
below: the committed list equals the library's, so adding or removing an instantiation means regenerating it with
tests/golden/make_kernel_manifest.py).  One GPU test per ring then arms the ledger, runs that ring's cases of
tests/_launch_matrix.py -- each comparing what the library returned -- and asserts that every manifest kernel of the
ring was launched or is in EXEMPT (the 6 instantiations no argument can launch), and that no EXEMPT kernel was
launched.  A kernel added later without such a case fails its ring's test by name."""
import ctypes
import json
import sys
from pathlib import Path

import pytest

import _launch_matrix as lm

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_kernel_manifest as mk  # noqa: E402


def manifest():
    return json.loads((GOLDEN / "kernel_manifest.json").read_text())["kernels"]


# ----------------------------------------------------------------------------- CPU
def test_manifest_equals_built_library():
    """The committed manifest is the built library's kernel list (kernel descriptors of its gfx950 code object), in
    the ledger's spelling, sorted."""
    if not mk.tools_present():
        pytest.skip("llvm-objdump of the ROCm toolchain is not on this machine")
    import pyPhantom  # noqa: F401  (the library is built)
    want = mk.kernel_names()
    got = manifest()
    assert got == sorted(got) and len(set(got)) == len(got)
    assert got == want, (f"kernel_manifest.json is stale: not in the library {sorted(set(got) - set(want))}, "
                         f"not in the manifest {sorted(set(want) - set(got))}; run tests/golden/make_kernel_manifest.py")


def test_manifest_spelling_and_exemptions():
    """Every name is a bare kernel with its template arguments; the per-ring families carry LOGN 8..15 first; EXEMPT
    names manifest kernels only, at most 8, each with a reason."""
    names = manifest()
    for n in names:
        assert n.startswith("k_") and "(" not in n and "::" not in n and " <" not in n and not n.startswith("void"), n
        assert lm.logn_of(n) in (None, 8, 9, 10, 11, 12, 13, 14, 15), n
    assert mk.normalise("void fhs::k_modup_h<12, 3, true>(fhs::DevTables, unsigned long const* const*, int)") == \
        "k_modup_h<12, 3, true>"
    assert mk.normalise("fhs::k_eltwise(fhs::DevTables, int, unsigned long const*)") == "k_eltwise"
    assert len(lm.EXEMPT) <= 8 and set(lm.EXEMPT) <= set(names)
    assert all(isinstance(r, str) and len(r) > 40 for r in lm.EXEMPT.values())


def test_ledger_hook_without_a_gpu():
    """arm / disarm / read through the C ABI with nothing launched: an empty ledger reads as the empty string, a
    short or null buffer is FHS_ERR_INVALID with the needed size still reported, an unknown operation is rejected."""
    import pyPhantom as ph
    fn = ph._lib.fhs_debug_launch_ledger
    ARM, DISARM, READ, INVALID = 0, 1, 2, 1
    need = ctypes.c_uint64(99)
    for op in (ARM, DISARM, ARM, ARM, DISARM):
        assert fn(op, None, 0, None) == 0
        buf = ctypes.create_string_buffer(b"x" * 7, 8)
        assert fn(READ, buf, 8, ctypes.byref(need)) == 0
        assert need.value == 1 and buf.value == b""
        need.value = 99
        assert fn(READ, buf, 0, ctypes.byref(need)) == INVALID and need.value == 1
        assert fn(READ, None, 8, ctypes.byref(need)) == INVALID
        assert fn(READ, buf, 1, None) == 0
    assert fn(3, None, 0, None) == INVALID
    assert ph.debug_launch_ledger("arm") is None and ph.debug_launch_ledger("read") == []
    assert ph.debug_launch_ledger("disarm") is None and ph.debug_launch_ledger() == []
    with pytest.raises(ValueError):
        ph.debug_launch_ledger("clear")


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


def _launched(ph, run):
    """What `run` launched (run may return further names: a child process's own ledger).  Arming again afterwards
    must clear what was recorded."""
    ph.debug_launch_ledger("arm")
    try:
        more = run()
    finally:
        ph.debug_launch_ledger("disarm")
    launched = set(ph.debug_launch_ledger("read"))
    assert launched, "the armed ledger recorded nothing"
    ph.debug_launch_ledger("arm")
    assert ph.debug_launch_ledger("read") == [], "arming did not clear the ledger"
    ph.debug_launch_ledger("disarm")
    return launched | set(more or ())


def _judge(launched, mine, what):
    names = set(manifest())
    assert launched <= names, f"{what}: the ledger names kernels the manifest does not: {sorted(launched - names)}"
    missing = sorted(mine - launched - set(lm.EXEMPT))
    assert not missing, f"{what}: no oracle-checked case launched {missing}"
    stale = sorted(launched & set(lm.EXEMPT))
    assert not stale, f"{what}: EXEMPT lists kernels that were launched: {stale}"


@pytest.mark.gpu
@pytest.mark.parametrize("N", lm.RINGS)
def test_every_kernel_of_the_ring_has_a_checked_case(ph, orc, tmp_path, N):
    """Arm, run the ring's cases (each compares its outputs), read: every manifest kernel with LOGN = log2 N was
    launched or is exempt.  The unfused encoder needs an environment knob, so a child process runs it and prints its
    own ledger, which is united with this process's."""
    def run():
        shared = lm.shared_contexts(ph, orc, N)
        lm.run_ring(ph, orc, N, shared)
        return lm.case_encode_unfused(N, shared[1], tmp_path)
    launched = _launched(ph, run)
    logn = N.bit_length() - 1
    _judge(launched, {k for k in manifest() if lm.logn_of(k) == logn}, f"N = {N}")


@pytest.mark.gpu
def test_every_ring_independent_kernel_has_a_checked_case(ph, orc):
    """The kernels without a ring in their name, at N = 1024 (the compact Hadamard also at N = 512 and 2048, one
    tiling factor each): the per-ring cases, the element-wise ops, all ten k_bsgs_inner and all four k_dot_tensor."""
    launched = _launched(ph, lambda: lm.run_independent(ph, orc))
    _judge(launched, {k for k in manifest() if lm.logn_of(k) is None}, "ring-independent kernels")
