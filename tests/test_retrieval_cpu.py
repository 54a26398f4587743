"""k_dot_tensor's per-coefficient schedule on the host (no GPU): fhs_debug_dot_accumulate runs the shared
__host__ __device__ routines of fhs_modarith.h (dot3_term: split-30 accumulate and the Acc3 folds, s1 folding
twice as often as s0 / s2; dot3_finish: 128-bit sums, one reduce128 each, windows of 64 terms adding their
reduced sums) for one coefficient.  Checked against Python big integers on the primes of the two retrieval
test chains: [60, 40, 40, 60] (the reference's EncryptedSimilarityJoins set: 8 products per fold on the 60-bit
primes, the 40-bit ones off the usual 59/60-bit pseudo-Mersenne fold) and the all-59-bit chain (16 per fold)."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
U64 = ctypes.c_uint64
U64P = ctypes.POINTER(U64)


@pytest.fixture(scope="module")
def dot_accumulate():
    lib_path = REPO / "fhe-spear_amd" / "lib" / "libfhespear_hip.so"
    if not lib_path.exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(str(lib_path))
    fn = lib.fhs_debug_dot_accumulate          # AttributeError here: the library predates the fused dot product
    fn.argtypes = [U64, U64P, U64P, U64P, U64P, ctypes.c_int, U64P]
    fn.restype = ctypes.c_int

    def run(q, a0, a1, b0, b1):
        J = len(a0)
        out = (U64 * 3)()
        rc = fn(q, *[(U64 * J)(*v) for v in (a0, a1, b0, b1)], J, out)
        return rc, [int(x) for x in out]
    return run


@pytest.fixture(scope="module")
def chain_primes(orc):
    a = orc.create_coeff_modulus(1024, [60, 40, 40, 60])
    b = orc.create_coeff_modulus(1024, [59] * 12)
    assert [q.bit_length() for q in a] == [60, 40, 40, 60] and all(q.bit_length() == 59 for q in b)
    return a + b[:3] + b[-1:]


def _want(q, a0, a1, b0, b1):
    return [sum(x * y for x, y in zip(a0, b0)) % q,
            sum(x * w + z * y for x, z, y, w in zip(a0, a1, b0, b1)) % q,
            sum(z * w for z, w in zip(a1, b1)) % q]


@pytest.mark.parametrize("J", [1, 8, 16, 17, 64])
def test_dot_accumulate_worst_case_operands(dot_accumulate, chain_primes, J):
    """Every operand q - 1: the largest split-30 partials and the largest 128-bit sums the schedule can see
    (the accumulator-overflow case: a fold one product late or a window one term long shows here)."""
    for q in chain_primes:
        v = [q - 1] * J
        rc, got = dot_accumulate(q, v, v, v, v)
        assert rc == 0 and got == _want(q, v, v, v, v), (q, J)


@pytest.mark.parametrize("J", [1, 8, 16, 17, 64])
def test_dot_accumulate_random_operands(dot_accumulate, chain_primes, J):
    rng = np.random.default_rng(1000 + J)
    for q in chain_primes:
        for _ in range(8):
            v = [[int(x) for x in rng.integers(0, q, J, dtype=np.uint64)] for _ in range(4)]
            rc, got = dot_accumulate(q, *v)
            assert rc == 0 and got == _want(q, *v), (q, J)


def test_dot_accumulate_across_windows_and_mixed_extremes(dot_accumulate, chain_primes):
    """Past one window (J = 65, 130: the reduced sums of 64-term windows are added) and operands that are
    extreme in one component only (s1's two products per term with one of them zero)."""
    for q in chain_primes:
        for J in (65, 130):
            v = [q - 1] * J
            assert dot_accumulate(q, v, v, v, v) == (0, _want(q, v, v, v, v))
        z, m = [0] * 17, [q - 1] * 17
        for v in ((m, z, m, m), (z, m, m, m), (m, m, z, m), (m, m, m, z)):
            assert dot_accumulate(q, *v) == (0, _want(q, *v))


def test_dot_accumulate_rejects_operands_outside_the_contract(dot_accumulate, chain_primes):
    q = chain_primes[0]
    assert dot_accumulate(q, [q], [0], [0], [0])[0] != 0          # operand not reduced
    assert dot_accumulate((1 << 61) - 1, [0], [0], [0], [0])[0] != 0   # prime above the 60-bit limit
