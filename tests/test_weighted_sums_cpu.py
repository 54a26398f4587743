"""The host side of the batched plaintext-weighted sums (fhs_weighted_sums, pyPhantom.weighted_sums) without a GPU: the
symbols the header, the library and the binding export; validation, weight tables and chunk plan (fhs_tables.h) checked
by the stand-alone program tools/debug/weighted_sums_check.cpp under the address and undefined-behaviour sanitizers;
the kernel's per-coefficient routines (fhs_debug_wsum_round / fhs_debug_wsum_accumulate) against Python big integers;
and the identity that makes the loop one pass, evaluated in Python on the oracle's own transforms against the oracle's
loop o.add(o.rescale(o.multiply_plain(...)))."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
FS = (1, 63, 64, 65, 128, 129, 4096)


def test_header_library_and_binding_export_weighted_sums():
    import pyPhantom as ph
    header = re.sub(r"\s+", " ", (REPO / "include" / "fhespear.h").read_text())
    assert ("fhs_status fhs_weighted_sums(fhs_context* ctx, const fhs_ciphertext* const* in, int F, "
            "const double* W, int64_t ldw, int E, double scale, fhs_ciphertext** out_array);") in header
    assert "fhs_status fhs_debug_wsum_round(uint64_t qL, const uint64_t* k, const uint64_t* d, int F, int64_t* hi, uint64_t* lo);" in header
    assert "fhs_status fhs_debug_wsum_accumulate(uint64_t q, const uint64_t* kprime, const uint64_t* c, int F, uint64_t wT," in header
    res, args = ph._SIGS["fhs_weighted_sums"]
    vp, pvp = C.c_void_p, C.POINTER(C.c_void_p)
    assert res is C.c_int and args == [vp, pvp, C.c_int, C.POINTER(C.c_double), C.c_int64, C.c_int, C.c_double, pvp]
    fn = ph._lib.fhs_weighted_sums                  # the built library has it
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    assert list(inspect.signature(ph.weighted_sums).parameters) == ["ctx", "cts", "W", "scale"]
    assert list(inspect.signature(ph.weighted_sum).parameters) == ["ctx", "cts", "weights", "scale"]


def test_null_context_is_rejected_before_the_device_is_touched():
    import pyPhantom as ph
    assert ph._lib.fhs_weighted_sums(None, None, 1, None, 1, 1, 1.0, None) == 1
    assert b"null context" in ph._lib.fhs_last_error()


def test_shape_mismatch_is_rejected_in_the_binding():
    """Before the C call and before any handle is read: W's rows must be the inputs, and weighted_sum's weights a vector."""
    import pyPhantom as ph
    with pytest.raises(ValueError, match=r"\(F, E\) array with F = 2 rows"):
        ph.weighted_sums(None, [object(), object()], np.zeros((3, 2)), 2.0 ** 40)
    with pytest.raises(ValueError, match=r"\(F, E\) array"):
        ph.weighted_sums(None, [object()], np.zeros(1), 2.0 ** 40)
    with pytest.raises(ValueError, match="one-dimensional"):
        ph.weighted_sum(None, [object()], np.zeros((1, 1)), 2.0 ** 40)
    with pytest.raises(ValueError, match="F = 1 rows"):
        ph.weighted_sum(None, [object()], [0.5, 0.25], 2.0 ** 40)


def test_validation_tables_and_chunk_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "weighted_sums_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'tools/debug/shim'}", f"-I{REPO / 'fhe-spear_amd/csrc'}",
                    str(REPO / "tools/debug/weighted_sums_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    assert [ln.split()[0] for ln in r.stdout.splitlines()] == ["errors", "tables", "chunks", "routines", "OK"]


# ------------------------------------------------------------------------------------------------ the two hooks
@pytest.fixture(scope="module")
def hooks():
    import pyPhantom as ph
    U64 = C.c_uint64

    def rnd(q, k, d):
        F = len(k)
        hi, lo = C.c_int64(), U64()
        rc = ph._lib.fhs_debug_wsum_round(q, (U64 * F)(*k), (U64 * F)(*d), F, C.byref(hi), C.byref(lo))
        return rc, hi.value * (1 << 64) + lo.value

    def acc(q, kp, c, wT, t):
        F = len(kp)
        out = U64()
        rc = ph._lib.fhs_debug_wsum_accumulate(q, (U64 * F)(*kp), (U64 * F)(*c), F, wT, t, C.byref(out))
        return rc, out.value
    return rnd, acc


@pytest.fixture(scope="module")
def primes(orc):
    a = orc.create_coeff_modulus(1024, [60, 40, 40, 60])
    b = orc.create_coeff_modulus(1024, [59] * 12)
    assert [q.bit_length() for q in a] == [60, 40, 40, 60] and all(q.bit_length() == 59 for q in b)
    return a + b[:2]


def _centre(u, q):
    half = q >> 1
    return ((u + half) % q) - half


def _want_round(q, k, d):
    return sum(_centre(x * y % q, q) for x, y in zip(k, d))


def _want_acc(q, kp, c, wT, t):
    return (sum(x * y for x, y in zip(kp, c)) + wT * t) % q


@pytest.mark.parametrize("F", FS)
def test_hooks_worst_case_operands(hooks, primes, F):
    """Every operand q - 1: the largest split-30 partials, the largest 128-bit window sums (a fold one product late or
    a window one product long shows here), and for the rounding sum u = 1 in every term; then k = q - 1 (weight -1)
    on d = half + 1, the most negative centred terms."""
    rnd, acc = hooks
    for q in primes:
        v = [q - 1] * F
        assert acc(q, v, v, q - 1, q - 1) == (0, _want_acc(q, v, v, q - 1, q - 1)), (q, F)
        assert rnd(q, v, v) == (0, _want_round(q, v, v)), (q, F)
        d = [(q >> 1) + 1] * F
        assert rnd(q, [1] * F, d) == (0, -F * (q >> 1)), (q, F)
        assert rnd(q, v, d) == (0, F * (q >> 1)), (q, F)


@pytest.mark.parametrize("F", FS)
def test_hooks_random_operands_with_negative_and_zero_weights(hooks, primes, F):
    rnd, acc = hooks
    rng = np.random.default_rng(3000 + F)
    for q in primes:
        for _ in range(3 if F < 4096 else 1):
            k, d = [[int(x) for x in rng.integers(0, q, F, dtype=np.uint64)] for _ in range(2)]
            for j in range(0, F, 5):       # weights 0, 1, -1, 2, -2 (as residues) among the random ones
                k[j] = [0, 1, q - 1, 2, q - 2][(j // 5) % 5]
            wT, t = int(rng.integers(0, q, dtype=np.uint64)), int(rng.integers(0, q, dtype=np.uint64))
            assert acc(q, k, d, wT, t) == (0, _want_acc(q, k, d, wT, t)), (q, F)
            assert rnd(q, k, d) == (0, _want_round(q, k, d)), (q, F)


def test_round_hook_at_the_rounding_boundaries(hooks, primes):
    """u = k d mod q at 0, half - 1, half, half + 1 and q - 1, reached with weight 1 and with weight -1: the centred
    value changes sign between half and half + 1 (q is odd: no tie)."""
    rnd, _ = hooks
    for q in primes:
        half = q >> 1
        us = [0, half - 1, half, half + 1, q - 1]
        assert [rnd(q, [1], [u])[1] for u in us] == [0, half - 1, half, -half, -1]
        assert [rnd(q, [q - 1], [(q - u) % q])[1] for u in us] == [0, half - 1, half, -half, -1]
        assert rnd(q, [1] * 5, us) == (0, sum([0, half - 1, half, -half, -1]))
        assert rnd(q, [0] * 5, us) == (0, 0)


def test_hooks_reject_operands_outside_the_contract(hooks, primes):
    rnd, acc = hooks
    q = primes[0]
    assert rnd(q, [q], [0])[0] != 0 and rnd(q, [0], [q])[0] != 0
    assert acc(q, [q], [0], 0, 0)[0] != 0 and acc(q, [0], [0], q, 0)[0] != 0 and acc(q, [0], [0], 0, q)[0] != 0
    assert rnd((1 << 61) - 1, [0], [0])[0] != 0 and acc((1 << 61) - 1, [0], [0], 0, 0)[0] != 0
    assert rnd(q, [], [])[0] != 0 and acc(q, [0] * 4097, [0] * 4097, 0, 0)[0] != 0


# ------------------------------------------------------------------------------------------------ the identity
def _const_pt(primes, l, N, c):
    return np.stack([np.full(N, c % primes[m], dtype=np.uint64) for m in range(l)])


def oracle_loop(o, xs, cs, l):
    """The reference's loop for one output: every term multiplied, rescaled on its own, then added."""
    acc = None
    for x, c in zip(xs, cs):
        t = o.rescale(o.multiply_plain(x, _const_pt(o.primes, l, o.N, c)))
        acc = t if acc is None else o.add(acc, t)
    return acc


def formula(o, xs, cs, l):
    """out[comp][m] = sum_j (k_jm inv_m) c_j[comp][m] - inv_m NTT_m(S[comp] mod q_m),
    S[comp][n] = sum_j centre(k_jL d_j[comp][n] mod q_L), d_j = INTT_L(c_j[comp][L])."""
    L, N, q = l - 1, o.N, o.primes
    out = np.empty((2, L, N), dtype=np.uint64)
    for comp in range(2):
        S = [0] * N
        for x, c in zip(xs, cs):
            d = o.intt(x[comp, L], L)
            S = [s + _centre((c % q[L]) * int(v) % q[L], q[L]) for s, v in zip(S, d)]
        for m in range(L):
            inv = pow(q[L], -1, q[m])
            T = o.ntt(np.array([s % q[m] for s in S], dtype=np.uint64), m)
            row = [(sum((c % q[m]) * inv * int(x[comp, m, n]) for x, c in zip(xs, cs)) - inv * int(T[n])) % q[m] for n in range(N)]
            out[comp, m] = np.array(row, dtype=np.uint64)
    return out


@pytest.mark.parametrize("bits,l,worst", [((60, 40, 40, 60), 3, False), ((60, 40, 40, 60), 2, False),
                                          ((60,) + (40,) * 9 + (60,), 7, False), ((59,) * 5, 4, True)])
def test_the_identity_equals_the_oracle_loop(orc, bits, l, worst):
    N = 256
    primes = orc.create_coeff_modulus(N, list(bits))
    o = orc.Oracle(N, primes, 1)
    rng = np.random.default_rng(l + len(bits))
    F = 5
    if worst:
        xs = [np.stack([np.stack([np.full(N, primes[i] - 1, dtype=np.uint64) for i in range(l)])] * 2)] * F
    else:
        xs = [np.stack([np.stack([rng.integers(0, primes[i], N, dtype=np.uint64) for i in range(l)]) for _ in range(2)])
              for _ in range(F)]
    cs = [-1, 0, 1, int(rng.integers(-2 ** 40, 2 ** 40)), -int(rng.integers(1, 2 ** 61))]
    assert np.array_equal(formula(o, xs, cs, l), oracle_loop(o, xs, cs, l))
