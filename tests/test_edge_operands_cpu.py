"""The fixtures and the judge of test_edge_operands.py, pinned on the CPU so the GPU file cannot pass vacuously:
the crafted digits really sit in k_centered's slow-path window (and the fast path alone would get them wrong), the
oracle's centred count, rescale and ModRaise equal big-integer arithmetic on the boundary values, and its
worst-case (all q - 1) key switch and Hadamard sums equal their closed forms."""
from math import prod

import numpy as np
import pytest

import _edge_inputs as ei


def _crt(res, qs):
    Q = prod(qs)
    return sum(int(r) * pow(Q // q % q, -1, q) % q * (Q // q) for r, q in zip(res, qs)) % Q


@pytest.mark.parametrize("bits", [59, 60])
@pytest.mark.parametrize("ns", [2, 3])
def test_crafted_digits_cover_the_slow_path(orc, ns, bits):
    """near_half_digits on one full digit of ns limbs: at least 90 % of the coefficients inside the window
    |lo - 2^63| <= 64 of the kernel's fixed-point sum, the fast path wrong on at least a quarter of those, every
    rounding count 0..ns present (so both sides of each threshold k + 1/2), and the oracle's count exact on all."""
    N = 256
    qs = orc.create_coeff_modulus(N, [bits] * ns)
    Q = prod(qs)
    coef = ei.near_half_digits(qs, ns, ns, N, np.random.default_rng(100 * ns + bits))
    inside = wrong = 0
    seen, sides = set(), set()
    for n in range(N):
        a = [int(coef[u, n]) for u in range(ns)]
        y = ei.digit_y(a, qs)
        win, exact, fast = ei.slow_path_stats(y, qs)
        x = _crt(a, qs)
        S = sum(yu * (Q // q) for yu, q in zip(y, qs))
        assert S % Q == x and exact == S // Q + (1 if 2 * x > Q else 0)
        assert orc.centered_count(y, qs) == exact, (n, a)
        seen.add(exact)
        if win:
            inside += 1
            wrong += fast != exact
            sides.add((S // Q, 2 * x > Q))
    assert inside >= 0.9 * N, inside
    assert wrong >= 0.25 * inside, (wrong, inside)
    assert seen == set(range(ns + 1)), seen
    assert sides == {(k, s) for k in range(ns) for s in (False, True)}, sides


def test_one_limb_digits_cycle_through_the_branch_values(orc):
    N = 64
    qs = orc.create_coeff_modulus(1024, [59, 59, 60])
    rng = np.random.default_rng(1)
    coef = ei.near_half_digits(qs, 1, 3, N, rng)
    for i, q in enumerate(qs):
        assert set(int(v) for v in coef[i]) == set(ei.one_limb_set(q))
        assert orc.centered_count([q >> 1], [q]) == 0 and orc.centered_count([(q >> 1) + 1], [q]) == 1
    assert not (ei.near_half_digits(qs, 1, 3, N, rng, exclude_zero=True) == 0).any()
    part = ei.near_half_digits(qs, 2, 3, N, rng)     # a 2-limb digit and a partial one-limb digit
    assert set(int(v) for v in part[2]) == set(ei.one_limb_set(qs[2]))


CHAINS = [[59] * 4, [60] * 4, [60, 40, 40, 60]]


@pytest.mark.parametrize("bits", CHAINS, ids=["59x4", "60x4", "60-40-40-60"])
@pytest.mark.parametrize("N", [256, 1024, 32768])
def test_oracle_rescale_and_mod_raise_on_edge_limbs(orc, N, bits):
    """Oracle.rescale == floor((x + (q_l >> 1)) / q_l) and Oracle.mod_raise == the centred lift of limb 0, in big
    integers, with the rounded limb cycling through {0, 1, 2, h-1, h, h+1, h+2, q-2, q-1}."""
    primes = orc.create_coeff_modulus(N, bits)
    o = orc.Oracle(N, primes, 1)
    L0 = o.L0
    rng = np.random.default_rng(N + len(bits))
    for l in ([L0] if N > 1024 else range(2, L0 + 1)):
        qs = primes[:l]
        coef = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in qs])
        coef[l - 1] = ei.edge_limb(qs[-1], N, rng)
        ct = ei.to_ntt(o, coef)[None]
        half = qs[-1] >> 1
        Y = [(_crt(coef[:, n], qs) + half) // qs[-1] for n in range(N)]
        want = np.stack([o.ntt(np.array([y % q for y in Y], dtype=np.uint64), i) for i, q in enumerate(qs[:-1])])
        assert np.array_equal(o.rescale(ct)[0], want), f"rescale l={l}"
    for l in (L0, 2):
        coef = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in primes[:l]])
        coef[0] = ei.edge_limb(primes[0], N, rng)
        q0 = primes[0]
        c = [int(x) if int(x) <= q0 >> 1 else int(x) - q0 for x in coef[0]]
        want = np.stack([o.ntt(np.array([v % q for v in c], dtype=np.uint64), i) for i, q in enumerate(primes[:L0])])
        assert np.array_equal(o.mod_raise(ei.to_ntt(o, coef)[None])[0], want), f"mod_raise from l={l}"


@pytest.mark.parametrize("bits,P,levels", [
    ([59] * 39, 3, (36,)), ([60] * 39, 3, (36,)), ([59] * 42, 3, (39, 37)), ([59] * 18 + [60], 1, (18,)),
    ([59] * 6, 2, (4, 3)), ([60, 40, 40, 60], 1, (3,))], ids=["dnum12-59", "dnum12-60", "dnum13", "dnum18", "P2", "60-40"])
def test_oracle_worst_case_keyswitch_closed_form(orc, bits, P, levels):
    N = 1024
    primes = orc.create_coeff_modulus(N, bits)
    o = orc.Oracle(N, primes, P)
    key = ei.max_key(o)
    elt = orc.galois_elt(1, N)
    rng = np.random.default_rng(len(bits))
    for l in levels:
        ei.check_worst_case_keyswitch(o, lambda c3: o.relinearize(c3, key), lambda c2: o.rotate_elt(c2, key, elt), elt, l, rng)


def test_oracle_hoisted_equals_individual_on_near_half(orc):
    N, L0, P = 1024, 6, 3
    primes = orc.create_coeff_modulus(N, [59] * (L0 + P))
    o = orc.Oracle(N, primes, P)
    s = o.gen_secret(8)
    rng = np.random.default_rng(4)
    elts = [orc.galois_elt(k, N) for k in (1, -1, 3)]
    keys = [o.gen_galois_key(8, s, e) for e in elts]
    for l in (6, 5, 4):
        c0 = np.stack([rng.integers(0, primes[i], N, dtype=np.uint64) for i in range(l)])
        ct = np.stack([c0, ei.to_ntt(o, ei.near_half_digits(primes, P, l, N, rng))])
        for h, k, e in zip(o.rotate_hoisted(ct, keys, elts), keys, elts):
            assert np.array_equal(h, o.rotate_elt(ct, k, e)), (l, e)


HADAMARD_N = (8, 9, 16, 17, 33, 64, 66)


@pytest.mark.parametrize("bits", [[59] * 7, [60] * 7, [60, 40, 40, 60]], ids=["59", "60", "60-40"])
def test_oracle_hadamard_closed_form(orc, bits):
    """A sum of n products of all-(q - 1) operands is n mod q_i in every slot."""
    N = 256
    primes = orc.create_coeff_modulus(N, bits)
    o = orc.Oracle(N, primes, 1)
    l = o.L0
    term = o.multiply_plain(ei.all_max(primes, l, N, 2), ei.all_max(primes, l, N))
    acc = None
    for n in range(1, max(HADAMARD_N) + 1):
        acc = term if acc is None else o.add(acc, term)
        if n in HADAMARD_N:
            want = ei.constant_limbs(primes, l, N, n)
            assert np.array_equal(acc, np.stack([want, want])), n
    m = o.multiply(ei.all_max(primes, l, N, 2), ei.all_max(primes, l, N, 2))
    assert np.array_equal(m, np.stack([ei.constant_limbs(primes, l, N, k) for k in (1, 2, 1)]))
