"""Crafted operands for the edge-operand parity tests (test_edge_operands_cpu.py, test_edge_operands.py):
residues at the rounding boundaries of the centred ModUp, of rescale and of ModRaise, and all-(q - 1)
operands that drive the lazy accumulators to their bound.  Host only: numpy and Python integers; nothing
here touches the GPU library."""
from math import prod

import numpy as np

_M64 = (1 << 64) - 1


def _fill(values, N, rng):
    """`values` (cyclically repeated to N entries if shorter) at permuted positions."""
    vals = [values[i % len(values)] for i in range(N)]
    perm = rng.permutation(N)
    out = [0] * N
    for pos, v in zip(perm, vals):
        out[int(pos)] = v
    return out


def one_limb_set(q, exclude_zero=False):
    """The one-limb digit's boundary values: the y > q/2 branch flips between q >> 1 and (q >> 1) + 1."""
    h = q >> 1
    s = [0, 1, h, h + 1, h - 1, q - 1]
    return s[1:] if exclude_zero else s


def near_half_values(Q, N, rng):
    """N digit integers in [0, Q) with x / Q within 2^41 / Q of 1/2 (alternately just below and just above;
    Q is odd, so never on it), after the fixed set {0, 1, Q-1, h, h+1, h-1, h+2, h-64, h+65}, h = (Q-1)/2."""
    h = (Q - 1) // 2
    vals = [0, 1, Q - 1, h, h + 1, h - 1, h + 2, h - 64, h + 65][:N]
    while len(vals) < N:
        d = int(rng.integers(0, 1 << 40))
        vals.append(h - d if len(vals) % 2 else h + 1 + d)
    return vals


def near_half_digits(primes, P, l, N, rng, exclude_zero=False):
    """Coefficient-form limbs (l, N): in every key-switch digit j (limbs jP .. min(jP + P, l) - 1) every
    coefficient is a digit integer next to Q_S / 2 (near_half_values) reduced to the digit's primes, at permuted
    positions; a one-limb digit (P = 1 or a partial last digit) cycles through one_limb_set."""
    out = np.empty((l, N), dtype=np.uint64)
    for s0 in range(0, l, P):
        qs = [int(q) for q in primes[s0:min(s0 + P, l)]]
        if len(qs) == 1:
            xs = _fill(one_limb_set(qs[0], exclude_zero), N, rng)
        else:
            xs = _fill(near_half_values(prod(qs), N, rng), N, rng)
        for u, q in enumerate(qs):
            out[s0 + u] = np.array([x % q for x in xs], dtype=np.uint64)
    return out


def edge_set(q):
    h = q >> 1
    return [0, 1, 2, h - 1, h, h + 1, h + 2, q - 2, q - 1]


def edge_limb(q, N, rng):
    """One coefficient-form limb cycling through the nine values around 0, q >> 1 and q, permuted."""
    return np.array(_fill(edge_set(int(q)), N, rng), dtype=np.uint64)


def all_max(primes, l, N, ncomp=None):
    """Every word q_i - 1: (ncomp, l, N), or (l, N) when ncomp is None (a plaintext).  In NTT form this is the
    constant polynomial -1."""
    limb = np.stack([np.full(N, int(primes[i]) - 1, dtype=np.uint64) for i in range(l)])
    return limb if ncomp is None else np.stack([limb] * ncomp)


def max_key(o, every=1):
    """A switching key (Oracle.key_shape(): dnum, 2, K, N) with every word q_t - 1.  every = 2: only on the even
    limbs t, the word 1 on the odd ones -- an accumulator that overflows then does so in every other limb, which
    the ModDown cannot absorb (the same wrap in all limbs is one small integer over Q P, which its division by P
    mostly hides)."""
    k = np.ones(o.key_shape(), dtype=np.uint64)
    for t, q in enumerate(o.primes):
        if t % every == 0:
            k[:, :, t, :] = q - 1
    return k


def to_ntt(o, coef):
    """Oracle.ntt per limb of (l, N) or (ncomp, l, N) coefficient-form limbs; limb i is modulo primes[i]."""
    coef = np.asarray(coef, dtype=np.uint64)
    if coef.ndim == 3:
        return np.stack([to_ntt(o, c) for c in coef])
    return np.stack([o.ntt(coef[i], i) for i in range(coef.shape[0])])


def digit_y(a, qs):
    """The residues the centred count reads: y_u = a_u (Q_S / q_u)^-1 mod q_u for a digit's coefficient residues."""
    Q = prod(qs)
    return [int(au) * pow(Q // q % q, -1, q) % q for au, q in zip(a, qs)]


def slow_path_stats(y, qs):
    """k_centered's fixed-point sum restated: F_u = y_u hi(R_u) + mulhi(y_u, lo(R_u)) mod 2^64 with
    R_u = floor(2^128 / q_u), lo = sum F_u mod 2^64 with its carries counted.  Returns (inside, exact, fast):
    whether |lo - 2^63| <= 64 (the kernel then decides with multi-word integers), the exact count
    (2 S + Q) // (2 Q) for S = sum y_u Q / q_u, and what the fast path alone would answer."""
    lo, carry = 0, 0
    for yu, q in zip(y, qs):
        R = ((1 << 128) - 1) // q
        F = (yu * (R >> 64) + ((yu * (R & _M64)) >> 64)) & _M64
        lo += F
        if lo > _M64:
            lo &= _M64
            carry += 1
    half = 1 << 63
    Q = prod(qs)
    S = sum(yu * (Q // q) for yu, q in zip(y, qs))
    return abs(lo - half) <= 64, (2 * S + Q) // (2 * Q), carry + (1 if lo >= half else 0)


def keyswitch_worst_case_constant(primes, L0, P, l):
    """Exact convention, input the constant -1 (all_max) under max_key: every accumulator slot is dn = ceil(l / P)
    products of (-1)^2, i.e. the constant dn over Q_l P.  The ModDown subtracts the uncentred conversion
    S = sum_k (dn (P/p_k)^-1 mod p_k) (P/p_k) of the special limbs (S = dn mod P) and divides by P: both switched
    components are the constant v = -(S div P)."""
    dn = -(-l // P)
    ps = [int(p) for p in primes[L0:L0 + P]]
    Pp = prod(ps)
    S = sum((dn * pow(Pp // p % p, -1, p) % p) * (Pp // p) for p in ps)
    assert S % Pp == dn
    return -(S // Pp)


def constant_limbs(primes, l, N, v):
    """(l, N) NTT-form limbs of the constant polynomial v."""
    return np.stack([np.full(N, v % int(primes[i]), dtype=np.uint64) for i in range(l)])


def check_worst_case_keyswitch(o, relin, rotate, elt, l, rng, closed_form=True):
    """The switched component (c2 for relinearize, c1 for a rotation by `elt`) all q - 1, the others random, the key
    max_key: `relin(c3)` and `rotate(c2)` are the implementation under test, run at level l and (exact convention)
    asserted against the closed form c + v.  Returns the inputs and outputs for a further comparison."""
    N, primes = o.N, o.primes
    v = constant_limbs(primes, l, N, keyswitch_worst_case_constant(primes, o.L0, o.P, l))
    rnd = [np.stack([rng.integers(0, primes[i], N, dtype=np.uint64) for i in range(l)]) for _ in range(3)]
    worst = all_max(primes, l, N)
    c3 = np.stack([rnd[0], rnd[1], worst])
    got = relin(c3)
    if closed_form:
        assert np.array_equal(got, o.add(c3[:2], np.stack([v, v]))), f"relinearize closed form, l={l}"
    c2 = np.stack([rnd[2], worst])
    got_r = rotate(c2)
    if closed_form:
        s0 = np.stack([o.galois_ntt(c2[0, i], elt) for i in range(l)])
        assert np.array_equal(got_r, np.stack([o.add(s0[None], v[None])[0], v])), f"rotate closed form, l={l}"
    return c3, got, c2, got_r
