"""An independent reference for the CKKS encoder and decoder: the canonical embedding and its inverse in x87 long
double (64-bit mantissa) with exact Python-integer rounding and CRT.  Plain numpy and Python ints; nothing from the
library under test.  tests/test_embedding_reference.py proves it against a naive DFT and the C oracle before it
judges the GPU kernels.

Conventions: zeta = exp(i pi / N), slot j is m(zeta^(g_j)) / scale with g_j = 5^j mod 2N = 4 s_j + 1.
zeta^(g N/2) = i for every such g, so with c_k = m_k + i m_(k+N/2), k < H = N/2,

    scale z_j = sum_k c_k zeta^k omega^(s_j k),  omega = zeta^4 = exp(2 pi i / H),

an H-point DFT (sign +1) of the twisted half-pairs read at s_j, and the encoder is its inverse:
c_k = (2/N) zeta^-k sum_s Z[s] omega^(-s k) with Z[s_j] = scale z_j."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs x87 extended precision (64-bit mantissa)"
PI = np.arccos(LD(-1))


def _bitrev_perm(n):
    bits = n.bit_length() - 1
    r = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        r |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    return r


def ld_fft(re, im, sign):
    """X_k = sum_t x_t exp(sign 2 pi i t k / n), n a power of two: iterative radix-2 DIT on long-double arrays, the
    twiddles from np.cos / np.sin of long-double angles.  Returns new (re, im)."""
    re = np.asarray(re, dtype=LD)
    im = np.asarray(im, dtype=LD)
    n = len(re)
    assert n >= 1 and n & (n - 1) == 0 and len(im) == n
    perm = _bitrev_perm(n)
    re, im = re[perm].copy(), im[perm].copy()
    length = 2
    while length <= n:
        half = length // 2
        ang = (np.arange(half, dtype=LD) / LD(length)) * (2 * PI) * sign    # k / length is exact
        wr, wi = np.cos(ang), np.sin(ang)
        r2, i2 = re.reshape(-1, length), im.reshape(-1, length)
        ar, ai = r2[:, :half].copy(), i2[:, :half].copy()
        br, bi = r2[:, half:], i2[:, half:]
        xr, xi = br * wr - bi * wi, br * wi + bi * wr
        r2[:, :half], i2[:, :half] = ar + xr, ai + xi
        r2[:, half:], i2[:, half:] = ar - xr, ai - xi
        length *= 2
    return re, im


def slot_positions(N):
    """s_j with 5^j = 4 s_j + 1 (mod 2N), j < N/2"""
    out = np.empty(N // 2, dtype=np.int64)
    e = 1
    for j in range(N // 2):
        out[j] = (e - 1) // 4
        e = e * 5 % (2 * N)
    return out


def _zeta_powers(N, sign):
    ang = (np.arange(N // 2, dtype=LD) / LD(N)) * PI * sign
    return np.cos(ang), np.sin(ang)


def encode_pre(z, N, scale):
    """The N long-double coefficients of the encoding of z (len(z) <= N/2 values, the remaining slots zero) at
    `scale`, BEFORE rounding."""
    z = np.asarray(z)
    H = N // 2
    assert len(z) <= H
    s = slot_positions(N)[:len(z)]
    zr, zi = np.zeros(H, dtype=LD), np.zeros(H, dtype=LD)
    zr[s] = np.real(z).astype(LD)
    if np.iscomplexobj(z):
        zi[s] = np.imag(z).astype(LD)
    fr, fi = ld_fft(zr, zi, -1)
    tr, ti = _zeta_powers(N, -1)
    f = LD(2) / LD(N) * LD(scale)    # 2/N and every scale used are powers of two or small: one rounding at most
    return np.concatenate([(fr * tr - fi * ti) * f, (fr * ti + fi * tr) * f])


def round_half_away(v):
    """round to the nearest integer, halves away from zero, exactly (long double in, integral long double out)"""
    v = np.asarray(v, dtype=LD)
    a = np.abs(v)
    t = np.floor(a)
    r = t + (a - t >= LD(0.5))      # a - t is exact; a + 0.5 would round when a >= 2^63
    return np.where(v < 0, -r, r)


def to_ints(v):
    """integral long doubles of magnitude below 2^128 -> Python ints, exactly (32-bit pieces)"""
    v = np.asarray(v, dtype=LD)
    assert np.all(v == np.floor(v)) and np.all(np.abs(v) < LD(2) ** 128)
    x = np.abs(v)
    two32 = LD(2 ** 32)
    pieces = []
    for _ in range(4):
        hi = np.floor(x / two32)
        pieces.append((x - hi * two32).astype(np.int64).tolist())
        x = hi
    neg = (v < 0).tolist()
    out = []
    for j in range(len(neg)):
        m = pieces[0][j] | pieces[1][j] << 32 | pieces[2][j] << 64 | pieces[3][j] << 96
        out.append(-m if neg[j] else m)
    return out


def from_ints(c):
    """Python ints -> long doubles, correctly rounded for |c| < 2^64 and to ~2^-63 relative above (top 128 bits)"""
    out = np.empty(len(c), dtype=LD)
    for j, x in enumerate(c):
        a = abs(x)
        sh = max(0, a.bit_length() - 128)
        a >>= sh
        v = LD(0)
        for p in (96, 64, 32, 0):
            v = v * LD(2 ** 32) + LD((a >> p) & 0xFFFFFFFF)
        v = v * LD(2) ** sh
        out[j] = -v if x < 0 else v
    return out


def slots_ref(c, N, scale):
    """(re, im) long-double slots z_j = sum_k c_k zeta^(g_j k) / scale of the N Python-int coefficients c"""
    H = N // 2
    assert len(c) == N
    v = from_ints(c) / LD(scale)
    lo, hi = v[:H], v[H:]
    tr, ti = _zeta_powers(N, +1)
    fr, fi = ld_fft(lo * tr - hi * ti, lo * ti + hi * tr, +1)
    s = slot_positions(N)
    return fr[s], fi[s]


def crt_centered(coefs, primes):
    """exact centred CRT: coefs[i][k] = c_k mod primes[i] -> Python ints c_k in (-Q/2, Q/2)"""
    primes = [int(q) for q in primes]
    assert len(coefs) == len(primes)
    Q = 1
    for q in primes:
        Q *= q
    acc = None
    for a, q in zip(coefs, primes):
        hat = Q // q
        w = hat * pow(hat % q, -1, q) % Q
        term = np.array([int(x) for x in np.asarray(a).tolist()], dtype=object) * w
        acc = term if acc is None else acc + term
    half = Q // 2
    return [x - Q if x > half else x for x in (int(y) % Q for y in acc)]


def coeffs_of(o, limbs):
    """the integer coefficients of a plaintext's NTT-form limbs (l, N): the oracle's INTT per limb + crt_centered"""
    limbs = np.asarray(limbs)
    l = limbs.shape[0]
    return crt_centered([o.intt(limbs[i], i) for i in range(l)], o.primes[:l])


def tie_window(pre, width=2.0 ** -12):
    """mask of the coefficients whose pre-rounding value is closer than `width` to a half-integer"""
    pre = np.asarray(pre, dtype=LD)
    frac = pre - np.floor(pre)
    return np.abs(frac - LD(0.5)) < LD(width)
