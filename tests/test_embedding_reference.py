"""The float64 CKKS encoder and decoder (fhs_kernels.hip k_encode / k_enc_period / k_ntt_fwd_from_dbl[_sp] / dbl_mod,
k_crt_compose[_jobs] / k_decode_fft, k_reduce_i128) against an extended-precision reference of the canonical
embedding (tests/_embedding_ref.py: x87 long double, exact Python-integer rounding and CRT over the oracle's INTT).

The CPU part proves the reference: against a naive long-double DFT, and against the C oracle's encoder / decoder (an
independent float64 N-point FFT).  The GPU part then pins

  (a) exact rounding (half away from zero) of every coefficient at scales 2^30 and 2^40, ties included;
  (b) at scales 2^59 and 2^70: every composed coefficient is one double reduced into every limb (both dbl_mod
      branches), and the float64 FFT's error is within 8x the oracle's own error on the same input;
  (c) the decoder from known integers (shortcut, its boundary, the fallbacks, GPU and host composition);
  (d) the precise encoder through all limbs (k_reduce_i128 with a nonzero high word of both signs).

Measured e_gpu / e_ref ratios are printed per vector (run with -s) and recorded in DESIGN.md §5."""
import random

import numpy as np
import pytest

import _embedding_ref as er

LD = np.longdouble
BITS = {"59": [59] * 4, "60": [60] * 4, "retrieval": [60, 40, 40, 60]}   # 3 data limbs + 1 special prime each


def _rand(rng, n, cplx, sigma=1.0):
    return rng.normal(0, sigma, n) + 1j * rng.normal(0, sigma, n) if cplx else rng.normal(0, sigma, n)


def _want(z, N, scale):
    pre = er.encode_pre(z, N, scale)
    return pre, er.to_ints(er.round_half_away(pre))


def _maxdiff(a, b):
    return max(abs(x - y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- CPU: the reference itself
def _naive_exponents(N):
    g = [pow(5, j, 2 * N) for j in range(N // 2)]
    return np.array(g, dtype=np.int64)


def _naive_angles(N, kmax):
    """pi (g_j k mod 2N) / N as long doubles, [j, k]: the exponent reduced in exact integer arithmetic"""
    e = np.outer(_naive_exponents(N), np.arange(kmax, dtype=np.int64)) % (2 * N)
    return er.PI * e.astype(LD) / LD(N)


def test_reference_equals_naive_dft():
    """encode_pre and slots_ref (H-point FFT forms) against the defining sums evaluated term by term in long
    double, N = 256: 1e-16 relative."""
    N, H = 256, 128
    rng = np.random.default_rng(1)
    ang = _naive_angles(N, H)                      # [j, k]
    cr, ci = np.cos(ang), np.sin(ang)
    for scale, n in ((2.0 ** 40, H), (2.0 ** 59, H - 1), (1.0, 1)):
        z = _rand(rng, n, True)
        zr, zi = np.zeros(H, dtype=LD), np.zeros(H, dtype=LD)
        zr[:n], zi[:n] = z.real, z.imag
        # c_k = (2/N) sum_j z_j zeta^(-g_j k): real part -> c_k, imaginary part -> c_(k+H)
        re = (zr @ cr + zi @ ci) * 2 / N * LD(scale)
        im = (zi @ cr - zr @ ci) * 2 / N * LD(scale)
        naive = np.concatenate([re, im])
        pre = er.encode_pre(z, N, scale)
        assert np.max(np.abs(pre - naive)) <= 1e-16 * np.max(np.abs(naive)), (scale, n)
    ang = _naive_angles(N, N)
    cr, ci = np.cos(ang), np.sin(ang)
    for bits, scale in ((45, 2.0 ** 40), (100, 2.0 ** 59)):
        pyr = random.Random(bits)
        c = [pyr.randrange(-2 ** bits, 2 ** bits) for _ in range(N)]
        c[1] = 0
        v = er.from_ints(c) / LD(scale)
        sr, si = er.slots_ref(c, N, scale)
        nr, ni = cr @ v, ci @ v
        tol = 1e-16 * max(np.max(np.abs(nr)), np.max(np.abs(ni)))
        assert max(np.max(np.abs(sr - nr)), np.max(np.abs(si - ni))) <= tol, bits


def test_reference_integer_helpers():
    """round_half_away / to_ints / from_ints / crt_centered on hand-made values"""
    v = np.array([2.5, -2.5, -0.5, 1.5, 3.0, 0.0, 0.49999, -1.50001, 2.0 ** 63 + 2048, -(2.0 ** 100)], dtype=LD)
    assert er.to_ints(er.round_half_away(v)) == [3, -3, -1, 2, 3, 0, 0, -2, 2 ** 63 + 2048, -2 ** 100]
    big = LD(2) ** 63 + LD(1)                    # needs all 64 bits of the mantissa: odd and above 2^63
    assert er.to_ints(er.round_half_away(np.array([big, -big]))) == [2 ** 63 + 1, -2 ** 63 - 1]
    assert er.to_ints(er.from_ints([2 ** 63 + 1, -(2 ** 64 - 1), 0, 12345])) == [2 ** 63 + 1, -(2 ** 64 - 1), 0, 12345]
    assert er.from_ints([3 << 400])[0] == LD(3) * LD(2) ** 400
    primes = [2 ** 61 - 1, 2 ** 31 - 1, 2 ** 19 - 1, 2 ** 17 - 1, 2 ** 13 - 1]      # Mersenne primes: Q ~ 2^141
    Q = int(np.prod(primes, dtype=object))
    cs = [0, 1, -1, (Q - 1) // 2, -(Q - 1) // 2, 2 ** 100 + 7, -2 ** 130 - 5]
    coefs = [np.array([c % q for c in cs], dtype=np.uint64) for q in primes]
    assert er.crt_centered(coefs, primes) == cs
    assert list(er.tie_window(np.array([2.5, 2.5 + 2.0 ** -13, 2.5 + 2.0 ** -11, -0.5 - 2.0 ** -13, 3.0], dtype=LD))) \
        == [True, True, False, True, False]


def _oracle(orc, N, bits):
    primes = orc.create_coeff_modulus(N, bits)
    return orc.Oracle(N, primes, 1)


def test_reference_equals_oracle_encoder(orc):
    """The oracle's encoder (float64 N-point FFT, cos/sin twiddles, round(), double_to_mod into every limb) against
    the rounded reference at N = 4096, 59-bit chain, l = 3, complex N(0,1) input, scales 2^30 and 2^40: equal on
    every coefficient at least 2^-12 from a half-integer, within 1 inside that window."""
    N = 4096
    o = _oracle(orc, N, BITS["59"])
    rng = np.random.default_rng(2)
    for scale in (2.0 ** 30, 2.0 ** 40):
        z = _rand(rng, N // 2, True)
        pre, want = _want(z, N, scale)
        limbs = o.encode(z, scale, 3)
        got = er.coeffs_of(o, limbs)
        assert _representable(got)
        c1 = o.intt(limbs[1], 1)                   # one residue of one limb off by one: no longer a double
        c1[5] = (int(c1[5]) + 1) % o.primes[1]
        limbs[1] = o.ntt(c1, 1)
        assert not _representable(er.coeffs_of(o, limbs))
        win = er.tie_window(pre)
        d = np.array([abs(a - b) for a, b in zip(got, want)], dtype=np.int64)
        print(f"oracle encode scale=2^{int(np.log2(scale))}: mismatches {int((d != 0).sum())}, in window "
              f"{int(win.sum())}")
        assert not d[~win].any()
        assert d.max() <= 1


def test_reference_equals_oracle_decoder(orc):
    """The oracle's decoder (multi-word CRT to double, float64 N-point FFT) on limbs built from known integers
    against slots_ref: below 1e-13 of the RMS slot magnitude."""
    N = 4096
    o = _oracle(orc, N, [59] * 8)
    for l, bits, scale in ((3, 45, 2.0 ** 40), (3, 100, 2.0 ** 59), (7, 400, 2.0 ** 100)):
        pyr = random.Random(l * 1000 + bits)
        Q = 1
        for q in o.primes[:l]:
            Q *= q
        bound = min(2 ** bits, Q // 2)
        c = [pyr.randrange(-bound, bound) for _ in range(N)]
        c[1] = 0
        limbs = np.stack([o.ntt(np.array([x % q for x in c], dtype=np.uint64), i) for i, q in enumerate(o.primes[:l])])
        assert er.coeffs_of(o, limbs) == c
        sr, si = er.slots_ref(c, N, scale)
        z = o.decode(limbs, scale)
        err = max(np.max(np.abs(z.real.astype(LD) - sr)), np.max(np.abs(z.imag.astype(LD) - si)))
        rms = np.sqrt(np.mean(sr * sr + si * si))
        print(f"oracle decode l={l} |c|<2^{bits}: err/rms = {float(err / rms):.2e}")
        assert err < 1e-13 * rms


# ----------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


class _Ring:
    def __init__(self, ph, orc, N, bits, seed=77):
        primes = ph.create_coeff_modulus(N, list(bits))
        parms = ph.params(ph.scheme_type.ckks)
        parms.set_poly_modulus_degree(N)
        parms.set_special_modulus_size(1)
        parms.set_coeff_modulus(primes)
        self.ph, self.N, self.L0 = ph, N, len(bits) - 1
        self.ctx = ph.context(parms)
        self.enc = ph.ckks_encoder(self.ctx)
        self.primes = [int(q) for q in primes]
        self.o = orc.Oracle(N, self.primes, 1)
        self.seed = seed
        self._sk = None

    @property
    def sk(self):
        if self._sk is None:
            self._sk = self.ph.secret_key(self.ctx, seed=self.seed)
        return self._sk

    def encode(self, z, scale, ci):
        if np.iscomplexobj(z):
            return self.enc.encode_complex_vector(self.ctx, z, scale, ci)
        return self.enc.encode_double_vector(self.ctx, z, scale, ci)

    def coeffs(self, pt):
        return er.coeffs_of(self.o, pt.to_numpy())


@pytest.fixture(scope="module")
def rings(ph, orc):
    """one context + oracle per (N, prime set), shared by every case of this module"""
    cache = {}

    def get(N, bits):
        key = (N, tuple(bits))
        if key not in cache:
            cache[key] = _Ring(ph, orc, N, bits)
        return cache[key]
    yield get
    cache.clear()


def _representable(c):
    """every coefficient is exactly a double: the encoder rounds to ONE integral double and reduces that number into
    every limb, so a wrong residue in any limb composes to a value of the size of Q, which is not one"""
    return all(int(float(x)) == x for x in c)


# ---- (a) exact regime
@pytest.mark.gpu
@pytest.mark.parametrize("N,name", [(1024, "59"), (1024, "60"), (1024, "retrieval"), (4096, "59"), (16384, "59"),
                                    (32768, "59"), (32768, "60")])
def test_encoder_rounds_exactly_at_small_scales(rings, N, name):
    """Scales 2^30 and 2^40, |z| ~ 1: the float64 pre-rounding error is ~2^33 2^-50 = 2^-17, so every coefficient
    whose exact value is at least 2^-12 from a half-integer (2^5 of room) must be the reference's rounding half away
    from zero, and the others within 1.  The excluded share, from the reference alone, is capped at 0.2 % (expected
    2^-11).  Real and complex, n = N/2, N/2 - 1 and 1, chain index 1 and 2, a tiled row (sparse form)."""
    r = rings(N, BITS[name])
    H = N // 2
    rng = np.random.default_rng(N + len(name))
    cases = [(2.0 ** 30, True, H, 1), (2.0 ** 40, False, H, 2), (2.0 ** 40, True, H - 1, 2),
             (2.0 ** 30, False, H - 1, 1), (2.0 ** 40, True, 1, 1), (2.0 ** 30, False, 1, 2)]
    vecs = [(s, _rand(rng, n, cplx), ci) for s, cplx, n, ci in cases]
    vecs.append((2.0 ** 40, np.tile(_rand(rng, H // 4, True), 4), 1))
    excluded = total = 0
    for scale, z, ci in vecs:
        pre, want = _want(z, N, scale)
        got = r.coeffs(r.encode(z, scale, ci))
        assert _representable(got)
        win = er.tie_window(pre)
        d = np.array([abs(a - b) for a, b in zip(got, want)], dtype=object)
        tag = f"N={N} {name} scale=2^{int(np.log2(scale))} n={len(z)} ci={ci}"
        print(f"exact {tag}: mismatches {sum(1 for x in d if x)}, in window {int(win.sum())}")
        assert not any(d[~win]), tag
        assert max(d) <= 1, tag
        excluded += int(win.sum())
        total += N
    assert excluded <= 0.002 * total, (excluded, total)


@pytest.mark.gpu
@pytest.mark.parametrize("N,name", [(256, "59"), (1024, "59"), (1024, "60"), (32768, "59")])
def test_encoder_ties_round_half_away(rings, N, name):
    """The constant vector z_j = a + b i is exact input (zeta^(g_j N/2) = i for every slot): at scale 1 it encodes to
    a + b X^(N/2), so coefficients 0 and N/2 are round-half-away of a and b and every other one is 0.  A constant
    row takes the sparse form when n = N/2 (rings of 512 and above).  The dense form is reached by perturbing the
    last value by 2^-10: coefficient 0 becomes a + 2^-9 / N exactly (bin 0 and the constant part of a radix-2 FFT
    involve only the twiddle 1 and exact sums), coefficient N/2 stays the exact tie b, the others are below 2^-18."""
    r = rings(N, BITS[name])
    H = N // 2
    for a, b, c0, ch in ((2.5, -2.5, 3, -3), (-0.5, 1.5, -1, 2), (3.0, 0.0, 3, 0)):
        want = [0] * N
        want[0], want[H] = c0, ch
        z = np.full(H, a + 1j * b)
        assert r.coeffs(r.encode(z, 1.0, 1)) == want, (a, b, "constant row")
        z[-1] += 2.0 ** -10
        wantd = er.to_ints(er.round_half_away(er.encode_pre(z, N, 1.0)))
        assert wantd[H] == ch and wantd[0] == (0 if a == -0.5 else c0) and not any(wantd[1:H] + wantd[H + 1:])
        assert r.coeffs(r.encode(z, 1.0, 1)) == wantd, (a, b, "dense row")
        want[H] = 0
        x = np.full(H, a)                                        # the real entry point
        assert r.coeffs(r.encode(x, 1.0, 2)) == want, (a, "real constant row")


# ---- (b) float64 regime
def _check_float64(r, z, scale, ci, tag, extra=0, pt=None, got=None):
    """representability + max |c_gpu - round(pre)| <= 8 e_ref + 1 (+ extra), e_ref the oracle encoder's error on the
    same input.  The factor 8 covers two correct float64 FFTs of different butterfly order, contraction and table
    twiddles; a lost stage, a float32 intermediate or a wrong twiddle misses by more than 2^20 times that."""
    N, l = r.N, r.L0 + 1 - ci
    pre, want = _want(z, N, scale)
    if got is None:
        got = r.coeffs(pt if pt is not None else r.encode(z, scale, ci))
        assert _representable(got), tag
    e_ref = _maxdiff(er.coeffs_of(r.o, r.o.encode(z, scale, l)), want)
    e_gpu = _maxdiff(got, want)
    print(f"encode {tag}: e_gpu={e_gpu} e_ref={e_ref} ratio={e_gpu / max(e_ref, 1):.3f}")
    assert e_gpu <= 8 * e_ref + 1 + extra, (tag, e_gpu, e_ref)
    return pre, got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["59", "60", "retrieval"])
@pytest.mark.parametrize("N", [1024, 16384, 32768])
def test_encoder_float64_error_and_limb_consistency(rings, N, name):
    """Scales 2^59 and 2^70 (at 2^70 the coefficients straddle 9.2e18, so both dbl_mod branches occur in one vector):
    the smallest ring, the largest unsplit FFT (N = 16384) and the split FFT / half-limb NTT / lazy encoder NTT
    (N = 32768); fold1 (59-bit), reduce64 + Harvey (60-bit) and mixed 60/40-bit primes; real and complex, n = N/2,
    N/2 - 1, 1, chain index 1 and 2."""
    r = rings(N, BITS[name])
    H = N // 2
    rng = np.random.default_rng(3 * N + len(name))
    cases = [(2.0 ** 59, False, H, 1), (2.0 ** 59, True, H - 1, 2), (2.0 ** 59, True, 1, 1), (2.0 ** 59, False, H, 2),
             (2.0 ** 70, True, H, 1), (2.0 ** 70, False, H - 1, 2), (2.0 ** 70, False, 1, 2), (2.0 ** 70, True, H, 2)]
    for scale, cplx, n, ci in cases:
        z = _rand(rng, n, cplx)
        tag = f"N={N} {name} scale=2^{int(np.log2(scale))} {'complex' if cplx else 'real'} n={n} ci={ci}"
        pre, _ = _check_float64(r, z, scale, ci, tag)
        if scale == 2.0 ** 70 and n >= H - 1:     # from the reference alone: both dbl_mod branches are exercised
            a = np.abs(pre)
            assert (a >= 9.3e18).sum() > N // 64 and ((a < 9.1e18) & (a > 1)).sum() > N // 64, tag


@pytest.mark.gpu
@pytest.mark.parametrize("N,ts", [(1024, (2, 4)), (2048, (8,)), (32768, (8, 16))])
@pytest.mark.parametrize("name", ["59", "60"])
def test_sparse_form_float64_error_and_zeros(rings, N, ts, name):
    """np.tile'd rows take the sparse form p(X^t'), t' = min(t, 8) (N = 2048, t = 8: M = 256, its floor): the same
    bound against the dense reference of the tiled vector, and exact zeros off the multiples of t'."""
    r = rings(N, BITS[name])
    H = N // 2
    rng = np.random.default_rng(5 * N + len(name))
    for t in ts:
        for scale, cplx, ci in ((2.0 ** 59, True, 1), (2.0 ** 70, False, 2)):
            z = np.tile(_rand(rng, H // t, cplx), t)
            tag = f"N={N} {name} tiled t={t} scale=2^{int(np.log2(scale))} {'complex' if cplx else 'real'} ci={ci}"
            _, got = _check_float64(r, z, scale, ci, tag)
            tt = min(t, 8)
            assert not any(c for k, c in enumerate(got) if k % tt), tag
            assert any(got[::tt])


def _bg_rows(W, D, G, slots):
    """the caller's diagonal rows: extraction, giant-group roll, tiling to the slot count"""
    j = np.arange(D)
    d = W[j[None, :], (j[None, :] + j[:, None]) % D]
    r = d.copy()
    for g in range(1, (D + G - 1) // G):
        s, e = g * G, min((g + 1) * G, D)
        r[s:e, g * G:] = d[s:e, :D - g * G]
        r[s:e, :g * G] = d[s:e, D - g * G:]
    return np.tile(r, (1, slots // D))


@pytest.mark.gpu
def test_other_encode_entry_points(rings):
    """encode_matrix_diagonals (rows_known: only the first period is read), a batch of >= 32 tiled rows (stored
    compact only) and encode_encrypt_batch + decrypt (c_ref + e, |e| <= 21: k_sample_small's centred binomial of
    2 x 21 bits) at N = 1024, 59-bit chain, scale 2^59."""
    N, H, scale = 1024, 512, 2.0 ** 59
    r = rings(N, BITS["59"])
    rng = np.random.default_rng(11)
    D = 128
    G = int(np.ceil(np.sqrt(D)))
    W = rng.normal(0, 1, (D, D))
    rows = _bg_rows(W, D, G, H)
    pts = r.enc.encode_matrix_diagonals(r.ctx, W, G, scale, chain_index=1)
    for k in (0, G, D - 1):
        _, got = _check_float64(r, rows[k], scale, 1, f"diagonal {k}", pt=pts[k])
        assert not any(c for j, c in enumerate(got) if j % 4)             # period 128 in 512 slots: t = 4
    tiled = np.tile(rng.normal(0, 1, (40, H // 4)), (1, 4))
    batch = r.enc.encode_double_vector_batch(r.ctx, tiled, scale, chain_index=2)
    _check_float64(r, tiled[7], scale, 2, "compact batch row 7", pt=batch[7])
    zc = _rand(rng, H, True).reshape(1, H).repeat(2, axis=0)
    zc[1] = _rand(rng, H, True)
    cts = r.sk.encode_encrypt_batch(r.ctx, zc, scale, chain_index=1)
    dec = r.coeffs(r.sk.decrypt(r.ctx, cts[1]))
    _check_float64(r, zc[1], scale, 1, "encode_encrypt_batch row 1", extra=21, got=dec)


# ---- (c) decoder from known integers
def _limbs_of(o, c, l):
    return np.stack([o.ntt(np.array([x % q for x in c], dtype=np.uint64), i) for i, q in enumerate(o.primes[:l])])


def _slot_err(z, sr, si):
    z = np.asarray(z)
    return max(np.max(np.abs(z.real.astype(LD) - sr)), np.max(np.abs(z.imag.astype(LD) - si)))


def _check_decode(r, c, l, scale, tag, batch_with=None):
    """max |z_gpu - slots_ref| <= 8 e_ref + 2^-52 rms|z|, e_ref = the oracle decoder's error on the same limbs (the
    factor 8 as for the encoder; the second term for an oracle that happens to be exact)"""
    o, N = r.o, r.N
    limbs = _limbs_of(o, c, l)
    pt = r.ph.plaintext_from_numpy(r.ctx, limbs, r.L0 + 1 - l, scale)
    sr, si = er.slots_ref(c, N, scale)
    rms = np.sqrt(np.mean(sr * sr + si * si))
    e_ref = _slot_err(o.decode(limbs, scale), sr, si)
    bound = 8 * e_ref + LD(2.0 ** -52) * rms
    e_gpu = _slot_err(r.enc.decode_complex_vector(r.ctx, pt), sr, si)
    print(f"decode {tag}: e_gpu/rms={float(e_gpu / rms):.2e} e_ref/rms={float(e_ref / rms):.2e} "
          f"ratio={float(e_gpu / e_ref) if e_ref else float('inf'):.3f}")
    assert e_gpu <= bound, (tag, float(e_gpu), float(e_ref))
    if batch_with is not None:
        batch_with.append((pt, sr, si, bound, tag))


def _known_ints(seed, N, bound):
    pyr = random.Random(seed)
    c = [pyr.randrange(-bound + 1, bound) for _ in range(N)]
    c[1], c[2], c[3] = 0, bound - 1, -(bound - 1)      # a zero and both signs at the edge of the range
    return c


@pytest.mark.gpu
def test_decoder_from_known_integers(rings):
    """N = 4096, 9 data limbs: the shortcut (l = 6, scale 2^40, |c| < 2^45: 3 limbs composed, checked against 3), its
    last accepted value (Q_3 - 1)/2 and the first that must fall back (Q_3 + 1)/2, all limbs on the GPU (l = 3, scale
    2^59, |c| ~ 2^100), the widest GPU composition (l = 7, uniform below Q_7/2, scale 2^100: multi-word -> double)
    and the check failure that takes the host composition (l = 9, |c| ~ 2^400); decode_batch over the l = 6 cases."""
    N = 4096
    r = rings(N, [59] * 10)
    q = r.primes
    Q3, Q7 = q[0] * q[1] * q[2], int(np.prod([int(x) for x in q[:7]], dtype=object))
    batch = []
    c = _known_ints(1, N, 2 ** 45)
    _check_decode(r, c, 6, 2.0 ** 40, "l=6 shortcut", batch)
    for name, v in (("(Q3-1)/2", (Q3 - 1) // 2), ("(Q3+1)/2", (Q3 + 1) // 2)):
        c2 = list(c)
        c2[5] = v
        _check_decode(r, c2, 6, 2.0 ** 40, f"l=6 with {name}", batch)
        c2[5] = -v
        _check_decode(r, c2, 6, 2.0 ** 40, f"l=6 with -{name}")
    pts = [b[0] for b in batch]
    zb = r.enc.decode_batch(r.ctx, pts, nslots=64)
    for k, (_, sr, si, bound, tag) in enumerate(batch):
        assert _slot_err(zb[k], sr[:64], si[:64]) <= bound, f"decode_batch: {tag}"
    _check_decode(r, _known_ints(2, N, 2 ** 100), 3, 2.0 ** 59, "l=3 all limbs")
    _check_decode(r, _known_ints(3, N, Q7 // 2), 7, 2.0 ** 100, "l=7 widest GPU composition")
    _check_decode(r, _known_ints(4, N, 2 ** 400), 9, 2.0 ** 59, "l=9 host composition")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 32768])
def test_decoder_small_and_split_rings(rings, N):
    """l = 3, scale 2^40, |c| < 2^45 at the smallest ring and at N = 32768 (split decode FFT)"""
    r = rings(N, BITS["59"])
    _check_decode(r, _known_ints(N, N, 2 ** 45), 3, 2.0 ** 40, f"N={N} l=3")


# ---- (d) precise encoder through all limbs
@pytest.mark.gpu
@pytest.mark.parametrize("log_scale", [59, 100])
def test_precise_encoder_all_limbs(rings, log_scale):
    """encode_complex_vector_batch(precise=True) at N = 1024, l = 3 (Q ~ 2^177 > 2^128): composed over ALL limbs,
    |c - round(pre)| <= 1 + 2^-56 max|pre| (both sides are 64-bit-mantissa FFTs of ~10 stages: 2^8 over the unit
    roundoff; one wrong residue misses by 2^50 times that).  At 2^100 the coefficients are ~2^95: k_reduce_i128 sees
    a nonzero high word of both signs."""
    N, H = 1024, 512
    r = rings(N, BITS["59"])
    scale = 2.0 ** log_scale
    rng = np.random.default_rng(log_scale)
    z = np.stack([_rand(rng, H, True), _rand(rng, H, True) * 1e-3, _rand(rng, H, True) * 4])
    pts = r.enc.encode_complex_vector_batch(r.ctx, z, scale, chain_index=1, precise=True)
    for k in range(len(z)):
        pre, want = _want(z[k], N, scale)
        got = r.coeffs(pts[k])
        bound = 1 + int(np.max(np.abs(pre)) * LD(2.0 ** -56))
        e = _maxdiff(got, want)
        print(f"precise scale=2^{log_scale} row {k}: e={e} bound={bound}")
        assert e <= bound, (k, e, bound)
        if log_scale == 100 and k != 1:
            assert min(got) < -2 ** 64 and max(got) > 2 ** 64
