"""The launch-coverage matrix (tests/test_launch_coverage.py): the smallest oracle-checked cases that between them
launch every kernel compiled into libfhespear_hip.so (tests/golden/kernel_manifest.json), ring by ring.

Rule of this file: every library call made while the launch ledger is armed has its output compared -- limbs with
np.array_equal against the CPU oracle, the float64 encoder and decoder against the extended-precision reference of
tests/_embedding_ref.py in the way tests/test_embedding_reference.py does.  A case that only launched a kernel
without judging what it wrote would turn the ledger into a list of names.

Chains (create_coeff_modulus sizes, every prime listed; the dispatch flags are those of fhs_tables.h for these
primes at every ring):

    name   sizes              P   modup_dp  md_xform  conv_b59  all_b59
    X59    [59]*9             3   3         1         1         1
    X60s   [60]*6 + [59]*3    3   3         1         0         0
    S59    [59]*5             1   1         0         0         1
    S60    [59]*4 + [60]      1   1         0         0         0
"""
import numpy as np

import _edge_inputs as ei
import _embedding_ref as er
from test_edge_operands import SCALE, make_ctx, same, up
from test_embedding_reference import _Ring, _check_decode, _known_ints, _maxdiff, _representable, _want
from test_gpu_parity import rand_ct, rand_pt

LD = np.longdouble
RINGS = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768)
STEPS = (1, -1, 3)
GIANT = 2                        # the BSGS case: G = 2, B = 2, D = 4 (one giant rotation, by 2)
SEED = 177

CHAINS = {"X59": ([59] * 9, 3), "X60s": ([60] * 6 + [59] * 3, 3), "S59": ([59] * 5, 1), "S60": ([59] * 4 + [60], 1)}
# levels of the three-rotations-and-one-relinearisation case.  N >= 512: X59 l = 6 -> k_modup_h<.., 3, true>, l = 5 ->
# k_modup_h<.., 0, false>, both k_moddown_h<.., true, true> (N = 32768: its SPLIT form, 2 l R < 256); X60s ->
# k_modup_h<.., 3, false>, k_moddown_h<.., true, false>; S59 -> <.., 1, true>, <.., false, true>; S60 -> <.., 1, false>,
# <.., false, false>.  N = 256: k_modup<8>, k_moddown<8>, k_ks_intt<8> throughout.
KS_LEVELS = {"X59": (6, 5), "X60s": (6,), "S59": (4,), "S60": (4,)}

# Kernels that no argument can launch, each with the line that proves it (fhs_kernels.hip).  Nothing else may be
# listed, and a listed kernel that IS launched fails the test (a stale exemption).
_SPLIT_WHY = ("ks_moddown_stage selects the SPLIT form only under `LOGN == 15 && nwg < FHS_SPLIT_MAX_WG`; its "
              "function-pointer table instantiates it for every LOGN >= 9")
EXEMPT = {f"k_moddown_h<{n}, true, true, true>": _SPLIT_WHY for n in range(9, 15)}
# Not exempt: k_rescale_intt<14, true> (FHS_NTT_LAUNCH from FHS_FULL_FORM_MAX_WG = 256 workgroups).  The single rescale
# passes ncomp <= 3, but fhs_multiply_relin_many passes ocomp * R and fhs_dot_product_many ocomp * C components to
# launch_rescale, and launch_last_limbs_intt (fhs_weighted_sums) 2 * F: 128 pairs, chunks or inputs at N = 16384
# reach it.  case_multiply_many_at_128_pairs launches it.


def logn_of(kernel):
    """LOGN of a per-ring instantiation (first template argument 8..15 of every family but the two below); None for
    the ring-independent kernels."""
    if "<" not in kernel or kernel.startswith(("k_bsgs_inner<", "k_dot_tensor<")):
        return None
    return int(kernel[kernel.index("<") + 1:].split(",")[0].rstrip(">"))


class KsEnv:
    """One chain at one ring: context, seeded keys for STEPS, the giant step and relinearisation, and the oracle with
    the same keys.  The generated secret and every Galois key are compared on creation."""

    def __init__(self, ph, N, chain, mode="exact"):
        bits, P = CHAINS[chain]
        self.ph, self.N, self.P, self.chain = ph, N, P, chain
        steps = STEPS + (GIANT,)
        self.ctx, self.sk, self.o = make_ctx(ph, N, bits, P, steps=steps, seed=SEED, mode=mode)
        self.s = self.o.gen_secret(SEED)
        same(self.sk.export(), self.s, f"{chain}: secret key")
        self.gk = self.sk.create_galois_keys(self.ctx)
        self.elt = {st: ph.get_elt_from_step(st, N) for st in steps}
        self.okey = {st: self.o.gen_galois_key(SEED, self.s, e) for st, e in self.elt.items()}
        for st in steps:
            same(self.gk.export(self.elt[st]), self.okey[st], f"{chain}: Galois key of step {st}")

    def relin_keys(self):
        return self.sk.gen_relinkey(self.ctx), self.o.gen_relin_key(SEED, self.s)

    def near_half_ct(self, rng, l):
        return np.stack([rand_pt(self.o, rng, l), ei.to_ntt(self.o, ei.near_half_digits(self.o.primes, self.P, l, self.N, rng))])


# ------------------------------------------------------------------ per-ring cases
def case_keyswitch_selectors(ph, N, envs):
    """Per chain and level: three rotations queued before any readback (one hoisted ModUp) and one relinearisation,
    the switched component next to Q_S / 2 in every digit."""
    for chain, levels in KS_LEVELS.items():
        e = envs(chain)
        rlk, orlk = e.relin_keys()
        rng = np.random.default_rng(N + len(chain))
        for l in levels:
            a = e.near_half_ct(rng, l)
            A = up(ph, e.ctx, e.o, a)
            outs = [ph.rotate(e.ctx, A, st, e.gk) for st in STEPS]
            for st, out in zip(STEPS, outs):
                same(out.to_numpy(), e.o.rotate_elt(a, e.okey[st], e.elt[st]), f"{chain} l={l}: rotate by {st}")
            c3 = np.concatenate([rand_ct(e.o, rng, 2, l), e.near_half_ct(rng, l)[1:]])
            same(ph.relinearize(e.ctx, up(ph, e.ctx, e.o, c3), rlk).to_numpy(), e.o.relinearize(c3, orlk),
                 f"{chain} l={l}: relinearize")


def batch_size(N):
    return 22 if N == 32768 else 43


def case_keyswitch_batch(ph, N, envs):
    """One queued batch of distinct inputs on X59 at l = 6.  43 inputs: l U = 258 >= 256 workgroups select
    k_ks_intt_h (N = 512 .. 16384; the small cases take the full-limb k_ks_intt) and P 2 R = 258 selects
    k_ks_special_intt<14, true>.  N = 32768: 22 inputs, 2 l R = 264 selects the non-SPLIT k_moddown_h<15, true, true>."""
    e = envs("X59")
    l, R = 6, batch_size(N)
    rng = np.random.default_rng(N + R)
    ins = [e.near_half_ct(rng, l) if i < 2 else rand_ct(e.o, rng, 2, l) for i in range(R)]
    cts = [up(ph, e.ctx, e.o, a) for a in ins]
    outs = [ph.rotate(e.ctx, c, STEPS[i % 3], e.gk) for i, c in enumerate(cts)]
    for i, (a, out) in enumerate(zip(ins, outs)):
        st = STEPS[i % 3]
        same(out.to_numpy(), e.o.rotate_elt(a, e.okey[st], e.elt[st]), f"batch of {R}: input {i}, step {st}")


def case_bsgs(ph, N, envs):
    """bsgs_multiply_accumulate with B = 2 on X59 (l = 6): k_bsgs_inner, the giant-step key switch (k_ks_ip with
    k_ks_ip_sum, k_giant_sum) and k_giant_final, against Oracle.bsgs_loop; the diagonals are the oracle's own."""
    e = envs("X59")
    G, B, D, l = GIANT, 2, 4, 6
    rng = np.random.default_rng(N + 4)
    baby_np = [rand_ct(e.o, rng, 2, l) for _ in range(G)]
    baby = [up(ph, e.ctx, e.o, a) for a in baby_np]
    pts = ph.random_plaintexts(e.ctx, 7, D, 1, SCALE)
    pn = [e.o.random_plaintext(7, k, l) for k in range(D)]
    for k in range(D):
        same(pts[k].to_numpy(), pn[k], f"random plaintext {k}")
    y = ph.bsgs_multiply_accumulate(e.ctx, baby, pts, G, B, D, e.gk)
    same(y.to_numpy(), e.o.bsgs_loop(baby_np, pn, [None, e.okey[GIANT]], G, B, D), "bsgs_multiply_accumulate")


def case_giant_final_at_128_limbs(ph, N, envs):
    """N = 16384 only: k_giant_final takes its half-limb form K<14, true> from l 2 >= 256 workgroups, i.e. l >= 128.
    The smallest such matvec: a 128 + 8 chain of 59-bit primes (modup_dp = 0: k_modup_h<14, 0, false>), G = 1,
    B = 2, D = 2 -- one baby step, one giant rotation by 1 under a 570 MB switching key."""
    if N != 16384:
        return
    L0, P, seed = 128, 8, SEED + 1
    ctx, sk, o = make_ctx(ph, N, [59] * (L0 + P), P, steps=(1,), seed=seed)
    s = o.gen_secret(seed)
    same(sk.export(), s, "128 + 8: secret key")
    gk = sk.create_galois_keys(ctx)
    elt = ph.get_elt_from_step(1, N)
    okey = o.gen_galois_key(seed, s, elt)
    same(gk.export(elt), okey, "128 + 8: Galois key of step 1")
    rng = np.random.default_rng(N + L0)
    a = rand_ct(o, rng, 2, L0)
    pts = ph.random_plaintexts(ctx, 9, 2, 1, SCALE)
    pn = [o.random_plaintext(9, k, L0) for k in range(2)]
    for k in range(2):
        same(pts[k].to_numpy(), pn[k], f"128 + 8: random plaintext {k}")
    y = ph.bsgs_multiply_accumulate(ctx, [up(ph, ctx, o, a)], pts, 1, 2, 2, gk)
    same(y.to_numpy(), o.bsgs_loop([a], pn, [None, okey], 1, 2, 2), "128 + 8: bsgs_multiply_accumulate")


def case_multiply_many_at_128_pairs(ph, N, envs):
    """N = 16384 only: multiply_relin_many of 128 pairs on [60, 40, 40, 60], P = 1 at l = 2 (pair i is (x_i, x_{i+1})).
    Its rescale is one launch_rescale over 2 * 128 = 256 components: k_rescale_intt<14, true> (and, (l - 1) * 256
    workgroups, k_rescale_ntt<14, true>) into the 128 results' block.  tests/test_batched_rings.py runs both sides of
    this threshold with the ledger's names asserted."""
    if N != 16384:
        return
    n, l, seed = 128, 2, SEED + 2
    ctx, sk, o = make_ctx(ph, N, [60, 40, 40, 60], 1, steps=(1,), seed=seed)
    s = o.gen_secret(seed)
    same(sk.export(), s, "128 pairs: secret key")
    rlk, orlk = sk.gen_relinkey(ctx), o.gen_relin_key(seed, s)
    rng = np.random.default_rng(N + n)
    xs = [rand_ct(o, rng, 2, l) for _ in range(n + 1)]
    cts = [up(ph, ctx, o, a) for a in xs]
    outs = ph.multiply_relin_many(ctx, cts[:n], cts[1:], rlk)
    assert len(outs) == n
    for i, out in enumerate(outs):
        assert out.size() == 2 and out.chain_index() == o.L0 + 2 - l
        same(out.to_numpy(), o.rescale(o.relinearize(o.multiply(xs[i], xs[i + 1]), orlk)), f"128 pairs: pair {i}")


def case_seal(ph, N, envs):
    """SEAL convention on S60: hoisting() without a zero coefficient shares one decomposition (k_seal_mask,
    k_seal_corr), with zeros present it takes SEAL's per-rotation path (k_galois_perm_batch)."""
    e = envs("S60", "seal")
    l = 4
    rng = np.random.default_rng(N + 5)
    for zeros, path in ((False, 0), (True, 1)):
        c1 = ei.near_half_digits(e.o.primes, 1, l, N, rng, exclude_zero=not zeros)
        assert (c1 == 0).any() == zeros
        a = np.stack([rand_pt(e.o, rng, l), ei.to_ntt(e.o, c1)])
        h0 = e.ctx.seal_hoist_stats()
        rots = ph.hoisting(e.ctx, up(ph, e.ctx, e.o, a), e.gk, list(STEPS))
        for st, r in zip(STEPS, rots):
            same(r.to_numpy(), e.o.rotate(a, e.okey[st], st), f"seal step {st}, zeros={zeros}")
        h1 = e.ctx.seal_hoist_stats()
        assert h1[path] == h0[path] + 1 and h1[1 - path] == h0[1 - path], (zeros, h0, h1)


def case_rescale(ph, N, envs):
    """Two and three components, the divided limb on its rounding boundaries (N = 32768: k_rescale_*_hs for two,
    the generic half form for three).  N = 16384 adds three components at l = 88 on [59]*89, P = 1: (l - 1) 3 = 261
    workgroups select k_rescale_ntt<14, true>."""
    shapes = [([59] * 5, 4)] + ([([59] * 89, 88)] if N == 16384 else [])
    for bits, l in shapes:
        ctx, _, o = make_ctx(ph, N, bits, 1)
        rng = np.random.default_rng(N + l)
        for ncomp in ((2, 3) if l == 4 else (3,)):
            a = rand_ct(o, rng, ncomp, l)
            for k in range(ncomp):
                a[k, l - 1] = o.ntt(ei.edge_limb(o.primes[l - 1], N, rng), l - 1)
            r = ph.rescale_to_next(ctx, up(ph, ctx, o, a))
            assert r.chain_index() == o.L0 + 2 - l
            same(r.to_numpy(), o.rescale(a), f"rescale l={l}, {ncomp} components")


def check_encode_exact(r, z, scale, pt, tag, period=1):
    """|z| ~ 1 at scale 2^40: every coefficient at least 2^-12 from a half-integer is the reference's rounding half
    away from zero, the others within 1 (test_embedding_reference.py (a)); a row of period N/2/t: exact zeros off
    the multiples of min(t, 8)."""
    pre, want = _want(z, r.N, scale)
    got = r.coeffs(pt)
    assert _representable(got), tag
    win = er.tie_window(pre)
    d = np.array([abs(a - b) for a, b in zip(got, want)], dtype=object)
    assert not any(d[~win]), tag
    assert max(d) <= 1, tag
    assert int(win.sum()) <= max(8, r.N // 64), (tag, int(win.sum()))
    if period > 1:
        assert not any(c for k, c in enumerate(got) if k % period), tag
        assert any(got[::period]), tag


def _rand(rng, n, cplx):
    return rng.normal(0, 1, n) + 1j * rng.normal(0, 1, n) if cplx else rng.normal(0, 1, n)


def encode_rows(N):
    """The encoder cases' rows: a full real row, a complex row one value short, and one real row tiled t times per
    sparse factor the ring has (t = 2, 4, 8 while N / t >= 256).  (tag, values, chain index, period)."""
    H = N // 2
    rng = np.random.default_rng(N + 6)
    rows = [("real", _rand(rng, H, False), 1, 1), ("complex", _rand(rng, H - 1, True), 2, 1)]
    rows += [(f"tiled {t}", np.tile(_rand(rng, H // t, False), t), 2, t) for t in (2, 4, 8) if N // t >= 256]
    return rows


def encode_and_check(r, scale=2.0 ** 40):
    """Encode encode_rows (the tiled rows as one batch), check every plaintext against the reference, return the
    limbs.  The tiled rows must come out with exact zeros off the multiples of their period."""
    rows = encode_rows(r.N)
    pts = [r.encode(z, scale, ci) for _, z, ci, t in rows if t == 1]
    tiled = [z for _, z, _, t in rows if t > 1]
    if tiled:
        pts += r.enc.encode_double_vector_batch(r.ctx, np.stack(tiled), scale, chain_index=2)
    for (tag, z, _, t), pt in zip(rows, pts):
        check_encode_exact(r, z, scale, pt, f"N={r.N} {tag}", period=t)
    return [pt.to_numpy() for pt in pts]


def case_encode(ph, N, ring):
    """k_encode and k_ntt_fwd_from_dbl on a real and a complex row; rows tiled 2, 4 and 8 times in one batch, one
    row per sparse factor the ring has (k_enc_period, k_ntt_fwd_from_dbl_sp<LOGN, 1..3> from N / 2^S >= 256); the
    precise encoder (k_reduce_i128 and the in-place k_ntt_fwd_ptrs).

    For these kernels "launched" is weaker than "did work": launch_ntt_fwd_sparse launches every
    k_ntt_fwd_from_dbl_sp<LOGN, S> whenever the period scratch exists, and each returns early on rows whose period is
    not 2^S (k_ntt_fwd_from_dbl likewise on periodic rows), so the full real row alone puts all of them into the
    ledger.  That each one wrote its row is shown by the values, not by the ledger: row "tiled t" equals the
    reference and has exact zeros off the multiples of t, which only k_ntt_fwd_from_dbl_sp<LOGN, log2 t> produces.
    The unfused encoder (k_encode reducing into every limb, then k_ntt_fwd_ptrs) is case_encode_unfused."""
    r = ring(N)
    H = N // 2
    rng = np.random.default_rng(N + 16)
    encode_and_check(r)
    zp = _rand(rng, H, True)
    pts = r.enc.encode_complex_vector_batch(r.ctx, zp[None], 2.0 ** 59, chain_index=1, precise=True)
    pre, want = _want(zp, N, 2.0 ** 59)
    assert _maxdiff(r.coeffs(pts[0]), want) <= 1 + int(np.max(np.abs(pre)) * LD(2.0 ** -56)), f"N={N} precise"


def case_client(ph, N, ring):
    """Key generation, symmetric and asymmetric encryption, the batched symmetric encryption (k_ntt_fwd_small) and
    the fused encode + encrypt (k_ntt_fwd_msg_err), decryption, and the decoder (k_decode_fft) from known integers."""
    r = ring(N)
    o, l = r.o, r.L0
    s = o.gen_secret(r.seed)
    sk = r.sk
    same(sk.export(), s, "secret key")
    rng = np.random.default_rng(N + 7)
    p = rand_pt(o, rng, l)
    pt = ph.plaintext_from_numpy(r.ctx, p, 1, SCALE)
    ct = sk.encrypt_symmetric(r.ctx, pt)
    a = o.encrypt_symmetric(r.seed, 0, s, p)
    same(ct.to_numpy(), a, "encrypt_symmetric")
    cta = sk.gen_publickey(r.ctx).encrypt_asymmetric(r.ctx, pt)
    same(cta.to_numpy(), o.encrypt_asymmetric(r.seed, 1 << 20, o.gen_public_key(r.seed, s), p), "encrypt_asymmetric")
    same(sk.decrypt(r.ctx, ct).to_numpy(), o.decrypt(s, a), "decrypt")
    p2 = [rand_pt(o, rng, l) for _ in range(2)]
    batch = sk.encrypt_symmetric_batch(r.ctx, [ph.plaintext_from_numpy(r.ctx, q, 1, SCALE) for q in p2])
    for k, c in enumerate(batch):
        same(c.to_numpy(), o.encrypt_symmetric(r.seed, 1 + k, s, p2[k]), f"encrypt_symmetric_batch {k}")
    rows = _rand(rng, 2 * (N // 2), False).reshape(2, N // 2)
    enc_pts = r.enc.encode_double_vector_batch(r.ctx, rows, 2.0 ** 40, chain_index=1)
    for k in range(2):
        check_encode_exact(r, rows[k], 2.0 ** 40, enc_pts[k], f"N={N} client row {k}")
    for k, c in enumerate(sk.encode_encrypt_batch(r.ctx, rows, 2.0 ** 40, 1)):
        same(c.to_numpy(), o.encrypt_symmetric(r.seed, 3 + k, s, enc_pts[k].to_numpy()), f"encode_encrypt_batch row {k}")
    _check_decode(r, _known_ints(N, N, 2 ** 45), 3, 2.0 ** 40, f"N={N} decode")


def case_encode_unfused(N, ring, tmp_path):
    """FHESPEAR_ENCODE_UNFUSED=1 is read once per process, so a child (tests/_launch_worker.py) encodes encode_rows
    with it set: k_encode reduces every rounded coefficient into every limb (the spread coefficients of a periodic
    row) and k_ntt_fwd_ptrs transforms in place.  The child checks its plaintexts against the reference itself; here
    its limbs must equal the fused encoder's.  Returns the child's ledger."""
    import json
    import os
    import subprocess
    import sys
    out = tmp_path / f"unfused_{N}.npz"
    env = dict(os.environ, FHESPEAR_ENCODE_UNFUSED="1")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_launch_worker.py")
    p = subprocess.run([sys.executable, worker, str(N), str(out)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    ledger = [json.loads(l[len("LEDGER "):]) for l in p.stdout.splitlines() if l.startswith("LEDGER ")]
    assert len(ledger) == 1, p.stdout[-1500:]
    fused = encode_and_check(ring(N))
    with np.load(out) as z:
        assert len(z.files) == len(fused)
        for k, ((tag, _, _, _), want) in enumerate(zip(encode_rows(N), fused)):
            same(z[f"pt{k}"], want, f"N={N} unfused {tag} against the fused limbs")
    logn = N.bit_length() - 1
    assert f"k_ntt_fwd_ptrs<{logn}>" in ledger[0] and not any(k.startswith("k_ntt_fwd_from_dbl") for k in ledger[0]), \
        f"the child did not take the unfused path: {ledger[0]}"
    return set(ledger[0])


RING_CASES = [case_keyswitch_selectors, case_keyswitch_batch, case_bsgs, case_giant_final_at_128_limbs,
              case_multiply_many_at_128_pairs, case_seal, case_rescale, case_encode, case_client]


def shared_contexts(ph, orc, N):
    """(envs, ring): one KsEnv per (chain, mode) and one encoder ring, made on first use and shared by the cases"""
    kenv, rings = {}, {}

    def envs(chain, mode="exact"):
        if (chain, mode) not in kenv:
            kenv[chain, mode] = KsEnv(ph, N, chain, mode)
        return kenv[chain, mode]

    def ring(n):
        if n not in rings:
            rings[n] = _Ring(ph, orc, n, [59] * 4, seed=SEED)
        return rings[n]
    return envs, ring


def run_ring(ph, orc, N, shared=None):
    """Every per-ring case at ring N."""
    envs, ring = shared or shared_contexts(ph, orc, N)
    for case in RING_CASES:
        case(ph, N, ring if case in (case_encode, case_client) else envs)


# ------------------------------------------------------------------ ring-independent kernels (N = 1024 unless noted)
def case_elementwise(ph, N, envs):
    """k_eltwise, k_tensor, k_scalar, k_mod_raise_lift on S59."""
    e = envs("S59")
    ctx, o, l = e.ctx, e.o, 4
    rng = np.random.default_rng(N + 8)
    a, b, p = rand_ct(o, rng, 2, l), rand_ct(o, rng, 2, l), rand_pt(o, rng, l)
    A, B_, P_ = up(ph, ctx, o, a), up(ph, ctx, o, b), ph.plaintext_from_numpy(ctx, p, 1, SCALE)
    same(ph.add(ctx, A, B_).to_numpy(), o.add(a, b), "add")
    same(ph.sub(ctx, A, B_).to_numpy(), o.sub(a, b), "sub")
    same(ph.negate(ctx, A).to_numpy(), o.negate(a), "negate")
    same(ph.multiply_plain(ctx, A, P_).to_numpy(), o.multiply_plain(a, p), "multiply_plain")
    same(ph.add_plain(ctx, A, P_).to_numpy(), o.add_plain(a, p), "add_plain")
    same(ph.multiply(ctx, A, B_).to_numpy(), o.multiply(a, b), "multiply")
    same(ph.multiply_const(ctx, A, 3.0).to_numpy(), o.scalar(a, 3, False), "multiply_const")
    same(ph.add_const(ctx, A, 2.0).to_numpy(), o.scalar(a, int(2.0 * SCALE), True), "add_const")
    m = rand_ct(o, rng, 2, 2)
    for k in range(2):
        m[k, 0] = o.ntt(ei.edge_limb(o.primes[0], N, rng), 0)
    same(ph.mod_raise(ctx, up(ph, ctx, o, m)).to_numpy(), o.mod_raise(m), "mod_raise")


def _inner_sums(o, baby_np, pn, G, B):
    out = []
    for g in range(B):
        acc = None
        for b in range(G):
            t = o.multiply_plain(baby_np[b], pn[g * G + b])
            acc = t if acc is None else o.add(acc, t)
        out.append(acc)
    return out


def case_inner_windows(ph, orc, bits, what):
    """bsgs_inner_products with G = 65 (a 64-step window, then one that adds to its sums: ACC) on dense diagonals:
    59-bit primes fold every 16 products, 60-bit ones every 8."""
    N, G, l = 1024, 65, 2
    ctx, _, o = make_ctx(ph, N, [bits] * 3, 1)
    rng = np.random.default_rng(bits)
    baby_np = [rand_ct(o, rng, 2, l) for _ in range(G)]
    pn = [rand_pt(o, rng, l) for _ in range(G)]
    inner = ph.bsgs_inner_products(ctx, [up(ph, ctx, o, a) for a in baby_np],
                                   [ph.plaintext_from_numpy(ctx, p, 1, SCALE) for p in pn], G, 1)
    same(inner[0].to_numpy(), _inner_sums(o, baby_np, pn, G, 1)[0], what)


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


def case_inner_compact(ph, orc, N):
    """D = 128 diagonals tiled N/256 times (encode_matrix_diagonals: k_diag_gather, stored compact only at
    tlog = log2(N / 256)), read by k_bsgs_inner<.., TL = tlog> in two windows (G = 65: plain and ACC); the inner
    product against the oracle's sums over the expanded limbs (k_expand_compact); the expanded limbs of diagonals from
    both giant groups (the second is rolled by G) are the encoding of the caller's rows."""
    D, G, l, scale = 128, 65, 3, 2.0 ** 40
    r = _Ring(ph, orc, N, [59] * 4, seed=SEED)
    rng = np.random.default_rng(N + 9)
    W = rng.normal(0, 1, (D, D))
    every = r.enc.encode_matrix_diagonals(r.ctx, W, G, scale, chain_index=1)
    pts = every[:G]
    baby_np = [rand_ct(r.o, rng, 2, l) for _ in range(G)]
    inner = ph.bsgs_inner_products(r.ctx, [up(ph, r.ctx, r.o, a) for a in baby_np], pts, G, 1)
    pn = [p.to_numpy() for p in pts]
    same(inner[0].to_numpy(), _inner_sums(r.o, baby_np, pn, G, 1)[0], f"compact inner product, N={N}")
    rows = _bg_rows(W, D, G, N // 2)
    for k in (0, G - 1, G, G + 7, D - 1):      # giant group 0 and the rolled group 1 (k >= G)
        check_encode_exact(r, rows[k], scale, every[k], f"N={N} diagonal {k}", period=N // 256)


def case_dot(ph, orc):
    """k_dot_tensor, all four: J = 3 and J = 65 (a second window: ACC) on the 60/40/40/60 chain (8 products per
    fold) and on 59-bit primes (16)."""
    from test_retrieval_dot import CHAINS as DOT_CHAINS, Env
    for chain in ("a", "b"):
        N, bits, P = DOT_CHAINS[chain]
        e = Env(ph, orc, N, bits, P)
        for J in (3, 65):
            rng = np.random.default_rng(J)
            q = [e.rand(rng, 2, 2) for _ in range(J)]
            e.check(q, [[e.rand(rng, 2, 2) for _ in range(J)]], what=f"chain {chain} J={J}")


def case_decode_batches(ph, orc):
    """decode_batch (k_crt_compose_jobs) and decrypt_decode_batch (k_decrypt_many) from known integers below 2^45 at
    l = 6, scale 2^40: three limbs are composed and checked against the other three, the batched shortcut."""
    N, l, scale = 1024, 6, 2.0 ** 40
    r = _Ring(ph, orc, N, [59] * 7, seed=SEED)
    o = r.o
    s = o.gen_secret(SEED)
    cs = [_known_ints(k, N, 2 ** 45) for k in (1, 2)]
    limbs = [np.stack([o.ntt(np.array([x % q for x in c], dtype=np.uint64), i) for i, q in enumerate(o.primes[:l])])
             for c in cs]
    pts = [ph.plaintext_from_numpy(r.ctx, a, 1, scale) for a in limbs]
    cts = [r.sk.encrypt_symmetric(r.ctx, p) for p in pts]
    for k, c in enumerate(cts):
        same(c.to_numpy(), o.encrypt_symmetric(SEED, k, s, limbs[k]), f"encrypt_symmetric {k}")
    dec = [o.decrypt(s, c.to_numpy()) for c in cts]
    for what, z, lm in (("decode_batch", r.enc.decode_batch(r.ctx, pts, nslots=64), limbs),
                        ("decrypt_decode_batch", r.sk.decrypt_decode_batch(r.ctx, cts, 64), dec)):
        for k in range(2):
            sr, si = er.slots_ref(er.coeffs_of(o, lm[k]), N, scale)
            zo = o.decode(lm[k], scale)
            err = lambda v: max(np.max(np.abs(v.real.astype(LD) - sr[:len(v)])), np.max(np.abs(v.imag.astype(LD) - si[:len(v)])))
            bound = 8 * err(zo) + LD(2.0 ** -52) * np.sqrt(np.mean(sr * sr + si * si))
            assert err(np.asarray(z[k])) <= bound, (what, k)


def run_independent(ph, orc):
    """The single-instance kernels ride on the per-ring cases at N = 1024 (key switch, BSGS, SEAL, client, encoder);
    the rest is added here."""
    N = 1024
    shared = shared_contexts(ph, orc, N)
    run_ring(ph, orc, N, shared)
    case_elementwise(ph, N, shared[0])
    case_inner_windows(ph, orc, 59, "G = 65 on 59-bit primes")
    case_inner_windows(ph, orc, 60, "G = 65 on 60-bit primes")
    for n in (512, 1024, 2048):
        case_inner_compact(ph, orc, n)
    case_dot(ph, orc)
    case_decode_batches(ph, orc)
