"""Edge-operand parity: the GPU kernels against the CPU oracle, limb for limb, on operands random data never
produces (tests/_edge_inputs.py; test_edge_operands_cpu.py pins these inputs and the oracle on them):
  (a) key-switch digits next to Q_S / 2 -- k_centered's exact fallback (centered_exact), k_centered_x's three
      thresholds, the y > q/2 branch of the one-limb conversions -- through every ModUp / ModDown launch shape;
  (b) rescale and (c) ModRaise with the rounded limb at 0, q >> 1 and q - 1 and their neighbours;
  (d) the key inner product and (e) the BSGS Hadamard and the tensor product on all-(q - 1) operands, at digit and
      baby-step counts on both sides of every accumulator fold, also against their closed forms;
  (f) the element-wise ops on constant and boundary operands.
Every comparison is np.array_equal on limbs."""
import numpy as np
import pytest

import _edge_inputs as ei
from test_gpu_parity import PARAMS, oracle_for, rand_ct, rand_pt

pytestmark = pytest.mark.gpu

SCALE = 2.0 ** 40
STEPS = (1, -1, 3)


@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


def _bits(bits, L0, P):
    return list(bits) if isinstance(bits, (list, tuple)) else [bits] * (L0 + P)


def make_ctx(ph, N, bits, P, steps=(), seed=None, mode="exact"):
    """Context (+ seeded secret key when `seed` is given) on create_coeff_modulus(N, bits); bits lists every prime."""
    primes = ph.create_coeff_modulus(N, list(bits))
    parms = ph.params(ph.scheme_type.ckks)
    parms.set_poly_modulus_degree(N)
    parms.set_special_modulus_size(P)
    if steps:
        parms.set_galois_elts(sorted(set(ph.get_elts_from_steps(list(steps), N))))
    parms.set_coeff_modulus(primes)
    ctx = ph.context(parms)
    if mode != "exact":
        ctx.set_key_switch_mode(mode)
    o = oracle_for([int(q) for q in primes], N, P)
    if mode != "exact":
        o.set_key_switch_mode(mode)
    sk = ph.secret_key(ctx, seed=seed) if seed is not None else None
    return ctx, sk, o


def same(got, want, what):
    """np.array_equal with the first differing (component, limb, slot) in the message."""
    got = np.asarray(got)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(int(v) for v in bad[0])
        pytest.fail(f"{what}: {len(bad)} words differ, first at (component, limb, slot) {i}: "
                    f"got {int(got[i])}, want {int(want[i])}")


def up(ph, ctx, o, limbs):
    return ph.ciphertext_from_numpy(ctx, limbs, o.L0 + 1 - limbs.shape[1], SCALE)


# ------------------------------------------------------------------ (a) near-half ModUp
# (N, L0, P, bits, levels)
NEAR_HALF = [
    (256, 6, 3, 59, (6, 5, 4, 2)),
    (1024, 6, 3, 59, (6, 3, 5, 4, 2)),
    (1024, 6, 3, 60, (6, 3, 5, 4, 2)),
    (1024, 6, 3, [60] * 6 + [59] * 3, (6, 3, 5)),   # 59-bit special primes under 60-bit data primes: the X-form
                                                    # ModDown without the all-59-bit folds (k_moddown_h<.., true>)
    (1024, 4, 2, 59, (4, 3, 2)),
    (1024, 4, 2, 60, (4, 3, 2)),
    (1024, 4, 1, 59, (4, 2)),
    (1024, 4, 1, [59] * 4 + [60], (4, 2)),
    (32768, 3, 3, 59, (3, 2)),
    (32768, 4, 2, 59, (4, 3)),
    (32768, 3, 1, 59, (3,)),
]


@pytest.mark.parametrize("N,L0,P,bits,levels", NEAR_HALF,
                         ids=[f"N{c[0]}-L{c[1]}-P{c[2]}-{'mixed' if isinstance(c[3], list) else c[3]}" for c in NEAR_HALF])
def test_near_half_digits_rotate_and_relinearize(ph, N, L0, P, bits, levels):
    """The switched component (c1 of the rotations, c2 of the relinearisation) has every digit coefficient next to
    Q_S / 2 (one-limb digits: at q >> 1 and its neighbours): three rotations queued before any readback (one
    hoisted ModUp) and one relinearisation per level, against the oracle with the same seeded keys."""
    seed = 77
    ctx, sk, o = make_ctx(ph, N, _bits(bits, L0, P), P, steps=STEPS, seed=seed)
    s = o.gen_secret(seed)
    gk = sk.create_galois_keys(ctx)
    rlk = sk.gen_relinkey(ctx)
    elts = [ph.get_elt_from_step(st, N) for st in STEPS]
    okeys = [o.gen_galois_key(seed, s, e) for e in elts]
    orlk = o.gen_relin_key(seed, s)
    rng = np.random.default_rng(N + 10 * L0 + P)
    for l in levels:
        a = np.stack([rand_pt(o, rng, l), ei.to_ntt(o, ei.near_half_digits(o.primes, P, l, N, rng))])
        A = up(ph, ctx, o, a)
        outs = [ph.rotate(ctx, A, st, gk) for st in STEPS]
        for st, e, k, out in zip(STEPS, elts, okeys, outs):
            same(out.to_numpy(), o.rotate_elt(a, k, e), f"rotate step {st} at l={l}")
        c3 = np.concatenate([rand_ct(o, rng, 2, l), ei.to_ntt(o, ei.near_half_digits(o.primes, P, l, N, rng))[None]])
        same(ph.relinearize(ctx, up(ph, ctx, o, c3), rlk).to_numpy(), o.relinearize(c3, orlk), f"relinearize at l={l}")


@pytest.mark.parametrize("l", [36, 35, 34])
def test_near_half_digits_in_a_batch_of_distinct_inputs(ph, l):
    """Eight distinct near-half inputs rotated in one queued batch on the 36 + 3 chain at N = 1024: 8 l >= 256
    workgroups, so the key switch's INTT runs in its half-limb form (k_ks_intt_h) on boundary data."""
    N, L0, P, seed, U = 1024, 36, 3, 79, 8
    ctx, sk, o = make_ctx(ph, N, [59] * (L0 + P), P, steps=STEPS, seed=seed)
    s = o.gen_secret(seed)
    gk = sk.create_galois_keys(ctx)
    okeys = {st: o.gen_galois_key(seed, s, ph.get_elt_from_step(st, N)) for st in STEPS}
    rng = np.random.default_rng(l)
    ins = [np.stack([rand_pt(o, rng, l), ei.to_ntt(o, ei.near_half_digits(o.primes, P, l, N, rng))]) for _ in range(U)]
    cts = [up(ph, ctx, o, a) for a in ins]
    outs = [ph.rotate(ctx, c, STEPS[i % 3], gk) for i, c in enumerate(cts)]
    for i, (a, out) in enumerate(zip(ins, outs)):
        st = STEPS[i % 3]
        same(out.to_numpy(), o.rotate_elt(a, okeys[st], ph.get_elt_from_step(st, N)), f"input {i}, step {st}, l={l}")


def test_seal_one_limb_edge_set_hoisted_and_fallback(ph):
    """SEAL convention (P = 1, [59]*4 + [60]) on the one-limb boundary set: without a zero coefficient the batch
    shares one decomposition (hoisted), with zeros present it takes SEAL's per-rotation path; both limb-identical
    to the oracle's SEAL rotation."""
    N, L0, seed = 1024, 4, 81
    ctx, sk, o = make_ctx(ph, N, [59] * L0 + [60], 1, steps=STEPS, seed=seed, mode="seal")
    assert ctx.key_switch_mode() == "seal"
    s = o.gen_secret(seed)
    gk = sk.create_galois_keys(ctx)
    okeys = {st: o.gen_galois_key(seed, s, ph.get_elt_from_step(st, N)) for st in STEPS}
    rng = np.random.default_rng(82)
    for l in (L0, 2):
        for zeros, path in ((False, 0), (True, 1)):
            c1 = ei.near_half_digits(o.primes, 1, l, N, rng, exclude_zero=not zeros)
            assert (c1 == 0).any() == zeros
            a = np.stack([rand_pt(o, rng, l), ei.to_ntt(o, c1)])
            h0 = ctx.seal_hoist_stats()
            rots = ph.hoisting(ctx, up(ph, ctx, o, a), gk, list(STEPS))
            for st, r in zip(STEPS, rots):
                same(r.to_numpy(), o.rotate(a, okeys[st], st), f"seal step {st}, l={l}, zeros={zeros}")
            h1 = ctx.seal_hoist_stats()
            assert h1[path] == h0[path] + 1 and h1[1 - path] == h0[1 - path], (zeros, h0, h1)


# ------------------------------------------------------------------ (b) rescale, (c) ModRaise
MIXED = [60, 40, 40, 60]
RESCALE = [(N, bits, None, (2, 3)) for N in (256, 1024) for bits in ([59] * 5, [60] * 5, MIXED)] + \
          [(16384, [59] * 4, (3,), (2, 3)), (32768, [59] * 4, (3,), (2, 3))]


@pytest.mark.parametrize("N,bits,levels,comps", RESCALE, ids=[f"N{c[0]}-{c[1][0]}x{len(c[1])}" for c in RESCALE])
def test_rescale_edge_limbs_match_oracle(ph, N, bits, levels, comps):
    """The divided limb of every component cycles through {0, 1, 2, h-1, h, h+1, h+2, q-2, q-1} (coefficient form),
    the other limbs random: rescale_to_next == Oracle.rescale.  N = 32768: two components take k_rescale_*_hs,
    three the generic form."""
    ctx, _, o = make_ctx(ph, N, bits, 1)
    rng = np.random.default_rng(N + len(bits))
    for l in levels or range(2, o.L0 + 1):
        for ncomp in comps:
            a = rand_ct(o, rng, ncomp, l)
            for k in range(ncomp):
                a[k, l - 1] = o.ntt(ei.edge_limb(o.primes[l - 1], N, rng), l - 1)
            r = ph.rescale_to_next(ctx, up(ph, ctx, o, a))
            assert r.chain_index() == o.L0 + 2 - l
            same(r.to_numpy(), o.rescale(a), f"rescale l={l}, {ncomp} components")


@pytest.mark.parametrize("bits", [[59] * 7, MIXED], ids=["59x7", "60-40-40-60"])
def test_mod_raise_edge_limbs_match_oracle(ph, bits):
    """Limb 0 cycles through the boundary set of q_0 (x <= half, and q_i - m with m = 0): mod_raise == Oracle.mod_raise
    from the top level and from l = 2."""
    N = 1024
    ctx, _, o = make_ctx(ph, N, bits, 1)
    rng = np.random.default_rng(len(bits))
    for l in (o.L0, 2):
        a = rand_ct(o, rng, 2, l)
        for k in range(2):
            a[k, 0] = o.ntt(ei.edge_limb(o.primes[0], N, rng), 0)
        same(ph.mod_raise(ctx, up(ph, ctx, o, a)).to_numpy(), o.mod_raise(a), f"mod_raise from l={l}")


# ------------------------------------------------------------------ (d) worst-case key inner product
KEY_IP = [
    ([59] * 39, 3, (36, 35, 25, 24, 2), "exact"),      # dnum 12, 12, 9, 8, 1: both sides of k_ks_ip's 8-digit fold
    ([60] * 39, 3, (36, 27, 24), "exact"),             # dnum 12, 9, 8 where 9 products of (q - 1)^2 exceed an Acc3
    ([59] * 18 + [60], 1, (18, 17, 9, 8), "exact"),
    (MIXED, 1, (3,), "exact"),
    ([59] * 18 + [60], 1, (18,), "seal"),              # no closed form (uncentred lift): the oracle alone judges
]


@pytest.mark.parametrize("bits,P,levels,mode", KEY_IP, ids=["36+3-59", "36+3-60", "18+1", "60-40-40-60", "18+1-seal"])
def test_worst_case_key_inner_product(ph, bits, P, levels, mode):
    """The switched component is all q - 1 (the constant -1: every extension slot p_t - 1) and the imported key has
    every word q_t - 1, so each accumulator slot is dnum products of (q - 1)^2: relinearize and rotate equal the
    oracle and (exact convention) the closed form c + v, v = -(S div P).  Then the same with the key at q_t - 1 on
    the even limbs only (max_key(o, 2)), judged by the oracle: a wrapped accumulator there cannot hide as one
    consistent small integer that the division by P drops."""
    N = 1024
    ctx, _, o = make_ctx(ph, N, bits, P, steps=(1,), mode=mode)
    elt = ph.get_elt_from_step(1, N)
    rng = np.random.default_rng(len(bits) + P)
    for every in (1, 2):
        key = ei.max_key(o, every)
        rlk = ph.relin_key_from_numpy(ctx, key)
        gk = ph.galois_keys_from_numpy(ctx, {elt: key})
        for l in levels:
            c3, got, c2, got_r = ei.check_worst_case_keyswitch(
                o, lambda c: ph.relinearize(ctx, up(ph, ctx, o, c), rlk).to_numpy(),
                lambda c: ph.rotate(ctx, up(ph, ctx, o, c), 1, gk).to_numpy(), elt, l, rng,
                closed_form=mode == "exact" and every == 1)
            same(got, o.relinearize(c3, key), f"relinearize vs oracle, l={l}, key on every {every} limb")
            same(got_r, o.rotate_elt(c2, key, elt), f"rotate vs oracle, l={l}, key on every {every} limb")


# ------------------------------------------------------------------ (e) worst-case Hadamard and tensor
HADAMARD_G = (7, 8, 9, 15, 16, 17, 24, 33, 64, 66)


@pytest.mark.parametrize("bits", [[59] * 7, [60] * 7, MIXED], ids=["59x7", "60x7", "60-40-40-60"])
def test_worst_case_hadamard_and_tensor(ph, bits):
    """bsgs_inner_products with every baby step and every diagonal all q - 1 (B = 2, D = 2G - 1, the missing
    diagonal zero): group 0 sums G products of (q - 1)^2, group 1 G - 1 -- on both sides of k_bsgs_inner's folds
    (every 16 products on 59-bit chains, every 8 on 60-bit ones) and into the second baby-step window (G = 66).
    Equal to the oracle's multiply_plain / add sums and to n mod q_i; multiply of two all-max ciphertexts equals
    the oracle and (1, 2, 1)."""
    N = 1024
    ctx, _, o = make_ctx(ph, N, bits, 1)
    for l in (o.L0, 2):
        ci = o.L0 + 1 - l
        worst = ei.all_max(o.primes, l, N, 2)
        wpt = ei.all_max(o.primes, l, N)
        term = o.multiply_plain(worst, wpt)
        sums, acc = {}, None
        for n in range(1, max(HADAMARD_G) + 1):
            acc = term if acc is None else o.add(acc, term)
            sums[n] = acc
            assert np.array_equal(acc, np.stack([ei.constant_limbs(o.primes, l, N, n)] * 2))
        baby = [up(ph, ctx, o, worst) for _ in range(max(HADAMARD_G))]
        P_ = ph.plaintext_from_numpy(ctx, wpt, ci, SCALE)
        zero = ph.plaintext_from_numpy(ctx, np.zeros((l, N), dtype=np.uint64), ci, SCALE)
        for G in HADAMARD_G:
            inner = ph.bsgs_inner_products(ctx, baby[:G], [P_] * (2 * G - 1) + [zero], G, 2)
            same(inner[0].to_numpy(), sums[G], f"G={G}, l={l}, group 0")
            same(inner[1].to_numpy(), sums[G - 1], f"G={G}, l={l}, group 1")
        m = ph.multiply(ctx, baby[0], baby[1]).to_numpy()
        same(m, o.multiply(worst, worst), f"multiply, l={l}")
        same(m, np.stack([ei.constant_limbs(o.primes, l, N, k) for k in (1, 2, 1)]), f"multiply closed form, l={l}")


@pytest.mark.parametrize("bits", [[59] * 7, [60] * 7], ids=["59x7", "60x7"])
def test_worst_case_bsgs_multiply_accumulate(ph, bits):
    """The whole fused BSGS (G = 17, B = 2, D = 33) on all-max baby steps and diagonals with the all-max Galois key
    for the giant step, against Oracle.bsgs_loop."""
    N, G, B, D = 1024, 17, 2, 33
    ctx, _, o = make_ctx(ph, N, bits, 1, steps=(G,))
    elt = ph.get_elt_from_step(G, N)
    key = ei.max_key(o)
    gk = ph.galois_keys_from_numpy(ctx, {elt: key})
    l = o.L0
    worst, wpt = ei.all_max(o.primes, l, N, 2), ei.all_max(o.primes, l, N)
    baby = [up(ph, ctx, o, worst) for _ in range(G)]
    pts = [ph.plaintext_from_numpy(ctx, wpt, 1, SCALE) for _ in range(D)]
    y = ph.bsgs_multiply_accumulate(ctx, baby, pts, G, B, D, gk)
    same(y.to_numpy(), o.bsgs_loop([worst] * G, [wpt] * D, [None, key], G, B, D), "bsgs_multiply_accumulate")


# ------------------------------------------------------------------ (f) element-wise edges
@pytest.mark.parametrize("N,L0,P", PARAMS)
def test_elementwise_edge_operands_match_oracle(ph, N, L0, P):
    """add, sub (both orders), negate, add_plain, sub_plain, multiply_plain on operand pairs drawn from
    {all 0, all 1, all q - 1, the boundary set around q >> 1}: sums that land on q exactly, differences that land
    on 0, and negate(0) = 0, not q."""
    ctx, _, o = make_ctx(ph, N, [59] * (L0 + P), P)
    rng = np.random.default_rng(N)
    l = L0
    const = lambda f: np.stack([np.full(N, f(q), dtype=np.uint64) for q in o.primes[:l]])
    kinds = {"0": lambda: const(lambda q: 0), "1": lambda: const(lambda q: 1), "q-1": lambda: const(lambda q: q - 1),
             "edge": lambda: np.stack([ei.edge_limb(q, N, rng) for q in o.primes[:l]])}
    for ka, fa in kinds.items():
        a = np.stack([fa(), fa()])
        A = up(ph, ctx, o, a)
        same(ph.negate(ctx, A).to_numpy(), o.negate(a), f"negate {ka}")
        if ka == "0":
            assert not ph.negate(ctx, A).to_numpy().any(), "negate(0) must be 0"
        for kb, fb in kinds.items():
            b = np.stack([fb(), fb()])
            p = b[1]
            Bc = up(ph, ctx, o, b)
            Pp = ph.plaintext_from_numpy(ctx, p, 1, SCALE)
            what = f"{ka} op {kb}"
            same(ph.add(ctx, A, Bc).to_numpy(), o.add(a, b), "add " + what)
            same(ph.sub(ctx, A, Bc).to_numpy(), o.sub(a, b), "sub " + what)
            same(ph.sub(ctx, A, Bc, True).to_numpy(), o.sub(b, a), "negated sub " + what)
            same(ph.add_plain(ctx, A, Pp).to_numpy(), o.add_plain(a, p), "add_plain " + what)
            want = a.copy()
            want[0] = o.sub(a[:1], p[None])[0]
            same(ph.sub_plain(ctx, A, Pp).to_numpy(), want, "sub_plain " + what)
            same(ph.sub_plain(ctx, A, Pp).to_numpy(), o.add_plain(a, o.negate(p[None])[0]), "sub_plain as add " + what)
            same(ph.multiply_plain(ctx, A, Pp).to_numpy(), o.multiply_plain(a, p), "multiply_plain " + what)
