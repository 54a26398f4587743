"""Fused batched CT x PT multiply and rescale (pyPhantom.multiply_plain_rescale_many / rescale_many /
ct_pt_dot_columns, fhs_multiply_plain_rescale_many): the head of the reference's ct_pt_dot
(fhe_rwkv_inference.py:67-70), rescale_to_next(multiply_plain(ct, pt)), for n pairs in one call -- per chunk the two
launches of one rescale (k_rescale_intt, k_rescale_ntt) that form the product in their loads and never store it.

The judge is the CPU oracle's own loop o.rescale(o.multiply_plain(a, p)) per pair, compared limb for limb, on random
residues uploaded with ciphertext_from_numpy / plaintext_from_numpy.  N = 256, 512 and 1024: chain "a"
(60, 40, 40, 60) with P = 1 at l = 3 and 2, chain "b" (59,) * 12 with P = 3 at l = 9, 6 and 2; every larger ring once,
with the half-limb instantiations at N = 16384 (a launch of 256 workgroups) and N = 32768.  The recorded reference run tests/golden/fri_trace.json (8 FFN columns) is
replayed through one call.  Every test here needs an MI355X: -m gpu."""
import ctypes as C
import gc
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest

import _edge_inputs as edge

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tools"))
SCALE = 2.0 ** 40
SEED = 6767
CHAINS = {"a": ((60, 40, 40, 60), 1), "b": ((59,) * 12, 3)}
# (N, chain, l): the top level and lower ones of every chain and ring
CONFIGS = [(N, ch, l) for N in (256, 512, 1024) for ch, levels in (("a", (3, 2)), ("b", (9, 6, 2))) for l in levels]
OK, INVALID, OOM, LEVEL = 0, 1, 2, 4
_SENTINEL = 0xDEAD0


@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


class Env:
    """GPU context and the oracle over the same primes; the keys (Galois keys for steps 1, 2, 4 and 8, the
    relinearization key, the oracle's copies) are made on first use."""

    def __init__(self, ph, orc, N, bits, P, steps=(1, 2, 4, 8)):
        primes = ph.create_coeff_modulus(N, list(bits))
        self.steps = list(steps)
        parms = ph.params(ph.scheme_type.ckks)
        parms.set_poly_modulus_degree(N)
        parms.set_special_modulus_size(P)
        parms.set_galois_elts(sorted(set(ph.get_elts_from_steps(self.steps, N))))
        parms.set_coeff_modulus(primes)
        self.ph, self.N, self.P = ph, N, P
        self.ctx = ph.context(parms)
        self.primes = [int(q) for q in primes]
        self.L0 = len(self.primes) - P
        self.o = orc.Oracle(N, self.primes, P)
        self._keys = {}

    def _key(self, name, make):
        if name not in self._keys:
            self._keys[name] = make()
        return self._keys[name]

    @property
    def sk(self):
        return self._key("sk", lambda: self.ph.secret_key(self.ctx, seed=SEED))

    @property
    def gk(self):
        return self._key("gk", lambda: self.sk.create_galois_keys(self.ctx))

    @property
    def rk(self):
        return self._key("rk", lambda: self.sk.gen_relinkey(self.ctx))

    @property
    def s(self):
        return self._key("s", lambda: self.o.gen_secret(SEED))

    @property
    def rlk(self):
        return self._key("rlk", lambda: self.o.gen_relin_key(SEED, self.s))

    def okey(self, step):
        return self._key(("g", step), lambda: self.o.gen_galois_key(SEED, self.s, self.ph.get_elt_from_step(step, self.N)))

    def rand(self, rng, l, ncomp=2):
        """Random residues: (ncomp, l, N), or (l, N) for a plaintext (ncomp=None)."""
        limbs = lambda: np.stack([rng.integers(0, self.primes[i], self.N, dtype=np.uint64) for i in range(l)])
        return limbs() if ncomp is None else np.stack([limbs() for _ in range(ncomp)])

    def up(self, a, scale=SCALE):
        return self.ph.ciphertext_from_numpy(self.ctx, a, self.L0 + 1 - a.shape[1], scale)

    def upp(self, p, scale=SCALE):
        return self.ph.plaintext_from_numpy(self.ctx, p, self.L0 + 1 - p.shape[0], scale)

    def want(self, a, p=None):
        """The reference's two calls on the oracle (p None: the rescale alone)."""
        return self.o.rescale(a if p is None else self.o.multiply_plain(a, p))

    def check(self, got, wants, l, what, scale=SCALE * SCALE):
        assert len(got) == len(wants), what
        for i, (g, w) in enumerate(zip(got, wants)):
            assert g.size() == 2 and g.chain_index() == self.L0 + 2 - l, f"{what} item {i}"
            assert g.scale() == scale / float(self.primes[l - 1]), f"{what} item {i}"
            assert np.array_equal(g.to_numpy(), w), f"{what} item {i}"


_ENVS = {}


@pytest.fixture(scope="module")
def env(ph, orc):
    def get(N, chain):
        key = (N, chain)
        if key not in _ENVS:
            bits, P = CHAINS[chain]
            _ENVS[key] = Env(ph, orc, N, bits, P)
        return _ENVS[key]
    yield get
    _ENVS.clear()


def _raw(e, a, p, n=None, ctx=True, ins=True, outs=True):
    """The C call itself: (status, the output array as Python ints), the array pre-filled with a sentinel."""
    ph = e.ph
    n = len(a) if n is None else n
    m = max(1, len(a))
    aa = (C.c_void_p * m)(*[c._h for c in a])
    pp = None if p is None else (C.c_void_p * max(1, len(p)))(*[x._h for x in p])
    out = (C.c_void_p * m)(*([_SENTINEL] * m))
    rc = ph._lib.fhs_multiply_plain_rescale_many(e.ctx._h if ctx else None, aa if ins else None, pp, n,
                                                 out if outs else None)
    return rc, [int(v or 0) for v in out]


@pytest.mark.parametrize("N,chain,l", CONFIGS)
def test_pairs_match_oracle_loop(env, N, chain, l):
    """n = 1, 2, 5 and 9 in one call as pairs of distinct handles and as rescale_many; one ciphertext against 9
    plaintexts, given as a repeated handle and as the binding's single-ciphertext form; one plaintext against 9
    ciphertexts.  Inputs are never written."""
    e = env(N, chain)
    ph = e.ph
    rng = np.random.default_rng(N + 10 * l)
    xs, ps = [e.rand(rng, l) for _ in range(9)], [e.rand(rng, l, None) for _ in range(9)]
    A, Pt = [e.up(x) for x in xs], [e.upp(p) for p in ps]
    pair = [e.want(x, p) for x, p in zip(xs, ps)]
    alone = [e.want(x) for x in xs]
    what = f"N={N} chain {chain} l={l}"
    for n in (1, 2, 5, 9):
        e.check(ph.multiply_plain_rescale_many(e.ctx, A[:n], Pt[:n]), pair[:n], l, f"{what} n={n} pairs")
        e.check(ph.rescale_many(e.ctx, A[:n]), alone[:n], l, f"{what} n={n} rescale_many", SCALE)
    one_ct = [e.want(xs[0], p) for p in ps]
    e.check(ph.multiply_plain_rescale_many(e.ctx, [A[0]] * 9, Pt), one_ct, l, f"{what} one ciphertext, repeated handle")
    e.check(ph.multiply_plain_rescale_many(e.ctx, A[0], Pt), one_ct, l, f"{what} one ciphertext, single form")
    e.check(ph.multiply_plain_rescale_many(e.ctx, A, [Pt[3]] * 9), [e.want(x, ps[3]) for x in xs], l, f"{what} one plaintext")
    for c, x in zip(A, xs):
        assert np.array_equal(c.to_numpy(), x), f"{what}: a ciphertext was written"
    for c, p in zip(Pt, ps):
        assert np.array_equal(c.to_numpy(), p), f"{what}: a plaintext was written"


@pytest.mark.parametrize("N", [2048, 4096, 8192, 16384, 32768])
def test_every_ring_once(ph, orc, N):
    """Chain "a", l = 2, n = 3 at every larger ring; at N = 32768 also n = 1, where the batched call (the general
    kernel pair) must equal the single calls, which take the two-workgroup _hs kernels there."""
    bits, P = CHAINS["a"]
    e = Env(ph, orc, N, bits, P, steps=[1])
    l = 2
    rng = np.random.default_rng(N)
    xs, ps = [e.rand(rng, l) for _ in range(3)], [e.rand(rng, l, None) for _ in range(3)]
    A, Pt = [e.up(x) for x in xs], [e.upp(p) for p in ps]
    wants = [e.want(x, p) for x, p in zip(xs, ps)]
    e.check(ph.multiply_plain_rescale_many(e.ctx, A, Pt), wants, l, f"N={N} n=3")
    e.check(ph.rescale_many(e.ctx, A), [e.want(x) for x in xs], l, f"N={N} n=3 rescale_many", SCALE)
    if N == 16384:   # 128 pairs: 256 and 256 workgroups, the half-limb instantiations of this ring
        ia, ip = [k % 3 for k in range(128)], [(k // 3) % 3 for k in range(128)]
        ph.debug_launch_ledger("arm")
        try:
            got = ph.multiply_plain_rescale_many(e.ctx, [A[i] for i in ia], [Pt[j] for j in ip])
            names = set(ph.debug_launch_ledger("read"))
        finally:
            ph.debug_launch_ledger("disarm")
        assert names == {"k_rescale_intt<14, true>", "k_rescale_ntt<14, true>"}, names
        want = {(i, j): e.want(xs[i], ps[j]) for i in range(3) for j in range(3)}
        e.check(got, [want[i, j] for i, j in zip(ia, ip)], l, "N=16384 n=128")
    if N == 32768:
        ph.debug_launch_ledger("arm")
        try:
            got = ph.multiply_plain_rescale_many(e.ctx, A[:1], Pt[:1])
            many = set(ph.debug_launch_ledger("read"))
            ph.debug_launch_ledger("arm")
            single = ph.rescale_to_next(e.ctx, ph.multiply_plain(e.ctx, A[0], Pt[0]))
            singles = set(ph.debug_launch_ledger("read"))
        finally:
            ph.debug_launch_ledger("disarm")
        e.check(got, wants[:1], l, "N=32768 n=1")
        assert np.array_equal(single.to_numpy(), wants[0]) and single.scale() == got[0].scale()
        assert many == {"k_rescale_intt<15, true>", "k_rescale_ntt<15, true>"}, many
        assert {"k_rescale_intt_hs<15>", "k_rescale_ntt_hs<15>"} <= singles, singles


def _boundary_ct(e, l, p, rng):
    """A ciphertext whose product with the plaintext p has, in its last limb, the coefficients of
    _edge_inputs.edge_limb: the nine values around 0, q_last >> 1 and q_last, so that after the INTT the rounding
    term + floor(q_last / 2) wraps between q_last >> 1 and (q_last >> 1) + 1.  The last limb is NTT(edge) / p."""
    q = e.primes[l - 1]
    x = e.rand(rng, l)
    for comp in range(2):
        t = e.o.ntt(edge.edge_limb(q, e.N, rng), l - 1)
        x[comp, l - 1] = np.array([int(tv) * pow(int(pv), -1, q) % q for tv, pv in zip(t, p[l - 1])], dtype=np.uint64)
    return x


@pytest.mark.parametrize("N", [256, 1024])
@pytest.mark.parametrize("chain,l", [("a", 3), ("b", 9)])
def test_worst_case_operands(env, N, chain, l):
    """Every residue q_i - 1 in ciphertext and plaintext (every product is (q - 1)^2), and a ciphertext whose
    last-limb product lands on the rounding boundary after the INTT (checked on the CPU first)."""
    e = env(N, chain)
    ph = e.ph
    rng = np.random.default_rng(N + l + 1)
    wc, wp = edge.all_max(e.primes, l, N, 2), edge.all_max(e.primes, l, N)
    p = e.rand(rng, l, None)
    p[l - 1][p[l - 1] == 0] = 1                      # invertible in the last limb
    b = _boundary_ct(e, l, p, rng)
    q = e.primes[l - 1]
    coef = e.o.intt(e.o.multiply_plain(b, p)[0, l - 1], l - 1)
    assert {q >> 1, (q >> 1) + 1, 0, q - 1} <= set(int(v) for v in coef), "the crafted product misses the boundary"
    WC, WP, Pp, B = e.up(wc), e.upp(wp), e.upp(p), e.up(b)
    what = f"worst N={N} chain {chain} l={l}"
    got = ph.multiply_plain_rescale_many(e.ctx, [WC, B, WC, B], [WP, Pp, Pp, WP])
    e.check(got, [e.want(wc, wp), e.want(b, p), e.want(wc, p), e.want(b, wp)], l, what)
    e.check(ph.multiply_plain_rescale_many(e.ctx, [B], [Pp]), [e.want(b, p)], l, what + " boundary alone")
    e.check(ph.rescale_many(e.ctx, [WC, B]), [e.want(wc), e.want(b)], l, what + " rescale_many", SCALE)
    assert np.array_equal(WC.to_numpy(), wc) and np.array_equal(B.to_numpy(), b) and np.array_equal(WP.to_numpy(), wp)


def test_scales_differ_per_pair(env):
    """Three pairs with different ciphertext and plaintext scales: each output's scale and chain index are those of
    the two single calls, bit for bit; rescale_many keeps the ciphertext's scale over the prime."""
    e = env(512, "a")
    ph = e.ph
    rng = np.random.default_rng(63)
    xs, ps = [e.rand(rng, 3) for _ in range(3)], [e.rand(rng, 3, None) for _ in range(3)]
    sa, sp = [2.0 ** 40, 2.0 ** 33, 3.0 * 2.0 ** 20], [2.0 ** 38, 5.0 * 2.0 ** 30, 2.0 ** 40 / 3.0]
    A, Pt = [e.up(x, s) for x, s in zip(xs, sa)], [e.upp(p, s) for p, s in zip(ps, sp)]
    got = ph.multiply_plain_rescale_many(e.ctx, A, Pt)
    for g, a, p, x, y in zip(got, A, Pt, xs, ps):
        one = ph.rescale_to_next(e.ctx, ph.multiply_plain(e.ctx, a, p))
        assert g.scale() == one.scale() and g.chain_index() == one.chain_index()
        assert np.array_equal(g.to_numpy(), e.want(x, y)) and np.array_equal(one.to_numpy(), e.want(x, y))
    for g, a in zip(ph.rescale_many(e.ctx, A), A):
        one = ph.rescale_to_next(e.ctx, a)
        assert g.scale() == one.scale() and g.chain_index() == one.chain_index()


def test_compact_plaintexts_get_their_dense_limbs(ph, orc):
    """The 64 diagonals of encode_matrix_diagonals at N = 1024 are compact-only until first dense use: as p of the
    batched call (their first dense use) they give the limbs of the single calls on a second, identical encoding, and
    the fused BSGS, which reads the compact shadow, gives the same limbs before and after."""
    bits, P = CHAINS["b"]
    D, G = 64, 8
    e = Env(ph, orc, 1024, bits, P, steps=list(range(1, G)) + [g * G for g in range(1, D // G)])
    rng = np.random.default_rng(36)
    enc = ph.ckks_encoder(e.ctx)
    W = rng.normal(0, 0.02, (D, D))
    x = e.rand(rng, 9)
    ct = e.up(x)
    baby = [ct] + [ph.rotate(e.ctx, ct, b, e.gk) for b in range(1, G)]
    pts = enc.encode_matrix_diagonals(e.ctx, W, G, SCALE, chain_index=1)
    before = ph.bsgs_multiply_accumulate(e.ctx, baby, pts, G, D // G, D, e.gk).to_numpy()
    got = ph.multiply_plain_rescale_many(e.ctx, ct, pts)
    again = enc.encode_matrix_diagonals(e.ctx, W, G, SCALE, chain_index=1)
    for k, (g, p2) in enumerate(zip(got, again)):
        one = ph.rescale_to_next(e.ctx, ph.multiply_plain(e.ctx, ct, p2))
        assert np.array_equal(g.to_numpy(), one.to_numpy()), f"diagonal {k}"
        assert g.scale() == one.scale() and g.chain_index() == one.chain_index() == 2
    e.check(got[:3], [e.want(x, p.to_numpy()) for p in pts[:3]], 9, "compact diagonals against the oracle")
    after = ph.bsgs_multiply_accumulate(e.ctx, baby, pts, G, D // G, D, e.gk).to_numpy()
    assert np.array_equal(before, after)


def test_more_pairs_than_one_chunk(env):
    """n = 513 distinct pairs at N = 256, l = 2: two chunks (257 + 256), each within the 512-item bound; every result
    is checked, as pairs and as rescale_many."""
    e = env(256, "a")
    rng = np.random.default_rng(513)
    xs, ps = [e.rand(rng, 2) for _ in range(513)], [e.rand(rng, 2, None) for _ in range(513)]
    A = [e.up(x) for x in xs]
    got = e.ph.multiply_plain_rescale_many(e.ctx, A, [e.upp(p) for p in ps])
    e.check(got, [e.want(x, p) for x, p in zip(xs, ps)], 2, "n=513")
    e.check(e.ph.rescale_many(e.ctx, A), [e.want(x) for x in xs], 2, "n=513 rescale_many", SCALE)


def test_launch_count(env):
    """With the ledger armed one call with n = 9 records only the ring's k_rescale_intt and k_rescale_ntt, no
    k_eltwise; with the kernel timer armed on the rescale id, `launches` grows by one per chunk (1 for n = 9, 2 for
    n = 513)."""
    e = env(512, "a")
    ph = e.ph
    rng = np.random.default_rng(99)
    l = 3
    xs, ps = [e.rand(rng, l) for _ in range(9)], [e.rand(rng, l, None) for _ in range(9)]
    A, Pt = [e.up(x) for x in xs], [e.upp(p) for p in ps]
    e.ctx.synchronize()
    ph.debug_launch_ledger("arm")
    try:
        got = ph.multiply_plain_rescale_many(e.ctx, A, Pt)
        e.ctx.synchronize()
        names = ph.debug_launch_ledger("read")
    finally:
        ph.debug_launch_ledger("disarm")
    assert len(names) == 2 and names[0].startswith("k_rescale_intt<9, ") and names[1].startswith("k_rescale_ntt<9, "), names
    assert not any("k_eltwise" in n for n in names)
    e.check(got, [e.want(x, p) for x, p in zip(xs, ps)], l, "ledger armed")
    ph.kernel_timer_arm(e.ctx, ["rescale"])
    try:
        ph.kernel_timer_read(e.ctx, reset=True)
        one = ph.multiply_plain_rescale_many(e.ctx, A, Pt)
        assert ph.kernel_timer_read(e.ctx)["rescale"][1] == 1
        two = ph.multiply_plain_rescale_many(e.ctx, [A[k % 9] for k in range(513)], [Pt[k % 7] for k in range(513)])
        assert ph.kernel_timer_read(e.ctx)["rescale"][1] == 3
        alone = ph.rescale_many(e.ctx, A)
        assert ph.kernel_timer_read(e.ctx, reset=True)["rescale"][1] == 4
    finally:
        ph.kernel_timer_arm(e.ctx, [])
    e.check(one, [e.want(x, p) for x, p in zip(xs, ps)], l, "timer armed")
    e.check(alone, [e.want(x) for x in xs], l, "timer armed, rescale_many", SCALE)
    want = {(i, j): e.want(xs[i], ps[j]) for i in range(9) for j in range(7)}
    e.check(two, [want[k % 9, k % 7] for k in range(513)], l, "timer armed, two chunks")


# ---------------------------------------------------------------------------------------------- reference fixture
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def _fri_head(ph, orc):
    """tests/golden/fri_trace.json case inference_n4096 up to its first multiply: (ctx, gk, the encrypted input, the
    8 column plaintexts, the recorded objects after the multiply_plain / rescale_to_next pairs, the recorded final
    objects of the 8 rotate / add chains)."""
    import fri_replay
    case = json.loads((REPO / "tests" / "golden" / "fri_trace.json").read_text())["cases"]["inference_n4096"]
    ctx, sk, pk, rlk, gk = fri_replay.make_context(ph, case)
    primes = [int(q) for q in ph.create_coeff_modulus(case["N"], case["bit_sizes"])]
    o = orc.Oracle(case["N"], primes, 1)
    objs, prod_of, root, final = {}, {}, {}, {}
    pts, cts, heads = [], [], []
    for op, out, ins, extra in case["ops"]:
        if op == "multiply":
            break
        if op == "encode":
            v = np.concatenate([np.asarray(extra["prefix"], dtype=np.float64), np.zeros(extra["n"] - len(extra["prefix"]))])
            limbs = o.encode(v, extra["scale"], o.L0 + 1 - extra["chain_index"])
            objs[out] = ph.plaintext_from_numpy(ctx, limbs, extra["chain_index"], extra["scale"])
        elif op == "encrypt_asymmetric":
            objs[out] = pk.encrypt_asymmetric(ctx, objs[ins[0]])
        elif op == "multiply_plain":
            prod_of[out] = (ins[0], ins[1])
        elif op == "rescale_to_next":
            c, p = prod_of[ins[0]]
            cts.append(objs[c])
            pts.append(objs[p])
            heads.append(out)
            root[out] = out
        elif op == "rotate":
            root[out] = root[ins[0]]
        elif op == "add":
            root[out] = root[ins[0]]
            final[root[out]] = out
        else:
            raise AssertionError(f"unexpected op {op} before the first multiply")
    assert len(heads) == 8 and all(c is cts[0] for c in cts)
    return ctx, gk, cts[0], pts, [case["objects"][h] for h in heads], [case["objects"][final[h]] for h in heads]


def test_reference_run_heads_as_one_call(ph, orc):
    """The 8 multiply_plain / rescale_to_next pairs of the recorded reference run through ONE
    multiply_plain_rescale_many: the recorded SHA-256, chain index and scale; the 8 final ct_pt_dot objects through ONE
    ct_pt_dot_many."""
    ctx, gk, ct, pts, heads, finals = _fri_head(ph, orc)
    for got, want in ((ph.multiply_plain_rescale_many(ctx, ct, pts), heads), (ph.ct_pt_dot_many(ctx, ct, pts, 8, gk), finals)):
        assert len(got) == 8
        for g, w in zip(got, want):
            assert g.chain_index() == w["ci"] and abs(g.scale() - w["scale"]) <= 1e-9 * abs(w["scale"])
            assert g.size() == 2 and _sha(g.to_numpy()) == w["sha"]


def test_ct_pt_dot_columns(env):
    """N = 512, W of shape (8, 5): the limbs of the reference's sequence of single calls on this library (encode the
    padded column, multiply_plain, rescale_to_next, the rotate / add loop), and slot 0 decrypts to x @ W.

    The bound on the decrypted error is worked out, not measured: at scale 2^40 a slot of the encrypted x is off by
    at most N (21 + 1/2) / 2^40 = 1.0e-8 (every coefficient of the fresh noise is at most 21, of the encoder's
    rounding 1/2, and a slot is a sum of N coefficients of modulus 1), a slot of an encoded column by N / 2^41; the
    rescale adds r0 + r1 s with |r| <= 1/2 per coefficient and a ternary s, at most N (1 + N) / 2 per slot, 1.2e-7 at
    the new scale (>= 2^39.9), and each of the three key switches at most as much again.  With |x|, |w| <= 1 slot 0,
    a sum of 8 such slots, is within 8 (1.1e-8 + 1.2e-7) + 7 * 1.2e-7 < 2e-6 of x @ W."""
    e = env(512, "a")
    ph, dim, F = e.ph, 8, 5
    rng = np.random.default_rng(85)
    x, W = rng.uniform(-1, 1, dim), rng.uniform(-1, 1, (dim, F))
    enc = ph.ckks_encoder(e.ctx)
    slots = enc.slot_count()
    ct = e.sk.encrypt_symmetric(e.ctx, enc.encode_double_vector(e.ctx, list(x) + [0.0] * (slots - dim), SCALE))
    got = ph.ct_pt_dot_columns(e.ctx, ct, W, dim, SCALE, e.gk)
    assert len(got) == F
    for f, g in enumerate(got):
        w_pt = enc.encode_double_vector(e.ctx, list(W[:, f]) + [0.0] * (slots - dim), SCALE)
        prod = ph.rescale_to_next(e.ctx, ph.multiply_plain(e.ctx, ct, w_pt))
        step = 1
        while step < dim:
            prod = ph.add(e.ctx, prod, ph.rotate(e.ctx, prod, step, e.gk))
            step *= 2
        assert g.chain_index() == prod.chain_index() == 2 and g.scale() == prod.scale(), f
        assert np.array_equal(g.to_numpy(), prod.to_numpy()), f
        slot0 = enc.decode_double_vector(e.ctx, e.sk.decrypt(e.ctx, g))[0]
        assert abs(slot0 - float(x @ W[:, f])) < 2e-6, (f, slot0, float(x @ W[:, f]))
    with pytest.raises(ValueError, match=r"\(dim, F\) array"):
        ph.ct_pt_dot_columns(e.ctx, ct, W[:4], dim, SCALE, e.gk)


def test_ct_pt_dot_many_and_dot_product_plain_many_keep_their_limbs(env):
    """ct_pt_dot_many (now one batched head and one inner_sum_many) against the oracle's per-column loop, and
    dot_product_plain_many(rescale=True) (now one rescale_many) against the oracle's sums."""
    e = env(1024, "b")
    ph, o, l = e.ph, e.o, 6
    rng = np.random.default_rng(86)
    x, ps = e.rand(rng, l), [e.rand(rng, l, None) for _ in range(5)]
    got = ph.ct_pt_dot_many(e.ctx, e.up(x), [e.upp(p) for p in ps], 4, e.gk)
    for g, p in zip(got, ps):
        w = e.want(x, p)
        for step in (1, 2):
            w = o.add(w, o.rotate(w, e.okey(step), step))
        assert np.array_equal(g.to_numpy(), w) and g.chain_index() == e.L0 + 2 - l
    q = [e.rand(rng, l) for _ in range(2)]
    rows = [[e.rand(rng, l, None) for _ in range(2)] for _ in range(3)]
    got = ph.dot_product_plain_many(e.ctx, [e.up(a) for a in q], [[e.upp(p) for p in row] for row in rows])
    for g, row in zip(got, rows):
        w = o.rescale(o.add(o.multiply_plain(q[0], row[0]), o.multiply_plain(q[1], row[1])))
        assert np.array_equal(g.to_numpy(), w) and g.chain_index() == e.L0 + 2 - l


# ---------------------------------------------------------------------------------------------- ordering, lifetime
def test_queued_rotations_as_inputs(env):
    """Inputs that are still-queued outputs of rotate: the entry flushes first."""
    e = env(512, "b")
    ph = e.ph
    rng = np.random.default_rng(71)
    a, b, p = e.rand(rng, 6), e.rand(rng, 6), e.rand(rng, 6, None)
    ca, cb, cp = e.up(a), e.up(b), e.upp(p)
    ra, rb = e.o.rotate(a, e.okey(1), 1), e.o.rotate(b, e.okey(2), 2)
    got = ph.multiply_plain_rescale_many(e.ctx, [ph.rotate(e.ctx, ca, 1, e.gk), cb, ph.rotate(e.ctx, cb, 2, e.gk)], [cp] * 3)
    e.check(got, [e.want(ra, p), e.want(b, p), e.want(rb, p)], 6, "queued inputs")
    got = ph.rescale_many(e.ctx, [ph.rotate(e.ctx, ca, 1, e.gk), ph.rotate(e.ctx, cb, 2, e.gk)])
    e.check(got, [e.want(ra), e.want(rb)], 6, "queued inputs, rescale_many", SCALE)


def test_inputs_may_die_at_once_and_memory_returns(env):
    """Destroying the inputs right after the call is safe (their blocks are reused before the results are read), and
    memory_in_use is back at its earlier value once all results are gone -- not before the last one goes."""
    e = env(1024, "b")
    ph = e.ph
    rng = np.random.default_rng(72)
    xs, ps = [e.rand(rng, 6) for _ in range(5)], [e.rand(rng, 6, None) for _ in range(5)]
    wants = [e.want(x, p) for x, p in zip(xs, ps)]
    warm = ph.multiply_plain_rescale_many(e.ctx, [e.up(x) for x in xs], [e.upp(p) for p in ps])   # warms the scratch slot
    del warm
    gc.collect()
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    A, Pt = [e.up(x) for x in xs], [e.upp(p) for p in ps]
    got = ph.multiply_plain_rescale_many(e.ctx, A, Pt)
    del A[:], Pt[:]
    gc.collect()
    filler = [e.up(x) for x in xs] + [e.upp(p) for p in ps]   # takes the inputs' blocks back from the cache, overwrites them
    e.ctx.synchronize()
    assert all(np.array_equal(got[i].to_numpy(), wants[i]) for i in range(5))   # (no loop variable keeps a result)
    keep = got.pop()                                 # one result keeps the shared block
    del got[:]
    gc.collect()
    assert e.ctx.memory_in_use() >= before + sum(f.to_numpy().nbytes for f in filler) + 5 * wants[0].nbytes
    assert np.array_equal(keep.to_numpy(), wants[-1])
    del keep, filler
    gc.collect()
    e.ctx.synchronize()
    assert e.ctx.memory_in_use() == before


# ---------------------------------------------------------------------------------------------- error contract
def test_argument_errors(env):
    e = env(256, "a")
    ph = e.ph
    rng = np.random.default_rng(80)
    a, b = e.up(e.rand(rng, 3)), e.up(e.rand(rng, 3))
    p, plow = e.upp(e.rand(rng, 3, None)), e.upp(e.rand(rng, 2, None))
    low = e.up(e.rand(rng, 2))
    three = ph.multiply(e.ctx, a, b)
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    untouched = [_SENTINEL, _SENTINEL]
    assert _raw(e, [a, b], [p, p], ctx=False)[0] == INVALID
    assert "null context" in ph._lib.fhs_last_error().decode()
    assert _raw(e, [a, b], [p, p], ins=False) == (INVALID, untouched)
    assert "null argument" in ph._lib.fhs_last_error().decode()
    assert _raw(e, [a, b], [p, p], outs=False)[0] == INVALID
    assert "null argument" in ph._lib.fhs_last_error().decode()
    assert _raw(e, [a, b], [p, p], n=0) == (INVALID, untouched)
    assert "n >= 1" in ph._lib.fhs_last_error().decode()
    assert _raw(e, [a, b], None, n=-1) == (INVALID, untouched)
    for aa, pp in (([a, three], None), ([three, b], [p, p])):
        assert _raw(e, aa, pp) == (INVALID, untouched)
        assert "2-component" in ph._lib.fhs_last_error().decode()
    for aa, pp in (([a, low], None), ([low, a], [p, p])):
        assert _raw(e, aa, pp) == (LEVEL, untouched)
        assert "share one chain index" in ph._lib.fhs_last_error().decode()
    for aa, pp in (([a, b], [p, plow]), ([low, low], [p, p])):
        assert _raw(e, aa, pp) == (LEVEL, untouched)
        assert "different chain indices" in ph._lib.fhs_last_error().decode()
    with pytest.raises(ValueError, match="n >= 1"):
        ph.multiply_plain_rescale_many(e.ctx, [], [])
    with pytest.raises(ValueError, match="n >= 1"):
        ph.rescale_many(e.ctx, [])
    with pytest.raises(ValueError, match="different length"):
        ph.multiply_plain_rescale_many(e.ctx, [a, b], [p])
    with pytest.raises(ValueError, match="chain ind"):
        ph.multiply_plain_rescale_many(e.ctx, a, [p, plow])
    with pytest.raises(ValueError, match="2-component"):
        ph.rescale_many(e.ctx, [a, three])
    e.ctx.synchronize()
    assert e.ctx.memory_in_use() == before


def test_last_level(env):
    """l = 1: FHS_ERR_LEVEL with and without plaintexts, nothing allocated, the output array untouched."""
    e = env(256, "a")
    ph = e.ph
    rng = np.random.default_rng(62)
    A = [e.up(e.rand(rng, 1)) for _ in range(2)]
    Pt = [e.upp(e.rand(rng, 1, None)) for _ in range(2)]
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    for pp in (Pt, None):
        assert _raw(e, A, pp) == (LEVEL, [_SENTINEL] * 2)
        assert "rescale_to_next: no level left" in ph._lib.fhs_last_error().decode()
    with pytest.raises(ValueError, match="no level left"):
        ph.multiply_plain_rescale_many(e.ctx, A, Pt)
    assert e.ctx.memory_in_use() == before


def test_lost_input_is_rejected(env):
    e = env(256, "a")
    ph = e.ph
    rng = np.random.default_rng(81)
    x, p = e.rand(rng, 3), e.rand(rng, 3, None)
    a, cp = e.up(x), e.upp(p)
    ph.debug_fail_next_flushes(e.ctx, 1)
    r = ph.rotate(e.ctx, a, 1, e.gk)
    with pytest.raises(RuntimeError, match="out of memory"):
        ph.multiply_plain_rescale_many(e.ctx, [r], [cp])         # the entry's flush fails: r is lost
    with pytest.raises(ValueError, match="ciphertext lost"):
        ph.multiply_plain_rescale_many(e.ctx, [a, r], [cp, cp])
    with pytest.raises(ValueError, match="ciphertext lost"):
        ph.rescale_many(e.ctx, [r])
    e.check(ph.multiply_plain_rescale_many(e.ctx, [a], [cp]), [e.want(x, p)], 3, "after a lost input")


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("plain", [True, False])
def test_every_allocation_failing_once(env, n, plain):
    """fhs_debug_fail_alloc at each allocation a warm call makes: each is "out of memory", leaves nothing allocated
    and the output array untouched, and the next call gives the same limbs."""
    e = env(512, "a")
    ph = e.ph
    rng = np.random.default_rng(82)
    xs, ps = [e.rand(rng, 3) for _ in range(n)], [e.rand(rng, 3, None) for _ in range(n)]
    A, Pt = [e.up(x) for x in xs], ([e.upp(p) for p in ps] if plain else None)
    want = [e.want(x, p if plain else None) for x, p in zip(xs, ps)]
    warm = ph.multiply_plain_rescale_many(e.ctx, A, Pt)
    assert all(np.array_equal(g.to_numpy(), w) for g, w in zip(warm, want))
    del warm
    gc.collect()
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    for k in range(16):
        ph.debug_fail_alloc(e.ctx, k)
        rc, outs = _raw(e, A, Pt)
        pending = ph.debug_fail_alloc(e.ctx, -1)
        if rc != OK:
            assert rc == OOM and "out of memory" in ph._lib.fhs_last_error().decode() and not pending, k
            assert outs == [_SENTINEL] * n
            e.ctx.synchronize()
            assert e.ctx.memory_in_use() == before, f"allocation {k} failed: {e.ctx.memory_in_use() - before} bytes left"
        else:
            assert k >= 1 and pending, "a warm call allocates its results' block at least"
            got = [ph.ciphertext(e.ctx, C.c_void_p(h)) for h in outs]
            assert all(np.array_equal(g.to_numpy(), w) for g, w in zip(got, want))
            break
    else:
        raise AssertionError("the sweep never reached a call without a failing allocation")


# ---------------------------------------------------------------------------------------------- nothing else moved
def test_neighbours_around_a_batched_call(env):
    """One rescale_to_next, one weighted_sums and one square_many on the same context before and after a batched
    call (they share the rescale scratch slot and the staged pointer buffer): the oracle's limbs both times."""
    e = env(1024, "b")
    ph, o, l = e.ph, e.o, 6
    rng = np.random.default_rng(90)
    xs, ps = [e.rand(rng, l) for _ in range(3)], [e.rand(rng, l, None) for _ in range(3)]
    X, Pt = [e.up(x) for x in xs], [e.upp(p) for p in ps]
    Wm = np.array([[3.0, -2.0], [-1.0, 5.0], [4.0, 1.0]])
    want_ws = []
    for i in range(2):
        acc = None
        for j in range(3):
            t = o.rescale(o.multiply_plain(xs[j], edge.constant_limbs(e.primes, l, e.N, int(Wm[j, i]))))
            acc = t if acc is None else o.add(acc, t)
        want_ws.append(acc)
    want_sq = [o.rescale(o.relinearize(o.multiply(x, x), e.rlk)) for x in xs[:2]]
    for when in ("before", "after"):
        assert np.array_equal(ph.rescale_to_next(e.ctx, X[0]).to_numpy(), e.want(xs[0])), when
        for g, w in zip(ph.weighted_sums(e.ctx, X, Wm, 1.0), want_ws):
            assert np.array_equal(g.to_numpy(), w), when
        for g, w in zip(ph.square_many(e.ctx, X[:2], e.rk), want_sq):
            assert np.array_equal(g.to_numpy(), w), when
        if when == "before":
            e.check(ph.multiply_plain_rescale_many(e.ctx, X, Pt), [e.want(x, p) for x, p in zip(xs, ps)], l, "between")
            e.check(ph.rescale_many(e.ctx, X), [e.want(x) for x in xs], l, "between, rescale_many", SCALE)
