"""Batched CT x CT multiply, relinearize and rescale (pyPhantom.multiply_relin_many / square_many,
fhs_multiply_relin_many, kernel k_tensor): the reference's ct_ct_square / ct_ct_multiply (fhe_rwkv_inference.py:97-108)
for n pairs in one call -- per chunk one tensor launch, one batched key switch, one rescale launch.

The judge is the CPU oracle's own loop o.rescale(o.relinearize(o.multiply(a, b), rlk)) per pair, compared limb for
limb, on random residues uploaded with ciphertext_from_numpy.  N = 256 runs the full-limb key switch, N = 512 and 1024
the half-limb forms: chain "a" (60, 40, 40, 60) with P = 1 (exact and SEAL convention) and chain "b" (59,) * 12 with
P = 3, each at its top level and lower ones (l = 3, 2; l = 9, 6, 2).  The recorded reference run
tests/golden/fri_trace.json (8 FFN columns squared) is replayed through one call.
Every test here needs an MI355X: -m gpu."""
import ctypes as C
import gc
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tools"))
SCALE = 2.0 ** 40
SEED = 6262
CHAINS = {"a": ((60, 40, 40, 60), 1), "b": ((59,) * 12, 3)}
# (N, chain, key-switch mode, l): the top level and lower ones of every chain and ring
CONFIGS = [(N, ch, mode, l) for N in (256, 512, 1024)
           for ch, mode, levels in (("a", "exact", (3, 2)), ("b", "exact", (9, 6, 2)), ("a", "seal", (3, 2))) for l in levels]
OK, INVALID, OOM, LEVEL = 0, 1, 2, 4
_SENTINEL = 0xDEAD0


@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


class Env:
    """GPU context with a relinearization key and Galois keys for steps 1, 2 and 8, and the oracle with the same keys."""

    def __init__(self, ph, orc, N, bits, P, mode="exact"):
        primes = ph.create_coeff_modulus(N, list(bits))
        self.steps = [1, 2, 8]
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
        if mode != "exact":
            self.ctx.set_key_switch_mode(mode)
            self.o.set_key_switch_mode(mode)
        self.sk = ph.secret_key(self.ctx, seed=SEED)
        self.gk = self.sk.create_galois_keys(self.ctx)
        self.rk = self.sk.gen_relinkey(self.ctx)
        self.s = self.o.gen_secret(SEED)
        self.rlk = self.o.gen_relin_key(SEED, self.s)
        self._okeys = {}

    def okey(self, step):
        if step not in self._okeys:
            self._okeys[step] = self.o.gen_galois_key(SEED, self.s, self.ph.get_elt_from_step(step, self.N))
        return self._okeys[step]

    def rand(self, rng, l, ncomp=2):
        return np.stack([np.stack([rng.integers(0, self.primes[i], self.N, dtype=np.uint64) for i in range(l)])
                         for _ in range(ncomp)])

    def worst(self, l):
        return np.stack([np.stack([np.full(self.N, self.primes[i] - 1, dtype=np.uint64) for i in range(l)])
                         for _ in range(2)])

    def up(self, a, scale=SCALE):
        return self.ph.ciphertext_from_numpy(self.ctx, a, self.L0 + 1 - a.shape[1], scale)

    def want(self, a, b, relin=True, rescale=True):
        """The reference's three calls on the oracle."""
        t = self.o.multiply(a, b)
        if relin:
            t = self.o.relinearize(t, self.rlk)
        return self.o.rescale(t) if rescale else t

    def out_scale(self, l, rescale=True, sa=SCALE, sb=SCALE):
        return sa * sb / float(self.primes[l - 1]) if rescale else sa * sb

    def check(self, got, wants, l, what, ncomp=2, rescale=True):
        assert len(got) == len(wants), what
        for i, (g, w) in enumerate(zip(got, wants)):
            assert g.size() == ncomp and g.chain_index() == self.L0 + 1 - l + (1 if rescale else 0), f"{what} item {i}"
            assert g.scale() == self.out_scale(l, rescale), f"{what} item {i}"
            assert np.array_equal(g.to_numpy(), w), f"{what} item {i}"


_ENVS = {}


@pytest.fixture(scope="module")
def env(ph, orc):
    def get(N, chain, mode="exact"):
        key = (N, chain, mode)
        if key not in _ENVS:
            bits, P = CHAINS[chain]
            _ENVS[key] = Env(ph, orc, N, bits, P, mode)
        return _ENVS[key]
    yield get
    _ENVS.clear()


def _raw(e, a, b, rk, rescale=1, n=None, ctx=True, ins=True, outs=True):
    """The C call itself: (status, the output array as Python ints), the array pre-filled with a sentinel."""
    ph = e.ph
    n = len(a) if n is None else n
    m = max(1, len(a))
    aa = (C.c_void_p * m)(*[c._h for c in a])
    bb = None if b is None else (C.c_void_p * m)(*[c._h for c in b])
    out = (C.c_void_p * m)(*([_SENTINEL] * m))
    rc = ph._lib.fhs_multiply_relin_many(e.ctx._h if ctx else None, aa if ins else None, bb, n,
                                         rk._h if rk is not None else None, rescale, out if outs else None)
    return rc, [int(v or 0) for v in out]


@pytest.mark.parametrize("N,chain,mode,l", CONFIGS)
def test_pairs_and_squares_match_oracle_loop(env, N, chain, mode, l):
    """n = 1, 2, 5 and 9 in one call, as pairs and as squares given three ways (b = None; b[i] the same handle as
    a[i]; b[i] a distinct handle with equal limbs), and one handle used in three pairs.  Inputs are never written."""
    e = env(N, chain, mode)
    ph = e.ph
    rng = np.random.default_rng(N + 10 * l)
    xs, ys = [e.rand(rng, l) for _ in range(9)], [e.rand(rng, l) for _ in range(9)]
    A, B, A2 = [e.up(x) for x in xs], [e.up(y) for y in ys], [e.up(x) for x in xs]
    pair = [e.want(x, y) for x, y in zip(xs, ys)]
    sq = [e.want(x, x) for x in xs]
    what = f"N={N} chain {chain} {mode} l={l}"
    for n in (1, 2, 5, 9):
        e.check(ph.multiply_relin_many(e.ctx, A[:n], B[:n], e.rk), pair[:n], l, f"{what} n={n} pairs")
        e.check(ph.square_many(e.ctx, A[:n], e.rk), sq[:n], l, f"{what} n={n} squares, b=None")
        e.check(ph.multiply_relin_many(e.ctx, A[:n], A[:n], e.rk), sq[:n], l, f"{what} n={n} squares, same handles")
        e.check(ph.multiply_relin_many(e.ctx, A[:n], A2[:n], e.rk), sq[:n], l, f"{what} n={n} squares, equal limbs")
    # A[0] in three pairs (as a, as b, as both), pairs and a square in one launch
    got = ph.multiply_relin_many(e.ctx, [A[0], A[1], A[0]], [B[0], A[0], A[0]], e.rk)
    e.check(got, [pair[0], e.want(xs[1], xs[0]), sq[0]], l, f"{what} shared handle")
    for c, x in zip(A + B + A2, xs + ys + xs):
        assert np.array_equal(c.to_numpy(), x), f"{what}: an input was written"


@pytest.mark.parametrize("N,chain,mode,l", CONFIGS)
def test_wrapping_operands(env, N, chain, mode, l):
    """Every residue of every operand q_i - 1, as pairs and as squares: every product is (q - 1)^2 and the 128-bit
    middle term 2 (q - 1)^2 sits at its maximum (on the 60-bit limbs of chain "a" too)."""
    e = env(N, chain, mode)
    ph = e.ph
    w = e.worst(l)
    want = e.want(w, w)
    W1, W2 = e.up(w), e.up(w)
    what = f"worst N={N} chain {chain} {mode} l={l}"
    e.check(ph.multiply_relin_many(e.ctx, [W1, W1], [W2, W2], e.rk), [want, want], l, what + " pairs")
    e.check(ph.multiply_relin_many(e.ctx, [W1], [W2], e.rk), [want], l, what + " one pair")
    e.check(ph.square_many(e.ctx, [W1, W2], e.rk), [want, want], l, what + " squares")
    e.check(ph.square_many(e.ctx, [W1], e.rk), [want], l, what + " one square")
    assert np.array_equal(W1.to_numpy(), w) and np.array_equal(W2.to_numpy(), w)


def test_stage_combinations(env):
    """N = 512, chain "b", l = 6: without the key the 3-component product (o.multiply itself), rescaled or not;
    with the key and no rescale 2 components at the product scale and the same chain index."""
    e = env(512, "b")
    ph, l = e.ph, 6
    rng = np.random.default_rng(61)
    xs, ys = [e.rand(rng, l) for _ in range(3)], [e.rand(rng, l) for _ in range(3)]
    A, B = [e.up(x) for x in xs], [e.up(y) for y in ys]
    for relin, rescale in ((False, False), (False, True), (True, False)):
        rk = e.rk if relin else None
        ncomp = 2 if relin else 3
        for n in (1, 3):
            got = ph.multiply_relin_many(e.ctx, A[:n], B[:n], rk, rescale=rescale)
            e.check(got, [e.want(x, y, relin, rescale) for x, y in zip(xs[:n], ys[:n])], l,
                    f"relin={relin} rescale={rescale} n={n}", ncomp, rescale)
            got = ph.square_many(e.ctx, A[:n], rk, rescale=rescale)
            e.check(got, [e.want(x, x, relin, rescale) for x in xs[:n]], l,
                    f"squares relin={relin} rescale={rescale} n={n}", ncomp, rescale)
    plain = ph.multiply_relin_many(e.ctx, A[:1], B[:1], None, rescale=False)[0]
    assert np.array_equal(plain.to_numpy(), e.o.multiply(xs[0], ys[0])) and plain.size() == 3
    assert plain.chain_index() == e.L0 + 1 - l and plain.scale() == SCALE * SCALE


def test_last_level(env):
    """l = 1: the call works without rescale (relinearized at the last level) and is FHS_ERR_LEVEL with it."""
    e = env(256, "a")
    ph = e.ph
    rng = np.random.default_rng(62)
    xs = [e.rand(rng, 1) for _ in range(2)]
    A = [e.up(x) for x in xs]
    got = ph.square_many(e.ctx, A, e.rk, rescale=False)
    e.check(got, [e.want(x, x, True, False) for x in xs], 1, "l=1", 2, False)
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    assert _raw(e, A, None, e.rk, 1) == (LEVEL, [_SENTINEL] * 2)
    assert "rescale_to_next: no level left" in ph._lib.fhs_last_error().decode()
    with pytest.raises(ValueError, match="no level left"):
        ph.multiply_relin_many(e.ctx, A, A, e.rk)
    assert e.ctx.memory_in_use() == before


def test_more_pairs_than_one_item_buffer(env):
    """n = 513 squares at N = 256, l = 2: two chunks (257 + 256), each within the 512-item buffer; every result
    is checked."""
    e = env(256, "a")
    rng = np.random.default_rng(513)
    xs = [e.rand(rng, 2) for _ in range(513)]
    got = e.ph.square_many(e.ctx, [e.up(x) for x in xs], e.rk)
    e.check(got, [e.want(x, x) for x in xs], 2, "n=513")


@pytest.mark.parametrize("N", [512, 1024])
def test_large_grid_takes_two_vectors_per_thread(env, N):
    """k_tensor reads two 16-byte vectors per thread once that leaves 8 workgroups per CU (2048): n = 230 at l = 9 is
    2070 workgroups of 1024 coefficients (at N = 512 the second vector of every thread lies past the row and is
    masked).  8 ciphertexts in 230 pairs, squares among them, without key and rescale: every product equals
    o.multiply."""
    e = env(N, "b")
    l, n = 9, 230
    rng = np.random.default_rng(N + 230)
    xs = [e.rand(rng, l) for _ in range(7)] + [e.worst(l)]
    X = [e.up(x) for x in xs]
    ia, ib = [i % 8 for i in range(n)], [(3 * i + i // 8) % 8 for i in range(n)]
    assert any(p == q for p, q in zip(ia, ib)) and any(p != q for p, q in zip(ia, ib))
    want = {}
    for p, q in set(zip(ia, ib)):
        want[p, q] = e.o.multiply(xs[p], xs[q])
    got = e.ph.multiply_relin_many(e.ctx, [X[p] for p in ia], [X[q] for q in ib], None, rescale=False)
    e.check(got, [want[p, q] for p, q in zip(ia, ib)], l, f"N={N} n={n}", 3, False)
    sq = e.ph.square_many(e.ctx, [X[p] for p in ia], None, rescale=False)
    e.check(sq, [e.o.multiply(xs[p], xs[p]) for p in range(8)] * 28 + [e.o.multiply(xs[p], xs[p]) for p in range(6)], l,
            f"N={N} n={n} squares", 3, False)
    for c, x in zip(X, xs):
        assert np.array_equal(c.to_numpy(), x)


def test_scales_differ_per_pair(env):
    """Three pairs with a different scale per operand: each output's scale is that of the three single calls."""
    e = env(512, "a")
    ph = e.ph
    rng = np.random.default_rng(63)
    xs, ys = [e.rand(rng, 3) for _ in range(3)], [e.rand(rng, 3) for _ in range(3)]
    sa, sb = [2.0 ** 40, 2.0 ** 33, 3.0 * 2.0 ** 20], [2.0 ** 38, 5.0 * 2.0 ** 30, 2.0 ** 40 / 3.0]
    A, B = [e.up(x, s) for x, s in zip(xs, sa)], [e.up(y, s) for y, s in zip(ys, sb)]
    for rescale in (True, False):
        got = ph.multiply_relin_many(e.ctx, A, B, e.rk, rescale=rescale)
        for g, a, b, x, y in zip(got, A, B, xs, ys):
            one = ph.relinearize(e.ctx, ph.multiply(e.ctx, a, b), e.rk)
            if rescale:
                one = ph.rescale_to_next(e.ctx, one)
            assert g.scale() == one.scale() and g.chain_index() == one.chain_index()
            assert np.array_equal(g.to_numpy(), e.want(x, y, True, rescale))
    sq = ph.square_many(e.ctx, A, e.rk)
    for g, a in zip(sq, A):
        assert g.scale() == ph.rescale_to_next(e.ctx, ph.relinearize(e.ctx, ph.multiply(e.ctx, a, a), e.rk)).scale()


@pytest.mark.parametrize("N", [256, 1024])
@pytest.mark.parametrize("chain,l", [("a", 3), ("b", 9)])
def test_single_multiply_is_the_same_kernel(env, N, chain, l):
    """ph.multiply (the n = 1 case of k_tensor, its pointers as kernel arguments) still equals o.multiply, for a
    pair, for one handle twice and for worst-case operands."""
    e = env(N, chain)
    ph = e.ph
    rng = np.random.default_rng(N + l)
    x, y, w = e.rand(rng, l), e.rand(rng, l), e.worst(l)
    X, Y, W = e.up(x), e.up(y), e.up(w)
    for a, b, ca, cb in ((x, y, X, Y), (x, x, X, X), (w, w, W, W), (w, y, W, Y)):
        got = ph.multiply(e.ctx, ca, cb)
        assert got.size() == 3 and got.scale() == SCALE * SCALE and got.chain_index() == e.L0 + 1 - l
        assert np.array_equal(got.to_numpy(), e.o.multiply(a, b))
    assert np.array_equal(X.to_numpy(), x) and np.array_equal(Y.to_numpy(), y)


# ---------------------------------------------------------------------------------------------- reference fixture
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def _fri_front(ph, orc):
    """tests/golden/fri_trace.json case inference_n4096 replayed up to its first multiply, the rotate / add chains
    left out: (ctx, gk, rlk, the rescaled products, the recorded objects of the 8 rescale_to_next that follow the
    trace's multiply / relinearize ops)."""
    import fri_replay
    case = json.loads((REPO / "tests" / "golden" / "fri_trace.json").read_text())["cases"]["inference_n4096"]
    ctx, sk, pk, rlk, gk = fri_replay.make_context(ph, case)
    primes = [int(q) for q in ph.create_coeff_modulus(case["N"], case["bit_sizes"])]
    o = orc.Oracle(case["N"], primes, 1)
    objs, root, steps = {}, {}, {}
    prods = []
    relins, squared = set(), []
    front = True
    for op, out, ins, extra in case["ops"]:
        if op == "multiply":
            front = False
            assert ins[0] == ins[1]
        if not front:
            if op == "relinearize":
                relins.add(out)
            elif op == "rescale_to_next" and ins[0] in relins:
                squared.append(case["objects"][out])
            continue
        if op == "encode":
            v = np.concatenate([np.asarray(extra["prefix"], dtype=np.float64), np.zeros(extra["n"] - len(extra["prefix"]))])
            limbs = o.encode(v, extra["scale"], o.L0 + 1 - extra["chain_index"])
            objs[out] = ph.plaintext_from_numpy(ctx, limbs, extra["chain_index"], extra["scale"])
        elif op == "encrypt_asymmetric":
            objs[out] = pk.encrypt_asymmetric(ctx, objs[ins[0]])
        elif op == "multiply_plain":
            objs[out] = ph.multiply_plain(ctx, objs[ins[0]], objs[ins[1]])
        elif op == "rescale_to_next":
            objs[out] = ph.rescale_to_next(ctx, objs[ins[0]])
            assert _sha(objs[out].to_numpy()) == case["objects"][out]["sha"]
            root[out] = out
            prods.append(out)
        elif op == "rotate":
            root[out] = root[ins[0]]
            steps.setdefault(root[out], []).append(extra["step"])
        elif op == "add":
            root[out] = root[ins[0]]
        else:
            raise AssertionError(f"unexpected op {op} before the first multiply")
    assert len(prods) == 8 and all(steps[r] == [1, 2, 4] for r in prods) and len(squared) == 8
    return ctx, gk, rlk, [objs[r] for r in prods], squared


def test_reference_run_squares_as_one_call(ph, orc):
    """The 8 FFN columns of the recorded reference run (rebuilt with one inner_sum_many(dim=8)) through ONE
    square_many: the 8 results carry the recorded SHA-256, chain index and scale of the trace's 8 rescale_to_next
    objects that follow its multiply / relinearize ops."""
    ctx, gk, rlk, prods, want = _fri_front(ph, orc)
    cols = ph.inner_sum_many(ctx, prods, 8, gk)
    got = ph.square_many(ctx, cols, rlk)
    assert len(got) == 8
    for g, w in zip(got, want):
        assert g.chain_index() == w["ci"] and abs(g.scale() - w["scale"]) <= 1e-9 * abs(w["scale"])
        assert g.size() == 2 and _sha(g.to_numpy()) == w["sha"]


# ---------------------------------------------------------------------------------------------- ordering, lifetime
def test_queued_rotations_as_inputs(env):
    """Inputs that are still-queued outputs of rotate: the entry flushes first."""
    e = env(512, "b")
    ph = e.ph
    rng = np.random.default_rng(71)
    a, b = e.rand(rng, 6), e.rand(rng, 6)
    ca, cb = e.up(a), e.up(b)
    got = ph.multiply_relin_many(e.ctx, [ph.rotate(e.ctx, ca, 1, e.gk), cb], [ph.rotate(e.ctx, cb, 2, e.gk), ca], e.rk)
    ra, rb = e.o.rotate(a, e.okey(1), 1), e.o.rotate(b, e.okey(2), 2)
    e.check(got, [e.want(ra, rb), e.want(b, a)], 6, "queued pairs")
    got = ph.square_many(e.ctx, [ph.rotate(e.ctx, ca, 1, e.gk), ph.rotate(e.ctx, cb, 2, e.gk)], e.rk)
    e.check(got, [e.want(ra, ra), e.want(rb, rb)], 6, "queued squares")


def test_inputs_may_die_at_once_and_memory_returns(env):
    """Destroying the inputs right after the call is safe (their blocks are reused before the results are read), and
    memory_in_use is back at its earlier value once all results are gone -- not before the last one goes."""
    e = env(1024, "b")
    ph = e.ph
    rng = np.random.default_rng(72)
    xs, ys = [e.rand(rng, 6) for _ in range(5)], [e.rand(rng, 6) for _ in range(5)]
    wants = [e.want(x, y) for x, y in zip(xs, ys)]
    warm = ph.multiply_relin_many(e.ctx, [e.up(x) for x in xs], [e.up(y) for y in ys], e.rk)   # warms the scratch slots
    del warm
    gc.collect()
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    A, B = [e.up(x) for x in xs], [e.up(y) for y in ys]
    got = ph.multiply_relin_many(e.ctx, A, B, e.rk)
    del A[:], B[:]
    gc.collect()
    filler = [e.up(x) for x in xs + ys]              # takes the inputs' blocks back from the cache and overwrites them
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
    low = e.up(e.rand(rng, 2))
    three = ph.multiply(e.ctx, a, b)
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    untouched = [_SENTINEL, _SENTINEL]
    assert _raw(e, [a, b], [b, a], e.rk, ctx=False)[0] == INVALID
    assert "null context" in ph._lib.fhs_last_error().decode()
    assert _raw(e, [a, b], [b, a], e.rk, ins=False) == (INVALID, untouched)
    assert "null argument" in ph._lib.fhs_last_error().decode()
    assert _raw(e, [a, b], [b, a], e.rk, outs=False)[0] == INVALID
    assert _raw(e, [a, b], [b, a], e.rk, n=0) == (INVALID, untouched)
    assert "n >= 1" in ph._lib.fhs_last_error().decode()
    assert _raw(e, [a, b], None, e.rk, n=-1) == (INVALID, untouched)
    for aa, bb in (([a, three], None), ([a, b], [b, three]), ([three, b], [a, b])):
        assert _raw(e, aa, bb, e.rk) == (INVALID, untouched)
        assert "2-component" in ph._lib.fhs_last_error().decode()
    for aa, bb in (([a, low], None), ([a, b], [b, low]), ([low, low], [a, b])):    # inside a; between a and b
        assert _raw(e, aa, bb, e.rk) == (LEVEL, untouched)
        assert "chain index" in ph._lib.fhs_last_error().decode()
    with pytest.raises(ValueError, match="n >= 1"):
        ph.multiply_relin_many(e.ctx, [], [], e.rk)
    with pytest.raises(ValueError, match="n >= 1"):
        ph.square_many(e.ctx, [], e.rk)
    with pytest.raises(ValueError, match="different length"):
        ph.multiply_relin_many(e.ctx, [a, b], [a], e.rk)
    with pytest.raises(ValueError, match="chain index"):
        ph.multiply_relin_many(e.ctx, [a, b], [a, low], e.rk)
    with pytest.raises(ValueError, match="2-component"):
        ph.square_many(e.ctx, [a, three], e.rk)
    e.ctx.synchronize()
    assert e.ctx.memory_in_use() == before


def test_lost_input_is_rejected(env):
    e = env(256, "a")
    ph = e.ph
    x = e.rand(np.random.default_rng(81), 3)
    a = e.up(x)
    ph.debug_fail_next_flushes(e.ctx, 1)
    r = ph.rotate(e.ctx, a, 1, e.gk)
    with pytest.raises(RuntimeError, match="out of memory"):
        ph.square_many(e.ctx, [r], e.rk)             # the entry's flush fails: r is lost
    with pytest.raises(ValueError, match="ciphertext lost"):
        ph.square_many(e.ctx, [a, r], e.rk)
    with pytest.raises(ValueError, match="ciphertext lost"):
        ph.multiply_relin_many(e.ctx, [a, a], [a, r], e.rk)
    e.check(ph.square_many(e.ctx, [a], e.rk), [e.want(x, x)], 3, "after a lost input")


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("rescale", [1, 0])
def test_every_allocation_failing_once(env, n, rescale):
    """fhs_debug_fail_alloc at each allocation a warm call makes: each is "out of memory", leaves nothing allocated
    and the output array untouched, and the next call gives the same limbs."""
    e = env(512, "a")
    ph = e.ph
    rng = np.random.default_rng(82)
    xs, ys = [e.rand(rng, 3) for _ in range(n)], [e.rand(rng, 3) for _ in range(n)]
    A, B = [e.up(x) for x in xs], [e.up(y) for y in ys]
    want = [e.want(x, y, True, bool(rescale)) for x, y in zip(xs, ys)]
    warm = ph.multiply_relin_many(e.ctx, A, B, e.rk, rescale=bool(rescale))
    assert all(np.array_equal(g.to_numpy(), w) for g, w in zip(warm, want))
    del warm
    gc.collect()
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    for k in range(16):
        ph.debug_fail_alloc(e.ctx, k)
        rc, outs = _raw(e, A, B, e.rk, rescale)
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
def test_dot_product_and_hoisting_around_a_multiply_many(env):
    """One dot_product_many (its own relinearization through the same scratch slots and key-switch workspace) and one
    hoisting call at N = 1024, before and after a multiply_relin_many on the same context: the oracle's limbs both
    times."""
    e = env(1024, "b")
    ph, o = e.ph, e.o
    rng = np.random.default_rng(90)
    l = 9
    q = [e.rand(rng, l) for _ in range(2)]
    db = [[e.rand(rng, l) for _ in range(2)] for _ in range(3)]
    Q, DB = [e.up(x) for x in q], [[e.up(x) for x in row] for row in db]
    want_dot = []
    for row in db:
        t = o.add(o.multiply(q[0], row[0]), o.multiply(q[1], row[1]))
        want_dot.append(o.rescale(o.relinearize(t, e.rlk)))
    want_rot = {st: o.rotate(q[0], e.okey(st), st) for st in e.steps}
    xs = [e.rand(rng, l) for _ in range(3)]
    for when in ("before", "after"):
        got = ph.dot_product_many(e.ctx, Q, DB, e.rk)
        for g, w in zip(got, want_dot):
            assert np.array_equal(g.to_numpy(), w), when
        for st, r in zip(e.steps, ph.hoisting(e.ctx, Q[0], e.gk, e.steps)):
            assert np.array_equal(r.to_numpy(), want_rot[st]), (when, st)
        if when == "before":
            A = [e.up(x) for x in xs]
            e.check(ph.multiply_relin_many(e.ctx, A, A[::-1], e.rk), [e.want(x, y) for x, y in zip(xs, xs[::-1])], l, "between")
            e.check(ph.square_many(e.ctx, A, e.rk), [e.want(x, x) for x in xs], l, "between, squares")
