"""Batched plaintext-weighted sums of ciphertexts (pyPhantom.weighted_sums / weighted_sum, fhs_weighted_sums; kernels
k_rescale_intt over a pointer list and k_scalar's two weighted-sum ops): the reference's ct_pt_weighted_sum
(fhe_rwkv_inference.py:79-94) for every output column in one call.

The judge is the CPU oracle's own loop -- o.add over o.rescale(o.multiply_plain(x_j, constant plaintext)) per term --
compared limb for limb (np.array_equal, no tolerance) on random residues uploaded with ciphertext_from_numpy.  The
rings, chains and Env are test_multiply_many's: N = 256 (full-limb kernels), 512 and 1024 (half-limb), chain "a"
(60, 40, 40, 60) with P = 1 at l = 3 and 2, chain "b" (59,) * 12 with P = 3 at l = 9, 6 and 2.  The recorded reference
runs of tests/golden/fri_trace.json are replayed with their 8 x 8 and 8 x 4 weighted sums as two calls.
Every test here needs an MI355X: -m gpu."""
import ctypes as C
import gc
import hashlib
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest

from test_multiply_many import CHAINS, SCALE, Env

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tools"))
CONFIGS = [(N, ch, l) for N in (256, 512, 1024) for ch, levels in (("a", (3, 2)), ("b", (9, 6, 2))) for l in levels]
SHAPES = [(1, 1), (2, 3), (5, 9), (65, 2), (129, 1)]
OK, INVALID, OOM, LEVEL, SCALE_ERR = 0, 1, 2, 4, 5
_SENTINEL = 0xDEAD0


@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


_ENVS = {}


@pytest.fixture(scope="module")
def env(ph, orc):
    def get(N, chain):
        if (N, chain) not in _ENVS:
            bits, P = CHAINS[chain]
            _ENVS[N, chain] = Env(ph, orc, N, bits, P)
        return _ENVS[N, chain]
    yield get
    _ENVS.clear()


def const_of(w, scale=SCALE):
    """round(w * scale), half away from zero, as an exact integer."""
    x = float(w) * float(scale)
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def const_pt(e, l, c):
    return np.stack([np.full(e.N, c % e.primes[m], dtype=np.uint64) for m in range(l)])


def oracle_loop(e, xs, W, l, scale=SCALE):
    """The reference's loop per output column: every term multiplied and rescaled on its own, then added.  A term is
    computed once per distinct (input, constant)."""
    W = np.asarray(W, dtype=np.float64)
    terms, outs = {}, []
    for i in range(W.shape[1]):
        acc = None
        for j in range(W.shape[0]):
            key = (id(xs[j]), const_of(W[j, i], scale))
            if key not in terms:
                terms[key] = e.o.rescale(e.o.multiply_plain(xs[j], const_pt(e, l, key[1])))
            acc = terms[key] if acc is None else e.o.add(acc, terms[key])
        outs.append(acc)
    return outs


def check(e, got, wants, l, what, scale=SCALE, in_scale=SCALE):
    assert len(got) == len(wants), what
    for i, (g, w) in enumerate(zip(got, wants)):
        assert g.size() == 2 and g.chain_index() == e.L0 + 2 - l, f"{what} output {i}"
        assert g.scale() == in_scale * scale / float(e.primes[l - 1]), f"{what} output {i}"
        assert np.array_equal(g.to_numpy(), w), f"{what} output {i}"


def weights(rng, F, E):
    """Random weights (negatives among them) with 0, +-1 and +-2^-40 (constants +-1) planted."""
    W = rng.normal(0.0, 1.0, (F, E))
    special = [0.0, 1.0, -1.0, 2.0 ** -40, -(2.0 ** -40)]
    flat = W.reshape(-1)
    for k in range(0, flat.size, 3):
        flat[k] = special[(k // 3) % 5]
    if F * E == 1:
        flat[0] = -0.75
    return W


def _raw(e, cts, W, scale=SCALE, F=None, E=None, ldw=None, ctx=True, ins=True, wp=True, outs=True):
    """The C call itself: (status, the output array as Python ints), the array pre-filled with a sentinel."""
    W = np.ascontiguousarray(W, dtype=np.float64)
    F = len(cts) if F is None else F
    E = W.shape[1] if E is None else E
    n = max(1, len(cts))
    m = max(1, W.shape[1], E)
    aa = (C.c_void_p * n)(*[c._h for c in cts])
    out = (C.c_void_p * m)(*([_SENTINEL] * m))
    rc = e.ph._lib.fhs_weighted_sums(e.ctx._h if ctx else None, aa if ins else None, F,
                                     W.ctypes.data_as(C.POINTER(C.c_double)) if wp else None,
                                     W.shape[1] if ldw is None else ldw, E, scale, out if outs else None)
    return rc, [int(v or 0) for v in out]


# ------------------------------------------------------------------------------------------------ limbs
@pytest.mark.parametrize("N,chain,l", CONFIGS)
def test_random_residues_match_the_oracle_loop(env, N, chain, l):
    """(F, E) = (1, 1), (2, 3), (5, 9), (65, 2) and (129, 1): below, at and past one tile of outputs, one and several
    64-product windows (65 inputs + the correction = 66 products; 129 + 1 = 130).  Inputs are never written."""
    e = env(N, chain)
    rng = np.random.default_rng(N + 10 * l)
    xs = [e.rand(rng, l) for _ in range(8)]
    X = [e.up(x) for x in xs]
    for F, E in SHAPES:
        W = weights(rng, F, E)
        idx = [j % 8 for j in range(F)]                 # 8 ciphertexts fill the longer input lists
        got = e.ph.weighted_sums(e.ctx, [X[j] for j in idx], W, SCALE)
        check(e, got, oracle_loop(e, [xs[j] for j in idx], W, l), l, f"N={N} chain {chain} l={l} F={F} E={E}")
    for c, x in zip(X, xs):
        assert np.array_equal(c.to_numpy(), x), "an input was written"


@pytest.mark.parametrize("N,chain,l", CONFIGS)
def test_wrapping_operands_with_weight_minus_one(env, N, chain, l):
    """Every residue of every input q_i - 1 and every weight -1 (constant -2^40), F = 65 and 3, E = 5 and 1: the largest
    split-30 partials and window sums on every limb (the 60-bit ones of chain "a" too); and constant -1 (weight -2^-40),
    whose products are q - (q - 1) = 1."""
    e = env(N, chain)
    w = e.worst(l)
    X = e.up(w)
    for F, E in ((65, 5), (3, 1)):
        for weight in (-1.0, -(2.0 ** -40)):
            W = np.full((F, E), weight)
            check(e, e.ph.weighted_sums(e.ctx, [X] * F, W, SCALE), oracle_loop(e, [w] * F, W, l), l,
                  f"worst N={N} chain {chain} l={l} F={F} E={E} w={weight}")
    assert np.array_equal(X.to_numpy(), w)


def test_repeated_handle_ldw_and_single_sum(env):
    """One handle several times in `in` (next to a distinct handle with equal limbs); ldw > E through the C call; the
    E = 1 binding."""
    e = env(512, "b")
    ph, l = e.ph, 6
    rng = np.random.default_rng(41)
    xs = [e.rand(rng, l) for _ in range(2)]
    A, B, A2 = e.up(xs[0]), e.up(xs[1]), e.up(xs[0])
    W = weights(rng, 5, 3)
    want = oracle_loop(e, [xs[0], xs[1], xs[0], xs[0], xs[1]], W, l)
    check(e, ph.weighted_sums(e.ctx, [A, B, A, A2, B], W, SCALE), want, l, "repeated handle")
    wide = np.full((5, 7), np.nan)                    # the columns past E are never read
    wide[:, :3] = W
    rc, outs = _raw(e, [A, B, A, A2, B], wide, E=3, ldw=7)
    assert rc == OK
    check(e, [ph.ciphertext(e.ctx, C.c_void_p(h)) for h in outs[:3]], want, l, "ldw > E")
    assert outs[3:] == [_SENTINEL] * 4
    one = ph.weighted_sum(e.ctx, [A, B, A, A2, B], W[:, 1], SCALE)
    check(e, [one], [want[1]], l, "weighted_sum")


@pytest.mark.parametrize("N,chain,l", [(256, "a", 3), (1024, "b", 9)])
def test_one_term_equals_multiply_plain_and_rescale(env, N, chain, l):
    """F = 1, E = 1 against the GPU's own multiply_plain + rescale_to_next of the imported constant plaintext; another
    scale than the inputs'."""
    e = env(N, chain)
    ph = e.ph
    x = e.rand(np.random.default_rng(N), l)
    X = e.up(x)
    for w, scale in ((0.3712, SCALE), (-1.5, 2.0 ** 33), (3.0, 1.0)):
        pt = ph.plaintext_from_numpy(e.ctx, const_pt(e, l, const_of(w, scale)), e.L0 + 1 - l, scale)
        want = ph.rescale_to_next(e.ctx, ph.multiply_plain(e.ctx, X, pt))
        got = ph.weighted_sum(e.ctx, [X], [w], scale)
        assert np.array_equal(got.to_numpy(), want.to_numpy())
        assert got.scale() == want.scale() and got.chain_index() == want.chain_index() == e.L0 + 2 - l
        check(e, [got], oracle_loop(e, [x], [[w]], l, scale), l, "one term", scale)


def test_more_outputs_than_one_chunk(env):
    """E = 513 at N = 256, l = 2, F = 2: two chunks (257 + 256 outputs, the second starting inside a tile); every
    result is checked."""
    e = env(256, "a")
    rng = np.random.default_rng(513)
    xs = [e.rand(rng, 2) for _ in range(2)]
    W = rng.integers(-3, 4, (2, 513)).astype(np.float64) * 0.25   # 7 x 7 distinct terms
    got = e.ph.weighted_sums(e.ctx, [e.up(x) for x in xs], W, SCALE)
    check(e, got, oracle_loop(e, xs, W, 2), 2, "E=513")


# ------------------------------------------------------------------------------------------------ reference fixture
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def _symbolic(case):
    """The trace's weighted sums read off its ops: sym[id] = list of (input ciphertext id, weight) for every object
    that is a sum of rescaled constant products; finals = those a non-add op consumes (the next stage, decrypt)."""
    const, sym, skipped = {}, {}, set()
    for op, out, ins, extra in case["ops"]:
        if op == "encode" and "const" in extra:
            const[out] = (extra["const"], extra["scale"])
        elif op == "mod_switch_to" and ins[0] in const:
            const[out] = const[ins[0]]
        elif op == "multiply_plain" and ins[1] in const:
            sym[out] = ("prod", ins[0], const[ins[1]])
        elif op == "rescale_to_next" and ins[0] in sym:
            _, ct, (w, scale) = sym[ins[0]]
            sym[out] = ("sum", [(ct, w)], scale)
        elif op == "add" and ins[0] in sym and ins[1] in sym:
            assert sym[ins[0]][2] == sym[ins[1]][2]
            sym[out] = ("sum", sym[ins[0]][1] + sym[ins[1]][1], sym[ins[0]][2])
        else:
            continue
        skipped.add(out)
    used = {v[1] for v in sym.values() if v[0] == "prod" and v[1] in sym}   # the next stage's inputs
    for op, out, ins, extra in case["ops"]:
        if out not in skipped:
            used.update(i for i in ins if i in sym)
    finals = [o for o in sorted(used) if sym[o][0] == "sum"]
    return sym, skipped, finals


@pytest.mark.parametrize("name", ["inference_n4096", "inference_n32768"])
def test_reference_run_weighted_sums_as_two_calls(ph, orc, name):
    """The recorded reference run replayed op by op up to ct_k_sq; its 8 x 8 weighted sums at chain index 3 and 8 x 4 at
    chain index 4 (per term: encode a constant, mod_switch_to, multiply_plain, rescale_to_next, add) made by two
    weighted_sums calls from the recorded constants.  The outputs carry the recorded SHA-256, scale and chain index of
    the loop's final add objects, the decrypted plaintexts the recorded SHA-256, and the logits decoded from them by
    the reference run's decoder equal the recorded ones."""
    import fri_replay
    from test_fri_ring import _OracleEncoder
    case = json.loads((REPO / "tests" / "golden" / "fri_trace.json").read_text())["cases"][name]
    sym, skipped, finals = _symbolic(case)
    stages = {}
    for f in finals:
        stages.setdefault(tuple(ct for ct, _ in sym[f][1]), []).append(f)
    assert sorted((len(k), len(v)) for k, v in stages.items()) == [(8, 4), (8, 8)]
    ctx, sk, pk, rlk, gk = fri_replay.make_context(ph, case)
    primes = [int(q) for q in ph.create_coeff_modulus(case["N"], case["bit_sizes"])]
    encode = _OracleEncoder(ph, case["N"], primes)
    objs, want, calls, logits = {}, case["objects"], [], []

    def need(oid):
        """The stage that makes `oid` (its inputs' stages first), as one weighted_sums call."""
        if oid in objs:
            return
        cts, outs = next((k, v) for k, v in stages.items() if oid in v)
        for ct in cts:
            need(ct)
        W = np.array([[dict(sym[f][1])[ct] for f in outs] for ct in cts])
        assert all([ct for ct, _ in sym[f][1]] == list(cts) for f in outs)
        res = ph.weighted_sums(ctx, [objs[ct] for ct in cts], W, sym[outs[0]][2])
        calls.append((len(cts), len(outs), objs[cts[0]].chain_index()))
        for f, r in zip(outs, res):
            objs[f] = r
            assert r.chain_index() == want[f]["ci"] and r.size() == 2, f
            assert abs(r.scale() - want[f]["scale"]) <= 1e-9 * abs(want[f]["scale"]), f
            assert _sha(r.to_numpy()) == want[f]["sha"], f"object {f}: limbs differ from the reference run"

    for op, out, ins, extra in case["ops"]:
        if out in skipped:
            continue
        for i in ins:
            if i in sym:
                need(i)
        a = [objs[k] for k in ins]
        if op == "encode":
            v = np.concatenate([np.asarray(extra["prefix"], dtype=np.float64), np.zeros(extra["n"] - len(extra["prefix"]))])
            r = encode(ctx, v, extra["scale"], extra["chain_index"])
        elif op == "encrypt_asymmetric":
            r = pk.encrypt_asymmetric(ctx, a[0])
        elif op == "multiply_plain":
            r = ph.multiply_plain(ctx, a[0], a[1])
        elif op == "rescale_to_next":
            r = ph.rescale_to_next(ctx, a[0])
        elif op == "rotate":
            r = ph.rotate(ctx, a[0], extra["step"], gk)
        elif op == "add":
            r = ph.add(ctx, a[0], a[1])
        elif op == "multiply":
            r = ph.multiply(ctx, a[0], a[1])
        elif op == "relinearize":
            r = ph.relinearize(ctx, a[0], rlk)
        elif op == "decrypt":
            r = sk.decrypt(ctx, a[0])
            assert _sha(r.to_numpy()) == want[out]["sha"]
        elif op == "decode":
            logits.append((float(encode.o.decode(a[0].to_numpy(), a[0].scale())[0].real), extra["slot0"]))
            continue
        else:
            raise AssertionError(f"unexpected op {op}")
        objs[out] = r
    assert calls == [(8, 8, 3), (8, 4, 4)]
    assert len(logits) == 4 and np.array_equal(np.array([g for g, _ in logits]), np.array([w for _, w in logits]))


# ------------------------------------------------------------------------------------------------ ordering, lifetime
def test_queued_rotations_as_inputs(env):
    """Inputs that are still-queued outputs of rotate: the entry flushes first."""
    e = env(512, "b")
    ph = e.ph
    rng = np.random.default_rng(71)
    a, b = e.rand(rng, 6), e.rand(rng, 6)
    ca, cb = e.up(a), e.up(b)
    W = weights(rng, 3, 2)
    got = ph.weighted_sums(e.ctx, [ph.rotate(e.ctx, ca, 1, e.gk), cb, ph.rotate(e.ctx, cb, 2, e.gk)], W, SCALE)
    ra, rb = e.o.rotate(a, e.okey(1), 1), e.o.rotate(b, e.okey(2), 2)
    check(e, got, oracle_loop(e, [ra, b, rb], W, 6), 6, "queued inputs")


def test_inputs_may_die_at_once_and_memory_returns(env):
    """Destroying the inputs right after the call is safe (their blocks are reused before the results are read), and
    memory_in_use is back at its earlier value once all results are gone -- not before the last one goes."""
    e = env(1024, "b")
    ph, l = e.ph, 6
    rng = np.random.default_rng(72)
    xs = [e.rand(rng, l) for _ in range(5)]
    W = weights(rng, 5, 6)
    wants = oracle_loop(e, xs, W, l)
    warm = ph.weighted_sums(e.ctx, [e.up(x) for x in xs], W, SCALE)       # warms the scratch slots
    del warm
    gc.collect()
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    A = [e.up(x) for x in xs]
    got = ph.weighted_sums(e.ctx, A, W, SCALE)
    del A[:]
    gc.collect()
    filler = [e.up(x) for x in xs]                   # takes the inputs' blocks back from the cache and overwrites them
    e.ctx.synchronize()
    assert all(np.array_equal(got[i].to_numpy(), wants[i]) for i in range(6))   # (no loop variable keeps a result)
    keep = got.pop()                                 # one result keeps the shared block
    del got[:]
    gc.collect()
    assert e.ctx.memory_in_use() >= before + sum(f.to_numpy().nbytes for f in filler) + 6 * wants[0].nbytes
    assert np.array_equal(keep.to_numpy(), wants[-1])
    del keep, filler
    gc.collect()
    e.ctx.synchronize()
    assert e.ctx.memory_in_use() == before


@pytest.mark.parametrize("F,E", [(1, 1), (3, 5)])
def test_every_allocation_failing_once(env, F, E):
    """fhs_debug_fail_alloc at each allocation a warm call makes: each is "out of memory", leaves nothing allocated
    and the output array untouched, and the next call gives the same limbs."""
    e = env(512, "a")
    ph, l = e.ph, 3
    rng = np.random.default_rng(82)
    xs = [e.rand(rng, l) for _ in range(F)]
    A = [e.up(x) for x in xs]
    W = weights(rng, F, E)
    want = oracle_loop(e, xs, W, l)
    warm = ph.weighted_sums(e.ctx, A, W, SCALE)
    check(e, warm, want, l, "warm")
    del warm
    gc.collect()
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    for k in range(16):
        ph.debug_fail_alloc(e.ctx, k)
        rc, outs = _raw(e, A, W)
        pending = ph.debug_fail_alloc(e.ctx, -1)
        if rc != OK:
            assert rc == OOM and "out of memory" in ph._lib.fhs_last_error().decode() and not pending, k
            assert outs == [_SENTINEL] * E
            e.ctx.synchronize()
            assert e.ctx.memory_in_use() == before, f"allocation {k} failed: {e.ctx.memory_in_use() - before} bytes left"
        else:
            assert k >= 1 and pending, "a warm call allocates its results' block at least"
            check(e, [ph.ciphertext(e.ctx, C.c_void_p(h)) for h in outs], want, l, "after the sweep")
            break
    else:
        raise AssertionError("the sweep never reached a call without a failing allocation")


# ------------------------------------------------------------------------------------------------ error contract
def test_argument_errors(env):
    e = env(256, "a")
    ph = e.ph
    rng = np.random.default_rng(80)
    a, b = e.up(e.rand(rng, 3)), e.up(e.rand(rng, 3))
    low, last = e.up(e.rand(rng, 2)), e.up(e.rand(rng, 1))
    other = e.up(e.rand(rng, 3), 2.0 ** 39)
    three = ph.multiply(e.ctx, a, b)
    W = np.array([[0.5, -0.25], [1.0, 0.0]])
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    untouched = [_SENTINEL, _SENTINEL]
    err = lambda: ph._lib.fhs_last_error().decode()   # noqa: E731
    assert _raw(e, [a, b], W, ctx=False)[0] == INVALID and "null context" in err()
    for kw in ({"ins": False}, {"wp": False}):
        assert _raw(e, [a, b], W, **kw) == (INVALID, untouched) and "null argument" in err()
    assert _raw(e, [a, b], W, outs=False)[0] == INVALID
    for F in (0, -1, 4097):
        assert _raw(e, [a, b], W, F=F) == (INVALID, untouched) and "1 <= F <= 4096" in err()
    for E in (0, -3):
        assert _raw(e, [a, b], W, E=E) == (INVALID, untouched) and "E >= 1" in err()
    assert _raw(e, [a, b], W, ldw=1) == (INVALID, untouched) and "ldw >= E" in err()
    for scale in (0.0, -SCALE, float("inf"), float("nan")):
        assert _raw(e, [a, b], W, scale=scale) == (INVALID, untouched) and "bad scale" in err()
    for bad in (float("nan"), float("inf"), -float("inf")):
        Wb = W.copy()
        Wb[1, 1] = bad
        assert _raw(e, [a, b], Wb) == (INVALID, untouched) and "not finite" in err()
    Wb = W.copy()
    Wb[1, 0] = -(2.0 ** 22)                              # constant -2^62
    assert _raw(e, [a, b], Wb) == (INVALID, untouched) and ">= 2^62" in err()
    for cts in ([a, three], [three, b]):
        assert _raw(e, cts, W) == (INVALID, untouched) and "2-component" in err()
    for cts in ([a, low], [low, a]):
        assert _raw(e, cts, W) == (LEVEL, untouched) and "chain index" in err()
    assert _raw(e, [last, last], W) == (LEVEL, untouched) and "no level left" in err()
    for cts in ([a, other], [other, a]):
        assert _raw(e, cts, W) == (SCALE_ERR, untouched) and "scale mismatch" in err()
    with pytest.raises(ValueError, match="F = 2 rows"):
        ph.weighted_sums(e.ctx, [a, b], W[:1], SCALE)
    with pytest.raises(ValueError, match="1 <= F"):
        ph.weighted_sums(e.ctx, [], np.zeros((0, 2)), SCALE)
    with pytest.raises(ValueError, match="E >= 1"):
        ph.weighted_sums(e.ctx, [a, b], np.zeros((2, 0)), SCALE)
    with pytest.raises(ValueError, match="no level left"):
        ph.weighted_sum(e.ctx, [last], [0.5], SCALE)
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
        ph.weighted_sum(e.ctx, [r], [0.5], SCALE)        # the entry's flush fails: r is lost
    with pytest.raises(ValueError, match="ciphertext lost"):
        ph.weighted_sums(e.ctx, [a, r], np.ones((2, 2)), SCALE)
    check(e, [ph.weighted_sum(e.ctx, [a], [0.5], SCALE)], oracle_loop(e, [x], [[0.5]], 3), 3, "after a lost input")


# ------------------------------------------------------------------------------------------------ nothing else moved
@pytest.mark.parametrize("N,chain,l", [(256, "a", 3), (1024, "a", 2), (512, "b", 9), (1024, "b", 6)])
def test_constant_ops_of_the_same_kernel_still_equal_the_oracle(env, N, chain, l):
    """multiply_const / add_const (k_scalar's first two ops) before and after a weighted_sums on the same context,
    random and worst-case operands, negative and zero constants."""
    e = env(N, chain)
    ph = e.ph
    rng = np.random.default_rng(N + l)
    x, w = e.rand(rng, l), e.worst(l)
    X, Wc = e.up(x), e.up(w)
    for when in ("before", "after"):
        for v in (0.0, 1.0, -1.0, 0.3712, -123.456):
            for a, ca in ((x, X), (w, Wc)):
                got = ph.multiply_const(e.ctx, ca, v, SCALE)
                assert got.scale() == SCALE * SCALE and got.chain_index() == e.L0 + 1 - l
                assert np.array_equal(got.to_numpy(), e.o.scalar(a, const_of(v), False)), (when, v)
                got = ph.add_const(e.ctx, ca, v)
                assert np.array_equal(got.to_numpy(), e.o.scalar(a, const_of(v), True)), (when, v)
        if when == "before":
            check(e, ph.weighted_sums(e.ctx, [X, Wc], [[0.5], [-2.0]], SCALE), oracle_loop(e, [x, w], [[0.5], [-2.0]], l), l, "between")
    three = ph.multiply(e.ctx, X, Wc)                       # 3 components: add_const touches component 0 only
    assert np.array_equal(ph.add_const(e.ctx, three, -7.0).to_numpy()[1:], e.o.multiply(x, w)[1:])
