"""Batched rotate-and-sum (pyPhantom.inner_sum_many / fhs_inner_sum_many): the tail of the reference's ct_pt_dot
(fhe_rwkv_inference.py:71-75), x = add(x, rotate(x, stride * step)) for step = 1, 2, 4, ... < dim, for n
ciphertexts at once -- one batched key switch per step whose ModDown also adds x (KsItem::add0i into component 0
after the rotated c0, add1 into component 1).

The judge is the CPU oracle's own loop o.add(x, o.rotate(x, key, step)) per step, compared limb for limb, on random
residues uploaded with ciphertext_from_numpy.  N = 256 runs the full-limb k_moddown, N = 512 and 1024 the half-limb
forms: chain "a" (60, 40, 40, 60) with P = 1 (exact and SEAL convention) and chain "b" (59,) * 12 with P = 3 (the
X-form / B59 ModDown), each at its top level and lower ones (l = 3, 2; l = 9, 6, 2); one case at N = 32768 takes
the SPLIT form.  The recorded reference run tests/golden/fri_trace.json (8 FFN columns x 3 rotations) is replayed through one call.
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
SEED = 5151
CHAINS = {"a": ((60, 40, 40, 60), 1), "b": ((59,) * 12, 3)}
# (N, chain, key-switch mode, l): the top level and lower ones of every chain and ring
CONFIGS = [(N, ch, mode, l) for N in (256, 512, 1024)
           for ch, mode, levels in (("a", "exact", (3, 2)), ("b", "exact", (9, 6, 2)), ("a", "seal", (3, 2))) for l in levels]
OK, INVALID, LEVEL, KEY = 0, 1, 4, 6
_SENTINEL = 0xDEAD0


@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


class Env:
    """GPU context + Galois keys for every power-of-two step and N/2 - 1, and the oracle with the same keys."""

    def __init__(self, ph, orc, N, bits, P, mode="exact", steps=None):
        primes = ph.create_coeff_modulus(N, list(bits))
        self.steps = steps or sorted({1 << k for k in range((N // 2).bit_length() - 1)} | {N // 2 - 1})
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
        self.s = self.o.gen_secret(SEED)
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

    def want(self, x, dim, stride=1):
        """The reference loop on the oracle."""
        step = 1
        while step < dim:
            x = self.o.add(x, self.o.rotate(x, self.okey(stride * step), stride * step))
            step *= 2
        return x

    def check(self, xs, dim, stride=1, what=""):
        ins = [self.up(x) for x in xs]
        got = self.ph.inner_sum_many(self.ctx, ins, dim, self.gk, stride)
        assert len(got) == len(xs)
        for i, (g, x) in enumerate(zip(got, xs)):
            assert g.chain_index() == self.L0 + 1 - x.shape[1] and g.scale() == SCALE and g.size() == 2
            assert np.array_equal(g.to_numpy(), self.want(x, dim, stride)), f"{what} dim={dim} stride={stride} item {i}"
        for i, (c, x) in enumerate(zip(ins, xs)):
            assert np.array_equal(c.to_numpy(), x), f"{what} dim={dim} stride={stride}: input {i} was written"
        return got


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


def _raw(e, cts, dim, stride, gk, n=None, ctx=True, ins=True, outs=True):
    """The C call itself: (status, the output array as Python ints), the array pre-filled with a sentinel."""
    ph = e.ph
    n = len(cts) if n is None else n
    arr = (C.c_void_p * max(1, len(cts)))(*[c._h for c in cts])
    out = (C.c_void_p * max(1, len(cts)))(*([_SENTINEL] * max(1, len(cts))))
    rc = ph._lib.fhs_inner_sum_many(e.ctx._h if ctx else None, arr if ins else None, n, dim, stride,
                                    gk._h if gk is not None else None, out if outs else None)
    return rc, [int(v or 0) for v in out]


@pytest.mark.parametrize("N,chain,mode,l", CONFIGS)
def test_inner_sum_many_matches_oracle_loop(env, N, chain, mode, l):
    """dim 1 (copies), 2, 3 (steps 1 and 2), 8 and N/2 (every power-of-two step); stride 1, 4 and the largest one
    legal for dim = 2 (N/2 - 1); n = 1, 3, 4, 5 and 9 ciphertexts in one call.  Inputs are never written."""
    e = env(N, chain, mode)
    rng = np.random.default_rng(N + 10 * l)
    xs = [e.rand(rng, l) for _ in range(9)]
    for dim, stride, n in ((1, 1, 3), (2, 1, 1), (3, 1, 4), (8, 1, 5), (N // 2, 1, 1), (8, 4, 9), (2, N // 2 - 1, 3),
                           (1, 4, 1)):
        e.check(xs[:n], dim, stride, what=f"N={N} chain {chain} {mode} l={l} n={n}")


@pytest.mark.parametrize("N,chain,mode,l", CONFIGS)
def test_every_add_wraps(env, N, chain, mode, l):
    """Every residue of both components q_i - 1: each of the fused adds (the rotated c0, x0, x1) wraps."""
    e = env(N, chain, mode)
    w = e.worst(l)
    e.check([w, w], 8, what=f"worst N={N} chain {chain} {mode} l={l}")
    e.check([w], 2, N // 2 - 1, what=f"worst N={N} chain {chain} {mode} l={l}")


def test_more_ciphertexts_than_one_item_buffer(env):
    """n = 513 at N = 256, l = 2, dim = 2: two chunks (257 + 256), each within the 512-item buffer."""
    e = env(256, "a")
    rng = np.random.default_rng(513)
    e.check([e.rand(rng, 2) for _ in range(513)], 2, what="n=513")


def test_single_key_switch_at_n32768_takes_the_split_moddown(ph, orc):
    """N = 32768, six 59-bit primes with P = 3, n = 1, dim = 2: one key switch of few workgroups, whose ModDown is
    k_moddown_h's SPLIT form (two workgroups per limb and component) -- it must add x0 and x1 too."""
    e = Env(ph, orc, 32768, (59,) * 6, 3, steps=[1])
    rng = np.random.default_rng(15)
    x = e.rand(rng, 3)
    ph.debug_launch_ledger("arm")
    try:
        e.check([x], 2, what="N=32768")
    finally:
        ph.debug_launch_ledger("disarm")
    assert "k_moddown_h<15, true, true, true>" in ph.debug_launch_ledger("read")


def test_scales_may_differ_and_are_kept(env):
    e = env(512, "a")
    rng = np.random.default_rng(7)
    xs = [e.rand(rng, 3) for _ in range(3)]
    scales = [2.0 ** 40, 2.0 ** 33, 3.0 * 2.0 ** 20]
    got = e.ph.inner_sum_many(e.ctx, [e.up(x, s) for x, s in zip(xs, scales)], 4, e.gk)
    for g, x, s in zip(got, xs, scales):
        assert g.scale() == s and g.chain_index() == 1
        assert np.array_equal(g.to_numpy(), e.want(x, 4))
    one = e.ph.inner_sum(e.ctx, e.up(xs[0], scales[1]), 4, e.gk, stride=2)
    assert one.scale() == scales[1] and np.array_equal(one.to_numpy(), e.want(xs[0], 4, 2))


# ---------------------------------------------------------------------------------------------- reference fixture
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def _fri_front(ph, orc):
    """tests/golden/fri_trace.json case inference_n4096 replayed up to its first multiply, the rotate / add chains
    left out: (ctx, gk, the encrypted input, the column plaintexts, the rescaled products, the recorded digests of
    the chains' final objects)."""
    import fri_replay
    case = json.loads((REPO / "tests" / "golden" / "fri_trace.json").read_text())["cases"]["inference_n4096"]
    ctx, sk, pk, rlk, gk = fri_replay.make_context(ph, case)
    primes = [int(q) for q in ph.create_coeff_modulus(case["N"], case["bit_sizes"])]
    o = orc.Oracle(case["N"], primes, 1)
    objs, root, final, steps = {}, {}, {}, {}
    pts, prods = [], []
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
            objs[out] = ph.multiply_plain(ctx, objs[ins[0]], objs[ins[1]])
            pts.append(objs[ins[1]])
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
            final[root[out]] = out
        else:
            raise AssertionError(f"unexpected op {op} before the first multiply")
    assert len(prods) == 8 and all(steps[r] == [1, 2, 4] for r in prods)
    want = [case["objects"][final[r]] for r in prods]
    return ctx, gk, objs[1], pts, [objs[r] for r in prods], want


def test_reference_run_chains_as_one_call(ph, orc):
    """The 8 recorded rotate / add chains (steps 1, 2, 4) of the reference's FFN columns as ONE inner_sum_many(dim=8):
    the 8 final objects have the recorded SHA-256, chain index and scale; the same through ct_pt_dot_many."""
    ctx, gk, ct, pts, prods, want = _fri_front(ph, orc)
    for got in (ph.inner_sum_many(ctx, prods, 8, gk), ph.ct_pt_dot_many(ctx, ct, pts, 8, gk)):
        assert len(got) == 8
        for g, w in zip(got, want):
            assert g.chain_index() == w["ci"] and abs(g.scale() - w["scale"]) <= 1e-9 * abs(w["scale"])
            assert _sha(g.to_numpy()) == w["sha"]


# ---------------------------------------------------------------------------------------------- ordering, lifetime
def test_queued_rotations_as_inputs(env):
    """Inputs that are still-queued outputs of rotate: the entry flushes first -- the same limbs as after an
    explicit flush, both the oracle's."""
    e = env(512, "b")
    rng = np.random.default_rng(21)
    a, b = e.rand(rng, 6), e.rand(rng, 6)
    ca, cb = e.up(a), e.up(b)
    queued = e.ph.inner_sum_many(e.ctx, [e.ph.rotate(e.ctx, ca, 1, e.gk), cb, e.ph.rotate(e.ctx, cb, 2, e.gk)], 4, e.gk)
    r1, r2 = e.ph.rotate(e.ctx, ca, 1, e.gk), e.ph.rotate(e.ctx, cb, 2, e.gk)
    e.ctx.synchronize()
    r1.to_numpy()                                    # an entry of its own: the queue is flushed
    flushed = e.ph.inner_sum_many(e.ctx, [r1, cb, r2], 4, e.gk)
    wants = [e.want(e.o.rotate(a, e.okey(1), 1), 4), e.want(b, 4), e.want(e.o.rotate(b, e.okey(2), 2), 4)]
    for q, f, w in zip(queued, flushed, wants):
        assert np.array_equal(q.to_numpy(), w) and np.array_equal(f.to_numpy(), w)


def test_inputs_may_die_at_once_and_memory_returns(env):
    """Destroying the inputs right after the call is safe (the results are read after synchronize), and
    memory_in_use is back at its earlier value once the results are destroyed."""
    e = env(1024, "b")
    rng = np.random.default_rng(22)
    xs = [e.rand(rng, 6) for _ in range(5)]
    wants = [e.want(x, 8) for x in xs]
    warm = e.ph.inner_sum_many(e.ctx, [e.up(x) for x in xs], 8, e.gk)         # warms the key-switch workspace
    del warm
    gc.collect()
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    ins = [e.up(x) for x in xs]
    got = e.ph.inner_sum_many(e.ctx, ins, 8, e.gk)
    del ins[:]
    gc.collect()
    filler = [e.up(x) for x in xs]                   # takes the inputs' blocks back from the cache and overwrites them
    e.ctx.synchronize()
    assert all(np.array_equal(got[i].to_numpy(), wants[i]) for i in range(5))   # (no loop variable keeps a result)
    keep = got.pop()                                 # one result keeps the shared block
    del got[:]
    gc.collect()
    assert e.ctx.memory_in_use() > before + sum(f.to_numpy().nbytes for f in filler)
    assert np.array_equal(keep.to_numpy(), wants[-1])
    del keep, filler
    gc.collect()
    e.ctx.synchronize()
    assert e.ctx.memory_in_use() == before


# ---------------------------------------------------------------------------------------------- error contract
def test_argument_errors(env):
    e = env(256, "a")
    ph = e.ph
    rng = np.random.default_rng(30)
    a, b = e.up(e.rand(rng, 3)), e.up(e.rand(rng, 3))
    low = e.up(e.rand(rng, 2))
    before = e.ctx.memory_in_use()
    untouched = [_SENTINEL, _SENTINEL]
    assert _raw(e, [a, b], 2, 1, e.gk, ctx=False)[0] == INVALID
    assert _raw(e, [a, b], 2, 1, e.gk, ins=False) == (INVALID, untouched)
    assert _raw(e, [a, b], 2, 1, None) == (INVALID, untouched)
    assert _raw(e, [a, b], 2, 1, e.gk, outs=False)[0] == INVALID
    assert _raw(e, [a, b], 2, 1, e.gk, n=0) == (INVALID, untouched)
    assert _raw(e, [a, b], 0, 1, e.gk) == (INVALID, untouched)
    assert _raw(e, [a, b], 2, 0, e.gk) == (INVALID, untouched)
    assert _raw(e, [a, b], 2, e.N // 2, e.gk) == (INVALID, untouched)          # step N/2: no rotation
    assert _raw(e, [a, b], 4, e.N // 4, e.gk) == (INVALID, untouched)          # steps N/4 and N/2
    assert _raw(e, [a, b], e.N, 1, e.gk) == (INVALID, untouched)
    assert _raw(e, [a, ph.multiply(e.ctx, a, b)], 2, 1, e.gk) == (INVALID, untouched)
    assert "2-component" in ph._lib.fhs_last_error().decode()
    assert _raw(e, [a, low], 2, 1, e.gk) == (LEVEL, untouched)
    with pytest.raises(ValueError, match="n >= 1"):
        ph.inner_sum_many(e.ctx, [], 2, e.gk)
    with pytest.raises(ValueError, match="dim >= 1"):
        ph.inner_sum(e.ctx, a, 0, e.gk)
    with pytest.raises(ValueError, match="stride >= 1"):
        ph.inner_sum(e.ctx, a, 2, e.gk, stride=-1)
    with pytest.raises(ValueError, match="largest step"):
        ph.inner_sum(e.ctx, a, e.N, e.gk)
    with pytest.raises(ValueError, match="chain index"):
        ph.inner_sum_many(e.ctx, [a, low], 2, e.gk)
    e.ctx.synchronize()
    assert e.ctx.memory_in_use() == before


def test_missing_key_is_found_before_anything_is_allocated(env):
    """A key set with steps 1 and 4 but not 2: dim = 8 is FHS_ERR_KEY with memory_in_use unchanged and the output
    list untouched."""
    e = env(256, "b")
    ph = e.ph
    few = e.sk.create_galois_keys(e.ctx, ph.get_elts_from_steps([1, 4], e.N))
    rng = np.random.default_rng(31)
    cts = [e.up(e.rand(rng, 6)) for _ in range(3)]
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    assert _raw(e, cts, 8, 1, few) == (KEY, [_SENTINEL] * 3)
    with pytest.raises(ValueError, match="galois key"):
        ph.inner_sum_many(e.ctx, cts, 8, few)
    assert e.ctx.memory_in_use() == before
    got = ph.inner_sum_many(e.ctx, cts, 2, few)      # step 1 alone is there
    assert np.array_equal(got[0].to_numpy(), e.want(cts[0].to_numpy(), 2))


def test_lost_input_is_rejected(env):
    e = env(256, "a")
    ph = e.ph
    a = e.up(e.rand(np.random.default_rng(32), 3))
    ph.debug_fail_next_flushes(e.ctx, 1)
    r = ph.rotate(e.ctx, a, 1, e.gk)
    with pytest.raises(RuntimeError, match="out of memory"):
        ph.inner_sum_many(e.ctx, [r], 2, e.gk)       # the entry's flush fails: r is lost
    with pytest.raises(ValueError, match="ciphertext lost"):
        ph.inner_sum_many(e.ctx, [a, r], 2, e.gk)
    assert np.array_equal(ph.inner_sum(e.ctx, a, 2, e.gk).to_numpy(), e.want(a.to_numpy(), 2))


@pytest.mark.parametrize("dim,n,allocs", [(1, 1, 1), (2, 1, 1), (2, 3, 1), (8, 1, 2), (8, 4, 2)])
def test_every_allocation_failing_once(env, dim, n, allocs):
    """fhs_debug_fail_alloc at each allocation the call makes once its workspace is warm -- the ping-pong block (two
    steps or more) and the results' block: each is "out of memory", leaves nothing allocated and the output list
    untouched, and the next call succeeds with the same limbs."""
    e = env(512, "a")
    ph = e.ph
    rng = np.random.default_rng(33)
    cts = [e.up(e.rand(rng, 3)) for _ in range(n)]
    want = [g.to_numpy() for g in ph.inner_sum_many(e.ctx, cts, dim, e.gk)]
    gc.collect()
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    for k in range(allocs + 1):
        ph.debug_fail_alloc(e.ctx, k)
        rc, outs = _raw(e, cts, dim, 1, e.gk)
        pending = ph.debug_fail_alloc(e.ctx, -1)
        if k < allocs:
            assert rc == 2 and "out of memory" in ph._lib.fhs_last_error().decode() and not pending, k
            assert outs == [_SENTINEL] * n
            e.ctx.synchronize()
            assert e.ctx.memory_in_use() == before, f"allocation {k} failed: {e.ctx.memory_in_use() - before} bytes left"
        else:
            assert rc == OK and pending, "the call makes more allocations than the sweep walks"
            got = [ph.ciphertext(e.ctx, C.c_void_p(h)) for h in outs]
            assert all(np.array_equal(g.to_numpy(), w) for g, w in zip(got, want))


# ---------------------------------------------------------------------------------------------- nothing else moved
def test_hoisting_and_fused_bsgs_around_an_inner_sum(env):
    """One hoisting call and one fused BSGS at N = 1024, before and after an inner_sum_many on the same context
    (which leaves its items, with the new field set, in the context's item buffer): the oracle's limbs both times."""
    e = env(1024, "b")
    ph, o = e.ph, e.o
    rng = np.random.default_rng(40)
    x = e.rand(rng, 9)
    cx = e.up(x)
    pts = ph.random_plaintexts(e.ctx, 7, 4, 1, SCALE)
    baby_np = [x, o.rotate(x, e.okey(1), 1)]
    want_rot = {st: o.rotate(x, e.okey(st), st) for st in (1, 2, 8)}
    want_bsgs = o.bsgs_loop(baby_np, [p.to_numpy() for p in pts], [None, e.okey(2)], 2, 2, 4)
    for when in ("before", "after"):
        rots = ph.hoisting(e.ctx, cx, e.gk, [1, 2, 8])
        for st, r in zip((1, 2, 8), rots):
            assert np.array_equal(r.to_numpy(), want_rot[st]), (when, st)
        y = ph.bsgs_multiply_accumulate(e.ctx, [cx, rots[0]], pts, 2, 2, 4, e.gk)
        assert np.array_equal(y.to_numpy(), want_bsgs), when
        if when == "before":
            e.check([x, e.rand(rng, 9)], 8, what="between")
