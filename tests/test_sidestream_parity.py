"""The giant steps' side stream and the balanced block maps against the CPU oracle, limb for limb (np.array_equal).

Large giant-step launches run the special limbs' chain beside ModUp of the data limbs on a second stream (DESIGN.md
section 3); the launcher forks by the size of that ModUp, which no quick test reaches, so every ring here runs twice:
as the library decides (single stream at these sizes) and with pyPhantom.debug_force_fork, which makes every
giant-step launch at N >= 512 take the forked form.  Key switches of queued rotations and relinearisations stay on
one stream either way.  Rings: N = 256 (full-limb kernels, one 256-slot block
per limb: never forks), N = 512 (two blocks per limb: the half-limb maps), N = 1024 on nine 59-bit primes with P = 3
at l = 6, 5 and 3 (E = 9, 8, 6 extended limbs: above, at and below the maps' group of 8), and five 59-bit primes
with P = 1 in SEAL's convention (the hoisted path and its zero-digit fallback).  Every test needs an MI355X: -m gpu."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, SCALE = 4177, 2.0 ** 40
G = 3
ROT3 = [1, 2, 3]
STEPS = sorted(set(ROT3 + list(range(1, G)) + [g * G for g in range(1, 5)]))

# (N, L0, P, l, seal)
RINGS = {
    "n256": (256, 6, 3, 6, False),
    "n512": (512, 6, 3, 6, False),
    "n1024_l6": (1024, 6, 3, 6, False),
    "n1024_l5": (1024, 6, 3, 5, False),
    "n1024_l3": (1024, 6, 3, 3, False),
    "seal_p1": (1024, 4, 1, 4, True),
}


@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


class Env:
    """One ring: context, keys, the oracle with its keys, and the expected limbs of every call, computed once."""

    def __init__(self, ph, orc, N, L0, P, l, seal):
        self.ph, self.N, self.L0, self.P, self.l, self.seal = ph, N, L0, P, l, seal
        self.ci = L0 + 1 - l
        self.elts = {st: ph.get_elt_from_step(st, N) for st in STEPS}
        self.primes = [int(q) for q in ph.create_coeff_modulus(N, [59] * (L0 + P))]
        self.o = orc.Oracle(N, self.primes, P)
        if seal:
            self.o.set_key_switch_mode("seal")
        self.s = self.o.gen_secret(SEED)
        self.okeys = {st: self.o.gen_galois_key(SEED, self.s, e) for st, e in self.elts.items()}
        self.orlk = self.o.gen_relin_key(SEED, self.s)
        rng = np.random.default_rng(N + 16 * l + P)
        self.inputs = [self.rand(rng, 2) for _ in range(9)]
        self.c3 = self.rand(rng, 3)
        self.want_rot = {(i, st): self.o.rotate_elt(self.inputs[i], self.okeys[st], self.elts[st])
                         for i in range(9) for st in (ROT3 if i < 2 else [1])}
        self.want_relin = self.o.relinearize(self.c3, self.orlk)
        self._bsgs = {}
        self.ctx, self.sk, self.gk, self.rlk = self.make_ctx()

    def make_ctx(self):
        ph = self.ph
        parms = ph.params(ph.scheme_type.ckks)
        parms.set_poly_modulus_degree(self.N)
        parms.set_special_modulus_size(self.P)
        parms.set_galois_elts(sorted(set(self.elts.values())))
        parms.set_coeff_modulus(self.primes)
        ctx = ph.context(parms)
        if self.seal:
            ctx.set_key_switch_mode("seal")
        sk = ph.secret_key(ctx, seed=SEED)
        return ctx, sk, sk.create_galois_keys(ctx), sk.gen_relinkey(ctx)

    def rand(self, rng, ncomp):
        return np.stack([np.stack([rng.integers(0, self.primes[i], self.N, dtype=np.uint64) for i in range(self.l)])
                         for _ in range(ncomp)])

    def up(self, a, ctx=None):
        return self.ph.ciphertext_from_numpy(ctx or self.ctx, a, self.ci, SCALE)

    def baby_want(self, i):
        return [self.inputs[i]] + [self.want_rot[(i, b)] for b in range(1, G)]

    def bsgs_want(self, i, B, pts_np):
        key = (i, B)
        if key not in self._bsgs:
            gkeys = [None] + [self.okeys[g * G] for g in range(1, B)]
            self._bsgs[key] = self.o.bsgs_loop(self.baby_want(i), pts_np, gkeys, G, B, G * B)
        return self._bsgs[key]

    def bsgs(self, i, B, ctx=None, gk=None):
        """(result, expected limbs): baby rotations queued, then the fused BSGS, on input i"""
        ph, ctx, gk = self.ph, ctx or self.ctx, gk or self.gk
        A = self.up(self.inputs[i], ctx)
        baby = [A] + [ph.rotate(ctx, A, b, gk) for b in range(1, G)]
        pts = ph.random_plaintexts(ctx, 100 + B, G * B, self.ci, SCALE)
        y = ph.bsgs_multiply_accumulate(ctx, baby, pts, G, B, G * B, gk)
        return y, self.bsgs_want(i, B, [p.to_numpy() for p in pts])


_ENVS = {}


@pytest.fixture
def env(ph, orc):
    def get(name):
        if name not in _ENVS:
            _ENVS[name] = Env(ph, orc, *RINGS[name])
        return _ENVS[name]
    yield get
    for e in _ENVS.values():
        ph.debug_force_fork(e.ctx, False)


def _forks(e):
    return e.N >= 512


@pytest.mark.parametrize("fork", [False, True], ids=["auto", "forked"])
@pytest.mark.parametrize("ring", list(RINGS))
def test_calls_match_oracle(env, ring, fork):
    """A queued batch of 3 rotations of one input, a queued batch of 9 distinct inputs, the fused BSGS with G = 3 and
    B = 2, 3, 5, and one relinearisation.  Forced, every giant-step launch at N >= 512 forks (the counter moves with
    each) and nothing else does; as the library decides, nothing this small does."""
    e = env(ring)
    ph, ctx = e.ph, e.ctx
    ph.debug_force_fork(ctx, fork)
    n0 = ph.debug_force_fork(ctx)
    A = e.up(e.inputs[0])
    outs = [ph.rotate(ctx, A, st, e.gk) for st in ROT3]
    for st, r in zip(ROT3, outs):
        assert np.array_equal(r.to_numpy(), e.want_rot[(0, st)]), f"3 rotations of one input: step {st}"
    n1 = ph.debug_force_fork(ctx)
    assert n1 == n0, "a key switch of queued rotations stays on one stream"
    ins = [e.up(a) for a in e.inputs]
    outs = [ph.rotate(ctx, c, 1, e.gk) for c in ins]
    for i, r in enumerate(outs):
        assert np.array_equal(r.to_numpy(), e.want_rot[(i, 1)]), f"9 distinct inputs: input {i}"
    n2 = ph.debug_force_fork(ctx)
    assert n2 == n1
    for B in (2, 3, 5):
        y, want = e.bsgs(0, B)
        assert np.array_equal(y.to_numpy(), want), f"fused BSGS G = {G}, B = {B}"
    n3 = ph.debug_force_fork(ctx)
    assert n3 - n2 == (3 if fork and _forks(e) else 0), "one per giant-step launch"
    got = ph.relinearize(ctx, e.up(e.c3), e.rlk).to_numpy()
    assert np.array_equal(got, e.want_relin)
    assert ph.debug_force_fork(ctx) == n3


@pytest.mark.parametrize("fork", [False, True], ids=["auto", "forked"])
def test_seal_hoisted_and_zero_digit_fallback(env, fork):
    """SEAL's convention, P = 1: rotations of one input take the hoisted path (the first call of the ring's test above
    too); a digit coefficient that is exactly 0 sends the flush down SEAL's per-rotation path, which re-enters the
    key switch after the flag has been read.  Both are the oracle's limbs, and neither forks."""
    e = env("seal_p1")
    ph, ctx, o = e.ph, e.ctx, e.o
    ph.debug_force_fork(ctx, fork)
    c = e.inputs[0].copy()
    e1 = e.elts[1]
    neg = [i for i in range(e.N) if (i * e1) % (2 * e.N) >= e.N]
    for limb, i in ((0, neg[5]), (e.l - 1, neg[-3])):
        coef = np.array(o.intt(c[1, limb], limb), dtype=np.uint64)
        coef[i] = 0
        c[1, limb] = o.ntt(coef, limb)
    for a, path in ((c, 1), (e.inputs[0], 0)):
        h0, n0 = ctx.seal_hoist_stats(), ph.debug_force_fork(ctx)
        rots = ph.hoisting(ctx, e.up(a), e.gk, ROT3)
        for st, r in zip(ROT3, rots):
            assert np.array_equal(r.to_numpy(), o.rotate_elt(a, e.okeys[st], e.elts[st])), (path, st)
        h1 = ctx.seal_hoist_stats()
        assert h1[path] == h0[path] + 1 and h1[1 - path] == h0[1 - path]
        assert ph.debug_force_fork(ctx) == n0


@pytest.mark.parametrize("fork", [False, True], ids=["auto", "forked"])
def test_back_to_back_iterations_without_synchronisation(env, fork):
    """20 iterations of {3 queued rotations, fused BSGS} on one context, inputs alternating so that consecutive
    iterations' limbs differ, nothing read back or synchronised in between: every iteration reuses the key-switch
    workspace the iteration before may still be working in on the side stream.  Every output is compared."""
    e = env("n512")
    ph, ctx = e.ph, e.ctx
    ph.debug_force_fork(ctx, fork)
    n0 = ph.debug_force_fork(ctx)
    kept = []
    for it in range(20):
        i = it & 1
        A = e.up(e.inputs[i])
        rots = [ph.rotate(ctx, A, st, e.gk) for st in ROT3]
        y, want = e.bsgs(i, 3)
        kept.append((i, rots, y, want))
    for it, (i, rots, y, want) in enumerate(kept):
        for st, r in zip(ROT3, rots):
            assert np.array_equal(r.to_numpy(), e.want_rot[(i, st)]), f"iteration {it}, rotation {st}"
        assert np.array_equal(y.to_numpy(), want), f"iteration {it}, BSGS"
    assert ph.debug_force_fork(ctx) - n0 == (20 if fork else 0), "one giant-step launch per iteration"


def test_context_destroyed_right_after_its_last_call(env):
    """A context of its own, forked launches, destroyed with the last call's work still queued on both streams;
    the ring's shared context then still gives the oracle's limbs."""
    e = env("n512")
    ph = e.ph
    ctx, sk, gk, rlk = e.make_ctx()
    ph.debug_force_fork(ctx, True)
    y, want = e.bsgs(1, 5, ctx, gk)
    assert ph.debug_force_fork(ctx) == 1
    del y, sk, gk, rlk, ctx
    gc.collect()
    y, want = e.bsgs(1, 5)
    assert np.array_equal(y.to_numpy(), want)


@pytest.mark.parametrize("fork", [False, True], ids=["auto", "forked"])
def test_failed_flush_then_good_call(env, fork):
    """One flush fails before launching (debug_fail_next_flushes); the next calls' limbs -- queued rotations, then a
    fused BSGS -- are the oracle's and memory_in_use is back where it was once their results are released."""
    e = env("n512")
    ph, ctx = e.ph, e.ctx
    ph.debug_force_fork(ctx, fork)
    A = e.up(e.inputs[0])
    warm = [ph.rotate(ctx, A, st, e.gk) for st in ROT3]
    assert np.array_equal(warm[0].to_numpy(), e.want_rot[(0, 1)])
    y, want = e.bsgs(0, 3)
    assert np.array_equal(y.to_numpy(), want)
    del warm, y
    ctx.synchronize()
    before = ctx.memory_in_use()
    lost = [ph.rotate(ctx, A, st, e.gk) for st in ROT3]
    ph.debug_fail_next_flushes(ctx, 1)
    with pytest.raises(RuntimeError, match="out of memory"):
        ph.add(ctx, A, A)
    with pytest.raises(ValueError, match="lost"):
        lost[0].to_numpy()
    del lost
    good = [ph.rotate(ctx, A, st, e.gk) for st in ROT3]
    for st, r in zip(ROT3, good):
        assert np.array_equal(r.to_numpy(), e.want_rot[(0, st)]), f"after the failed flush: step {st}"
    y, want = e.bsgs(0, 3)
    assert np.array_equal(y.to_numpy(), want), "fused BSGS after the failed flush"
    del good, r, y
    ctx.synchronize()
    assert ctx.memory_in_use() == before
