"""Fused CT x CT dot-product scoring (pyPhantom.dot_product_many / fhs_dot_product_many, kernel k_dot_tensor):
the encrypted similarity scores of the reference's EncryptedSimilarityJoins.search (ct_ct_search.py:92-106) with
the tensor products summed before ONE relinearization and ONE rescale per database chunk.

The judge is the CPU oracle's composition multiply / add (3 components) / relinearize / rescale, limb for limb,
on the reference's retrieval modulus set [60, 40, 40, 60] (P = 1; chain "a") and on an all-59-bit chain with
P = 3 (chain "b").  The committed fixture tests/golden/retrieval_ctct_n512.npz (the reference's own search run
on the oracle, tests/golden/make_retrieval_golden.py) is replayed: the per-op loop must reproduce the recorded
score ciphertexts limb for limb, and the fused scores must decode as accurately as the recorded loop did.
Every test here needs an MI355X: -m gpu."""
import ctypes as C
import gc
import json
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
WAVES = 8                     # FHS_DOT_WAVES: waves of a k_dot_tensor workgroup, each owning chunks c = w, w + 8, ...
SCALE = 2.0 ** 40
CHAINS = {"a": (1024, (60, 40, 40, 60), 1), "b": (1024, (59,) * 12, 3)}
SEED = 4242
OK, INVALID, OOM, LEVEL, SCALE_ERR = 0, 1, 2, 4, 5     # fhs_status
_SENTINEL = 0xDEAD0


@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


class Env:
    """GPU context + keys and the oracle with the same keys for one parameter set."""

    def __init__(self, ph, orc, N, bits, P, mode="exact"):
        primes = ph.create_coeff_modulus(N, list(bits))
        parms = ph.params(ph.scheme_type.ckks)
        parms.set_poly_modulus_degree(N)
        parms.set_special_modulus_size(P)
        parms.set_galois_elts([ph.get_elt_from_step(1, N)])
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
        self.rk = self.sk.gen_relinkey(self.ctx)
        self.rlk = self.o.gen_relin_key(SEED, self.o.gen_secret(SEED))

    def rand(self, rng, ncomp, l):
        return np.stack([np.stack([rng.integers(0, self.primes[i], self.N, dtype=np.uint64) for i in range(l)])
                         for _ in range(ncomp)])

    def worst(self, ncomp, l):
        return np.stack([np.stack([np.full(self.N, self.primes[i] - 1, dtype=np.uint64) for i in range(l)])
                         for _ in range(ncomp)])

    def up(self, a, scale=SCALE):
        return self.ph.ciphertext_from_numpy(self.ctx, a, self.L0 + 1 - a.shape[1], scale)

    def want(self, q, chunk, relin=True, rescale=True):
        """The oracle's fused composition for one chunk."""
        t = None
        for a, b in zip(q, chunk):
            m = self.o.multiply(a, b)
            t = m if t is None else self.o.add(t, m)
        if relin:
            t = self.o.relinearize(t, self.rlk)
        return self.o.rescale(t) if rescale else t

    def check(self, q, chunks, relin=True, rescale=True, what=""):
        got = self.ph.dot_product_many(self.ctx, [self.up(a) for a in q], [[self.up(b) for b in row] for row in chunks],
                                       self.rk if relin else None, rescale)
        assert len(got) == len(chunks)
        for c, (g, row) in enumerate(zip(got, chunks)):
            assert np.array_equal(g.to_numpy(), self.want(q, row, relin, rescale)), f"{what} chunk {c}"
        return got


_ENVS = {}


@pytest.fixture(scope="module")
def env(ph, orc):
    def get(chain, mode="exact"):
        key = (chain, mode)
        if key not in _ENVS:
            N, bits, P = CHAINS[chain] if isinstance(chain, str) else chain
            _ENVS[key] = Env(ph, orc, N, bits, P, mode)
        return _ENVS[key]
    yield get
    _ENVS.clear()


CHAIN_LEVELS = [("a", 3), ("a", 2), ("b", 6), ("b", 2)]


@pytest.mark.parametrize("J", [1, 3, 8, 9, 17, 33])
@pytest.mark.parametrize("chain,l", CHAIN_LEVELS)
def test_dot_product_many_matches_oracle(env, chain, l, J):
    """J below one load batch, whole batches, across the Acc3 folds (every 8 or 16 products; s1 twice as often)
    and the Lorentz 65-d vector's 33; one chunk and two."""
    e = env(chain)
    rng = np.random.default_rng(100 * J + l)
    q = [e.rand(rng, 2, l) for _ in range(J)]
    chunks = [[e.rand(rng, 2, l) for _ in range(J)] for _ in range(2)]
    for C in (1, 2):
        e.check(q, chunks[:C], what=f"chain {chain} l={l} J={J} C={C}")


@pytest.mark.parametrize("chain,l", [("a", 3), ("b", 6)])
def test_one_wave_owns_two_chunks(env, chain, l):
    """C = WAVES + 1: wave 0 streams chunks 0 and WAVES, the others one each."""
    e = env(chain)
    rng = np.random.default_rng(9)
    q = [e.rand(rng, 2, l) for _ in range(2)]
    chunks = [[e.rand(rng, 2, l) for _ in range(2)] for _ in range(WAVES + 1)]
    e.check(q, chunks, what=f"chain {chain} C={WAVES + 1}")


def test_more_chunks_than_one_key_switch_batch(env):
    """C = 65: the relinearizations run as two key-switch batches (64 + 1) through one workspace."""
    e = env("a")
    rng = np.random.default_rng(65)
    q = [e.rand(rng, 2, 2)]
    e.check(q, [[e.rand(rng, 2, 2)] for _ in range(65)], what="C=65")


@pytest.mark.parametrize("J", [65, 130])
@pytest.mark.parametrize("chain", ["a", "b"])
def test_windows_accumulate(env, chain, J):
    """J above the 64-term window: further launches add to the reduced sums (one and two extra windows)."""
    e = env(chain)
    rng = np.random.default_rng(J)
    q = [e.rand(rng, 2, 2) for _ in range(J)]
    chunks = [[e.rand(rng, 2, 2) for _ in range(J)] for _ in range(2)]
    e.check(q, chunks, what=f"chain {chain} J={J}")


@pytest.mark.parametrize("J", [64, 65])
@pytest.mark.parametrize("chain,l", [("a", 3), ("b", 6)])
def test_worst_case_operands(env, chain, l, J):
    """Every residue q_i - 1: the largest partial products and 128-bit sums (a full window, and one term more)."""
    e = env(chain)
    w = e.worst(2, l)
    e.check([w] * J, [[w] * J], what=f"chain {chain} worst case J={J}")


@pytest.mark.parametrize("relin", [False, True])
@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("chain,l", [("a", 3), ("b", 6)])
def test_flag_combinations(env, chain, l, relin, rescale):
    e = env(chain)
    rng = np.random.default_rng(31)
    q = [e.rand(rng, 2, l) for _ in range(3)]
    chunks = [[e.rand(rng, 2, l) for _ in range(3)] for _ in range(2)]
    got = e.check(q, chunks, relin, rescale, what=f"relin={relin} rescale={rescale}")
    ci = e.L0 + 1 - l
    for g in got:
        assert g.size() == (2 if relin else 3)
        assert g.chain_index() == (ci + 1 if rescale else ci)
        assert g.coeff_modulus_size() == (l - 1 if rescale else l)
        assert g.scale() == (SCALE * SCALE / e.primes[l - 1] if rescale else SCALE * SCALE)


def test_seal_key_switch_mode(env):
    """The relinearization honours the context's SEAL convention (P = 1), as fhs_relinearize does."""
    e = env("a", "seal")
    assert e.ctx.key_switch_mode() == "seal"
    rng = np.random.default_rng(77)
    for l in (3, 2):
        q = [e.rand(rng, 2, l) for _ in range(3)]
        chunks = [[e.rand(rng, 2, l) for _ in range(3)] for _ in range(2)]
        e.check(q, chunks, what=f"seal l={l}")
    exact = env("a")                      # the two conventions give different limbs: the mode was really taken
    a = [exact.up(x) for x in q]
    b = [[exact.up(x) for x in row] for row in chunks]
    other = exact.ph.dot_product_many(exact.ctx, a, b, exact.rk)
    assert not np.array_equal(other[0].to_numpy(), e.want(q, chunks[0]))


def test_largest_ring(env):
    """N = 32768 (three 59-bit primes + P = 1): the key switch and the rescale take their half-limb forms."""
    e = env((32768, (59,) * 4, 1))
    rng = np.random.default_rng(5)
    q = [e.rand(rng, 2, 3) for _ in range(2)]
    e.check(q, [[e.rand(rng, 2, 3) for _ in range(2)]], what="N=32768")


def test_workload_shape_equals_the_engines_own_ops(env):
    """N = 8192, the retrieval chain, J = 32 (64-d embeddings), C = 3 (10 000 docs): the fused call equals the GPU's
    own multiply / add / relinearize / rescale_to_next composition limb for limb (a self-comparison at the
    demo's shape, next to the oracle cases above)."""
    e = env((8192, (60, 40, 40, 60), 1))
    ph, ctx = e.ph, e.ctx
    rng = np.random.default_rng(8192)
    J, C = 32, 3
    q = [e.up(e.rand(rng, 2, 3)) for _ in range(J)]
    chunks = [[e.up(e.rand(rng, 2, 3)) for _ in range(J)] for _ in range(C)]
    got = ph.dot_product_many(ctx, q, chunks, e.rk)
    for c in range(C):
        t = ph.multiply(ctx, q[0], chunks[c][0])
        for j in range(1, J):
            t = ph.add(ctx, t, ph.multiply(ctx, q[j], chunks[c][j]))
        want = ph.rescale_to_next(ctx, ph.relinearize(ctx, t, e.rk))
        assert np.array_equal(got[c].to_numpy(), want.to_numpy()), f"chunk {c}"
        assert got[c].chain_index() == want.chain_index() and got[c].scale() == want.scale()


def test_dot_product_plain_many_matches_oracle(env):
    """CT-PT scores (fc:112-147) through the BSGS Hadamard: multiply_plain / add / rescale in the oracle."""
    e = env("a")
    rng = np.random.default_rng(13)
    J, C, l = 3, 2, 3
    q = [e.rand(rng, 2, l) for _ in range(J)]
    pts = [[e.rand(rng, 1, l)[0] for _ in range(J)] for _ in range(C)]
    up_pts = [[e.ph.plaintext_from_numpy(e.ctx, p, 1, SCALE) for p in row] for row in pts]
    for rescale in (True, False):
        got = e.ph.dot_product_plain_many(e.ctx, [e.up(a) for a in q], up_pts, rescale=rescale)
        for c in range(C):
            t = None
            for a, p in zip(q, pts[c]):
                m = e.o.multiply_plain(a, p)
                t = m if t is None else e.o.add(t, m)
            assert np.array_equal(got[c].to_numpy(), e.o.rescale(t) if rescale else t)
            assert got[c].scale() == (SCALE * SCALE / e.primes[l - 1] if rescale else SCALE * SCALE)
    with pytest.raises(ValueError, match="ragged"):
        e.ph.dot_product_plain_many(e.ctx, [e.up(a) for a in q], [up_pts[0], up_pts[1][:2]])


def test_error_contract(env):
    """Bad arguments raise ValueError with the messages the single ops give, nothing is allocated and the
    context keeps working."""
    e = env("a")
    ph, ctx = e.ph, e.ctx
    rng = np.random.default_rng(3)
    q = [e.up(e.rand(rng, 2, 3)) for _ in range(2)]
    row = [e.up(e.rand(rng, 2, 3)) for _ in range(2)]
    low, three = e.up(e.rand(rng, 2, 2)), e.up(e.rand(rng, 3, 3))
    other_scale = e.up(e.rand(rng, 2, 3), 2.0 ** 30)
    last = [e.up(e.rand(rng, 2, 1)) for _ in range(4)]
    ph.dot_product_many(ctx, q, [row], e.rk)        # warm: the scratch buffers exist before the baseline
    ctx.synchronize()
    before = ctx.memory_in_use()
    with pytest.raises(ValueError, match="at least one"):
        ph.dot_product_many(ctx, [], [[]], e.rk)                                    # J = 0
    with pytest.raises(ValueError, match="at least one"):
        ph.dot_product_many(ctx, q, [], e.rk)                                       # C = 0
    with pytest.raises(ValueError, match="ragged"):
        ph.dot_product_many(ctx, q, [row, row[:1]], e.rk)
    with pytest.raises(ValueError, match="different chain indices"):
        ph.dot_product_many(ctx, q, [[row[0], low]], e.rk)
    with pytest.raises(ValueError, match="2-component"):
        ph.dot_product_many(ctx, q, [[row[0], three]], e.rk)
    with pytest.raises(ValueError, match="scale mismatch"):
        ph.dot_product_many(ctx, q, [[row[0], other_scale]], e.rk)
    with pytest.raises(ValueError, match="scale mismatch"):
        ph.dot_product_many(ctx, [q[0], other_scale], [row], e.rk)
    with pytest.raises(ValueError, match="too many"):
        ph.dot_product_many(ctx, q[:1], [row[:1]] * 21846, e.rk)                   # 3 C components > one launch's grid
    with pytest.raises(ValueError, match="no level left"):
        ph.dot_product_many(ctx, last[:2], [last[2:]], e.rk)                       # rescale at l = 1
    ctx.synchronize()
    assert ctx.memory_in_use() == before            # every operand above is still alive: nothing new is held
    assert ph.dot_product_many(ctx, last[:2], [last[2:]], e.rk, rescale=False)[0].chain_index() == 3
    a = [e.rand(rng, 2, 3) for _ in range(2)]
    e.check(a, [[e.rand(rng, 2, 3) for _ in range(2)]], what="after the failures")


def _raw(e, q, chunks, rk, rescale):
    """The C call itself: (status, the output array as Python ints), the array pre-filled with a sentinel."""
    J, Cn = len(q), len(chunks)
    qq = (C.c_void_p * J)(*[c._h for c in q])
    dd = (C.c_void_p * (J * Cn))(*[c._h for row in chunks for c in row])
    out = (C.c_void_p * Cn)(*([_SENTINEL] * Cn))
    rc = e.ph._lib.fhs_dot_product_many(e.ctx._h, qq, J, dd, Cn, rk._h if rk is not None else None, rescale, out)
    return rc, [int(v or 0) for v in out]


@pytest.mark.parametrize("Cn", [1, 2])
@pytest.mark.parametrize("relin,rescale", [(True, 1), (False, 0)])
def test_every_allocation_failing_once(env, Cn, relin, rescale):
    """fhs_debug_fail_alloc at each of the first 16 allocations of a warm call (J = 2): a failing call is "out of
    memory", leaves nothing allocated and every slot of `outs` as it was (include/fhespear.h: on failure outs is
    untouched); a call the armed failure does not reach gives the oracle's limbs.  At least one k fails."""
    e = env("a")
    ph = e.ph
    rng = np.random.default_rng(410 + Cn)
    q = [e.rand(rng, 2, 3) for _ in range(2)]
    rows = [[e.rand(rng, 2, 3) for _ in range(2)] for _ in range(Cn)]
    Q, D = [e.up(a) for a in q], [[e.up(b) for b in row] for row in rows]
    rk = e.rk if relin else None
    want = [e.want(q, row, relin, bool(rescale)) for row in rows]
    warm = ph.dot_product_many(e.ctx, Q, D, rk, bool(rescale))
    assert all(np.array_equal(g.to_numpy(), w) for g, w in zip(warm, want))
    del warm
    gc.collect()
    e.ctx.synchronize()
    before = e.ctx.memory_in_use()
    failed = 0
    for k in range(16):
        ph.debug_fail_alloc(e.ctx, k)
        rc, outs = _raw(e, Q, D, rk, rescale)
        pending = ph.debug_fail_alloc(e.ctx, -1)
        if rc != OK:
            failed += 1
            assert rc == OOM and "out of memory" in ph._lib.fhs_last_error().decode() and not pending, k
            assert outs == [_SENTINEL] * Cn, k
            e.ctx.synchronize()
            assert e.ctx.memory_in_use() == before, f"allocation {k} failed: {e.ctx.memory_in_use() - before} bytes left"
            rc, outs = _raw(e, Q, D, rk, rescale)        # the next call
        assert rc == OK and _SENTINEL not in outs, k
        got = [ph.ciphertext(e.ctx, C.c_void_p(h)) for h in outs]
        assert all(np.array_equal(g.to_numpy(), w) for g, w in zip(got, want)), k
        del got
        gc.collect()
    assert failed >= 1, "a warm call allocates its results' block at least"


def test_argument_errors_leave_outs_untouched(env):
    """The raw call with a 3-component input, a chain-index mismatch and a scale mismatch: the status codes behind
    test_error_contract's messages, and `outs` still holds the sentinel in every slot."""
    e = env("a")
    rng = np.random.default_rng(4)
    q = [e.up(e.rand(rng, 2, 3)) for _ in range(2)]
    row = [e.up(e.rand(rng, 2, 3)) for _ in range(2)]
    low, three = e.up(e.rand(rng, 2, 2)), e.up(e.rand(rng, 3, 3))
    other_scale = e.up(e.rand(rng, 2, 3), 2.0 ** 30)
    err = lambda: e.ph._lib.fhs_last_error().decode()   # noqa: E731
    for bad, code, word in [(three, INVALID, "2-component"), (low, LEVEL, "different chain indices"),
                            (other_scale, SCALE_ERR, "scale mismatch")]:
        for rk, rescale in [(e.rk, 1), (None, 0)]:
            assert _raw(e, q, [row, [row[0], bad]], rk, rescale) == (code, [_SENTINEL] * 2) and word in err(), word
    assert _raw(e, [q[0], other_scale], [row], e.rk, 1) == (SCALE_ERR, [_SENTINEL]) and "scale mismatch" in err()
    rc, outs = _raw(e, q, [row], e.rk, 1)
    assert rc == OK and outs != [_SENTINEL]
    e.ph.ciphertext(e.ctx, C.c_void_p(outs[0]))          # owned, so destroyed


# ---------------------------------------------------------------- the reference's search, replayed
@pytest.fixture(scope="module")
def replay(ph):
    man = json.loads((GOLDEN / "retrieval_manifest.json").read_text())
    z = np.load(GOLDEN / man["file"])
    N, J, C = man["N"], man["J"], man["C"]
    primes = ph.create_coeff_modulus(N, man["bits"])
    assert [int(p) for p in primes] == [int(p) for p in z["primes"]]
    parms = ph.params(ph.scheme_type.ckks)
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(primes)
    parms.set_special_modulus_size(man["P"])
    ctx = ph.context(parms)
    sk = ph.secret_key(ctx, seed=int(z["sk_seed"]))
    pk = sk.gen_publickey(ctx)
    rk = sk.gen_relinkey(ctx)
    cts = [pk.encrypt_asymmetric(ctx, ph.plaintext_from_numpy(ctx, p, 1, man["scale"])) for p in z["pts"]]
    chunks = [cts[c * J:(c + 1) * J] for c in range(C)]
    return dict(ph=ph, ctx=ctx, sk=sk, rk=rk, z=z, man=man, chunks=chunks, query=cts[C * J:], J=J, C=C)


def test_fixture_per_op_loop_reproduces_the_reference_limbs(replay):
    """ct_ct_search.py:92-106 op for op on the GPU (multiply, relinearize, rescale per term, then add) on the
    reference's own modulus set [60, 40, 40, 60], from the recorded plaintexts encrypted under the seeded public
    key: the recorded score ciphertexts, limb for limb."""
    r = replay
    ph, ctx, q = r["ph"], r["ctx"], r["query"]
    for c, chunk in enumerate(r["chunks"]):
        res = None
        for j in range(r["J"]):
            p = ph.rescale_to_next(ctx, ph.relinearize(ctx, ph.multiply(ctx, q[j], chunk[j]), r["rk"]))
            res = p if res is None else ph.add(ctx, res, p)
        assert res.chain_index() == r["man"]["chain_index_out"] and res.scale() == r["man"]["scale_out"]
        assert np.array_equal(res.to_numpy(), r["z"]["scores_ct"][c]), f"chunk {c}"


def test_fixture_fused_scores_are_as_accurate_as_the_loop(replay):
    """The fused scores, decrypted and decoded, within 2 x the recorded loop's error of float64 docs @ q (the
    fused error measured on the oracle was 0.95 x the loop's; the factor 2 allows for another noise sample), and
    the same top-10."""
    r = replay
    ph, ctx, z = r["ph"], r["ctx"], r["z"]
    outs = ph.dot_product_many(ctx, r["query"], r["chunks"], r["rk"])
    assert [o.chain_index() for o in outs] == [r["man"]["chain_index_out"]] * r["C"]
    enc = ph.ckks_encoder(ctx)
    n_docs = len(z["docs"])
    scores = np.concatenate([np.real(enc.decode_complex_vector(ctx, r["sk"].decrypt(ctx, o))) for o in outs])[:n_docs]
    exact = z["docs"] @ z["query"]
    err, bound = float(np.max(np.abs(scores - exact))), 2.0 * float(z["max_err_loop"])
    print(f"fused max|score - docs@q| = {err:.3e}; recorded loop {float(z['max_err_loop']):.3e}; bound {bound:.3e}")
    assert err <= bound
    assert list(np.argsort(-scores)[:10]) == list(np.argsort(-exact)[:10])
