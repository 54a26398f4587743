"""Batched public-key encryption (public_key.encrypt_asymmetric_batch / encode_encrypt_batch: the
sampler, the forward NTTs of u, e0 (+ m), e1 and the combine with pk each launched once over the batch).

The judge is always the CPU oracle: o.encrypt_asymmetric(seed, (1 << 20) + k, o.gen_public_key(seed, s), pt) -- the
counter base of a public key under FHESPEAR_PARITY_RNG=1 -- never the GPU's own single call.  Every comparison is
np.array_equal.  Every test here needs an MI355X: -m gpu."""
import json
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
SCALE = 2.0 ** 40
SEED = 9090
BASE = 1 << 20               # first encryption counter of a public key in the parity mode
MAX_BATCH = 4096             # kMaxBatch: ciphertexts per launch

# N -> (prime sizes, P): one fwd_limb path each
RINGS = {
    256: ([59] * 3, 1),                       # full-limb form, 16 threads
    8192: ([60, 40, 40, 60], 1),              # the retrieval chain: fold1 / lazy off for some limbs
    16384: ([59] * 4, 1),                     # half-limb form, radix-4 first stages
    32768: ([60] * 3 + [59] * 3, 3),          # half-limb form, radix-8 first stages, 1024 threads
    1024: ([59] * 4, 1),                      # counter discipline
}


@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


class Env:
    """One ring: context, oracle, the oracle's secret and public key for SEED.  pk() is a fresh public key of a
    fresh secret key with that seed: its encryption counter starts at BASE."""

    def __init__(self, ph, orc, N, bits, P):
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
        self.s = self.o.gen_secret(SEED)
        self.opk = self.o.gen_public_key(SEED, self.s)
        self.enc = ph.ckks_encoder(self.ctx)

    def pk(self):
        return self.ph.secret_key(self.ctx, seed=SEED).gen_publickey(self.ctx)

    def rand_pt(self, rng, l):
        return np.stack([rng.integers(0, self.primes[i], self.N, dtype=np.uint64) for i in range(l)])

    def up(self, p, scale=SCALE):
        return self.ph.plaintext_from_numpy(self.ctx, p, self.L0 + 1 - p.shape[0], scale)

    def want(self, k, p):
        return self.o.encrypt_asymmetric(SEED, BASE + k, self.opk, p)

    def same(self, ct, k, p, what):
        got = ct.to_numpy()
        want = self.want(k, p)
        assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            i = tuple(int(v) for v in bad[0])
            pytest.fail(f"{what}: {len(bad)} words differ from the oracle at counter base + {k}, first at (component, "
                        f"limb, slot) {i}: got {int(got[i])}, want {int(want[i])}")


_ENVS = {}


@pytest.fixture(scope="module")
def env(ph, orc):
    def get(N, chain=None):
        key = (N, None if chain is None else (tuple(chain[0]), chain[1]))
        if key not in _ENVS:
            bits, P = chain or RINGS[N]
            _ENVS[key] = Env(ph, orc, N, bits, P)
        return _ENVS[key]
    yield get
    _ENVS.clear()


# ---------------------------------------------------------------- per-ring parity
@pytest.mark.parametrize("ci", [1, 2])
@pytest.mark.parametrize("N", [256, 8192, 16384, 32768])
def test_batch_of_three_matches_oracle(env, N, ci):
    """Count 3 of random residues at the top level and at chain_index 2 (l = L0 - 1 < L0: the key's limbs are read at
    stride L0 N)."""
    e = env(N)
    l = e.L0 + 1 - ci
    rng = np.random.default_rng(N + ci)
    ps = [e.rand_pt(rng, l) for _ in range(3)]
    cts = e.pk().encrypt_asymmetric_batch(e.ctx, [e.up(p) for p in ps])
    assert len(cts) == 3
    for k, (ct, p) in enumerate(zip(cts, ps)):
        assert ct.chain_index() == ci and ct.scale() == SCALE and ct.coeff_modulus_size() == l
        e.same(ct, k, p, f"N={N} chain_index={ci} ciphertext {k}")


def test_counters_single_batch_single(env):
    """One key at N = 1024: a single call, a batch of 3, a single call -- the oracle's ciphertexts at counters base + 0
    .. 4, in that order."""
    e = env(1024)
    rng = np.random.default_rng(5)
    ps = [e.rand_pt(rng, e.L0) for _ in range(5)]
    pts = [e.up(p) for p in ps]
    pk = e.pk()
    cts = [pk.encrypt_asymmetric(e.ctx, pts[0])] + pk.encrypt_asymmetric_batch(e.ctx, pts[1:4]) + \
        [pk.encrypt_asymmetric(e.ctx, pts[4])]
    for k, (ct, p) in enumerate(zip(cts, ps)):
        e.same(ct, k, p, f"call sequence 1 + 3 + 1, ciphertext {k}")
    assert pk.encrypt_asymmetric_batch(e.ctx, []) == []
    e.same(pk.encrypt_asymmetric(e.ctx, pts[0]), 5, ps[0], "after an empty batch")


def test_chunk_boundary_4097(env):
    """N = 256, l = 2, count = 4097: two launches (4096 + 1) with consecutive counters; every ciphertext against the
    oracle, indices 0, 4095 and 4096 named."""
    e = env(256)
    count = MAX_BATCH + 1
    rng = np.random.default_rng(4097)
    ps = np.stack([rng.integers(0, e.primes[i], (count, e.N), dtype=np.uint64) for i in range(e.L0)], axis=1)
    cts = e.pk().encrypt_asymmetric_batch(e.ctx, [e.up(p) for p in ps])
    assert len(cts) == count
    for k in (0, MAX_BATCH - 1, MAX_BATCH):
        e.same(cts[k], k, ps[k], f"count 4097, ciphertext {k}")
    for k in range(count):
        assert np.array_equal(cts[k].to_numpy(), e.want(k, ps[k])), f"count 4097, ciphertext {k}"


# ---------------------------------------------------------------- fused encode + encrypt
@pytest.mark.parametrize("N", [8192, 32768])
def test_encode_encrypt_batch_matches_oracle_on_the_encoders_plaintexts(env, N):
    """Real rows (random; period N/8) and complex rows (random; one value in every slot -- the query's form, the
    sparse encoder path): each ciphertext is the oracle's encryption of the GPU encoder's own plaintext of that row
    (the encoder itself is pinned by test_embedding_reference.py)."""
    e = env(N)
    n = N // 2
    rng = np.random.default_rng(N + 11)
    real = np.stack([rng.normal(0, 0.1, n), np.tile(rng.normal(0, 0.1, N // 8), n // (N // 8))])
    cplx = np.stack([rng.normal(0, 0.1, n) + 1j * rng.normal(0, 0.1, n), np.full(n, 0.25 - 0.125j)])
    pk = e.pk()
    k = 0
    for rows, encode, kind in ((real, e.enc.encode_double_vector_batch, "real"),
                               (cplx, e.enc.encode_complex_vector_batch, "complex")):
        cts = pk.encode_encrypt_batch(e.ctx, rows, SCALE)
        pts = encode(e.ctx, rows, SCALE, chain_index=1)
        assert len(cts) == len(rows)
        for r, (ct, pt) in enumerate(zip(cts, pts)):
            assert ct.chain_index() == 1 and ct.scale() == SCALE
            e.same(ct, k, pt.to_numpy(), f"N={N} {kind} row {r}")
            k += 1
    cts = pk.encode_encrypt_batch(e.ctx, real, SCALE, chain_index=2)          # l < L0
    pts = e.enc.encode_double_vector_batch(e.ctx, real, SCALE, chain_index=2)
    for r, (ct, pt) in enumerate(zip(cts, pts)):
        assert ct.chain_index() == 2
        e.same(ct, k + r, pt.to_numpy(), f"N={N} real row {r} at chain_index 2")


# ---------------------------------------------------------------- plaintext kinds
_KINDS = ([59] * 9, 3)       # N = 1024, L0 = 6, P = 3: the ring of test_error_contract.py's compact batches


def test_dense_compact_and_mixed_levels(env):
    """A same-level batch of a dense plaintext and compact ones (periodic rows of encode_double_vector_batch and of
    encode_matrix_diagonals: they reach the kernel through their dense expansion), then a batch over two levels,
    which goes one plaintext at a time with the same counters."""
    e = env(1024, _KINDS)
    ctx, enc = e.ctx, e.enc
    rng = np.random.default_rng(21)
    dense_np = e.rand_pt(rng, e.L0)
    tiled = np.tile(rng.normal(0, 0.1, (4, 16)), (1, (e.N // 2) // 16))
    diag = enc.encode_matrix_diagonals(ctx, rng.normal(0, 0.02, (8, 8)), 4, SCALE)
    comp = enc.encode_double_vector_batch(ctx, tiled, SCALE)
    low = enc.encode_double_vector(ctx, rng.normal(0, 0.1, e.N // 2), SCALE, chain_index=2)
    pk = e.pk()
    batch = [e.up(dense_np), comp[1], diag[3]]
    cts = pk.encrypt_asymmetric_batch(ctx, batch)
    for k, (ct, pt) in enumerate(zip(cts, batch)):
        e.same(ct, k, pt.to_numpy(), f"same level, plaintext {k}")
    mixed = [e.up(dense_np), comp[2], low, diag[5]]
    cts = pk.encrypt_asymmetric_batch(ctx, mixed)
    assert [c.chain_index() for c in cts] == [1, 1, 2, 1]
    for k, (ct, pt) in enumerate(zip(cts, mixed)):
        e.same(ct, 3 + k, pt.to_numpy(), f"two levels, plaintext {k}")
    slab = enc.encode_double_vector_batch(ctx, rng.normal(0, 0.1, (3, e.N // 2)), SCALE)
    for k, ct in enumerate(pk.encrypt_asymmetric_batch(ctx, slab)):       # dense, evenly spaced in one block
        e.same(ct, 7 + k, slab[k].to_numpy(), f"one block of plaintexts, plaintext {k}")
    for k, ct in enumerate(pk.encrypt_asymmetric_batch(ctx, slab[::-1])):  # the same block, not in order
        e.same(ct, 10 + k, slab[2 - k].to_numpy(), f"one block reversed, plaintext {k}")


# ---------------------------------------------------------------- the retrieval run with the public key only
def test_retrieval_with_public_key_batches(ph, orc):
    """The recorded retrieval run (tests/golden/retrieval_manifest.json: N = 512, [60, 40, 40, 60], J = 8, C = 2): the
    database and the query encrypted in ONE encrypt_asymmetric_batch call from the recorded plaintexts.  Each
    ciphertext is the oracle's; dot_product_many gives the limbs of the oracle's op-by-op composition (multiply,
    add, relinearize, rescale: the judge of test_retrieval_dot.py) on the oracle's own public-key ciphertexts; and
    the reference's per-term loop run on these ciphertexts gives the recorded score ciphertexts."""
    man = json.loads((GOLDEN / "retrieval_manifest.json").read_text())
    z = np.load(GOLDEN / man["file"])
    N, J, C, seed = man["N"], man["J"], man["C"], int(z["sk_seed"])
    assert man["pk_enc_counter"] == BASE
    primes = ph.create_coeff_modulus(N, man["bits"])
    parms = ph.params(ph.scheme_type.ckks)
    parms.set_poly_modulus_degree(N)
    parms.set_coeff_modulus(primes)
    parms.set_special_modulus_size(man["P"])
    ctx = ph.context(parms)
    sk = ph.secret_key(ctx, seed=seed)
    pk, rk = sk.gen_publickey(ctx), sk.gen_relinkey(ctx)
    o = orc.Oracle(N, [int(p) for p in primes], man["P"])
    s = o.gen_secret(seed)
    opk, orlk = o.gen_public_key(seed, s), o.gen_relin_key(seed, s)
    cts = pk.encrypt_asymmetric_batch(ctx, [ph.plaintext_from_numpy(ctx, p, 1, man["scale"]) for p in z["pts"]])
    want = [o.encrypt_asymmetric(seed, BASE + k, opk, p) for k, p in enumerate(z["pts"])]
    for k, ct in enumerate(cts):
        assert np.array_equal(ct.to_numpy(), want[k]), f"ciphertext {k}"
    chunks, query = [cts[c * J:(c + 1) * J] for c in range(C)], cts[C * J:]
    outs = ph.dot_product_many(ctx, query, chunks, rk)
    for c in range(C):
        t = None
        for a, b in zip(want[C * J:], want[c * J:(c + 1) * J]):
            m = o.multiply(a, b)
            t = m if t is None else o.add(t, m)
        assert np.array_equal(outs[c].to_numpy(), o.rescale(o.relinearize(t, orlk))), f"fused scores, chunk {c}"
        res = None
        for j in range(J):
            p = ph.rescale_to_next(ctx, ph.relinearize(ctx, ph.multiply(ctx, query[j], chunks[c][j]), rk))
            res = p if res is None else ph.add(ctx, res, p)
        assert np.array_equal(res.to_numpy(), z["scores_ct"][c]), f"per-term loop, chunk {c}"


# ---------------------------------------------------------------- allocation failures
_MAX_STEPS = 64


def _sweep(e, pk, used, op, count):
    """The pattern of test_error_contract._sweep, with ONE key throughout: the unarmed run warms the caches; then
    device allocation k = 0, 1, 2, ... of the call fails.  A raise must be RuntimeError("... out of memory ...") and
    leave memory_in_use unchanged; a return with the hook still pending ends the sweep.  Every call, failed or not,
    has taken `count` counters: op(pk, first) checks a returned batch against the oracle at the counters after all
    earlier calls', so a counter given back by a failed call (a mask stream used twice) fails the comparison.
    Returns (injected failures, counters used)."""
    ph, ctx = e.ph, e.ctx
    op(pk, used)
    used += count
    ctx.synchronize()
    before = ctx.memory_in_use()
    failures = 0
    for k in range(_MAX_STEPS):
        ph.debug_fail_alloc(ctx, k)
        try:
            op(pk, used)
            raised = False
        except RuntimeError as err:
            assert "out of memory" in str(err), (k, str(err))
            raised = True
        used += count
        pending = ph.debug_fail_alloc(ctx, -1)
        if raised:
            assert not pending, f"allocation {k}: an out-of-memory error the hook did not inject"
        elif pending:
            return failures, used
        failures += 1
        ctx.synchronize()
        assert ctx.memory_in_use() == before, f"allocation {k} failed: {ctx.memory_in_use() - before} bytes left behind"
    raise AssertionError(f"sweep did not end within {_MAX_STEPS} steps")


def test_alloc_failures_leave_nothing_and_keep_their_counters(env):
    """Both new calls at N = 1024 with every device allocation failing once: "out of memory", memory_in_use unchanged,
    at least one failure injected per call; afterwards the next batch is the oracle's at the counters the failed calls
    did not give back."""
    e = env(1024, _KINDS)
    ctx = e.ctx
    rng = np.random.default_rng(31)
    ps = [e.rand_pt(rng, e.L0) for _ in range(3)]
    pts = [e.up(p) for p in ps]
    rows = rng.normal(0, 0.1, (3, e.N // 2))
    rows_np = [p.to_numpy() for p in e.enc.encode_double_vector_batch(ctx, rows, SCALE)]
    pk = e.pk()

    def op_batch(pk, first):
        for k, ct in enumerate(pk.encrypt_asymmetric_batch(ctx, pts)):
            e.same(ct, first + k, ps[k], f"encrypt_asymmetric_batch at counters base + {first}..")

    def op_fused(pk, first):
        for k, ct in enumerate(pk.encode_encrypt_batch(ctx, rows, SCALE)):
            e.same(ct, first + k, rows_np[k], f"encode_encrypt_batch at counters base + {first}..")

    used = 0
    for op in (op_batch, op_fused):
        failures, used = _sweep(e, pk, used, op, 3)
        assert failures >= 1, "no allocation failure was injected: the sweep checked nothing"
    op_batch(pk, used)
    op_fused(pk, used + 3)
    e.same(pk.encrypt_asymmetric(ctx, pts[0]), used + 6, ps[0], "single call after the sweeps")
    ctx.synchronize()
