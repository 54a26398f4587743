"""Error contract the reference relies on: device OOM surfaces as RuntimeError whose
text contains "out of memory" (bg:1164-1166 falls back to on-the-fly encoding on it), a failed
batch leaves no HBM behind, and a process holding more than 100 GB of cached device
blocks exits cleanly (round-1 exit-handler crash)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


def _ctx(ph, N=16384, L0=36, P=3):
    parms = ph.params(ph.scheme_type.ckks)
    parms.set_poly_modulus_degree(N)
    parms.set_special_modulus_size(P)
    parms.set_galois_elts([ph.get_elt_from_step(1, N)])
    parms.set_coeff_modulus(ph.create_coeff_modulus(N, [59] * (L0 + P)))
    return ph.context(parms)


@pytest.mark.gpu
def test_oom_in_batch_is_runtime_error_and_frees_partial_batch(ph):
    """random_plaintexts of more plaintexts than HBM holds (4.72 MB each at N = 16384, L0 = 36:
    70000 = 330 GB > 288 GB): RuntimeError("... out of memory ..."), every plaintext the batch had
    already created is released, and the context keeps working."""
    ctx = _ctx(ph)
    before = ctx.memory_in_use()
    with pytest.raises(RuntimeError, match="out of memory"):
        ph.random_plaintexts(ctx, 3, 70000, 1, 2.0 ** 59)
    ctx.synchronize()
    assert ctx.memory_in_use() == before
    pts = ph.random_plaintexts(ctx, 4, 8, 1, 2.0 ** 59)     # the context still allocates
    assert len(pts) == 8 and pts[0].coeff_modulus_size() == 36


@pytest.mark.gpu
def test_oom_in_batch_encode_with_hbm_held_elsewhere(ph):
    """The reference's pre-encoding loop (bg:1124-1170) hits OOM inside encode_double_vector_batch
    when another allocation holds the HBM: same exception text, nothing left allocated."""
    import torch
    ctx = _ctx(ph)
    enc = ph.ckks_encoder(ctx)
    before = ctx.memory_in_use()
    free, _ = torch.cuda.mem_get_info(0)
    hold = torch.empty(int(free) - (3 << 30), dtype=torch.uint8, device="cuda:0")   # leave ~3 GB
    try:
        rows = np.random.default_rng(0).normal(0, 0.02, (1024, 8192))     # 1024 x 4.72 MB = 4.8 GB
        with pytest.raises(RuntimeError, match="out of memory"):
            enc.encode_double_vector_batch(ctx, rows, 2.0 ** 59, chain_index=1)
        ctx.synchronize()
        assert ctx.memory_in_use() == before
    finally:
        del hold
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_exit_with_100gb_cache_returns_zero(require_gpu):
    """The round-1 crash: a 13-block d = 2048 FFN chain (bootstrapped) with the device-block cache uncapped
    (FHESPEAR_CACHE_BYTES = 200 GB) segfaulted in the HIP runtime's exit handler.  Each context now
    owns its memory pool, destroyed with the context and trimmed by an atexit hook that runs before
    the runtime's; the process must exit with status 0."""
    env = dict(os.environ, FHESPEAR_DEVICE="0", FHESPEAR_CACHE_BYTES=str(200 * 10 ** 9))
    cmd = [sys.executable, "-X", "faulthandler", str(REPO / "tools" / "ffn_block.py"), "--N", "16384", "--L0", "36",
           "--P", "3", "--D", "2048", "--F", "4096", "--blocks", "13", "--bootstrap"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, f"rc {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_failed_flush_drops_the_queue_and_marks_its_outputs_lost(ph):
    """The round-5 world-8 rehearsal's rank-0 abort (gpurun_out/r05l): a flush of queued rotations failed out of
    memory in its workspace, the queue kept its pointers, the caller destroyed the objects (their blocks went back
    to the device when the cache was trimmed) and a later flush launched the key switch on freed memory -- an
    illegal address at exit.  Now a failed flush empties the queue: the error surfaces as RuntimeError("... out of
    memory ..."), the queued outputs are marked lost (every later use raises instead of reading undefined limbs),
    destroying the inputs launches nothing, and the context keeps working (bit-exact rotations afterwards)."""
    from oracle.oracle import Oracle
    N, L0, P = 4096, 6, 3
    parms = ph.params(ph.scheme_type.ckks)
    parms.set_poly_modulus_degree(N)
    parms.set_special_modulus_size(P)
    parms.set_galois_elts(sorted(set(ph.get_elts_from_steps([1, 2], N))))
    primes = ph.create_coeff_modulus(N, [59] * (L0 + P))
    parms.set_coeff_modulus(primes)
    ctx = ph.context(parms)
    sk = ph.secret_key(ctx, seed=5)
    gk = sk.create_galois_keys(ctx)
    o = Oracle(N, [int(q) for q in primes], P)
    s = o.gen_secret(5)
    rng = np.random.default_rng(2)
    a = np.stack([np.stack([rng.integers(0, int(primes[i]), N, dtype=np.uint64) for i in range(L0)]) for _ in range(2)])
    ct = ph.ciphertext_from_numpy(ctx, a, 1, 2.0 ** 40)
    r1, r2 = ph.rotate(ctx, ct, 1, gk), ph.rotate(ctx, ct, 2, gk)     # queued, not yet launched
    ph.debug_fail_next_flushes(ctx, 1)
    with pytest.raises(RuntimeError, match="out of memory"):
        ph.add(ctx, ct, ct)                                              # its entry flushes the queue: fails
    del ct                                                               # nothing queued references it now
    ctx.synchronize()
    for r in (r1, r2):
        with pytest.raises(ValueError, match="lost"):
            r.to_numpy()
        with pytest.raises(ValueError, match="lost"):
            ph.add(ctx, r, r)
    del r1, r2
    ct = ph.ciphertext_from_numpy(ctx, a, 1, 2.0 ** 40)
    e = ph.get_elt_from_step(1, N)
    assert np.array_equal(ph.rotate(ctx, ct, 1, gk).to_numpy(), o.rotate_elt(a, o.gen_galois_key(5, s, e), e))
    ctx.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# Allocation-failure sweep: every device allocation of every entry point fails once (debug_fail_alloc), and each
# failure must leave memory_in_use exactly where it was -- the temporaries of the call, its half-made result and
# the context reference that result holds are all released.  Host logic only, so the smallest ring of the smoke
# check: N = 1024, nine 59-bit primes (L0 = 6, P = 3), Galois keys for steps 1, 2 and 4.
_N, _L0, _P, _SEED, _SC = 1024, 6, 3, 77, 2.0 ** 40
_MAX_STEPS = 64


class _Small:
    """Context, keys and fixed seeded operands shared by the sweeps (built once; never modified)."""

    def __init__(self, ph):
        from oracle.oracle import Oracle
        N = _N
        self.ph = ph
        parms = ph.params(ph.scheme_type.ckks)
        parms.set_poly_modulus_degree(N)
        parms.set_special_modulus_size(_P)
        parms.set_galois_elts(sorted(set(ph.get_elts_from_steps([1, 2, 4], N))))
        self.primes = [int(q) for q in ph.create_coeff_modulus(N, [59] * (_L0 + _P))]
        parms.set_coeff_modulus(self.primes)
        self.ctx = ctx = ph.context(parms)
        self.oracle = Oracle(N, self.primes, _P)
        self.enc = enc = ph.ckks_encoder(ctx)
        self.sk = sk = ph.secret_key(ctx, seed=_SEED)
        self.gk = sk.create_galois_keys(ctx)
        self.rk = sk.gen_relinkey(ctx)
        rng = np.random.default_rng(11)
        self.x = rng.normal(0, 0.1, N // 2)
        self.z = rng.normal(0, 0.1, 64) + 1j * rng.normal(0, 0.1, 64)
        self.tiled = np.tile(rng.normal(0, 0.1, (32, 16)), (1, (N // 2) // 16))     # 32 periodic rows: compact batch
        self.W = rng.normal(0, 0.02, (8, 8))
        self.rows3 = rng.normal(0, 0.1, (3, N // 2))

        def limbs(ncomp, l):
            return np.stack([np.stack([rng.integers(0, self.primes[i], N, dtype=np.uint64) for i in range(l)])
                             for _ in range(ncomp)])
        self.a_np, self.b_np = limbs(2, _L0), limbs(2, _L0)
        self.p_np = limbs(1, _L0)[0]
        self.a = ph.ciphertext_from_numpy(ctx, self.a_np, 1, _SC)
        self.b = ph.ciphertext_from_numpy(ctx, self.b_np, 1, _SC)
        self.ab3 = ph.multiply(ctx, self.a, self.b)
        self.low = ph.mod_switch_to(ctx, self.a, _L0)                                 # one limb: mod_raise operand
        self.pt = enc.encode_double_vector(ctx, self.x, _SC)
        self.pts3 = [enc.encode_double_vector(ctx, self.rows3[0], _SC), enc.encode_double_vector(ctx, self.rows3[1], _SC),
                     enc.encode_double_vector(ctx, self.rows3[2], _SC, chain_index=2)]
        self.cts3 = sk.encrypt_symmetric_batch(ctx, self.pts3[:2])
        r1 = ph.rotate(ctx, self.a, 1, self.gk)
        self.baby = [self.a, r1, ph.rotate(ctx, self.a, 2, self.gk), ph.rotate(ctx, r1, 2, self.gk)]
        self.diag = ph.random_plaintexts(ctx, 7, 8, 1, _SC)
        self.db = [[ph.ciphertext_from_numpy(ctx, limbs(2, _L0), 1, _SC) for _ in range(2)] for _ in range(3)]
        self.gk_np = {e: self.gk.export(e) for e in ph.get_elts_from_steps([1, 2], N)}
        self.rk_np = self._rk_export(self.rk)
        ctx.synchronize()
        self.swept = {}      # operation -> injected failures seen

    def _rk_export(self, rk):
        import ctypes as C
        ph, c = self.ph, self.ctx
        out = np.empty((-(-_L0 // _P), 2, _L0 + _P, _N), dtype=np.uint64)
        rc = ph._lib.fhs_relin_key_export(c._h, rk._h, out.ctypes.data_as(C.POINTER(C.c_uint64)))
        ph._check(rc, "relin key export")
        return out

    def fresh_sk(self):
        """Encryption counters advance with every call, failed ones included: a fresh key per run keeps the bits fixed."""
        return self.ph.secret_key(self.ctx, seed=_SEED)


def _u64(a):
    return np.ascontiguousarray(np.asarray(a)).view(np.uint64)


def _op_rotate_flush(s):
    r = s.ph.rotate(s.ctx, s.a, 1, s.gk)         # queued; the add's entry flushes it
    return s.ph.add(s.ctx, r, r).to_numpy()


def _op_pk_asym(s):
    pk = s.fresh_sk().gen_publickey(s.ctx)
    return pk.encrypt_asymmetric(s.ctx, s.pt).to_numpy()


def _op_gk_roundtrip(s):
    gk = s.sk.create_galois_keys(s.ctx, s.ph.get_elts_from_steps([1, 2], _N))
    return np.stack([gk.export(e) for e in sorted(s.gk_np)])


def _op_gk_import(s):
    gk = s.ph.galois_keys_from_numpy(s.ctx, s.gk_np)
    return np.stack([gk.export(e) for e in sorted(s.gk_np)])


def _op_decode_fallback(s):
    p = s.ph.plaintext_from_numpy(s.ctx, s.p_np, 1, _SC)
    q = s.ph.plaintext_from_numpy(s.ctx, s.p_np, 1, _SC)
    return _u64(s.enc.decode_batch(s.ctx, [p, q, q], 64))


# name -> callable(state) returning the result's bits as an array; every object it makes dies with its frame
_OPS = {
    "add": lambda s: s.ph.add(s.ctx, s.a, s.b).to_numpy(),
    "encode": lambda s: s.enc.encode_double_vector(s.ctx, s.x, _SC).to_numpy(),
    "encode_batch_compact": lambda s: np.stack([p.to_numpy() for p in
                                                s.enc.encode_double_vector_batch(s.ctx, s.tiled, _SC)]),
    "encode_matrix_diagonals": lambda s: np.stack([p.to_numpy() for p in
                                                   s.enc.encode_matrix_diagonals(s.ctx, s.W, 4, _SC)]),
    "encode_precise": lambda s: s.enc.encode_complex_vector_batch(s.ctx, s.z[None, :], _SC, precise=True)[0].to_numpy(),
    "decode": lambda s: _u64(s.enc.decode_complex_vector(s.ctx, s.pt)),
    "decode_batch": lambda s: _u64(s.enc.decode_batch(s.ctx, s.pts3, 64)),
    "decrypt_decode_batch": lambda s: _u64(s.sk.decrypt_decode_batch(s.ctx, s.cts3, 64)),
    # uniformly random limbs: the check against the limbs not composed fails, so every item takes the exact
    # fallback (all six limbs recomposed, decoded on its own)
    "decode_fallback": _op_decode_fallback,
    "decrypt_decode_fallback": lambda s: _u64(s.sk.decrypt_decode_batch(s.ctx, [s.a, s.b], 64)),
    "encrypt_symmetric": lambda s: s.fresh_sk().encrypt_symmetric(s.ctx, s.pt).to_numpy(),
    "encrypt_symmetric_batch": lambda s: np.stack([c.to_numpy() for c in
                                                   s.fresh_sk().encrypt_symmetric_batch(s.ctx, s.pts3[:2] + [s.pt])]),
    "encode_encrypt_batch": lambda s: np.stack([c.to_numpy() for c in
                                                s.fresh_sk().encode_encrypt_batch(s.ctx, s.rows3, _SC)]),
    "gen_publickey+encrypt_asymmetric": _op_pk_asym,
    "decrypt": lambda s: s.sk.decrypt(s.ctx, s.a).to_numpy(),
    "negate": lambda s: s.ph.negate(s.ctx, s.a).to_numpy(),
    "multiply_plain": lambda s: s.ph.multiply_plain(s.ctx, s.a, s.pt).to_numpy(),
    "multiply_plain_compact": lambda s: s.ph.multiply_plain(
        s.ctx, s.a, s.enc.encode_double_vector_batch(s.ctx, s.tiled, _SC)[3]).to_numpy(),
    "multiply": lambda s: s.ph.multiply(s.ctx, s.a, s.b).to_numpy(),
    "relinearize": lambda s: s.ph.relinearize(s.ctx, s.ab3, s.rk).to_numpy(),
    "rescale": lambda s: s.ph.rescale_to_next(s.ctx, s.a).to_numpy(),
    "mod_switch_to_ct": lambda s: s.ph.mod_switch_to(s.ctx, s.a, 3).to_numpy(),
    "mod_switch_to_pt": lambda s: s.ph.mod_switch_to(s.ctx, s.pt, 3).to_numpy(),
    "rotate+flush": _op_rotate_flush,
    "bsgs_multiply_accumulate": lambda s: s.ph.bsgs_multiply_accumulate(s.ctx, s.baby, s.diag, 4, 2, 8, s.gk).to_numpy(),
    "bsgs_inner_products": lambda s: np.stack([c.to_numpy() for c in
                                               s.ph.bsgs_inner_products(s.ctx, s.baby, s.diag, 4, 2)]),
    "linear_transform": lambda s: s.ph.linear_transform(s.ctx, s.baby, s.diag, 4, [1, s.ph.get_elt_from_step(4, _N)],
                                                        s.gk, rescale=False).to_numpy(),
    "dot_product_many": lambda s: np.stack([c.to_numpy() for c in
                                            s.ph.dot_product_many(s.ctx, [s.a, s.b], s.db, s.rk, True)]),
    "multiply_const": lambda s: s.ph.multiply_const(s.ctx, s.a, 3.0, 2.0 ** 20).to_numpy(),
    "mod_raise": lambda s: s.ph.mod_raise(s.ctx, s.low).to_numpy(),
    "gen_relinkey+export": lambda s: s._rk_export(s.sk.gen_relinkey(s.ctx)),
    "relin_key_import+export": lambda s: s._rk_export(s.ph.relin_key_from_numpy(s.ctx, s.rk_np)),
    "create_galois_keys+export": _op_gk_roundtrip,
    "galois_keys_import+export": _op_gk_import,
    "ciphertext_import": lambda s: s.ph.ciphertext_from_numpy(s.ctx, s.a_np, 1, _SC).to_numpy(),
    "plaintext_import": lambda s: s.ph.plaintext_from_numpy(s.ctx, s.p_np, 1, _SC).to_numpy(),
}


@pytest.fixture(scope="module")
def small(ph):
    return _Small(ph)


def _sweep(s, op):
    """The unarmed run warms scratch slots, dense expansions and CRT tables and keeps the bits.  Then allocation k
    = 0, 1, 2, ... fails: a raise must be RuntimeError("... out of memory ...") and leave memory_in_use unchanged;
    a return with the hook still pending ends the sweep (the call makes at most k allocations) with the kept bits.
    A return with the hook consumed is a call that absorbed the failure by its documented fallback (a periodic
    batch without room for its compact block is encoded dense): same bits, same memory check, the sweep goes on.
    Returns the number of injected failures."""
    ph, ctx = s.ph, s.ctx
    want = op(s)
    ctx.synchronize()
    before = ctx.memory_in_use()
    failures = 0
    for k in range(_MAX_STEPS):
        ph.debug_fail_alloc(ctx, k)
        try:
            got = op(s)
        except RuntimeError as e:
            assert "out of memory" in str(e), (k, str(e))
            got = None
        pending = ph.debug_fail_alloc(ctx, -1)
        if got is None:
            assert not pending, f"allocation {k}: an out-of-memory error the hook did not inject"
        else:
            assert got.dtype == want.dtype and np.array_equal(got, want), f"allocation {k}: result bits changed"
            if pending:
                return failures
        failures += 1
        ctx.synchronize()
        assert ctx.memory_in_use() == before, f"allocation {k} failed: {ctx.memory_in_use() - before} bytes left behind"
    raise AssertionError(f"sweep did not end within {_MAX_STEPS} steps")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_OPS))
def test_alloc_failure_leaves_no_hbm_behind(small, name):
    """Before device temporaries and results were owned by scope (the hook alone applied to that tree), three of
    these cases failed, each with one 98304-byte ciphertext (2 x 6 x 1024 words) left behind: encrypt_symmetric
    (allocation 2: the error buffer after the result), gen_publickey+encrypt_asymmetric (allocation 4: the samplers'
    buffer after the result) and multiply_plain_compact (allocation 5: the dense expansion of a compact plaintext
    after the result).  The other returns past a live result were behind failed launches or copies, which an
    allocation hook does not reach."""
    small.swept[name] = _sweep(small, _OPS[name])
    assert small.swept[name] >= 1, "no allocation failure was injected: the sweep checked nothing"


@pytest.mark.gpu
def test_context_computes_after_the_sweeps(small):
    """After every sweep the context's first operation, and a rotation through the key switch, still give the
    oracle's limbs."""
    s, ph = small, small.ph
    assert np.array_equal(_OPS["add"](s), s.oracle.add(s.a_np, s.b_np))
    e = ph.get_elt_from_step(1, _N)
    sec = s.oracle.gen_secret(_SEED)
    assert np.array_equal(ph.rotate(s.ctx, s.a, 1, s.gk).to_numpy(),
                          s.oracle.rotate_elt(s.a_np, s.oracle.gen_galois_key(_SEED, sec, e), e))
    s.ctx.synchronize()
