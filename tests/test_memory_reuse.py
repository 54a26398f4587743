"""Memory-reuse parity: the host layer's reuse paths against the CPU oracle, limb for limb (np.array_equal).

The kernels are judged at every ring elsewhere; this file judges the code that decides which device bytes they read
and write, on rings small enough that every case takes seconds:
  (a) a level walk under three block-cache caps (default, 0 and 262144 bytes): evict_cold and dfree over cache_cap,
      with every dropped block's readers still queued; once more with the giant steps on the side stream;
  (b) dalloc_fit: a batch taking a cached block of up to 1.5 times its request whole;
  (c) the SEAL correction cache: its cap, a key pointer reused by another secret's keys, its out-of-memory fallback;
  (d) the pinned staging ring wrapping twice with nothing read back in between, and its boundary sizes;
  (e) the rotation queue's own limits (512 items, a level change, a queued output as input, an input destroyed);
  (f) the grow-only key-switch workspace growing while a smaller flush is still queued.
What keeps a case from passing vacuously is the allocator's own counters (pyPhantom context.debug_alloc_stats,
staging_stats, seal_hoist_stats): a cap that stopped being read, or a ring that never wrapped, fails the case.
Every test needs an MI355X: -m gpu."""
import ctypes as C
import gc

import numpy as np
import pytest

import _edge_inputs as ei
import _embedding_ref as er
from _launch_matrix import check_encode_exact
from test_edge_operands import SCALE, make_ctx, same, up
from test_gpu_parity import rand_ct, rand_pt

pytestmark = pytest.mark.gpu

# ring of (a), (b) and (f): the smoke check's
N_A, BITS_A, P_A, L0_A, SEED_A = 1024, [59] * 9, 3, 6, 4242
STEPS_A = (1, 2, 4, -1)
ROT3 = (1, 4, -1)
LEVELS = (6, 5, 4, 3, 2)
ROW_A = 8 * N_A                      # bytes of one limb
PARTIAL_CAP = 262144                 # under three top-level ciphertexts (2 x 6 x 1024 words = 96 KiB each)


@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


def limbs_of(handles):
    """to_numpy of every handle; no name of this frame outlives the call, so the caller alone decides lifetimes"""
    return [h.to_numpy() for h in handles]


def rk_export(ph, ctx, rk, o):
    out = np.empty(o.key_shape(), dtype=np.uint64)
    ph._check(ph._lib.fhs_relin_key_export(ctx._h, rk._h, out.ctypes.data_as(C.POINTER(C.c_uint64))), "relin key export")
    return out


# ---------------------------------------------------------------------------------------------- (a) level walk
class WalkPlan:
    """The walk's top-level inputs and the oracle's value of every result at every level, computed once and shared
    by every run.  Ten ciphertexts walk down together (mod_switch_to_next is slicing): x (rotations, BSGS), three
    pairs (multiply_relin_many) and three inner-sum inputs."""

    def __init__(self, ph, orc):
        self.primes = [int(q) for q in ph.create_coeff_modulus(N_A, BITS_A)]
        o = self.o = orc.Oracle(N_A, self.primes, P_A)
        self.s = o.gen_secret(SEED_A)
        self.elt = {st: ph.get_elt_from_step(st, N_A) for st in STEPS_A}
        self.okey = {st: o.gen_galois_key(SEED_A, self.s, e) for st, e in self.elt.items()}
        self.orlk = o.gen_relin_key(SEED_A, self.s)
        rng = np.random.default_rng(61)
        self.top = [rand_ct(o, rng, 2, L0_A) for _ in range(10)]
        self.rows = rng.normal(0, 1, (3, N_A // 2))
        self.want = {l: self._level(l) for l in LEVELS}
        # the encoder's rows: one quiet batch per level on a context of its own, one row per level against the
        # extended-precision reference (the float64 encoder has no limb-exact oracle)
        ctx, _, _ = make_ctx(ph, N_A, BITS_A, P_A)
        enc = ph.ckks_encoder(ctx)
        self.N = N_A
        for l in LEVELS:
            pts = enc.encode_double_vector_batch(ctx, self.rows, SCALE, chain_index=L0_A + 1 - l)
            check_encode_exact(self, self.rows[l % 3], SCALE, pts[l % 3], f"quiet encode, l={l}, row {l % 3}")
            self.want[l]["enc"] = limbs_of(pts)

    def coeffs(self, pt):            # what check_encode_exact reads of its ring
        return er.coeffs_of(self.o, pt.to_numpy())

    def _level(self, l):
        o = self.o
        w = [np.ascontiguousarray(t[:, :l]) for t in self.top]
        x, A, B, S = w[0], w[1:4], w[4:7], w[7:10]
        rot = {st: o.rotate_elt(x, self.okey[st], self.elt[st]) for st in ROT3}
        pn = [o.random_plaintext(100 + l, k, l) for k in range(4)]
        sums = []
        for v in S:
            for step in (1, 2):
                v = o.add(v, o.rotate(v, self.okey[step], step))
            sums.append(v)
        return {"rot": [rot[st] for st in ROT3],
                "bsgs": o.bsgs_loop([x, rot[1]], pn, [None, self.okey[2]], 2, 2, 4),
                "prods": [o.rescale(o.relinearize(o.multiply(a, b), self.orlk)) for a, b in zip(A, B)],
                "sums": sums,
                "next": [np.ascontiguousarray(t[:, :l - 1]) for t in w]}


@pytest.fixture(scope="module")
def plan(ph, orc):
    return WalkPlan(ph, orc)


def walk_ctx(ph, plan):
    """Context of ring (a) with seeded keys, each compared with the oracle's on creation."""
    ctx, sk, _ = make_ctx(ph, N_A, BITS_A, P_A, steps=STEPS_A, seed=SEED_A)
    same(sk.export(), plan.s, "secret key")
    gk = sk.create_galois_keys(ctx)
    for st in STEPS_A:
        same(gk.export(plan.elt[st]), plan.okey[st], f"Galois key of step {st}")
    rlk = sk.gen_relinkey(ctx)
    same(rk_export(ph, ctx, rlk, plan.o), plan.orlk, "relinearisation key")
    return ctx, sk, gk, rlk


def walk(ph, ctx, gk, rlk, plan, after_call):
    """l = 6, 5, 4, 3, 2: three queued rotations of x, a fused BSGS (G = 2, B = 2) whose baby rotation and diagonals
    are dropped right after the call, multiply_relin_many on three pairs, inner_sum_many (dim 4) on three inputs, a
    batch encode of three rows, and mod_switch_to_next of all ten walkers, whose level-l handles are dropped right
    after it.  Nothing is synchronised or read between the first call of a level and its last; after_call(what)
    runs after each (it reads the allocator's counters only).  Then everything is read back and compared."""
    enc = ph.ckks_encoder(ctx)
    W = [up(ph, ctx, plan.o, t) for t in plan.top]
    for l in LEVELS:
        ci, want = L0_A + 1 - l, plan.want[l]
        rots = [ph.rotate(ctx, W[0], st, gk) for st in ROT3]
        after_call("rotate")
        b1 = ph.rotate(ctx, W[0], 1, gk)
        pts = ph.random_plaintexts(ctx, 100 + l, 4, ci, SCALE)
        after_call("random_plaintexts")
        y = ph.bsgs_multiply_accumulate(ctx, [W[0], b1], pts, 2, 2, 4, gk)
        del pts, b1
        gc.collect()
        after_call("bsgs_multiply_accumulate")
        prods = ph.multiply_relin_many(ctx, W[1:4], W[4:7], rlk)
        after_call("multiply_relin_many")
        sums = ph.inner_sum_many(ctx, W[7:10], 4, gk)
        after_call("inner_sum_many")
        epts = enc.encode_double_vector_batch(ctx, plan.rows, SCALE, chain_index=ci)
        after_call("encode_double_vector_batch")
        nxt = [ph.mod_switch_to_next(ctx, c) for c in W]
        del W
        gc.collect()
        after_call("mod_switch_to_next")
        for name, handles in (("rot", rots), ("bsgs", [y]), ("prods", prods), ("sums", sums), ("enc", epts),
                              ("next", nxt)):
            w = want[name] if isinstance(want[name], list) else [want[name]]
            for i, (g, e) in enumerate(zip(limbs_of(handles), w)):
                same(g, e, f"l={l}: {name}[{i}]")
        del handles, rots, y, prods, sums
        p0, p1, p2 = epts
        del epts, p1
        del p0
        del p2
        gc.collect()
        after_call("results dropped")
        W = nxt
        del nxt
    del W
    gc.collect()


def run_walks(ph, plan, after_call, fork=False):
    """A context of its own, the walk twice: the first pass grows every scratch slot from nothing (the outgrown
    workspaces go through dfree too), the second must leave memory_in_use where it found it."""
    ctx, sk, gk, rlk = walk_ctx(ph, plan)
    if fork:
        ph.debug_force_fork(ctx, True)
    hook = lambda what: after_call(ctx, what)
    walk(ph, ctx, gk, rlk, plan, hook)
    ctx.synchronize()
    before = ctx.memory_in_use()
    walk(ph, ctx, gk, rlk, plan, hook)
    ctx.synchronize()
    assert ctx.memory_in_use() == before, f"{ctx.memory_in_use() - before} bytes left behind by the walk"
    st = ctx.debug_alloc_stats()
    print(f"level walk: cache_cap {st['cache_cap']}, evicted {st['evicted']}, fit {st['fit']}, "
          f"forked {ph.debug_force_fork(ctx)}")
    return ctx, st


def test_walk_default_cap_evicts_nothing(ph, plan, monkeypatch):
    """Control: under the default cap (a quarter of HBM) the same walk never reaches evict_cold."""
    monkeypatch.delenv("FHESPEAR_CACHE_BYTES", raising=False)
    ctx, st = run_walks(ph, plan, lambda ctx, what: None)
    assert st["evicted"] == 0 and st["cache_cap"] > 1 << 30
    assert st["cached_bytes"] > 0, "the walk's dropped blocks are in the cache"


def test_walk_every_free_evicts(ph, plan, monkeypatch):
    """FHESPEAR_CACHE_BYTES=0: every dfree returns its block to the device (the `keep` size is the only one cached,
    so evict_cold sheds it) after synchronising both streams; nothing is ever cached."""
    monkeypatch.setenv("FHESPEAR_CACHE_BYTES", "0")

    def empty(ctx, what):
        st = ctx.debug_alloc_stats()
        assert st["cache_cap"] == 0 and st["cached_bytes"] == 0, (what, st)
    ctx, st = run_walks(ph, plan, empty)
    assert st["evicted"] > 0


@pytest.mark.parametrize("fork", [False, True], ids=["auto", "forked"])
def test_walk_partial_eviction(ph, plan, monkeypatch, fork):
    """FHESPEAR_CACHE_BYTES=262144: the cache holds some blocks and sheds the least recently used sizes, or the size
    in hand when nothing else is cached; never over the cap after a call.  Forced to fork, every BSGS's special-limb
    chain runs on the side stream while blocks are being evicted."""
    monkeypatch.setenv("FHESPEAR_CACHE_BYTES", str(PARTIAL_CAP))
    most = [0]

    def bounded(ctx, what):
        st = ctx.debug_alloc_stats()
        assert st["cache_cap"] == PARTIAL_CAP and st["cached_bytes"] <= PARTIAL_CAP, (what, st)
        most[0] = max(most[0], st["cached_bytes"])
    ctx, st = run_walks(ph, plan, bounded, fork)
    assert st["evicted"] > 0
    assert most[0] > 0, "the cap is partial: something was cached at some point"
    assert ph.debug_force_fork(ctx) >= (2 * len(LEVELS) if fork else 0)
    if not fork:
        assert ph.debug_force_fork(ctx) == 0


# ---------------------------------------------------------------------------------------------- (b) dalloc_fit
def test_batch_takes_a_larger_cached_block_whole(ph, orc):
    """A destroyed batch of four plaintexts at l = 5 leaves a 20-row block cached; a batch of three at l = 5 (15 rows,
    20 <= 22.5) takes it whole, a batch of two at l = 6 (12 rows, 20 > 18) does not."""
    ctx, _, o = make_ctx(ph, N_A, BITS_A, P_A)
    st = ctx.debug_alloc_stats()
    assert st["fit"] == 0 and st["cached_bytes"] == 0
    base = ctx.memory_in_use()
    four = ph.random_plaintexts(ctx, 31, 4, 2, SCALE)
    assert ctx.memory_in_use() == base + 20 * ROW_A
    del four
    gc.collect()
    assert ctx.memory_in_use() == base and ctx.debug_alloc_stats()["cached_bytes"] == 20 * ROW_A
    three = ph.random_plaintexts(ctx, 32, 3, 2, SCALE)
    st = ctx.debug_alloc_stats()
    assert st["fit"] == 1 and st["cached_bytes"] == 0
    assert ctx.memory_in_use() == base + 20 * ROW_A, "the 20-row block was taken whole"
    for k, got in enumerate(limbs_of(three)):
        same(got, o.random_plaintext(32, k, 5), f"batch of three in the larger block: plaintext {k}")
    del three[1]
    assert ctx.memory_in_use() == base + 20 * ROW_A, "the block stays until its last plaintext goes"
    del three
    gc.collect()
    assert ctx.memory_in_use() == base
    four = ph.random_plaintexts(ctx, 33, 4, 2, SCALE)         # the exact size: a plain cache hit, not a fit
    same(four[3].to_numpy(), o.random_plaintext(33, 3, 5), "refill: plaintext 3")
    del four
    gc.collect()
    st = ctx.debug_alloc_stats()
    assert st["fit"] == 1 and st["cached_bytes"] == 20 * ROW_A
    two = ph.random_plaintexts(ctx, 34, 2, 1, SCALE)
    st = ctx.debug_alloc_stats()
    assert st["fit"] == 1 and st["cached_bytes"] == 20 * ROW_A, "20 rows are more than 1.5 x 12: not taken"
    assert ctx.memory_in_use() == base + 12 * ROW_A
    for k, got in enumerate(limbs_of(two)):
        same(got, o.random_plaintext(34, k, 6), f"batch of two in a block of its own: plaintext {k}")


# ---------------------------------------------------------------------------------------------- (c) SEAL corrections
N_C, BITS_C, L0_C, STEPS_C = 1024, [59] * 4 + [60], 4, (1, -1, 3)


def corr_bytes(l):
    return 8 * 2 * (l + 1) * N_C


class SealEnv:
    """SEAL-convention context on [59]*4 + [60], P = 1, with the Galois keys of `seed` and the oracle's."""

    def __init__(self, ph, seed=91):
        self.ph = ph
        self.ctx, self.sk, self.o = make_ctx(ph, N_C, BITS_C, 1, steps=STEPS_C, seed=seed, mode="seal")
        self.gk = self.sk.create_galois_keys(self.ctx)
        self.okeys = self.oracle_keys(seed)
        self.rng = np.random.default_rng(seed)

    def oracle_keys(self, seed):
        s = self.o.gen_secret(seed)
        return {st: self.o.gen_galois_key(seed, s, self.ph.get_elt_from_step(st, N_C)) for st in STEPS_C}

    def operand(self, l):
        """as case_seal: the switched component on the one-limb boundary set without a zero coefficient"""
        c1 = ei.near_half_digits(self.o.primes, 1, l, N_C, self.rng, exclude_zero=True)
        return np.stack([rand_pt(self.o, self.rng, l), ei.to_ntt(self.o, c1)])

    def hoist(self, l, what, path=0, gk=None, okeys=None, a=None):
        """One hoisting() call at level l, equal to Oracle.rotate per step, taken the given way (0 hoisted,
        1 per-rotation fallback) and no other."""
        ph, ctx = self.ph, self.ctx
        a = self.operand(l) if a is None else a
        h0 = ctx.seal_hoist_stats()
        rots = ph.hoisting(ctx, up(ph, ctx, self.o, a), gk or self.gk, list(STEPS_C))
        for st, got in zip(STEPS_C, limbs_of(rots)):
            same(got, self.o.rotate(a, (okeys or self.okeys)[st], st), f"{what}: l={l}, step {st}")
        h1 = ctx.seal_hoist_stats()
        assert h1[path] == h0[path] + 1 and h1[1 - path] == h0[1 - path], (what, l, h0, h1)


def test_seal_corrections_without_room(ph, orc, monkeypatch):
    """FHESPEAR_SEAL_CORR_BYTES=0: every flush at a level whose corrections are not cached empties the cache first
    -- l = 4, 3, 4 drops the previous level's at each change (the first flush finds nothing to drop) -- and every
    flush is hoisted with the oracle's limbs."""
    monkeypatch.setenv("FHESPEAR_SEAL_CORR_BYTES", "0")
    e = SealEnv(ph)
    assert e.ctx.debug_alloc_stats()["seal_corr_cap"] == 0
    drops = []
    for l in (4, 3, 4):
        e.hoist(l, "no room")
        st = e.ctx.debug_alloc_stats()
        drops.append(st["seal_corr_drops"])
        assert st["seal_corr_bytes"] == 3 * corr_bytes(l), "this flush's corrections only"
    assert drops == [0, 1, 2]
    e.hoist(4, "no room, same level again")
    assert e.ctx.debug_alloc_stats()["seal_corr_drops"] == 2, "cached corrections are used, not dropped"


def test_seal_corrections_cap_of_one_level(ph, orc, monkeypatch):
    """The cap at exactly one level-4 set (three keys): l = 4 twice drops nothing, l = 3 afterwards drops once."""
    monkeypatch.setenv("FHESPEAR_SEAL_CORR_BYTES", str(3 * corr_bytes(4)))
    e = SealEnv(ph)
    for k in range(2):
        e.hoist(4, f"one level fits, call {k}")
        st = e.ctx.debug_alloc_stats()
        assert st["seal_corr_drops"] == 0 and st["seal_corr_bytes"] == st["seal_corr_cap"] == 3 * corr_bytes(4)
    e.hoist(3, "the next level does not fit beside it")
    st = e.ctx.debug_alloc_stats()
    assert st["seal_corr_drops"] == 1 and st["seal_corr_bytes"] == 3 * corr_bytes(3)


def test_seal_corrections_of_a_reused_key_pointer(ph, orc, monkeypatch):
    """The corrections are keyed by (device pointer of the key, level).  Secret A's key set is destroyed and secret
    B's created on the same context: its key blocks come from the block cache, so the pointers repeat, and the
    hoisted limbs must be the oracle's under B's keys, not A's corrections.

    Device pointers are not visible from Python.  What is: the key blocks have a size nothing else has
    (dnum K N + dnum words), dalloc hands out cached blocks of the exact size only, and memory_in_use + cached_bytes
    (all the context holds from the device) is the same after B's keys exist as before A's were destroyed -- so no
    allocation of B's key generation went to the device, and each of B's keys sits in a block one of A's had."""
    monkeypatch.delenv("FHESPEAR_SEAL_CORR_BYTES", raising=False)
    e = SealEnv(ph, seed=92)
    ctx = e.ctx
    sk_b = ph.secret_key(ctx, seed=93)      # before the hoisted flush: its limbs are not a block that flush frees
    a = e.operand(4)
    e.hoist(4, "keys of secret A", a=a)
    assert ctx.debug_alloc_stats()["seal_corr_bytes"] == 3 * corr_bytes(4)
    okeys_b = e.oracle_keys(93)
    key_bytes = e.gk.nbytes()
    ctx.synchronize()
    held = ctx.memory_in_use() + ctx.debug_alloc_stats()["cached_bytes"]
    e.gk = None
    gc.collect()
    st = ctx.debug_alloc_stats()
    assert st["seal_corr_bytes"] == 0, "a key's corrections leave with the key"
    assert st["cached_bytes"] >= key_bytes + 3 * corr_bytes(4)
    gk_b = sk_b.create_galois_keys(ctx)
    assert ctx.memory_in_use() + ctx.debug_alloc_stats()["cached_bytes"] == held, "B's key blocks are A's"
    for st_ in STEPS_C:
        same(gk_b.export(ph.get_elt_from_step(st_, N_C)), okeys_b[st_], f"secret B: Galois key of step {st_}")
    e.hoist(4, "keys of secret B in A's blocks", gk=gk_b, okeys=okeys_b, a=a)
    assert ctx.debug_alloc_stats()["seal_corr_drops"] == 0


def test_seal_corrections_out_of_memory_fallback(ph, orc, monkeypatch):
    """debug_fail_alloc at every allocation of one hoisted flush whose corrections are not cached (the workspace and
    the zero flag are warm).  The first three are the outputs of the queued rotations: "out of memory" with nothing
    left allocated (fhs_rotate_many used to leave the outputs made before the failing one allocated and queued, with
    no handle for its caller to destroy them by: 65536 bytes left when allocation 1 failed).  Every later
    one is inside seal_prepare (the mask scratch, then one correction per key): the flush takes the per-rotation path
    -- the oracle's limbs, the fallback count + 1 -- and memory_in_use is back at its baseline once the results are
    destroyed and the corrections dropped.  Either way the next hoisted flush is correct."""
    monkeypatch.delenv("FHESPEAR_SEAL_CORR_BYTES", raising=False)
    e = SealEnv(ph, seed=94)
    ph_, ctx = ph, e.ctx
    a = e.operand(4)
    A = up(ph, ctx, e.o, a)
    want = [e.o.rotate(a, e.okeys[st], st) for st in STEPS_C]

    def uncache():                   # setting the mode again empties the correction cache (not a cap drop)
        ctx.set_key_switch_mode("seal")
        assert ctx.debug_alloc_stats()["seal_corr_bytes"] == 0

    e.hoist(4, "warm", a=a)
    uncache()
    ctx.synchronize()
    before = ctx.memory_in_use()
    raised, fell_back = [], []
    for k in range(16):
        h0 = ctx.seal_hoist_stats()
        ph_.debug_fail_alloc(ctx, k)
        try:
            rots = ph_.hoisting(ctx, A, e.gk, list(STEPS_C))
        except RuntimeError as err:
            assert "out of memory" in str(err), (k, str(err))
            rots = None
        pending = ph_.debug_fail_alloc(ctx, -1)
        if rots is None:
            assert not pending, f"allocation {k}: an out-of-memory error the hook did not inject"
            raised.append(k)
            assert ctx.seal_hoist_stats()[1] == h0[1]      # (the outputs already queued are flushed as they go)
        else:
            for st, got, w in zip(STEPS_C, limbs_of(rots), want):
                same(got, w, f"allocation {k} failed: step {st}")
            h1 = ctx.seal_hoist_stats()
            if pending:                                  # the flush makes k allocations: the sweep is over
                assert h1 == (h0[0] + 1, h0[1])
                break
            fell_back.append(k)
            assert h1 == (h0[0], h0[1] + 1), (k, h0, h1)
        del rots
        gc.collect()
        uncache()
        ctx.synchronize()
        assert ctx.memory_in_use() == before, f"allocation {k} failed: {ctx.memory_in_use() - before} bytes left"
        e.hoist(4, f"after allocation {k} failed", a=a)
        uncache()
    else:
        raise AssertionError("the sweep did not end within 16 allocations")
    assert raised == [0, 1, 2], "the three queued outputs"
    assert fell_back == [3, 4, 5, 6], "seal_prepare: the mask scratch and one correction per key"
    assert ctx.debug_alloc_stats()["seal_corr_drops"] == 0


# ---------------------------------------------------------------------------------------------- (d) staging ring
N_D, BITS_D, STEPS_D = 1024, [59] * 4, (1, 2, 3, 64)
SEG_ROWS = 512                       # kSegBytes = 2 MiB = 512 rows x 512 values x 8 bytes


class _EncRing:
    """what check_encode_exact reads of its ring"""

    def __init__(self, o):
        self.N, self.o = o.N, o

    def coeffs(self, pt):
        return er.coeffs_of(self.o, pt.to_numpy())


def test_staging_ring_wraps_twice_without_a_readback(ph, orc):
    """768 KiB value uploads (192 rows of 512 doubles) with pointer arrays and key-switch descriptors in between, 48
    iterations and nothing read back: two uploads fill most of a 2 MiB segment, the third skips to the next one, and
    the ring is lapped twice.  A segment re-entered too early would put a later iteration's values or pointers into
    an earlier iteration's copy; every plaintext, rotation and product of every iteration is compared.

    A row's limbs do not depend on its position in the batch (each row is encoded on its own), so the rolled batches
    are compared row by row with ONE quiet batch: this context's first call.  Batches of 32 rows or more wait for
    the detected periods (encode_rows_dev), so the host does not run far ahead here and the re-entries that waited
    are printed, not asserted."""
    seed = 95
    ctx, sk, o = make_ctx(ph, N_D, BITS_D, 1, steps=STEPS_D, seed=seed)
    enc = ph.ckks_encoder(ctx)
    rng = np.random.default_rng(96)
    bank = rng.normal(0, 1, (192, N_D // 2))
    quiet = enc.encode_double_vector_batch(ctx, bank, SCALE)
    assert ph.staging_stats(ctx)[0] == 0
    ring = _EncRing(o)
    for j in range(0, 192, 24):
        check_encode_exact(ring, bank[j], SCALE, quiet[j], f"quiet batch, row {j}")
    want_row = limbs_of(quiet)
    del quiet
    s = o.gen_secret(seed)
    gk, rlk = sk.create_galois_keys(ctx), sk.gen_relinkey(ctx)
    elt = {st: ph.get_elt_from_step(st, N_D) for st in STEPS_D}
    okey = {st: o.gen_galois_key(seed, s, e) for st, e in elt.items()}
    orlk = o.gen_relin_key(seed, s)
    l = o.L0
    x, pa, pb = rand_ct(o, rng, 2, l), [rand_ct(o, rng, 2, l) for _ in range(2)], [rand_ct(o, rng, 2, l) for _ in range(2)]
    X, PA, PB = up(ph, ctx, o, x), [up(ph, ctx, o, v) for v in pa], [up(ph, ctx, o, v) for v in pb]
    want_rot = [o.rotate_elt(x, okey[st], elt[st]) for st in (1, 2, 3)]
    want_prod = [o.rescale(o.relinearize(o.multiply(u, v), orlk)) for u, v in zip(pa, pb)]
    # a long job on this context's stream first: G = 64, B = 2 over 128 diagonals
    dpts = ph.random_plaintexts(ctx, 97, 128, 1, SCALE)
    want_first = o.bsgs_loop([x] * 64, [o.random_plaintext(97, k, l) for k in range(128)], [None, okey[64]], 64, 2, 128)
    first = ph.bsgs_multiply_accumulate(ctx, [X] * 64, dpts, 64, 2, 128, gk)
    kept = []
    for i in range(48):
        pts = enc.encode_double_vector_batch(ctx, np.roll(bank, 7 * i, axis=0), SCALE)
        rots = [ph.rotate(ctx, X, st, gk) for st in (1, 2, 3)]
        prods = ph.multiply_relin_many(ctx, PA, PB, rlk)
        kept.append((pts, rots, prods))
    reentries, waited = ph.staging_stats(ctx)
    print(f"staging ring after 48 iterations: {reentries} segment re-entries, {waited} waited for the GPU")
    assert reentries >= 16, "two full laps of the eight segments"
    same(first.to_numpy(), want_first, "the long first job")
    for i, (pts, rots, prods) in enumerate(kept):
        for j, got in enumerate(limbs_of(pts)):
            same(got, want_row[(j - 7 * i) % 192], f"iteration {i}: plaintext {j} (limb, slot)")
        for k, got in enumerate(limbs_of(rots)):
            same(got, want_rot[k], f"iteration {i}: rotation {k}")
        for k, got in enumerate(limbs_of(prods)):
            same(got, want_prod[k], f"iteration {i}: product {k}")
    del kept, pts, rots, prods
    gc.collect()
    # boundary sizes, the head mid-segment: exactly one segment (skips to the next one and fills it, so the pointer
    # array behind it enters a third), and one row more (stage_h2d's synchronous copy, past the ring)
    for rows in (SEG_ROWS, SEG_ROWS + 1):
        idx = (np.arange(rows) * 5 + 3) % 192
        r0 = ph.staging_stats(ctx)[0]
        small = enc.encode_double_vector_batch(ctx, bank[:2], SCALE)         # leaves the head inside a segment
        pts = enc.encode_double_vector_batch(ctx, bank[idx], SCALE)
        after = [ph.rotate(ctx, X, st, gk) for st in (1, 2, 3)]
        for j, got in enumerate(limbs_of(pts)):
            same(got, want_row[idx[j]], f"{rows}-row upload: plaintext {j} (limb, slot)")
        for j, got in enumerate(limbs_of(small)):
            same(got, want_row[j], f"before the {rows}-row upload: plaintext {j} (limb, slot)")
        for k, got in enumerate(limbs_of(after)):
            same(got, want_rot[k], f"after the {rows}-row upload: rotation {k}")
        if rows == SEG_ROWS:
            assert ph.staging_stats(ctx)[0] - r0 >= 2, "a whole segment, entered from mid-segment and left full"


# ---------------------------------------------------------------------------------------------- (e) queue limits
N_E, BITS_E, STEPS_E = 256, [60, 40, 40, 60], (1, 2)


@pytest.mark.parametrize("mode", ["exact", "seal"])
def test_rotation_queue_limits(ph, orc, mode):
    """The plain queue at its own limits (the batched ops have their 513-item tests, tests/test_inner_sum.py and
    tests/test_multiply_many.py; nothing else queues this many): 513 rotations of distinct inputs before any readback
    (a flush at 512 items, then one), rotations at l = 3 queued when one at l = 2 arrives, a rotation of a queued
    output, and an input destroyed while its rotation is queued."""
    seed = 98
    ctx, sk, o = make_ctx(ph, N_E, BITS_E, 1, steps=STEPS_E, seed=seed, mode=mode)
    s = o.gen_secret(seed)
    gk = sk.create_galois_keys(ctx)
    elt = {st: ph.get_elt_from_step(st, N_E) for st in STEPS_E}
    okey = {st: o.gen_galois_key(seed, s, e) for st, e in elt.items()}
    for st in STEPS_E:
        same(gk.export(elt[st]), okey[st], f"Galois key of step {st}")
    rot = lambda a, st: o.rotate_elt(a, okey[st], elt[st])
    rng = np.random.default_rng(513)
    ins = [rand_ct(o, rng, 2, 2) for _ in range(513)]
    cts = [up(ph, ctx, o, a) for a in ins]
    outs = [ph.rotate(ctx, c, 1 + (i & 1), gk) for i, c in enumerate(cts)]
    for i, got in enumerate(limbs_of(outs)):
        same(got, rot(ins[i], 1 + (i & 1)), f"513 queued rotations: input {i}")
    del outs, cts
    # a level change
    hi, lo = rand_ct(o, rng, 2, 3), rand_ct(o, rng, 2, 2)
    HI, LO = up(ph, ctx, o, hi), up(ph, ctx, o, lo)
    outs = [ph.rotate(ctx, HI, 1, gk), ph.rotate(ctx, HI, 2, gk), ph.rotate(ctx, LO, 1, gk), ph.rotate(ctx, HI, 1, gk)]
    for k, (got, w) in enumerate(zip(limbs_of(outs), [rot(hi, 1), rot(hi, 2), rot(lo, 1), rot(hi, 1)])):
        same(got, w, f"level change in the queue: rotation {k}")
    del outs
    # an input that is a queued output
    r1 = ph.rotate(ctx, HI, 1, gk)
    r2 = ph.rotate(ctx, r1, 2, gk)
    same(r2.to_numpy(), rot(rot(hi, 1), 2), "rotate(rotate(x, 1), 2) queued back to back")
    same(r1.to_numpy(), rot(hi, 1), "the queued output that was an input")
    # an input destroyed while its rotation is queued
    gone = rand_ct(o, rng, 2, 3)
    G_ = up(ph, ctx, o, gone)
    r = ph.rotate(ctx, G_, 2, gk)
    del G_
    gc.collect()
    filler = up(ph, ctx, o, hi)      # takes the destroyed input's block from the cache and overwrites it
    same(r.to_numpy(), rot(gone, 2), "input destroyed while queued")
    same(filler.to_numpy(), hi, "the block's next owner")


# ---------------------------------------------------------------------------------------------- (f) scratch growth
@pytest.mark.parametrize("cap", [None, 0], ids=["default-cap", "cap-0"])
def test_keyswitch_workspace_grows_under_a_queued_flush(ph, plan, monkeypatch, cap):
    """Ring (a): a 3-rotation flush at l = 2, a flush of 43 distinct inputs at l = 6 (the grow-only SCR_KS slot is
    outgrown while the small flush is only queued: the old workspace goes to the cache, or with
    FHESPEAR_CACHE_BYTES=0 straight back to the device), then the 3-rotation flush again in the grown workspace.
    Nothing is read before all three are queued."""
    if cap is None:
        monkeypatch.delenv("FHESPEAR_CACHE_BYTES", raising=False)
    else:
        monkeypatch.setenv("FHESPEAR_CACHE_BYTES", str(cap))
    ctx, sk, gk, rlk = walk_ctx(ph, plan)
    o = plan.o
    rng = np.random.default_rng(43)
    small = rand_ct(o, rng, 2, 2)
    big = [rand_ct(o, rng, 2, 6) for _ in range(43)]
    S, B = up(ph, ctx, o, small), [up(ph, ctx, o, b) for b in big]
    ev0 = ctx.debug_alloc_stats()["evicted"]
    first = [ph.rotate(ctx, S, st, gk) for st in ROT3]
    outs = [ph.rotate(ctx, c, ROT3[i % 3], gk) for i, c in enumerate(B)]          # its first rotation flushes `first`
    again = [ph.rotate(ctx, S, st, gk) for st in ROT3]                            # ... and this one the 43
    ctx.debug_alloc_stats()                                                       # (reads counters, flushes nothing)
    rot = lambda a, st: o.rotate_elt(a, plan.okey[st], plan.elt[st])
    for k, got in enumerate(limbs_of(again)):                                     # the entry flushes `again`
        same(got, rot(small, ROT3[k]), f"3 rotations at l=2 after the growth: step {ROT3[k]}")
    for k, got in enumerate(limbs_of(first)):
        same(got, rot(small, ROT3[k]), f"3 rotations at l=2 before the growth: step {ROT3[k]}")
    for i, got in enumerate(limbs_of(outs)):
        same(got, rot(big[i], ROT3[i % 3]), f"43 inputs at l=6: input {i}")
    st = ctx.debug_alloc_stats()
    if cap == 0:
        assert st["cache_cap"] == 0 and st["cached_bytes"] == 0 and st["evicted"] > ev0, st
    else:
        assert st["evicted"] == 0 and st["cached_bytes"] > 0, st
