"""The batched ops (pyPhantom.inner_sum_many, multiply_relin_many / square_many, weighted_sums) at every ring from
N = 2048 to 32768 and on both sides of every launch-form threshold their batch size crosses.

None of the three added a kernel name: each drives the per-ring kernels through argument paths of its own --
KsItem::add0i in every ModDown form, the device pointer list of k_rescale_intt, launch_rescale over ocomp R
components straight into a results block, a key switch with U = R = n distinct inputs -- and which instantiation
runs depends on workgroup counts that grow with the batch.  Their own files stay at N <= 1024 with n <= 9 (and one
n = 1 inner sum at N = 32768), i.e. on one side of every threshold.

The judge is the one of those files: np.array_equal against the CPU oracle's own per-op loop, on random residues
uploaded with ciphertext_from_numpy; every case also asserts chain index, scale and size, and that no input was
written.  The Env, the loops and the constant rounding are imported from them.  A case that claims a launch form
arms the launch ledger around the call and asserts the named kernel was launched and the other form of the pair was
not (names as in tests/golden/kernel_manifest.json) -- without that it would pass on the wrong form.

Chains: X59 = [59]*9, P = 3 (the launch matrix's); A = [60, 40, 40, 60], P = 1, exact and SEAL convention;
FRI = [60] + [40]*9 + [60], P = 1, the reference inference's, at the levels where it calls these ops.
Every test here needs an MI355X: -m gpu."""
import json
from pathlib import Path

import numpy as np
import pytest

import test_inner_sum as _is
import test_multiply_many as _mm
import test_weighted_sums as _ws

pytestmark = pytest.mark.gpu

SCALE = _is.SCALE
# sizes of every prime, special primes, the rotation steps the cases need
CHAINS = {"X59": ([59] * 9, 3, (1, 2)), "A": ([60, 40, 40, 60], 1, (1, 2)), "FRI": ([60] + [40] * 9 + [60], 1, (32, 64, 128))}
RINGS = (2048, 4096, 8192, 16384, 32768)
# (chain, key-switch convention, levels): X59 at l = 6 (X-form ModUp, l % 3 == 0) and l = 5 (count form)
SWEEP = [("X59", "exact", (6, 5)), ("A", "exact", (3,)), ("A", "seal", (3,))]
SWEEP_IDS = ["X59", "A-exact", "A-seal"]
# the launchers' own constants (fhs_kernels.hip)
FULL_FORM_MAX_WG = 256      # FHS_FULL_FORM_MAX_WG: FHS_NTT_LAUNCH and ks_intt_stage take the half-limb form from here
SPLIT_MAX_WG = 256          # FHS_SPLIT_MAX_WG: ks_moddown_stage takes SPLIT at N = 32768 below it
PERM_BATCH = 32             # kPermBatch: polynomials per k_galois_perm_batch launch
MANIFEST = set(json.loads((Path(__file__).resolve().parent / "golden" / "kernel_manifest.json").read_text())["kernels"])


@pytest.fixture(scope="module")
def ph(require_gpu):
    import pyPhantom
    return pyPhantom


class Env(_is.Env):
    """test_inner_sum's Env (context, Galois keys, oracle; its check() is the inner-sum judge) with a relinearization
    key on both sides and test_multiply_many's loop and judge next to it.  The oracle's inner sums are kept per input
    array, so the two sides of a threshold share one reference."""

    def __init__(self, ph, orc, N, chain, mode):
        bits, P, steps = CHAINS[chain]
        super().__init__(ph, orc, N, bits, P, mode, steps=list(steps))
        self.rk = self.sk.gen_relinkey(self.ctx)
        self.rlk = self.o.gen_relin_key(_is.SEED, self.s)
        self._sums = {}

    out_scale = _mm.Env.out_scale
    product = _mm.Env.want
    check_products = _mm.Env.check

    def want(self, x, dim, stride=1):
        key = (id(x), dim, stride)
        if key not in self._sums:
            self._sums[key] = (x, super().want(x, dim, stride))   # x is held: its id stays its own
        return self._sums[key][1]


_ENVS = {}
_DATA = {}


@pytest.fixture(scope="module")
def env(ph, orc):
    """One context per (ring, chain, convention), shared by the module."""
    def get(N, chain, mode="exact"):
        key = (N, chain, mode)
        if key not in _ENVS:
            _ENVS[key] = Env(ph, orc, N, chain, mode)
        return _ENVS[key]
    yield get
    _ENVS.clear()
    _DATA.clear()


def shared(key, make):
    """Inputs and references that two cases share, made once and never written."""
    if key not in _DATA:
        _DATA[key] = make()
    return _DATA[key]


def armed(ph, call, launched=(), absent=()):
    """Run `call` with the launch ledger armed: every kernel of `launched` is in the ledger, none of `absent` is."""
    assert set(launched) | set(absent) <= MANIFEST, sorted((set(launched) | set(absent)) - MANIFEST)
    ph.debug_launch_ledger("arm")
    try:
        out = call()
    finally:
        ph.debug_launch_ledger("disarm")
    ledger = set(ph.debug_launch_ledger("read"))
    missing, wrong = sorted(set(launched) - ledger), sorted(set(absent) & ledger)
    assert not missing and not wrong, f"not launched: {missing}; launched, but the other form was claimed: {wrong}"
    return out


def products(e, xs, ys, l, what, relin=True, rescale=True, launched=(), absent=(), wants=None):
    """multiply_relin_many on the pairs (xs[i], ys[i]), square_many when ys is None, against the oracle's three calls
    per pair."""
    ph = e.ph
    A = [e.up(x) for x in xs]
    B = None if ys is None else [e.up(y) for y in ys]
    rk = e.rk if relin else None
    if B is None:
        got = armed(ph, lambda: ph.square_many(e.ctx, A, rk, rescale=rescale), launched, absent)
    else:
        got = armed(ph, lambda: ph.multiply_relin_many(e.ctx, A, B, rk, rescale=rescale), launched, absent)
    if wants is None:
        wants = [e.product(x, x if ys is None else ys[i], relin, rescale) for i, x in enumerate(xs)]
    e.check_products(got, wants, l, what, 2 if relin else 3, rescale)
    for c, x in zip(A + (B or []), list(xs) + list(ys or [])):
        assert np.array_equal(c.to_numpy(), x), f"{what}: an input was written"


def weighted(e, xs, W, l, what, launched=(), absent=()):
    """weighted_sums against the oracle's loop of multiply_plain, rescale and add per term."""
    X = [e.up(x) for x in xs]
    got = armed(e.ph, lambda: e.ph.weighted_sums(e.ctx, X, W, SCALE), launched, absent)
    _ws.check(e, got, _ws.oracle_loop(e, xs, W, l), l, what)
    for c, x in zip(X, xs):
        assert np.array_equal(c.to_numpy(), x), f"{what}: an input was written"


def sweep_weights(rng, F, E):
    """test_weighted_sums' weights: random ones with a negative, 0 and +-2^-40 (constants +-1) among them."""
    W = _ws.weights(rng, F, E)
    consts = {_ws.const_of(w) for w in W.reshape(-1)}
    assert (W < 0).any() and {0, 1, -1} <= consts and 2.0 ** -40 in W and -(2.0 ** -40) in W
    return W


# ------------------------------------------------------------------------------------------------ 1. ring sweep
@pytest.mark.parametrize("chain,mode,levels", SWEEP, ids=SWEEP_IDS)
@pytest.mark.parametrize("N", RINGS)
def test_ring_inner_sum(env, N, chain, mode, levels):
    """n = 3, dim = 4 (steps 1 and 2: the second step reads the first one's block)."""
    e = env(N, chain, mode)
    for l in levels:
        rng = np.random.default_rng(N + l)
        e.check([e.rand(rng, l) for _ in range(3)], 4, what=f"N={N} {chain} {mode} l={l}")


@pytest.mark.parametrize("chain,mode,levels", SWEEP, ids=SWEEP_IDS)
@pytest.mark.parametrize("N", RINGS)
def test_ring_multiply_relin(env, N, chain, mode, levels):
    """3 distinct pairs and 2 squares with key and rescale; on X59 at l = 6 also with the key and no rescale (the key
    switch writes the results) and with rescale and no key (3 components per pair through launch_rescale)."""
    e = env(N, chain, mode)
    for l in levels:
        rng = np.random.default_rng(N + 10 * l)
        xs, ys = [e.rand(rng, l) for _ in range(3)], [e.rand(rng, l) for _ in range(3)]
        what = f"N={N} {chain} {mode} l={l}"
        products(e, xs, ys, l, what + " pairs")
        products(e, xs[:2], None, l, what + " squares")
        if chain == "X59" and l == 6:
            products(e, xs, ys, l, what + " key, no rescale", rescale=False)
            products(e, xs, ys, l, what + " rescale, no key", relin=False)


@pytest.mark.parametrize("chain,mode,levels", SWEEP, ids=SWEEP_IDS)
@pytest.mark.parametrize("N", RINGS)
def test_ring_weighted_sums(env, N, chain, mode, levels):
    """(F, E) = (3, 5): one full tile of outputs and a tile remainder; a negative weight, 0 and +-2^-40 among them."""
    e = env(N, chain, mode)
    for l in levels:
        rng = np.random.default_rng(N + 100 * l)
        weighted(e, [e.rand(rng, l) for _ in range(3)], sweep_weights(rng, 3, 5), l, f"N={N} {chain} {mode} l={l}")


# ------------------------------------------------------------------------------------------------ 2. thresholds
def _inner_sum_side(e, l, n, nmax, launched=(), absent=()):
    """One step (dim = 2) over the first n of nmax shared inputs."""
    xs = shared(("inner", e.N, l, nmax), lambda: [e.rand(np.random.default_rng(e.N + nmax + i), l) for i in range(nmax)])
    armed(e.ph, lambda: e.check(xs[:n], 2, what=f"N={e.N} l={l} n={n}"), launched, absent)


SPLIT, NOSPLIT = "k_moddown_h<15, true, true, true>", "k_moddown_h<15, true, true, false>"


@pytest.mark.parametrize("n", [42, 43])
def test_inner_sum_at_n32768_on_both_sides_of_the_split_moddown(env, n):
    """N = 32768, X59, l = 3: l 2 R = 252 workgroups take k_moddown_h's SPLIT form, 258 the plain one -- the one 64
    FFN columns run -- and both add x0 and x1 (KsItem::add0i, add1) to what they write."""
    l = 3
    below = l * 2 * n < SPLIT_MAX_WG
    assert below == (n == 42)
    _inner_sum_side(env(32768, "X59"), l, n, 43, [SPLIT if below else NOSPLIT], [NOSPLIT if below else SPLIT])


@pytest.mark.parametrize("n", [42, 43])
def test_inner_sum_at_n16384_on_both_sides_of_the_half_limb_intts(env, n):
    """N = 16384, X59, l = 6: l U = P 2 R = 252 workgroups take the full-limb k_ks_intt<14> and
    k_ks_special_intt<14, false>, 258 the half-limb forms."""
    l, P = 6, 3
    below = l * n < FULL_FORM_MAX_WG
    assert below == (P * 2 * n < FULL_FORM_MAX_WG) == (n == 42)
    full, half = ["k_ks_intt<14>", "k_ks_special_intt<14, false>"], ["k_ks_intt_h<14>", "k_ks_special_intt<14, true>"]
    _inner_sum_side(env(16384, "X59"), l, n, 43, full if below else half, half if below else full)


@pytest.mark.parametrize("n", [16, 17])
def test_seal_inner_sum_on_both_sides_of_one_permutation_launch(env, n):
    """N = 1024, A in the SEAL convention, l = 3: an item permutes 2 polynomials (its input and the c0 that the
    ModDown adds), so 16 items fill one k_galois_perm_batch launch and the 17th opens a second one.  No name flips:
    judged by values alone, with the kernel in the ledger."""
    assert (2 * n <= PERM_BATCH) == (n == 16)
    _inner_sum_side(env(1024, "A", "seal"), 3, n, 17, ["k_galois_perm_batch"])


def _pairs_16384(e):
    def make():
        xs = [e.rand(np.random.default_rng(16384 + i), 2) for i in range(129)]
        return xs, [e.product(xs[i], xs[i + 1]) for i in range(128)]
    return shared("pairs 16384", make)


def multiply_128_pairs_at_n16384(e, n):
    """The case of the next test, also run by the launch-coverage matrix (n = 128): pair i is (x_i, x_{i+1})."""
    l = 2
    below = 2 * n < FULL_FORM_MAX_WG
    assert below == ((l - 1) * 2 * n < FULL_FORM_MAX_WG) == (l * n < FULL_FORM_MAX_WG) == (n < 128)
    full = ["k_rescale_intt<14, false>", "k_rescale_ntt<14, false>", "k_ks_intt<14>", "k_ks_special_intt<14, false>"]
    half = ["k_rescale_intt<14, true>", "k_rescale_ntt<14, true>", "k_ks_intt_h<14>", "k_ks_special_intt<14, true>"]
    xs, wants = _pairs_16384(e)
    products(e, xs[:n], xs[1:n + 1], l, f"N=16384 A l=2 n={n}", launched=full if below else half,
             absent=half if below else full, wants=wants[:n])


@pytest.mark.parametrize("n", [127, 128])
def test_multiply_relin_at_n16384_on_both_sides_of_the_half_limb_rescale(env, n):
    """N = 16384, A, l = 2: the rescale of 2 R components is 2 R workgroups in either launch -- 254 take
    k_rescale_intt<14, false> and k_rescale_ntt<14, false>, 256 the half-limb forms, writing a 128-item block; the key
    switch's l R = P 2 R = 254 / 256 workgroups flip its two INTTs at the same n."""
    multiply_128_pairs_at_n16384(env(16384, "A"), n)


HS = ["k_rescale_intt_hs<15>", "k_rescale_ntt_hs<15>"]
GENERIC = ["k_rescale_intt<15, true>", "k_rescale_ntt<15, true>"]


@pytest.mark.parametrize("n,relin", [(1, True), (2, True), (1, False)])
def test_multiply_relin_at_n32768_on_both_sides_of_the_two_component_rescale(env, n, relin):
    """N = 32768, X59, l = 3: launch_rescale takes the k_rescale_*_hs pair for ncomp <= 2 only -- one relinearized
    pair; two pairs (ncomp = 4) and one pair without the key (ncomp = 3) take the generic half-limb pair."""
    e = env(32768, "X59")
    ncomp = (2 if relin else 3) * n
    assert (ncomp <= 2) == (n == 1 and relin)
    rng = np.random.default_rng(32768 + ncomp)
    xs, ys = [e.rand(rng, 3) for _ in range(n)], [e.rand(rng, 3) for _ in range(n)]
    products(e, xs, ys, 3, f"N=32768 X59 l=3 n={n} relin={relin}", relin=relin,
             launched=HS if ncomp <= 2 else GENERIC, absent=GENERIC if ncomp <= 2 else HS)


@pytest.mark.parametrize("F", [127, 128])
def test_weighted_sums_at_n16384_on_both_sides_of_the_half_limb_pointer_list_intt(env, F):
    """N = 16384, A, l = 2, E = 1: the last limbs of F inputs go to coefficient form in one k_rescale_intt launch of
    2 F workgroups over the device pointer list -- 254 take K<14, false>, 256 K<14, true>."""
    e = env(16384, "A")
    below = 2 * F < FULL_FORM_MAX_WG
    assert below == (F == 127)
    xs = shared("wsum 16384", lambda: [e.rand(np.random.default_rng(3 * 16384 + i), 2) for i in range(128)])
    full, half = ["k_rescale_intt<14, false>"], ["k_rescale_intt<14, true>"]
    weighted(e, xs[:F], sweep_weights(np.random.default_rng(F), F, 1), 2, f"N=16384 A l=2 F={F}",
             full if below else half, half if below else full)


# ------------------------------------------------------------------------------------------------ 3. production chain
FRI_LEVELS = [("exact", 9), ("exact", 8), ("seal", 9)]      # chain index 2 and 3: where the reference calls these ops


@pytest.mark.parametrize("mode,l", FRI_LEVELS)
def test_fri_chain_inner_sum(env, mode, l):
    """N = 32768 on the reference inference's chain: n = 2, dim = 8, stride 32 (steps 32, 64, 128), limb by limb."""
    e = env(32768, "FRI", mode)
    assert e.L0 + 1 - l in (2, 3)
    rng = np.random.default_rng(l)
    e.check([e.rand(rng, l) for _ in range(2)], 8, 32, what=f"FRI {mode} l={l}")


@pytest.mark.parametrize("mode,l", FRI_LEVELS)
def test_fri_chain_squares(env, mode, l):
    e = env(32768, "FRI", mode)
    rng = np.random.default_rng(10 + l)
    products(e, [e.rand(rng, l) for _ in range(2)], None, l, f"FRI {mode} l={l} squares")


def test_fri_chain_weighted_sums(env):
    """(F, E) = (5, 3) at l = 8 (chain index 3)."""
    e = env(32768, "FRI")
    rng = np.random.default_rng(58)
    weighted(e, [e.rand(rng, 8) for _ in range(5)], sweep_weights(rng, 5, 3), 8, "FRI l=8")
