// fhs_tables.h -- host-only derivation of a context's parameter tables: the host number theory, the
// coefficient-modulus search, argument validation for fhs_context_create and fhs_inner_sum_many (with its step
// list: tools/debug/inner_sum_check.cpp), fhs_multiply_relin_many (with its chunk plan:
// tools/debug/multiply_many_check.cpp), fhs_multiply_plain_rescale_many (with its chunk plan:
// tools/debug/mulp_rescale_check.cpp) and fhs_weighted_sums (with its weight tables and chunk plan:
// tools/debug/weighted_sums_check.cpp), every table DevTables points
// to (as std::vectors, HostTables) and the constants of the decoder's CRT composition.  No HIP runtime
// call: fhs_host.hip uploads what build_host_tables returns, and tools/debug/tables_check.cpp checks the
// same tables with plain g++ (through tools/debug/shim) under the host sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "fhs_modarith.h"

typedef unsigned __int128 hu128;

// ============================================================================ host number theory
static inline uint64_t h_mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)(((hu128)a * b) % q); }
static uint64_t h_pow(uint64_t b, uint64_t e, uint64_t q) {
    uint64_t r = 1 % q;
    b %= q;
    while (e) {
        if (e & 1) r = h_mulmod(r, b, q);
        b = h_mulmod(b, b, q);
        e >>= 1;
    }
    return r;
}
static uint64_t h_inv(uint64_t a, uint64_t q) { return h_pow(a % q, q - 2, q); }
static uint64_t h_shoup(uint64_t w, uint64_t q) { return (uint64_t)(((hu128)w << 64) / q); }
// floor((2^128 - 1) / q): the Barrett / centred-count constant (= floor(2^128 / q) for every odd q > 1)
static hu128 h_floor128(uint64_t q) { return (~(hu128)0) / q; }
// product of primes[s0 .. s0 + ns) except index s0 + skip (skip < 0: of all of them), mod m
static uint64_t h_prod_except(const uint64_t* primes, int s0, int ns, int skip, uint64_t m) {
    uint64_t h = 1;
    for (int v = 0; v < ns; ++v)
        if (v != skip) h = h_mulmod(h, primes[s0 + v] % m, m);
    return h;
}

// q = 2^b - d qualifies for pm_reduce128 (fhs_modarith.h) when its three folds provably take
// every 128-bit input below 2q: B_{k+1} = (B_k >> b) d + 2^b - 1 from B_0 = 2^128 - 1, with the
// fold-2 quotient < 2^64 and the fold-3 quotient < 2^32.  Returns the PrimeK.pm word or 0.
static uint64_t pm_word(uint64_t q, int logN) {
    int b = 64 - __builtin_clzll(q);
    if (b < 40 || b > 62) return 0;
    const uint64_t d = (1ull << b) - q;
    if (d >= (1ull << 32)) return 0;
    const hu128 lim = ((hu128)1 << b) - 1;
    const hu128 B0 = ~(hu128)0;
    const hu128 h1 = B0 >> b;                       // < 2^88: product with d may overflow -> check
    if ((h1 >> 96) != 0) return 0;
    const hu128 B1 = h1 * d + lim;                  // h1 < 2^96, d < 2^32 -> < 2^128
    if (B1 < h1 * d) return 0;
    const hu128 h2 = B1 >> b;
    if ((h2 >> 64) != 0) return 0;
    const hu128 B2 = h2 * d + lim;
    const hu128 h3 = B2 >> b;
    if ((h3 >> 32) != 0) return 0;
    const hu128 B3 = h3 * d + lim;
    if (B3 >= 2 * (hu128)q) return 0;
    const bool lazy = (hu128)q * (uint64_t)(4 + 2 * logN) < ((hu128)1 << 64);   // fhs_ntt.h LAZY bound
    return (d << 8) | (lazy ? 128u : 0u) | (uint64_t)b;
}

// A 59-bit prime q = 2^59 - d with d < 2^27: the precondition of convert3x_b59's bounds.
static bool b59_prime(uint64_t q) { return q < (1ull << 59) && (1ull << 59) - q < (1ull << 27); }
// Bit 40 of PrimeK.pm: the ModUp conversion may reduce its split-30 sums directly
// (fhs_modarith.h acc3_reduce_pm): with ns <= P source limbs (< 2^60 each) and the v (Q mod m)
// correction folded into L, every intermediate of that routine stays in its word and the result is
// below 2q.  Checked here with exact bounds for this prime.
static bool conv_pm_ok(uint64_t q, int ns) {
    const int b = 64 - __builtin_clzll(q);
    if (b < 40 || b > 60 || ns < 1 || ns > 7) return false;
    const hu128 d = ((hu128)1 << b) - q;
    const hu128 p30 = ((hu128)1 << 30) - 1, M64 = ~(hu128)0 >> 64;   // 2^64 - 1
    const hu128 Lmax = (hu128)ns * p30 * p30 + (hu128)ns * (q - 1);
    const hu128 Mmax = (hu128)2 * ns * p30 * p30, Hmax = (hu128)ns * p30 * p30;
    const int sh = b - 30;
    const hu128 Amax = Lmax + ((((hu128)1 << sh) - 1) << 30);
    const hu128 Bmax = (Mmax >> sh) + (Hmax << (60 - b));
    if (Lmax > M64 || Mmax > M64 || Amax > M64 || Bmax > M64) return false;
    if ((Bmax >> 64) != 0 || d >= ((hu128)1 << 32)) return false;
    const hu128 Smax = Amax + Bmax * d;   // < 2^96
    const hu128 Sh = Smax >> b;
    if (Sh >= ((hu128)1 << 32)) return false;
    const hu128 rmax = (((hu128)1 << b) - 1) + Sh * d;
    return rmax < 2 * (hu128)q;
}
// X form of the centred extension for full 3-limb digits (fhs_modarith.h centered_x_pack /
// convert3x_value, fhs_kernels.hip k_centered_x): per digit j (primes 3j..3j+2, j < dnum with 3j + 3 <=
// L0) the exact Q_S / q_u, the rounding thresholds ((2k - 1) Q_S + 1) / 2 and 2^179 - v Q_S (192-bit
// words, little-endian) into xd[j][32]; per prime m the base-2^60 weights 2^60, 2^120 mod m (split-30
// packed) and -2^179 mod m into xt[i][4].  |X| < Q_S / 2 < 2^179 (three primes below 2^60; < 2^176 for the
// 59-bit chain), so U = X + 2^179 lies in (0, 2^180): exactly three 60-bit words.
static void modup_xform_tables(const uint64_t* primes, int K, int L0, int dnum, uint64_t* xd, uint64_t* xt) {
    auto mul192 = [](const uint64_t a[3], uint64_t m, uint64_t r[3]) {   // r = a m mod 2^192
        hu128 cy = 0;
        for (int w = 0; w < 3; ++w) {
            const hu128 t = (hu128)a[w] * m + cy;
            r[w] = (uint64_t)t;
            cy = t >> 64;
        }
    };
    for (int j = 0; j < dnum && 3 * j + 3 <= L0; ++j) {
        const uint64_t* q3 = &primes[3 * j];
        uint64_t* d = &xd[(size_t)j * 32];
        for (int u = 0; u < 3; ++u) {
            const hu128 h = (hu128)q3[(u + 1) % 3] * q3[(u + 2) % 3];
            d[2 * u] = (uint64_t)h;
            d[2 * u + 1] = (uint64_t)(h >> 64);
        }
        const uint64_t one[3] = {1, 0, 0};
        uint64_t Q[3], t[3];
        mul192(one, q3[0], t);
        mul192(t, q3[1], Q);
        mul192(Q, q3[2], t);
        std::copy(t, t + 3, Q);
        for (int k = 1; k <= 3; ++k) {   // ((2k - 1) Q + 1) / 2: (2k - 1) Q is odd, so + 1 is carry-free
            uint64_t m[3];
            mul192(Q, (uint64_t)(2 * k - 1), m);
            m[0] += 1;
            uint64_t* th = d + 6 + 3 * (k - 1);
            th[0] = (m[0] >> 1) | (m[1] << 63);
            th[1] = (m[1] >> 1) | (m[2] << 63);
            th[2] = m[2] >> 1;
        }
        for (int v = 0; v <= 3; ++v) {   // 2^179 - v Q
            uint64_t m[3];
            mul192(Q, (uint64_t)v, m);
            uint64_t* c = d + 15 + 3 * v;
            const uint64_t top[3] = {0, 0, 1ull << (179 - 128)};
            uint64_t br = 0;
            for (int w = 0; w < 3; ++w) {
                const hu128 s = (hu128)top[w] - m[w] - br;
                c[w] = (uint64_t)s;
                br = (uint64_t)(s >> 64) ? 1 : 0;
            }
        }
    }
    for (int i = 0; i < K; ++i) {
        const uint64_t m = primes[i];
        uint64_t p60 = 1 % m;
        for (int e = 0; e < 60; ++e) p60 = h_mulmod(p60, 2, m);
        const uint64_t p120 = h_mulmod(p60, p60, m);
        uint64_t p179 = 1 % m;
        for (int e = 0; e < 179; ++e) p179 = h_mulmod(p179, 2, m);
        xt[(size_t)i * 4 + 0] = p60;   // convert3x_value takes it as one 32-bit word (< 2^30 checked by the caller)
        xt[(size_t)i * 4 + 1] = pack30(p120);
        xt[(size_t)i * 4 + 2] = p179 ? m - p179 : 0;
    }
}
static bool h_is_prime(uint64_t n) {
    if (n < 2) return false;
    const uint64_t bases[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
    for (uint64_t p : bases) {
        if (n == p) return true;
        if (n % p == 0) return false;
    }
    uint64_t d = n - 1;
    int s = 0;
    while (!(d & 1)) { d >>= 1; ++s; }
    for (uint64_t a : bases) {
        uint64_t x = h_pow(a, d, n);
        if (x == 1 || x == n - 1) continue;
        bool comp = true;
        for (int r = 1; r < s && comp; ++r) {
            x = h_mulmod(x, x, n);
            if (x == n - 1) comp = false;
        }
        if (comp) return false;
    }
    return true;
}
static uint32_t h_bitrev(uint32_t x, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
}
// minimal primitive 2N-th root of unity mod q (SEAL / Phantom convention)
static uint64_t h_min_root(uint64_t q, uint64_t N) {
    const uint64_t cof = (q - 1) / (2 * N);
    uint64_t g = 0;
    for (uint64_t c = 2;; ++c) {
        g = h_pow(c, cof, q);
        if (h_pow(g, N, q) == q - 1) break;
    }
    const uint64_t g2 = h_mulmod(g, g, q);
    uint64_t best = g, cur = g;
    for (uint64_t k = 1; k < N; ++k) {
        cur = h_mulmod(cur, g2, q);
        if (cur < best) best = cur;
    }
    return best;
}

// SEAL's CoeffModulus::Create: per bit size the largest primes = 1 mod 2N below 2^bits, handed out in the
// order asked for.  bits[i] in [2, 61] (the caller checks); false when a size has too few primes.
static bool coeff_modulus_search(uint64_t N, const int* bits, int n, uint64_t* out) {
    const uint64_t fac = 2 * N;
    std::map<int, std::vector<uint64_t>> pool;
    std::map<int, int> need, used;
    for (int i = 0; i < n; ++i) need[bits[i]]++;
    for (auto& kv : need) {
        const int b = kv.first;
        uint64_t v = ((uint64_t)1 << b) - fac + 1;
        const uint64_t lo = (uint64_t)1 << (b - 1);
        while ((int)pool[b].size() < kv.second && v > lo) {
            if (h_is_prime(v)) pool[b].push_back(v);
            v -= fac;
        }
        if ((int)pool[b].size() < kv.second) return false;
    }
    for (int i = 0; i < n; ++i) out[i] = pool[bits[i]][used[bits[i]]++];
    return true;
}

static uint64_t galois_elt_from_step(int step, uint64_t N) {
    const uint64_t m = 2 * N;
    if (step == 0) return m - 1;
    const uint64_t slots = N / 2;
    uint64_t s = step > 0 ? (uint64_t)step : slots - (uint64_t)(-(int64_t)step);
    s %= slots;
    uint64_t e = 1;
    for (uint64_t i = 0; i < s; ++i) e = (e * 5) & (m - 1);
    return e;
}
// the default Galois elements: +-2^k steps and conjugation (SEAL/Phantom create_galois_keys default)
static std::vector<uint64_t> default_galois_elts(uint64_t N) {
    std::set<uint64_t> s;
    for (uint64_t k = 1; k < N / 2; k <<= 1) {
        s.insert(galois_elt_from_step((int)k, N));
        s.insert(galois_elt_from_step(-(int)k, N));
    }
    s.insert(2 * N - 1);
    return std::vector<uint64_t>(s.begin(), s.end());
}

// Every argument of fhs_context_create but the device: the message of the first one that is wrong, or null.
static const char* context_params_error(uint64_t N, const uint64_t* primes, int nprimes, int special,
                                        const uint64_t* galois_elts, int n_elts) {
    if (!primes) return "context_create: null argument";
    if (N < 256 || N > 32768 || (N & (N - 1)))
        return "context_create: poly_modulus_degree must be a power of two in [256, 32768]";
    if (special < 1 || special >= nprimes) return "context_create: bad special modulus size";
    if ((nprimes - special) % special != 0)
        return "context_create: data primes (L0) must be a multiple of special_modulus_size (README.md:59)";
    if (special > 8) return "context_create: special_modulus_size > 8 unsupported";
    for (int i = 0; i < nprimes; ++i) {
        if (primes[i] >= (1ull << 60) || (primes[i] - 1) % (2 * N) != 0 || !h_is_prime(primes[i]))
            return "context_create: every modulus must be a prime < 2^60 (SEAL's 60-bit "
                   "limit; Acc3 in fhs_modarith.h relies on it), = 1 mod 2N";
        for (int j = 0; j < i; ++j)
            if (primes[j] == primes[i]) return "context_create: duplicate modulus";
    }
    for (int i = 0; galois_elts && i < n_elts; ++i)
        if ((galois_elts[i] & 1) == 0 || galois_elts[i] >= 2 * N) return "context_create: invalid galois element";
    return nullptr;
}

// The rotation steps of fhs_inner_sum_many over a ring of N coefficients -- the reference loop's
// (step = 1; while step < dim: rotate by stride * step; step *= 2), so a dim that is no power of two takes the steps
// below it -- into `steps` (cleared first): the message of the first argument that is wrong, or null.  dim = 1 gives
// no step.  The largest step must be a rotation fhs_rotate accepts (< N/2 slots).
static const char* inner_sum_steps(int n, int dim, int stride, uint64_t N, std::vector<int>& steps) {
    steps.clear();
    if (n < 1) return "inner_sum_many: n >= 1";
    if (dim < 1) return "inner_sum_many: dim >= 1";
    if (stride < 1) return "inner_sum_many: stride >= 1";
    const uint64_t slots = N / 2;
    for (uint64_t s = 1; s < (uint64_t)dim; s <<= 1) {
        const uint64_t step = (uint64_t)stride * s;   // < 2^31 * 2^31
        if (step >= slots) {
            steps.clear();
            return "inner_sum_many: the largest step, stride * 2^(K-1), must be < slot count";
        }
        steps.push_back((int)step);
    }
    return nullptr;
}

// The status class of the argument a batched entry's validator rejects (the host's fail_arg maps it to FHS_ERR_INVALID,
// FHS_ERR_LEVEL or FHS_ERR_SCALE); an accepted call leaves ARG_INVALID.
enum ArgErr { ARG_INVALID, ARG_LEVEL, ARG_SCALE };
// The arguments of fhs_multiply_relin_many, from what the host layer reads off the handles: n pairs, `count`
// operand entries (n for squares, 2 n for pairs: a's then b's) with their component counts and chain indices, the
// context's L0 and the rescale flag.  The message of the first argument that is wrong, or null; *cls is its class.
static const char* multiply_many_error(bool null_arg, int n, const int* ncomp, const int* ci, size_t count, int L0,
                                       int rescale, ArgErr* cls) {
    *cls = ARG_INVALID;
    if (null_arg) return "null argument";
    if (n < 1) return "multiply_relin_many: n >= 1";
    if (!ncomp || !ci || count < (size_t)n) return "null argument";
    for (size_t k = 0; k < count; ++k)
        if (ncomp[k] != 2) return "multiply expects 2-component ciphertexts";
    *cls = ARG_LEVEL;
    for (size_t k = 1; k < count; ++k)
        if (ci[k] != ci[0]) return "multiply_relin_many: inputs must share one chain index";
    if (ci[0] < 1 || ci[0] > L0) return "chain index out of range";
    if (rescale && L0 + 1 - ci[0] < 2) return "rescale_to_next: no level left (end of modulus switching chain)";
    *cls = ARG_INVALID;
    return nullptr;
}
// The item buffer of a key-switch launch (fhs_context::kMaxItems) and the scratch a chunk of fhs_multiply_relin_many
// may ask for.  That scratch -- key-switch workspace, tensor products, relinearized pairs, the rescale's last limbs
// -- lives in the context's grow-only slots, held for its life, so the cap is what a long-lived context pays for
// having used the entry once: 1 GiB, the cap fhs_inner_sum_many already puts on the same key-switch slot (a context
// that ran one holds little more after the other), under 0.4 % of the MI355X's HBM.  At fri's ring (N = 32768, l = 9,
// P = 1) an item costs 31.7 + 7.1 + 4.7 MB = 43.5 MB, so a chunk is at most 24 pairs however many columns there
// are: 6912 workgroups of k_tensor and 7680 of k_ks_ip per launch, tens per CU -- a larger chunk would add scratch
// but no parallelism, and a thousand columns ask for 1 GiB, not 43 GB.
constexpr int kKsMaxItems = 512;
constexpr size_t kMulManyCap = (size_t)1 << 30;
// The chunks of a batch of n items whose scratch costs item_bytes each: (first item, item count) per chunk, in
// order, covering [0, n) once.  The fewest chunks with none above max_items items or cap_bytes of scratch (a single
// item is always allowed: it cannot be split), sized within one of each other, the larger ones first.
static std::vector<std::pair<int, int>> batch_chunks(int n, size_t item_bytes, int max_items, size_t cap_bytes) {
    std::vector<std::pair<int, int>> chunks;
    if (n < 1) return chunks;
    size_t rmax = item_bytes ? cap_bytes / item_bytes : (size_t)n;
    if (max_items >= 1 && rmax > (size_t)max_items) rmax = (size_t)max_items;
    if (rmax < 1) rmax = 1;
    const size_t count = ((size_t)n + rmax - 1) / rmax, base = (size_t)n / count, rem = (size_t)n % count;
    size_t at = 0;
    for (size_t k = 0; k < count; ++k) {
        const size_t r = base + (k < rem ? 1 : 0);
        chunks.emplace_back((int)at, (int)r);
        at += r;
    }
    return chunks;
}

// ============================================================================ fhs_multiply_plain_rescale_many (host side)
// The arguments of fhs_multiply_plain_rescale_many, from what the host layer reads off the handles: the n
// ciphertexts' component counts and chain indices and (pci non-null: the call has plaintexts) the n plaintexts' chain
// indices.  The message of the first argument that is wrong, or null; *cls is its class.
static const char* mulp_rescale_many_error(bool null_arg, int n, const int* ncomp, const int* ci, const int* pci, int L0,
                                           ArgErr* cls) {
    *cls = ARG_INVALID;
    if (null_arg) return "null argument";
    if (n < 1) return "multiply_plain_rescale_many: n >= 1";
    if (!ncomp || !ci) return "null argument";
    for (int k = 0; k < n; ++k)
        if (ncomp[k] != 2) return "multiply_plain_rescale_many expects 2-component ciphertexts";
    *cls = ARG_LEVEL;
    for (int k = 1; k < n; ++k)
        if (ci[k] != ci[0]) return "multiply_plain_rescale_many: inputs must share one chain index";
    for (int k = 0; pci && k < n; ++k)
        if (pci[k] != ci[0]) return "ciphertext and plaintext are at different chain indices";
    if (ci[0] < 1 || ci[0] > L0) return "chain index out of range";
    if (L0 + 1 - ci[0] < 2) return "rescale_to_next: no level left (end of modulus switching chain)";
    *cls = ARG_INVALID;
    return nullptr;
}
// The chunks of one call over n items at ring size N.  An item is one (ciphertext, plaintext) pair: two staged device
// pointers, two workgroups of the rescale's first launch and 2 (l - 1) of its second (grid.y = 2 items), and the two
// components' last limbs in coefficient form, 16 N bytes of the grow-only rescale scratch (8 MB per 16 columns at
// N = 32768; the cap kMulManyCap is never the bound below N = 2^17).  So a chunk is bound by the item buffer's length
// (the batch bound of every batched entry), by the staged pointer buffer and by the grid limit; the first is the
// tightest today and all three are stated so that none is assumed.
constexpr int kStagedMaxPtrs = 1 << 16;   // the context's staged pointer buffer holds 2 x this many pointers
constexpr int kGridMaxY = 65535;
constexpr int kMulpRescaleMaxItems = std::min(kKsMaxItems, std::min(kStagedMaxPtrs, kGridMaxY / 2));
static size_t mulp_rescale_item_bytes(size_t N) { return 16 * N; }
static std::vector<std::pair<int, int>> mulp_rescale_chunks(int n, size_t N, size_t cap = kMulManyCap) {
    return batch_chunks(n, mulp_rescale_item_bytes(N), kMulpRescaleMaxItems, cap);
}

// ============================================================================ fhs_weighted_sums (host side)
// Two scales are one scale when they agree to 1e-9 relative (fhs_add's judgement).
static bool scales_close(double a, double b) { return std::fabs(a - b) <= 1e-9 * std::max(std::fabs(a), std::fabs(b)); }
constexpr int kWsumMaxF = 4096;               // inputs per call: the rounding sum stays below 2^72 (wsum_round_term)
constexpr int kWsumMaxOutputs = kKsMaxItems;  // outputs per chunk
// The arguments of fhs_weighted_sums, from what the host layer reads off the F handles (component counts, chain
// indices, scales).  The message of the first argument that is wrong, or null; *cls is its status class.
static const char* weighted_sums_error(bool null_arg, int F, int E, int64_t ldw, double scale, const int* ncomp,
                                       const int* ci, const double* scales, int L0, ArgErr* cls) {
    *cls = ARG_INVALID;
    if (null_arg) return "null argument";
    if (F < 1 || F > kWsumMaxF) return "weighted_sums: 1 <= F <= 4096";
    if (E < 1) return "weighted_sums: E >= 1";
    if (ldw < (int64_t)E) return "weighted_sums: ldw >= E";
    if (!(scale > 0) || !std::isfinite(scale)) return "weighted_sums: bad scale";
    if (!ncomp || !ci || !scales) return "null argument";
    for (int j = 0; j < F; ++j)
        if (ncomp[j] != 2) return "weighted_sums expects 2-component ciphertexts";
    *cls = ARG_LEVEL;
    for (int j = 1; j < F; ++j)
        if (ci[j] != ci[0]) return "weighted_sums: inputs must share one chain index";
    if (ci[0] < 1 || ci[0] > L0) return "chain index out of range";
    if (L0 + 1 - ci[0] < 2) return "rescale_to_next: no level left (end of modulus switching chain)";
    *cls = ARG_SCALE;
    for (int j = 1; j < F; ++j)
        if (!scales_close(scales[j], scales[0])) return "scale mismatch";
    *cls = ARG_INVALID;
    return nullptr;
}
// The weight tables of one call at l limbs (L = l - 1, the limb the rescale drops): the plaintext of (output i, input j)
// is the constant c_ij = round(W[j ldw + i] scale), half away from zero as fhs_multiply_const rounds, k_ijm = c_ij mod q_m.
//   wl [2][F][Epad]      k_ijL and its Shoup word                              (the rounding sum's weights)
//   wt [L][F + 1][Epad]  pack30(k_ijm inv_m mod q_m), inv_m = q_L^-1 mod q_m;  row F: pack30(q_m - inv_m), the weight
//                        of the NTT'd rounding sum
// Rows are Epad = E rounded up to the tile, plus one tile, words long (a chunk may start inside a tile; the padding
// is zero).  Returns an error message (a weight not finite, or |c_ij| >= 2^62), or null.
struct WsumTables {
    int Epad = 0;
    std::vector<uint64_t> wl, wt;
};
static const char* weighted_sums_tables(const double* W, int64_t ldw, int F, int E, double scale, const uint64_t* q, int l,
                                        int tile, WsumTables& Wt) {
    const int L = l - 1;
    const size_t Epad = Wt.Epad = (E + tile - 1) / tile * tile + tile;
    Wt.wl.assign((size_t)2 * F * Epad, 0);
    Wt.wt.assign((size_t)L * (F + 1) * Epad, 0);
    const uint64_t qL = q[L];
    std::vector<uint64_t> inv(L), inv_s(L);
    for (int m = 0; m < L; ++m) {
        inv[m] = h_inv(qL % q[m], q[m]);
        inv_s[m] = h_shoup(inv[m], q[m]);
        for (int i = 0; i < E; ++i) Wt.wt[((size_t)m * (F + 1) + F) * Epad + i] = pack30(q[m] - inv[m]);
    }
    for (int j = 0; j < F; ++j)
        for (int i = 0; i < E; ++i) {
            const double p = std::round(W[(size_t)j * ldw + i] * scale);
            if (!std::isfinite(p)) return "weighted_sums: a weight is not finite";
            if (!(std::fabs(p) < 4611686018427387904.0)) return "weighted_sums: |weight x scale| >= 2^62";
            const int64_t c = (int64_t)p;
            const uint64_t mag = c < 0 ? (uint64_t)0 - (uint64_t)c : (uint64_t)c;
            auto res = [&](uint64_t m) {
                const uint64_t r = mag % m;
                return c < 0 && r ? m - r : r;
            };
            const uint64_t kL = res(qL);
            Wt.wl[(size_t)j * Epad + i] = kL;
            Wt.wl[((size_t)F + j) * Epad + i] = h_shoup(kL, qL);
            for (int m = 0; m < L; ++m)
                Wt.wt[((size_t)m * (F + 1) + j) * Epad + i] = pack30(shoup_hd(res(q[m]), inv[m], inv_s[m], q[m]));
        }
    return nullptr;
}
// The chunks over the E outputs: per output the rounding sums (2 components x 2 words per coefficient) and their NTT'd
// residues (2 (l - 1) N words); once per call the inputs' coefficient-form last limbs (2 F N words), which come off
// the cap (kMulManyCap, as fhs_multiply_relin_many).  At fri's ring (N = 32768, l = 9, F = 256) that is 5.2 MB per
// output and 134 MB once: a chunk is at most 179 outputs.
static size_t weighted_sums_item_bytes(size_t N, int l) { return 8 * N * (4 + 2 * (size_t)(l - 1)); }
static std::vector<std::pair<int, int>> weighted_sums_chunks(int E, int F, size_t N, int l, size_t cap = kMulManyCap) {
    const size_t fixed = 16 * (size_t)F * N;
    return batch_chunks(E, weighted_sums_item_bytes(N, l), kWsumMaxOutputs, cap > fixed ? cap - fixed : 0);
}

// ============================================================================ parameter tables
// One vector per DevTables pointer (fhs_kernels.h; each builder below restates its table's layout), the
// dispatch flags DevTables carries, and the host encoder / decoder tables the context keeps.
struct HostTables {
    int N = 0, logN = 0, L0 = 0, P = 0, K = 0, dnum = 0;
    std::vector<PrimeK> primes;
    std::vector<uint64_t> tw_fwd, tw_inv, modup_intt, modup_hat, modup_R, modup_Q, modup_xd, modup_xt, md_xd, md_intt,
        md_hat, md_pinv, rescale, pow2;
    std::vector<double> enc_w, enc_twist, dec_w;
    std::vector<unsigned> enc_pos, dec_pos;
    int max_qbits = 0, modup_dp = 0, md_xform = 0, conv_b59 = 0, all_b59 = 0;
    std::vector<std::complex<double>> fft_w;       // exp(2 pi i k / N), k < N
    std::vector<std::complex<double>> dec_twist;   // (cos, sin)(pi k / N), k < N; DevTables.dec_twist is its first half
    std::vector<uint64_t> slot_index;          // (5^j mod 2N - 1)/2, j < N/2
};

// primes: PrimeK[K].  tw_fwd / tw_inv: [K][N][2] = psi^rev(k) / psi^-rev(k) and its Shoup companion.
static void build_prime_tables(const uint64_t* primes, HostTables& H) {
    const size_t N = (size_t)H.N;
    H.primes.resize(H.K);
    H.tw_fwd.assign((size_t)H.K * N * 2, 0);
    H.tw_inv.assign((size_t)H.K * N * 2, 0);
    for (int i = 0; i < H.K; ++i) {
        const uint64_t q = primes[i];
        uint64_t* twf = &H.tw_fwd[(size_t)i * N * 2];
        uint64_t* twi = &H.tw_inv[(size_t)i * N * 2];
        const hu128 r = h_floor128(q);
        const uint64_t psi = h_min_root(q, N), ipsi = h_inv(psi, q);
        uint64_t pw = 1, ipw = 1;
        for (size_t k = 0; k < N; ++k) {
            const uint32_t rv = h_bitrev((uint32_t)k, H.logN);
            twf[(size_t)rv * 2] = pw;
            twi[(size_t)rv * 2] = ipw;
            pw = h_mulmod(pw, psi, q);
            ipw = h_mulmod(ipw, ipsi, q);
        }
        for (size_t k = 0; k < N; ++k) {
            twf[k * 2 + 1] = h_shoup(twf[k * 2], q);
            twi[k * 2 + 1] = h_shoup(twi[k * 2], q);
        }
        const uint64_t ninv = h_inv(N % q, q);
        const uint64_t w1n = h_mulmod(twi[2], ninv, q);
        const uint64_t pm = pm_word(q, H.logN);
        H.primes[i] = PrimeK{q, (uint64_t)r, (uint64_t)(r >> 64), ninv, h_shoup(ninv, q), w1n, h_shoup(w1n, q),
                             pm | (pm && conv_pm_ok(q, H.P) ? (1ull << 40) : 0ull)};
    }
}

// ModUp, per level l and digit j covering primes [s0, s0 + ns) = [jP, min(jP + P, l)), u < ns, t < K:
//   modup_intt [L0+1][L0][4]       at (l, i = s0 + u): N^-1 inv_hat, psi_rev_inv[1] N^-1 inv_hat mod q_i, each + Shoup
//   modup_hat  [L0+1][dnum][P][K]  (Q_S / q_u) mod prime(t)
//   modup_R    [L0+1][dnum][P][2]  floor(2^128 / q_u), low and high word
//   modup_Q    [L0+1][dnum][K][2]  Q_S mod prime(t), ns Q_S mod prime(t)
//   modup_xd [dnum][32], modup_xt [K][4]: modup_xform_tables (P = 3), else zero
static void build_modup_tables(const uint64_t* primes, HostTables& H) {
    const int L0 = H.L0, P = H.P, K = H.K, dnum = H.dnum;
    H.modup_intt.assign((size_t)(L0 + 1) * L0 * 4, 0);
    H.modup_hat.assign((size_t)(L0 + 1) * dnum * P * K, 0);
    H.modup_R.assign((size_t)(L0 + 1) * dnum * P * 2, 0);
    H.modup_Q.assign((size_t)(L0 + 1) * dnum * K * 2, 0);
    for (int l = 1; l <= L0; ++l)
        for (int j = 0; j < (l + P - 1) / P; ++j) {
            const int s0 = j * P, ns = std::min(s0 + P, l) - s0;
            const size_t lj = (size_t)l * dnum + j;
            for (int u = 0; u < ns; ++u) {
                const int i = s0 + u;
                const uint64_t q = primes[i];
                const uint64_t ih = h_inv(h_prod_except(primes, s0, ns, u, q), q);
                const uint64_t a = h_mulmod(H.primes[i].ninv, ih, q), b = h_mulmod(H.primes[i].w1ninv, ih, q);
                uint64_t* d = &H.modup_intt[((size_t)l * L0 + i) * 4];
                d[0] = a; d[1] = h_shoup(a, q); d[2] = b; d[3] = h_shoup(b, q);
                for (int t = 0; t < K; ++t) H.modup_hat[(lj * P + u) * K + t] = h_prod_except(primes, s0, ns, u, primes[t]);
                const hu128 R = h_floor128(q);
                H.modup_R[(lj * P + u) * 2 + 0] = (uint64_t)R;
                H.modup_R[(lj * P + u) * 2 + 1] = (uint64_t)(R >> 64);
            }
            for (int t = 0; t < K; ++t) {
                const uint64_t m = primes[t], Qm = h_prod_except(primes, s0, ns, -1, m);
                H.modup_Q[(lj * K + t) * 2 + 0] = Qm;
                H.modup_Q[(lj * K + t) * 2 + 1] = h_mulmod(Qm, (uint64_t)ns, m);
            }
        }
    H.modup_xd.assign((size_t)dnum * 32, 0);
    H.modup_xt.assign((size_t)K * 4, 0);
    if (P == 3) modup_xform_tables(primes, K, L0, dnum, H.modup_xd.data(), H.modup_xt.data());
}

// ModDown, special primes p_k = primes[L0 + k], k < P, data primes q_i, i < L0:
//   md_intt [P][4]   N^-1 inv(P/p_k), psi_rev_inv[1] N^-1 inv(P/p_k) mod p_k, each + Shoup
//   md_hat  [P][L0]  (P / p_k) mod q_i
//   md_pinv [L0][2] P^-1 mod q_i + Shoup; then [L0] P mod q_i; then [L0] floor(p/2) mod q_i (P = 1: SEAL rounding)
//   md_xd   [32]  X form of the special digit (fhs_kernels.hip k_special_x): Y = sum_k y_k (P/p_k) < 3P stored as
//           base-2^60 words -- P/p_k (2 words each), no centring (thresholds all ones), no offset (C_0 = 0); needs
//           3P < 2^180, so P = 3 special primes below 2^59 (returns whether that holds), else zero
static bool build_moddown_tables(const uint64_t* primes, HostTables& H) {
    const int L0 = H.L0, P = H.P;
    H.md_xd.assign(32, 0);
    bool md_x_ok = P == 3;
    for (int k = 0; k < P && md_x_ok; ++k) md_x_ok = primes[L0 + k] < (1ull << 59);
    if (md_x_ok) {
        for (int u = 0; u < 3; ++u) {
            const hu128 h = (hu128)primes[L0 + (u + 1) % 3] * primes[L0 + (u + 2) % 3];
            H.md_xd[2 * u] = (uint64_t)h;
            H.md_xd[2 * u + 1] = (uint64_t)(h >> 64);
        }
        for (int w = 6; w < 15; ++w) H.md_xd[w] = ~0ull;
    }
    H.md_intt.assign((size_t)P * 4, 0);
    H.md_hat.assign((size_t)P * L0, 0);
    H.md_pinv.assign((size_t)4 * L0, 0);
    for (int k = 0; k < P; ++k) {
        const uint64_t p = primes[L0 + k];
        const uint64_t ih = h_inv(h_prod_except(primes, L0, P, k, p), p);
        const uint64_t a = h_mulmod(H.primes[L0 + k].ninv, ih, p), b = h_mulmod(H.primes[L0 + k].w1ninv, ih, p);
        uint64_t* d = &H.md_intt[(size_t)k * 4];
        d[0] = a; d[1] = h_shoup(a, p); d[2] = b; d[3] = h_shoup(b, p);
        for (int i = 0; i < L0; ++i) H.md_hat[(size_t)k * L0 + i] = h_prod_except(primes, L0, P, k, primes[i]);
    }
    for (int i = 0; i < L0; ++i) {
        const uint64_t q = primes[i], pm = h_prod_except(primes, L0, P, -1, q), pinv = h_inv(pm, q);
        H.md_pinv[2 * i] = pinv;
        H.md_pinv[2 * i + 1] = h_shoup(pinv, q);
        H.md_pinv[2 * L0 + i] = pm;
        H.md_pinv[3 * L0 + i] = P == 1 ? (primes[L0] >> 1) % q : 0;
    }
    return md_x_ok;
}

// rescale [L0+1][L0][4]: level l (limbs) drops q_{l-1}; at (l, i < l - 1): inv(q_{l-1}) mod q_i + Shoup,
// half mod q_i, half = q_{l-1} >> 1
static void build_rescale_table(const uint64_t* primes, HostTables& H) {
    H.rescale.assign((size_t)(H.L0 + 1) * H.L0 * 4, 0);
    for (int l = 2; l <= H.L0; ++l) {
        const uint64_t ql = primes[l - 1], half = ql >> 1;
        for (int i = 0; i < l - 1; ++i) {
            const uint64_t q = primes[i];
            const uint64_t inv = h_inv(ql % q, q);
            uint64_t* d = &H.rescale[((size_t)l * H.L0 + i) * 4];
            d[0] = inv; d[1] = h_shoup(inv, q); d[2] = half % q; d[3] = half;
        }
    }
}

// pow2 [K][1088]: 2^e mod q_i (exact double reduction)
constexpr int kPow2Words = 1088;
static void build_pow2_table(const uint64_t* primes, HostTables& H) {
    H.pow2.assign((size_t)H.K * kPow2Words, 0);
    for (int i = 0; i < H.K; ++i) {
        uint64_t v = 1 % primes[i];
        for (int e = 0; e < kPow2Words; ++e) {
            H.pow2[(size_t)i * kPow2Words + e] = v;
            v = h_mulmod(v, 2, primes[i]);
        }
    }
}

// Host decoder: fft_w [N], dec_twist [N], slot_index [N/2].  GPU decoder (fhs_kernels.hip k_decode_fft), the host
// decoder's own values: dec_w [N/2][2] = fft_w[2k], dec_twist [N/2][2] = the host's first N/2 (re, im) pairs,
// dec_pos [N/2] = slot_index >> 1.
// GPU encoder (k_encode): enc_w [N/2][2] = omega^-k, omega = exp(2 pi i / (N/2)); enc_twist [N/2][2] =
// (2/N) zeta^-k, zeta = exp(i pi / N); enc_pos [N/2] = rev_{log N - 1}((5^j mod 2N - 1) / 4).
static void build_codec_tables(HostTables& H) {
    const uint64_t N = (uint64_t)H.N;
    const size_t h = N / 2;
    H.fft_w.resize(N);
    for (uint64_t k = 0; k < N; ++k) H.fft_w[k] = std::polar(1.0, 2.0 * M_PI * (double)k / (double)N);
    H.dec_twist.resize(N);
    for (uint64_t k = 0; k < N; ++k)
        H.dec_twist[k] = {std::cos(M_PI * (double)k / (double)N), std::sin(M_PI * (double)k / (double)N)};
    H.slot_index.resize(h);
    H.enc_pos.resize(h);
    uint64_t e5 = 1;
    for (size_t j = 0; j < h; ++j) {
        H.slot_index[j] = (e5 - 1) / 2;
        H.enc_pos[j] = h_bitrev((uint32_t)((e5 - 1) / 4), H.logN - 1);
        e5 = (e5 * 5) & (2 * N - 1);
    }
    H.dec_w.resize(2 * h);
    H.dec_pos.resize(h);
    H.enc_w.resize(2 * h);
    H.enc_twist.resize(2 * h);
    for (size_t k = 0; k < h; ++k) {
        H.dec_w[2 * k] = H.fft_w[2 * k].real();
        H.dec_w[2 * k + 1] = H.fft_w[2 * k].imag();
        H.dec_pos[k] = (unsigned)(H.slot_index[k] >> 1);
        const double th = -2.0 * M_PI * (double)k / (double)h;
        H.enc_w[2 * k] = std::cos(th);
        H.enc_w[2 * k + 1] = std::sin(th);
        const double tz = -M_PI * (double)k / (double)N;
        H.enc_twist[2 * k] = 2.0 / (double)N * std::cos(tz);
        H.enc_twist[2 * k + 1] = 2.0 / (double)N * std::sin(tz);
    }
}

// The dispatch flags (DevTables' comments say what each selects).  Returns an error message or null.
static const char* build_dispatch_flags(const uint64_t* primes, bool md_x_ok, HostTables& H) {
    const int K = H.K, P = H.P;
    H.max_qbits = 0;
    for (int i = 0; i < K; ++i) H.max_qbits = std::max(H.max_qbits, 64 - __builtin_clzll(primes[i]));
    // ModUp's specialised conversion: 3-limb digits with every target on the pseudo-Mersenne fold (the
    // generic loop is then not compiled into the kernel), one-limb digits, or the generic loop
    bool all_cpm = true;
    for (int i = 0; i < K; ++i) all_cpm = all_cpm && ((H.primes[i].pm >> 40) & 1);
    bool small_e1 = true;   // the X form's weight 2^60 mod m below 2^30 for every prime (modup_xform_tables)
    for (int i = 0; i < K && P == 3; ++i) small_e1 = small_e1 && H.modup_xt[(size_t)i * 4] < (1ull << 30);
    H.modup_dp = (P == 3 && H.L0 % 3 == 0 && all_cpm && small_e1) ? 3 : (P == 1 ? 1 : 0);
    H.md_xform = H.modup_dp == 3 && md_x_ok;
    // every prime 2^59 - d with d < 2^27 (SEAL's 59-bit Create() primes at N <= 65536): the X-form
    // conversions reduce with compile-time folds (convert3x_b59)
    bool all59 = true;
    for (int i = 0; i < K && all59; ++i) all59 = b59_prime(primes[i]);
    H.all_b59 = all59;
    H.conv_b59 = H.modup_dp == 3 && all59;
    // the B59 kernels compile the forward NTT's lazy mode in for N <= 16384 (fhs_kernels.hip lazy_of): every
    // prime must carry the lazy bit there, which q < 2^59 implies -- checked, not assumed
    for (int i = 0; i < K && all59 && H.logN <= 14; ++i)
        if (!((H.primes[i].pm >> 7) & 1)) return "context: a 59-bit prime without the lazy NTT bound (internal)";
    return nullptr;
}

// Every table of a context with validated parameters (context_params_error).  Returns an error message or null.
static const char* build_host_tables(uint64_t N, const uint64_t* primes, int K, int special, HostTables& H) {
    H.N = (int)N;
    H.logN = 0;
    while ((1ull << H.logN) < N) H.logN++;
    H.K = K;
    H.P = special;
    H.L0 = K - special;
    H.dnum = (H.L0 + special - 1) / special;
    build_prime_tables(primes, H);
    build_modup_tables(primes, H);
    const bool md_x_ok = build_moddown_tables(primes, H);
    build_rescale_table(primes, H);
    build_pow2_table(primes, H);
    build_codec_tables(H);
    return build_dispatch_flags(primes, md_x_ok, H);
}

// ============================================================================ decoder CRT constants
// The centred CRT over the first l primes, W = l + 1 words per integer: Q = prod q_i, hat[i] = Q / q_i ([l][W]),
// ihat[i] = hat[i]^-1 mod q_i with its Shoup companion, halfQ = Q >> 1.  crt_compose (fhs_host.hip) reads it;
// crt_consts packs it into fhs::CrtConsts for the GPU composition.
struct CrtHost {
    int l = 0, W = 0;
    std::vector<uint64_t> Q, halfQ, hat, ihat, ihat_s;
};
static CrtHost crt_host_consts(const uint64_t* q, int l) {
    CrtHost C;
    C.l = l;
    const int W = C.W = l + 1;
    auto mul_word = [W](uint64_t* x, uint64_t m) {   // x *= m over W words
        hu128 carry = 0;
        for (int w = 0; w < W; ++w) {
            const hu128 t = (hu128)x[w] * m + carry;
            x[w] = (uint64_t)t;
            carry = t >> 64;
        }
    };
    C.Q.assign(W, 0);
    C.Q[0] = 1;
    for (int i = 0; i < l; ++i) mul_word(C.Q.data(), q[i]);
    C.hat.assign((size_t)l * W, 0);
    C.ihat.resize(l);
    C.ihat_s.resize(l);
    for (int i = 0; i < l; ++i) {
        uint64_t* h = &C.hat[(size_t)i * W];
        h[0] = 1;
        for (int k = 0; k < l; ++k)
            if (k != i) mul_word(h, q[k]);
        C.ihat[i] = h_inv(h_prod_except(q, 0, l, i, q[i]), q[i]);
        C.ihat_s[i] = h_shoup(C.ihat[i], q[i]);
    }
    C.halfQ.resize(W);
    for (int w = 0; w < W; ++w) C.halfQ[w] = (C.Q[w] >> 1) | (w + 1 < W ? C.Q[w + 1] << 63 : 0);
    return C;
}
// Check table of one further limb q for a composition of W words (fhs_kernels.h launch_crt_compose_jobs):
// {q, floor(2^128/q) lo, hi, (2^64)^w mod q for w < W}
static void crt_check_table(uint64_t q, int W, uint64_t* v) {
    const hu128 R = h_floor128(q);
    v[0] = q;
    v[1] = (uint64_t)R;
    v[2] = (uint64_t)(R >> 64);
    const uint64_t t64 = (uint64_t)((((hu128)1) << 64) % q);
    uint64_t pw = 1 % q;
    for (int w = 0; w < W; ++w) {
        v[3 + w] = pw;
        pw = h_mulmod(pw, t64, q);
    }
}
