// weighted_sums_check.cpp -- host-side check of fhs_weighted_sums' argument validation, weight tables and chunk plan
// (fhe-spear_amd/csrc/fhs_tables.h weighted_sums_error, weighted_sums_tables, weighted_sums_chunks) and of the
// per-coefficient routines its kernel shares with the host (fhs_modarith.h wsum_round_*, wsum_*):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Itools/debug/shim \
//       -Ifhe-spear_amd/csrc tools/debug/weighted_sums_check.cpp -o weighted_sums_check && ./weighted_sums_check
// 1. Rejections: null, F, E, ldw, scale, component count, chain index, last level and scale mismatch each carry their
//    own message and status class; a non-finite weight and |round(w scale)| >= 2^62 are rejected by the tables.
// 2. Tables, for chains (60, 40, 40, 60), 59-bit and 40-bit primes at every l, F in {1, 5, 64}, E in {1, 3, 4, 9},
//    tiles 4 and 8, ldw > E: every word equals the definition computed with plain 128-bit arithmetic (k_ijm =
//    round(W scale) mod q_m, wl = k_ijL and floor(k_ijL 2^64 / q_L), wt = pack30(k_ijm inv_m mod q_m), row F =
//    pack30(q_m - inv_m)), the padding is zero and long enough for a chunk that starts inside a tile.
// 3. Chunk plan, N = 256..32768, l = 2..12, F in {1, 256, 4096}, E = 1..3000: covers [0, E) once in order, sizes
//    within one, none above kWsumMaxOutputs, none above what the cap leaves after the inputs' last limbs unless it is
//    a single output; fri's shape gives 179 outputs per chunk.
// 4. Routines: rounding sums and weighted sums of random and extreme operands against 128-bit / big-step references.
// Prints one line per part, then OK; exits non-zero at the first violation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "fhs_tables.h"

#define REQUIRE(cond, ...)                                       \
    do {                                                         \
        if (!(cond)) {                                           \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                        \
            fprintf(stderr, "\n");                               \
            exit(1);                                             \
        }                                                        \
    } while (0)

typedef __int128 hi128;

static bool is_prime(uint64_t n) {
    for (uint64_t a : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
        if (n % a == 0) return n == a;
        uint64_t d = n - 1;
        int r = 0;
        while (!(d & 1)) d >>= 1, ++r;
        uint64_t x = h_pow(a, d, n);
        if (x == 1 || x == n - 1) continue;
        bool comp = true;
        for (int i = 1; i < r && comp; ++i) {
            x = h_mulmod(x, x, n);
            if (x == n - 1) comp = false;
        }
        if (comp) return false;
    }
    return true;
}
// the `count` largest primes below 2^bits that are 1 mod 2N
static std::vector<uint64_t> ntt_primes(int bits, int count, uint64_t N) {
    std::vector<uint64_t> out;
    for (uint64_t c = ((1ull << bits) - 1) / (2 * N) * (2 * N) + 1; (int)out.size() < count; c -= 2 * N)
        if (c < (1ull << bits) && is_prime(c)) out.push_back(c);
    return out;
}

static void check_errors() {
    const int L0 = 3;
    const int two[3] = {2, 2, 2}, three[3] = {2, 3, 2}, ci1[3] = {1, 1, 1}, ci_mixed[3] = {1, 2, 1}, ci_last[3] = {3, 3, 3},
              ci_bad[3] = {4, 4, 4};
    const double sc[3] = {1e12, 1e12, 1e12 * (1 + 1e-12)}, sc_bad[3] = {1e12, 1e12, 1.1e12};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    struct Bad {
        bool null_arg;
        int F, E;
        int64_t ldw;
        double scale;
        const int *ncomp, *ci;
        const double* scales;
        ArgErr cls;
        const char* word;
    };
    const Bad bad[] = {{true, 3, 2, 2, 2.0, two, ci1, sc, ARG_INVALID, "null argument"},
                       {false, 0, 2, 2, 2.0, two, ci1, sc, ARG_INVALID, "1 <= F <= 4096"},
                       {false, -1, 2, 2, 2.0, two, ci1, sc, ARG_INVALID, "1 <= F <= 4096"},
                       {false, 4097, 2, 2, 2.0, two, ci1, sc, ARG_INVALID, "1 <= F <= 4096"},
                       {false, 3, 0, 2, 2.0, two, ci1, sc, ARG_INVALID, "E >= 1"},
                       {false, 3, 2, 1, 2.0, two, ci1, sc, ARG_INVALID, "ldw >= E"},
                       {false, 3, 2, 2, 0.0, two, ci1, sc, ARG_INVALID, "bad scale"},
                       {false, 3, 2, 2, -4.0, two, ci1, sc, ARG_INVALID, "bad scale"},
                       {false, 3, 2, 2, inf, two, ci1, sc, ARG_INVALID, "bad scale"},
                       {false, 3, 2, 2, nan, two, ci1, sc, ARG_INVALID, "bad scale"},
                       {false, 3, 2, 2, 2.0, nullptr, ci1, sc, ARG_INVALID, "null argument"},
                       {false, 3, 2, 2, 2.0, three, ci_mixed, sc_bad, ARG_INVALID, "2-component"},
                       {false, 3, 2, 2, 2.0, two, ci_mixed, sc_bad, ARG_LEVEL, "share one chain index"},
                       {false, 3, 2, 2, 2.0, two, ci_bad, sc, ARG_LEVEL, "chain index out of range"},
                       {false, 3, 2, 2, 2.0, two, ci_last, sc_bad, ARG_LEVEL, "no level left"},
                       {false, 3, 2, 2, 2.0, two, ci1, sc_bad, ARG_SCALE, "scale mismatch"}};
    for (const Bad& b : bad) {
        ArgErr cls = b.cls == ARG_INVALID ? ARG_LEVEL : ARG_INVALID;
        const char* err = weighted_sums_error(b.null_arg, b.F, b.E, b.ldw, b.scale, b.ncomp, b.ci, b.scales, L0, &cls);
        REQUIRE(err && strstr(err, b.word) && cls == b.cls, "\"%s\": \"%s\", class %d", b.word, err ? err : "accepted", (int)cls);
    }
    ArgErr cls = ARG_LEVEL;
    REQUIRE(!weighted_sums_error(false, 3, 2, 5, 2.0, two, ci1, sc, L0, &cls) && cls == ARG_INVALID, "accepted call");
    REQUIRE(!weighted_sums_error(false, 1, 1, 1, 1e-3, two, ci1, sc, L0, &cls), "F = E = 1");
    // the weights
    const std::vector<uint64_t> q = ntt_primes(40, 2, 256);
    WsumTables Wt;
    double w[2] = {1.0, nan};
    REQUIRE(strstr(weighted_sums_tables(w, 1, 2, 1, 2.0, q.data(), 2, 4, Wt), "not finite"), "nan weight");
    w[1] = -inf;
    REQUIRE(strstr(weighted_sums_tables(w, 1, 2, 1, 2.0, q.data(), 2, 4, Wt), "not finite"), "inf weight");
    w[1] = 4611686018427387904.0;   // 2^62
    REQUIRE(strstr(weighted_sums_tables(w, 1, 2, 1, 1.0, q.data(), 2, 4, Wt), ">= 2^62"), "2^62");
    w[1] = -4611686018427387904.0;
    REQUIRE(strstr(weighted_sums_tables(w, 1, 2, 1, 1.0, q.data(), 2, 4, Wt), ">= 2^62"), "-2^62");
    w[0] = 0.0, w[1] = 1e300;
    REQUIRE(strstr(weighted_sums_tables(w, 1, 2, 1, 1e300, q.data(), 2, 4, Wt), "not finite"), "overflowing product");
    w[1] = -4611686018427387392.0;   // -(2^62 - 512): the largest double below 2^62
    REQUIRE(!weighted_sums_tables(w, 1, 2, 1, 1.0, q.data(), 2, 4, Wt), "largest weight");
    REQUIRE(Wt.wl[1 * Wt.Epad] == q[1] - (uint64_t)4611686018427387392ull % q[1], "largest weight's residue");
    printf("errors ok\n");
}

static uint64_t res_of(hi128 c, uint64_t q) {
    hi128 r = c % (hi128)q;
    if (r < 0) r += q;
    return (uint64_t)r;
}
static void check_tables() {
    long long words = 0;
    std::mt19937_64 rng(7);
    const uint64_t N = 256;
    std::vector<std::vector<uint64_t>> chains;
    {
        std::vector<uint64_t> a = ntt_primes(60, 2, N), b = ntt_primes(40, 2, N);
        chains.push_back({a[0], b[0], b[1], a[1]});
        chains.push_back(ntt_primes(59, 6, N));
        chains.push_back(ntt_primes(40, 3, N));
    }
    const double scale = 1099511627776.0;   // 2^40
    for (const auto& q : chains)
        for (int l = 2; l <= (int)q.size(); ++l)
            for (int F : {1, 5, 64})
                for (int E : {1, 3, 4, 9})
                    for (int tile : {4, 8}) {
                        const int64_t ldw = E + 2;
                        std::vector<double> W((size_t)F * ldw);
                        for (auto& x : W) {
                            switch (rng() % 8) {
                            case 0: x = 0.0; break;
                            case 1: x = 1.0; break;
                            case 2: x = -1.0; break;
                            case 3: x = 1.0 / scale; break;
                            case 4: x = -1.0 / scale; break;
                            case 5: x = ((double)(rng() % 2001) - 1000.0 + 0.5) / scale; break;   // ties: half away from zero
                            default: x = ((double)(int64_t)(rng() >> 12) / 4503599627370496.0 - 0.5) * 4.0;
                            }
                        }
                        WsumTables Wt;
                        REQUIRE(!weighted_sums_tables(W.data(), ldw, F, E, scale, q.data(), l, tile, Wt), "tables rejected");
                        const int L = l - 1;
                        const size_t Epad = (size_t)Wt.Epad;
                        REQUIRE(Epad % tile == 0 && Epad >= (size_t)E + tile && Epad < (size_t)E + 2 * tile, "Epad %zu for E=%d", Epad, E);
                        REQUIRE(Wt.wl.size() == 2 * F * Epad && Wt.wt.size() == (size_t)L * (F + 1) * Epad, "table sizes");
                        for (int j = 0; j < F; ++j)
                            for (size_t i = 0; i < Epad; ++i, ++words) {
                                if (i >= (size_t)E) {
                                    REQUIRE(Wt.wl[j * Epad + i] == 0 && Wt.wl[(F + j) * Epad + i] == 0, "wl padding");
                                    for (int m = 0; m < L; ++m) REQUIRE(Wt.wt[((size_t)m * (F + 1) + j) * Epad + i] == 0, "wt padding");
                                    continue;
                                }
                                const double x = W[(size_t)j * ldw + i] * scale;
                                const double fl = std::floor(std::fabs(x)), fr = std::fabs(x) - fl;   // exact for |x| < 2^52
                                hi128 c = (hi128)fl + (fr >= 0.5 ? 1 : 0);
                                if (x < 0) c = -c;
                                const uint64_t kL = res_of(c, q[L]);
                                REQUIRE(Wt.wl[j * Epad + i] == kL, "kL at (%d, %zu)", j, i);
                                REQUIRE(Wt.wl[(F + j) * Epad + i] == (uint64_t)(((hu128)kL << 64) / q[L]), "Shoup word at (%d, %zu)", j, i);
                                for (int m = 0; m < L; ++m) {
                                    const uint64_t inv = h_inv(q[L] % q[m], q[m]);
                                    REQUIRE(h_mulmod(inv, q[L] % q[m], q[m]) == 1, "inverse");
                                    const uint64_t kp = h_mulmod(res_of(c, q[m]), inv, q[m]);
                                    REQUIRE(Wt.wt[((size_t)m * (F + 1) + j) * Epad + i] == pack30(kp), "k' at (%d, %d, %zu)", m, j, i);
                                    const Split30 sp = unpack30(pack30(kp));
                                    REQUIRE((((uint64_t)sp.hi << 30) | sp.lo) == kp, "pack30 round trip");
                                }
                            }
                        for (int m = 0; m < L; ++m)
                            for (size_t i = 0; i < Epad; ++i) {
                                const uint64_t inv = h_inv(q[L] % q[m], q[m]);
                                REQUIRE(Wt.wt[((size_t)m * (F + 1) + F) * Epad + i] == (i < (size_t)E ? pack30(q[m] - inv) : 0),
                                        "correction weight at (%d, %zu)", m, i);
                            }
                    }
    printf("tables ok: %lld weights\n", words);
}

static void check_chunks() {
    long long plans = 0;
    for (uint64_t N = 256; N <= 32768; N <<= 1)
        for (int l = 2; l <= 12; ++l)
            for (int F : {1, 256, 4096})
                for (size_t cap : {kMulManyCap, (size_t)1 << 20, (size_t)0})
                    for (int E = 1; E <= 3000; E += (E < 600 ? 1 : 37), ++plans) {
                        const auto ch = weighted_sums_chunks(E, F, N, l, cap);
                        const size_t fixed = 16 * (size_t)F * N, item = weighted_sums_item_bytes(N, l);
                        const size_t room = cap > fixed ? cap - fixed : 0;
                        REQUIRE(item == 8 * N * 4 + 8 * N * 2 * (size_t)(l - 1), "item bytes");
                        REQUIRE(!ch.empty(), "no chunk");
                        int at = 0, lo = ch[0].second, hi = ch[0].second;
                        for (const auto& c : ch) {
                            REQUIRE(c.first == at && c.second >= 1, "chunk (%d, %d) at %d", c.first, c.second, at);
                            at += c.second;
                            lo = std::min(lo, c.second);
                            hi = std::max(hi, c.second);
                            REQUIRE(c.second <= kWsumMaxOutputs, "chunk of %d outputs", c.second);
                            REQUIRE(c.second == 1 || (size_t)c.second * item <= room, "chunk of %d outputs over the cap", c.second);
                        }
                        REQUIRE(at == E && hi - lo <= 1 && ch[0].second == hi, "E=%d: cover %d, sizes %d..%d", E, at, lo, hi);
                        if (ch.size() > 1) {
                            const size_t fewer = ch.size() - 1, need = ((size_t)E + fewer - 1) / fewer;
                            REQUIRE(need > (size_t)kWsumMaxOutputs || need * item > room, "E=%d: %zu chunks where %zu fit", E, ch.size(), fewer);
                        }
                    }
    REQUIRE(weighted_sums_chunks(1000, 256, 32768, 9)[0].second == 167 && weighted_sums_chunks(179, 256, 32768, 9).size() == 1 &&
                weighted_sums_chunks(180, 256, 32768, 9).size() == 2,
            "fri: 179 outputs per chunk");
    REQUIRE(weighted_sums_chunks(513, 1, 256, 2).size() == 2 && weighted_sums_chunks(513, 1, 256, 2)[0].second == 257, "513 outputs");
    printf("chunks ok: %lld plans\n", plans);
}

static void check_routines() {
    std::mt19937_64 rng(11);
    long long sums = 0;
    std::vector<uint64_t> primes;
    for (int bits : {40, 59, 60})
        for (uint64_t q : ntt_primes(bits, 2, 32768)) primes.push_back(q);
    for (uint64_t q : primes) {
        const hu128 r = ~(hu128)0 / q;
        const uint64_t pw = pm_word(q, 14);
        const RedU R{q, (uint64_t)r, (uint64_t)(r >> 64), (unsigned)(pw & 127), (unsigned)((pw >> 8) & 0xFFFFFFFFu), false, false};
        const unsigned fmask = wsum_fmask(q);
        REQUIRE(fmask == (q < (1ull << 59) ? 15u : 7u), "fold mask");
        const uint64_t half = q >> 1, edge[5] = {0, half - 1, half, half + 1, q - 1};
        for (int F : {1, 2, 7, 8, 15, 16, 63, 64, 65, 127, 128, 129, 1000, 4096})
            for (int mode = 0; mode < 4; ++mode, ++sums) {
                std::vector<uint64_t> k(F), d(F);
                for (int j = 0; j < F; ++j) {
                    k[j] = mode == 0 ? rng() % q : mode == 1 ? q - 1 : mode == 2 ? 1 : (j & 1 ? q - 1 : 0);
                    d[j] = mode == 0   ? rng() % q
                           : mode == 1 ? q - 1
                           : mode == 2 ? edge[j % 5]
                                       : half + 1;
                }
                // the rounding sum
                WsumRound s{0, 0, 0};
                hi128 want = 0;
                for (int j = 0; j < F; ++j) {
                    wsum_round_term(s, d[j], k[j], h_shoup(k[j], q), q);
                    const uint64_t u = h_mulmod(k[j], d[j], q);
                    want += (hi128)((u + half) % q) - (hi128)half;
                }
                int64_t hi;
                uint64_t lo;
                wsum_round_finish(s, q, hi, lo);
                REQUIRE((hi128)(((hu128)(uint64_t)hi << 64) | lo) == want, "rounding sum q=%llu F=%d mode %d", (unsigned long long)q, F, mode);
                // the weighted sum with its correction term
                const uint64_t wT = mode == 1 ? q - 1 : rng() % q, t = mode == 1 ? q - 1 : rng() % q;
                Wsum a;
                wsum_clear(a);
                uint64_t acc = h_mulmod(wT, t, q);
                for (int j = 0; j < F; ++j) {
                    wsum_mac(a, unpack30(pack30(k[j])), split30(d[j]));
                    wsum_after(a, j + 1, fmask, R);
                    acc = (uint64_t)(((hu128)acc + h_mulmod(k[j], d[j], q)) % q);
                }
                wsum_mac(a, unpack30(pack30(wT)), split30(t));
                REQUIRE(wsum_finish(a, R) == acc, "weighted sum q=%llu F=%d mode %d", (unsigned long long)q, F, mode);
            }
    }
    printf("routines ok: %lld sums\n", sums);
}

int main() {
    check_errors();
    check_tables();
    check_chunks();
    check_routines();
    printf("OK\n");
    return 0;
}
