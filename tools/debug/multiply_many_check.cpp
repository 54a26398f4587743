// multiply_many_check.cpp -- host-side check of fhs_multiply_relin_many's argument validation and chunk plan
// (fhe-spear_amd/csrc/fhs_tables.h multiply_many_error, batch_chunks, kKsMaxItems, kMulManyCap):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Itools/debug/shim \
//       -Ifhe-spear_amd/csrc tools/debug/multiply_many_check.cpp -o multiply_many_check && ./multiply_many_check
// For every N = 256..32768, every level l = 1..12, P = 1 and 3, both key-switch conventions and every stage
// combination (relinearize and / or rescale), with the per-item scratch the host layer charges --
//   key-switch workspace 8 N (l + dn E + 2 E + 2 P) (+ 16 l N, SEAL convention; E = l + P, dn = ceil(l / P)),
//   tensor products 24 l N, relinearized pairs 16 l N, the rescale's last limbs 8 N per output component --
// and every n = 1..5000 (all stages, exact convention; the other stage sets at n = 1..64, around every chunk-count
// boundary up to 8 chunks, and at 4999 and 5000): the chunks cover [0, n) exactly once in order, their sizes differ by at most one, none has
// more than kKsMaxItems items, none costs more than kMulManyCap bytes unless it is a single item, and no plan with
// fewer chunks would fit.  Then fhs_inner_sum_many's former plan, written out, against batch_chunks for n = 1..1100 and
// seven chunk bounds: the same chunk count and the same largest chunk.  Then the rejections: null, n, component count, chain index and the last level each carry
// their own message and status class.  Prints one line per N, then OK; exits non-zero at the first violation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static size_t item_bytes(size_t N, int l, int P, bool seal, bool relin, bool rescale) {
    const size_t E = (size_t)l + P, dn = ((size_t)l + P - 1) / P, S = (size_t)l * N;
    const size_t ks = 8 * N * (l + dn * E + 2 * E + 2 * P) + (seal ? 16 * S : 0);
    const int ocomp = relin ? 2 : 3;
    return (relin ? ks : 0) + ((relin || rescale) ? 24 * S : 0) + ((relin && rescale) ? 16 * S : 0) +
           (rescale ? 8 * (size_t)ocomp * N : 0);
}

static void check_plan(int n, size_t item, int max_items, size_t cap, const char* what) {
    const std::vector<std::pair<int, int>> ch = batch_chunks(n, item, max_items, cap);
    REQUIRE(!ch.empty(), "%s n=%d: no chunk", what, n);
    int at = 0, lo = ch[0].second, hi = ch[0].second;
    for (const auto& c : ch) {
        REQUIRE(c.first == at && c.second >= 1, "%s n=%d: chunk (%d, %d) at %d", what, n, c.first, c.second, at);
        at += c.second;
        lo = std::min(lo, c.second);
        hi = std::max(hi, c.second);
        REQUIRE(c.second <= max_items, "%s n=%d: chunk of %d items", what, n, c.second);
        REQUIRE(c.second == 1 || (size_t)c.second * item <= cap, "%s n=%d: chunk of %d items is %zu bytes", what, n, c.second,
                (size_t)c.second * item);
    }
    REQUIRE(at == n, "%s n=%d: chunks cover %d", what, n, at);
    REQUIRE(hi - lo <= 1, "%s n=%d: chunk sizes %d..%d", what, n, lo, hi);
    // no fewer chunks would do: one chunk less forces a chunk above a bound
    if (ch.size() > 1) {
        const size_t fewer = ch.size() - 1, need = ((size_t)n + fewer - 1) / fewer;
        REQUIRE(need > (size_t)max_items || need * item > cap, "%s n=%d: %zu chunks where %zu fit", what, n, ch.size(), fewer);
    }
}

int main() {
    for (uint64_t N = 256; N <= 32768; N <<= 1) {
        long long plans = 0, multi = 0, single_over = 0;
        for (int P : {1, 3})
            for (int l = 1; l <= 12; ++l)
                for (int mode = 0; mode < 6; ++mode) {
                    const bool relin = mode < 4, rescale = mode & 1, seal = relin && (mode & 2);
                    if (seal && P != 1) continue;
                    char what[96];
                    snprintf(what, sizeof what, "N=%llu l=%d P=%d relin=%d rescale=%d seal=%d", (unsigned long long)N, l, P,
                             relin, rescale, seal);
                    const size_t item = item_bytes(N, l, P, seal, relin, rescale);
                    if (mode == 1) {   // every stage, exact convention: every n
                        for (int n = 1; n <= 5000; ++n, ++plans) check_plan(n, item, kKsMaxItems, kMulManyCap, what);
                    } else {           // the other stage sets: small n, every chunk-count boundary up to 8 chunks, the ends
                        const long long rmax = std::max<long long>(1, std::min<long long>(kKsMaxItems, item ? kMulManyCap / item : kKsMaxItems));
                        for (int n = 1; n <= 64; ++n, ++plans) check_plan(n, item, kKsMaxItems, kMulManyCap, what);
                        for (long long k = 1; k <= 8; ++k)
                            for (long long n = k * rmax - 1; n <= k * rmax + 1; ++n)
                                if (n >= 1 && n <= 5000) check_plan((int)n, item, kKsMaxItems, kMulManyCap, what), ++plans;
                        for (int n : {4999, 5000}) check_plan(n, item, kKsMaxItems, kMulManyCap, what), ++plans;
                    }
                    multi += batch_chunks(5000, item, kKsMaxItems, kMulManyCap).size() > 1;
                }
        // a cap below one item: every chunk is a single item; no item cost at all: the item buffer alone bounds
        for (int n : {1, 2, 7, 513}) {
            check_plan(n, 1000, kKsMaxItems, 999, "cap below an item");
            REQUIRE(batch_chunks(n, 1000, kKsMaxItems, 999).size() == (size_t)n, "cap below an item: n=%d", n);
            ++single_over;
            check_plan(n, 0, kKsMaxItems, kMulManyCap, "free items");
            REQUIRE(batch_chunks(n, 0, kKsMaxItems, kMulManyCap).size() == (size_t)(n + kKsMaxItems - 1) / kKsMaxItems,
                    "free items: n=%d", n);
        }
        REQUIRE(batch_chunks(0, 8, kKsMaxItems, kMulManyCap).empty() && batch_chunks(-3, 8, kKsMaxItems, kMulManyCap).empty(),
                "n < 1 gives no chunk");
        printf("N=%-5llu ok: %lld plans, %lld shapes take several chunks at n=5000\n", (unsigned long long)N, plans, multi);
    }
    // fri's ring: N = 32768, l = 9, P = 1, all stages -- a thousand columns ask for at most the cap
    {
        const size_t item = item_bytes(32768, 9, 1, false, true, true);
        const auto ch = batch_chunks(1000, item, kKsMaxItems, kMulManyCap);
        REQUIRE((size_t)ch[0].second * item <= kMulManyCap && ch[0].second == 24, "fri: %d pairs per chunk, %zu bytes each",
                ch[0].second, item);
    }
    // fhs_inner_sum_many's former hand-rolled plan (rmax items at most per chunk, nchunks = ceil(n / rmax), steps of
    // rchunk = ceil(n / nchunks)): batch_chunks gives the same chunk count and the same largest (first) chunk, so the
    // key-switch workspace, sized by that chunk, is what it was
    int former = 0;
    for (int rmax : {1, 2, 3, 4, 31, 32, 512})
        for (int n = 1; n <= 1100; ++n, ++former) {
            const int nchunks = (n + rmax - 1) / rmax, rchunk = (n + nchunks - 1) / nchunks;
            const auto ch = batch_chunks(n, 8, rmax, (size_t)8 * 512);          // bound by the item buffer
            const auto cb = batch_chunks(n, 8, kKsMaxItems, (size_t)8 * rmax);   // bound by the bytes
            REQUIRE((int)ch.size() == nchunks && ch[0].second == rchunk, "n=%d rmax=%d: %zu chunks, first of %d", n, rmax,
                    ch.size(), ch[0].second);
            REQUIRE((int)cb.size() == nchunks && cb[0].second == rchunk, "n=%d rmax=%d (bytes): %zu chunks, first of %d", n, rmax,
                    cb.size(), cb[0].second);
        }
    printf("inner_sum_many ok: %d plans keep their chunk count and largest chunk\n", former);
    // the rejections, each with its own message and status class
    const int L0 = 3;
    const int two[4] = {2, 2, 2, 2}, three[4] = {2, 2, 3, 2}, ci1[4] = {1, 1, 1, 1}, ci_mixed[4] = {1, 1, 1, 2},
              ci_last[4] = {3, 3, 3, 3}, ci_bad[4] = {4, 4, 4, 4};
    struct Bad {
        bool null_arg;
        int n;
        const int *ncomp, *ci;
        size_t count;
        int rescale;
        bool level;
        const char* word;
    };
    const Bad bad[] = {{true, 2, two, ci1, 4, 1, false, "null argument"},
                       {false, 0, two, ci1, 0, 1, false, "n >= 1"},
                       {false, -7, two, ci1, 0, 1, false, "n >= 1"},
                       {false, 2, nullptr, ci1, 4, 1, false, "null argument"},
                       {false, 2, two, ci1, 1, 1, false, "null argument"},
                       {false, 2, three, ci1, 4, 1, false, "2-component"},
                       {false, 2, three, ci_mixed, 4, 1, false, "2-component"},
                       {false, 2, two, ci_mixed, 4, 1, true, "share one chain index"},
                       {false, 2, two, ci_mixed, 4, 0, true, "share one chain index"},
                       {false, 2, two, ci_last, 4, 1, true, "rescale_to_next: no level left"},
                       {false, 2, two, ci_bad, 4, 0, true, "chain index out of range"}};
    for (const Bad& b : bad) {
        ArgErr cls = b.level ? ARG_INVALID : ARG_LEVEL;
        const char* err = multiply_many_error(b.null_arg, b.n, b.ncomp, b.ci, b.count, L0, b.rescale, &cls);
        REQUIRE(err && strstr(err, b.word) && cls == (b.level ? ARG_LEVEL : ARG_INVALID), "n=%d \"%s\": \"%s\", class %d", b.n,
                b.word, err ? err : "accepted", (int)cls);
    }
    for (int rescale = 0; rescale < 2; ++rescale)
        for (size_t count : {(size_t)2, (size_t)4}) {
            ArgErr cls = ARG_LEVEL;
            REQUIRE(multiply_many_error(false, 2, two, ci1, count, L0, rescale, &cls) == nullptr && cls == ARG_INVALID, "accepted call");
        }
    {   // the last level without rescale is a legal call
        ArgErr cls = ARG_LEVEL;
        REQUIRE(multiply_many_error(false, 2, two, ci_last, 4, L0, 0, &cls) == nullptr && cls == ARG_INVALID, "last level, no rescale");
    }
    printf("OK\n");
    return 0;
}
