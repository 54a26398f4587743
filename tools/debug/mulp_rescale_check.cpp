// mulp_rescale_check.cpp -- host-side check of fhs_multiply_plain_rescale_many's argument validation and chunk plan
// (fhe-spear_amd/csrc/fhs_tables.h mulp_rescale_many_error, mulp_rescale_chunks, kMulpRescaleMaxItems):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Itools/debug/shim \
//       -Ifhe-spear_amd/csrc tools/debug/mulp_rescale_check.cpp -o mulp_rescale_check && ./mulp_rescale_check
// For every N = 256..32768, every level l = 1..12 and every n = 1..5000, with the per-item costs the host layer
// charges -- 16 N bytes of rescale scratch, two staged pointers, two workgroups of the first launch and a grid.y of
// two in the second -- the chunks cover [0, n) exactly once in order, their sizes differ by at most one, and none is
// over the item bound (kKsMaxItems), the staged pointer buffer (2 kStagedMaxPtrs pointers), the grid limit (65535)
// or the byte cap (kMulManyCap) unless it is a single item; no plan with fewer chunks would fit.  (The plan does not
// depend on l; the walk over l re-checks the validation's level rule at every level instead.)  Then the rejections:
// null, n, component count, the chain indices of ciphertexts and plaintexts and the last level each carry their own
// message and status class.  Prints one line per N, then OK; exits non-zero at the first violation.
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

static void check_plan(int n, size_t N, size_t cap, const char* what) {
    const std::vector<std::pair<int, int>> ch = mulp_rescale_chunks(n, N, cap);
    const size_t item = mulp_rescale_item_bytes(N);
    REQUIRE(item == 16 * N, "%s: item of %zu bytes", what, item);
    REQUIRE(!ch.empty(), "%s n=%d: no chunk", what, n);
    int at = 0, lo = ch[0].second, hi = ch[0].second;
    for (const auto& c : ch) {
        REQUIRE(c.first == at && c.second >= 1, "%s n=%d: chunk (%d, %d) at %d", what, n, c.first, c.second, at);
        at += c.second;
        lo = std::min(lo, c.second);
        hi = std::max(hi, c.second);
        REQUIRE(c.second <= kKsMaxItems, "%s n=%d: chunk of %d items", what, n, c.second);
        REQUIRE(2 * (long long)c.second <= 2 * (long long)kStagedMaxPtrs, "%s n=%d: %d staged pointers", what, n, 2 * c.second);
        REQUIRE(2 * (long long)c.second <= 65535, "%s n=%d: grid of %d", what, n, 2 * c.second);
        REQUIRE(c.second == 1 || (size_t)c.second * item <= cap, "%s n=%d: chunk of %d items is %zu bytes", what, n, c.second,
                (size_t)c.second * item);
    }
    REQUIRE(at == n, "%s n=%d: chunks cover %d", what, n, at);
    REQUIRE(hi - lo <= 1, "%s n=%d: chunk sizes %d..%d", what, n, lo, hi);
    if (ch.size() > 1) {   // no fewer chunks would do: one chunk less forces a chunk above a bound
        const size_t fewer = ch.size() - 1, need = ((size_t)n + fewer - 1) / fewer;
        REQUIRE(need > (size_t)kMulpRescaleMaxItems || need * item > cap, "%s n=%d: %zu chunks where %zu fit", what, n, ch.size(),
                fewer);
    }
}

int main() {
    REQUIRE(kMulpRescaleMaxItems >= 1 && kMulpRescaleMaxItems <= kKsMaxItems && kMulpRescaleMaxItems <= kStagedMaxPtrs &&
                2 * kMulpRescaleMaxItems <= kGridMaxY,
            "item bound %d", kMulpRescaleMaxItems);
    const int L0 = 12;
    std::vector<int> two(5000, 2), ci(5000), pci(5000);
    for (uint64_t N = 256; N <= 32768; N <<= 1) {
        long long plans = 0;
        char what[64];
        for (int l = 1; l <= 12; ++l) {
            snprintf(what, sizeof what, "N=%llu l=%d", (unsigned long long)N, l);
            std::fill(ci.begin(), ci.end(), L0 + 1 - l);
            std::fill(pci.begin(), pci.end(), L0 + 1 - l);
            for (int n = 1; n <= 5000; ++n, ++plans) {
                check_plan(n, N, kMulManyCap, what);
                if (n > 64 && n % 97) continue;   // the validation at every small n and a stride of the large ones
                for (const int* pc : {(const int*)pci.data(), (const int*)nullptr}) {
                    ArgErr cls = l >= 2 ? ARG_LEVEL : ARG_INVALID;
                    const char* err = mulp_rescale_many_error(false, n, two.data(), ci.data(), pc, L0, &cls);
                    if (l >= 2) REQUIRE(!err && cls == ARG_INVALID, "%s n=%d: rejected \"%s\"", what, n, err ? err : "");
                    else REQUIRE(err && strstr(err, "no level left") && cls == ARG_LEVEL, "%s n=%d: last level \"%s\"", what, n, err ? err : "accepted");
                }
            }
        }
        // a cap below one item: single items; a cap of a few items: the byte bound is the one that cuts
        for (int n : {1, 2, 7, 513, 5000}) {
            check_plan(n, N, 16 * N - 1, "cap below an item");
            REQUIRE(mulp_rescale_chunks(n, N, 16 * N - 1).size() == (size_t)n, "cap below an item: n=%d", n);
            check_plan(n, N, 3 * 16 * N + 5, "cap of three items");
            REQUIRE(mulp_rescale_chunks(n, N, 3 * 16 * N + 5).size() == ((size_t)n + 2) / 3, "cap of three items: n=%d", n);
            plans += 2;
        }
        REQUIRE(mulp_rescale_chunks(0, N).empty() && mulp_rescale_chunks(-3, N).empty(), "n < 1 gives no chunk");
        const auto c513 = mulp_rescale_chunks(kMulpRescaleMaxItems + 1, N);
        REQUIRE(c513.size() == 2 && c513[0].second == kMulpRescaleMaxItems / 2 + 1 && c513[1].second == kMulpRescaleMaxItems / 2,
                "one more than the item bound: %zu chunks", c513.size());
        printf("N=%-5llu ok: %lld plans, %zu chunks at n=5000\n", (unsigned long long)N, plans, mulp_rescale_chunks(5000, N).size());
    }
    // fri's ring: N = 32768, 1024 columns per batch -- two chunks of 512, 256 MiB of scratch each, under the cap
    {
        const auto ch = mulp_rescale_chunks(1024, 32768);
        REQUIRE(ch.size() == 2 && ch[0].second == 512 && 512 * mulp_rescale_item_bytes(32768) <= kMulManyCap, "fri: %zu chunks",
                ch.size());
    }
    // the rejections, each with its own message and status class
    const int L3 = 3;
    const int c2[3] = {2, 2, 2}, c3[3] = {2, 3, 2}, ci1[3] = {1, 1, 1}, ci_mixed[3] = {1, 1, 2}, ci_last[3] = {3, 3, 3},
              ci_bad[3] = {4, 4, 4}, ci_zero[3] = {0, 0, 0};
    struct Bad {
        bool null_arg;
        int n;
        const int *ncomp, *ci, *pci;
        bool level;
        const char* word;
    };
    const Bad bad[] = {{true, 3, c2, ci1, ci1, false, "null argument"},
                       {false, 0, c2, ci1, ci1, false, "n >= 1"},
                       {false, -7, c2, ci1, nullptr, false, "n >= 1"},
                       {false, 3, nullptr, ci1, ci1, false, "null argument"},
                       {false, 3, c2, nullptr, ci1, false, "null argument"},
                       {false, 3, c3, ci1, ci1, false, "2-component"},
                       {false, 3, c3, ci_mixed, ci_mixed, false, "2-component"},
                       {false, 3, c2, ci_mixed, nullptr, true, "share one chain index"},
                       {false, 3, c2, ci_mixed, ci1, true, "share one chain index"},
                       {false, 3, c2, ci1, ci_mixed, true, "different chain indices"},
                       {false, 3, c2, ci_last, ci1, true, "different chain indices"},
                       {false, 3, c2, ci_last, ci_last, true, "rescale_to_next: no level left"},
                       {false, 3, c2, ci_last, nullptr, true, "rescale_to_next: no level left"},
                       {false, 3, c2, ci_bad, ci_bad, true, "chain index out of range"},
                       {false, 3, c2, ci_zero, nullptr, true, "chain index out of range"}};
    for (const Bad& b : bad) {
        ArgErr cls = b.level ? ARG_INVALID : ARG_LEVEL;
        const char* err = mulp_rescale_many_error(b.null_arg, b.n, b.ncomp, b.ci, b.pci, L3, &cls);
        REQUIRE(err && strstr(err, b.word) && cls == (b.level ? ARG_LEVEL : ARG_INVALID), "n=%d \"%s\": \"%s\", class %d", b.n,
                b.word, err ? err : "accepted", (int)cls);
    }
    for (const int* pc : {ci1, (const int*)nullptr})
        for (int n : {1, 3}) {
            ArgErr cls = ARG_LEVEL;
            REQUIRE(mulp_rescale_many_error(false, n, c2, ci1, pc, L3, &cls) == nullptr && cls == ARG_INVALID, "accepted call");
        }
    printf("OK\n");
    return 0;
}
