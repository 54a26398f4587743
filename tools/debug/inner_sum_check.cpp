// inner_sum_check.cpp -- host-side check of fhs_inner_sum_many's argument validation and step list
// (fhe-spear_amd/csrc/fhs_tables.h inner_sum_steps) against the loop it stands for,
//   step = 1; while step < dim: rotate by stride * step; step *= 2        (fhe_rwkv_inference.py ct_pt_dot)
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Itools/debug/shim \
//       -Ifhe-spear_amd/csrc tools/debug/inner_sum_check.cpp -o inner_sum_check && ./inner_sum_check
// For every N = 256..32768, every dim = 1..64 (and N/2, N/2 + 1, N), strides {1, 2, 3, 4, 7, 64, N/4 - 1, N/4,
// N/2 - 1, N/2}: the accepted calls give exactly the loop's steps, each a rotation fhs_rotate accepts; a call is
// rejected exactly when the loop's largest step is no such rotation; n, dim, stride < 1 are rejected with their own
// messages and leave no steps.  Prints one line per N, then OK; exits non-zero at the first violated property.
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

int main() {
    std::vector<int> steps;
    for (uint64_t N = 256; N <= 32768; N <<= 1) {
        const long long slots = (long long)N / 2;
        std::vector<int> dims;
        for (int d = 1; d <= 64; ++d) dims.push_back(d);
        for (long long d : {slots, slots + 1, (long long)N}) dims.push_back((int)d);
        const long long strides[] = {1, 2, 3, 4, 7, 64, slots / 2 - 1, slots / 2, slots - 1, slots};
        long long ok = 0, rejected = 0;
        for (int dim : dims)
            for (long long stride : strides) {
                std::vector<long long> want;
                for (long long s = 1; s < dim; s *= 2) want.push_back(stride * s);
                const bool legal = want.empty() || want.back() < slots;
                steps.assign(3, -1);   // stale content must not survive
                const char* err = inner_sum_steps(1, dim, (int)stride, N, steps);
                REQUIRE((err == nullptr) == legal, "N=%llu dim=%d stride=%lld: %s", (unsigned long long)N, dim, stride,
                        err ? err : "accepted");
                if (!legal) {
                    REQUIRE(steps.empty() && strstr(err, "largest step"), "N=%llu dim=%d stride=%lld: %zu steps, \"%s\"",
                            (unsigned long long)N, dim, stride, steps.size(), err);
                    ++rejected;
                    continue;
                }
                REQUIRE(steps.size() == want.size(), "N=%llu dim=%d stride=%lld: %zu steps for %zu", (unsigned long long)N,
                        dim, stride, steps.size(), want.size());
                for (size_t k = 0; k < want.size(); ++k)
                    REQUIRE(steps[k] == want[k] && steps[k] >= 1 && steps[k] < slots, "N=%llu dim=%d stride=%lld: step %zu is %d",
                            (unsigned long long)N, dim, stride, k, steps[k]);
                ++ok;
            }
        REQUIRE(ok > 0 && rejected > 0, "N=%llu: %lld accepted, %lld rejected", (unsigned long long)N, ok, rejected);
        // the other rejections, each with its own message and no steps; the extremes of int do not overflow
        struct Bad {
            int n, dim, stride;
            const char* word;
        };
        const Bad bad[] = {{0, 8, 1, "n >= 1"},      {-1, 8, 1, "n >= 1"},          {1, 0, 1, "dim >= 1"},
                           {1, -5, 1, "dim >= 1"},   {1, 8, 0, "stride >= 1"},      {1, 8, -2, "stride >= 1"},
                           {1, 2, 0x7fffffff, "largest step"}, {1, 0x7fffffff, 0x7fffffff, "largest step"},
                           {1, 0x7fffffff, 1, "largest step"}};
        for (const Bad& b : bad) {
            steps.assign(2, 7);
            const char* err = inner_sum_steps(b.n, b.dim, b.stride, N, steps);
            REQUIRE(err && strstr(err, b.word) && steps.empty(), "N=%llu n=%d dim=%d stride=%d: \"%s\", %zu steps",
                    (unsigned long long)N, b.n, b.dim, b.stride, err ? err : "accepted", steps.size());
        }
        // dim = 1: copies, whatever the stride
        REQUIRE(inner_sum_steps(513, 1, 0x7fffffff, N, steps) == nullptr && steps.empty(), "N=%llu dim=1", (unsigned long long)N);
        // the largest legal stride for dim = 2
        REQUIRE(inner_sum_steps(1, 2, (int)slots - 1, N, steps) == nullptr && steps.size() == 1 && steps[0] == slots - 1,
                "N=%llu dim=2 stride=%lld", (unsigned long long)N, slots - 1);
        printf("N=%-5llu ok: %lld accepted step lists equal the loop's, %lld rejected\n", (unsigned long long)N, ok, rejected);
    }
    printf("OK\n");
    return 0;
}
