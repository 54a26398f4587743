// The host-only context tables (fhs_tables.h build_host_tables) against the identities that define them, on the
// context shapes of the GPU parity and edge-operand tests plus the special = 8 limit.  Prints one 64-bit digest
// (FNV-1a over the table's bytes) per table and shape, then OK.
// Build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Itools/debug/shim
//        -Ifhe-spear_amd/csrc tools/debug/tables_check.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fhs_tables.h"
typedef unsigned __int128 u128c;
static uint64_t mm(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((u128c)a * b % q); }
static uint64_t shoup(uint64_t w, uint64_t q) { return (uint64_t)(((u128c)w << 64) / q); }
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            printf("FAIL shape %s line %d: %s\n", g_shape, __LINE__, #cond);         \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)
static const char* g_shape = "";

static void digest(const char* name, const void* data, size_t bytes) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 1099511628211ull;
    printf("%s %-10s %016llx\n", g_shape, name, (unsigned long long)h);
}
template <class T>
static void digest(const char* name, const std::vector<T>& v) {
    digest(name, v.data(), v.size() * sizeof(T));
}

struct Shape {
    const char* name;
    uint64_t N;
    std::vector<int> bits;   // data primes, then the special ones
    int P;
    bool all59;
};

static void run(const Shape& s) {
    g_shape = s.name;
    const int K = (int)s.bits.size(), P = s.P, L0 = K - P;
    const uint64_t N = s.N;
    std::vector<uint64_t> q(K);
    CHECK(coeff_modulus_search(N, s.bits.data(), K, q.data()));
    CHECK(context_params_error(N, q.data(), K, P, nullptr, 0) == nullptr);
    HostTables H;
    CHECK(build_host_tables(N, q.data(), K, P, H) == nullptr);
    const int dnum = H.dnum;
    CHECK(H.L0 == L0 && H.K == K && H.P == P && (1ull << H.logN) == N && dnum == (L0 + P - 1) / P);

    for (int i = 0; i < K; ++i) {
        const uint64_t* f = &H.tw_fwd[(size_t)i * N * 2];
        const uint64_t* v = &H.tw_inv[(size_t)i * N * 2];
        for (uint64_t k = 0; k < N; ++k) {
            CHECK(mm(f[2 * k], v[2 * k], q[i]) == 1);
            CHECK(f[2 * k + 1] == shoup(f[2 * k], q[i]) && v[2 * k + 1] == shoup(v[2 * k], q[i]));
        }
        uint64_t x = f[2 * (N / 2)];   // bit-reversed index 1: psi, a primitive 2N-th root
        for (uint64_t e = 1; e < N; e <<= 1) x = mm(x, x, q[i]);
        CHECK(x == q[i] - 1);
        const PrimeK& pk = H.primes[i];
        const u128c R = (~(u128c)0) / q[i];
        CHECK(pk.q == q[i] && pk.r0 == (uint64_t)R && pk.r1 == (uint64_t)(R >> 64));
        CHECK(mm(pk.ninv, N % q[i], q[i]) == 1 && pk.ninv_s == shoup(pk.ninv, q[i]));
        CHECK(pk.w1ninv == mm(v[2], pk.ninv, q[i]) && pk.w1ninv_s == shoup(pk.w1ninv, q[i]));
        for (int e = 0; e + 1 < kPow2Words; ++e)
            CHECK(H.pow2[(size_t)i * kPow2Words + e + 1] == mm(H.pow2[(size_t)i * kPow2Words + e], 2, q[i]));
        CHECK(H.pow2[(size_t)i * kPow2Words] == 1);
    }
    for (int l = 1; l <= L0; ++l)
        for (int j = 0; j < (l + P - 1) / P; ++j) {
            const int s0 = j * P, ns = (s0 + P < l ? s0 + P : l) - s0;
            const size_t lj = (size_t)l * dnum + j;
            for (int u = 0; u < ns; ++u) {
                const int i = s0 + u;
                const uint64_t* hat = &H.modup_hat[(lj * P + u) * K];
                for (int t = 0; t < K; ++t) {
                    const uint64_t* Q = &H.modup_Q[(lj * K + t) * 2];
                    CHECK(Q[0] == mm(hat[t], q[i] % q[t], q[t]));
                    CHECK(Q[1] == mm(Q[0], (uint64_t)ns, q[t]));
                }
                const uint64_t* d = &H.modup_intt[((size_t)l * L0 + i) * 4];
                CHECK(mm(mm(d[0], N % q[i], q[i]), hat[i], q[i]) == 1);
                CHECK(d[2] == mm(d[0], H.tw_inv[((size_t)i * N + 1) * 2], q[i]));
                CHECK(d[1] == shoup(d[0], q[i]) && d[3] == shoup(d[2], q[i]));
                const u128c R = (~(u128c)0) / q[i];
                CHECK(H.modup_R[(lj * P + u) * 2] == (uint64_t)R && H.modup_R[(lj * P + u) * 2 + 1] == (uint64_t)(R >> 64));
            }
        }
    for (int i = 0; i < L0; ++i) {
        CHECK(mm(H.md_pinv[2 * i], H.md_pinv[2 * L0 + i], q[i]) == 1);
        CHECK(H.md_pinv[2 * i + 1] == shoup(H.md_pinv[2 * i], q[i]));
        for (int k = 0; k < P; ++k)
            CHECK(mm(H.md_hat[(size_t)k * L0 + i], q[L0 + k] % q[i], q[i]) == H.md_pinv[2 * L0 + i]);
    }
    for (int k = 0; k < P; ++k) {
        const uint64_t* d = &H.md_intt[(size_t)k * 4];
        CHECK(d[1] == shoup(d[0], q[L0 + k]) && d[3] == shoup(d[2], q[L0 + k]));
    }
    for (int l = 2; l <= L0; ++l)
        for (int i = 0; i < l - 1; ++i) {
            const uint64_t* d = &H.rescale[((size_t)l * L0 + i) * 4];
            CHECK(mm(d[0], q[l - 1] % q[i], q[i]) == 1 && d[1] == shoup(d[0], q[i]));
            CHECK(d[3] == q[l - 1] >> 1 && d[2] == d[3] % q[i]);
        }
    CHECK(H.modup_dp == (P == 3 ? 3 : P == 1 ? 1 : 0));
    CHECK((H.all_b59 != 0) == s.all59);

    digest("primes", H.primes);
    digest("tw_fwd", H.tw_fwd);
    digest("tw_inv", H.tw_inv);
    digest("modup_intt", H.modup_intt);
    digest("modup_hat", H.modup_hat);
    digest("modup_R", H.modup_R);
    digest("modup_Q", H.modup_Q);
    digest("modup_xd", H.modup_xd);
    digest("modup_xt", H.modup_xt);
    digest("md_xd", H.md_xd);
    digest("md_intt", H.md_intt);
    digest("md_hat", H.md_hat);
    digest("md_pinv", H.md_pinv);
    digest("rescale", H.rescale);
    digest("pow2", H.pow2);
    digest("enc_w", H.enc_w);
    digest("enc_twist", H.enc_twist);
    digest("enc_pos", H.enc_pos);
    digest("dec_w", H.dec_w);
    digest("dec_twist", H.dec_twist.data(), 16 * (size_t)(N / 2));   // the half the GPU decoder gets
    digest("dec_twist_h", H.dec_twist);
    digest("dec_pos", H.dec_pos);
    digest("fft_w", H.fft_w);
    digest("slot_index", H.slot_index);
    const std::vector<int> flags = {H.max_qbits, H.modup_dp, H.md_xform, H.conv_b59, H.all_b59};
    digest("flags", flags);
}

int main() {
    auto bits = [](int n, int b) { return std::vector<int>(n, b); };
    std::vector<int> mixed = bits(4, 59);
    mixed.push_back(60);
    const Shape shapes[] = {
        {"256/6+3/59", 256, bits(9, 59), 3, true},
        {"1024/6+3/60", 1024, bits(9, 60), 3, false},
        {"1024/4+2/59", 1024, bits(6, 59), 2, true},
        {"1024/4+1/59,60", 1024, mixed, 1, false},
        {"1024/36+3/59", 1024, bits(39, 59), 3, true},
        {"256/8+8/59", 256, bits(16, 59), 8, true},
        {"32768/3+3/59", 32768, bits(6, 59), 3, true},
        {"8192/3+1/60,40,40,60", 8192, {60, 40, 40, 60}, 1, false},
    };
    for (const Shape& s : shapes) run(s);
    printf("OK\n");
    return 0;
}
