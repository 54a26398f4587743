// xcd_map_check.cpp -- host-side proof of the block maps in fhe-spear_amd/csrc/fhs_xcdmap.h.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I fhe-spear_amd/csrc tools/debug/xcd_map_check.cpp -o xcd_map_check && ./xcd_map_check
// For every map, over E = 1..48, M in {1, 2, 3, 12, 45, 64, 528}, NB in {1, 2, 64}:
//   - every pair of the domain is produced by exactly one block of the grid, no block produces a pair outside it;
//   - the per-XCD balance the map's comment states (block b runs on XCD b & 7);
//   - k_ks_ip's map keeps all blocks of one limb on one XCD.
// Prints one line per map, then OK; exits non-zero at the first violated property.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fhs_xcdmap.h"

using namespace fhs;

static const int kM[] = {1, 2, 3, 12, 45, 64, 528};
static const int kNB[] = {1, 2, 64};

#define REQUIRE(cond, ...)                                  \
    do {                                                    \
        if (!(cond)) {                                      \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                   \
            fprintf(stderr, "\n");                          \
            exit(1);                                        \
        }                                                   \
    } while (0)

struct Spread {
    long long lo, hi;
};
static Spread spread(const long long* v) {
    Spread s{v[0], v[0]};
    for (int x = 1; x < kXcds; ++x) {
        s.lo = v[x] < s.lo ? v[x] : s.lo;
        s.hi = v[x] > s.hi ? v[x] : s.hi;
    }
    return s;
}

// a (t, m) map over the domain [0, E) x [0, M): exact cover; per-XCD counts of produced pairs in cnt
template <class Map>
static void cover(const char* name, int grid, int E, int M, Map map, long long* cnt) {
    std::vector<unsigned char> seen((size_t)E * M, 0);
    for (int x = 0; x < kXcds; ++x) cnt[x] = 0;
    for (int b = 0; b < grid; ++b) {
        int t = -1, m = -1;
        if (!map(b, t, m)) continue;
        REQUIRE(t >= 0 && t < E && m >= 0 && m < M, "%s E=%d M=%d: block %d gives (%d, %d) outside the domain", name, E, M,
                b, t, m);
        REQUIRE(!seen[(size_t)m * E + t], "%s E=%d M=%d: (%d, %d) produced twice (block %d)", name, E, M, t, m, b);
        seen[(size_t)m * E + t] = 1;
        ++cnt[b & 7];
    }
    for (int m = 0; m < M; ++m)
        for (int t = 0; t < E; ++t) REQUIRE(seen[(size_t)m * E + t], "%s E=%d M=%d: (%d, %d) never produced", name, E, M, t, m);
}

int main() {
    long long cnt[kXcds];
    long long cases = 0;

    // plain (k_ks_ip_sum over (limb, n-block); k_ks_ip's special limbs; k_moddown): no padding, XCDs within one block
    for (int E = 1; E <= 48; ++E)
        for (int M : kM)
            for (int NB : kNB) {
                const int MM = M * NB;
                cover("plain_tm", plain_grid(E, MM), E, MM, [&](int b, int& t, int& m) { return plain_tm(b, E, MM, t, m); },
                      cnt);
                const Spread s = spread(cnt);
                REQUIRE(s.hi - s.lo <= 1, "plain_tm E=%d M=%d: XCD counts %lld..%lld", E, MM, s.lo, s.hi);
                ++cases;
            }
    printf("plain_tm      ok (%lld cases): exact cover, XCD block counts within 1\n", cases);

    // limbs mod 8 (k_modup, N = 256): exact cover; an XCD's share is its limbs' (ceil or floor of E/8) x M
    cases = 0;
    for (int E = 1; E <= 48; ++E)
        for (int M : kM) {
            cover("xcd_tinner", xcd_grid(E, M), E, M, [&](int b, int& t, int& m) { return xcd_tinner(b, E, M, t, m); }, cnt);
            const Spread s = spread(cnt);
            REQUIRE(s.hi - s.lo <= M, "xcd_tinner E=%d M=%d: XCD counts %lld..%lld", E, M, s.lo, s.hi);
            ++cases;
        }
    printf("xcd_tinner    ok (%lld cases): exact cover, XCDs within one limb\n", cases);

    // limbs mod 8, one limb at a time (k_ks_ip, t0 = 0): exact cover; XCDs within one limb (M blocks); all blocks
    // of a limb on one XCD, and consecutive there (the limb's extension is in that L2 while its rotations run)
    cases = 0;
    for (int E = 1; E <= 48; ++E)
        for (int M : kM)
            for (int NB : kNB) {
                const int MM = M * NB;
                std::vector<int> owner(E, -1), first(E, -1), last(E, -1);
                cover("xcd_touter", xcd_grid(E, MM), E, MM,
                      [&](int b, int& t, int& m) {
                          if (!xcd_touter(b, E, MM, t, m)) return false;
                          REQUIRE(t >= 0 && t < E, "xcd_touter E=%d M=%d: block %d gives limb %d", E, MM, b, t);
                          REQUIRE(owner[t] < 0 || owner[t] == (b & 7), "xcd_touter E=%d M=%d: limb %d on XCDs %d and %d", E, MM,
                                  t, owner[t], b & 7);
                          owner[t] = b & 7;
                          if (first[t] < 0) first[t] = b >> 3;
                          last[t] = b >> 3;
                          return true;
                      },
                      cnt);
                for (int t = 0; t < E; ++t)
                    REQUIRE(last[t] - first[t] == MM - 1, "xcd_touter E=%d M=%d: limb %d spread over %d of its XCD's blocks", E,
                            MM, t, last[t] - first[t] + 1);
                const Spread s = spread(cnt);
                REQUIRE(s.hi - s.lo <= MM, "xcd_touter E=%d M=%d: XCD counts %lld..%lld", E, MM, s.lo, s.hi);
                ++cases;
            }
    printf("xcd_touter    ok (%lld cases): exact cover, one XCD per limb, XCDs within one limb\n", cases);

    // ModUp: E = l + P, inputs M = dn U with U from the M list; the three parts.  Real workgroups = produced pairs
    // that are not a digit's own limb.
    cases = 0;
    long long levelled = 0;
    for (int P = 1; P <= 4; ++P)
        for (int E = P + 1; E <= 48; ++E)
            for (int U : kM) {
                const int l = E - P, dn = (E - 1) / P, M = dn * U;
                long long real[3][kXcds];
                for (int part = 0; part < 3; ++part) {
                    const ModupMap mp = modup_map_build(l, P, U, part);
                    const int t_lo = part == kModupSpecial ? l : 0, t_hi = part == kModupData ? l : E;
                    for (int x = 0; x < kXcds; ++x) real[part][x] = 0;
                    REQUIRE(mp.grid % kXcds == 0 && mp.sp[kXcds] == (part == kModupData ? 0 : P * M),
                            "modup_map l=%d P=%d U=%d part=%d: grid %d, %d special pairs", l, P, U, part, mp.grid, mp.sp[kXcds]);
                    cover("modup_map", mp.grid, t_hi - t_lo, M,
                          [&](int b, int& t, int& m) {
                              if (!modup_map(mp, b, l, P, t, m)) return false;
                              REQUIRE(t >= t_lo && t < t_hi, "modup_map l=%d P=%d U=%d part=%d: block %d gives limb %d", l, P, U,
                                      part, b, t);
                              const int j = m % dn, s0 = j * P, s1 = s0 + P < l ? s0 + P : l;
                              if (!(t >= s0 && t < s1)) ++real[part][b & 7];
                              t -= t_lo;
                              return true;
                          },
                          cnt);
                    ++cases;
                }
                const Spread all = spread(real[kModupAll]), sp = spread(real[kModupSpecial]), da = spread(real[kModupData]);
                REQUIRE(sp.hi - sp.lo <= 1, "modup_map l=%d P=%d U=%d: special part %lld..%lld", l, P, U, sp.lo, sp.hi);
                // the special pairs level the data limbs' spread where they suffice; elsewhere they only narrow it
                long long deficit = 0;
                for (int x = 0; x < kXcds; ++x) deficit += da.hi - real[kModupData][x];
                if ((long long)P * M >= deficit) {
                    REQUIRE(all.hi - all.lo <= 1, "modup_map l=%d P=%d U=%d: real workgroups %lld..%lld with %d special pairs "
                            "for a deficit of %lld", l, P, U, all.lo, all.hi, P * M, deficit);
                    ++levelled;
                } else {
                    REQUIRE(all.hi == da.hi && all.lo >= da.lo && all.hi - all.lo <= da.hi - da.lo,
                            "modup_map l=%d P=%d U=%d: real workgroups %lld..%lld, data limbs alone %lld..%lld", l, P, U, all.lo,
                            all.hi, da.lo, da.hi);
                }
                // one target limb's worth per XCD (ceil(M / 2) workgroups) wherever both input halves have work
                if (P == 3 && M >= 2 && l >= 4)
                    REQUIRE(all.hi - all.lo <= (M + 1) / 2, "modup_map l=%d P=%d U=%d: real workgroups %lld..%lld, a limb is %d", l,
                            P, U, all.lo, all.hi, (M + 1) / 2);
            }
    printf("modup_map     ok (%lld cases, %lld levelled to within 1): exact cover per part, balance after the own-limb skip\n",
           cases, levelled);
    {   // the flagship shape: l = 36, P = 3, 44 giant inputs and the baby input alone
        for (int U : {44, 1}) {
            const ModupMap mp = modup_map_build(36, 3, U, kModupAll);
            printf("  l=36 P=3 U=%-2d grid %d, special pairs per XCD:", U, mp.grid);
            for (int x = 0; x < kXcds; ++x) printf(" %d", mp.sp[x + 1] - mp.sp[x]);
            printf("\n");
        }
    }
    printf("OK\n");
    return 0;
}
