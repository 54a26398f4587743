// fhs_xcdmap.h -- block index -> (target limb, item) maps of the key-switch kernels.  Plain functions of the
// block index (the kernels pass blockIdx.x), shared by the device code, the launchers' grid sizes and the
// host-side checker (tools/debug/xcd_map_check.cpp), which proves for every map that each pair of its domain
// is produced by exactly one block of the grid, and the balance stated with each map.
//
// Workgroups are dealt round-robin over the 8 XCDs (observed placement; speed only, never correctness), so
// block b runs on XCD b & 7 and an XCD's k-th block is b = x + 8 k.  A map returns false for padding blocks.
#pragma once

#if defined(__HIPCC__)
#define FHS_HD __host__ __device__ __forceinline__
#else
#define FHS_HD inline
#endif

namespace fhs {

constexpr int kXcds = 8;

// plain: b = t + E m (t fastest).  Grid E M, no padding: per-XCD block counts differ by at most one.
FHS_HD int plain_grid(int E, int M) { return E * M; }
FHS_HD bool plain_tm(int b, int E, int M, int& t, int& m) {
    t = b % E;
    m = b / E;
    return m < M;
}

// XCD x takes the limbs t == x (mod 8): its L2 holds ~E/8 primes' twiddle tables instead of all E.
// Grid 8 ceil(E/8) M.  t-inner: an XCD cycles its limbs fastest (blocks sharing an input m run together).
FHS_HD int xcd_grid(int E, int M) { return kXcds * ((E + 7) / 8) * M; }
FHS_HD bool xcd_tinner(int b, int E, int M, int& t, int& m) {
    const int x = b & 7, k = b >> 3, nx = (E - x + 7) >> 3;
    if (nx <= 0 || k >= nx * M) return false;
    t = x + 8 * (k % nx);
    m = k / nx;
    return true;
}

// t-outer (k_ks_ip, hoisted rotations of one input): XCD x takes the limbs t == x (mod 8) and finishes one limb
// across all its items m before the next, so the limb's share of the extension, which every rotation reads,
// stays hot in that XCD's L2.  Grid as xcd_grid; XCDs within one limb (M blocks) of each other.
// (A finer unit -- half a limb per XCD, 2 E units over 8 XCDs -- balances better and ran 5 % slower: DESIGN.md
// section 3.)
FHS_HD bool xcd_touter(int b, int E, int M, int& t, int& m) {
    const int x = b & 7, k = b >> 3, nx = (E - x + 7) >> 3;
    if (nx <= 0 || k >= nx * M) return false;
    t = x + 8 * (k / M);
    m = k % M;
    return true;
}

// ModUp (k_modup_h): pairs (target limb t < E = l + P, input m < M = dn U; m = digit + dn * ciphertext).
// Data limbs keep four twiddle classes: XCD x takes the limbs t == x & 3 (mod 4), t < l, of the inputs
// m == x >> 2 (mod 2), t fastest -- ~l/4 primes' twiddle tables per L2, each input read by 4 XCDs.  A digit's
// own limbs are skipped by the kernel (the key product reads them from the input itself), and class sizes
// differ, so the XCDs' real workgroup counts differ: the P M special-limb pairs, which are never skipped,
// fill the short XCDs up (modup_map_build: each pair to the XCD with the fewest real workgroups so far).
// XCD x takes the contiguous run [sp[x], sp[x + 1]) of the special pairs in the order s = P m + k (limb l + k): the P
// targets of one input follow each other on one XCD, so its digit is read from HBM once.
// Balance: the real counts differ by at most 1 wherever the special pairs suffice to level the data limbs'
// spread; elsewhere the spread is no larger than that of the data limbs alone.
// part: kModupAll, or one half of a launch split in two: kModupSpecial (t >= l only, dealt evenly) and
// kModupData (t < l only).
enum ModupPart { kModupAll = 0, kModupSpecial = 1, kModupData = 2 };
struct ModupMap {
    int nd[kXcds];       // blocks of the XCD's data-limb section (own-limb blocks included)
    int sp[kXcds + 1];   // its run of special pairs
    int grid;
};
// data limbs of class pg that an input of digit j really extends (the digit's own limbs excluded)
FHS_HD int modup_real_limbs(int l, int P, int j, int pg) {
    const int s0 = j * P, s1 = s0 + P < l ? s0 + P : l;
    int n = 0;
    for (int t = pg; t < l; t += 4) n += !(t >= s0 && t < s1);
    return n;
}
inline ModupMap modup_map_build(int l, int P, int U, int part) {
    const int E = l + P, dn = (E - 1) / P, M = dn * U;
    ModupMap mp;
    long long real[kXcds];
    int cnt[kXcds];
    for (int x = 0; x < kXcds; ++x) {
        const int pg = x & 3, mh = x >> 2;
        const int nxd = l > pg ? (l - pg + 3) >> 2 : 0, nm = M > mh ? (M - mh + 1) >> 1 : 0;
        mp.nd[x] = part == kModupSpecial ? 0 : nxd * nm;
        real[x] = 0;
        cnt[x] = 0;
        if (part == kModupSpecial) continue;
        for (int j = 0; j < dn; ++j) {   // inputs m = j + dn u, u < U, with m == mh (mod 2)
            const int same = (j & 1) == mh;
            const int nu = dn & 1 ? (U + same) / 2 : same * U;
            real[x] += (long long)nu * modup_real_limbs(l, P, j, pg);
        }
    }
    const long long S = part == kModupData ? 0 : (long long)P * M;
    // water-filling: raise the lowest XCDs together.  Level by level instead of pair by pair (S is up to
    // thousands): find the lowest level every pair fits under, then deal the remainder one each from XCD 0
    long long left = S;
    for (;;) {
        long long lo = real[0] + cnt[0], next = -1;
        for (int x = 1; x < kXcds; ++x) lo = real[x] + cnt[x] < lo ? real[x] + cnt[x] : lo;
        int nlo = 0;
        for (int x = 0; x < kXcds; ++x) {
            const long long v = real[x] + cnt[x];
            if (v == lo) ++nlo;
            else if (next < 0 || v < next) next = v;
        }
        if (left <= 0) break;
        long long rise = next < 0 ? (left + nlo - 1) / nlo : next - lo;   // per XCD at the low level
        if (rise * nlo > left) rise = left / nlo;
        if (rise == 0) {   // fewer pairs left than XCDs at the low level: one each
            for (int x = 0; x < kXcds && left > 0; ++x)
                if (real[x] + cnt[x] == lo) { ++cnt[x]; --left; }
            break;
        }
        for (int x = 0; x < kXcds; ++x)
            if (real[x] + cnt[x] == lo) cnt[x] += (int)rise;
        left -= rise * nlo;
    }
    mp.sp[0] = 0;
    int g = 0;
    for (int x = 0; x < kXcds; ++x) {
        mp.sp[x + 1] = mp.sp[x] + cnt[x];
        g = mp.nd[x] + cnt[x] > g ? mp.nd[x] + cnt[x] : g;
    }
    mp.grid = kXcds * g;
    return mp;
}
FHS_HD bool modup_map(const ModupMap& mp, int b, int l, int P, int& t, int& m) {
    const int x = b & 7, pg = x & 3, mh = x >> 2;
    int k = b >> 3;
    if (k < mp.nd[x]) {
        const int nxd = (l - pg + 3) >> 2;
        t = pg + 4 * (k % nxd);
        m = mh + 2 * (k / nxd);
        return true;
    }
    k -= mp.nd[x];
    if (k >= mp.sp[x + 1] - mp.sp[x]) return false;
    const int s = mp.sp[x] + k;
    t = l + s % P;
    m = s / P;
    return true;
}

}  // namespace fhs
