// Sanitizer driver for the global percentile's host-compilable core (csrc/wt_global_core.h, via
// globalcore.cpp): random pools of four kinds cut at random into 1 to 30 pieces (empty pieces
// among them) against std::sort of the concatenation, the overflow rule at its edge, and the
// record layout.  Built and run by tests/test_global_core.py with -fsanitize=address,undefined
// -fno-sanitize-recover=all: any report aborts the run.
#include <cstdio>

#include "globalcore.cpp"

int main() {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        return x;
    };
    long cases = 0;
    int bad = 0;
    for (int trial = 0; trial < 48; ++trial) {
        const long long n = 1 + (long long)(next() % 60000);
        std::vector<uint32_t> keys(n);
        const int kind = trial % 4;
        for (auto& k : keys) {
            const uint64_t r = next();
            k = kind == 0 ? (uint32_t)(r & 0x7FFFFFFFu)                      // every bit pattern
                : kind == 1 ? (uint32_t)(0x3D000000u + (r & 0xFFFFFFu))      // one octave range
                : kind == 2 ? (uint32_t)(r % 5) * 0x00100401u                // five distinct values
                            : ((r & 3) ? 0u : (uint32_t)(r >> 33));           // 75 % zeros
        }
        const int npieces = 1 + (int)(next() % 30);
        std::vector<long long> cut(npieces + 1, 0), len(npieces);
        cut[npieces] = n;
        for (int p = 1; p < npieces; ++p) cut[p] = (long long)(next() % (uint64_t)(n + 1));
        std::sort(cut.begin(), cut.end());
        for (int p = 0; p < npieces; ++p) len[p] = cut[p + 1] - cut[p];
        uint32_t ranks[SW_MAX_RANKS], sel[SW_MAX_RANKS], mk;
        const int nranks = 1 + (int)(next() % SW_MAX_RANKS);
        for (int i = 0; i < nranks; ++i) ranks[i] = (uint32_t)(next() % (uint64_t)n);
        if (trial & 1) { ranks[0] = 0; ranks[nranks - 1] = (uint32_t)(n - 1); }
        int slots[2];
        if (global_core_select(keys.data(), len.data(), npieces, ranks, nranks, sel, slots, &mk)) { ++bad; continue; }
        std::vector<uint32_t> sorted(keys);
        std::sort(sorted.begin(), sorted.end());
        for (int i = 0; i < nranks; ++i) bad += sel[i] != sorted[ranks[i]];
        bad += mk != sorted.back() || slots[0] < 1 || slots[0] > nranks || slots[1] < slots[0] || slots[1] > nranks;
        ++cases;
    }
    // the overflow rule: 2^32 - 1 keys are a pool, one more is not; the sum is exact either way
    {
        const long long big = 0x7FFFFFFFll;
        const long long a[3] = {big, big, 1}, b[3] = {big, big, 2}, c[2] = {big + 1, big + 1};
        unsigned long long t = 0;
        bad += global_core_pool(a, 3, &t) != 1 || t != 0xFFFFFFFFull;
        bad += global_core_pool(b, 3, &t) != 0 || t != 0x100000000ull;
        bad += global_core_pool(c, 2, &t) != 0 || t != 0x100000000ull;
        bad += global_core_pool(a, 0, &t) != 1 || t != 0;
        cases += 4;
    }
    // the records: every (k, t) its own slot, the pool's values in each
    {
        const int npct = 3, nt = 5;
        std::vector<wtp_result> recs(npct * nt);
        memset(recs.data(), 0xAB, recs.size() * sizeof(wtp_result));
        std::vector<int> seen(npct * nt, 0);
        for (int k = 0; k < npct; ++k)
            for (int t = 0; t < nt; ++t) {
                const long long ri = global_core_record(recs.data(), k, nt, t, 100 + t, 200 + t, t % 3, 0.5 * k, 7u + k, 99u);
                bad += ri != (long long)k * nt + t;
                ++seen[ri];
                const wtp_result& r = recs[ri];
                bad += r.numel != 100 + t || r.coeff_numel != 200 + t || r.eff_level != t % 3 || r.zero_count != 0;
                bad += r.thr64 != 0.5 * k || r.thr32_bits != 7u + k || r.max_abs_bits != 99u || r.path != WTP_PATH_GLOBAL;
                ++cases;
            }
        for (int v : seen) bad += v != 1;
    }
    if (bad) {
        std::printf("sanglobal: FAILED (%d)\n", bad);
        return 1;
    }
    std::printf("sanglobal: %ld cases clean\n", cases);
    return 0;
}
