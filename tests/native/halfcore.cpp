// Host build of the float16 path's arithmetic (csrc/wt_half_core.h): the key, the two histogram
// passes and their rank searches, NumPy's float16 percentile rule, the mask and the conversions,
// exactly as the kernels of csrc/half.hip run them.  tests/test_half_core.py loads it as a shared
// object; built as a program, main() reads cases from stdin and writes results to stdout, or with
// no input checks itself against std::sort (a sanitizer build of the program needs nothing else).
//   g++ -O2 -std=c++17 -ffp-contract=off [-shared -fPIC] halfcore.cpp
// Input, one case a line:  n r0 above gamma_hex w0 w1 ... (words as decimal integers)
// Output, one line a case: thr64_hex ckey maxkey zero_count out0 out1 ...
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../wavelettransforms_amd/csrc/wt_half_core.h"

extern "C" {

// The selection of half.hip over words[0 .. n): keys[0..2] = the keys of rank r0, of rank
// r0 + 1 (r0 under `above`) and of rank n - 1, found by the 11 + 4 bit passes.  Returns 0, -1 on
// a bad argument.
int half_core_select(const uint16_t* words, long long n, long long r0, int above, uint32_t* keys) {
    if (n < 1 || r0 < 0 || r0 >= n || (!above && r0 + 1 >= n)) return -1;
    const long long rank[H16_NRANK] = {r0, above ? r0 : r0 + 1, n - 1};
    std::vector<uint32_t> h1(H16_BINS1, 0u);
    for (long long i = 0; i < n; ++i) ++h1[h16_digit1(h16_key(words[i]))];
    // the groups' inclusive prefix sums, as k_h16_scan1's 256 threads hold them (8 bins a thread)
    const int per = H16_BINS1 / 256;
    std::vector<uint32_t> gincl(H16_BINS1 / per);
    uint32_t run = 0;
    for (int g = 0; g < H16_BINS1 / per; ++g) {
        for (int k = 0; k < per; ++k) run += h1[g * per + k];
        gincl[g] = run;
    }
    uint32_t d1[H16_NRANK], resid[H16_NRANK];
    for (int j = 0; j < H16_NRANK; ++j) {
        d1[j] = (uint32_t)h16_locate_grouped(h1.data(), gincl.data(), H16_BINS1, per, (uint32_t)rank[j], &resid[j]);
        uint32_t flat_res;
        if ((uint32_t)h16_locate(h1.data(), H16_BINS1, (uint32_t)rank[j], &flat_res) != d1[j] || flat_res != resid[j]) return -2;
    }
    uint32_t h2[H16_NRANK][H16_BINS2] = {};
    for (long long i = 0; i < n; ++i) {
        const uint32_t key = h16_key(words[i]);
        for (int j = 0; j < H16_NRANK; ++j)
            if (h16_digit1(key) == d1[j]) ++h2[j][h16_digit2(key)];
    }
    for (int j = 0; j < H16_NRANK; ++j) {
        uint32_t r;
        keys[j] = h16_join(d1[j], (uint32_t)h16_locate(h2[j], H16_BINS2, resid[j], &r));
    }
    return 0;
}

// One kind-B tensor end to end: the selection, the threshold, the mask.  out may be words.
int half_core_prune(const uint16_t* words, long long n, long long r0, int above, double gamma, uint16_t* out,
                    double* thr64, uint32_t* ckey, uint32_t* maxkey, long long* zeros) {
    uint32_t k[H16_NRANK];
    const int rc = half_core_select(words, n, r0, above, k);
    if (rc) return rc;
    *ckey = h16_threshold(k[0], k[1], k[2], gamma, above, thr64);
    *maxkey = k[2];
    long long z = 0;
    for (long long i = 0; i < n; ++i) {
        out[i] = h16_mask(words[i], *ckey);
        z += h16_is_zero(out[i]);
    }
    *zeros = z;
    return 0;
}

uint16_t half_core_from_double(double x) { return h16_from_double(x); }
uint16_t half_core_from_float(float x) { return h16_from_float(x); }
uint32_t half_core_to_float_bits(uint16_t h) { return h16_to_float_bits(h); }
uint16_t half_core_diff(uint32_t ka, uint32_t kb) { return h16_diff(ka, kb); }
void half_core_from_double_n(const double* x, long long n, uint16_t* out) {
    for (long long i = 0; i < n; ++i) out[i] = h16_from_double(x[i]);
}
void half_core_from_float_n(const float* x, long long n, uint16_t* out) {
    for (long long i = 0; i < n; ++i) out[i] = h16_from_float(x[i]);
}
void half_core_split(unsigned long long addr, long long n, long long* head, long long* nvec, long long* tail) {
    const h16_span s = h16_split(addr, n);
    *head = s.head;
    *nvec = s.nvec;
    *tail = s.tail;
}

}  // extern "C"

namespace {

int self_check() {
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    // every half survives the round trip through float32 and float64
    for (uint32_t h = 0; h < 65536; ++h) {
        const uint32_t fb = h16_to_float_bits((uint16_t)h);
        float f;
        memcpy(&f, &fb, 4);
        const bool nan = (h & 0x7FFF) > 0x7C00;
        if (!nan && (h16_from_float(f) != h || h16_from_double((double)f) != h)) {
            printf("halfcore: round trip of 0x%04x failed\n", h);
            return 1;
        }
    }
    for (int trial = 0; trial < 60; ++trial) {
        const long long n = 1 + (long long)(next() % (trial < 30 ? 40 : 70000));
        std::vector<uint16_t> w(n), srt(n);
        const uint32_t span = trial % 3 == 0 ? 0x40 : (trial % 3 == 1 ? 0x7C00 : 0x8000); // ties, every finite key, or inf and NaN keys too
        for (auto& x : w) x = (uint16_t)((next() % span) | ((next() & 1) << 15));
        for (long long i = 0; i < n; ++i) srt[i] = (uint16_t)h16_key(w[i]);
        std::sort(srt.begin(), srt.end());
        const long long r0 = (long long)(next() % n);
        const int above = r0 == n - 1;
        uint32_t k[H16_NRANK];
        if (half_core_select(w.data(), n, r0, above, k) != 0 || k[0] != srt[r0] || k[1] != srt[above ? r0 : r0 + 1] ||
            k[2] != srt[n - 1]) {
            printf("halfcore: selection failed at trial %d (n = %lld, r0 = %lld)\n", trial, n, r0);
            return 1;
        }
    }
    printf("halfcore: ok\n");
    return 0;
}

}  // namespace

int main() {
    char* line = nullptr;
    size_t cap = 0;
    long cases = 0;
    while (getline(&line, &cap, stdin) > 0) {
        char* p = line;
        const long long n = strtoll(p, &p, 10), r0 = strtoll(p, &p, 10);
        const int above = (int)strtol(p, &p, 10);
        const double gamma = strtod(p, &p);
        if (n < 1) continue;
        std::vector<uint16_t> w(n), out(n);
        for (auto& x : w) x = (uint16_t)strtoul(p, &p, 10);
        double thr64;
        uint32_t ckey, maxkey;
        long long zeros;
        if (half_core_prune(w.data(), n, r0, above, gamma, out.data(), &thr64, &ckey, &maxkey, &zeros) != 0) {
            printf("error\n");
            free(line);
            return 2;
        }
        printf("%a %u %u %lld", thr64, ckey, maxkey, zeros);
        for (auto x : out) printf(" %u", (unsigned)x);
        printf("\n");
        ++cases;
    }
    free(line);
    return cases ? 0 : self_check();
}
