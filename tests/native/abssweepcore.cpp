// Host build of the two per-image routines of the absolute-threshold sweep's tiny-image kernel
// (csrc/wt_abs_sweep_core.h: abs_forward_raw and abs_inverse_masked, the body of k_abs_tiny_sweep)
// so the CPU suite can check them against the oracle and against abs_image without a GPU: one
// forward, then every threshold's inverse over the SAME arena.
// Built by tests/test_abs_sweep_core.py twice:
//   g++ -O2 -ffp-contract=off -shared -fPIC                      the library the test calls
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -DABS_SWEEP_MAIN
//                                                                a stand-alone program (below)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../wavelettransforms_amd/csrc/wt_abs_sweep_core.h"

// B images of H x W, NL at a time in an arena of EXACTLY abs_tiny_words(H, W, L) * NL words laid
// out like the kernel's (word s of image i of a group at s * NL + i): one abs_forward_raw per
// image, then for each of the nthr thresholds in turn abs_inverse_masked per image and the copy
// of A into outs[k] (at level 0 the copy masks, as the kernel's store pass does).  Returns the
// arena words one image needs.
extern "C" int abs_sweep_core_run(const float* in, float* outs, long long B, int H, int W, int L, int F, const float* taps,
                                  const float* thrs, int nthr, int NL) {
    const int aw = abs_area_a(H, W, L), tw = abs_area_t(H, W, L), dw = abs_area_d(H, W, L);
    std::vector<float> arena((size_t)(aw + tw + dw) * NL, -77.0f);
    float* A = arena.data();
    float* T = A + (size_t)aw * NL;
    float* D = T + (size_t)tw * NL;
    const long long HW = (long long)H * W;
    for (long long b0 = 0; b0 < B; b0 += NL) {
        const int n = (int)(B - b0 < NL ? B - b0 : NL);
        for (int i = 0; i < n; ++i)
            for (int s = 0; s < HW; ++s) A[(size_t)s * NL + i] = in[(b0 + i) * HW + s];
        for (int i = 0; i < n; ++i) abs_forward_raw(A + i, T + i, D + i, NL, H, W, L, F, taps, taps + F);
        for (int k = 0; k < nthr; ++k) {
            for (int i = 0; i < n; ++i)
                abs_inverse_masked(A + i, T + i, D + i, NL, H, W, L, F, taps + 2 * F, taps + 3 * F, thrs[k]);
            float* out = outs + (size_t)k * B * HW;
            for (int i = 0; i < n; ++i)
                for (int s = 0; s < HW; ++s) {
                    const float v = A[(size_t)s * NL + i];
                    out[(b0 + i) * HW + s] = L ? v : wt_thr_mask(v, thrs[k]);
                }
        }
    }
    return aw + tw + dw;
}

// abs_image afresh (one threshold, an arena of its own): what every threshold of the sweep equals
extern "C" void abs_sweep_core_image(const float* in, float* out, long long B, int H, int W, int L, int F,
                                     const float* taps, float thr, int NL) {
    const int aw = abs_area_a(H, W, L), tw = abs_area_t(H, W, L), dw = abs_area_d(H, W, L);
    std::vector<float> arena((size_t)(aw + tw + dw) * NL, -77.0f);
    const long long HW = (long long)H * W;
    for (long long b0 = 0; b0 < B; b0 += NL) {
        const int n = (int)(B - b0 < NL ? B - b0 : NL);
        for (int i = 0; i < n; ++i)
            for (int s = 0; s < HW; ++s) arena[(size_t)s * NL + i] = in[(b0 + i) * HW + s];
        for (int i = 0; i < n; ++i)
            abs_image(arena.data() + i, arena.data() + (size_t)aw * NL + i, arena.data() + (size_t)(aw + tw) * NL + i, NL,
                      H, W, L, F, taps, taps + F, taps + 2 * F, taps + 3 * F, thr);
        for (int i = 0; i < n; ++i)
            for (int s = 0; s < HW; ++s) out[(b0 + i) * HW + s] = arena[(size_t)s * NL + i];
    }
}

extern "C" int abs_sweep_core_words(int H, int W, int L) { return abs_tiny_words(H, W, L); }

#ifdef ABS_SWEEP_MAIN
// abssweepcore_san TAPS F: TAPS holds the four filters of one wavelet (4 * F float32: dec_lo,
// dec_hi, rec_lo, rec_hi).  Runs the sweep sequence over a shape grid with an exactly sized heap
// arena (the sanitizers see every word the routines touch) and compares every threshold's result
// with abs_image run afresh, bit for bit.  Exit status 0: no difference.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int F = atoi(argv[2]);
    if (F < 2 || F > WTP_MAX_F) return 2;
    std::vector<float> taps(4 * (size_t)F);
    FILE* fh = fopen(argv[1], "rb");
    if (!fh || fread(taps.data(), sizeof(float), taps.size(), fh) != taps.size()) return 2;
    fclose(fh);
    const float thrs[6] = {__builtin_inff(), 0.3f, __builtin_nanf(""), 0.6745f, 0.3f, 0.0f};
    const int shapes[13][2] = {{1, 1}, {3, 3}, {5, 5}, {7, 7}, {8, 8}, {2, 3}, {3, 2}, {1, 8}, {8, 1}, {6, 5}, {4, 7}, {7, 8}, {6, 6}};
    const int levels[5] = {0, 1, 2, 5, 32}, nls[2] = {1, 4};
    const long long B = 5;
    unsigned seed = 12345u;
    long long words = 0, bad = 0;
    for (const auto& hw : shapes)
        for (int L : levels)
            for (int NL : nls) {
                const int H = hw[0], W = hw[1];
                std::vector<float> x((size_t)B * H * W), outs(6 * x.size()), ref(x.size());
                for (float& v : x) { /* uniform in [-2, 2): about a third of the values below 0.6745 */
                    seed = seed * 1664525u + 1013904223u;
                    v = (float)(seed >> 8) / 4194304.0f - 2.0f;
                }
                abs_sweep_core_run(x.data(), outs.data(), B, H, W, L, F, taps.data(), thrs, 6, NL);
                for (int k = 0; k < 6; ++k) {
                    abs_sweep_core_image(x.data(), ref.data(), B, H, W, L, F, taps.data(), thrs[k], NL);
                    bad += memcmp(ref.data(), outs.data() + (size_t)k * x.size(), x.size() * sizeof(float)) != 0;
                    words += (long long)x.size();
                }
            }
    printf("abs sweep core: %lld words compared, %lld cases differ\n", words, bad);
    return bad ? 1 : 0;
}
#endif
