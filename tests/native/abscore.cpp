// Host build of the per-image routine of the absolute-threshold method's tiny-image kernel
// (csrc/wt_abs_core.h: abs_image, the body of k_abs_tiny) so the CPU suite can check its index
// arithmetic, arena layout and summation order against the oracle without a GPU.
// Built by tests/test_abs_core.py with: g++ -O2 -ffp-contract=off -shared -fPIC
#include <vector>

#include "../../wavelettransforms_amd/csrc/wt_abs_core.h"

// B images of H x W, one after another with word stride NL in an arena laid out like the
// kernel's (image i of a group at word offset i); returns the arena words one image needs.
extern "C" int abs_core_run(const float* in, float* out, long long B, int H, int W, int L, int F, const float* taps,
                            float thr, int NL) {
    const int aw = abs_area_a(H, W, L), tw = abs_area_t(H, W, L), dw = abs_area_d(H, W, L);
    std::vector<float> arena((size_t)(aw + tw + dw) * NL, -77.0f);
    for (long long b0 = 0; b0 < B; b0 += NL) {
        const int n = (int)(B - b0 < NL ? B - b0 : NL);
        for (int i = 0; i < n; ++i)
            for (int s = 0; s < H * W; ++s) arena[(size_t)s * NL + i] = in[(b0 + i) * H * W + s];
        for (int i = 0; i < n; ++i)
            abs_image(arena.data() + i, arena.data() + (size_t)aw * NL + i, arena.data() + (size_t)(aw + tw) * NL + i, NL,
                      H, W, L, F, taps, taps + F, taps + 2 * F, taps + 3 * F, thr);
        for (int i = 0; i < n; ++i)
            for (int s = 0; s < H * W; ++s) out[(b0 + i) * H * W + s] = arena[(size_t)s * NL + i];
    }
    return aw + tw + dw;
}

extern "C" int abs_core_mod(int t, int m) { return abs_mod(t, m, abs_inv(m)); }

// the planner's lane choice for k_abs_tiny (log2 of the images a wave takes; -1: not a tiny image)
extern "C" int abs_core_lanes_log2(long long H, long long W, int L) { return abs_lanes_log2(H, W, L); }
extern "C" int abs_core_wave_words() { return ABS_WAVE_WORDS; }
