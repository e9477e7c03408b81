/*
 * host_chains.hip -- the chain runners: pywt.wavedec2 / waverec2 of a list of image batches level
 * by level (the tiled kernels, the per-point passes, the extension modes' kernels and their
 * one-launch tiny form), and pywt.wavedec / waverec of one flattened tensor.
 */
#include "wtp_host.h"

namespace wtp {

Chain make_chain(const TPlan& p, const float* in, float* out, float* P, void* temps, size_t stride, const float* thr,
                 unsigned long long* zc) {
    return Chain{&p, in, out, P, {wsb<float>(temps, 0), wsb<float>(temps, stride), wsb<float>(temps, 2 * stride)}, thr, zc};
}

/* The chains whose images are tiny under an extension mode (TPlan::tiny_lg): all of them in one
 * launch of k_mtiny_fwd (every analysis level, the packed image with its padding zeros) or of
 * k_mtiny_inv (threshold on load, every synthesis level, the crops, the zero count). */
static void launch_tiny_chains(const std::vector<Chain>& cs, const Taps& tp, hipStream_t s, bool inverse) {
    MTinyTable tab;
    memset(&tab, 0, sizeof tab);
    for (const Chain& c : cs) {
        const TPlan& p = *c.p;
        if (p.tiny_lg < 0) continue;
        MTinySeg& sg = tiny_append(tab, c.in, p.B, p.H, p.W, p.L, p.tiny_lg);
        sg.out = c.out;
        sg.P = c.P;
        sg.thr = c.thr;
        sg.zc = c.zc;
        tab.mode = p.mode;
    }
    if (!tab.nseg) return;
    tab.F = tp.F;
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < tp.F && j < WTM_TINY_F_MAX; ++j) tab.f[k][j] = tp.f[k][j];
    if (inverse) launch_mtiny_inv(tab, s);
    else launch_mtiny_fwd(tab, s);
}

/* pywt.wavedec2 (dwt_pruning.py:67-68) of every chain into its packed layout.  Level k of all
 * chains is ONE tiled launch (filterbank.hip) where the level is large enough, else the two
 * per-point passes of that chain.  Each approximation ping-pongs between the chain's own temps
 * so no launch reads what it writes. */
void forward_chains(const std::vector<Chain>& cs, const Taps& tp, hipStream_t s, bool fused) {
    int maxL = 0;
    for (const Chain& c : cs) maxL = std::max(maxL, c.p->L);
    std::vector<const float*> cur(cs.size());
    for (size_t j = 0; j < cs.size(); ++j) cur[j] = cs[j].in;
    std::vector<uint32_t*> fcur(cs.size()); /* fused selection: each chain's next level's slots */
    for (size_t j = 0; j < cs.size(); ++j) fcur[j] = (fused && cs[j].fsl) ? cs[j].fsl + FSL_HDR_WORDS : nullptr;
    std::vector<FwdItem> items;
    launch_tiny_chains(cs, tp, s, false);
    for (int k = 1; k <= maxL; ++k) {
        items.clear();
        for (size_t j = 0; j < cs.size(); ++j) {
            const TPlan& p = *cs[j].p;
            if (p.L < k || p.tiny_lg >= 0) continue;
            float *tL = cs[j].T[0], *tH = cs[j].T[1], *tA = cs[j].T[2];
            const int64_t R0 = p.g.R[k - 1], C0 = p.g.C[k - 1];
            if (p.mode) { /* both passes through tL / tH, the approximations in tA */
                launch_mdwt_level(cur[j], p.B, R0, C0, p.g.R[k], p.g.C[k], tp, p.mode, tL, tH, tA, cs[j].P, p.g.PR,
                                  p.g.PC, p.g.offR[k], p.g.offC[k], k == p.L, s);
                cur[j] = tA;
                continue;
            }
            if (lvl_tiled(p, p.B, R0, C0, tp)) {
                float* an = (cur[j] == tA) ? tL : tA;
                items.push_back(FwdItem{cur[j], p.B, R0, C0, an, cs[j].P, p.g.PR, p.g.PC, p.g.offR[k], p.g.offC[k],
                                        k == p.L});
                int64_t sl = 0;
                if (fcur[j] && fwd_level_fused_ok(items.back(), tp, &sl)) { /* prune_impl checked every level */
                    items.back().fslot = fcur[j];
                    items.back().fhdr = reinterpret_cast<FslHeader*>(cs[j].fsl);
                    fcur[j] += sl * FSL_WORDS;
                }
                cur[j] = an;
            } else {
                float* t0 = (cur[j] == tL) ? tA : tL;
                float* t1 = (cur[j] == tH) ? tA : tH;
                float* an = (cur[j] == tL || cur[j] == tH || cur[j] == tA) ? const_cast<float*>(cur[j]) : tA;
                launch_dwt_cols(cur[j], p.B, R0, C0, tp, t0, t1, s);
                launch_dwt_rows(t0, t1, p.B, p.g.R[k], C0, tp, an, cs[j].P, p.g.PR, p.g.PC, p.g.offR[k], p.g.offC[k],
                                k == p.L, s);
                cur[j] = an;
            }
        }
        if (!items.empty()) launch_fwd_levels(items.data(), (int)items.size(), tp, s, fused);
    }
}

/* pywt.waverec2 (dwt_pruning.py:75-77) of every chain from its packed layout, thresholding the
 * packed coefficients as they are loaded (the np.where of :31), cropping and counting zeros on
 * the last level (:79-88).  Level k of all chains is one launch, as in forward_chains(). */
void inverse_chains(const std::vector<Chain>& cs, const Taps& tp, hipStream_t s) {
    int maxL = 0;
    for (const Chain& c : cs) maxL = std::max(maxL, c.p->L);
    std::vector<const float*> cur(cs.size(), nullptr); /* nullptr: the packed cA */
    std::vector<InvItem> items;
    launch_tiny_chains(cs, tp, s, true);
    for (int k = maxL; k >= 1; --k) {
        items.clear();
        for (size_t j = 0; j < cs.size(); ++j) {
            const TPlan& p = *cs[j].p;
            if (p.L < k || p.tiny_lg >= 0) continue;
            float *tL = cs[j].T[0], *tH = cs[j].T[1], *tA = cs[j].T[2];
            const int64_t R = p.g.R[k], C = p.g.C[k];
            const bool fromP = k == p.L;
            if (p.mode) { /* every level writes R[k-1] x C[k-1]: waverec2's crop between the levels, the
                           * reference's crop after the last (wt_modes_core.h) */
                launch_midwt_level(fromP ? nullptr : tA, fromP, cs[j].P, p.g.PR, p.g.PC, p.g.offR[k], p.g.offC[k], p.B,
                                   R, C, tp, cs[j].thr, tL, tH, k == 1 ? cs[j].out : tA, p.g.R[k - 1], p.g.C[k - 1],
                                   k == 1 ? cs[j].zc : nullptr, s);
                continue;
            }
            const int64_t a_bs = fromP ? 0 : 4 * p.g.R[k + 1] * p.g.C[k + 1];
            const int64_t lda = fromP ? 0 : 2 * p.g.C[k + 1];
            const bool final = k == 1;
            const int64_t oH = final ? p.H : 2 * R, oW = final ? p.W : 2 * C;
            unsigned long long* zc = final ? cs[j].zc : nullptr;
            if (lvl_tiled(p, p.B, 2 * R, 2 * C, tp)) {
                float* y = final ? cs[j].out : ((cur[j] == tA) ? tL : tA);
                items.push_back(InvItem{cur[j], a_bs, lda, fromP, cs[j].P, p.g.PR, p.g.PC, p.g.offR[k], p.g.offC[k],
                                        p.B, R, C, cs[j].thr, y, oH, oW, zc});
                cur[j] = y;
            } else {
                float* t0 = (cur[j] == tL) ? tA : tL;
                float* t1 = (cur[j] == tH) ? tA : tH;
                launch_idwt_rows(cur[j], a_bs, lda, fromP, cs[j].P, p.g.PR, p.g.PC, p.g.offR[k], p.g.offC[k], p.B, R,
                                 C, tp, cs[j].thr, t0, t1, s);
                float* y = final ? cs[j].out : (cur[j] ? const_cast<float*>(cur[j]) : tA);
                launch_idwt_cols(t0, t1, p.B, R, C, tp, y, oH, oW, zc, s);
                cur[j] = y;
            }
        }
        if (!items.empty()) launch_inv_levels(items.data(), (int)items.size(), tp, s);
    }
}

/* pywt.wavedec / waverec (periodization) of one flattened tensor (1-D mode): packed layout
 * [cA_L | cD_L | cD_L-1 | ... | cD_1] (pywt.coeffs_to_array of a 1-D list) */
static int64_t flat_off_d(const TPlan& p, int k) {
    int64_t off = p.len[p.L];
    for (int j = p.L; j > k; --j) off += p.len[j];
    return off;
}

void forward_flat(const TPlan& p, const float* in, float* P, float* T0, float* T1, const Taps& tp, hipStream_t s) {
    const float* cur = in;
    for (int k = 1; k <= p.L; ++k) {
        float* a = (k == p.L) ? P : ((cur == T0) ? T1 : T0);
        launch_dwt1_level(cur, p.len[k - 1], tp, a, P + flat_off_d(p, k), s);
        cur = a;
    }
}

/* each level reads a (the packed cA at the top, thresholded on load; then the previous level's
 * output, of which the first len[k] samples are used -- waverec's crop) and the packed cD_k */
void inverse_flat(const TPlan& p, const float* P, float* out, float* T0, float* T1, const Taps& tp, const float* thr,
                  unsigned long long* zc, hipStream_t s) {
    const float* a = P;
    int a_thr = 1;
    for (int k = p.L; k >= 1; --k) {
        const bool final = k == 1;
        float* y = final ? out : ((a == T0) ? T1 : T0);
        launch_idwt1_level(a, a_thr, P + flat_off_d(p, k), p.len[k], tp, thr, y, final ? p.len[0] : 2 * p.len[k],
                           final ? zc : nullptr, s);
        a = y;
        a_thr = 0;
    }
}

}  // namespace wtp
