/* small_taps.h -- the index and order arithmetic of the one-launch small path (k_small,
 * small.hip): which window slot every tap of an output reads and in which order the taps are
 * added.  The order is the bit-parity contract (wt_dwt_core.h), so this is plain integer code,
 * shared by the device and by the host check tests/native/smalltaps.cpp, which walks every tile
 * window of small_geom.h's sweep against wt_ana_point / wt_syn_pass bit for bit.
 *
 * Taps of one output, summed in PyWavelets' order.  The interior form -- taps j = 0, 1, ...
 * ascending at consecutive descending window slots -- is recognised by its first slot (the fast
 * path: samples read back to back, taps by constant index); anything else (the periodic wrap at
 * the image edges, the split order of wt_ana_point / wt_syn_pass) walks the taps one by one:
 * tap q is j(q) = q < c1 ? c1 - 1 - q : q.
 *
 * The level clamp (pywt.dwt_max_level) keeps every line the kernel runs at least as long as the
 * filter; the host check's sweep also holds lines of one or two samples under a 20-tap filter,
 * so the walks reduce a tap's position by sm_mod16, branch-free and right for both.
 */
#ifndef WT_SMALL_TAPS_H
#define WT_SMALL_TAPS_H

#include "small_geom.h"

/* the filter lengths k_small has an instance for (besides the generic <0>): the occupancy check,
 * the launch dispatch and the host check of sm_order are all generated from this list */
#define SM_SPECIALISED(X) X(2) X(4) X(6) X(8) X(10) X(12) X(16) X(18)

/* e / n and e % n for e < 2^24 without an integer division (n uniform, inv = 1.0f / n) */
WT_SM void sm_divmod(int e, int n, float inv, int* q, int* r) {
    int d = (int)((float)e * inv);
    int m = e - d * n;
    if (m < 0) { --d; m += n; }
    if (m >= n) { ++d; m -= n; }
    *q = d;
    *r = m;
}
WT_SM int sm_wrap(int a, int N) { return a < N ? a : a - N; } /* a < 2N */
WT_SM int sm_mod1(int a, int m) { /* a in [-m, 2m) */
    a += a < 0 ? m : 0;
    return a >= m ? a - m : a;
}
/* a mod n for a in [-8n, 8n), n >= 1: bias, then subtractions that a minimum undoes (unsigned wrap) */
WT_SM int sm_mod16(int a, int n) {
    unsigned u = (unsigned)(a + 8 * n), t;
    t = u - 8u * (unsigned)n; u = t < u ? t : u;
    t = u - 4u * (unsigned)n; u = t < u ? t : u;
    t = u - 2u * (unsigned)n; u = t < u ? t : u;
    t = u - (unsigned)n; u = t < u ? t : u;
    return (int)u;
}
WT_SM int sm_modneg(int d, int n) { /* d in [-n, n): a negative d is the larger one as unsigned */
    const unsigned u = (unsigned)d, t = u + (unsigned)n;
    return (int)(t < u ? t : u);
}
WT_SM int sm_r4(int x) { return (x + 3) & ~3; } /* LDS regions start 16-byte aligned */
WT_SM int sm_clamp(int x, int hi) { /* min(max(x, 0), hi) */
    const int p = x > 0 ? x : 0;
    return p < hi ? p : hi;
}

/* analysis output m of window W (line N) reading line Np: the position i of tap 0, the count
 * c1 of taps wt_ana_point adds first in descending j (0 in the interior), the even period Ne */
struct SmAna {
    int i, c1, Ne;
};
WT_SM SmAna sm_ana_at(SmIvl W, int N, int Np, int F, int m) {
    SmAna a;
    a.i = F / 2 + 2 * sm_wrap(W.s + m, N);
    a.c1 = sm_clamp(a.i - Np + 1, F);
    a.Ne = Np + (Np & 1);
    return a;
}
/* the general form: tap q's slot in window Wp, and its tap index *j */
WT_SM int sm_ana_tap(const SmAna& a, SmIvl Wp, int Np, int q, int* j) {
    const int jj = q < a.c1 ? a.c1 - 1 - q : q;
    /* a.i - jj in (-F / 2, F / 2 + Np), Ne >= 2, F <= 20: inside [-8 Ne, 8 Ne) */
    const int r = sm_mod16(a.i - jj, a.Ne);
    const int src = r < Np ? r : Np - 1;
    *j = jj;
    return sm_modneg(src - Wp.s, Np); /* both in [0, Np) */
}
/* when the samples of the taps j sit at consecutive window slots s0 - j (always for an even
 * line: the periodic wrap keeps them contiguous; for an odd line only away from the repeated
 * end), (s0 << 5) | c1; else -1 */
WT_SM int sm_ana_fast(SmIvl W, int N, SmIvl Wp, int Np, int F, int m) {
    const SmAna a = sm_ana_at(W, N, Np, F, m);
    const int s0 = sm_mod1(a.i - Wp.s, Np);
    return (s0 >= F - 1 && s0 < Np && ((Np & 1) == 0 || (a.i < Np && a.i - F + 1 >= 0))) ? (s0 << 5) | a.c1 : -1;
}

/* synthesis output m of window O (line No) reading line N: its site (sm_site) and the count c1
 * of taps wt_syn_pass adds first in descending j */
struct SmSyn {
    int i, par, c1;
};
WT_SM SmSyn sm_syn_at(SmIvl O, int No, int N, int F, int m) {
    const SmSite s = sm_site(sm_wrap(O.s + m, No), N, F);
    SmSyn y;
    y.i = s.i;
    y.par = s.par;
    y.c1 = s.special ? sm_clamp(s.i + 1, F / 2) : (s.i < N ? 0 : sm_clamp(s.i - N + 1, F / 2));
    return y;
}
/* the general form: tap q's slot in window S, and its coefficient index *ci */
WT_SM int sm_syn_tap(const SmSyn& y, SmIvl S, int N, int q, int* ci) {
    const int j = q < y.c1 ? y.c1 - 1 - q : q;
    *ci = 2 * j + y.par;
    /* y.i - j in [-F / 4, F / 4 + N), N >= 1, F <= 20: inside [-8 N, 8 N) */
    return sm_modneg(sm_mod16(y.i - j, N) - S.s, N);
}
/* the wrap is purely periodic, so the sources of the taps j sit at slots s0 - j whenever the
 * window holds them: (s0 << 6) | (parity << 5) | c1, else -1 */
WT_SM int sm_syn_fast(SmIvl O, int No, SmIvl S, int N, int F, int m) {
    const SmSyn y = sm_syn_at(O, No, N, F, m);
    const int s0 = sm_mod1(y.i - S.s, N);
    return (s0 >= F / 2 - 1 && s0 < N) ? (s0 << 6) | (y.par << 5) | y.c1 : -1;
}

/* sum over T taps in PyWavelets' order: the c1 taps j = c1-1 .. 0 first, then j = c1 .. T-1;
 * v(j) the sample of tap j, c(j) its coefficient (compile-time j: registers, no indexing) */
template <int T, class V, class C, class A>
WT_SM void sm_order(int c1, bool plain, const V& v, const C& c, const A& acc) {
    if (plain) {
        SM_UNROLL
        for (int j = 0; j < T; ++j) acc(c(j), v(j));
    } else {
        SM_UNROLL
        for (int j = T - 1; j >= 0; --j)
            if (j < c1) acc(c(j), v(j));
        SM_UNROLL
        for (int j = 0; j < T; ++j)
            if (j >= c1) acc(c(j), v(j));
    }
}

#endif
