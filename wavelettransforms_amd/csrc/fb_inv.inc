/*
 * fb_inv.inc -- one synthesis level as one launch: the kernel arguments (InvArgs, InvGroup), the
 * general kernel k_inv_level and the interior kernel k_inv_int with its EDGE form; both threshold
 * the coefficients as they load them and count the zeros they write.  After fb_device.inc.
 */
#pragma clang fp contract(off)

namespace wtp {

constexpr int INV_RG = 2; /* synthesis row-pass rows interleaved per wave */

/* ------------------------------------------------------------ synthesis --- */
struct InvArgs {
    const float* a;      /* approximation (B, R, C) with row pitch lda, batch stride a_bs */
    int64_t a_bs;
    int lda, a_from_P;   /* a_from_P: the approximation is the packed cA (thresholded) */
    const float* P;
    int64_t P_bs;
    int PC, offR, offC;
    int R, C;            /* coefficient dims of this level */
    float* y;            /* output (B, outH, outW), row pitch outW */
    int outH, outW;
    const float* thr;    /* per-tensor float32 threshold applied to packed coefficients */
    unsigned long long* zc;
    int tilesC, tilesR;
    int tr0, nTR, tc0, nTC, frame; /* as FwdArgs: k_inv_int's rectangle, k_inv_level's frame */
};

/* the inverse's items of one geometry: per item its approximation source, packed array and output,
 * and its threshold / zero-count words as element offsets from the geometry's thr / zc (every
 * tensor of a call has them in one array) */
__host__ __device__ inline int thr_off_of(int32_t v) { return (int)(int16_t)(v & 0xFFFF); }
__host__ __device__ inline int zc_off_of(int32_t v) { return (int)(v >> 16); }
struct InvGroup {
    InvArgs geo;
    int n, tiles;
    FastDiv dv_tiles, dv_per, dv_ntc; /* as FwdGroup */
    FastDiv dv_tc, dv_side;
    const float* a[FB_UNI];
    const float* P[FB_UNI];
    float* y[FB_UNI];
    /* threshold (low 16 bits) and zero-count (high 16 bits) word offsets, signed, packed in one
     * 32-bit element: a scalar load (a 16-bit kernarg element is a vector load and a wait) */
    int32_t tz_off[FB_UNI];
};

template <int FT>
__global__ __launch_bounds__(FB_THREADS) WTP_FB_INV_WPE void k_inv_level(InvGroup g, TapsT<FT> tp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int gt = xcd_tile(blockIdx.x, gridDim.x);
    const int F = FT ? FT : tp.F;
    const int H = F / 2;
    const int item = gt / g.tiles;
    InvArgs a = g.geo;
    a.a = g.a[item];
    a.P = g.P[item];
    a.y = g.y[item];
    a.thr = a.thr ? a.thr + thr_off_of(g.tz_off[item]) : nullptr;
    a.zc = a.zc ? a.zc + zc_off_of(g.tz_off[item]) : nullptr;
    const int tile = gt - item * g.tiles;
    int tc, tr, b;
    if (a.frame) {
        const int per = a.tilesR * a.tilesC - a.nTR * a.nTC;
        b = tile / per;
        frame_tile(tile - b * per, a.tilesC, a.tr0, a.nTR, a.tc0, a.nTC, &tr, &tc);
    } else {
        tc = tile % a.tilesC;
        tr = (tile / a.tilesC) % a.tilesR;
        b = tile / (a.tilesC * a.tilesR);
    }
    const int n0 = tr * IR, m0 = tc * IC;
    const int nl = min(n0 + IR, a.outH) - 1, ml = min(m0 + IC, a.outW) - 1;
    const int r_lo = site_u(n0, a.R, F).iu - H + 1, r_hi = site_u(nl, a.R, F).iu;
    const int c_lo = site_u(m0, a.C, F).iu - H + 1, c_hi = site_u(ml, a.C, F).iu;
    const int NRr = r_hi - r_lo + 1, NCc = c_hi - c_lo + 1;
    float2* Aq = reinterpret_cast<float2*>(lds);  /* (cA, cH=da) at each tile position  */
    float2* Dq = Aq + NRr * NCc;                  /* (cV=ad, cD=dd)                     */
    /* NRr x IC: (lo, hi) row-pass output; specialised filters keep their rows in registers
     * across a barrier and write them over Aq/Dq (half the LDS per workgroup) */
    float2* LoHi = FT > 0 ? Aq : Dq + NRr * NCc;
    const float thr = a.thr ? *a.thr : 0.0f;      /* |c| < 0 never holds: no threshold  */
    auto tl = [&](float c) { return wt_thr_mask(c, thr); };
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const float* Pb = a.P + (int64_t)b * a.P_bs;
    const float* ab = a.a + (int64_t)b * a.a_bs;
    WTP_FPROBE(0);
    /* 1. the four coefficient tiles (periodic wrap, thresholded on load); all loads of a
     *    thread issued before the LDS writes (compile-time trip count) */
    {
        /* a tile's coefficient rows / columns: NRr <= IR/2 + H, NCc <= IC/2 + H (its IR outputs sit on
         * IR/2 consecutive synthesis sites; the H-even special last output n = 2N - 1 included) */
        constexpr int NR_MAX = IR / 2 + (FT ? FT : 2) / 2, NC_MAX = IC / 2 + (FT ? FT : 2) / 2;
        const bool inner = r_lo >= 0 && r_hi < a.R && c_lo >= 0 && c_hi < a.C;
        auto load4 = [&](int rr, int cc, float4& q) {
            const int r = inner ? r_lo + rr : pmod32(r_lo + rr, a.R), c = inner ? c_lo + cc : pmod32(c_lo + cc, a.C);
            const float* prow = Pb + (int64_t)r * a.PC;
            const float* drow = Pb + (int64_t)(a.offR + r) * a.PC;
            const float va = a.a_from_P ? prow[c] : ab[(int64_t)r * a.lda + c];
            q = make_float4(va, prow[a.offC + c], drow[c], drow[a.offC + c]); /* cA, cV=ad, cH=da, cD=dd */
        };
        auto store4 = [&](int rr, int cc, float4 q) {
            const float va = a.a_from_P ? tl(q.x) : q.x;
            Aq[rr * NCc + cc] = make_float2(va, tl(q.z));
            Dq[rr * NCc + cc] = make_float2(tl(q.y), tl(q.w));
        };
        if (FT) {
            constexpr int K = (NR_MAX * NC_MAX + FB_THREADS - 1) / FB_THREADS;
            float4 q[K];
#pragma unroll
            for (int k = 0; k < K; ++k) { /* unconditional (clamped) loads: no per-load wait */
                const int e = k * FB_THREADS + threadIdx.x;
                const int rr = e / NC_MAX, cc = e - rr * NC_MAX;
                load4(min(rr, NRr - 1), min(cc, NCc - 1), q[k]);
            }
            /* stored at the clamped position it was loaded from (duplicates rewrite their own
             * value): no predicate, so no load is sunk into a branch behind its own wait */
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int e = k * FB_THREADS + threadIdx.x;
                const int rr = e / NC_MAX, cc = e - rr * NC_MAX;
                store4(min(rr, NRr - 1), min(cc, NCc - 1), q[k]);
            }
        } else {
            for (int e = threadIdx.x; e < NRr * NCc; e += FB_THREADS) {
                const int rr = e / NCc, cc = e - rr * NCc;
                float4 q;
                load4(rr, cc, q);
                store4(rr, cc, q);
            }
        }
    }
    __syncthreads();
    WTP_FPROBE(1);
    /* 2. axis -1 synthesis of every tile row: lo = rec(cA, cV), hi = rec(cH, cD), carried
     *    packed as (lo, hi): rec_lo over (cA, cH), then rec_hi over (cV, cD).  Each lane's
     *    taps (its output parity) are resolved into registers once. */
    const float* rlo = tp.f[2];
    const float* rhi = tp.f[3];
    constexpr int HM = FT ? FT / 2 : 1;
    const int m = m0 + lane;
    /* rows per wave: a tile's coefficient rows NRr = r_hi - r_lo + 1 <= IR/2 + H (the sites of
     * IR consecutive outputs span IR/2 positions; H even: exactly IR/2 + H) */
    constexpr int RRN = (IR / 2 + HM + 3) / 4;
    f2 rowres[FT ? RRN : 1];
    if (lane < IC && m <= ml) {
        const SiteU s = site_u(m, a.C, F);
        auto getA = [&](int rr) {
            return [&, rr](int g) { const float2 v = Aq[rr * NCc + (g - c_lo)]; return f2{v.x, v.y}; };
        };
        auto getD = [&](int rr) {
            return [&, rr](int g) { const float2 v = Dq[rr * NCc + (g - c_lo)]; return f2{v.x, v.y}; };
        };
        if (FT) {
            float tlo[HM], thi[HM];
#pragma unroll
            for (int j = 0; j < HM; ++j) {
                const float l0 = rlo[2 * j], l1 = rlo[2 * j + 1], h0 = rhi[2 * j], h1 = rhi[2 * j + 1];
                tlo[j] = s.par ? l1 : l0;
                thi[j] = s.par ? h1 : h0;
            }
            auto tl_ = [&](int j) { return tlo[j]; };
            auto th_ = [&](int j) { return thi[j]; };
            if (__all(!s.special && s.i < a.C)) {
                /* interior columns: no branch between the rows (rows past NRr are clamped, computed
                 * and dropped at the write), so their independent sums interleave */
                /* INV_RG rows at a time, tap-major: their chains are independent, so they
                 * interleave instead of running one 2H-long dependent chain after another */
                constexpr int G = INV_RG;
#pragma unroll
                for (int q0 = 0; q0 < RRN; q0 += G) {
                    f2 acc[G], v[G][HM];
                    int rb[G];
#pragma unroll
                    for (int gq = 0; gq < G; ++gq) {
                        acc[gq] = f2{0.0f, 0.0f};
                        rb[gq] = min(wv + 4 * min(q0 + gq, RRN - 1), NRr - 1) * NCc + s.iu - c_lo;
                    }
                    /* each row's HM samples from ONE base address (the lowest), so the reads take
                     * immediate offsets (ds_read2_b64 offset0 / offset1) instead of an address each */
                    const float2* pa[G];
#pragma unroll
                    for (int gq = 0; gq < G; ++gq) pa[gq] = Aq + (rb[gq] - (HM - 1));
#pragma unroll
                    for (int gq = 0; gq < G; ++gq)
#pragma unroll
                        for (int j = 0; j < HM; ++j) {
                            const float2 t = pa[gq][HM - 1 - j];
                            v[gq][j] = f2{t.x, t.y};
                        }
#pragma unroll
                    for (int j = 0; j < HM; ++j)
#pragma unroll
                        for (int gq = 0; gq < G; ++gq)
                            if (q0 + gq < RRN) acc[gq] = acc[gq] + tlo[j] * v[gq][j];
#pragma unroll
                    for (int gq = 0; gq < G; ++gq)
#pragma unroll
                        for (int j = 0; j < HM; ++j) {
                            const float2 t = (pa[gq] + (Dq - Aq))[HM - 1 - j];
                            v[gq][j] = f2{t.x, t.y};
                        }
#pragma unroll
                    for (int j = 0; j < HM; ++j)
#pragma unroll
                        for (int gq = 0; gq < G; ++gq)
                            if (q0 + gq < RRN) acc[gq] = acc[gq] + thi[j] * v[gq][j];
#pragma unroll
                    for (int gq = 0; gq < G; ++gq)
                        if (q0 + gq < RRN) rowres[q0 + gq] = acc[gq];
                }
            } else {
#pragma unroll
                for (int q = 0; q < RRN; ++q) {
                    const int rr = wv + 4 * q;
                    if (rr < NRr) {
                        f2 acc = {0.0f, 0.0f};
                        acc = syn_pass_u<FT>(s, a.C, F, tl_, getA(rr), acc);
                        acc = syn_pass_u<FT>(s, a.C, F, th_, getD(rr), acc);
                        rowres[q] = acc;
                    }
                }
            }
        } else {
            auto tl_ = [&](int j) { return rlo[2 * j + s.par]; };
            auto th_ = [&](int j) { return rhi[2 * j + s.par]; };
            for (int rr = wv; rr < NRr; rr += FB_THREADS / 64) {
                f2 acc = {0.0f, 0.0f};
                acc = syn_pass_u<FT>(s, a.C, F, tl_, getA(rr), acc);
                acc = syn_pass_u<FT>(s, a.C, F, th_, getD(rr), acc);
                LoHi[rr * IC + lane] = make_float2(acc.x, acc.y);
            }
        }
    }
    if constexpr (FT > 0) {
        __syncthreads(); /* every read of Aq/Dq is done: LoHi overwrites them */
        if (lane < IC && m <= ml) {
#pragma unroll
            for (int q = 0; q < RRN; ++q)
                if (wv + 4 * q < NRr) LoHi[(wv + 4 * q) * IC + lane] = make_float2(rowres[q].x, rowres[q].y);
        }
    }
    __syncthreads();
    WTP_FPROBE(2);
    /* 3. axis -2 synthesis: y = rec_lo over lo, then rec_hi over hi, down each column (the
     *    site of a row is wave-uniform: scalar taps) */
    unsigned long long z = 0;
    if (lane < IC && m <= ml) {
        float* yb = a.y + (int64_t)b * a.outH * a.outW;
        /* specialised filters: each wave owns RB consecutive rows.  Interior blocks run from
         * registers: outputs k and k + RB/2 share taps (same parity) and sit four sites apart,
         * so they are computed packed, and each LoHi row is read from LDS once for the block
         * (H + RB/2 - 1 + E rows instead of H per output) */
        constexpr int RB = IR / (FB_THREADS / 64);
        const int nf = FT ? n0 + RB * wv : n0 + wv;
        const int nend = FT ? min(nf + RB - 1, nl) : nl;
        const int nstep = FT ? 1 : FB_THREADS / 64;
        bool fast = false;
        if constexpr (FT > 0) {
            constexpr int H = FT / 2, E = (H & 1) ? 0 : 1, NV = H + RB / 2 - 1 + E, RB2 = RB / 2;
            static_assert(RB % 4 == 0, "packed column blocks pair rows k and k + RB/2, RB/4 sites apart");
            const SiteU s0 = site_u(nf, a.R, F);
            const int nlast = nf + RB - 1;
            fast = nlast <= nl && !s0.special && (E == 0 || nlast < 2 * a.R - 1) &&
                              s0.i + ((RB - 1 + E) >> 1) < a.R;
            if (fast) {
                const int g0 = s0.i - H + 1 - r_lo;
                float2 r[NV];
#pragma unroll
                for (int q = 0; q < NV; ++q) r[q] = LoHi[(g0 + q) * IC + lane];
                /* tap-major over the RB2 output pairs: RB2 independent chains interleave, and
                 * each tap is read once per j (two parities) instead of once per output */
                f2 acc[RB2];
#pragma unroll
                for (int k = 0; k < RB2; ++k) acc[k] = f2{0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < H; ++j) {
                    const float t0 = rlo[2 * j], t1 = rlo[2 * j + 1];
#pragma unroll
                    for (int k = 0; k < RB2; ++k) {
                        const int par = (k + E) & 1, base = ((k + E) >> 1) + H - 1;
                        const float t = par ? t1 : t0;
                        acc[k] = acc[k] + f2{t, t} * f2{r[base - j].x, r[base - j + RB2 / 2].x};
                    }
                }
#pragma unroll
                for (int j = 0; j < H; ++j) {
                    const float t0 = rhi[2 * j], t1 = rhi[2 * j + 1];
#pragma unroll
                    for (int k = 0; k < RB2; ++k) {
                        const int par = (k + E) & 1, base = ((k + E) >> 1) + H - 1;
                        const float t = par ? t1 : t0;
                        acc[k] = acc[k] + f2{t, t} * f2{r[base - j].y, r[base - j + RB2 / 2].y};
                    }
                }
#pragma unroll
                for (int k = 0; k < RB2; ++k) {
                    yb[(int64_t)(nf + k) * a.outW + m] = acc[k].x;
                    yb[(int64_t)(nf + k + RB2) * a.outW + m] = acc[k].y;
                    z += (acc[k].x == 0.0f) + (acc[k].y == 0.0f);
                }
            }
        }
        for (int n = nf; !fast && n <= nend; n += nstep) {
            const SiteU s = site_u(n, a.R, F);
            auto tl_ = [&](int j) { return rlo[2 * j + s.par]; };
            auto th_ = [&](int j) { return rhi[2 * j + s.par]; };
            auto gl = [&](int g) { return LoHi[(g - r_lo) * IC + lane].x; };
            auto gh = [&](int g) { return LoHi[(g - r_lo) * IC + lane].y; };
            float acc = 0.0f;
            if (!s.special && s.i < a.R) {
                acc = syn_pass_inner<FT>(s, F, tl_, gl, acc);
                acc = syn_pass_inner<FT>(s, F, th_, gh, acc);
            } else {
                acc = syn_pass_u<FT>(s, a.R, F, tl_, gl, acc);
                acc = syn_pass_u<FT>(s, a.R, F, th_, gh, acc);
            }
            yb[(int64_t)n * a.outW + m] = acc;
            z += acc == 0.0f;
        }
    }
    if (a.zc) {
        __shared__ unsigned long long zs;
        if (threadIdx.x == 0) zs = 0;
        __syncthreads();
        if (z) atomicAdd(&zs, z);
        __syncthreads();
        if (threadIdx.x == 0 && zs) atomicAdd(a.zc, zs);
    }
    WTP_FPROBE(3);
}

/* One synthesis level over the INTERIOR tiles of a group (InvGroup geo: tr0/nTR/tc0/nTC): every
 * output of the tile is a full-tile non-special site whose coefficient window lies inside the
 * level (no wrap), so the tile's coefficient rows / columns are exactly IR/2 + H - (H & 1) and
 * only wt_syn_pass's ascending interior order occurs.  EDGE: the same kernel over the FRAME of tiles
 * around that rectangle (InvArgs.frame's decode; the host runs it when the level is at least a
 * window tall and wide, so one wrap brings every coefficient position into range): the window
 * loaded with the periodic wrap, wt_syn_pass's special / wrapped-first orders only where a site
 * needs them (the samples and taps are the interior ones -- unwrapped positions stay monotonic),
 * stores and zero counts masked to the output extent.
 * Same sums in the same order as k_inv_level's interior forms (from 0, as pywt).  Instruction shape: coefficient loads are buffer loads
 * whose four subband offsets are scalars (one lane offset per element), the row pass's per-lane
 * taps are register pairs broadcast by op_sel, the output stores take the row as a scalar
 * offset, and zeros are counted by ballot. */
template <int FT, bool EDGE>
__global__ __launch_bounds__(FB_THREADS) WTP_FB_INT_WPE void k_inv_int(InvGroup g, SmallTaps tp) {
    static_assert(FT > 0 && FT % 2 == 0, "specialised even filters");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int H = FT / 2, HM = H;
    constexpr int NR = inv_win(FT), NC = inv_win(FT); /* coefficient rows / columns */
    const int gt = xcd_tile(blockIdx.x, gridDim.x);
    const int item = fdiv(gt, g.dv_tiles);
    const InvArgs& a = g.geo;
    const int tile = gt - item * g.tiles;
    int b, trow, tcol;
    if constexpr (EDGE) {
        const int per = a.tilesR * a.tilesC - a.nTR * a.nTC;
        b = fdiv(tile, g.dv_per);
        frame_tile_fd(tile - b * per, a.tilesC, a.tr0, a.nTR, a.tc0, a.nTC, g.dv_tc, g.dv_side, &trow, &tcol);
    } else {
        const int per = a.nTR * a.nTC;
        b = fdiv(tile, g.dv_per);
        const int t2 = tile - b * per, trr = fdiv(t2, g.dv_ntc);
        trow = a.tr0 + trr;
        tcol = a.tc0 + t2 - trr * a.nTC;
    }
    const int n0 = trow * IR, m0 = tcol * IC;
    const int nl = min(n0 + IR, a.outH) - 1, ml = min(m0 + IC, a.outW) - 1; /* EDGE: the last stored output */
    const int r_lo = site_u(n0, a.R, FT).iu - H + 1, c_lo = site_u(m0, a.C, FT).iu - H + 1;
    float2* Aq = reinterpret_cast<float2*>(lds); /* (cA, cH=da) */
    float2* Dq = Aq + NR * NC;                   /* (cV=ad, cD=dd) */
    float2* LoHi = Aq;                           /* NR x IC, written over Aq/Dq after the row pass */
    const float* thrp = a.thr ? a.thr + thr_off_of(g.tz_off[item]) : nullptr;
    const float thr = thrp ? *thrp : 0.0f; /* |c| < 0 never holds: no threshold */
    auto tl = [&](float c) { return wt_thr_mask(c, thr); };
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    WTP_FPROBE(0);
    /* 1. the four coefficient tiles, thresholded on load: element e of the NR x NC window at
     *    lane offset (r_lo + rr) * PC + c_lo + cc; the subbands differ by scalar offsets */
    {
        const __amdgpu_buffer_rsrc_t rP =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.P[item]) + (int64_t)b * a.P_bs, 0, (int)(4 * a.P_bs), 0x00020000);
        const __amdgpu_buffer_rsrc_t rA = a.a_from_P ? rP
            : __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.a[item]) + (int64_t)b * a.a_bs, 0, (int)(4 * a.a_bs), 0x00020000);
        const int sV = 4 * a.offC, sH = 4 * a.offR * a.PC, sD = sH + sV;
        constexpr int NE = NR * NC, K = (NE + FB_THREADS - 1) / FB_THREADS;
        float4 q[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int e = min(k * FB_THREADS + (int)threadIdx.x, NE - 1);
            const int rr = e / NC, cc = e - rr * NC;
            int r = r_lo + rr, c = c_lo + cc;
            if constexpr (EDGE) { /* one wrap suffices: the level is at least NR x NC */
                r = r < 0 ? r + a.R : (r >= a.R ? r - a.R : r);
                c = c < 0 ? c + a.C : (c >= a.C ? c - a.C : c);
            }
            const int vo = 4 * (r * a.PC + c);
            const int va = a.a_from_P ? vo : 4 * (r * a.lda + c);
            q[k].x = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rA, va, 0, 0));
            q[k].y = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rP, vo, sV, 0));
            q[k].z = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rP, vo, sH, 0));
            q[k].w = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rP, vo, sD, 0));
        }
#pragma unroll
        for (int k = 0; k < K; ++k) { /* clamped duplicates rewrite their own value */
            const int e = min(k * FB_THREADS + (int)threadIdx.x, NE - 1);
            const float va = a.a_from_P ? tl(q[k].x) : q[k].x;
            Aq[e] = make_float2(va, tl(q[k].z));
            Dq[e] = make_float2(tl(q[k].y), tl(q[k].w));
        }
    }
    __syncthreads();
    WTP_FPROBE(1);
    /* 2. axis -1 synthesis of the NR coefficient rows.  Lane = (row ro = lane / 32 of a row pair,
     *    column slot c = lane % 32); sub-pass p computes output column m0 + 2c + p, so the output's
     *    parity -- its taps -- and its site offset are uniform: the taps stay scalar.  A wave takes
     *    the row pairs wv, wv + 4, ...; results wait in registers until every read of Aq/Dq is done
     *    (LoHi is written over them). */
    const int m = m0 + lane;
    constexpr int KP = (NR + 7) / 8; /* row pairs per wave */
    f2 rowres[KP][2];
    /* EDGE: the exact-order results of this lane's fix-up entry (row fxrow, column pair fxc) */
    f2 fx[2] = {f2{0.0f, 0.0f}, f2{0.0f, 0.0f}};
    int fxrow = -1, fxc = 0;
    {
        const int ro = lane >> 5, c = lane & 31;
        /* both sub-passes from one sample window: p's samples start at column c + pe(p), and the
         * two sums are independent chains that interleave */
        constexpr int PE1 = (H & 1) ? 0 : 1, NS = HM + PE1;
        constexpr int PAR0 = (H & 1) ? 0 : 1, PAR1 = 1 - PAR0;
        /* the two outputs of column pair cp at (unwrapped) sample row pa / pd in wt_syn_pass's
         * order: the terms with i - j >= T by descending j first (T = 0 at a special site, N past
         * the end), then the others ascending */
        auto exact_pair = [&](const float2* pa, const float2* pd, int cp, f2& a0, f2& a1) {
            const SiteU s0 = site_u(m0 + 2 * cp, a.C, FT), s1 = site_u(m0 + 2 * cp + 1, a.C, FT);
            const int i0 = s0.i, T0 = s0.special ? 0 : a.C, i1 = s1.i, T1 = s1.special ? 0 : a.C;
            f2 v[NS];
            auto sp = [&](int p, int j) { return v[(p ? PE1 : 0) + HM - 1 - j]; };
            a0 = f2{0.0f, 0.0f};
            a1 = f2{0.0f, 0.0f};
            auto pass = [&](const float* rec) {
#pragma unroll
                for (int j = HM - 1; j >= 0; --j) {
                    if (i0 - j >= T0) a0 = a0 + rec[2 * j + PAR0] * sp(0, j);
                    if (i1 - j >= T1) a1 = a1 + rec[2 * j + PAR1] * sp(1, j);
                }
#pragma unroll
                for (int j = 0; j < HM; ++j) {
                    if (i0 - j < T0) a0 = a0 + rec[2 * j + PAR0] * sp(0, j);
                    if (i1 - j < T1) a1 = a1 + rec[2 * j + PAR1] * sp(1, j);
                }
            };
#pragma unroll
            for (int q = 0; q < NS; ++q) { const float2 t = pa[q]; v[q] = f2{t.x, t.y}; }
            pass(tp.f[2]);
#pragma unroll
            for (int q = 0; q < NS; ++q) { const float2 t = pd[q]; v[q] = f2{t.x, t.y}; }
            pass(tp.f[3]);
        };
        /* EDGE: the column pairs whose sites are special or past the end get the exact order in
         * a compact fix-up after the uniform pass: lane e of this wave = (its row e / nsc, the
         * (e % nsc)-th such pair).  Such pairs within the stored extent are the first one (H
         * even: output 0) or the last F/4 + 1 of the level, never both in one tile (the host runs
         * the frame only when the level is >= NC coefficients wide, so 2N > IC): at most F/4 + 1
         * pairs, and the wave's 2 KP rows times that fit its 64 lanes. */
        static_assert(2 * KP * (FT / 4 + 1) <= 64, "one fix-up pass per wave");
        uint32_t fxmask = 0;
        int nsc = 0;
        if constexpr (EDGE) {
            const SiteU s0 = site_u(m0 + 2 * c, a.C, FT), s1 = site_u(m0 + 2 * c + 1, a.C, FT);
            /* pairs past the stored extent (a partial last tile) are never read: left out */
            const bool need = (s0.special || s0.i >= a.C || s1.special || s1.i >= a.C) && m0 + 2 * c <= ml;
            fxmask = (uint32_t)__ballot(need && ro == 0); /* lanes 0..31: bit c */
            nsc = __builtin_popcount(fxmask);
        }
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const int row = min(2 * (wv + 4 * k) + ro, NR - 1);
            const float2* pa = Aq + row * NC + c;
            const float2* pd = Dq + row * NC + c;
            f2 a0, a1;
            {
                f2 v[NS];
                /* sample of sub-pass p at tap j: column c + pe(p) + HM - 1 - j */
                auto sp = [&](int p, int j) { return v[(p ? PE1 : 0) + HM - 1 - j]; };
#pragma unroll
                for (int q = 0; q < NS; ++q) { const float2 t = pa[q]; v[q] = f2{t.x, t.y}; }
                const f2 z2 = {0.0f, 0.0f};
                a0 = z2 + tp.f[2][PAR0] * sp(0, 0);
                a1 = z2 + tp.f[2][PAR1] * sp(1, 0);
#pragma unroll
                for (int j = 1; j < HM; ++j) {
                    a0 = a0 + tp.f[2][2 * j + PAR0] * sp(0, j);
                    a1 = a1 + tp.f[2][2 * j + PAR1] * sp(1, j);
                }
#pragma unroll
                for (int q = 0; q < NS; ++q) { const float2 t = pd[q]; v[q] = f2{t.x, t.y}; }
#pragma unroll
                for (int j = 0; j < HM; ++j) {
                    a0 = a0 + tp.f[3][2 * j + PAR0] * sp(0, j);
                    a1 = a1 + tp.f[3][2 * j + PAR1] * sp(1, j);
                }
            }
            /* computed HERE: without this the compiler sinks the sums past the barrier below
             * (their only use is the LoHi write) and keeps every sample alive across it */
            asm volatile("" : "+v"(a0), "+v"(a1));
            rowres[k][0] = a0;
            rowres[k][1] = a1;
        }
        if (EDGE && fxmask) { /* uniform */
            if (lane < 2 * KP * nsc) {
                const int rs = lane / nsc, ci = lane - rs * nsc;
                uint32_t mm = fxmask;
                for (int t = 0; t < ci; ++t) mm &= mm - 1u;
                const int cp = __builtin_ctz(mm);
                const int row = 2 * (wv + 4 * (rs >> 1)) + (rs & 1);
                if (row < NR) {
                    f2 a0, a1;
                    exact_pair(Aq + row * NC + cp, Dq + row * NC + cp, cp, a0, a1);
                    asm volatile("" : "+v"(a0), "+v"(a1));
                    fx[0] = a0;
                    fx[1] = a1;
                    fxrow = row;
                    fxc = cp;
                }
            }
        }
    }
    __syncthreads(); /* every read of Aq/Dq is done: LoHi overwrites them */
    {
        const int ro = lane >> 5, c = lane & 31;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const int row = 2 * (wv + 4 * k) + ro;
            if (row < NR) {
#pragma unroll
                for (int p = 0; p < 2; ++p) LoHi[row * IC + 2 * c + p] = make_float2(rowres[k][p].x, rowres[k][p].y);
            }
        }
        /* the fix-up's exact values over the uniform pass's (this wave's own rows; a wave's LDS
         * writes land in program order) */
        if (EDGE && fxrow >= 0) {
#pragma unroll
            for (int p = 0; p < 2; ++p) LoHi[fxrow * IC + 2 * fxc + p] = make_float2(fx[p].x, fx[p].y);
        }
    }
    __syncthreads();
    WTP_FPROBE(2);
    /* 3. axis -2: each wave owns RB consecutive output rows; outputs k and k + RB/2 share taps and
     *    sit four sites apart, computed packed from the block's LoHi rows held in registers */
    constexpr int RB = IR / (FB_THREADS / 64);
    constexpr int E = (H & 1) ? 0 : 1, NV = H + RB / 2 - 1 + E, RB2 = RB / 2;
    static_assert(RB % 4 == 0, "packed column blocks pair rows k and k + RB/2, RB/4 sites apart");
    const int nf = n0 + RB * wv;
    const int g0 = site_u(nf, a.R, FT).i - H + 1 - r_lo;
    float2 r[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) r[q] = LoHi[(g0 + q) * IC + lane];
    const __amdgpu_buffer_rsrc_t rY =
        __builtin_amdgcn_make_buffer_rsrc(g.y[item] + (int64_t)b * a.outH * a.outW, 0, 4 * a.outH * a.outW, 0x00020000);
    const int vy = 4 * m;
    uint32_t z = 0; /* wave-uniform: zeros of this wave's outputs */
    /* EDGE: rows whose site is special or wrapped (the image's first / last few) are computed
     * again one by one in wt_syn_pass's order after the packed pass, which skips storing them;
     * rows past the extent are not stored.  The row's site is wave-uniform, so are the masks. */
    uint32_t xmask = 0, smask = (1u << RB) - 1u;
    if constexpr (EDGE) {
        for (int k = 0; k < RB; ++k) {
            const SiteU s = site_u(nf + k, a.R, FT);
            if (s.special || s.i >= a.R) xmask |= 1u << k;
            if (nf + k > nl) smask &= ~(1u << k);
        }
    }
    const bool min_ = !EDGE || m <= ml; /* EDGE: a partial last tile column */
    {
        const uint32_t wmask = smask & ~xmask; /* the rows the packed pass stores */
        f2 acc[RB2];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const float t0 = tp.f[2][2 * j], t1 = tp.f[2][2 * j + 1];
#pragma unroll
            for (int k = 0; k < RB2; ++k) {
                const int par = (k + E) & 1, base = ((k + E) >> 1) + H - 1;
                const float t = par ? t1 : t0;
                const f2 p = f2{t, t} * f2{r[base - j].x, r[base - j + RB2 / 2].x};
                acc[k] = (j == 0 ? f2{0.0f, 0.0f} : acc[k]) + p;
            }
        }
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const float t0 = tp.f[3][2 * j], t1 = tp.f[3][2 * j + 1];
#pragma unroll
            for (int k = 0; k < RB2; ++k) {
                const int par = (k + E) & 1, base = ((k + E) >> 1) + H - 1;
                const float t = par ? t1 : t0;
                acc[k] = acc[k] + f2{t, t} * f2{r[base - j].y, r[base - j + RB2 / 2].y};
            }
        }
        if constexpr (!EDGE) {
#pragma unroll
            for (int k = 0; k < RB2; ++k) {
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[k].x), rY, vy, 4 * (nf + k) * a.outW, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[k].y), rY, vy, 4 * (nf + k + RB2) * a.outW, 0);
                z += (uint32_t)__popcll(__ballot(acc[k].x == 0.0f)) + (uint32_t)__popcll(__ballot(acc[k].y == 0.0f));
            }
        } else {
#pragma unroll
            for (int k = 0; k < RB2; ++k) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int kk = k + u * RB2;
                    const float y = u ? acc[k].y : acc[k].x;
                    if ((wmask >> kk) & 1u) {
                        if (min_) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y), rY, vy, 4 * (nf + kk) * a.outW, 0);
                        z += (uint32_t)__popcll(__ballot(min_ && y == 0.0f));
                    }
                }
            }
        }
    }
    if (EDGE && (xmask & smask)) { /* uniform */
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            if (!(((xmask & smask) >> k) & 1u)) continue;
            const int n = nf + k;
            const SiteU s = site_u(n, a.R, FT);
            const int Tn = s.special ? 0 : a.R;
            const int par = (k + E) & 1, base = ((k + E) >> 1) + H - 1;
            float y = 0.0f;
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const float* rec = tp.f[2 + pass];
#pragma unroll
                for (int j = H - 1; j >= 0; --j)
                    if (s.i - j >= Tn) y = y + rec[2 * j + par] * (pass ? r[base - j].y : r[base - j].x);
#pragma unroll
                for (int j = 0; j < H; ++j)
                    if (s.i - j < Tn) y = y + rec[2 * j + par] * (pass ? r[base - j].y : r[base - j].x);
            }
            if (min_) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y), rY, vy, 4 * n * a.outW, 0);
            z += (uint32_t)__popcll(__ballot(min_ && y == 0.0f));
        }
    }
    if (a.zc) {
        /* 8 bytes: the dynamic LDS follows the static variables, and a 4-byte one would leave
         * every float2 of the tiles 4-byte misaligned (measured: k_inv_int 4x slower, LDS
         * instruction issue stalls) */
        __shared__ unsigned long long zs;
        if (threadIdx.x == 0) zs = 0;
        __syncthreads();
        if (lane == 0 && z) atomicAdd(&zs, (unsigned long long)z);
        __syncthreads();
        if (threadIdx.x == 0 && zs) atomicAdd(a.zc + zc_off_of(g.tz_off[item]), zs);
    }
    WTP_FPROBE(3);
}

}  // namespace wtp
