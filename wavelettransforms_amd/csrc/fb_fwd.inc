/*
 * fb_fwd.inc -- one analysis level as one launch: the kernel arguments (FwdArgs, FwdGroup), the
 * general kernel k_fwd_level (any filter, every tile) and the interior kernel k_fwd_int with its
 * EDGE form (specialised filters; it also classifies what it writes for the fused selection).
 * After fb_device.inc.
 */
#pragma clang fp contract(off)

namespace wtp {

/* ------------------------------------------------------------- analysis --- */
struct FwdArgs {
    const float* in;
    int64_t in_bs;       /* batch stride of the input level */
    int R, C;            /* input level dims (row pitch C) */
    int Ro, Co;          /* output dims per subband */
    float* P;
    int64_t P_bs;        /* packed image per batch item: PR * PC */
    int PC, offR, offC;  /* level-k detail origin in the packed image */
    float* anext;        /* (B, Ro, Co) next-level approximation; unused when last */
    int last, tilesC, tilesR;
    int al16;            /* in is 16-byte aligned and C % 4 == 0: interior tiles load float4 rows */
    /* the interior tiles (k_fwd_int): rows tr0 .. tr0 + nTR - 1, columns tc0 .. tc0 + nTC - 1 of
     * the tile grid; frame != 0: k_fwd_level runs only the tiles around that rectangle */
    int tr0, nTR, tc0, nTC, frame;
};

/* One launch covers the same level of up to FB_UNI items of the SAME geometry (same filter; the
 * cfg5 blocks of a call, the batch of one tensor): the geometry once, the pointers per item, and
 * a block's item is its tile / tiles-per-item.  The specialised kernels take their taps as a
 * SmallTaps (F <= 20): the whole argument stays near 2 KB. */
struct FwdGroup {
    FwdArgs geo;            /* the items' geometry; its pointers are unused */
    int n, tiles;           /* items; tiles per item */
    FastDiv dv_tiles, dv_per, dv_ntc; /* k_*_int: by tiles, by the rectangle's (or frame's) tiles, by nTC */
    FastDiv dv_tc, dv_side;           /* the frame's decode: by tilesC, by tilesC - nTC */
    const float* in[FB_UNI];
    float* anext[FB_UNI];
    float* P[FB_UNI];
};

/* taps of the interior kernels: analysis {dec_lo[j], dec_hi[j]} adjacent, so one SGPR pair is
 * both bands' packed tap */
struct FwdIntTaps {
    f2 t[SM_F_MAX];
};

template <int FT>
__global__ __launch_bounds__(FB_THREADS) WTP_FB_FWD_WPE void k_fwd_level(FwdGroup g, TapsT<FT> tp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int F = FT ? FT : tp.F;
    const int NR = 2 * FR + F - 2, NC = 2 * FC + F - 2;
    float* T = lds;                /* NR x NC input tile */
    /* FR x NC: (L, H) column-pass outputs, even columns then odd (row-pass reads at stride 2
     * stay conflict-free).  Specialised filters hold their column results in registers across
     * a barrier and write them over the input tile: half the LDS, twice the workgroups per CU */
    float2* LH = reinterpret_cast<float2*>(FT > 0 ? lds : lds + NR * NC);
    const int HALF = (NC + 1) / 2;
    auto lhi = [&](int o, int cc) { return o * NC + (cc & 1) * HALF + (cc >> 1); };
    const int gt = xcd_tile(blockIdx.x, gridDim.x);
    const int item = gt / g.tiles;
    FwdArgs a = g.geo;
    a.in = g.in[item];
    a.anext = g.anext[item];
    a.P = g.P[item];
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
    const int o0r = tr * FR, o0c = tc * FC;
    const int gr0 = 2 * o0r - F / 2 + 1, gc0 = 2 * o0c - F / 2 + 1;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const float* x = a.in + (int64_t)b * a.in_bs;
    WTP_FPROBE(0);
    /* 1. input tile with the periodic (odd: repeat-last) extension applied on load.  Rows
     *    go by wave (row index and extension are scalar work), columns by lane (a plain add
     *    except on edge tiles); for the specialised filters the trip counts are compile-time,
     *    so every load of a thread is issued before the first LDS write. */
    {
        const bool cin = gc0 >= 0 && gc0 + NC <= a.C; /* no column extension in this tile */
        auto rowptr = [&](int rr) {
            const int gr = gr0 + rr;
            return x + (int64_t)((gr >= 0 && gr < a.R) ? gr : ext_idx(gr, a.R)) * a.C;
        };
        auto colidx = [&](int cc) {
            const int gc = gc0 + cc;
            return cin ? gc : ((gc >= 0 && gc < a.C) ? gc : ext_idx(gc, a.C));
        };
        if constexpr (FT > 0) {
            constexpr int NRc = 2 * FR + FT - 2, NCc = 2 * FC + FT - 2;
            constexpr int S0 = FWD_S0<FT>, TP = FWD_TP<FT>, W4 = TP / 4;
            const int start = gc0 - S0; /* 16-byte aligned column of the tile's first float4 */
            if (a.al16 && gr0 >= 0 && gr0 + NRc <= a.R && start >= 0 && start + TP <= a.C) {
                /* interior tile: whole float4 rows [start, start + TP), every load of a thread in
                 * flight before its first LDS write (ds_write_b128) */
                constexpr int NE = NRc * W4, K = (NE + FB_THREADS - 1) / FB_THREADS;
                const float* x0 = x + (int64_t)gr0 * a.C + start;
                float4 q[K];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int e = min(k * FB_THREADS + (int)threadIdx.x, NE - 1);
                    const int rr = e / W4, j4 = e - rr * W4;
                    q[k] = *reinterpret_cast<const float4*>(x0 + (int64_t)rr * a.C + 4 * j4);
                }
                /* stored at the same clamped index it was loaded from (a duplicate of element
                 * NE - 1 rewrites its own value): no predicate, so the compiler cannot sink a
                 * load into a branch behind its own wait */
#pragma unroll
                for (int k = 0; k < K; ++k)
                    reinterpret_cast<float4*>(T)[min(k * FB_THREADS + (int)threadIdx.x, NE - 1)] = q[k];
            } else {
                constexpr int RW = (NRc + 3) / 4, CW = (NCc + 63) / 64; /* rows per wave, column chunks */
                int col[CW];
#pragma unroll
                for (int c = 0; c < CW; ++c) col[c] = colidx(min(lane + 64 * c, NCc - 1));
                float v[RW][CW];
#pragma unroll
                for (int k = 0; k < RW; ++k) {
                    const float* xr = rowptr(min(wv + 4 * k, NRc - 1));
#pragma unroll
                    for (int c = 0; c < CW; ++c) v[k][c] = xr[col[c]];
                }
#pragma unroll
                for (int k = 0; k < RW; ++k)
#pragma unroll
                    for (int c = 0; c < CW; ++c) /* clamped like the loads: duplicates rewrite their own value */
                        T[min(wv + 4 * k, NRc - 1) * TP + S0 + min(lane + 64 * c, NCc - 1)] = v[k][c];
            }
        } else {
            for (int rr = wv; rr < NR; rr += FB_THREADS / 64) {
                const float* xr = rowptr(rr);
                for (int cc = lane; cc < NC; cc += 64) T[rr * NC + cc] = xr[colidx(cc)];
            }
        }
    }
    __syncthreads();
    WTP_FPROBE(1);
    /* 2. axis -2 analysis of every tile column: L, H for the tile's output rows */
    const float* flo = tp.f[0];
    const float* fhi = tp.f[1];
    const int nrow = min(FR, a.Ro - o0r);
    if constexpr (FT > 0) {
        /* one tile column and FR/2 consecutive output rows per item: the column's
         * FR + F - 2 samples are read once into registers and shared by the rows */
        constexpr int RH = FR / 2, NV = 2 * RH + FT - 2, NCc = 2 * FC + FT - 2;
        constexpr int NIT = (2 * NCc + FB_THREADS - 1) / FB_THREADS;
        f2 res[NIT][RH];
#pragma unroll
        for (int q = 0; q < NIT; ++q) {
            const int it = threadIdx.x + q * FB_THREADS;
            if (it < 2 * NCc) {
                const int h = it >= NCc, cc = it - h * NCc;
                float v[NV];
#pragma unroll
                for (int k = 0; k < NV; ++k) v[k] = T[(2 * RH * h + k) * FWD_TP<FT> + FWD_S0<FT> + cc];
                const int i0 = FT / 2 + 2 * (o0r + RH * h);
                if (__all(i0 + 2 * (RH - 1) < a.R)) {
                    /* all RH outputs interior: tap-major, so the RH independent sums interleave */
#pragma unroll
                    for (int r = 0; r < RH; ++r) res[q][r] = f2{0.0f, 0.0f};
#pragma unroll
                    for (int j = 0; j < FT; ++j) {
                        const f2 t = {flo[j], fhi[j]};
#pragma unroll
                        for (int r = 0; r < RH; ++r) res[q][r] = res[q][r] + t * v[2 * r + FT - 1 - j];
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < RH; ++r)
                        res[q][r] = ana2_j<FT>(i0 + 2 * r, a.R, flo, fhi, [&](int j) { return v[2 * r + FT - 1 - j]; });
                }
            }
        }
        __syncthreads(); /* every read of T is done: LH overwrites it */
#pragma unroll
        for (int q = 0; q < NIT; ++q) {
            const int it = threadIdx.x + q * FB_THREADS;
            if (it < 2 * NCc) {
                const int h = it >= NCc, cc = it - h * NCc;
#pragma unroll
                for (int r = 0; r < RH; ++r)
                    if (RH * h + r < nrow) LH[lhi(RH * h + r, cc)] = make_float2(res[q][r].x, res[q][r].y);
            }
        }
    } else {
        for (int o = wv; o < nrow; o += FB_THREADS / 64) {
            const int i = F / 2 + 2 * (o0r + o);
            for (int cc = lane; cc < NC; cc += 64) {
                const f2 r = ana2<FT>(i, a.R, F, flo, fhi, [&](int g) { return T[(g - gr0) * NC + cc]; });
                LH[lhi(o, cc)] = make_float2(r.x, r.y);
            }
        }
    }
    __syncthreads();
    WTP_FPROBE(2);
    /* 3. axis -1 analysis of the L and H rows -> aa, ad, da, dd (packed layout) */
    float* Pb = a.P + (int64_t)b * a.P_bs;
    const int oc = o0c + lane;
    if (lane < FC && oc < a.Co) {
        const int i = F / 2 + 2 * oc;
        auto put = [&](int o, f2 low, f2 high) { /* low = (aa, da), high = (ad, dd) */
            const int r = o0r + o;
            if (a.last) Pb[(int64_t)r * a.PC + oc] = low.x;
            else a.anext[((int64_t)b * a.Ro + r) * a.Co + oc] = low.x;
            Pb[(int64_t)r * a.PC + a.offC + oc] = high.x;
            Pb[(int64_t)(a.offR + r) * a.PC + oc] = low.y;
            Pb[(int64_t)(a.offR + r) * a.PC + a.offC + oc] = high.y;
        };
        bool done = false;
        if constexpr (FT > 0) {
            if (nrow == FR && __all(i < a.C)) {
                /* full tile, interior columns: two rows at a time, their four sums interleaved */
                constexpr int NW = FB_THREADS / 64;
                static_assert(FR % (2 * NW) == 0, "row pairs per wave");
#pragma unroll
                for (int pr = 0; pr < FR / (2 * NW); ++pr) {
                    const int oA = wv + 2 * NW * pr, oB = oA + NW;
                    f2 vA[FT], vB[FT];
#pragma unroll
                    for (int j = 0; j < FT; ++j) {
                        const float2 xa = LH[lhi(oA, i - j - gc0)], xb = LH[lhi(oB, i - j - gc0)];
                        vA[j] = f2{xa.x, xa.y};
                        vB[j] = f2{xb.x, xb.y};
                    }
                    f2 aA = {0.0f, 0.0f}, dA = {0.0f, 0.0f}, aB = {0.0f, 0.0f}, dB = {0.0f, 0.0f};
#pragma unroll
                    for (int j = 0; j < FT; ++j) {
                        aA = aA + flo[j] * vA[j];
                        dA = dA + fhi[j] * vA[j];
                        aB = aB + flo[j] * vB[j];
                        dB = dB + fhi[j] * vB[j];
                    }
                    put(oA, aA, dA);
                    put(oB, aB, dB);
                }
                done = true;
            }
        }
        for (int o = wv; !done && o < nrow; o += FB_THREADS / 64) {
            f2 low, high;
            ana2x2<FT>(i, a.C, F, flo, fhi,
                       [&](int g) {
                           const float2 v = LH[lhi(o, g - gc0)];
                           return f2{v.x, v.y};
                       },
                       low, high);
            put(o, low, high);
        }
    }
    WTP_FPROBE(3);
}

/* One analysis level over the INTERIOR tiles of a group (FwdGroup geo: tr0/nTR/tc0/nTC): every
 * tile's input window lies inside the image and its float4 rows are aligned, every output is a
 * full-tile interior site (i < N: ascending taps), so none of k_fwd_level's edge forms is compiled
 * in.  EDGE: the same kernel over the FRAME of tiles around that rectangle (FwdArgs.frame's decode):
 * the input tile gathered with the periodic (odd: repeat-last) extension as k_fwd_level loads it,
 * pywt's split order (wrapped terms first, wt_ana_point) only in the waves holding an output site
 * i >= N, stores masked to the level's extent.  Same sums in the same order (pywt's
 * ascending-tap interior form, every sum from 0 as pywt starts it, so even the sign of a zero
 * matches).  Instruction shape:
 *   column pass: a thread's column samples are read as PAIRS of consecutive rows into aligned
 *   register pairs, so the packed multiply broadcasts either sample by op_sel (no realigning
 *   move), against the {lo[j], hi[j]} tap pair in one SGPR pair;
 *   row pass: as k_fwd_level's interior form; stores by buffer instructions whose row offset is a
 *   scalar (the row is wave-uniform) and column offset the lane's -- no 64-bit address math. */
template <int FT, bool EDGE>
__global__ __launch_bounds__(FB_THREADS) WTP_FB_INT_WPE void k_fwd_int(FwdGroup g, FwdIntTaps tp, FwdSel fs) {
    static_assert(FT > 0 && FT % 2 == 0, "specialised even filters");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NRc = 2 * FR + FT - 2, NCc = 2 * FC + FT - 2;
    constexpr int S0 = FWD_S0<FT>, TP = FWD_TP<FT>, W4 = TP / 4;
    constexpr int HALF = fwd_lhh(NCc);
    static_assert(HALF % 16 == 8 && HALF >= (NCc + 1) / 2, "LH half pitch");
    float* T = lds;
    float2* LH = reinterpret_cast<float2*>(lds);
    const int gt = xcd_tile(blockIdx.x, gridDim.x);
    const int item = fdiv(gt, g.dv_tiles);
    const FwdArgs& a = g.geo;
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
    const int o0r = trow * FR, o0c = tcol * FC;
    const int gr0 = 2 * o0r - FT / 2 + 1, gc0 = 2 * o0c - FT / 2 + 1;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const float* x = g.in[item] + (int64_t)b * a.in_bs;
    /* fused selection (FwdSel): the window of the item's segment, by scalar loads in flight with
     * the tile's, and the wave's slot */
    const bool fsel = fs.on != 0;
    uint32_t skl = 0, sspan = 0;
    FslHeader* sst = nullptr;
    uint32_t* wslot = nullptr;
    if (fsel) {
        sst = fs.hdr[item];
        skl = sst->kl;
        sspan = sst->kh - skl;
        wslot = fs.slots[item] + ((int64_t)tile * (FB_THREADS / 64) + wv) * FSL_WORDS;
    }
    WTP_FPROBE(0);
    /* 1. the input tile; every load of a thread in flight before its first LDS write */
    if (EDGE && a.al16 && !(a.R & 1) && a.R >= NRc && a.C >= TP) {
        /* a frame tile of an even, aligned level: the interior kernel's float4 rows, each row and
         * each float4 wrapped once (C % 4 == 0 and the tile's first column is 16-byte aligned, so
         * a float4 lies wholly inside or wholly across the edge; periodic, no repeat-last) */
        constexpr int NE = NRc * W4, K = (NE + FB_THREADS - 1) / FB_THREADS;
        const int start = gc0 - S0;
        float4 q[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int e = min(k * FB_THREADS + (int)threadIdx.x, NE - 1);
            const int rr = e / W4, j4 = e - rr * W4;
            int r = gr0 + rr, c = start + 4 * j4;
            r = r < 0 ? r + a.R : (r >= a.R ? r - a.R : r);
            c = c < 0 ? c + a.C : (c >= a.C ? c - a.C : c);
            q[k] = *reinterpret_cast<const float4*>(x + (int64_t)r * a.C + c);
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            reinterpret_cast<float4*>(T)[min(k * FB_THREADS + (int)threadIdx.x, NE - 1)] = q[k];
    } else if constexpr (EDGE) {
        /* rows by wave (row index and extension are scalar work), columns by lane; clamped
         * duplicates rewrite their own value */
        constexpr int RW = (NRc + 3) / 4, CW = (NCc + 63) / 64;
        int col[CW];
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            const int gc = gc0 + min(lane + 64 * c, NCc - 1);
            col[c] = (gc >= 0 && gc < a.C) ? gc : ext_idx(gc, a.C);
        }
        float v[RW][CW];
#pragma unroll
        for (int k = 0; k < RW; ++k) {
            const int gr = gr0 + min(wv + 4 * k, NRc - 1);
            const float* xr = x + (int64_t)((gr >= 0 && gr < a.R) ? gr : ext_idx(gr, a.R)) * a.C;
#pragma unroll
            for (int c = 0; c < CW; ++c) v[k][c] = xr[col[c]];
        }
#pragma unroll
        for (int k = 0; k < RW; ++k)
#pragma unroll
            for (int c = 0; c < CW; ++c) T[min(wv + 4 * k, NRc - 1) * TP + S0 + min(lane + 64 * c, NCc - 1)] = v[k][c];
    } else {
        /* whole float4 rows from the aligned column gc0 - S0: buffer loads over the tile's rows, a
         * 32-bit offset each (fwd_interior bounds the tile's span below 2^31 bytes) */
        constexpr int NE = NRc * W4, K = (NE + FB_THREADS - 1) / FB_THREADS;
        const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(x) + (int64_t)gr0 * a.C + (gc0 - S0), 0, 4 * ((NRc - 1) * a.C + TP), 0x00020000);
        float4 q[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int e = min(k * FB_THREADS + (int)threadIdx.x, NE - 1);
            const int rr = e / W4, j4 = e - rr * W4;
            typedef uint32_t u4 __attribute__((ext_vector_type(4)));
            const u4 w = __builtin_amdgcn_raw_buffer_load_b128(rX, 4 * (rr * a.C + 4 * j4), 0, 0);
            q[k] = make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            reinterpret_cast<float4*>(T)[min(k * FB_THREADS + (int)threadIdx.x, NE - 1)] = q[k];
    }
    __syncthreads();
    WTP_FPROBE(1);
    /* 2. axis -2: one tile column and FR/2 consecutive output rows per item; item it = h HP + cc, with
     * HP a multiple of 64 when NC fits in 128 (F <= 18): no wave holds items of both halves, whose
     * column reads 2 RH rows apart would otherwise share LDS banks (round 6, with the LH pitch) */
    constexpr int RH = FR / 2, NV = 2 * RH + FT - 2, NP = NV / 2;
    constexpr int HP = NCc <= 128 ? 128 : NCc;
    constexpr int NIT = (2 * HP + FB_THREADS - 1) / FB_THREADS;
    static_assert(NV % 2 == 0, "sample pairs");
    f2 res[NIT][RH];
#pragma unroll
    for (int q = 0; q < NIT; ++q) {
        const int it = threadIdx.x + q * FB_THREADS;
        const int h = it >= HP, cc = it - h * HP;
        if (it < 2 * HP && cc < NCc) {
            const float* col = T + (2 * RH * h) * TP + S0 + cc;
            f2 P[NP];
#pragma unroll
            for (int m = 0; m < NP; ++m) P[m] = f2{col[(2 * m) * TP], col[(2 * m + 1) * TP]};
            auto smp = [&](int s) { return (s & 1) ? P[s >> 1].yy : P[s >> 1].xx; };
            const int i0 = FT / 2 + 2 * (o0r + RH * h); /* the site of the item's first output row */
            if (!EDGE || __all(i0 + 2 * (RH - 1) < a.R)) {
#pragma unroll
                for (int r = 0; r < RH; ++r) res[q][r] = f2{0.0f, 0.0f} + tp.t[0] * smp(2 * r + FT - 1);
#pragma unroll
                for (int j = 1; j < FT; ++j)
#pragma unroll
                    for (int r = 0; r < RH; ++r) res[q][r] = res[q][r] + tp.t[j] * smp(2 * r + FT - 1 - j);
            } else {
                /* wt_ana_point's order: the wrapped terms (i - j >= N) by descending j, then the
                 * rest ascending -- for a site i < N that is the ascending interior sum */
#pragma unroll
                for (int r = 0; r < RH; ++r) {
                    const int i = i0 + 2 * r;
                    f2 acc = {0.0f, 0.0f};
#pragma unroll
                    for (int j = FT - 1; j >= 0; --j)
                        if (i - j >= a.R) acc = acc + tp.t[j] * smp(2 * r + FT - 1 - j);
#pragma unroll
                    for (int j = 0; j < FT; ++j)
                        if (i - j < a.R) acc = acc + tp.t[j] * smp(2 * r + FT - 1 - j);
                    res[q][r] = acc;
                }
            }
        }
    }
    __syncthreads(); /* every read of T is done: LH overwrites it */
    auto lhi = [&](int o, int cc) { return o * (2 * HALF) + (cc & 1) * HALF + (cc >> 1); };
#pragma unroll
    for (int q = 0; q < NIT; ++q) {
        const int it = threadIdx.x + q * FB_THREADS;
        const int h = it >= HP, cc = it - h * HP;
        if (it < 2 * HP && cc < NCc) {
#pragma unroll
            for (int r = 0; r < RH; ++r) LH[lhi(RH * h + r, cc)] = make_float2(res[q][r].x, res[q][r].y);
        }
    }
    __syncthreads();
    WTP_FPROBE(2);
    /* 3. axis -1 of the L and H rows -> aa, ad, da, dd; two rows per step, four sums interleaved */
    constexpr int NW = FB_THREADS / 64, NPR = FR / (2 * NW);
    static_assert(FR % (2 * NW) == 0, "row pairs per wave");
    auto flo = [&](int k) { return (k & 1) ? tp.t[k >> 1].y : tp.t[k >> 1].x; };
    /* EDGE: the outputs whose site wraps past the row's end (ic >= C: the level's last F/4 or so
     * columns) are skipped by the uniform pass and computed in wt_ana_point's split order by a
     * compact fix-up: lane e of the wave = (its row e / nsc, the (e % nsc)-th such column) */
    uint64_t fxm = 0;
    if constexpr (EDGE) {
        const int ic = FT / 2 + 2 * (o0c + lane);
        fxm = __ballot(lane < FC && ic >= a.C && o0c + lane < a.Co);
    }
    /* fused selection: every coefficient the wave writes to P is classified against the window
     * [kl, kh] as k_collect classifies a chunk: keys < kl and == kl counted (ballot popcounts), the
     * largest key kept, the keys inside (kl, kh] appended to the wave's slot in write order.  Every
     * lane of the row pass takes every call (ok = the output exists), so the running count stays
     * the same in all of them. */
    uint32_t f_below = 0, f_eq = 0, f_cnt = 0, f_mx = 0;
    /* keys <= kl are counted together as "below" (one compare a key): the select then sees no key
     * at kl, so a rank at or under kl -- ties at the window's lower edge -- reads as a miss and is
     * retried over P, exactly.  The largest key is kept three at a time (fmax3). */
    auto fcls = [&](float v, bool ok) {
        const uint32_t k = __float_as_uint(v) & 0x7FFFFFFFu;
        f_below += (uint32_t)__popcll(__ballot(ok && k <= skl));
        const bool in = ok && k - skl - 1u < sspan;
        const uint64_t m = __ballot(in);
        if (m) {
            const uint32_t pos = f_cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (in && pos < (uint32_t)FSL_KEYS) wslot[1 + pos] = k;
            f_cnt += (uint32_t)__popcll(m);
        }
    };
    auto fmax3 = [&](float a, float b, float c, bool ok) {
        const uint32_t m3 = max(max(__float_as_uint(a) & 0x7FFFFFFFu, __float_as_uint(b) & 0x7FFFFFFFu),
                                __float_as_uint(c) & 0x7FFFFFFFu);
        f_mx = ok ? max(f_mx, m3) : f_mx;
    };
    if (lane < FC) {
        const __amdgpu_buffer_rsrc_t rP =
            __builtin_amdgcn_make_buffer_rsrc(g.P[item] + (int64_t)b * a.P_bs, 0, (int)(4 * a.P_bs), 0x00020000);
        const __amdgpu_buffer_rsrc_t rA = a.last ? rP
            : __builtin_amdgcn_make_buffer_rsrc(g.anext[item] + (int64_t)b * a.Ro * a.Co, 0, 4 * a.Ro * a.Co, 0x00020000);
        const int pitchA = a.last ? a.PC : a.Co;
        const int voff = 4 * (o0c + lane);
        const int ic = FT / 2 + 2 * (o0c + lane); /* the lane's output site along the row */
        const bool cin = !EDGE || (o0c + lane < a.Co && ic < a.C);
#pragma unroll
        for (int pr = 0; pr < NPR; ++pr) {
            const int oA = wv + 2 * NW * pr, oB = oA + NW;
            f2 vA[FT], vB[FT];
#pragma unroll
            for (int j = 0; j < FT; ++j) { /* sample cc = 2 lane + FT - 1 - j of the row */
                const float2 xa = LH[lhi(oA, 2 * lane + FT - 1 - j)], xb = LH[lhi(oB, 2 * lane + FT - 1 - j)];
                vA[j] = f2{xa.x, xa.y};
                vB[j] = f2{xb.x, xb.y};
            }
            const f2 z2 = {0.0f, 0.0f};
            f2 aA, dA, aB, dB;
            aA = z2 + flo(0) * vA[0];
            dA = z2 + flo(1) * vA[0];
            aB = z2 + flo(0) * vB[0];
            dB = z2 + flo(1) * vB[0];
#pragma unroll
            for (int j = 1; j < FT; ++j) {
                const float tl = flo(2 * j), th = flo(2 * j + 1);
                aA = aA + tl * vA[j];
                dA = dA + th * vA[j];
                aB = aB + tl * vB[j];
                dB = dB + th * vB[j];
            }
            /* low = (aa, da), high = (ad, dd) */
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int r = o0r + (u ? oB : oA);
                const bool ok = !EDGE || (cin && r < a.Ro);
                const f2 lw = u ? aB : aA, hg = u ? dB : dA;
                if (fsel) {
                    fcls(hg.x, ok);
                    fcls(lw.y, ok);
                    fcls(hg.y, ok);
                    fmax3(hg.x, lw.y, hg.y, ok);
                    if (a.last) { fcls(lw.x, ok); fmax3(lw.x, lw.x, lw.x, ok); }
                }
                if (!ok) continue;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(lw.x), rA, voff, 4 * r * pitchA, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hg.x), rP, voff, 4 * (r * a.PC + a.offC), 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(lw.y), rP, voff, 4 * ((a.offR + r) * a.PC), 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hg.y), rP, voff, 4 * ((a.offR + r) * a.PC + a.offC), 0);
            }
        }
    }
    if (EDGE && fxm) { /* uniform */
        const int nsc = __builtin_popcountll(fxm);
        /* the fix-up lanes are row-pass lanes (lane < FC): their running slot count is current */
        static_assert(2 * NPR * (FT / 4 + 2) <= FC, "one fix-up pass per wave");
        if (lane < 2 * NPR * nsc) {
            const int rs = lane / nsc, ci = lane - rs * nsc;
            uint64_t mm = fxm;
            for (int t = 0; t < ci; ++t) mm &= mm - 1ull;
            const int cl = __builtin_ctzll(mm); /* the column's lane in the uniform pass */
            const int o = wv + NW * rs;       /* the wave's rows: wv + NW * (2 pr + u) */
            const int r = o0r + o;
            {
                const bool ok = r < a.Ro;
                const int ic = FT / 2 + 2 * (o0c + cl);
                f2 v[FT];
#pragma unroll
                for (int j = 0; j < FT; ++j) { const float2 xv = LH[lhi(o, 2 * cl + FT - 1 - j)]; v[j] = f2{xv.x, xv.y}; }
                f2 lw = {0.0f, 0.0f}, hg = {0.0f, 0.0f};
                auto term = [&](int j) { lw = lw + flo(2 * j) * v[j]; hg = hg + flo(2 * j + 1) * v[j]; };
#pragma unroll
                for (int j = FT - 1; j >= 0; --j)
                    if (ic - j >= a.C) term(j);
#pragma unroll
                for (int j = 0; j < FT; ++j)
                    if (ic - j < a.C) term(j);
                const __amdgpu_buffer_rsrc_t rP =
                    __builtin_amdgcn_make_buffer_rsrc(g.P[item] + (int64_t)b * a.P_bs, 0, (int)(4 * a.P_bs), 0x00020000);
                const __amdgpu_buffer_rsrc_t rA = a.last ? rP
                    : __builtin_amdgcn_make_buffer_rsrc(g.anext[item] + (int64_t)b * a.Ro * a.Co, 0, 4 * a.Ro * a.Co, 0x00020000);
                const int pitchA = a.last ? a.PC : a.Co;
                const int vo = 4 * (o0c + cl);
                if (fsel) {
                    fcls(hg.x, ok);
                    fcls(lw.y, ok);
                    fcls(hg.y, ok);
                    fmax3(hg.x, lw.y, hg.y, ok);
                    if (a.last) { fcls(lw.x, ok); fmax3(lw.x, lw.x, lw.x, ok); }
                }
                if (ok) {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(lw.x), rA, vo, 4 * r * pitchA, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hg.x), rP, vo, 4 * (r * a.PC + a.offC), 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(lw.y), rP, vo, 4 * ((a.offR + r) * a.PC), 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hg.y), rP, vo, 4 * ((a.offR + r) * a.PC + a.offC), 0);
                }
            }
        }
    }
    if (fsel) { /* the wave's slot count (lane 0 took every call); the workgroup's counters */
        __shared__ uint32_t s_fc[FB_THREADS / 64][3];
        uint32_t mx = f_mx;
#pragma unroll
        for (int o = 32; o; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
        if (lane == 0) {
            wslot[0] = f_cnt;
            s_fc[wv][0] = f_below;
            s_fc[wv][1] = f_eq;
            s_fc[wv][2] = mx;
            if (f_cnt > (uint32_t)FSL_KEYS) atomicOr(&sst->overflow, 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t b = 0, e = 0, m = 0;
#pragma unroll
            for (int w = 0; w < FB_THREADS / 64; ++w) { b += s_fc[w][0]; e += s_fc[w][1]; m = max(m, s_fc[w][2]); }
            const int sh8 = blockIdx.x & (NSHARD - 1);
            if (b | e) atomicAdd(&sst->be[sh8], ((unsigned long long)e << 32) | b);
            if (m) atomicMax(&sst->maxkey[sh8], m);
        }
    }
    WTP_FPROBE(3);
}

}  // namespace wtp
