"""Device unit tests of the exact percentile selection's wave and block steps (csrc/wtp_device.h,
csrc/wtp_select.h, the window search of csrc/resident.inc, collect_body of csrc/select.inc), each
called directly through tests/native/selcheck.hip and held to numpy on the same integers
(np.sort, np.cumsum, np.searchsorted; equality is exact), and select_body / collect_body at windows
the test chooses, against the C oracle's percentile.  Inputs stay inside every step's documented
domain (keys in [lo, hi], r < m, W <= HS_PER * THREADS, m <= 64 * KPL): outside it the steps index
LDS out of bounds, which is not what is tested here."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import selcheck_shim as S
from tests.ref_helpers import SEL_NB, np_key_bin, np_ranks
from tests.special_values import assert_same_bits, f32_from_bits

pytestmark = pytest.mark.gpu

NB = SEL_NB
OPEN = 0xFFFFFFFF
U32 = np.uint32


@pytest.fixture(scope="module")
def lib():
    L = S.load()
    if S.BUILD_SECONDS is not None:
        print("\nselcheck harness built in %.1f s" % S.BUILD_SECONDS)
    return L


@pytest.fixture(scope="module")
def edges(lib):
    """(bin_lo_key, bin_hi_key) of every bin, as tests/test_select_host.py pins them"""
    lo, hi, b = np.zeros(NB, U32), np.zeros(NB, U32), np.zeros(1, np.int32)
    lib.sc_bins_host(S.ptr(np.zeros(1, U32)), 1, S.ptr(b), S.ptr(lo), S.ptr(hi))
    return lo, hi


def u32(a):
    return np.ascontiguousarray(np.asarray(a).astype(U32))


def i32(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.int32))


def i64(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.int64))


# ----------------------------------------------------------------------------- wave primitives
def wave_cases(kind):
    rng = np.random.default_rng(11)
    if kind == "random_lanes":
        v = rng.integers(0, 1 << 32, (6, 64), dtype=np.uint64)
        v[4] >>= 12
        v[5] &= 1
        w = rng.integers(0, (1 << 40) + 1, (6, 64), dtype=np.uint64)
        w[0, :] = 1 << 40
    elif kind == "one_nonzero_lane_each_of_64":  # rows end at lanes 15 / 31 / 47: the row_bcast steps
        v = np.zeros((64, 64), np.uint64)
        w = np.zeros((64, 64), np.uint64)
        for l in range(64):
            v[l, l] = 0x80000001 + 977 * l
            w[l, l] = (1 << 40) - l
    else:  # all_lanes_ffffffff: the scan wraps
        v = np.full((1, 64), 0xFFFFFFFF, np.uint64)
        w = np.full((1, 64), 1 << 40, np.uint64)
    return v, w


@pytest.mark.parametrize("kind", ["random_lanes", "one_nonzero_lane_each_of_64", "all_lanes_ffffffff"])
def test_wave_scan_sum_max_min_or_sum64(lib, kind):
    v, w = wave_cases(kind)
    n = len(v)
    vin, win = u32(v), np.ascontiguousarray(w)
    scan, red, s64 = np.zeros((n, 64), U32), np.zeros((n, 2, 4), U32), np.zeros((n, 2), np.uint64)
    assert lib.sc_wave_prims(S.ptr(vin), S.ptr(win), n, S.ptr(scan), S.ptr(red), S.ptr(s64)) == 0
    want_scan = (np.cumsum(v, axis=1) & 0xFFFFFFFF).astype(U32)
    assert np.array_equal(scan, want_scan)
    want = np.stack([want_scan[:, 63], vin.max(axis=1), vin.min(axis=1), np.bitwise_or.reduce(vin, axis=1)], axis=1)
    for lane in (0, 1):  # as lane 0 and as lane 63 hold them
        assert np.array_equal(red[:, lane, :], want), lane
        assert np.array_equal(s64[:, lane], w.sum(axis=1)), lane


# ------------------------------------------------------------------------------ wave_pick_digit
def digit_hist(kind):
    rng = np.random.default_rng(12)
    h = np.zeros(256, np.int64)
    if kind == "sparse_bins_first_and_last_key":
        idx = rng.choice(256, 60, replace=False)
        h[idx] = rng.integers(1, 50, 60)
        h[[0, 3, 4, 7, 255]] = [2, 1, 1, 5, 3]
    elif kind == "empty_bins_around_the_rank":
        h[[2, 101, 102, 103, 250]] = [7, 1, 9, 1, 4]
    elif kind == "all_in_bin_0":
        h[0] = 1000
    elif kind == "all_in_bin_255":
        h[255] = 1000
    else:  # total_near_2p31
        h[:] = (1 << 23) - 1
        h[[5, 6, 200]] = 0
        h[255] += (1 << 31) - 9 - h.sum()
    return h


@pytest.mark.parametrize("kind", ["sparse_bins_first_and_last_key", "empty_bins_around_the_rank", "all_in_bin_0",
                                  "all_in_bin_255", "total_near_2p31"])
def test_wave_pick_digit(lib, kind):
    h = digit_hist(kind)
    cs = np.cumsum(h)
    ne = np.nonzero(h)[0]
    ranks = i64(np.unique(np.concatenate([cs[ne] - h[ne], cs[ne] - 1, cs[ne] - h[ne] + h[ne] // 2])))
    assert ranks.min() == 0 and ranks.max() == cs[-1] - 1 and cs[-1] < 1 << 31
    digit, below = np.full(len(ranks), -1, np.int32), np.full(len(ranks), -1, np.int64)
    assert lib.sc_pick_digit(S.ptr(u32(h)), S.ptr(ranks), len(ranks), S.ptr(digit), S.ptr(below)) == 0
    want = np.searchsorted(cs, ranks, side="right")
    assert np.array_equal(digit, want)
    assert np.array_equal(below, cs[want] - h[want])


# -------------------------------------------------------- wave_find_bin, wave_find_bins_flat
def bin_hist(kind):
    rng = np.random.default_rng(13)
    h = np.zeros(NB, np.int64)
    if kind == "ones_every_fine_bin":
        h[:] = 1
    elif kind == "random_sparse":
        idx = rng.choice(NB, 300, replace=False)
        h[idx] = rng.integers(1, 6, 300)
        h[[0, 127, 128, 4095, 4096, 4098]] = [1, 2, 1, 3, 1, 2]
    elif kind == "short_last_coarse_bin_4096_to_4098":
        h[[4096, 4097, 4098]] = [3, 1, 2]
    elif kind == "one_bin_only":
        h[1777] = 11
    else:  # last_bin_of_every_lane: bin 65 l + 64, found by elimination in the flat search
        h[65 * np.arange(63) + 64] = rng.integers(1, 4, 63)
    return h


BIN_KINDS = ["ones_every_fine_bin", "random_sparse", "short_last_coarse_bin_4096_to_4098", "one_bin_only",
             "last_bin_of_every_lane"]


def bin_of_rank(h, r):
    """the bin holding 0-based rank r of the histogram, -1 outside [0, total)"""
    cs = np.cumsum(h)
    r = np.asarray(r, np.int64)
    b = np.searchsorted(cs, np.clip(r, 0, cs[-1] - 1), side="right")
    return np.where((r < 0) | (r >= cs[-1]), -1, b)


@pytest.mark.parametrize("kind", BIN_KINDS)
def test_wave_find_bin(lib, kind):
    h = bin_hist(kind)
    total = int(h.sum())
    ranks = i32(np.concatenate([np.arange(total), [-1, -5, total, total + 7]]))
    out = np.full(len(ranks), -9, np.int32)
    assert lib.sc_find_bin(S.ptr(u32(h)), S.ptr(ranks), len(ranks), S.ptr(out)) == 0
    assert np.array_equal(out, bin_of_rank(h, ranks))
    if kind == "ones_every_fine_bin":
        assert np.array_equal(out[:NB], np.arange(NB))


@pytest.mark.parametrize("kind", BIN_KINDS)
def test_wave_find_bins_flat(lib, kind):
    h = bin_hist(kind)
    total = int(h.sum())
    allr = np.arange(total)
    ra = np.concatenate([allr, allr, np.full(total, -1), allr[::-1], [-1, total, -1]])
    rb = np.concatenate([allr, np.full(total, -1), allr, np.roll(allr, 1), [-1, -1, total + 3]])  # ra == rb first
    ra, rb = i32(ra), i32(rb)
    fa, fb = np.full(len(ra), -9, np.int32), np.full(len(ra), -9, np.int32)
    assert lib.sc_find_bins_flat(S.ptr(u32(h)), S.ptr(ra), S.ptr(rb), len(ra), S.ptr(fa), S.ptr(fb)) == 0
    assert np.array_equal(fa, bin_of_rank(h, ra))
    assert np.array_equal(fb, bin_of_rank(h, rb))
    if kind == "last_bin_of_every_lane":
        assert set(fa[:total] % 65) == {64}


# --------------------------------------------------------------------------- the window searches
def np_window(h, edges, n, r0, above, nsub_log2, MS=4096, sig=6.0, add=24.0):
    """The header comment's rule: sample ranks r0, r1 for n <= MS, else floor(s0 - d), ceil(s1 + d)
    with d = 6 sqrt(m p (1 - p)) + 24; window edges are the bin edges of the bins holding them
    (open where a rank falls off the sample); sh from the span and nsub_log2."""
    lo, hi = edges
    m = n if n <= MS else MS
    r1 = r0 if above else r0 + 1
    if n <= MS:
        sa, sb = r0, r1
    else:
        p = r0 / (n - 1)
        s0, s1 = p * (m - 1), r1 / (n - 1) * (m - 1)
        d = sig * math.sqrt(m * p * (1.0 - p)) + add
        sa, sb = math.floor(s0 - d), math.ceil(s1 + d)
    assert int(h.sum()) == m
    f0 = int(bin_of_rank(h, sa))
    f1 = int(bin_of_rank(h, sb)) if sb < m else -1
    kl = 0 if sa < 0 or f0 < 0 else int(lo[f0])
    kh = OPEN if sb >= m or f1 < 0 else int(hi[f1])
    sh = 0
    if kh > kl + 1:
        sh = max(0, (kh - kl - 1).bit_length() - nsub_log2)
    return kl, kh, sh


def window_keys(kind, m):
    rng = np.random.default_rng(14)
    if kind == "normal":
        x = (rng.standard_normal(m) * 0.05).astype(np.float32)
        return x.view(U32) & U32(0x7FFFFFFF)
    if kind == "all_in_BIN_ZERO":
        return np.zeros(m, U32)
    if kind == "all_in_BIN_UNDER":
        return rng.integers(1, 0x32800000, m).astype(U32)
    if kind == "all_in_BIN_OVER":
        return rng.integers(0x42800000, 0x7F800001, m).astype(U32)
    return rng.integers(0x3D010000, 0x3D020000, m).astype(U32)  # one_bin_wide


WINDOW_CASES = [("normal", n) for n in (1, 2, 3, 4095, 4096, 4097, 10 ** 6)] + [
    (k, n) for k in ("all_in_BIN_ZERO", "all_in_BIN_UNDER", "all_in_BIN_OVER", "one_bin_wide") for n in (3, 10 ** 6)]


@pytest.mark.parametrize("kind,n", WINDOW_CASES, ids=["%s-n%d" % c for c in WINDOW_CASES])
def test_window_searches_agree_and_follow_the_rule(lib, edges, kind, n):
    """window_search<256, 4096> (k_collect's inline window), <1024, 4096>, window_search_wave<4096>
    and window_search_flat give the same (kl, kh, sh), which is the rule's; window_search<1024, 65536>
    (k_window, k_fwin) follows the rule at its own sample size.  Cases per histogram: r0 = 0 (open
    below), the middle, n - 2, and above = 1 at r0 = n - 1 (open above), each at nsub_log2 6..10;
    all_in_BIN_ZERO gives kh <= kl + 1 (sh = 0), one_bin_wide a window one bin wide."""
    keys65 = window_keys(kind, min(n, 65536))
    assert len(np.unique(np_key_bin(keys65))) == 1 or kind == "normal"
    r0s = sorted(c for c in {(0, 0), (n // 2, 0), (n - 2, 0), (n - 1, 1)} if c[1] or 0 <= c[0] <= n - 2)
    cases = i64([(n, r0, above, nl) for r0, above in r0s for nl in range(6, 11)])
    got = {}
    for which, ms in ((0, 4096), (1, 4096), (2, 4096), (3, 4096), (4, 65536)):
        h = np.bincount(np_key_bin(keys65[:min(n, ms)]), minlength=NB)
        out = np.zeros((len(cases), 3), U32)
        assert lib.sc_window(which, S.ptr(u32(h)), S.ptr(cases), len(cases), S.ptr(out)) == 0
        want = [np_window(h, edges, int(c[0]), int(c[1]), int(c[2]), int(c[3]), MS=ms) for c in cases]
        assert out.tolist() == [list(w) for w in want], which
        got[which] = out
    for which in (1, 2, 3):
        assert np.array_equal(got[which], got[0]), which
    if kind == "all_in_BIN_ZERO" and n == 3:
        assert got[0][0].tolist() == [0, 1, 0]
    if kind == "one_bin_wide" and n <= 4096:
        assert np.all(got[0][:, 1] - got[0][:, 0] == 0x10000)
    if n > 4096:  # sampled: r0 = 0 is open below, above = 1 open above
        assert got[0][0, 0] == 0 and got[0][-1, 1] == OPEN


# ------------------------------------------------------------------------- the bin functions
def test_bin_functions_device(lib):
    """key_bin / bin_lo_key / bin_hi_key on the device: tests/test_select_host.py's checks"""
    keys, _, _ = S.round_trip_keys()
    bin_ = np.zeros(len(keys), np.int32)
    lo, hi = np.zeros(NB, U32), np.zeros(NB, U32)
    assert lib.sc_bins(S.ptr(keys), len(keys), S.ptr(bin_), S.ptr(lo), S.ptr(hi)) == 0
    S.bins_checks(keys, bin_, lo, hi)
    e = len(S.EDGE_KEYS)
    assert np.array_equal(bin_[e:e + NB], np.arange(NB))
    assert np.array_equal(bin_[e + NB:e + 2 * NB], np.arange(NB))


# ----------------------------------------------------------------------------- wave_select_rank
def wsel_keys(kind, m):
    rng = np.random.default_rng(15 + m)
    if kind == "narrow_range":
        lo, hi = 0x3D000123, 0x3D000123 + 0xFFF
        k = rng.integers(lo, hi + 1, m)
    elif kind == "all_equal_lo_eq_hi":
        lo = hi = 0x3D5A5A5A
        k = np.full(m, lo)
    elif kind == "keys_at_lo_and_hi":
        lo, hi = 0x3CFFFF00, 0x3D0000FF  # differ from bit 24 down
        k = rng.integers(lo, hi + 1, m)
        k[rng.integers(0, m, max(1, m // 4))] = lo
        k[rng.integers(0, m, max(1, m // 4))] = hi
        k[0] = lo
        k[-1] = hi if m > 1 else lo
    elif kind == "lo_0_hi_ffffffff_top_31":
        lo, hi = 0, OPEN
        k = rng.integers(0, 1 << 31, m)
        k[0] = 0x7FFFFFFF
        k[-1] = 0 if m > 1 else 0x7FFFFFFF
    else:  # heavy_ties
        lo, hi = 0x3D000000, 0x3D00FFFF
        k = rng.choice([lo, lo + 1, lo + 0x8000, hi], m)
    return u32(k), lo, hi


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1023, 1024])
@pytest.mark.parametrize("kind", ["narrow_range", "all_equal_lo_eq_hi", "keys_at_lo_and_hi", "lo_0_hi_ffffffff_top_31",
                                  "heavy_ties"])
def test_wave_select_rank_every_rank(lib, kind, m):
    keys, lo, hi = wsel_keys(kind, m)
    assert keys.min() >= lo and keys.max() <= hi and m <= 64 * S.const(lib, "WSEL_KPL")
    out = np.zeros(m, U32)
    assert lib.sc_wave_select(S.ptr(keys), m, lo, hi, S.ptr(out)) == 0
    assert np.array_equal(out, np.sort(keys))


# ------------------------------------------------------------------------------ select_in_range
def range_of_top(top, rng):
    """[lo, hi] whose highest differing bit is `top` (-1: lo == hi)"""
    if top < 0:
        return 0x3D123456, 0x3D123456
    if top == 31:
        return 0, OPEN
    prefix = 0x3C000000 & ~((2 << top) - 1) if top < 30 else 0
    a, b = (int(rng.integers(0, 1 << top)), int(rng.integers(0, 1 << top))) if top else (0, 0)
    return prefix + a, prefix + (1 << top) + b


@pytest.mark.parametrize("m", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("top", [-1, 0, 6, 7, 8, 15, 16, 30, 31])
def test_select_in_range_first_and_last_digit_widths(lib, top, m):
    """top + 1 bits are unknown: the digits are 8 bits wide from the top, the last one (top + 1) % 8
    bits wide when that is not 0 -- top 0, 6, 8, 16, 30 end in a digit narrower than 8 bits.  Queries:
    first and last rank, ra == rb, adjacent ranks (those whose keys differ in the first digit
    included), need_a only, need_b only."""
    rng = np.random.default_rng(100 * m + top + 1)
    lo, hi = range_of_top(top, rng)
    keys = rng.integers(lo, hi + 1, m, dtype=np.uint64)
    ties = rng.integers(lo, hi + 1, 5, dtype=np.uint64)
    sel = rng.random(m) < 0.4
    keys[sel] = rng.choice(ties, int(sel.sum()))
    keys[0] = lo
    keys[-1] = hi if m > 1 else lo
    keys = u32(keys)
    srt = np.sort(keys)
    rs = set(np.linspace(0, m - 1, min(m, 24)).astype(int).tolist())
    if top >= 0 and m > 1:  # adjacent ranks in different first digits
        shift = max(0, top + 1 - 8)
        rs |= set(np.nonzero(np.diff(srt >> U32(shift)))[0][:8].tolist())
    q = []
    for r in sorted(rs):
        r1 = min(r + 1, m - 1)
        q += [(r, r1, 1, 1), (r, r, 1, 1), (r, m - 1 - r, 1, 0), (m - 1 - r, r, 0, 1)]
    q = i64(q)
    out = np.zeros((len(q), 2), U32)
    assert lib.sc_select_in_range(S.ptr(keys), m, lo, hi, S.ptr(q), len(q), S.ptr(out)) == 0
    na, nb = q[:, 2] == 1, q[:, 3] == 1
    assert np.array_equal(out[na, 0], srt[q[na, 0]])
    assert np.array_equal(out[nb, 1], srt[q[nb, 1]])


# ---------------------------------------------------- block_hist_select, block_count_below
@pytest.mark.parametrize("W", [1, 255, 256, 257, 4095, 4096])
def test_block_hist_select_and_count_below(lib, W):
    """block_hist_select has no caller in the library today (select_body is never given an
    hscratch); it stays in the shared header and is pinned like the rest.  Ranks at the first and
    the last key; block_count_below with tk below all keys, above all keys and at a tied key."""
    rng = np.random.default_rng(W)
    lo = 0x3D000000
    m = 3000
    keys = rng.integers(lo, lo + W, m)
    keys[rng.random(m) < 0.3] = lo + W // 2  # a tied key
    keys[0], keys[1] = lo, lo + W - 1
    keys = u32(keys)
    srt = np.sort(keys)
    ra = i32([0, m - 1, m // 2, 1, m - 2, 1234, 0, m - 1])
    rb = i32([m - 1, 0, m // 2 + 1, 1, m - 2, 77, 0, m - 1])
    sel = np.zeros((len(ra), 2), U32)
    tks = u32([0, lo - 1, lo, lo + 1, lo + W // 2, lo + W // 2 + 1, lo + W - 1, lo + W, OPEN])
    cnt = np.full(len(tks), -1, np.int64)
    assert W <= S.const(lib, "HS_PER") * S.const(lib, "STREAM_THREADS")
    assert lib.sc_block_hist(S.ptr(keys), m, lo, W, S.ptr(ra), S.ptr(rb), len(ra), S.ptr(sel), S.ptr(tks), len(tks),
                             S.ptr(cnt)) == 0
    assert np.array_equal(sel[:, 0], srt[ra]) and np.array_equal(sel[:, 1], srt[rb])
    assert np.array_equal(cnt, np.searchsorted(srt, tks, side="left"))


# ----------------------------------------------------------------------------- wave_find_buckets
@pytest.mark.parametrize("nsub", [64, 128, 256, 512, 1024])
def test_wave_find_buckets(lib, nsub):
    """Ranks in bucket 0, in the last bucket and in the last bucket of a lane, behind runs of empty
    buckets; one rank wanted, both wanted, both in one bucket, adjacent ranks in two buckets."""
    rng = np.random.default_rng(nsub)
    per = nsub // 64
    sub = np.zeros(nsub, np.int64)
    sub[0] = 5
    sub[nsub - 1] = 9000  # counts may pass any bucket capacity
    lanes = rng.choice(np.arange(1, 63), 6, replace=False)
    sub[lanes * per + per - 1] = rng.integers(1, 2000, 6)  # the last bucket of a lane
    free = np.setdiff1d(np.arange(nsub), np.nonzero(sub)[0])
    sub[rng.choice(free, min(6, len(free)), replace=False)] = rng.integers(1, 300, min(6, len(free)))
    cs = np.cumsum(sub)
    ne = np.nonzero(sub)[0]
    first, last = cs[ne] - sub[ne], cs[ne] - 1
    q = []
    for i in range(len(ne)):
        q += [(first[i], last[i], 1, 1), (last[i], last[i], 1, 1), (first[i], 0, 1, 0), (0, last[i], 0, 1)]
        if i + 1 < len(ne):
            q.append((last[i], first[i + 1], 1, 1))  # adjacent ranks, empty buckets between
    q = i64(q)
    bucket, before = np.full((len(q), 2), -7, np.int32), np.full((len(q), 2), -7, np.int64)
    assert lib.sc_find_buckets(S.ptr(u32(sub)), nsub, S.ptr(q), len(q), S.ptr(bucket), S.ptr(before)) == 0
    for col in (0, 1):
        need = q[:, 2 + col] == 1
        b = np.searchsorted(cs, q[:, col], side="right")
        assert np.array_equal(bucket[need, col], b[need]), col
        assert np.array_equal(before[need, col], (cs[b] - sub[b])[need]), col
        assert np.all(bucket[~need, col] == -1) and np.all(before[~need, col] == -1)


# ============================================================ select_body at a chosen window
CAND, WINDOW, FULL = 1, 2, 3
SEG_MASK, SEG_MINPRUNE = 1, 4
REC0 = dict(numel=-11, zero_count=0, coeff_numel=-13, thr64=-17.5, thr32_bits=0xABABABAB, max_abs_bits=0xCDCDCDCD,
            eff_level=0x55, path=0)


def keys_of(x):
    return np.ascontiguousarray(x, np.float32).view(U32) & U32(0x7FFFFFFF)


def run_select(lib, x, r0, above, gamma, kl, kh, flags=SEG_MASK, nl=6, cap=8192, overflow=0, publish=1, hs=0, pw=0):
    x = np.ascontiguousarray(x, np.float32)
    ret, path = np.zeros(1, np.float32), np.zeros(1, np.int32)
    ri = i64([REC0["numel"], REC0["zero_count"], REC0["coeff_numel"]])
    rd = np.array([REC0["thr64"]], np.float64)
    ru = u32([REC0["thr32_bits"], REC0["max_abs_bits"], REC0["eff_level"], REC0["path"]])
    tw = np.array([-3.25], np.float32)
    rc = lib.sc_select_body(S.ptr(x), len(x), r0, above, gamma, flags, nl, cap, kl, kh, overflow, publish, hs, pw,
                            S.ptr(ret), S.ptr(path), S.ptr(ri), S.ptr(rd), S.ptr(ru), S.ptr(tw))
    assert rc == 0, rc
    return dict(ret=ret[0], ret_path=int(path[0]), numel=int(ri[0]), zero_count=int(ri[1]), coeff_numel=int(ri[2]),
                thr64=rd[0], thr32_bits=int(ru[0]), max_abs_bits=int(ru[1]), eff_level=int(ru[2]), path=int(ru[3]),
                thr_word=tw[0])


def np_lerp(ka, kb, g):
    """numpy/lib/function_base.py _lerp of NumPy 1.x on float32 order statistics: the difference
    in float32, the blend in float64"""
    fa, fb = f32_from_bits(ka), f32_from_bits(kb)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.float32(fb - fa)
        return np.float64(fb) - np.float64(diff) * (1.0 - g) if g >= 0.5 else np.float64(fa) + np.float64(diff) * g


def want_record(x, r0, above, gamma, pct=None, minprune=False):
    """(thr64, thr32, zero_count, max key): from the oracle when the ranks come from a percentile,
    from np_lerp on the sorted keys otherwise; NaN thresholds count no zeros in the select"""
    keys = keys_of(x)
    srt = np.sort(keys)
    ka, kb = int(srt[r0]), int(srt[r0 if above else r0 + 1])
    if minprune:
        return None, f32_from_bits(ka), (int((keys < ka).sum()) if ka > 0 else 0), int(srt[-1])
    if pct is not None:
        assert np_ranks(len(x), pct) == (r0, above, gamma)
        _, d = O.prune_tensor(x, "haar", 0, pct)
        thr64, thr32 = np.float64(d["thr64"]), np.float32(d["thr32"])
        zc = 0 if math.isnan(thr64) else d["zero_count"]
        assert_same_bits(thr64, np.where(srt[-1] > 0x7F800000, np.float64("nan"), np_lerp(ka, kb, gamma)), "np_lerp")
    else:
        thr64 = np.float64("nan") if srt[-1] > 0x7F800000 else np.float64(np_lerp(ka, kb, gamma))
        with np.errstate(over="ignore"):
            thr32 = np.float32(thr64)
        tk = int(thr32.view(U32)) if thr32 > 0 else 1
        zc = 0 if math.isnan(thr32) else int((keys < tk).sum())
    return thr64, thr32, zc, int(srt[-1])


def check_select(lib, edges, x, rk, kl, kh, path, pct=None, shifted=True, **kw):
    """select_body on x's host-built state at window (kl, kh]: the returned float, the returned
    path and the whole record; then, for CAND / WINDOW, the same at the window moved one bin down and
    one bin up where the ranks' keys stay inside it -- the result must not move."""
    r0, above, gamma = rk
    minp = bool(kw.get("flags", SEG_MASK) & SEG_MINPRUNE)
    thr64, thr32, zc, mk = want_record(x, r0, above, gamma, pct, minp)
    g = run_select(lib, x, r0, above, gamma, kl, kh, **kw)
    assert g["ret_path"] == path and g["path"] == path, (g["ret_path"], g["path"], path)
    assert_same_bits(np.float32(g["ret"]), np.float32(thr32), "returned threshold")
    if not minp:
        assert_same_bits(np.float64(g["thr64"]), np.float64(thr64), "thr64")
        assert_same_bits(f32_from_bits(g["thr32_bits"]), np.float32(thr32), "thr32")
    assert_same_bits(np.float32(g["thr_word"]), f32_from_bits(g["thr32_bits"]), "threshold word")
    assert g["zero_count"] == zc, (g["zero_count"], zc)
    assert (g["numel"], g["coeff_numel"], g["max_abs_bits"], g["eff_level"]) == (len(x), len(x), mk, 0)
    if not shifted or path == FULL:
        return g
    lo, hi = edges
    srt = np.sort(keys_of(x))
    ka, kb = int(srt[r0]), int(srt[r0 if above else r0 + 1])
    b0 = int(np_key_bin(u32([kl]))[0])
    b1 = int(np_key_bin(u32([kh - 1]))[0]) if kh != OPEN else NB - 1
    assert kl == int(lo[b0]) and kh == int(hi[b1]), "windows are made of bin edges"
    for d in (-1, 1):
        if not (0 <= b0 + d and b1 + d <= NB - 1):
            continue
        kl2, kh2 = int(lo[b0 + d]), int(hi[b1 + d])
        if not (kl2 <= ka and kb <= kh2):
            continue
        g2 = run_select(lib, x, r0, above, gamma, kl2, kh2, **kw)
        assert g2["ret_path"] in (CAND, WINDOW), (d, g2["ret_path"])
        for f in ("ret", "thr64", "thr32_bits", "zero_count", "max_abs_bits", "thr_word"):
            assert np.atleast_1d(g2[f]).tobytes() == np.atleast_1d(g[f]).tobytes(), (d, f, g2[f], g[f])
    return g


class Pop:
    """A population around a window of whole bins: `below` keys under kl, `eq` keys == kl, inside
    keys per bucket, `above` keys over kh; nsub_log2 = 6.  wide: 64 bins, one bin (65536 key
    values) per bucket; narrow: one bin, 1024 key values per bucket (within block_hist_select's
    HS_PER * THREADS values)."""

    def __init__(self, edges, wide=True, seed=0):
        lo, hi = edges
        self.b0 = int(np_key_bin(u32([0x3D000000]))[0])
        self.kl, self.kh = int(lo[self.b0]), int(hi[self.b0 + (63 if wide else 0)])
        self.sh = 16 if wide else 10
        assert (self.kh - self.kl - 1).bit_length() - 6 == self.sh
        self.rng = np.random.default_rng(seed)

    def build(self, below, eq, buckets, above=0, zeros=0, extra=()):
        rng, parts = self.rng, []
        parts.append(np.zeros(zeros, np.int64))
        parts.append(rng.integers(1, self.kl, below - zeros))
        parts.append(np.full(eq, self.kl))
        self.first = {}
        at = below + eq
        for b in sorted(buckets):
            lo_b = self.kl + 1 + (b << self.sh)
            hi_b = min(self.kh, self.kl + ((b + 1) << self.sh))
            k = rng.integers(lo_b, hi_b + 1, buckets[b])
            if buckets[b] > 1:
                k[0], k[1] = lo_b, hi_b
            parts.append(k)
            self.first[b] = at
            at += buckets[b]
        self.first_above = at
        parts.append(rng.integers(self.kh + 1, 0x7F000000, above))
        parts.append(np.asarray(extra, np.int64))
        keys = u32(np.concatenate(parts))
        rng.shuffle(keys)
        keys |= (rng.integers(0, 2, len(keys)).astype(U32) << U32(31))  # random signs
        return keys.view(np.float32)


def pct_for(n, r0, frac=0.37):
    """a percentile whose lower order statistic is r0, and its np_ranks"""
    pct = (r0 + frac) / (n - 1) * 100.0
    rk = np_ranks(n, pct)
    assert rk[0] == r0 and rk[1] == 0
    return pct, rk


def test_select_a_both_ranks_in_one_bucket_wave_select(lib, edges):
    P = Pop(edges, seed=1)
    x = P.build(700, 3, {2: 40, 5: 300, 9: 60}, above=500)
    pct, rk = pct_for(len(x), P.first[5] + 100)
    check_select(lib, edges, x, rk, P.kl, P.kh, CAND, pct)


@pytest.mark.parametrize("gap", ["adjacent_buckets", "empty_buckets_between"])
def test_select_b_ranks_in_two_buckets(lib, edges, gap):
    P = Pop(edges, seed=2)
    nxt = 6 if gap == "adjacent_buckets" else 10
    x = P.build(700, 3, {2: 40, 5: 300, nxt: 200}, above=500)
    pct, rk = pct_for(len(x), P.first[nxt] - 1)
    check_select(lib, edges, x, rk, P.kl, P.kh, CAND, pct)


@pytest.mark.parametrize("staged", [1025, 4096])
def test_select_c_select_in_range_over_lds(lib, edges, staged):
    P = Pop(edges, seed=3)
    x = P.build(700, 3, {2: 40, 5: staged, 9: 60}, above=500)
    pct, rk = pct_for(len(x), P.first[5] + staged // 3)
    check_select(lib, edges, x, rk, P.kl, P.kh, CAND, pct)


@pytest.mark.parametrize("staged", [4097, 8192])
def test_select_d_select_in_range_over_global_buckets(lib, edges, staged):
    P = Pop(edges, seed=4)
    x = P.build(700, 3, {2: 40, 5: staged, 9: 60}, above=500)
    pct, rk = pct_for(len(x), P.first[5] + staged // 3)
    check_select(lib, edges, x, rk, P.kl, P.kh, CAND, pct)


def test_select_d_two_buckets_over_stage_cap(lib, edges):
    P = Pop(edges, seed=4)
    x = P.build(700, 3, {5: 3000, 6: 2500}, above=500)
    pct, rk = pct_for(len(x), P.first[6] - 1)
    check_select(lib, edges, x, rk, P.kl, P.kh, CAND, pct)


@pytest.mark.parametrize("which", ["lower_ranks_bucket", "upper_ranks_bucket"])
def test_select_e_bucket_over_capacity_full_scan(lib, edges, which):
    P = Pop(edges, seed=5)
    x = P.build(700, 3, {5: 300 if which == "lower_ranks_bucket" else 50, 6: 50 if which == "lower_ranks_bucket" else 300},
                above=500)
    pct, rk = pct_for(len(x), P.first[6] - 1)
    check_select(lib, edges, x, rk, P.kl, P.kh, FULL, pct, cap=100)


def test_select_f_overflow_flag_full_scan(lib, edges):
    P = Pop(edges, seed=6)
    x = P.build(700, 3, {5: 300}, above=500)
    pct, rk = pct_for(len(x), P.first[5] + 100)
    check_select(lib, edges, x, rk, P.kl, P.kh, FULL, pct, overflow=1)


def test_select_g_both_ranks_tie_at_kl_window(lib, edges):
    P = Pop(edges, seed=7)
    x = P.build(700, 50, {5: 300}, above=500)
    pct, rk = pct_for(len(x), 700 + 20)
    check_select(lib, edges, x, rk, P.kl, P.kh, WINDOW, pct)


def test_select_g_last_tie_at_kl_and_first_inside_key(lib, edges):
    P = Pop(edges, seed=8)
    x = P.build(700, 50, {5: 300}, above=500)
    pct, rk = pct_for(len(x), 700 + 49)
    check_select(lib, edges, x, rk, P.kl, P.kh, CAND, pct)


def test_select_g_last_tie_at_kl_gamma_0_threshold_is_kl(lib, edges):
    """class 1 with class 2 at gamma 0: the threshold is kl itself, so the keys == kl are not below
    it and the candidate path's zero count leaves them out (tk > kl ? eq_lo : 0)"""
    P = Pop(edges, seed=8)
    x = P.build(700, 50, {5: 300}, above=500)
    g = check_select(lib, edges, x, (700 + 49, 0, 0.0), P.kl, P.kh, CAND)
    assert g["thr32_bits"] == P.kl and g["zero_count"] == 700


@pytest.mark.parametrize("where", ["rank_below_kl", "upper_rank_above_kh", "both_above_kh"])
def test_select_h_rank_outside_the_window_full_scan(lib, edges, where):
    P = Pop(edges, seed=9)
    x = P.build(700, 3, {5: 300}, above=500)
    r0 = {"rank_below_kl": 699, "upper_rank_above_kh": P.first_above - 1, "both_above_kh": P.first_above + 7}[where]
    pct, rk = pct_for(len(x), r0)
    check_select(lib, edges, x, rk, P.kl, P.kh, FULL, pct)


@pytest.mark.parametrize("pctile", [10.0, 61.8])
def test_select_i_kl_0_with_zeros_kh_open(lib, edges, pctile):
    """the fully open window: exact zeros are the keys == kl; 10 % lands among them (threshold 0)"""
    rng = np.random.default_rng(10)
    x = (rng.standard_normal(3000) * 0.05).astype(np.float32)
    x[rng.choice(3000, 400, replace=False)] = 0.0
    x[5] = -0.0
    rk = np_ranks(len(x), pctile)
    check_select(lib, edges, x, rk, 0, OPEN, WINDOW if pctile == 10.0 else CAND, pctile)


def test_select_j_above_both_ranks_are_the_maximum(lib, edges):
    P = Pop(edges, seed=11)
    x = P.build(700, 3, {5: 300, 63: 20})
    rk = np_ranks(len(x), 100.0)
    assert rk[:2] == (len(x) - 1, 1)
    check_select(lib, edges, x, rk, P.kl, P.kh, CAND, 100.0)


GAMMAS = {"0": 0.0, "below_half": math.nextafter(0.5, 0.0), "half": 0.5, "above_half": math.nextafter(0.5, 1.0),
          "1_minus_2p-52": 1.0 - 2.0 ** -52}


@pytest.mark.parametrize("gname", list(GAMMAS))
@pytest.mark.parametrize("apart", ["ka_eq_kb", "1_ulp", "2p40_double_ulps"])
def test_select_k_lerp_gamma_by_key_distance(lib, edges, apart, gname):
    """ka and kb equal, one float32 ulp apart, and 2^40 ulps of the float64 blend (2^11 float32
    ulps) apart; the reference is NumPy 1.x's _lerp restated (np_lerp), gamma given directly"""
    P = Pop(edges, seed=12)
    lo_b = P.kl + 1 + (5 << P.sh)
    d = {"ka_eq_kb": 0, "1_ulp": 1, "2p40_double_ulps": 1 << 11}[apart]
    # bucket 5 holds 100 keys at its low end, then ka, kb, then 100 keys above them
    low = P.rng.integers(lo_b, lo_b + 1000, 100)
    high = P.rng.integers(lo_b + 20000, lo_b + 30000, 100)
    x = P.build(700, 3, {}, above=500, extra=np.concatenate([low, [lo_b + 5000, lo_b + 5000 + d], high]))
    r0 = 703 + 100
    srt = np.sort(keys_of(x))
    assert (int(srt[r0]), int(srt[r0 + 1])) == (lo_b + 5000, lo_b + 5000 + d)
    check_select(lib, edges, x, (r0, 0, GAMMAS[gname]), P.kl, P.kh, CAND)


def test_select_l_nan_in_the_population(lib, edges):
    """maxkey above inf's key: the threshold is NaN and the select counts no zeros"""
    P = Pop(edges, seed=13)
    x = P.build(700, 3, {5: 300}, above=500, extra=[0x7FC00000])
    pct, rk = pct_for(len(x), P.first[5] + 100)
    g = check_select(lib, edges, x, rk, P.kl, P.kh, CAND, pct)
    assert math.isnan(g["ret"]) and math.isnan(g["thr64"]) and g["zero_count"] == 0


@pytest.mark.parametrize("gname", ["0", "below_half", "half", "1_minus_2p-52"])
def test_select_l_inf_as_kb(lib, edges, gname):
    """+inf as the upper order statistic: gamma 0 and gamma in (0, 0.5) give fa + inf * g (NaN at
    0, inf above), gamma >= 0.5 gives inf - inf = NaN; NaN compares as NaN"""
    rng = np.random.default_rng(14)
    x = (rng.standard_normal(2000) * 0.05).astype(np.float32)
    x[17] = -np.inf
    g = check_select(lib, edges, x, (len(x) - 2, 0, GAMMAS[gname]), 0, OPEN, CAND)
    assert math.isinf(g["ret"]) if gname == "below_half" else math.isnan(g["ret"])


def test_select_m_threshold_exactly_zero_counts_only_zeros(lib, edges):
    P = Pop(edges, seed=15)
    x = P.build(700, 3, {5: 300}, above=500, zeros=300)
    pct, rk = pct_for(len(x), 150)
    g = check_select(lib, edges, x, rk, 0, P.kh, WINDOW, pct, shifted=False)
    assert g["ret"] == 0.0 and g["zero_count"] == 300


@pytest.mark.parametrize("case", ["cand", "window", "full"])
def test_select_n_publish_false_same_value_record_untouched(lib, edges, case):
    P = Pop(edges, seed=16)
    x = P.build(700, 50, {5: 300}, above=500)
    r0 = {"cand": P.first[5] + 100, "window": 720, "full": 10}[case]
    pct, rk = pct_for(len(x), r0)
    g = check_select(lib, edges, x, rk, P.kl, P.kh, {"cand": CAND, "window": WINDOW, "full": FULL}[case], pct,
                     shifted=False)
    q = run_select(lib, x, rk[0], rk[1], rk[2], P.kl, P.kh, publish=0)
    assert_same_bits(np.float32(q["ret"]), np.float32(g["ret"]))
    assert q["ret_path"] == g["ret_path"]
    assert {k: q[k] for k in REC0} == REC0 and q["thr_word"] == np.float32(-3.25)


@pytest.mark.parametrize("case", ["cand", "cand_with_nan", "cand_ka_is_last_tie_at_kl", "window_ka_is_kl", "full",
                                  "ka_zero"])
def test_select_o_minprune_returns_ka_and_counts_below_it(lib, edges, case):
    """SEG_MINPRUNE: the return value is the r0-th key itself, zero_count = #(key < ka) (none when
    ka = 0), and no NaN rule applies"""
    P = Pop(edges, seed=17)
    x = P.build(700, 50, {5: 300}, above=500, zeros=40, extra=[0x7FC00000] if case == "cand_with_nan" else ())
    r0 = {"cand": P.first[5] + 100, "cand_with_nan": P.first[5] + 100, "cand_ka_is_last_tie_at_kl": 749,
          "window_ka_is_kl": 720, "full": 100, "ka_zero": 10}[case]
    path = {"cand": CAND, "cand_with_nan": CAND, "cand_ka_is_last_tie_at_kl": CAND, "window_ka_is_kl": WINDOW,
            "full": FULL, "ka_zero": FULL}[case]
    g = check_select(lib, edges, x, (r0, 0, 0.0), P.kl, P.kh, path, flags=SEG_MINPRUNE, shifted=case != "ka_zero")
    assert g["ret"].view(U32) == np.sort(keys_of(x))[r0]


@pytest.mark.parametrize("hs,pw", [(1, 0), (1, 1), (0, 1)], ids=["hscratch", "hscratch_prefer_wave", "prefer_wave"])
@pytest.mark.parametrize("staged", [300, 2000], ids=["case_a_300_keys", "case_c_2000_keys"])
def test_select_p_hscratch_and_prefer_wave(lib, edges, staged, hs, pw):
    """the arguments no caller passes today: a bucket 1024 key values wide goes through
    block_hist_select when hscratch is given (unless prefer_wave and at most 1024 keys)"""
    P = Pop(edges, wide=False, seed=18)
    x = P.build(700, 3, {2: 40, 5: staged, 9: 60}, above=500)
    pct, rk = pct_for(len(x), P.first[5] + staged // 3)
    check_select(lib, edges, x, rk, P.kl, P.kh, CAND, pct, hs=hs, pw=pw)
    pct, rk = pct_for(len(x), P.first[9] - 1)  # two buckets
    check_select(lib, edges, x, rk, P.kl, P.kh, CAND, pct, hs=hs, pw=pw)


# =================================================================== collect_body, one chunk
def run_collect(lib, x, off, length, full, kl, kh, nl, cap):
    nsub = 1 << nl
    sums, sub, cand = np.zeros(5, np.int64), np.zeros(nsub, U32), np.zeros(nsub * cap, U32)
    xx = np.ascontiguousarray(x[:off + length], np.float32)
    assert lib.sc_collect_body(S.ptr(xx), off, length, full, kl, kh, nl, cap, S.ptr(sums), S.ptr(sub), S.ptr(cand)) == 0
    return sums, sub, cand.reshape(nsub, cap)


def host_state(lib, x, kl, kh, nl, cap):
    nsub = 1 << nl
    sums, sub, cand = np.zeros(5, np.int64), np.zeros(nsub, U32), np.zeros(nsub * cap, U32)
    xx = np.ascontiguousarray(x, np.float32)
    assert lib.sc_build_state(S.ptr(xx), len(xx), kl, kh, nl, cap, S.ptr(sums), S.ptr(sub), S.ptr(cand)) == 0
    return sums, sub, cand.reshape(nsub, cap)


def collect_data(seed, n=16385):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 0.05).astype(np.float32)
    x[rng.choice(n, 200, replace=False)] = 0.0
    return x


def collect_window(x, edges, qlo=0.58, qhi=0.66):
    lo, hi = edges
    srt = np.sort(keys_of(x))
    b0, b1 = int(np_key_bin(srt[int(qlo * len(x))])), int(np_key_bin(srt[int(qhi * len(x))]))
    return int(lo[b0]), int(hi[b1])


def compare_collect(dev, host, x, kl, kh, cap):
    (ds, dsub, dc), (hs, hsub, hc) = dev, host
    assert list(ds) == list(hs), (ds, hs)  # below, eq_lo, maxkey, overflow, shift
    assert np.array_equal(dsub, hsub)
    keys = keys_of(x).astype(np.int64)
    inside = keys[(keys > kl) & (keys <= kh)]
    b = (inside - kl - 1) >> int(hs[4])
    for j in np.nonzero(hsub)[0]:
        stored = int(min(hsub[j], cap))
        if hsub[j] <= cap:
            assert np.array_equal(np.sort(dc[j, :stored]), np.sort(hc[j, :stored])), j
        else:  # counted beyond capacity, stored up to it: any `cap` of the bucket's keys
            pool = np.sort(inside[b == j])
            got = np.sort(dc[j, :stored].astype(np.int64))
            uv, uc = np.unique(got, return_counts=True)
            pv, pc = np.unique(pool, return_counts=True)
            assert np.all(np.isin(uv, pv)) and np.all(uc <= pc[np.searchsorted(pv, uv)]), j


@pytest.mark.parametrize("nl", [6, 10])
def test_collect_full_chunk(lib, edges, nl):
    x = collect_data(21)[:16384]
    kl, kh = collect_window(x, edges)
    compare_collect(run_collect(lib, x, 0, 16384, 1, kl, kh, nl, 4096), host_state(lib, x, kl, kh, nl, 4096), x, kl, kh, 4096)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset_one_float"])
@pytest.mark.parametrize("length", [1, 4095, 16383])
def test_collect_ragged_chunk(lib, edges, length, off):
    x = collect_data(22)
    kl, kh = collect_window(x[off:off + length] if length > 100 else x, edges)
    part = x[off:off + length]
    compare_collect(run_collect(lib, x, off, length, 0, kl, kh, 6, 4096), host_state(lib, part, kl, kh, 6, 4096), part,
                    kl, kh, 4096)


def test_collect_ragged_whole_chunk_unaligned(lib, edges):
    x = collect_data(23, 16385)
    part = x[1:]
    kl, kh = collect_window(part, edges)
    compare_collect(run_collect(lib, x, 1, 16384, 0, kl, kh, 8, 4096), host_state(lib, part, kl, kh, 8, 4096), part, kl, kh,
                    4096)


@pytest.mark.parametrize("nl", [6, 10])
def test_collect_keys_on_bucket_boundaries(lib, edges, nl):
    """keys kl + (j << shift), the last key of bucket j - 1 (bucket = (key - kl - 1) >> shift), and
    kl + 1 + (j << shift), the first of bucket j: an off-by-one in the bucket index moves them"""
    x = collect_data(26)[:16384]
    kl, kh = collect_window(x, edges)
    sh = max(0, (kh - kl - 1).bit_length() - nl)
    js = np.arange(1, 9)
    x[100:108] = f32_from_bits(kl + (js << sh))
    x[9000:9008] = -f32_from_bits(kl + 1 + (js << sh))
    host = host_state(lib, x, kl, kh, nl, 4096)
    assert host[0][4] == sh and np.all(kl + 1 + (js << sh) <= kh)
    compare_collect(run_collect(lib, x, 0, 16384, 1, kl, kh, nl, 4096), host, x, kl, kh, 4096)


def test_collect_thread_over_STG_sets_overflow(lib, edges):
    """thread 3 holds 25 inside keys (its slots 4 (it 256 + 3) + c): the overflow flag is set and
    the counters stay exact; nothing else is required of the buckets"""
    x = collect_data(24)[:16384]
    kl, kh = collect_window(x, edges, 0.70, 0.72)
    keys = keys_of(x)
    inside = (keys > kl) & (keys <= kh)
    mine = np.array([4 * (it * 256 + 3) + c for it in range(16) for c in range(4)])
    assert S.const(lib, "STG") == 24 and inside.reshape(-1, 4).reshape(16, 256, 4).sum(axis=(0, 2)).max() <= 24
    x[mine[:25]] = f32_from_bits(np.full(25, kl + 1))
    ds, dsub, dc = run_collect(lib, x, 0, 16384, 1, kl, kh, 6, 4096)
    hs, _, _ = host_state(lib, x, kl, kh, 6, 4096)
    assert ds[3] == 1 and list(ds[:3]) == list(hs[:3]) and ds[4] == hs[4]


def test_collect_bucket_over_capacity_counted_not_stored(lib, edges):
    x = collect_data(25)[:16384]
    kl, kh = collect_window(x, edges)
    host = host_state(lib, x, kl, kh, 6, 16)
    assert host[1].max() > 16
    compare_collect(run_collect(lib, x, 0, 16384, 1, kl, kh, 6, 16), host, x, kl, kh, 16)


# ============================================= end to end: a rank's bucket of one key value
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "three_launch"])
def test_prune_ranks_in_a_bucket_of_one_key_value(resident):
    """The bug the lo == hi cases above found, through engine.prune: with lo == hi the selects
    shifted by -1 and returned 0 for the key.  The sample reads only zeros (every sampled position
    holds one), so the window is (0, 1] and its one bucket holds the single key value 1 (the smallest
    subnormal), where both ranks lie: the threshold is 2^-149, not 0.  The three-launch form takes the
    candidate path there (200 keys, under the smallest bucket capacity).  The resident form counts the
    keys == kl as inside keys, about 48 zeros in every thread's 96 weights against the 32 it may stage,
    so it always takes the full scan here and is the control."""
    import torch
    from wavelettransforms_amd import engine
    n, nz, n1 = 100000, 49900, 200  # n1 below the smallest bucket capacity (256)
    rng = np.random.default_rng(31)
    x = (rng.standard_normal(n) * 0.05).astype(np.float32)
    assert np.all(x != 0)
    starts = (np.arange(256) * (n - 16)) // 255  # the sample's groups of 16, one position of slack each side
    forced = np.unique(np.clip((starts[:, None] + np.arange(-1, 18)[None, :]).ravel(), 0, n - 1))
    rest = rng.permutation(np.setdiff1d(np.arange(n), forced))
    x[forced] = 0.0
    x[rest[:nz - len(forced)]] = 0.0
    x[rest[nz - len(forced):nz - len(forced) + n1]] = f32_from_bits(np.full(n1, 1))
    assert int((x == 0).sum()) == nz and nz <= (n - 1) // 2 < (n - 1) // 2 + 1 < nz + n1
    ref, rr = O.prune_tensor(x, "haar", 0, 50.0)
    assert rr["thr64"] == 2.0 ** -149 and rr["zero_count"] == nz
    prev = engine.set_resident(resident)
    try:
        outs, res = engine.prune([torch.from_numpy(x).cuda()], "haar", 0, 50.0, carry_level=False)
    finally:
        engine.set_resident(prev)
    r = res[0]
    assert_same_bits(np.float64(r["thr64"]), np.float64(rr["thr64"]), "thr64")
    assert r["zero_count"] == rr["zero_count"] and r["path"] == (FULL if resident else CAND), (r["zero_count"], r["path"])
    assert_same_bits(outs[0].cpu().numpy(), ref, "out")
