"""CPU check of the float16 path's arithmetic (csrc/wt_half_core.h: the 15-bit key, the 11 + 4 bit
histogram passes and their rank searches, NumPy's float16 percentile rule, the float16 compare and
the conversions that csrc/half.hip's kernels run, compiled for the host in
tests/native/halfcore.cpp) against the oracle's fixtures (tools/gen_golden_f16.py): thresholds bit
for bit, masks, zero counts, and both conversion routines against NumPy over every half and every
midpoint between neighbouring halves."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import half_ref as H
from tests import special_values as SV
from wavelettransforms_amd import workloads as W

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
SO = os.path.join(BUILD, "libhalfcore.so")
EXE = os.path.join(BUILD, "halfcore")
EXE_SAN = os.path.join(BUILD, "halfcore_san")
SRC = os.path.join(HERE, "native", "halfcore.cpp")
CSRC = os.path.join(HERE, "..", "wavelettransforms_amd", "csrc")
CXX = ["g++", "-std=c++17", "-ffp-contract=off"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def _build(target, extra):
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(CSRC, "wt_half_core.h"), os.path.join(CSRC, "wt_dwt_core.h")]
    if not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(CXX + extra + ["-o", target, SRC])
    return target


@pytest.fixture(scope="module")
def core():
    L = ctypes.CDLL(_build(SO, ["-O2", "-shared", "-fPIC"]))
    u16p, ll, dbl = ctypes.POINTER(ctypes.c_uint16), ctypes.c_longlong, ctypes.c_double
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.half_core_select.argtypes = [u16p, ll, ll, ctypes.c_int, u32p]
    L.half_core_prune.argtypes = [u16p, ll, ll, ctypes.c_int, dbl, u16p, ctypes.POINTER(dbl), u32p, u32p,
                                  ctypes.POINTER(ll)]
    L.half_core_from_double_n.argtypes = [ctypes.POINTER(dbl), ll, u16p]
    L.half_core_from_float_n.argtypes = [ctypes.POINTER(ctypes.c_float), ll, u16p]
    L.half_core_to_float_bits.argtypes = [ctypes.c_uint16]
    L.half_core_to_float_bits.restype = ctypes.c_uint32
    L.half_core_diff.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.half_core_diff.restype = ctypes.c_uint16
    L.half_core_split.argtypes = [ctypes.c_ulonglong, ll] + [ctypes.POINTER(ll)] * 3
    return L


def _u16(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))


def prune(core, words, pct):
    """(out words, thr64, compare key, max key, zero count) of one kind-B population"""
    words = np.ascontiguousarray(words, np.uint16).reshape(-1)
    n = len(words)
    r0, above, gamma = H.np_ranks(n, pct)
    out = np.zeros(n, np.uint16)
    thr, ck, mk, z = ctypes.c_double(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_longlong()
    assert core.half_core_prune(_u16(words), n, r0, above, gamma, _u16(out), ctypes.byref(thr), ctypes.byref(ck),
                                ctypes.byref(mk), ctypes.byref(z)) == 0
    return out, thr.value, ck.value, mk.value, z.value


def f32_bits_of_half_word(w):
    return int(np.array(w, np.uint16).view(np.float16).astype(np.float32).view(np.uint32))


def kind_b_records():
    """(call key, tensor index, call, record) of every kind-B tensor of the fixture calls"""
    for key, call in sorted(H.manifest()["calls"].items()):
        for ti, rec in enumerate(call["tensors"]):
            if rec["kind"] == "B":
                yield key, ti, call, rec


def test_program_self_check():
    """The stand-alone program without input: every half through float32 and float64 and back, 60
    random populations against std::sort."""
    out = subprocess.run([_build(EXE, ["-O2"])], input="", capture_output=True, text=True)
    assert out.returncode == 0 and "halfcore: ok" in out.stdout, out.stdout + out.stderr


def _program_lines(exe):
    """the wide group through the program's stdin: thresholds, compare keys, outputs"""
    wide = H.manifest()["wide"]
    words = H.arrays()["wide/words"]
    lines = []
    for c in wide:
        x = words[c["offset"]:c["offset"] + c["n"]]
        r0, above, gamma = H.np_ranks(c["n"], c["pct"])
        lines.append("%d %d %d %s %s" % (c["n"], r0, above, float(gamma).hex(), " ".join(str(int(v)) for v in x)))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
    got = out.stdout.strip().split("\n")
    assert len(got) == len(wide)
    for c, line in zip(wide, got):
        f = line.split()
        want_out = words[c["offset"] + c["n"]:c["offset"] + 2 * c["n"]]
        assert float.fromhex(f[0]).hex() == c["thr64_hex"], (c, f[0])
        assert f32_bits_of_half_word(int(f[1])) == c["cmp_bits"]
        assert f32_bits_of_half_word(int(f[2])) == c["max_bits"]
        assert int(f[3]) == c["zero_count"]
        assert [int(v) for v in f[4:]] == [int(v) for v in want_out]


def test_program_reads_cases_and_writes_results():
    _program_lines(_build(EXE, ["-O2"]))


def test_program_under_asan_ubsan():
    """The same stand-alone program built with the address and undefined-behaviour sanitizers: its
    self check and the wide group.  Nothing is preloaded; the program is its own process."""
    exe = _build(EXE_SAN, SAN)
    out = subprocess.run([exe], input="", capture_output=True, text=True)
    assert out.returncode == 0 and "halfcore: ok" in out.stdout, out.stdout + out.stderr[-2000:]
    _program_lines(exe)


def test_fixture_calls_kind_b(core):
    """Every kind-B tensor of the fixture calls: thr64 bit for bit, the compare value, the maximum,
    the zero count and the output words (stored, or their hash)."""
    n = 0
    for key, ti, call, rec in kind_b_records():
        x = H.make_input(rec, W.synth_numpy)
        out, thr, ck, mk, z = prune(core, x.view(np.uint16), call["pct"])
        assert float(thr).hex() == rec["thr64_hex"], (key, ti)
        assert f32_bits_of_half_word(ck) == rec["cmp_bits"], (key, ti)
        assert f32_bits_of_half_word(mk) == rec["max_bits"], (key, ti)
        assert z == rec["zero_count"], (key, ti)
        assert H.words_hash(out.view(np.float16)) == rec["out_hash"], (key, ti)
        stored = H.arrays().get("%s/%d" % (key, ti))
        if stored is not None:
            assert np.array_equal(stored.view(np.uint16).reshape(-1), out), (key, ti)
        n += 1
    assert n >= 40


def test_wide_group_and_the_rules_it_rules_out(core):
    """The wide group bit for bit; its flags mark where the exact difference b - a or a float32
    compare gives another answer than NumPy (recomputed here), often enough to catch either."""
    wide = H.manifest()["wide"]
    words = H.arrays()["wide/words"]
    n_exact = n_f32 = 0
    for c in wide:
        x = words[c["offset"]:c["offset"] + c["n"]]
        want = words[c["offset"] + c["n"]:c["offset"] + 2 * c["n"]]
        out, thr, ck, mk, z = prune(core, x, c["pct"])
        assert float(thr).hex() == c["thr64_hex"], c
        assert f32_bits_of_half_word(ck) == c["cmp_bits"] and f32_bits_of_half_word(mk) == c["max_bits"]
        assert np.array_equal(out, want) and z == c["zero_count"]
        # the two rules the fixtures rule out
        a = np.abs(x.view(np.float16))
        s = np.sort(a).astype(np.float64)
        lo, above, g = H.np_ranks(c["n"], c["pct"])
        if above:
            exact = s[-1]
        else:
            d = s[lo + 1] - s[lo]
            exact = s[lo + 1] - d * (1 - g) if g >= 0.5 else s[lo] + d * g
        differs_exact = float(exact).hex() != c["thr64_hex"]
        mask32 = a.astype(np.float32) < np.float32(float.fromhex(c["thr64_hex"]))
        differs_f32 = not np.array_equal(np.where(mask32, np.uint16(0), x), want)
        assert differs_exact == c["differs_exact_diff"] and differs_f32 == c["differs_f32_compare"], c
        n_exact += differs_exact
        n_f32 += differs_f32
    assert n_exact >= 20 and n_f32 >= 5, (n_exact, n_f32)


def test_half_from_double_every_half_and_midpoint(core):
    """h16_from_double against NumPy's float64 -> float16 (round to nearest even, once): all 65 536
    halves, the midpoints between neighbouring finite halves and their float64 neighbours, the
    overflow threshold, float64 subnormals and tiny values."""
    allw = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    vals = allw.view(np.float16).astype(np.float64)
    finite = np.isfinite(vals)
    pos = np.sort(vals[finite & (vals >= 0)])
    mid = (pos[:-1] + pos[1:]) / 2  # exact in float64
    pts = np.concatenate([vals[finite], mid, -mid, np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf),
                          [65504.0, 65519.99, 65520.0, 65520.01, 1e6, -1e6, np.inf, -np.inf, 5e-324, -5e-324, 1e-310,
                           2.0 ** -25, np.nextafter(2.0 ** -25, 1), np.nextafter(2.0 ** -25, 0), -2.0 ** -25,
                           3 * 2.0 ** -25, 0.0, -0.0]])
    got = np.zeros(len(pts), np.uint16)
    core.half_core_from_double_n(pts.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(pts), _u16(got))
    with np.errstate(over="ignore"):
        want = pts.astype(np.float16).view(np.uint16)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    nan = np.array([np.nan], np.float64)
    one = np.zeros(1, np.uint16)
    core.half_core_from_double_n(nan.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1, _u16(one))
    assert (int(one[0]) & 0x7FFF) > 0x7C00


def test_half_from_float_and_widening(core):
    """h16_from_float against NumPy's float32 -> float16 on every half, every float32 midpoint
    between halves and 200 000 random float32 bit patterns; h16_to_float_bits against NumPy."""
    allw = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    f = allw.view(np.float16).astype(np.float32)
    for w in (0, 1, 0x3FF, 0x400, 0x3C00, 0x7BFF, 0x7C00, 0x8001, 0xFBFF, 0xFC00):
        assert core.half_core_to_float_bits(w) == int(f[w].view(np.uint32))
    assert all(core.half_core_to_float_bits(int(w)) == int(f[w].view(np.uint32)) for w in range(0, 65536, 7)
               if np.isfinite(f[w]))
    pos = np.sort(f[np.isfinite(f) & (f >= 0)].astype(np.float64))
    mid = ((pos[:-1] + pos[1:]) / 2).astype(np.float32)  # 11 + 1 significant bits: exact in float32
    rng = np.random.default_rng(3)
    rnd = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    rnd = rnd[np.isfinite(rnd)]
    pts = np.ascontiguousarray(np.concatenate([f[np.isfinite(f)], mid, -mid, np.nextafter(mid, np.float32(np.inf)),
                                               np.nextafter(mid, np.float32(-np.inf)), rnd]), np.float32)
    got = np.zeros(len(pts), np.uint16)
    core.half_core_from_float_n(pts.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(pts), _u16(got))
    with np.errstate(over="ignore"):
        want = pts.astype(np.float16).view(np.uint16)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


def test_half_difference_is_one_rounding_of_the_float32_difference(core):
    rng = np.random.default_rng(4)
    keys = rng.integers(0, 0x7C00, (20000, 2)).astype(np.uint16)
    keys.sort(axis=1)
    a, b = keys[:, 0].view(np.float16), keys[:, 1].view(np.float16)
    want = (b - a).view(np.uint16)  # NumPy's half subtraction
    got = np.array([core.half_core_diff(int(x), int(y)) for x, y in keys[:4000]], np.uint16)
    assert np.array_equal(got, want[:4000])


def test_selection_over_digit_boundaries(core):
    """ranks lo and lo + 1 on opposite sides of a top-digit boundary (keys ...F | ...0), inside one
    top digit, and all in one key"""
    for edge in (0x2C10, 0x0010, 0x7BF0):
        keys = np.concatenate([np.full(501, edge - 1), np.full(500, edge)]).astype(np.uint16)
        np.random.default_rng(9).shuffle(keys)
        words = keys | (np.arange(len(keys), dtype=np.uint16) % 2 << 15).astype(np.uint16)
        k = (ctypes.c_uint32 * 3)()
        assert core.half_core_select(_u16(np.ascontiguousarray(words)), len(words), 500, 0, k) == 0
        assert list(k) == [edge - 1, edge, edge]
    one = np.full(4097, 0x1234, np.uint16)
    k = (ctypes.c_uint32 * 3)()
    assert core.half_core_select(_u16(one), len(one), 4096, 1, k) == 0 and list(k) == [0x1234] * 3


def test_split_of_an_unaligned_tensor(core):
    """head words up to the 16-byte boundary, whole vectors, tail: they tile [0, n) for every phase
    of a 2-byte aligned address and every short length"""
    ll = ctypes.c_longlong
    for addr in range(0x1000, 0x1010, 2):
        for n in list(range(0, 40)) + [41145, 16384 * 3 + 5]:
            h, v, t = ll(), ll(), ll()
            core.half_core_split(addr, n, ctypes.byref(h), ctypes.byref(v), ctypes.byref(t))
            assert 0 <= h.value <= min(n, 7) and v.value >= 0
            assert t.value == h.value + 8 * v.value and 0 <= n - t.value < 8
            if v.value:
                assert (addr + 2 * h.value) % 16 == 0
            if h.value < n and h.value:
                assert (addr + 2 * h.value) % 16 == 0


# ---- the rule restated in NumPy scalars (half_ref.kind_b_ref), and special values ----

def _half_word(w):
    return np.array(w, np.uint16).view(np.float16)


def test_restated_rule_reproduces_every_stored_kind_b_result():
    """half_ref.kind_b_ref against the NumPy 1.26.4 run that made the fixtures: thr64, the compare
    value, the maximum, the zero count and the output words (stored, or their hash) of every
    kind-B tensor of the fixture calls and of the whole wide group."""
    n = 0
    for key, ti, call, rec in kind_b_records():
        x = H.make_input(rec, W.synth_numpy)
        ref = H.kind_b_ref(x.view(np.uint16), call["pct"])
        assert float(ref["thr64"]).hex() == rec["thr64_hex"], (key, ti)
        assert int(ref["cmp"].astype(np.float32).view(np.uint32)) == rec["cmp_bits"], (key, ti)
        assert int(ref["max"].astype(np.float32).view(np.uint32)) == rec["max_bits"], (key, ti)
        assert ref["zero_count"] == rec["zero_count"], (key, ti)
        assert H.words_hash(ref["out"].view(np.float16)) == rec["out_hash"], (key, ti)
        stored = H.arrays().get("%s/%d" % (key, ti))
        if stored is not None:
            assert np.array_equal(stored.view(np.uint16).reshape(-1), ref["out"]), (key, ti)
        n += 1
    assert n == 51
    wide = H.manifest()["wide"]
    words = H.arrays()["wide/words"]
    assert len(wide) == 156
    for c in wide:
        ref = H.kind_b_ref(words[c["offset"]:c["offset"] + c["n"]], c["pct"])
        assert float(ref["thr64"]).hex() == c["thr64_hex"], c
        assert int(ref["cmp"].astype(np.float32).view(np.uint32)) == c["cmp_bits"], c
        assert int(ref["max"].astype(np.float32).view(np.uint32)) == c["max_bits"], c
        assert ref["zero_count"] == c["zero_count"], c
        assert np.array_equal(ref["out"], words[c["offset"] + c["n"]:c["offset"] + 2 * c["n"]]), c


@pytest.fixture(scope="module")
def special():
    """[(name, pct, words, reference)] of half_ref.special_populations at half_ref.SPECIAL_PCTS"""
    return [(name, pct, w, H.kind_b_ref(w, pct)) for name, w in H.special_populations() for pct in H.SPECIAL_PCTS]


def test_special_populations_are_what_they_are_named(special):
    """On the reference alone: a NaN leaves the tensor as it is, infs above the ranks leave a finite
    threshold that prunes some and not all, an inf at rank lo + 1 over a finite rank lo gives NaN
    at gamma 0, inf below one half and NaN from one half on, and -0.0 and subnormals are there."""
    branches = {"zero": 0, "below_half": 0, "from_half": 0}
    n_nan = n_above = n_both = n_top_inf = 0
    for name, pct, w, ref in special:
        n = len(w)
        keys = np.sort(w & np.uint16(0x7FFF))
        lo, above, g = H.np_ranks(n, pct)
        tag = (name, pct)
        if keys[-1] >= H.NAN_KEY_MIN:
            assert np.isnan(ref["thr64"]) and np.isnan(ref["cmp"]) and np.isnan(ref["max"]), tag
            assert np.array_equal(ref["out"], w), tag
            n_nan += 1
            continue
        assert not np.isnan(ref["max"]), tag
        if name.startswith("inf_above") and 0 < pct < 100:
            assert not above and keys[lo + 1] < H.INF == keys[-1], tag
            assert np.isfinite(ref["thr64"]), tag
            pruned = int((ref["out"] != w).sum())
            assert 0 < pruned < n, tag
            assert np.array_equal(ref["out"][(w & 0x7FFF) == H.INF], w[(w & 0x7FFF) == H.INF]), tag
            n_above += 1
        if above and keys[-1] == H.INF:  # the percentile is an infinite maximum: inf - inf
            assert np.isnan(ref["thr64"]) and np.array_equal(ref["out"], w), tag
            n_top_inf += 1
        if not above and keys[lo] < H.INF == keys[lo + 1]:
            if g == 0:
                assert np.isnan(ref["thr64"]) and np.array_equal(ref["out"], w), tag
                branches["zero"] += 1
            elif g < 0.5:
                assert ref["thr64"] == np.inf and ref["cmp"] == np.inf, tag
                finite = (w & 0x7FFF) < H.INF
                assert not ref["out"][finite].any() and np.array_equal(ref["out"][~finite], w[~finite]), tag
                branches["below_half"] += 1
            else:
                assert np.isnan(ref["thr64"]) and np.array_equal(ref["out"], w), tag
                branches["from_half"] += 1
        if not above and keys[lo] == H.INF:
            assert np.isnan(ref["thr64"]), tag
            n_both += 1
    assert min(branches.values()) >= 2, branches
    assert n_nan >= 5 * 10 * 6 and n_above == 2 * 2 * 4 and n_both >= 10 and n_top_inf >= 10
    by_name = {name: w for name, _, w, _ in special}
    assert int((by_name["neg_zero_block_2000"] == H.NEG_ZERO).sum()) == 666
    assert all(0 < (k & 0x7FFF) < 0x400 for k in by_name["subnormal_37"])
    # -0.0 under a threshold of 0 keeps its sign; a pruned word is +0 and both count as zeros
    ref = [r for name, pct, _, r in special if name == "neg_zero_block_2000" and pct == 23.6][0]
    assert ref["thr64"] == 0.0 and int((ref["out"] == H.NEG_ZERO).sum()) == 666 and ref["zero_count"] == 668
    ref = [r for name, pct, _, r in special if name == "neg_zero_block_2000" and pct == 90.0][0]
    assert not (ref["out"] == H.NEG_ZERO).any() and ref["zero_count"] > 1000


def _assert_special(tag, ref, out, thr, ck, mk, z, cmp_word):
    """one result of the core against the restated rule: words exactly, thr64, the compare value
    and the maximum by NaN-ness first and bits otherwise"""
    assert np.array_equal(out, ref["out"]), (tag, np.flatnonzero(out != ref["out"])[:5])
    SV.assert_same_bits(np.float64(thr), ref["thr64"], (tag, "thr64"))
    SV.assert_same_bits(_half_word(cmp_word), ref["cmp"], (tag, "compare value"))
    SV.assert_same_bits(_half_word(mk), ref["max"], (tag, "max"))
    # the key the mask compares with: the compare value's, 0 (nothing is below it) when it is NaN
    assert ck == (0 if np.isnan(ref["cmp"]) else int(ref["cmp"].view(np.uint16))), tag
    assert z == ref["zero_count"], tag


def test_special_populations_through_the_core(core, special):
    core.half_core_from_double.argtypes = [ctypes.c_double]
    core.half_core_from_double.restype = ctypes.c_uint16
    for name, pct, w, ref in special:
        out, thr, ck, mk, z = prune(core, w, pct)
        _assert_special((name, pct), ref, out, thr, ck, mk, z, core.half_core_from_double(thr))


def _special_program_lines(exe, special):
    lines = []
    for name, pct, w, ref in special:
        r0, above, gamma = H.np_ranks(len(w), pct)
        lines.append("%d %d %d %s %s" % (len(w), r0, above, float(gamma).hex(), " ".join(str(int(v)) for v in w)))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
    got = out.stdout.strip().split("\n")
    assert len(got) == len(special)
    for (name, pct, w, ref), line in zip(special, got):
        f = line.split()
        thr = float.fromhex(f[0])
        with np.errstate(over="ignore"):
            cmp_word = int(np.float64(thr).astype(np.float16).view(np.uint16))  # the program prints the key alone
        _assert_special((name, pct), ref, np.array([int(v) for v in f[4:]], np.uint16), thr, int(f[1]), int(f[2]),
                        int(f[3]), cmp_word)


def test_special_populations_through_the_program(special):
    _special_program_lines(_build(EXE, ["-O2"]), special)


def test_special_populations_through_the_program_under_asan_ubsan(special):
    """the stand-alone sanitizer build of test_program_under_asan_ubsan on the special populations"""
    _special_program_lines(_build(EXE_SAN, SAN), special)
