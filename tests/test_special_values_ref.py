"""CPU checks of the special-value cases (tests/special_values.py) on the reference alone: the cases
are not trivial (NaN and inf spread but do not flood, the subnormal case is subnormal after the
transform, 2^126 overflows only where the filter's gain takes it there, the zero blocks survive)
and at the shape tests/test_gpu_special_values.py runs them they reach the kernels they are meant
for (interior and frame tiles at both levels, the generic tiled kernels up to F = 34, the per-point
kernels from F = 36).  Oracle and tests/fbplan_shim.py only -- and the host build of the shared
point evaluators (csrc/wt_dwt_core.h), held to the oracle on lines of signed zeros by
assert_same_bits: it is the code the kernels share, and the one place a CPU test can see an
accumulator that does not start at +0 (one started from its first product gives -0.0 where every
product is -0.0: a line of -0.0 under haar's low-pass taps, which have one sign; nothing else in
the CPU suite tells the two apart).  The last test regenerates the extension modes' fixture
(tools/gen_golden_special_modes.py, the reference chain of tests/modes_ref.py).

Why no output may hold -0.0: pywt starts every analysis and synthesis sum at +0 and adds to it,
under round-to-nearest +0 + x is never -0, and np.where writes +0.  So no packed coefficient and no
output of a transformed tensor is -0.0 whatever the input holds; the checks below assert it of the
oracle and of the shared core, tests/test_gpu_special_values.py of the kernels.

Figures (seed 97, tid 0, (1, 2, 161, 464), level 2, percentile 61.8) are asserted as inequalities;
the values they had when this was written stand beside them."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import corecheck_shim
from tests import fbplan_shim as S
from tests import special_values as SV

SHAPE, SEED, TID, LEVEL, PCT = (1, 2, 161, 464), 97, 0, 2, 61.8
WAVELETS = ["haar", "bior3.3", "db8", "db9", "db10", "db17", "db18"]
TINY32 = np.float32(2.0 ** -126)   # the smallest normal float32


@pytest.fixture(scope="module")
def inputs():
    cs = SV.cases(SHAPE, SEED, TID)
    cs["plain"] = SV.plain(SHAPE, SEED, TID)
    return cs


def _oracle(x, wavelet):
    with np.errstate(all="ignore"):
        return O.prune_tensor(x, wavelet, LEVEL, PCT, want_coeffs=True)


def test_inputs_are_what_they_are_named(inputs):
    n = int(np.prod(SHAPE))
    zb = inputs["zero_blocks"]
    assert SV.neg_zero_words(zb) == 40 * 464 + 61 * 264 and int((zb == 0).sum()) == 100 * 340 + 40 * 464 + 61 * 264
    assert np.all(inputs["constant"] == np.float32(0.0371))
    sub = inputs["subnormal"]
    assert np.all(np.abs(sub) < TINY32) and int((sub != 0).sum()) > 0.99 * n
    assert np.abs(inputs["huge"]).max() == np.float32(2.0 ** 126) and np.isfinite(inputs["huge"]).all()
    for name, where in (("nan_interior", (0, 0, 70, 230)), ("nan_corner", (0, 1, 0, 0))):
        assert int(np.isnan(inputs[name]).sum()) == 1 and np.isnan(inputs[name][where])
    assert inputs["infs"][0, 0, 160, 463] == np.inf and inputs["infs"][0, 1, 75, 100] == -np.inf
    assert int(np.isinf(inputs["infs"]).sum()) == 2
    assert np.array_equal(inputs["scaled_up"], inputs["plain"] * np.float32(4096))
    assert np.array_equal(inputs["scaled_down"] * np.float32(2.0 ** 30), inputs["plain"])
    # other shapes: the positions scale with the extent, a single image takes both images' marks
    small = SV.cases((6, 4, 10, 12), SEED, TID)
    assert np.isnan(small["nan_interior"].reshape(24, 10, 12)[0, 4, 5]) and np.isnan(small["nan_corner"].reshape(24, 10, 12)[1, 0, 0])
    assert SV.neg_zero_words(small["zero_blocks"]) == 2 * 12 + 4 * 7
    one = SV.cases((96, 100), SEED, TID)
    assert int(np.isinf(one["infs"]).sum()) == 2 and SV.neg_zero_words(one["zero_blocks"]) > 0


def test_the_comparison_rule():
    """assert_same_bits: a NaN equals a NaN of any payload, a zero only the zero of its sign, and
    everything else its own word; np.array_equal sees neither the sign nor, without equal_nan, the NaN"""
    f32 = lambda *bits: np.array(bits, np.uint32).view(np.float32)  # noqa: E731
    SV.assert_same_bits(f32(0x7FC00000, 0, 0x80000000, 0x3F800000), f32(0xFFC00001, 0, 0x80000000, 0x3F800000))
    SV.assert_same_bits(np.float64(np.nan), -np.float64(np.nan))
    SV.assert_same_bits(np.float32(1.5), np.float32(1.5))
    assert np.array_equal(f32(0x80000000), f32(0))
    for got, ref in ((f32(0x80000000), f32(0)), (f32(0), f32(0x80000000)), (f32(0x7FC00000), f32(0x7F800000)),
                     (f32(0x3F800000), f32(0x7FC00000)), (f32(0x3F800000), f32(0x3F800001)),
                     (np.float64(-0.0), np.float64(0.0)), (np.float64(1.0), np.float64(np.nan)),
                     (np.float32(1.0), np.float64(1.0)), (f32(0, 0), f32(0))):
        with pytest.raises(AssertionError):
            SV.assert_same_bits(got, ref, "must differ")
    good = dict(thr64=0.5, thr32_bits=0x3F000000, max_abs_bits=0x7FC00000, zero_count=3, eff_level=2, coeff_numel=8)
    ref = dict(thr64=0.5, thr32=np.float32(0.5), max_abs=-np.float32(np.nan), zero_count=3, eff_level=2, coeff_numel=8)
    SV.assert_same_record(good, ref)
    for field, value in (("thr64", -0.5), ("thr32_bits", 0x3F000001), ("max_abs_bits", 0x7F800000), ("zero_count", 4),
                         ("eff_level", 1), ("coeff_numel", 9)):
        with pytest.raises(AssertionError):
            SV.assert_same_record(dict(good, **{field: value}), ref)
    assert SV.neg_zero_words(f32(0x80000000, 0, 0x80000001, 0x80000000)) == 2


@pytest.mark.parametrize("wavelet", WAVELETS)
def test_cases_are_not_trivial(inputs, wavelet):
    n = int(np.prod(SHAPE))
    res = {name: _oracle(x, wavelet) for name, x in inputs.items()}
    for name, (out, d, P) in res.items():
        assert d["eff_level"] == LEVEL and P.size == d["coeff_numel"] == 151264, name
        # no -0.0 after a transform, whatever the input holds
        assert SV.neg_zero_words(P) == 0 and SV.neg_zero_words(out) == 0, name
        assert d["zero_count"] == int((out == 0).sum()), name
    for name in ("nan_interior", "nan_corner"):
        out, d, P = res[name]
        assert np.isnan(d["thr64"]) and np.isnan(d["thr32"]), name
        # haar 16, bior3.3 1 444 / 1 638, db8 7 396 / 7 830, db17 31 556: the NaN spreads and does not flood
        assert 1 <= int(np.isnan(out).sum()) <= n // 2, name
        assert 1 <= int(np.isnan(P).sum()) and not np.isinf(P).any(), name
    out, d, P = res["infs"]
    # haar 10 inf and 4 NaN, bior3.3 38 and 382: inf - inf and, under bior3.3, 0 x inf
    assert np.isinf(P).any() and np.isnan(P).any() and np.isnan(d["thr64"])
    assert 1 <= int(np.isnan(out).sum()) <= n // 2
    out, d, P = res["subnormal"]
    # 150 800 of 151 264 cells (haar 149 407): every coefficient but the exact zeros is subnormal
    assert int(((np.abs(P) < TINY32) & (P != 0)).sum()) >= 0.9 * P.size
    assert 0.0 < d["thr64"] < float(TINY32) and 0.0 < d["thr32"] < TINY32
    out, d, P = res["huge"]
    if wavelet == "bior3.3":  # its synthesis gain is above 1: 66 inf and 26 NaN of 151 264
        assert np.isinf(P).any() and int((~np.isfinite(P)).sum()) < 0.01 * P.size
    elif wavelet in ("haar", "db8", "db17"):
        assert np.isfinite(P).all() and np.isfinite(out).all() and np.isfinite(d["thr64"])
    if wavelet in ("haar", "db8"):  # 68 680 and 12 398 zeros survive the round trip
        assert res["zero_blocks"][1]["zero_count"] > 0
    if wavelet == "haar":
        out, d, P = res["constant"]
        assert d["thr64"] == 0.0 and d["zero_count"] == 0  # the details are exact zeros, the median with them
    for name in ("plain", "scaled_up", "scaled_down", "zero_blocks"):
        assert np.isfinite(res[name][0]).all() and np.isfinite(res[name][1]["thr64"]), name
    # scaled by a power of two: the same masks, every coefficient outside the fused window's bins
    assert res["scaled_up"][1]["zero_count"] == res["scaled_down"][1]["zero_count"] == res["plain"][1]["zero_count"]
    assert np.abs(res["scaled_up"][2]).max() > 2.0 ** 6 and np.abs(res["scaled_down"][2]).max() < 2.0 ** -26


def test_levels_of_the_long_filter_and_small_image_cases():
    """eff_level as tests/test_gpu_special_values.py asserts it"""
    for wavelet, shape, level, eff in (("db10", SHAPE, 2, 2), ("db17", SHAPE, 2, 2), ("db18", SHAPE, 2, 2),
                                       ("coif17", (1, 1, 230, 470), 1, 1), ("db38", (1, 1, 230, 470), 1, 1),
                                       ("haar", (6, 4, 10, 12), 2, 2), ("db2", (6, 4, 10, 12), 1, 1)):
        assert min(level, O.dwt_max_level(min(shape[-2:]), O.dec_len(wavelet))) == eff, (wavelet, shape)
    assert [O.dec_len(w) for w in ("db10", "db17", "db18", "db38", "coif17")] == [20, 34, 36, 76, 102]


def test_the_shape_reaches_interior_and_frame_tiles():
    fb = S.load_shim()
    c = S.consts(fb)
    q = (ctypes.c_int * 4)()
    R, C = SHAPE[-2:]
    R1, C1, R2, C2 = (R + 1) // 2, (C + 1) // 2, (R + 3) // 4, (C + 3) // 4
    assert (R1, C1, R2, C2) == (81, 232, 41, 116)

    def fwd(R, C, F):
        Ro, Co = (R + 1) // 2, (C + 1) // 2
        grid = (-(-Ro // c["FR"]), -(-Co // c["FC"]))
        return grid, (q[1], q[3]) if fb.fbp_fwd_interior(R, C, 1, 4 * Ro * Co, F, q) else None

    def inv(R, C, oH, oW, F):
        grid = (-(-oH // c["IR"]), -(-oW // c["IC"]))
        return grid, (q[1], q[3]) if fb.fbp_inv_interior(R, C, oH, oW, 4 * R * C, R * C, F, q) else None

    for F in (8, 16, 18):
        assert F in c["spec"] and fb.fbp_tiled_ok(2, R, C, F) and fb.fbp_tiled_ok(2, R1, C1, F)
        assert fwd(R, C, F) == ((6, 5), (3, 3))     # level 1: interior tiles inside a frame
        assert fwd(R1, C1, F) == ((3, 3), (1, 1))   # level 2: one interior tile
        grid, rect = inv(R1, C1, R, C, F)
        assert grid == (3, 8) and rect is not None and 0 < rect[0] * rect[1] < 24
        assert inv(R2, C2, R1, C1, F)[1] is None    # level 2: the general inverse also runs in mode 2
    assert 2 in c["spec"] and fwd(R, C, 2) == ((6, 5), (5, 4))
    grid, rect = inv(R1, C1, R, C, 2)
    assert grid == (3, 8) and rect is not None and rect[0] * rect[1] < 24
    # the images of 10 x 12 stay below the tiled kernels' 512 cells: the per-point kernels of levels.inc
    assert not fb.fbp_tiled_ok(24, 10, 12, 2) and not fb.fbp_tiled_ok(24, 10, 12, 4)


def test_filter_length_dispatch_boundary():
    fb = S.load_shim()
    c = S.consts(fb)
    R, C = SHAPE[-2:]
    for F, ok in ((20, True), (34, True), (36, False), (76, False), (102, False)):
        assert bool(fb.fbp_tiled_ok(2, R, C, F)) == ok and bool(fb.fbp_tiled_ok(2, (R + 1) // 2, (C + 1) // 2, F)) == ok, F
        assert F not in c["spec"]
    assert S.per_filter(fb, 34)["inv_lds"] == 63504 <= c["FB_MAX_LDS"] < S.per_filter(fb, 36)["inv_lds"] == 65600


_p = corecheck_shim.fptr


@pytest.fixture(scope="module")
def core():
    return corecheck_shim.load()


@pytest.mark.parametrize("wavelet", ["haar", "bior3.3", "db8", "db9", "db10", "db18"])
def test_shared_core_on_lines_of_signed_zeros(core, inputs, wavelet):
    """csrc/wt_dwt_core.h on the host, one level each way over lines of the zero_blocks case (a
    line of -0.0 throughout, a line that enters the -0.0 block, the +0.0 block, the odd-length
    column with its repeated sample) and of the infs case: the oracle's words, and no -0.0."""
    f = O.filters(wavelet)
    F = f.shape[1]
    lo, hi, rlo, rhi = [np.ascontiguousarray(f[i]) for i in range(4)]
    zb, infs = inputs["zero_blocks"], inputs["infs"]
    lines = [zb[0, 1, 5, :], zb[0, 1, 120, :], zb[0, 0, 60, :], zb[0, 1, :, 300], zb[0, 1, :, 10], infs[0, 0, 160, :],
             infs[0, 0, :, 463], np.full(37, -0.0, np.float32)]
    assert all(SV.neg_zero_words(ln) > 0 for ln in lines[:2] + lines[3:5] + lines[7:])
    for k, x in enumerate(lines):
        x = np.ascontiguousarray(x)
        N = x.size
        a, d = np.empty((N + 1) // 2, np.float32), np.empty((N + 1) // 2, np.float32)
        core.core_dwt1(_p(x), ctypes.c_longlong(N), F, _p(lo), _p(hi), _p(a), _p(d))
        with np.errstate(all="ignore"):
            ea, ed = O.dwt1(x, wavelet)
        # the synthesis over bands that hold -0.0 themselves: the input line's halves
        ca, cd = np.ascontiguousarray(x[:N // 2]), np.ascontiguousarray(x[N - N // 2:])
        y = np.empty(2 * ca.size, np.float32)
        core.core_idwt1(_p(ca), _p(cd), ctypes.c_longlong(ca.size), F, _p(rlo), _p(rhi), _p(y))
        with np.errstate(all="ignore"):
            ey = O.idwt1(ca, cd, wavelet)
        assert SV.neg_zero_words(ea) == SV.neg_zero_words(ed) == SV.neg_zero_words(ey) == 0, (wavelet, k)
        assert SV.neg_zero_words(a) == SV.neg_zero_words(d) == SV.neg_zero_words(y) == 0, (wavelet, k, "-0.0 from the core")
        SV.assert_same_bits(a, ea, (wavelet, k, "cA"))
        SV.assert_same_bits(d, ed, (wavelet, k, "cD"))
        SV.assert_same_bits(y, ey, (wavelet, k, "y"))


def test_generator_gives_the_committed_modes_fixture():
    """tools/gen_golden_special_modes.py, run in memory, gives tests/golden/special_modes_*; the
    fixture holds what its cases are for, and no -0.0 under any extension mode either"""
    import importlib.util
    import json
    import os

    from tests import golden_io as G
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(G.GOLDEN, "special_modes_manifest.json")) as fh:
        man = json.load(fh)
    arrs = np.load(os.path.join(G.GOLDEN, "special_modes_cases.npz"))
    spec = importlib.util.spec_from_file_location("gen_golden_special_modes",
                                                  os.path.join(root, "tools", "gen_golden_special_modes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    man2, arrs2 = gen.generate()
    assert json.loads(json.dumps(man2, sort_keys=True)) == man
    assert sorted(arrs2) == sorted(arrs.files)
    for k in arrs.files:
        assert arrs2[k].dtype == arrs[k].dtype == np.float32 and arrs2[k].shape == arrs[k].shape, k
        assert arrs2[k].tobytes() == arrs[k].tobytes(), k
    size = sum(os.path.getsize(os.path.join(G.GOLDEN, f)) for f in ("special_modes_manifest.json", "special_modes_cases.npz"))
    assert size < 500000
    cases = man["cases"]
    assert len(cases) == len(gen.SETTINGS) * len(gen.CASES) * len(gen.MODES) == 80
    for key, c in cases.items():
        out = arrs[key + "/out"]
        assert c["eff_level"] == c["level"] >= 1 and c["neg_zero_words"] == 0, key
        nan_bits = out.view(np.uint32)[np.isnan(out)]
        assert np.all(nan_bits == 0x7FC00000), key  # one quiet pattern
        if c["case"] == "nan_corner":
            assert c["thr64_hex"] == "nan" and c["thr32_bits"] == 0x7FC00000 and 1 <= int(np.isnan(out).sum()) <= out.size // 2, key
        elif c["case"] == "infs":
            assert c["packed_inf"] >= 1 and not np.isfinite(out).all(), key
        elif c["case"] == "subnormal":
            assert c["packed_subnormal"] >= 0.75 * c["coeff_numel"] and 0 < c["thr32_bits"] < 0x00800000, key
        else:
            assert c["packed_nan"] == c["packed_inf"] == 0, key
    for name in ("tiny_haar", "tiny_db2", "level_bior33"):  # exact zeros survive the round trip
        assert any(c["zero_count"] > 0 for k, c in cases.items() if k.startswith(name + "/zero_blocks/")), name
    # under the zero extension an inf never meets its negative: a finite threshold beside inf coefficients
    assert any(c["case"] == "infs" and c["thr64_hex"] != "nan" for c in cases.values())
    assert any(c["case"] == "infs" and c["packed_nan"] for c in cases.values())


def test_float16_cases_are_not_trivial():
    """special_values.cases_f16 at the settings tests/test_gpu_special_values.py runs them, on the
    oracle alone (and the modes' reference chain for the symmetric setting): `overflow` holds finite
    inputs only and narrows at least one finite float32 result to inf; `half_subnormal` is mostly
    half subnormals, at least one nonzero float32 result below 2^-25 narrows to a signed zero and
    at least one result to a subnormal; a NaN or an inf in the input reaches the narrowed result.
    Figures at the time of writing: overflow 16 / 2 / 15 / 2620 results narrowed to inf at the four
    settings, half_subnormal 30 / 1 / 32 / 6760 narrowed to zero (21 / 1 / 22 / 3400 of them -0.0)."""
    from tests import modes_ref
    from tests.ref_helpers import f16_transformed_ref
    settings = [(s, w, lv, "periodization") for s, w, lv in SV.F16_SETTINGS] + [SV.F16_SYMMETRIC + ("symmetric",)]
    for tid, (shape, wavelet, level, mode) in enumerate(settings):
        cs = SV.cases_f16(shape, SV.F16_SEED, tid)
        res = {}
        for name, x16 in cs.items():
            if mode == "periodization":
                out32, out16, d = f16_transformed_ref(x16, wavelet, level, SV.F16_PCT)
                assert d["eff_level"] == level, (shape, name)
            else:
                with np.errstate(all="ignore"):
                    out32 = modes_ref.chain(x16.astype(np.float32), wavelet, level, mode, SV.F16_PCT)[4]
                    out16 = out32.astype(np.float16)
            res[name] = (out32, out16)
        tag = (shape, wavelet)
        x16 = cs["overflow"]
        assert np.isfinite(x16).all() and np.abs(x16).max() == np.float16(SV.OVERFLOW_MAX), tag
        out32, out16 = res["overflow"]
        assert int((np.isfinite(out32) & np.isinf(out16)).sum()) >= 1 and np.isfinite(out32).all(), tag
        x16 = cs["half_subnormal"]
        assert int(((np.abs(x16) < SV.HALF_TINY) & (x16 != 0)).sum()) > 0.9 * x16.size, tag
        out32, out16 = res["half_subnormal"]
        assert int(((out32 != 0) & (np.abs(out32) < 2.0 ** -25) & (out16 == 0)).sum()) >= 1, tag
        assert int(((out16 != 0) & (np.abs(out16) < SV.HALF_TINY)).sum()) >= 1, tag
        for name in ("nan_interior", "nan_corner", "infs"):
            assert not np.isfinite(cs[name]).all() and 1 <= int(np.isnan(res[name][1]).sum()) <= x16.size // 2, (tag, name)
        x16 = cs["zero_blocks"]
        assert int((x16.view(np.uint16) == 0x8000).sum()) > 0 and np.isfinite(res["zero_blocks"][1]).all(), tag


def test_the_comparison_rule_on_halves():
    """assert_same_bits on float16 words: the same rule at 16 bits"""
    f16 = lambda *bits: np.array(bits, np.uint16).view(np.float16)  # noqa: E731
    SV.assert_same_bits(f16(0x7E00, 0, 0x8000, 0x3C00, 0x7C00), f16(0xFE01, 0, 0x8000, 0x3C00, 0x7C00))
    for got, ref in ((f16(0x8000), f16(0)), (f16(0x7E00), f16(0x7C00)), (f16(0x3C00), f16(0x3C01)), (f16(1), f16(0)),
                     (f16(0x3C00), np.float32(1.0))):
        with pytest.raises(AssertionError):
            SV.assert_same_bits(got, ref, "must differ")
