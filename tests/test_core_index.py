"""CPU check of the product's gather-form filter-bank math (csrc/wt_dwt_core.h, compiled for
the host here) against the oracle's literal scatter restatement and the pywt 1-D KATs."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import corecheck_shim
from tests import golden_io as G


@pytest.fixture(scope="module")
def core():
    return corecheck_shim.load()


_p = corecheck_shim.fptr


def test_gather_matches_kat_and_oracle(core):
    z = np.load(G.GOLDEN + "/dwt1d_kat.npz")
    keys = sorted({k.rsplit("/", 1)[0] for k in z.files})
    for key in keys:
        wname = key.split("/")[0]
        f = O.filters(wname)
        F = f.shape[1]
        lo, hi, rlo, rhi = [np.ascontiguousarray(f[i]) for i in range(4)]
        x = z[key + "/x"]
        N = x.size
        a = np.empty((N + 1) // 2, np.float32)
        d = np.empty_like(a)
        core.core_dwt1(_p(x), ctypes.c_longlong(N), F, _p(lo), _p(hi), _p(a), _p(d))
        assert np.array_equal(a, z[key + "/a"]) and np.array_equal(d, z[key + "/d"]), key
        ca, cd = z[key + "/ca"], z[key + "/cd"]
        y = np.empty(2 * ca.size, np.float32)
        core.core_idwt1(_p(ca), _p(cd), ctypes.c_longlong(ca.size), F, _p(rlo), _p(rhi), _p(y))
        assert np.array_equal(y, z[key + "/y"]), key


def test_gather_matches_oracle_scatter_wide(core):
    rng = np.random.default_rng(7)
    for wname in ["haar", "db2", "db8", "bior3.3", "rbio2.2", "coif3", "sym11", "dmey", "db38", "coif17"]:
        f = O.filters(wname)
        F = f.shape[1]
        rlo, rhi = np.ascontiguousarray(f[2]), np.ascontiguousarray(f[3])
        for N in list(range(1, 80)) + [127, 128, 129]:
            ca = rng.standard_normal(N).astype(np.float32)
            cd = rng.standard_normal(N).astype(np.float32)
            y = np.empty(2 * N, np.float32)
            core.core_idwt1(_p(ca), _p(cd), ctypes.c_longlong(N), F, _p(rlo), _p(rhi), _p(y))
            assert np.array_equal(y, O.idwt1(ca, cd, wname)), (wname, N)
            x = rng.standard_normal(N).astype(np.float32)
            a = np.empty((N + 1) // 2, np.float32)
            d = np.empty_like(a)
            core.core_dwt1(_p(x), ctypes.c_longlong(N), F, _p(np.ascontiguousarray(f[0])),
                           _p(np.ascontiguousarray(f[1])), _p(a), _p(d))
            ea, ed = O.dwt1(x, wname)
            assert np.array_equal(a, ea) and np.array_equal(d, ed), (wname, N)


def test_geometry_matches_oracle_packing(core):
    for H, W, L in [(3, 3, 1), (7, 7, 2), (96, 100, 3), (4096, 4096, 5), (5, 5, 2), (130, 97, 3), (10, 128, 1)]:
        buf = (ctypes.c_longlong * (2 + 4 * (L + 1)))()
        core.core_geom(H, W, L, buf)
        assert (buf[0], buf[1]) == O.packed_shape(H, W, L)
