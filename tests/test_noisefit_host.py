"""CPU: the host side of the fitted noise floor (get_noise_fit / find_kc,
pplib.py:2341-2373, 1530-1561) -- the entry points' argument checks, the
width grid and its kc table against the grids the reference's brute walked,
the host one-liners against the reference's values, and the well-posedness
margins of tests/golden/noisefit.npz (make_golden_noisefit.py)."""
import ctypes
import os

import numpy as np
import pytest

from pulseportraiture_amd import _lib, engine, pplib

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "noisefit.npz"))
ROW_CASES = [str(c) for c in G["cases"]] + ["clamp_64", "edge_4095", "edge_8192",
                                            "port_8x2048", "port_9x1000",
                                            "degenerate"]


def _tables(fn="exp_dc", n=33):
    return engine.find_kc_tables(n, fn)


def _batch(lib, nbin=64, dtype=_lib.PPF_F64, fact=1.1, a=True, kc=True,
           null_in=False, kc_table=None):
    ag, kt = _tables(n=nbin // 2 + 1)
    if kc_table is not None:
        kt = np.array(kc_table, dtype=np.int32)
    one = ctypes.c_void_p(8)       # never dereferenced: no context, no launch
    return lib.ppf_noise_fit_batch(
        None, 2, nbin, dtype, None if null_in else one, fact,
        ag.ctypes.data if a else None, kt.ctypes.data if kc else None, one,
        one, None)


def _long(lib, nbin=16384, dtype=_lib.PPF_F32, fact=1.1, ws=1 << 40,
          null_out=False):
    ag, kt = _tables()             # their values are not looked at here
    one = ctypes.c_void_p(8)
    return lib.ppf_noise_fit_long(
        None, 2, nbin, dtype, one, fact, ag.ctypes.data, kt.ctypes.data,
        None if null_out else one, one, one, ws, None)


def _find(lib, nharm=129, errs_len=1, fn=0, errs=True, null_pows=False):
    ag, kt = _tables(n=nharm)
    one = ctypes.c_void_p(8)
    return lib.ppf_find_kc_batch(
        None, 1, nharm, None if null_pows else one, one if errs else None,
        errs_len, fn, ag.ctypes.data, kt.ctypes.data, one, None)


def test_noise_fit_entries_validate_on_the_host():
    """The documented codes, before the context is looked at (no GPU)."""
    lib = _lib.load()
    E, U = _lib.PPF_EINVAL, _lib.PPF_EUNSUP
    # ppf_noise_fit_batch: the lengths of ppf_noise_batch
    for nbin in (30, 31, 8194, 4097, 16384):
        assert _batch(lib, nbin=nbin) == U, nbin
    assert _batch(lib, dtype=7) == E
    for fact in (0.0, -1.1, np.nan, np.inf):
        assert _batch(lib, fact=fact) == E, fact
    assert _batch(lib, a=False) == E
    assert _batch(lib, kc=False) == E
    assert _batch(lib, null_in=True) == E
    assert _batch(lib, kc_table=[-1] + [3] * 19) == E
    # a valid call stops at the NULL context
    for nbin in (32, 33, 1001, 4095, 8192):
        assert _batch(lib, nbin=nbin) == E, nbin
    # ppf_noise_fit_long: any length ppf_noise_long takes from 3 samples on
    wsb = lib.ppf_noise_fit_long_workspace_bytes
    for nbin in (3, 30, 8194, 9000, 16384, 1 << 25):
        assert wsb(2, nbin) > lib.ppf_noise_long_workspace_bytes(2, nbin), nbin
    # ... the power spectra beside ppf_noise_long's buffers
    assert wsb(2, 16384) - lib.ppf_noise_long_workspace_bytes(2, 16384) >= \
        2 * 8193 * 8
    for nbin in (0, 1, 2, (1 << 25) + 2):
        assert wsb(2, nbin) == 0, nbin
        if nbin > 0:
            assert _long(lib, nbin=nbin) == U, nbin
    assert _long(lib, nbin=0) == E
    assert _long(lib, dtype=2) == E
    assert _long(lib, fact=-2.0) == E
    assert _long(lib, fact=np.nan) == E
    assert _long(lib, null_out=True) == E
    assert _long(lib, ws=wsb(2, 16384) - 1) == E
    assert _long(lib, ws=wsb(2, 16384)) == E           # valid: NULL context
    # ppf_find_kc_batch
    assert _find(lib, nharm=1) == E
    assert _find(lib, fn=2) == E
    assert _find(lib, fn=-1) == E
    for el in (0, 2, 128, 130):
        assert _find(lib, errs_len=el) == E, el
    assert _find(lib, null_pows=True) == E
    for kw in (dict(), dict(errs_len=129), dict(errs=False, errs_len=0),
               dict(fn=1), dict(nharm=2)):
        assert _find(lib, **kw) == E, kw                # valid: NULL context
    # the Python wrappers: an unknown fn never reaches the library
    assert pplib.find_kc(np.ones(16), fn="gaussian") == 0
    with pytest.raises(KeyError):
        engine.find_kc_tables(16, "gaussian")


@pytest.mark.parametrize("case", ROW_CASES)
def test_tables_match_the_reference_grids(case):
    """engine.find_kc_tables against the a grid scipy.optimize.brute walked
    in the reference's find_kc and the kc of each of its values, bit for
    bit, at every stored N."""
    for sfx in ("", "__f32"):
        if case + "__a_grid" + sfx not in G:
            continue
        N = G[case + "__pows" + sfx].shape[1]
        a, kc = engine.find_kc_tables(N)
        assert a.dtype == np.float64 and kc.dtype == np.int32
        for ref in G[case + "__a_grid" + sfx]:
            np.testing.assert_array_equal(a, ref)
        np.testing.assert_array_equal(kc, G[case + "__kc_table" + sfx])
        # the stored winner's kc is the reference's find_kc
        np.testing.assert_array_equal(kc[G[case + "__win" + sfx] // 400],
                                      G[case + "__kc" + sfx])


def test_half_tri_tables_match_the_reference_grid():
    for key in ("scalar", "array"):
        a, kc = engine.find_kc_tables(len(G["half_tri__pows_" + key]),
                                      "half_tri")
        np.testing.assert_array_equal(a, G["half_tri__a_grid_" + key])
        np.testing.assert_array_equal(kc, G["half_tri__kc_table_" + key])
        assert kc[G["half_tri__win_" + key] // 400] == \
            G["half_tri__kc_" + key]


def test_mgrid_is_not_linspace_everywhere():
    """brute's grid is np.mgrid[lo:hi:20j], whose last element is 19 * step +
    lo and not hi itself: at N = 4501 (the 9 x 1000 portrait) they differ."""
    a, _ = engine.find_kc_tables(4501)
    np.testing.assert_array_equal(a, G["port_9x1000__a_grid"][0])
    assert a[-1] != 1.0 and abs(a[-1] - 1.0) < 1e-15


def test_host_one_liners_match_the_reference():
    prof = G["host__prof"]
    for i, (a, b, dc, n) in enumerate(G["host__half_tri_args"]):
        np.testing.assert_array_equal(
            pplib.half_triangle_function(a, b, dc, int(n)),
            G["host__half_tri_%d" % i])
    FFT = np.fft.rfft(prof)
    d = np.log10(np.real(FFT * np.conj(FFT)) / len(prof))
    errs = G["half_tri__errs_array"]
    for p, e, h in zip(G["host__chi2_params"], G["host__chi2_exp_dc"],
                       G["host__chi2_half_tri"]):
        assert pplib.find_kc_function(p, d, 0.5, "exp_dc") == e
        with np.errstate(divide="ignore"):      # a < 1: a base of 0 bins
            assert pplib.find_kc_function(p, d, errs, "half_tri") == h
        assert pplib.find_kc_function(p, d, errs, "gaussian") == 0.0
    np.testing.assert_array_equal(pplib.brickwall_filter(12, 5),
                                  G["host__brickwall_12_5"])
    np.testing.assert_array_equal(pplib.wiener_filter(prof, 1.3),
                                  G["host__wiener"])
    assert pplib.fit_brickwall(prof, 1.3) == G["host__fit_brickwall"]


def test_stored_winners_are_well_posed():
    """Every stored row with a finite spectrum: the best chi-squared at
    another a index exceeds the winner's by more than a relative 1e-6 (the
    condition make_golden_noisefit.py refuses a case on), so kc parity does
    not hang on rounding; the clamp case reaches k_crit >= N."""
    assert G["gap_min"] == 1e-6
    n = 0
    for key in G.files:
        if "__gap" not in key:
            continue
        gaps = np.atleast_1d(G[key])
        if key.startswith("degenerate"):
            assert np.isnan(gaps[[1, 2]]).all()
            gaps = gaps[[0, 3]]
        assert (gaps > 1e-6).all(), (key, gaps)
        n += len(gaps)
    assert n == 2 * 15 + 1 + 2 + 2 + 2 + 1 + 2
    assert G["fact"] * G["clamp_64__kc"][0] >= G["clamp_64__pows"].shape[1]
