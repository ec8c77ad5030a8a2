"""Host side of make_fake_pulsar (no GPU): the ephemeris parser, epochs and
periods, the per-row tables against tests/golden/fake.npz, ppf_fake_batch's
host-side refusals and the Python refusals."""
import ctypes

import numpy as np
import pytest

import fakecases as F
from pulseportraiture_amd import _lib, fake, pplib, psrfits


def test_read_par_example():
    par = fake.read_par(F.PAR)
    assert par.PSR == "J1234-5678"
    assert par.RAJ == "01:02:03.45678901" and par.DECJ == "-04:05:06.7890123"
    assert par.F0 == 345.67890123456789 and par.P0 == par.F0 ** -1
    assert par.F1 == -1.2345679978e-13          # a Fortran D exponent
    assert par.PEPOCH == 50000.0 and par.DM == 34.56789
    # the C-commented binary lines are not read
    assert "A1" not in par and "PB" not in par


def test_read_par_variants(tmp_path):
    p = tmp_path / "b.par"
    p.write_text("PSRJ   J0000+0000\n\nRAJ 00:00:01\nDECJ 10:00:00\n"
                 "P0 2.5D-3 1\nPEPOCH 55000.5\nDM 1.25D1\nC F1 9.9\nUNITS TDB\n"
                 "JUMP\n")
    par = fake.read_par(str(p))
    assert par.PSR == "J0000+0000" and par.P0 == 2.5e-3 and par.F0 == 400.0
    assert par.F1 == 0.0 and par.DM == 12.5 and par.PEPOCH == 55000.5
    p.write_text("PSR X\nRAJ 0\nDECJ 0\nF0 1\nPEPOCH 5\n")
    with pytest.raises(KeyError):
        fake.read_par(str(p))


@pytest.mark.parametrize("start", [None, 55000.25, pplib.MJD(55000, 0.25)])
def test_epochs_and_periods(start):
    par = fake.read_par(F.PAR)
    par.F1 = np.float64(-3e-9)            # large enough to see per sub-int
    nsub, tsub = 3, 100.0
    ep = fake.fake_epochs(par, nsub, tsub, start)
    day0 = 50000.0 if start is None else 55000.25
    np.testing.assert_array_equal(ep.offs_sub, [50.0, 150.0, 250.0])
    dt = (day0 - 50000.0) * 86400.0 + ep.offs_sub
    np.testing.assert_allclose(ep.Ps, 1.0 / (par.F0 + par.F1 * dt), rtol=1e-15)
    assert ep.Ps[0] < ep.Ps[1] < ep.Ps[2]
    # the header fields give the epochs back as psrfits.PSRFITS.epochs does
    assert ep.stt_imjd == int(day0) and 0.0 <= ep.stt_offs < 1.0
    assert ep.stt_smjd == int((day0 - int(day0)) * 86400.0)
    for i, e in enumerate(ep.epochs):
        tot = ep.stt_smjd + ep.stt_offs + ep.offs_sub[i]
        assert e.intday() == ep.stt_imjd
        assert abs(e.fracday() - tot / 86400.0) < 1e-15
        assert abs((e.in_days() - day0) * 86400.0 -
                   (tsub / 2 + i * tsub)) < 1e-5


@pytest.mark.parametrize("case", F.CASES)
def test_tables_match_golden(case):
    """phi, tau_n and gain are plain arithmetic on the reference's own
    formulas: 1e-15 relative."""
    par, ep, tab = F.case_tables(case)
    assert ep.Ps[0] == F.golden(case, "P")
    np.testing.assert_array_equal(tab.freqs, F.golden(case, "freqs"))
    for key in ("phi", "tau_n", "gain"):
        got, want = tab[key].reshape(-1), F.golden(case, key)
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=1e-15, atol=0.0,
                                   err_msg=key)
    # the modelfile's TAU overrides t_scat
    if F.golden(case, "model_tau") != 0:
        assert not tab.tau_n.any() and F.golden(case, "t_scat") != 0
        np.testing.assert_allclose(
            tab.tau_bins, F.golden(case, "model_tau") *
            F.golden(case, "nbin") / ep.Ps, rtol=1e-15)
    else:
        assert tab.tau_bins.tolist() == [0.0]
    assert tab.model_of.tolist() == [0]


def test_tables_per_subint_and_pol():
    par = fake.read_par(F.PAR)
    par.F1 = np.float64(-3e-9)
    ep = fake.fake_epochs(par, 3, 100.0)
    # a modelfile TAU: one template per distinct period
    tab = fake.fake_tables(7.69e-6, par.DM, ep.Ps, nsub=3, npol=4, nchan=8,
                           nbin=64, phase=0.1, dDM=1e-3, t_scat=1e-4)
    assert tab.phi.shape == (3, 8) and tab.gain.shape == (3, 4, 8)
    assert len(tab.tau_bins) == 3 and sorted(tab.model_of) == [0, 1, 2]
    np.testing.assert_array_equal(tab.tau_bins[tab.model_of],
                                  7.69e-6 * 64 / ep.Ps)
    assert not tab.tau_n.any()
    for s in range(3):
        want = -0.1 - pplib.Dconst * (par.DM + 1e-3) / ep.Ps[s] * \
            (tab.freqs ** -2.0 - 1500.0 ** -2.0)
        np.testing.assert_allclose(tab.phi[s], want, rtol=1e-14)
    # xs: the caller's phase is transformed afresh for every sub-int
    t2 = fake.fake_tables(0.0, par.DM, np.full(3, ep.Ps[0]), nsub=3, nchan=8,
                          nbin=64, phase=0.1, dDM=1e-3, xs=[-2.0], Cs=None,
                          nu_DM=1400.0)
    np.testing.assert_array_equal(t2.phi[0], t2.phi[1])
    np.testing.assert_array_equal(t2.phi[0], t2.phi[2])
    # scint=True: nsin = 3 draws per (sub-int, pol) in the reference's order
    np.random.seed(5)
    t3 = fake.fake_tables(0.0, par.DM, ep.Ps[:2], nsub=2, npol=4, nchan=8,
                          nbin=64, scint=True, scales=2.0)
    np.random.seed(5)
    for s in range(2):
        for p in range(4):
            pat = np.zeros(8)
            for _ in range(3):
                a, w, ph = (np.random.uniform(0, 1.0), np.random.chisquare(5.0),
                            np.random.uniform(0, 1))
                pat += a * np.sin(np.linspace(0, w * np.pi, 8) +
                                  ph * np.pi) ** 2
            np.testing.assert_allclose(t3.gain[s, p], 2.0 * pat, rtol=1e-15)


def _fake_call(lib, nsub=1, npol=1, nchan=2, nbin=64, nmodel=1, first=0,
               kind=_lib.PPF_FAKE_I16, null=None, out_off=0):
    """ppf_fake_batch with a NULL context on host buffers (never launched)."""
    # (the arrays are never read: every call here returns before a launch)
    bufs = dict(model=np.zeros(8), model_of=np.zeros(8, np.int32),
                phase=np.zeros(8), tau=np.zeros(8), gain=np.zeros(8),
                noise=np.zeros(8), out=np.zeros(64, np.uint8),
                scl=np.zeros(8, np.float32), offs=np.zeros(8, np.float32))
    p = {k: v.ctypes.data for k, v in bufs.items()}
    p["out"] = (p["out"] + 15) // 16 * 16 + out_off
    if null:
        p[null] = None
    return lib.ppf_fake_batch(
        None, nsub, npol, nchan, nbin, nmodel, p["model"], p["model_of"],
        p["phase"], p["tau"], p["gain"], p["noise"], ctypes.c_uint64(1),
        first, kind, p["out"], p["scl"], p["offs"], None)


def test_fake_batch_validates_on_the_host():
    """The documented codes, before the context is looked at (no GPU)."""
    lib = _lib.load()
    for nbin in (30, 33, 63, 1001, 8194, 16384):
        assert _fake_call(lib, nbin=nbin) == _lib.PPF_EUNSUP, nbin
    assert _fake_call(lib, nsub=1 << 20, npol=4, nchan=1 << 10) == \
        _lib.PPF_EUNSUP                                  # 2^32 rows
    assert _fake_call(lib, nsub=-1) == _lib.PPF_EINVAL
    assert _fake_call(lib, npol=0) == _lib.PPF_EINVAL
    assert _fake_call(lib, nchan=0) == _lib.PPF_EINVAL
    assert _fake_call(lib, nmodel=0) == _lib.PPF_EINVAL
    assert _fake_call(lib, first=-1) == _lib.PPF_EINVAL
    assert _fake_call(lib, kind=2) == _lib.PPF_EINVAL
    assert _fake_call(lib, out_off=4) == _lib.PPF_EINVAL
    for name in ("model", "model_of", "phase", "tau", "gain", "noise", "out",
                 "scl", "offs"):
        assert _fake_call(lib, null=name) == _lib.PPF_EINVAL, name
    # the float64 kind needs no DAT_SCL / DAT_OFFS; valid calls (32, a mixed
    # radix, 8192 bins) then stop at the NULL context
    for nbin in (32, 100, 8192):
        assert _fake_call(lib, nbin=nbin) == _lib.PPF_EINVAL
    assert _fake_call(lib, kind=_lib.PPF_FAKE_F64, null="scl") == \
        _lib.PPF_EINVAL


def test_make_fake_pulsar_refusals(tmp_path, capsys):
    out = str(tmp_path / "x.fits")
    kw = dict(outfile=out, nchan=8, nbin=64, quiet=True)
    with pytest.raises(NotImplementedError):
        pplib.make_fake_pulsar(F.GMODEL, F.PAR, dedispersed=True, **kw)
    with pytest.raises(NotImplementedError):
        pplib.make_fake_pulsar(F.GMODEL, F.PAR, npol=2, **kw)
    with pytest.raises(NotImplementedError):
        pplib.make_fake_pulsar(F.GMODEL, F.PAR, npol=4, state="Intensity",
                               **kw)
    for nbin in (16, 65, 8194, 16384):
        with pytest.raises(NotImplementedError):
            pplib.make_fake_pulsar(F.GMODEL, F.PAR, **dict(kw, nbin=nbin))
    capsys.readouterr()
    assert pplib.make_fake_pulsar(F.GMODEL, F.PAR, noise_stds=np.ones(7),
                                  **kw) == 0
    assert capsys.readouterr().out == "\nlen(noise_stds) != nchan\n\n"
    assert pplib.make_fake_pulsar(F.GMODEL, F.PAR, scales=[1.0] * 9,
                                  **kw) == 0
    assert capsys.readouterr().out == "\nlen(scales) != nchan\n\n"
    import os
    assert not os.path.exists(out)


def test_add_scintillation_host():
    port = np.arange(12.0).reshape(4, 3)
    assert pplib.add_scintillation(port, params=None, random=False) is port
    got = pplib.add_scintillation(port, [0.5, 2.0, 0.25])
    pat = 0.5 * np.sin(np.linspace(0, 2.0 * np.pi, 4) + 0.25 * np.pi) ** 2
    np.testing.assert_array_equal(got, (port.T * pat).T)
    np.testing.assert_allclose(
        pplib.add_scintillation(F.Z["fn__port"], list(F.Z["fn__scint_params"])),
        F.Z["fn__scint"], rtol=1e-15)


def test_write_psrfits_rows_round_trip(tmp_path):
    """The byte path writes what write_psrfits writes for the same integers."""
    rng = np.random.default_rng(0)
    nsub, npol, nchan, nbin = 2, 4, 3, 32
    q = rng.integers(-32768, 32768, size=(nsub, npol, nchan, nbin)).astype(np.int16)
    scl = rng.uniform(0.5, 2.0, (nsub, npol * nchan)).astype(np.float32)
    offs = rng.normal(size=(nsub, npol * nchan)).astype(np.float32)
    freqs = np.tile(np.linspace(1200.0, 1800.0, nchan), (nsub, 1))
    wts = np.ones((nsub, nchan))
    P, osub, ts = np.full(nsub, 0.003), np.array([5.0, 15.0]), np.full(nsub, 10.0)
    a, b = str(tmp_path / "a.fits"), str(tmp_path / "b.fits")
    psrfits.write_psrfits(a, q, scl, offs, freqs, wts, P, osub, ts, npol=npol,
                          pol_type="IQUV", dm=3.5)
    raw = q.astype(">i2").view(np.uint8).reshape(nsub, -1)
    psrfits.write_psrfits_rows(b, raw, scl, offs, freqs, wts, P, osub, ts, nbin,
                               npol=npol, pol_type="IQUV", dm=3.5,
                               obsfreq=1490.0, obsbw=900.0, ra="01:02:03",
                               dec="-04:05:06")
    fa, fb = psrfits.PSRFITS(a), psrfits.PSRFITS(b)
    try:
        for name in ("TSUBINT", "OFFS_SUB", "PERIOD", "DAT_FREQ", "DAT_WTS",
                     "DAT_OFFS", "DAT_SCL", "DATA"):
            np.testing.assert_array_equal(fa.subint.column(name),
                                          fb.subint.column(name), err_msg=name)
        assert fb.primary["OBSFREQ"] == 1490.0 and fb.primary["OBSBW"] == 900.0
        assert fb.primary["RA"].strip() == "01:02:03"
        assert fb.primary["DEC"].strip() == "-04:05:06"
        assert fb.pol_type == "IQUV" and fb.subint.header["DM"] == 3.5
    finally:
        fa.close()
        fb.close()
    with pytest.raises(ValueError):
        psrfits.write_psrfits_rows(b, raw[:, :-2], scl, offs, freqs, wts, P,
                                   osub, ts, nbin, npol=npol)
