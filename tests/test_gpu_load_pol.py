"""psrfits.load_data on four-polarisation files, polarised: IQUV and AABBCRCI
files of float32 and 16-bit samples written by pplib.write_archive (2 x 4 x 17
x 64, one zero-weight channel), loaded as Stokes, as Coherence and as stored.
Polarisation 0 against the total-intensity load of the same file (bitwise),
the others against psrfits.unpack_host_pol and the baseline restatement of
tests/unpackpolcases.py, to the bars of test_gpu_unpack._check."""
import os

import numpy as np
import pytest

import unpackpolcases as UP
from test_gpu_unpack import _bits, _check

pytestmark = pytest.mark.gpu

PAR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                   "example.par")
NSUB, NCHAN, NBIN = 2, 17, 64
ZAP = 5
FILES = [("IQUV", "E"), ("IQUV", "I"), ("AABBCRCI", "E"), ("AABBCRCI", "I")]
STATE = {"IQUV": "Stokes", "AABBCRCI": "Coherence"}


def _write(tmp, pol_type, elem, fd_poln=None):
    """(file name, weights): four polarisations of distinct baselines and
    pulse amplitudes (unpackpolcases._values)."""
    from pulseportraiture_amd import pplib
    rng = np.random.default_rng(31)
    data = UP._values(rng, NSUB, NCHAN, NBIN).astype(np.float32)
    w = np.ones((NSUB, NCHAN))
    w[:, ZAP] = 0.0
    fn = os.path.join(str(tmp), "%s_%s_%s.fits" % (pol_type, elem, fd_poln))
    pplib.write_archive(data, PAR, np.linspace(1100.0, 1900.0, NCHAN),
                        outfile=fn, tsub=10.0, weights=w,
                        state=STATE[pol_type], quiet=True, elem=elem,
                        fd_poln=fd_poln)
    return fn, w


def _restated(fn, conv, wts):
    """The file's DATA through psrfits.unpack_host_pol and the baseline
    restatement."""
    from pulseportraiture_amd import psrfits as PF
    f = PF.PSRFITS(fn)
    raw, dt = f.data_bytes()
    scl, offs = f.scales_offsets()
    rows = PF.unpack_host_pol(np.array(raw), dt, scl, offs, f.nchan, f.nbin,
                              conv)
    f.close()
    return UP.restate(rows, conv, wts.astype(np.float32))


def _check_bunch(d, r, rm):
    """A polarised DataBunch against the restatement r: rows and S/N by
    test_gpu_unpack._check's bars, noise_stds = get_noise per profile."""
    from pulseportraiture_amd import pplib
    rows = np.asarray(d.subints)
    c = dict(nsub=d.nsub, nchan=4 * d.nchan)
    # (_check reads the mean and sigma too: the bunch carries the S/N only)
    stats = np.array(r["stats"])
    stats[..., 2] = d.SNRs
    got = UP.flatten(dict(rows=rows, stats=stats, total=r["total"],
                          wstart=r["wstart"]))
    _check(c, UP.flatten(r), got, rm)
    np.testing.assert_allclose(d.SNRs, r["stats"][..., 2], rtol=1e-9, atol=0)
    for s in range(d.nsub):
        for p in range(4):
            np.testing.assert_allclose(
                d.noise_stds[s, p],
                pplib.get_noise(rows[s, p].astype(float), chans=True),
                rtol=1e-9)


@pytest.mark.parametrize("pol_type,elem", FILES)
def test_stokes_load(tmp_path, pol_type, elem):
    from pulseportraiture_amd import psrfits as PF
    fn, w = _write(tmp_path, pol_type, elem)
    conv = 0 if pol_type == "IQUV" else 2
    r = _restated(fn, conv, w)
    for rm in (False, True):
        d = PF.load_data(fn, state="Stokes", pscrunch=False, rm_baseline=rm,
                         quiet=True)
        one = PF.load_data(fn, pscrunch=True, rm_baseline=rm, quiet=True)
        assert (d.npol, d.state, d.nsub, d.nchan, d.nbin) == \
            (4, "Stokes", NSUB, NCHAN, NBIN)
        assert d.fd_poln == "LIN" and one.npol == 1
        assert d.subints.shape == d.masks.shape == (NSUB, 4, NCHAN, NBIN)
        assert d.subints.device_rows.shape == (NSUB, 4, NCHAN, NBIN)
        assert d.noise_stds.shape == d.SNRs.shape == (NSUB, 4, NCHAN)
        rows = np.asarray(d.subints)
        assert rows.shape == (NSUB, 4, NCHAN, NBIN)
        # pol 0 is the total-intensity load, bit for bit
        np.testing.assert_array_equal(_bits(rows[:, 0]),
                                      _bits(np.asarray(one.subints)[:, 0]))
        np.testing.assert_array_equal(d.SNRs[:, 0], one.SNRs[:, 0])
        np.testing.assert_array_equal(d.noise_stds[:, 0],
                                      one.noise_stds[:, 0])
        np.testing.assert_allclose(d.prof, one.prof, rtol=1e-12)
        assert d.prof_SNR == pytest.approx(one.prof_SNR, rel=1e-9)
        np.testing.assert_array_equal(np.asarray(d.masks)[:, 2],
                                      np.asarray(one.masks)[:, 0])
        np.testing.assert_array_equal(d.masks[1, 3], one.masks[1, 0])
        np.testing.assert_array_equal(d.weights, w)
        _check_bunch(d, r, rm)


def test_state_none_keeps_the_files_state(tmp_path):
    from pulseportraiture_amd import psrfits as PF
    for pol_type, conv in (("IQUV", 0), ("AABBCRCI", 1)):
        fn, w = _write(tmp_path, pol_type, "I")
        r = _restated(fn, conv, w)
        for state in (None, STATE[pol_type]):
            d = PF.load_data(fn, state=state, pscrunch=False,
                             rm_baseline=False, quiet=True)
            assert d.state == STATE[pol_type] and d.npol == 4
            _check_bunch(d, r, False)
        d = PF.load_data(fn, pscrunch=False, quiet=True)
        _check_bunch(d, r, True)


def test_conversions_land_in_the_right_slots(tmp_path):
    """Stokes -> Coherence on an IQUV file; Coherence -> Stokes on files of
    linear and circular feeds: Q, U, V of the circular one are U, V, Q of
    the linear one."""
    from pulseportraiture_amd import psrfits as PF
    kw = dict(pscrunch=False, rm_baseline=False, quiet=True)
    fn, w = _write(tmp_path, "IQUV", "E")
    d = PF.load_data(fn, state="Coherence", **kw)
    assert d.state == "Coherence"
    s = np.asarray(PF.load_data(fn, state="Stokes", **kw).subints)
    h = np.float32(0.5)
    want = np.stack([h * (s[:, 0] + s[:, 1]), h * (s[:, 0] - s[:, 1]),
                     h * s[:, 2], h * s[:, 3]], axis=1)
    np.testing.assert_array_equal(_bits(np.asarray(d.subints)), _bits(want))
    _check_bunch(d, _restated(fn, 4, w), False)
    fc, _ = _write(tmp_path, "IQUV", "E", fd_poln="CIRC")
    d = PF.load_data(fc, state="Coherence", **kw)
    assert d.fd_poln == "CIRC"
    want = np.stack([h * (s[:, 0] + s[:, 3]), h * (s[:, 0] - s[:, 3]),
                     h * s[:, 1], h * s[:, 2]], axis=1)
    np.testing.assert_array_equal(_bits(np.asarray(d.subints)), _bits(want))
    _check_bunch(d, _restated(fc, 5, w), False)
    # coherence files: the same samples under the two feed bases
    fl, _ = _write(tmp_path, "AABBCRCI", "I", fd_poln="LIN")
    fc, _ = _write(tmp_path, "AABBCRCI", "I", fd_poln="CIRC")
    lin = PF.load_data(fl, state="Stokes", **kw)
    circ = PF.load_data(fc, state="Stokes", **kw)
    assert (lin.fd_poln, circ.fd_poln) == ("LIN", "CIRC")
    assert lin.state == circ.state == "Stokes"
    a, b = np.asarray(lin.subints), np.asarray(circ.subints)
    coh = np.asarray(PF.load_data(fl, state="Coherence", **kw).subints)
    np.testing.assert_array_equal(_bits(a[:, 1]), _bits(coh[:, 0] - coh[:, 1]))
    np.testing.assert_array_equal(_bits(a[:, 3]),
                                  _bits(np.float32(2) * coh[:, 3]))
    for p_circ, p_lin in ((0, 0), (1, 2), (2, 3), (3, 1)):
        np.testing.assert_array_equal(_bits(b[:, p_circ]), _bits(a[:, p_lin]))
    assert not np.array_equal(a[:, 1], b[:, 1])
    _check_bunch(circ, _restated(fc, 3, w), False)
    # kept, the feed basis does not matter
    np.testing.assert_array_equal(
        _bits(np.asarray(PF.load_data(fc, state="Coherence", **kw).subints)),
        _bits(coh))


@pytest.mark.parametrize("pol_type", ["IQUV", "AABBCRCI"])
def test_dedisperse_tscrunch(tmp_path, pol_type):
    """dedisperse + tscrunch of a polarised load: pol 0 is the intensity
    path's result; every pol is pplib.rotate_data of the loaded rows, the
    baseline of the total intensity's window removed, and the weighted mean
    over the sub-ints (test_psrfits._check_dedisperse_tscrunch's bars)."""
    from pulseportraiture_amd import pplib, psrfits as PF
    fn, w = _write(tmp_path, pol_type, "I")
    kw = dict(rm_baseline=True, dedisperse=True, tscrunch=True, quiet=True)
    both = PF.load_data(fn, state="Stokes", pscrunch=False, **kw)
    one = PF.load_data(fn, pscrunch=True, **kw)
    assert (both.nsub, both.npol, both.dmc, both.state) == (1, 4, 1, "Stokes")
    assert both.subints.shape == both.masks.shape == (1, 4, NCHAN, NBIN)
    assert both.SNRs.shape == both.noise_stds.shape == (1, 4, NCHAN)
    got = np.asarray(both.subints)
    ref0 = np.asarray(one.subints)[0, 0]
    np.testing.assert_allclose(
        got[0, 0], ref0, rtol=0,
        atol=2 * np.spacing(np.float32(np.abs(ref0).max())))
    np.testing.assert_array_equal(both.weights, one.weights)
    assert both.epochs[0].in_days() == one.epochs[0].in_days()
    # the host side of the API on the loaded rows
    base = PF.load_data(fn, state="Stokes", pscrunch=False,
                        rm_baseline=False, quiet=True)
    U4 = np.asarray(base.subints)
    wts = base.weights
    assert base.DM != 0.0
    R = pplib.rotate_data(U4, 0.0, base.DM, base.Ps, base.freqs,
                          base.nu0).astype(np.float32)
    r = UP.restate(R, 0, wts.astype(np.float32))
    Rb = r["removed"]
    dd = PF.load_data(fn, state="Stokes", pscrunch=False, rm_baseline=True,
                      dedisperse=True, quiet=True)
    np.testing.assert_allclose(
        np.asarray(dd.subints), Rb, rtol=0,
        atol=2 * np.spacing(np.float32(np.abs(Rb).max())))
    np.testing.assert_allclose(dd.SNRs, r["stats"][..., 2], rtol=1e-6)
    wsum = wts.sum(axis=0)
    mb = (wts[:, None, :, None] * Rb.astype(float)).sum(axis=0) / \
        np.where(wsum > 0, wsum, 1.0)[None, :, None]
    for p in range(4):
        np.testing.assert_allclose(
            got[0, p], mb[p].astype(np.float32), rtol=0,
            atol=4 * np.spacing(np.float32(np.abs(mb[p]).max())))
        np.testing.assert_allclose(
            both.noise_stds[0, p],
            pplib.get_noise(got[0, p].astype(float), chans=True), rtol=1e-9)
    # tscrunch alone
    ts = PF.load_data(fn, state="Stokes", pscrunch=False, rm_baseline=False,
                      tscrunch=True, quiet=True)
    mean = (wts[:, None, :, None] * U4.astype(float)).sum(axis=0) / \
        np.where(wsum > 0, wsum, 1.0)[None, :, None]
    np.testing.assert_allclose(
        np.asarray(ts.subints)[0], mean.astype(np.float32), rtol=0,
        atol=4 * np.spacing(np.float32(np.abs(mean).max())))


def test_pscrunch_loads_keep_their_path(tmp_path, monkeypatch):
    """pscrunch=True (whatever the state) and state="Intensity" still go
    through engine.unpack_psrfits; the polarised wrapper is not called."""
    from pulseportraiture_amd import engine, psrfits as PF
    seen = []
    real, real_pol = engine.unpack_psrfits, engine.unpack_psrfits_pol

    def spy(*a, **k):
        seen.append("one")
        return real(*a, **k)

    def spy_pol(*a, **k):
        seen.append("pol")
        return real_pol(*a, **k)

    monkeypatch.setattr(engine, "unpack_psrfits", spy)
    monkeypatch.setattr(engine, "unpack_psrfits_pol", spy_pol)
    fn, _ = _write(tmp_path, "AABBCRCI", "I")
    ref = PF.load_data(fn, pscrunch=True, quiet=True)
    for kw in (dict(state="Stokes", pscrunch=True),
               dict(state="Coherence", pscrunch=True),
               dict(state="Intensity", pscrunch=False),
               dict(state="Intensity", pscrunch=True)):
        d = PF.load_data(fn, quiet=True, **kw)
        assert (d.npol, d.state) == (1, "Intensity")
        np.testing.assert_array_equal(_bits(np.asarray(d.subints)),
                                      _bits(np.asarray(ref.subints)))
    assert seen == ["one"] * 5
    PF.load_data(fn, state="Stokes", pscrunch=False, quiet=True)
    assert seen == ["one"] * 5 + ["pol"]
