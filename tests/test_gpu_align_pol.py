"""ppalign.align_archives(pscrunch=False), the reference's "average Stokes
portraits": against the reference's own output on four-polarisation
DataBunches (tests/golden/align_pol.npz), and from IQUV PSRFITS files with a
PSRFITS template, where it writes a four-polarisation .algnd.fits.

The bar is the project's align bar per polarisation, 1e-6 of max |ref[pol]|:
a phase error moves each polarisation in proportion to its own amplitude."""
import os

import numpy as np
import pytest

import alignpolcases as AP
import goldens as G

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


class _Profile(object):
    def __init__(self, store, ipol, ichan):
        self.store, self.ipol, self.ichan = store, ipol, ichan

    def get_amps(self):
        return self.store[self.ipol, self.ichan]


class _Subint(object):
    def __init__(self, arch):
        self.arch = arch

    def get_Profile(self, ipol, ichan):
        return _Profile(self.arch.amps, ipol, ichan)

    def set_weight(self, ichan, w):
        self.arch.weights[ichan] = w


class _Arch(object):
    """The PSRCHIVE calls of ppalign.py:259-277 on a four-polarisation
    archive, recorded."""

    def __init__(self, nchan, nbin):
        self.amps = np.zeros((4, nchan, nbin))
        self.weights = np.full(nchan, -1.0)
        self.dm = self.outfile = self.state = None

    def tscrunch(self):
        pass

    def pscrunch(self):
        raise AssertionError("pscrunch() on a polarised alignment")

    def convert_state(self, state):
        self.state = state

    def set_dispersion_measure(self, dm):
        self.dm = dm

    def get_npol(self):
        return 4

    def get_nchan(self):
        return self.amps.shape[1]

    def __iter__(self):
        return iter([_Subint(self)])

    def unload(self, outfile):
        self.outfile = outfile


def _assert_per_pol(got, ref, what=""):
    for p in range(4):
        np.testing.assert_allclose(
            got[p], ref[p], rtol=0, atol=1e-6 * np.abs(ref[p]).max(),
            err_msg="%s pol %d" % (what, p))


def test_align_pol_matches_reference(monkeypatch):
    """3 files x 2 sub-ints x 17 channels x 64 bins, one file with zapped
    channels, 2 iterations: every polarisation of the aligned portrait, the
    channel weights, DM 0 in the recorder."""
    from pulseportraiture_amd import ppalign, pptoas
    c = AP.golden()
    archives, model_data = AP.inputs(c)
    rec = _Arch(int(c["nchan"]), int(c["nbin"]))
    model_data["arch"] = rec
    files = {"arch%d.fits" % i: a for i, a in enumerate(archives)}
    files["guess.fits"] = model_data
    asked = []

    def load(name, **kw):
        asked.append((kw.get("state"), kw.get("pscrunch")))
        return files[name]

    monkeypatch.setattr(pptoas, "load_data", load)
    r = ppalign.align_archives(["arch%d.fits" % i for i in
                                range(int(c["nfile"]))], "guess.fits",
                               fit_dm=True, pscrunch=False,
                               niter=int(c["niter"]), outfile="aligned.fits",
                               quiet=True)
    assert set(asked) == {("Stokes", False)}
    ref = c["out_aligned"]
    assert r.port.shape == ref.shape == (4, int(c["nchan"]), int(c["nbin"]))
    assert r.nsub_fit == int(c["nfile"]) * int(c["nsub"])
    _assert_per_pol(r.port, ref, "returned")
    _assert_per_pol(rec.amps, ref, "recorded")
    np.testing.assert_array_equal(rec.weights, c["out_weights"])
    assert rec.dm == 0.0 and float(c["out_dm"]) == 0.0
    assert rec.state == "Stokes" and rec.outfile == "aligned.fits"


def _host_bunch(d):
    """A loaded DataBunch with its rows and masks handed over as NumPy
    arrays and no file behind it."""
    h = G.Bunch(d)
    h["subints"] = np.array(np.asarray(d.subints))
    h["masks"] = np.array(np.asarray(d.masks))
    h["filename"] = None
    return h


def test_align_pol_from_files(tmp_path, monkeypatch):
    from pulseportraiture_amd import ppalign, pptoas, psrfits as PF
    c = AP.golden()
    nchan, nbin = int(c["nchan"]), int(c["nbin"])
    meta, tmpl = AP.write_files(tmp_path, c)
    r = ppalign.align_archives(meta, tmpl, pscrunch=False,
                               niter=int(c["niter"]), quiet=True)
    assert r.port.shape == (4, nchan, nbin)
    assert r.nsub_fit == int(c["nfile"]) * int(c["nsub"])
    # the same rows handed over as host DataBunches
    names = [ln.strip() for ln in open(meta)]
    files = {n: _host_bunch(PF.load_data(
        n, state="Stokes", pscrunch=False, rm_baseline=ppalign.rm_baseline,
        quiet=True)) for n in names}
    for d in files.values():
        assert d.subints.shape == (int(c["nsub"]), 4, nchan, nbin)
        assert d.state == "Stokes" and d.npol == 4
    files[tmpl] = _host_bunch(PF.load_data(
        tmpl, state="Stokes", pscrunch=False, dedisperse=True, tscrunch=True,
        rm_baseline=True, quiet=True))
    monkeypatch.setattr(pptoas, "load_data", lambda name, **kw: files[name])
    h = ppalign.align_archives(names, tmpl, pscrunch=False,
                               niter=int(c["niter"]), quiet=True)
    _assert_per_pol(r.port, h.port, "files vs host bunches")
    np.testing.assert_array_equal(r.total_weights, h.total_weights)
    # one file has zapped channels, yet every channel got weight
    assert (r.total_weights > 0).all()
    monkeypatch.undo()
    # the written archive
    out = meta + ".algnd.fits"
    assert os.path.isfile(out)
    f = PF.PSRFITS(out)
    assert (f.nsub, f.npol, f.nchan, f.nbin) == (1, 4, nchan, nbin)
    assert f.pol_type == "IQUV"
    assert float(f.subint.header["DM"]) == 0.0
    assert float(f.primary["CHAN_DM"]) == 0.0
    scl, offs = f.scales_offsets()
    f.close()
    s = scl[0].astype(float).reshape(4, nchan, 1)
    o = offs[0].astype(float).reshape(4, nchan, 1)
    bound = 0.5 * s + 2 * EPS32 * (np.abs(o) + 32768 * s)
    back = PF.load_data(out, pscrunch=False, rm_baseline=False, quiet=True)
    assert (back.npol, back.state, back.nsub, back.DM) == (4, "Stokes", 1, 0.0)
    err = np.abs(np.asarray(back.subints)[0].astype(float) - r.port)
    print("\nstored vs returned: max err / bound %.3f" % (err / bound).max())
    assert (err <= bound).all()
    np.testing.assert_array_equal(back.weights[0], np.ones(nchan))
