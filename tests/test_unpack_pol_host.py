"""CPU: the host side of full-polarisation PSRFITS loading.  The NumPy
restatement of the device's polarised unpack (psrfits.unpack_host_pol)
against hand-written formulas, the FD_POLN card, load_data's refusals (all
raised while the file is parsed: no device) and the inputs of the polarised
ppalign golden.  The device side: tests/test_gpu_unpack_pol.py,
tests/test_gpu_load_pol.py, tests/test_gpu_align_pol.py."""
import os

import numpy as np
import pytest

import alignpolcases as AP
import unpackcases as U
import unpackpolcases as UP
from pulseportraiture_amd import psrfits as PF

SHAPE = (2, 4, 3, 10)


def _samples(elem, seed=5):
    rng = np.random.default_rng(seed)
    nsub, _, nchan, nbin = SHAPE
    if elem == 0:
        x = rng.integers(-32768, 32768, SHAPE).astype(np.int16)
    elif elem == 1:
        x = rng.integers(0, 256, SHAPE).astype(np.uint8)
    else:
        x = rng.normal(0, 30.0, SHAPE).astype(np.float32)
    scl = rng.uniform(0.5, 1.5, (nsub, 4 * nchan)).astype(np.float32)
    offs = rng.uniform(20.0, 60.0, (nsub, 4 * nchan)).astype(np.float32)
    raw = np.ascontiguousarray(x.astype(U.DT[elem])).view(np.uint8)
    return x, raw.reshape(nsub, -1), scl, offs


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("elem", [0, 1, 2])
def test_unpack_host_pol_formulas(elem):
    """All six conv values on the three file sample types: every output is
    the hand-written float32 formula of the four twice-rounded values."""
    nsub, _, nchan, nbin = SHAPE
    x, raw, scl, offs = _samples(elem)
    f = np.float32
    v = (x.astype(f) * scl.reshape(nsub, 4, nchan, 1)).astype(f) + \
        offs.reshape(nsub, 4, nchan, 1)
    assert v.dtype == f
    a, b, c, d = (v[:, p] for p in range(4))
    want = {0: (a, b, c, d), 1: (a, b, c, d),
            2: (a + b, a - b, f(2) * c, f(2) * d),
            3: (a + b, f(2) * c, f(2) * d, a - b),
            4: (f(.5) * (a + b), f(.5) * (a - b), f(.5) * c, f(.5) * d),
            5: (f(.5) * (a + d), f(.5) * (a - d), f(.5) * b, f(.5) * c)}
    for conv in range(6):
        got = PF.unpack_host_pol(raw, U.DT[elem], scl, offs, nchan, nbin,
                                 conv)
        assert got.shape == SHAPE and got.dtype == f
        for p in range(4):
            assert want[conv][p].dtype == f
            np.testing.assert_array_equal(_bits(got[:, p]),
                                          _bits(want[conv][p]),
                                          err_msg="conv %d pol %d" % (conv, p))
    with pytest.raises(ValueError):
        PF.unpack_host_pol(raw, U.DT[elem], scl, offs, nchan, nbin, 6)


@pytest.mark.parametrize("elem", [0, 1, 2])
def test_unpack_host_pol_pol0_is_the_intensity_restatement(elem):
    """conv 2 pol 0 is unpack_host's AA + BB, conv 0 pol 0 its I, bitwise;
    the window's total intensity is pol 0, or pol 0 + pol 1 of a Coherence
    output."""
    nsub, _, nchan, nbin = SHAPE
    x, raw, scl, offs = _samples(elem, seed=6)
    n2 = 2 * nchan * nbin * x.dtype.itemsize
    s4, o4 = scl.reshape(nsub, 4, nchan), offs.reshape(nsub, 4, nchan)
    aabb = PF.unpack_host(raw[:, :n2], U.DT[elem], s4[:, :2], o4[:, :2], 2,
                          nchan, nbin)
    i = PF.unpack_host(raw[:, :n2 // 2], U.DT[elem], s4[:, :1], o4[:, :1], 1,
                       nchan, nbin)
    for conv, ref in ((2, aabb), (3, aabb), (0, i), (1, i)):
        got = PF.unpack_host_pol(raw, U.DT[elem], scl, offs, nchan, nbin,
                                 conv)
        np.testing.assert_array_equal(_bits(got[:, 0]), _bits(ref))
    for conv in range(6):
        got = PF.unpack_host_pol(raw, U.DT[elem], scl, offs, nchan, nbin,
                                 conv)
        t = PF.total_intensity_host(got, conv)
        ref = got[:, 0] + got[:, 1] if conv in (1, 4, 5) else got[:, 0]
        np.testing.assert_array_equal(_bits(t), _bits(ref))
    # Coherence kept: its total is the intensity path's AA + BB
    got = PF.unpack_host_pol(raw, U.DT[elem], scl, offs, nchan, nbin, 1)
    np.testing.assert_array_equal(_bits(PF.total_intensity_host(got, 1)),
                                  _bits(aabb))


def test_pol_conv_table():
    assert PF.pol_conv("Stokes", None) == PF.pol_conv("Stokes", "Stokes") == 0
    assert PF.pol_conv("Coherence", None, "CIRC") == 1
    assert PF.pol_conv("Coherence", "Coherence") == 1
    assert PF.pol_conv("Coherence", "Stokes", "LIN") == 2
    assert PF.pol_conv("Coherence", "Stokes", "CIRC") == 3
    assert PF.pol_conv("Stokes", "Coherence", "LIN") == 4
    assert PF.pol_conv("Stokes", "Coherence", "CIRC") == 5


@pytest.mark.parametrize("name", UP.CASE_NAMES)
def test_device_cases_meet_their_bars(name):
    """Every case of the device test builds, has a window minimum clear of
    rounding and no compared row with an off-pulse mean within one sigma of
    zero (asserted by reference()); only finite rows are compared."""
    c, r = UP.case(name), UP.reference(name)
    assert r["rows"].shape == (c["nsub"], 4, c["nchan"], c["nbin"])
    assert np.isfinite(r["rows"][UP.live(c)]).all()
    assert np.isfinite(r["total"]).all()
    es = np.dtype(U.DT[c["elem"]]).itemsize
    assert c["raw"].shape[1] == 4 * c["nchan"] * c["nbin"] * es + c["pad"]
    if c["pad"]:                         # whole elements, not 8 bytes
        assert c["raw"].shape[1] % es == 0 and c["raw"].shape[1] % 8


# ---------------------------------------------------------------- FD_POLN --
def _write(path, npol=4, pol_type="IQUV", **kw):
    nsub, nchan, nbin = 2, 3, 16
    rng = np.random.default_rng(1)
    q, scl, offs = PF.quantize(rng.normal(5.0, 1.0, (nsub, npol, nchan, nbin)))
    PF.write_psrfits(path, q, scl, offs,
                     np.tile(np.linspace(1100.0, 1900.0, nchan), (nsub, 1)),
                     np.ones((nsub, nchan)), np.full(nsub, 0.00289),
                     5.0 + 10.0 * np.arange(nsub), np.full(nsub, 10.0),
                     npol=npol, pol_type=pol_type, dm=12.5, **kw)
    return path


def test_fd_poln_card(tmp_path):
    plain = _write(str(tmp_path / "plain.fits"))
    none = _write(str(tmp_path / "none.fits"), fd_poln=None)
    circ = _write(str(tmp_path / "circ.fits"), fd_poln="CIRC")
    lin = _write(str(tmp_path / "lin.fits"), fd_poln="LIN")
    # no keyword, or None: the bytes written before the card existed
    assert open(plain, "rb").read() == open(none, "rb").read()
    assert b"FD_POLN" not in open(plain, "rb").read()
    assert open(circ, "rb").read() != open(plain, "rb").read()
    for fn, want in ((plain, "LIN"), (circ, "CIRC"), (lin, "LIN")):
        f = PF.PSRFITS(fn)
        assert f.fd_poln == want
        assert f.primary.get("FD_POLN") == (None if fn == plain else want)
        f.close()
        assert PF.archive_meta(fn)["fd_poln"] == want
    with pytest.raises(ValueError):
        _write(str(tmp_path / "bad.fits"), fd_poln="XY")


# ---------------------------------------------------------------- refusals --
def test_load_data_refusals_need_no_device(tmp_path, monkeypatch):
    """Every refusal is raised while the file is parsed: engine.device is
    never asked for."""
    from pulseportraiture_amd import engine

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(engine, "device", no_device)
    one = _write(str(tmp_path / "one.fits"), npol=1, pol_type="AA+BB")
    for state in ("Stokes", "Coherence"):
        with pytest.raises(IndexError):
            PF.load_data(one, state=state, pscrunch=False, quiet=True)
    other = _write(str(tmp_path / "other.fits"), pol_type="XXYYCRCI")
    for state in (None, "Stokes", "Coherence"):
        with pytest.raises(NotImplementedError):
            PF.load_data(other, state=state, pscrunch=False, quiet=True)
    four = _write(str(tmp_path / "four.fits"))
    with pytest.raises(NotImplementedError):
        PF.load_data(four, state="Stokes", pscrunch=False, fscrunch=True)
    with pytest.raises(NotImplementedError):
        PF.load_data(four, state="PPQQ", pscrunch=False)
    two = _write(str(tmp_path / "two.fits"), npol=2, pol_type="AABB")
    for kw in (dict(state="Stokes", pscrunch=False), dict(pscrunch=False),
               dict(state="Coherence", pscrunch=True)):
        with pytest.raises(NotImplementedError):
            PF.load_data(two, quiet=True, **kw)


def test_masks_and_rows_polarisation_axis():
    wn = np.array([[1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
    m1, m4 = PF._Masks(wn, 5), PF._Masks(wn, 5, npol=4)
    assert m1.shape == (2, 1, 3, 5) and m4.shape == (2, 4, 3, 5)
    full = np.asarray(m4)
    assert full.shape == m4.shape
    for p in range(4):
        np.testing.assert_array_equal(full[:, p], np.asarray(m1)[:, 0])
        np.testing.assert_array_equal(m4[1, p], np.asarray(m1)[1, 0])
    np.testing.assert_array_equal(m4[0, 1:3], full[0, 1:3])


# ------------------------------------------------------------------ golden --
def test_align_pol_golden_inputs_rebuild():
    """tests/golden/align_pol.npz holds what make_golden_align_pol.py says:
    pols 1..3 of every file are c_p I + noise from the script's seed, exact
    in float32; the guess is c_p times its pol 0; one file has zapped
    channels; the recorded DM is 0."""
    c = AP.golden()
    shape = (int(c["nsub"]), 4, int(c["nchan"]), int(c["nbin"]))
    assert (int(c["nfile"]),) + shape == (3, 2, 4, 17, 64)
    assert int(c["niter"]) == 2 and tuple(c["coeff"]) == AP.COEFF
    files, guess = AP.rebuilt_pols(c)
    for i, pols in enumerate(files):
        sub = c["f%d_subints" % i]
        assert sub.shape == shape and sub.dtype == np.float32
        np.testing.assert_array_equal(_bits(sub[:, 1:]), _bits(pols))
    np.testing.assert_array_equal(c["guess"], guess)
    zapped = [int((c["f%d_weights" % i] == 0).any()) for i in range(3)]
    assert sum(zapped) == 1
    assert c["out_aligned"].shape == shape[1:] and float(c["out_dm"]) == 0.0
    assert set(np.unique(c["out_weights"])) <= {0.0, 1.0}
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden",
                                        "align_pol.npz")) < 256 * 1024
    archives, model = AP.inputs(c)
    assert archives[0].subints.shape == shape and model.subints.shape == \
        (1,) + shape[1:]
