"""CPU: the host side of the PSRFITS pack path.  ppf_pack_psrfits_batch
validates its arguments before it looks at the context or launches anything,
and the archive writers (pplib.write_archive, pplib.unload_new_archive) refuse
what they cannot write -- dedispersed output, non-finite samples, a shape that
disagrees with the archive -- before they touch the device."""
import ctypes
import os

import numpy as np
import pytest

from pulseportraiture_amd import _lib, pplib, psrfits

HERE = os.path.dirname(os.path.abspath(__file__))
PAR = os.path.join(HERE, "golden", "example.par")


def _call(lib, nrow=1, nbin=64, in_dtype=_lib.PPF_F64, elem=0, ctx=None,
          rows=8, raw=8, scl=8, offs=8):
    # the pointers are never dereferenced: no context, no launch
    def p(v):
        return None if v is None else ctypes.c_void_p(v)
    return lib.ppf_pack_psrfits_batch(ctx, nrow, nbin, in_dtype, p(rows),
                                      elem, p(raw), p(scl), p(offs), None)


def test_pack_entry_refuses_bad_arguments_on_the_host():
    lib = _lib.load()
    # a valid call stops at the NULL context
    assert _call(lib) == _lib.PPF_EINVAL
    assert _call(lib, nrow=-1) == _lib.PPF_EINVAL
    assert _call(lib, nbin=0) == _lib.PPF_EINVAL
    assert _call(lib, nbin=-5) == _lib.PPF_EINVAL
    for elem in (-1, 1, 3, 4):           # uint8 and native rows: unpack only
        assert _call(lib, elem=elem) == _lib.PPF_EINVAL, elem
    for dt in (-1, 2, 7):
        assert _call(lib, in_dtype=dt) == _lib.PPF_EINVAL, dt
    # the bad scalars are refused whatever else is wrong, empty batch included
    assert _call(lib, nrow=0, nbin=0) == _lib.PPF_EINVAL
    assert _call(lib, nrow=0, elem=1) == _lib.PPF_EINVAL
    assert _call(lib, nrow=0, in_dtype=5) == _lib.PPF_EINVAL
    # a byte count past int64
    assert _call(lib, nrow=2 ** 62, nbin=2 ** 30) == _lib.PPF_EINVAL
    for name in ("rows", "raw", "scl", "offs"):
        assert _call(lib, **{name: None}) == _lib.PPF_EINVAL, name


def test_pack_entry_empty_batch_is_ok():
    lib = _lib.load()
    for elem in (0, 2):
        for dt in (_lib.PPF_F32, _lib.PPF_F64):
            assert _call(lib, nrow=0, elem=elem, in_dtype=dt) == _lib.PPF_OK
    assert _call(lib, nrow=0, nbin=1, rows=None, raw=None, scl=None,
                 offs=None) == _lib.PPF_OK


def _data(nsub=2, npol=1, nchan=4, nbin=32):
    return np.random.default_rng(5).normal(size=(nsub, npol, nchan, nbin))


def test_write_archive_refusals(tmp_path):
    out = str(tmp_path / "w.fits")
    freqs = np.linspace(1200.0, 1500.0, 4)
    with pytest.raises(NotImplementedError):
        pplib.write_archive(_data(), PAR, freqs, outfile=out, dedispersed=True)
    for bad in (np.nan, np.inf, -np.inf):
        x = _data()
        x[1, 0, 2, 7] = bad
        with pytest.raises(ValueError):
            pplib.write_archive(x, PAR, freqs, outfile=out)
        with pytest.raises(ValueError):
            pplib.write_archive(x.astype(np.float32), PAR, freqs, outfile=out)
    with pytest.raises(ValueError):
        pplib.write_archive(_data()[0], PAR, freqs, outfile=out)     # 3-D
    with pytest.raises(ValueError):
        pplib.write_archive(_data(), PAR, freqs[:3], outfile=out)
    with pytest.raises(ValueError):
        pplib.write_archive(_data(), PAR, freqs, outfile=out,
                            weights=np.ones((2, 3)))
    with pytest.raises(ValueError):
        pplib.write_archive(_data(nchan=1), PAR, freqs[:1], outfile=out)  # bw
    with pytest.raises(NotImplementedError):
        pplib.write_archive(_data(npol=2), PAR, freqs, outfile=out)
    with pytest.raises(NotImplementedError):
        pplib.write_archive(_data(npol=4), PAR, freqs, outfile=out,
                            state="Intensity")
    with pytest.raises(ValueError):
        psrfits.write_archive_rows(out, _data(), np.tile(freqs, (2, 1)),
                                   np.ones((2, 4)), np.ones(2), np.zeros(2),
                                   np.ones(2), elem="B")
    assert not os.path.exists(out)


@pytest.fixture()
def archive(tmp_path):
    """A 2 x 1 x 4 x 32 file written on the host."""
    nsub, nchan, nbin = 2, 4, 32
    q, scl, offs = psrfits.quantize(_data())
    name = str(tmp_path / "a.fits")
    psrfits.write_psrfits(name, q, scl, offs,
                          np.tile(np.linspace(1200.0, 1500.0, nchan),
                                  (nsub, 1)),
                          np.ones((nsub, nchan)), np.full(nsub, 0.003),
                          np.array([5.0, 15.0]), np.full(nsub, 10.0),
                          dm=12.5, telescope="PKS", source="J0437-4715")
    return name


def test_archive_meta_reads_the_file_without_a_device(archive):
    m = psrfits.archive_meta(archive)
    assert (m["nsub"], m["npol"], m["nchan"], m["nbin"]) == (2, 1, 4, 32)
    assert m["telescope"] == "PKS" and m["source"] == "J0437-4715"
    assert m["DM"] == 12.5 and m["pol_type"] == "AA+BB"
    np.testing.assert_array_equal(m["Ps"], [0.003, 0.003])
    np.testing.assert_array_equal(m["subtimes"], [10.0, 10.0])
    assert m["freqs"].shape == (2, 4) and m["weights"].shape == (2, 4)
    d = (m["epochs"][1].in_days() - m["epochs"][0].in_days()) * 86400.0
    assert abs(d - 10.0) < 1e-4


def test_unload_new_archive_refusals(archive, tmp_path):
    out = str(tmp_path / "u.fits")
    x = _data()
    for dmc in (1, True):
        with pytest.raises(NotImplementedError):
            pplib.unload_new_archive(x, archive, out, dmc=dmc)
    for shape in ((1, 1, 4, 32), (2, 1, 4, 64), (2, 1, 3, 32), (2, 2, 4, 32)):
        with pytest.raises(ValueError):
            pplib.unload_new_archive(np.zeros(shape), archive, out)
    with pytest.raises(ValueError):
        pplib.unload_new_archive(x[0], archive, out)
    with pytest.raises(ValueError):
        pplib.unload_new_archive(x, archive, out, weights=np.ones((1, 4)))
    bad = x.copy()
    bad[0, 0, 0, 0] = np.nan
    with pytest.raises(ValueError):
        pplib.unload_new_archive(bad, archive, out)
    # a DataBunch stands in for the archive as well
    bunch = pplib.DataBunch(**psrfits.archive_meta(archive))
    with pytest.raises(ValueError):
        pplib.unload_new_archive(np.zeros((2, 1, 4, 16)), bunch, out)
    with pytest.raises(NotImplementedError):
        pplib.unload_new_archive(x, bunch, out, dmc=1)
    assert not os.path.exists(out)
