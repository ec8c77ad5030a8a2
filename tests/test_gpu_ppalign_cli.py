"""GPU: the ppalign command line and what it needs: psradd_archives,
make_constant_portrait, main's three initial-guess routes, -s
(psrsmooth_archive: smart_smooth(search="batched") on the written archive),
the smoothed archive as a pptoas template, DataPortrait.smooth_portrait.

Archives: test_gpu_archive_template.build_archives (3 archives of 2 x 16 x
128, channel 5 given weight 0)."""
import glob
import os

import numpy as np
import pytest

from test_gpu_archive_template import (BW, EPS32, NBIN, NCHAN, NSUB, NU0, PAR,
                                       ZAPPED, build_archives)
from pulseportraiture_amd import pplib, psrfits

pytestmark = pytest.mark.gpu


def stored(fn):
    """(rows [nsub, npol, nchan, nbin] as stored, the round-trip bound of
    every row [nsub, nchan, 1], the loaded bunch) of a written file."""
    f = psrfits.PSRFITS(fn)
    scl, offs = f.scales_offsets()
    f.close()
    s = np.asarray(scl, dtype=float).reshape(-1, NCHAN)[:, :, None]
    o = np.asarray(offs, dtype=float).reshape(-1, NCHAN)[:, :, None]
    bound = 0.5 * s + 2 * EPS32 * (np.abs(o) + 32768 * s)
    d = psrfits.load_data(fn, rm_baseline=False, quiet=True)
    return np.asarray(d.subints).astype(float), bound, d


def same_file(a, b):
    xa, _, da = stored(a)
    xb, _, db = stored(b)
    return np.array_equal(xa, xb) and \
        np.array_equal(da.weights, db.weights) and \
        np.array_equal(da.freqs, db.freqs) and da.DM == db.DM and \
        da.Ps[0] == db.Ps[0]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli")
    files, meta = build_archives(d)
    loads = [psrfits.load_data(f, tscrunch=True, quiet=True) for f in files]
    profs = [psrfits.load_data(f, dedisperse=True, tscrunch=True,
                               pscrunch=True, quiet=True).prof for f in files]
    return dict(dir=str(d), files=files, meta=meta, loads=loads, profs=profs)


@pytest.fixture(scope="module")
def smoothed(world):
    """main -s, run once: (out, out + '.sm')."""
    from pulseportraiture_amd import ppalign
    out = os.path.join(world["dir"], "cli_s.fits")
    ppalign.main(["-M", world["meta"], "-o", out, "--niter", "1", "-s"])
    return out, out + ".sm"


@pytest.mark.parametrize("palign", [False, True])
def test_psradd_archives(world, palign):
    from pulseportraiture_amd import ppalign
    out = os.path.join(world["dir"], "add%d.fits" % palign)
    ppalign.psradd_archives(world["meta"], out, palign=palign)
    X = [np.asarray(d.subints)[0, 0].astype(float) for d in world["loads"]]
    W = [np.asarray(d.weights, dtype=float)[0] for d in world["loads"]]
    profs = world["profs"]
    if palign:
        ph = [pplib.fit_phase_shift(p, profs[0], Ns=NBIN).phase
              for p in profs]
        X = [pplib.rotate_data(x, p) for x, p in zip(X, ph)]
        # what the rotations leave of each archive's shift against the first
        for p, prof in zip(ph, profs):
            left = pplib.fit_phase_shift(pplib.rotate_data(prof, p),
                                         profs[0], Ns=NBIN).phase
            print("phase %.6f, left %.2e rot" % (p, left))
            assert abs(left) < 1.0 / NBIN
        assert max(abs(p) for p in ph) > 1.0 / NBIN    # there was a shift
    wsum = np.sum(W, axis=0)
    want = np.sum([w[:, None] * x for w, x in zip(W, X)], axis=0) / \
        np.where(wsum > 0, wsum, 1.0)[:, None]
    got, bound, d = stored(out)
    assert got.shape == (1, 1, NCHAN, NBIN)
    err = np.abs(got[0, 0] - want)
    print("max err / bound %.3f" % (err / bound[0]).max())
    assert (err <= bound[0]).all()
    assert d.weights[0, ZAPPED] == 0.0 and not got[0, 0, ZAPPED].any()
    assert (np.delete(d.weights[0], ZAPPED) > 0).all()
    assert d.DM == world["loads"][0].DM and d.DM != 0.0
    np.testing.assert_array_equal(d.freqs, world["loads"][0].freqs)


def test_make_constant_portrait(world):
    src = world["files"][0]
    out = os.path.join(world["dir"], "const.fits")
    prof = pplib.gaussian_profile(NBIN, 0.5, 0.05)
    w = np.ones((NSUB, NCHAN))
    w[0, 3] = w[1, 7] = 0.0
    pplib.make_constant_portrait(src, out, profile=prof, DM=3.5, weights=w,
                                 quiet=True)
    got, bound, d = stored(out)
    assert got.shape == (NSUB, 1, NCHAN, NBIN)
    assert (np.abs(got[:, 0] - prof) <= bound.reshape(NSUB, NCHAN, 1)).all()
    assert d.DM == 3.5
    np.testing.assert_array_equal(d.weights, w)
    # profile=None: the archive's own average profile, unit weights
    pplib.make_constant_portrait(src, out, quiet=True)
    got, bound, d = stored(out)
    assert (np.abs(got[:, 0] - world["profs"][0]) <=
            bound.reshape(NSUB, NCHAN, 1)).all()
    assert d.DM == 0.0 and (d.weights == 1.0).all()
    with pytest.raises(AssertionError):
        pplib.make_constant_portrait(src, out, profile=prof[:-2], quiet=True)


def _guess(world, route, fn):
    from pulseportraiture_amd import ppalign
    if route == "add":
        ppalign.psradd_archives(world["meta"], fn)
        return []
    if route == "gauss":
        pplib.make_constant_portrait(
            world["files"][0], fn,
            profile=pplib.gaussian_profile(NBIN, 0.5, 0.05), DM=0.0,
            quiet=True)
        return ["-g", "0.05"]
    one = os.path.join(world["dir"], "one_chan.fits")
    pplib.write_archive(world["profs"][0][None, None, None], PAR,
                        np.array([NU0]), nu0=NU0, bw=BW, outfile=one,
                        tsub=60.0, quiet=True, elem="E")
    pplib.make_constant_portrait(world["files"][0], fn, profile=None, DM=0.0,
                                 quiet=True)
    return ["-I", one]


@pytest.mark.parametrize("route", ["add", "gauss", "one_channel"])
def test_main_is_align_archives_by_hand(world, route, tmp_path, monkeypatch):
    from pulseportraiture_amd import ppalign
    guess = os.path.join(world["dir"], "guess_%s.fits" % route)
    want = os.path.join(world["dir"], "want_%s.fits" % route)
    out = os.path.join(world["dir"], "main_%s.fits" % route)
    args = _guess(world, route, guess)
    ppalign.align_archives(world["meta"], guess, outfile=want, niter=2,
                           quiet=True)
    monkeypatch.chdir(tmp_path)
    ppalign.main(["-M", world["meta"], "-o", out, "--niter", "2"] + args)
    assert same_file(out, want)
    assert glob.glob(os.path.join(world["dir"], "ppalign.*.tmp.fits")) == []
    assert os.listdir(str(tmp_path)) == []
    assert not os.path.exists(out + ".sm")


def test_smooth_option_writes_the_smoothed_archive(world, smoothed):
    out, sm = smoothed
    assert os.path.isfile(sm)
    assert glob.glob(os.path.join(world["dir"], "ppalign.*.tmp.fits")) == []
    rows, _, src = stored(out)
    want = pplib.smart_smooth(rows[0, 0], search="batched",
                              try_nlevels=min(8, 7))
    got, bound, d = stored(sm)
    assert got.shape == (1, 1, NCHAN, NBIN)
    err = np.abs(got[0, 0] - want)
    print("max err / bound %.3f" % (err / bound[0]).max())
    assert (err <= bound[0]).all()
    zero = ~want.any(axis=1)
    assert zero[ZAPPED]
    print("rows the smoother zeroed:", np.where(zero)[0])
    assert (d.weights[0, zero] == 0.0).all()
    np.testing.assert_array_equal(d.weights[0, ~zero], src.weights[0, ~zero])
    assert (d.weights[0, ~zero] > 0).all() and (~zero).any()
    assert d.DM == src.DM
    with pytest.raises(NotImplementedError):
        from pulseportraiture_amd import ppalign
        ppalign.psrsmooth_archive(out, options="-W -n 3")


def test_smoothed_archive_is_a_template(world, smoothed):
    from pulseportraiture_amd import pptoas
    gt = pptoas.GetTOAs(world["meta"], smoothed[1], quiet=True)
    gt.get_TOAs(quiet=True)
    assert len(gt.TOA_list) == 3 * NSUB


def test_smooth_portrait(world, smoothed):
    dp = pplib.DataPortrait(smoothed[0], quiet=True)
    port, portx = np.array(dp.port), np.array(dp.portx)
    dp.smooth_portrait(smart=True)
    kw = dict(search="batched", try_nlevels=min(8, 7))
    assert np.array_equal(dp.port, pplib.smart_smooth(port, **kw))
    assert np.array_equal(dp.portx, pplib.smart_smooth(portx, **kw))
    assert dp.port.any() and not np.array_equal(dp.port, port)
    np.testing.assert_array_equal(dp.noise_stds[0, 0],
                                  pplib.get_noise(dp.port, chans=True))
    np.testing.assert_array_equal(dp.noise_stdsxs,
                                  pplib.get_noise(dp.portx, chans=True))
    np.testing.assert_array_equal(dp.flux_prof, dp.port.mean(axis=1))
    np.testing.assert_array_equal(dp.flux_profx, dp.portx.mean(axis=1))
    # the plain smoother takes the same road
    dq = pplib.DataPortrait(smoothed[0], quiet=True)
    dq.smooth_portrait(nlevel=3, fact=0.5)
    assert np.array_equal(dq.port, pplib.wavelet_smooth(port, nlevel=3,
                                                        fact=0.5))
