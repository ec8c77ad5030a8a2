"""GPU: simulated archives built on the device (ppf_fake_batch / k_fake,
engine.fake_subints, pplib.make_fake_pulsar).  The noiseless float64 rows
against tests/golden/fake.npz (rows composed from the reference's own
functions), the device quantiser against psrfits.quantize bit for bit, the
counter RNG's keying and moments, the file round trip through
psrfits.load_data, injection and recovery through GetTOAs, the dedispersed
average through ppgauss.DataPortrait and the polarisation layouts."""
import os

import numpy as np
import pytest

import fakecases as F
from pulseportraiture_amd import engine, fake, pplib, psrfits

pytestmark = pytest.mark.gpu

GAUSS_ATOL = 1e-11          # the bar of the templates the rows start from
NU0 = 1500.0


def _rows(tab, model, seed=1, noise=None, first=0, quantized=False, sl=None):
    """engine.fake_subints on (a slice of the sub-ints of) a table set."""
    sl = slice(None) if sl is None else sl
    return engine.fake_subints(
        model, tab.model_of[sl], tab.phi[sl], tab.tau_n[sl], tab.gain[sl],
        tab.noise if noise is None else noise, seed, first_sub=first,
        quantized=quantized)


def _case_rows(case):
    par, ep, tab = F.case_tables(case)
    mdl = _mdl(os.path.join(F.GOLDEN, str(F.golden(case, "modelfile"))))
    return _rows(tab, fake.templates(mdl, tab))[0, 0].cpu().numpy(), tab, mdl


def _mdl(modelfile):
    (name, code, nu_ref, ngauss, params, ff, alpha, fa) = \
        pplib.read_model(modelfile, quiet=True)
    return pplib.DataBunch(name=name, code=code, nu_ref=nu_ref, params=params,
                           alpha=alpha)


def _parent_chain(tab, mdl):
    """The parent commit's two steps on the same tables: the template
    (engine.gauss_portraits), then engine.rotate_rows by phi."""
    model = fake.templates(mdl, tab)[0]
    return engine.rotate_rows(model, tab.phi[0], ref_len=True).cpu().numpy()


@pytest.fixture(scope="module")
def parent_rel():
    """Relative deviation of the parent's own two-step chain from the golden
    rows of the plain case."""
    par, ep, tab = F.case_tables("plain")
    want = F.golden("plain", "rows")
    got = _parent_chain(tab, _mdl(F.GMODEL))
    rel = np.abs(got - want).max() / np.abs(want).max()
    print("\nparent chain (gauss_portraits -> rotate_rows) vs golden, plain: "
          "%.3e of max|golden|" % rel)
    return rel


def _bar(parent_rel):
    # GAUSS_ATOL, or twice the parent chain's own figure where that is larger
    return max(GAUSS_ATOL, 2.0 * parent_rel)


# ------------------------------------------------------------- 1. the rows --
@pytest.mark.parametrize("case", F.CASES)
def test_noiseless_rows_match_golden(case, parent_rel):
    got, tab, mdl = _case_rows(case)
    want = F.golden(case, "rows")
    assert got.shape == want.shape
    rel = np.abs(got - want).max() / np.abs(want).max()
    print("\nk_fake vs golden, %s: %.3e of max|golden| (bar %.1e)"
          % (case, rel, _bar(parent_rel)))
    assert rel <= _bar(parent_rel)


@pytest.mark.parametrize("nchan,nbin", [(3, 32), (2, 8192), (3, 96)])
def test_noiseless_rows_match_parent_chain(nchan, nbin, parent_rel):
    """No golden at these lengths (the smallest, the largest: 64 KB of LDS,
    and a mixed-radix one): the parent's two-step chain is the reference."""
    par = fake.read_par(F.PAR)
    ep = fake.fake_epochs(par, 1, 300.0)
    tab = fake.fake_tables(0.0, par.DM, ep.Ps, nchan=nchan, nbin=nbin,
                           phase=0.013, dDM=3e-4, noise_stds=0.0)
    mdl = _mdl(F.GMODEL)
    got = _rows(tab, fake.templates(mdl, tab))[0, 0].cpu().numpy()
    want = _parent_chain(tab, mdl)
    rel = np.abs(got - want).max() / np.abs(want).max()
    print("\nk_fake vs parent chain, %d x %d: %.3e" % (nchan, nbin, rel))
    assert rel <= _bar(parent_rel)


def test_add_DM_nu_matches_golden(parent_rel):
    Z = F.Z
    port, freqs, P = Z["fn__port"], Z["fn__freqs"], float(Z["fn__P"])
    phase, DM, nu_ref = Z["fn__dmnu_args"]
    got = pplib.add_DM_nu(port, phase, DM, P, freqs, list(Z["fn__xs"]),
                          list(Z["fn__Cs"]), nu_ref)
    want = Z["fn__dmnu"]
    assert np.abs(got - want).max() <= _bar(parent_rel) * np.abs(want).max()
    got = pplib.add_DM_nu(port, phase=-0.31)
    want = Z["fn__dmnu_plain"]
    assert np.abs(got - want).max() <= _bar(parent_rel) * np.abs(want).max()
    # the defaults are rotate_portrait
    np.testing.assert_array_equal(
        pplib.add_DM_nu(port, 0.1, 1e-3, P, freqs),
        pplib.rotate_portrait(port, 0.1, 1e-3, P, freqs))


# ------------------------------------------------------ 2. the quantiser --
def _quant_problem():
    nsub, npol, nchan, nbin = 3, 2, 5, 64
    par = fake.read_par(F.PAR)
    ep = fake.fake_epochs(par, nsub, 10.0)
    scales = np.array([1.0, 0.0, 2.0, 0.5, 1.5])     # channel 1: constant rows
    noise = np.array([0.3, 0.0, 1.0, 0.0, 0.1])      # channel 3: noise-free
    tab = fake.fake_tables(0.0, par.DM, ep.Ps, nsub=nsub, npol=npol,
                           nchan=nchan, nbin=nbin, phase=0.2, dDM=1e-3,
                           noise_stds=noise, scales=scales)
    return ep, tab, fake.templates(_mdl(F.GMODEL), tab)


def test_quantisation_is_exact(tmp_path):
    nsub, npol, nchan, nbin = 3, 2, 5, 64
    ep, tab, model = _quant_problem()
    rows = _rows(tab, model, seed=11).cpu().numpy()
    data, scl, offs = _rows(tab, model, seed=11, quantized=True)
    data, scl, offs = data.cpu().numpy(), scl.cpu().numpy(), offs.cpu().numpy()
    q, qscl, qoffs = psrfits.quantize(rows)
    got = data.view(">i2").reshape(nsub, npol, nchan, nbin)
    np.testing.assert_array_equal(got, q)
    assert scl.dtype == np.float32 and offs.dtype == np.float32
    np.testing.assert_array_equal(scl, qscl)
    np.testing.assert_array_equal(offs, qoffs)
    # the zero-gain, noise-free channel is constant: the floor of the scale
    assert np.all(scl.reshape(nsub, npol, nchan)[:, :, 1] == np.float32(1e-30))
    assert not got[:, :, 1].any()
    # the full range of the sample type is used elsewhere
    assert got[:, :, 0].max() == 32767 and got[:, :, 0].min() in (-32767, -32768)
    # the bytes are the file's: written as they are, read back the same
    fn = str(tmp_path / "q.fits")
    psrfits.write_psrfits_rows(
        fn, data, scl, offs, np.tile(tab.freqs, (nsub, 1)),
        np.ones((nsub, nchan)), ep.Ps, ep.offs_sub, np.full(nsub, 10.0), nbin,
        npol=npol, pol_type="AABB")
    f = psrfits.PSRFITS(fn)
    try:
        back = np.array(f.subint.column("DATA")).reshape(nsub, npol, nchan, nbin)
        np.testing.assert_array_equal(back, q)
        fs, fo = f.scales_offsets()
        np.testing.assert_array_equal(fs, qscl)
        np.testing.assert_array_equal(fo, qoffs)
    finally:
        f.close()


@pytest.mark.parametrize("nbin", [36, 8192])
def test_quantisation_both_store_widths(nbin):
    """nbin % 8 != 0 takes the 4-byte stores, 8192 fills the LDS row."""
    par = fake.read_par(F.PAR)
    ep = fake.fake_epochs(par, 2, 10.0)
    tab = fake.fake_tables(0.0, par.DM, ep.Ps, nsub=2, npol=1, nchan=3,
                           nbin=nbin, phase=0.4, noise_stds=0.2)
    model = fake.templates(_mdl(F.GMODEL), tab)
    rows = _rows(tab, model, seed=3).cpu().numpy()
    data, scl, offs = _rows(tab, model, seed=3, quantized=True)
    q, qscl, qoffs = psrfits.quantize(rows)
    np.testing.assert_array_equal(
        data.cpu().numpy().view(">i2").reshape(q.shape), q)
    np.testing.assert_array_equal(scl.cpu().numpy(), qscl)
    np.testing.assert_array_equal(offs.cpu().numpy(), qoffs)


# ---------------------------------------------------------------- 3. RNG --
def test_rng_keying():
    nsub, npol, nchan, nbin = 5, 2, 4, 64
    par = fake.read_par(F.PAR)
    ep = fake.fake_epochs(par, nsub, 10.0)
    noise = np.array([0.5, 0.0, 1.0, 2.0])
    tab = fake.fake_tables(0.0, par.DM, ep.Ps, nsub=nsub, npol=npol,
                           nchan=nchan, nbin=nbin, phase=0.1, noise_stds=noise)
    model = fake.templates(_mdl(F.GMODEL), tab)
    a = _rows(tab, model, seed=7, quantized=True)
    b = _rows(tab, model, seed=7, quantized=True)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    # 5 sub-ints in one call == 2 + 3 with first_sub
    whole = _rows(tab, model, seed=7).cpu().numpy()
    head = _rows(tab, model, seed=7, sl=slice(0, 2)).cpu().numpy()
    tail = _rows(tab, model, seed=7, sl=slice(2, 5), first=2).cpu().numpy()
    np.testing.assert_array_equal(whole, np.concatenate([head, tail]))
    qa = a[0].cpu().numpy()
    qh = _rows(tab, model, seed=7, sl=slice(0, 2), quantized=True)[0]
    qt = _rows(tab, model, seed=7, sl=slice(2, 5), first=2, quantized=True)[0]
    assert qa.tobytes() == qh.cpu().numpy().tobytes() + qt.cpu().numpy().tobytes()
    # another seed, and another first_sub, differ
    other = _rows(tab, model, seed=8).cpu().numpy()
    assert np.all(other[:, :, 0] != whole[:, :, 0])
    shifted = _rows(tab, model, seed=7, first=1).cpu().numpy()
    assert np.all(shifted[:, :, 0] != whole[:, :, 0])
    # noise[n] == 0: exactly the noiseless rows
    clean = _rows(tab, model, seed=7, noise=np.zeros(nchan)).cpu().numpy()
    np.testing.assert_array_equal(whole[:, :, 1], clean[:, :, 1])
    assert np.all(whole[:, :, 0] != clean[:, :, 0])
    # the polarisations draw their own noise
    assert np.all(whole[:, 0, 0] != whole[:, 1, 0])
    np.testing.assert_array_equal(clean[:, 0], clean[:, 1])


def test_rng_moments():
    """m samples per channel: the residual's standard deviation within
    5 / sqrt(2 m) relative of noise_stds[n] (the standard error of a normal
    sample's standard deviation), its mean within 5 sigma / sqrt(m) of 0."""
    nsub, nchan, nbin = 8, 4, 1024
    par = fake.read_par(F.PAR)
    ep = fake.fake_epochs(par, nsub, 10.0)
    noise = np.array([0.5, 1.0, 2.0, 4.0])
    tab = fake.fake_tables(0.0, par.DM, ep.Ps, nsub=nsub, nchan=nchan,
                           nbin=nbin, noise_stds=noise)
    model = fake.templates(_mdl(F.GMODEL), tab)
    noisy = _rows(tab, model, seed=2024).cpu().numpy()
    clean = _rows(tab, model, seed=2024, noise=np.zeros(nchan)).cpu().numpy()
    m = nsub * nbin
    for n in range(nchan):
        r = (noisy - clean)[:, 0, n].reshape(-1)
        print("\nchannel %d: std / sigma - 1 = %+.4f (bound %.4f), mean / "
              "sigma = %+.4f (bound %.4f)"
              % (n, r.std() / noise[n] - 1, 5 / np.sqrt(2 * m),
                 r.mean() / noise[n], 5 / np.sqrt(m)))
        assert abs(r.std() / noise[n] - 1.0) <= 5.0 / np.sqrt(2.0 * m)
        assert abs(r.mean()) <= 5.0 * noise[n] / np.sqrt(m)


# ---------------------------------------------------------- 4. the file --
ARCH = dict(nsub=3, npol=1, nchan=16, nbin=256, nu0=NU0, bw=800.0, tsub=60.0,
            phase=0.07, noise_stds=0.05)


def test_file_round_trip(tmp_path):
    fn = str(tmp_path / "rt.fits")
    weights = np.ones((3, 16))
    weights[:, 3] = weights[:, 11] = 0.0
    start = pplib.MJD(57000, 0.123456789)
    kw = dict(ARCH, dDM=2e-4, start_MJD=start)
    pplib.make_fake_pulsar(F.GMODEL, F.PAR, outfile=fn, weights=weights,
                           telescope="GBT", quiet=True, seed=99, **kw)
    d = psrfits.load_data(fn, pscrunch=True, rm_baseline=False, quiet=True)
    par, ep, tab, mdl = fake.fake_setup(F.GMODEL, F.PAR, **kw)
    assert d.nbin == 256 and d.nchan == 16 and d.nsub == 3
    np.testing.assert_array_equal(d.freqs, np.tile(tab.freqs, (3, 1)))
    np.testing.assert_array_equal(d.weights, weights)
    ok = [i for i in range(16) if i not in (3, 11)]
    for isub in range(3):
        assert list(d.ok_ichans[isub]) == ok
    np.testing.assert_array_equal(d.Ps, ep.Ps)
    assert d.DM == par.DM and d.source == "J1234-5678"
    assert d.telescope == "GBT" and d.nu0 == NU0 and d.bw == 800.0
    for i, e in enumerate(d.epochs):
        want = start + (30.0 + 60.0 * i)
        assert e.intday() == want.intday()
        assert abs(e.fracday() - want.fracday()) * 86400.0 < 1e-9
    f = psrfits.PSRFITS(fn)
    try:
        assert f.pol_type == "AA+BB"
        assert f.primary["RA"].strip() == par.RAJ
        assert f.primary["DEC"].strip() == par.DECJ
        scl, offs = f.scales_offsets()
    finally:
        f.close()
    # every sample within half a step, plus the float32 rounding of the
    # loader's DATA * DAT_SCL + DAT_OFFS (two roundings), of the float64 rows
    rows = _rows(tab, fake.templates(mdl, tab), seed=99).cpu().numpy()[:, 0]
    got = np.asarray(d.subints)[:, 0].astype(np.float64)
    scl = scl.reshape(3, 16, 1).astype(np.float64)
    tol = scl / 2 + 2.0 ** -23 * (np.abs(rows).max(axis=-1, keepdims=True) +
                                   np.abs(offs).reshape(3, 16, 1) + scl)
    assert np.all(np.abs(got - rows) <= tol)
    # ... zero-weight channels included: they get data as in the reference
    assert np.abs(got[:, 3]).max() > 1.0


def test_tutorial_arguments(tmp_path, capsys):
    """The reference tutorial's first call (examples/example.py:51-60): its
    arguments, scint=True and seed=None included, both drawn from np.random."""
    kw = dict(nsub=10, npol=1, nchan=64, nbin=512, nu0=1500.0, bw=800.0,
              tsub=60.0, phase=0.0, dDM=3e-4, start_MJD=pplib.MJD(57202.00),
              weights=np.ones([10, 64]), noise_stds=1.5, scales=1.0,
              dedispersed=False, scint=True, state="Stokes", telescope="GBT")
    a, b = str(tmp_path / "example-1.fits"), str(tmp_path / "example-2.fits")
    np.random.seed(12)
    capsys.readouterr()
    pplib.make_fake_pulsar(F.GMODEL, F.PAR, outfile=a, quiet=False, **kw)
    assert capsys.readouterr().out == "\nUnloaded %s.\n\n" % a
    np.random.seed(12)
    pplib.make_fake_pulsar(F.GMODEL, F.PAR, outfile=b, quiet=True, **kw)
    assert capsys.readouterr().out == ""
    with open(a, "rb") as fa, open(b, "rb") as fb:
        assert fa.read() == fb.read()
    d = psrfits.load_data(a, pscrunch=True, quiet=True)
    assert (d.nsub, d.nchan, d.nbin) == (10, 64, 512)
    assert d.epochs[0].intday() == 57202
    assert abs(d.epochs[0].fracday() * 86400.0 - 30.0) < 1e-6
    # the scintillation pattern differs from sub-int to sub-int, and the
    # injected noise is what the loader measures
    rows = np.asarray(d.subints)[:, 0]
    assert not np.allclose(rows[0].max(axis=-1), rows[1].max(axis=-1),
                           rtol=0.05)
    assert abs(np.asarray(d.noise_stds).mean() / 1.5 - 1.0) < 0.05


# ------------------------------------------------- 5, 6. recovery, average --
DDMS = (2e-4, 5e-4)


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    d = tmp_path_factory.mktemp("fake")
    files = []
    for i, dDM in enumerate(DDMS):
        fn = str(d / ("a%d.fits" % i))
        pplib.make_fake_pulsar(F.GMODEL, F.PAR, outfile=fn, dDM=dDM,
                               quiet=True, seed=1000 + i, **ARCH)
        files.append(fn)
    meta = d / "meta.txt"
    meta.write_text("\n".join(files) + "\n")
    return files, str(meta)


def test_injection_recovery(archives):
    from pulseportraiture_amd import pptoas
    files, meta = archives
    DM_par = fake.read_par(F.PAR).DM
    gt = pptoas.GetTOAs(meta, F.GMODEL, quiet=True)
    gt.get_TOAs(DM0=DM_par, nu_refs=(NU0, None), quiet=True)
    for i, dDM in enumerate(DDMS):
        DMs, DM_errs = np.asarray(gt.DMs[i]), np.asarray(gt.DM_errs[i])
        phis, phi_errs = np.asarray(gt.phis[i]), np.asarray(gt.phi_errs[i])
        rcs = np.asarray(gt.red_chi2s[i])
        assert len(DMs) == 3
        pull_DM = (DMs - DM_par - dDM) / DM_errs
        dphi = (phis - ARCH["phase"] + 0.5) % 1.0 - 0.5
        pull_phi = dphi / phi_errs
        print("\narchive %d: DM pulls %s, phase pulls %s, red. chi2 %s"
              % (i, pull_DM, pull_phi, rcs))
        assert np.all(np.abs(pull_DM) <= 5.0)
        assert np.all(np.abs(pull_phi) <= 5.0)
        assert np.all((rcs >= 0.8) & (rcs <= 1.25))
        # the errors are those of the injected noise, not vacuous
        assert np.all(DM_errs < 1e-4) and np.all(phi_errs < 1e-3)


def test_dedispersed_average_matches_template(archives):
    from pulseportraiture_amd import ppgauss
    files, meta = archives
    dp = ppgauss.DataPortrait(files[1], quiet=True)
    par, ep, tab, mdl = fake.fake_setup(F.GMODEL, F.PAR, dDM=DDMS[1], **ARCH)
    assert dp.nchan == 16 and dp.nbin == 256 and dp.DM == par.DM
    # what the loader's dedispersion by the header DM leaves: the residual
    # (phase, dDM) rotation, per sub-int, then the mean of the three
    left = [engine.rotate_rows(
        fake.templates(mdl, tab)[0],
        -ARCH["phase"] - pplib.DM_delay(DDMS[1], tab.freqs, NU0, P),
        ref_len=True).cpu().numpy() for P in ep.Ps]
    want = np.mean(left, axis=0)
    got = np.asarray(dp.port, dtype=np.float64)
    # the loader removed a baseline: compare about each channel's mean
    r = (got - got.mean(axis=1, keepdims=True)) - \
        (want - want.mean(axis=1, keepdims=True))
    sigma = ARCH["noise_stds"] / np.sqrt(3.0)
    rchi2 = np.sum((r / sigma) ** 2) / (16 * (256 - 1))
    print("\ndedispersed average vs template: reduced chi2 %.4f" % rchi2)
    assert 0.8 <= rchi2 <= 1.25
    # the wrong sign of dDM, or no dDM, does not fit
    off = engine.rotate_rows(
        fake.templates(mdl, tab)[0],
        -ARCH["phase"] + pplib.DM_delay(20 * DDMS[1], tab.freqs, NU0, ep.Ps[0]),
        ref_len=True).cpu().numpy()
    r = (got - got.mean(axis=1, keepdims=True)) - \
        (off - off.mean(axis=1, keepdims=True))
    assert np.sum((r / sigma) ** 2) / (16 * 255) > 1.25


# -------------------------------------------------------- 7. polarisation --
@pytest.mark.parametrize("state,pol_type,factor", [("Stokes", "IQUV", 1.0),
                                                   ("Coherence", "AABBCRCI", 2.0)])
def test_polarisation(tmp_path, state, pol_type, factor):
    fn = str(tmp_path / "pol.fits")
    kw = dict(ARCH, npol=4, nsub=2, dDM=1e-4)
    pplib.make_fake_pulsar(F.GMODEL, F.PAR, outfile=fn, state=state,
                           quiet=True, seed=5, **kw)
    f = psrfits.PSRFITS(fn)
    try:
        assert f.npol == 4 and f.pol_type == pol_type
    finally:
        f.close()
    d = psrfits.load_data(fn, pscrunch=True, rm_baseline=False, quiet=True)
    par, ep, tab, mdl = fake.fake_setup(F.GMODEL, F.PAR, **kw)
    model = fake.templates(mdl, tab)
    clean = _rows(tab, model, seed=5, noise=np.zeros(16)).cpu().numpy()
    noisy = _rows(tab, model, seed=5).cpu().numpy()
    # total intensity: I (IQUV) or AA + BB, each polarisation the same model
    got = np.asarray(d.subints)[:, 0].astype(np.float64)
    r = (got - factor * clean[:, 0]).reshape(-1)
    m = r.size
    sigma = ARCH["noise_stds"] * np.sqrt(factor)     # two independent draws
    assert abs(r.std() / sigma - 1.0) <= 5.0 / np.sqrt(2.0 * m)
    # (+ the digitisation: at most half a step of ~1.5e-4 per polarisation)
    assert abs(r.mean()) <= 5.0 * sigma / np.sqrt(m) + 1e-4
    # the four polarisations' noise draws differ (and are uncorrelated)
    res = (noisy - clean).transpose(1, 0, 2, 3).reshape(4, -1)
    for p in range(4):
        for q in range(p + 1, 4):
            assert np.all(res[p] != res[q])
            c = np.corrcoef(res[p], res[q])[0, 1]
            assert abs(c) <= 5.0 / np.sqrt(res.shape[1])
