"""GPU: the joined Gaussian model (several archives under one model, each
with a phase and a DM offset): ppf_gauss_portrait_join_batch against the
reference's portraits (tests/golden/gaussjoin.npz), njoin = 0 against the
unjoined entry points bit for bit, the Gram matrix of
ppf_gauss_lsq_join_batch against NumPy at the summation bound,
fit_gaussian_portrait(join_params=...) at the project's parity bar (0.01
sigma, 1e-8 in chi^2), the refusals, and ppgauss.DataPortrait end to end on
two archives."""
import os

import numpy as np
import pytest

import joincases as J
from pulseportraiture_amd import engine, pplib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "gaussjoin.npz"))
EPS = np.finfo(np.float64).eps
GAUSS_ATOL = 1e-11                  # x max|portrait|: test_gpu_parity.py's bar
SIGMA_TOL, CHI2_RTOL = 0.01, 1e-8


# ------------------------------------------------------------ 1. portraits --
@pytest.mark.parametrize("name", sorted(J.PORT_CASES))
def test_joined_portrait_matches_reference(name):
    c = J.port_case(name)
    ref = G[name + "__port"]
    got = pplib.gen_gaussian_portrait(
        c["code"], c["p_ext"][:-1], c["p_ext"][-1], np.zeros(c["nbin"]),
        c["freqs"], J.NU_REF, c["join_ichans"], J.P)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("%s: max |dev| / max|portrait| = %.2e" % (name, err))
    assert got.shape == ref.shape
    assert err <= GAUSS_ATOL
    ids = J.join_ids(c["join_ichans"], len(c["freqs"]))
    if (ids < 0).any():
        # a channel in no archive: the unjoined build, bit for bit
        npar = len(c["p_ext"]) - 1 - 2 * c["njoin"]
        plain = pplib.gen_gaussian_portrait(
            c["code"], c["p_ext"][:npar], c["p_ext"][-1], np.zeros(c["nbin"]),
            c["freqs"], J.NU_REF)
        assert got[ids < 0].tobytes() == plain[ids < 0].tobytes()
        assert got[ids >= 0].tobytes() != plain[ids >= 0].tobytes()


# -------------------------------------------------------------- 2. njoin 0 --
@pytest.mark.parametrize("nbin,tau", [(64, 0.0), (100, 2.5), (1536, 2.5)])
def test_njoin_zero_is_the_unjoined_call_bit_for_bit(nbin, tau):
    rng = np.random.default_rng(nbin)
    nfit, nchan = 2, 5
    prm = np.tile(np.array([0.02, tau] + [v for c in J.COMPS_000 for v in c]),
                  (nfit, 1))
    prm[1, 2] += 0.05
    freqs = np.sort(rng.uniform(1100.0, 1900.0, size=(nfit, nchan)), axis=1)
    nu_ref, alpha = np.array([1500.0, 1400.0]), np.array([-4.0, -3.9])
    ids = np.full((nfit, nchan), -1, dtype=np.int32)
    jp = np.zeros((nfit, 0))
    old = engine.gauss_portraits("000", prm, alpha, freqs, nu_ref, nbin)
    new = engine.gauss_portraits("000", prm, alpha, freqs, nu_ref, nbin,
                                 join_id=ids, join_params=jp, P=[J.P, J.P])
    assert old.cpu().numpy().tobytes() == new.cpu().numpy().tobytes()
    data = old.cpu().numpy() + 0.1 * rng.normal(size=old.shape)
    w = 1.0 / rng.uniform(0.05, 0.2, size=data.shape)
    free_idx = [0, 2, 3, 4, 6, 7, 14]              # 14: the scattering index
    ext = np.concatenate([prm, alpha[:, None]], axis=1)
    delta = np.sqrt(EPS) * np.abs(ext[:, free_idx])
    g_old = engine.gauss_lsq("000", prm, alpha, freqs, nu_ref, free_idx,
                             delta, data, w)
    g_new = engine.gauss_lsq("000", prm, alpha, freqs, nu_ref, free_idx,
                             delta, data, w, join_id=ids, join_params=jp,
                             P=[J.P, J.P])
    assert g_old.cpu().numpy().tobytes() == g_new.cpu().numpy().tobytes()


# ----------------------------------------------------------------- 3. Gram --
def _join_problem(seed, nfit, nchan, nbin, njoin, tau, f32, code="000"):
    rng = np.random.default_rng(seed)
    comps = J.COMPS_000 if code == "000" else J.COMPS_111
    prm = np.tile(np.array([0.02, tau] + [v for c in comps for v in c]),
                  (nfit, 1))
    prm[:, 2] += 0.01 * rng.normal(size=nfit)
    freqs = np.sort(rng.uniform(1100.0, 1900.0, size=(nfit, nchan)), axis=1)
    nu_ref = rng.uniform(1300.0, 1700.0, size=nfit)
    alpha = np.full(nfit, -4.0) + 0.1 * rng.normal(size=nfit)
    # interleaved archives, every archive present in every fit
    ids = np.array([rng.permutation(np.arange(nchan) % njoin)
                    for _ in range(nfit)], dtype=np.int32)
    jp = np.zeros((nfit, 2 * njoin))
    jp[:, 0::2] = 0.02 * rng.normal(size=(nfit, njoin))
    jp[:, 1::2] = 3e-4 * rng.normal(size=(nfit, njoin))
    jp[:, 1] = 0.0                                  # a DM that starts at 0
    Ps = np.full(nfit, J.P)
    model = engine.gauss_portraits(code, prm, alpha, freqs, nu_ref, nbin,
                                   join_id=ids, join_params=jp,
                                   P=Ps).cpu().numpy()
    data = model + 0.1 * rng.normal(size=model.shape)
    if f32:
        data = data.astype(np.float32)
    w = 1.0 / rng.uniform(0.05, 0.2, size=model.shape)
    return prm, alpha, freqs, nu_ref, ids, jp, Ps, data, w


# (nfit, nchan, nbin, njoin, tau, f32, free indices into [params (14), join
# params, index])
GRAM_SHAPES = [
    (1, 6, 64, 2, 0.0, False, [0, 2, 4, 6, 14, 15, 16, 17, 18]),
    (2, 7, 100, 2, 2.5, True,
     [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 16, 17, 18]),  # 17 columns
    (1, 5, 1536, 3, 0.0, False, [2, 8, 14, 15, 16, 17, 18, 19, 20]),
]


@pytest.mark.parametrize("shape", GRAM_SHAPES,
                         ids=lambda s: "%dx%dx%d_j%d" % s[:4])
def test_joined_gram_matches_numpy(shape):
    nfit, nchan, nbin, njoin, tau, f32, free_idx = shape
    code = "000"
    prm, alpha, freqs, nu_ref, ids, jp, Ps, data, w = _join_problem(
        7 + nbin, nfit, nchan, nbin, njoin, tau, f32)
    npar, nfree = prm.shape[1], len(free_idx)
    nxt = npar + 2 * njoin
    assert free_idx[-1] == nxt and any(npar <= i < nxt and (i - npar) % 2
                                       for i in free_idx)
    ext = np.concatenate([prm, jp, alpha[:, None]], axis=1)
    delta = np.sqrt(EPS) * np.where(ext[:, free_idx] == 0, 1.0,
                                    np.abs(ext[:, free_idx]))

    def build(e):
        return engine.gauss_portraits(
            code, e[:, :npar], e[:, -1], freqs, nu_ref, nbin, join_id=ids,
            join_params=e[:, npar:-1], P=Ps).cpu().numpy()

    def lsq():
        return engine.gauss_lsq(code, prm, alpha, freqs, nu_ref, free_idx,
                                delta, data, w, join_id=ids, join_params=jp,
                                P=Ps).cpu().numpy()
    g1, g2 = lsq(), lsq()
    assert g1.shape == (nfit, nfree + 1, nfree + 1)
    assert g1.tobytes() == g2.tobytes()            # bitwise reproducible
    m0 = build(ext)
    K = nchan * nbin
    for f in range(nfit):
        C = np.empty((nfree + 1, K))
        for j, i in enumerate(free_idx):
            e = ext.copy()
            e[f, i] = e[f, i] + delta[f, j]
            C[j] = (((build(e)[f] - m0[f]) / delta[f, j]) * w[f]).ravel()
        C[-1] = ((data[f].astype(np.float64) - m0[f]) * w[f]).ravel()
        ref = C @ C.T
        assert np.isfinite(g1[f]).all()
        np.testing.assert_array_equal(g1[f], g1[f].T)
        d = np.sqrt(np.diag(ref))
        bound = 2 * K * EPS * np.outer(d, d)
        err = np.abs(g1[f] - ref)
        print("fit %d: max |G - CC^T| / bound = %.3g" % (
            f, (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
        # join columns of two different archives share no channel
        for ja, ia in enumerate(free_idx):
            for jb, ib in enumerate(free_idx):
                if npar <= ia < nxt and npar <= ib < nxt and \
                        (ia - npar) // 2 != (ib - npar) // 2:
                    assert g1[f][ja, jb] == 0.0
        # every join column is live (the scattering index's is zero at tau 0)
        assert all(g1[f][j, j] > 0 for j, i in enumerate(free_idx)
                   if npar <= i < nxt)


# ------------------------------------------------------------------ 4. fit --
@pytest.mark.parametrize("name", sorted(J.FIT_CASES))
def test_fit_gaussian_portrait_join_matches_golden(name):
    c = J.fit_case(name)
    data, errs = G[name + "__data"], G[name + "__errs"]
    npar, v = c["npar"], c["vary"]
    r = pplib.fit_gaussian_portrait(
        c["code"], data, c["start"][:npar], c["start"][-1], errs,
        v[:npar].astype(int), bool(v[-1]), pplib.get_bin_centers(c["nbin"]),
        c["freqs"], J.NU_REF,
        join_params=[c["join_ichans"], c["start"][npar:-1],
                     v[npar:-1].astype(int)], P=J.P)
    assert r.lm_results.success and r.lm_results.nfev > 0
    assert len(r.fitted_params) == len(r.fit_errs) == npar + 2 * c["njoin"]
    assert abs(np.sum(r.lm_results.residual ** 2) / r.chi2 - 1) < 1e-10
    p = np.append(r.fitted_params, r.scattering_index)
    perr = np.append(r.fit_errs, r.scattering_index_err)
    sol, serr = G[name + "__solution"], G[name + "__sol_errs"]
    dev = (np.abs(p - sol)[v] / serr[v]).max()
    rel = abs(r.chi2 / float(G[name + "__chi2"]) - 1)
    erel = np.abs(perr[v] / serr[v] - 1).max()
    print(name, "max dev %.2e sigma, chi2 rel %.1e, errs rel %.1e, nfev %d" % (
        dev, rel, erel, r.lm_results.nfev))
    assert dev <= SIGMA_TOL
    assert rel <= CHI2_RTOL
    assert erel <= 2 * float(G[name + "__spread_errs"])
    assert r.dof == int(G[name + "__dof"])
    np.testing.assert_array_equal(p[~v], c["start"][~v])   # fixed: untouched
    assert (perr[~v] == 0.0).all()


# ------------------------------------------------------------- 5. refusals --
def test_joined_calls_refuse_odd_nbin_and_bad_join_id():
    c = J.port_case("p100")
    npar = len(c["p_ext"]) - 1 - 2 * c["njoin"]
    with pytest.raises(NotImplementedError):       # odd nbin
        pplib.gen_gaussian_portrait(c["code"], c["p_ext"][:-1], -4.0,
                                    np.zeros(99), c["freqs"], J.NU_REF,
                                    c["join_ichans"], J.P)
    ids = J.join_ids(c["join_ichans"], len(c["freqs"]))[None]
    for bad in (c["njoin"], -2):
        b = ids.copy()
        b[0, 3] = bad
        with pytest.raises(ValueError):
            engine.gauss_portraits(c["code"], c["p_ext"][None, :npar], [-4.0],
                                   c["freqs"][None], [J.NU_REF], 100,
                                   join_id=b,
                                   join_params=c["p_ext"][None, npar:-1],
                                   P=[J.P])
    data = np.zeros((1, len(c["freqs"]), 100))
    with pytest.raises(ValueError):                # past the scattering index
        engine.gauss_lsq(c["code"], c["p_ext"][None, :npar], [-4.0],
                         c["freqs"][None], [J.NU_REF], [npar + 5], [[1e-8]],
                         data, np.ones_like(data), join_id=ids,
                         join_params=c["p_ext"][None, npar:-1], P=[J.P])
    with pytest.raises(NotImplementedError):       # odd nbin
        engine.gauss_lsq(c["code"], c["p_ext"][None, :npar], [-4.0],
                         c["freqs"][None], [J.NU_REF], [0], [[1e-8]],
                         data[:, :, :99], np.ones_like(data[:, :, :99]),
                         join_id=ids, join_params=c["p_ext"][None, npar:-1],
                         P=[J.P])


# ------------------------------------------------------------ 6. end to end --
def _archive(name, port, freqs, P, noise):
    nchan, nbin = port.shape
    return pplib.DataBunch(
        subints=port[None, None], masks=np.ones((1, 1, nchan, nbin)),
        freqs=freqs[None], ok_ichans=[np.arange(nchan)],
        noise_stds=np.full((1, 1, nchan), noise),
        SNRs=np.full((1, 1, nchan), 100.0), Ps=np.array([P]),
        phases=pplib.get_bin_centers(nbin), nu0=freqs.mean(),
        bw=(freqs[-1] - freqs[0]) * nchan / (nchan - 1), source="PSR_SYNTH",
        nbin=nbin, nchan=nchan, filename=name)


def test_dataportrait_joined_end_to_end(tmp_path, monkeypatch):
    """Two synthetic 8 x 256 archives of the example model over interleaving
    bands, the second offset by a known (phase, DM)
    (make_golden_gaussjoin.py checked the seed on the CPU: largest pull < 3),
    from a perturbed .gmodel, niter=1: converges, every fitted model and join
    parameter within 5 of its own errors of the injected value, and the
    join file is written and read back."""
    from pulseportraiture_amd import ppgauss
    monkeypatch.chdir(tmp_path)                  # the .join file lands here
    ports, freqs, P = G["e2e__ports"], G["e2e__freqs"], float(G["e2e__P"])
    noise = float(G["e2e__noise"])
    truth, flags = G["e2e__truth"], G["e2e__flags"]
    bunches = [_archive("lo.fits", ports[0], freqs[0], P, noise),
               _archive("hi.fits", ports[1], freqs[1], P, noise)]
    nbin = ports.shape[2]
    start = str(tmp_path / "start.gmodel")
    sp = G["e2e__start"].copy()
    sp[1] *= P / nbin
    pplib.write_model(start, "joined", str(G["e2e__code"]),
                      float(G["e2e__nu_ref"]), sp, flags,
                      float(G["e2e__alpha"]), 0, quiet=True)
    dp = ppgauss.DataPortrait(bunches)
    assert dp.njoin == 2 and dp.nchan == 16
    assert any(np.any(np.diff(ic) > 1) for ic in dp.join_ichans)
    np.testing.assert_array_equal(dp.join_fit_flags, [0, 1, 1, 1])
    assert dp.join_params[0] == dp.join_params[1] == dp.join_params[3] == 0.0
    # the start phase of the second archive is a profile cross-correlation:
    # profile evolution between the bands moves it by less than the
    # components' spread (0.04 rot)
    assert 0.0 < abs(dp.join_params[2]) and \
        abs(dp.join_params[2] - truth[-2]) < 0.05
    port0 = dp.port.copy()
    dp.make_gaussian_model(modelfile=start, niter=1, writemodel=True,
                           outfile=str(tmp_path / "fit.gmodel"), quiet=True)
    assert dp.cnvrgnc == 1
    npar = len(truth) - 4
    p = np.r_[dp.model_params, dp.join_params]
    perr = np.r_[dp.model_param_errs, dp.join_param_errs]
    vary = np.r_[flags != 0, dp.join_fit_flags != 0]
    assert len(dp.model_params) == npar
    pull = np.abs(p - truth)[vary] / perr[vary]
    print("largest pull %.2f (CPU loop: %.2f)" % (pull.max(),
                                                  float(G["e2e__cpu_pull"])))
    assert pull.max() <= 5.0
    np.testing.assert_array_equal(p[~vary], np.r_[G["e2e__start"], 0, 0, 0,
                                                  0][~vary])
    assert (perr[~vary] == 0.0).all()
    # port / portx / model de-rotated by the join parameters at nu_ref
    jic = dp.join_ichans[1]
    want = pplib.rotate_data(port0[jic], -dp.join_params[2],
                             -dp.join_params[3], P, dp.freqs[0, jic],
                             dp.nu_ref)
    np.testing.assert_array_equal(dp.port[jic], want)
    assert dp.model.shape == dp.port.shape
    # the join file: written after each fit, accepted back
    jf = tmp_path / "joined.join"
    lines = jf.read_text().splitlines()
    assert lines[0].startswith("# archive name") and len(lines) % 3 == 0
    assert lines[-2].split()[0] == "lo.fits"
    assert lines[-1].split()[0] == "hi.fits"
    back = ppgauss.DataPortrait(bunches, joinfile=str(jf))
    np.testing.assert_allclose(back.join_params[0::2], dp.join_params[0::2],
                               rtol=0, atol=0.5e-10)
    np.testing.assert_allclose(back.join_params[1::2], dp.join_params[1::2],
                               rtol=0, atol=0.5e-6)
    assert back.join_params[2] != 0.0 and back.join_params[3] != 0.0


# --------------------------------------------------- 7. metafile from files --
def test_metafile_of_psrfits_files(tmp_path):
    """pplib.DataPortrait(metafile) loads each listed PSRFITS file on the
    fast path (dedispersed, tscrunched, pscrunched): the same object as from
    the list of the loaded DataBunches, zero-weight channels condensed."""
    import fakecases as F
    from pulseportraiture_amd import ppgauss
    names = [str(tmp_path / "lo.fits"), str(tmp_path / "hi.fits")]
    weights = np.ones((2, 8))
    weights[:, 5] = 0.0
    for name, nu0, bw, ph, w in zip(names, (1300.0, 1650.0), (400.0, 500.0),
                                    (0.0, 0.03), (None, weights)):
        pplib.make_fake_pulsar(F.GMODEL, F.PAR, outfile=name, nsub=2, npol=1,
                               nchan=8, nbin=256, nu0=nu0, bw=bw, tsub=60.0,
                               phase=ph, noise_stds=0.05, weights=w,
                               quiet=True, seed=5)
    meta = tmp_path / "meta.txt"
    meta.write_text("\n".join(names) + "\n")
    dp = ppgauss.DataPortrait(str(meta), quiet=True)
    bunches = [pplib.load_data(n, dedisperse=True, dededisperse=False,
                               tscrunch=True, pscrunch=True, fscrunch=False,
                               quiet=True) for n in names]
    ref = pplib.DataPortrait(bunches)
    assert dp.njoin == 2 and dp.datafiles == names and dp.metafile == str(meta)
    assert (dp.nchan, dp.nchanx, dp.nbin) == (16, 15, 256)
    assert (np.diff(dp.freqs[0]) > 0).all()
    assert any(np.any(np.diff(ic) > 1) for ic in dp.join_ichans)
    for a in ("port", "portx", "freqs", "noise_stdsxs", "SNRsxs", "masks",
              "join_params", "join_fit_flags", "isort", "isortx", "weights"):
        np.testing.assert_array_equal(getattr(dp, a), getattr(ref, a), a)
    for a in ("join_ichans", "join_ichanxs"):
        for x, y in zip(getattr(dp, a), getattr(ref, a)):
            np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(dp.freqsxs[0], ref.freqsxs[0])
    assert dp.Ps == ref.Ps
    for ia, b in enumerate(bunches):
        jic = dp.join_ichans[ia]
        np.testing.assert_array_equal(dp.freqs[0, jic], b.freqs[0])
        np.testing.assert_array_equal(
            dp.port[jic], np.asarray(b.subints[0, 0]) * b.masks[0, 0])
    # the zero-weight channel of the second archive is condensed away
    assert len(dp.join_ichanxs[1]) == 7 and len(dp.join_ichanxs[0]) == 8
    # the second archive was written 0.03 rot later: the start value finds it
    assert dp.join_params[0] == 0.0 and abs(abs(dp.join_params[2]) - 0.03) < 0.01
