"""Every FFT plan class through the row kernels and the fit (tests/
fftplans.py; the host side of the same lengths: tests/
test_fftplans_inputs.py).

The stage sequence of the block and wave transforms is chosen at run time
from the factorisation of the transform length, and a wrong twiddle index
or span gives plausible numbers, not a crash.  Each row kernel is compared
at every length of fftplans.ROW_LENGTHS with its NumPy arithmetic or the
oracle, at the bar the project already holds at the neighbouring lengths,
and the same call made twice must be bitwise equal; each case of
fftplans.FIT_CASES is one engine.fit_batch call of four sub-ints against
the oracle's fit of the kept channels (ragged.compare_row).

Rows: three rows of unit-variance normals seeded by nbin, f32 and f64 input
alternating from length to length."""
import numpy as np
import pytest

import fftplans as F
import goldens as G
import ragged as R
from test_gpu_parity import GAUSS_ATOL

pytestmark = pytest.mark.gpu

SIG = G.SIGMA_TOL
PHASES = np.array([0.2718, -0.4999, 0.0])       # one per row
EVEN = [n for n in F.ROW_LENGTHS if n % 2 == 0]


def _plan(nbin):
    N = F.rfft_len(nbin)
    return "N=%d %s KMAX %d" % (N, "x".join(map(str, F.fft_radices(N)))
                                if F.stages(N) else "pow2", F.kmax(nbin))


def _rows(nbin, n=3):
    """(the rows as the device gets them, the same values in float64)."""
    x = F.rows(nbin, n).astype(F.row_dtype(nbin))
    return x, x.astype(np.float64)


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("nbin", F.ROW_LENGTHS)
def test_rotate_rows_match_numpy(nbin):
    """k_rotate through engine.rotate_rows (nbin samples) and its ref_len
    form (the reference's length-less irfft: nbin - 1 samples at odd nbin,
    forward at nbin points and inverse at (nbin - 1) / 2), one phase per
    row, and through pplib.rotate_data / rotate_portrait, against rfft x
    phasor x irfft at test_rotate_any_nbin_matches_numpy's atol 1e-11."""
    from pulseportraiture_amd import engine, pplib
    x, x64 = _rows(nbin)
    k = np.arange(nbin // 2 + 1)
    X = np.fft.rfft(x64, axis=-1)
    Xr = X * np.exp(2j * np.pi * np.outer(PHASES, k))
    full, ref = np.fft.irfft(Xr, n=nbin, axis=-1), np.fft.irfft(Xr, axis=-1)
    assert ref.shape[-1] == nbin - nbin % 2
    got = _np(engine.rotate_rows(x, PHASES))
    got_ref = _np(engine.rotate_rows(x, PHASES, ref_len=True))
    # the public routines take one phase for all rows
    pub = []
    for ph, fn in ((PHASES[0], pplib.rotate_data),
                   (PHASES[1], pplib.rotate_portrait)):
        pub.append((fn(x, ph),
                    np.fft.irfft(X * np.exp(2j * np.pi * k * ph), axis=-1)))
    print("FFTPLANS rotate %d (%s): max |dev| %.1e (nbin) %.1e (ref_len) "
          "%.1e %.1e (pplib)" %
          ((nbin, _plan(nbin), np.abs(got - full).max(),
            np.abs(got_ref - ref).max()) +
           tuple(np.abs(g - w).max() for g, w in pub)))
    np.testing.assert_allclose(got, full, rtol=0, atol=1e-11)
    np.testing.assert_allclose(got_ref, ref, rtol=0, atol=1e-11)
    for g, w in pub:
        np.testing.assert_allclose(g, w, rtol=0, atol=1e-11)
    # the row with phase 0 comes back
    np.testing.assert_allclose(got[2], x64[2], rtol=0, atol=1e-11)
    np.testing.assert_array_equal(_np(engine.rotate_rows(x, PHASES)), got)
    np.testing.assert_array_equal(
        _np(engine.rotate_rows(x, PHASES, ref_len=True)), got_ref)


@pytest.mark.parametrize("nbin", F.ROW_LENGTHS)
def test_noise_rows_match_numpy(nbin):
    """k_noise (get_noise_PS, pplib.py:2312-2338) against the NumPy
    arithmetic of test_noise_matches_reference, rtol 1e-12."""
    from pulseportraiture_amd import engine
    x, x64 = _rows(nbin)
    Fx = np.fft.rfft(x64, axis=-1)
    p = np.real(Fx * np.conj(Fx)) / nbin
    want = np.sqrt(np.mean(p[:, int((1 - 4 ** -1) * p.shape[-1]):], axis=-1))
    got = _np(engine.noise_rows(x))
    print("FFTPLANS noise %d (%s): max rel dev %.1e" %
          (nbin, _plan(nbin), np.abs(got / want - 1).max()))
    np.testing.assert_allclose(got, want, rtol=1e-12)
    np.testing.assert_array_equal(_np(engine.noise_rows(x)), got)


@pytest.mark.parametrize("nbin", F.ROW_LENGTHS)
def test_resid_chi2_rows_match_oracle(nbin):
    """k_resid_chi2 (rotation at full length, then the residual against one
    of two model rows) against oracle.channel_red_chi2s, rtol 1e-12."""
    import oracle as O
    from pulseportraiture_amd import engine
    x, x64 = _rows(nbin)
    rng = np.random.default_rng(nbin + 1)
    mrows = rng.normal(size=(2, nbin))
    mi = np.array([1, 0, 1], dtype=np.int32)
    sc, er = rng.uniform(0.5, 2.0, 3), rng.uniform(0.5, 1.5, 3)
    want = O.channel_red_chi2s(x64, PHASES, mrows[mi], sc, er, nbin - 2.0)
    got = _np(engine.resid_chi2_rows(x, PHASES, mrows, mi, sc, er,
                                     nbin - 2.0))
    print("FFTPLANS resid_chi2 %d (%s): max rel dev %.1e" %
          (nbin, _plan(nbin), np.abs(got / want - 1).max()))
    np.testing.assert_allclose(got, want, rtol=1e-12)
    np.testing.assert_array_equal(
        _np(engine.resid_chi2_rows(x, PHASES, mrows, mi, sc, er, nbin - 2.0)),
        got)


def _shifted(models, which, shifts, nbin, rng):
    import oracle as O
    d = np.stack([O.rotate_rows(models[m][None, :] * 2.5, [-s])[0] +
                  rng.normal(scale=0.05, size=nbin)
                  for m, s in zip(which, shifts)]).astype(F.row_dtype(nbin))
    return d, d.astype(np.float64)


def _phase_shift_close(tag, got, want):
    assert abs(G.phase_diff(got[0], want["phase"])) < \
        SIG * want["phase_err"], (tag, got, want)
    assert abs(got[1] / want["phase_err"] - 1) < 1e-4, (tag, got, want)
    assert abs(got[2] / want["scale"] - 1) < 1e-6, (tag, got, want)
    assert abs(got[4] / want["snr"] - 1) < 1e-6, (tag, got, want)
    return abs(G.phase_diff(got[0], want["phase"])) / want["phase_err"]


@pytest.mark.parametrize("nbin", F.ROW_LENGTHS)
def test_phase_shift_batch_matches_oracle(nbin):
    """k_phase_shift (pplib.fit_phase_shift, pplib.py:2136-2182) against the
    oracle's brute + fmin at the bars of
    test_odd_nbin_block_kernels_match_oracle: three shifted noisy profiles
    with the defaults; with bounds = (-0.2, 0.3) and a given per-profile
    noise; with two models and a model_index."""
    import oracle as O
    from pulseportraiture_amd import engine
    rng = np.random.default_rng(nbin + 2)
    ph = np.linspace(0, 1, nbin, endpoint=False)
    models = np.stack([
        np.exp(-0.5 * ((ph - 0.4) / 0.03) ** 2) +
        0.3 * np.exp(-0.5 * ((ph - 0.55) / 0.05) ** 2),
        np.exp(-0.5 * ((ph - 0.6) / 0.045) ** 2) +
        0.5 * np.exp(-0.5 * ((ph - 0.3) / 0.06) ** 2)])
    worst = 0.0
    # the defaults
    d, d64 = _shifted(models, (0, 0, 0), (0.123, -0.31, 0.0), nbin, rng)
    got = _np(engine.phase_shift_batch(d, models[0]))
    for i in range(3):
        worst = max(worst, _phase_shift_close(
            ("default", i), got[i], O.fit_phase_shift(d64[i], models[0])))
    np.testing.assert_array_equal(
        _np(engine.phase_shift_batch(d, models[0])), got)
    # bounds and noise given (shifts inside the bounds: the brute grid is
    # another, the minimum the same)
    d, d64 = _shifted(models, (0, 0, 0), (0.123, -0.15, 0.27), nbin, rng)
    noise = np.array([0.05, 0.04, 0.07])
    kw = dict(noise=noise, bounds=(-0.2, 0.3))
    got = _np(engine.phase_shift_batch(d, models[0], **kw))
    for i in range(3):
        worst = max(worst, _phase_shift_close(
            ("bounds", i), got[i], O.fit_phase_shift(
                d64[i], models[0], noise=noise[i], bounds=(-0.2, 0.3))))
    np.testing.assert_array_equal(
        _np(engine.phase_shift_batch(d, models[0], **kw)), got)
    # two models
    mi = np.array([1, 0, 1], dtype=np.int32)
    d, d64 = _shifted(models, mi, (-0.41, 0.2, 0.05), nbin, rng)
    got = _np(engine.phase_shift_batch(d, models, model_index=mi))
    for i in range(3):
        worst = max(worst, _phase_shift_close(
            ("index", i), got[i], O.fit_phase_shift(d64[i], models[mi[i]])))
    np.testing.assert_array_equal(
        _np(engine.phase_shift_batch(d, models, model_index=mi)), got)
    print("FFTPLANS phase_shift %d (%s): max phase dev %.1e sigma" %
          (nbin, _plan(nbin), worst))


@pytest.mark.parametrize("nbin", EVEN)
def test_inst_response_rows_match_numpy(nbin):
    """k_inst_resp (even nbin only) against the NumPy restatement of
    test_inst_response_kernel_matches_numpy, atol 1e-11: five rows fanned
    out of two sources, with and without a table."""
    from pulseportraiture_amd import engine
    src = F.rows(nbin, 2)
    src_row = np.array([1, 0, 0, 1, 0], dtype=np.int32)
    k = np.arange(nbin // 2 + 1)
    w = np.array([0.0, 0.013, 3.3 / len(k), 0.1, 1e-4])
    T = np.sinc(k * 0.02) * np.exp(-(np.pi * k * 0.01) ** 2 / (4 * np.log(2)))
    X = np.fft.rfft(src[src_row], axis=-1) * np.sinc(np.outer(w, k))
    devs = []
    for table, spec in ((None, X), (T, X * T)):
        want = np.fft.irfft(spec, axis=-1)
        got = _np(engine.inst_response_rows(src, src_row, table, w))
        assert got.shape == want.shape == (5, nbin)
        devs.append(np.abs(got - want).max())
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-11)
        np.testing.assert_array_equal(
            _np(engine.inst_response_rows(src, src_row, table, w)), got)
    print("FFTPLANS inst_response %d (%s): max |dev| %.1e (no table) %.1e" %
          (nbin, _plan(nbin), devs[0], devs[1]))


@pytest.mark.parametrize("nbin", F.ROW_LENGTHS)
def test_gauss_portrait_matches_oracle(nbin):
    """k_gauss_port through pplib.gen_gaussian_portrait, without and with
    scattering (tau = 0.02 bin: rfft, 1 / (1 + 2 pi i k tau_n), irfft; at
    odd nbin forward at nbin points, inverse at (nbin - 1) / 2, nbin - 1
    bins out), against oracle.gen_gaussian_portrait at GAUSS_ATOL x the
    portrait's maximum; eight channels of the example template."""
    import oracle as O
    from pulseportraiture_amd import pplib
    c = G.gauss_case(G.gauss(), "example_64x512")
    freqs = np.asarray(c["freqs"])[::8]
    devs = []
    for tau in (0.0, 0.02):
        prm = np.array(c["params"], dtype=float)
        prm[1] = tau
        args = (c["code"], prm, c["alpha"], np.zeros(nbin), freqs,
                c["nu_ref"])
        got = pplib.gen_gaussian_portrait(*args)
        want = O.gen_gaussian_portrait(*args)
        assert got.shape == want.shape == \
            (len(freqs), nbin - (nbin % 2 and tau != 0))
        devs.append(np.abs(got - want).max() / np.abs(want).max())
        np.testing.assert_array_equal(pplib.gen_gaussian_portrait(*args), got)
    print("FFTPLANS gauss_portrait %d (%s): max rel dev %.1e (tau 0) %.1e" %
          (nbin, _plan(nbin), devs[0], devs[1]))
    assert max(devs) <= GAUSS_ATOL, devs


@pytest.mark.parametrize("nbin", F.ROW_LENGTHS)
def test_align_accum_matches_numpy(nbin):
    """k_align_part / k_align_fin: three sub-ints of five channels summed in
    the frequency domain against the rotate-then-sum of
    test_align_accum_matches_numpy, accumulated twice as there, at its
    atol of 1e-12 x max |sum|."""
    import torch
    import oracle as O
    from pulseportraiture_amd import engine
    rng = np.random.default_rng(nbin + 3)
    nsub, nchan = 3, 5
    x = rng.normal(size=(nsub, nchan, nbin)).astype(F.row_dtype(nbin))
    ph = rng.uniform(-0.5, 0.5, size=(nsub, nchan))
    w = rng.uniform(0.1, 2.0, size=(nsub, nchan))
    w[1, 3] = 0.0

    def run(n):
        out = torch.zeros((nchan, nbin), dtype=torch.float64, device="cuda")
        ws = torch.zeros(nchan, dtype=torch.float64, device="cuda")
        for _ in range(n):
            engine.align_accum(x, ph, w, out, ws)
        return _np(out), _np(ws)
    ref = np.zeros((nchan, nbin))
    for s in range(nsub):
        ref += w[s][:, None] * O.rotate_rows(x[s].astype(np.float64), ph[s])
    once, wonce = run(1)
    twice, wtwice = run(2)
    print("FFTPLANS align_accum %d (%s): max |dev| / max |sum| %.1e" %
          (nbin, _plan(nbin), np.abs(twice - 2 * ref).max() /
           np.abs(ref).max()))
    np.testing.assert_allclose(twice, 2 * ref, rtol=0,
                               atol=1e-12 * np.abs(ref).max())
    np.testing.assert_allclose(wtwice, 2 * w.sum(axis=0), rtol=1e-14)
    again, wagain = run(1)
    np.testing.assert_array_equal(again, once)
    np.testing.assert_array_equal(wagain, wonce)


def test_refused_lengths_return_eunsup():
    """The lengths the restated nbin_supported refuses, asked of the library
    with a context: PPF_EUNSUP before any argument is read (NULL pointers)
    or anything launched -- 30 and 31 everywhere, the odd 4097 on the entry
    points that have no long-row path of their own, 8194 (and odd nbin) on
    ppf_inst_response_batch."""
    from pulseportraiture_amd import _lib, engine
    lib = _lib.load()
    ctx = _lib.context(engine.device().index)
    N = None

    def calls(nbin):
        return dict(
            rotate=lambda: lib.ppf_rotate_batch(ctx, 1, nbin, 1, N, N, N, N),
            rotate_ref=lambda: lib.ppf_rotate_batch_ref(ctx, 1, nbin, 1, N, N,
                                                        N, N),
            noise=lambda: lib.ppf_noise_batch(ctx, 1, nbin, 1, N, 4, N, N),
            resid=lambda: lib.ppf_resid_chi2_batch(ctx, 1, nbin, 1, N, N, N,
                                                   N, N, N, 1.0, N, N),
            align=lambda: lib.ppf_align_accum(ctx, 1, 1, nbin, 1, N, N, N, N,
                                              N, N, 0, N),
            inst=lambda: lib.ppf_inst_response_batch(ctx, 1, nbin, N, N, N, N,
                                                     N, N),
            shift=lambda: lib.ppf_phase_shift_batch(ctx, 1, nbin, 1, N, N, N,
                                                    N, 100, -0.5, 0.5, N, N),
            gauss=lambda: lib.ppf_gauss_portrait_batch(ctx, 1, 1, nbin, 1,
                                                       b"000", N, N, N, N, N,
                                                       N))
    for nbin in (30, 31):
        assert not F.nbin_supported(nbin)
        for name, f in calls(nbin).items():
            assert f() == _lib.PPF_EUNSUP, (name, nbin)
    assert not F.nbin_supported(4097)
    for name in ("rotate", "rotate_ref", "noise", "resid", "align", "inst"):
        assert calls(4097)[name]() == _lib.PPF_EUNSUP, name
    assert not F.nbin_supported(8194)
    for nbin in (8194, 33, 4095):
        assert calls(nbin)["inst"]() == _lib.PPF_EUNSUP, nbin
    with pytest.raises(NotImplementedError):
        _lib.check(calls(8194)["inst"](), ctx)


# ------------------------------------------------------------------- fits ---
def _compare(c, r, j, i):
    b = R.inputs(c)
    return R.compare_row("FFTPLANS %s sub %d" % (c["name"], i),
                         (c["name"], i), r, j, R.oracle_fit(c, i),
                         b["keep"][i], b["P"], b["scat"])


@pytest.mark.parametrize("name", F.FIT_NAMES)
def test_fit_batch_matches_oracle(name):
    """One engine.fit_batch call of the case's four sub-ints (the four masks
    of ragged.masks; host-built inputs) against the oracle's fit of the kept
    channels at the project's bars (ragged.compare_row): the leading radix
    2, radix 7 and two generic stages in k_xspec_wm / k_xspec_wo, both of
    their instantiations on either side of 512 points, k_xspec_any with even
    and odd nbin and its guess pass k_dsum<8>, k_dsum_wn<1024 | 2048>."""
    c = F.fit_case(name)
    r = R.device_fit(c)
    worst = [_compare(c, r, i, i) for i in range(R.inputs(c)["nsub"])]
    print("FFTPLANS fit %s (%s, N=%d %s): worst dev %.2e sigma, chi2_red "
          "rel %.1e" % (name, F.fit_path(name), F.rfft_len(c["nbin"]),
                        "x".join(map(str, F.fft_radices(
                            F.rfft_len(c["nbin"])))),
                        max(w[0] for w in worst), max(w[1] for w in worst)))


@pytest.mark.parametrize("name", F.SINGLE_EQUALS_BATCH)
def test_fit_single_equals_batch(name):
    """Each sub-int fitted alone is bitwise the batch's (as
    test_ragged_single_equals_batch), on a wave kernel and on
    k_xspec_any."""
    c = F.fit_case(name)
    full = R.device_fit(c)
    for i in range(R.inputs(c)["nsub"]):
        one = R.device_fit(c, [i])
        for k in ("results", "scales", "scale_errs", "channel_snrs",
                  "covariance"):
            np.testing.assert_array_equal(one[k][0], full[k][i],
                                          err_msg="%s sub %d" % (k, i))


def test_long_rows_chunked_equal_unchunked():
    """The long transforms with more rows than one 256-MB chunk of work rows
    holds (at 4097 and 8194 bins the plan is M = 16384: 512 rows per chunk):
    a row's transform does not depend on its chunk, so the same rows sent as
    two calls that fit one chunk each are bitwise equal.
    (a) 600 f32 rows of 4097 bins through ppf_noise_long (also against
    NumPy's rFFT at test_noise_long_rows_match_numpy's rtol 1e-11) and
    ppf_rotate_long; (b) one fit of 10 sub-ints x 64 channels at 8194 bins
    (phase + DM, GetTOAs guess: 640 data rows through long_rfft_rows)
    against the same sub-ints as two calls of 5."""
    from pulseportraiture_amd import engine
    rng = np.random.default_rng(4097)
    x = rng.normal(size=(600, 4097)).astype(np.float32)
    ph = rng.uniform(-0.5, 0.5, 600)
    noise = _np(engine.noise_rows_long(x))
    np.testing.assert_array_equal(
        noise, np.concatenate([_np(engine.noise_rows_long(x[:300])),
                               _np(engine.noise_rows_long(x[300:]))]))
    F64 = np.fft.rfft(x.astype(np.float64), axis=-1)
    p = np.real(F64 * np.conj(F64)) / x.shape[-1]
    np.testing.assert_allclose(
        noise, np.sqrt(np.mean(p[:, int((1 - 4 ** -1) * p.shape[-1]):],
                               axis=-1)), rtol=1e-11)
    np.testing.assert_array_equal(
        _np(engine.rotate_rows(x, ph)),
        np.concatenate([_np(engine.rotate_rows(x[:300], ph[:300])),
                        _np(engine.rotate_rows(x[300:], ph[300:]))]))
    # (b) the case's four sub-ints (ragged.masks), repeated to ten
    c = R._case("long", 8194, 64, R.PD, guess=True)
    subs = [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    full = R.device_fit(c, subs)
    halves = [R.device_fit(c, subs[:5]), R.device_fit(c, subs[5:])]
    for k in ("results", "scales", "scale_errs", "channel_snrs",
              "covariance"):
        np.testing.assert_array_equal(
            full[k], np.concatenate([h[k] for h in halves]), err_msg=k)
