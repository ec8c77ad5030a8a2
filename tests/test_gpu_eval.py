"""GPU: the likelihood evaluators (ppf_eval_batch, ppf_eval.hip) against the
reference's goldens (tests/golden/eval.npz), the oracle, and themselves.

Bars (tests/evalcases.py): a per-channel term within 256 eps of its absolute
companion; f, g, H within 256 eps of their propagated scale; the covariance
within cond(H) 256 eps |scale| / |H| relative.  Every test prints the largest
error / (eps * scale) it met.  Measured on one MI355X: terms 151 (c65x33),
f / g / H 17, per-channel H 30, scales 38, the pplib families 7, the batch of
three problems 35; covariance 1.4e-13 relative against a bar of 5e-5.
"""
import numpy as np
import pytest

import evalcases as E
import oracle as O

pytestmark = pytest.mark.gpu

NAMES = [E.case_name(*s) for s in E.SHAPES]
EPS = E.EPS


def _args(p):
    return (p["D"], p["M"], p["errs_FT"], p["P"], p["freqs"]) + tuple(p["nus"])


def _terms(bunch, i):
    return {k: v[i] for k, v in bunch.items()}


_CACHE = {}


def _dev(shape, mode):
    """The device's evaluation of every golden point of a case and mode,
    both flag patterns (computed once, shared)."""
    from pulseportraiture_amd import pptoaslib
    key = (shape, mode)
    if key not in _CACHE:
        p = E.inputs(*shape)
        th = E.golden()["%s/%s/theta" % (E.case_name(*shape), mode)]
        lt = mode == "log"
        a = pptoaslib.eval_portrait_full(th, *_args(p), fit_flags=E.FLAGS_A,
                                         log10_tau=lt, per_channel=True)
        b = pptoaslib.eval_portrait_full(th, *_args(p), fit_flags=E.FLAGS_B,
                                         log10_tau=lt)
        _CACHE[key] = (p, th, a, b)
    return _CACHE[key]


@pytest.mark.parametrize("mode", ["log", "lin"])
@pytest.mark.parametrize("shape", E.SHAPES, ids=NAMES)
def test_terms_f_g_H_against_the_reference(shape, mode):
    G = E.golden()
    pre = "%s/%s/" % (E.case_name(*shape), mode)
    p, th, a, b = _dev(shape, mode)
    assert str(G[E.case_name(*shape) + "/sha"]) == E.input_sha(p)
    rt = rf = rs = 0.0
    for i in range(len(th)):
        t = _terms(a.terms, i)
        rt = max(rt, E.terms_ratio(t, G[pre + "terms"][i], G[pre + "hat"][i]))
        rf = max(rf, E.ratio(a.f[i], G[pre + "f"][i], G[pre + "sf"][i]),
                 E.ratio(a.grad[i], G[pre + "g"][i], G[pre + "sg"][i]),
                 E.ratio(a.hess[i], G[pre + "H"][i], G[pre + "sH"][i]),
                 E.ratio(b.grad[i], G[pre + "gB"][i], G[pre + "sg"][i]),
                 E.ratio(b.hess[i], G[pre + "HB"][i], G[pre + "sH"][i]))
        assert np.all(b.grad[i][[2, 4]] == 0.0)
        assert np.all(b.hess[i][[2, 4]] == 0.0)
        assert np.all(b.hess[i][:, [2, 4]] == 0.0)
        np.testing.assert_array_equal(a.hess[i], a.hess[i].T)
        # the scales C / S: |C / S| (C^ / |C| + S^ / S)
        h = E.unpack_terms(G[pre + "hat"][i].astype(float))
        r = E.unpack_terms(G[pre + "terms"][i])
        sc = h["C"] / r["S"] + np.abs(r["C"]) * h["S"] / r["S"] ** 2
        rs = max(rs, E.ratio(t["C"] / t["S"], G[pre + "scl"][i], sc))
    print("%s%s: terms %.1f, f/g/H %.1f, scales %.1f (x eps x scale)" %
          (pre, "", rt, rf, rs))
    assert rt <= E.BAR_EPS and rf <= E.BAR_EPS and rs <= E.BAR_EPS


@pytest.mark.parametrize("shape", sorted(E.PER_CHANNEL_H),
                         ids=lambda s: E.case_name(*s))
def test_per_channel_hessian_and_return_tuples(shape):
    """fit_portrait_full_function_2deriv's return rules: the bare Hessian,
    or a tuple with the covariance and / or the scales appended in that
    order; per_channel gives [5, 5, nchan]."""
    from pulseportraiture_amd import pptoaslib as pl
    G = E.golden()
    name = E.case_name(*shape)
    p = E.inputs(*shape)
    worst = 0.0
    for mode, lt in (("log", True), ("lin", False)):
        pre = "%s/%s/" % (name, mode)
        for i in (0, 1, 3):
            th = G[pre + "theta"][i]
            out = pl.fit_portrait_full_function_2deriv(
                th, *_args(p), np.array(E.FLAGS_A), lt, per_channel=True,
                return_scales=True)
            assert isinstance(out, tuple) and len(out) == 2
            assert out[0].shape == (5, 5, shape[0])
            assert out[1].shape == (shape[0],)
            worst = max(worst, E.ratio(out[0], G[pre + "Hn"][i],
                                       G[pre + "sHn"][i].astype(float)))
    H = pl.fit_portrait_full_function_2deriv(th, *_args(p),
                                             np.array(E.FLAGS_A), lt)
    assert isinstance(H, np.ndarray) and H.shape == (5, 5)
    print("%s: per-channel H %.1f x eps x scale" % (name, worst))
    assert worst <= E.BAR_EPS


def _cov_bar(H, sH, ifit):
    Hs, ss = H[np.ix_(ifit, ifit)], sH[np.ix_(ifit, ifit)]
    return (np.linalg.cond(Hs) * E.BAR_EPS * EPS * np.linalg.norm(ss) /
            np.linalg.norm(Hs))


def test_reference_signatures_pptoaslib():
    """The four pptoaslib signatures at one point of the small case, both
    flag patterns: values, shapes, tuples, the covariance matrices."""
    from pulseportraiture_amd import pptoaslib as pl
    G = E.golden()
    shape = E.WITH_SCALES
    name = E.case_name(*shape)
    p = E.inputs(*shape)
    a = _args(p)
    th = G[name + "/log/theta"][0]
    n = shape[0]
    for tag, fl, gk, hk in (("A", E.FLAGS_A, "g", "H"),
                            ("B", E.FLAGS_B, "gB", "HB")):
        fl = np.array(fl)
        ifit = np.where(fl)[0]
        sH = G[name + "/log/sH"][0]
        f = pl.fit_portrait_full_function(th, *a, fl, True)
        assert np.ndim(f) == 0
        assert E.ratio(f, G[name + "/log/f"][0], G[name + "/log/sf"][0]) <= 256
        g = pl.fit_portrait_full_function_deriv(th, *a, fl, True)
        assert g.shape == (5,)
        assert E.ratio(g, G[name + "/log/" + gk][0],
                       G[name + "/log/sg"][0]) <= 256
        H, cov = pl.fit_portrait_full_function_2deriv(
            th, *a, fl, True, return_covariance_matrix=True)
        assert E.ratio(H, G[name + "/log/" + hk][0], sH) <= 256
        ref = G["%s/cov%s" % (name, tag)]
        assert cov.shape == ref.shape == (len(ifit),) * 2
        bar = _cov_bar(G[name + "/log/" + hk][0], sH, ifit)
        err = np.linalg.norm(cov - ref) / np.linalg.norm(ref)
        print("cov%s: relative error %.2e, bar %.2e" % (tag, err, bar))
        assert err <= bar
        Hn, cov2, scl = pl.fit_portrait_full_function_2deriv(
            th, *a, fl, True, per_channel=True,
            return_covariance_matrix=True, return_scales=True)
        assert Hn.shape == (5, 5, n) and scl.shape == (n,)
        np.testing.assert_array_equal(cov2, cov)
        # with the scales as parameters
        Hs, covs, scl2 = pl.fit_portrait_full_function_2deriv_with_scales(
            th, *a, fl, True, return_covariance_matrix=True,
            return_scales=True)
        rH, rc = G["%s/ws%s/H" % (name, tag)], G["%s/ws%s/cov" % (name, tag)]
        assert Hs.shape == rH.shape == (5 + n, 5 + n)
        assert covs.shape == rc.shape == (len(ifit) + n,) * 2
        # entries are -2 (C d2C / S - C^2 d2S / 2 S^2) f f, -2 (dC - C dS / S)
        # f and 2 S: bars from the same propagation
        h = E.unpack_terms(G[name + "/log/hat"][0].astype(float))
        r = E.unpack_terms(G[name + "/log/terms"][0])
        C, S, Ch, Sh = r["C"], r["S"], h["C"], h["S"]
        sw = np.zeros_like(rH)
        for i in range(5):
            for j in range(5):
                sw[i, j] = 2 * np.sum(
                    E._prop(1.0, [(C, Ch, 1), (r["d2C"][i, j], h["d2C"][i, j],
                                               1), (S, Sh, -1)]) +
                    E._prop(0.5, [(C, Ch, 2), (r["d2S"][i, j], h["d2S"][i, j],
                                               1), (S, Sh, -2)]))
            sw[i, 5:] = sw[5:, i] = 2 * (h["dC"][i] + E._prop(
                1.0, [(C, Ch, 1), (r["dS"][i], h["dS"][i], 1), (S, Sh, -1)]))
        sw[5:, 5:] = np.diag(2 * Sh)
        assert E.ratio(Hs, rH, sw) <= 256
        assert E.ratio(scl2, G["%s/ws%s/scl" % (name, tag)],
                       Ch / S + np.abs(C) * Sh / S ** 2) <= 256
        sel = np.concatenate([ifit, 5 + np.arange(n)])
        bar = (np.linalg.cond(rH[np.ix_(sel, sel)]) * 256 * EPS *
               np.linalg.norm(sw[np.ix_(sel, sel)]) /
               np.linalg.norm(rH[np.ix_(sel, sel)]))
        err = np.linalg.norm(covs - rc) / np.linalg.norm(rc)
        print("with_scales cov%s: relative error %.2e, bar %.2e" %
              (tag, err, bar))
        assert err <= bar
    cube = pl.fit_portrait_full_function_2deriv_with_scales(
        th, *a, np.array(E.FLAGS_A), True, per_channel=True)
    ref = G[name + "/wsA/Hn"]
    assert cube.shape == ref.shape == (5 + n, 5 + n, n)
    assert E.ratio(cube.sum(axis=-1), G[name + "/wsA/H"], sw) <= E.BAR_EPS
    assert E.ratio(cube, ref, sw[:, :, None]) <= E.BAR_EPS
    assert np.all((cube == 0.0) == (ref == 0.0))


@pytest.mark.parametrize("shape", [(3, 17), (67, 65), (2, 4100)],
                         ids=lambda s: E.case_name(*s))
def test_reference_signatures_pplib(shape):
    """pplib.fit_portrait_function / _deriv / _2deriv (p_n in place of S,
    the P / freqs = None branch, nu_zero) and fit_phase_shift_function /
    _deriv / _2deriv on the same spectra, at a near and a far point."""
    from pulseportraiture_amd import pplib
    G = E.golden()
    name = E.case_name(*shape)
    p = E.inputs(*shape)
    D, M, e, P, fr = _args(p)[:5]
    nu = p["nus"][0]
    p_n = np.real(np.sum(M * np.conj(M), axis=1))
    worst = 0.0
    for i in (0, 4):
        th = G[name + "/log/theta"][i]
        x = th[:2]
        g = {k: G["%s/pplib%d/%s" % (name, i, k)] for k in
             ("fp", "fp_noP", "fp_d", "fp_2d", "fp_nz", "ps", "ps_d", "ps_2d")}
        # Cdp, its phase derivatives and their companions (unit errors)
        one = np.ones(len(fr))
        t = O.channel_terms([x[0], x[1], 0, 0, 0], D, M, one, P, fr, nu,
                            np.inf, 1.0, False)
        h = E.companions([x[0], x[1], 0, 0, 0], D, M, one, P, fr, nu, np.inf,
                         1.0, False)
        w = 1.0 / (e ** 2 * p_n)
        C, d1, d2 = t["C"], t["dC"][0], t["d2C"][0, 0]
        Ch, d1h, d2h = h["C"], h["dC"][0], h["d2C"][0, 0]
        dDM = (fr ** -2.0 - nu ** -2.0) * (E.DCONST / P)
        f = pplib.fit_portrait_function(x, M, p_n, D, e, P, fr, nu)
        r = [E.ratio(f, g["fp"], np.sum(2 * np.abs(C) * Ch * w))]
        f0 = pplib.fit_portrait_function(x, M, p_n, D, e, None, None, nu)
        a0 = ([x[0], 0, 0, 0, 0], D, M, one, 1.0, one, np.inf, np.inf, 1.0,
              False)
        r.append(E.ratio(f0, g["fp_noP"], np.sum(
            2 * np.abs(O.channel_terms(*a0)["C"]) * E.companions(*a0)["C"] *
            w)))
        sg = 2 * (Ch * np.abs(d1) + np.abs(C) * d1h) * w
        gd = pplib.fit_portrait_function_deriv(x, M, p_n, D, e, P, fr, nu)
        assert gd.shape == (2,)
        r.append(E.ratio(gd, g["fp_d"], [sg.sum(), (sg * np.abs(dDM)).sum()]))
        sW = (2 * np.abs(d1) * d1h + Ch * np.abs(d2) + np.abs(C) * d2h) * w
        h2, nz = pplib.fit_portrait_function_2deriv(x, M, p_n, D, e, P, fr, nu)
        assert h2.shape == (3,)
        r.append(E.ratio(h2, g["fp_2d"], [2 * sW.sum(), 2 * (sW * dDM ** 2).sum(),
                                          2 * (sW * np.abs(dDM)).sum()]))
        Wn = (d1 ** 2 + C * d2) * w
        A, B = Wn.sum(), np.sum(Wn * fr ** -2)
        r.append(E.ratio(nz, g["fp_nz"], 0.5 * np.abs(g["fp_nz"]) * (
            sW.sum() / abs(A) + np.sum(sW * fr ** -2) / abs(B))))
        ps = [pplib.fit_phase_shift_function(x[0], M[0], D[0], e[0]),
              pplib.fit_phase_shift_function_deriv(x[0], M[0], D[0], e[0]),
              pplib.fit_phase_shift_function_2deriv(x[0], M[0], D[0], e[0])]
        hp = E.companions([x[0], 0, 0, 0, 0], D[:1], M[:1], e[:1], 1.0,
                          one[:1], np.inf, np.inf, 1.0, False)
        for v, k, s in zip(ps, ("ps", "ps_d", "ps_2d"),
                           (hp["C"][0], hp["dC"][0, 0], hp["d2C"][0, 0, 0])):
            assert np.ndim(v) == 0
            r.append(E.ratio(v, g[k], s))
        worst = max([worst] + r)
    print("%s: pplib families %.1f x eps x scale" % (name, worst))
    assert worst <= E.BAR_EPS


def _batch_call(poison, **kw):
    from pulseportraiture_amd import pptoaslib
    probs, models = E.batch_inputs()
    b = E.BATCH
    mask = np.array(b["mask"], dtype=np.uint8)
    D = np.array([p["D"] for p in probs])
    if poison:
        D[mask == 0] = np.nan + 1j * np.nan
    G = E.golden()
    th = np.array([G["batch%d/log/theta" % s] for s in range(3)])
    r = pptoaslib.eval_portrait_full(
        th, D, models, np.array([p["errs_FT"] for p in probs]),
        np.array([p["P"] for p in probs]),
        np.array([p["freqs"] for p in probs]),
        *np.array([p["nus"] for p in probs]).T, log10_tau=True,
        per_channel=True, mask=mask, model_index=b["model_index"], **kw)
    return probs, mask, th, r


def test_three_problems_shared_model_mask_and_poison():
    """nprob = 3 with their own P, freqs and reference frequencies, a shared
    model through model_index and ragged masks (one problem keeps a single
    channel), the masked channels' data NaN: each problem equals the
    reference on its unmasked channels; masked channels are exact zeros."""
    G = E.golden()
    probs, mask, th, r = _batch_call(True)
    assert r.f.shape == (3, 7) and r.hess.shape == (3, 7, 5, 5)
    rt = rf = 0.0
    for s in range(3):
        pre = "batch%d/log/" % s
        ok = mask[s] != 0
        for i in range(7):
            t = {k: v[s, i] for k, v in r.terms.items()}
            for k, v in t.items():
                assert np.all(v[..., ~ok] == 0.0), k
            t = {k: v[..., ok] for k, v in t.items()}
            rt = max(rt, E.terms_ratio(t, G[pre + "terms"][i],
                                       G[pre + "hat"][i]))
            rf = max(rf, E.ratio(r.f[s, i], G[pre + "f"][i], G[pre + "sf"][i]),
                     E.ratio(r.grad[s, i], G[pre + "g"][i], G[pre + "sg"][i]),
                     E.ratio(r.hess[s, i], G[pre + "H"][i], G[pre + "sH"][i]))
    print("batch: terms %.1f, f/g/H %.1f (x eps x scale)" % (rt, rf))
    assert np.all(np.isfinite(r.hess))
    assert rt <= E.BAR_EPS and rf <= E.BAR_EPS


def test_masked_equals_deleted_bitwise():
    """A masked (and poisoned) channel changes no bit of f, g, H or of the
    other channels' terms against the same problem with it deleted."""
    from pulseportraiture_amd import pptoaslib
    probs, mask, th, r = _batch_call(True)
    for s in (1, 2):
        p, ok = probs[s], mask[s] != 0
        m = E.batch_inputs()[1][E.BATCH["model_index"][s]]
        d = pptoaslib.eval_portrait_full(
            th[s], p["D"][ok], m[ok], p["errs_FT"][ok], p["P"],
            p["freqs"][ok], *p["nus"], log10_tau=True, per_channel=True)
        np.testing.assert_array_equal(d.f, r.f[s])
        np.testing.assert_array_equal(d.grad, r.grad[s])
        np.testing.assert_array_equal(d.hess, r.hess[s])
        for k in d.terms:
            np.testing.assert_array_equal(d.terms[k], r.terms[k][s][..., ok])


@pytest.mark.parametrize("shape", [(67, 65), (2, 4100)],
                         ids=lambda s: E.case_name(*s))
def test_k_points_equal_k_one_point_calls_bitwise(shape):
    """K in {1, 2, block - 1, block + 1}: a point's bits do not depend on
    the call it is in, nor on the call being repeated."""
    from pulseportraiture_amd import pptoaslib, engine
    pb = engine.eval_point_block()
    G = E.golden()
    p = E.inputs(*shape)
    name = E.case_name(*shape)
    th = np.concatenate([G[name + "/log/theta"], G[name + "/log/theta"][:3] +
                         [1e-3, 1e-4, 0.1, 0.01, 0.02]])[:pb + 1]
    assert len(th) == pb + 1

    def run(x, order=2):
        return pptoaslib.eval_portrait_full(x, *_args(p), log10_tau=True,
                                            per_channel=True, order=order)
    whole = run(th)
    again = run(th)
    ones = [run(th[i:i + 1]) for i in range(len(th))]
    for K in (2, pb - 1):
        part = run(th[1:1 + K])
        for k in ("f", "grad", "hess"):
            np.testing.assert_array_equal(part[k], whole[k][1:1 + K])
    for k in ("f", "grad", "hess"):
        np.testing.assert_array_equal(whole[k], again[k])
        np.testing.assert_array_equal(
            whole[k], np.concatenate([o[k] for o in ones]))
    for k in whole.terms:
        np.testing.assert_array_equal(whole.terms[k], again.terms[k])
        np.testing.assert_array_equal(
            whole.terms[k], np.concatenate([o.terms[k] for o in ones]))
    # the lower orders give the same f (and gradient) bits
    o1, o0 = run(th, 1), run(th, 0)
    assert o0.grad is None and o0.hess is None and o1.hess is None
    np.testing.assert_array_equal(o1.f, whole.f)
    np.testing.assert_array_equal(o0.f, whole.f)
    np.testing.assert_array_equal(o1.grad, whole.grad)
    # chunked over the points (a tiny byte budget): the same bits
    f, g, H, _ = engine.eval_points(th, *_args(p)[:5], p["nus"],
                                    log10_tau=True, max_bytes=1)
    np.testing.assert_array_equal(f.cpu().numpy()[0], whole.f)
    np.testing.assert_array_equal(H.cpu().numpy()[0], whole.hess)


def test_linear_tau_zero_is_exact():
    """Linear tau = 0: B = 1 and every tau / alpha derivative of C and S,
    and so of f, is exactly 0; C and S are the unscattered sums."""
    p, th, a, _ = _dev((67, 65), "lin")
    for i in (2, 3):
        assert th[i, 3] == 0.0
        t = _terms(a.terms, i)
        assert np.all(t["dC"][3:] == 0.0) and np.all(t["dS"] == 0.0)
        assert np.all(t["d2C"][3:] == 0.0) and np.all(t["d2C"][:, 3:] == 0.0)
        assert np.all(t["d2S"] == 0.0)
        assert np.all(a.grad[i][3:] == 0.0)
        assert np.all(a.hess[i][3:] == 0.0) and np.all(a.hess[i][:, 3:] == 0.0)
        assert np.all(t["dC"][0] != 0.0)
        S0 = np.sum(np.abs(p["M"]) ** 2, axis=-1) / p["errs_FT"] ** 2
        assert E.ratio(t["S"], S0, S0) <= E.BAR_EPS


def test_log10_tau_is_the_chain_rule_of_linear_tau():
    """log10_tau: tau = 10^theta_3 and d/dtheta_3 = ln 10 tau d/dtau."""
    from pulseportraiture_amd import pptoaslib
    p = E.inputs(5, 130)
    th = E.golden()["c5x130/log/theta"][[0, 5]]
    lin = th.copy()
    lin[:, 3] = 10.0 ** th[:, 3]
    a = pptoaslib.eval_portrait_full(th, *_args(p), log10_tau=True,
                                     per_channel=True)
    b = pptoaslib.eval_portrait_full(lin, *_args(p), log10_tau=False,
                                     per_channel=True)
    # (10^theta_3 on the host and on the device may differ in the last bit:
    # a relative 1e-16 of tau, far inside these)
    np.testing.assert_allclose(a.f, b.f, rtol=1e-12)
    k = E.LN10 * lin[:, 3]
    np.testing.assert_allclose(a.terms.dC[:, 3], k[:, None] * b.terms.dC[:, 3],
                               rtol=1e-11)
    np.testing.assert_allclose(a.terms.dS[:, 3], k[:, None] * b.terms.dS[:, 3],
                               rtol=1e-11)
    np.testing.assert_allclose(
        a.terms.d2S[:, 3, 3], k[:, None] ** 2 * b.terms.d2S[:, 3, 3] +
        E.LN10 * k[:, None] * b.terms.dS[:, 3], rtol=1e-9)


def test_harmonic_zero_is_summed_and_phase_is_not_wrapped():
    """Harmonic 0 counts as given: zeroing it changes C by Re(D_0 conj(M_0))
    / sigma^2 and S by |M_0|^2 / sigma^2 (B_0 = 1).  Per-channel phases far
    outside [-0.5, 0.5) (phase_shifts mod = False) agree with the oracle."""
    from pulseportraiture_amd import pptoaslib
    p = E.inputs(3, 17)
    th = E.golden()["c3x17/log/theta"][:1].copy()
    a = pptoaslib.eval_portrait_full(th, *_args(p), per_channel=True, order=0)
    q = dict(p, D=p["D"].copy(), M=p["M"].copy())
    q["D"][:, 0] = 0.0
    q["M"][:, 0] = 0.0
    b = pptoaslib.eval_portrait_full(th, *_args(q), per_channel=True, order=0)
    e2 = p["errs_FT"] ** 2
    dC = np.real(p["D"][:, 0] * np.conj(p["M"][:, 0])) / e2
    dS = np.abs(p["M"][:, 0]) ** 2 / e2
    assert np.all(np.abs(dC) > 0)
    h = E.companions(th[0], *_args(p), True)
    assert E.ratio(a.terms.C[0] - b.terms.C[0], dC, h["C"]) <= E.BAR_EPS
    assert E.ratio(a.terms.S[0] - b.terms.S[0], dS, h["S"]) <= E.BAR_EPS
    th[0, 0] += 7.0
    th[0, 1] += 9.0
    c = pptoaslib.eval_portrait_full(th, *_args(p), per_channel=True)
    t = O.channel_terms(th[0], *_args(p), True)
    ph = th[0, 0] + th[0, 1] * t["dphi"][1]
    assert np.all(np.abs(ph) > 2.0)
    h = E.companions(th[0], *_args(p), True)
    r = E.ratio(E.pack_terms(_terms(c.terms, 0)), E.pack_terms(t),
                E.pack_terms(h))
    print("unwrapped phases of %s turns: terms %.1f x eps x companion" %
          (np.round(ph, 1), r))
    assert r <= E.BAR_EPS


@pytest.mark.parametrize("nchan,nharm", [(7, 200), (130, 40)])
def test_against_the_oracle_at_other_shapes(nchan, nharm):
    """Two shapes the goldens do not hold, the oracle as the reference.  The
    oracle runs on this machine's NumPy, whose SIMD array power is not
    correctly rounded (nu ** -2 is an ulp off in a few channels of every
    array tried), while the device rounds nu^-2 once; nu^-2 - nu_ref^-2
    turns that ulp into nu / (2 |nu - nu_ref|) ulps of d phi_n / d DM.  The
    reference frequencies therefore sit outside the band here (at least 50
    MHz from every channel: under 13 ulps), as the default nu_ref = inf
    does; the goldens, frozen, keep theirs inside.  The oracle also forms
    phi_n as phi + DM (Dconst f / P), the reference and the device as phi +
    (Dconst DM f) / P: an ulp of phi_n apart, which harmonic k turns into
    2 pi k ulp(phi_n) of its term -- 250 eps at k = 40 and two turns.  The
    far points' DM and GM offsets are therefore a quarter of the goldens'
    here (phi_n within about a turn); at the goldens' own far points the
    device is held to the reference, not to the oracle.  And the oracle
    restates the reference's B (B - 1) / tau_n, whose B - 1 cancels at small
    u = 2 pi k tau_n: its scattering derivatives of C are eps / u of their
    companion off (280 eps here at tau = 1e-4, against the device's closed
    form within 10 eps of the extended-precision value), so the smallest
    far tau is 1e-3 here."""
    from pulseportraiture_amd import pptoaslib
    p = E._problem(31 * nchan + nharm, nchan, nharm, 1250.0, 400.0,
                   (1200.0, 1700.0, 1180.0), 1.21, False)
    sig = np.array([1e-4, 1e-5, 1e-2, 1e-2, 1e-2])
    log_pts, lin_pts = E.make_points(p["truth"], sig, nchan)
    for pts in (log_pts, lin_pts):
        pts[:, 1:3] = p["truth"][1:3] + 0.25 * (pts[:, 1:3] - p["truth"][1:3])
    log_pts[3, 3] = -3.0
    worst = np.zeros(4)
    for pts, lt in ((log_pts, True), (lin_pts, False)):
        d = pptoaslib.eval_portrait_full(pts, *_args(p), log10_tau=lt,
                                         per_channel=True)
        for i, th in enumerate(pts):
            t = O.channel_terms(th, *_args(p), lt)
            h = E.companions(th, *_args(p), lt)
            sf, sg, sH = E.scales(t, h)
            r = [E.ratio(E.pack_terms(_terms(d.terms, i)), E.pack_terms(t),
                         E.pack_terms(h)),
                 E.ratio(d.f[i], O.objective(t), sf),
                 E.ratio(d.grad[i], O.gradient(t, E.FLAGS_A), sg),
                 E.ratio(d.hess[i], O.hessian(t, E.FLAGS_A), sH)]
            print("  log10 %d point %d: terms %.1f f %.1f g %.1f H %.1f" %
                  ((lt, i) + tuple(r)))
            worst = np.maximum(worst, r)
    print("%d x %d vs oracle (terms, f, g, H): %s x eps x scale" %
          (nchan, nharm, np.round(worst, 1)))
    assert worst.max() <= E.BAR_EPS


def test_at_the_fits_stationary_point():
    """At fit_portrait_full's returned parameters (golden case pdta_64x512,
    its output reference frequencies) the evaluator's gradient is that of a
    point within goldens.SIGMA_TOL sigma of the optimum, |g_i| <= SIGMA_TOL
    sum_j |H_ij| sigma_j, and inv(0.5 H) over the fitted parameters is the
    covariance the fit reports, to the bar tests/test_gpu_parity.py holds
    that covariance to (rtol 1e-3, atol 1e-6 of its largest entry)."""
    import goldens as G
    from pulseportraiture_amd import pptoaslib
    c = G.full_case("pdta_64x512")
    a = G.full_case_args(c)
    a["data_port"] = c["data"]
    r = pptoaslib.fit_portrait_full(**a)
    data = a["data_port"].astype(float)
    nbin = data.shape[-1]
    D = np.fft.rfft(data, axis=-1)
    M = np.fft.rfft(a["model_port"], axis=-1)
    D[:, 0] = 0.0
    M[:, 0] = 0.0
    errs = O.noise_ps(data) if a["errs"] is None else np.asarray(a["errs"])
    errs_FT = errs * np.sqrt(nbin / 2.0)
    flags = np.array(a["fit_flags"])
    ifit = np.where(flags)[0]
    e = pptoaslib.eval_portrait_full(
        np.array([r.params]), D, M, errs_FT, a["P"], a["freqs"], r.nu_DM,
        r.nu_GM, r.nu_tau, fit_flags=flags, log10_tau=a["log10_tau"],
        per_channel=True)
    g, H = e.grad[0], e.hess[0]
    t = _terms(e.terms, 0)
    h = E.companions(r.params, D, M, errs_FT, a["P"], a["freqs"], r.nu_DM,
                     r.nu_GM, r.nu_tau, a["log10_tau"])
    _, sg, _ = E.scales(t, h, flags)
    bound = G.SIGMA_TOL * np.abs(H) @ np.asarray(r.param_errs)
    print("g / scale at the fit:", np.abs(g[ifit]) / sg[ifit],
          " g / bound:", np.abs(g[ifit]) / bound[ifit])
    assert np.all(np.abs(g[ifit]) <= bound[ifit])
    cov = np.linalg.inv(0.5 * H[np.ix_(ifit, ifit)])
    cm = np.asarray(r.covariance_matrix)
    np.testing.assert_allclose(cov, cm, rtol=1e-3, atol=1e-6 * np.abs(cm).max())
    H2, cov2 = pptoaslib.fit_portrait_full_function_2deriv(
        r.params, D, M, errs_FT, a["P"], a["freqs"], r.nu_DM, r.nu_GM,
        r.nu_tau, flags, a["log10_tau"], return_covariance_matrix=True)
    np.testing.assert_array_equal(H2, H)
    np.testing.assert_array_equal(cov2, cov)


def test_bad_arguments_are_refused_with_a_context():
    """PPF_EINVAL for nharm < 2, nchan < 1, npoint < 1 and an unknown order
    with a live context, before any launch (NULL arrays would fault
    otherwise)."""
    import torch
    from pulseportraiture_amd import _lib
    lib = _lib.load()
    ctx = _lib.context(torch.cuda.current_device())
    tail = [None] * 5 + [0, None]
    for nchan, nharm, npoint, order in ((4, 1, 1, 2), (0, 17, 1, 2),
                                        (4, 17, 0, 2), (4, 17, 1, 3),
                                        (4, 17, 1, -1)):
        rc = lib.ppf_eval_batch(ctx, 1, nchan, nharm, npoint, None, None, 1,
                                *[None] * 8, 1, order, *tail)
        assert rc == _lib.PPF_EINVAL
    assert lib.ppf_eval_batch(ctx, 1, 4, 17, 1, None, None, 1, *[None] * 8, 1,
                              2, *tail) == _lib.PPF_EINVAL      # NULL arrays
    assert lib.ppf_eval_batch(ctx, 0, 4, 17, 1, None, None, 1, *[None] * 8, 1,
                              2, *tail) == _lib.PPF_OK
