"""Drop-in mirror of PulsePortraiture's ``pptoaslib`` hot path.

``fit_portrait_full`` keeps the reference signature and DataBunch, and runs
the whole per-sub-integration fit on the GPU (libppfit ``ppf_fit_batch``):
rfft + power-spectrum noise + cross spectrum, the scipy trust-ncg replica
over phi/DM/GM/tau/alpha, zero-covariance frequencies, output transform and
the O(nchan) Schur-complement covariance.  ``fit_portrait_full_batch`` is the
batched entry the GetTOAs driver uses.

Reference: /root/reference/pptoaslib.py (file:line cited per function).
"""
import sys
import time

import numpy as np

from . import _lib, engine
from .pplib import (DataBunch, Dconst, RCSTRINGS, _raise_status, _box,  # noqa: F401
                    scattering_times, scattering_portrait_FT, phase_transform,
                    get_bin_centers, guess_fit_freq, rotate_data)

METHODS = ("trust-ncg", "Newton-CG", "TNC")


def phase_shifts(phi, DM, GM, freqs, nu_DM=np.inf, nu_GM=np.inf, P=None,
                 mod=False):
    """pptoaslib.py:195-228 (host)."""
    if P is None:
        P, mod = 1.0, False
    delays = phi + Dconst * DM * (freqs ** -2 - nu_DM ** -2) / P + \
        Dconst ** 2 * GM * (freqs ** -4 - nu_GM ** -4) / P
    if mod:
        delays = np.where(abs(delays) >= 0.5, delays % 1, delays)
        delays = np.where(delays >= 0.5, delays - 1.0, delays)
        if not delays.shape:
            delays = np.float64(delays)
    return delays


def phase_shifts_deriv(freqs, nu_DM=np.inf, nu_GM=np.inf, P=None):
    """pptoaslib.py:231-242 (host)."""
    if P is None:
        P = 1.0
    one = np.ones(len(freqs)) if hasattr(freqs, "shape") else 1.0
    return np.array([one, Dconst * (freqs ** -2 - nu_DM ** -2) / P,
                     Dconst ** 2 * (freqs ** -4 - nu_GM ** -4) / P])


def GM_from_DMc(DMc, D, a_perp):
    """pptoaslib.py:93-105."""
    c = 3e10 / 3.1e21
    return DMc ** 2 * (c * D) / (2.0 * (a_perp * 4.8e-9) ** 2)


def DMc_from_GM(GM, D, a_perp):
    """pptoaslib.py:108-121."""
    c = 3e10 / 3.1e21
    return (GM * (2.0 * a_perp * (4.8e-9) ** 2) / (c * D)) ** 0.5


# widest 'gauss' response [rot] served: up to here the reference's factor is
# the plain Gaussian to rounding (see instrumental_response_FT)
GAUSS_IRF_MAX_WID = 0.1


def instrumental_response_FT(nbin, wid=0.0, irf_type='rect'):
    """pptoaslib.py:124-155: the Fourier transform [nbin // 2 + 1] of one
    instrumental response of width wid [rot]: the width of the rectangle
    ('rect') or the FWHM of the Gaussian ('gauss').

    'rect' is np.sinc(k wid), as in the reference.  'gauss' is the closed
    form exp(-(pi k wid)**2 / (4 ln 2)): the reference's
    gaussian_profile_FT(nbin, 0, wid, 1) / [0] (pplib.py:1229-1263) is
    exp(-b**2) Re erf(a + i b) normalised at k = 0, which equals the plain
    Gaussian to 4e-16 for wid <= 0.12 and departs from it above (8e-15 at
    0.15, 1.5e-4 and overflow artefacts at 0.3); so 0 < wid <=
    GAUSS_IRF_MAX_WID = 0.1 is served and a wider 'gauss' raises
    NotImplementedError.

    wid == 0.0 returns None, as the reference does (its `inst_resp_FT` is
    never returned, pptoaslib.py:143-144).  An unknown irf_type raises
    ValueError; the reference prints a message and returns 0 (which silently
    zeroes the model it multiplies)."""
    nharm = nbin // 2 + 1
    if wid == 0.0:
        return None
    if irf_type == 'rect':
        return np.sinc(np.arange(nharm) * wid)
    if irf_type == 'gauss':
        if not abs(wid) <= GAUSS_IRF_MAX_WID:
            raise NotImplementedError(
                "'gauss' instrumental response of FWHM %g rot: only widths "
                "up to %g rot are supported (beyond, the reference's erf "
                "formula is no longer a Gaussian)" % (wid, GAUSS_IRF_MAX_WID))
        return np.exp(-(np.pi * np.arange(nharm) * wid) ** 2 /
                      (4.0 * np.log(2.0)))
    raise ValueError("Unrecognized instrumental response function type '%s'."
                     % irf_type)


def instrumental_response_table(nbin, wids=[], irf_types=[]):
    """The product [nbin // 2 + 1] of the constant-width factors of
    instrumental_response_port_FT (pptoaslib.py:183-185), real, in the
    reference's order; None without any.  A width of exactly 0 raises
    TypeError (the reference multiplies by None there)."""
    table = None
    for wid, irf_type in zip(wids, irf_types):
        f = instrumental_response_FT(nbin, wid, irf_type)
        if f is None:
            raise TypeError("instrumental response width 0.0: the reference "
                            "multiplies by None (pptoaslib.py:143-144, 184)")
        table = f if table is None else table * f
    return table


def dispersive_smearing_widths(freqs, DM, P, chan_bw):
    """pptoaslib.py:189: the per-channel width [rot] of the 'rect' response
    of dispersive smearing across a channel of chan_bw [MHz]."""
    if not DM:
        return np.zeros(len(freqs))
    # scalar arithmetic per channel, as the reference's loop (an array power
    # may round differently from the scalar one)
    return np.array([8.3e-6 * chan_bw / (np.float64(f) / 1e3) ** 3 / P
                     for f in freqs])


def instrumental_response_port_FT(nbin, freqs, DM=0.0, P=1.0, wids=[],
                                  irf_types=[]):
    """pptoaslib.py:158-192: the combined instrumental responses
    [nchan, nbin // 2 + 1]: one factor per entry of wids / irf_types
    (instrumental_response_FT) and, if DM is non-zero, a per-channel 'rect' of
    width 8.3e-6 chan_bw / (nu / 1e3)**3 / P with chan_bw = |freqs[1] -
    freqs[0]|.  Ones (float) when DM == 0 and wids is empty, else complex
    with zero imaginary part, as the reference returns.  A zero width raises
    TypeError, an unknown type ValueError, 'gauss' above GAUSS_IRF_MAX_WID
    NotImplementedError; fewer than two freqs with DM raise IndexError."""
    nharm = nbin // 2 + 1
    nchan = len(freqs)
    if DM == len(wids) == 0.0:
        return np.ones([nchan, nharm])
    out = np.ones([nchan, nharm], dtype=np.complex128)
    for wid, irf_type in zip(wids, irf_types):
        f = instrumental_response_table(nbin, [wid], [irf_type])
        out *= f
    if DM:
        chan_bw = abs(freqs[1] - freqs[0])
        w = dispersive_smearing_widths(freqs, DM, P, chan_bw)
        out *= np.sinc(np.arange(nharm) * w[:, None])
    return out


def rotate_portrait_full(port, phi, DM, GM, freqs, nu_DM=np.inf,
                         nu_GM=np.inf, P=None):
    """pptoaslib.py:61-90: per-channel phase on the host, rotation on the
    GPU."""
    if P is None:
        P = 1.0
    ph = phase_shifts(phi, DM, GM, np.asarray(freqs, dtype=float), nu_DM,
                      nu_GM, P, False)
    port = np.asarray(port)
    ph = np.broadcast_to(np.asarray(ph, dtype=float), (port.shape[0],))
    return engine.rotate_rows(port, ph, ref_len=True).cpu().numpy()


def _status_message(rc, sub_id):
    rcstring = RCSTRINGS.get(str(rc), "")
    if sub_id is not None:
        ii = sub_id[::-1].index("_")
        sys.stderr.write("Fit 'failed' with return code %d: %s -- %s subint "
                         "%s\n" % (rc, rcstring, sub_id[:-ii - 1],
                                   sub_id[-ii:]))
    else:
        sys.stderr.write("Fit 'failed' with return code %d -- %s" %
                         (rc, rcstring))


def _nu_zero_text(fit_flags):
    """The line get_nu_zeros prints for these fit flags when a reference
    frequency is not given (pptoaslib.py:941, 947-948), or None."""
    flags = [int(bool(f)) for f in fit_flags]
    known = ([1, 1, 0, 0, 0], [1, 0, 1, 0, 0], [0, 0, 0, 1, 1],
             [1, 1, 0, 1, 0], [1, 1, 1, 0, 0], [1, 1, 0, 1, 1],
             [1, 1, 1, 1, 0])
    if flags == [1, 1, 1, 1, 1]:
        return "Approximating zero-covariance frequencies..."
    if flags not in known and sum(flags) > 1:
        return "No zero-covariance frequencies found."
    return None


def _nu_zero_messages(fit_flags, nu_outs):
    """Reproduce get_nu_zeros' prints (pptoaslib.py:941, 947-948)."""
    if bool(np.all(nu_outs)):
        return
    text = _nu_zero_text(fit_flags)
    if text is not None:
        print(text)


def unpack_result(R, scales, scale_errs, channel_snrs, cov, fit_flags,
                  duration):
    """Build the fit_portrait_full DataBunch (pptoaslib.py:1134-1143) from one
    device result record."""
    I = _lib.RESULT_INDEX
    flags = [int(bool(f)) for f in fit_flags]
    nfit = int(sum(flags))
    params = list(np.asarray(R[I["params"]], dtype=float))
    param_errs = np.asarray(R[I["param_errs"]], dtype=float).copy()
    status = int(R[I["status"]])
    return DataBunch(
        params=params, param_errs=param_errs, phi=params[0],
        phi_err=param_errs[0], DM=params[1], DM_err=param_errs[1],
        GM=params[2], GM_err=param_errs[2], tau=params[3],
        tau_err=param_errs[3], alpha=params[4], alpha_err=param_errs[4],
        scales=scales, scale_errs=scale_errs, nu_DM=R[I["nu_out"]][0],
        nu_GM=R[I["nu_out"]][1], nu_tau=R[I["nu_out"]][2],
        covariance_matrix=np.asarray(cov)[:nfit, :nfit].copy(),
        chi2=R[I["chi2"]], red_chi2=R[I["red_chi2"]], snr=R[I["snr"]],
        channel_snrs=channel_snrs, duration=duration,
        nfeval=int(R[I["nfeval"]]), return_code=status & 0xff)


def fit_portrait_full(data_port, model_port, init_params, P, freqs,
                      nu_fits=[None, None, None], nu_outs=[None, None, None],
                      errs=None, fit_flags=[1, 1, 1, 1, 1],
                      bounds=[(None, None), (None, None), (None, None),
                              (None, None), (None, None)], log10_tau=True,
                      option=0, sub_id=None, method="trust-ncg", is_toa=True,
                      quiet=True):
    """pptoaslib.py:974-1144 on the GPU (single sub-integration).

    ``method`` 'trust-ncg' is the reference default: the device minimises
    the same objective to the same stationary point with a Newton trust
    region (scaled coordinates, exact subproblem; scipy's own path with
    engine.SOLVER = 'scipy'); 'Newton-CG' runs the same solver.  'TNC'
    applies ``bounds`` as the reference does
    (pptoaslib.py:1041-1046: only for TNC): the device trust-region steps
    are projected onto the box, so the fit ends at the bounded stationary
    point TNC converges to."""
    if method not in METHODS:
        print("Method '%s' is not implemented." % method)
        sys.exit()
    data_port = np.asarray(data_port)
    freqs = np.asarray(freqs, dtype=float)
    nchan, nbin = data_port.shape
    nu_f = np.array([np.nan if v is None else float(v) for v in nu_fits])
    nu_o = np.array([np.nan if v is None else float(v) for v in nu_outs])
    if not bool(np.all(nu_outs)):
        nu_o = np.where(np.array([v is None for v in nu_outs]), np.nan, nu_o)
    init = np.asarray(init_params, dtype=float).reshape(1, 5)
    t0 = time.time()
    res = engine.fit_batch(
        data_port[None], np.asarray(model_port, dtype=float)[None], freqs[None],
        [P], init, [int(bool(f)) for f in fit_flags], nu_fits=nu_f[None],
        nu_outs=nu_o[None],
        errs=None if errs is None else np.asarray(errs, dtype=float)[None],
        log10_tau=log10_tau, option=option, is_toa=is_toa,
        bounds=_box(bounds, 5) if method == "TNC" else None)
    r = engine.results_numpy(res)
    duration = time.time() - t0
    _nu_zero_messages(fit_flags, nu_outs)
    R = r["results"][0]
    status = int(R[_lib.RESULT_INDEX["status"]])
    _raise_status(status)
    rc = status & 0xff
    if rc not in (0, 1, 2, 4):
        _status_message(rc, sub_id)
    return unpack_result(R, r["scales"][0], r["scale_errs"][0],
                         r["channel_snrs"][0], r["covariance"][0], fit_flags,
                         duration)


def get_scales_full(params, data_portrait_FT, model_portrait_FT, errs_FT, P,
                    freqs, nu_DM, nu_GM, nu_tau, log10_tau):
    """pptoaslib.py:953-971: a_n = C_n / S_n at given params, from the given
    data and model spectra, on the GPU (ppf_scales_batch, k_scales: one wave
    per channel, the phasor with exact argument reduction)."""
    D = np.asarray(data_portrait_FT)
    out = engine.scales_batch(
        D, np.asarray(model_portrait_FT), np.asarray(params, dtype=float),
        float(P), np.asarray(freqs, dtype=float),
        [float(nu_DM), float(nu_GM), float(nu_tau)], log10_tau,
        errs_FT=None if errs_FT is None else np.asarray(errs_FT, dtype=float))
    return out[0].cpu().numpy()


# ---------------------------------------------------------------------------
# The likelihood itself: pptoaslib.py:564-773 evaluated on the GPU
# (ppf_eval_batch, ppf_eval.hip).  eval_portrait_full is the batched entry;
# the reference's four signatures are one-point calls of the same kernel.
# ---------------------------------------------------------------------------
def _terms_bunch(terms):
    """[..., 62, nchan] -> DataBunch of C, S [..., nchan], dC, dS
    [..., 5, nchan], d2C, d2S [..., 5, 5, nchan] (oracle.channel_terms'
    layout behind the leading axes)."""
    lead, nchan = terms.shape[:-2], terms.shape[-1]
    return DataBunch(C=terms[..., 0, :], S=terms[..., 1, :],
                     dC=terms[..., 2:7, :], dS=terms[..., 7:12, :],
                     d2C=terms[..., 12:37, :].reshape(lead + (5, 5, nchan)),
                     d2S=terms[..., 37:62, :].reshape(lead + (5, 5, nchan)))


def eval_portrait_full(params, data_portrait_FT, model_portrait_FT, errs_FT,
                       P, freqs, nu_DM, nu_GM, nu_tau,
                       fit_flags=(1, 1, 1, 1, 1), log10_tau=True, order=2,
                       per_channel=False, mask=None, model_index=None,
                       dev=None):
    """fit_portrait_full_function and its derivatives (pptoaslib.py:564-684)
    at K parameter points in one device call (not in the reference).

    params [K, 5] for one problem -- data_portrait_FT, model_portrait_FT
    [nchan, nharm], errs_FT, freqs [nchan], scalar P and reference
    frequencies -- or [nprob, K, 5] with a leading problem axis on the other
    arrays (model_portrait_FT may hold fewer models, chosen by model_index
    [nprob]).  mask [.., nchan]: 0 drops a channel.  order 0 / 1 / 2: f /
    + gradient / + Hessian.  Returns DataBunch(f [.., K], grad [.., K, 5],
    hess [.., K, 5, 5]) of NumPy arrays (None past `order`), with
    per_channel also terms: C, S [.., K, nchan], dC, dS [.., K, 5, nchan],
    d2C, d2S [.., K, 5, 5, nchan]."""
    th = np.asarray(params, dtype=float)
    if th.ndim not in (2, 3) or th.shape[-1] != 5:
        raise ValueError("params must be [K, 5] or [nprob, K, 5], got %s" %
                         (th.shape,))
    single = th.ndim == 2
    if single and np.ndim(data_portrait_FT) != 2:
        raise ValueError("params [K, 5] go with one [nchan, nharm] problem")
    nprob = 1 if single else th.shape[0]
    nus = np.empty((nprob, 3))
    for i, v in enumerate((nu_DM, nu_GM, nu_tau)):
        nus[:, i] = np.asarray(v, dtype=float)
    f, g, H, t = engine.eval_points(
        th, data_portrait_FT, model_portrait_FT,
        np.ones(np.shape(freqs)) if errs_FT is None else errs_FT, P, freqs,
        nus, fit_flags=fit_flags, log10_tau=log10_tau, order=order,
        per_channel=per_channel, mask=mask, model_index=model_index, dev=dev)
    out = [None if x is None else x.cpu().numpy() for x in (f, g, H, t)]
    if single:
        out = [None if x is None else x[0] for x in out]
    res = DataBunch(f=out[0], grad=out[1], hess=out[2])
    if per_channel:
        res["terms"] = _terms_bunch(out[3])
    return res


def _eval_one(params, data_portrait_FT, model_portrait_FT, errs_FT, P, freqs,
              nu_DM, nu_GM, nu_tau, fit_flags, log10_tau, order,
              per_channel=False):
    r = eval_portrait_full(
        np.asarray(params, dtype=float).reshape(1, 5),
        np.asarray(data_portrait_FT), np.asarray(model_portrait_FT), errs_FT,
        P, np.asarray(freqs, dtype=float), nu_DM, nu_GM, nu_tau,
        fit_flags=np.asarray(fit_flags, dtype=float), log10_tau=log10_tau,
        order=order, per_channel=per_channel)
    t = None
    if per_channel:
        t = DataBunch(**{k: v[0] for k, v in r.terms.items()})
    return r, t


def fit_portrait_full_function(params, data_portrait_FT, model_portrait_FT,
                               errs_FT, P, freqs, nu_DM, nu_GM, nu_tau,
                               fit_flags, log10_tau):
    """pptoaslib.py:564-581: chi'^2 = -sum C_n^2 / S_n (a float)."""
    r, _ = _eval_one(params, data_portrait_FT, model_portrait_FT, errs_FT, P,
                     freqs, nu_DM, nu_GM, nu_tau, fit_flags, log10_tau, 0)
    return np.float64(r.f[0])


def fit_portrait_full_function_deriv(params, data_portrait_FT,
                                     model_portrait_FT, errs_FT, P, freqs,
                                     nu_DM, nu_GM, nu_tau, fit_flags,
                                     log10_tau):
    """pptoaslib.py:584-614: the gradient [5], times fit_flags."""
    r, _ = _eval_one(params, data_portrait_FT, model_portrait_FT, errs_FT, P,
                     freqs, nu_DM, nu_GM, nu_tau, fit_flags, log10_tau, 1)
    return r.grad[0].copy()


def _channel_hessian(t, flags):
    """Per-channel profiled Hessian [5, 5, nchan] from the channel terms
    (pptoaslib.py:662-671 multiplied out, so a channel with C = 0 gives its
    finite value instead of the reference's 0 / 0)."""
    C, S, dC, dS = t.C, t.S, t.dC, t.dS
    ff = flags[:, None] * flags[None, :]
    return -2.0 * (C * t.d2C / S - 0.5 * C ** 2 * t.d2S / S ** 2 +
                   dC[:, None] * dC[None, :] / S +
                   C ** 2 * dS[:, None] * dS[None, :] / S ** 3 -
                   C * (dC[:, None] * dS[None, :] + dS[:, None] * dC[None, :])
                   / S ** 2) * ff[:, :, None]


def _returns(hessian, extra):
    return hessian if not extra else tuple([hessian] + extra)


def fit_portrait_full_function_2deriv(params, data_portrait_FT,
                                      model_portrait_FT, errs_FT, P, freqs,
                                      nu_DM, nu_GM, nu_tau, fit_flags,
                                      log10_tau, per_channel=False,
                                      return_covariance_matrix=False,
                                      return_scales=False):
    """pptoaslib.py:617-684: the Hessian [5, 5] (summed on the device), or
    [5, 5, nchan] with per_channel (assembled from the device's channel
    terms); then, as asked, the covariance matrix inv(0.5 H) over the fitted
    parameters and the scales C / S, in the reference's return order (the
    bare Hessian when nothing else is asked)."""
    flags = np.asarray(fit_flags, dtype=float)
    need_t = per_channel or return_scales
    r, t = _eval_one(params, data_portrait_FT, model_portrait_FT, errs_FT, P,
                     freqs, nu_DM, nu_GM, nu_tau, flags, log10_tau, 2, need_t)
    hess = r.hess[0].copy()
    extra = []
    if return_covariance_matrix:
        ifit = np.where(np.asarray(fit_flags))[0]
        extra.append(np.linalg.inv(0.5 * hess[np.ix_(ifit, ifit)]))
    if return_scales:
        extra.append(t.C / t.S)
    return _returns(_channel_hessian(t, flags) if per_channel else hess,
                    extra)


def fit_portrait_full_function_2deriv_with_scales(
        params, data_portrait_FT, model_portrait_FT, errs_FT, P, freqs,
        nu_DM, nu_GM, nu_tau, fit_flags, log10_tau, per_channel=False,
        return_covariance_matrix=False, return_scales=False):
    """pptoaslib.py:687-773: the Hessian over (theta, a_n), (5 + nchan)^2
    (with per_channel one more axis of nchan, as the reference builds it),
    assembled on the host from the device's channel terms -- it is
    O(nchan^2) by definition -- and its block inverse (Schur complement of
    the diagonal a_n block) as the covariance matrix."""
    flags = np.asarray(fit_flags, dtype=float)
    _, t = _eval_one(params, data_portrait_FT, model_portrait_FT, errs_FT, P,
                     freqs, nu_DM, nu_GM, nu_tau, flags, log10_tau, 2, True)
    C, S = t.C, t.S
    n = len(C)
    scales = C / S
    ff = flags[:, None] * flags[None, :]
    top = -2.0 * (C * t.d2C / S - 0.5 * C ** 2 * t.d2S / S ** 2) * \
        ff[:, :, None]                                   # [5, 5, n]
    cross = -2.0 * (t.dC - scales * t.dS)                # [5, n]
    total = np.zeros((5 + n, 5 + n))
    total[:5, :5] = top.sum(axis=-1)
    total[:5, 5:] = cross * flags[:, None]
    total[5:, :5] = total[:5, 5:].T
    total[5:, 5:] = np.diag(2.0 * S)
    if per_channel:
        hessian = np.zeros((5 + n, 5 + n, n))
        hessian[:5, :5] = top
        ic = np.arange(n)
        hessian[5 + ic, 5 + ic, ic] = 2.0 * S
        for j in range(5):
            hessian[5 + ic, j, ic] = hessian[j, 5 + ic, ic] = \
                cross[j] * flags[j]
    else:
        hessian = total
    extra = []
    if return_covariance_matrix:
        ifit = np.where(np.asarray(fit_flags))[0]
        A = total[np.ix_(ifit, ifit)]
        U = cross[ifit]
        cinv = 1.0 / (2.0 * S)
        Xinv = np.linalg.inv(A - (U * cinv) @ U.T)
        UR = -(Xinv @ U) * cinv
        LL = -cinv[:, None] * (U.T @ Xinv)
        LR = -(LL @ U) * cinv + np.diag(cinv)
        extra.append(2.0 * np.block([[Xinv, UR], [LL, LR]]))
    if return_scales:
        extra.append(scales)
    return _returns(hessian, extra)
