"""Drop-in mirror of the parts of PulsePortraiture's ``pplib`` on the hot path.

Compute-bearing routines (FFT rotation, power-spectrum noise, 1-D FFTFIT and
the legacy 2-parameter portrait fit) run on the GPU through libppfit; the
rest is host bookkeeping (constants, reference-frequency algebra, Gaussian
model generation from .gmodel files, TOA text output) with the reference's
signatures.  There is no CPU fallback for the compute routines.

Reference: /root/reference/pplib.py (file:line cited per function).
"""
import os
import sys
import time

import pickle

import math

import numpy as np

from . import _lib, engine

# ---------------------------------------------------------------- settings --
Dconst_exact = 4.148808e3          # pplib.py:61
Dconst_trad = 0.000241 ** -1       # pplib.py:64
Dconst = Dconst_trad               # pplib.py:67
scattering_alpha = -4.0            # pplib.py:70
use_get_noise = True               # pplib.py:74
default_noise_method = "PS"        # pplib.py:78
F0_fact = 0                        # pplib.py:82
wid_max = 0.25                     # pplib.py:86
default_model = "000"              # pplib.py:95
binshift = 1.0                     # pplib.py:99

# scipy.optimize.fmin_tnc return codes (pplib.py:127-135)
RCSTRINGS = {"-1": "INFEASIBLE: Infeasible (low > up).",
             "0": "LOCALMINIMUM: Local minima reach (|pg| ~= 0).",
             "1": "FCONVERGED: Converged (|f_n-f_(n-1)| ~= 0.)",
             "2": "XCONVERGED: Converged (|x_n-x_(n-1)| ~= 0.)",
             "3": "MAXFUN: Max. number of function evaluations reach.",
             "4": "LSFAIL: Linear search failed.",
             "5": "CONSTANT: All lower bounds are equal to the upper bounds.",
             "6": "NOPROGRESS: Unable to progress.",
             "7": "USERABORT: User requested end of minimization."}


class DataBunch(dict):
    """dict with attribute access (pplib.py:142-152)."""

    def __init__(self, **kwds):
        dict.__init__(self, kwds)
        self.__dict__ = self


class MJD(object):
    """A PSRCHIVE-free MJD (psrchive.MJD's interface as get_TOAs and
    write_TOAs use it): integer day + fractional day, so a TOA keeps
    sub-nanosecond resolution.  MJD(days) or MJD(intday, fracday)."""

    def __init__(self, intday=0.0, fracday=None):
        # math.floor: the same integers as np.floor, without the NumPy
        # scalar round trip (GetTOAs makes two of these per TOA)
        if fracday is None:
            d = float(intday)
            i = math.floor(d)
            intday, fracday = i, d - i
        i, f = int(intday), float(fracday)
        k = math.floor(f)
        self._i, self._f = i + k, f - k

    @classmethod
    def _make(cls, i, f):
        """An MJD from an integer day and a fraction already in [0, 1)."""
        m = cls.__new__(cls)
        m._i, m._f = i, f
        return m

    def __add__(self, other):
        if isinstance(other, MJD):
            return MJD(self._i + other._i, self._f + other._f)
        return MJD(self._i, self._f + float(other) / 86400.0)   # seconds

    def intday(self):
        return self._i

    def fracday(self):
        return self._f

    def in_days(self):
        return self._i + self._f

    def __repr__(self):
        return "MJD(%d, %.15f)" % (self._i, self._f)


# ------------------------------------------------------------ host helpers --
def get_bin_centers(nbin, lo=0.0, hi=1.0):
    """pplib.py:694-707."""
    lo, hi = np.double(lo), np.double(hi)
    diff = hi - lo
    return np.double(np.linspace(lo + diff / (nbin * 2),
                                 hi - diff / (nbin * 2), nbin))


def weighted_mean(data, errs=1.0):
    """pplib.py:721-735."""
    if hasattr(errs, "is_integer"):
        errs = np.ones(len(data))
    iis = np.where(errs > 0.0)[0]
    w = errs[iis] ** -2.0
    return (data[iis] * w).sum() / w.sum(), w.sum() ** -0.5


def DM_delay(DM, freq, freq_ref=np.inf, P=None):
    """pplib.py:2672-2685."""
    delay = Dconst * DM * ((freq ** -2.0) - (freq_ref ** -2.0))
    return delay / P if P else delay


def phase_transform(phi, DM, nu_ref1=np.inf, nu_ref2=np.inf, P=None,
                    mod=False):
    """pplib.py:2688-2712."""
    if P is None:
        P, mod = 1.0, False
    phi_prime = phi + (Dconst * DM * P ** -1 *
                       (nu_ref2 ** -2.0 - nu_ref1 ** -2.0))
    if mod:
        phi_prime = np.where(abs(phi_prime) >= 0.5, phi_prime % 1, phi_prime)
        phi_prime = np.where(phi_prime >= 0.5, phi_prime - 1.0, phi_prime)
        if not phi_prime.shape:
            phi_prime = np.float64(phi_prime)
    return phi_prime


def guess_fit_freq(freqs, SNRs=None):
    """pplib.py:2715-2729: SNR * nu**-2 weighted centre frequency."""
    nu0 = (freqs.min() + freqs.max()) * 0.5
    if SNRs is None:
        SNRs = np.ones(len(freqs))
    w = SNRs * freqs ** -2
    return nu0 + np.sum((freqs - nu0) * w) / np.sum(w)


def scattering_times(tau, alpha, freqs, nu_tau):
    """pplib.py:4212-4216."""
    return tau * (freqs / nu_tau) ** alpha


def scattering_profile_FT(tau, nbin, binshift=binshift):
    """pplib.py:4219-4242 (host; model generation / flux only)."""
    nharm = nbin // 2 + 1
    if tau == 0.0:
        return np.ones(nharm)
    return (1.0 + 2 * np.pi * 1.0j * np.arange(nharm) * tau) ** -1


def scattering_portrait_FT(taus, nbin, binshift=binshift):
    """pplib.py:4245-4260 (host; complex128 on every NumPy)."""
    taus = np.asarray(taus, dtype=float)
    nharm = nbin // 2 + 1
    if not np.any(taus):
        return np.ones([len(taus), nharm])
    k = np.arange(nharm)
    out = 1.0 / (1.0 + 2j * np.pi * np.outer(taus, k))
    out[taus == 0.0] = 1.0
    return out


# ------------------------------------------ Gaussian models (device) --------
def gaussian_profile(nbin, loc, wid, norm=False, abs_wid=False, zeroout=True):
    """pplib.py:801-856 (unit peak, zeroout): one row of k_gauss_port with
    the linear evolution code at nu = nu_ref, which passes loc, wid and the
    unit amplitude through exactly."""
    if norm or not zeroout:
        raise NotImplementedError("gaussian_profile(norm=True / zeroout="
                                  "False) is outside the accelerated path")
    if abs_wid:
        wid = abs(wid)
    params = [0.0, 0.0, loc, 0.0, wid, 0.0, 1.0, 0.0]
    return gen_gaussian_portrait("111", params, 0.0, np.zeros(nbin), [1.0],
                                 1.0)[0]


def _join_ids(join_ichans, nchan):
    """join_ichans (one list of channel indices per archive) -> the archive
    of each channel, int32 [nchan], -1 for a channel in none.  A channel
    listed by two archives would be rotated twice by the reference; that is
    refused."""
    join_id = np.full(nchan, -1, dtype=np.int32)
    for ia, ichans in enumerate(join_ichans):
        ichans = np.arange(nchan)[np.asarray(ichans)]
        if np.any(join_id[ichans] >= 0):
            raise ValueError("join_ichans: a channel belongs to two archives")
        join_id[ichans] = ia
    return join_id


def gen_gaussian_portrait(model_code, params, scattering_index, phases, freqs,
                          nu_ref, join_ichans=[], P=None):
    """pplib.py:886-963, built on the device by ppf_gauss_portrait_batch
    (k_gauss_port).  With join_ichans (one list of channel indices per
    archive) params carries 2 len(join_ichans) trailing values, (phase, DM)
    per archive, and the period P [s] is needed: each archive's rows are
    rotated in the same kernel (ppf_gauss_portrait_join_batch; even nbin in
    [32, 8192], anything else raises NotImplementedError)."""
    from . import engine
    params = np.asarray(params, dtype=float)
    njoin = len(join_ichans)
    if njoin:
        if P is None:
            raise ValueError("join_ichans needs the period P")
        join_id = _join_ids(join_ichans, len(freqs))
        out = engine.gauss_portraits(
            model_code, params[None, :-2 * njoin], [scattering_index],
            np.asarray(freqs, dtype=float)[None, :], [nu_ref], len(phases),
            join_id=join_id[None, :], join_params=params[None, -2 * njoin:],
            P=[P])
        return out[0].cpu().numpy()
    out = engine.gauss_portraits(model_code, params[None, :],
                                 [scattering_index],
                                 np.asarray(freqs, dtype=float)[None, :],
                                 [nu_ref], len(phases))
    out = out[0].cpu().numpy()
    if len(phases) % 2 and params[1] != 0.0:
        # the reference's scattering irfft takes no length (pplib.py:957):
        # nbin - 1 bins at odd nbin
        out = out[:, :-1]
    return out


def _profile_to_portrait(params):
    """2 + 3 ngauss profile values (DC, tau, loc, wid, amp ...) -> the 2 + 6
    ngauss portrait parameters with zero slopes: with the linear code '111'
    at freqs = [nu_ref] every value passes through exactly."""
    params = np.asarray(params, dtype=float)
    ngauss = (len(params) - 2) // 3
    out = np.zeros(2 + 6 * ngauss)
    out[:2] = params[:2]
    out[2::6], out[4::6], out[6::6] = params[2::3], params[3::3], params[4::3]
    return out


def gen_gaussian_profile(params, nbin):
    """pplib.py:859-883: a profile of ngauss components (DC, tau [bin], then
    loc, wid, amp each), one row of k_gauss_port."""
    return gen_gaussian_portrait("111", _profile_to_portrait(params), 0.0,
                                 np.zeros(nbin), [1.0], 1.0)[0]


def _gauss_fit(model_code, data, params, alpha, errs, vary, freqs, nu_ref,
               evaluator, join_id=None, P=None, njoin=0):
    """The Levenberg-Marquardt fit both Gaussian fits share
    (_gaussfit.levenberg_marquardt on ppf_gauss_lsq_batch).  With join_id
    (the archive of each channel) params ends in the 2 njoin join values."""
    from . import _gaussfit
    data = np.asarray(data)
    errs = np.broadcast_to(np.asarray(errs, dtype=float), data.shape)
    if evaluator is None:
        evaluator = engine.GaussLsqEvaluator(model_code, data, 1.0 / errs,
                                             freqs, nu_ref, join_id=join_id,
                                             P=P, njoin=njoin)
    p0 = np.append(np.asarray(params, dtype=float), float(alpha))
    lo, hi = _gaussfit.portrait_bounds(len(p0) - 1 - 2 * njoin, njoin)
    return _gaussfit.levenberg_marquardt(evaluator, p0, vary, lo, hi,
                                         data.size)


def fit_gaussian_profile(data, init_params, errs, fit_flags=None,
                         fit_scattering=False, quiet=True, evaluator=None):
    """pplib.py:1922-2002 without lmfit: the same bounded least-squares
    problem (tau >= 0, 0 <= wid <= wid_max, amp >= 0 through lmfit's MINUIT
    transforms) solved by _gaussfit's MINPACK-style Levenberg-Marquardt on
    the device's normal equations (one channel of ppf_gauss_lsq_batch).
    As in the reference a given fit_flags has NO tau entry: it lists DC and
    then the 3 ngauss component values, and fit_scattering is spliced in.
    Returns DataBunch(fitted_params, fit_errs, residuals, chi2, dof); a
    fixed parameter's error is 0.0 (lmfit gives None).  evaluator (not in
    the reference) replaces the device evaluator, see _gaussfit."""
    data = np.asarray(data)
    nparam = len(init_params)
    ngauss = (nparam - 2) // 3
    if fit_flags is None:
        flags = [True] * nparam
        flags[1] = bool(fit_scattering)
    else:
        flags = [bool(fit_flags[0]), bool(fit_scattering)] + \
                [bool(fit_flags[i]) for i in range(1, nparam - 1)]
    vary = np.zeros(2 + 6 * ngauss + 1, dtype=bool)
    vary[:2] = flags[:2]
    vary[2:-1:6], vary[4:-1:6], vary[6:-1:6] = \
        flags[2::3], flags[3::3], flags[4::3]
    errs = np.broadcast_to(np.asarray(errs, dtype=float), data.shape)
    p, perr, chi2, dof, lm_results = _gauss_fit(
        "111", data[None, :], _profile_to_portrait(init_params), 0.0,
        errs[None, :], vary, [1.0], 1.0, evaluator)
    pick = np.r_[0, 1, np.ravel([[2 + 6 * g, 4 + 6 * g, 6 + 6 * g]
                                 for g in range(ngauss)])].astype(int)
    fitted_params, fit_errs = p[pick], perr[pick]
    if evaluator is None:
        residuals = data - gen_gaussian_profile(fitted_params, len(data))
    else:
        residuals = None
    if not quiet:
        print("Multi-Gaussian Profile Fit Results")
        print("status:", lm_results.message)
        print("Gaussians:", ngauss)
        print("DoF:", dof)
        print("reduced chi-sq: %.2f" % (chi2 / dof))
    return DataBunch(fitted_params=fitted_params, fit_errs=fit_errs,
                     residuals=residuals, chi2=chi2, dof=dof)


def fit_gaussian_portrait(model_code, data, init_params, scattering_index,
                          errs, fit_flags, fit_scattering_index, phases, freqs,
                          nu_ref, join_params=[], P=None, quiet=True,
                          evaluator=None):
    """pplib.py:2005-2133 without lmfit: evolving Gaussian components fitted
    to a portrait by _gaussfit's MINPACK-style Levenberg-Marquardt on lmfit's
    internal variables (limits pplib.py:2041-2101), every Jacobian and
    chi^2 from one ppf_gauss_lsq_batch call.  Returns DataBunch(lm_results,
    fitted_params, fit_errs, scattering_index, scattering_index_err, chi2,
    dof); lm_results has message, nfev, success, covar and residual (the
    weighted residuals, flat).  A fixed parameter's error is 0.0 (lmfit
    gives None).  join_params = [join_ichans, values, flags] fits several
    archives at once (pplib.py:2073-2098): values / flags hold (phase, DM)
    per archive, P [s] is the period, and fitted_params / fit_errs end in
    the join values, as the reference returns them (ppf_gauss_lsq_join_batch;
    even nbin).  evaluator (not in the reference) replaces the device
    evaluator, see _gaussfit."""
    data = np.asarray(data)
    errs = np.broadcast_to(np.asarray(errs, dtype=float), data.shape)
    init_params = np.asarray(init_params, dtype=float)
    flags = np.asarray(fit_flags, dtype=float) != 0
    join_ichans, join_id = [], None
    if len(join_params):
        join_ichans = join_params[0]
        if P is None:
            # (the reference divides by None in rotate_data)
            raise NotImplementedError("fit_gaussian_portrait(join_params="
                                      "...) without the period P")
        if len(join_params[1]) != 2 * len(join_ichans) or \
                len(join_params[2]) != 2 * len(join_ichans):
            raise ValueError("join_params: (phase, DM) values and flags per "
                             "archive")
        join_id = _join_ids(join_ichans, data.shape[0])
        init_params = np.append(init_params,
                                np.asarray(join_params[1], dtype=float))
        flags = np.append(flags, np.asarray(join_params[2], dtype=float) != 0)
    vary = np.append(flags, bool(fit_scattering_index))
    p, perr, chi2, dof, lm_results = _gauss_fit(
        model_code, data, init_params, scattering_index, errs, vary,
        np.asarray(freqs, dtype=float), nu_ref, evaluator, join_id, P,
        len(join_ichans))
    if evaluator is None:
        model = gen_gaussian_portrait(model_code, p[:-1], p[-1], phases,
                                      freqs, nu_ref, join_ichans, P)
        lm_results.residual = np.ravel((data - model) / errs)
    if not quiet:
        print("Gaussian Portrait Fit")
        print("status:", lm_results.message)
        print("Gaussians:", (len(init_params) - 2) // 6)
        print("DoF:", dof)
        print("reduced chi-sq: %.2g" % (chi2 / dof))
    return DataBunch(lm_results=lm_results, fitted_params=p[:-1],
                     fit_errs=perr[:-1], scattering_index=p[-1],
                     scattering_index_err=perr[-1], chi2=chi2, dof=dof)


def write_model(filename, name, model_code, nu_ref, model_params, fit_flags,
                alpha, fit_alpha, append=False, quiet=False):
    """pplib.py:2931-2968: a .gmodel file in the reference's format, byte
    for byte (read_model and the CPU package read it).  model_params[1] is
    the scattering timescale in seconds."""
    lines = ["MODEL   %s\n" % name, "CODE    %s\n" % model_code,
             "FREQ    %.5f\n" % nu_ref,
             "DC     % .8f %d\n" % (model_params[0], fit_flags[0]),
             "TAU    % .8f %d\n" % (model_params[1], fit_flags[1]),
             "ALPHA  % .3f      %d\n" % (alpha, fit_alpha)]
    for ig in range((len(model_params) - 2) // 6):
        vals = []
        for v, f in zip(model_params[2 + ig * 6:8 + ig * 6],
                        fit_flags[2 + ig * 6:8 + ig * 6]):
            vals.append("% .8f %d" % (v, f))
        lines.append("COMP%02d %s\n" % (ig + 1, "  ".join(vals)))
    with open(filename, "a" if append else "w") as fh:
        fh.writelines(lines)
    if not quiet:
        print("%s written." % filename)


def read_model(modelfile, phases=None, freqs=None, P=None, quiet=False):
    """pplib.py:2971-3057: parse a .gmodel file; build the portrait if
    phases/freqs are given."""
    read_only = phases is None and freqs is None
    comps, fit_comps = [], []
    name = code = nu_ref = dc = tau = alpha = None
    fit_dc = fit_tau = fit_alpha = None
    with open(modelfile) as fh:      # a pickled spline model: UnicodeDecodeError
        lines = fh.readlines()
    for line in lines:
        info = line.split()
        if not info:
            continue
        key = info[0]
        try:
            if key == "MODEL":
                name = info[1]
            elif key == "CODE":
                code = info[1]
            elif key == "FREQ":
                nu_ref = np.float64(info[1])
            elif key == "DC":
                dc, fit_dc = np.float64(info[1]), int(info[2])
            elif key == "TAU":
                tau, fit_tau = np.float64(info[1]), int(info[2])
            elif key == "ALPHA":
                alpha, fit_alpha = np.float64(info[1]), int(info[2])
            elif key[:4] == "COMP":
                comps.append([np.float64(v) for v in info[1::2]])
                fit_comps.append([int(v) for v in info[2::2]])
        except IndexError:
            pass
    # a missing line leaves the reference's local unbound (pplib.py:3022-3026)
    for var, val in (("dc", dc), ("tau", tau), ("fit_dc", fit_dc),
                     ("fit_tau", fit_tau)):
        if val is None:
            raise UnboundLocalError("local variable '%s' referenced before "
                                    "assignment" % var)
    ngauss = len(comps)
    params = np.zeros(ngauss * 6 + 2)
    fit_flags = np.zeros(len(params))
    params[0], params[1] = dc, tau
    fit_flags[0], fit_flags[1] = fit_dc, fit_tau
    for ig in range(ngauss):
        params[2 + ig * 6:8 + ig * 6] = comps[ig]
        fit_flags[2 + ig * 6:8 + ig * 6] = fit_comps[ig]
    for var, val in (("modelname", name), ("model_code", code),
                     ("nu_ref", nu_ref), ("alpha", alpha)) + \
            ((("fit_alpha", fit_alpha),) if read_only else ()):
        if val is None:
            raise UnboundLocalError("local variable '%s' referenced before "
                                    "assignment" % var)
    if read_only:
        return (name, code, nu_ref, ngauss, params, fit_flags, alpha,
                fit_alpha)
    nbin = len(phases)
    if params[1] != 0:
        if P is None:
            print("Need period P for non-zero scattering value TAU.")
            return 0
        params[1] *= nbin / P
    model = gen_gaussian_portrait(code, params, alpha, phases, freqs, nu_ref)
    if not quiet:
        print("Model Name: %s" % name)
    return name, ngauss, model


def gen_spline_portrait(mean_prof, freqs, eigvec, tck, nbin=None):
    """pplib.py:966-990 on the device (ppf_spline_portrait_batch: splev of
    the B-spline curve per channel, eigenvector expansion, mean profile and,
    for nbin != len(mean_prof), scipy.signal.resample + the half-bin
    rotate_portrait)."""
    from . import engine
    out = engine.spline_portraits(mean_prof, eigvec, tck,
                                  np.asarray(freqs, dtype=float)[None, :],
                                  nbin)
    return out[0].cpu().numpy()


class _SplineUnpickler(pickle.Unpickler):
    """The reference reads spline models with a plain pickle.load
    (pplib.py:3083-3088), which runs whatever a crafted file names.  The
    6-tuple of strings, numpy arrays and splprep's tck needs only numpy's
    array reconstruction and a few builtins; any other global is refused."""
    _ALLOWED = {
        ("numpy.core.multiarray", "_reconstruct"),
        ("numpy._core.multiarray", "_reconstruct"),
        ("numpy.core.multiarray", "scalar"),
        ("numpy._core.multiarray", "scalar"),
        ("numpy", "ndarray"), ("numpy", "dtype"),
        ("builtins", "list"), ("builtins", "tuple"), ("builtins", "int"),
        ("builtins", "float"), ("builtins", "str"), ("builtins", "bytes"),
        ("__builtin__", "list"), ("__builtin__", "tuple"),
        # protocol 2 spells an EMPTY array's buffer bytes(): the empty tck of
        # a mean-profile model (make_spline_model with no component)
        ("__builtin__", "bytes"),
        ("_codecs", "encode"), ("copy_reg", "_reconstructor"),
        ("copyreg", "_reconstructor"), ("__builtin__", "object"),
        ("builtins", "object"),
    }

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError("spline model file names %s.%s, which "
                                     "a spline model never holds" %
                                     (module, name))


def read_spline_model(modelfile, freqs=None, nbin=None, quiet=False):
    """pplib.py:3060-3096: a make_spline_model(...) file -- the pickled
    (model name, source, datafile, mean profile, eigenvectors, tck) -- read
    as the reference reads it; with freqs, the portrait built on the device
    by gen_spline_portrait."""
    if not quiet:
        print("Reading model from %s..." % modelfile)
    try:
        with open(modelfile, "rb") as fh:
            modelname, source, datafile, mean_prof, eigvec, tck = \
                _SplineUnpickler(fh).load()
    except UnicodeDecodeError:       # python2 to python3 pickling issues
        with open(modelfile, "rb") as fh:
            modelname, source, datafile, mean_prof, eigvec, tck = \
                _SplineUnpickler(fh, encoding="bytes").load()
    if freqs is None:
        return (modelname, source, datafile, mean_prof, eigvec, tck)
    return (modelname, gen_spline_portrait(mean_prof, freqs, eigvec, tck,
                                           nbin))


# --------------------------------------------------------- device routines --
def get_noise(data, method=default_noise_method, **kwargs):
    """pplib.py:2290-2309."""
    if method == "PS":
        return get_noise_PS(data, **kwargs)
    if method == "fit":
        return get_noise_fit(data, **kwargs)
    print("Unknown get_noise method.")
    return 0


def get_noise_fit(data, fact=1.1, chans=False):
    """pplib.py:2341-2373 on the GPU (ppf_noise_fit_batch; the flattened
    portrait of chans=False, or rows past the LDS transforms, on
    ppf_noise_fit_long)."""
    data = np.asarray(data)
    if chans:
        return engine.noise_fit_rows(np.atleast_2d(data), fact)[0] \
            .cpu().numpy()
    noise = engine.noise_fit_rows(data.ravel()[None, :], fact)[0]
    return np.float64(noise.cpu().numpy()[0])


def find_kc(pows, errs=1.0, fn="exp_dc"):
    """pplib.py:1530-1561 on the GPU (ppf_find_kc_batch): the cutoff harmonic
    where the noise floor of the power spectrum pows begins."""
    if fn not in engine.FIND_KC_FN:
        return 0
    pows = np.asarray(pows, dtype=np.float64)
    return int(engine.find_kc_rows(pows[None, :], errs, fn).cpu().numpy()[0])


def half_triangle_function(a, b, dc, N):
    """pplib.py:1496-1506: N points of the baseline dc carrying a half
    triangle that falls from b at index 0 to zero at its base floor(a)."""
    base = int(np.floor(a))
    out = np.zeros(N) + dc
    out[:base] += b - (np.float64(b) / base) * np.arange(base)
    return out


def find_kc_function(params, data, errs=1.0, fn="exp_dc"):
    """pplib.py:1509-1527: the (weighted) chi-squared find_kc minimises over
    params = (a, b, dc); 0.0 for an unknown fn."""
    a, b, dc = params[:3]
    nharm = len(data)
    if fn == "half_tri":
        model = half_triangle_function(a, b, dc, nharm)
    elif fn == "exp_dc":
        model = b * np.exp(-a * np.arange(nharm)) + dc
    else:
        return 0.0
    return np.sum(((data - model) / errs) ** 2.0)


def brickwall_filter(N, kc):
    """pplib.py:1468-1476: N points, ones before index kc and zeros from
    it."""
    wall = np.zeros(N)
    wall[:kc] = 1.0
    return wall


def wiener_filter(prof, noise):
    """pplib.py:1450-1464 (marked under construction in the reference, whose
    behaviour is kept): pows / (pows + noise**2) of the profile's power
    spectrum."""
    spec = np.fft.rfft(prof)
    pows = np.real(spec * np.conj(spec)) / len(prof)
    return pows / (pows + noise ** 2)


def fit_brickwall(prof, noise):
    """pplib.py:1479-1493 (under construction in the reference, kept as it
    is): the kc whose brickwall lies nearest the Wiener filter."""
    wf = wiener_filter(prof, noise)
    nharm = len(wf)
    dist = [np.sum((wf - brickwall_filter(nharm, kc)) ** 2)
            for kc in range(nharm)]
    return np.array(dist).argmin()


def get_noise_PS(data, frac=4, chans=False):
    """pplib.py:2312-2338 on the GPU (ppf_noise_batch)."""
    data = np.asarray(data)
    if chans:
        return engine.noise_rows(np.atleast_2d(data), frac).cpu().numpy()
    row = data.ravel()
    if not engine.noise_len_supported(row.size):
        # the flattened portrait (nchan nbin samples; pplib.py:2334-2338) is
        # longer than the LDS transforms of ppf_noise_batch (even <= 8192,
        # odd <= 4095 points): the long transforms of ppf_noise_long
        return engine.noise_long(row, frac)
    return float(engine.noise_rows(row[None, :], frac).cpu().numpy()[0])


def get_red_chi2(data, model, errs=None, dof=None):
    """pplib.py:754-779 (host: a single residual sum; the batched per-channel
    form used by get_channels_to_zap runs on the GPU, ppf_resid_chi2_batch)."""
    data = np.asarray(data, dtype=np.float64)
    resids = data - model
    if errs is None:
        if len(data.shape) == 1:
            errs = get_noise(data)
        elif len(data.shape) == 2:
            errs = get_noise(data, chans=True)
        else:
            print("Can only handle 1- or 2-D input.")
    if dof is None:
        dof = sum(data.shape)
    if len(data.shape) == 1:
        return np.sum((resids / errs) ** 2.0) / dof
    return np.array([(resids[ii] / errs[ii]) ** 2.0 for ii in
                     range(len(resids))]).sum() / dof


def rotate_data(data, phase=0.0, DM=0.0, Ps=None, freqs=None, nu_ref=np.inf):
    """pplib.py:2427-2515: per-row phases on the host, FFT rotation on the
    GPU (ppf_rotate_batch)."""
    data = np.asarray(data)
    shape, ndim = data.shape, data.ndim
    nbin = shape[-1]
    if DM == 0.0:
        nrows = int(np.prod(shape[:-1])) if ndim > 1 else 1
        out = engine.rotate_rows(data.reshape(nrows, nbin),
                                 np.full(nrows, float(phase)), ref_len=True)
        return engine.dev_to_host(out).reshape(shape[:-1] + (out.shape[-1],))
    d4 = data                       # only read: the result is a new array
    while d4.ndim != 4:
        d4 = d4[None]
    nsub, npol, nchan = d4.shape[:3]
    D = Dconst * DM / (np.ones(nsub) * Ps)
    if len(D) != nsub:
        print("Wrong shape for array of periods.")
        return 0
    try:
        float(nu_ref)
    except TypeError:
        print("Only one nu_ref permitted.")
        return 0
    if not hasattr(freqs, "ndim"):
        freqs = np.ones(nchan) * freqs
    if freqs.ndim == 0:
        freqs = np.ones(nchan) * float(freqs)
    if freqs.ndim == 1:
        if nchan != len(freqs):
            print("Wrong number of frequencies.")
            return 0
        fterm = np.tile(freqs, nsub).reshape(nsub, nchan) ** -2.0 - \
            nu_ref ** -2.0
    else:
        fterm = freqs ** -2.0 - nu_ref ** -2.0
    if fterm.shape[1] != nchan or fterm.shape[0] != nsub:
        print("Wrong shape for frequency array.")
        return 0
    if ndim not in (1, 2, 4):
        print("Wrong number of dimensions.")
        return 0
    ph = phase + D[:, None] * fterm
    ph = np.broadcast_to(ph[:, None, :], (nsub, npol, nchan))
    out = engine.rotate_rows(d4.reshape(-1, nbin), ph.reshape(-1),
                             ref_len=True)
    out = engine.dev_to_host(out).reshape(d4.shape[:3] + (out.shape[-1],))
    if ndim == 1:
        return out[0, 0, 0]
    if ndim == 2:
        return out[0, 0]
    return out


def rotate_portrait(port, phase=0.0, DM=None, P=None, freqs=None,
                    nu_ref=np.inf):
    """pplib.py:2518-2550."""
    port = np.asarray(port)
    nchan = len(port)
    if DM is None and freqs is None:
        ph = np.full(nchan, float(phase))
    else:
        D = Dconst * DM / P
        ph = phase + D * (np.asarray(freqs, dtype=float) ** -2.0 -
                          nu_ref ** -2.0)
    return engine.rotate_rows(port, ph, ref_len=True).cpu().numpy()


def rotate_profile(profile, phase=0.0):
    """pplib.py:2641-2652."""
    profile = np.asarray(profile)
    return engine.rotate_rows(profile[None, :], [phase],
                              ref_len=True).cpu().numpy()[0]


def add_DM_nu(port, phase=0.0, DM=None, P=None, freqs=None, xs=[-2.0],
              Cs=[1.0], nu_ref=np.inf):
    """pplib.py:2601-2638: rotate_portrait with the dispersive term sum_j C_j
    (nu**x_j - nu_ref**x_j); the per-channel phases on the host, the
    rotation on the GPU (ppf_rotate_batch)."""
    port = np.asarray(port)
    nchan = len(port)
    if DM is None and freqs is None:
        ph = np.full(nchan, float(phase))
    else:
        D = Dconst * DM / P
        freqs = np.asarray(freqs, dtype=float)
        if not hasattr(Cs, "__iter__"):
            Cs = np.ones(len(xs))
        if len(Cs) < len(xs):
            Cs = list(Cs) + list(np.ones(len(xs) - len(Cs)))
        freq_term = 0.0
        for C, x in zip(Cs, xs):
            freq_term = freq_term + C * (freqs ** x - nu_ref ** x)
        ph = phase + (D * freq_term)
    return engine.rotate_rows(port, ph, ref_len=True).cpu().numpy()


def add_scintillation(port, params=None, random=True, nsin=2, amax=1.0,
                      wmax=3.0):
    """pplib.py:1190-1218: the sinusoidal pattern on the host, the product a
    broadcast."""
    from . import fake
    port = np.asarray(port)
    if params is None and random is False:
        return port
    if params is None:
        params = fake.random_scint_params(nsin, amax, wmax)
    pattern = fake.scint_pattern(len(port), params)
    return np.transpose(np.transpose(port) * pattern)


def fit_phase_shift(data, model, noise=None, bounds=[-0.5, 0.5], Ns=100):
    """pplib.py:2136-2182 on the GPU: brute grid of Ns points + scipy-fmin
    replica (Nelder-Mead) polish, then the reference's error formulas."""
    t0 = time.time()
    out = engine.phase_shift_batch(
        np.asarray(data)[None, :], np.asarray(model, dtype=float)[None, :],
        None if noise is None else np.array([noise], dtype=float), Ns,
        bounds).cpu().numpy()[0]
    return DataBunch(phase=out[0], phase_err=out[1], scale=out[2],
                     scale_err=out[3], snr=out[4], red_chi2=out[5],
                     duration=time.time() - t0)


def _phase_terms(theta, model, data, freqs, P, nu_ref, order):
    """Per channel Cdp = Re sum_k d_k conj(m_k) e^{2 pi i k phi_n} and its
    first two phase derivatives (pplib.py:1373-1377, 1400-1401, 1438-1439) at
    (phase, DM) on the GPU: ppf_eval_batch without scattering and with unit
    errors, whose channel terms C, dC[0], d2C[0, 0] they are."""
    model = np.atleast_2d(np.asarray(model))
    data = np.atleast_2d(np.asarray(data))
    nchan = model.shape[0]
    _, _, _, t = engine.eval_points(
        np.array([[theta[0], theta[1], 0.0, 0.0, 0.0]]), data, model,
        np.ones(nchan), P, freqs, [nu_ref, np.inf, np.inf], log10_tau=False,
        order=order, per_channel=True)
    t = t.cpu().numpy()[0, 0]
    return t[0], t[2], t[12]


def fit_phase_shift_function(phase, model=None, data=None, err=None):
    """pplib.py:1294-1306: -Re sum_k d_k conj(m_k) e^{2 pi i k phase} /
    err^2 (Fourier-domain model and data of one profile)."""
    C, _, _ = _phase_terms([phase, 0.0], model, data, [1.0], 1.0, np.inf, 0)
    return -C[0] / err ** 2.0


def fit_phase_shift_function_deriv(phase, model=None, data=None, err=None):
    """pplib.py:1309-1319: the first derivative of fit_phase_shift_function."""
    _, dC, _ = _phase_terms([phase, 0.0], model, data, [1.0], 1.0, np.inf, 1)
    return -dC[0] / err ** 2.0


def fit_phase_shift_function_2deriv(phase, model=None, data=None, err=None):
    """pplib.py:1322-1332: the second derivative."""
    _, _, d2C = _phase_terms([phase, 0.0], model, data, [1.0], 1.0, np.inf, 2)
    return -d2C[0] / err ** 2.0


def fit_portrait_function(params, model=None, p_n=None, data=None, errs=None,
                          P=None, freqs=None, nu_ref=np.inf):
    """pplib.py:1335-1379: -sum_n Cdp_n^2 / (err_n^2 p_n) at params =
    (phase, DM); the caller's p_n stands where the full function has S.
    Without P or freqs the DM term is dropped, as in the reference."""
    if P is None or freqs is None:
        theta, fr, per = [params[0], 0.0], np.ones(len(model)), 1.0
    else:
        theta, fr, per = params, np.asarray(freqs, dtype=float), P
    Cdp, _, _ = _phase_terms(theta, model, data, fr, per, nu_ref, 0)
    return -np.sum(Cdp ** 2.0 / (np.asarray(errs) ** 2.0 * np.asarray(p_n)))


def fit_portrait_function_deriv(params, model=None, p_n=None, data=None,
                                errs=None, P=None, freqs=None, nu_ref=np.inf):
    """pplib.py:1382-1405: the two first derivatives of
    fit_portrait_function."""
    freqs = np.asarray(freqs, dtype=float)
    Cdp, d1, _ = _phase_terms(params, model, data, freqs, P, nu_ref, 1)
    w = -2 * Cdp * d1 / (np.asarray(errs) ** 2.0 * np.asarray(p_n))
    dDM = (freqs ** -2.0 - nu_ref ** -2.0) * (Dconst / P)
    return np.array([w.sum(), (w * dDM).sum()])


def fit_portrait_function_2deriv(params, model=None, p_n=None, data=None,
                                 errs=None, P=None, freqs=None,
                                 nu_ref=np.inf):
    """pplib.py:1408-1447: (d2/dphi2, d2/dDM2, d2/dphi dDM) of
    fit_portrait_function and the zero-covariance frequency nu_zero."""
    freqs = np.asarray(freqs, dtype=float)
    Cdp, d1, d2 = _phase_terms(params, model, data, freqs, P, nu_ref, 2)
    W_n = (d1 ** 2.0 + Cdp * d2) / (np.asarray(errs) ** 2.0 *
                                    np.asarray(p_n))
    dDM = (freqs ** -2.0 - nu_ref ** -2.0) * (Dconst / P)
    nu_zero = (W_n.sum() / np.sum(W_n * freqs ** -2)) ** 0.5
    return (np.array([(-2.0 * W_n).sum(), (-2.0 * W_n * dDM ** 2.0).sum(),
                      (-2.0 * W_n * dDM).sum()]), nu_zero)


def fit_portrait(data, model, init_params, P, freqs, nu_fit=None, nu_out=None,
                 errs=None, bounds=[(None, None), (None, None)], id=None,
                 quiet=True):
    """pplib.py:2185-2287: phase + DM FFTFIT on the GPU (ppf_fit2_batch).

    The reference minimises with scipy TNC; the device runs the trust-region
    Newton solver of fit_portrait_full on the same objective
    (pplib.py:1335-1447), which converges to the same stationary point
    (SURVEY.md Appendix A.5).  ``bounds`` on (phase, DM) hold as TNC's
    do: the device trust-region steps are projected onto the box
    (ppf_fit_desc.bounds)."""
    data = np.asarray(data)
    freqs = np.asarray(freqs, dtype=float)
    nchan, nbin = data.shape
    if nu_fit is None:
        nu_fit = freqs.mean()
    init = np.zeros((1, 5))
    init[0, :2] = np.asarray(init_params, dtype=float)[:2]
    t0 = time.time()
    res = engine.fit_batch(
        data[None], np.asarray(model, dtype=float)[None], freqs[None], [P],
        init, [1, 1, 0, 0, 0], nu_fits=np.full((1, 3), nu_fit),
        nu_outs=np.full((1, 3), np.nan if nu_out is None else nu_out),
        errs=None if errs is None else np.asarray(errs, dtype=float)[None],
        mode=_lib.PPF_MODE_LEGACY2, bounds=_box(bounds, 2))
    r = engine.results_numpy(res)
    duration = time.time() - t0
    R, I = r["results"][0], _lib.RESULT_INDEX
    status = int(R[I["status"]])
    _raise_status(status)
    rc = status & 0xff
    if not quiet and rc not in (1, 2, 4):
        sys.stderr.write("Fit failed with return code %d -- %s" %
                         (rc, RCSTRINGS.get(str(rc), "")))
    cov = r["covariance"][0]
    return DataBunch(phase=R[I["params"]][0], phase_err=R[I["param_errs"]][0],
                     DM=R[I["params"]][1], DM_err=R[I["param_errs"]][1],
                     scales=r["scales"][0], scale_errs=r["scale_errs"][0],
                     nu_ref=R[I["nu_out"]][0], covariance=cov[0, 1],
                     chi2=R[I["chi2"]], red_chi2=R[I["red_chi2"]],
                     snr=R[I["snr"]], duration=duration,
                     nfeval=int(R[I["nfeval"]]), return_code=rc)


def _box(bounds, n):
    """[5, 2] device bounds from the first n (lower, upper) pairs of a
    scipy bounds list (None: unbounded); None when nothing is bounded."""
    if bounds is None:
        return None
    b = np.full((5, 2), np.nan)
    for i, lu in enumerate(list(bounds)[:n]):
        if lu is None:
            continue
        for j in (0, 1):
            if lu[j] is not None:
                b[i, j] = float(lu[j])
    return None if np.isnan(b).all() else b


def _raise_status(status):
    """Map device status bits to the exceptions the reference raises."""
    if status & _lib.ST_NO_ROOT:
        raise ValueError("attempt to get argmin of an empty sequence "
                         "(no positive real zero-covariance frequency)")
    if status & _lib.ST_SINGULAR:
        raise np.linalg.LinAlgError("Singular matrix")
    if status & _lib.ST_NOFIT:
        raise ValueError("nothing to fit (no fit flag set or no channel)")
    if status & _lib.ST_NOSPACE:
        # the workspace had fewer cross-spectrum slots than fits that stream
        # it (the host's count disagreed with the device's k_classify): an
        # internal error, never a fit outcome
        raise RuntimeError("internal error: no cross-spectrum slot for a "
                           "scattering fit (PPF_ST_NOSPACE)")


# ------------------------------------- PCA + wavelet smoothing (ppspline) --
def count_crossings(x, x0):
    """pplib.py:710-718: how often x crosses the level x0 (changes of the
    sign of x - x0 between neighbours, less the samples exactly on it)."""
    d = np.asarray(x) - x0
    s = np.sign(d)
    return int(np.count_nonzero(s[1:] != s[:-1]) - np.count_nonzero(d == 0))


def get_SNR(prof, fudge=3.25):
    """pplib.py:2376-2395: sum / (noise sqrt(W_eq)) / fudge of a
    baseline-removed profile; 0 where the equivalent width is not positive."""
    prof = np.asarray(prof, dtype=float)
    noise = get_noise(prof)
    Weq = prof.sum() / prof.max()
    mask = np.where(Weq <= 0.0, 0.0, 1.0)
    Weq = np.where(Weq <= 0.0, 1.0, Weq)
    return prof.sum() / (noise * Weq ** 0.5) * mask / fudge


def normalize_portrait(port, method="rms", weights=None, return_norms=False):
    """pplib.py:2553-2598: each non-zero profile divided by its mean
    ('mean'), maximum ('max'), fitted scale against the weighted mean
    profile ('prof', fit_phase_shift), off-pulse noise ('rms', get_noise)
    or Euclidean length ('abs')."""
    if method not in ("mean", "max", "prof", "rms", "abs"):
        print("Unknown method for normalize_portrait(...), '%s'." % method)
        return None
    port = np.asarray(port, dtype=float)
    norm_port = np.zeros(port.shape)
    norm_vals = np.ones(len(port))
    if method == "prof":
        good = np.where(port.sum(axis=1) != 0.0)[0]
        w = np.ones(len(good)) if weights is None else \
            np.asarray(weights)[good]
        mean_prof = np.average(port[good], axis=0, weights=w)
    for ichan, prof in enumerate(port):
        if not prof.any():
            continue
        if method == "mean":
            norm = prof.mean()
        elif method == "max":
            norm = prof.max()
        elif method == "prof":
            norm = fit_phase_shift(prof, mean_prof).scale
        elif method == "rms":
            norm = get_noise(prof)
        else:
            norm = (prof ** 2.0).sum() ** 0.5
        norm_port[ichan] = prof / norm
        norm_vals[ichan] = norm
    if return_norms:
        return norm_port, norm_vals
    return norm_port


def pca(port, mean_prof=None, weights=None, quiet=False):
    """pplib.py:1564-1602: principal components of the nchan x nbin port,
    the eigen-decomposition of np.cov(delta_port.T, aweights=weights,
    ddof=1), sorted by decreasing eigenvalue (eigenvectors are columns).

    The covariance follows np.cov exactly: it subtracts its own weighted
    average of delta_port again and normalises by sum(w) - sum(w^2) /
    sum(w).  Host float64; the eigh is LAPACK either way.

    Deviation from the reference: with nchan < nbin the nbin x nbin
    covariance (rank <= nchan) is never formed; the nchan x nchan dual
    sqrt(w) Xc Xc^T sqrt(w) is diagonalised and its eigenvectors projected
    back.  Returned are eigval [nbin] (zero beyond the rank) and eigvec
    [nbin, min(nchan, nbin)] with unit columns, where the reference returns
    nbin x nbin; a column whose eigenvalue is below n eps lambda_max (n the
    diagonalised dimension) is zero, where the reference returns an
    arbitrary basis of the null space.  Only the first ten columns are ever
    looked at (find_significant_eigvec).  Eigenvector signs are LAPACK's and
    may differ from the reference's."""
    port = np.asarray(port, dtype=np.float64)
    nmes, ndim = port.shape
    if not quiet:
        print("Performing principal component analysis on data with %d "
              "dimensions and %d measurements..." % (ndim, nmes))
    w = np.ones(nmes) if weights is None else \
        np.asarray(weights, dtype=np.float64)
    if mean_prof is None:
        mean_prof = (port.T * w).T.sum(axis=0) / w.sum()
    X = port - mean_prof
    wsum = w.sum()
    X = X - (X * w[:, None]).sum(axis=0) / wsum     # np.cov's own average
    norm = wsum - (w * w).sum() / wsum
    ncol = min(nmes, ndim)
    eigval = np.zeros(ndim)
    if nmes < ndim:
        Z = X * np.sqrt(w)[:, None]
        lam, U = np.linalg.eigh(np.dot(Z, Z.T) / norm)
        order = np.argsort(lam)[::-1]
        lam, U = lam[order], U[:, order]
        V = np.dot(Z.T, U)
    else:
        lam, V = np.linalg.eigh(np.dot(X.T * w, X) / norm)
        order = np.argsort(lam)[::-1]
        lam, V = lam[order], V[:, order]
    keep = lam >= len(lam) * np.finfo(np.float64).eps * max(lam[0], 0.0)
    keep &= lam > 0.0
    eigvec = np.zeros((ndim, ncol))
    lengths = np.sqrt((V * V).sum(axis=0))
    eigvec[:, keep] = V[:, keep] / lengths[keep]
    eigval[:ncol] = np.where(keep, lam, 0.0)
    return eigval, eigvec


def reconstruct_portrait(port, mean_prof, eigvec):
    """pplib.py:1605-1622: port projected onto the column space of eigvec
    about mean_prof."""
    delta_port = np.asarray(port) - mean_prof
    return np.dot(np.dot(delta_port, eigvec), eigvec.T) + mean_prof


def _swt_evaluator(evaluator):
    from . import _swt
    return _swt.default_evaluator() if evaluator is None else evaluator


def _check_wavelet(wavelet):
    if wavelet != "db8":
        raise NotImplementedError("only the 'db8' wavelet is built (the "
                                  "reference's default), got %r" % (wavelet,))


def _soft(threshtype):
    if threshtype not in ("hard", "soft"):
        raise ValueError("threshtype must be 'hard' or 'soft'")
    return int(threshtype == "soft")


def wavelet_smooth(port, wavelet="db8", nlevel=5, threshtype="hard", fact=1.0,
                   evaluator=None):
    """pplib.py:1692-1737 without PyWavelets: the stationary-wavelet
    denoised portrait or profile (ppf_swt_analyse_batch /
    ppf_swt_score_batch; the transform is written from its definition, see
    _swt.py, and has not been compared with PyWavelets itself).  Only 'db8';
    even nbin in [32, 8192], nlevel <= log2(nbin) for a power of two and 1
    otherwise, else NotImplementedError.  evaluator (not in the reference)
    replaces the device evaluator, see _swt."""
    from . import _swt
    _check_wavelet(wavelet)
    port = np.asarray(port, dtype=np.float64)
    one_prof = port.ndim == 1
    rows = np.atleast_2d(port)
    _swt.check_shape(rows.shape[1], nlevel)
    ev = _swt_evaluator(evaluator)
    h = ev.analyse(rows, nlevel, len(rows))
    soft = _soft(threshtype)
    smooth = ev.score(h, [(i, nlevel, soft) for i in range(len(rows))],
                      [fact] * len(rows), smooth=True)[1]
    return smooth[0] if one_prof else smooth


def _wavelet_snr(score, rchi2_tol):
    """The figure of merit of fit_wavelet_smooth_function from one
    (signal, noise, red_chi2) triple."""
    from . import _swt
    return _swt.wavelet_snr(score, rchi2_tol)


def fit_wavelet_smooth_function(fact, prof, wavelet, nlevel, threshtype,
                                rchi2_tol, evaluator=None):
    """pplib.py:1814-1838: minus the pseudo-S/N of the smoothed profile
    (Fourier-domain signal over noise), 0 when the reduced chi^2 between
    profile and smoothed profile is further than rchi2_tol from 1."""
    from . import _swt
    _check_wavelet(wavelet)
    prof = np.asarray(prof, dtype=np.float64)
    _swt.check_shape(len(prof), nlevel)
    ev = _swt_evaluator(evaluator)
    h = ev.analyse(prof[None, :], nlevel, 1)
    fact = float(np.ravel(fact)[0])
    out = ev.score(h, [(0, nlevel, _soft(threshtype))], [fact])[0]
    return _wavelet_snr(out[0], rchi2_tol)


def smart_smooth(port, try_nlevels=None, rchi2_tol=0.1, **kwargs):
    """pplib.py:1740-1811: per profile the (nlevel, fact) of wavelet_smooth
    that maximise the pseudo-S/N with the reduced chi^2 within rchi2_tol of
    1, searched as the reference searches: scipy.optimize.brute over fact
    in [0, 3] (Ns = 30, the default fmin finish) for every level, the best
    level kept; a profile whose final chi^2 fails the gate comes back zero.
    The 30 grid values of every (profile, level) are computed by ONE batched
    evaluator call up front and served to brute from a table; the fmin
    finish evaluates singly.  try_nlevels = 0, odd nbin (the input back; a
    single profile as a [1, nbin] array, as the reference has it) and
    all-zero rows return as in the reference; a length that is not a power
    of two tries one level.  kwargs: threshtype, wavelet ('db8' only) and evaluator (not
    in the reference: replaces the device evaluator, see _swt).
    search (not in the reference) = "brute" is the above; "batched" gives
    the same result from at most four evaluator calls whatever the number
    of rows: analyse, ev.search (the grid table and every (profile, level)'s
    fmin finish, on the device one workgroup each, k_swt_search), and one
    smoothing call for all rows at their best (level, fact)."""
    import scipy.optimize as opt
    from . import _swt
    search = kwargs.get("search", "brute")
    if search not in ("brute", "batched"):
        raise ValueError("search must be 'brute' or 'batched'")
    if try_nlevels == 0:
        return port
    port = np.asarray(port, dtype=np.float64)
    one_prof = port.ndim == 1
    rows = np.atleast_2d(port)
    nbin = rows.shape[1]
    if nbin % 2 != 0:
        # as the reference: a single odd-length profile comes back wrapped
        # in a [1, nbin] array (pplib.py:1765-1769), which is why
        # find_significant_eigvec finds nothing significant at odd nbin
        return rows if one_prof else port
    if np.modf(np.log2(nbin))[0] != 0.0:
        try_nlevels = 1
    elif try_nlevels is None:
        try_nlevels = int(np.log2(nbin))
    _check_wavelet(kwargs.get("wavelet", "db8"))
    soft = _soft(kwargs.get("threshtype", "hard"))
    _swt.check_shape(nbin, try_nlevels)
    ev = _swt_evaluator(kwargs.get("evaluator"))
    smooth_port = np.zeros(rows.shape)
    todo = [i for i, prof in enumerate(rows) if np.any(prof)]
    if not todo:
        return smooth_port[0] if one_prof else smooth_port
    Ns = 30
    # brute's own grid: the table is keyed by the very floats it will pass
    grid = np.mgrid[slice(0.0, 3.0, complex(Ns))]
    ncase = len(todo) * try_nlevels * Ns
    h = ev.analyse(rows[todo], try_nlevels, ncase)
    if search == "batched":
        fact_mins, fun_vals, _ = ev.search(h, soft, rchi2_tol, grid)
        levels = np.argmin(fun_vals, axis=1)
        ips = np.arange(len(todo))
        out, srows = ev.score(h, [(ip, lev + 1, soft)
                                  for ip, lev in zip(ips, levels)],
                              fact_mins[ips, levels], smooth=True)
        keep = ~(np.abs(out[:, 2] - 1.0) > rchi2_tol)
        smooth_port[np.asarray(todo)[keep]] = srows[keep]
        return smooth_port[0] if one_prof else smooth_port
    cases = [(ip, lev, soft) for ip in range(len(todo))
             for lev in range(1, try_nlevels + 1) for _ in range(Ns)]
    table = ev.score(h, cases, np.tile(grid, len(todo) * try_nlevels))[0]
    table = table.reshape(len(todo), try_nlevels, Ns, 3)
    for ip, iprof in enumerate(todo):
        fun_vals = np.zeros(try_nlevels)
        fact_mins = np.zeros(try_nlevels)
        for ilevel in range(try_nlevels):
            known = dict((float(f), table[ip, ilevel, ig])
                         for ig, f in enumerate(grid))

            def objective(fact, ip=ip, lev=ilevel + 1, known=known):
                f = float(np.ravel(fact)[0])
                score = known.get(f)
                if score is None:
                    score = ev.score(h, [(ip, lev, soft)], [f])[0][0]
                return _wavelet_snr(score, rchi2_tol)

            results = opt.brute(objective, ranges=[(0.0, 3.0)], Ns=Ns,
                                full_output=True)
            fact_mins[ilevel] = results[0][0]
            fun_vals[ilevel] = results[1]
        ilevel_min = fun_vals.argmin()
        out, srow = ev.score(h, [(ip, ilevel_min + 1, soft)],
                             [fact_mins[ilevel_min]], smooth=True)
        if not abs(out[0, 2] - 1.0) > rchi2_tol:
            smooth_port[iprof] = srow[0]
    return smooth_port[0] if one_prof else smooth_port


def find_significant_eigvec(eigvec, check_max=10, return_max=10,
                            snr_cutoff=150.0, check_crossings=True,
                            check_acorr=True, return_smooth=True, **kwargs):
    """pplib.py:1625-1689: the indices of the leading eigenvectors (columns
    of eigvec) whose smart_smooth-ed version has a Fourier-domain S/N of at
    least snr_cutoff, with the reference's extra look at borderline ones
    (zero crossings; its autocorrelation branch is kept as written there,
    where it cannot be reached); with return_smooth also the array of
    smoothed eigenvectors.  At odd nbin smart_smooth hands a single profile
    back as a [1, nbin] array, whose rfft(...)[1:] is empty: the S/N is 0 and
    no eigenvector is significant, as in the reference (make_spline_model
    then writes the mean-profile model).  At most eigvec.shape[1] columns are examined
    (pca returns min(nchan, nbin) of them).  kwargs go to smart_smooth."""
    eigvec = np.asarray(eigvec, dtype=np.float64)
    ev_ = _swt_evaluator(kwargs.get("evaluator")) \
        if eigvec.shape[1] else None
    if return_smooth:
        smooth_eigvec = np.zeros(eigvec.shape)
    ieig = []
    for ivec in range(min(max(check_max, return_max), eigvec.shape[1])):
        add_eigvec = False
        raw = eigvec[:, ivec]
        ev = smart_smooth(raw, **kwargs)
        ev_noise = ev_.noise(raw[None, :])[0] * np.sqrt(len(ev) / 2.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ev_snr = np.sum(np.abs(np.fft.rfft(ev)[1:]) ** 2) / ev_noise
        if ev_snr >= snr_cutoff:
            close = ev_snr < 3 * snr_cutoff
            if check_crossings and close:
                ncross = count_crossings(abs(ev), 0.1 * abs(ev).max())
                if ncross < int(0.02 * len(ev)):
                    add_eigvec = True
            elif check_acorr and close and add_eigvec:
                acorr = np.correlate(ev, ev, "same")
                fwhm = acorr.argmax() - \
                    np.where(acorr > acorr.max() / 2.0)[0].min()
                add_eigvec = bool(fwhm > 5)
                if not add_eigvec:
                    print("Borderline case eigenvector %d failed test." % ivec)
            else:
                add_eigvec = True
        if add_eigvec:
            ieig.append(ivec)
            if return_smooth:
                smooth_eigvec[:, ivec] = ev
        if ivec + 1 == check_max or len(ieig) == return_max:
            break
    ieig = np.array(ieig)
    if return_smooth:
        return ieig, smooth_eigvec
    return ieig


# ------------------------------------------------------- simulated archives --
def make_fake_pulsar(modelfile, ephemeris, outfile="fake_pulsar.fits", nsub=1,
                     npol=1, nchan=512, nbin=2048, nu0=1500.0, bw=800.0,
                     tsub=300.0, phase=0.0, dDM=0.0, start_MJD=None,
                     weights=None, noise_stds=1.0, scales=1.0,
                     dedispersed=False, t_scat=0.0, alpha=scattering_alpha,
                     scint=False, xs=None, Cs=None, nu_DM=np.inf,
                     state="Stokes", telescope="GBT", quiet=False, seed=None,
                     dev=None):
    """pplib.py:3302-3499 without PSRCHIVE: one fold-mode PSRFITS file of
    simulated data.  The profiles are built and digitised on the device
    (engine.fake_subints, k_fake) and cross to the host as the 2-byte samples
    the file stores (psrfits.write_psrfits_rows).

    The arguments are the reference's, plus seed (the device RNG's; None
    draws one from np.random) and dev.  Departures, all of them documented in
    fake.fake_tables / fake.read_par / fake.fake_epochs:
      - the ephemeris is read by the reference's plain-text fallback parser
        (PSR or PSRJ, RAJ, DECJ, F0 or P0, F1, PEPOCH, DM);
      - the folding period of a sub-int is 1 / (F0 + F1 dt) at its centre;
        the reference takes it from a TEMPO polyco through PSRCHIVE,
        topocentric Doppler shift included;
      - with xs=None the rows are rotated by phase and DM + dDM (the
        ephemeris DM goes into the header), which the reference leaves to
        PSRCHIVE's dededisperse() with the effect that its phase and dDM do
        nothing; with xs given, phase is transformed once per sub-int, not
        compounded;
      - the noise comes from the device RNG, so the global NumPy stream is
        consumed only by seed=None and by scint=True, not once per profile.
    Every channel gets data whatever its weight.  Each polarisation is the
    same model with its own noise draw; npol = 1 is written as AA+BB, npol =
    4 as IQUV (state "Stokes") or AABBCRCI ("Coherence").  Other npol and
    dedispersed=True raise NotImplementedError (the loader does not recognise
    dedispersed files), as does an odd nbin or one outside [32, 8192]."""
    from . import fake, psrfits
    if dedispersed:
        raise NotImplementedError("dedispersed=True: psrfits.load_data does "
                                  "not recognise dedispersed files")
    if npol == 1:
        pol_type = "AA+BB"
    elif npol == 4 and state in ("Stokes", "Coherence"):
        pol_type = "IQUV" if state == "Stokes" else "AABBCRCI"
    else:
        raise NotImplementedError("npol=%r state=%r: npol 1, or 4 as Stokes "
                                  "/ Coherence" % (npol, state))
    if nbin % 2 or nbin < 32 or nbin > 8192:
        raise NotImplementedError("nbin=%d: even nbin in [32, 8192]" % nbin)
    setup = fake.fake_setup(modelfile, ephemeris, nsub=nsub, npol=npol,
                            nchan=nchan, nbin=nbin, nu0=nu0, bw=bw, tsub=tsub,
                            phase=phase, dDM=dDM, start_MJD=start_MJD,
                            noise_stds=noise_stds, scales=scales,
                            t_scat=t_scat, alpha=alpha, scint=scint, xs=xs,
                            Cs=Cs, nu_DM=nu_DM)
    if setup == 0:
        return 0
    par, ep, tab, mdl = setup
    if weights is None:
        weights = np.ones([nsub, nchan])
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1))
    dev = engine.device(dev)
    data, scl, offs = engine.fake_subints(
        fake.templates(mdl, tab, dev=dev), tab.model_of, tab.phi, tab.tau_n,
        tab.gain, tab.noise, seed, quantized=True, dev=dev)
    DECJ = par.DECJ if par.DECJ[0] in "+-" else "+" + par.DECJ
    psrfits.write_psrfits_rows(
        outfile, engine.dev_to_host_view(data), engine.dev_to_host(scl),
        engine.dev_to_host(offs), np.tile(tab.freqs, (nsub, 1)), weights,
        ep.Ps, ep.offs_sub, np.full(nsub, float(tsub)), nbin,
        stt_imjd=ep.stt_imjd, stt_smjd=ep.stt_smjd, stt_offs=ep.stt_offs,
        npol=npol, pol_type=pol_type, telescope=telescope, source=par.PSR,
        dm=par.DM, obsfreq=nu0, obsbw=bw, ra=par.RAJ, dec=DECJ)
    if not quiet:
        print("\nUnloaded %s.\n" % outfile)


# ------------------------------------------------------- archive writers --
def _pol_type(npol, state):
    """The POL_TYPE make_fake_pulsar writes: npol 1 as AA+BB, npol 4 as IQUV
    (state "Stokes") or AABBCRCI ("Coherence")."""
    if npol == 1:
        return "AA+BB"
    if npol == 4 and state in ("Stokes", "Coherence"):
        return "IQUV" if state == "Stokes" else "AABBCRCI"
    raise NotImplementedError("npol=%r state=%r: npol 1, or 4 as Stokes / "
                              "Coherence" % (npol, state))


def write_archive(data, ephemeris, freqs, nu0=None, bw=None,
                  outfile="pparchive.fits", tsub=1.0, start_MJD=None,
                  weights=None, dedispersed=False, state="Stokes",
                  telescope="GBT", quiet=False, elem="I", dev=None,
                  fd_poln=None):
    """pplib.py:3189-3299 without PSRCHIVE: data [nsub, npol, nchan, nbin]
    (a NumPy array or a device tensor) becomes one fold-mode PSRFITS file.
    The samples are digitised on the device (psrfits.write_archive_rows,
    ppf_pack_psrfits_batch) and cross to the host as the bytes of the file.

    The arguments are the reference's, with its defaults for nu0 (the mean
    of freqs) and bw (the span of freqs plus one channel spacing), plus elem
    ("I": 16-bit samples with per-profile DAT_SCL / DAT_OFFS, "E": float32
    samples), dev and fd_poln (the feed basis, "LIN" or "CIRC": the FD_POLN
    card, written only when given).  freqs: [nchan], or [nsub, nchan].
    Departures:
      - the ephemeris, the epochs and the folding periods are
        make_fake_pulsar's (fake.read_par, fake.fake_epochs): start_MJD
        defaults to PEPOCH, and sub-int i is centred tsub / 2 + i tsub
        seconds after it with the period 1 / (F0 + F1 dt);
      - the rows are stored as they are given: the reference hands them to
        PSRCHIVE as dedispersed and lets its dededisperse() rotate them by
        the ephemeris DM before unloading.  dedispersed=True raises
        NotImplementedError (psrfits.load_data does not recognise
        dedispersed files);
      - npol 1 is written as AA+BB, npol 4 as IQUV ("Stokes") or AABBCRCI
        ("Coherence"); other npol raise NotImplementedError.
    Non-finite data raises ValueError before anything is launched."""
    from . import fake, psrfits
    if dedispersed:
        raise NotImplementedError("dedispersed=True: psrfits.load_data does "
                                  "not recognise dedispersed files")
    if len(data.shape) != 4:
        raise ValueError("data must be [nsub, npol, nchan, nbin]")
    nsub, npol, nchan, nbin = (int(n) for n in data.shape)
    pol_type = _pol_type(npol, state)
    freqs = np.asarray(freqs, dtype=np.float64)
    if freqs.shape not in ((nchan,), (nsub, nchan)):
        raise ValueError("freqs must be [nchan] = [%d]" % nchan)
    if nu0 is None:
        nu0 = freqs.mean()
    if bw is None:
        if nchan < 2:
            raise ValueError("bw must be given for a single channel")
        f1 = freqs.reshape(-1, nchan)[0]
        bw = (freqs.max() - freqs.min()) + abs(f1[1] - f1[0])
    if weights is None:
        weights = np.ones([nsub, nchan])
    weights = np.asarray(weights, dtype=np.float64)
    if weights.shape != (nsub, nchan):
        raise ValueError("weights must be [nsub, nchan] = [%d, %d]"
                         % (nsub, nchan))
    psrfits.check_finite(data)
    par = fake.read_par(ephemeris)
    ep = fake.fake_epochs(par, nsub, tsub, start_MJD)
    DECJ = par.DECJ if par.DECJ[0] in "+-" else "+" + par.DECJ
    psrfits.write_archive_rows(
        outfile, data, np.broadcast_to(freqs, (nsub, nchan)), weights, ep.Ps,
        ep.offs_sub, np.full(nsub, float(tsub)), stt_imjd=ep.stt_imjd,
        stt_smjd=ep.stt_smjd, stt_offs=ep.stt_offs, pol_type=pol_type,
        telescope=telescope, source=par.PSR, dm=par.DM, obsfreq=float(nu0),
        obsbw=float(bw), ra=par.RAJ, dec=DECJ, elem=elem, dev=dev,
        fd_poln=fd_poln)
    if not quiet:
        print("\nUnloaded %s.\n" % outfile)


def unload_new_archive(data, arch, outfile, DM=None, dmc=0, weights=None,
                       quiet=False, elem="I", dev=None, fd_poln=None):
    """pplib.py:3146-3186 without PSRCHIVE: a copy of an archive with new
    amplitudes.  arch stands in for the PSRCHIVE object: the name of a
    fold-mode PSRFITS file, or a DataBunch from psrfits.load_data.
    Telescope, frontend, backend, source, centre frequency, bandwidth,
    channel frequencies, periods, epochs, sub-int lengths, parallactic
    angles, weights and DM are copied from it; DM and weights ([nsub,
    nchan]) override when given.  The feed basis (the FD_POLN card) is
    written when fd_poln is given or arch's is CIRC (LIN, what a file
    without the card reads as, writes none).  data: [nsub,
    npol, nchan, nbin] of arch's shape (a DataBunch from load_data is total
    intensity, npol 1, or a polarised load's npol 4 in its state), a NumPy
    array or a device tensor, digitised on the device
    (psrfits.write_archive_rows; elem "I" or "E").

    The data are stored as given, dededispersed (dmc = 0); dmc true raises
    NotImplementedError (psrfits.load_data does not recognise dedispersed
    files).  A shape that disagrees with arch and non-finite data raise
    ValueError.  A DataBunch carries no coordinates: the RA / DEC cards are
    copied only from a file."""
    from . import psrfits
    if dmc:
        raise NotImplementedError("dmc=%r: psrfits.load_data does not "
                                  "recognise dedispersed files" % (dmc,))
    m = psrfits.archive_meta(arch) if isinstance(arch, str) else arch
    shape = tuple(int(m[k]) for k in ("nsub", "npol", "nchan", "nbin"))
    if len(data.shape) != 4 or tuple(int(n) for n in data.shape) != shape:
        raise ValueError("data shape %s != the archive's %s"
                         % (tuple(data.shape), shape))
    nsub, npol, nchan, nbin = shape
    pol_type = m.get("pol_type") or _pol_type(
        npol, "Stokes" if m.get("state") in (None, "Intensity") else m["state"])
    weights = np.asarray(m["weights"] if weights is None else weights,
                         dtype=np.float64)
    if weights.shape != (nsub, nchan):
        raise ValueError("weights must be [nsub, nchan] = [%d, %d]"
                         % (nsub, nchan))
    if fd_poln is None and m.get("fd_poln") == "CIRC":
        fd_poln = "CIRC"
    psrfits.check_finite(data)
    # the start of the first sub-int, whose epoch is its centre; OFFS_SUB
    # counts from there to every centre
    tsub = np.asarray(m["subtimes"], dtype=np.float64).reshape(nsub)
    epochs = list(m["epochs"])
    start = epochs[0] + (-tsub[0] / 2.0)
    sec = start.fracday() * 86400.0
    smjd = int(np.floor(sec))
    offs_sub = np.array([((e.intday() - start.intday()) +
                          (e.fracday() - start.fracday())) * 86400.0
                         for e in epochs])
    psrfits.write_archive_rows(
        outfile, data, np.asarray(m["freqs"], dtype=np.float64), weights,
        np.asarray(m["Ps"], dtype=np.float64), offs_sub, tsub,
        stt_imjd=start.intday(), stt_smjd=smjd, stt_offs=sec - smjd,
        pol_type=pol_type, telescope=m["telescope"], frontend=m["frontend"],
        backend=m["backend"], source=m["source"],
        dm=float(m["DM"] if DM is None else DM),
        be_delay=float(m.get("backend_delay", 0.0)),
        par_ang=m.get("parallactic_angles"), obsfreq=float(m["nu0"]),
        obsbw=float(m["bw"]), ra=m.get("ra"), dec=m.get("dec"), elem=elem,
        dev=dev, fd_poln=fd_poln)
    if not quiet:
        print("\nUnloaded %s.\n" % outfile)


def make_constant_portrait(archive, outfile, profile=None, DM=0.0, dmc=False,
                           weights=None, quiet=False):
    """pplib.py:993-1029 without PSRCHIVE: outfile is the fold-mode PSRFITS
    file archive with every (sub-int, polarisation, channel) holding
    profile, header DM as given, unit weights unless weights [nsub, nchan]
    is.  profile=None takes the archive's dedispersed, tscrunched total-
    intensity mean profile (load_data's prof).  A profile of another length
    than the archive's nbin raises AssertionError, as the reference does."""
    from . import psrfits
    m = psrfits.archive_meta(archive)
    shape = tuple(int(m[k]) for k in ("nsub", "npol", "nchan", "nbin"))
    if profile is None:
        profile = load_data(archive, dedisperse=True, tscrunch=True,
                            pscrunch=True, quiet=True).prof
    assert len(profile) == shape[3], \
        "len(profile) != number of bins in dummy archive"
    if weights is None:
        weights = np.ones((shape[0], shape[2]))
    data = np.empty(shape)
    data[:] = np.asarray(profile, dtype=np.float64)
    unload_new_archive(data, archive, outfile, DM=DM, dmc=dmc,
                       weights=weights, quiet=quiet)


# ------------------------------------------------------------- TOA output --
def filter_TOAs(TOAs, flag, cutoff, criterion=">=", pass_unflagged=False,
                return_culled=False):
    """pplib.py:3502-3548 (the >= / <= criteria used by write_TOAs)."""
    import operator
    ops = {">=": operator.ge, "<=": operator.le, ">": operator.gt,
           "<": operator.lt, "==": operator.eq}
    keep, culled = [], []
    for toa in TOAs:
        if flag in toa.flags:
            (keep if ops[criterion](toa.flags[flag], cutoff) else
             culled).append(toa)
        elif pass_unflagged:
            keep.append(toa)
        else:
            culled.append(toa)
    return (keep, culled) if return_culled else keep


def write_TOAs(TOAs, inf_is_zero=True, SNR_cutoff=0.0, outfile=None,
               append=True):
    """pplib.py:3588-3649: loosely IPTA-formatted TOA lines."""
    toas = TOAs if hasattr(TOAs, "__len__") else [TOAs]
    toas = filter_TOAs(toas, "snr", SNR_cutoff, ">=", pass_unflagged=False)
    of = open(outfile, "a" if append else "w") if outfile is not None \
        else None
    for toa in toas:
        freq = 0.0 if (toa.frequency == np.inf and inf_is_zero) else \
            toa.frequency
        line = "%s %.8f %d" % (toa.archive, freq, toa.MJD.intday()) + \
            ("%.15f   %.3f  %s" % (toa.MJD.fracday(), toa.TOA_error,
                                   toa.telescope_code))[1:]
        if toa.DM is not None:
            line += " -pp_dm %.7f" % toa.DM
        if toa.DM_error is not None:
            line += " -pp_dme %.7f" % toa.DM_error
        for flag, value in list(toa.flags.items()):
            if value is None:
                continue
            if hasattr(value, "lower"):
                line += " -%s %s" % (flag, value)
            elif "int" in str(type(value)):
                line += " -%s %d" % (flag, value)
            elif flag.find("_cov") >= 0:
                line += " -%s %.1e" % (flag, value)
            elif flag.find("phs") >= 0:
                line += " -%s %.8f" % (flag, value)
            elif flag.find("flux") >= 0:
                line += " -%s %.5f" % (flag, value)
            else:
                line += " -%s %.3f" % (flag, value)
        if of is not None:
            of.write(line + "\n")
        else:
            print(line)
    if of is not None:
        of.close()


# ------------------------------------------------------------ archive I/O --
def load_data(filename, **kwargs):
    """pplib.py:2749-2915.  Fold-mode PSRFITS files take the PSRCHIVE-free
    fast path (psrfits.load_data: raw DATA bytes to the device, unpacked,
    baseline-removed and pscrunched there); any other archive format needs
    PSRCHIVE, which is not installed in this image."""
    if file_is_type(filename, "FITS"):
        from . import psrfits
        return psrfits.load_data(filename, **kwargs)
    try:
        import psrchive  # noqa: F401
    except ImportError as exc:
        raise ImportError("load_data needs the PSRCHIVE Python bindings for "
                          "non-PSRFITS archives (archive I/O is host-side "
                          "and out of the accelerated path)") from exc
    raise NotImplementedError("PSRCHIVE-backed load_data is not provided in "
                              "this build; pass a DataBunch with the keys of "
                              "pplib.py:2904-2914")


def file_is_type(filename, filetype="ASCII"):
    """pplib.py:3126-3143 without the `file -L` subprocess: FITS files start
    with 'SIMPLE  =', ASCII metafiles decode as text."""
    with open(filename, "rb") as fh:
        head = fh.read(4096)
    if filetype == "FITS":
        return head.startswith(b"SIMPLE")
    if filetype == "ASCII":
        if b"\x00" in head or head.startswith(b"SIMPLE"):
            return False
        try:
            head.decode("ascii")
            return True
        except UnicodeDecodeError:
            return False
    return False


# ------------------------------------------------------------ DataPortrait --
_OUTSIDE = "%s is outside the accelerated path"


class DataPortrait(object):
    """The data a portrait model is made from (pplib.py:155-349);
    ppgauss.DataPortrait and ppspline.DataPortrait add their model makers.
    datafile: a fold-mode PSRFITS file (loaded with dedisperse=True,
    tscrunch=True on the PSRFITS fast path) or an in-memory DataBunch with
    load_data's keys (subints [nsub, npol, nchan, nbin], masks, freqs [nsub,
    nchan], ok_ichans, noise_stds, SNRs [nsub, npol, nchan], Ps, phases,
    nu0, bw, source; weights [nsub, nchan], unit on ok_ichans when missing);
    its first sub-integration is the portrait.

    A metafile (an ASCII list of fold-mode PSRFITS files, one per line) or,
    not in the reference, a list / tuple of DataBunches joins several
    archives of one pulsar (pplib.py:179-326): their channels are
    concatenated and sorted by frequency, join_ichans / join_ichanxs list
    each archive's channels in the sorted full / condensed portrait, and
    join_params holds a (phase, DM) pair per archive: the first archive's
    phase 0 and fixed, every other phase started at
    -fit_phase_shift(prof, first prof).phase, every DM 0, all free.  A bunch
    without prof gets the mean of its ok rows.  joinfile (the output of
    write_join_parameters, either format) overrides the start values."""

    def __init__(self, datafile=None, joinfile=None, quiet=False,
                 **load_data_kwargs):
        self.init_params = []
        self.njoin = 0
        self.join_params = []
        self.join_ichans = []
        self.all_join_params = []
        bunches = None
        if isinstance(datafile, (list, tuple)):
            bunches = list(datafile)
            names = [str(b.get("filename", "DataBunch%d" % i))
                     for i, b in enumerate(bunches)]
            self.metafile = self.datafile = "DataBunches"
        elif not isinstance(datafile, dict) and \
                file_is_type(datafile, "ASCII"):
            with open(datafile) as fh:
                names = [line.strip() for line in fh if line.strip()]
            for name in names:
                # PSRCHIVE reads the other formats in the reference
                if not (os.path.isfile(name) and file_is_type(name, "FITS")):
                    raise NotImplementedError(
                        _OUTSIDE % ("DataPortrait(metafile): '%s' is not a "
                                    "PSRFITS file, which" % name))
            bunches = [load_data(name, dedisperse=True, dededisperse=False,
                                 tscrunch=True, pscrunch=True, fscrunch=False,
                                 quiet=quiet, **load_data_kwargs)
                       for name in names]
            self.metafile = self.datafile = datafile
        if bunches is not None:
            self.joinfile = joinfile
            self._join_archives(bunches, names)
            return
        if joinfile is not None:
            raise NotImplementedError(_OUTSIDE % "DataPortrait(joinfile=...) "
                                      "with a single archive")
        self.joinfile = None
        if isinstance(datafile, dict):
            self.datafile = datafile.get("filename", "DataBunch")
            self.data = datafile
        else:
            self.datafile = datafile
            self.data = load_data(datafile, dedisperse=True,
                                  dededisperse=False, tscrunch=True,
                                  pscrunch=True, fscrunch=False,
                                  quiet=quiet, **load_data_kwargs)
        self.datafiles = [self.datafile]
        self.__dict__.update(**self.data)
        if getattr(self, "source", None) is None:
            self.source = "noname"
        self.freqs = np.asarray(self.freqs, dtype=float)
        self.nchan, self.nbin = np.asarray(self.subints[0, 0]).shape
        ok = np.asarray(self.ok_ichans[0], dtype=int)
        self.port = np.asarray(self.masks[0, 0]) * \
            np.asarray(self.subints[0, 0], dtype=float)
        self.portx = self.port[ok]
        self.freqsxs = [self.freqs[0, ok]]
        self.noise_stdsxs = np.asarray(self.noise_stds)[0, 0, ok]
        self.SNRsxs = np.asarray(self.SNRs)[0, 0, ok]
        self.nchanx = len(ok)
        if getattr(self, "weights", None) is None:
            self.weights = np.zeros((1, self.nchan))
            self.weights[0, ok] = 1.0

    def _join_archives(self, bunches, names):
        """The metafile branch of pplib.py:179-326 on loaded archives."""
        if not bunches:
            raise ValueError("no archive to join")
        self.datafiles = list(names)
        self.njoin = len(bunches)
        self.join_nchans, self.join_nchanxs = [0], [0]
        join_params, join_fit_flags = [], []
        freqs, freqsxs, masks, port, portx = [], [], [], [], []
        noise, noisex, snrs, snrsx, wts, wtsx = [], [], [], [], [], []
        self.nchans = []
        self.Ps = 0.0
        self.lofreq, self.hifreq = np.inf, 0.0
        refprof = None
        for ia, data in enumerate(bunches):
            sub = np.asarray(data["subints"][0, 0], dtype=float)
            mask = np.asarray(data["masks"][0, 0], dtype=float)
            nchan, nbin = sub.shape
            ok = np.asarray(data["ok_ichans"][0], dtype=int)
            f = np.asarray(data["freqs"], dtype=float)[0]
            prof = data.get("prof", None)
            if prof is None:
                prof = sub[ok].mean(axis=0)
            prof = np.asarray(prof, dtype=float)
            if ia == 0:
                self.nbin = nbin
                self.phases = np.asarray(data["phases"])
                self.source = data.get("source", None) or "noname"
                refprof = prof
                join_params += [0.0, 0.0]
                join_fit_flags += [0, 1]
            else:
                if nbin != self.nbin:
                    raise ValueError("archive '%s' has nbin=%d, the first "
                                     "one %d: joined archives need the same "
                                     "nbin" % (names[ia], nbin, self.nbin))
                phi = -fit_phase_shift(prof, refprof, Ns=self.nbin).phase
                join_params += [phi, 0.0]
                join_fit_flags += [1, 1]
            self.nchans.append(nchan)
            self.join_nchans.append(self.join_nchans[-1] + nchan)
            self.join_nchanxs.append(self.join_nchanxs[-1] + len(ok))
            self.Ps += float(np.mean(data["Ps"]))
            half = abs(float(data["bw"])) / (2 * nchan)
            self.lofreq = min(self.lofreq, f.min() - half)
            self.hifreq = max(self.hifreq, f.max() + half)
            w = data.get("weights", None)
            if w is None:
                w = np.zeros((1, nchan))
                w[0, ok] = 1.0
            w = np.asarray(w, dtype=float)[0]
            ns = np.asarray(data["noise_stds"], dtype=float)[0, 0]
            sn = np.asarray(data["SNRs"], dtype=float)[0, 0]
            freqs.append(f), freqsxs.append(f[ok]), masks.append(mask)
            port.append(sub * mask), portx.append(sub[ok])
            noise.append(ns), noisex.append(ns[ok])
            snrs.append(sn), snrsx.append(sn[ok])
            wts.append(w), wtsx.append(w[ok])
        self.nchan, self.nchanx = self.join_nchans[-1], self.join_nchanxs[-1]
        self.Ps = [self.Ps / self.njoin]
        self.bw = self.hifreq - self.lofreq
        freqs, freqsxs = np.concatenate(freqs), np.concatenate(freqsxs)
        self.nu0 = freqs.mean()
        self.isort, self.isortx = np.argsort(freqs), np.argsort(freqsxs)
        self.join_ichans, self.join_ichanxs = [], []
        for ia in range(self.njoin):
            self.join_ichans.append(np.flatnonzero(
                (self.isort >= self.join_nchans[ia]) &
                (self.isort < self.join_nchans[ia + 1])))
            self.join_ichanxs.append(np.flatnonzero(
                (self.isortx >= self.join_nchanxs[ia]) &
                (self.isortx < self.join_nchanxs[ia + 1])))
        self.masks = np.concatenate(masks)[self.isort][None, None]
        self.port = np.concatenate(port)[self.isort]
        self.portx = np.concatenate(portx)[self.isortx]
        self.flux_prof = self.port.mean(axis=1)
        self.flux_profx = self.portx.mean(axis=1)
        self.noise_stds = np.concatenate(noise)[self.isort][None, None]
        self.noise_stdsxs = np.concatenate(noisex)[self.isortx]
        self.SNRs = np.concatenate(snrs)[self.isort][None, None]
        self.SNRsxs = np.concatenate(snrsx)[self.isortx]
        self.weights = np.concatenate(wts)[self.isort][None]
        self.weightsxs = np.concatenate(wtsx)[self.isortx][None]
        self.ok_ichans = [np.flatnonzero(self.masks[0, 0].mean(axis=1) > 0)]
        self.freqs = freqs[self.isort][None]
        self.freqsxs = [freqsxs[self.isortx]]
        self.join_params = np.array(join_params, dtype=float)
        self.join_fit_flags = np.array(join_fit_flags)
        if self.joinfile:
            self._read_joinfile()
        self.all_join_params = [self.join_ichanxs, self.join_params,
                                self.join_fit_flags]

    def _read_joinfile(self):
        """pplib.py:300-315: the last njoin lines of the join file, either
        format (old: name phi DM; new: name phi err DM err), matched to the
        archives by name.  (The reference parses the DM with np.float, which
        current NumPy no longer has: its reader always prints "Bad join
        file."; plain float here.)"""
        with open(self.joinfile) as fh:
            lines = [line.split() for line in fh.readlines()[-self.njoin:]]
        try:
            vals = []
            for info in lines:
                ijoin = self.datafiles.index(info[0])
                phi = float(info[1])
                DM = float(info[3]) if len(info) > 3 else float(info[2])
                vals.append((ijoin, phi, DM))
        except (ValueError, IndexError):
            print("Bad join file.")
            return
        for ijoin, phi, DM in vals:
            self.join_params[ijoin * 2] = phi
            self.join_params[ijoin * 2 + 1] = DM

    def apply_joinfile(self, nu_ref, undo=False):
        """pplib.py:351-370: rotate every archive's channels of port and
        portx by the negated join parameters at nu_ref (the fitted model's
        reference frequency); undo=True rotates back."""
        sign = (-1) ** int(undo)
        for ii in range(self.njoin):
            phi = -self.join_params[0::2][ii] * sign
            DM = -self.join_params[1::2][ii] * sign
            jic, jicx = self.join_ichans[ii], self.join_ichanxs[ii]
            self.port[jic] = rotate_data(self.port[jic], phi, DM, self.Ps[0],
                                         self.freqs[0, jic], nu_ref)
            self.portx[jicx] = rotate_data(self.portx[jicx], phi, DM,
                                           self.Ps[0],
                                           self.freqsxs[0][jicx], nu_ref)

    def write_join_parameters(self):
        """pplib.py:508-543: append the join parameters and their errors to
        the join file (joinfile, or model_name + '.join'), the reference's
        line format byte for byte.  The values are the NEGATIVES of the
        rotations that align the data (rotate_data)."""
        joinfile = self.joinfile if self.joinfile is not None \
            else self.model_name + ".join"
        lines = ["# archive name" + " " * 32 + "-phase offset & err [rot]" +
                 " " * 2 + "-delta-DM & err [cm**-3 pc]\n"]
        for ifile, datafile in enumerate(self.datafiles):
            lines.append(
                datafile + " " * abs(45 - len(datafile)) +
                "% .10f" % self.join_params[ifile * 2] + " " +
                "%.10f" % self.join_param_errs[::2][ifile] + "  " +
                "% .6f" % self.join_params[ifile * 2 + 1] + " " +
                "%.6f" % self.join_param_errs[1::2][ifile] + "\n")
        with open(joinfile, "a") as jf:
            jf.writelines(lines)

    def normalize_portrait(self, method="rms"):
        """pplib.py:379-404: normalize_portrait(...) on the full and the
        condensed portrait, the noise levels re-measured."""
        if method not in ("mean", "max", "prof", "rms", "abs"):
            print("Unknown method for normalize_portrait(...), '%s'." % method)
            return
        weights = weightsx = None
        if method == "prof":
            w = np.asarray(self.weights, dtype=float)
            weights, weightsx = w[0], w[w > 0]
        self.noise_stds = np.array(self.noise_stds, dtype=float)
        self.unnorm_noise_stds = np.copy(self.noise_stds)
        self.port, self.norm_values = normalize_portrait(
            self.port, method, weights=weights, return_norms=True)
        self.noise_stds[0, 0] = get_noise(self.port, chans=True)
        self.flux_prof = self.port.mean(axis=1)
        self.unnorm_noise_stdsxs = np.copy(self.noise_stdsxs)
        self.portx = normalize_portrait(self.portx, method, weights=weightsx,
                                        return_norms=False)
        self.noise_stdsxs = get_noise(self.portx, chans=True)
        self.flux_profx = self.portx.mean(axis=1)

    def smooth_portrait(self, smart=False, **kwargs):
        """pplib.py:422-446: the full and the condensed portrait through
        wavelet_smooth, or with smart through smart_smooth (at most eight
        levels; search="batched" unless kwargs say otherwise: every
        channel's search in one launch), the noise levels re-measured and
        the flux profiles recomputed.  kwargs go to the smoother."""
        def smooth(port):
            if not smart:
                return wavelet_smooth(port, **kwargs)
            kw = dict(search="batched")
            kw.update(kwargs)
            return smart_smooth(
                port, try_nlevels=min(8, int(np.log2(self.nbin))), **kw)

        self.port = smooth(self.port)
        self.noise_stds = np.array(self.noise_stds, dtype=float)
        self.noise_stds[0, 0] = get_noise(self.port, chans=True)
        self.flux_prof = self.port.mean(axis=1)
        self.portx = smooth(self.portx)
        self.noise_stdsxs = get_noise(self.portx, chans=True)
        self.flux_profx = self.portx.mean(axis=1)

    def unnormalize_portrait(self):
        """pplib.py:406-420: undo normalize_portrait."""
        if not hasattr(self, "unnorm_noise_stds"):
            return
        ok = np.asarray(self.ok_ichans[0], dtype=int)
        self.port = (self.norm_values * self.port.T).T
        self.noise_stds = np.copy(self.unnorm_noise_stds)
        del self.unnorm_noise_stds
        self.flux_prof = self.port.mean(axis=1)
        self.portx = (self.norm_values[ok] * self.portx.T).T
        self.noise_stdsxs = np.copy(self.unnorm_noise_stdsxs)
        del self.unnorm_noise_stdsxs
        self.flux_profx = self.portx.mean(axis=1)
        self.norm_values = np.ones(len(self.port))
