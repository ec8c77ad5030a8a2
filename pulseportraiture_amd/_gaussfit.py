"""Levenberg-Marquardt driver of the Gaussian-component fits
(pplib.fit_gaussian_profile / fit_gaussian_portrait).

The reference hands these fits to lmfit, which maps bounded parameters to
unbounded internal variables (the MINUIT transforms) and runs MINPACK's
lmdif on them with a forward-difference Jacobian.  This module follows the
same algorithm (More's 1978 description of lmder/lmpar: diagonal scaling by
the column norms, the trust region |D p| <= delta with the parameter found
to 10 %, the ratio tests and the ftol / xtol stopping rules) but works from
the normal equations, because that is what the device returns: an evaluator

    evaluator(p_ext, free_idx, delta) -> Gram matrix [nfree + 1, nfree + 1]

gives, for the extended parameter vector p_ext (the model parameters with the
scattering index appended; a joined fit has the (phase, DM) pairs of its
archives between the two: [params, join params, index]), the Gram matrix of
the columns
((m(p + delta_j e_j) - m(p)) / delta_j) / errs (j over free_idx) and
(data - m(p)) / errs: J^T J, J^T r and chi^2 in one call, chi^2 alone with
no free index.  engine.GaussLsqEvaluator is the device one
(ppf_gauss_lsq_batch); numpy_evaluator below runs any portrait builder on
the host, so the driver is testable without a GPU.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
SQRT_EPS = np.sqrt(EPS)
WID_MAX = 0.25           # the reference's wid_max (pplib.py:86)


# ---------------------------------------------------------------------------
# lmfit's MINUIT bound transforms (lmfit/parameter.py setup_bounds,
# from_internal): p external, x internal
# ---------------------------------------------------------------------------
def to_external(x, lo, hi):
    """Internal variables -> bounded parameters.  lo / hi: arrays with NaN
    for "no bound".  Lower bound only: p = lo - 1 + sqrt(x^2 + 1); both:
    p = lo + (sin x + 1)(hi - lo) / 2; upper only: p = hi + 1 - sqrt(x^2 + 1);
    none: p = x."""
    x = np.asarray(x, dtype=np.float64)
    p = x.copy()
    has_lo, has_hi = ~np.isnan(lo), ~np.isnan(hi)
    m = has_lo & ~has_hi
    p[m] = lo[m] - 1.0 + np.sqrt(x[m] * x[m] + 1.0)
    m = ~has_lo & has_hi
    p[m] = hi[m] + 1.0 - np.sqrt(x[m] * x[m] + 1.0)
    m = has_lo & has_hi
    p[m] = lo[m] + (np.sin(x[m]) + 1.0) * (hi[m] - lo[m]) / 2.0
    return p


def to_internal(p, lo, hi):
    """The inverse of to_external (values outside the bounds are clipped to
    them first, as lmfit does when a Parameter is set)."""
    p = np.asarray(p, dtype=np.float64)
    x = p.copy()
    has_lo, has_hi = ~np.isnan(lo), ~np.isnan(hi)
    m = has_lo & ~has_hi
    x[m] = np.sqrt(np.maximum(p[m] - lo[m] + 1.0, 1.0) ** 2 - 1.0)
    m = ~has_lo & has_hi
    x[m] = np.sqrt(np.maximum(hi[m] - p[m] + 1.0, 1.0) ** 2 - 1.0)
    m = has_lo & has_hi
    x[m] = np.arcsin(np.clip(2.0 * (p[m] - lo[m]) / (hi[m] - lo[m]) - 1.0,
                             -1.0, 1.0))
    return x


def portrait_bounds(nparam, njoin=0):
    """(lo, hi) of the 2 + 6 ngauss portrait parameters, the 2 njoin join
    parameters (phase, DM per archive; unbounded) and the scattering index
    last, the reference's limits (pplib.py:2041-2101): tau >= 0,
    0 <= wid <= wid_max, amp >= 0, everything else free."""
    lo = np.full(nparam + 2 * njoin + 1, np.nan)
    hi = np.full(nparam + 2 * njoin + 1, np.nan)
    lo[1] = 0.0
    lo[4:nparam:6] = 0.0
    hi[4:nparam:6] = WID_MAX
    lo[6:nparam:6] = 0.0
    return lo, hi


class LMResult:
    """What the fits return as lm_results: message, nfev, success, covar
    (external parameters, the varied ones in order) and residual (the
    weighted residuals, filled by the caller that can build the model)."""

    def __init__(self, **kw):
        self.residual = None
        self.__dict__.update(kw)


def numpy_evaluator(model, data, errs):
    """A host evaluator for levenberg_marquardt: model(p_ext) -> array of
    data's shape.  Forward differences and C @ C.T in the device's column
    order."""
    data = np.asarray(data, dtype=np.float64)
    w = 1.0 / np.asarray(errs, dtype=np.float64)

    def evaluate(p_ext, free_idx, delta):
        p_ext = np.asarray(p_ext, dtype=np.float64)
        m0 = model(p_ext)
        C = np.empty((len(free_idx) + 1, data.size))
        for j, (i, d) in enumerate(zip(free_idx, delta)):
            q = p_ext.copy()
            q[i] = q[i] + d
            C[j] = (((model(q) - m0) / d) * w).ravel()
        C[-1] = ((data - m0) * w).ravel()
        return C @ C.T
    return evaluate


def _lmpar(lam, a, delta):
    """The LM parameter of |p(par)| = delta to 10 % (MINPACK lmpar) in the
    eigenbasis of the scaled normal matrix: lam its eigenvalues, a the
    gradient's components.  Returns (par, step components)."""
    keep = lam > lam.max() * len(lam) * EPS if lam.size and lam.max() > 0 \
        else np.zeros_like(lam, dtype=bool)
    full_rank = bool(keep.all())
    p = np.where(keep, a / np.where(keep, lam, 1.0), 0.0)
    pn = np.linalg.norm(p)
    if pn - delta <= 0.1 * delta:
        return 0.0, p                       # the Gauss-Newton step is inside
    # bounds on par (More 1978, section 5)
    parl = 0.0
    if full_rank:
        parl = (pn - delta) / (np.sum(a * a / lam ** 3) / pn)
    gnorm = np.linalg.norm(a)
    paru = gnorm / delta
    if paru == 0.0:
        paru = np.finfo(float).tiny / min(delta, 0.1)
    par = min(max(gnorm / pn if pn > 0 else paru, parl), paru)
    for _ in range(10):
        if par == 0.0:
            par = max(np.finfo(float).tiny, 0.001 * paru)
        p = a / (lam + par)
        pn = np.linalg.norm(p)
        fp = pn - delta
        if abs(fp) <= 0.1 * delta or (parl == 0.0 and fp <= 0.0):
            break
        parc = (fp / delta) / (np.sum(a * a / (lam + par) ** 3) / (pn * pn))
        if fp > 0.0:
            parl = max(parl, par)
        else:
            paru = min(paru, par)
        par = max(parl, par + parc)
    return par, a / (lam + par)


def levenberg_marquardt(evaluator, p0, vary, lo, hi, ndata, ftol=SQRT_EPS,
                        xtol=SQRT_EPS, maxfev=None, factor=100.0):
    """Minimise chi^2 over the varied entries of the extended parameter
    vector p0 within [lo, hi] (NaN = unbounded).  Returns (p, errs, chi2,
    dof, LMResult): errs are sqrt(diag((J^T J)^-1) chi^2 / dof) in the
    external parameters, from a Jacobian taken at the solution; a fixed
    parameter has error 0.0 (lmfit reports None there).  dof = ndata -
    nvar.  The evaluation cap is 2000 (nvar + 1), lmfit's."""
    p0 = np.array(p0, dtype=np.float64)
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    idx = np.flatnonzero(np.asarray(vary, dtype=bool))
    n = idx.size
    dof = int(ndata) - n
    if maxfev is None:
        maxfev = 2000 * (n + 1)
    vlo, vhi = lo[idx], hi[idx]
    x = to_internal(p0[idx], vlo, vhi)
    p = p0.copy()
    p[idx] = to_external(x, vlo, vhi)
    nfev = [0]

    def chi2_at(xt):
        q = p.copy()
        q[idx] = to_external(xt, vlo, vhi)
        nfev[0] += 1
        with np.errstate(all="ignore"):
            return float(np.asarray(evaluator(q, [], []))[-1, -1])

    def normal_equations(xt, external=False):
        """(J^T J, J^T r, chi2) in the internal variables: a step of
        sqrt(eps) |x| (sqrt(eps) at 0) in each, the external increment it
        causes as the device's delta, and the chain rule delta / h on the
        Gram matrix.  A variable whose step does not move its parameter (a
        bound's stationary point) gets a zero column, as in MINPACK."""
        q = p.copy()
        q[idx] = to_external(xt, vlo, vhi)
        h = SQRT_EPS * np.abs(xt)
        h[h == 0.0] = SQRT_EPS
        d = to_external(xt + h, vlo, vhi) - q[idx]
        live = (d != 0.0) & np.isfinite(d)
        nfev[0] += n
        with np.errstate(all="ignore"):
            G = np.asarray(evaluator(q, idx[live], d[live]), dtype=np.float64)
        nl = int(live.sum())
        s = np.ones(nl) if external else d[live] / h[live]
        A = np.zeros((n, n))
        g = np.zeros(n)
        A[np.ix_(live, live)] = G[:nl, :nl] * np.outer(s, s)
        g[live] = G[:nl, nl] * s
        return A, g, float(G[nl, nl])

    if n == 0:
        chi2 = chi2_at(x)
        return p, np.zeros_like(p), chi2, dof, LMResult(
            message="no parameter varies", nfev=nfev[0], success=True,
            covar=np.zeros((0, 0)))
    A, g, chi2 = normal_equations(x)
    if not np.isfinite(chi2):
        raise ValueError("chi^2 is not finite at the initial parameters")
    fnorm = np.sqrt(chi2)
    diag = np.sqrt(np.diag(A)).copy()
    diag[diag == 0.0] = 1.0
    xnorm = np.linalg.norm(diag * x)
    delta = factor * xnorm if xnorm > 0 else factor
    par, info, message = 0.0, 0, ""
    while info == 0:
        diag = np.maximum(diag, np.sqrt(np.diag(A)))
        As = A / np.outer(diag, diag)
        lam, V = np.linalg.eigh((As + As.T) / 2.0)
        lam = np.maximum(lam, 0.0)
        a = V.T @ (g / diag)
        while True:
            par, pz = _lmpar(lam, a, delta)
            step = (V @ pz) / diag
            pnorm = np.linalg.norm(diag * step)
            xt = x + step
            chi2_t = chi2_at(xt)
            fnorm1 = np.sqrt(chi2_t) if np.isfinite(chi2_t) and chi2_t >= 0 \
                else np.inf
            actred = -1.0
            if 0.1 * fnorm1 < fnorm:
                actred = 1.0 - (fnorm1 / fnorm) ** 2
            t1 = np.sqrt(max(step @ A @ step, 0.0)) / fnorm   # |J p| / |f|
            t2 = np.sqrt(par) * pnorm / fnorm
            prered = t1 * t1 + 2.0 * t2 * t2
            dirder = -(t1 * t1 + t2 * t2)
            ratio = actred / prered if prered != 0.0 else 0.0
            if ratio <= 0.25:
                temp = 0.5 if actred >= 0.0 else \
                    0.5 * dirder / (dirder + 0.5 * actred)
                if 0.1 * fnorm1 >= fnorm or temp < 0.1:
                    temp = 0.1
                delta = temp * min(delta, pnorm / 0.1)
                par /= temp
            elif par == 0.0 or ratio >= 0.75:
                delta = pnorm / 0.5
                par *= 0.5
            if ratio >= 1e-4:           # accept
                x, chi2, fnorm = xt, chi2_t, fnorm1
                xnorm = np.linalg.norm(diag * x)
            if abs(actred) <= ftol and prered <= ftol and 0.5 * ratio <= 1.0:
                info = 1
            if delta <= xtol * xnorm:
                info = 3 if info == 1 else 2
            if info == 0:
                if nfev[0] >= maxfev:
                    info = 5
                elif abs(actred) <= EPS and prered <= EPS and \
                        0.5 * ratio <= 1.0:
                    info = 6
                elif delta <= EPS * xnorm:
                    info = 7
            if info != 0 or ratio >= 1e-4:
                break
        if info == 0:
            A, g, _ = normal_equations(x)
    message = {1: "Fit succeeded (ftol).", 2: "Fit succeeded (xtol).",
               3: "Fit succeeded (ftol and xtol).",
               5: "Too many function calls (max set to %i)." % maxfev,
               6: "ftol is too small.", 7: "xtol is too small."}[info]
    p[idx] = to_external(x, vlo, vhi)
    # errors in the external parameters at the solution
    Ae, _, chi2 = normal_equations(x, external=True)
    errs = np.zeros_like(p)
    try:
        covar = np.linalg.inv(Ae) * (chi2 / dof)
        with np.errstate(invalid="ignore"):
            errs[idx] = np.sqrt(np.diag(covar))
    except np.linalg.LinAlgError:
        covar = None
        errs[idx] = np.nan
    return p, errs, chi2, dof, LMResult(message=message, nfev=nfev[0],
                                        success=info in (1, 2, 3),
                                        covar=covar, info=info)
