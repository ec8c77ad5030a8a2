"""The stationary 'db8' wavelet transform behind pplib.wavelet_smooth and
smart_smooth, and its NumPy evaluator.

PyWavelets is not a dependency: the transform is written from its
definition.  For a periodic row x of even length n (a_0 = x)

    a_j = a_{j-1} (*) up_{j-1}(dec_lo)        d_j = a_{j-1} (*) up_{j-1}(dec_hi)

with (*) circular convolution and up_j the filter with 2^j - 1 zeros between
its taps (longer than the row at small n: it wraps).  dec_lo is rec_lo
reversed, dec_hi[k] = (-1)^(k+1) rec_lo[k].  Synthesis is half the adjoint,

    a'_{j-1} = (a'_j (x) up_{j-1}(dec_lo) + d'_j (x) up_{j-1}(dec_hi)) / 2

with (x) circular correlation; for an orthogonal wavelet this is the average
of the two shifted inverse transforms PyWavelets' iswt takes.  That this
equals PyWavelets' swt / iswt bit for bit or even to rounding has NOT been
checked against PyWavelets itself (it is absent here); sample shifts and the
sign of dec_hi cancel between analysis and synthesis.

An evaluator is what pplib.wavelet_smooth / smart_smooth /
find_significant_eigvec compute with:

    ev.noise(rows)                    -> get_noise_PS per row [nrow]
    h = ev.analyse(profs, nlevel)     -> a handle for score(); h.medians
                                         [nprof, nlevel], h.noise [nprof]
    ev.score(h, cases, facts, smooth) -> out [ncase, 3] = (signal, noise,
                                         red_chi2) and the smoothed rows
                                         [ncase, n] (None unless smooth)
    ev.search(h, soft, rchi2_tol, grid)
                                      -> fact_min, fun_min, nfev, each
                                         [nprof, nlevel]: per (profile,
                                         level) what scipy.optimize.brute
                                         over that grid of factors returns
                                         with its fmin finish (x, fval) and
                                         the calls the finish made (fmin_1d)

cases is a sequence of (profile, level, soft).  NumpyEvaluator (this file,
FFT-based convolutions, no GPU) and engine.SwtEvaluator (the device kernels
of ppf_swt.hip) are interchangeable; the device one is the default.
"""
import numpy as np

# PyWavelets' table for 'db8' (rec_lo).  It sums to sqrt(2), is orthonormal
# under even shifts to 2.3e-12 and has eight vanishing moments.
REC_LO = np.array([
    0.05441584224308161, 0.3128715909144659, 0.6756307362980128,
    0.5853546836548691, -0.015829105256023893, -0.2840155429624281,
    0.00047248457399797254, 0.128747426620186, -0.01736930100202211,
    -0.04408825393106472, 0.013981027917015516, 0.008746094047015655,
    -0.00487035299301066, -0.0003917403729959771, 0.0006754494059985568,
    -0.00011747678400228192])
DEC_LO = REC_LO[::-1].copy()
DEC_HI = REC_LO * (-1.0) ** (np.arange(16) + 1)

NBIN_MIN, NBIN_MAX = 32, 8192


def max_level(nbin):
    """The deepest supported decomposition of a row of nbin samples: log2
    for a power of two, 1 for any other even length in [32, 8192], 0 (no
    transform) otherwise."""
    nbin = int(nbin)
    if nbin % 2 or nbin < NBIN_MIN or nbin > NBIN_MAX:
        return 0
    if nbin & (nbin - 1):
        return 1
    return nbin.bit_length() - 1


def check_shape(nbin, nlevel):
    """NotImplementedError for what neither evaluator transforms."""
    top = max_level(nbin)
    if top == 0:
        raise NotImplementedError(
            "wavelet smoothing needs an even number of bins in [%d, %d], got "
            "%d" % (NBIN_MIN, NBIN_MAX, nbin))
    if nlevel < 1 or nlevel > top:
        raise NotImplementedError(
            "nlevel = %d with %d bins: 1 <= nlevel <= log2(nbin) for a power "
            "of two, nlevel = 1 for any other length" % (nlevel, nbin))


def _filter_ft(h, step, n):
    """rfft of the filter h upsampled by step and wrapped onto n samples."""
    up = np.zeros(n)
    np.add.at(up, (np.arange(len(h)) * step) % n, h)
    return np.fft.rfft(up)


def swt(x, nlevel):
    """[(a_1, d_1), ..., (a_L, d_L)] of the row x."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    out = []
    A = np.fft.rfft(x)
    for j in range(1, nlevel + 1):
        step = 1 << (j - 1)
        D = A * _filter_ft(DEC_HI, step, n)
        A = A * _filter_ft(DEC_LO, step, n)
        out.append((np.fft.irfft(A, n), np.fft.irfft(D, n)))
    return out


def iswt(a_top, details):
    """The row from a_L and [d_1, ..., d_L] (half-adjoint synthesis)."""
    n = len(a_top)
    A = np.fft.rfft(np.asarray(a_top, dtype=np.float64))
    for j in range(len(details), 0, -1):
        step = 1 << (j - 1)
        D = np.fft.rfft(np.asarray(details[j - 1], dtype=np.float64))
        A = 0.5 * (A * np.conj(_filter_ft(DEC_LO, step, n)) +
                   D * np.conj(_filter_ft(DEC_HI, step, n)))
    return np.fft.irfft(A, n)


def threshold(c, lam, soft):
    """hard: 0 where |c| < lam; soft: c * max(1 - lam / |c|, 0)."""
    c = np.asarray(c, dtype=np.float64)
    m = np.abs(c)
    if soft:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(m <= lam, 0.0, c * (1.0 - lam / m))
    return np.where(m < lam, 0.0, c)


def noise_PS(row, frac=4):
    """pplib.get_noise_PS of one row: the root mean of the top 1 / frac of
    the power spectrum."""
    row = np.asarray(row, dtype=np.float64).ravel()
    F = np.fft.rfft(row)
    pows = np.real(F * np.conj(F)) / len(row)
    kc = int((1 - frac ** -1) * len(pows))
    return np.sqrt(np.mean(pows[kc:]))


def lam_of(fact, median, nbin):
    """The threshold of wavelet_smooth (pplib.py:1726)."""
    return fact * (median / 0.6745) * np.sqrt(2 * np.log(nbin))


FMIN_MAXFUN = 200
FMIN_TOL = 1e-4


def fmin_1d(func, x0):
    """scipy.optimize.fmin(func, x0, full_output=True, disp=False) for a
    scalar x0, (x, fval, calls): _minimize_neldermead in one dimension,
    where the simplex is two points, (s0, f0) the better one (xatol = fatol
    = 1e-4, at most 200 calls; the iteration cap of 200 cannot bind first,
    every iteration makes a call).  The products 3 * s0, 1.5 * s0, 1.05 * x0
    round before the subtraction, as NumPy's array arithmetic does there.
    A call that would be number 201 is not made and the step it belongs to
    is abandoned with what it had already assigned (_MaxFuncCallError).  The
    comparisons are IEEE ones; k_swt_search (ppf_swt.hip) is this function
    on the device.  An objective returning NaN is outside what this
    reproduces (scipy sorts a NaN last)."""
    x0 = float(x0)
    calls = [0]

    class _Cap(Exception):
        pass

    def f(x):
        if calls[0] >= FMIN_MAXFUN:
            raise _Cap()
        calls[0] += 1
        return float(func(x))

    s0, s1 = x0, ((1 + 0.05) * x0 if x0 != 0 else 0.00025)
    f0, f1 = f(s0), f(s1)
    if f1 < f0:
        s0, s1, f0, f1 = s1, s0, f1, f0
    while calls[0] < FMIN_MAXFUN:
        if abs(s1 - s0) <= FMIN_TOL and abs(f0 - f1) <= FMIN_TOL:
            break
        try:
            xr = 2.0 * s0 - 1.0 * s1
            fxr = f(xr)
            shrink = False
            if fxr < f0:
                xe = 3.0 * s0 - 2.0 * s1
                fxe = f(xe)
                s1, f1 = (xe, fxe) if fxe < fxr else (xr, fxr)
            elif fxr < f1:
                xc = 1.5 * s0 - 0.5 * s1
                fxc = f(xc)
                if fxc <= fxr:
                    s1, f1 = xc, fxc
                else:
                    shrink = True
            else:
                xcc = 0.5 * s0 + 0.5 * s1
                fxcc = f(xcc)
                if fxcc < f1:
                    s1, f1 = xcc, fxcc
                else:
                    shrink = True
            if shrink:
                s1 = s0 + 0.5 * (s1 - s0)
                f1 = f(s1)
        except _Cap:
            pass
        if f1 < f0:
            s0, s1, f0, f1 = s1, s0, f1, f0
    return s0, (f1 if f1 < f0 else f0), calls[0]


def wavelet_snr(score, rchi2_tol):
    """The figure of merit of pplib.fit_wavelet_smooth_function from one
    (signal, noise, red_chi2) triple: minus the pseudo-S/N, 0 where the
    reduced chi^2 is further than rchi2_tol from 1."""
    signal, noise, red_chi2 = score
    if signal:
        snr = signal / noise if noise else np.inf
    else:
        snr = 0.0
    if abs(red_chi2 - 1.0) > rchi2_tol:
        snr = 0.0
    return -snr


def grid_cases(nprof, nlevel, soft, grid):
    """The case list and factors of the grid table of search(): (profile,
    level, soft) x grid, the grid fastest."""
    cases = [(ip, lev, soft) for ip in range(nprof)
             for lev in range(1, nlevel + 1) for _ in range(len(grid))]
    return cases, np.tile(np.asarray(grid, dtype=np.float64), nprof * nlevel)


class _Handle(object):
    pass


class NumpyEvaluator(object):
    """The evaluator on NumPy (float64, FFT-based circular convolutions)."""

    def noise(self, rows):
        return np.array([noise_PS(r) for r in np.atleast_2d(rows)])

    def analyse(self, profs, nlevel, max_ncase=0):
        profs = np.atleast_2d(np.asarray(profs, dtype=np.float64))
        check_shape(profs.shape[1], nlevel)
        h = _Handle()
        h.profs, h.nlevel = profs, nlevel
        h.coefs = [swt(p, nlevel) for p in profs]
        h.medians = np.array([[np.median(np.abs(np.concatenate(ad)))
                               for ad in c] for c in h.coefs])
        h.noise = self.noise(profs)
        return h

    def score(self, h, cases, facts, smooth=False):
        n = h.profs.shape[1]
        out = np.zeros((len(cases), 3))
        rows = np.zeros((len(cases), n)) if smooth else None
        for ic, ((ip, lev, soft), fact) in enumerate(zip(cases, facts)):
            if not (0 <= ip < len(h.profs) and 1 <= lev <= h.nlevel):
                raise ValueError("case %d: profile %d / level %d out of range"
                                 % (ic, ip, lev))
            c = h.coefs[ip]
            lam = lam_of(float(fact), h.medians[ip, lev - 1], n)
            s = iswt(threshold(c[lev - 1][0], lam, soft),
                     [threshold(c[j][1], lam, soft) for j in range(lev)])
            F = np.fft.rfft(s)
            out[ic, 0] = np.sum(np.abs(F[1:]) ** 2)
            out[ic, 1] = noise_PS(s) * np.sqrt(n / 2.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                out[ic, 2] = np.sum(((h.profs[ip] - s) / h.noise[ip]) ** 2) / n
            if smooth:
                rows[ic] = s
        return out, rows

    def search(self, h, soft, rchi2_tol, grid):
        grid = np.asarray(grid, dtype=np.float64)
        nprof, nlevel = len(h.profs), h.nlevel
        table = self.score(h, *grid_cases(nprof, nlevel, soft, grid))[0]
        table = table.reshape(nprof, nlevel, len(grid), 3)
        fact_min = np.zeros((nprof, nlevel))
        fun_min = np.zeros((nprof, nlevel))
        nfev = np.zeros((nprof, nlevel), dtype=np.int32)
        for ip in range(nprof):
            for il in range(nlevel):
                J = np.array([wavelet_snr(t, rchi2_tol)
                              for t in table[ip, il]])

                def func(x, ip=ip, lev=il + 1):
                    return wavelet_snr(
                        self.score(h, [(ip, lev, soft)], [x])[0][0], rchi2_tol)

                fact_min[ip, il], fun_min[ip, il], nfev[ip, il] = \
                    fmin_1d(func, grid[np.argmin(J)])
        return fact_min, fun_min, nfev


def default_evaluator():
    """The device evaluator (ppf_swt_analyse_batch / ppf_swt_score_batch)."""
    from . import engine
    return engine.SwtEvaluator()
