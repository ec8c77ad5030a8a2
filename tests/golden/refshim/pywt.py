"""A minimal NumPy stand-in for the three PyWavelets calls the reference's
wavelet_smooth makes (swt, threshold, iswt), for the 'db8' wavelet only.

It is NOT PyWavelets.  It exists so that the reference's own smart_smooth,
find_significant_eigvec and make_spline_model can run in the build container
(make_golden_spline.py), where PyWavelets is not installed.  It is written
from the definition of the periodic stationary transform,

    a_j[i] = sum_k dec_lo[k] a_{j-1}[(i - k 2^(j-1)) mod n]      (a_0 = x)
    d_j[i] = sum_k dec_hi[k] a_{j-1}[(i - k 2^(j-1)) mod n]
    a'_{j-1}[i] = (sum_k dec_lo[k] a'_j[(i + k 2^(j-1)) mod n]
                   + sum_k dec_hi[k] d'_j[(i + k 2^(j-1)) mod n]) / 2

with dec_lo = rec_lo reversed and dec_hi[k] = (-1)^(k+1) rec_lo[k], by direct
index loops over the taps (no FFT), independently of the package's NumPy
evaluator (_swt.py, FFT-based) and of its kernels.  Agreement with the real
PyWavelets is UNVERIFIED: the synthesis above equals PyWavelets' iswt (the
average of the two shifted inverse transforms) for an orthogonal wavelet on
paper only, and PyWavelets' sample shifts and sign conventions are not
reproduced -- they cancel between swt and iswt, so the denoised row does not
depend on them, but individual coefficients may sit at other indices.
"""
import numpy as np

_REC_LO = [
    0.05441584224308161, 0.3128715909144659, 0.6756307362980128,
    0.5853546836548691, -0.015829105256023893, -0.2840155429624281,
    0.00047248457399797254, 0.128747426620186, -0.01736930100202211,
    -0.04408825393106472, 0.013981027917015516, 0.008746094047015655,
    -0.00487035299301066, -0.0003917403729959771, 0.0006754494059985568,
    -0.00011747678400228192]
_NTAP = len(_REC_LO)
_DEC_LO = [_REC_LO[_NTAP - 1 - k] for k in range(_NTAP)]
_DEC_HI = [(-1.0 if k % 2 == 0 else 1.0) * _REC_LO[k] for k in range(_NTAP)]


def _only_db8(wavelet):
    if wavelet != "db8":
        raise NotImplementedError("the pywt stand-in knows 'db8' only")


def _taps(row, filt, step, sign):
    """sum_k filt[k] row[(i + sign k step) mod n] for every i."""
    n = len(row)
    idx = np.arange(n)
    out = np.zeros(n)
    for k in range(_NTAP):
        out += filt[k] * row[(idx + sign * k * step) % n]
    return out


def swt(data, wavelet, level=None, start_level=0, axis=-1):
    """[(cA_L, cD_L), ..., (cA_1, cD_1)], coarsest first, as pywt.swt."""
    _only_db8(wavelet)
    if start_level != 0 or axis != -1:
        raise NotImplementedError("stand-in: start_level=0, axis=-1 only")
    a = np.asarray(data, dtype=np.float64)
    if a.ndim != 1 or len(a) % 2:
        raise ValueError("stand-in: one row of even length")
    out = []
    for j in range(1, level + 1):
        step = 2 ** (j - 1)
        d = _taps(a, _DEC_HI, step, -1)
        a = _taps(a, _DEC_LO, step, -1)
        out.append((a, d))
    return out[::-1]


def iswt(coeffs, wavelet):
    """The row from [(cA_L, cD_L), ..., (cA_1, cD_1)]; only cA_L and the
    cD_j enter, as in pywt.iswt."""
    _only_db8(wavelet)
    a = np.asarray(coeffs[0][0], dtype=np.float64)
    nlevel = len(coeffs)
    for m, (_, d) in enumerate(coeffs):
        step = 2 ** (nlevel - m - 1)
        a = 0.5 * (_taps(a, _DEC_LO, step, +1) +
                   _taps(np.asarray(d, dtype=np.float64), _DEC_HI, step, +1))
    return a


def threshold(data, value, mode="soft", substitute=0.0):
    """pywt.threshold for mode 'hard' (substitute where |x| < value) and
    'soft' (x (1 - value / |x|) where that is positive, else substitute)."""
    data = np.asarray(data, dtype=np.float64)
    mag = np.abs(data)
    if mode == "hard":
        return np.where(mag < value, substitute, data)
    if mode == "soft":
        with np.errstate(divide="ignore", invalid="ignore"):
            shrunk = data * (1.0 - value / mag)
        return np.where(mag <= value, substitute, shrunk)
    raise NotImplementedError("stand-in: 'hard' and 'soft' only")
