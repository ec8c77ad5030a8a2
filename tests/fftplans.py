"""Transform lengths that put every FFT plan class in front of the row
kernels and the fit (TEST INFRASTRUCTURE; no pytest hooks).

Every routine rests on a block or wave FFT whose stage sequence is chosen at
run time from the factorisation of the transform length N (nbin / 2 for even
nbin, nbin for odd): fft_radices / lds_fft_mixed in ppf_device.hpp and their
wave-per-row restatement in k_xspec_wm / k_xspec_wo (ppf_xspec.hip).  The
host restatements below say which stages and which kernel instantiation a
length takes; ROW_LENGTHS and FIT_CASES are chosen so that every one of them
runs.  tests/test_fftplans_inputs.py asserts that coverage and the
well-posedness of the fits on the host, tests/test_gpu_fftplans.py compares
the device with NumPy and the oracle."""
import functools

import numpy as np

import ragged as R

K_BLOCK = 256            # ppf_device.hpp kBlock: threads per workgroup
MAX_FFT_N = 4096         # ppf_device.hpp kMaxFftN
WM_MAX_N = 1024          # ppf_xspec.hip kWmMaxN: complex points per wave
GENERIC = "g"            # a prime factor above 7: mr_stage_g


# ------------------------------------------------------ host restatements ---
def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def rfft_len(nbin):
    """ppf_device.hpp rfft_len: complex points of a real row's transform."""
    return nbin if nbin & 1 else nbin >> 1


def fft_radices(N):
    """ppf_device.hpp fft_radices: one leading 2 when the power of two in N
    is odd, then 4s, then the odd prime factors ascending."""
    if N < 2:
        return []
    n, p2, r = N, 0, []
    while n & 1 == 0:
        n >>= 1
        p2 += 1
    if p2 & 1:
        r.append(2)
    r += [4] * (p2 // 2)
    f = 3
    while f * f <= n:
        while n % f == 0:
            n //= f
            r.append(f)
        f += 2
    if n > 1:
        r.append(n)
    return r


def stages(N, wave=False):
    """[(radix class, span L)] of lds_fft_mixed's switch (ppf_device.hpp):
    butterflies for 2, 3, 4, 5 and 7, mr_stage_g (GENERIC) above.  wave: the
    stage switch of k_xspec_wm / k_xspec_wo (ppf_xspec.hip), where 7 goes to
    wmr_stage_g as well.  A power-of-two N runs on lds_fft / the wave FFT
    and has no mixed-radix stage: []."""
    if is_pow2(N):
        return []
    out, L = [], 1
    for r in fft_radices(N):
        hard = (2, 3, 4, 5) if wave else (2, 3, 4, 5, 7)
        out.append((r if r in hard else GENERIC, L))
        L *= r
    assert L == N
    return out


def nbin_supported(nbin):
    """ppf_api.cpp nbin_supported (with fft_len_supported): even 32..8192,
    odd 33..4095."""
    return 32 <= nbin <= 8192 and 2 <= rfft_len(nbin) <= MAX_FFT_N


def xspec_wm_supported(nbin):
    """ppf_xspec.hip xspec_wm_supported: the wave-per-row spectrum pass."""
    if nbin & 1:
        return 33 <= nbin < WM_MAX_N
    N = nbin // 2
    return not is_pow2(N) and N <= WM_MAX_N and 2 <= N <= MAX_FFT_N


def xspec_path(nbin, nchan):
    """The spectrum pass of a fit at nbin whose transform length is not a
    power of two: launch_xspec's log2N == 0 arm (ppf_kernels.hip; cb =
    min(nchan, 32) of fit_layout, ppf_api.cpp) and the 512 / 1024 split of
    launch_xspec_wm (ppf_xspec.hip): "wm512", "wm1024" (even nbin,
    k_xspec_wm), "wo512", "wo1024" (odd nbin, k_xspec_wo), k_xspec_any
    otherwise ("any-even", "any-odd")."""
    assert nbin_supported(nbin) and (nbin & 1 or not is_pow2(nbin // 2))
    cb = min(nchan, 32)
    if xspec_wm_supported(nbin) and cb <= 64:
        return "%s%d" % ("wo" if nbin & 1 else "wm",
                         512 if rfft_len(nbin) <= 512 else 1024)
    return "any-odd" if nbin & 1 else "any-even"


def dsum_kernel(nbin, nchan):
    """launch_dsum (ppf_kernels.hip), the guess pass of a fit that does not
    carry the guess in its spectrum pass (cbd = min(nchan, 128) of
    fit_layout): k_dsum_w at power-of-two nbin 256..2048, k_dsum_wn<1024 |
    2048> at the other nbin <= 2048, k_dsum<jb> above."""
    cbd = min(nchan, 128)
    if 256 <= nbin <= 2048 and is_pow2(nbin):
        return "k_dsum_w"
    if nbin <= 2048 and cbd <= 128:
        return "k_dsum_wn<%d>" % (1024 if nbin <= 1024 else 2048)
    jb = 8 if nbin >= 2048 else (nbin + K_BLOCK - 1) // K_BLOCK
    return "k_dsum<%d>" % (8 if jb >= 8 else 4 if jb >= 4 else 2 if jb >= 2
                           else 1)


def kmax(nbin):
    """kmax_pow2(nbin / 2 + (nbin & 1)) (ppf_launch.hpp): the per-thread
    harmonic slots of the k_rotate, k_resid_chi2, k_inst_resp and
    k_gauss_port instantiation, the smallest power of two that holds
    ceil(harmonics / kBlock)."""
    q = (nbin // 2 + (nbin & 1) + K_BLOCK - 1) // K_BLOCK
    k = 1
    while k < q:
        k <<= 1
    return k


# ------------------------------------------------------------ row lengths ---
# even nbin (N = nbin / 2) ...
ROW_EVEN = (
    34,      # 17: one generic stage, the smallest
    36,      # 2 3^2: radix 2 first, radix 3 at L = 2, 6
    50,      # 5^2: radix 5 first and at L = 5
    98,      # 7^2: radix 7 first and at L = 7
    100,     # 2 5^2
    242,     # 11^2: generic at L = 11, the previous generic radix
    286,     # 11 13: two generic stages in a row
    360,     # 4 3^2 5: radix 4 first
    770,     # 5 7 11: KMAX 2 with N not a power of two (385 harmonics)
    1026,    # 3^3 19: radix 3 first; 513 points
    1200,    # 2 4 3 5^2: radix 4 after the leading 2
    1372,    # 2 7^3
    2046,    # 3 11 31: 1023 points, the last of the wave kernels
    2050,    # 5^2 41: 1025 points, the first of k_xspec_any
    6144,    # 4^5 3
    8188,    # 2 23 89
    8190,    # 4095 = 3^2 5 7 13: the longest
)
# ... odd nbin (N = nbin) ...
ROW_ODD = (33, 35, 243, 513, 625, 1025, 2187, 2401, 3125)
# ... and the power-of-two controls (lds_fft)
ROW_POW2 = (64, 8192)
ROW_LENGTHS = ROW_EVEN + ROW_ODD + ROW_POW2


def rows(nbin, n=3):
    """n rows of unit-variance normals seeded by nbin (float64)."""
    return np.random.default_rng(nbin).normal(size=(n, nbin))


def row_dtype(nbin):
    """f32 and f64 input alternate along ROW_LENGTHS."""
    return np.float32 if ROW_LENGTHS.index(nbin) % 2 == 0 else np.float64


# -------------------------------------------------------------- fit cases ---
# ragged._SC (tau = 3e-3 rot at 1500 MHz) at noise 0.2 instead of 0.5 for the
# nine-channel scattering cases.  Mask 3 keeps channels 0 and 8: phase, DM,
# tau and alpha from two channels.  At 0.5 the oracle, restarted 1e-2 sigma
# from its solution of that sub-int, ends 1500 (1200 bins) and 750 (243
# bins) sigma away from it; at 242 bins it returns, but its alpha error is
# 92 -- the inverse of a near-singular matrix, which the device reproduced
# to 2.5e-4 with the parameters themselves within 2e-6 sigma.  At 0.2 the
# alpha error is below 3 and the restart returns to within 5e-7 sigma
# (tests/test_fftplans_inputs.py asserts both).  The seven-channel cases
# (channels 0 and 6, longer rows) are sharp at 0.5.
_SC2 = dict(R._SC, noise=0.2)
ALPHA_ERR_MAX = 5.0      # a quarter of alpha's range in the reference, +-10


def _fit_cases():
    table = (
        # (path, nbin, flags, guess, extra)
        ("wm512", 100, R.PD, False, {}),
        ("wm512", 98, R.PD, False, {}),
        ("wm512", 286, R.PD, True, {}),
        ("wm512", 242, R.PDTA, False, _SC2),
        ("wm1024", 1026, R.PD, False, {}),
        ("wm1024", 1200, R.PDTA, False, _SC2),
        ("wm1024", 1372, R.PD, True, {}),
        ("wm1024", 2046, R.PD, False, {}),
        ("wo512", 33, R.PD, False, {}),
        ("wo512", 35, R.PD, True, {}),
        ("wo512", 243, R.PDTA, False, _SC2),
        ("wo512", 511, R.PD, False, {}),
        ("wo1024", 513, R.PD, False, {}),
        ("any-even", 2050, R.PD, True, {}),
        ("any-even", 8190, R.PD, True, {}),
        ("any-even", 8188, R.PDTA, False, R._SC),
        ("any-odd", 1025, R.PD, True, {}),
        ("any-odd", 2401, R.PD, False, {}),
        ("any-odd", 4095, R.PDTA, False, R._SC),
    )
    out = []
    for i, (path, nbin, flags, guess, kw) in enumerate(table):
        # 9 channels: three rounds of four rows with a partial last one in
        # k_xspec_wm, an unpaired last row in k_xspec_wo; 7 at the two
        # longest even and the two longest odd lengths
        nchan = 7 if nbin in (8190, 8188, 2401, 4095) else 9
        out.append(R._case(path, nbin, nchan, flags, template="cut",
                           guess=guess, dtype=("f32", "f64")[i % 2], **kw))
    return tuple(out)


FIT_CASES = _fit_cases()
FIT_NAMES = [c["name"] for c in FIT_CASES]
# each sub-int alone must equal the batch bitwise: one wave case, one block
SINGLE_EQUALS_BATCH = ("wm1024-9x1372-pd-cut-f32", "any-even-9x2050-pd-cut-f64")


def fit_case(name):
    return FIT_CASES[FIT_NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def fit_path(name):
    c = fit_case(name)
    return xspec_path(c["nbin"], c["nchan"])
