"""Host checks of the FFT plan sweep (tests/fftplans.py): the lengths reach
every stage class of the mixed-radix transforms and every dispatch class of
the spectrum pass, asserted from host restatements of the stage selection
and the launchers; the fits are well posed, so that a device deviation in
tests/test_gpu_fftplans.py is the device's; and the restated length rules
agree with the library where it answers without a device.  No GPU."""
import ctypes

import numpy as np
import pytest

import fftplans as F
import ragged as R
from test_ragged_inputs import _well_posed

G_ = F.GENERIC


# ----------------------------------------------------------- restatements ---
def test_fft_radices_restates_the_device_order():
    """One leading 2 when the power of two is odd, 4s, odd primes
    ascending; the lengths the suite already pins, by their documented
    factorisations."""
    assert F.fft_radices(500) == [4, 5, 5, 5]
    assert F.fft_radices(768) == [4, 4, 4, 4, 3]
    assert F.fft_radices(511) == [7, 73]
    assert F.fft_radices(501) == [3, 167]
    assert F.fft_radices(4095) == [3, 3, 5, 7, 13]
    assert F.fft_radices(600) == [2, 4, 3, 5, 5]
    assert F.fft_radices(2048) == [2] + [4] * 5
    assert F.fft_radices(4093) == [4093]
    assert F.fft_radices(1) == []
    for N in range(2, 4097):
        r = F.fft_radices(N)
        assert int(np.prod(r)) == N
        assert r.count(2) <= 1 and (2 not in r or r[0] == 2)
        odd = [x for x in r if x & 1]
        assert odd == sorted(odd) and r[len(r) - len(odd):] == odd
        for p in odd:
            assert all(p % q for q in range(3, int(p ** 0.5) + 1, 2)), (N, p)
    assert F.stages(50) == [(2, 1), (5, 2), (5, 10)]
    assert F.stages(49) == [(7, 1), (7, 7)]
    assert F.stages(49, wave=True) == [(G_, 1), (G_, 7)]
    assert F.stages(143) == [(G_, 1), (G_, 11)]
    assert F.stages(1024) == []


def test_dispatch_restatements():
    assert [F.kmax(n) for n in (32, 512, 514, 1024, 1026, 2048, 2050, 4096,
                                4098, 8192, 33, 511, 513, 1023, 1025, 2047,
                                2049, 4095)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 1, 1, 2, 2, 4, 4, 8, 8]
    assert [F.nbin_supported(n) for n in (30, 31, 32, 33, 4095, 4097, 8192,
                                          8193, 8194)] == \
        [False, False, True, True, True, False, True, False, False]
    for nbin, want in ((34, "wm512"), (1022, "wm512"), (1026, "wm1024"),
                       (2046, "wm1024"), (2050, "any-even"),
                       (8190, "any-even"), (33, "wo512"), (511, "wo512"),
                       (513, "wo1024"), (1023, "wo1024"), (1025, "any-odd"),
                       (4095, "any-odd")):
        assert F.xspec_path(nbin, 9) == want, nbin
    assert not F.xspec_wm_supported(2048) and not F.xspec_wm_supported(31)
    assert F.dsum_kernel(2048, 9) == "k_dsum_w"
    assert F.dsum_kernel(286, 9) == "k_dsum_wn<1024>"
    assert F.dsum_kernel(1024 + 2, 9) == "k_dsum_wn<2048>"
    assert F.dsum_kernel(2047, 300) == "k_dsum_wn<2048>"
    assert F.dsum_kernel(2050, 9) == F.dsum_kernel(8190, 7) == "k_dsum<8>"


# ----------------------------------------------------- row-length coverage ---
def row_gaps(lengths):
    """What of the stage and instantiation classes the lengths leave out."""
    first, later, twog = set(), set(), False
    k_even, k_odd = set(), set()
    for nbin in lengths:
        N = F.rfft_len(nbin)
        st = F.stages(N)
        for (r, L), nxt in zip(st, st[1:] + [None]):
            (first if L == 1 else later).add(r)
            twog |= r == G_ and nxt is not None and nxt[0] == G_
        if st and not nbin & 1:
            k_even.add(F.kmax(nbin))
        if nbin & 1:
            k_odd.add(F.kmax(nbin))
    gaps = ["first stage radix %s" % r
            for r in (2, 3, 4, 5, 7, G_) if r not in first]
    # radix 2 is the leading stage by construction: L = 1 only
    gaps += ["later stage radix %s" % r
             for r in (3, 4, 5, 7, G_) if r not in later]
    assert 2 not in later
    if not twog:
        gaps.append("two generic stages in a row")
    # even nbin apart from odd: k_inst_resp takes even nbin only
    gaps += ["KMAX %d, even nbin, N not a power of two" % k
             for k in (1, 2, 4, 8, 16) if k not in k_even]
    # odd nbin <= 4095 has at most 2048 harmonics: KMAX 16 is out of reach
    gaps += ["KMAX %d, odd nbin" % k for k in (1, 2, 4, 8) if k not in k_odd]
    assert 16 not in k_odd
    return gaps


def test_row_lengths_cover_every_stage_class():
    """Over ROW_LENGTHS every radix class is the first stage (L = 1) and a
    later stage (L > 1) of some plan, two generic stages follow each other,
    and every KMAX instantiation of the block row kernels runs with a
    mixed-radix N and with an odd nbin.  The check has teeth: without the
    only members of a class it reports the class."""
    assert all(F.nbin_supported(n) for n in F.ROW_LENGTHS)
    assert len(set(F.ROW_LENGTHS)) == len(F.ROW_LENGTHS)
    assert row_gaps(F.ROW_LENGTHS) == []
    without = [n for n in F.ROW_LENGTHS if n not in (242, 286, 2046, 8188)]
    assert row_gaps(without) == ["two generic stages in a row"]
    without = [n for n in F.ROW_LENGTHS if n not in (98, 2401)]
    assert row_gaps(without) == ["first stage radix 7"]
    without = [n for n in F.ROW_LENGTHS if n != 770]
    assert row_gaps(without) == [
        "KMAX 2, even nbin, N not a power of two"]
    # the issue's table, none thinned; the power-of-two controls
    for n in (34, 36, 50, 98, 100, 242, 286, 360, 1026, 1200, 1372, 2046,
              2050, 6144, 8188, 8190, 33, 35, 243, 513, 625, 1025, 2187,
              2401, 3125, 64, 8192):
        assert n in F.ROW_LENGTHS, n
    assert all(F.stages(F.rfft_len(n)) == [] for n in F.ROW_POW2)
    # f32 and f64 rows both occur among the even and among the odd lengths
    for group in (F.ROW_EVEN, F.ROW_ODD):
        assert {F.row_dtype(n) for n in group} == {np.float32, np.float64}


# ------------------------------------------------------- fit-case coverage ---
# the issue's table: (path, nbin, nchan, flags, guess); none may go missing
EXPECTED = {
    ("wm512", 100, 9, R.PD, False), ("wm512", 98, 9, R.PD, False),
    ("wm512", 286, 9, R.PD, True), ("wm512", 242, 9, R.PDTA, False),
    ("wm1024", 1026, 9, R.PD, False), ("wm1024", 1200, 9, R.PDTA, False),
    ("wm1024", 1372, 9, R.PD, True), ("wm1024", 2046, 9, R.PD, False),
    ("wo512", 33, 9, R.PD, False), ("wo512", 35, 9, R.PD, True),
    ("wo512", 243, 9, R.PDTA, False), ("wo512", 511, 9, R.PD, False),
    ("wo1024", 513, 9, R.PD, False),
    ("any-even", 2050, 9, R.PD, True), ("any-even", 8190, 7, R.PD, True),
    ("any-even", 8188, 7, R.PDTA, False),
    ("any-odd", 1025, 9, R.PD, True), ("any-odd", 2401, 7, R.PD, False),
    ("any-odd", 4095, 7, R.PDTA, False),
}


def _wave(c):
    return F.fit_path(c["name"])[:2] in ("wm", "wo")


def _wave_stages(c):
    return F.stages(F.rfft_len(c["nbin"]), wave=True) if _wave(c) else []


def _generic_pair(st, radices):
    """Two consecutive generic stages, both of a prime above 7."""
    return any(a[0] == b[0] == G_ and radices[i] > 7 and radices[i + 1] > 7
               for i, (a, b) in enumerate(zip(st, st[1:])))


FIT_CLASSES = {
    "wm<512>": lambda c: F.fit_path(c["name"]) == "wm512",
    "wm<1024>": lambda c: F.fit_path(c["name"]) == "wm1024",
    "wo<512>": lambda c: F.fit_path(c["name"]) == "wo512",
    "wo<1024>": lambda c: F.fit_path(c["name"]) == "wo1024",
    "k_xspec_any, even nbin": lambda c: F.fit_path(c["name"]) == "any-even",
    "k_xspec_any, odd nbin": lambda c: F.fit_path(c["name"]) == "any-odd",
    # the guess passes reachable with these channel counts (k_dsum<1 | 2 | 4>
    # would need a k_dsum channel block above 128, which fit_layout never
    # makes; k_dsum_w is power-of-two nbin)
    "k_dsum_wn<1024>": lambda c: c["guess"] and F.dsum_kernel(
        c["nbin"], c["nchan"]) == "k_dsum_wn<1024>",
    "k_dsum_wn<2048>": lambda c: c["guess"] and F.dsum_kernel(
        c["nbin"], c["nchan"]) == "k_dsum_wn<2048>",
    "k_dsum<8>": lambda c: c["guess"] and F.dsum_kernel(
        c["nbin"], c["nchan"]) == "k_dsum<8>",
    "wave kernels: leading radix 2": lambda c: (2, 1) in _wave_stages(c),
    "wave kernels: radix 7 first": lambda c: _wave(c) and F.fft_radices(
        F.rfft_len(c["nbin"]))[0] == 7,
    "wave kernels: radix 7 at L > 1": lambda c: _wave(c) and 7 in F.fft_radices(
        F.rfft_len(c["nbin"]))[1:],
    "wave kernels: radix 3 at L = 3": lambda c: (3, 3) in _wave_stages(c),
    "wave kernels: two generic stages, primes above 7": lambda c: _generic_pair(
        _wave_stages(c), F.fft_radices(F.rfft_len(c["nbin"]))),
    "wave kernels: a generic stage at L = its own radix": lambda c: any(
        r == G_ and L == p for (r, L), p in zip(
            _wave_stages(c), F.fft_radices(F.rfft_len(c["nbin"])))),
    "block kernel: radix 7 at L > 1": lambda c: not _wave(c) and any(
        r == 7 and L > 1 for r, L in F.stages(F.rfft_len(c["nbin"]))),
    "block kernel: leading radix 2": lambda c: not _wave(c) and (2, 1) in
    F.stages(F.rfft_len(c["nbin"])),
    "scattering fit on k_xspec_any": lambda c: not _wave(c) and c["flags"][3],
    "f32 rows": lambda c: c["dtype"] == "f32",
    "f64 rows": lambda c: c["dtype"] == "f64",
}


def fit_gaps(cases):
    return [k for k, f in FIT_CLASSES.items() if not any(f(c) for c in cases)]


def test_fit_cases_cover_every_dispatch_class():
    """The table of the issue, complete; every spectrum-pass instantiation,
    every reachable guess pass and the stage classes new to the wave kernels
    have a case; the boundary lengths are there (1023 is fitted by
    test_gpu_fullshape.py's pd_128x1023)."""
    got = {(c["family"], c["nbin"], c["nchan"], c["flags"], c["guess"])
           for c in F.FIT_CASES}
    assert got == EXPECTED
    assert len(set(F.FIT_NAMES)) == len(F.FIT_CASES) == len(EXPECTED)
    for c in F.FIT_CASES:
        # the family names the path the restated dispatch gives
        assert F.fit_path(c["name"]) == c["family"], c["name"]
        assert c["template"] == "cut" and c["mom_x"] is None
        assert c["tau"] == (3e-3 if c["flags"][3] else 0.0)
    assert [c["dtype"] for c in F.FIT_CASES] == \
        [("f32", "f64")[i % 2] for i in range(len(F.FIT_CASES))]
    assert fit_gaps(F.FIT_CASES) == []
    nbins = {c["nbin"] for c in F.FIT_CASES}
    assert {33, 511, 513, 1025, 2046, 2050, 8190} <= nbins
    for name in F.SINGLE_EQUALS_BATCH:
        assert name in F.FIT_NAMES
    assert {_wave(F.fit_case(n)) for n in F.SINGLE_EQUALS_BATCH} == \
        {True, False}
    # teeth: without the only members of a class the class is reported
    without = [c for c in F.FIT_CASES if c["nbin"] not in (242, 286, 2046)]
    assert fit_gaps(without) == [
        "wave kernels: two generic stages, primes above 7"]
    without = [c for c in F.FIT_CASES if c["nbin"] != 513]
    assert fit_gaps(without) == ["wo<1024>"]
    without = [c for c in F.FIT_CASES if c["nbin"] not in (286, 35)]
    assert fit_gaps(without) == ["k_dsum_wn<1024>"]


def test_fit_inputs_reach_the_row_tiling():
    """9 (7) channels: a partial last round of four rows in k_xspec_wm, an
    unpaired last row in k_xspec_wo; the four masks of ragged.masks, the
    last with two channels; the cut template cuts wherever nbin leaves it
    room."""
    for c in F.FIT_CASES:
        b = R.inputs(c)
        assert b["data"].shape == (4, c["nchan"], c["nbin"])
        assert c["nchan"] % 4 != 0 and c["nchan"] % 2 == 1
        assert list(b["keep"].sum(axis=1)) == \
            ([9, 6, 5, 2] if c["nchan"] == 9 else [7, 5, 4, 2])
        assert b["scat"] == bool(c["flags"][3])
        if c["nbin"] >= 1000:
            assert R.kc(b["model"]).max() < c["nbin"] // 2 + 1


@pytest.mark.parametrize("name", F.FIT_NAMES)
def test_oracle_fit_is_well_posed(name):
    """test_ragged_inputs.test_oracle_fit_is_well_posed's check (the oracle
    converges with code 2; restarted 1e-2 sigma from its solution it lands
    within 1e-3 sigma of it) on every sub-int of every case.  The two-channel
    sub-int of a four-parameter scattering fit is the fragile one
    (fftplans._SC2): its alpha error must stay below fftplans.ALPHA_ERR_MAX,
    a quarter of the range pptoas.py:511 allows alpha -- beyond that the
    errors are the inverse of a near-singular matrix and not defined to the
    1e-4 they are compared at."""
    c = F.fit_case(name)
    worst = max(_well_posed(c, i) for i in range(4))
    print("FFTPLANS well-posed %s: restart within %.1e sigma" % (name, worst))
    if c["flags"][4]:
        aerr = [R.oracle_fit(c, i)["param_errs"][4] for i in range(4)]
        print("FFTPLANS well-posed %s: alpha errors %s" % (name, aerr))
        assert 0 < max(aerr) < F.ALPHA_ERR_MAX, aerr
    assert c["noise"] == (1.5 if not c["flags"][3] else
                          0.2 if c["nchan"] == 9 else 0.5)


# ------------------------------------------------ the library's own rules ---
def test_length_rules_match_the_library():
    """nbin_supported as the library applies it, asked through the
    workspace queries that need no device: 0 bytes where the length is
    refused (the entry points then return PPF_EUNSUP; with a device:
    tests/test_gpu_fftplans.py)."""
    from pulseportraiture_amd import _lib
    lib = _lib.load()
    d = _lib.FitDesc()
    d.nsub, d.nchan, d.nmodel = 4, 9, 1
    for nbin in F.ROW_LENGTHS + tuple(c["nbin"] for c in F.FIT_CASES):
        d.nbin = nbin
        assert F.nbin_supported(nbin)
        assert lib.ppf_fit_workspace_bytes(ctypes.byref(d)) > 0, nbin
        # the LDS-only entry points: even lengths alone
        for nb in (lib.ppf_gauss_lsq_workspace_bytes(1, 9, nbin, 3),
                   lib.ppf_swt_workspace_bytes(1, nbin, 1, 0)):
            assert (nb > 0) == (nbin % 2 == 0), nbin
    for nbin in (30, 31):
        d.nbin = nbin
        assert not F.nbin_supported(nbin)
        assert lib.ppf_fit_workspace_bytes(ctypes.byref(d)) == 0, nbin
    for nbin in (30, 31, 4097, 8194):
        assert not F.nbin_supported(nbin)
        assert lib.ppf_gauss_lsq_workspace_bytes(1, 9, nbin, 3) == 0, nbin
        assert lib.ppf_swt_workspace_bytes(1, nbin, 1, 0) == 0, nbin
    # a NULL context is refused before the length is looked at
    assert lib.ppf_inst_response_batch(None, 1, 8194, None, None, None, None,
                                       None, None) == _lib.PPF_EINVAL
