"""ppf_align_accum where a wave sums several sub-ints, and ppf_align_phases
against the formula (tests/aligncases.py; the host side of the same inputs:
tests/test_align_inputs.py).

The align shapes of test_gpu_parity.py, test_gpu_degenerate.py,
test_gpu_fftplans.py and test_gpu_fullshape.py give every wave of
k_align_part_w at most one row, so the prefetch of the next live row, the
walk over rows of weight 0 inside a wave's stride and the second trip through
the accumulation never ran there; neither did the 256- and 2048-bin nor any
float64 instantiation.  Every comparison here goes through
engine.align_accum, called twice into the same out / wsum, at the bars of
test_gpu_parity.py::test_align_accum_matches_numpy: out within 1e-12 of the
largest reference value, wsum to 1e-14 (non-negative weights, at most 50
terms: below 50 x 2^-53 = 5.6e-15 in any order)."""
import numpy as np
import pytest

import aligncases as A

pytestmark = pytest.mark.gpu

OUT_ATOL = 1e-12         # x max |ref| (test_gpu_parity.py)
WSUM_RTOL = 1e-14


def _dev(a):
    import torch
    from pulseportraiture_amd import engine
    if isinstance(a, torch.Tensor):
        return a
    a = np.asarray(a)
    dt = {np.dtype(np.float32): torch.float32,
          np.dtype(np.uint8): torch.uint8}.get(a.dtype, torch.float64)
    return engine.to_dev(a, engine.device(None), dt)


def _accum(x, ph, w, times=2):
    """engine.align_accum times over into fresh out / wsum -> NumPy."""
    import torch
    from pulseportraiture_amd import engine
    nsub, nchan, nbin = x.shape
    d, p, wt = _dev(x), _dev(ph), _dev(w)
    out = torch.zeros((nchan, nbin), dtype=torch.float64, device=d.device)
    ws = torch.zeros(nchan, dtype=torch.float64, device=d.device)
    for _ in range(times):
        engine.align_accum(d, p, wt, out, ws)
    got = out.cpu().numpy(), ws.cpu().numpy()
    del d, p, wt, out, ws
    torch.cuda.empty_cache()
    return got


def _check(tag, got, ref, w, atol=None, wsum_rtol=WSUM_RTOL):
    out, ws = got
    top = np.abs(ref).max()
    print("ALIGN groups %s: max |dev| / max |sum| %.1e" %
          (tag, np.abs(out - 2 * ref).max() / top))
    assert np.isfinite(out).all()
    if atol is None:
        np.testing.assert_allclose(out, 2 * ref, rtol=0, atol=OUT_ATOL * top)
    else:
        assert (np.abs(out - 2 * ref) <= atol).all(), \
            (np.abs(out - 2 * ref) / atol).max()
    np.testing.assert_allclose(ws, 2 * w.sum(axis=0), rtol=wsum_rtol)
    dead = ~(w != 0.0).any(axis=0)
    assert not out[dead].any() and not ws[dead].any() and ws[~dead].all()
    return dead


# ---------------------------------------------------------------------------
# a. values at 256 bins, every case, every zero pattern
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,dtype", [(c, "f32") for c in A.CASES] +
                         [((37, 1024), "f64")],
                         ids=lambda v: v if isinstance(v, str)
                         else A.case_id(v))
def test_several_rows_per_wave_match_numpy(case, dtype):
    x, ph, w = A.inputs(case, 256, dtype)
    dead = _check("%s 256 %s" % (A.case_id(case), dtype), _accum(x, ph, w),
                  A.reference(case, 256, dtype), w)
    assert dead.sum() == 1               # the "channel" pattern


# ---------------------------------------------------------------------------
# b. every instantiation of the wave kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nbin", A.WAVE_NBINS)
def test_every_wave_instantiation(nbin, dtype):
    """k_align_part_w<7..10, f32 | f64> on 18 x 1024 (wave 0 of each group
    takes two rows), the first row of a stride and a whole wave of weight 0."""
    case = (18, 1024)
    x, ph, w = A.inputs(case, nbin, dtype, A.REDUCED)
    got = _accum(x, ph, w)
    _check("%s %d %s" % (A.case_id(case), nbin, dtype), got,
           A.reference(case, nbin, dtype, A.REDUCED), w)


# ---------------------------------------------------------------------------
# c. the block-FFT kernel on the same partitions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nbin", A.BLOCK_NBINS)
def test_block_kernel_with_many_rows_per_group(nbin):
    """k_align_part (rows the wave kernel does not take: a power of two
    below its range, an even length with a generic stage, an odd length)
    with 19 and 18 rows per group and every zero pattern."""
    case = (37, 1024)
    x, ph, w = A.inputs(case, nbin, "f32")
    dead = _check("%s %d block" % (A.case_id(case), nbin), _accum(x, ph, w),
                  A.reference(case, nbin, "f32"), w)
    assert dead.sum() == 1


# ---------------------------------------------------------------------------
# d. rows of weight 0 are never read
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,nbin,dtype", [((37, 1024), 256, "f32"),
                                             ((37, 1024), 256, "f64"),
                                             ((18, 1024), 2048, "f32")],
                         ids=["37x1024-256-f32", "37x1024-256-f64",
                              "18x1024-2048-f32"])
def test_nan_rows_of_zero_weight_are_skipped(case, nbin, dtype):
    """NaN in every row of weight 0 (the assertion of test_gpu_degenerate.py
    ::test_align_accum_skips_nan_rows_of_zero_weight, here on the prefetch
    and the in-stride skip): out and wsum are bitwise those of the clean
    run."""
    x, ph, w = A.inputs(case, nbin, dtype)
    clean = _accum(x, ph, w)
    bad = _accum(A.poisoned(x, w), ph, w)
    for b, c in zip(bad, clean):
        assert np.isfinite(b).all()
        np.testing.assert_array_equal(b, c)
    assert clean[0].any()


# ---------------------------------------------------------------------------
# e. fixed summation order
# ---------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal():
    x, ph, w = A.inputs((50, 700), 256, "f32")
    one, two = _accum(x, ph, w), _accum(x, ph, w)
    np.testing.assert_array_equal(one[0], two[0])
    np.testing.assert_array_equal(one[1], two[1])


# ---------------------------------------------------------------------------
# f. align_phases against the formula
# ---------------------------------------------------------------------------
def _phases(c, mask, over=None):
    """engine.align_phases on a phase case -> device tensors."""
    from pulseportraiture_amd import engine
    v = dict(c, **(over or {}))
    return engine.align_phases(
        _dev(A.results_rows(c["phi"], c["DM"], c["nu_ref"])),
        _dev(v["freqs"]), _dev(c["P"]),
        None if mask is None else _dev(mask.astype(np.uint8)),
        _dev(v["scales"]), _dev(v["errs"]))


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", A.PHASE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_align_phases_match_the_formula(shape, masked):
    """k_align_phases against phases_reference rounded to float64.  Phase:
    |dev| <= 8 x 2^-53 (|phi| + A (nu^-2 + nu_ref^-2)), A = Dconst |DM| / P
    (two pow calls, three roundings in A, a subtraction, a product, a sum);
    weight: 4 x 2^-53 relative (a product and a division).  The float64
    NumPy evaluation stays within a fifth of the phase bar
    (tests/test_align_inputs.py), and so does the kernel (worst 0.20 at
    7 x 37) now that it takes nu^-2 as 1 / (nu nu); with the device's
    pow(nu, -2.0), up to 9.8 ulp off, it reached 1.02 there (DESIGN.md
    section 4)."""
    c = A.phase_case(*shape)
    mask = c["mask"] if masked else None
    ph, wt = (t.cpu().numpy() for t in _phases(c, mask))
    rp, rw = (a.astype(np.float64) for a in A.phases_reference(
        c["phi"], c["DM"], c["P"], c["nu_ref"], c["freqs"], c["scales"],
        c["errs"], mask))
    keep = np.ones(shape, bool) if mask is None else mask
    bound = A.phase_bound(c["phi"], c["DM"], c["P"], c["nu_ref"], c["freqs"])
    rel = np.abs(ph - rp) / bound
    relw = np.abs(wt - rw)[keep] / (4 * A.U * np.abs(rw[keep]))
    print("ALIGN phases %dx%d %s: worst |dev| / bar %.2f (phases) %.2f "
          "(weights)" % (shape + ("mask" if masked else "nomask", rel.max(),
                                  relw.max() if relw.size else 0.0)))
    assert np.isfinite(ph).all() and np.isfinite(wt).all()
    assert (np.abs(ph - rp) <= bound).all()
    assert (relw <= 1.0).all()
    z = (c["DM"] == 0.0)[:, None] & keep
    assert (ph[z] == np.broadcast_to(c["phi"][:, None], shape)[z]).all()
    assert (ph[~keep] == 0.0).all() and (wt[~keep] == 0.0).all()
    assert wt[keep].all()


# ---------------------------------------------------------------------------
# g. the two kernels together
# ---------------------------------------------------------------------------
def test_phases_feed_accum_on_the_device():
    """align_phases' device tensors go straight into align_accum, with NaN in
    the data, freqs, scales and errs of every masked (sub-int, channel).
    The reference is align_reference at phases_reference.

    The bar of (a) is widened by what the phase and weight errors allowed in
    (f) can do to the sum, and by nothing else.  A phase error d turns
    harmonic k of a row by exp(2 pi i k d), a change of at most 2 pi k d
    |X_k|; in the time domain (irfft: harmonics 1 .. K - 1 count twice, K =
    nbin / 2 once) a sample moves by at most
        (2 pi d / nbin) sum_k c_k k |X_k|
          <= (2 pi d / nbin) sqrt(sum_k c_k k^2) sqrt(sum_k c_k |X_k|^2)
          <= 2 pi d sqrt(K (K + 1) (2 K + 1) / 3) rms(x)
    (Cauchy-Schwarz, then Parseval: sum_k c_k |X_k|^2 <= nbin sum_t x_t^2).
    A relative weight error of 4 x 2^-53 moves a sample by at most that
    times w |rotated x| <= w sqrt(nbin) rms(x).  Summed over the live
    sub-ints with their weights, twice for the two calls.  The phase case is
    a slow pulsar (dispersive term below a rotation), which keeps d, and so
    the widening, near the bar itself."""
    case, nbin = (37, 1024), 256
    x = A.inputs(case, nbin, "f32")[0]
    c = A.phase_case(*case, slow=True)
    mask = c["mask"].copy()
    mask[:, 5] = False                   # a channel with no live row
    bad = {k: np.where(mask, c[k], np.nan)
           for k in ("freqs", "scales", "errs")}
    ph, wt = _phases(c, mask, bad)
    assert (wt.cpu().numpy()[~mask] == 0.0).all()
    got = _accum(np.where(mask[:, :, None], x, np.float32(np.nan)), ph, wt)
    rp, rw = (a.astype(np.float64) for a in A.phases_reference(
        c["phi"], c["DM"], c["P"], c["nu_ref"], c["freqs"], c["scales"],
        c["errs"], mask))
    ref = A.align_reference(x, rp, rw)
    K = nbin // 2
    rms = np.sqrt((x.astype(np.float64) ** 2).mean(axis=-1))
    d = A.phase_bound(c["phi"], c["DM"], c["P"], c["nu_ref"], c["freqs"])
    per_row = rw * rms * (2 * np.pi * d * np.sqrt(K * (K + 1) * (2 * K + 1)
                                                  / 3.0) +
                          4 * A.U * np.sqrt(nbin))
    widen = 2 * per_row.sum(axis=0)
    base = OUT_ATOL * np.abs(ref).max()
    print("ALIGN groups phases -> accum: widening / bar %.2f (worst channel)"
          % (widen.max() / base))
    dead = _check("phases -> accum %s %d" % (A.case_id(case), nbin), got, ref,
                  rw, atol=(base + widen)[:, None],
                  wsum_rtol=WSUM_RTOL + 4 * A.U)
    assert dead[5] and dead.sum() == 1
