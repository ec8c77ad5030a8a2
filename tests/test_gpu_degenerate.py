"""Degenerate sub-integrations and poisoned masked channels on every fit
kernel family (tests/degenerate.py; the host side of the same inputs:
tests/test_degenerate_inputs.py).

include/ppfit.h: "Per-sub-integration numerical outcomes are reported in
ppf_result.status, never by aborting the batch", values in masked channels
reach no result, and (engine.fit_batch) "a sub-int's result does not depend
on the batch it is in".  Parts A, B and D compare the library with itself
on cleaner input, bit for bit; part C goes against the oracle at the
project's bars (ragged.compare_row)."""
import functools

import numpy as np
import pytest

import degenerate as D
import ragged as R

pytestmark = pytest.mark.gpu


def _index():
    from pulseportraiture_amd import _lib
    return _lib.RESULT_INDEX


@functools.lru_cache(maxsize=None)
def _clean(name):
    """The case's clean batch of four (shared, read-only)."""
    r = R.device_fit(R.case(name))
    for a in r.values():
        a.setflags(write=False)
    return r


# ---------------------------------------------------------------------------
# A. poisoned masked channels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_masked_channels_are_never_read_into_a_result(name):
    """NaN rows, +-Inf and NaN samples, and a constant near the top of the
    number format in every masked channel (data, errs, guess weight): all
    five tables are bitwise those of the clean call, and the per-channel
    tables are exactly 0 where masked.  Sub-int 0 masks nothing: the
    control row.  A kernel that weights a masked row by 0 instead of
    skipping it fails here (NaN * 0), and so does one that sums every row
    and subtracts the masked ones (the huge constant)."""
    c = R.case(name)
    keep = R.inputs(c)["keep"]
    clean = _clean(name)
    for v in D.VARIANTS:
        r = R.device_fit(c, over=D.poisoned(c, v))
        for t in D.TABLES:
            np.testing.assert_array_equal(
                r[t], clean[t], err_msg="%s variant %d %s" % (name, v, t))
        for t in D.PER_CHANNEL:
            assert (r[t][~keep] == 0.0).all(), (name, v, t)


# ---------------------------------------------------------------------------
# B. degenerate sub-ints inside a batch
# ---------------------------------------------------------------------------
def _check_nofit(r, j, tag):
    """Row j holds the PPF_ST_NOFIT record of include/ppfit.h: zeros but
    for status and phi_guess, every field finite, zero tables."""
    from pulseportraiture_amd import _lib
    I = _index()
    rec = r["results"][j]
    assert rec[I["status"]] == _lib.ST_NOFIT, (tag, rec[I["status"]])
    assert np.isfinite(rec).all(), (tag, rec)
    rest = np.delete(rec, [I["status"], I["phi_guess"]])
    assert (rest == 0.0).all(), (tag, rec)
    for t in D.PER_CHANNEL + ("covariance",):
        assert (r[t][j] == 0.0).all(), (tag, t)


def _check_nonfinite(r, j, tag, cap=1000):
    from pulseportraiture_amd import _lib
    I = _index()
    rec = r["results"][j]
    st = int(rec[I["status"]])
    print("DEGENERATE %s: status 0x%x niter %d nfeval %d chi2 %r" %
          (tag, st, rec[I["niter"]], rec[I["nfeval"]], rec[I["chi2"]]))
    assert st & _lib.ST_NONFINITE, (tag, hex(st), rec[I["chi2"]])
    assert rec[I["niter"]] <= cap, (tag, rec[I["niter"]])
    assert rec[I["nfeval"]] >= 1, (tag, rec[I["nfeval"]])


def _check_batch(name, order, over_more=None, clean=None):
    c = R.case(name)
    subs, over = D.degenerate(c, order)
    over.update(over_more or {})
    r = R.device_fit(c, subs, over)        # returns: PPF_OK
    clean = _clean(name) if clean is None else clean
    for j, k in enumerate(order):
        tag = (name, k)
        if k[0] == "s":
            for t in D.TABLES:
                np.testing.assert_array_equal(
                    r[t][j], clean[t][int(k[1:])], err_msg=str(tag + (t,)))
        elif k in ("N", "Z"):
            _check_nonfinite(r, j, tag)
        else:
            _check_nofit(r, j, tag)
    return r


@pytest.mark.parametrize("name", D.FAMILIES)
def test_degenerate_subints_end_alone(name):
    """E, s0, F, s1, N, s2, Z, s3, E2 in one call: the call returns, the
    case's own sub-ints are bitwise those of the clean batch of four (the
    degenerate neighbours shift every X slot and list entry of k_classify),
    E / F / E2 hold the documented PPF_ST_NOFIT record, N and Z end with
    PPF_ST_NONFINITE within the iteration cap.  The reference raises on N
    and Z (test_degenerate_inputs.py); a success status with a finite chi2
    there is the failure this test is for."""
    _check_batch(name, D.ORDER)


@pytest.mark.parametrize("name", D.SCIPY)
def test_degenerate_subints_scipy_solver(name):
    """The same through tr_update_t (PPF_OPT_SCIPY_TR), on the moment path
    and on the streaming one; the case's own sub-ints against a clean call
    with that solver."""
    _check_batch(name, D.ORDER, dict(solver="scipy"),
                 R.device_fit(R.case(name), over=dict(solver="scipy")))


def test_degenerate_subints_without_x_slots():
    """n_x = 0 (PPF_OPT_NO_X) on the fused guess path at 2048 bins: the
    list-strided launches with degenerate entries in and around the lists.
    No scattering sub-int, so nothing is dropped and E, F, N, Z apply."""
    from pulseportraiture_amd import _lib
    r = _check_batch(D.NO_X, D.NO_X_ORDER, dict(n_x=0))
    st = r["results"][:, _index()["status"]].astype(int)
    assert not (st & _lib.ST_NOSPACE).any(), st


@pytest.mark.parametrize("name", D.ONLY)
def test_only_degenerate_subints(name):
    """E, F, E2 alone: no fit iterates (kinds = {0, 0}), no iteration
    kernel is launched and nothing is read that was never written."""
    _check_batch(name, D.ONLY_DEGENERATE)


# ---------------------------------------------------------------------------
# C. minimal channel counts against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.MINIMAL_NAMES)
def test_minimal_channel_counts_match_oracle(name):
    """One usable channel fitted for the phase, two for phase and DM, at
    the band's first channel, its last (a partial tile) and apart, in one
    batch per family; and a true one-channel array.  ragged.compare_row's
    bars."""
    m = D.minimal(name)
    r = D.minimal_device_fit(name)
    for j in range(m["nsub"]):
        R.compare_row("MINIMAL %s sub %d" % (name, j), (name, j), r, j,
                      D.minimal_oracle(name, j), m["keep"][j], m["P"], False)


# ---------------------------------------------------------------------------
# D. the other entry points that take a mask or a weight
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nchan,nbin", [(12, 512), (37, 1001)])
def test_align_accum_skips_nan_rows_of_zero_weight(nchan, nbin):
    import torch
    from pulseportraiture_amd import engine
    rng = np.random.default_rng(nchan)
    nsub = 5
    x = rng.normal(size=(nsub, nchan, nbin)).astype(np.float32)
    ph = rng.uniform(-0.5, 0.5, size=(nsub, nchan))
    w = rng.uniform(0.1, 2.0, size=(nsub, nchan))
    zero = rng.random((nsub, nchan)) < 0.3
    zero[0, 0] = zero[-1, -1] = True
    zero[:, 3] = True                  # a channel with no weight at all
    w[zero] = 0.0
    bad = x.copy()
    bad[zero] = np.nan
    got = []
    for rows in (x, bad):
        out = torch.zeros((nchan, nbin), dtype=torch.float64, device="cuda")
        ws = torch.zeros(nchan, dtype=torch.float64, device="cuda")
        engine.align_accum(rows, ph, w, out, ws)
        got.append((out.cpu().numpy(), ws.cpu().numpy()))
    np.testing.assert_array_equal(got[1][0], got[0][0])
    np.testing.assert_array_equal(got[1][1], got[0][1])
    assert np.isfinite(got[1][0]).all() and not got[1][0][3].any()


def test_align_phases_ignores_masked_inputs():
    import torch
    from pulseportraiture_amd import _lib, engine
    I = _lib.RESULT_INDEX
    rng = np.random.default_rng(3)
    nsub, nchan = 5, 37
    res = np.zeros((nsub, _lib.RESULT_DOUBLES))
    res[:, I["params"].start] = rng.uniform(-0.5, 0.5, nsub)
    res[:, I["params"].start + 1] = 34.5 + rng.normal(0, 1e-3, nsub)
    res[:, I["nu_out"].start] = 1500.0
    freqs = np.tile(np.linspace(1100.0, 1900.0, nchan), (nsub, 1))
    P = np.full(nsub, 2.9e-3)
    scales = rng.uniform(0.5, 2.0, (nsub, nchan))
    errs = rng.uniform(0.5, 1.5, (nsub, nchan))
    mask = rng.random((nsub, nchan)) > 0.3
    mask[0, 0] = mask[-1, -1] = False

    def run(freqs, scales, errs):
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda()
             for a in (res, freqs, P, scales, errs)]
        ph, wt = engine.align_phases(
            t[0], t[1], t[2], torch.from_numpy(mask.astype(np.uint8)).cuda(),
            t[3], t[4])
        return ph.cpu().numpy(), wt.cpu().numpy()
    clean = run(freqs, scales, errs)
    bad = [a.copy() for a in (freqs, scales, errs)]
    for a in bad:
        a[~mask] = np.nan
    got = run(*bad)
    for g, c in zip(got, clean):
        np.testing.assert_array_equal(g, c)
        assert (g[~mask] == 0.0).all() and g[mask].all()


def test_unpack_psrfits_ignores_zero_weight_channels():
    """elem 2 (big-endian float32 samples), 32 channels: NaN samples in the
    zero-weight channels leave total, wstart and the other channels' rows
    and stats bitwise unchanged."""
    import torch
    from pulseportraiture_amd import engine
    rng = np.random.default_rng(8)
    nsub, nchan, nbin = 3, 32, 256
    x = rng.normal(size=(nsub, 1, nchan, nbin)).astype(np.float32)
    x[..., 100:120] += 5.0
    wts = np.ones((nsub, nchan), dtype=np.float32)
    zero = rng.random((nsub, nchan)) < 0.25
    zero[0, 0] = zero[1, 15] = zero[1, 16] = zero[2, 31] = True
    wts[zero] = 0.0
    scl = rng.uniform(0.5, 2.0, (nsub, nchan)).astype(np.float32)
    offs = rng.normal(size=(nsub, nchan)).astype(np.float32)

    def run(x):
        raw = torch.from_numpy(np.ascontiguousarray(
            x.astype(">f4")).view(np.uint8).reshape(nsub, -1)).cuda()
        r = engine.unpack_psrfits(raw, 2, 1, nchan, nbin, scl, offs, wts=wts)
        torch.cuda.synchronize()
        return {k: r[k].cpu().numpy()
                for k in ("rows", "stats", "total", "wstart")}
    clean = run(x)
    bad = x.copy()
    bad[:, 0][zero] = np.nan
    got = run(bad)
    np.testing.assert_array_equal(got["total"], clean["total"])
    np.testing.assert_array_equal(got["wstart"], clean["wstart"])
    np.testing.assert_array_equal(got["rows"][~zero], clean["rows"][~zero])
    np.testing.assert_array_equal(got["stats"][~zero], clean["stats"][~zero])
    assert np.isfinite(got["total"]).all()
    assert np.isnan(got["rows"][zero]).all()


@pytest.mark.parametrize("nbin", [512, 1001])
def test_per_row_kernels_keep_a_nan_row_to_itself(nbin):
    """ppf_resid_chi2_batch and ppf_noise_batch take four rows per
    workgroup: a NaN row gives a NaN output, its neighbours' are bitwise
    unchanged."""
    from pulseportraiture_amd import engine
    rng = np.random.default_rng(nbin)
    n = 11
    rows = rng.normal(size=(n, nbin)).astype(np.float32)
    model = rng.normal(size=(2, nbin))
    ph = rng.uniform(-0.5, 0.5, n)
    mi = (np.arange(n) % 2).astype(np.int32)
    sc, er = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 1.5, n)
    bad = rows.copy()
    nan = np.zeros(n, dtype=bool)
    nan[[1, 4, 7, 10]] = True      # one of each position in a group of four
    bad[nan, 5] = np.nan
    for fn in (lambda x: engine.resid_chi2_rows(x, ph, model, mi, sc, er,
                                                nbin - 2),
               engine.noise_rows):
        clean, got = fn(rows).cpu().numpy(), fn(bad).cpu().numpy()
        assert np.isfinite(clean).all()
        assert np.isnan(got[nan]).all(), got
        np.testing.assert_array_equal(got[~nan], clean[~nan])
