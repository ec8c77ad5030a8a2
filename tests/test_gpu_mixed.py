"""Mixed per-sub-int fit configurations in one engine.fit_batch call, on
every fit kernel family, against the f64 oracle's fit of each sub-int alone
(tests/mixed.py; the host side of the same batches:
tests/test_mixed_inputs.py).

Inside one call the sub-ints differ in fit_flags (moment and streaming kinds
interleaved: k_classify's X slots are a real compaction, k_tr_init counts
both kinds for the host loop), model_index (three models; k_gflag's choice
depends on the sub-int's own), P, freqs, nu_fits, nu_outs and mask.  Bars:
the project's, through ragged.compare_row (shared with
tests/test_gpu_ragged.py).  There is no skip list: every sub-int of every
batch is compared."""
import functools

import numpy as np
import pytest

import goldens as G
import mixed as M
import ragged as R

pytestmark = pytest.mark.gpu

SIG, RCHI2 = G.SIGMA_TOL, G.RCHI2_RTOL


@functools.lru_cache(maxsize=None)
def _full(name):
    """The batch in one call (numpy tables, read-only, shared)."""
    r = M.device_fit(M.batch(name))
    for a in r.values():
        a.setflags(write=False)
    return r


def _index():
    from pulseportraiture_amd import _lib
    return _lib.RESULT_INDEX


def _assert_same(a, b, rows_a=None, rows_b=None, msg=""):
    """Every output table of a (rows rows_a) bitwise that of b (rows_b)."""
    for k in M.TABLES:
        x = a[k] if rows_a is None else a[k][rows_a]
        y = b[k] if rows_b is None else b[k][rows_b]
        np.testing.assert_array_equal(x, y, err_msg="%s %s" % (k, msg))


def _held_exact(c, r, j, i):
    """Held parameters keep their initial value exactly (phase and tau at
    nu_fit: x_fit_phi, x_fit_tau), with an error of exactly 0."""
    I = _index()
    b = M.inputs(c)
    res = r["results"][j]
    at_fit = np.array(res[I["params"]])
    at_fit[0], at_fit[3] = res[I["x_fit_phi"]], res[I["x_fit_tau"]]
    held = b["flags"][i] == 0
    tag = (c["name"], i, c["order"][i])
    assert np.all(at_fit[held] == b["init"][i][held]), (tag, at_fit)
    assert np.all(res[I["param_errs"]][held] == 0.0), tag
    assert np.all(res[I["param_errs"]][~held] > 0.0), tag


def _compare(c, r, j, i):
    b = M.inputs(c)
    out = R.compare_row(
        "MIXED %s sub %d %s" % (c["name"], i, c["order"][i]),
        (c["name"], i, c["order"][i]), r, j, M.oracle_fit(c, i, False),
        b["keep"][i], b["P"][i], c["log10_tau"])
    _held_exact(c, r, j, i)
    return out


@pytest.mark.parametrize("name", M.ORACLE_NAMES)
def test_mixed_batch_matches_oracle(name):
    """Each sub-int of a mixed batch against the oracle's fit of that
    sub-int alone (its kept channels, its own model, flags, P, freqs,
    nu_fits, nu_outs, the batch's option): fused k_xmom_g with X only for
    the streaming sub-ints, forced moments from X, the guess in the spectrum
    pass and through k_dsum_w in one call (default moments from X: by model;
    fused moments: by kind and by model), mixed-radix and odd-nbin wave
    passes, block FFT, long rows, and the all-scattering log10-tau batches
    (k_pass warm start at stride 2; option 0 and 1)."""
    c = M.batch(name)
    r = _full(name)
    for i in range(M.inputs(c)["nsub"]):
        _compare(c, r, i, i)


@pytest.mark.parametrize("name", M.WAVE_NAMES)
def test_mixed_single_equals_batch(name):
    """Each sub-int fitted alone (batch of one, its own model as nmodel = 1)
    is bitwise its row of the mixed batch, and a permutation of the batch,
    which changes every X slot, gives the permuted rows bitwise.

    (k_xmom_g once failed the last step at [fused-100x1024] and
    [guessf-100x2048]: with nmodel == 1 it stopped each channel's folded
    harmonic sum at the cutoff KC_n and spread the shorter range over its
    eight waves, with nmodel > 1 it summed the whole range, so the
    moment-mode sub-ints with a cut model differed by up to 6.4e-12 relative
    from their batch rows.  Its blocks of harmonics now go to the waves in
    turn, in an order that does not depend on the cutoff: DESIGN.md, mixed
    configurations.)"""
    c = M.batch(name)
    full = _full(name)
    nsub = M.inputs(c)["nsub"]
    perm = np.array([3, 7, 0, 5, 2, 6, 1, 4])
    assert sorted(perm) == list(range(nsub))
    st = M.streams(c)
    before = dict(zip(np.where(st)[0], range(st.sum())))
    after = dict(zip(perm[st[perm]], range(st.sum())))
    assert all(before[i] != after[i] for i in before), (before, after)
    p = M.device_fit(c, perm)
    _assert_same(p, full, None, perm, "%s permuted" % name)
    # alone, the batch's model table kept (nmodel = 3, model_index = [mi])
    for i in range(nsub):
        one = M.device_fit(c, [i])
        _assert_same(one, full, 0, i, "%s sub %d alone, nmodel 3" % (name, i))
    # alone, its own model as nmodel = 1: every sub-int is run and its
    # largest relative deviation printed before any is asserted
    bad = []
    for i in range(nsub):
        one = M.device_fit(c, [i], single_model=True)
        worst, where = 0.0, ""
        for k in M.TABLES:
            x, y = one[k][0].ravel(), full[k][i].ravel()
            ne = np.where(x != y)[0]
            if len(ne):
                rel = np.abs(x[ne] - y[ne]) / np.maximum(np.abs(y[ne]), 1e-300)
                j = ne[np.argmax(rel)]
                if rel.max() > worst:
                    worst = float(rel.max())
                    where = " at %s[%d]: %.17g vs %.17g" % (k, j, x[j], y[j])
        print("MIXED %s sub %d %s alone, nmodel 1: max rel diff %.1e%s" %
              (name, i, c["order"][i], worst, where))
        if worst:
            bad.append((i, c["order"][i], worst))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", ["fused-100x1024", "momx-100x512"])
@pytest.mark.parametrize("frac", [(7, 8), (1, 8)])
def test_mixed_chunked_equals_one_call(name, frac):
    """A workspace budget that splits the mixed batch into chunks of 1-3
    sub-ints (engine.fit_batch's per-chunk X slot count xsel[c0:c1] with
    both kinds in the batch): every output table bitwise the one call's."""
    c = M.batch(name)
    nsub = M.inputs(c)["nsub"]
    _, raw = M.device_fit(c, raw=True)
    need = raw["workspace"].numel()
    assert not isinstance(raw["_keep"][0], tuple)       # one call
    r, raw = M.device_fit(c, raw=True,
                          max_workspace=need * frac[0] // frac[1])
    chunks = raw["_keep"]
    assert isinstance(chunks[0], tuple)
    assert nsub / 3.0 <= len(chunks) <= nsub, len(chunks)
    print("MIXED chunked %s budget %d/%d: %d chunks" %
          (name, frac[0], frac[1], len(chunks)))
    _assert_same(r, _full(name), msg="%s in %d chunks" % (name, len(chunks)))


@pytest.mark.parametrize("a,b", [("guessf-100x2048", "scat-97x512"),
                                 ("blk-45x4096", "fused-37x512")])
def test_workspace_reuse_across_kinds_and_shapes(a, b):
    """GetTOAs hands one archive's workspace to the next: batch B fitted in
    the workspace batch A left (another family, a larger shape, another kind
    mix) is bitwise B in a fresh workspace, and A fitted again in that
    workspace after B is bitwise A."""
    ca, cb = M.batch(a), M.batch(b)
    ra, raw_a = M.device_fit(ca, raw=True)
    ws = raw_a["workspace"]
    _assert_same(ra, _full(a), msg=a)
    rb, raw_b = M.device_fit(cb, raw=True, workspace=ws)
    assert raw_b["workspace"] is ws                     # reused, not replaced
    _assert_same(rb, _full(b), msg="%s in the workspace of %s" % (b, a))
    ra2, raw_a2 = M.device_fit(ca, raw=True, workspace=ws)
    assert raw_a2["workspace"] is ws
    _assert_same(ra2, _full(a), msg="%s in the workspace of %s" % (a, b))


@pytest.mark.parametrize("name", M.BOUNDS_NAMES)
def test_nan_bounds_rows_equal_unbounded(name):
    """bounds [nsub, 5, 2]: the all-NaN rows are bitwise the same sub-ints
    fitted with bounds=None (the Newton trust region) and match the oracle's
    trust-ncg; the boxed rows match the oracle's method='TNC' fit at
    test_gettoas_branches_match_reference's bars for TNC (the phase compared
    at the oracle's nu_DM), with the active alpha bound hit exactly."""
    I = _index()
    c = M.batch(name)
    b = M.inputs(c)
    full = _full(name)
    boxed = np.array(b["boxed"])
    free = np.where(~boxed)[0]
    unb = M.device_fit(c, free, bounds=None)
    _assert_same(unb, full, None, free, "%s NaN rows" % name)
    for i in free:
        _compare(c, full, i, i)
    for i in np.where(boxed)[0]:
        tag = (name, i, c["order"][i])
        o = M.oracle_fit(c, i)
        res = full["results"][i]
        assert int(res[I["status"]]) >> 8 == 0, (tag, res[I["status"]])
        assert res[I["params"]][4] == M.ALPHA_UPPER, (tag, res[I["params"]])
        assert o["params"][4] == M.ALPHA_UPPER
        got = dict(params=res[I["params"]], nu_DM=res[I["nu_out"]][0],
                   nu_GM=res[I["nu_out"]][1], nu_tau=res[I["nu_out"]][2])
        dev = G.param_deviation_sigma(got, o, b["P"][i], False)
        rel = abs(res[I["red_chi2"]] / o["red_chi2"] - 1)
        print("MIXED %s sub %d %s TNC: dev %.2e sigma, chi2_red rel %.1e" %
              (name, i, c["order"][i], dev.max(), rel))
        assert dev.max() < SIG, (tag, dev)
        assert rel < RCHI2, (tag, rel)
        np.testing.assert_allclose(res[I["param_errs"]], o["param_errs"],
                                   rtol=1e-4, err_msg=str(tag))
        np.testing.assert_allclose(res[I["snr"]], o["snr"], rtol=1e-6,
                                   err_msg=str(tag))
        np.testing.assert_allclose(
            res[I["nu_out"]], [o["nu_DM"], o["nu_GM"], o["nu_tau"]],
            rtol=1e-5, err_msg=str(tag))
        assert res[I["dof"]] == o["dof"] and \
            res[I["nchanx"]] == b["keep"][i].sum(), tag
        _held_exact(c, full, i, i)


def test_max_iter_caps_each_fit():
    """solver="scipy", max_iter = m between the fastest and the slowest
    sub-int of a mixed batch: the fits that needed at most m iterations are
    bitwise unchanged, the others end with PPF_ST_MAXITER after exactly m
    and within goldens.SIGMA_TOL of the oracle's trust-ncg under the same
    cap (the host loop queues whole groups of iterations without looking:
    the cap is each fit's own)."""
    from pulseportraiture_amd import _lib
    I = _index()
    name = "fused-37x512"
    c = M.batch(name)
    b = M.inputs(c)
    free = M.device_fit(c, solver="scipy")
    nit = free["results"][:, I["niter"]].astype(int)
    st = free["results"][:, I["status"]].astype(int)
    assert np.all(st == _lib.ST_CONVERGED), st
    lo, hi = nit.min(), nit.max()
    assert lo < hi, nit
    # below the slowest, not below the fastest; where there is a choice, a
    # count no fit ends on
    cand = [v for v in range(lo, hi) if v not in nit] or [(lo + hi) // 2]
    m = cand[0]
    assert lo <= m < hi
    print("MIXED max_iter: uncapped niter %s, cap %d" % (nit, m))
    cap = M.device_fit(c, solver="scipy", max_iter=m)
    done = np.where(nit <= m)[0]
    cut = np.where(nit > m)[0]
    assert len(done) and len(cut)
    _assert_same(cap, free, done, done, "fits within the cap")
    for i in cut:
        tag = (name, i, c["order"][i])
        res = cap["results"][i]
        assert int(res[I["status"]]) == _lib.ST_MAXITER, (tag, res[I["status"]])
        assert res[I["niter"]] == m, (tag, res[I["niter"]])
        o = M.oracle_fit(c, i, False, maxiter=int(m))
        assert o["return_code"] == 1, tag
        got = dict(params=res[I["params"]], nu_DM=res[I["nu_out"]][0],
                   nu_GM=res[I["nu_out"]][1], nu_tau=res[I["nu_out"]][2])
        dev = G.param_deviation_sigma(got, o, b["P"][i], False)
        print("MIXED max_iter sub %d %s niter %d -> %d: dev %.2e sigma" %
              (i, c["order"][i], nit[i], m, dev.max()))
        assert dev.max() < SIG, (tag, dev)


@pytest.mark.parametrize("name", M.NO_X_NAMES)
def test_no_x_is_ignored_where_every_fit_streams(name):
    """engine.fit_batch(..., n_x=0) (PPF_OPT_NO_X) off the fused path (4096
    bins) and with the moments from X (forced; the default of the guess at
    2048 bins): every sub-int holds an X slot there, so the option changes
    nothing -- all tables bitwise those of n_x=None, no PPF_ST_NOSPACE.  (The
    host once skipped the read-back of the kind counts whenever the option
    was set and launched no k_pass: the streaming sub-ints came back
    unfitted with a success status.)"""
    from pulseportraiture_amd import _lib
    I = _index()
    c = M.batch(name)
    r = M.device_fit(c, n_x=0)
    st = r["results"][:, I["status"]].astype(int)
    assert not (st & _lib.ST_NOSPACE).any(), st
    _assert_same(r, _full(name), msg="%s n_x=0" % name)
