"""Host checks of the mixed-configuration batches (tests/mixed.py): every
batch mixes what tests/test_gpu_mixed.py relies on, and the oracle's fit of
EVERY sub-int of EVERY batch converges and is sharply defined, so that a
device deviation there is the device's.  No sub-int is left out, here or on
the GPU.  No GPU."""
import numpy as np
import pytest

import goldens as G
import mixed as M
import ragged as R

# the families and shapes of the issue's table: none may go missing
EXPECTED = {
    "fused": {(37, 512), (100, 1024)}, "momx": {(100, 512)},
    "guess": {(100, 2048)}, "guessf": {(100, 2048)}, "wm": {(45, 1000)},
    "wo": {(33, 1001)}, "blk": {(17, 512), (45, 4096)}, "long": {(5, 8194)},
    "scat": {(257, 256), (97, 512)}, "scat1": {(257, 256), (97, 512)},
    "bounds": {(37, 512), (97, 512)},
}


def test_batch_table_is_complete():
    got = {}
    for c in M.BATCHES:
        got.setdefault(c["name"].split("-")[0], set()).add(
            (c["nchan"], c["nbin"]))
    assert got == EXPECTED
    assert len(set(M.NAMES)) == len(M.BATCHES)
    assert M.batch("fused-37x512")["mom_x"] is False
    assert M.batch("momx-100x512")["mom_x"] is True
    assert M.batch("guess-100x2048")["mom_x"] is None
    assert M.batch("guessf-100x2048")["mom_x"] is False
    for n in M.WAVE_NAMES + M.NO_X_NAMES:
        assert n in M.NAMES
    assert {M.batch(n)["option"] for n in M.NAMES
            if n.startswith("scat")} == {0, 1}
    assert R.warm_stride(257) == 2
    # estimated and given errors both occur
    given = [M.inputs(c)["errs_given"] for c in M.BATCHES]
    assert any(given) and not all(given)


@pytest.mark.parametrize("name", M.MIXED_KIND)
def test_batch_mixes_every_per_subint_input(name):
    """fit_flags (at least six kinds, or the long rows' four), streaming and
    moment sub-ints interleaved with a streaming one last and no streaming
    sub-int's X slot equal to its index on the fused path, three models in a
    non-monotone order with repeats, P, freqs, nu_fits, nu_outs (NaN rows
    and explicit ones) and both masks differ inside the batch."""
    c = M.batch(name)
    b = M.inputs(c)
    nsub = b["nsub"]
    st = M.streams(c)
    kinds = set(c["order"])
    if name.startswith("long"):
        assert kinds == {"PD", "P", "PDT", "PDfix"}
    elif name.startswith("bounds"):
        assert kinds == {"PDTA", "TA", "PD", "PDT", "PDG"}
    else:
        assert len(kinds) >= 6
    assert 0 < M.x_subints(c) < nsub
    assert M.x_subints(c) == st.sum()
    assert st[-1] and st.any() and not st.all()
    assert np.any(st[1:] != st[:-1])
    if not name.startswith(("long", "bounds")):
        assert not st[0]
        slots = np.cumsum(st) - 1
        assert np.all(slots[st] != np.arange(nsub)[st])
        assert np.where(st)[0][2] != 2       # the third streaming sub-int
    mi = b["mi"]
    assert set(mi) == {0, 1, 2} and np.any(np.diff(mi) < 0) and \
        np.any(np.diff(mi) > 0) and len(mi) > len(set(mi))
    assert b["models"].shape == (3, c["nchan"], c["nbin"])
    assert len(set(b["P"])) == nsub
    assert len({tuple(f) for f in b["freqs"]}) == nsub
    assert np.all(np.abs(b["freqs"] - b["freqs"][0]) < 20.0)
    assert len({tuple(f) for f in b["nu_fits"]}) == nsub
    nan_rows = np.isnan(b["nu_outs"]).all(axis=1)
    assert nan_rows.any() and (~np.isnan(b["nu_outs"])).all(axis=1).any()
    assert b["keep"][0::2].all() and not b["keep"][1::2].all(axis=1).any()
    # linear tau: the non-scattering sub-ints start (and stay) at tau = 0
    assert not c["log10_tau"]
    assert np.all((b["init"][:, 3] != 0) == st)
    # a held tau is never given a bound ("Not in this change": a positive
    # lower tau bound on a sub-int held at tau = 0 must not be constructed)
    assert np.isnan(b["bounds"][:, 3]).all()
    for a in (b["data"], b["init"], b["freqs"], b["keep"], b["models"]):
        assert not a.flags.writeable


@pytest.mark.parametrize("name", [n for n in M.NAMES if n.startswith("scat")])
def test_all_scattering_batches(name):
    c = M.batch(name)
    b = M.inputs(c)
    assert c["log10_tau"] and M.x_subints(c) == b["nsub"]
    assert set(c["order"]) == {"PDTA", "PDT", "TA", "ALL", "PDGT", "PDfix"}
    assert set(b["mi"]) == {0, 1, 2}


@pytest.mark.parametrize("name", M.BOUNDS_NAMES)
def test_bounds_rows(name):
    """Half the rows all-NaN, the others with a DM box that contains the
    truth and an alpha upper bound the oracle's TNC ends on exactly."""
    c = M.batch(name)
    b = M.inputs(c)
    boxed = np.array(b["boxed"])
    assert boxed.sum() * 2 == b["nsub"]
    assert np.isnan(b["bounds"][~boxed]).all()
    for i in np.where(boxed)[0]:
        lo, hi = b["bounds"][i, 1]
        assert lo < b["truth"][i, 1] < hi and lo < b["init"][i, 1] < hi
        assert b["bounds"][i, 4, 1] == M.ALPHA_UPPER and b["flags"][i, 4]
        assert b["truth"][i, 4] == -4.0
        o = M.oracle_fit(c, i)
        assert o["params"][4] == M.ALPHA_UPPER
        # active beyond doubt: the unbounded fit sits many sigma above it
        u = M.oracle_fit(c, i, bounded=False)
        assert u["params"][4] - M.ALPHA_UPPER > 3 * u["param_errs"][4]


@pytest.mark.parametrize("name", ["guess-100x2048", "guessf-100x2048"])
def test_guess_batches_hold_models_on_both_sides_of_the_cutoff(name):
    """k_gflag: a sub-int's guess rides in the spectrum pass only where its
    OWN model has no harmonic above the fused range."""
    c = M.batch(name)
    b = M.inputs(c)
    assert c["guess"]
    kmax = np.array([R.kc(m).max() for m in b["models"]])
    per_sub = kmax[b["mi"]]
    assert (per_sub > R.GUESS_HARMONICS).any()
    assert (per_sub < R.GUESS_HARMONICS).any()
    # model 0 is below: a gflag computed from model 0 for every sub-int
    # would differ from the right one
    assert kmax[0] < R.GUESS_HARMONICS
    st = M.streams(c)
    # with fused moments gflag needs both: streaming and a cut model
    assert (st & (per_sub < R.GUESS_HARMONICS)).any()
    assert (st & (per_sub > R.GUESS_HARMONICS)).any()
    assert (~st & (per_sub < R.GUESS_HARMONICS)).any()


@pytest.mark.parametrize("name", M.NAMES)
def test_every_oracle_fit_is_well_posed(name):
    """Every sub-int of the batch: the oracle converges (trust-ncg: return
    code 2; TNC: not 3 = MAXFUN, the code test_gettoas_branches_match_
    reference excludes, and here one of scipy's converged codes), and
    restarted from its own solution plus 1e-2 sigma in every fitted
    parameter it lands within goldens.SIGMA_TOL of it."""
    c = M.batch(name)
    b = M.inputs(c)
    for i in range(b["nsub"]):
        tag = (name, i, c["order"][i])
        o = M.oracle_fit(c, i)
        o2 = M.oracle_refit(c, i, o)
        if b["boxed"][i]:
            assert o["return_code"] in (0, 1, 2), (tag, o["return_code"])
            # (restarted 1e-2 sigma from the minimum, TNC may also end with
            # 4, "linear search failed": there is nothing left to gain)
            assert o2["return_code"] in (0, 1, 2, 4), (tag, o2["return_code"])
        else:
            assert o["return_code"] == 2 and o2["return_code"] == 2, \
                (tag, o["return_code"], o2["return_code"])
        keep = b["keep"][i]
        assert len(o["scales"]) == keep.sum()
        assert o["dof"] == keep.sum() * (c["nbin"] - 1) - b["flags"][i].sum()
        dev = G.param_deviation_sigma(o2, o, b["P"][i], c["log10_tau"])
        assert dev.max() < G.SIGMA_TOL, (tag, dev)
        # held parameters stay where they start
        held = b["flags"][i] == 0
        x0 = M.start(c, i)
        assert np.all(np.asarray(o["x_fit"])[held] == x0[held]), tag
        assert np.all(o["param_errs"][held] == 0.0), tag


def test_oracle_maxiter_caps_trust_ncg():
    """fit_portrait_full(maxiter=m) stops trust-ncg after m iterations
    (warnflag 1); the default leaves the fit as it was."""
    c = M.batch("fused-37x512")
    full = M.oracle_fit(c, 2)
    capped = M.oracle_fit(c, 2, maxiter=2)
    assert full["return_code"] == 2 and capped["return_code"] == 1
    assert capped["fun"] > full["fun"]
    assert capped["nfeval"] < full["nfeval"]
