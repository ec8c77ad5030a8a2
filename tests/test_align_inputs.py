"""Host side of tests/aligncases.py: the shapes do put several sub-ints in
front of one wave of k_align_part_w, the zero-weight patterns leave what they
say, and phases_reference is the formula it claims to be.  A change of
align_groups' 2048 or of kXW that empties tests/test_gpu_align_groups.py
fails here."""
import numpy as np
import pytest

import aligncases as A


# ------------------------------------------------------------- the shapes ---
def test_case_table_is_the_partition_it_claims():
    want = {(18, 1024): (2, 9, [9, 9]), (37, 1024): (2, 19, [19, 18]),
            (50, 700): (3, 17, [17, 17, 16]), (19, 2048): (1, 19, [19])}
    assert set(A.CASES) == set(want)
    for case in A.CASES:
        p = A.partition(*case)
        assert (p["ngroup"], p["per"],
                [s1 - s0 for s0, s1 in p["groups"]]) == want[case], case
        # the groups tile [0, nsub) and the waves tile each group, in order
        rows = [s for g in p["waves"] for s in sorted(sum(g, []))]
        assert rows == list(range(case[0])), case
        for (s0, s1), g in zip(p["groups"], p["waves"]):
            for w, r in enumerate(g):
                assert r == list(range(s0 + w, s1, A.WAVES)), (case, w)


def test_every_case_gives_a_wave_a_second_row():
    for case in A.CASES:
        p = A.partition(*case)
        assert p["per"] > A.WAVES, case
        assert A.rows_per_wave(*case) >= 2, case
    # 18 x 1024: wave 0 alone takes two rows, the smallest second trip
    for g in A.partition(18, 1024)["waves"]:
        assert [len(r) for r in g] == [2] + [1] * 7
    assert any(A.rows_per_wave(*c) >= 3 for c in A.CASES)
    ragged = [c for c in A.CASES
              if len({s1 - s0 for s0, s1 in A.partition(*c)["groups"]}) > 1]
    assert (37, 1024) in ragged and (50, 700) in ragged
    assert [c for c in A.CASES if A.partition(*c)["ngroup"] == 1] == \
        [(19, 2048)]


def test_earlier_shapes_never_did():
    """Why the cases exist: every align shape the suite ran before them
    (parity 37 x 12 / 37 / 100, degenerate 5 x 12 / 37, plan sweep 3 x 5,
    full-shape C4 16 / 24 x 256) gives each wave at most one row."""
    for shape in A.OLD_SHAPES:
        assert A.rows_per_wave(*shape) <= 1, shape
        assert A.partition(*shape)["per"] <= A.WAVES, shape


def test_partition_matches_the_library():
    """ngroup as ppf_align_accum sizes its workspace (ngroup partial spectra
    of nbin / 2 + 1 harmonics and ngroup weight sums per channel, each part
    rounded up to 256 bytes): the one group count that explains the byte
    count is partition()'s."""
    from pulseportraiture_amd import _lib
    lib = _lib.load()

    def up(n):
        return (n + 255) & ~255

    for nsub, nchan in A.CASES + A.OLD_SHAPES:
        for nbin in (128, 243, 256, 2048):
            got = lib.ppf_align_workspace_bytes(nsub, nchan, nbin)
            fits = [g for g in range(1, nsub + 1)
                    if up(g * nchan * (nbin // 2 + 1) * 16) +
                    up(g * nchan * 8) == got]
            assert fits == [A.partition(nsub, nchan)["ngroup"]], \
                (nsub, nchan, nbin, got)


# ------------------------------------------------------- the zero weights ---
@pytest.mark.parametrize("case", A.CASES, ids=A.case_id)
@pytest.mark.parametrize("only", [A.ALL_PATTERNS, A.REDUCED],
                         ids=["all", "reduced"])
def test_zero_patterns_leave_what_they_say(case, only):
    nsub, nchan = case
    p = A.partition(nsub, nchan)
    pats = A.zero_patterns(nsub, nchan, only)
    w = A.weights(nsub, nchan, only)
    assert w.shape == case and (w >= 0).all() and w.max() < 2.0
    chans = [q["chan"] for q in pats]
    assert len(set(chans)) == len(chans)
    assert 0 in chans and nchan - 1 in chans
    names = {q["name"] for q in pats}
    assert names == set(only) - ({"group"} if p["ngroup"] == 1 else set())
    for q in pats:
        n, z = q["chan"], np.flatnonzero(w[:, q["chan"]] == 0.0)
        assert list(z) == sorted(q["rows"]), q
        if q["wave"] is not None:
            rows = p["waves"][q["group"]][q["wave"]]
            assert len(rows) >= 2
            live = [s for s in rows if w[s, n] != 0.0]
            assert len(live) == q["live"], q
            want = dict(first=rows[1:], first2=rows[2:], wave=[],
                        last=rows[:-1],
                        middle=[s for s in rows if s != rows[len(rows) // 2]])
            assert live == want[q["name"]], q
        elif q["name"] == "group":
            s0, s1 = p["groups"][q["group"]]
            assert list(z) == list(range(s0, s1)) and q["live"] == 0
        elif q["name"] == "channel":
            assert len(z) == nsub and q["live"] == 0
        else:
            assert 0 < len(z) < nsub and q["live"] == nsub - len(z)
    # per-wave patterns sit in the first and in the last group
    if p["ngroup"] > 1 and "first" in only:
        assert {q["group"] for q in pats if q["name"] == "first"} == \
            {0, p["ngroup"] - 1}
    # every other channel keeps a live row; unpatterned ones keep them all
    dead = np.flatnonzero((w != 0.0).sum(axis=0) == 0)
    assert list(dead) == [q["chan"] for q in pats if q["name"] == "channel"]
    rest = np.setdiff1d(np.arange(nchan), chans)
    assert (w[:, rest] > 0.1).all()


def test_a_three_row_wave_has_a_true_middle_and_37_hits_the_ragged_group():
    p = A.partition(37, 1024)
    pats = A.zero_patterns(37, 1024)
    mids = [q for q in pats if q["name"] == "middle"]
    for q in mids:
        rows = p["waves"][q["group"]][q["wave"]]
        assert len(rows) == 3 and q["rows"] == [rows[1]]
    # the last group's target is wave 1 of 18 rows: 19 + 1, 28, 36
    assert [q["wave"] for q in mids] == [0, 1]
    assert p["waves"][1][1] == [20, 28, 36]


def test_inputs_are_what_the_device_tests_assume():
    x, ph, w = A.inputs((18, 1024), 256, "f32")
    assert x.dtype == np.float32 and x.shape == (18, 1024, 256)
    assert not x.flags.writeable and np.abs(ph).max() < 0.5
    x, ph, w = A.inputs((18, 1024), 256, "f64")
    # float64 rows that a float32 round trip would change
    assert x.dtype == np.float64 and (x.astype(np.float32) != x).mean() > 0.99
    bad = A.poisoned(x, w)
    assert np.isnan(bad[w == 0.0]).all() and np.isfinite(bad[w != 0.0]).all()
    assert (w == 0.0).sum() > 18


def test_align_reference_leaves_zero_weight_rows_out():
    """NaN rows of weight 0 do not reach the reference, and it is the plain
    rotate-then-sum of tests/test_gpu_parity.py on finite input."""
    import oracle as O
    rng = np.random.default_rng(2)
    nsub, nchan, nbin = 7, 5, 64
    x = rng.normal(size=(nsub, nchan, nbin))
    ph = rng.uniform(-0.5, 0.5, (nsub, nchan))
    w = rng.uniform(0.1, 2.0, (nsub, nchan))
    w[rng.random((nsub, nchan)) < 0.3] = 0.0
    w[:, 2] = 0.0
    plain = np.zeros((nchan, nbin))
    for s in range(nsub):
        plain += w[s][:, None] * O.rotate_rows(x[s], ph[s])
    ref = A.align_reference(A.poisoned(x, w), ph, w, chunk=2)
    assert np.isfinite(ref).all() and not ref[2].any()
    np.testing.assert_allclose(ref, plain, rtol=0, atol=1e-14)


# --------------------------------------------------- phases_reference ------
def test_phase_cases_cover_what_they_say():
    from pulseportraiture_amd import pplib
    assert pplib.Dconst == 1.0 / 0.000241        # ppf_device.hpp kDconst
    n = [ns * nc for ns, nc in A.PHASE_SHAPES]
    assert n[:4] == [1, A.K_BLOCK - 1, A.K_BLOCK, A.K_BLOCK + 1]
    assert n[4] == 2 * A.K_BLOCK + 1 and A.K_BLOCK % 171
    c = A.phase_case(7, 37)
    assert (c["DM"][0::3] > 0).all() and (c["DM"][1::3] < 0).all() and \
        (c["DM"][2::3] == 0.0).all()
    lo, hi = c["freqs"].min(axis=1), c["freqs"].max(axis=1)
    inside = (c["nu_ref"] > lo) & (c["nu_ref"] < hi)
    assert inside[0::2].all() and not inside[1::2].any()
    assert (c["nu_ref"][1::4] < lo[1::4]).all() and \
        (c["nu_ref"][3::4] > hi[3::4]).all()
    assert len(set(c["P"])) == 7 and len(set(c["phi"])) == 7
    assert not c["mask"].flat[0] and not c["mask"].flat[-1] and \
        c["mask"].any()
    res = A.results_rows(c["phi"], c["DM"], c["nu_ref"])
    assert np.isfinite(res).sum() == 3 * 7 and res.shape[1] == 32
    # the slow-pulsar variant keeps the dispersive term below a rotation
    s = A.phase_case(37, 1024, slow=True)
    ph, _ = A.phases_reference(s["phi"], s["DM"], s["P"], s["nu_ref"],
                               s["freqs"], s["scales"], s["errs"])
    assert np.abs(ph - s["phi"][:, None]).max() < 1.0


@pytest.mark.parametrize("shape", A.PHASE_SHAPES + ((37, 1024),),
                         ids=lambda s: "%dx%d" % s)
def test_phases_reference_against_float64(shape):
    """A check of the reference, not of the device: the longdouble formula
    against its direct float64 evaluation, within 4 ulp of the largest term
    (phases) and of the quotient (weights), and within the bars the device
    is held to in tests/test_gpu_align_groups.py."""
    c = A.phase_case(*shape, slow=shape == (37, 1024))
    ph, wt = A.phases_reference(c["phi"], c["DM"], c["P"], c["nu_ref"],
                                c["freqs"], c["scales"], c["errs"])
    assert ph.dtype == np.longdouble and \
        np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    p64, w64 = A.float64_phases(c)
    from pulseportraiture_amd import pplib
    Aa = (pplib.Dconst * np.abs(c["DM"]) / c["P"])[:, None]
    big = np.maximum(np.abs(c["phi"])[:, None],
                     Aa * np.maximum(c["freqs"] ** -2.0,
                                     c["nu_ref"][:, None] ** -2.0))
    dp = np.abs((p64 - ph).astype(np.float64))
    dw = np.abs((w64 - wt).astype(np.float64))
    bound = A.phase_bound(c["phi"], c["DM"], c["P"], c["nu_ref"], c["freqs"])
    print("ALIGN phases float64 %dx%d: worst |dev| / (4 ulp of the largest "
          "term) %.2f, / device bar %.2f, weights / (4 u) %.2f" %
          (shape + ((dp / (4 * A.U * big)).max(), (dp / bound).max(),
                    (dw / (4 * A.U * np.abs(w64))).max())))
    assert (dp <= 4 * A.U * big).all()
    assert (dp <= bound).all()
    assert (dw <= 4 * A.U * np.abs(w64)).all()
    # DM == 0: the phase is phi exactly
    z = c["DM"] == 0.0
    assert (ph[z] == c["phi"][z, None]).all()
    # masked entries are 0 and the others untouched
    mp, mw = A.phases_reference(c["phi"], c["DM"], c["P"], c["nu_ref"],
                                c["freqs"], c["scales"], c["errs"], c["mask"])
    assert (mp[~c["mask"]] == 0).all() and (mw[~c["mask"]] == 0).all()
    assert (mp[c["mask"]] == ph[c["mask"]]).all() and \
        (mw[c["mask"]] == wt[c["mask"]]).all() and mw[c["mask"]].all()
