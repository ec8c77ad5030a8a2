"""Host checks of the degenerate-input cases (tests/degenerate.py): the
routines the device shares with the host return on non-finite input, the
poison touches only masked channels and reaches the paths it is meant for,
the oracle rejects the N and Z sub-ints, and the minimal-channel fits are
well posed.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import degenerate as D
import goldens as G
import ragged as R

TESTS = os.path.dirname(os.path.abspath(__file__))

_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import degenerate as D
for label, call in D.termination_calls():
    if not label.startswith(%r):
        continue
    print(label, flush=True)
    print("rc", call(), flush=True)
"""


@pytest.mark.parametrize("group", ["roots", "subproblem"])
def test_shared_routines_return_on_nonfinite_input(group):
    """ppf_poly_real_roots_host (degrees 1..8) and ppf_tr_subproblem_host
    (n 1..5) with a NaN, +Inf or -Inf in the leading entry, the trailing
    one or all of them (coefficients; H, g, R) return a count, -1 or a
    negative code.  k_postfit runs the same code (ppf_device.hpp) on a
    PPF_ST_NONFINITE sub-int.  The calls run in a child process under a time
    limit, so that a loop that never ends fails here instead of hanging.

    Why each loop ends:
    - balance_small.  NaN: c or r NaN makes `c < g`, `c > g` and
      `(c + r) / f < 0.95 s` false, so nothing is scaled and `last` stays 1.
      r = Inf beside a finite c: `c < g` quadruples c until it is Inf (at
      most 540 trips), then Inf < Inf is false.  c = Inf beside a finite r
      was the one that spun: `while (c > g) c /= 4` keeps c = Inf.  The
      companion matrix has c = Inf, r = 1 in column j whenever coefficient
      j >= 1 is Inf beside a finite leading one ([1, .3, Inf, 2] never
      returned).  Rows and columns with a non-finite norm are now left
      unscaled; finite norms take the branch as before, so healthy input
      gives the same bits.  With finite norms every trip of the outer
      `while (last == 0)` loop that goes round again has shrunk c + r by
      more than 5 % at a power-of-two factor: the textbook argument.
    - hqr_small.  Each trip of the inner do-loop either deflates one or two
      eigenvalues (nn falls) or counts `its` up; at its == 60 it returns
      false (-1).  NaN entries make `fabs(a[l][l-1]) + s == s` false, so l
      runs down to 0 and the same two cases apply.  All other loops run over
      matrix indices.
    - tr_exact.  sym_eig_jacobi: at most 40 sweeps; the secular iteration:
      at most 100 trips.  ppf_tr_subproblem_host refuses R that is not > 0
      (NaN, -Inf) with -1."""
    code = _CHILD % (os.path.dirname(TESTS), TESTS, group)
    try:
        out = subprocess.run([sys.executable, "-c", code], cwd=TESTS,
                             capture_output=True, text=True, timeout=20)
    except subprocess.TimeoutExpired as e:
        lines = (e.stdout or b"").decode().splitlines() \
            if isinstance(e.stdout, bytes) else (e.stdout or "").splitlines()
        pytest.fail("no return from: %s" % (lines[-1] if lines else "?"))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    want = [l for l, _ in D.termination_calls() if l.startswith(group)]
    assert lines[0::2] == want
    assert len(want) == (8 * 9 if group == "roots" else 5 * 3 * 7)
    for label, rc in zip(lines[0::2], lines[1::2]):
        rc = int(rc.split()[1])
        if group == "roots":
            assert -2 <= rc <= 8, (label, rc)
        else:
            assert rc in (0, 1, -1), (label, rc)
            if " R " in label and not label.endswith(" inf"):
                assert rc == -1, (label, rc)


def test_root_finder_is_unchanged_on_finite_input():
    """The guard in balance_small leaves finite polynomials alone: roots of
    badly scaled coefficients (the balancing does scale them) are numpy's."""
    from pulseportraiture_amd import _lib
    rng = np.random.default_rng(11)
    for deg in range(2, 9):
        co = rng.normal(size=deg + 1) * 10.0 ** rng.integers(-6, 7, deg + 1)
        got = np.sort(_lib.poly_real_roots(co))
        r = np.roots(co)
        want = np.sort(r[r.imag == 0].real)
        assert len(got) == len(want), (deg, got, want)
        np.testing.assert_allclose(got, want, rtol=1e-9)


# ---------------------------------------------------------------------------
# A
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_poison_touches_only_masked_channels(name):
    c = R.case(name)
    b = R.inputs(c)
    keep = b["keep"]
    assert keep[0].all() and not keep[1:].all(axis=1).any()
    for v in D.VARIANTS:
        o = D.poisoned(c, v)
        for i in range(b["nsub"]):
            np.testing.assert_array_equal(o["data"][i][keep[i]],
                                          b["data"][i][keep[i]])
            rows = o["data"][i][~keep[i]]
            if v == 1:
                assert np.isnan(rows).all()
            elif v == 2:
                assert (rows[:, 0] == np.inf).all()
                assert (rows[:, -1] == -np.inf).all()
                assert np.isnan(rows[:, c["nbin"] // 2]).all()
                assert np.isfinite(rows).sum() == rows.size - 3 * len(rows)
            else:
                assert (rows == D.huge(c)).all()
                # the constant survives the cast to the rows' format
                assert np.isfinite(rows.astype(
                    np.float32 if c["dtype"] == "f32" else np.float64)).all()
        assert ("errs" in o) == (b["errs"] is not None)
        if "errs" in o:
            np.testing.assert_array_equal(o["errs"][keep], b["errs"][keep])
            bad = o["errs"][~keep]
            assert np.isnan(bad).all() if v == 1 else (bad == 0.0).all()
        assert ("guess_weights" in o) == c["guess"]
        if c["guess"]:
            assert (o["guess_weights"][keep] == 1.0).all()
            bad = o["guess_weights"][~keep]
            assert np.isnan(bad).all() if v == 1 else (bad == 0.0).all()
    # a masked channel in the last, partial tile, and a masked last row of
    # a 32- and of a 64-channel block beside a live row of the block
    last = (c["nchan"] - 1) // 32 * 32
    assert (~keep[:, last:]).any()
    assert D.block_last_masked(keep, 32) and D.block_last_masked(keep, 64)


def test_block_last_masked():
    k = np.ones((1, 70), dtype=bool)
    assert not D.block_last_masked(k, 32)
    k[0, 31] = False
    assert D.block_last_masked(k, 32) and not D.block_last_masked(k, 64)
    k[0, :32] = False                       # no live row left in that block
    assert not D.block_last_masked(k, 32)
    k[0, 69] = False                        # the band's last channel
    assert D.block_last_masked(k, 32) and D.block_last_masked(k, 64)


# ---------------------------------------------------------------------------
# B
# ---------------------------------------------------------------------------
def test_degenerate_families():
    assert len(D.FAMILIES) == 12 and set(D.FAMILIES) <= set(R.CASE_NAMES)
    fam = [R.case(n)["family"] for n in D.FAMILIES]
    # ("swz" has no kernel of its own: the other families' spectrum kernels
    # at 256 channels, on the swizzled block map)
    assert set(fam) == {c["family"] for c in R.CASES} - {"swz"}
    for n in D.SCIPY + D.ONLY + (D.NO_X,):
        assert n in R.CASE_NAMES
    c = R.case(D.NO_X)
    assert c["guess"] and c["nbin"] == 2048 and c["flags"] == R.PD
    moment, scat = (R.inputs(R.case(n))["scat"] for n in D.ONLY)
    assert not moment and scat


@pytest.mark.parametrize("name", D.FAMILIES)
def test_degenerate_batch(name):
    c = R.case(name)
    b = R.inputs(c)
    subs, o = D.degenerate(c)
    assert subs == [0, 0, 0, 1, 0, 2, 0, 3, 0]
    keep, data, flags = o["mask"], o["data"], o["flags"]
    assert flags.shape == (9, 5)
    for j, k in enumerate(D.ORDER):
        src = b["data"][subs[j]]
        if k[0] == "s":
            np.testing.assert_array_equal(data[j], src)
            np.testing.assert_array_equal(keep[j], b["keep"][subs[j]])
            continue
        assert keep[j].any() == (k not in ("E", "E2"))
        assert keep[j].all() or not keep[j].any()
        assert tuple(flags[j]) == ((0,) * 5 if k == "F" else c["flags"])
        bad = ~np.isfinite(data[j])
        if k == "E2":
            assert bad.all()
        elif k == "N":
            n = D.nan_channel(c)
            assert bad.sum() == 1 and bad[n, D.NAN_BIN]
            assert n >= (c["nchan"] - 1) // 32 * 32     # the last block
        else:
            assert not bad.any()
        if k == "Z":
            z = D.zero_channel(c)
            if b["errs"] is None:
                assert not data[j, z].any() and data[j, z - 1].any()
            else:
                np.testing.assert_array_equal(data[j], src)
                assert o["errs"][j, z] == 0.0
                assert (np.delete(o["errs"][j], z) > 0.0).all()
        elif k not in ("N", "E2"):
            np.testing.assert_array_equal(data[j], src)


@pytest.mark.parametrize("kind", ["N", "Z"])
@pytest.mark.parametrize("name", D.FAMILIES)
def test_oracle_rejects_nonfinite_subints(name, kind):
    """The reference has no outcome for the N and Z sub-ints: SciPy raises
    from its finiteness check.  The device ends them with PPF_ST_NONFINITE
    (test_gpu_degenerate.py)."""
    with np.errstate(all="ignore"), pytest.raises(
            ValueError, match="must not contain infs or NaNs"):
        D.oracle_degenerate(R.case(name), kind)


# ---------------------------------------------------------------------------
# C
# ---------------------------------------------------------------------------
def test_minimal_placements():
    assert [D.MINIMAL[n]["nchan"] for n in D.MINIMAL_NAMES] == \
        [33, 37, 45, 33, 3, 1]
    assert [D.MINIMAL[n]["nbin"] for n in D.MINIMAL_NAMES] == \
        [2048, 512, 1000, 1001, 512, 512]
    for name in D.MINIMAL_NAMES:
        m = D.minimal(name)
        nchan = m["c"]["nchan"]
        ones = [j for j in range(m["nsub"]) if m["keep"][j].sum() == 1]
        twos = [j for j in range(m["nsub"]) if m["keep"][j].sum() == 2]
        assert len(ones) + len(twos) == m["nsub"]
        for j in ones:
            assert tuple(m["flags"][j]) == D.P_ONLY
        for j in twos:
            assert tuple(m["flags"][j]) == R.PD
        if nchan == 1:
            assert len(ones) == 2 and not twos
            continue
        assert {int(np.flatnonzero(m["keep"][j])[0]) for j in ones} == \
            {0, nchan - 1, nchan // 2}
        assert {tuple(np.flatnonzero(m["keep"][j])) for j in twos} == \
            {(0, 1), (nchan - 2, nchan - 1), (0, nchan - 1)}


@pytest.mark.parametrize("name", D.MINIMAL_NAMES)
def test_minimal_fits_are_well_posed(name):
    """test_ragged_inputs.py's probe on every minimal sub-int: the oracle
    converges (return code 2) and, restarted 1e-2 sigma away, lands within
    1e-3 sigma of its solution."""
    m = D.minimal(name)
    for j in range(m["nsub"]):
        o = D.minimal_oracle(name, j)
        k = m["keep"][j]
        assert o["return_code"] == 2, (name, j, o["return_code"])
        assert len(o["scales"]) == k.sum()
        assert o["dof"] == k.sum() * (m["c"]["nbin"] - 1) - m["flags"][j].sum()
        o2 = D.minimal_refit(name, j, o)
        assert o2["return_code"] == 2, (name, j)
        dev = G.param_deviation_sigma(o2, o, m["P"], False)
        print("MINIMAL %s sub %d kept %s: restart moves %.1e sigma" %
              (name, j, np.flatnonzero(k), dev.max()))
        assert dev.max() < 1e-3, (name, j, dev)
