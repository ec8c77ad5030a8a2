"""CPU: the likelihood evaluators' goldens, bars and host-side validation.

The oracle (oracle.channel_terms / objective / gradient / hessian) is held to
the same goldens and the same bars as the device (tests/test_gpu_eval.py):
every per-channel term within 256 eps of its absolute companion, f, g and H
within 256 eps of their propagated scale (tests/evalcases.py).  Measured here
(error / (eps * scale), the largest over all cases and points): terms 105,
f / g / H 34 -- the rounding of k * phi_n in the reference's own phasor, which
the oracle forms with another association of the same products.
"""
import json
import os

import numpy as np
import pytest

import evalcases as E
import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = [E.case_name(*s) for s in E.SHAPES]


def _oracle_ratios(name, p):
    G = E.golden()
    rt = rf = 0.0
    for mode, lt in (("log", True), ("lin", False)):
        pre = "%s/%s/" % (name, mode)
        for i, th in enumerate(G[pre + "theta"]):
            t = O.channel_terms(th, p["D"], p["M"], p["errs_FT"], p["P"],
                                p["freqs"], *p["nus"], lt)
            rt = max(rt, E.terms_ratio(t, G[pre + "terms"][i],
                                       G[pre + "hat"][i]))
            rf = max(rf, E.ratio(O.objective(t), G[pre + "f"][i],
                                 G[pre + "sf"][i]),
                     E.ratio(O.gradient(t, E.FLAGS_A), G[pre + "g"][i],
                             G[pre + "sg"][i]),
                     E.ratio(O.hessian(t, E.FLAGS_A), G[pre + "H"][i],
                             G[pre + "sH"][i]),
                     E.ratio(O.gradient(t, E.FLAGS_B), G[pre + "gB"][i],
                             G[pre + "sg"][i]),
                     E.ratio(O.hessian(t, E.FLAGS_B), G[pre + "HB"][i],
                             G[pre + "sH"][i]))
    return rt, rf


@pytest.mark.parametrize("shape", E.SHAPES, ids=NAMES)
def test_oracle_within_the_device_bars(shape):
    p = E.inputs(*shape)
    name = E.case_name(*shape)
    assert str(E.golden()[name + "/sha"]) == E.input_sha(p)
    rt, rf = _oracle_ratios(name, p)
    print("%s: oracle terms %.1f, f/g/H %.1f (x eps x scale)" % (name, rt, rf))
    assert rt <= E.BAR_EPS and rf <= E.BAR_EPS


def test_oracle_batch_problems_within_bars():
    probs, _ = E.batch_inputs()
    G = E.golden()
    for s, p in enumerate(probs):
        assert str(G["batch%d/sha_full" % s]) == E.input_sha(p)
        ok = np.array(E.BATCH["mask"][s], dtype=bool)
        q = dict(p, D=p["D"][ok], M=p["M"][ok], errs_FT=p["errs_FT"][ok],
                 freqs=p["freqs"][ok])
        rt, rf = _oracle_ratios("batch%d" % s, q)
        assert rt <= E.BAR_EPS and rf <= E.BAR_EPS


def test_generator_conditions():
    """No golden value is non-finite; nu_tau sits on no channel; at the near
    points |C_n| >= 0.1 C^_n in every channel; every term is bounded by its
    companion; tau = 0 points carry exact zeros."""
    G = E.golden()
    for k, v in G.items():
        if v.dtype.kind in "fc":
            assert np.all(np.isfinite(v)), k
    for shape in E.SHAPES:
        p = E.inputs(*shape)
        name = E.case_name(*shape)
        assert np.all(p["freqs"] != p["nus"][2])
        C, Ch = G[name + "/log/terms"][:3, 0], G[name + "/log/hat"][:3, 0]
        assert np.all(np.abs(C) >= 0.1 * Ch), name
        for mode in ("log", "lin"):
            t, h = G["%s/%s/terms" % (name, mode)], G["%s/%s/hat" % (name, mode)]
            assert np.all(np.abs(t) <= h.astype(float) * (1 + 1e-6) + 1e-300)
        th = G[name + "/lin/theta"]
        assert np.all(th[2:, 3] == 0.0) and np.all(th[:2, 3] > 0.0)
        z = E.unpack_terms(G[name + "/lin/terms"][2])
        for key in ("dC", "dS"):
            assert np.all(z[key][3:] == 0.0)
        assert np.all(z["d2C"][3:] == 0.0) and np.all(z["d2S"] == 0.0)
        assert np.all(G[name + "/lin/g"][2:, 3:] == 0.0)
    th = G["c64x33/log/theta"]
    assert np.abs(th[3:, 0] - th[0, 0]).max() > 0.4          # |phi| far
    assert th[3:, 3].min() <= -4.0 and th[3:, 3].max() >= np.log10(0.3)


def test_golden_file_size_and_manifest():
    assert os.path.getsize(E.GOLDEN) < (1 << 20)
    with open(os.path.join(HERE, "golden", "MANIFEST_eval.json")) as f:
        m = json.load(f)
    assert m["eval"]["file"] == "eval.npz"
    assert m["eval"]["bytes"] == os.path.getsize(E.GOLDEN)
    assert set(NAMES) <= set(m["eval"]["cases"])


def test_public_names_exist():
    from pulseportraiture_amd import pplib, pptoaslib, engine
    for n in ("fit_portrait_full_function", "fit_portrait_full_function_deriv",
              "fit_portrait_full_function_2deriv",
              "fit_portrait_full_function_2deriv_with_scales",
              "eval_portrait_full"):
        assert callable(getattr(pptoaslib, n)), n
    for n in ("fit_portrait_function", "fit_portrait_function_deriv",
              "fit_portrait_function_2deriv", "fit_phase_shift_function",
              "fit_phase_shift_function_deriv",
              "fit_phase_shift_function_2deriv"):
        assert callable(getattr(pplib, n)), n
    assert callable(engine.eval_points)


def test_entry_validates_without_gpu():
    """PPF_EINVAL before anything touches the device; the workspace query
    returns 0 for a bad shape."""
    from pulseportraiture_amd import _lib
    lib = _lib.load()
    assert lib.ppf_eval_point_block() >= 1
    assert lib.ppf_eval_harm_tile() % 64 == 0
    assert lib.ppf_eval_harm_tile() // 64 <= 64       # recurrence <= 64 steps
    assert lib.ppf_eval_workspace_bytes(2, 64, 9, 2) >= 2 * 64 * 9 * 21 * 8
    assert lib.ppf_eval_workspace_bytes(2, 64, 9, 0) >= 2 * 64 * 9 * 8
    for bad in ((0, 64, 9, 2), (2, 0, 9, 2), (2, 64, 0, 2), (2, 64, 9, 3),
                (2, 64, 9, -1)):
        assert lib.ppf_eval_workspace_bytes(*bad) == 0, bad
    rc = lib.ppf_eval_batch(None, 1, 4, 17, 1, None, None, 1, *[None] * 8,
                            1, 2, *[None] * 5, 0, None)
    assert rc == _lib.PPF_EINVAL


def test_wrong_shapes_raise_value_error_before_any_launch():
    """Shape errors are ValueErrors raised on the host arrays' shapes alone:
    they come before the device is looked for (no GPU here)."""
    from pulseportraiture_amd import pptoaslib
    p = E.inputs(3, 17)
    a = (p["D"], p["M"], p["errs_FT"], p["P"], p["freqs"]) + tuple(p["nus"])
    th = np.zeros((2, 5))

    def call(theta=th, D=a[0], M=a[1], e=a[2], fr=a[4], **kw):
        return pptoaslib.eval_portrait_full(theta, D, M, e, a[3], fr, *a[5:],
                                            **kw)
    for kw in (dict(theta=np.zeros((2, 4))), dict(theta=np.zeros(5)),
               dict(M=a[1][:, :-1]), dict(M=a[1][:2]), dict(e=a[2][:2]),
               dict(fr=a[4][:1]), dict(D=a[0][:, :1], M=a[1][:, :1]),
               dict(order=3), dict(mask=np.ones(2)),
               dict(fit_flags=(1, 1, 1)), dict(model_index=[1]),
               dict(theta=np.zeros((2, 2, 5)))):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):
        pptoaslib.fit_portrait_full_function(
            np.zeros(5), a[0], a[1][:, :-1], *a[2:], (1, 1, 1, 1, 1), True)
