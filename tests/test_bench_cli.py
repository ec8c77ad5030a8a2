"""bench.py's options that need no device: --full / --dump-outputs parsing
and the size limit of the dumped arrays."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _parse(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not a.full and a.dump_outputs is None
    assert (a.steps, a.warmup, a.fit) == (7, 3, "phase+DM")
    a = _parse(monkeypatch, ["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


@pytest.mark.parametrize("fit", ["gettoas", "single"])
def test_dump_outputs_refused_where_no_records_exist(monkeypatch, fit):
    with pytest.raises(SystemExit) as e:
        _parse(monkeypatch, ["--fit", fit, "--dump-outputs", "d"])
    assert e.value.code == 2


def test_dump_outputs_writes_float64_within_the_limit(tmp_path, monkeypatch):
    """Below the limit every row is written; above it the arrays share the
    limit in proportion, each keeping the same sorted sample of its rows on
    every call."""
    rng = np.random.default_rng(1)
    res = rng.standard_normal((1000, 32))
    tmpl = rng.standard_normal((64, 128)).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "a"), dict(results=res, template=tmpl))
    assert sorted(os.listdir(tmp_path / "a")) == ["results.npy",
                                                  "template.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "results.npy"), res)
    t = np.load(tmp_path / "a" / "template.npy")
    assert t.dtype == np.float64
    np.testing.assert_array_equal(t, tmpl.astype(np.float64))
    assert bench.DUMP_MAX_BYTES == 64 << 20
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", (res.nbytes + 8 * tmpl.size) // 4)
    for d in "bc":
        bench.dump_outputs(str(tmp_path / d), dict(results=res, template=tmpl))
    b = np.load(tmp_path / "b" / "results.npy")
    assert b.shape == (250, 32)
    # the sample: rows of the input, in their order
    idx = [int(np.flatnonzero((res == r).all(axis=1))[0]) for r in b]
    assert idx == sorted(set(idx))
    assert np.load(tmp_path / "b" / "template.npy").shape == (16, 128)
    for n in ("results.npy", "template.npy"):
        np.testing.assert_array_equal(np.load(tmp_path / "b" / n),
                                      np.load(tmp_path / "c" / n))
