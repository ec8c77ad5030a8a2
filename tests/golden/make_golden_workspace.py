#!/usr/bin/env python
"""Golden table of ppf_fit_workspace_bytes: the exact byte count of the fit
workspace over a grid of descriptors (fit_workspace.json, checked byte for
byte by tests/test_abi.py).  The query needs no device.

The table pins the workspace layout against refactors of fit_layout, so it is
generated from a build of the commit BEFORE the change under test, never from
the tree being tested:

    PPFIT_LIB=/path/to/parent/pulseportraiture_amd/lib/libppfit.so \\
        python tests/golden/make_golden_workspace.py

Each entry is [nbin, nchan, nsub, nmodel, guess, guess_Ns, options,
x_subints, bytes].
"""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from pulseportraiture_amd import _lib  # noqa: E402

NBIN = (64, 1000, 1001, 1024, 2048, 4096, 8194, 16384)
NCHAN = (1, 33, 512)
NSUB = (1, 10)
NMODEL = (1, 3)
GUESS = ("off", 100, "nbin")          # off, guess_Ns = 100, guess_Ns = nbin
OPTIONS = (0, _lib.OPT_NO_X, _lib.OPT_MOM_X, _lib.OPT_FUSED_MOM)
X_SUBINTS = (0, 2)


def grid():
    for nbin, nchan, nsub, nmodel, g, opt, xs in itertools.product(
            NBIN, NCHAN, NSUB, NMODEL, GUESS, OPTIONS, X_SUBINTS):
        guess = 0 if g == "off" else 1
        guess_Ns = 0 if g == "off" else (nbin if g == "nbin" else g)
        yield nbin, nchan, nsub, nmodel, guess, guess_Ns, opt, xs


def workspace_bytes(lib, nbin, nchan, nsub, nmodel, guess, guess_Ns, options,
                    x_subints):
    d = _lib.FitDesc()
    d.nbin, d.nchan, d.nsub, d.nmodel = nbin, nchan, nsub, nmodel
    d.guess, d.guess_Ns = guess, guess_Ns
    d.options, d.x_subints = options, x_subints
    return int(lib.ppf_fit_workspace_bytes(ctypes.byref(d)))


def main():
    lib = _lib.load()
    entries = [list(g) + [workspace_bytes(lib, *g)] for g in grid()]
    out = os.path.join(HERE, "fit_workspace.json")
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, separators=(",", ":"))
                                   for e in entries) + "\n]\n")
    print("%d entries from %s -> %s" % (len(entries), _lib.LIB_PATH, out))


if __name__ == "__main__":
    main()
