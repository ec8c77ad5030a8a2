"""tests/golden/fake.npz (make_golden_fake.py): the reference-composed
noiseless rows of make_fake_pulsar and their per-row tables, and the host
tables of the same cases from pulseportraiture_amd.fake."""
import os

import numpy as np

from pulseportraiture_amd import fake

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAR = os.path.join(GOLDEN, "example.par")
GMODEL = os.path.join(GOLDEN, "example.gmodel")
Z = np.load(os.path.join(GOLDEN, "fake.npz"))
CASES = [str(c) for c in Z["cases"]]


def golden(case, key):
    return Z["%s__%s" % (case, key)]


def has(case, key):
    return "%s__%s" % (case, key) in Z.files


def case_kwargs(case):
    """make_fake_pulsar / fake_tables keyword arguments of a golden case."""
    g = lambda k: golden(case, k)       # noqa: E731
    kw = dict(nchan=int(g("nchan")), nbin=int(g("nbin")), nu0=float(g("nu0")),
              bw=float(g("bw")), phase=float(g("phase")), dDM=float(g("dDM")),
              t_scat=float(g("t_scat")), alpha=float(g("alpha")),
              scales=g("scales"))
    if has(case, "scint"):
        kw["scint"] = list(g("scint"))
    if has(case, "xs"):
        kw.update(xs=list(g("xs")), Cs=list(g("Cs")),
                  nu_DM=float(g("nu_DM")))
    return kw


def case_tables(case, noise_stds=0.0):
    """(par, epochs, tables) of a golden case: one sub-int that starts at
    PEPOCH."""
    par = fake.read_par(PAR)
    ep = fake.fake_epochs(par, 1, float(golden(case, "tsub")))
    tab = fake.fake_tables(float(golden(case, "model_tau")), par.DM, ep.Ps,
                           noise_stds=noise_stds, **case_kwargs(case))
    return par, ep, tab
