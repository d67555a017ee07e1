"""Shared by tests/test_coarsen_host.py (no GPU), tests/test_gpu_coarsen.py and tests/golden/make_cbin_fixtures.py: the CPU
build of the coarsening arithmetic (tests/host_shim/coarsen_host.cpp), a CPU backend that adds it to the oracle-as-akmi
stand-in, the wide-range synthetic fields, what a Simulation's coarsen() has to return (restated from its arrays) and the
deck of the committed .cbin fixture."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import coarsen_restate as R  # noqa: E402

SHIM = os.path.join(ROOT, "tests", "host_shim")
SO = os.path.join(SHIM, "libcoarsen_host.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "cbin_fixture.cbin")
FIXTURE_NPZ = os.path.join(GOLDEN, "cbin_reader.npz")
U = 2.0**-53


def build_shim():
    src = os.path.join(SHIM, "coarsen_host.cpp")
    csrc = os.path.join(ROOT, "athenak_amd", "csrc")
    deps = [src, os.path.join(csrc, "akmi_coarsen.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        # -ffp-contract=off: products and sums rounded separately, as in the device build
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", SHIM, "-I", csrc,
                               src, "-o", SO])
    return C.CDLL(SO)


def install_cpu_backend():
    """tests/cpu_backend.py plus the derived variables and akmi_coarsen from the CPU builds"""
    import cpu_backend
    import derived_cases as dc
    from athenak_amd import capi
    H, D = build_shim(), dc.build_shim()

    class Backend(cpu_backend.OracleAsAkmi):
        def akmi_derived_var(self, *args):
            return D.hd_derived_var(*args[:-1])

        def akmi_derived_ncomp(self, which):
            return D.hd_derived_ncomp(which)

        def akmi_coarsen(self, *args):
            return H.hc_coarsen(*args[:8])               # without staged and stream

    capi._LIB = Backend()
    capi.DEVICE = "cpu"


def uninstall_cpu_backend():
    import cpu_backend
    cpu_backend.uninstall()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def wide_field(shape, seed):
    """signed values of magnitude 1e-150 ... 1e150 (x^4 overflows to inf and underflows to 0), with one NaN and one -0.0
    planted at seeded places; returns (array, index of the NaN, index of the -0.0)"""
    rng = np.random.default_rng(seed)
    a = 10.0**rng.uniform(-150.0, 150.0, shape)*rng.choice([-1.0, 1.0], shape)
    flat = rng.choice(a.size, size=2, replace=False)
    at_nan, at_zero = (tuple(int(v) for v in np.unravel_index(q, shape)) for q in flat)
    a[at_nan] = np.nan
    a[at_zero] = -0.0
    return a, at_nan, at_zero


def assert_same_bits(got, want, what):
    """NaN where the restatement has NaN (whatever the payload), the same bits everywhere else"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN positions differ", int(np.isnan(got).sum()), int(nan.sum()))
    bad = (got.view(np.uint64) != want.view(np.uint64)) & ~nan
    assert not bad.any(), "%s: %d of %d values differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def _np(t):
    return t.detach().cpu().numpy()


def fine_arrays(sim, variable):
    """(outvars, list of (nmb, N3, N2, N1) numpy arrays): the fine data of every variable of an output group"""
    from athenak_amd import outputs
    pk = sim.pmesh.pmb_pack
    phys = sim.phys
    ov = outputs._outvars(variable, pk.pmhd is not None, phys.peos.eos_data.is_ideal,
                          getattr(pk, "pturb", None) is not None, getattr(phys, "nscalars", 0))
    arrays = []
    for (_, comp, arr) in ov:
        if arr.startswith("dv:"):
            arrays.append(_np(sim.derived(variable))[:, 0])
        elif arr == "force":
            arrays.append(_np(pk.pturb.force)[:, comp])
        else:
            arrays.append(_np(getattr(phys, arr))[:, comp])
    return ov, arrays


def output_range(sim, f, ghost_zones):
    """(lo, nc) of a cbin output without slices: first fine cell and coarse extents"""
    ind = sim.pmesh.mb_indcs
    n3, n2, n1 = ind.ncells if ghost_zones else (ind.nx3, ind.nx2, ind.nx1)
    lo = (0, 0, 0) if ghost_zones else (ind.is_, ind.js, ind.ks)
    assert n1 % f == 0 and n2 % f == 0 and n3 % f == 0
    return lo, (n1//f, n2//f, n3//f)


def restated(sim, variable, f, moments, ghost_zones=False):
    """(labels, array) that sim.coarsen(variable, f, moments, ghost_zones) has to return"""
    ov, arrays = fine_arrays(sim, variable)
    lo, nc = output_range(sim, f, ghost_zones)
    sfx = ("_1st", "_2nd", "_3rd", "_4th") if moments else ("",)
    return [lab + s for (lab, _, _) in ov for s in sfx], R.restate_vars(arrays, f, lo, nc, moments)


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


# ---- the committed fixture: 16^3 in 8^3 blocks, mhd_bcc, f = 2, moments -------------------------------------------
def fixture_deck():
    import output_cases as oc
    text = oc.OT_DECK.replace("FUSED", "false").replace("nx3 = 8\nx3min", "nx3 = 16\nx3min")
    text = text[:text.index("<output1>")]
    return text + "<output1>\nfile_type = cbin\nvariable = mhd_bcc\ncoarsen_factor = 2\ncompute_moments = true\ndcycle = 1\n"


FIXTURE_NAME = os.path.join("cbin_mhd_bcc_2", "OrszagTang.mhd_bcc.00000.cbin")


def write_fixture(workdir):
    """the fixture's run (CPU backend installed by the caller): two cycles, one output; (sim, path of the file)"""
    import derived_cases as dc
    sim = dc.run_and_write(fixture_deck(), workdir, cycles=2)
    return sim, os.path.join(workdir, FIXTURE_NAME)
