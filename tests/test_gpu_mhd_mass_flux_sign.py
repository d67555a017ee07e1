"""GPU tests of the byte form of the mass-flux sign (AKMI_MF_BYTES, akmi_stage.hpp): on the fused 3-D MHD paths without
passive scalars the sweeps leave `(unsigned char)(mass flux >= 0.0)` per face instead of the mass flux, and k_corner_ct,
their only reader, tests the byte.  Results may not move by a bit, -0.0 counts as non-negative, and the paths on which
k_scalar_update reads the fluxes keep doubles.  Everything is compared bit for bit, ghost zones included: u0, the three
face fields and (time, dt).
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity_util as pu  # noqa: E402

MESHES = [
    # id, mesh, meshblock
    ("24x20x28", (24, 20, 28), (24, 20, 28)),       # several chunks of both marches, seven k-chunks of k_corner_ct, 60-cell
                                                    # waves end inside rows
    ("27x20x28", (27, 20, 28), (27, 20, 28)),       # byte rows of 31 and 32: no 4- or 8-byte alignment of a row
    ("32x16x16-2blocks", (32, 16, 16), 16),         # the per-block byte base
]
FIRST = MESHES[0]


class _Bare(str):
    """a deck value that parity_util's params (repr of the value) writes without quotes"""
    __repr__ = str.__str__


def _clock(sim, native):
    return (sim.time, sim.dt) if native else (sim.pmesh.time, sim.pmesh.dt)


def _modify(osim, nscalars, at_rest):
    """the oracle's state after its problem generator, changed in place (and its Initialize repeated): at rest = momenta to
    zero, everything else as generated; the scalars as in test_gpu_schemes.py.  Returns u0 for the product."""
    u = osim.array("u0")
    if at_rest:
        u[:, 1:4] = 0.0
    if nscalars:
        nf = u.shape[1] - nscalars
        prof = 0.5 + 0.25*np.sin(np.arange(u[:, 0].size, dtype=np.float64)*0.37).reshape(u[:, 0].shape)
        u[:, nf] = u[:, 0]*1.0
        u[:, nf + 1] = u[:, 0]*prof
    osim.reinitialize()
    return u


def _pair(mesh, mb, native, integrator="rk2", recon=None, ng=None, nscalars=0, at_rest=False):
    """product and oracle at the end of Initialize on identical data; the C++ host runs with every new form on"""
    kw = {}
    if nscalars:
        kw["extra"] = ["mhd/nscalars=%d" % nscalars]
    params = {"lean_prims": _Bare("true")} if native and recon is None and not nscalars else None
    sim, osim, _ = pu.make_pair("orszag_tang", mesh, 3, mb, fused=True, native=native, params=params, cfl=0.3,
                                integrator=integrator, recon=recon, ng=ng, **kw)
    if nscalars or at_rest:
        import torch
        u = _modify(osim, nscalars, at_rest)
        sim.phys.u0.copy_(torch.from_numpy(u.copy()))
        if native:
            sim.Initialize()
        else:
            sim.pdriver.Initialize(sim.pmesh, sim.pin)
    return sim, osim


@functools.lru_cache(maxsize=None)
def _oracle(mesh, mb, integrator, cycles, recon=None, ng=None, nscalars=0, at_rest=False):
    """the oracle's arrays and clock after `cycles` steps: computed once per case, shared, never written"""
    from athenak_amd.main import load_deck
    kw = {"extra": ["mhd/nscalars=%d" % nscalars]} if nscalars else {}
    deck, ov = pu.deck_overrides("orszag_tang", mesh, 3, mb, cfl=0.3, integrator=integrator, recon=recon, ng=ng, **kw)
    okw = pu.oracle_kwargs(load_deck(deck, ov))
    osim = pu.akref.Sim(**okw)
    osim.initialize()
    if nscalars or at_rest:
        _modify(osim, nscalars, at_rest)
    first = _first_stage_mass_fluxes(osim) if at_rest else None
    for _ in range(cycles):
        assert osim.step()
    out = {k: v.copy() for k, v in pu.oracle_arrays(osim, True).items()}
    for v in out.values():
        v.setflags(write=False)
    res = dict(arrays=out, clock=(osim.time, osim.dt), first=first)
    osim.close()
    return res


def _first_stage_mass_fluxes(osim):
    """mass fluxes of the first stage from the oracle's flux task (CPU), on the faces the CT-extended sweeps compute:
    per direction the numbers of positive, negative and exactly-zero ones"""
    L = osim.L
    pk = osim.pack()
    shp = {k: osim.array(k).shape for k in ("flx1", "flx2", "flx3", "e3x1")}
    f = [np.full(shp[k], np.nan) for k in ("flx1", "flx2", "flx3")]
    e = [np.zeros(shp["e3x1"]) for _ in range(6)]
    w0, bcc0 = osim.array("w0"), osim.array("bcc0")
    b = [osim.array(k) for k in ("b0x1f", "b0x2f", "b0x3f")]
    p = osim.params
    rc = L.akref_mhd_fluxes(C.byref(pk), p.recon, p.rsolver, pu.akref.ptr(w0), pu.akref.ptr(bcc0), *[pu.akref.ptr(x) for x in b],
                            *[pu.akref.ptr(x) for x in f], *[pu.akref.ptr(x) for x in e])
    assert rc == 0, rc
    counts = []
    for fx in f:
        d = fx[:, 0]
        d = d[~np.isnan(d)]
        counts.append((int((d > 0.0).sum()), int((d < 0.0).sum()), int((d == 0.0).sum())))
    return counts


def _run(mesh, mb, native, cycles, **kw):
    sim, osim = _pair(mesh, mb, native, **kw)
    osim.close()
    if native:
        assert sim.Execute(max_cycles=cycles) == cycles
    else:
        for _ in range(cycles):
            assert sim.Execute(max_cycles=1)
    got = dict(arrays=pu.product_arrays(sim), clock=_clock(sim, native))
    if native:
        got["forms"] = [sim.stage_forms(s) for s in range(1, {"rk2": 2, "rk3": 3}[kw.get("integrator", "rk2")] + 1)]
        sim.close()
    return got


def _check(got, want):
    print("clock", got["clock"], want["clock"])
    for k, v in want["arrays"].items():
        print(k, "differing values:", int((got["arrays"][k] != v).sum()), "of", v.size)
    assert got["clock"] == want["clock"], (got["clock"], want["clock"])
    for k, v in want["arrays"].items():
        assert np.array_equal(got["arrays"][k], v), k


RUN_CASES = [(m, "rk2") for m in MESHES] + [(FIRST, "rk3")]


@pytest.mark.parametrize("host", ["cxx", "python"])
@pytest.mark.parametrize("case", RUN_CASES, ids=lambda c: "%s-%s" % (c[0][0], c[1]))
def test_whole_run_against_oracle(case, host):
    """3 cycles of 3-D Orszag-Tang: the C++ host (u0 and face forms of the sweeps, out-of-place stages; rk3's second stage
    in place, i.e. the w0 form of the x3 march) and the Python host (old forms, stages in place) against the oracle"""
    (_, mesh, mb), integrator = case
    native = host == "cxx"
    got = _run(mesh, mb, native, 3, integrator=integrator)
    if native:
        assert got["forms"][0] & 1 and got["forms"][-1] & 1, got["forms"]       # capi.FORM_X3_U0: the new forms ran
    _check(got, _oracle(mesh, mb, integrator, 3))


@pytest.mark.parametrize("host", ["cxx", "python"])
def test_generic_sweeps_ppm4(host):
    """PPM4 with four ghost cells: the three generic sweeps (plain x1 sweep, x2 and x3 marches) with bytes"""
    _, mesh, mb = FIRST
    _check(_run(mesh, mb, host == "cxx", 3, recon="ppm4", ng=4), _oracle(mesh, mb, "rk2", 3, recon="ppm4", ng=4))


@pytest.mark.parametrize("host", ["cxx", "python"])
def test_passive_scalars_keep_doubles(host):
    """two passive scalars: k_scalar_update reads the three mass fluxes, so this path has to stay on doubles -- the scalars
    (and, through nothing else, the selection of the form) are compared with the oracle's"""
    _, mesh, mb = FIRST
    got = _run(mesh, mb, host == "cxx", 3, nscalars=2)
    want = _oracle(mesh, mb, "rk2", 3, nscalars=2)
    assert got["arrays"]["u0"].shape[1] == 7
    _check(got, want)


@pytest.mark.parametrize("case", MESHES, ids=lambda c: c[0])
def test_signed_zeros(case):
    """A state at rest with a non-uniform field (Orszag-Tang with the momenta set to zero): mass fluxes of both signs and
    exact zeros of both signs occur side by side.  `>= 0.0` takes -0.0 as non-negative; the sign bit or `> 0.0` would not."""
    _, mesh, mb = case
    want = _oracle(mesh, mb, "rk2", 2, at_rest=True)
    for d, (npos, nneg, nzero) in enumerate(want["first"]):
        print("x%d mass fluxes of the first stage: %d positive, %d negative, %d exactly zero" % (d + 1, npos, nneg, nzero))
    for d, (npos, nneg, nzero) in enumerate(want["first"]):
        assert npos > 0 and nneg > 0 and nzero > 0, (d, npos, nneg, nzero)
    _check(_run(mesh, mb, True, 2, at_rest=True), want)
