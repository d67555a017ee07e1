"""not gpu: two-fluid (ion-neutral) MHD on the host -- the ImEx tables, the properties of the three-pass restatement
the GPU tests compare the kernel with (tests/ionn_restate.py), the deck refusals and the C-shock ODE profile."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ionn_restate as R  # noqa: E402

INTEGRATORS = ("imex2", "imex2+", "imex3")


def _deck(extra=(), drop=()):
    """the oblique C-shock deck without its output blocks, blocks of `drop` removed, "block/name=value" of `extra` added"""
    from athenak_amd.parameter_input import ParameterInput
    text = open(os.path.join(ROOT, "athenak_amd", "inputs", "cshock.athinput")).read()
    text = text[:text.index("<output1>")]
    for blk in drop:
        a = text.index("<%s>" % blk)
        b = text.index("\n<", a + 1)
        text = text[:a] + text[b + 1:]
    for e in extra:
        blk, rest = e.split("/", 1)
        if "<%s>" % blk in text:
            name = rest.split("=")[0].strip()
            a = text.index("<%s>" % blk)
            b = text.find("\n<", a + 1)
            body = "\n".join(l for l in text[a:b].split("\n") if l.split("=")[0].strip() != name)
            text = text[:a] + body + "\n" + rest + "\n" + text[b:]
        else:
            text += "\n<%s>\n%s\n" % (blk, rest)
    return ParameterInput(text=text)


# ---- the tables ------------------------------------------------------------------------
@pytest.mark.parametrize("integ", INTEGRATORS)
def test_driver_tables_equal_the_literals(integ):
    from athenak_amd.driver import Driver
    d = Driver(_deck(["time/integrator=" + integ]), None)
    t = R.tables(integ)
    assert (d.nimp_stages, d.nexp_stages, d.cfl_limit) == (t["nimp_stages"], t["nexp_stages"], 1.0)
    assert d.gam0 == t["gam0"] and d.gam1 == t["gam1"] and d.beta == t["beta"]
    assert d.a_twid == t["a_twid"] and d.a_impl == t["a_impl"] and d.gamma == t["gamma"]
    # stage 1 keeps u0 (it has been through two implicit stages), not u1
    assert (d.gam0[0], d.gam1[0]) == (1.0, 0.0)


def test_table_values():
    """a few entries as plain numbers, so that the two statements of the tables cannot be wrong together"""
    t2, tp, t3 = R.tables("imex2"), R.tables("imex2+"), R.tables("imex3")
    assert t2["a_twid"][:3] == [[-1.0, 0.0, 0.0, 0.0], [0.5, 0.0, 0.0, 0.0], [0.0, 0.25, 0.25, 0.0]] and t2["a_impl"] == 0.5
    g = 1.707106781186547
    assert tp["a_impl"] == g and tp["beta"][:3] == [g, 1.0/(2.0*g), 0.0]
    nz = [(r, c) for r in range(4) for c in range(4) if tp["a_twid"][r][c] != 0.0]
    assert nz == [(2, 2)] and abs(tp["a_twid"][2][2] - (-1.4142135623730945)) < 1e-14
    a = 0.24169426078821
    assert t3["a_impl"] == a and t3["a_twid"][0][0] == -2.0*a and t3["a_twid"][3][3] == 2.0*(1.0 - a)/3.0
    assert abs(t3["a_twid"][3][3] - 0.5055371594745267) < 1e-15 and abs(t3["a_twid"][2][1] - (-0.0604235651970475)) < 1e-15


# ---- the uniform drag ODE --------------------------------------------------------------
_RI, _RN = 0.3, 1.7


def _cell():
    ui = np.array([[[_RI], [_RI*1.5], [_RI*-0.5], [_RI*0.25]]])
    un = np.array([[[_RN], [_RN*-1.0], [_RN*2.0], [_RN*0.75]]])
    return ui, un


def _dv(ui, un):
    return ui[0, 1:, 0]/ui[0, 0, 0] - un[0, 1:, 0]/un[0, 0, 0]


def _drag_error(integ, lam_dt, drag=1.0):
    """one cell, no fluxes, to t = 1/lambda: max error of v_i - v_n against exp(-gamma (rho_i + rho_n) t)"""
    tab = R.tables(integ)
    lam = drag*(_RI + _RN)
    n = int(round(1.0/lam_dt))
    dt = 1.0/(lam*n)
    ui, un = _cell()
    dv0 = _dv(ui, un)
    for _ in range(n):
        R.cycle_no_flux(ui, un, tab, dt, drag)
    return float(np.abs(_dv(ui, un) - dv0*math.exp(-lam*dt*n)).max())


@pytest.mark.parametrize("integ,order", [("imex2", 1.8), ("imex2+", 1.8), ("imex3", 2.7)])
def test_drag_ode_convergence_order(integ, order):
    """three halvings of dt from lambda*dt = 0.05 (lambda = gamma (rho_i + rho_n)).  The observed order of a method of
    order p differs from p by O(lambda*dt): the coarsest step is chosen so that this term is a few per cent, and the
    finest error of imex3 (some 1e-11) is still far above the rounding error of 160 steps."""
    errs = [_drag_error(integ, 0.05/2**k) for k in range(4)]
    orders = [math.log2(errs[k]/errs[k + 1]) for k in range(3)]
    print(integ, errs, orders)
    assert min(orders) >= order, (errs, orders)


@pytest.mark.parametrize("integ", INTEGRATORS)
def test_stiff_limit_equalises_and_stays_bounded(integ):
    """gamma*dt = 1e6: the implicit stages are L-stable, each solve divides v_i - v_n by 1 + a gamma dt (rho_i+rho_n) and
    what the explicit combinations add back is O(1/(gamma dt)) of it: after a cycle |dv| <= 10/(gamma dt) |dv0| = 1e-5"""
    tab = R.tables(integ)
    ui, un = _cell()
    dv0, tot0 = _dv(ui, un), ui[0, :, 0] + un[0, :, 0]
    big = np.abs(ui[0, 1:, 0]) + np.abs(un[0, 1:, 0])
    for _ in range(5):
        R.cycle_no_flux(ui, un, tab, 1.0, 1.0e6)
        assert np.all(np.isfinite(ui)) and np.all(np.isfinite(un))
        assert np.all(np.abs(_dv(ui, un)) <= 1e-5*np.abs(dv0).max())
        assert np.all(np.abs(ui[0, 1:, 0]) <= big*(1 + 1e-9)) and np.all(np.abs(un[0, 1:, 0]) <= big*(1 + 1e-9))
    assert np.allclose(ui[0, :, 0] + un[0, :, 0], tot0, rtol=1e-12, atol=0)


@pytest.mark.parametrize("coef", [(0.7, 0.0, 0.0), (0.7, 0.2, 0.9), (1e6, 3.0, 50.0)])
def test_implicit_solve_conserves_sums_to_4_ulp(coef):
    """u_n = sum - u_i and rho_n = (rho_i + rho_n) - rho_i are kept: the sums of the pair change by the rounding of
    one subtraction and one addition"""
    rng = np.random.default_rng(7)
    n = 4096
    ui = np.empty((1, 4, n))
    un = np.empty((1, 4, n))
    ui[0, 0], un[0, 0] = rng.uniform(1e-3, 2.0, n), rng.uniform(0.1, 3.0, n)
    ui[0, 1:], un[0, 1:] = rng.normal(0, 1.0, (3, n)), rng.normal(0, 30.0, (3, n))
    s0 = ui + un
    g, xi, al = (np.float64(c*0.37) for c in coef)
    R.imex_imp(ui, un, g, xi, al)
    s1 = ui + un
    scale = np.maximum(np.maximum(np.abs(ui), np.abs(un)), np.abs(s0))
    assert np.all(np.abs(s1 - s0) <= 4*np.spacing(scale))
    assert np.all(ui[0, 0] > 0) and np.all(un[0, 0] > 0)


def test_zero_coefficient_slabs_are_not_read():
    """a NaN in a slab whose coefficient is 0.0 must not reach the state"""
    tab = R.tables("imex2+")
    ui, un = _cell()
    ru = np.full((4, 1, 8, 1), np.nan)
    ru[2] = 1.0
    a, b = ui.copy(), un.copy()
    R.imex_exp(a, b, ru, tab["a_twid"], 4, 0.1)             # row 2: only s = 2 is non-zero
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and not np.array_equal(a, ui)
    a, b = ui.copy(), un.copy()
    R.imex_exp(a, b, ru, tab["a_twid"], 5, 0.1)             # row 3: nothing
    assert np.array_equal(a, ui) and np.array_equal(b, un)


def test_host_coefficients_match_the_restatement():
    """IonNeutral.imp_coefficients (what the kernel is given) against the restatement, every estage of every integrator"""
    from athenak_amd.driver import Driver
    from athenak_amd.ion_neutral import IonNeutral
    ion = IonNeutral.__new__(IonNeutral)
    ion.drag_coeff, ion.ionization_coeff, ion.recombination_coeff = 0.7, 0.2, 0.9
    dt = 0.0123
    for integ in INTEGRATORS:
        d, t = Driver(_deck(["time/integrator=" + integ]), None), R.tables(integ)
        for estage in range(-1, t["nexp_stages"] + 1):
            istage, do_solve, adt, g, xi, al = ion.imp_coefficients(d, estage, dt)
            assert istage == estage + 2 and do_solve == (estage < t["nexp_stages"])
            assert adt == [t["a_twid"][istage - 2][s]*dt for s in range(istage - 1)]
            assert (g, xi, al) == tuple(float(x) for x in R.imp_coefficients(t, istage, dt, 0.7, 0.2, 0.9))


# ---- deck refusals -----------------------------------------------------------------------
def test_imex_without_ion_neutral_is_refused():
    from athenak_amd.driver import Driver
    for integ in INTEGRATORS:
        with pytest.raises(RuntimeError, match="ion-neutral"):
            Driver(_deck(["time/integrator=" + integ], drop=("ion-neutral",)), None)
    with pytest.raises(RuntimeError, match="not implemented"):
        Driver(_deck(["time/integrator=imex4"]), None)


@pytest.mark.parametrize("integ", ["rk1", "rk2", "rk3", "rk4"])
def test_ion_neutral_with_rk_is_refused(integ):
    from athenak_amd.driver import Driver
    with pytest.raises(RuntimeError, match="IonNeutral MHD can only be run with ImEx integrators"):
        Driver(_deck(["time/integrator=" + integ]), None)


@pytest.mark.parametrize("extra,drop,nranks,what", [
    ([], ("hydro",), 1, "either <hydro> or <mhd>"),
    ([], ("mhd",), 1, "either <hydro> or <mhd>"),
    ([], (), 2, "nranks"),
    (["mesh_refinement/refinement=static"], (), 1, "mesh_refinement"),
    (["mesh_refinement/refinement=adaptive"], (), 1, "mesh_refinement"),
    (["hydro_srcterms/const_accel=true"], (), 1, "hydro_srcterms"),
    (["mhd_srcterms/const_accel=true"], (), 1, "mhd_srcterms"),
    (["hydro/fofc=true"], (), 1, "hydro>/fofc"),
    (["mhd/fofc=true"], (), 1, "mhd>/fofc"),
    (["hydro/nu_iso=0.1"], (), 1, "hydro>/nu_iso"),
    (["hydro/alpha_iso=0.1"], (), 1, "hydro>/alpha_iso"),
    (["mhd/eta_ohm=0.1"], (), 1, "mhd>/eta_ohm"),
    (["mhd/eta_ad=0.1"], (), 1, "mhd>/eta_ad"),
])
def test_deck_refusals(extra, drop, nranks, what):
    from athenak_amd.ion_neutral import ionn_deck_checks
    from athenak_amd.mesh import MeshBlockPack
    pin = _deck(extra, drop)
    with pytest.raises(RuntimeError, match=what):
        ionn_deck_checks(pin, nranks)
    # AddPhysics says it before any physics module is built

    class _M:
        pass
    pk = MeshBlockPack.__new__(MeshBlockPack)
    pk.phydro = pk.pmhd = None
    pk.pmesh = _M()
    pk.pmesh.nranks = nranks
    with pytest.raises(RuntimeError, match=what):
        MeshBlockPack.AddPhysics(pk, pin)


def test_turb_driving_is_refused():
    from athenak_amd.mesh import MeshBlockPack
    pin = _deck(["turb_driving/driving_type=0"])
    pk = MeshBlockPack.__new__(MeshBlockPack)
    pk.phydro = pk.pmhd = None
    with pytest.raises(RuntimeError, match="turb_driving"):
        MeshBlockPack.AddPhysics(pk, pin)


def test_drag_coeff_is_required():
    from athenak_amd.ion_neutral import IonNeutral
    from athenak_amd.parameter_input import ParameterInput
    pin = ParameterInput(text="<ion-neutral>\nionization_coeff = 1.0\n")
    ion = IonNeutral.__new__(IonNeutral)
    with pytest.raises(Exception, match="drag_coeff"):
        ion.drag_coeff = pin.GetReal("ion-neutral", "drag_coeff")


def test_native_host_and_restart_outputs_are_refused():
    from athenak_amd.main import Simulation
    from athenak_amd.mesh import Mesh
    from athenak_amd.native import NativeSimulation
    from athenak_amd.outputs import Outputs
    with pytest.raises(RuntimeError, match="--host"):
        NativeSimulation(_deck())
    pin = _deck(["output1/file_type=rst", "output1/dt=1.0"])
    with pytest.raises(RuntimeError, match="rst output with <ion-neutral>"):
        Outputs(pin, Mesh(pin))
    with pytest.raises(RuntimeError, match="-r of a deck with <ion-neutral>"):
        Simulation(_deck(), restart=({}, None))


# ---- the C-shock profile -------------------------------------------------------------------
_OBLIQUE = dict(di=1e-3, dn=1.0, vix=20.0, vnx=20.0, viy=20.0, vny=20.0, bx=2.83, by=2.83)
_PERP = dict(di=1e-3, dn=1.0, vix=30.0, vnx=30.0, viy=0.0, vny=0.0, bx=0.0, by=10.0)


@pytest.mark.parametrize("init,pert,xmax", [(_OBLIQUE, 1e-5, 1.0e4), (_PERP, 1e-2, 3.5e4)])
def test_cshock_profile_is_monotone_and_conserves_mass_flux(init, pert, xmax):
    """the decks' settings at 128 cells.  Both fluids are compressed through the shock: the shock-normal velocities
    fall monotonically from the upstream value to a common downstream one (the ions first).  The transverse ion
    velocity of the oblique shock overshoots -- the ions follow the field line before the neutrals catch up -- and is
    not asserted; the neutrals' rises monotonically.  rho v_x of either fluid is the upstream constant."""
    from athenak_amd.pgen import cshock_profile
    soln, shk = cshock_profile(init, pert, 1.0, 1.0, 1.0, 128, -xmax, xmax)
    vix, vnx, viy, vny = soln.T
    assert np.all(np.diff(vix) <= 0) and np.all(np.diff(vnx) <= 0)
    assert np.all(vix <= vnx) and abs(vix[-1] - vnx[-1]) <= 1e-3*vnx[-1] and vnx[-1] < 0.5*vnx[0]
    if init["bx"] != 0.0:
        assert np.all(np.diff(vny) >= 0)
    else:
        assert np.all(viy == 0.0) and np.all(vny == 0.0)
    di, dn = init["di"]*init["vix"]/vix, init["dn"]*init["vnx"]/vnx
    assert np.all(np.abs(di*vix - init["di"]*init["vix"]) <= 1e-12*init["di"]*init["vix"])
    assert np.all(np.abs(dn*vnx - init["dn"]*init["vnx"]) <= 1e-12*init["dn"]*init["vnx"])
    # the cell values are means of ten points each: between the extremes of the fine profile, monotone as well
    for k, fine in (("vix", vix), ("vnx", vnx)):
        assert np.all(np.diff(shk[k]) <= 0) and fine.min() <= shk[k].min() and shk[k].max() <= fine.max()
    assert np.all(np.abs(shk["bx"] - init["bx"]) <= 16*np.spacing(init["bx"]))     # ten additions and a division
