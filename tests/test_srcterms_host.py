"""<hydro_srcterms> / <mhd_srcterms> and <units> on the host, no GPU: keys, defaults and refusals of both hosts, the unit
factors against the restatement of tests/srcterms_restate.py bit for bit, the place of the `srctrms` task, and the
restated ISMCoolFn against an evaluation at 50 digits (Python `decimal`)."""
import ctypes as C
import decimal
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import srcterms_restate as R  # noqa: E402
from athenak_amd import capi  # noqa: E402
from athenak_amd.parameter_input import ParameterInput  # noqa: E402

UNITS = {"length_cgs": 3.0856775809623245e+18, "mass_cgs": 6.83e+31, "time_cgs": 3.15576e+13, "mu": 1.4}


def _deck(name, extra=(), drop=()):
    """a shipped deck up to its outputs, with blocks / parameters of `extra` ("block/name=value") added"""
    text = open(os.path.join(ROOT, "athenak_amd", "inputs", name)).read()
    if "<output1>" in text:
        text = text[:text.index("<output1>")]
    for d in drop:
        text = "\n".join(l for l in text.split("\n") if not l.startswith(d))
    for e in extra:
        blk, rest = e.split("/", 1)
        text += "\n<%s>\n%s\n" % (blk, rest)
    return ParameterInput(text=text)


def _bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


@pytest.fixture
def cpu_device(monkeypatch):
    """host objects on CPU tensors: nothing is launched by building them"""
    monkeypatch.setattr(capi, "DEVICE", "cpu")


def _physics(pin):
    from athenak_amd.mesh import Mesh
    pm = Mesh(pin)
    pm.AddCoordinatesAndPhysics(pin)
    return pm, (pm.pmb_pack.phydro or pm.pmb_pack.pmhd)


def _cpp(pin, fluid):
    c = capi.SrcTerms()
    rc = capi.lib().akmi_srcterms_from_deck(pin.Dump().encode(), fluid.encode(), C.byref(c))
    return rc, c


# ---- keys and defaults ------------------------------------------------------------------
def test_struct_layout():
    assert C.sizeof(capi.SrcTerms) == 64


def test_no_block_no_psrc_both_hosts(cpu_device):
    pin = _deck("sod.athinput")
    _, ph = _physics(pin)
    assert ph.psrc is None
    rc, _ = _cpp(pin, "hydro")
    assert rc == 0


def test_empty_block_gives_inactive_psrc_with_reference_defaults(cpu_device):
    pin = _deck("sod.athinput", ["hydro_srcterms/dummy=1"])
    _, ph = _physics(pin)
    s = ph.psrc
    assert s is not None and not s.active
    assert (s.const_accel, s.ism_cooling, s.rel_cooling, s.rad_beam, s.self_gravity) == (False,)*5
    for k in ("const_accel", "ism_cooling", "rel_cooling", "rad_beam", "self_gravity"):     # GetOrAddBoolean adds them
        assert pin.GetBoolean("hydro_srcterms", k) is False
    assert s.dtnew == R.FLT_MAX
    rc, c = _cpp(_deck("sod.athinput", ["hydro_srcterms/dummy=1"]), "hydro")
    assert rc == 1 and (c.const_accel, c.ism_cooling) == (0, 0)


def test_const_accel_keys_both_hosts(cpu_device):
    pin = _deck("rt2d.athinput")
    _, ph = _physics(pin)
    s = ph.psrc
    assert s.const_accel and not s.ism_cooling and s.const_accel_val == -0.1 and s.const_accel_dir == 2
    assert (s.c.const_accel, s.c.const_accel_dir, s.c.ism_cooling, s.c.const_accel_val, s.c.gamma) == (1, 2, 0, -0.1, 1.4)
    rc, c = _cpp(_deck("rt2d.athinput"), "hydro")
    assert rc == 1
    assert bytes(c) == bytes(s.c)
    assert ph.psrc.pmy_fluid.pmy_pack.punit is None          # <units> is created iff the block exists


def test_missing_value_of_an_enabled_term_is_an_error(cpu_device):
    with pytest.raises(Exception, match="const_accel_val"):
        _physics(_deck("rt2d.athinput", drop=["const_accel_val"]))
    with pytest.raises(Exception, match="hrate"):
        _physics(_deck("turb_cooling.athinput", drop=["hrate", "<turb_driving>", "tcorr", "dedt", "nlow", "nhigh",
                                                      "driving_type"]))


def test_units_and_cooling_factors_bitwise_both_hosts(cpu_device):
    pin = _deck("turb_cooling.athinput")
    pm, ph = _physics(pin)
    un = pm.pmb_pack.punit
    ref = R.Units(**UNITS)
    assert (un.length_cgs(), un.mass_cgs(), un.time_cgs(), un.mu()) == (UNITS["length_cgs"], UNITS["mass_cgs"],
                                                                      UNITS["time_cgs"], UNITS["mu"])
    for got, want in ((un.velocity_cgs(), ref.velocity), (un.density_cgs(), ref.density), (un.energy_cgs(), ref.energy),
                      (un.pressure_cgs(), ref.pressure), (un.temperature_cgs(), ref.temperature)):
        assert _bits(got) == _bits(want)
    want3 = R.cooling_units(ref)
    s = ph.psrc
    assert s.ism_cooling and s.hrate == 2.0e-26
    for got, want in zip((s.temp_unit, s.cooling_unit, s.heating_unit), want3):
        assert _bits(got) == _bits(want)
    rc, c = _cpp(_deck("turb_cooling.athinput"), "mhd")
    assert rc == 1 and c.ism_cooling == 1 and c.hrate == 2.0e-26 and c.gamma == pin.GetReal("mhd", "gamma")
    for got, want in zip((c.temp_unit, c.cooling_unit, c.heating_unit), want3):
        assert _bits(got) == _bits(want)


def test_units_defaults():
    from athenak_amd.units import Units
    pin = ParameterInput(text="<units>\nmu = 0.6\n")
    un = Units(pin)
    assert (un.length_cgs(), un.mass_cgs(), un.time_cgs(), un.mu()) == (1.0, 1.0, 1.0, 0.6)
    assert _bits(un.temperature_cgs()) == _bits(R.Units(mu=0.6).temperature)


# ---- refusals ----------------------------------------------------------------------------
REFUSALS = [
    ("rt2d.athinput", ["hydro_srcterms/rel_cooling=true"], (), "rel_cooling = true is not on this path"),
    ("rt2d.athinput", ["hydro_srcterms/self_gravity=true"], (), "self_gravity = true is not on this path"),
    ("rt2d.athinput", ["hydro_srcterms/rad_beam=true"], (), "rad_beam = true is not on this path"),
    ("rt2d.athinput", ["hydro_srcterms/const_accel_dir=4"], ("const_accel_dir",), "const_accel_dir must be 1, 2 or 3"),
    ("rt2d.athinput", ["hydro_srcterms/const_accel_dir=0"], ("const_accel_dir",), "const_accel_dir must be 1, 2 or 3"),
    ("rt2d.athinput", ["hydro_srcterms/ism_cooling=true\nhrate=1.0e-26"], (), "needs a <units> block"),
    ("linear_wave_mhd.athinput", ["mhd_srcterms/ism_cooling=true\nhrate=1.0e-26", "units/mu=1.0", "mhd/eos=isothermal"],
     ("eos",), "ideal-gas EOS"),
    ("rt2d.athinput", ["hydro_srcterms/ism_cooling=true\nhrate=1.0e-26", "units/mu=1.0", "coord/general_rel=true"], (),
     "general_rel"),
]


@pytest.mark.parametrize("deck,extra,drop,what", REFUSALS)
def test_python_host_refuses(deck, extra, drop, what):
    from athenak_amd.mesh import MeshBlockPack
    pin = _deck(deck, extra, drop)
    if "eos=isothermal" in " ".join(extra):
        pin.SetString("mhd", "iso_sound_speed", "1.0")
    # AddPhysics says it before any physics module is built
    pk = MeshBlockPack.__new__(MeshBlockPack)
    pk.phydro = pk.pmhd = None
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*" + what):
        MeshBlockPack.AddPhysics(pk, pin)
    assert pk.phydro is None and pk.pmhd is None


@pytest.mark.parametrize("deck,extra,drop,what", REFUSALS)
def test_cpp_host_refuses(deck, extra, drop, what):
    """akmi_sim_create stops with the reference's "### FATAL ERROR" before anything is allocated (no GPU here)"""
    pin = _deck(deck, extra, drop)
    if "eos=isothermal" in " ".join(extra):
        pin.SetString("mhd", "iso_sound_speed", "1.0")
    body = r"""
import sys
sys.path.insert(0, %r)
from athenak_amd import capi
L = capi.lib()
h = L.akmi_sim_create(%r.encode(), None)
print(L.akmi_last_error().decode())
print("not refused")
""" % (ROOT, pin.Dump())
    r = subprocess.run([sys.executable, "-c", body], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "not refused" not in r.stdout
    assert "### FATAL ERROR" in r.stderr and what in r.stderr, r.stderr[-2000:]


def test_rt_generator_refuses_random_perturbations(cpu_device):
    from athenak_amd.pgen import ProblemGenerator
    for ip in (2, 3):
        pin = _deck("rt2d.athinput")
        pin.SetInteger("problem", "iprob", ip)
        pm, _ = _physics(pin)
        with pytest.raises(RuntimeError, match="iprob"):
            ProblemGenerator(pin, pm)


def test_rt_generator_hydrostatic_and_perturbed(cpu_device):
    """rt.cpp:108-131: density jump (smooth: tanh), single-mode momentum, pressure in hydrostatic balance with g"""
    from athenak_amd.pgen import ProblemGenerator
    pin = _deck("rt2d.athinput")
    pm, ph = _physics(pin)
    ProblemGenerator(pin, pm)
    ng = pm.mb_indcs.ng
    u = ph.u0.numpy()[:, :, 0, ng:-ng, ng:-ng]
    g, gam, amp, drat = -0.1, 1.4, 0.01, 2.0
    x2 = np.concatenate([np.linspace(-0.6, 0.0, 73)[:-1], np.linspace(0.0, 0.6, 73)[:-1]]) + 0.6/72/2
    den = 0.5*((drat + 1.0) + (drat - 1.0)*np.tanh(x2/0.01))
    got_den = np.concatenate([u[0, 0, :, 0], u[1, 0, :, 0]])
    assert np.allclose(got_den, den, rtol=1e-13)
    p0 = 1.0/gam - g*0.6
    mom = np.concatenate([u[0, 2], u[1, 2]])
    en = np.concatenate([u[0, 4], u[1, 4]])
    pres = (en - 0.5*mom*mom/got_den[:, None])*(gam - 1.0)
    assert np.allclose(pres, (p0 + g*den*x2)[:, None]*np.ones_like(pres), rtol=1e-12)
    assert 0.0 < np.abs(mom).max() <= amp*drat and np.all(u[:, 1] == 0.0) and np.all(u[:, 3] == 0.0)


# ---- the task ----------------------------------------------------------------------------
@pytest.mark.parametrize("deck,fluid", [("sod.athinput", "Hydro"), ("rt2d.athinput", "Hydro"),
                                        ("linear_wave_mhd.athinput", "MHD"), ("turb_cooling.athinput", "MHD")])
def test_srctrms_follows_rkupdt_and_sendu_depends_on_it(cpu_device, deck, fluid):
    pin = _deck(deck)
    pm, ph = _physics(pin)
    tl = pm.pmb_pack.tl_map["stagen"].task_list_
    names = [t.name for t in tl]
    k = names.index(fluid + "SrcTerms")
    assert names[k - 1] == "RKUpdate"
    by_id = {t.GetID().bits: t for t in tl}
    assert tl[k].GetDependency() == ph.id["rkupdt"] and tl[k].GetID() == ph.id["srctrms"]
    assert by_id[ph.id["sendu_oa"].bits].GetDependency() == ph.id["srctrms"]
    if pin.DoesBlockExist("turb_driving"):          # AddForcing before the update, the source terms after it
        assert names.index("AddForcing") == k - 2


def test_task_list_is_the_same_with_and_without_the_block(cpu_device):
    a = _physics(_deck("rt2d.athinput"))[0]
    pin = _deck("rt2d.athinput", drop=["<hydro_srcterms>", "const_accel"])
    from athenak_amd.mesh import Mesh
    b = Mesh(pin)
    b.AddCoordinatesAndPhysics(pin)
    na = [t.name for t in a.pmb_pack.tl_map["stagen"].task_list_]
    nb = [t.name for t in b.pmb_pack.tl_map["stagen"].task_list_]
    assert na == nb and b.pmb_pack.phydro.psrc is None


def test_source_terms_keep_the_separate_c2p_pass(cpu_device):
    """a hydro pack with source terms does not take the stage kernel with the conversion inside"""
    _, ph = _physics(_deck("rt3d.athinput"))
    assert ph.fused and ph._has_srcterms() and not ph._w_eligible()


def test_mesh_newtimestep_takes_the_source_dt(cpu_device):
    pm, ph = _physics(_deck("turb_cooling.athinput"))
    ph.dtnew = 1.0
    ph.psrc.dtnew = 0.25
    pm.dt = 10.0
    pm.NewTimeStep(1.0e9)
    assert pm.dt == pm.cfl_no*0.25


# ---- ISMCoolFn of the restatement against 50 digits ---------------------------------------
def _cool_hp(temp):
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        t = D(float(temp))
        logt = t.log10()
        if logt <= D("4.2"):
            return float(D("2.0e-19")*(-D("1.184e5")/(t + D("1.0e3"))).exp() + D("2.8e-28")*t.sqrt()*(-D("92.0")/t).exp())
        if logt > D("8.15"):
            return float(D(10)**(D("0.45")*logt - D("26.065")))
        ipps = min(max(int(D(25)*logt) - 103, 0), 100)
        x0 = D("4.12") + D("0.04")*ipps
        dx = logt - x0
        l1, l0 = D(float(R.LHD[ipps + 1])), D(float(R.LHD[ipps]))       # the float data, widened exactly
        return float(D(10)**((l1*dx - l0*(dx - D("0.04")))*25))


def test_coolfn_restatement_against_high_precision():
    """three branches and both sides of both branch points.  Double rounding of log T (<= 1 ulp(8.2) = 1.8e-15) enters
    log Lambda with the table's largest slope, 25*0.63 = 15.7, and 10^x turns an absolute 3e-14 into 7e-14 relative:
    bound 2e-13."""
    rng = np.random.default_rng(11)
    logs = np.concatenate([rng.uniform(1.0, 4.2, 400), rng.uniform(4.2, 8.15, 1200), rng.uniform(8.15, 9.0, 200),
                           4.2 + np.array([-1e-9, 1e-9, -1e-6, 1e-6]), 8.15 + np.array([-1e-9, 1e-9, -1e-6, 1e-6]),
                           4.12 + 0.04*np.arange(2, 101) + 1e-7])
    temp = 10.0**logs
    got = R.ism_cool_fn(temp)
    want = np.array([_cool_hp(t) for t in temp])
    rel = np.abs(got - want)/want
    assert rel.max() <= 2e-13, (rel.max(), temp[rel.argmax()])
    # the jump at log T = 4.2 and the continuity class of the fit at 8.15
    lo, hi = R.ism_cool_fn(10.0**np.array([4.2 - 1e-9, 4.2 + 1e-9]))
    assert abs(np.log10(lo) + 21.75) < 0.02 and abs(np.log10(hi) + 21.60) < 0.02
    # table nodes: the interpolation returns the tabulated value
    assert abs(np.log10(R.ism_cool_fn(np.array([10.0**6.0]))[0]) - float(R.LHD[47])) < 1e-6
