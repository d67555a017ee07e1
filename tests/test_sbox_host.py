"""The hydro shearing box on the host, no GPU: the reference's three-case integer shift (tests/sbox_restate.py, written out
literally) against the single gather akmi_sbox_shift_x1 performs, the remap fluxes, the mesh's shear_periodic checks,
and every refusal of a deck with <shearing_box>."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sbox_restate as R  # noqa: E402
from athenak_amd import capi  # noqa: E402
from athenak_amd.parameter_input import ParameterInput  # noqa: E402

U = 2.0**-52


# ---- 1. the three cases and FindTargetMB against g -/+ joffset mod Ny: indices only -------------------------------------
@pytest.mark.parametrize("ng", [2, 3, 4])
@pytest.mark.parametrize("nx2", [8, 12])
@pytest.mark.parametrize("nmbx2", [1, 2, 3])
def test_case_logic_is_one_gather(ng, nx2, nmbx2):
    """every ghost row of every block is filled, and from global row (g - joffset) mod Ny on the inner face,
    (g + joffset) mod Ny on the outer one, for every offset from 0 to 2 Ny + 1"""
    js, N2, ny = ng, nx2 + 2*ng, nmbx2*nx2
    send = []
    for l in range(nmbx2):
        s = np.full(N2, -1, dtype=np.int64)
        s[js:js + nx2] = l*nx2 + np.arange(nx2)          # the global row each send-buffer row holds
        send.append(s)
    seen_jr = set()
    for n in (0, 1):
        for joffset in range(0, 2*ny + 2):
            seen_jr.add(joffset % nx2)
            recv = R.shift_cases(send, n, joffset, ng, nx2)
            for t in range(nmbx2):
                g = t*nx2 + (np.arange(N2) - js)
                want = (g - joffset) % ny if n == 0 else (g + joffset) % ny
                assert np.array_equal(recv[t], want), (n, joffset, t, recv[t], want)
    assert {ng - 1, ng, nx2 - ng - 1, nx2 - ng} <= seen_jr


# ---- 2. remap fluxes ----------------------------------------------------------------------------------------------------
def _remap(recon, eps, a, jl, ju):
    """a(j) - (flx(j+1) - flx(j)) for j in [jl, ju], as shearing_box_cc.cpp:113"""
    flx = R.remap_flux_of(recon)(jl, ju + 1, eps, a)
    j = np.arange(jl, ju + 1)
    return a[j] - (flx[j + 1] - flx[j])


@pytest.mark.parametrize("recon", ["dc", "plm", "ppmx"])
def test_zero_offset_is_the_identity(recon):
    rng = np.random.default_rng(3)
    a = rng.standard_normal((30, 4))
    for eps in (0.0, -0.0):
        assert np.array_equal(_remap(recon, eps, a, 3, 26), a[3:27])


@pytest.mark.parametrize("recon", ["plm", "ppmx"])
@pytest.mark.parametrize("eps", [0.3, -0.3, 0.9, -1e-12])
def test_linear_profile_is_shifted_exactly(recon, eps):
    """the average of c + s x over a cell moved by eps cells is a(j) - s eps: both schemes reconstruct a linear profile
    exactly.  Some ten rounded operations on values of at most max|a| + |s| stand between the two: 32 ulp of max|a|."""
    j = np.arange(30, dtype=np.float64)
    a = (1.7 + 0.37*j)[:, None]
    got = _remap(recon, eps, a, 3, 26)
    assert np.abs(got - (a[3:27] - 0.37*eps)).max() <= 32*U*np.abs(a).max()


@pytest.mark.parametrize("recon", ["dc", "plm", "ppmx"])
@pytest.mark.parametrize("eps", [0.41, -0.41, 0.97])
def test_periodic_pencil_keeps_its_sum(recon, eps):
    ng, nx2 = 3, 24
    rng = np.random.default_rng(11)
    act = rng.standard_normal((nx2, 6))
    a = np.concatenate([act[-ng:], act, act[:ng]])               # ghost rows = periodic images
    new = _remap(recon, eps, a, ng, ng + nx2 - 1)
    bound = nx2*U*np.abs(act).max()*R.conservation_factor(recon)
    defect = R.periodic_sum_defect(new, act)
    print(recon, eps, "largest defect of a pencil sum", defect.max(), "bound", bound)
    assert defect.max() <= bound
    assert np.abs(new - act).max() > 1e-3                        # (the remap did move something)


# ---- 3. decks -------------------------------------------------------------------------------------------------------------
def _deck(name="hydro_shwave.athinput", extra=(), drop_outputs=True):
    text = open(os.path.join(ROOT, "athenak_amd", "inputs", name)).read()
    if drop_outputs and "<output1>" in text:
        text = text[:text.index("<output1>")]
    pin = ParameterInput(text=text)
    pin.ModifyFromCmdline([e for e in extra if "\n" not in e and not e.startswith("+")])
    for e in extra:
        if e.startswith("+"):                        # "+block/name=value": a block the deck does not have
            blk, rest = e[1:].split("/", 1)
            pin.LoadFromString("<%s>\n%s\n" % (blk, rest))
    return pin


@pytest.fixture
def cpu_device(monkeypatch):
    monkeypatch.setattr(capi, "DEVICE", "cpu")


def _mesh(pin, nranks=1):
    from athenak_amd.mesh import Mesh
    pm = Mesh(pin, 0, nranks)
    pm.AddCoordinatesAndPhysics(pin)
    return pm


def test_shear_periodic_deck_is_accepted(cpu_device):
    """(raises "boundary flag 'shear_periodic' not supported" before this feature)"""
    from athenak_amd.mesh import SHEAR_PERIODIC
    pm = _mesh(_deck())
    ph = pm.pmb_pack.phydro
    assert not pm.strictly_periodic and pm.shear_periodic
    assert ph.psbox_u is not None and ph.porb_u is not None and ph.fused is False and ph.uflx is not None
    assert (ph.psbox_u.qshear, ph.psbox_u.omega0, ph.psbox_u.is_stratified) == (1.5, 1.0, False)
    assert ph.porb_u.maxjshift == int(0.3*0.25) + 1 == 1
    # the four blocks of 32 x 32 x 4 each sit on one x1 face: the flag on that face, block or periodic on the others
    bcs = np.asarray(pm.pmb_pack.pmb.mb_bcs)
    for m, l in enumerate(pm.lloc_eachmb):
        assert bcs[m, 0] == (SHEAR_PERIODIC if l[0] == 0 else capi.BC["block"])
        assert bcs[m, 1] == (SHEAR_PERIODIC if l[0] == 1 else capi.BC["block"])
    assert ph.psbox_u.nmb_x1bndry == [2, 2]
    # the neighbour table wraps across the shear-periodic faces, and the gather leaves the boundary functions alone
    assert (np.asarray(pm.pmb_pack.pmb.nghbr_gid)[:, [12, 14]] >= 0).all() and ph.pbval_u.fold_bcs is False
    # a deck without the block: nothing is created
    assert _mesh(_deck("linear_wave_hydro.athinput")).pmb_pack.phydro.psbox_u is None


def test_block_without_shear_periodic_faces(cpu_device):
    """the reference's hydro_orb_adv deck has outflow x1: source terms and orbital advection, no boundary block"""
    pm = _mesh(_deck(extra=["mesh/ix1_bc=outflow", "mesh/ox1_bc=outflow"]))
    ph = pm.pmb_pack.phydro
    assert ph.psbox_u.nmb_x1bndry == [0, 0] and ph.psbox_u.buf is None and ph.porb_u is not None and not pm.shear_periodic


MESH_ERRORS = [
    (["mesh/ox1_bc=periodic"], "both x1 bcs must be shear_periodic"),
    (["mesh/ix1_bc=outflow"], "both x1 bcs must be shear_periodic"),
    (["mesh/nx2=1", "mesh/nx3=1", "meshblock/nx2=1", "meshblock/nx3=1"], "Shear Periodic Boundaries require 2D or 3D"),
    (["mesh/ix2_bc=shear_periodic"], "cannot be applied in x2"),
    (["mesh/ox2_bc=shear_periodic"], "cannot be applied in x2"),
    (["mesh/ix3_bc=shear_periodic"], "cannot be applied in x3"),
    (["mesh/ox3_bc=shear_periodic"], "cannot be applied in x3"),
]


@pytest.mark.parametrize("extra,msg", MESH_ERRORS, ids=["%s %s" % (e[0][0], e[1][:12]) for e in MESH_ERRORS])
def test_mesh_flag_checks(cpu_device, extra, msg):
    """mesh.cpp:95-165"""
    with pytest.raises(RuntimeError) as e:
        _mesh(_deck(extra=extra))
    assert "### FATAL ERROR" in str(e.value) and msg in str(e.value), str(e.value)


def test_shear_periodic_needs_the_block(cpu_device):
    pin = _deck()
    del pin.blocks["shearing_box"]
    with pytest.raises(RuntimeError, match="Shear Periodic Boundaries set but no <shearing_box> block"):
        _mesh(pin)


def test_required_parameters_and_pgen_errors(cpu_device):
    from athenak_amd.main import Simulation
    pin = _deck()
    del pin.blocks["shearing_box"]["omega0"]
    with pytest.raises(RuntimeError, match="omega0"):
        _mesh(pin)
    with pytest.raises(RuntimeError, match="ipert must be 1,2, or 3 for hydro shwaves"):
        Simulation(_deck(extra=["problem/ipert=4"]), initialize=False)
    pin = _deck(extra=["mesh/ix1_bc=periodic", "mesh/ox1_bc=periodic"])
    del pin.blocks["shearing_box"]
    with pytest.raises(RuntimeError, match="shwave problem generator only works in shearing box"):
        Simulation(pin, initialize=False)


MHD_BLOCK = "+mhd/eos=isothermal\nreconstruct=plm\nrsolver=hlle\niso_sound_speed=1.0"
REFUSALS = [
    ([MHD_BLOCK], "<shearing_box> with <mhd>"),
    (["+ion-neutral/drag_coeff=1.0", MHD_BLOCK], "<shearing_box> with <mhd>"),
    (["+ion-neutral/drag_coeff=1.0"], "<shearing_box> with <ion-neutral>"),
    (["+mesh_refinement/refinement=static"], "<mesh_refinement>/refinement = static"),
    (["+mesh_refinement/refinement=adaptive"], "<mesh_refinement>/refinement = adaptive"),
    (["+turb_driving/dedt=0.1"], "<shearing_box> with <turb_driving>"),
    (["+gravity/four_pi_G=1.0\nthreshold=0.0"], "<shearing_box> with <gravity>"),
    (["+output1/file_type=rst\ndt=1.0"], "rst outputs (<output1>/file_type = rst)"),
]


@pytest.mark.parametrize("extra,msg", REFUSALS, ids=[r[1] for r in REFUSALS])
def test_refusals(cpu_device, extra, msg):
    with pytest.raises(RuntimeError) as e:
        _mesh(_deck(extra=extra))
    assert "### FATAL ERROR" in str(e.value) and msg in str(e.value), str(e.value)


def test_refusal_several_ranks(cpu_device):
    with pytest.raises(RuntimeError, match="<shearing_box> runs on one rank"):
        _mesh(_deck(), nranks=2)


def test_refusal_restart_and_native_host(cpu_device):
    from athenak_amd.main import Simulation
    from athenak_amd.native import NativeSimulation
    with pytest.raises(RuntimeError, match="-r of a deck with <shearing_box>"):
        Simulation(_deck(), restart=(None, None))
    with pytest.raises(RuntimeError, match="<shearing_box> runs on the Python host only"):
        NativeSimulation(_deck())
    with pytest.raises(RuntimeError, match="<shearing_box> runs on the Python host only"):
        NativeSimulation(_deck(extra=["mesh/ix1_bc=outflow", "mesh/ox1_bc=outflow"]))


def test_user_history_is_enrolled_for_the_compressible_wave_only(cpu_device):
    from athenak_amd.outputs import user_hist_of
    assert user_hist_of(_deck("hydro_compress_shwave.athinput")) is True
    with pytest.raises(RuntimeError, match="enrolled for ipert = 3"):
        user_hist_of(_deck("hydro_compress_shwave.athinput", ["problem/ipert=2"]))
    assert user_hist_of(_deck()) is False


def test_allowed_combinations_are_built(cpu_device):
    """passive scalars and const_accel alongside; every reconstruction and Riemann solver of the task-granular path"""
    pm = _mesh(_deck(extra=["+hydro/nscalars=2", "+hydro_srcterms/const_accel=true\nconst_accel_val=0.1\nconst_accel_dir=3"]))
    ph = pm.pmb_pack.phydro
    assert ph.psbox_u.nvar == ph.nvars == 6 and ph.psrc.active and ph.fused is False
    assert tuple(ph.psbox_u.buf.shape) == (2, 2, 6, 4 + 6, 32, 3)
    for recon, rs in (("dc", "llf"), ("plm", "roe"), ("ppm4", "hlle"), ("wenoz", "llf")):
        assert _mesh(_deck(extra=["hydro/reconstruct=" + recon, "hydro/rsolver=" + rs])).pmb_pack.phydro.porb_u is not None
    assert _mesh(_deck(extra=["hydro/eos=ideal", "+hydro/gamma=1.4", "hydro/rsolver=hllc"])).pmb_pack.phydro.psbox_u is not None


def test_two_d_deck_takes_the_source_terms_only(cpu_device):
    pm = _mesh(_deck(extra=["mesh/nx3=1", "meshblock/nx3=1"]))
    ph = pm.pmb_pack.phydro
    assert pm.shear_periodic and ph.psbox_u.buf is None and not ph._sbox_3d()


# ---- 4. guards of orbital advection and of the boundary ---------------------------------------------------------------------
def test_block_too_short_for_the_orbital_shift(cpu_device):
    """maxjshift = int(0.3*10) + 1 = 4, nghost = 3: 7 rows of a block of 4"""
    extra = ["mesh/x1min=-10.0", "mesh/x1max=10.0", "mesh/nx2=8", "meshblock/nx2=4", "mesh/nx1=8", "meshblock/nx1=8"]
    with pytest.raises(RuntimeError) as e:
        _mesh(_deck(extra=extra))
    assert "nghost + maxjshift <= <meshblock>/nx2, but 3 + 4 > 4" in str(e.value)
    extra[3] = "meshblock/nx2=8"
    assert _mesh(_deck(extra=extra)).pmb_pack.phydro.porb_u.maxjshift == 4


def test_non_periodic_x2_in_three_d(cpu_device):
    with pytest.raises(RuntimeError, match="orbital advection in 3-D needs periodic x2 faces"):
        _mesh(_deck(extra=["mesh/ix2_bc=outflow", "mesh/ox2_bc=outflow"]))


def test_time_step_beyond_maxjshift_is_fatal(cpu_device):
    """|joffset| = int(qshear*omega0*|x1v|*dt/dx2) at the outermost column, x1v = 0.25 - dx1/2: 1.5*0.24609375*dt*128.
    dt = 0.02 gives 0, dt = 0.03 gives 1 = maxjshift, dt = 0.05 gives 2: fatal before the launch."""
    pm = _mesh(_deck())
    ph = pm.pmb_pack.phydro
    assert [ph.porb_u.max_joffset(dt) for dt in (0.02, 0.03, 0.05)] == [0, 1, 2]
    pm.dt = 0.05
    with pytest.raises(RuntimeError) as e:
        ph.porb_u.RecvAndUnpackCC(ph.u0, ph.u1, ph.recon_method)
    assert "dt = 0.05" in str(e.value) and "maxjshift = 1" in str(e.value) and "### FATAL ERROR" in str(e.value)


def test_negative_shear_is_refused(cpu_device):
    with pytest.raises(RuntimeError, match="qshear\\*omega0 >= 0"):
        _mesh(_deck(extra=["shearing_box/qshear=-1.5"]))
    ph = _mesh(_deck()).pmb_pack.phydro
    ph.psbox_u.InitRecv(2.0)
    assert ph.psbox_u.yshear == (1.5*1.0)*0.5*2.0
    with pytest.raises(RuntimeError, match="time >= 0"):
        ph.psbox_u.InitRecv(-1.0)
