"""The MHD shearing box on the host, no GPU: what a deck with <shearing_box> and <mhd> builds and what it is refused, the
problem generators' errors, and the restatement of the face-centred operators (tests/sbox_mhd_restate.py) checked against
properties that do not depend on it: the three-case shift of the face field is one gather, orbital CT keeps div B, a zero
shift is the identity."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sbox_mhd_restate as M  # noqa: E402
import sbox_restate as R  # noqa: E402
from athenak_amd import capi  # noqa: E402
from athenak_amd.parameter_input import ParameterInput  # noqa: E402

SMALL = ["mesh/nx1=16", "mesh/nx2=16", "mesh/nx3=16", "meshblock/nx1=8", "meshblock/nx2=16", "meshblock/nx3=16"]
MHD_BLOCK = "+mhd/eos=isothermal\nreconstruct=plm\nrsolver=hlle\niso_sound_speed=1.0"


def _deck(name="mhd_shwave.athinput", extra=(), drop_outputs=True):
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


# ---- 1. decks -----------------------------------------------------------------------------------------------------------
def test_mhd_deck_with_the_block_is_built(cpu_device):
    """(raises "<shearing_box> with <mhd> is not on this path" before this feature)"""
    pm = _mesh(_deck(extra=SMALL))
    pk = pm.pmb_pack
    ph = pk.pmhd
    assert pk.phydro is None and pm.shear_periodic
    assert ph.psbox_u is not None and ph.porb_u is not None and ph.psbox_b is not None and ph.porb_b is not None
    assert ph.fused is False and ph.uflx is not None and ph.efld is not None and ph.pbval_u.fold_bcs is False
    assert (ph.psbox_b.qshear, ph.psbox_b.omega0) == (1.5, 1.0) and ph.psbox_u.nvar == ph.nvars == 4
    assert ph.psbox_b.nmb_x1bndry == [1, 1] and ph.porb_b.maxjshift == ph.porb_u.maxjshift == 1
    assert tuple(ph.psbox_b.buf.shape) == (2, 1, 3, 16 + 6, 16, 3) and tuple(ph.psbox_u.buf.shape) == (2, 1, 4, 22, 16, 3)
    assert tuple(ph.porb_b.emfx.shape) == tuple(ph.porb_b.emfz.shape) == (2, 22, 22, 14)
    # the face pencils reach one position further out than the cell centres
    assert ph.porb_b.max_joffset(0.05) >= ph.porb_u.max_joffset(0.05)
    # a deck without the block: nothing is created, and the stage stays fused
    plain = _mesh(_deck("linear_wave_mhd.athinput")).pmb_pack.pmhd
    assert plain.psbox_u is None and plain.psbox_b is None and plain.porb_b is None


def test_hydro_next_to_mhd_is_still_refused(cpu_device):
    for extra in ([MHD_BLOCK], ["+ion-neutral/drag_coeff=1.0", MHD_BLOCK]):
        with pytest.raises(RuntimeError) as e:
            _mesh(_deck("hydro_shwave.athinput", extra))
        assert "### FATAL ERROR" in str(e.value) and "<shearing_box> with <mhd>" in str(e.value) and "one fluid" in str(e.value)


REFUSALS = [
    (["time/evolution=kinematic", "mhd/rsolver=advect"], "<shearing_box> with kinematic MHD"),
    (["+ion-neutral/drag_coeff=1.0"], "<shearing_box> with <ion-neutral>"),
    (["+mesh_refinement/refinement=static"], "<mesh_refinement>/refinement = static"),
    (["+turb_driving/dedt=0.1"], "<shearing_box> with <turb_driving>"),
    (["+gravity/four_pi_G=1.0\nthreshold=0.0"], "<shearing_box> with <gravity>"),
    (["+output1/file_type=rst\ndt=1.0"], "rst outputs (<output1>/file_type = rst)"),
]


@pytest.mark.parametrize("extra,msg", REFUSALS, ids=[r[1] for r in REFUSALS])
def test_refusals_of_an_mhd_deck(cpu_device, extra, msg):
    with pytest.raises(RuntimeError) as e:
        _mesh(_deck(extra=SMALL + extra))
    assert "### FATAL ERROR" in str(e.value) and msg in str(e.value), str(e.value)


def test_native_host_and_several_ranks_refuse(cpu_device):
    from athenak_amd.native import NativeSimulation
    with pytest.raises(RuntimeError, match="<shearing_box> runs on the Python host only"):
        NativeSimulation(_deck(extra=SMALL))
    with pytest.raises(RuntimeError, match="<shearing_box> runs on one rank"):
        _mesh(_deck(extra=SMALL), nranks=2)


def test_ipert_errors_both_ways_round(cpu_device):
    from athenak_amd.main import Simulation
    with pytest.raises(RuntimeError, match="MHD shwave test requires ipert = 4."):
        Simulation(_deck(extra=SMALL + ["problem/ipert=3"]), initialize=False)
    with pytest.raises(RuntimeError, match="ipert must be 1,2, or 3 for hydro shwaves"):
        Simulation(_deck("hydro_shwave.athinput", ["problem/ipert=4"]), initialize=False)
    pin = _deck(extra=SMALL + ["mesh/ix1_bc=periodic", "mesh/ox1_bc=periodic"])
    del pin.blocks["shearing_box"]
    with pytest.raises(RuntimeError, match="shwave problem generator only works in shearing box"):
        Simulation(pin, initialize=False)


def test_user_history_of_both_fluids(cpu_device):
    from athenak_amd.outputs import user_hist_of
    assert user_hist_of(_deck()) is True
    with pytest.raises(RuntimeError, match="dByc\\) is enrolled for ipert = 4"):
        user_hist_of(_deck(extra=["problem/ipert=3"]))
    assert user_hist_of(_deck(extra=["problem/user_hist=false"])) is False
    assert user_hist_of(_deck("hydro_compress_shwave.athinput")) is True
    with pytest.raises(RuntimeError, match="enrolled for ipert = 3"):
        user_hist_of(_deck("hydro_compress_shwave.athinput", ["problem/ipert=4"]))


def test_ipert4_initial_state(cpu_device):
    """the face field of the vector potentials is divergence-free to round-off, the mean field is (rbx, rby, 0) with
    |B0|^2 = p0/beta, and the density perturbation has the amplitude cf2"""
    from athenak_amd.main import Simulation
    sim = Simulation(_deck(extra=SMALL), initialize=False)
    ph = sim.phys
    pm = sim.pmesh
    ind = pm.mb_indcs
    K, J, I = slice(ind.ks, ind.ke + 1), slice(ind.js, ind.je + 1), slice(ind.is_, ind.ie + 1)
    b1, b2, b3 = (f.numpy() for f in (ph.b0.x1f, ph.b0.x2f, ph.b0.x3f))
    dx = 0.5/16
    div = ((b1[:, K, J, ind.is_ + 1:ind.ie + 2] - b1[:, K, J, I]) + (b2[:, K, ind.js + 1:ind.je + 2, I] - b2[:, K, J, I])
           + (b3[:, ind.ks + 1:ind.ke + 2, J, I] - b3[:, K, J, I]))/dx
    bmag = np.sqrt(1.0/20.0)
    assert np.abs(div).max() <= 16*2.0**-52*bmag/dx
    assert abs(b1[:, K, J, I].mean()**2 + b2[:, K, J, I].mean()**2 - 1.0/20.0) <= 1e-12 and np.abs(b3[:, K, J, I]).max() < 1e-5
    d = ph.u0[:, 0].numpy()[:, K, J, I]
    k2 = (4.0*np.pi)**2*(4.0 + 1.0 + 1.0)
    cf2 = 1.0e-6*np.sqrt(np.sqrt(k2*20.0/21.0))
    assert abs(d.max() - 1.0 - cf2) <= 0.05*cf2 and abs(d.mean() - 1.0) <= 1e-12
    assert pm.pgen.user_hist_func is not None


def test_face_guard_of_the_orbital_shift(cpu_device):
    """max_joffset of the field's pencils includes the face at x1max, where |x1| is largest: a time step that keeps every
    cell centre within maxjshift = 1 but not that face is fatal before the launch"""
    pm = _mesh(_deck(extra=SMALL))
    ph = pm.pmb_pack.pmhd
    dx2 = 0.5/16
    dt = 2.0*dx2/(1.5*0.25)*(1.0 - 1e-3)          # the face at |x1| = 0.25 moves by just under two cells
    assert ph.porb_u.max_joffset(dt) == 1 and ph.porb_b.max_joffset(dt) == 1
    dt = 2.0*dx2/(1.5*0.25)*(1.0 + 1e-3)
    assert ph.porb_u.max_joffset(dt) == 1 and ph.porb_b.max_joffset(dt) == 2
    pm.dt = dt
    with pytest.raises(RuntimeError) as e:
        ph.porb_b.RecvAndUnpackFC(ph.b0, ph.recon_method)
    assert "### FATAL ERROR" in str(e.value) and "maxjshift = 1" in str(e.value)


MRI_SMALL = ["mesh/nx1=8", "mesh/nx2=16", "mesh/nx3=8", "meshblock/nx1=8", "meshblock/nx2=8", "meshblock/nx3=8"]


def test_mri3d_refusals(cpu_device):
    from athenak_amd.main import Simulation
    with pytest.raises(RuntimeError, match="mri3d with <shearing_box>/stratified = true is not on this path"):
        Simulation(_deck("mri3d.athinput", MRI_SMALL + ["shearing_box/stratified=true"]), initialize=False)
    with pytest.raises(RuntimeError, match="pgen_name = mri2d is not on this path"):
        Simulation(_deck("mri3d.athinput", MRI_SMALL + ["problem/pgen_name=mri2d"]), initialize=False)
    with pytest.raises(RuntimeError, match="mri3d with user boundaries is not on this path"):
        Simulation(_deck("mri3d.athinput", MRI_SMALL + ["mesh/ix3_bc=user", "mesh/ox3_bc=user"]), initialize=False)
    with pytest.raises(RuntimeError, match="mri3d problem generator only works in 3D"):
        Simulation(_deck("mri3d.athinput", ["mesh/nx1=8", "mesh/nx2=16", "mesh/nx3=1", "meshblock/nx1=8", "meshblock/nx2=8",
                                            "meshblock/nx3=1"]), initialize=False)
    pin = _deck("mri3d.athinput", MRI_SMALL + ["mesh/ix1_bc=periodic", "mesh/ox1_bc=periodic"])
    del pin.blocks["shearing_box"]
    with pytest.raises(RuntimeError, match="Shearing box not enabled for mri3d problem"):
        Simulation(pin, initialize=False)


@pytest.mark.parametrize("eos", ["isothermal", "ideal"])
@pytest.mark.parametrize("ifield", [1, 2, 3])
def test_mri3d_initial_state(cpu_device, ifield, eos):
    """the field of ifield = 1, 2, 3 including the faces at ie+1, je+1, ke+1; perturbations within amp; the seed decides
    the stream and its default is the first gid of the pack"""
    from athenak_amd.main import Simulation
    from athenak_amd.outputs import user_hist_of
    extra = MRI_SMALL + ["problem/ifield=%d" % ifield]
    if eos == "ideal":
        extra += ["mhd/eos=ideal", "+mhd/gamma=1.4", "+problem/pres=1.0"]
    sim = Simulation(_deck("mri3d.athinput", extra), initialize=False)
    ph, ind = sim.phys, sim.pmesh.mb_indcs
    K, J, I = slice(ind.ks, ind.ke + 1), slice(ind.js, ind.je + 1), slice(ind.is_, ind.ie + 1)
    K1, J1, I1 = slice(ind.ks, ind.ke + 2), slice(ind.js, ind.je + 2), slice(ind.is_, ind.ie + 2)
    b1, b2, b3 = (f.numpy() for f in (ph.b0.x1f, ph.b0.x2f, ph.b0.x3f))
    binit = np.sqrt(2.0*1.0/400.0)
    assert not b1.any()
    if ifield == 1:
        x1v = -0.5 + (np.arange(8) + 0.5)/8.0
        assert np.abs(b3[:, K1, J, I] - binit*np.sin(2.0*np.pi*x1v)).max() <= 4*2.0**-52 and not b2.any()
    elif ifield == 2:
        assert (b3[:, K1, J, I] == binit).all() and not b2.any()
    else:
        assert (b2[:, K, J1, I] == binit).all() and not b3.any()
    u = ph.u0.numpy()
    amp = 0.025
    d = u[:, 0][:, K, J, I]
    if eos == "isothermal":
        assert np.abs(d - 1.0).max() <= amp and np.abs(d - 1.0).max() > 0.5*amp
    else:
        assert (d == 1.0).all()
        byc = 0.5*(b2[:, K, J, I] + b2[:, K, ind.js + 1:ind.je + 2, I])
        bzc = 0.5*(b3[:, K, J, I] + b3[:, ind.ks + 1:ind.ke + 2, J, I])
        e = u[:, 4][:, K, J, I] - 0.5*byc**2 - 0.5*bzc**2
        assert np.abs(e*0.4 - 1.0).max() <= amp*1.0001 and np.abs(e*0.4 - 1.0).max() > 0.5*amp
    for n in (1, 2, 3):
        v = u[:, n][:, K, J, I]/d
        assert np.abs(v).max() <= amp*(1.0 + 1e-15) and np.abs(v).max() > 0.5*amp and abs(v.mean()) < 0.1*amp
    assert sim.pmesh.pgen.user_hist_func is not None and user_hist_of(sim.pin) is True
    # the same seed gives the same state, another seed another one; the default seed is the first gid, 0
    again = Simulation(_deck("mri3d.athinput", extra), initialize=False).phys.u0.numpy()
    other = Simulation(_deck("mri3d.athinput", extra + ["problem/rseed=5"]), initialize=False).phys.u0.numpy()
    pin = _deck("mri3d.athinput", extra)
    del pin.blocks["problem"]["rseed"]
    default = Simulation(pin, initialize=False).phys.u0.numpy()
    assert np.array_equal(again, u) and not np.array_equal(other, u) and np.array_equal(default, u)


# ---- 2. the restatement: the FC case logic is one gather ------------------------------------------------------------------
@pytest.mark.parametrize("ng", [2, 3, 4])
@pytest.mark.parametrize("nx2", [8, 12])
@pytest.mark.parametrize("nmbx2", [1, 2, 3])
def test_fc_case_logic_is_one_gather(ng, nx2, nmbx2):
    """every row 0..nj-1 of the x1 ghost faces of the three components is filled from global row (g - joffset) mod Ny on
    the inner face, (g + joffset) mod Ny on the outer one, for every offset from 0 to 2 Ny + 1; the last x2f row and the
    last x3f plane stay.  Offsets are exact multiples of a dyadic dx2, so the fractional remap is the identity."""
    nx, nmb = (4, nx2, 2), (2, nmbx2, 1)
    pk = R.Pack(nx, nmb, ng, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    pk.dx[:, 1] = 0.0625
    ny, nj = nmbx2*nx2, nx2 + 2*ng
    b = []
    for v, sh in enumerate(M.face_shapes(pk)):
        f = np.empty(sh)
        for m, l in enumerate(pk.lloc):
            rows = (l[1]*nx2 + np.arange(sh[2]) - pk.js) % ny          # the global row every row of the block holds
            f[m] = (1000.0*(v + 1) + rows)[None, :, None]
        b.append(f)
    recon = "plm" if ng == 2 else "ppmx"
    for joffset in range(0, 2*ny + 2):
        out = M.shear_boundary_fc(pk, tuple(b), joffset*0.0625, recon)
        for v in range(3):
            for m, l in enumerate(pk.lloc):
                g = l[1]*nx2 + np.arange(nj) - pk.js
                n = 0 if l[0] == 0 else 1
                want = 1000.0*(v + 1) + ((g - joffset) % ny if n == 0 else (g + joffset) % ny)
                c0 = 0 if n == 0 else (pk.ie + 2 if v == 0 else pk.ie + 1)
                got = out[v][m][:pk.N3, :nj, c0:c0 + ng]
                assert np.array_equal(got, np.broadcast_to(want[None, :, None], got.shape)), (joffset, v, m)
                # nothing else changed: the interior, the other face's slab, the last x2f row, the last x3f plane
                mask = np.ones(out[v][m].shape, dtype=bool)
                mask[:pk.N3, :nj, c0:c0 + ng] = False
                assert np.array_equal(out[v][m][mask], b[v][m][mask])


# ---- 3. the restatement: orbital CT -----------------------------------------------------------------------------------------
def _orbital_pack(nx1, nx2, nmbx2, ng):
    xmin, xmax = (-2.13, -0.23, -0.11), (2.13, 0.37, 0.2)
    return R.Pack((nx1, nx2, 3), (1, nmbx2, 1), ng, xmin, xmax), xmin, xmax


@pytest.mark.parametrize("nx1,nx2,nmbx2,ng,recon", [(8, 8, 1, 2, "dc"), (8, 8, 2, 2, "plm"), (9, 8, 2, 3, "ppmx")])
def test_orbital_ct_keeps_div_b(nx1, nx2, nmbx2, ng, recon):
    pk, xmin, xmax = _orbital_pack(nx1, nx2, nmbx2, ng)
    dx2 = float(pk.dx[0, 1])
    dt = 2.5*dx2/(1.5*2.13)                       # the faces at |x1| = 2.13 move by 2.5 cells
    b = M.divfree_field(pk, np.random.default_rng(nx1 + nmbx2))
    new, jmax, emfx, emfz = M.orbital_advection_fc(pk, b, 1.5, 1.0, dt, 2, recon)
    assert jmax == 2 and all(np.isfinite(f).all() for f in new)
    bmax = max(np.abs(f).max() for f in b)
    change = np.abs(M.div_b(pk, new) - M.div_b(pk, b)).max()
    bound = M.ct_divb_bound(pk, recon, 2, bmax)
    moved = max(np.abs(n - o).max() for n, o in zip(new, b))
    print(recon, "largest change of div B", change, "bound", bound, "largest change of a face", moved)
    assert change <= bound and moved > 0.1*bmax
    # faces outside the updated ranges are untouched
    K, J, I = slice(pk.ks, pk.ke + 1), slice(pk.js, pk.je + 1), slice(pk.is_, pk.ie + 1)
    rng = [(K, J, slice(pk.is_, pk.ie + 2)), (K, slice(pk.js, pk.je + 2), I), (slice(pk.ks, pk.ke + 2), J, I)]
    for v in range(3):
        mask = np.ones(new[v].shape, dtype=bool)
        mask[(slice(None),) + rng[v]] = False
        assert np.array_equal(new[v][mask], b[v][mask])
    # the x2f face two blocks share (or a block shares with itself across the periodic x2 edge) gets the same bits
    for m in range(pk.nmb):
        hi = pk.neighbour(m, 0, 1, 0)
        assert np.array_equal(new[1][m][K, pk.je + 1, I], new[1][hi][K, pk.js, I])


@pytest.mark.parametrize("recon", ["dc", "plm", "ppmx"])
def test_zero_orbital_shift_is_the_identity(recon):
    pk, _, _ = _orbital_pack(8, 8, 2, 3)
    b = M.divfree_field(pk, np.random.default_rng(2))
    new, jmax, emfx, emfz = M.orbital_advection_fc(pk, b, 1.5, 1.0, 0.0, 1, recon)
    assert jmax == 0 and all(np.array_equal(n, o) for n, o in zip(new, b))
    assert not emfx.any() and not emfz.any()
    new, _, _, _ = M.orbital_advection_fc(pk, b, 0.0, 0.0, 0.3, 1, recon)
    assert all(np.array_equal(n, o) for n, o in zip(new, b))
