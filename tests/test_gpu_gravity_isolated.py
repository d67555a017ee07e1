"""gpu: isolated self-gravity on the device (csrc/akmi_mg.hip, gravity.py) against the numpy restatement of
tests/mg_isolated_restate.py, bit for bit: the ghost exchange and the root boundary with physical faces (zerofixed,
zerograd, multipole), the multipole moments, the mask, akmi_mg_solve, the launch count, and the two-sphere deck."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mg_isolated_restate as I  # noqa: E402
import mg_restate as R  # noqa: E402
import test_gpu_gravity as G  # noqa: E402
import test_gravity_host as H  # noqa: E402
import test_gravity_isolated_host as HT  # noqa: E402

pytestmark = pytest.mark.gpu
NG = 2
EXT = HT.EXT
_dev, _np, _call, _bytes_equal, _ghost_mask = G._dev, G._np, G._call, G._bytes_equal, G._ghost_mask
NOPER, X2PER = (0,)*6, (0, 0, 1, 1, 0, 0)
BCS = ["zerofixed", "zerograd", "multipole"]


def _mp(rng):
    """28 doubles: coefficients of order one, an origin inside the mesh and off every cell centre and face"""
    return np.concatenate([rng.standard_normal(25), np.array([0.03, -0.07, 0.11])])


# ---- 1. the exchange with physical faces ----------------------------------------------------------------------------------
#          root grid, periodic flags, edge of the level
LEVELS = [((2, 2, 2), NOPER, 4), ((2, 2, 2), NOPER, 2), ((3, 2, 2), NOPER, 2), ((3, 2, 2), X2PER, 2),
          ((1, 1, 1), X2PER, 4), ((2, 2, 2), NOPER, 1), ((1, 1, 1), X2PER, 1)]


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("nrb,per,edge", LEVELS, ids=["%dx%dx%d-%s-e%d" % (r + ("x2per" if p[2] else "open", e))
                                                      for r, p, e in LEVELS])
def test_exchange_with_physical_faces(nrb, per, edge, bc):
    rng = np.random.default_rng(edge + 10*sum(nrb) + len(bc))
    lloc = R.row_major_lloc(nrb)
    nmb = len(lloc)
    tab = I.neighbor_table(lloc, nrb, per)
    assert (tab[:, [12, 14, 4, 22]] < 0).any()
    xlim = I.block_extents(lloc, nrb, EXT)
    u = rng.standard_normal((nmb, edge + 2, edge + 2, edge + 2))
    gm = _ghost_mask(u.shape)
    for order in ((2, 4) if bc == "multipole" else (4,)):
        mp = _mp(rng)
        want = u.copy()
        I.exchange_bc(want, tab, I.BC[bc], mp[:25], mp[25:], order, xlim)
        got = _dev(u)
        _call("akmi_mg_exchange_bc", nmb, edge, edge, edge, _dev(tab.reshape(-1)), I.BC[bc], order, _dev(mp),
              _dev(xlim.reshape(-1)), got)
        got = _np(got)
        assert np.array_equal(got, want), (bc, order, np.argwhere(got != want)[:5])
        assert _bytes_equal(got[~gm], u[~gm])
        assert (got != u)[gm].any()
    if bc == "multipole":                 # edge and corner ghosts that touch a physical face keep what they held
        m = 0                             # block (0, 0, 0) has the inner x1 face of the mesh
        assert _bytes_equal(got[m, :, 0, 0], u[m, :, 0, 0]) and _bytes_equal(got[m, 0, :, 0], u[m, 0, :, 0])


def test_exchange_bc_none_is_the_periodic_exchange():
    """type none on a periodic table is akmi_mg_exchange; on a table with physical faces those ghosts are left alone"""
    rng = np.random.default_rng(3)
    nrb = (2, 2, 2)
    lloc = R.row_major_lloc(nrb)
    u = rng.standard_normal((8, 6, 6, 6))
    for per in ((1,)*6, NOPER):
        tab = I.neighbor_table(lloc, nrb, per)
        want = u.copy()
        I.exchange_bc(want, tab, I.NONE)
        if per[0]:
            alt = u.copy()
            R.exchange(alt, R.neighbor_table(lloc, nrb))
            assert np.array_equal(want, alt)
        got = _dev(u)
        _call("akmi_mg_exchange_bc", 8, 4, 4, 4, _dev(tab.reshape(-1)), I.NONE, 0, None, None, got)
        assert _bytes_equal(_np(got), want)


# ---- 2. the root boundary ------------------------------------------------------------------------------------------------
ROOTS = [((2, 2, 2), NOPER), ((4, 4, 4), NOPER), ((3, 2, 2), NOPER), ((3, 2, 2), X2PER), ((1, 1, 1), X2PER),
         ((1, 1, 1), NOPER), ((4, 2, 2), (1, 1, 0, 0, 0, 0))]


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("root,per", ROOTS, ids=["%dx%dx%d-%s" % (r + ("".join(map(str, p)),)) for r, p in ROOTS])
def test_root_boundary_with_physical_faces(root, per, bc):
    rng = np.random.default_rng(sum(root) + sum(per) + len(bc))
    nx, ny, nz = root
    u = rng.standard_normal((1, nz + 2, ny + 2, nx + 2))
    gm = _ghost_mask(u.shape)
    ext = (C.c_double*6)(*EXT)
    flags = (C.c_int*6)(*per)
    for order in ((2, 4) if bc == "multipole" else (4,)):
        mp = _mp(rng)
        want = u.copy()
        I.root_boundary_bc(want, I.BC[bc], per, mp[:25], mp[25:], order, EXT)
        got = _dev(u)
        _call("akmi_mg_root_boundary_bc", nz, ny, nx, I.BC[bc], flags, order, _dev(mp), ext, got)
        got = _np(got)
        assert np.array_equal(got, want), (bc, order, np.argwhere(got != want)[:5])
        assert _bytes_equal(got[~gm], u[~gm]) and (got != u)[gm].any()
    if bc != "multipole" and not any(per):          # the composite mirror of a corner: three signs
        s = -1.0 if bc == "zerofixed" else 1.0
        assert got[0, 0, 0, 0] == s*s*s*u[0, 1, 1, 1]


def test_root_boundary_all_periodic_is_the_old_one():
    rng = np.random.default_rng(9)
    u = rng.standard_normal((1, 4, 4, 5))
    want = u.copy()
    R.root_boundary(want)
    got = _dev(u)
    _call("akmi_mg_root_boundary_bc", 2, 2, 3, I.ZEROFIXED, (C.c_int*6)(*(1,)*6), 0, None, None, got)
    assert _bytes_equal(_np(got), want)


# ---- 3. the moments ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto", [True, False], ids=["com", "fixed"])
@pytest.mark.parametrize("order,nodipole", [(2, False), (4, False), (4, True), (2, True)])
@pytest.mark.parametrize("nrb,edge", [((2, 2, 2), 8), ((2, 1, 1), 32)], ids=["8x8^3", "2x32^3"])
def test_multipole_moments(nrb, edge, order, nodipole, auto):
    import torch
    from athenak_amd import capi
    rng = np.random.default_rng(edge + order)
    lloc = R.row_major_lloc(nrb)
    nmb = len(lloc)
    ext = (-0.5, 0.5, -0.5, -0.5 + 1.0*nrb[1]/nrb[0], -0.5, -0.5 + 1.0*nrb[2]/nrb[0])
    xlim = I.block_extents(lloc, nrb, ext)
    src = rng.standard_normal((nmb, edge + 2, edge + 2, edge + 2)) - 1.5
    org = None if auto else (0.0625, -0.03, 0.01)
    want, worg = I.multipole(src, xlim, order, nodipole, org)
    mp = np.full(28, 7.0)
    if not auto:
        mp[25:] = org
    got = _dev(mp)
    ns = 25*int(capi.lib().akmi_mg_reduce_scratch_doubles(nmb, edge, edge, edge))
    scratch = torch.zeros(ns, dtype=torch.float64, device="cuda")
    _call("akmi_mg_multipole_moments", nmb, edge, edge, edge, order, int(nodipole), int(auto), _dev(xlim.reshape(-1)),
          _dev(src), scratch, got)
    got = _np(got)
    nc = 9 if order == 2 else 25
    assert np.array_equal(got[:nc], want[:nc]), np.abs(got[:nc] - want[:nc]).max()
    assert np.array_equal(got[25:], worg)
    assert np.all(got[nc:25] == 7.0) and want[0] != 0.0 and (nodipole == (not want[1:4].any()))


# ---- 4. the mask ---------------------------------------------------------------------------------------------------------
def test_mask():
    rng = np.random.default_rng(4)
    nrb, edge = (2, 2, 2), 4
    lloc = R.row_major_lloc(nrb)
    xlim = I.block_extents(lloc, nrb, EXT)
    src = rng.standard_normal((8, edge + 2, edge + 2, edge + 2))
    org, rad = (0.03, -0.01, 0.0625), 0.3
    want = src.copy()
    I.apply_mask(want, xlim, rad, org)
    got = _dev(src)
    _call("akmi_mg_mask", 8, edge, edge, edge, _dev(xlim.reshape(-1)), C.c_double(rad), *[C.c_double(o) for o in org], got)
    assert _bytes_equal(_np(got), want) and 0 < (want != src).sum() < 8*edge**3


# ---- 5. akmi_mg_solve ----------------------------------------------------------------------------------------------------
def _sim(n, nb, extra=()):
    from athenak_amd.main import Simulation
    over = ["mesh/nx%d=%d" % (q, n) for q in (1, 2, 3)] + ["meshblock/nx%d=%d" % (q, nb) for q in (1, 2, 3)]
    return Simulation(H._deck("binary_gravity.athinput", over + list(extra)))


def _restated(sim, n, nb, **kw):
    pm = sim.pmesh
    d = pm.pmb_pack.pgrav.pmgd
    lloc = [tuple(pm.lloc_eachmb[int(g)])[:3] for g in pm.pmb_pack.pmb.mb_gid]
    return I.IsolatedSolver((n,)*3, nb, EXT, lloc, d.four_pi_G_, d.mg_bc_, periodic=d.periodic_, ng=NG, threshold=d.eps_,
                            niteration=d.niter_, npresmooth=d.npresmooth_, npostsmooth=d.npostsmooth_,
                            full_multigrid=d.full_multigrid_, mporder=max(d.mporder_, 2), nodipole=d.nodipole_,
                            mporigin=None if d.autompo_ else d.mpo_, mask_radius=d.mask_radius_,
                            mask_origin=d.mask_origin_, **kw)


SOLVES = [(bc, fmg, ()) for bc in BCS for fmg in (True, False)] + [
    ("zerofixed", True, ("mesh/ix2_bc=periodic", "mesh/ox2_bc=periodic")),
    ("multipole", True, ("gravity/mporder=2", "gravity/auto_mporigin=false", "+gravity/nodipole=true",
                         "+gravity/mporigin_x1=0.01\nmporigin_x2=-0.02\nmporigin_x3=0.03",
                         "+gravity/mask_radius=0.45\nmask_origin_x1=-0.05"))]


@pytest.mark.parametrize("bc,fmg,extra", SOLVES, ids=["%s-%s%s" % (b, "fmg" if f else "mgi", "-var" if e else "")
                                                      for b, f, e in SOLVES])
def test_solve_matches_restated_solve(bc, fmg, extra):
    """16^3 with blocks of 8^3, two consecutive calls: phi, the norms, the coefficients, the origin.  threshold 1e-7;
    zerograd on every face has no solution for a source with a net mass (the defect stalls at its mean), so there
    three V-cycles and the final norm of show_defect = 1"""
    stop = ["gravity/threshold=1.0e-7"] if bc != "zerograd" else ["gravity/threshold=-1.0",
                                                                  "+gravity/niteration=3\nshow_defect=1"]
    sim = _sim(16, 8, ["gravity/mg_bc=%s" % bc, "gravity/full_multigrid=%s" % ("true" if fmg else "false")] + stop
               + list(extra))
    pk = sim.pmesh.pmb_pack
    d = pk.pgrav.pmgd
    s = _restated(sim, 16, 8)
    assert (s.nrootlevel, s.nmblevel) == (d.nrootlevel_, d.nmblevel_) == (2, 4)
    rho = pk.phydro.u0[:, 0].clone()
    for call, scale in enumerate((1.0, 1.3)):
        pk.phydro.u0[:, 0].copy_(rho*scale)
        d.Solve()
        want = s.solve(pk.phydro.u0.cpu().numpy())
        got = _np(pk.pgrav.phi)
        assert np.array_equal(got, want), (call, np.abs(got - want).max())
        assert d.coffset_ == s.coffset and d.ncycles.value == s.ncycles
        if bc != "zerograd":
            assert np.array_equal(np.array(d.last_norms), np.array(s.norms)) and d.last_norms[-1] <= 1.0e-7
        else:
            assert d.ncycles.value == 3 and d.norms[41] == s.calculate_defect_norm()
        if bc == "multipole":
            nc = 9 if d.mporder_ == 2 else 25
            assert np.array_equal(d.mpcoeff(), s.mp[:nc]) and np.array_equal(d.mporigin(), s.org)
    assert np.abs(got).max() > 0.0


def _launches(sim, sub_avg_off=False):
    from athenak_amd import capi
    import torch
    d = sim.pmesh.pmb_pack.pgrav.pmgd
    if sub_avg_off:
        d.fsubtract_average_ = False
    capi.lib().akmi_mg_launch_count(1)
    d.Solve()
    torch.cuda.synchronize()
    return int(capi.lib().akmi_mg_launch_count(1))


def test_launch_count():
    """physical faces add no launch to a Solve: zerofixed = the periodic Solve of the same plan without
    subtract_average; multipole adds the moment prelude: centre of mass (rows, two axis sums, combine = 4) or the
    origin of the deck (1), then the moments (4) -- 8 and 5"""
    common = ["gravity/threshold=-1.0", "+gravity/niteration=2"]
    periodic = ["mesh/%sx%d_bc=periodic" % (s, q) for s in "io" for q in (1, 2, 3)]
    base = _launches(_sim(16, 8, common + periodic + ["gravity/mg_bc=none"]), sub_avg_off=True)
    assert base > 100
    assert _launches(_sim(16, 8, common + ["gravity/mg_bc=zerofixed"])) == base
    assert _launches(_sim(16, 8, common + ["gravity/mg_bc=zerograd", "mesh/ix3_bc=periodic", "mesh/ox3_bc=periodic"])) == base
    assert _launches(_sim(16, 8, common)) == base + 8
    assert _launches(_sim(16, 8, common + ["gravity/auto_mporigin=false",
                                           "+gravity/mporigin_x1=0.0\nmporigin_x2=0.0\nmporigin_x3=0.0"])) == base + 5
    assert _launches(_sim(16, 8, common + ["gravity/mg_bc=zerofixed", "+gravity/mask_radius=0.4"])) == base + 1


# ---- 6. the deck ---------------------------------------------------------------------------------------------------------
def test_binary_gravity_deck(tmp_path, capsys):
    """inputs/binary_gravity.athinput for its one cycle (rk1: one Solve, of the initial density): phi is the restated
    solve of the restated density, the four error numbers are those of tests/test_gravity_isolated_host.py, the
    final function prints them, grav_phi is written"""
    import derived_cases as dc
    text = open(os.path.join(ROOT, "athenak_amd", "inputs", "binary_gravity.athinput")).read()
    sim = dc.run_and_write(text, str(tmp_path), cycles=1)
    assert sim.pmesh.ncycle == 1
    want_phi, want_err, s = HT.binary_run(32, 16, "multipole")
    phi = _np(sim.phi())
    assert np.array_equal(phi, want_phi), np.abs(phi - want_phi).max()
    d = sim.pmesh.pmb_pack.pgrav.pmgd
    assert np.array_equal(d.mpcoeff(), s.mp) and np.array_equal(d.mporigin(), s.org)
    capsys.readouterr()
    err = sim.binary_gravity_errors()
    print("errors", err)
    assert err == want_err
    sim.pdriver.Finalize(sim.pmesh, sim.pin)
    out = capsys.readouterr().out
    for label, v in zip(("Potential    L2       : ", "Acceleration L2       : ", "Max Potential Error    : ",
                         "Max Acceleration Error : "), want_err):
        assert label + "%.16e" % v in out
    names, blocks = dc.read_bin(str(tmp_path/"bin"/"binary_gravity.grav_phi.00000.bin"))
    assert names == [b"grav_phi"] or names == ["grav_phi"]
    assert len(blocks) == 8
    for m, (_, data) in enumerate(blocks):
        assert np.array_equal(data[0], phi[m, 0, NG:-NG, NG:-NG, NG:-NG].astype(np.float32))


# ---- 7. the periodic Solve through the grown plan ---------------------------------------------------------------------
def test_periodic_solve_is_unchanged():
    """a plan whose new fields are zero: the existing restatement, as before"""
    import torch
    mesh, nb, L = (16, 8, 8), 8, (1.0, 0.5, 0.5)
    sim, _, _ = G._sim(mesh, ["gravity/niteration=2"])
    pk = sim.pmesh.pmb_pack
    d = pk.pgrav.pmgd
    lloc, u0, _ = G._density(sim, mesh, nb)
    pk.phydro.u0[:, 0].copy_(torch.from_numpy(u0[:, 0]).cuda())
    d.Solve()
    p = d.plan
    assert (p.mg_bc, p.mporder, p.nodipole, p.mask_radius) == (0, 0, 0, -1.0)
    p.periodic[:], p.mesh_ext[:], p.auto_mporigin, p.mask_radius, p.xlim = [0]*6, [0.0]*6, 0, 0.0, None
    s = R.MGSolver(mesh, nb, L, lloc, d.four_pi_G_, ng=NG, niteration=2, npresmooth=2, npostsmooth=2, full_multigrid=True)
    want = s.solve(pk.phydro.u0.cpu().numpy())
    assert np.array_equal(_np(pk.pgrav.phi), want)
    # the same plan with every new field zero, called directly
    co = C.c_int(d.coffset_)
    from athenak_amd import capi
    capi.check(d.L.akmi_mg_solve(p, pk.phydro.u0, pk.pgrav.phi, C.byref(co), d.norms, C.byref(d.ncycles), capi._stream()),
               "mg_solve")
    assert np.array_equal(_np(pk.pgrav.phi), s.solve(pk.phydro.u0.cpu().numpy()))
