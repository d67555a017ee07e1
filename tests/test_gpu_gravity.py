"""gpu: the multigrid Poisson solver and the self-gravity source term on the device (csrc/akmi_mg.hip, gravity.py)
against the numpy restatement of tests/mg_restate.py, bit for bit; the discrete closed form; whole Jeans-wave runs at
the reference's regression settings; outputs of grav_phi and a run with turbulence driving, an acceleration and gravity.

The sums (average, defect norm) are restated in the library's documented order, so the norms too compare with
array_equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mg_restate as R  # noqa: E402
import test_gravity_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
NG = 2


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _call(name, *args):
    import torch
    from athenak_amd import capi
    L = capi.lib()
    conv = [capi._p(a) if isinstance(a, torch.Tensor) else a for a in args]
    capi.check(getattr(L, name)(*conv, capi._stream()), name)
    torch.cuda.synchronize()


def _bytes_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _ghost_mask(shape):
    m = np.ones(shape, dtype=bool)
    m[:, 1:-1, 1:-1, 1:-1] = False
    return m


ROOTS = {1: (1, 1, 1), 3: (3, 1, 1), 16: (4, 2, 2)}      # nmb -> root grid: 1 and 3 hold blocks that are their own neighbour


# ---- 1. every operator against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("nmb", [1, 3, 16])
@pytest.mark.parametrize("edge", [1, 2, 4, 8, 16])
def test_level_operators(edge, nmb):
    from athenak_amd.capi import d
    rng = np.random.default_rng(100*edge + nmb)
    sh = (nmb, edge + 2, edge + 2, edge + 2)
    g = (nmb, edge, edge, edge)
    dx, omega = 0.0625*3.0, 1.15
    u, src = rng.standard_normal(sh), rng.standard_normal(sh)
    gm = _ghost_mask(sh)
    # smooth: both colours, both offsets
    for color in (0, 1):
        for coffset in (0, 1):
            want = u.copy()
            R.smooth(want, src, dx, omega, color, coffset)
            got = _dev(u)
            _call("akmi_mg_smooth", *g, d(dx), d(omega), color, coffset, got, _dev(src))
            got = _np(got)
            assert np.array_equal(got, want), ("smooth", color, coffset)
            keep = gm | (want == u)                 # ghosts and the other colour: untouched, byte for byte
            assert _bytes_equal(got[keep], u[keep]) and keep.sum() >= u.size - (nmb*edge**3 + 1)//2 - nmb*edge**2
    # defect, FAS right-hand side
    dfc0 = rng.standard_normal(sh)
    want = dfc0.copy()
    R.defect(u, src, want, dx)
    got = _dev(dfc0)
    _call("akmi_mg_defect", *g, d(dx), _dev(u), _dev(src), got)
    assert np.array_equal(_np(got), want) and _bytes_equal(_np(got)[gm], dfc0[gm])
    want = src.copy()
    R.fas_rhs(u, want, dx)
    got = _dev(src)
    _call("akmi_mg_fas_rhs", *g, d(dx), _dev(u), got)
    assert np.array_equal(_np(got), want) and _bytes_equal(_np(got)[gm], src[gm])
    # exchange, with blocks that are their own neighbour
    tab = R.neighbor_table(R.row_major_lloc(ROOTS[nmb]), ROOTS[nmb])
    want = u.copy()
    R.exchange(want, tab)
    got = _dev(u)
    _call("akmi_mg_exchange", *g, _dev(tab.reshape(-1)), got)
    assert np.array_equal(_np(got), want) and _bytes_equal(_np(got)[~gm], u[~gm])
    # the whole-array operators
    n = C.c_longlong(u.size)
    a, b = _dev(u), _dev(src)
    _call("akmi_mg_store_old", n, a, b)
    assert _bytes_equal(_np(a), src)
    a = _dev(u)
    _call("akmi_mg_correction", n, a, b)
    assert np.array_equal(_np(a), u - src)
    _call("akmi_mg_copy_source", n, a, b)
    assert _bytes_equal(_np(a), src)
    _call("akmi_mg_zero_clear", n, a)
    assert not _np(a).any()
    # sums in the documented order: average, subtract, defect norm
    from athenak_amd import capi
    import torch
    ns = int(capi.lib().akmi_mg_reduce_scratch_doubles(*g))
    scratch, out = torch.zeros(ns, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    length = dx*float(edge)
    _call("akmi_mg_average", *g, d(dx), d(length), _dev(u), scratch, out)
    ave = R.average(u, dx, length)
    assert float(_np(out)[0]) == ave
    a = _dev(u)
    _call("akmi_mg_subtract_average", n, a, out)
    assert np.array_equal(_np(a), u - ave)
    vol = 0.75
    _call("akmi_mg_defect_norm", *g, d(vol), _dev(u), scratch, out)
    assert float(_np(out)[0]) == R.defect_norm(u, vol)
    # load / retrieve
    nvar = 3
    u0 = rng.standard_normal((nmb, nvar) + (edge + 2*NG,)*3)
    got = _dev(np.zeros(sh))
    _call("akmi_mg_load_source", *g, NG, nvar, d(-2.5), _dev(u0), got)
    assert np.array_equal(_np(got), R.load_source(u0, NG, -2.5))
    phi = rng.standard_normal((nmb, 1) + (edge + 2*NG,)*3)
    got = _dev(u)
    _call("akmi_mg_load_finest", *g, NG, _dev(phi), got)
    want = u.copy()
    R.act(want)[...] = phi[:, 0, NG:-NG, NG:-NG, NG:-NG]
    assert _bytes_equal(_np(got), want)
    got = _dev(phi)
    _call("akmi_mg_retrieve", *g, NG, _dev(u), got)
    want = phi.copy()
    want[:, 0, 1:-1, 1:-1, 1:-1] = u
    assert _bytes_equal(_np(got), want)
    # between levels: this level is the coarse one
    if edge <= 8:
        fsh = (nmb, 2*edge + 2, 2*edge + 2, 2*edge + 2)
        fine = rng.standard_normal(fsh)
        fgm = _ghost_mask(fsh)
        want = u.copy()
        R.restrict(fine, want)
        got = _dev(u)
        _call("akmi_mg_restrict", *g, _dev(fine), got)
        assert np.array_equal(_np(got), want) and _bytes_equal(_np(got)[gm], u[gm])
        for name, fn in (("akmi_mg_prolongate_correct", R.prolongate_correct), ("akmi_mg_fmg_prolongate", R.fmg_prolongate)):
            want = fine.copy()
            fn(u, want)
            got = _dev(fine)
            _call(name, *g, _dev(u), got)
            assert np.array_equal(_np(got), want), name
            assert _bytes_equal(_np(got)[fgm], fine[fgm])


@pytest.mark.parametrize("root", [(2, 1, 1), (3, 2, 2), (4, 2, 2)])
def test_root_grid_operators(root):
    """the root grid (nmb = 1, not cubic): smoother, boundary, restriction, and the transfers to and from the blocks"""
    from athenak_amd.capi import d
    rng = np.random.default_rng(sum(root))
    nx, ny, nz = root
    sh = (1, nz + 2, ny + 2, nx + 2)
    g = (1, nz, ny, nx)
    u, src, uold = rng.standard_normal(sh), rng.standard_normal(sh), rng.standard_normal(sh)
    for color in (0, 1):
        want = u.copy()
        R.smooth(want, src, 0.5, 1.15, color, 1)
        got = _dev(u)
        _call("akmi_mg_smooth", *g, d(0.5), d(1.15), color, 1, got, _dev(src))
        assert np.array_equal(_np(got), want)
    want = u.copy()
    R.root_boundary(want)
    got = _dev(u)
    _call("akmi_mg_root_boundary", nz, ny, nx, got)
    assert _bytes_equal(_np(got), want)
    if all(n % 2 == 0 for n in root) or root == (4, 2, 2):
        c = (1, nz//2 + 2, ny//2 + 2, nx//2 + 2)
        coarse = rng.standard_normal(c)
        want = coarse.copy()
        R.restrict(u, want)
        got = _dev(coarse)
        _call("akmi_mg_restrict", 1, nz//2, ny//2, nx//2, _dev(u), got)
        assert np.array_equal(_np(got), want)
    lloc = R.row_major_lloc(root)[::-1]                # any order of the blocks
    nmb = len(lloc)
    ll = _dev(np.array(lloc, dtype=np.int32).reshape(-1))
    bsrc, bu = rng.standard_normal((nmb, 3, 3, 3)), rng.standard_normal((nmb, 3, 3, 3))
    for init in (0, 1):
        wsrc, wu = src.copy(), u.copy()
        R.blocks_to_root(lloc, bsrc, bu, wsrc, wu, init)
        gsrc, gu = _dev(src), _dev(u)
        _call("akmi_mg_blocks_to_root", nmb, nz, ny, nx, ll, init, _dev(bsrc), _dev(bu), gsrc, gu)
        assert _bytes_equal(_np(gsrc), wsrc) and _bytes_equal(_np(gu), wu)
    for fold in (0, 1):
        wu, wold = bu.copy(), bsrc.copy()
        R.set_from_root(lloc, u, uold, wu, wold, fold)
        gu, gold = _dev(bu), _dev(bsrc)
        _call("akmi_mg_set_from_root", nmb, nz, ny, nx, ll, fold, _dev(u), _dev(uold), gu, gold)
        assert _bytes_equal(_np(gu), wu) and _bytes_equal(_np(gold), wold)


# ---- 2, 3. akmi_mg_solve against the restated Solve and against the closed form -----------------------------------
MESHES = {(16, 8, 8): (8, (1.0, 0.5, 0.5)), (12, 8, 8): (4, (1.5, 1.0, 1.0)), (32, 16, 16): (8, (1.0, 0.5, 0.5))}


def _sim(mesh, extra=()):
    from athenak_amd.main import Simulation
    nb, L = MESHES[mesh] if mesh in MESHES else (max(mesh[0]//4, 8), (1.0, 0.5, 0.5))
    over = ["mesh/nx1=%d" % mesh[0], "mesh/nx2=%d" % mesh[1], "mesh/nx3=%d" % mesh[2], "mesh/x1max=%r" % L[0],
            "mesh/x2max=%r" % L[1], "mesh/x3max=%r" % L[2]] + ["meshblock/nx%d=%d" % (q, nb) for q in (1, 2, 3)]
    pin = H._deck(extra=over + list(extra))
    return Simulation(pin), nb, L


def _density(sim, mesh, nb, scale=1.0):
    """the sine problem of the host test in the MeshBlock order of the mesh; returns (u0 numpy, exact phi)"""
    pm = sim.pmesh
    lloc = [tuple(pm.lloc_eachmb[int(g)])[:3] for g in pm.pmb_pack.pmb.mb_gid]
    _, u0, ex = H.sine_problem(mesh, nb, lloc, MESHES[mesh][1][0])
    if scale != 1.0:
        u0 = 1.0 + (u0 - 1.0)*scale
    return lloc, u0, ex


@pytest.mark.parametrize("mode", ["niter2", "thr1e-8"])
@pytest.mark.parametrize("fmg", [True, False], ids=["fmg", "mgi"])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_solve_matches_restated_solve(mesh, fmg, mode):
    import torch
    stop = ["gravity/niteration=2"] if mode == "niter2" else ["gravity/niteration=40", "+gravity/threshold=1.0e-8"]
    sim, nb, L = _sim(mesh, stop + ["gravity/full_multigrid=%s" % ("true" if fmg else "false")])
    pk = sim.pmesh.pmb_pack
    d = pk.pgrav.pmgd
    lloc, u0, _ = _density(sim, mesh, nb)
    s = R.MGSolver(mesh, nb, L, lloc, d.four_pi_G_, ng=NG, threshold=d.eps_, niteration=d.niter_, npresmooth=2,
                   npostsmooth=2, full_multigrid=fmg)
    assert (s.nrootlevel, s.nmblevel) == (d.nrootlevel_, d.nmblevel_)
    for call, scale in enumerate((1.0, 1.7)):          # the second call starts from the first: coffset_, initial guess
        _, u0, _ = _density(sim, mesh, nb, scale)
        pk.phydro.u0[:, 0].copy_(torch.from_numpy(u0[:, 0]).cuda())
        d.Solve()
        want = s.solve(pk.phydro.u0.cpu().numpy())
        assert np.array_equal(_np(pk.pgrav.phi), want), (call, np.abs(_np(pk.pgrav.phi) - want).max())
        assert d.coffset_ == s.coffset
        if mode != "niter2":
            assert d.ncycles.value == s.ncycles and np.array_equal(np.array(d.last_norms), np.array(s.norms))
            assert d.last_norms[-1] <= 1.0e-8


@pytest.mark.parametrize("mesh", [(16, 8, 8), (12, 8, 8)])
def test_solve_reaches_the_discrete_solution(mesh):
    """the closed form of tests/test_gravity_host.py through the device path, same tolerance: 1e-10 of max|phi|"""
    import torch
    sim, nb, L = _sim(mesh, ["+gravity/threshold=0.0", "problem/n_jeans=-1.0"])
    pk = sim.pmesh.pmb_pack
    assert pk.pgrav.pmgd.four_pi_G_ == 1.0
    _, u0, ex = _density(sim, mesh, nb)
    pk.phydro.u0[:, 0].copy_(torch.from_numpy(u0[:, 0]).cuda())
    pk.pgrav.pmgd.Solve()
    got = _np(sim.phi())[:, 0, NG:-NG, NG:-NG, NG:-NG]
    err = np.abs(got - ex).max()/np.abs(ex).max()
    print("mesh", mesh, "V-cycles", pk.pgrav.pmgd.ncycles.value, "error/max|phi|", err)
    assert err <= 1e-10


# ---- 4. the source term ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmb", [1, 3])
@pytest.mark.parametrize("nx", [(4, 4, 4), (13, 7, 5)])
@pytest.mark.parametrize("ideal", [True, False], ids=["ideal", "isothermal"])
@pytest.mark.parametrize("mhd", [False, True], ids=["hydro", "mhd"])
def test_selfgravity_term(mhd, ideal, nx, nmb):
    from athenak_amd import capi
    rng = np.random.default_rng(nmb + nx[0])
    nvar = 5 if ideal else 4
    n1, n2, n3 = (n + 2*NG for n in nx)
    f = 1 if mhd else 0                           # the MHD flux arrays are face-shaped, the hydro ones cell-shaped
    w0, u0 = rng.standard_normal((nmb, nvar, n3, n2, n1)), rng.standard_normal((nmb, nvar, n3, n2, n1))
    phi = rng.standard_normal((nmb, 1, n3, n2, n1))
    flx = [rng.standard_normal((nmb, nvar, n3, n2, n1 + f)), rng.standard_normal((nmb, nvar, n3, n2 + f, n1)),
           rng.standard_normal((nmb, nvar, n3 + f, n2, n1))]
    dx = np.abs(rng.standard_normal((nmb, 3))) + 0.1
    bdt = 0.0371
    want = u0.copy()
    R.self_gravity(w0, phi, flx, want, dx, bdt, NG, ideal)
    dxd = _dev(dx)
    pack = capi.Pack(nmb, nvar, nx[0], nx[1], nx[2], NG, dxd.data_ptr(), 1.4, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0,
                     1 if ideal else 0)
    got = _dev(u0)
    _call("akmi_mg_selfgravity", C.byref(pack), f, capi.d(bdt), _dev(w0), _dev(phi), *[_dev(x) for x in flx], got)
    got = _np(got)
    assert np.array_equal(got, want)
    a = (slice(None), slice(None), slice(NG, -NG), slice(NG, -NG), slice(NG, -NG))
    untouched = np.ones(u0.shape, dtype=bool)
    untouched[a] = False
    untouched[:, 0] = True                        # the density is never written
    assert _bytes_equal(got[untouched], u0[untouched])
    assert not np.array_equal(got[:, 1:4], u0[:, 1:4])


# ---- 5. whole runs: the Jeans wave at the reference's regression settings ------------------------------------------
def _jeans_error(res, n_jeans, fmg):
    from athenak_amd.main import Simulation
    mb = max(res//4, 8)
    over = ["mesh/nx1=%d" % res, "mesh/nx2=%d" % (res//2), "mesh/nx3=%d" % (res//2)] + \
           ["meshblock/nx%d=%d" % (q, mb) for q in (1, 2, 3)] + \
           ["time/tlim=0.1", "time/cfl_number=0.3", "problem/n_jeans=%r" % n_jeans, "problem/amp=1.0e-6",
            "gravity/niteration=4", "gravity/npresmooth=2", "gravity/npostsmooth=2",
            "gravity/full_multigrid=%s" % ("true" if fmg else "false")]
    sim = Simulation(H._deck(extra=over))
    sim.Execute()
    sim.pdriver.Finalize(sim.pmesh, sim.pin)
    err = abs(sim.omega_measured - sim.omega_analytical)/sim.omega_analytical
    print("res", res, "n_jeans", n_jeans, "fmg", fmg, "cycles", sim.pmesh.ncycle, "omega", sim.omega_measured,
          sim.omega_analytical, "rel. error", err)
    return err


@pytest.mark.parametrize("fmg", [True, False], ids=["fmg", "mgi"])
def test_jeans_stable_convergence(fmg):
    """n_jeans = 0.5, resolutions 32 and 64: relative omega error <= 0.01 at 64, error ratio <= 0.3 (the reference's)"""
    e = [_jeans_error(res, 0.5, fmg) for res in (32, 64)]
    assert e[-1] <= 0.01
    assert e[-1]/e[-2] <= 0.3


@pytest.mark.parametrize("fmg", [True, False], ids=["fmg", "mgi"])
def test_jeans_unstable_convergence(fmg):
    """n_jeans = 2, resolutions 16 and 32: relative growth-rate error <= 0.03 at 32, error ratio <= 0.3"""
    e = [_jeans_error(res, 2.0, fmg) for res in (16, 32)]
    assert e[-1] <= 0.03
    assert e[-1]/e[-2] <= 0.3


# ---- 6. outputs and a combined run ------------------------------------------------------------------------------------
def test_grav_phi_outputs(tmp_path):
    import derived_cases as dc
    text = open(os.path.join(ROOT, "athenak_amd", "inputs", "jeans_wave.athinput")).read()
    text = text[:text.index("<output1>")].replace("nx1       = 64", "nx1       = 16").replace(
        "nx2       = 32", "nx2       = 8").replace("nx3       = 32", "nx3       = 8")
    text += ("<output1>\nfile_type = bin\nvariable = grav_phi\ndcycle = 1\n"
             "<output2>\nfile_type = tab\nvariable = grav_phi\nslice_x2 = 0.2\nslice_x3 = 0.3\ndata_format = %24.16e\ndcycle = 1\n")
    sim = dc.run_and_write(text, str(tmp_path), cycles=2)
    phi = _np(sim.phi())
    assert np.abs(phi).max() > 0.0
    ind = sim.pmesh.mb_indcs
    names, blocks = dc.read_bin(str(tmp_path/"bin"/"jeans_wave.grav_phi.00000.bin"))
    assert names == ["grav_phi"] and len(blocks) == phi.shape[0]
    for m, (_, data) in enumerate(blocks):
        assert np.array_equal(data[0], phi[m, 0, NG:-NG, NG:-NG, NG:-NG].astype(np.float32))
    head, rows = dc.read_tab(str(tmp_path/"tab"/"jeans_wave.grav_phi.00000.tab"))
    assert head[-1] == "grav_phi" and len(rows) == 16
    size = sim.pmesh.pmb_pack.pmb.mb_size
    for r in rows:
        m, i = int(r[0]), int(r[1])
        s = size[m]
        j = int(((0.2 - s.x2min)/(s.x2max - s.x2min))*float(ind.nx2)) + NG
        k = int(((0.3 - s.x3min)/(s.x3max - s.x3min))*float(ind.nx3)) + NG
        assert float(r[3]) == phi[m, 0, k, j, i]


COMBINED = """
<job>
basename = turb_grav
<mesh>
nghost = 2
nx1 = 16
x1min = 0.0
x1max = 1.0
nx2 = 16
x2min = 0.0
x2max = 1.0
nx3 = 16
x3min = 0.0
x3max = 1.0
<meshblock>
nx1 = 8
nx2 = 8
nx3 = 8
<time>
integrator = rk2
cfl_number = 0.3
nlim = 3
tlim = 1.0
<mhd>
eos = ideal
gamma = 1.6666666666666667
reconstruct = plm
rsolver = hlld
<mhd_srcterms>
const_accel = true
const_accel_val = 0.1
const_accel_dir = 3
self_gravity = true
<gravity>
four_pi_G = 2.0
niteration = 2
full_multigrid = true
<turb_driving>
tcorr = 0.5
dedt = 0.1
nlow = 1
nhigh = 2
<problem>
pgen_name = turb
"""


def test_turbulence_acceleration_and_gravity_run():
    from athenak_amd.main import Simulation
    from athenak_amd.parameter_input import ParameterInput
    sim = Simulation(ParameterInput(text=COMBINED))
    u = sim.phys.u0
    a = (slice(None), slice(None), slice(NG, -NG), slice(NG, -NG), slice(NG, -NG))
    before = _np(u)[a].sum(axis=(0, 2, 3, 4))
    assert sim.Execute() == 3
    after = _np(u)[a]
    assert np.isfinite(after).all() and np.isfinite(_np(sim.phi())).all() and np.abs(_np(sim.phi())).max() > 0.0
    tot = after.sum(axis=(0, 2, 3, 4))
    print("sums of the conserved variables before", before, "after", tot, "change", tot - before)
    # periodic box, conservative update, no mass source.  Round-off: 4096 cells of density one, each changed by at
    # most 6 stages x 8 roundings of 1.1e-16, summed in the worst case: 2.2e-11 (the pairwise sum adds 5e-12)
    assert abs(tot[0] - before[0]) <= 4096*6*8*1.1e-16 + 5e-12
