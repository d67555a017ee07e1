"""<gravity> on the host, no GPU: the numpy restatement of the multigrid solver (tests/mg_restate.py) against the closed
form of the discrete Poisson problem and at the reference's regression settings, the refusals of a deck with
<gravity>, and the level bookkeeping."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mg_restate as R  # noqa: E402
from athenak_amd import capi  # noqa: E402
from athenak_amd.parameter_input import ParameterInput  # noqa: E402

NG = 2


def sine_problem(mesh, nb, lloc, length=1.0):
    """rho - mean = a sum of two products of sines on [0, length] x [0, length*n2/n1] x [0, length*n3/n1] (cubic cells); the 7-point
    discrete solution of lap(phi) = four_pi_G*(rho - mean), four_pi_G = 1: every product of sines is an eigenvector
    of the periodic 7-point operator with eigenvalue -sum_d (2 - 2 cos(k_d dx))/dx^2.
    Returns (u0 (nmb, 1, nb+2ng, ..), phi_exact per block over the active cells)."""
    L = (length, length*mesh[1]/mesh[0], length*mesh[2]/mesh[0])
    dx = L[0]/mesh[0]
    ax = [(np.arange(-NG, mesh[q] + NG) + 0.5)*dx for q in range(3)]
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    k1, k2, k3 = 2*np.pi/L[0], 2*np.pi/L[1], 2*np.pi/L[2]

    def lam(*ks):
        return sum((2.0 - 2.0*np.cos(k*dx))/dx**2 for k in ks)
    m1 = 0.3*np.sin(k1*X)*np.sin(k2*Y)
    m2 = 0.2*np.sin(2*k1*X)*np.sin(k3*Z)
    rho = 1.0 + m1 + m2
    phi = -(m1/lam(k1, k2) + m2/lam(2*k1, k3))
    u0 = np.zeros((len(lloc), 1) + (nb + 2*NG,)*3)
    ex = np.zeros((len(lloc),) + (nb,)*3)
    for m, (i, j, k) in enumerate(lloc):
        u0[m, 0] = rho[k*nb:k*nb + nb + 2*NG, j*nb:j*nb + nb + 2*NG, i*nb:i*nb + nb + 2*NG]
        ex[m] = phi[k*nb + NG:k*nb + nb + NG, j*nb + NG:j*nb + nb + NG, i*nb + NG:i*nb + nb + NG]
    return L, u0, ex


# ---- 1. the restatement against the closed form -------------------------------------------------------------------
@pytest.mark.parametrize("mesh,nb", [((16, 8, 8), 8), ((12, 8, 8), 4)])
@pytest.mark.parametrize("fmg", [True, False])
def test_restated_solver_reaches_the_discrete_solution(mesh, nb, fmg):
    """threshold = 0.0 drives the solver to round-off: within 1e-10 of max|phi| (fp64 round-off times the condition
    number of a <= 32^3 grid is about 1e-13).  16x8x8 / 8^3: root grid 2x1x1, a block that is its own neighbour in two
    directions; 12x8x8 / 4^3: root grid 3x2x2, the iterative coarsest solve."""
    nrb = tuple(n//nb for n in mesh)
    lloc = R.row_major_lloc(nrb)
    L, u0, ex = sine_problem(mesh, nb, lloc)
    s = R.MGSolver(mesh, nb, L, lloc, 1.0, ng=NG, threshold=0.0, full_multigrid=fmg)
    phi = s.solve(u0)
    got = phi[:, 0, NG:-NG, NG:-NG, NG:-NG]
    err = np.abs(got - ex).max()/np.abs(ex).max()
    print("mesh", mesh, "fmg", fmg, "V-cycles", s.ncycles, "final defect", s.norms[-1], "error/max|phi|", err)
    assert err <= 1e-10
    # the ghost layer RetrieveResult copies is the periodic image
    assert np.array_equal(phi[0, 0, NG - 1, NG:-NG, NG:-NG],
                          phi[s.tab[0, 4], 0, -NG - 1, NG:-NG, NG:-NG])


def test_prolongations_reproduce_polynomials():
    """independent of the solver: the trilinear correction is exact for linear functions of cell centres, the
    tricubic FMG prolongation for quadratics (its per-axis weights (5, 30, -3)/32 interpolate a parabola)"""
    n = 4
    c = np.arange(-1, n + 1) + 0.5                   # coarse centres, ghosts included, width 1
    f = (np.arange(0, 2*n) + 0.5)*0.5                # fine centres, width 1/2
    Z, Y, X = np.meshgrid(c, c, c, indexing="ij")
    FZ, FY, FX = np.meshgrid(f, f, f, indexing="ij")
    coarse = (1.0 + 2.0*X - 3.0*Y + 0.5*Z)[None]
    fine = np.zeros((1, 2*n + 2, 2*n + 2, 2*n + 2))
    R.prolongate_correct(coarse, fine)
    assert np.abs(R.act(fine)[0] - (1.0 + 2.0*FX - 3.0*FY + 0.5*FZ)).max() < 1e-13
    q = lambda x, y, z: 1.0 + x*x - 2.0*y*y + 0.5*z*z + x*y - y*z + 3.0*z   # noqa: E731
    fine[...] = 7.0
    R.fmg_prolongate(q(X, Y, Z)[None], fine)
    assert np.abs(R.act(fine)[0] - q(FX, FY, FZ)).max() < 1e-12
    assert np.all(fine[0, 0] == 7.0) and np.all(fine[0, :, :, -1] == 7.0)


# ---- 2. convergence at the reference's regression settings ---------------------------------------------------------
def jeans_density(mesh, nb, lloc, n_jeans=2.0, amp=1.0e-6, rho0=1.0, cs=1.0):
    """the initial density of pgen_name = gravity (jeans_wave.cpp:113-145,207-213) and its four_pi_G"""
    L = (1.0, 0.5, 0.5)
    a3 = math.atan(L[0]/L[1])
    s3, c3 = math.sin(a3), math.cos(a3)
    a2 = math.atan(0.5*(L[0]*c3 + L[1]*s3)/L[2])
    s2, c2 = math.sin(a2), math.cos(a2)
    lam = min(L[0]*c2*c3, L[1]*c2*s3, L[2]*s2)
    lj = lam/n_jeans
    four_pi_G = 4*math.pi*(math.pi*cs*cs/(rho0*lj*lj))
    kw = 2.0*math.pi/lam
    dx = L[0]/mesh[0]
    ax = [(np.arange(-NG, mesh[q] + NG) + 0.5)*dx for q in range(3)]
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    x = c2*(X*c3 + Y*s3) + Z*s2
    rho = rho0*(1.0 + amp*np.sin(x*kw) + amp*amp*np.sin(X*kw))
    u0 = np.zeros((len(lloc), 1) + (nb + 2*NG,)*3)
    for m, (i, j, k) in enumerate(lloc):
        u0[m, 0] = rho[k*nb:k*nb + nb + 2*NG, j*nb:j*nb + nb + 2*NG, i*nb:i*nb + nb + 2*NG]
    return L, u0, four_pi_G


def test_restated_solver_convergence_at_regression_settings():
    """mesh 32x16x16, blocks 8^3, threshold 1e-8, FMG, 2+2 sweeps (the reference's test_jeans_solve_iterative): at
    most 4 V-cycles and a geometric-mean defect ratio <= 0.05 -- the reference's bars"""
    mesh, nb = (32, 16, 16), 8
    lloc = R.row_major_lloc((4, 2, 2))
    L, u0, fpg = jeans_density(mesh, nb, lloc)
    s = R.MGSolver(mesh, nb, L, lloc, fpg, ng=NG, threshold=1.0e-8, niteration=40, npresmooth=2, npostsmooth=2,
                   full_multigrid=True, fmg_ncycle=1)
    s.solve(u0)
    d = s.norms
    print("defects", d)
    assert d[-1] <= 1.0e-8
    assert len(d) - 1 <= 4
    ratios = [d[i + 1]/d[i] for i in range(len(d) - 1) if d[i] > 0]
    if ratios:
        assert math.exp(sum(math.log(r) for r in ratios)/len(ratios)) <= 0.05


# ---- 3. deck handling -------------------------------------------------------------------------------------------------
def _deck(name="jeans_wave.athinput", extra=(), drop_outputs=True):
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


REFUSALS = [
    (["+mesh_refinement/refinement=static"], "refinement = static"),
    (["+ion-neutral/drag_coeff=1.0"], "<ion-neutral>"),
    (["+output1/file_type=rst\ndt=1.0"], "rst outputs"),
    (["mesh/ox1_bc=outflow", "mesh/ix1_bc=outflow"], "periodic faces"),
    (["mesh/ix3_bc=reflect", "mesh/ox3_bc=reflect"], "periodic faces"),
    (["+gravity/mg_bc=multipole"], "mg_bc = multipole"),
    (["+gravity/mask_radius=0.25"], "mask_radius > 0"),
    (["+gravity/mg_nghost=2"], "mg_nghost = 2"),
    (["+gravity/root_on_host=true"], "root_on_host = true"),
    (["mesh/nx3=1", "meshblock/nx3=1", "mesh/x3max=1.0"], "works only in 3D"),
    (["mesh/nx2=1", "mesh/nx3=1", "meshblock/nx2=1", "meshblock/nx3=1"], "works only in 3D"),
    (["meshblock/nx1=16"], "logically cubic MeshBlock"),
    (["mesh/nx1=48", "mesh/nx2=24", "mesh/nx3=24", "meshblock/nx1=12", "meshblock/nx2=12", "meshblock/nx3=12"],
     "must be power of two"),
    (["mesh/x2max=1.0"], "cubic cells"),
    (["gravity/niteration=-1"], "Either \"threshold\" or \"niteration\" parameter must be set"),
    (["gravity/four_pi_G=-1.0"], "Gravitational constant must be set"),
]


@pytest.mark.parametrize("extra,msg", REFUSALS, ids=[r[1] for r in REFUSALS])
def test_refusals(cpu_device, extra, msg):
    pin = _deck(extra=extra)
    with pytest.raises(RuntimeError) as e:
        _mesh(pin)
    assert "### FATAL ERROR" in str(e.value) and msg in str(e.value), str(e.value)


def test_refusal_several_ranks(cpu_device):
    with pytest.raises(RuntimeError, match="one rank"):
        _mesh(_deck(), nranks=2)


def test_refusal_restart_and_native_host(cpu_device):
    from athenak_amd.main import Simulation
    from athenak_amd.native import NativeSimulation
    with pytest.raises(RuntimeError, match="-r of a deck with <gravity>"):
        Simulation(_deck(), restart=(None, None))
    with pytest.raises(RuntimeError, match="<gravity> runs on the Python host only"):
        NativeSimulation(_deck())


def test_grav_phi_output_needs_the_block(cpu_device):
    from athenak_amd.outputs import Outputs
    pin = _deck("linear_wave_hydro.athinput", ["+output1/file_type=bin\nvariable=grav_phi\ndt=1.0"])
    with pytest.raises(RuntimeError, match="output1' but gravity object not constructed"):
        Outputs(pin, _mesh(pin))
    pin = _deck(extra=["+output1/file_type=bin\nvariable=grav_phi\ndt=1.0"])
    out = Outputs(pin, _mesh(pin))
    assert [o.outvars for o in out.pout_list] == [[("grav_phi", 0, "phi")]]


def test_self_gravity_without_the_block_keeps_its_message(cpu_device):
    """a second guard next to tests/test_srcterms_host.py: the key is accepted only when <gravity> exists"""
    pin = _deck("rt2d.athinput", ["+hydro_srcterms/self_gravity=true"])
    with pytest.raises(RuntimeError) as e:
        _mesh(pin)
    assert "### FATAL ERROR" in str(e.value) and "self_gravity = true is not on this path" in str(e.value)


def test_accepted_deck_builds_gravity(cpu_device):
    pm = _mesh(_deck())
    pk = pm.pmb_pack
    assert pk.pgrav is not None and pk.phydro.psrc.self_gravity and pk.phydro.psrc.active
    assert pk.phydro.fused is False and pk.phydro.uflx is not None
    d = pk.pgrav.pmgd
    assert (d.npresmooth_, d.npostsmooth_, d.niter_, d.full_multigrid_, d.fmg_ncycle_) == (2, 2, 5, True, 1)
    assert (d.omega_, d.eps_, d.fsubtract_average_, d.fshowdef_) == (1.15, -1.0, True, 0)
    assert tuple(pk.pgrav.phi.shape) == (128, 1, 12, 12, 12) and float(pk.pgrav.phi.abs().max()) == 0.0
    # a deck without the block has no pgrav; the smoothing defaults are the multigrid driver's
    assert _mesh(_deck("linear_wave_hydro.athinput")).pmb_pack.pgrav is None
    pin = _deck(extra=[])
    del pin.blocks["gravity"]["npresmooth"], pin.blocks["gravity"]["npostsmooth"]
    d = _mesh(pin).pmb_pack.pgrav.pmgd
    assert (d.npresmooth_, d.npostsmooth_) == (1, 1)


# ---- 4. level bookkeeping ---------------------------------------------------------------------------------------------
LEVELS = [   # mesh, block edge -> nrootlevel, nmblevel, ntotallevel, ni: worked by hand from multigrid.cpp:100-145
    ((64, 32, 32), 8, (3, 4, 6, 2)),       # root 8x4x4 -> 4x2x2 -> 2x1x1
    ((16, 8, 8), 8, (1, 4, 4, 2)),         # root 2x1x1: one level, two sweeps on the coarsest grid
    ((12, 8, 8), 4, (1, 3, 3, 3)),         # root 3x2x2
    ((32, 16, 16), 8, (2, 4, 5, 2)),       # root 4x2x2 -> 2x1x1
    ((32, 32, 32), 8, (3, 4, 6, 1)),       # root 4^3 -> 2^3 -> 1
    ((24, 16, 16), 4, (2, 3, 4, 3)),       # root 6x4x4 -> 3x2x2
    ((16, 16, 16), 16, (1, 5, 5, 1)),      # one block
    ((128, 128, 128), 64, (2, 7, 8, 1)),
]


@pytest.mark.parametrize("mesh,nb,want", LEVELS)
def test_level_bookkeeping(mesh, nb, want):
    from athenak_amd.gravity import level_counts
    assert level_counts(mesh, (nb, nb, nb)) == want
    nrb = tuple(n//nb for n in mesh)
    assert (R.root_levels(nrb), R.block_levels(nb)) == want[:2]
