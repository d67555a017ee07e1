"""Isolated self-gravity on the host, no GPU: the numpy restatement (tests/mg_isolated_restate.py) against the closed form
of the discrete Dirichlet problem, the multipole expansion against a direct sum, the two-sphere problem at two
resolutions, every refusal and fatal error of a deck with physical faces, and the level table."""
import functools
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mg_isolated_restate as I  # noqa: E402
import mg_restate as R  # noqa: E402
import test_gravity_host as H  # noqa: E402
from test_gravity_host import cpu_device  # noqa: E402,F401

NG = 2


# ---- 1. closed form, zerofixed ---------------------------------------------------------------------------------------
def dirichlet_problem(n, nb, lloc, x2_periodic):
    """rho = a few eigenvectors of the 7-point operator with the mirror ghost u(-1) = -u(0): products of
    sin((i + 1/2) p pi / N), eigenvalue sum_d (2 - 2 cos(p_d pi / N))/dx^2 (the ghost value -v(0) = sin(-(1/2) p pi / N)
    continues the sine).  With x2 periodic that direction takes sin(2 pi q (j + 1/2)/N) (eigenvalue 2 - 2 cos(2 pi q/N),
    as in test_gravity_host.sine_problem).  Mesh [0, 1]^3, four_pi_G = 1: lap(phi) = rho."""
    dx = 1.0/n
    c = np.arange(-NG, n + NG) + 0.5
    Z, Y, X = np.meshgrid(c, c, c, indexing="ij")

    def s(a, p, per=False):
        w = 2.0*np.pi*p/n if per else np.pi*p/n
        return np.sin(a*w), (2.0 - 2.0*np.cos(w))/dx**2
    rho, phi = 0.0, 0.0
    for amp, (p1, p2, p3) in ((0.7, (1, 1, 1)), (0.3, (3, 1, 2)), (-0.2, (2, 2, 5))):
        (f1, l1), (f2, l2), (f3, l3) = s(X, p1), s(Y, p2, x2_periodic), s(Z, p3)
        mode = amp*f1*f2*f3
        rho = rho + mode
        phi = phi - mode/(l1 + l2 + l3)
    u0 = np.zeros((len(lloc), 1) + (nb + 2*NG,)*3)
    ex = np.zeros((len(lloc),) + (nb,)*3)
    for m, (i, j, k) in enumerate(lloc):
        u0[m, 0] = rho[k*nb:k*nb + nb + 2*NG, j*nb:j*nb + nb + 2*NG, i*nb:i*nb + nb + 2*NG]
        ex[m] = phi[k*nb + NG:k*nb + nb + NG, j*nb + NG:j*nb + nb + NG, i*nb + NG:i*nb + nb + NG]
    return u0, ex


@pytest.mark.parametrize("x2_periodic", [False, True], ids=["six-faces", "x2-periodic"])
@pytest.mark.parametrize("fmg", [True, False], ids=["fmg", "mgi"])
def test_zerofixed_reaches_the_discrete_solution(fmg, x2_periodic):
    """16^3 with blocks of 8^3, threshold = 0.0: within 1e-10 of max|phi|, the bar of the periodic closed-form test"""
    n, nb = 16, 8
    lloc = R.row_major_lloc((2, 2, 2))
    u0, ex = dirichlet_problem(n, nb, lloc, x2_periodic)
    per = (0, 0, 1, 1, 0, 0) if x2_periodic else (0,)*6
    s = I.IsolatedSolver((n,)*3, nb, (0.0, 1.0)*3, lloc, 1.0, "zerofixed", periodic=per, ng=NG, threshold=0.0,
                         full_multigrid=fmg)
    phi = s.solve(u0)
    got = phi[:, 0, NG:-NG, NG:-NG, NG:-NG]
    err = np.abs(got - ex).max()/np.abs(ex).max()
    print("fmg", fmg, "x2 periodic", x2_periodic, "V-cycles", s.ncycles, "final defect", s.norms[-1], "error/max|phi|", err)
    assert err <= 1e-10
    # the one-deep ghost layer of phi is the physical-boundary ghost: -interior on a zerofixed face
    m = 0                                           # block (0, 0, 0): inner x1 face of the mesh
    assert np.array_equal(phi[m, 0, NG:-NG, NG:-NG, NG - 1], -phi[m, 0, NG:-NG, NG:-NG, NG])


# ---- 2. the expansion against a direct sum ---------------------------------------------------------------------------
def point_sources():
    """six cell sources of three unequal strengths and one sign on a 16^3 mesh over [-1/2, 1/2]^3, all within a of the
    origin, centre of mass away from it in x and y.  They come in pairs mirrored in z, so every moment odd in z
    vanishes -- among them the (l, m) = (3, 0) term, which the reference forms as z(z^2 - 3r^2) in the moments and in
    EvalMultipolePhi where the solid harmonic is z(5z^2 - 3r^2); the restatement keeps the reference's expression, and
    with that term non-zero the expansion would not be inside the bound at L = 4.
    Returns (src level array of one block, xlim, [(q, centre)], a)"""
    n = 16
    ext = np.array([[-0.5, 0.5]*3])
    src = np.zeros((1, n + 2, n + 2, n + 2))
    cells = [((8, 8, 8), 3.0), ((7, 8, 8), 3.0), ((9, 8, 6), 1.5), ((6, 8, 6), 1.5), ((8, 6, 9), 0.7), ((7, 6, 9), 0.7)]  # (k, j, i), src
    dx = 1.0/n
    pts = []
    for (k, j, i), v in cells:
        src[0, k + 1, j + 1, i + 1] = v
        pts.append((v*dx**3, np.array([-0.5 + (i + 0.5)*dx, -0.5 + (j + 0.5)*dx, -0.5 + (k + 0.5)*dx])))
    a = max(float(np.linalg.norm(c)) for _, c in pts)
    return src, ext, pts, a


def face_points(n=16):
    """the points EvalMultipolePhi is evaluated at by the boundary fill: face position x cell centres, six faces"""
    c = -0.5 + (np.arange(n) + 0.5)/n
    out = []
    for q in range(3):
        for f in (-0.5, 0.5):
            g = [c, c, c]
            g[q] = np.array([f])
            X, Y, Z = np.meshgrid(*g, indexing="ij")
            out.append(np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1))
    return np.concatenate(out)


def test_expansion_against_direct_sum():
    """|EvalMultipolePhi(moments) - sum q_c/(4 pi |r - r_c|)| <= sum|q_c|/(4 pi R) (a/R)^(L+1)/(1 - a/R) at every face
    point, R the distance of the nearest one: the tail of the Legendre series of 1/|r - r_c|, |P_l| <= 1.  Independent
    of the reference's scaling constants; the origin (0, 0, 0) is not the centre of mass, so the dipole terms count."""
    src, xlim, pts, a = point_sources()
    P = face_points()
    direct = sum(q/(4.0*np.pi*np.linalg.norm(P - c, axis=1)) for q, c in pts)
    Rmin = float(np.linalg.norm(P, axis=1).min())
    qabs = sum(abs(q) for q, _ in pts)
    errs = {}
    for L in (2, 4):
        mp, org = I.multipole(src, xlim, L, origin=(0.0, 0.0, 0.0))
        assert np.array_equal(org, np.zeros(3)) and mp[1:4].any() and (L == 4 or not mp[9:].any())
        got = I.eval_multipole_phi(P[:, 0], P[:, 1], P[:, 2], mp, L)
        errs[L] = float(np.abs(got - direct).max())
        bound = qabs/(4.0*np.pi*Rmin)*(a/Rmin)**(L + 1)/(1.0 - a/Rmin)
        print("L", L, "max error", errs[L], "bound", bound, "a/R", a/Rmin, "max|phi|", np.abs(direct).max())
        assert errs[L] <= bound
    assert errs[4] < errs[2]
    # auto_mporigin: the origin is the centre of mass, and the dipole about it vanishes to rounding
    mp, org = I.multipole(src, xlim, 4)
    com = sum(q*c for q, c in pts)/sum(q for q, _ in pts)
    assert np.abs(org - com).max() <= 1e-15
    assert np.abs(mp[1:4]).max() <= 1e-16*abs(mp[0])*16
    # nodipole drops terms 1-3 and nothing else
    nd, _ = I.multipole(src, xlim, 4, nodipole=True, origin=(0.0, 0.0, 0.0))
    full, _ = I.multipole(src, xlim, 4, origin=(0.0, 0.0, 0.0))
    assert not nd[1:4].any() and np.array_equal(np.delete(nd, [1, 2, 3]), np.delete(full, [1, 2, 3]))


def test_mask_zeroes_the_source_outside_the_radius():
    rng = np.random.default_rng(5)
    src = rng.standard_normal((1, 10, 10, 10))
    xlim = np.array([[-0.5, 0.5]*3])
    want = src.copy()
    org, rad = (0.03, -0.01, 0.02), 0.3
    I.apply_mask(src, xlim, rad, org)
    c = -0.5 + (np.arange(8) + 0.5)/8
    Z, Y, X = np.meshgrid(c, c, c, indexing="ij")
    out = (X - org[0])**2 + (Y - org[1])**2 + (Z - org[2])**2 > rad*rad
    assert 0 < out.sum() < out.size
    R.act(want)[0][out] = 0.0
    assert np.array_equal(src, want)


# ---- 3. the two spheres ----------------------------------------------------------------------------------------------
EXT = (-0.5, 0.5)*3


@functools.lru_cache(maxsize=None)
def binary_run(n, nb, mg_bc):
    """(phi, the four error numbers, solver) of the deck inputs/binary_gravity.athinput restated at n^3"""
    nrb = (n//nb,)*3
    lloc = R.row_major_lloc(nrb)
    xlim = I.block_extents(lloc, nrb, EXT)
    u0, total = I.binary_density(nb, xlim, NG)
    assert 0.7*3.0 < total < 1.3*3.0                  # the spheres are resolved: no mass notice
    s = I.IsolatedSolver((n,)*3, nb, EXT, lloc, 1.0, mg_bc, ng=NG, threshold=0.0, full_multigrid=True, mporder=4)
    phi = s.solve(u0)
    return phi, I.binary_errors(phi, nb, xlim, NG, EXT), s


def test_binary_density_has_the_masses():
    nrb = (2, 2, 2)
    xlim = I.block_extents(R.row_major_lloc(nrb), nrb, EXT)
    u0, _ = I.binary_density(16, xlim, NG)
    dv = (1.0/32)**3
    assert abs(u0[:, 0, NG:-NG, NG:-NG, NG:-NG].sum()*dv - 3.0) <= 1e-12
    # the spheres do not touch a block face by accident: both masses are there, 2 : 1 to the sub-sampling error
    left = sum(u0[m, 0, NG:-NG, NG:-NG, NG:-NG].sum() for m in (0, 2, 4, 6))*dv     # x < 0: sphere 2
    assert abs(left - 1.0) <= 0.02 and abs(u0[:, 0].sum()*dv - left - 2.0) <= 0.02


def test_binary_potential_converges_and_multipole_beats_zerofixed():
    """potential L2 error against the analytic two-sphere solution: falls from 16^3 to 32^3 under multipole, and at
    32^3 is below that of zerofixed on the same deck (phi = 0 on the faces instead of -G m/r)"""
    e16 = binary_run(16, 8, "multipole")[1]
    e32 = binary_run(32, 16, "multipole")[1]
    z32 = binary_run(32, 16, "zerofixed")[1]
    print("multipole 16^3", e16, "\nmultipole 32^3", e32, "\nzerofixed 32^3", z32)
    assert e32[0] < e16[0]
    assert e32[0] < z32[0]
    s = binary_run(32, 16, "multipole")[2]
    com = (2.0*0.125 + 1.0*(-0.25))/3.0
    assert abs(s.org[0] - com) <= 0.01 and np.abs(s.org[1:]).max() <= 1e-12
    assert abs(s.mp[0] - (-3.0)/(4.0*math.pi)) <= 1e-12       # the monopole: sum(src*vol)/(4 pi), src = -rho


# ---- 4. deck handling ------------------------------------------------------------------------------------------------
def _binary(extra=()):
    return H._deck("binary_gravity.athinput", extra)


PHYSICAL = ["mesh/ix1_bc=outflow", "mesh/ox1_bc=outflow"]        # on the (periodic) Jeans deck

REFUSALS = [
    # kept refusals
    ("jeans", PHYSICAL, ["periodic faces", "mg_bc", "<mesh>/ix1_bc = outflow"]),
    ("binary", ["gravity/mg_bc=none"], ["periodic faces", "mg_bc"]),
    ("jeans", ["+gravity/mg_bc=zerofixed"], ["mg_bc = zerofixed", "six periodic faces"]),
    ("jeans", ["+gravity/mg_bc=multipole"], ["mg_bc = multipole"]),
    ("jeans", ["+gravity/mask_radius=0.25"], ["mask_radius > 0", "strictly periodic"]),
    # the reference's own fatal errors
    ("binary", ["gravity/mg_bc=dirichlet"], ["in MGGravityDriver", "Unknown mg_bc type: dirichlet"]),
    ("jeans", ["+gravity/mg_bc=dirichlet"], ["Unknown mg_bc type: dirichlet"]),
    ("binary", ["gravity/mporder=3"], ["mporder must be 2 (quadrupole) or 4 (hexadecapole)."]),
    ("binary", ["+gravity/nodipole=true"], ["auto_mporigin and nodipole cannot be used together."]),
    ("binary", ["gravity/auto_mporigin=false"], ["Parameter name 'mporigin_x1' not found in block 'gravity'"]),
    ("binary", ["gravity/auto_mporigin=false", "+gravity/mporigin_x1=0.0\nmporigin_x2=0.0"], ["'mporigin_x3' not found"]),
    # still refused with physical faces
    ("binary", ["+mesh_refinement/refinement=static"], ["refinement = static"]),
    ("binary", ["+output2/file_type=rst\ndt=1.0"], ["rst outputs"]),
    ("binary", ["+gravity/mg_nghost=2"], ["mg_nghost = 2"]),
    ("binary", ["+gravity/root_on_host=true"], ["root_on_host = true"]),
]


@pytest.mark.parametrize("deck,extra,msgs", REFUSALS, ids=["%s-%s" % (r[0], r[2][-1][:40]) for r in REFUSALS])
def test_refusals_and_fatal_errors(cpu_device, deck, extra, msgs):  # noqa: F811
    pin = H._deck(extra=extra, drop_outputs=False) if deck == "jeans" else H._deck("binary_gravity.athinput", extra, False)
    with pytest.raises(RuntimeError) as e:
        H._mesh(pin)
    assert "### FATAL ERROR" in str(e.value)
    for msg in msgs:
        assert msg in str(e.value), str(e.value)


def test_refusals_ranks_restart_native(cpu_device):  # noqa: F811
    from athenak_amd.main import Simulation
    from athenak_amd.native import NativeSimulation
    with pytest.raises(RuntimeError, match="one rank"):
        H._mesh(_binary(), nranks=2)
    with pytest.raises(RuntimeError, match="-r of a deck with <gravity>"):
        Simulation(_binary(), restart=(None, None))
    with pytest.raises(RuntimeError, match="<gravity> runs on the Python host only"):
        NativeSimulation(_binary())


def test_accepted_decks_build_the_driver(cpu_device):  # noqa: F811
    d = H._mesh(_binary()).pmb_pack.pgrav.pmgd
    assert (d.mg_bc_, d.mporder_, d.autompo_, d.nodipole_, d.fsubtract_average_) == ("multipole", 4, True, False, False)
    assert d.periodic_ == [0]*6 and d.mask_radius_ == -1.0 and d.mesh_ext_ == list(EXT)
    assert (d.nrootlevel_, d.nmblevel_, d.eps_, d.full_multigrid_) == (2, 5, 0.0, True)
    with pytest.raises(RuntimeError, match="need <gravity>/mg_bc = multipole and a Solve"):
        d.mpcoeff()
    d = H._mesh(_binary(["gravity/mg_bc=zerograd", "mesh/ix2_bc=periodic", "mesh/ox2_bc=periodic",
                         "+gravity/mask_radius=0.4\nmask_origin_x1=0.1", "+gravity/subtract_average=true"])).pmb_pack.pgrav.pmgd
    assert (d.mg_bc_, d.mporder_, d.fsubtract_average_) == ("zerograd", -1, False)
    assert d.periodic_ == [0, 0, 1, 1, 0, 0] and (d.mask_radius_, d.mask_origin_) == (0.4, [0.1, 0.0, 0.0])
    d = H._mesh(_binary(["gravity/mporder=2", "gravity/auto_mporigin=false", "+gravity/nodipole=true",
                         "+gravity/mporigin_x1=0.1\nmporigin_x2=-0.2\nmporigin_x3=0.3"])).pmb_pack.pgrav.pmgd
    assert (d.mporder_, d.autompo_, d.nodipole_, d.mpo_) == (2, False, True, [0.1, -0.2, 0.3])
    # the periodic deck is what it was: subtract_average on, no boundary type
    d = H._mesh(H._deck()).pmb_pack.pgrav.pmgd
    assert (d.mg_bc_, d.fsubtract_average_, d.periodic_) == ("none", True, [1]*6)


def test_binary_gravity_generator_restated(cpu_device):  # noqa: F811
    """pgen_name = binary_gravity fills the density the restatement forms, bit for bit, at the deck's 32^3"""
    pm = H._mesh(_binary())
    from athenak_amd.pgen import ProblemGenerator
    pm.pgen = ProblemGenerator(_binary(), pm)
    pk = pm.pmb_pack
    lloc = [tuple(pm.lloc_eachmb[int(g)])[:3] for g in pk.pmb.mb_gid]
    xlim = I.block_extents(lloc, (2, 2, 2), EXT)
    assert np.array_equal(xlim, np.array([[s.x1min, s.x1max, s.x2min, s.x2max, s.x3min, s.x3max] for s in pk.pmb.mb_size]))
    want, _ = I.binary_density(16, xlim, NG)
    got = pk.phydro.u0.cpu().numpy()
    assert np.array_equal(got[:, 0], want[:, 0]) and not got[:, 1:].any()


# ---- 5. level bookkeeping ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,nb,want", H.LEVELS + [((32, 32, 32), 16, (2, 5, 6, 1)), ((16, 16, 16), 8, (2, 4, 5, 1))])
def test_level_table_is_unchanged(mesh, nb, want):
    from athenak_amd.gravity import level_counts
    assert level_counts(mesh, (nb, nb, nb)) == want
    nrb = tuple(n//nb for n in mesh)
    assert (R.root_levels(nrb), R.block_levels(nb)) == want[:2]
    if max(mesh) <= 32:                   # the restated solver with physical faces keeps the same levels
        s = I.IsolatedSolver(mesh, nb, (0.0, 1.0, 0.0, mesh[1]/mesh[0], 0.0, mesh[2]/mesh[0]), R.row_major_lloc(nrb), 1.0,
                             "zerofixed", niteration=1)
        assert (s.nrootlevel, s.nmblevel, s.ntotallevel) == want[:3]
