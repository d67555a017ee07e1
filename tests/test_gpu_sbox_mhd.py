"""gpu: the MHD shearing box -- the new entries of csrc/akmi_sbox.hip against the restatement of
tests/sbox_mhd_restate.py, bit for bit, through the objects MHD creates (ShearingBoxCC, ShearingBoxFC, OrbitalAdvectionFC:
their tables are under test as well), then whole runs: a zero-shear run against the plain periodic MHD run, the user
history of the MHD shearing wave, div B after 20 cycles against the same run without the box, and the command line.

Every mesh has a different, non-dyadic cell width per direction; data are random."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sbox_mhd_restate as M  # noqa: E402
import sbox_restate as R  # noqa: E402
from test_gpu_sbox import ORB, SENTINEL, SRC_SHAPES, XMAX, XMIN, make_sim, read_hst, restate_pack, shear_offsets, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0**-52
SHWAVE4 = "pgen_name = shwave\nipert = 4\nd0 = 1.0\namp = 1.0e-6\nnwx = -2\nnwy = 1\nnwz = %d\nbeta = 20"


def deck_text(nx, nmb, ng, xmin=XMIN, xmax=XMAX, recon="plm", rsolver="hlle", eos="isothermal", nscalars=0, qshear=1.5,
              omega0=1.0, stratified=False, x1_bc="shear_periodic", cfl=0.3, integrator="rk2", tlim=1.0, nlim=-1,
              problem=None, sbox=True, extra="", fused=None):
    """the MHD twin of test_gpu_sbox.deck_text.  nx: cells of a MeshBlock, nmb: MeshBlocks per direction"""
    mhd = "eos = %s\nreconstruct = %s\nrsolver = %s\n" % (eos, recon, rsolver)
    mhd += "gamma = 1.4\n" if eos == "ideal" else "iso_sound_speed = 1.0\n"
    if nscalars:
        mhd += "nscalars = %d\n" % nscalars
    if fused is not None:
        mhd += "fused_stage = %s\n" % fused
    mesh = "nghost = %d\n" % ng
    for d in range(3):
        bc = x1_bc if d == 0 else "periodic"
        mesh += "nx%d = %d\nx%dmin = %r\nx%dmax = %r\nix%d_bc = %s\nox%d_bc = %s\n" % (
            d + 1, nx[d]*nmb[d], d + 1, xmin[d], d + 1, xmax[d], d + 1, bc, d + 1, bc)
    sb = "<shearing_box>\nqshear = %r\nomega0 = %r\nstratified = %s\n" % (qshear, omega0, "true" if stratified else "false")
    if problem is None:
        problem = SHWAVE4 % (1 if nx[2] > 1 else 0)
    return ("<job>\nbasename = sbox\n<mesh>\n%s<meshblock>\nnx1 = %d\nnx2 = %d\nnx3 = %d\n<time>\nevolution = dynamic\n"
            "integrator = %s\ncfl_number = %r\nnlim = %d\ntlim = %r\n%s<mhd>\n%s<problem>\n%s\n%s"
            % (mesh, nx[0], nx[1], nx[2], integrator, cfl, nlim, tlim, sb if sbox else "", mhd, problem, extra))


def face_tensors(sim):
    b = sim.phys.b0
    return b.x1f, b.x2f, b.x3f


def set_faces(sim, arrays):
    for t, a in zip(face_tensors(sim), arrays):
        assert tuple(t.shape) == a.shape
        t.copy_(to_dev(a))


def get_faces(sim):
    return tuple(t.cpu().numpy() for t in face_tensors(sim))


# ---- source terms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strat", [False, True])
@pytest.mark.parametrize("eos", ["ideal", "isothermal"])
@pytest.mark.parametrize("nx,nmb,ng", SRC_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_source_terms_bitwise(nx, nmb, ng, eos, strat):
    recon = "plm" if ng == 2 else "ppmx"
    sim = make_sim(deck_text(nx, nmb, ng, recon=recon, eos=eos, nscalars=2, stratified=strat,
                             rsolver="hlld" if eos == "ideal" else "hlle"))
    ph = sim.phys
    pk = restate_pack(sim, nx, nmb, ng)
    rng = np.random.default_rng(5)
    shape = pk.shape(ph.nvars)
    assert tuple(ph.u0.shape) == shape and tuple(ph.bcc0.shape) == pk.shape(3)
    w0 = rng.standard_normal(shape)
    w0[:, 0] = rng.uniform(0.5, 1.5, w0[:, 0].shape)
    bcc0 = rng.standard_normal(pk.shape(3))
    u0 = np.full(shape, SENTINEL)
    a = (slice(None), slice(None), slice(pk.ks, pk.ke + 1), slice(pk.js, pk.je + 1), slice(pk.is_, pk.ie + 1))
    u0[a] = rng.standard_normal(u0[a].shape)
    bdt = 0.0137
    want = M.source_terms_mhd(pk, w0, bcc0, u0, bdt, 1.5, 1.0, eos == "ideal", strat)
    ut = to_dev(u0)
    ph.psbox_u.SourceTermsCC(to_dev(w0), bdt, ut, bcc0=to_dev(bcc0))
    got = ut.cpu().numpy()
    assert np.array_equal(got, want)
    ghost = np.ones(shape, dtype=bool)
    ghost[a] = False
    assert (got[ghost] == SENTINEL).all() and not np.array_equal(got[a], u0[a])
    changed = [n for n in range(ph.nvars) if not np.array_equal(got[:, n], u0[:, n])]
    other = 2 if nx[2] > 1 else 3
    want_changed = sorted({1, other} | ({3} if strat and nx[2] > 1 else set()) | ({4} if eos == "ideal" else set()))
    assert changed == want_changed
    if eos == "ideal":
        # the Maxwell stress is in: the hydro form gives another energy
        hyd = R.source_terms_cc(pk, w0, u0, bdt, 1.5, 1.0, True, strat)
        assert not np.array_equal(hyd[:, 4], want[:, 4]) and np.array_equal(hyd[:, :4], want[:, :4])


@pytest.mark.parametrize("nx,nmb", [((16, 8, 1), (1, 2, 1)), ((65, 5, 1), (2, 1, 1))])
def test_efield_2d_bitwise(nx, nmb):
    ng = 2
    sim = make_sim(deck_text(nx, nmb, ng))
    ph = sim.phys
    pk = restate_pack(sim, nx, nmb, ng)
    rng = np.random.default_rng(nx[0])
    b1, b2, _ = (rng.standard_normal(s) for s in M.face_shapes(pk))
    e1 = rng.standard_normal(tuple(ph.efld.x1e.shape))
    e2 = rng.standard_normal(tuple(ph.efld.x2e.shape))
    e3 = rng.standard_normal(tuple(ph.efld.x3e.shape))
    assert e1.shape == (pk.nmb, 2, pk.N2 + 1, pk.N1) and e2.shape == (pk.nmb, 2, pk.N2, pk.N1 + 1)
    want1, want2 = M.efield_2d(pk, b1, b2, e1, e2, 1.5, 1.0)
    ph.b0.x1f.copy_(to_dev(b1))
    ph.b0.x2f.copy_(to_dev(b2))
    ph.efld.x1e.copy_(to_dev(e1))
    ph.efld.x2e.copy_(to_dev(e2))
    ph.efld.x3e.copy_(to_dev(e3))
    ph.psbox_b.SourceTermsFC(ph.b0, ph.efld)
    got1, got2 = ph.efld.x1e.cpu().numpy(), ph.efld.x2e.cpu().numpy()
    assert np.array_equal(got1, want1) and np.array_equal(got2, want2) and np.array_equal(ph.efld.x3e.cpu().numpy(), e3)
    assert not np.array_equal(got1, e1) and not np.array_equal(got2, e2)
    # only j in [js, je+1], i in [is, ie+1] changed
    for got, old in ((got1, e1), (got2, e2)):
        mask = np.ones(old.shape, dtype=bool)
        mask[:, :, pk.js:pk.je + 2, pk.is_:pk.ie + 2] = False
        assert np.array_equal(got[mask], old[mask])


# ---- shear-periodic x1 boundary of b0 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ng,recon", [(2, "plm"), (2, "dc"), (3, "ppmx"), (4, "ppmx")])
@pytest.mark.parametrize("nmbx2", [1, 2, 3])
@pytest.mark.parametrize("nx2", [8, 60, 61])
def test_shear_boundary_fc_bitwise(nx2, nmbx2, ng, recon):
    import torch
    nx, nmb = (6, nx2, 4), (2, nmbx2, 1)
    sim = make_sim(deck_text(nx, nmb, ng, recon=recon))
    ph = sim.phys
    pk = restate_pack(sim, nx, nmb, ng)
    sb = ph.psbox_b
    assert sb.nmb_x1bndry == [nmbx2, nmbx2]
    rng = np.random.default_rng(nx2*10 + nmbx2)
    b = tuple(rng.standard_normal(s) for s in M.face_shapes(pk))
    dx2 = float(pk.dx[0, 1])
    # what may change: x1 ghost faces, planes 0..N3-1, rows 0..N2-1
    may = []
    for v, s in enumerate(M.face_shapes(pk)):
        mk = np.zeros(s, dtype=bool)
        mk[:, :pk.N3, :pk.N2, :ng] = True
        c0 = pk.ie + 2 if v == 0 else pk.ie + 1
        mk[:, :pk.N3, :pk.N2, c0:c0 + ng] = True
        may.append(mk)
    cases = set()
    for yshear in shear_offsets(nx2, ng, dx2):
        joffset = int(yshear/dx2)
        jr = joffset % nx2
        cases.add((1 if jr < ng else (2 if jr < nx2 - ng else 3), min(joffset//nx2, 1)))
        want = M.shear_boundary_fc(pk, b, yshear, recon)
        assert all(np.isfinite(w).all() for w in want)
        set_faces(sim, b)
        sb.yshear = yshear
        sb.PackAndSendFC(ph.b0, ph.recon_method)
        sb.RecvAndUnpackFC(ph.b0)
        torch.cuda.synchronize()
        got = get_faces(sim)
        for v in range(3):
            assert np.array_equal(got[v], want[v]), (yshear/dx2, v, np.argwhere(got[v] != want[v])[:4])
            # (each block lies on one of the two x1 faces: half of the ghost faces of the mesh are remapped)
            assert np.array_equal(got[v][~may[v]], b[v][~may[v]]) and (got[v][may[v]] != b[v][may[v]]).mean() > 0.45
    want_cases = {(1, 0), (3, 0), (1, 1), (3, 1)} | ({(2, 0), (2, 1)} if ng <= nx2//2 < nx2 - ng else set())
    assert want_cases <= cases
    # yshear = 0: the boundary leaves exactly what the periodic exchange wrote.  Of a single-valued field, that is: the
    # gather fills row je+1 of x2f from row js of the next block, which is the same face (the random arrays above give the
    # two copies of a shared face different values, and then either copy is a legitimate ghost value)
    set_faces(sim, M.divfree_field(pk, rng))
    ph.pbval_b.PackAndSendFC(ph.b0)
    ph.pbval_b.RecvAndUnpackFC(ph.b0)
    before = [t.clone() for t in face_tensors(sim)]
    sb.yshear = 0.0
    sb.PackAndSendFC(ph.b0, ph.recon_method)
    sb.RecvAndUnpackFC(ph.b0)
    assert [torch.equal(t, o) for t, o in zip(face_tensors(sim), before)] == [True, True, True]


# ---- orbital advection of b0 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx1,nx2,nmbx2,ng,recon", ORB)
def test_orbital_advection_fc_bitwise(nx1, nx2, nmbx2, ng, recon):
    """x1 in [-2.13, 2.13], cfl = 0.9: maxjshift = 2; dt moves the faces at |x1| = 2.13 by 2.5 cells, so joffset runs through
    -2 .. 2 across the block and changes sign in its middle.  Two blocks along x1 in the last case share an x1 face."""
    nx, nmb = (nx1, nx2, 3), (1, nmbx2, 1)
    xmin, xmax = (-2.13, XMIN[1], XMIN[2]), (2.13, XMAX[1], XMAX[2])
    sim = make_sim(deck_text(nx, nmb, ng, xmin, xmax, recon=recon, cfl=0.9, eos="ideal", rsolver="hlld"))
    ph = sim.phys
    pk = restate_pack(sim, nx, nmb, ng, xmin, xmax)
    orb = ph.porb_b
    assert orb.maxjshift == 2
    dx2 = float(pk.dx[0, 1])
    dt = 2.5*dx2/(1.5*2.13)
    joffs = {int(-(1.5)*float(M.LeftEdgeX(i, nx1, xmin[0], xmax[0]))*dt/dx2) for i in range(nx1 + 1)}
    assert {0, 1, -1, 2, -2} <= joffs and max(joffs) == 2 and min(joffs) == -2
    b = M.divfree_field(pk, np.random.default_rng(nx1 + nx2))
    want, jmax, emfx, emfz = M.orbital_advection_fc(pk, b, 1.5, 1.0, dt, orb.maxjshift, recon)
    assert jmax == 2 == orb.max_joffset(dt)
    set_faces(sim, b)
    sim.pmesh.dt = dt
    orb.RecvAndUnpackFC(ph.b0, ph.recon_method)
    got = get_faces(sim)
    K, J, I = slice(pk.ks, pk.ke + 1), slice(pk.js, pk.je + 1), slice(pk.is_, pk.ie + 1)
    K1, J1, I1 = slice(pk.ks, pk.ke + 2), slice(pk.js, pk.je + 2), slice(pk.is_, pk.ie + 2)
    assert np.array_equal(orb.emfx.cpu().numpy()[:, K1, J1, I1], emfx[:, K1, J1, I1])
    assert np.array_equal(orb.emfz.cpu().numpy()[:, K1, J1, I1], emfz[:, K1, J1, I1])
    upd = [(K, J, I1), (K, J1, I), (K1, J, I)]
    for v in range(3):
        assert np.array_equal(got[v], want[v]), (v, np.argwhere(got[v] != want[v])[:4])
        mask = np.ones(got[v].shape, dtype=bool)
        mask[(slice(None),) + upd[v]] = False
        assert np.array_equal(got[v][mask], b[v][mask]) and not np.array_equal(got[v], b[v])
    bmax = max(np.abs(f).max() for f in b)
    change = np.abs(M.div_b(pk, got) - M.div_b(pk, b)).max()
    bound = M.ct_divb_bound(pk, recon, orb.maxjshift, bmax)
    print("largest change of div B", change, "bound", bound, "div B before", np.abs(M.div_b(pk, b)).max())
    assert change <= bound
    for m in range(pk.nmb):
        hi = pk.neighbour(m, 0, 1, 0)
        assert np.array_equal(got[1][m][K, pk.je + 1, I], got[1][hi][K, pk.js, I])


def test_orbital_advection_fc_shared_x1_face():
    """two blocks along x1 (and two along x2): x1f at ie+1 of the inner block and at is of the outer one are the same face,
    shifted by the same LeftEdgeX, and get the same bits; so do the shared x2f faces"""
    nx, nmb, ng = (8, 8, 3), (2, 2, 1), 3
    xmin, xmax = (-2.13, XMIN[1], XMIN[2]), (2.13, XMAX[1], XMAX[2])
    sim = make_sim(deck_text(nx, nmb, ng, xmin, xmax, recon="ppmx", cfl=0.9))
    ph = sim.phys
    pk = restate_pack(sim, nx, nmb, ng, xmin, xmax)
    dt = 2.5*float(pk.dx[0, 1])/(1.5*2.13)
    b = M.divfree_field(pk, np.random.default_rng(7))
    want, jmax, _, _ = M.orbital_advection_fc(pk, b, 1.5, 1.0, dt, 2, "ppmx")
    set_faces(sim, b)
    sim.pmesh.dt = dt
    ph.porb_b.RecvAndUnpackFC(ph.b0, ph.recon_method)
    got = get_faces(sim)
    assert jmax == 2 and all(np.array_equal(g, w) for g, w in zip(got, want))
    K, J, I = slice(pk.ks, pk.ke + 1), slice(pk.js, pk.je + 1), slice(pk.is_, pk.ie + 1)
    for m, l in enumerate(pk.lloc):
        hi = pk.neighbour(m, 0, 1, 0)
        assert np.array_equal(got[1][m][K, pk.je + 1, I], got[1][hi][K, pk.js, I])
        if l[0] == 0:
            right = pk.neighbour(m, 1, 0, 0)
            assert np.array_equal(got[0][m][K, J, pk.ie + 1], got[0][right][K, J, pk.is_])


# ---- whole runs ---------------------------------------------------------------------------------------------------------------
LWAVE = ("pgen_name = linear_wave\nwave_flag = 0\namp = 1.0e-2\ndens = 1.0\npgas = 0.6\nvx0 = 0.3\nvy0 = 0.0\nvz0 = 0.0\n"
         "bx0 = 1.0\nby0 = 1.4142136\nbz0 = 0.5\nalong_x1 = false\nalong_x2 = false\nalong_x3 = false")


def make_single_valued(sim, pk):
    """the upper copy of every active face two blocks share takes the value of the neighbour's lower copy"""
    t = face_tensors(sim)
    f = [x.clone() for x in t]
    K, J, I = slice(pk.ks, pk.ke + 1), slice(pk.js, pk.je + 1), slice(pk.is_, pk.ie + 1)
    for m in range(pk.nmb):
        t[0][m][K, J, pk.ie + 1] = f[0][pk.neighbour(m, 1, 0, 0)][K, J, pk.is_]
        t[1][m][K, pk.je + 1, I] = f[1][pk.neighbour(m, 0, 1, 0)][K, pk.js, I]
        t[2][m][pk.ke + 1, J, I] = f[2][pk.neighbour(m, 0, 0, 1)][pk.ks, J, I]


def test_zero_shear_run_equals_the_periodic_run():
    """qshear = omega0 = 0 with shear-periodic x1 against periodic x1 without the block, PLM + HLLD, 16^3 in 2 x 2 x 1
    blocks, 20 cycles of the task-granular chain: the second run has none of the new tasks active.
    The start is made single-valued first.  The linear-wave generator differences its vector potential block by block,
    and the two copies of a face that two blocks share differ in the last bit on some 900 faces of this mesh.  The periodic
    exchange fills row je+1 of x2f in the x1 ghost zone from the x1 neighbour's row je+1; the shear boundary, as in the
    reference, fills it from row js of the next block along x2, the other copy of the same face.  With equal copies both
    give the same bits, and CT keeps them equal (measured: zero differing copies after 20 cycles in either run)."""
    nx, nmb, ng = (8, 8, 16), (2, 2, 1), 2
    kw = dict(recon="plm", rsolver="hlld", eos="ideal", nlim=20, tlim=100.0, problem=LWAVE, fused="false")
    a = make_sim(deck_text(nx, nmb, ng, qshear=0.0, omega0=0.0, **kw))
    b = make_sim(deck_text(nx, nmb, ng, x1_bc="periodic", sbox=False, **kw))
    pk = restate_pack(a, nx, nmb, ng)
    for s in (a, b):
        make_single_valued(s, pk)
        s.pdriver.Initialize(s.pmesh, s.pin)
    assert a.phys.psbox_b is not None and b.phys.psbox_b is None and not a.phys.fused and not b.phys.fused
    assert a.Execute() == 20 and b.Execute() == 20
    assert a.pmesh.time == b.pmesh.time and a.pmesh.dt == b.pmesh.dt
    ua, ub = a.phys.u0.cpu().numpy(), b.phys.u0.cpu().numpy()
    assert np.isfinite(ua).all() and np.array_equal(ua, ub) and np.array_equal(a.phys.w0.cpu().numpy(), b.phys.w0.cpu().numpy())
    for fa, fb in zip(get_faces(a), get_faces(b)):
        assert np.array_equal(fa, fb)
    assert np.array_equal(a.phys.bcc0.cpu().numpy(), b.phys.bcc0.cpu().numpy()) and np.abs(ua[:, 1]).max() > 0.1


SHW_MESH = dict(xmin=(-0.25, -0.25, -0.25), xmax=(0.25, 0.25, 0.25))


def dbyc_start_window(n):
    """where dByc(0) of the deck on n^3 cells lies relative to the first value of the linear solution, 1.36931e-07.  The
    perturbed By on x2 faces is the difference of a3 over dx1 and of a1 over dx3: a difference of a sine over a cell is the
    derivative times sin(h)/h, h = k dx/2; the cell-centred By is the mean of two x2 faces: times cos(ky dx/2); the sum
    against cos(k.x) at cell centres projects exactly.  With nwx = -2, nwy = nwz = 1 the two terms carry
    sin(hx)/hx cos(hy) and sin(hz)/hz cos(hy), hx = 2 pi/n, hy = hz = pi/n: dByc(0) lies between the smaller of the two
    times the table's value and the value itself.  The table has six digits: 1e-5 relative on either side."""
    hx, hy = 2.0*math.pi/n, math.pi/n
    low = min(math.sin(hx)/hx, math.sin(hy)/hy)*math.cos(hy)
    return (low - 1e-5)*1.36931e-07, (1.0 + 1e-5)*1.36931e-07


def test_dbyc_at_the_start(tmp_path, monkeypatch):
    """dByc at t = 0 against the sum restated from shwave.cpp:406-408 over the cell-centred field the run holds (4096 terms
    of either sign, each of at most T = vol*2*(|By| + 0.2): 2 N ulp of T covers the order of the sum and the few ulp of each
    term)"""
    monkeypatch.chdir(tmp_path)
    from athenak_amd.outputs import Outputs
    nx, nmb, ng = (8, 16, 16), (2, 1, 1), 3
    text = deck_text(nx, nmb, ng, recon="wenoz", nlim=5, tlim=8.0, problem=(SHWAVE4 % 1) + "\nuser_hist = true", **SHW_MESH,
                     extra="<output1>\nfile_type = hst\ndt = 100.0\ndata_format = %24.16e\nuser_hist_only = true\n")
    sim = make_sim(text)
    pm, drv = sim.pmesh, sim.pdriver
    pout = Outputs(sim.pin, pm)
    drv.Initialize(pm, sim.pin, pout)
    h = read_hst("sbox.user.hst")
    assert list(h) == ["time", "dt", "dByc"]
    got = h["dByc"]
    pk = restate_pack(sim, nx, nmb, ng, **SHW_MESH)
    kx, ky, kz = (2.0*math.pi/0.5)*(-2.0), (2.0*math.pi/0.5)*1.0, (2.0*math.pi/0.5)*1.0
    by = sim.phys.bcc0[:, 1].cpu().numpy()
    terms, tmax = [], 0.0
    for m in range(pk.nmb):
        vol = pk.dx[m, 0]*pk.dx[m, 1]*pk.dx[m, 2]
        for k in range(nx[2]):
            x3v = float(R.CellCenterX(k, nx[2], pk.bounds[m, 4], pk.bounds[m, 5]))
            for j in range(nx[1]):
                x2v = float(R.CellCenterX(j, nx[1], pk.bounds[m, 2], pk.bounds[m, 3]))
                for i in range(nx[0]):
                    x1v = float(R.CellCenterX(i, nx[0], pk.bounds[m, 0], pk.bounds[m, 1]))
                    t = vol*2.0*(float(by[m, pk.ks + k, pk.js + j, pk.is_ + i]) - (0.2 - 0.15*0.0))
                    t *= math.cos(kx*x1v + ky*x2v + kz*x3v)
                    tmax = max(tmax, abs(t))
                    terms.append(t)
    want = math.fsum(terms)
    print("dByc(t = 0):", got[0], "restated", want, "first value of the linear solution 1.36931e-07")
    assert len(got) == 1 and abs(got[0] - want) <= 2*len(terms)*U*tmax
    lo, hi = dbyc_start_window(16)
    assert lo <= got[0] <= hi
    assert drv.Execute(pm, sim.pin) == 5 and np.isfinite(sim.phys.u0.cpu().numpy()).all()


def max_divb(sim):
    """largest |div B| dx / |B| over the active cells, dx the smallest cell width, |B| the cell-centred field strength"""
    pm = sim.pmesh
    ind = pm.mb_indcs
    K, J, I = slice(ind.ks, ind.ke + 1), slice(ind.js, ind.je + 1), slice(ind.is_, ind.ie + 1)
    b1, b2, b3 = get_faces(sim)
    dx = np.asarray(pm.pmb_pack.pmb.dx)
    div = ((b1[:, K, J, ind.is_ + 1:ind.ie + 2] - b1[:, K, J, I])/dx[:, 0, None, None, None]
           + (b2[:, K, ind.js + 1:ind.je + 2, I] - b2[:, K, J, I])/dx[:, 1, None, None, None]
           + (b3[:, ind.ks + 1:ind.ke + 2, J, I] - b3[:, K, J, I])/dx[:, 2, None, None, None])
    bcc = sim.phys.bcc0.cpu().numpy()[:, :, K, J, I]
    return float((np.abs(div)*dx.min()/np.sqrt((bcc*bcc).sum(axis=1))).max())


def test_div_b_after_twenty_cycles():
    """the ipert = 4 deck in 2 x 2 x 1 blocks of 8 x 8 x 16, 20 cycles, against the same initial state run periodic and
    without the block on the task-granular chain (the launch sequence without any of the box's tasks).  Orbital CT adds one
    more difference of EMFs of the size of the field per cycle to the three of the stage's CT, and the boundary remap only
    touches ghost faces: the bar is four times the periodic run's value."""
    kw = dict(recon="wenoz", nlim=20, tlim=100.0, **SHW_MESH)
    a = make_sim(deck_text((8, 8, 16), (2, 2, 1), 3, problem=SHWAVE4 % 1, **kw))
    b = make_sim(deck_text((8, 8, 16), (2, 2, 1), 3, x1_bc="periodic", sbox=False, fused="false",
                           problem=LWAVE.replace("pgas = 0.6", "pgas = 1.0"), **kw))
    assert a.phys.porb_b is not None and b.phys.porb_b is None and not b.phys.fused
    b.phys.u0.copy_(a.phys.u0)
    for tb, ta in zip(face_tensors(b), face_tensors(a)):
        tb.copy_(ta)
    for s in (a, b):
        s.pdriver.Initialize(s.pmesh, s.pin)
    d0a, d0b = max_divb(a), max_divb(b)
    assert d0a == d0b
    assert a.Execute() == 20 and b.Execute() == 20
    da, db = max_divb(a), max_divb(b)
    print("max |div B| dx/|B|: start", d0a, "after 20 cycles with the box", da, "periodic without it", db)
    assert np.isfinite(a.phys.u0.cpu().numpy()).all() and a.psbox_b.yshear > 0.0
    assert da <= 4.0*db


MRI = "pgen_name = mri3d\nifield = 1\nbeta = 100.0\namp = 0.01\nrseed = 3\nuser_hist = true%s"


@pytest.mark.parametrize("eos", ["isothermal", "ideal"])
@pytest.mark.parametrize("nx,nmb", [((8, 8, 8), (1, 2, 1)), ((17, 9, 11), (2, 1, 1))])
def test_mri_history_against_the_restatement(nx, nmb, eos):
    """akmi_mri_history through ProblemGenerator.MRIHistory on random data (17 x 9 x 11 = 1683 cells: two tiles per block,
    the second partly filled).  The labels are the reference's; every sum lies within n U max|term| of the exact sum of the
    restated terms (n - 1 additions in whatever order, each rounded to half an ulp of a partial sum of at most n max|term|,
    and the terms themselves a few ulp: n U max|term| covers both for n of a thousand); two calls give the same bits."""
    ng = 3
    sim = make_sim(deck_text(nx, nmb, ng, recon="ppm4", eos=eos, rsolver="hlld", cfl=0.3,
                             problem=MRI % ("\npres = 1.0" if eos == "ideal" else "")))
    ph = sim.phys
    pk = restate_pack(sim, nx, nmb, ng)
    rng = np.random.default_rng(nx[0])
    u0 = rng.standard_normal(pk.shape(ph.nvars))
    u0[:, 0] = rng.uniform(0.5, 1.5, u0[:, 0].shape)
    bcc = rng.standard_normal(pk.shape(3))
    b = tuple(rng.standard_normal(s) for s in M.face_shapes(pk))
    ph.u0.copy_(to_dev(u0))
    ph.bcc0.copy_(to_dev(bcc))
    set_faces(sim, b)
    labels, got = sim.pmesh.pgen.MRIHistory(sim.pmesh)
    want_labels, terms, tmax = M.mri_history(pk, u0, bcc, b, eos == "ideal")
    assert labels == want_labels and len(labels) == (16 if eos == "ideal" else 15)
    n = terms.shape[1]
    assert n == pk.nmb*nx[0]*nx[1]*nx[2]
    for q, lab in enumerate(labels):
        want = math.fsum(terms[q])
        assert abs(got[q] - want) <= n*U*tmax[q], (lab, got[q], want)
    _, again = sim.pmesh.pgen.MRIHistory(sim.pmesh)
    assert np.array_equal(got, again)


def test_mri3d_five_cycles_write_the_user_history(tmp_path, monkeypatch):
    """the deck inputs/mri3d.athinput at 16 x 16 x 16 for five cycles: mri3d.user.hst with the reference's columns, the net
    vertical flux B0 V kept, mass kept"""
    monkeypatch.chdir(tmp_path)
    from athenak_amd.__main__ import main
    assert main(["-i", "mri3d.athinput", "-d", str(tmp_path/"run"), "time/nlim=5", "mesh/nx1=16", "mesh/nx2=16", "mesh/nx3=16",
                 "meshblock/nx1=16", "meshblock/nx2=8", "meshblock/nx3=16", "output1/dt=0.001", "output1/data_format=%20.12e"]) == 0
    h = read_hst(str(tmp_path/"run"/"mri3d.user.hst"))
    assert list(h) == ["time", "dt", "mass", "1-mom", "2-mom", "3-mom"] + M.MRI_LABELS
    assert len(h["time"]) >= 2 and all(np.isfinite(v).all() for v in h.values())
    vol, b0 = 1.0*2.0*1.0, math.sqrt(2.0/400.0)
    # the first line is the start: uniform Bz = B0 (8192 equal terms: 1e-12 relative), no other field, |d - 1| <= amp.
    # (Later lines are not compared: without an EMF correction at the shear-periodic faces, which the reference has none of
    # either, the net vertical flux is kept to the order of the perturbation only.)
    assert abs(h["3-bcc"][0] - b0*vol) <= 1e-12*b0*vol and abs(h["3-ME"][0] - 0.5*b0*b0*vol) <= 1e-12*b0*b0*vol
    assert h["1-ME"][0] == 0.0 and h["2-ME"][0] == 0.0 and h["dBxBy"][0] == 0.0 and abs(h["mass"][0] - vol) <= 0.025*vol
    assert (tmp_path/"run"/"mri3d.mhd.hst").exists()


def test_command_line_five_cycles(tmp_path, monkeypatch):
    """python -m athenak_amd -i mhd_shwave.athinput for five cycles writes shwave4.user.hst with the dByc column"""
    monkeypatch.chdir(tmp_path)
    from athenak_amd.__main__ import main
    assert main(["-i", "mhd_shwave.athinput", "-d", str(tmp_path/"run"), "time/nlim=5", "mesh/nx1=16", "mesh/nx2=16", "mesh/nx3=16",
                 "meshblock/nx1=16", "meshblock/nx2=8", "meshblock/nx3=16", "output1/dt=0.001"]) == 0
    h = read_hst(str(tmp_path/"run"/"shwave4.user.hst"))
    assert list(h) == ["time", "dt", "dByc"] and len(h["time"]) >= 2 and np.isfinite(h["dByc"]).all()
    assert not (tmp_path/"run"/"shwave4.mhd.hst").exists()
    lo, hi = dbyc_start_window(16)
    assert lo*(1.0 - 1e-5) <= h["dByc"][0] <= hi*(1.0 + 1e-5)          # (%12.5e: six digits)
