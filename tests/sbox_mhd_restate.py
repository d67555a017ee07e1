"""NumPy restatement of the MHD half of the shearing box of the reference (src/shearing_box/), written from its lines with
the same parenthesisation on top of tests/sbox_restate.py (Pack, the remap fluxes, shift_cases, find_target_mb): the
yardstick of tests/test_sbox_mhd_host.py and tests/test_gpu_sbox_mhd.py.

  source_terms_mhd              shearing_box_srcterms.cpp:92-150
  efield_2d                     shearing_box_srcterms.cpp:159-200
  shear_boundary_fc             shearing_box_fc.cpp:48-286 (the remap per pencil, then the three cases applied to rows) and
                                :379-431 (unpack)
  orbital_advection_fc          orbital_advection_fc.cpp:58-132 (buffers from the x2 neighbours' active rows) and :223-358
                                (the pencil, the effective EMFs, CT)

A face field is the tuple (x1f, x2f, x3f) of arrays [nmb][N3][N2][N1+1], [nmb][N3][N2+1][N1], [nmb][N3+1][N2][N1].
"""
import math

import numpy as np

import sbox_restate as R


def LeftEdgeX(ith, n, xmin, xmax):      # coordinates/cell_locations.hpp:23-28
    x = np.float64(ith)/np.float64(n)
    return (x*xmax - x*xmin) - (0.5*xmax - 0.5*xmin) + (0.5*xmin + 0.5*xmax)


def face_shapes(pk):
    return ((pk.nmb, pk.N3, pk.N2, pk.N1 + 1), (pk.nmb, pk.N3, pk.N2 + 1, pk.N1), (pk.nmb, pk.N3 + 1, pk.N2, pk.N1))


# ---- shearing_box_srcterms.cpp:92-150 --------------------------------------------------------------------------------
def source_terms_mhd(pk, w0, bcc0, u0, bdt, qshear, omega0, is_ideal, is_strat):
    """returns the updated copy of u0; ghost cells as they were"""
    u = u0.copy()
    a = (slice(pk.ks, pk.ke + 1), slice(pk.js, pk.je + 1), slice(pk.is_, pk.ie + 1))
    IDN, IVX, IVY, IVZ, IEN = 0, 1, 2, 3, 4
    IM1, IM2, IM3 = 1, 2, 3
    IBX, IBY, IBZ = 0, 1, 2
    for m in range(pk.nmb):
        den = w0[m, IDN][a]
        if pk.three_d:
            coef1 = 2.0*bdt*omega0
            coef2 = (2.0 - qshear)*bdt*omega0
            qo = qshear*omega0
            coef3 = bdt*(omega0*omega0)
            mom1 = den*w0[m, IVX][a]
            mom2 = den*w0[m, IVY][a]
            u[m, IM1][a] += coef1*mom2
            u[m, IM2][a] -= coef2*mom1
            if is_strat:
                x3v = R.CellCenterX(np.arange(pk.nx3), pk.nx3, pk.bounds[m, 4], pk.bounds[m, 5])
                u[m, IM3][a] -= coef3*den*x3v[:, None, None]
            if is_ideal:
                u[m, IEN][a] += bdt*(mom1*mom2/den - bcc0[m, IBX][a]*bcc0[m, IBY][a])*qo
        else:
            coef1 = 2.0*bdt*omega0
            coef3 = (2.0 - qshear)*bdt*omega0
            qo = qshear*omega0
            mom1 = den*w0[m, IVX][a]
            mom3 = den*w0[m, IVZ][a]
            u[m, IM1][a] += coef1*mom3
            u[m, IM3][a] -= coef3*mom1
            if is_ideal:
                u[m, IEN][a] += bdt*(mom1*mom3/den - bcc0[m, IBX][a]*bcc0[m, IBZ][a])*qo
    return u


# ---- shearing_box_srcterms.cpp:159-200 -------------------------------------------------------------------------------
def efield_2d(pk, b1, b2, e1, e2, qshear, omega0):
    """2-D only; e1 [nmb][2][N2+1][N1], e2 [nmb][2][N2][N1+1]; returns the updated copies"""
    assert not pk.three_d and pk.ks == 0 and pk.ke == 0
    e1, e2 = e1.copy(), e2.copy()
    qomega = qshear*omega0
    ks, ke = pk.ks, pk.ke
    j = slice(pk.js, pk.je + 2)
    i = slice(pk.is_, pk.ie + 2)
    for m in range(pk.nmb):
        ii = np.arange(pk.nx1 + 1)
        x1v = R.CellCenterX(ii, pk.nx1, pk.bounds[m, 0], pk.bounds[m, 1])[None, :]
        e1[m, ks, j, i] -= qomega*x1v*b2[m, ks, j, i]
        e1[m, ke + 1, j, i] -= qomega*x1v*b2[m, ks, j, i]
        x1f = LeftEdgeX(ii, pk.nx1, pk.bounds[m, 0], pk.bounds[m, 1])[None, :]
        e2[m, ks, j, i] += qomega*x1f*b1[m, ks, j, i]
        e2[m, ke + 1, j, i] += qomega*x1f*b1[m, ks, j, i]
    return e1, e2


# ---- shearing_box_fc.cpp ---------------------------------------------------------------------------------------------
def shear_boundary_fc(pk, b, yshear, recon):
    """PackAndSendFC + RecvAndUnpackFC on one rank: returns copies of the three face arrays with the x1 ghost faces of the
    blocks on the x1 faces remapped and shifted.  kl..ku are the cell planes (ghost planes included in 3-D) and the rows
    are 0..nj-1: the last x3f plane and the last x2f row are not touched."""
    out = [f.copy() for f in b]
    ng, nx2 = pk.ng, pk.nx2
    js, je = pk.js, pk.je
    nj = nx2 + 2*ng
    kl, ku = (pk.ks - ng, pk.ke + ng) if pk.three_d else (pk.ks, pk.ke)
    remap = R.remap_flux_of(recon)
    faces = pk.x1_faces()
    for n in (0, 1):
        def col(v):
            if n == 0:
                return slice(0, ng)
            return slice(pk.ie + 2, pk.ie + 2 + ng) if v == 0 else slice(pk.ie + 1, pk.ie + 1 + ng)
        send = {}
        for mm in faces[n]:
            # a_(j) of pencil (v, k, i), stacked to (j, v, k, i)
            a_ = np.stack([np.moveaxis(b[v][mm][kl:ku + 1, 0:nj, col(v)], 1, 0) for v in range(3)], axis=1)
            dx2 = pk.dx[mm, 1]
            eps = math.fmod(yshear, dx2)/dx2
            if n == 1:
                eps *= -1.0
            flx = remap(js, je + 1, eps, a_)
            sb = np.full(a_.shape, np.nan)
            j = np.arange(js, je + 1)
            sb[j] = a_[j] - (flx[j + 1] - flx[j])
            send[mm] = sb
        for mm in faces[n]:
            l1, l2, l3 = pk.lloc[mm]
            if l2 != 0:
                continue
            row = [pk.gid[(l1, bx, l3)] for bx in range(pk.nmb2)]
            joffset = int(yshear/pk.dx[mm, 1])
            recv = R.shift_cases([send[r] for r in row], n, joffset, ng, nx2)
            for r, rb in zip(row, recv):
                for v in range(3):
                    out[v][r][kl:ku + 1, 0:nj, col(v)] = np.moveaxis(rb[:, v], 0, 1)
    return tuple(out)


# ---- orbital_advection_fc.cpp ----------------------------------------------------------------------------------------
def orbital_advection_fc(pk, b, qshear, omega0, dt, maxjshift, recon):
    """PackAndSendFC (:58-132: B3 and B1 of the x2 neighbours' active rows into the buffers) and RecvAndUnpackFC
    (:223-358); returns (the three updated face arrays, the largest |joffset|, emfx, emfz)"""
    x1f, x2f, x3f = (f.copy() for f in b)
    ng, nx2 = pk.ng, pk.nx2
    is_, ie, js, je, ks, ke = pk.is_, pk.ie, pk.js, pk.je, pk.ks, pk.ke
    remap = R.remap_flux_of(recon)
    nb = ng + maxjshift
    jfs = ng + maxjshift
    jfe = jfs + nx2 - 1
    nfx = nx2 + 2*(ng + maxjshift)
    qo = qshear*omega0
    jmax = 0
    emfx = np.zeros((pk.nmb, pk.N3, pk.N2, pk.N1))
    emfz = np.zeros((pk.nmb, pk.N3, pk.N2, pk.N1))
    src = (b[2], b[0])                                   # v = 0: x3f, v = 1: x1f
    for m in range(pk.nmb):
        lo, hi = pk.neighbour(m, 0, -1, 0), pk.neighbour(m, 0, 1, 0)
        for v in (0, 1):
            # rbuf[0] of m: what its inner neighbour packed with n = 1 (jl = je-(ng+maxjshift-1) .. je); rbuf[1]: what its
            # outer neighbour packed with n = 0 (js .. js+(ng+maxjshift-1)); k in ks..ke+1, i in is..ie+1
            rbuf0 = src[v][lo][ks:ke + 2, je - (nb - 1):je + 1, is_:ie + 2]
            rbuf1 = src[v][hi][ks:ke + 2, js:js + nb, is_:ie + 2]
            for i in range(is_, ie + 2):
                if v == 0:
                    x1 = float(R.CellCenterX(i - is_, pk.nx1, pk.bounds[m, 0], pk.bounds[m, 1]))
                else:
                    x1 = float(LeftEdgeX(i - is_, pk.nx1, pk.bounds[m, 0], pk.bounds[m, 1]))
                dx2 = pk.dx[m, 1]
                yshear = -(qo)*x1*dt
                joffset = int(yshear/dx2)
                jmax = max(jmax, abs(joffset))
                b0_ = np.empty((nfx, ke + 2 - ks))
                b0_[:jfs] = np.moveaxis(rbuf0[:, :, i - is_], 1, 0)
                b0_[jfs:jfe + 1] = np.moveaxis(src[v][m][ks:ke + 2, js:je + 1, i], 1, 0)
                b0_[jfe + 1:] = np.moveaxis(rbuf1[:, :, i - is_], 1, 0)
                epsi = math.fmod(yshear, dx2)/dx2
                flx = remap(jfs - joffset, jfe + 1 - joffset, epsi, b0_)
                jf = np.arange(js, je + 2) - js + jfs
                if v == 0:
                    e = -flx[jf - joffset]
                    for jj in range(1, joffset + 1):
                        e = e - b0_[jf - jj]
                    for jj in range(joffset + 1, 1):
                        e = e + b0_[jf - jj]
                    emfx[m, ks:ke + 2, js:je + 2, i] = np.moveaxis(e, 0, 1)
                else:
                    e = flx[jf - joffset].copy()
                    for jj in range(1, joffset + 1):
                        e = e + b0_[jf - jj]
                    for jj in range(joffset + 1, 1):
                        e = e - b0_[jf - jj]
                    emfz[m, ks:ke + 2, js:je + 2, i] = np.moveaxis(e, 0, 1)
    K, J, I = slice(ks, ke + 1), slice(js, je + 1), slice(is_, ie + 1)
    Kp, Jp, Ip = slice(ks + 1, ke + 2), slice(js + 1, je + 2), slice(is_ + 1, ie + 2)
    K1, J1, I1 = slice(ks, ke + 2), slice(js, je + 2), slice(is_, ie + 2)
    for m in range(pk.nmb):
        # ---- update B1
        x1f[m][K, J, I1] -= (emfz[m][K, Jp, I1] - emfz[m][K, J, I1])
        # ---- update B2
        dydx = pk.dx[m, 1]/pk.dx[m, 0]
        x2f[m][K, J1, I] += dydx*(emfz[m][K, J1, Ip] - emfz[m][K, J1, I])
        if pk.three_d:
            dydz = pk.dx[m, 1]/pk.dx[m, 2]
            x2f[m][K, J1, I] -= dydz*(emfx[m][Kp, J1, I] - emfx[m][K, J1, I])
        # ---- update B3
        x3f[m][K1, J, I] += (emfx[m][K1, Jp, I] - emfx[m][K1, J, I])
    return (x1f, x2f, x3f), jmax, emfx, emfz


# ---- pgen/tests/mri3d.cpp:233-336 --------------------------------------------------------------------------------------
MRI_LABELS = ["1-KE", "2-KE", "3-KE", "1-ME", "2-ME", "3-ME", "1-bcc", "2-bcc", "3-bcc", "dVxVy", "dBxBy"]


def mri_history(pk, u0, bcc, b, is_ideal):
    """(labels, the terms of every active cell as an array [nhist][cells of the mesh], the largest |term| per column)"""
    x1f, x2f, x3f = b
    nmhd = 5 if is_ideal else 4
    labels = ["mass", "1-mom", "2-mom", "3-mom"] + (["tot-E"] if is_ideal else []) + MRI_LABELS
    K, J, I = slice(pk.ks, pk.ke + 1), slice(pk.js, pk.je + 1), slice(pk.is_, pk.ie + 1)
    Kp, Jp, Ip = slice(pk.ks + 1, pk.ke + 2), slice(pk.js + 1, pk.je + 2), slice(pk.is_ + 1, pk.ie + 2)
    IDN, IM1, IM2, IM3, IEN = 0, 1, 2, 3, 4
    IBX, IBY, IBZ = 0, 1, 2
    SQR = lambda x: x*x
    cols = []
    for m in range(pk.nmb):
        vol = pk.dx[m, 0]*pk.dx[m, 1]*pk.dx[m, 2]
        u = lambda n: u0[m, n][K, J, I]
        h = [None]*(nmhd + 11)
        h[IDN] = vol*u(IDN)
        h[IM1] = vol*u(IM1)
        h[IM2] = vol*u(IM2)
        h[IM3] = vol*u(IM3)
        if is_ideal:
            h[IEN] = vol*u(IEN)
        h[nmhd] = vol*0.5*SQR(u(IM1))/u(IDN)
        h[nmhd + 1] = vol*0.5*SQR(u(IM2))/u(IDN)
        h[nmhd + 2] = vol*0.5*SQR(u(IM3))/u(IDN)
        h[nmhd + 3] = vol*0.25*(SQR(x1f[m][K, J, Ip]) + SQR(x1f[m][K, J, I]))
        h[nmhd + 4] = vol*0.25*(SQR(x2f[m][K, Jp, I]) + SQR(x2f[m][K, J, I]))
        h[nmhd + 5] = vol*0.25*(SQR(x3f[m][Kp, J, I]) + SQR(x3f[m][K, J, I]))
        h[nmhd + 6] = vol*bcc[m, IBX][K, J, I]
        h[nmhd + 7] = vol*bcc[m, IBY][K, J, I]
        h[nmhd + 8] = vol*bcc[m, IBZ][K, J, I]
        h[nmhd + 9] = vol*u(IM1)*u(IM2)/u(IDN)
        h[nmhd + 10] = -vol*bcc[m, IBX][K, J, I]*bcc[m, IBY][K, J, I]
        cols.append(np.array([x.ravel() for x in h]))
    terms = np.concatenate(cols, axis=1)
    return labels, terms, np.abs(terms).max(axis=1)


# ---- a divergence-free field from a random vector potential ------------------------------------------------------------
def divfree_field(pk, rng):
    """the three face arrays of every block (ghost faces filled periodically) from a random vector potential on the edges
    of the whole, periodic mesh: its discrete divergence is round-off.  Cell widths of block 0 (they differ between blocks
    in the last bits at most, which the bound of the caller's comparison does not see: it compares before and after)."""
    nx, ny, nz = pk.nx1*pk.nmb1, pk.nx2*pk.nmb2, pk.nx3*pk.nmb3
    a1, a2, a3 = (rng.standard_normal((nz, ny, nx)) for _ in range(3))
    dx1, dx2, dx3 = pk.dx[0]
    up = lambda a, ax: np.roll(a, -1, axis=ax)
    g1 = (up(a3, 1) - a3)/dx2 - (up(a2, 0) - a2)/dx3          # at (i face, j, k)
    g2 = (up(a1, 0) - a1)/dx3 - (up(a3, 2) - a3)/dx1          # at (i, j face, k)
    g3 = (up(a2, 2) - a2)/dx1 - (up(a1, 1) - a1)/dx2          # at (i, j, k face)
    shapes = face_shapes(pk)
    out = [np.empty(s) for s in shapes]
    for m, (l1, l2, l3) in enumerate(pk.lloc):
        for v, g in enumerate((g1, g2, g3)):
            n3, n2, n1 = shapes[v][1:]
            kk = (l3*pk.nx3 + np.arange(n3) - pk.ks) % nz
            jj = (l2*pk.nx2 + np.arange(n2) - pk.js) % ny
            ii = (l1*pk.nx1 + np.arange(n1) - pk.is_) % nx
            out[v][m] = g[np.ix_(kk, jj, ii)]
    return tuple(out)


# ---- div B and the bound on its change under the orbital CT ----------------------------------------------------------
def div_b(pk, b):
    """(nmb, nx3, nx2, nx1): the face differences over the cell widths, active cells"""
    x1f, x2f, x3f = b
    K, J, I = slice(pk.ks, pk.ke + 1), slice(pk.js, pk.je + 1), slice(pk.is_, pk.ie + 1)
    Kp, Jp, Ip = slice(pk.ks + 1, pk.ke + 2), slice(pk.js + 1, pk.je + 2), slice(pk.is_ + 1, pk.ie + 2)
    d = np.empty((pk.nmb, pk.nx3, pk.nx2, pk.nx1))
    for m in range(pk.nmb):
        d[m] = ((x1f[m][K, J, Ip] - x1f[m][K, J, I])/pk.dx[m, 0] + (x2f[m][K, Jp, I] - x2f[m][K, J, I])/pk.dx[m, 1]
                + (x3f[m][Kp, J, I] - x3f[m][K, J, I])/pk.dx[m, 2])
    return d


def ct_divb_bound(pk, recon, maxjshift, bmax):
    """bound on |div B(after) - div B(before)| of one orbital CT step, from the operation count.  In real arithmetic the
    EMF differences cancel in the divergence.  With E = (F + maxjshift) bmax >= |emf| (one flux of at most F bmax by
    R.FLUX_BOUND, plus at most maxjshift whole cells; its own roundings do not matter: the same rounded EMF enters every
    face that shares it), the faces of a cell take, in units of u = 2^-52 (a rounding is half an ulp of its result):
        x1f, x3f:  the EMF difference (|.| <= 2E): E; the sum into a face of at most bmax + 2E: (bmax + 2E)/2
        x2f:       per term, with r >= dy/dx, dy/dz: the difference times r: r E; the rounded quotient dy/dx, which stands
                   for the exact ratio of the widths in the divergence: r E; the product: r E; then the two sums into a face
                   of at most bmax + 2 r E and bmax + 4 r E: 6 r E + bmax + 3 r E
    Each face error enters the divergence over its cell width, two faces per direction.  The divergence itself is formed
    twice (before and after) with three differences (2B/dx each), three quotients and two sums (4B/dx, 6B/dx): 11 B/dxmin
    each time, B <= B' = bmax + 2 (1 + 2 r) E the largest face afterwards."""
    u = 2.0**-52
    F = R.FLUX_BOUND["ppmx" if recon not in ("dc", "plm") else recon]
    E = (F + maxjshift)*bmax
    r = max(max(pk.dx[m, 1]/pk.dx[m, 0], pk.dx[m, 1]/pk.dx[m, 2]) for m in range(pk.nmb))
    e13 = E + 0.5*(bmax + 2.0*E)
    e2 = 9.0*r*E + bmax
    bnew = bmax + 2.0*(1.0 + 2.0*r)*E
    dmin = pk.dx.min()
    return u*(2.0*e13/pk.dx[:, 0].min() + 2.0*e2/pk.dx[:, 1].min() + 2.0*e13/pk.dx[:, 2].min() + 22.0*bnew/dmin)
