"""NumPy restatement of the cell-centred shearing box of the reference (src/shearing_box/), written from its lines with
the same parenthesisation: the yardstick of tests/test_sbox_host.py and tests/test_gpu_sbox.py.

  DC_/PLM_/PPMX_RemapFlx        remap_fluxes.hpp:18-149
  source_terms_cc               shearing_box_srcterms.cpp:27-84
  shear_boundary_cc             shearing_box_cc.cpp:48-266 (PackAndSendCC: fractional remap, then the three cases of the
                                integer shift with FindTargetMB, shearing_box.cpp:108-122) and :359-388 (unpack)
  orbital_advection_cc          orbital_advection_cc.cpp:53-128 (buffers from the x2 neighbours) and :215-288 (remap)

A pencil is an array whose FIRST axis is the row index j; whatever axes follow ride along (NumPy's elementwise IEEE
operations are the scalar ones).  The integer shift is the reference's copy of row ranges between buffers, case by case:
nothing here computes a source row from a destination row.
"""
import math

import numpy as np

TWO_3RDS = 0.6666666666666667           # athena.hpp:54


def SIGN(x):                            # athena.hpp:52
    return np.where(x < 0.0, -1.0, 1.0)


def CellCenterX(ith, n, xmin, xmax):    # coordinates/cell_locations.hpp:35-39
    x = (np.float64(ith) + 0.5)/np.float64(n)
    return (x*xmax - x*xmin) - (0.5*xmax - 0.5*xmin) + (0.5*xmin + 0.5*xmax)


# ---- remap_fluxes.hpp ------------------------------------------------------------------------------------------------
def DC_RemapFlx(jl, ju, eps, u):
    ust = np.full(u.shape, np.nan)
    j = np.arange(jl, ju + 1)
    if eps > 0.0:
        ust[j] = eps*u[j - 1]
    else:
        ust[j] = eps*u[j]
    return ust


def PLM_RemapFlx(jl, ju, eps, u):
    ust = np.full(u.shape, np.nan)
    j = np.arange(jl, ju + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        if eps > 0.0:
            dql = u[j - 1] - u[j - 2]
            dqr = u[j] - u[j - 1]
            dq2 = dql*dqr
            dqm = 2.0*dq2/(dql + dqr)
            dqm = np.where(dq2 <= 0.0, 0.0, dqm)
            ust[j] = eps*(u[j - 1] + 0.5*(1.0 - eps)*dqm)
        else:
            dql = u[j] - u[j - 1]
            dqr = u[j + 1] - u[j]
            dq2 = dql*dqr
            dqm = 2.0*dq2/(dql + dqr)
            dqm = np.where(dq2 <= 0.0, 0.0, dqm)
            ust[j] = eps*(u[j] - 0.5*(1.0 + eps)*dqm)
    return ust


def PPMX_RemapFlx(jl, ju, eps, u):
    ust = np.full(u.shape, np.nan)
    j = np.arange(jl - 1, ju + 1)
    um2, um1, u0, up1, up2 = u[j - 2], u[j - 1], u[j], u[j + 1], u[j + 2]

    def limited(d2uc, d2ul, d2ur, lim_slope, extra=None, of=None):
        of = d2uc if of is None else of
        pos = (d2uc > 0.0) & (d2ul > 0.0) & (d2ur > 0.0)
        neg = (d2uc < 0.0) & (d2ul < 0.0) & (d2ur < 0.0)
        if extra is not None:
            pos, neg = pos & (extra > 0.0), neg & (extra < 0.0)
        return np.where(pos | neg, SIGN(of)*np.fmin(1.25*lim_slope, np.abs(of)), 0.0)

    ulv = (7.0*(um1 + u0) - (um2 + up1))/12.0
    d2uc = 3.0*(um1 - 2.0*ulv + u0)
    d2ul = (um2 - 2.0*um1 + u0)
    d2ur = (um1 - 2.0*u0 + up1)
    lim_slope = np.fmin(np.abs(d2ul), np.abs(d2ur))
    d2ulim = limited(d2uc, d2ul, d2ur, lim_slope)
    ulv = 0.5*((um1 + u0) - d2ulim/3.0)

    urv = (7.0*(u0 + up1) - (um1 + up2))/12.0
    d2uc = 3.0*(u0 - 2.0*urv + up1)
    d2ul = (um1 - 2.0*u0 + up1)
    d2ur = (u0 - 2.0*up1 + up2)
    lim_slope = np.fmin(np.abs(d2ul), np.abs(d2ur))
    d2ulim = limited(d2uc, d2ul, d2ur, lim_slope)
    urv = 0.5*((u0 + up1) - d2ulim/3.0)

    qa = (urv - u0)*(u0 - ulv)
    qb = (um1 - u0)*(u0 - up1)
    inner = (qa <= 0.0) & (qb <= 0.0)
    d2u = -12.0*(u0 - 0.5*(ulv + urv))
    d2uc = (um1 - 2.0*u0 + up1)
    d2ul = (um2 - 2.0*um1 + u0)
    d2ur = (u0 - 2.0*up1 + up2)
    lim_slope = np.fmin(np.abs(d2ul), np.abs(d2ur))
    lim_slope = np.fmin(np.abs(d2uc), lim_slope)
    d2ulim = limited(d2uc, d2ul, d2ur, lim_slope, extra=d2u, of=d2u)
    with np.errstate(divide="ignore", invalid="ignore"):
        ulv_in = np.where(d2u == 0.0, u0, u0 + (ulv - u0)*d2ulim/d2u)
        urv_in = np.where(d2u == 0.0, u0, u0 + (urv - u0)*d2ulim/d2u)
    ulv = np.where(inner, ulv_in, ulv)
    urv = np.where(inner, urv_in, urv)

    qa = (urv - u0)*(u0 - ulv)
    qb = urv - ulv
    qc = 6.0*(u0 - 0.5*(ulv + urv))
    c1 = qa <= 0.0
    c2 = ~c1 & ((qb*qc) > (qb*qb))
    c3 = ~c1 & ~c2 & ((qb*qc) < -(qb*qb))
    ulv_n = np.where(c1, u0, np.where(c2, 3.0*u0 - 2.0*urv, ulv))
    urv_n = np.where(c1, u0, np.where(c3, 3.0*u0 - 2.0*ulv, urv))
    ulv, urv = ulv_n, urv_n

    du = urv - ulv
    u6 = 6.0*(u0 - 0.5*(ulv + urv))
    if eps > 0.0:
        qx = TWO_3RDS*eps
        ust[j + 1] = eps*(urv - 0.75*qx*(du - (1.0 - qx)*u6))
    else:
        qx = -TWO_3RDS*eps
        ust[j] = eps*(ulv + 0.75*qx*(du + (1.0 - qx)*u6))
    return ust


def remap_flux_of(recon):
    """the switches of shearing_box_cc.cpp:93-108 and orbital_advection_cc.cpp:264-279"""
    return {"dc": DC_RemapFlx, "plm": PLM_RemapFlx}.get(recon, PPMX_RemapFlx)


# ---- a small uniform mesh: what the functions below need of Mesh / MeshBlockPack ---------------------------------------
class Pack:
    """nmb1 x nmb2 x nmb3 MeshBlocks of nx1 x nx2 x nx3 cells, x1 fastest in the block list, every face periodic or
    shear-periodic; mb_size from the mesh bounds as meshblock.cpp:25-131 computes them"""

    def __init__(self, nx, nmb, ng, xmin, xmax, lloc=None):
        """lloc: the order of the block list when it is not x1 fastest (the mesh under test lists blocks in Z-order)"""
        self.nx1, self.nx2, self.nx3 = nx
        self.nmb1, self.nmb2, self.nmb3 = nmb
        self.ng = ng
        self.three_d = self.nx3 > 1
        self.is_, self.ie = ng, ng + self.nx1 - 1
        self.js, self.je = ng, ng + self.nx2 - 1
        self.ks, self.ke = (ng, ng + self.nx3 - 1) if self.three_d else (0, 0)
        self.N1, self.N2 = self.nx1 + 2*ng, self.nx2 + 2*ng
        self.N3 = self.nx3 + 2*ng if self.three_d else 1
        self.lloc = [(l1, l2, l3) for l3 in range(self.nmb3) for l2 in range(self.nmb2) for l1 in range(self.nmb1)]
        if lloc is not None:
            assert sorted(tuple(l) for l in lloc) == sorted(self.lloc)
            self.lloc = [tuple(l) for l in lloc]
        self.gid = {l: m for m, l in enumerate(self.lloc)}
        self.nmb = len(self.lloc)
        self.mesh_min, self.mesh_max = xmin, xmax
        self.bounds = np.zeros((self.nmb, 6))
        for m, l in enumerate(self.lloc):
            for q in range(3):
                n = (self.nmb1, self.nmb2, self.nmb3)[q]
                lo = xmin[q] if l[q] == 0 else self._left_edge(l[q], n, xmin[q], xmax[q])
                hi = xmax[q] if l[q] == n - 1 else self._left_edge(l[q] + 1, n, xmin[q], xmax[q])
                self.bounds[m, 2*q], self.bounds[m, 2*q + 1] = lo, hi
        self.dx = np.array([[(b[1] - b[0])/float(self.nx1), (b[3] - b[2])/float(self.nx2), (b[5] - b[4])/float(self.nx3)]
                            for b in self.bounds])

    @staticmethod
    def _left_edge(ith, n, xmin, xmax):          # LeftEdgeX, cell_locations.hpp:23-28
        x = np.float64(ith)/np.float64(n)
        return float((x*xmax - x*xmin) - (0.5*xmax - 0.5*xmin) + (0.5*xmin + 0.5*xmax))

    def neighbour(self, m, ox1, ox2, ox3):
        l = self.lloc[m]
        return self.gid[((l[0] + ox1) % self.nmb1, (l[1] + ox2) % self.nmb2, (l[2] + ox3) % self.nmb3)]

    def nghbr_table(self):
        """[nmb][27] local indices, d = (ox3+1)*9 + (ox2+1)*3 + (ox1+1)"""
        t = -np.ones((self.nmb, 27), dtype=np.int32)
        for m in range(self.nmb):
            for d in range(27):
                o = (d % 3 - 1, (d//3) % 3 - 1, d//9 - 1)
                if d == 13 or (not self.three_d and o[2]):
                    continue
                t[m, d] = self.neighbour(m, *o)
        return t

    def shape(self, nvar):
        return (self.nmb, nvar, self.N3, self.N2, self.N1)

    def x1_faces(self):
        """x1bndry_mbgid of shearing_box.cpp:34-64: the blocks on the inner / outer x1 face, in block order"""
        return ([m for m, l in enumerate(self.lloc) if l[0] == 0],
                [m for m, l in enumerate(self.lloc) if l[0] == self.nmb1 - 1])


# ---- shearing_box_srcterms.cpp:27-84 ---------------------------------------------------------------------------------
def source_terms_cc(pk, w0, u0, bdt, qshear, omega0, is_ideal, is_strat):
    """returns the updated copy of u0; ghost cells as they were"""
    u = u0.copy()
    a = (slice(pk.ks, pk.ke + 1), slice(pk.js, pk.je + 1), slice(pk.is_, pk.ie + 1))
    IDN, IVX, IVY, IVZ, IEN = 0, 1, 2, 3, 4
    IM1, IM2, IM3 = 1, 2, 3
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
                x3v = CellCenterX(np.arange(pk.nx3), pk.nx3, pk.bounds[m, 4], pk.bounds[m, 5])
                u[m, IM3][a] -= coef3*den*x3v[:, None, None]
            if is_ideal:
                u[m, IEN][a] += bdt*mom1*mom2/den*qo
        else:
            coef1 = 2.0*bdt*omega0
            coef3 = (2.0 - qshear)*bdt*omega0
            qo = qshear*omega0
            mom1 = den*w0[m, IVX][a]
            mom3 = den*w0[m, IVZ][a]
            u[m, IM1][a] += coef1*mom3
            u[m, IM3][a] -= coef3*mom1
            if is_ideal:
                u[m, IEN][a] += bdt*mom1*mom3/den*qo
    return u


# ---- shearing_box_cc.cpp ---------------------------------------------------------------------------------------------
def _cmod(a, b):
    """the % of C: truncation toward zero"""
    return int(math.fmod(a, b))


def find_target_mb(lx2, jshift, nmbx2):
    """FindTargetMB, shearing_box.cpp:108-122: lx2 of the block jshift blocks along x2"""
    t = _cmod(lx2 + jshift, nmbx2)
    if t < 0:
        t += nmbx2
    return t


def shift_cases(send, n, joffset, ng, nx2):
    """shearing_box_cc.cpp:127-266 on one rank: send[l] is the send buffer (rows first, js..je filled) of the block at
    lx2 = l on face n (0 inner, 1 outer); returns the receive buffers, rows js-ng..je+ng.  Rows that no copy reaches stay
    NaN (float buffers) / -1 (integer buffers)."""
    nmbx2 = len(send)
    js, je = ng, ng + nx2 - 1
    recv = [np.full(s.shape, -1 if s.dtype.kind == "i" else np.nan, dtype=s.dtype) for s in send]
    for lx2 in range(nmbx2):
        ji = int(joffset/nx2)                 # (integer division of non-negative ints)
        jr = joffset - ji*nx2
        if jr < ng:                           # --- CASE 1
            if n == 0:
                jsrc = [(js, js + ng - jr), (js, je + 1), (je - (ng - 1) - jr, je + 1)]
                jdst = [(je + 1 + jr, je + ng + 1), (js + jr, je + jr + 1), (js - ng, js + jr)]
            else:
                jsrc = [(js, js + ng + jr), (js, je + 1), (je - (ng - 1) + jr, je + 1)]
                jdst = [(je + 1 - jr, je + ng + 1), (js - jr, je - jr + 1), (js - ng, js - jr)]
            for l in range(3):
                jshift = ji + l - 1 if n == 0 else l - 1 - ji
                t = find_target_mb(lx2, jshift, nmbx2)
                recv[t][jdst[l][0]:jdst[l][1]] = send[lx2][jsrc[l][0]:jsrc[l][1]]
        elif jr < (nx2 - ng):                 # --- CASE 2
            if n == 0:
                jsrc = [(js, je + ng - jr + 1), (je - (ng - 1) - jr, je + 1)]
                jdst = [(js + jr, je + ng + 1), (js - ng, js + jr)]
            else:
                jsrc = [(js, js + ng + jr), (js - ng + jr, je + 1)]
                jdst = [(je - jr + 1, je + ng + 1), (js - ng, je - jr + 1)]
            for l in range(2):
                jshift = ji + l if n == 0 else l - 1 - ji
                t = find_target_mb(lx2, jshift, nmbx2)
                recv[t][jdst[l][0]:jdst[l][1]] = send[lx2][jsrc[l][0]:jsrc[l][1]]
        else:                                 # --- CASE 3
            if n == 0:
                jsrc = [(js, js + ng + (nx2 - jr)), (js, je + 1), (je - (ng - 1) + (nx2 - jr), je + 1)]
                jdst = [(je + 1 - (nx2 - jr), je + ng + 1), (js - (nx2 - jr), je - (nx2 - jr) + 1), (js - ng, js - (nx2 - jr))]
            else:
                jsrc = [(js, js + ng - (nx2 - jr)), (js, je + 1), (je - (ng - 1) - (nx2 - jr), je + 1)]
                jdst = [(je + 1 + (nx2 - jr), je + ng + 1), (js + (nx2 - jr), je + (nx2 - jr) + 1), (js - ng, js + (nx2 - jr))]
            for l in range(3):
                jshift = ji + l if n == 0 else l - 2 - ji
                t = find_target_mb(lx2, jshift, nmbx2)
                recv[t][jdst[l][0]:jdst[l][1]] = send[lx2][jsrc[l][0]:jsrc[l][1]]
    return recv


def shear_boundary_cc(pk, u0, yshear, recon):
    """PackAndSendCC + RecvAndUnpackCC on one rank: returns the copy of u0 with the x1 ghost slabs of the blocks on the
    x1 faces remapped and shifted"""
    u = u0.copy()
    ng, nx2 = pk.ng, pk.nx2
    js, je = pk.js, pk.je
    remap = remap_flux_of(recon)
    faces = pk.x1_faces()
    for n in (0, 1):
        col = slice(0, ng) if n == 0 else slice(pk.ie + 1, pk.ie + 1 + ng)
        send = {}
        for mm in faces[n]:
            a_ = np.moveaxis(u0[mm][:, :, :, col], 2, 0)       # (j, v, k, i): all k, ghost planes included in 3-D
            dx2 = pk.dx[mm, 1]
            eps = math.fmod(yshear, dx2)/dx2
            if n == 1:
                eps *= -1.0
            flx = remap(js, je + 1, eps, a_)
            sb = np.full(a_.shape, np.nan)
            j = np.arange(js, je + 1)
            sb[j] = a_[j] - (flx[j + 1] - flx[j])
            send[mm] = sb
        # the integer shift, for every x2 row of blocks with the same lx1 and lx3
        for mm in faces[n]:
            l1, l2, l3 = pk.lloc[mm]
            if l2 != 0:
                continue
            row = [pk.gid[(l1, b, l3)] for b in range(pk.nmb2)]
            joffset = int(yshear/pk.dx[mm, 1])
            recv = shift_cases([send[r] for r in row], n, joffset, ng, nx2)
            for r, rb in zip(row, recv):
                u[r][:, :, :, col] = np.moveaxis(rb, 0, 2)
    return u


# ---- orbital_advection_cc.cpp ----------------------------------------------------------------------------------------
def orbital_advection_cc(pk, u0, qshear, omega0, dt, maxjshift, recon):
    """PackAndSendCC (:53-128, the buffers filled from the x2 neighbours' active rows) and RecvAndUnpackCC (:215-288);
    returns (copy of u0 with the active cells remapped, the largest |joffset|)"""
    u = u0.copy()
    ng, nx2 = pk.ng, pk.nx2
    js, je, ks, ke = pk.js, pk.je, pk.ks, pk.ke
    remap = remap_flux_of(recon)
    nb = ng + maxjshift
    jfs = ng + maxjshift
    jfe = jfs + nx2 - 1
    nfx = nx2 + 2*(ng + maxjshift)
    qo = qshear*omega0
    jmax = 0
    for m in range(pk.nmb):
        lo, hi = pk.neighbour(m, 0, -1, 0), pk.neighbour(m, 0, 1, 0)
        # rbuf[0] of m: what its inner neighbour packed with n = 1 (jl = je-(ng+maxjshift-1) .. je); rbuf[1]: what its
        # outer neighbour packed with n = 0 (js .. js+(ng+maxjshift-1))
        rbuf0 = u0[lo][:, ks:ke + 1, je - (nb - 1):je + 1, :]
        rbuf1 = u0[hi][:, ks:ke + 1, js:js + nb, :]
        for i in range(pk.is_, pk.ie + 1):
            x1v = float(CellCenterX(i - pk.is_, pk.nx1, pk.bounds[m, 0], pk.bounds[m, 1]))
            dx2 = pk.dx[m, 1]
            yshear = -(qo)*x1v*dt
            joffset = int(yshear/dx2)
            jmax = max(jmax, abs(joffset))
            a_ = np.empty((nfx, u0.shape[1], ke - ks + 1))
            a_[:jfs] = np.moveaxis(rbuf0[:, :, :, i], 2, 0)
            a_[jfs:jfe + 1] = np.moveaxis(u0[m][:, ks:ke + 1, js:je + 1, i], 2, 0)
            a_[jfe + 1:] = np.moveaxis(rbuf1[:, :, :, i], 2, 0)
            epsi = math.fmod(yshear, dx2)/dx2
            flx = remap(jfs - joffset, jfe + 1 - joffset, epsi, a_)
            jf = np.arange(js, je + 1) - js + jfs
            new = a_[jf - joffset] - (flx[jf + 1 - joffset] - flx[jf - joffset])
            u[m][:, ks:ke + 1, js:je + 1, i] = np.moveaxis(new, 0, 2)
    return u, jmax


# ---- the bound on the change of a periodic pencil's sum ----------------------------------------------------------------
# |flux| <= F max|a| for |eps| < 1, crude but derived from the formulas (A = max|a|):
#   DC    eps*u: F = 1.
#   PLM   the harmonic mean of two slopes of one sign is at most twice the smaller, |dqm| <= 2*2A; |1 -/+ eps| <= 2:
#         |u + 0.5 (1 -/+ eps) dqm| <= A + 0.5*2*4A: F = 5.
#   PPMX  fourth-order face (7*2A + 2A)/12 = 4A/3; |d2ulim| <= |d2uc| <= 3 (A + 8A/3 + A) = 14A, limited face
#         0.5 (2A + 14A/3) < 3.34A; the extremum branch moves it to u + (face - u) r with |r| <= 1: < 5.34A; the last limiter
#         may replace it by 3u - 2 face': < 14A.  Then |du| <= 28A, |u6| <= 6 (A + 14A) = 90A, 0.75 qx <= 0.5, |1 - qx| <= 1:
#         |face + 0.75 qx (du + (1 - qx) u6)| <= 14A + 0.5 (28 + 90) A: F = 73.
FLUX_BOUND = {"dc": 1, "plm": 5, "ppmx": 73}


def conservation_factor(recon):
    """sum_j new(j) = sum_j a(j) exactly in real arithmetic on a periodic pencil (the fluxes telescope).  Per cell two
    operations are rounded, d = fhi - flo and a - d, to half an ulp (2^-53) of results of at most 2F max|a| and (1 + 2F) max|a|:
    (4F + 1)/2 ulp(max|a|) per cell, in units of 2^-52.  The two sums themselves are taken with math.fsum (one rounding
    each, of at most nx2 max|a|): one more unit.  The bound is nx2 * 2^-52 * max|a| times this integer."""
    return math.ceil((4*FLUX_BOUND[recon] + 1)/2) + 1


def periodic_sum_defect(a_new, a_old):
    """(|fsum(new) - fsum(old)| per pencil, i.e. over axis 0), elementwise over the other axes"""
    flat_n, flat_o = a_new.reshape(a_new.shape[0], -1), a_old.reshape(a_old.shape[0], -1)
    return np.array([abs(math.fsum(flat_n[:, c]) - math.fsum(flat_o[:, c])) for c in range(flat_n.shape[1])])
