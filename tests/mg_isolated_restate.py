"""Plain-numpy restatement of the isolated-gravity half of the reference's multigrid solver, on top of tests/mg_restate.py:
the physical boundaries of the block levels (MultigridDriver::PhysicalBoundary, multigrid_tasks.cpp:129-360) and of the
root grid (MGRootBoundary, multigrid_driver.cpp:1835-2026), the multipole moments, their scaling and the centre of mass
(:2213-2434), EvalMultipolePhi (multigrid.hpp:680-708), the source mask (multigrid.cpp:360-388), MGGravityDriver::Solve
with all of these (mg_gravity.cpp:177-245), and the two-sphere problem (src/pgen/tests/binary_gravity.cpp).

Written from those sources; shares no code with athenak_amd/ or csrc/akmi_mg.hip.  The boundary fills are written the way
the reference runs them -- receive from the neighbours that exist, then sweep x1, x2, x3 -- and not as the one-pass
composite rule of the library, so comparing the two checks that rule.

Two things are the library's and not the reference's:
 * the moment sums have the order of mg_restate.ordered_sum (a row ascending in i from 0.0, rows ascending in j, planes
   in k, blocks in m from 0.0); the reference sums one block serially in one thread, which differs by rounding only;
 * under multipole, edge and corner ghosts that touch a multipole face are never written by a boundary fill.  On the
   block levels that is the reference too.  On the root grid with a PERIODIC direction next to a multipole one the
   reference's periodic sweep runs over the full extent and copies the face ghost of the previous call into the edge;
   the library leaves the edge alone, and so does root_boundary_bc here.  Those cells keep what the last whole-array
   operation left in them (StoreOldData / ComputeCorrection of the previous visit of the level, SetFromRootGrid on the
   1-cell block level, zero before any); both prolongations read them.
"""
import math

import numpy as np

import mg_restate as R

NONE, ZEROFIXED, ZEROGRAD, MULTIPOLE = 0, 1, 2, 3
BC = {"none": NONE, "zerofixed": ZEROFIXED, "zerograd": ZEROGRAD, "multipole": MULTIPOLE}


# ---- geometry ----------------------------------------------------------------------------------------------------------
def left_edge(ith, n, xmin, xmax):
    """LeftEdgeX, src/coordinates/cell_locations.hpp:23-28"""
    x = np.asarray(ith, dtype=np.float64)/np.float64(n)
    return (x*xmax - x*xmin) - (0.5*xmax - 0.5*xmin) + (0.5*xmin + 0.5*xmax)


def cell_center(ith, n, xmin, xmax):
    """CellCenterX, cell_locations.hpp:35-39"""
    x = (np.asarray(ith, dtype=np.float64) + 0.5)/np.float64(n)
    return (x*xmax - x*xmin) - (0.5*xmax - 0.5*xmin) + (0.5*xmin + 0.5*xmax)


def block_extents(lloc, nrb, ext):
    """mb_size of every block (meshblock.cpp:60-115): (nmb, 6) = x1min, x1max, x2min, ...; ext: the mesh's"""
    out = np.zeros((len(lloc), 6))
    for m, l in enumerate(lloc):
        for q in range(3):
            lo, hi = ext[2*q], ext[2*q + 1]
            out[m, 2*q] = lo if l[q] == 0 else float(left_edge(l[q], nrb[q], lo, hi))
            out[m, 2*q + 1] = hi if l[q] == nrb[q] - 1 else float(left_edge(l[q] + 1, nrb[q], lo, hi))
    return out


def neighbor_table(lloc, nrb, periodic):
    """same-level neighbours, -1 beyond a non-periodic face of the mesh; periodic: six flags ix1, ox1, ix2, ..."""
    where = {tuple(l): m for m, l in enumerate(lloc)}
    tab = -np.ones((len(lloc), 27), dtype=np.int32)
    for m, l in enumerate(lloc):
        for d in range(27):
            if d == 13:
                continue
            o = (d % 3 - 1, (d//3) % 3 - 1, d//9 - 1)
            n, ok = [0, 0, 0], True
            for q in range(3):
                n[q] = l[q] + o[q]
                if n[q] < 0:
                    ok, n[q] = ok and bool(periodic[2*q]), n[q] + nrb[q]
                elif n[q] >= nrb[q]:
                    ok, n[q] = ok and bool(periodic[2*q + 1]), n[q] - nrb[q]
            if ok:
                tab[m, d] = where[tuple(n)]
    return tab


# ---- the expansion -----------------------------------------------------------------------------------------------------
def eval_multipole_phi(x, y, z, mpc, order):
    """EvalMultipolePhi, multigrid.hpp:680-708"""
    x2, y2, z2 = x*x, y*y, z*z
    xy, yz, zx = x*y, y*z, z*x
    r2 = x2 + y2 + z2
    ir2 = 1.0/r2
    ir1 = np.sqrt(ir2)
    ir3 = ir2*ir1
    ir5 = ir3*ir2
    hx2my2 = 0.5*(x2 - y2)
    phis = (ir1*mpc[0]
            + ir3*(mpc[1]*y + mpc[2]*z + mpc[3]*x)
            + ir5*(mpc[4]*xy + mpc[5]*yz + (3.0*z2 - r2)*mpc[6]
                   + mpc[7]*zx + mpc[8]*hx2my2))
    if order == 4:
        ir7 = ir5*ir2
        ir9 = ir7*ir2
        x2mty2 = x2 - 3.0*y2
        tx2my2 = 3.0*x2 - y2
        phis = phis + (ir7*(y*tx2my2*mpc[9] + x*x2mty2*mpc[15]
                            + xy*z*mpc[10] + z*hx2my2*mpc[14]
                            + (5.0*z2 - r2)*(y*mpc[11] + x*mpc[13])
                            + z*(z2 - 3.0*r2)*mpc[12])
                       + ir9*(xy*hx2my2*mpc[16]
                              + 0.125*(x2*x2mty2 - y2*tx2my2)*mpc[24]
                              + yz*tx2my2*mpc[17] + zx*x2mty2*mpc[23]
                              + (7.0*z2 - r2)*(xy*mpc[18] + hx2my2*mpc[22])
                              + (7.0*z2 - 3.0*r2)*(yz*mpc[19] + zx*mpc[21])
                              + (35.0*z2*z2 - 30.0*z2*r2 + 3.0*r2*r2)*mpc[20]))
    return phis


def _sum0(v):
    """(nmb, n3, n2, n1) -> float: the row from 0.0 ascending in i, then j, then k from the first entry, the blocks from
    0.0 ascending in m"""
    s = np.zeros(v.shape[:-1])
    for i in range(v.shape[-1]):
        s = s + v[..., i]
    for _ in range(2):
        t = s[..., 0].copy()
        for q in range(1, s.shape[-1]):
            t = t + s[..., q]
        s = t
    tot = 0.0
    for m in range(s.shape[0]):
        tot += float(s[m])
    return tot


def _cell_offsets(src, xlim, origin):
    """x, y, z of the active cells as CalculateMultipoleCoefficients forms them, s = src*vol; each (nmb, n3, n2, n1)"""
    nmb = src.shape[0]
    n3, n2, n1 = (q - 2 for q in src.shape[1:])
    X, Y, Z, S = (np.zeros((nmb, n3, n2, n1)) for _ in range(4))
    for m in range(nmb):
        e = xlim[m]
        dx1 = (e[1] - e[0])/float(n1)
        dx2 = (e[3] - e[2])/float(n2)
        dx3 = (e[5] - e[4])/float(n3)
        vol = dx1*dx2*dx3
        x = e[0] + (np.arange(n1) + 0.5)*dx1 - origin[0]
        y = e[2] + (np.arange(n2) + 0.5)*dx2 - origin[1]
        z = e[4] + (np.arange(n3) + 0.5)*dx3 - origin[2]
        Z[m], Y[m], X[m] = np.meshgrid(z, y, x, indexing="ij")
        S[m] = R.act(src)[m]*vol
    return X, Y, Z, S


def center_of_mass(src, xlim):
    """CalculateCenterOfMass, multigrid_driver.cpp:2374-2434 -> (x, y, z)"""
    x, y, z, s = _cell_offsets(src, xlim, (0.0, 0.0, 0.0))
    m0, m1, m2, m3 = _sum0(s), _sum0(s*y), _sum0(s*z), _sum0(s*x)
    im = 1.0/m0
    return np.array([im*m3, im*m1, im*m2])


def raw_moments(src, xlim, origin, order, nodipole=False):
    """CalculateMultipoleCoefficients before the scaling, multigrid_driver.cpp:2232-2307"""
    x, y, z, s = _cell_offsets(src, xlim, origin)
    x2, y2, z2 = x*x, y*y, z*z
    xy, yz, zx = x*y, y*z, z*x
    r2 = x2 + y2 + z2
    hx2my2 = 0.5*(x2 - y2)
    zero = np.zeros_like(s)
    t = [s, zero if nodipole else s*y, zero if nodipole else s*z, zero if nodipole else s*x,
         s*xy, s*yz, s*(3.0*z2 - r2), s*zx, s*hx2my2]
    if order == 4:
        tx2my2 = 3.0*x2 - y2
        x2mty2 = x2 - 3.0*y2
        fz2mr2 = 5.0*z2 - r2
        sz2mr2 = 7.0*z2 - r2
        sz2mtr2 = 7.0*z2 - 3.0*r2
        t += [s*y*tx2my2, s*xy*z, s*y*fz2mr2, s*z*(z2 - 3.0*r2), s*x*fz2mr2, s*z*hx2my2, s*x*x2mty2,
              s*xy*hx2my2, s*yz*tx2my2, s*xy*sz2mr2, s*yz*sz2mtr2,
              s*(35.0*z2*z2 - 30.0*z2*r2 + 3.0*r2*r2), s*zx*sz2mtr2, s*hx2my2*sz2mr2, s*zx*x2mty2,
              s*0.125*(x2*x2mty2 - y2*tx2my2)]
    return np.array([_sum0(v) for v in t])


def scale_moments(mp):
    """ScaleMultipoleCoefficients, multigrid_driver.cpp:2322-2367"""
    pi = math.pi
    c0 = c1 = 0.25/pi
    c2, c2a = 0.0625/pi, 0.75/pi
    c30, c31, c32, c33 = 0.0625/pi, 0.0625*1.5/pi, 0.25*15.0/pi, 0.0625*2.5/pi
    c40, c41, c42, c43, c44 = 0.0625*0.0625/pi, 0.0625*2.5/pi, 0.0625*5.0/pi, 0.0625*17.5/pi, 0.25*35.0/pi
    sc = [c0, c1, c1, c1, c2a, c2a, c2, c2a, c2a, c33, c32, c31, c30, c31, c32, c33,
          c44, c43, c42, c41, c40, c41, c42, c43, c44]
    return np.array([mp[c]*sc[c] for c in range(len(mp))])


def multipole(src, xlim, order, nodipole=False, origin=None):
    """(25 coefficients -- those beyond the order zero --, origin): what Solve computes before the cycles"""
    org = center_of_mass(src, xlim) if origin is None else np.array(origin, dtype=np.float64)
    mp = np.zeros(25)
    c = scale_moments(raw_moments(src, xlim, org, order, nodipole))
    mp[:len(c)] = c
    return mp, org


def apply_mask(src, xlim, radius, origin):
    """Multigrid::ApplyMask, multigrid.cpp:360-388 (in place, active cells)"""
    if radius <= 0.0:
        return
    n3, n2, n1 = (q - 2 for q in src.shape[1:])
    for m in range(src.shape[0]):
        e = xlim[m]
        x = cell_center(np.arange(n1), n1, e[0], e[1])
        y = cell_center(np.arange(n2), n2, e[2], e[3])
        z = cell_center(np.arange(n3), n3, e[4], e[5])
        Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
        r2 = (X - origin[0])*(X - origin[0]) + (Y - origin[1])*(Y - origin[1]) + (Z - origin[2])*(Z - origin[2])
        R.act(src)[m][r2 > radius*radius] = 0.0


# ---- boundaries --------------------------------------------------------------------------------------------------------
def _multipole_faces(a, faces, ext, mp, org, order):
    """the six multipole loops of PhysicalBoundary / MGRootBoundary on one array a (n3+2, n2+2, n1+2); faces: six flags
    (ix1, ox1, ...) of the faces to fill; ext: the extents the cell widths are formed from"""
    n3, n2, n1 = (q - 2 for q in a.shape)
    n = (n1, n2, n3)
    cen = []
    for q in range(3):
        dxl = (ext[2*q + 1] - ext[2*q])/float(n[q])
        cen.append(ext[2*q] + (np.arange(n[q]) + 0.5)*dxl - org[q])
    for q in range(3):                              # x1, x2, x3 faces
        for side in (0, 1):
            if not faces[2*q + side]:
                continue
            c = list(cen)
            c[q] = np.array([ext[2*q + side] - org[q]])
            Z, Y, X = np.meshgrid(c[2], c[1], c[0], indexing="ij")
            phis = eval_multipole_phi(X, Y, Z, mp, order)
            g = [slice(1, n3 + 1), slice(1, n2 + 1), slice(1, n1 + 1)]
            s = list(g)
            g[2 - q] = slice(0, 1) if side == 0 else slice(n[q] + 1, n[q] + 2)
            s[2 - q] = slice(1, 2) if side == 0 else slice(n[q], n[q] + 1)
            a[tuple(g)] = 2.0*phis - a[tuple(s)]


def _mirror_sweeps(a, faces, sign):
    """the mirror loops over the FULL extent of the other two directions, x1 then x2 then x3"""
    if faces[0]:
        a[:, :, 0] = sign*a[:, :, 1]
    if faces[1]:
        a[:, :, -1] = sign*a[:, :, -2]
    if faces[2]:
        a[:, 0, :] = sign*a[:, 1, :]
    if faces[3]:
        a[:, -1, :] = sign*a[:, -2, :]
    if faces[4]:
        a[0, :, :] = sign*a[1, :, :]
    if faces[5]:
        a[-1, :, :] = sign*a[-2, :, :]


def exchange_bc(u, tab, bc, mp=None, org=None, order=4, xlim=None):
    """the receive of one level (every ghost region whose neighbour exists: mg_restate.exchange with the entries < 0
    skipped), then PhysicalBoundary on every block: the faces whose FACE entry of the table is < 0"""
    n3, n2, n1 = (s - 2 for s in u.shape[1:])
    n = (n1, n2, n3)
    old = u.copy()

    def dst(o, q):
        return slice(1, n[q] + 1) if o == 0 else (slice(0, 1) if o < 0 else slice(n[q] + 1, n[q] + 2))

    def srcs(o, q):
        return slice(1, n[q] + 1) if o == 0 else (slice(n[q], n[q] + 1) if o < 0 else slice(1, 2))
    for m in range(u.shape[0]):
        for d in range(27):
            if d == 13 or tab[m, d] < 0:
                continue
            o1, o2, o3 = d % 3 - 1, (d//3) % 3 - 1, d//9 - 1
            u[m, dst(o3, 2), dst(o2, 1), dst(o1, 0)] = old[tab[m, d], srcs(o3, 2), srcs(o2, 1), srcs(o1, 0)]
    if bc == NONE:
        return
    for m in range(u.shape[0]):
        faces = [tab[m, 12] < 0, tab[m, 14] < 0, tab[m, 10] < 0, tab[m, 16] < 0, tab[m, 4] < 0, tab[m, 22] < 0]
        if bc == MULTIPOLE:
            _multipole_faces(u[m], faces, xlim[m], mp, org, order)
        else:
            _mirror_sweeps(u[m], faces, -1.0 if bc == ZEROFIXED else 1.0)


def root_boundary_bc(u, bc, periodic, mp=None, org=None, order=4, ext=None):
    """MGRootBoundary, multigrid_driver.cpp:1857-2026: per direction the periodic copy or the mirror over the full
    extent, x1 then x2 then x3, then the multipole faces.  (Under multipole, see the head of this file: the edges and
    corners that touch a multipole face are put back.)"""
    a = u[0]
    keep = a.copy() if bc == MULTIPOLE else None
    sign = -1.0 if bc == ZEROFIXED else 1.0
    mirror = bc in (ZEROFIXED, ZEROGRAD)
    for q, ax in ((0, 2), (1, 1), (2, 0)):
        lo, lo_src, per_lo_src = [slice(None)]*3, [slice(None)]*3, [slice(None)]*3
        hi, hi_src, per_hi_src = [slice(None)]*3, [slice(None)]*3, [slice(None)]*3
        lo[ax], lo_src[ax], per_lo_src[ax] = 0, 1, -2
        hi[ax], hi_src[ax], per_hi_src[ax] = -1, -2, 1
        if periodic[2*q]:
            a[tuple(lo)] = a[tuple(per_lo_src)]
        elif mirror:
            a[tuple(lo)] = sign*a[tuple(lo_src)]
        if periodic[2*q + 1]:
            a[tuple(hi)] = a[tuple(per_hi_src)]
        elif mirror:
            a[tuple(hi)] = sign*a[tuple(hi_src)]
    if bc == MULTIPOLE:
        faces = [not p for p in periodic]
        n3, n2, n1 = (s - 2 for s in a.shape)
        touch = np.zeros(a.shape, dtype=bool)        # ghosts beyond a multipole face ...
        for q, ax in ((0, 2), (1, 1), (2, 0)):
            for side in (0, 1):
                if faces[2*q + side]:
                    sl = [slice(None)]*3
                    sl[ax] = 0 if side == 0 else -1
                    touch[tuple(sl)] = True
        K, J, I = np.meshgrid(np.arange(n3 + 2), np.arange(n2 + 2), np.arange(n1 + 2), indexing="ij")
        nout = ((K == 0) | (K == n3 + 1)).astype(int) + ((J == 0) | (J == n2 + 1)) + ((I == 0) | (I == n1 + 1))
        edge = touch & (nout > 1)                     # ... that are edges or corners
        a[edge] = keep[edge]
        _multipole_faces(a, faces, ext, mp, org, order)


# ---- the solver ----------------------------------------------------------------------------------------------------------
class IsolatedSolver(R.MGSolver):
    """MGGravityDriver with physical faces: mesh_ext = (x1min, x1max, x2min, ...), periodic = six flags, mg_bc one of
    BC.  subtract_average is off (mg_gravity.cpp:88-90, 119)."""

    def __init__(self, mesh_n, block_n, mesh_ext, lloc, four_pi_G, mg_bc, periodic=(0,)*6, mporder=4, nodipole=False,
                 mporigin=None, mask_radius=-1.0, mask_origin=(0.0, 0.0, 0.0), **kw):
        mesh_len = tuple(mesh_ext[2*q + 1] - mesh_ext[2*q] for q in range(3))
        kw["subtract_average"] = False
        super().__init__(mesh_n, block_n, mesh_len, lloc, four_pi_G, **kw)
        self.bc = BC[mg_bc] if isinstance(mg_bc, str) else mg_bc
        self.periodic = tuple(int(p) for p in periodic)
        self.ext = tuple(mesh_ext)
        self.tab = neighbor_table(self.lloc, self.nrb, self.periodic)
        self.xlim = block_extents(self.lloc, self.nrb, self.ext)
        self.blocks.rdx = (self.xlim[0][1] - self.xlim[0][0])/float(block_n)      # block_rdx, multigrid.cpp:87-92
        self.order, self.nodipole, self.fixed_origin = mporder, nodipole, mporigin
        self.mask_radius, self.mask_origin = mask_radius, mask_origin
        self.mp, self.org = np.zeros(25), np.zeros(3)

    def _bnd(self, mg):
        if mg.root:
            root_boundary_bc(mg.c.u, self.bc, self.periodic, self.mp, self.org, self.order, self.ext)
        else:
            exchange_bc(mg.c.u, self.tab, self.bc, self.mp, self.org, self.order, self.xlim)

    def solve(self, u0):
        """MGGravityDriver::Solve, mg_gravity.cpp:177-245"""
        mg = self.blocks
        self.norms, self.ncycles = [], 0
        mg.lev[-1].src[...] = R.load_source(u0, self.ng, -self.four_pi_G)
        apply_mask(mg.lev[-1].src, self.xlim, self.mask_radius, self.mask_origin)
        mg.current = mg.nlevel - 1
        if not self.fmg:
            o = self.ng
            R.act(mg.c.u)[...] = self.phi[:, 0, o:-o, o:-o, o:-o]
        self.current_level = self.ntotallevel - 1
        self.fmglevel = self.current_level
        if self.bc == MULTIPOLE:
            self.mp, self.org = multipole(mg.lev[-1].src, self.xlim, self.order, self.nodipole, self.fixed_origin)
        if self.fmg:
            self.solve_fmg()
        else:
            self.solve_mg()
        o = self.ng - 1
        self.phi[:, 0, o:self.phi.shape[2] - o, o:self.phi.shape[3] - o, o:self.phi.shape[4] - o] = mg.lev[-1].u
        return self.phi


# ---- the two-sphere problem, src/pgen/tests/binary_gravity.cpp -------------------------------------------------------
BINARY = dict(x1=0.125, y1=0.0, z1=0.0, x2=-0.25, y2=0.0, z2=0.0, radius=0.125, m1=2.0, m2=1.0)   # inputs/binary_gravity.athinput


def binary_density(block_n, xlim, ng, prm=BINARY):
    """binary_gravity.cpp:62-212 -> u0 (nmb, 1, n+2ng, ...): two uniform spheres, cells near a surface sub-sampled
    10^3, rescaled to the total mass m1 + m2"""
    r = prm["radius"]
    den = [prm["m1"]/((4.0*math.pi/3.0)*r*r*r), prm["m2"]/((4.0*math.pi/3.0)*r*r*r)]
    cen = [(prm["x1"], prm["y1"], prm["z1"]), (prm["x2"], prm["y2"], prm["z2"])]
    nmb, n = len(xlim), block_n
    u0 = np.zeros((nmb, 1) + (n + 2*ng,)*3)
    total = 0.0
    sub = np.arange(10) + 0.5
    for m in range(nmb):
        e = xlim[m]
        dx = (e[1] - e[0])/float(n)
        dd, dv, dr = 0.1*dx, 1.0e-3, 0.6*1.7320508075688772*dx
        c = [cell_center(np.arange(n), n, e[2*q], e[2*q + 1]) for q in range(3)]
        f = [left_edge(np.arange(n), n, e[2*q], e[2*q + 1]) for q in range(3)]
        rho = np.zeros((n, n, n))
        for k in range(n):
            for j in range(n):
                for i in range(n):
                    v = 1.0e-300
                    for s in (0, 1):
                        cx, cy, cz = cen[s]
                        rs = math.sqrt((c[0][i] - cx)*(c[0][i] - cx) + (c[1][j] - cy)*(c[1][j] - cy)
                                       + (c[2][k] - cz)*(c[2][k] - cz))
                        if not rs < r + dr:
                            continue
                        if rs < r - dr:
                            v = den[s]
                            continue
                        zz = (f[2][k] + sub*dd)[:, None, None]
                        yy = (f[1][j] + sub*dd)[None, :, None]
                        xx = (f[0][i] + sub*dd)[None, None, :]
                        rr = np.sqrt((xx - cx)*(xx - cx) + (yy - cy)*(yy - cy) + (zz - cz)*(zz - cz))
                        n_in = int((rr < r).sum())
                        v = (1.0e-300 if s == 0 else v) + dv*den[s]*float(n_in)
                    rho[k, j, i] = v
        u0[m, 0, ng:-ng, ng:-ng, ng:-ng] = rho
        total += float(np.sum(rho*(dx*dx*dx)))
    msum = prm["m1"] + prm["m2"]
    u0[:, 0] *= (msum/total) if total > 0.0 else 1.0
    return u0, total


def binary_errors(phi, block_n, xlim, ng, mesh_ext, four_pi_G=1.0, prm=BINARY):
    """BinaryGravityErrors, binary_gravity.cpp:240-383 -> (potential L2, acceleration L2, max potential, max accel.)"""
    G = four_pi_G/(4.0*math.pi)
    rad, n = prm["radius"], block_n
    den = [prm["m1"]/((4.0*math.pi/3.0)*rad*rad*rad), prm["m2"]/((4.0*math.pi/3.0)*rad*rad*rad)]
    mass = [prm["m1"], prm["m2"]]
    cen = [(prm["x1"], prm["y1"], prm["z1"]), (prm["x2"], prm["y2"], prm["z2"])]
    pot_l1 = acc_l1 = pot_max = acc_max = 0.0
    A = slice(ng, ng + n)
    P, M = slice(ng + 1, ng + n + 1), slice(ng - 1, ng + n - 1)
    for m in range(len(xlim)):
        e = xlim[m]
        dx, dy, dz = ((e[2*q + 1] - e[2*q])/float(n) for q in range(3))
        vol = dx*dy*dz
        c = [cell_center(np.arange(n), n, e[2*q], e[2*q + 1]) for q in range(3)]
        Z, Y, X = np.meshgrid(c[2], c[1], c[0], indexing="ij")
        pot0 = ax0 = ay0 = az0 = 0.0
        for s in (0, 1):
            cx, cy, cz = cen[s]
            rs = np.sqrt((X - cx)*(X - cx) + (Y - cy)*(Y - cy) + (Z - cz)*(Z - cz))
            out = rs > rad
            with np.errstate(divide="ignore", invalid="ignore"):
                pp = np.where(out, -G*mass[s]/rs, -G*math.pi*2.0/3.0*den[s]*(3.0*rad*rad - rs*rs))
                ff = np.where(out, -G*mass[s]/(rs*rs*rs), -G*math.pi*4.0/3.0*den[s])
            pot0 = pot0 + pp
            ax0, ay0, az0 = ax0 + ff*(X - cx), ay0 + ff*(Y - cy), az0 + ff*(Z - cz)
        p = phi[m, 0]
        ax_n = -(p[A, A, P] - p[A, A, M])/(2.0*dx)
        ay_n = -(p[A, P, A] - p[A, M, A])/(2.0*dy)
        az_n = -(p[P, A, A] - p[M, A, A])/(2.0*dz)
        perr = np.abs((pot0 - p[A, A, A])/pot0)
        d2 = ax0*ax0 + ay0*ay0 + az0*az0
        with np.errstate(divide="ignore", invalid="ignore"):
            aerr = np.where(d2 > 0.0, np.sqrt(((ax_n - ax0)*(ax_n - ax0) + (ay_n - ay0)*(ay_n - ay0)
                                               + (az_n - az0)*(az_n - az0))/d2), 0.0)
        pot_l1 += float(np.sum(perr*vol))
        acc_l1 += float(np.sum(aerr*vol))
        pot_max, acc_max = max(pot_max, float(perr.max())), max(acc_max, float(aerr.max()))
    tvol = (mesh_ext[1] - mesh_ext[0])*(mesh_ext[3] - mesh_ext[2])*(mesh_ext[5] - mesh_ext[4])
    return math.sqrt(pot_l1/tvol), math.sqrt(acc_l1/tvol), pot_max, acc_max
