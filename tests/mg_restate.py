"""Plain-numpy restatement of the multigrid Poisson solver of the reference (src/multigrid/multigrid.cpp,
multigrid.hpp, multigrid_driver.cpp, multigrid_tasks.cpp, src/gravity/mg_gravity.cpp, mg_gravity.hpp) and of
SourceTerms::SelfGravity (src/srcterms/srcterms.cpp:215-310), for one rank, a uniform periodic mesh and mg_nghost = 1.

Written from those sources; shares no code with athenak_amd/gravity.py or csrc/akmi_mg.hip.  Every expression keeps
the reference's order of operations, so the device results are compared with array_equal.  An MG level is an array
(nmb, n3+2, n2+2, n1+2) (the variable axis of the reference, always of length one here, is dropped).

The reference leaves the order of its parallel sums (average, defect norm) open; the order taken here is the one the
library documents: a row ascending in i, the rows of a plane ascending in j, the planes ascending in k, the blocks
ascending in m.
"""
import math

import numpy as np


# ---- operators -------------------------------------------------------------------------------------------------------
def act(a):
    return a[:, 1:-1, 1:-1, 1:-1]


def laplacian(u):
    """GravityStencil::Apply, mg_gravity.hpp:32-34, on the active cells"""
    return (6.0*u[:, 1:-1, 1:-1, 1:-1] - u[:, 2:, 1:-1, 1:-1] - u[:, 1:-1, 2:, 1:-1] - u[:, 1:-1, 1:-1, 2:]
            - u[:, :-2, 1:-1, 1:-1] - u[:, 1:-1, :-2, 1:-1] - u[:, 1:-1, 1:-1, :-2])


def smooth(u, src, dx, omega, color, coffset):
    """Multigrid::Smooth, multigrid.hpp:622-647 (in place).  Cells of one colour have no neighbour of that colour, so
    the Laplacian of the old array is the one the loop sees."""
    odiag = omega/6.0
    color ^= coffset
    dx2 = dx*dx
    lap = laplacian(u)
    n3, n2, n1 = lap.shape[1:]
    k = np.arange(1, n3 + 1)[:, None, None]
    j = np.arange(1, n2 + 1)[None, :, None]
    i = np.arange(1, n1 + 1)[None, None, :]
    c = (color + k + j) & 1                   # i = il + c, il + c + 2, ... with il = 1
    mask = np.broadcast_to(((i - 1 - c) % 2) == 0, lap.shape[1:])
    a = act(u)
    new = a - (lap - act(src)*dx2)*odiag
    a[:, mask] = new[:, mask]


def defect(u, src, dfc, dx):
    """CalculateDefect, multigrid.hpp:284-290"""
    idx2 = 1.0/(dx*dx)
    act(dfc)[...] = act(src) - laplacian(u)*idx2


def fas_rhs(u, src, dx):
    """CalculateFASRHS, multigrid.hpp:305-311"""
    idx2 = 1.0/(dx*dx)
    act(src)[...] = act(src) + laplacian(u)*idx2


def restrict(fine, coarse):
    """Multigrid::Restrict, multigrid.cpp:881-892: fk = 2k - ngh"""
    n3, n2, n1 = (s - 2 for s in coarse.shape[1:])

    def s(dk, dj, di):
        return fine[:, 1 + dk:1 + dk + 2*n3:2, 1 + dj:1 + dj + 2*n2:2, 1 + di:1 + di + 2*n1:2]
    act(coarse)[...] = 0.125*(s(0, 0, 0) + s(0, 0, 1) + s(0, 1, 0) + s(0, 1, 1)
                              + s(1, 0, 0) + s(1, 0, 1) + s(1, 1, 0) + s(1, 1, 1))


def _shifted(c):
    n3, n2, n1 = (s - 2 for s in c.shape[1:])
    return lambda a, b, d: c[:, 1 + a:1 + a + n3, 1 + b:1 + b + n2, 1 + d:1 + d + n1]


def prolongate_correct(coarse, fine):
    """ProlongateAndCorrect, trilinear, multigrid.cpp:1053-1092: the eight statements, one per child"""
    S = _shifted(coarse)
    n3, n2, n1 = (s - 2 for s in coarse.shape[1:])

    def child(ck, cj, ci):
        return fine[:, 1 + ck:1 + ck + 2*n3:2, 1 + cj:1 + cj + 2*n2:2, 1 + ci:1 + ci + 2*n1:2]
    c = S(0, 0, 0)
    child(0, 0, 0)[...] += 0.015625*(27.0*c + S(-1, -1, -1) + 9.0*(S(0, 0, -1) + S(0, -1, 0) + S(-1, 0, 0))
                                     + 3.0*(S(-1, -1, 0) + S(-1, 0, -1) + S(0, -1, -1)))
    child(0, 0, 1)[...] += 0.015625*(27.0*c + S(-1, -1, 1) + 9.0*(S(0, 0, 1) + S(0, -1, 0) + S(-1, 0, 0))
                                     + 3.0*(S(-1, -1, 0) + S(-1, 0, 1) + S(0, -1, 1)))
    child(0, 1, 0)[...] += 0.015625*(27.0*c + S(-1, 1, -1) + 9.0*(S(0, 0, -1) + S(0, 1, 0) + S(-1, 0, 0))
                                     + 3.0*(S(-1, 1, 0) + S(-1, 0, -1) + S(0, 1, -1)))
    child(1, 0, 0)[...] += 0.015625*(27.0*c + S(1, -1, -1) + 9.0*(S(0, 0, -1) + S(0, -1, 0) + S(1, 0, 0))
                                     + 3.0*(S(1, -1, 0) + S(1, 0, -1) + S(0, -1, -1)))
    child(1, 1, 0)[...] += 0.015625*(27.0*c + S(1, 1, -1) + 9.0*(S(0, 0, -1) + S(0, 1, 0) + S(1, 0, 0))
                                     + 3.0*(S(1, 1, 0) + S(1, 0, -1) + S(0, 1, -1)))
    child(1, 0, 1)[...] += 0.015625*(27.0*c + S(1, -1, 1) + 9.0*(S(0, 0, 1) + S(0, -1, 0) + S(1, 0, 0))
                                     + 3.0*(S(1, -1, 0) + S(1, 0, 1) + S(0, -1, 1)))
    child(0, 1, 1)[...] += 0.015625*(27.0*c + S(-1, 1, 1) + 9.0*(S(0, 0, 1) + S(0, 1, 0) + S(-1, 0, 0))
                                     + 3.0*(S(-1, 1, 0) + S(-1, 0, 1) + S(0, 1, 1)))
    child(1, 1, 1)[...] += 0.015625*(27.0*c + S(1, 1, 1) + 9.0*(S(0, 0, 1) + S(0, 1, 0) + S(1, 0, 0))
                                     + 3.0*(S(1, 1, 0) + S(1, 0, 1) + S(0, 1, 1)))


# the literals of the first statement of FMGProlongate (multigrid.cpp:1123-1133), rows k-1 / k / k+1, each j-1, j, j+1
# with i-1, i, i+1: the child (fk, fj, fi).  The other seven statements are its mirror images: the literal of a term
# moves with the term when an axis is reflected for an upper child (compare :1135-1217).
_FMG000 = np.array([[[125., 750., -75.], [750., 4500., -450.], [-75., -450., 45.]],
                    [[750., 4500., -450.], [4500., 27000., -2700.], [-450., -2700., 270.]],
                    [[-75., -450., 45.], [-450., -2700., 270.], [45., 270., -27.]]])


def fmg_prolongate(coarse, fine):
    """FMGProlongate, tricubic, overwrites: the 27 terms added in the written order, then / 32768.0"""
    S = _shifted(coarse)
    n3, n2, n1 = (s - 2 for s in coarse.shape[1:])
    for ck in (0, 1):
        for cj in (0, 1):
            for ci in (0, 1):
                w = _FMG000[::-1] if ck else _FMG000
                w = w[:, ::-1] if cj else w
                w = w[:, :, ::-1] if ci else w
                acc = None
                for a in (-1, 0, 1):
                    for b in (-1, 0, 1):
                        for d in (-1, 0, 1):
                            term = w[a + 1, b + 1, d + 1]*S(a, b, d)
                            acc = term if acc is None else acc + term
                fine[:, 1 + ck:1 + ck + 2*n3:2, 1 + cj:1 + cj + 2*n2:2, 1 + ci:1 + ci + 2*n1:2] = acc/32768.0


def neighbor_table(lloc, nroot):
    """same-level periodic neighbours: tab[m][(ox3+1)*9 + (ox2+1)*3 + (ox1+1)]"""
    where = {tuple(l): m for m, l in enumerate(lloc)}
    tab = np.zeros((len(lloc), 27), dtype=np.int32)
    for m, l in enumerate(lloc):
        for d in range(27):
            o = (d % 3 - 1, (d//3) % 3 - 1, d//9 - 1)
            tab[m, d] = where[tuple((l[q] + o[q]) % nroot[q] for q in range(3))]
    return tab


def exchange(u, tab):
    """periodic ghost fill of one level: a ghost cell is the image of an active cell of the neighbour across that
    face, edge or corner (the block itself where the root grid is one block wide)"""
    n3, n2, n1 = (s - 2 for s in u.shape[1:])
    n = (n1, n2, n3)
    old = u.copy()

    def dst(o, q):
        return slice(1, n[q] + 1) if o == 0 else (slice(0, 1) if o < 0 else slice(n[q] + 1, n[q] + 2))

    def srcs(o, q):
        return slice(1, n[q] + 1) if o == 0 else (slice(n[q], n[q] + 1) if o < 0 else slice(1, 2))
    for m in range(u.shape[0]):
        for d in range(27):
            if d == 13:
                continue
            o1, o2, o3 = d % 3 - 1, (d//3) % 3 - 1, d//9 - 1
            u[m, dst(o3, 2), dst(o2, 1), dst(o1, 0)] = old[tab[m, d], srcs(o3, 2), srcs(o2, 1), srcs(o1, 0)]


def root_boundary(u):
    """MGRootBoundary, periodic, multigrid_driver.cpp:1857-1930: x1, then x2 with the x1 ghosts, then x3"""
    u[:, :, :, 0] = u[:, :, :, -2]
    u[:, :, :, -1] = u[:, :, :, 1]
    u[:, :, 0, :] = u[:, :, -2, :]
    u[:, :, -1, :] = u[:, :, 1, :]
    u[:, 0, :, :] = u[:, -2, :, :]
    u[:, -1, :, :] = u[:, 1, :, :]


def blocks_to_root(lloc, bsrc, bu, rsrc, ru, initflag):
    """TransferFromBlocksToRoot, multigrid_driver.cpp:514-523"""
    for m, (i, j, k) in enumerate(lloc):
        rsrc[0, k + 1, j + 1, i + 1] = bsrc[m, 1, 1, 1]
        if not initflag:
            ru[0, k + 1, j + 1, i + 1] = bu[m, 1, 1, 1]


def set_from_root(lloc, ru, ruold, bu, buold, folddata):
    """Multigrid::SetFromRootGrid, multigrid.cpp:626-643"""
    for m, (ci, cj, ck) in enumerate(lloc):
        bu[m] = ru[0, ck:ck + 3, cj:cj + 3, ci:ci + 3]
        if folddata:
            buold[m] = ruold[0, ck:ck + 3, cj:cj + 3, ci:ci + 3]


def ordered_sum(v):
    """(nmb, n3, n2, n1) -> float, in the documented order"""
    for _ in range(4):
        s = v[..., 0].copy() if v.ndim > 1 else v[0]
        for q in range(1, v.shape[-1]):
            s = s + v[..., q]
        v = s
    return float(v)


def average(a, dx, length):
    """Multigrid::CalculateAverage, multigrid.cpp:763-818"""
    dV = dx*dx*dx
    total = ordered_sum(act(a)*dV)
    volume = 0.0
    for _ in range(a.shape[0]):
        volume += length*length*length
    return total/volume if volume > 0.0 else 0.0


def defect_norm(dfc, vol):
    """l2: multigrid.cpp:745-756 with multigrid_driver.cpp:927-935"""
    norm = ordered_sum(act(dfc)*act(dfc))
    norm /= vol
    return math.sqrt(norm)


def load_source(u0, ng, fac):
    """LoadSource, multigrid.cpp:289-320: the ghost layer too.  u0: (nmb, nvar, ...)"""
    o = ng - 1
    s = u0[:, 0, o:u0.shape[2] - o, o:u0.shape[3] - o, o:u0.shape[4] - o]
    return s.copy() if fac == 1.0 else s*fac


def self_gravity(w0, phi, flx, u0, dx, bdt, ng, is_ideal):
    """SourceTerms::SelfGravity, srcterms.cpp:248-303 (in place on u0).  dx: (nmb, 3); flx: three arrays whose variable
    0 is the mass flux, the left face of cell i at index i (cell-shaped or face-shaped); phi: (nmb, 1, ...)"""
    n3, n2, n1 = w0.shape[2:]
    dims = [q for q, n in ((0, n1), (1, n2), (2, n3)) if n > 1]
    A = tuple(slice(ng, n - ng) if n > 1 else slice(0, 1) for n in (n3, n2, n1))

    def sh(axis, o):
        a = list(A)
        q = 2 - axis
        a[q] = slice(A[q].start + o, A[q].stop + o)
        return tuple(a)
    for m in range(w0.shape[0]):
        p = phi[m, 0]
        for d in dims:
            hdtodx = 0.5*bdt/dx[m, d]
            dpl = -(p[A] - p[sh(d, -1)])
            dpr = -(p[sh(d, 1)] - p[A])
            u0[m, 1 + d][A] += hdtodx*w0[m, 0][A]*(dpl + dpr)
            if is_ideal:
                f = flx[d][m, 0]
                u0[m, 4][A] += hdtodx*(f[A]*dpl + f[sh(d, 1)]*dpr)


# ---- the driver ------------------------------------------------------------------------------------------------------
def root_levels(nrb):
    """multigrid.cpp:100-108"""
    nlevel = 0
    for l in range(20):
        if nrb[0] % (1 << l) == 0 and nrb[1] % (1 << l) == 0 and nrb[2] % (1 << l) == 0:
            nlevel = l + 1
    return nlevel


def block_levels(nx):
    """multigrid.cpp:133-138"""
    for l in range(20):
        if (1 << l) == nx:
            return l + 1
    return 0


class Level:
    def __init__(self, nmb, n3, n2, n1):
        sh = (nmb, n3 + 2, n2 + 2, n1 + 2)
        self.u, self.src, self.dfc, self.uold = (np.zeros(sh) for _ in range(4))


class MG:
    """one Multigrid object: the MeshBlock levels (root = False) or the root grid"""

    def __init__(self, nmb, n, rdx, root):
        self.nmb, self.n, self.rdx, self.root = nmb, n, rdx, root
        self.nlevel = root_levels(n) if root else block_levels(n[0])
        self.lev = [Level(nmb, n[2] >> (self.nlevel - 1 - l), n[1] >> (self.nlevel - 1 - l),
                          n[0] >> (self.nlevel - 1 - l)) for l in range(self.nlevel)]
        self.current = self.nlevel - 1

    def dx(self, l=None):
        ll = self.nlevel - 1 - (self.current if l is None else l)
        return self.rdx*float(1 << ll)

    @property
    def c(self):
        return self.lev[self.current]


class MGSolver:
    """MGGravityDriver + MultigridDriver for a uniform periodic mesh on one rank"""

    def __init__(self, mesh_n, block_n, mesh_len, lloc, four_pi_G, ng=2, omega=1.15, threshold=-1.0, niteration=-1,
                 npresmooth=1, npostsmooth=1, full_multigrid=False, fmg_ncycle=1, subtract_average=True):
        self.nrb = tuple(mesh_n[q]//block_n for q in range(3))
        self.lloc = [tuple(l) for l in lloc]
        self.nmb = len(self.lloc)
        self.ng = ng
        self.tab = neighbor_table(self.lloc, self.nrb)
        self.four_pi_G, self.omega, self.eps, self.niter = four_pi_G, omega, threshold, niteration
        self.npre, self.npost, self.fmg, self.fmg_ncycle = npresmooth, npostsmooth, full_multigrid, fmg_ncycle
        self.fsub = subtract_average
        self.vol = mesh_len[0]*mesh_len[1]*mesh_len[2]
        block_len = mesh_len[0]/self.nrb[0]
        self.blocks = MG(self.nmb, (block_n,)*3, block_len/float(block_n), False)
        self.rootg = MG(1, self.nrb, mesh_len[0]/float(self.nrb[0]), True)
        self.coffset = 0
        self.nrootlevel, self.nmblevel = self.rootg.nlevel, self.blocks.nlevel
        self.ntotallevel = self.nrootlevel + self.nmblevel - 1
        self.phi = np.zeros((self.nmb, 1) + (block_n + 2*ng,)*3)
        self.norms = []
        self.ncycles = 0
        self.launch_log = None

    # -- pieces
    def _smooth(self, mg, color):
        smooth(mg.c.u, mg.c.src, mg.dx(), self.omega, color, self.coffset)

    def _bnd(self, mg):
        if mg.root:
            root_boundary(mg.c.u)
        else:
            exchange(mg.c.u, self.tab)

    def _restrict_pack(self, mg):
        """RestrictPack, multigrid.cpp:515-535"""
        defect(mg.c.u, mg.c.src, mg.c.dfc, mg.dx())
        co = mg.lev[mg.current - 1]
        restrict(mg.c.dfc, co.src)
        restrict(mg.c.u, co.u)
        mg.current -= 1

    def _prolongate_pack(self, mg):
        """ProlongateAndCorrectPack, multigrid.cpp:563-582"""
        mg.c.u -= mg.c.uold
        prolongate_correct(mg.c.u, mg.lev[mg.current + 1].u)
        mg.current += 1

    def _sub_average(self, mg, which):
        """MultigridDriver::SubtractAverage: the average of the current level leaves the finest level of the object"""
        a = getattr(mg.c, which)
        ave = average(a, mg.dx(), mg.rdx*float(mg.n[0]))
        getattr(mg.lev[-1], which)[...] -= ave

    def _to_root(self, initflag):
        b, r = self.blocks.lev[0], self.rootg.lev[-1]
        blocks_to_root(self.lloc, b.src, b.u, r.src, r.u, initflag)
        self.rootg.current = self.nrootlevel - 1

    def _from_root(self, fold):
        b, r = self.blocks.lev[0], self.rootg.lev[self.rootg.current]
        self.blocks.current = 0
        set_from_root(self.lloc, r.u, r.uold, b.u, b.uold, fold)

    # -- multigrid_driver.cpp
    def one_step_to_coarser(self, ns):
        if self.current_level >= self.nrootlevel:
            mg = self.blocks
            self._bnd(mg)
            if self.current_level < self.fmglevel:
                mg.c.uold[...] = mg.c.u
                fas_rhs(mg.c.u, mg.c.src, mg.dx())
            if ns > 0:
                self._smooth(mg, self.coffset)
                self._bnd(mg)
                self._smooth(mg, 1 - self.coffset)
                self._bnd(mg)
                if ns > 1:
                    self._smooth(mg, self.coffset)
                    self._bnd(mg)
                    self._smooth(mg, 1 - self.coffset)
                    self._bnd(mg)
            self._restrict_pack(mg)
            if self.current_level == self.nrootlevel:
                self._to_root(False)
        else:
            mg = self.rootg
            self._bnd(mg)
            if self.current_level < self.fmglevel:
                mg.c.uold[...] = mg.c.u
                fas_rhs(mg.c.u, mg.c.src, mg.dx())
            for _ in range(ns):
                self._smooth(mg, self.coffset)
                self._bnd(mg)
                self._smooth(mg, 1 - self.coffset)
                self._bnd(mg)
            self._restrict_pack(mg)
        self.current_level -= 1

    def one_step_to_finer(self, ns):
        if self.current_level == self.nrootlevel - 1:
            self._bnd(self.rootg)
            self._from_root(True)
        if self.current_level >= self.nrootlevel - 1:
            mg = self.blocks
            flag = 0
            if self.current_level == self.nrootlevel - 1:
                flag = 1
            if self.current_level == self.ntotallevel - 2:
                flag = 2
            if flag != 1:
                self._bnd(mg)
            self._prolongate_pack(mg)
            if ns > 0:
                self._bnd(mg)
                self._smooth(mg, self.coffset)
                self._bnd(mg)
                self._smooth(mg, 1 - self.coffset)
                if ns > 1:
                    self._bnd(mg)
                    self._smooth(mg, self.coffset)
                    self._bnd(mg)
                    self._smooth(mg, 1 - self.coffset)
            if flag == 2:
                self._bnd(mg)
            self.current_level += 1
        else:
            mg = self.rootg
            self._bnd(mg)
            self._prolongate_pack(mg)
            self.current_level += 1
            for _ in range(ns):
                self._bnd(mg)
                self._smooth(mg, self.coffset)
                self._bnd(mg)
                self._smooth(mg, 1 - self.coffset)

    def fmg_prolongate(self):
        flag = 0
        if self.current_level == self.nrootlevel - 1:
            self._bnd(self.rootg)
            self._from_root(False)
            flag = 1
        if self.current_level >= self.nrootlevel - 1:
            mg = self.blocks
            if flag != 1:
                self._bnd(mg)
        else:
            mg = self.rootg
            self._bnd(mg)
        fmg_prolongate(mg.c.u, mg.lev[mg.current + 1].u)
        mg.current += 1
        self.current_level += 1

    def solve_coarsest_grid(self):
        mg = self.rootg
        ni = max(self.nrb) >> (self.nrootlevel - 1)
        if self.fsub and ni == 1:
            self._bnd(mg)
            mg.c.uold[...] = mg.c.u
            mg.c.u[...] = 0.0
            return
        if self.fsub:
            self._sub_average(mg, "src")
            self._sub_average(mg, "u")
        self._bnd(mg)
        mg.c.uold[...] = mg.c.u
        fas_rhs(mg.c.u, mg.c.src, mg.dx())
        for _ in range(ni):
            self._smooth(mg, self.coffset)
            self._bnd(mg)
            self._smooth(mg, 1 - self.coffset)
            self._bnd(mg)
        if self.fsub:
            self._sub_average(mg, "u")

    def solve_vcycle(self):
        start = self.current_level
        self.coffset ^= 1
        while self.current_level > 0:
            self.one_step_to_coarser(self.npre)
        self.solve_coarsest_grid()
        while self.current_level < start:
            self.one_step_to_finer(self.npost)

    def calculate_defect_norm(self):
        mg = self.blocks
        defect(mg.c.u, mg.c.src, mg.c.dfc, mg.dx())
        return defect_norm(mg.c.dfc, self.vol)

    def solve_mg(self):
        if self.eps >= 0.0:
            d = self.calculate_defect_norm()
            self.norms.append(d)
            n = 0
            while d > self.eps:
                self.solve_vcycle()
                self.ncycles += 1
                old = d
                d = self.calculate_defect_norm()
                self.norms.append(d)
                if d/old > 0.9:
                    if self.eps == 0.0:
                        break
                n += 1
                if n >= 40:
                    break
        else:
            for _ in range(self.niter):
                self.solve_vcycle()
                self.ncycles += 1

    def solve_fmg(self):
        cycles = max(1, self.fmg_ncycle)
        # SolveFMGCoarser
        while self.current_level >= self.nrootlevel:
            mg = self.blocks
            restrict(mg.c.src, mg.lev[mg.current - 1].src)
            mg.current -= 1
            if self.current_level == self.nrootlevel:
                self._to_root(True)
            self.current_level -= 1
        self.current_level = self.nrootlevel - 1
        while self.current_level > 0:
            mg = self.rootg
            restrict(mg.c.src, mg.lev[mg.current - 1].src)
            mg.current -= 1
            self.current_level -= 1
        while self.current_level < self.ntotallevel - 1:
            self.fmglevel = self.current_level + 1
            self.fmg_prolongate()
            self.fmglevel = self.current_level
            for _ in range(cycles):
                self.solve_vcycle()
        self.fmglevel = self.ntotallevel - 1
        if self.fsub:
            self._sub_average(self.blocks, "u")
        self.solve_mg()

    def solve(self, u0):
        """MGGravityDriver::Solve, mg_gravity.cpp:177-245; u0: (nmb, nvar, n+2ng, ...) -> phi (nmb, 1, n+2ng, ...)"""
        mg = self.blocks
        self.norms, self.ncycles = [], 0
        mg.lev[-1].src[...] = load_source(u0, self.ng, -self.four_pi_G)
        mg.current = mg.nlevel - 1
        if not self.fmg:
            o = self.ng
            act(mg.c.u)[...] = self.phi[:, 0, o:-o, o:-o, o:-o]
        if self.fsub:
            self._sub_average(mg, "src")
        self.current_level = self.ntotallevel - 1
        self.fmglevel = self.current_level
        if self.fmg:
            self.solve_fmg()
        else:
            self.solve_mg()
        o = self.ng - 1
        self.phi[:, 0, o:self.phi.shape[2] - o, o:self.phi.shape[3] - o, o:self.phi.shape[4] - o] = mg.lev[-1].u
        return self.phi


def row_major_lloc(nrb):
    return [(i, j, k) for k in range(nrb[2]) for j in range(nrb[1]) for i in range(nrb[0])]
