"""TEST INFRASTRUCTURE: the refinement criteria, the regrid plan and the regrid of the evolved arrays restated in
numpy from the reference (src/mesh/refinement_criteria.cpp:177-338, src/mesh/mesh_refinement.cpp:427-1382,
src/mesh/prolongation.hpp:19-230), written the reference's way and independently of csrc/akmi_amr.hip: coarse
arrays are materialised (RestrictCC/FC of every old block, CopyForRefinementCC/FC into the child's coarse array),
the children of a derefined block are copied one after the other so that a later one overwrites the plane it
shares with an earlier one, and the operators are whole-array expressions in the reference's order of operations.

Arrays: u (nmb, nvar, N3, N2, N1); face fields b = [x1f (nmb, N3, N2, N1+1), x2f (nmb, N3, N2+1, N1),
x3f (nmb, N3+1, N2, N1)].  plan: (nmb_new, 3) ints {kind, old, octant} (include/akmi.h)."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
METHODS = {"min_max": 0, "slope": 1, "second_deriv": 2}


class Geom:
    """RegionIndcs of a MeshBlock with its coarse index space (src/mesh/mesh.cpp:285-330)"""

    def __init__(self, nx1, nx2, nx3, ng):
        self.nx = (nx3, nx2, nx1)                       # axis order of the arrays: (k, j, i)
        self.ng = ng
        self.on = (nx3 > 1, nx2 > 1, True)
        self.ndim = sum(self.on)
        self.nleaf = 1 << self.ndim
        self.N = tuple(n + 2*ng if a else 1 for n, a in zip(self.nx, self.on))
        self.s = tuple(ng if a else 0 for a in self.on)                      # ks, js, is
        self.e = tuple(s + n - 1 if a else 0 for s, n, a in zip(self.s, self.nx, self.on))
        self.cnx = tuple(n//2 if a else 1 for n, a in zip(self.nx, self.on))
        self.cN = tuple(c + 2*ng if a else 1 for c, a in zip(self.cnx, self.on))
        self.cs = self.s
        self.ce = tuple(s + c - 1 if a else 0 for s, c, a in zip(self.cs, self.cnx, self.on))

    def face_shape(self, d, coarse=False):
        """shape of component d (0: x1f, 1: x2f, 2: x3f)"""
        n = list(self.cN if coarse else self.N)
        n[2 - d] += 1
        return tuple(n)


# ---- criteria ------------------------------------------------------------------------------------------------------
def criterion_values(G, method, q):
    """(nmb, nx3, nx2, nx1): the quantity whose extremum over the active cells is tested; q is (nmb, N3, N2, N1)"""
    (ks, js, is_), (ke, je, ie) = G.s, G.e
    act = lambda dk, dj, di: q[:, ks + dk:ke + dk + 1, js + dj:je + dj + 1, is_ + di:ie + di + 1]
    q0 = act(0, 0, 0)
    if method == "min_max":
        return q0
    if method == "slope":
        d2 = (act(0, 0, 1) - act(0, 0, -1))**2
        if G.on[1]:
            d2 = d2 + (act(0, 1, 0) - act(0, -1, 0))**2
        if G.on[0]:
            d2 = d2 + (act(1, 0, 0) - act(-1, 0, 0))**2
        return 0.5*np.sqrt(d2)/q0
    if method == "second_deriv":
        d2q = act(0, 0, 1) - 2.0*q0 + act(0, 0, -1)
        if G.on[1]:
            d2q = d2q + (act(0, 1, 0) - 2.0*q0 + act(0, -1, 0))
        if G.on[0]:
            d2q = d2q + (act(1, 0, 0) - 2.0*q0 + act(-1, 0, 0))
        return np.abs(d2q)/q0
    raise ValueError(method)


def check(G, method, q, value_min, value_max, flags):
    """one criterion applied to flags (nmb ints) in place, refinement_criteria.cpp:192-231,261-282,312-333"""
    val = criterion_values(G, method, q).reshape(q.shape[0], -1)
    if value_max < FLT_MAX:
        t = val.max(axis=1)
        for m in range(len(flags)):
            if t[m] > value_max:
                flags[m] = 1
            if t[m] < value_max and flags[m] == 0:
                flags[m] = -1
    if method == "min_max" and value_min > -FLT_MAX:
        t = val.min(axis=1)                      # the Min reducer: the minimum, whatever the variable was set to
        for m in range(len(flags)):
            if t[m] < value_min:
                flags[m] = 1
            if t[m] > value_min and flags[m] == 0:
                flags[m] = -1
    return flags


# ---- plan ------------------------------------------------------------------------------------------------------------
def old_to_new(newtoold, old_nmb, nleaf):
    """mesh_refinement.cpp:450-469"""
    new_nmb = len(newtoold)
    o2n = [0]*old_nmb
    idx = 1
    for n in range(1, new_nmb):
        if newtoold[n] == newtoold[n - 1] + 1:
            o2n[idx] = n
            idx += 1
        elif newtoold[n] == newtoold[n - 1] + nleaf:
            for _ in range(nleaf - 1):
                o2n[idx] = n - 1
                idx += 1
            o2n[idx] = n
            idx += 1
    while idx < old_nmb:
        o2n[idx] = new_nmb - 1
        idx += 1
    return o2n


def level_flags(old_lloc, new_lloc, o2n, nleaf):
    """mesh_refinement.cpp:495-506: what happened to every old block, whoever flagged it"""
    out = []
    for oldm, l in enumerate(old_lloc):
        nl = new_lloc[o2n[oldm]]
        out.append(-nleaf if l[3] > nl[3] else (1 if l[3] < nl[3] else 0))
    return out


def plan(old_lloc, new_lloc, newtoold, nleaf):
    o2n = old_to_new(newtoold, len(old_lloc), nleaf)
    fl = level_flags(old_lloc, new_lloc, o2n, nleaf)
    rows = []
    for newm, oldm in enumerate(newtoold):
        if fl[oldm] > 0:
            l = new_lloc[newm]
            rows.append((1, oldm, (l[0] & 1) + 2*(l[1] & 1) + 4*(l[2] & 1)))
        elif fl[oldm] < -1:
            rows.append((-1, oldm, 0))
        else:
            rows.append((0, oldm, 0))
    return np.array(rows, dtype=np.int32).reshape(-1, 3)


# ---- operators ---------------------------------------------------------------------------------------------------------
def _sgn(x):
    return np.where(x < 0.0, -1.0, 1.0)


def _slope(c, box, ax):
    sh = lambda d: tuple(slice(s.start + d, s.stop + d) if a == ax else s for a, s in enumerate(box))
    q = c[(Ellipsis,) + tuple(box)]
    dl = q - c[(Ellipsis,) + sh(-1)]
    dr = c[(Ellipsis,) + sh(1)] - q
    return 0.125*(_sgn(dl) + _sgn(dr))*np.minimum(np.abs(dl), np.abs(dr))


def _prolong(G, c, f, own):
    """piecewise-linear prolongation of the coarse array c (..., k, j, i) into the fine array f: cells (own = None:
    ProlongCC) or the faces of component own shared with coarse faces (ProlongFCSharedX{1,2,3}Face).  The slopes are
    taken along every active direction but the face's own and applied in the order x1, x2, x3."""
    own_ax = None if own is None else 2 - own
    box = []
    for a in range(3):
        hi = G.ce[a] + 1 + (1 if a == own_ax else 0)
        box.append(slice(G.cs[a], hi))
    q = c[(Ellipsis,) + tuple(box)]
    slopes = {a: _slope(c, box, a) for a in range(3) if G.on[a] and a != own_ax}
    axes = sorted(slopes, reverse=True)                  # i (2), j (1), k (0)
    for bits in range(1 << len(axes)):
        val = q
        sign = {}
        for n, a in enumerate(axes):
            sign[a] = (bits >> n) & 1
        for a in (2, 1, 0):
            if a == own_ax:
                continue
            if a in slopes:
                val = val + slopes[a] if sign[a] else val - slopes[a]
            else:
                val = val - 0.0
        dst = []
        for a in range(3):
            n = box[a].stop - box[a].start
            if a in slopes:
                lo = G.s[a] + sign[a]
                dst.append(slice(lo, lo + 2*n, 2))
            elif a == own_ax and G.on[a]:
                dst.append(slice(G.s[a], G.s[a] + 2*n - 1, 2))
            else:
                dst.append(box[a])                       # collapsed direction: fj = j, fk = k
        f[(Ellipsis,) + tuple(dst)] = val


def prolong_internal(G, b1, b2, b3):
    """ProlongFCInternal over every coarse cell of one block's fine arrays (k, j, i); 1-D: the mean"""
    ks, js, is_ = G.s
    c3, c2, c1 = G.cnx

    def view(b, dk, dj, di):
        k = slice(ks + dk, ks + dk + 2*c3, 2) if G.on[0] else slice(0, 1)
        j = slice(js + dj, js + dj + 2*c2, 2) if G.on[1] else slice(0, 1)
        return b[k, j, is_ + di:is_ + di + 2*c1:2]
    B1 = lambda dk, dj, di: view(b1, dk, dj, di)
    B2 = lambda dk, dj, di: view(b2, dk, dj, di)
    B3 = lambda dk, dj, di: view(b3, dk, dj, di)
    if G.ndim == 1:
        B1(0, 0, 1)[...] = 0.5*(B1(0, 0, 0) + B1(0, 0, 2))
    elif G.ndim == 2:
        tmp1 = 0.25*(B2(0, 2, 1) - B2(0, 0, 1) - B2(0, 2, 0) + B2(0, 0, 0))
        tmp2 = 0.25*(B1(0, 0, 0) - B1(0, 0, 2) - B1(0, 1, 0) + B1(0, 1, 2))
        n10 = 0.5*(B1(0, 0, 0) + B1(0, 0, 2)) + tmp1
        n11 = 0.5*(B1(0, 1, 0) + B1(0, 1, 2)) + tmp1
        n20 = 0.5*(B2(0, 0, 0) + B2(0, 2, 0)) + tmp2
        n21 = 0.5*(B2(0, 0, 1) + B2(0, 2, 1)) + tmp2
        B1(0, 0, 1)[...] = n10
        B1(0, 1, 1)[...] = n11
        B2(0, 1, 0)[...] = n20
        B2(0, 1, 1)[...] = n21
    else:
        Uxx = Vyy = Wzz = Uxyz = Vxyz = Wxyz = 0.0
        for jj in (0, 1):
            jsgn = 2*jj - 1
            for ii in (0, 1):
                isgn = 2*ii - 1
                Uxx = Uxx + isgn*(jsgn*(B2(0, 2*jj, ii) + B2(1, 2*jj, ii)) + (B3(2, jj, ii) - B3(0, jj, ii)))
                Vyy = Vyy + jsgn*((B3(2, jj, ii) - B3(0, jj, ii)) + isgn*(B1(0, jj, 2*ii) + B1(1, jj, 2*ii)))
                Wzz = Wzz + (isgn*(B1(1, jj, 2*ii) - B1(0, jj, 2*ii)) + jsgn*(B2(1, 2*jj, ii) - B2(0, 2*jj, ii)))
                Uxyz = Uxyz + isgn*jsgn*(B1(1, jj, 2*ii) - B1(0, jj, 2*ii))
                Vxyz = Vxyz + isgn*jsgn*(B2(1, 2*jj, ii) - B2(0, 2*jj, ii))
                Wxyz = Wxyz + isgn*jsgn*(B3(2, jj, ii) - B3(0, jj, ii))
        Uxx, Vyy, Wzz = Uxx*0.125, Vyy*0.125, Wzz*0.125
        Uxyz, Vxyz, Wxyz = Uxyz*0.0625, Vxyz*0.0625, Wxyz*0.0625
        new = []
        for dk in (0, 1):
            for dj in (0, 1):
                sv = Vxyz if dk else -Vxyz
                sw = Wxyz if dj else -Wxyz
                new.append((B1(dk, dj, 1), 0.5*(B1(dk, dj, 0) + B1(dk, dj, 2)) + Uxx + sv + sw))
        for dk in (0, 1):
            for di in (0, 1):
                su = Uxyz if dk else -Uxyz
                sw = Wxyz if di else -Wxyz
                new.append((B2(dk, 1, di), 0.5*(B2(dk, 0, di) + B2(dk, 2, di)) + Vyy + su + sw))
        for dj in (0, 1):
            for di in (0, 1):
                su = Uxyz if dj else -Uxyz
                sv = Vxyz if di else -Vxyz
                new.append((B3(1, dj, di), 0.5*(B3(2, dj, di) + B3(0, dj, di)) + Wzz + su + sv))
        for dst, val in new:
            dst[...] = val


def restrict_cc(G, u):
    """RestrictCC of every block: (nmb, nvar, cN3, cN2, cN1), active coarse cells filled"""
    cu = np.zeros(u.shape[:2] + G.cN)
    (ks, js, is_), (ke, je, ie) = G.s, G.e
    f = u[:, :, ks:ke + 1, js:je + 1, is_:ie + 1]
    p = lambda dk, dj, di: f[:, :, (dk if G.on[0] else 0)::(2 if G.on[0] else 1),
                             (dj if G.on[1] else 0)::(2 if G.on[1] else 1), di::2]
    if G.ndim == 1:
        r = 0.5*(p(0, 0, 0) + p(0, 0, 1))
    elif G.ndim == 2:
        r = 0.25*(p(0, 0, 0) + p(0, 0, 1) + p(0, 1, 0) + p(0, 1, 1))
    else:
        r = 0.125*(p(0, 0, 0) + p(0, 0, 1) + p(0, 1, 0) + p(0, 1, 1) + p(1, 0, 0) + p(1, 0, 1) + p(1, 1, 0) + p(1, 1, 1))
    cu[:, :, G.cs[0]:G.ce[0] + 1, G.cs[1]:G.ce[1] + 1, G.cs[2]:G.ce[2] + 1] = r
    return cu


def restrict_fc(G, b):
    """RestrictFC of every block: coarse x1f, x2f, x3f with their active faces (upper plane included) filled"""
    nmb = b[0].shape[0]
    cb = [np.zeros((nmb,) + G.face_shape(d, coarse=True)) for d in range(3)]
    (ks, js, is_), (ke, je, ie) = G.s, G.e
    cks, cjs, cis = G.cs
    cke, cje, cie = G.ce
    K = slice(cks, cke + 1)
    J = slice(cjs, cje + 1)
    I = slice(cis, cie + 1)
    if G.ndim == 1:
        cb[0][:, 0, 0, cis:cie + 2] = b[0][:, 0, 0, is_:ie + 2:2]
        b2c = 0.5*(b[1][:, 0, 0, is_:ie + 1:2] + b[1][:, 0, 0, is_ + 1:ie + 2:2])
        cb[1][:, 0, 0, I] = b2c
        cb[1][:, 0, 1, I] = b2c
        b3c = 0.5*(b[2][:, 0, 0, is_:ie + 1:2] + b[2][:, 0, 0, is_ + 1:ie + 2:2])
        cb[2][:, 0, 0, I] = b3c
        cb[2][:, 1, 0, I] = b3c
    elif G.ndim == 2:
        f = b[0][:, 0]
        cb[0][:, 0, J, cis:cie + 2] = 0.5*(f[:, js:je + 1:2, is_:ie + 2:2] + f[:, js + 1:je + 2:2, is_:ie + 2:2])
        f = b[1][:, 0]
        cb[1][:, 0, cjs:cje + 2, I] = 0.5*(f[:, js:je + 2:2, is_:ie + 1:2] + f[:, js:je + 2:2, is_ + 1:ie + 2:2])
        f = b[2][:, 0]
        b3c = 0.25*(f[:, js:je + 1:2, is_:ie + 1:2] + f[:, js:je + 1:2, is_ + 1:ie + 2:2]
                    + f[:, js + 1:je + 2:2, is_:ie + 1:2] + f[:, js + 1:je + 2:2, is_ + 1:ie + 2:2])
        cb[2][:, 0, J, I] = b3c
        cb[2][:, 1, J, I] = b3c
    else:
        k0, k1 = slice(ks, ke + 1, 2), slice(ks + 1, ke + 2, 2)
        j0, j1 = slice(js, je + 1, 2), slice(js + 1, je + 2, 2)
        i0, i1 = slice(is_, ie + 1, 2), slice(is_ + 1, ie + 2, 2)
        kf, jf, if_ = slice(ks, ke + 2, 2), slice(js, je + 2, 2), slice(is_, ie + 2, 2)
        f = b[0]
        cb[0][:, K, J, cis:cie + 2] = 0.25*(f[:, k0, j0, if_] + f[:, k0, j1, if_] + f[:, k1, j0, if_] + f[:, k1, j1, if_])
        f = b[1]
        cb[1][:, K, cjs:cje + 2, I] = 0.25*(f[:, k0, jf, i0] + f[:, k0, jf, i1] + f[:, k1, jf, i0] + f[:, k1, jf, i1])
        f = b[2]
        cb[2][:, cks:cke + 2, J, I] = 0.25*(f[:, kf, j0, i0] + f[:, kf, j0, i1] + f[:, kf, j1, i0] + f[:, kf, j1, i1])
    return cb


def _octant(G, l):
    return [((l >> 2) & 1) if G.on[0] else 0, ((l >> 1) & 1) if G.on[1] else 0, l & 1]        # (ox3, ox2, ox1)


def regrid_cc(G, plan_rows, u_old, u_new):
    """u_new (sized for the new mesh) from u_old, in place; what no row writes keeps its value"""
    cu = restrict_cc(G, u_old)
    ng = G.ng
    for m, (kind, old, octant) in enumerate(np.asarray(plan_rows).tolist()):
        if kind == 0:                                                      # CopyCC
            u_new[m] = u_old[old]
        elif kind < 0:                                                     # DerefineCCSameRank
            for l in range(G.nleaf):
                ox = _octant(G, l)
                dst = tuple(slice(G.s[a] + ox[a]*G.cnx[a], G.s[a] + (ox[a] + 1)*G.cnx[a]) for a in range(3))
                src = tuple(slice(G.cs[a], G.ce[a] + 1) for a in range(3))
                u_new[(m, slice(None)) + dst] = cu[(old + l, slice(None)) + src]
        else:                                                              # CopyForRefinementCC + RefineCC
            ox = _octant(G, octant)
            ca = np.zeros((u_old.shape[1],) + G.cN)
            dst, src = [], []
            for a in range(3):
                lo, hi = (G.cs[a] - ng, G.ce[a] + ng) if G.on[a] else (G.cs[a], G.ce[a])
                dst.append(slice(lo, hi + 1))
                src.append(slice(lo + ox[a]*G.cnx[a], hi + 1 + ox[a]*G.cnx[a]))
            ca[(slice(None),) + tuple(dst)] = u_old[(old, slice(None)) + tuple(src)]
            _prolong(G, ca, u_new[m], None)
    return u_new


def regrid_fc(G, plan_rows, b_old, b_new):
    cb = restrict_fc(G, b_old)
    ng = G.ng
    for m, (kind, old, octant) in enumerate(np.asarray(plan_rows).tolist()):
        if kind == 0:                                                      # CopyFC
            for d in range(3):
                b_new[d][m] = b_old[d][old]
        elif kind < 0:                                                     # DerefineFCSameRank, child after child
            for l in range(G.nleaf):
                ox = _octant(G, l)
                for d in range(3):
                    own = 2 - d
                    dst = tuple(slice(G.s[a] + ox[a]*G.cnx[a], G.s[a] + (ox[a] + 1)*G.cnx[a] + (1 if a == own else 0))
                                for a in range(3))
                    src = tuple(slice(G.cs[a], G.ce[a] + 1 + (1 if a == own else 0)) for a in range(3))
                    b_new[d][(m,) + dst] = cb[d][(old + l,) + src]
        else:                                                              # CopyForRefinementFC + RefineFC
            ox = _octant(G, octant)
            for d in range(3):
                own = 2 - d
                c = np.zeros(G.face_shape(d, coarse=True))
                dst, src = [], []
                for a in range(3):
                    lo, hi = (G.cs[a] - ng, G.ce[a] + ng) if G.on[a] else (G.cs[a], G.ce[a])
                    hi += 1 if a == own else 0
                    dst.append(slice(lo, hi + 1))
                    src.append(slice(lo + ox[a]*G.cnx[a], hi + 1 + ox[a]*G.cnx[a]))
                c[tuple(dst)] = b_old[d][(old,) + tuple(src)]
                _prolong(G, c, b_new[d][m], d)
            prolong_internal(G, b_new[0][m], b_new[1][m], b_new[2][m])
    return b_new


def repair_fc(G, repair, b):
    """RepairAMRFC, mesh_refinement.cpp:1189-1220"""
    for m, r in enumerate(repair):
        if r != 0:
            prolong_internal(G, b[0][m], b[1][m], b[2][m])
    return b


def divb(G, b, dx):
    """face-centred div B of the active cells, (nmb, nx3, nx2, nx1); dx (nmb, 3) = dx1, dx2, dx3"""
    (ks, js, is_), (ke, je, ie) = G.s, G.e
    K, J, I = slice(ks, ke + 1), slice(js, je + 1), slice(is_, ie + 1)
    sh = (-1, 1, 1, 1)
    d = (b[0][:, K, J, is_ + 1:ie + 2] - b[0][:, K, J, I])/dx[:, 0].reshape(sh)
    if G.on[1]:
        d = d + (b[1][:, K, js + 1:je + 2, I] - b[1][:, K, J, I])/dx[:, 1].reshape(sh)
    if G.on[0]:
        d = d + (b[2][:, ks + 1:ke + 2, J, I] - b[2][:, K, J, I])/dx[:, 2].reshape(sh)
    return d
