"""numpy restatement of the derived output variables, written from the formulas (no GPU, no product code).

Every function takes the arrays of a pack -- w0 / bcc0 (nmb, nvar, N3, N2, N1), the face fields, dx (nmb, 3) -- and
returns the (nmb, N3, N2, N1) array the kernel has to produce: the variable over the reference's index range, zero
elsewhere.  numpy evaluates one correctly rounded IEEE operation per ufunc call and fuses nothing, so the bits depend
only on the ASSOCIATION, which each function states:

  wz, jz     ((a - b)/dx1 - (c - d)/dx2)*0.5                            -- the division precedes the 0.5
  w2, j2     0.25*((c1*c1 + c2*c2) + c3*c3), each c_n accumulated in the order x1, x2, x3 difference
             (c1 = 0.0 + d2 - d3,  c2 = -d1 + d3,  c3 = d1 - d2)
  curv       gradients (a - b)/(2.0*dx); B.gradB = (Bx*dx + By*dy) + Bz*dz; projector 1.0 - Bx*Bx/B2 (the product is
             divided, then subtracted); |.| = sqrt((c1*c1 + c2*c2) + c3*c3)/B2
  k_jxb      j as in j2 (without the 0.25), (j2*Bz - j3*By, j3*Bx - j1*Bz, j1*By - j2*Bx), sqrt(sum)/B2
  curv_perp  the same cross product divided by B2 component by component; unit vectors B_n/sqrt(B2) at the six
             neighbours; (b+ - b-)/(2.0*dx); (b1*d1 + b2*d2) + b3*d3; sqrt(((f1-c1)*(f1-c1) + (f2-c2)*(f2-c2)) + ...)
  bmag       sqrt((Bx*Bx + By*By) + Bz*Bz)
  divb       ((x1f[i+1] - x1f[i])/dx1 + (x2f[j+1] - x2f[j])/dx2) + (x3f[k+1] - x3f[k])/dx3 over EVERY cell of the array
  temperature  w0[4]/w0[0]

The two curvature variables on 1-D / 2-D meshes: a difference across a direction the mesh does not have is the
difference of the cell with itself (exactly +0), which is what the library defines there.
"""
import numpy as np


class Box:
    def __init__(self, nx1, nx2, nx3, ng):
        self.ng = ng
        self.multi_d, self.three_d = nx2 > 1, nx3 > 1
        self.N1 = nx1 + 2*ng
        self.N2 = nx2 + 2*ng if self.multi_d else 1
        self.N3 = nx3 + 2*ng if self.three_d else 1
        self.i = (ng, ng + nx1)
        self.j = (ng, ng + nx2) if self.multi_d else (0, 1)
        self.k = (ng, ng + nx3) if self.three_d else (0, 1)

    def act(self, q, dk=0, dj=0, di=0):
        """q[..., k + dk, j + dj, i + di] over the active cells"""
        return q[..., self.k[0] + dk:self.k[1] + dk, self.j[0] + dj:self.j[1] + dj, self.i[0] + di:self.i[1] + di]

    def full(self, nmb, active):
        out = np.zeros((nmb, self.N3, self.N2, self.N1))
        self.act(out)[...] = active
        return out


def _dx(dx, n):
    return dx[:, n][:, None, None, None]


def _curl_parts(bx, q, c1, c2, c3, dx):
    """(c1, c2, c3) of the curl of q[:, (c1, c2, c3)] without the centred difference's 1/2"""
    A = bx.act
    v1 = np.zeros_like(A(q[:, c1]))
    v2 = -(A(q[:, c3], di=1) - A(q[:, c3], di=-1))/_dx(dx, 0)
    v3 = (A(q[:, c2], di=1) - A(q[:, c2], di=-1))/_dx(dx, 0)
    if bx.multi_d:
        v1 = v1 + (A(q[:, c3], dj=1) - A(q[:, c3], dj=-1))/_dx(dx, 1)
        v3 = v3 - (A(q[:, c1], dj=1) - A(q[:, c1], dj=-1))/_dx(dx, 1)
    if bx.three_d:
        v1 = v1 - (A(q[:, c2], dk=1) - A(q[:, c2], dk=-1))/_dx(dx, 2)
        v2 = v2 + (A(q[:, c1], dk=1) - A(q[:, c1], dk=-1))/_dx(dx, 2)
    return v1, v2, v3


def _curl_z(bx, q, c1, c2, dx):
    A = bx.act
    v = (A(q[:, c2], di=1) - A(q[:, c2], di=-1))/_dx(dx, 0)
    if bx.multi_d:
        v = v - (A(q[:, c1], dj=1) - A(q[:, c1], dj=-1))/_dx(dx, 1)
    return v*0.5


def _sq3(a, b, c):
    return (a*a + b*b) + c*c


def wz(bx, w0, dx):
    return bx.full(len(w0), _curl_z(bx, w0, 1, 2, dx))


def w2(bx, w0, dx):
    return bx.full(len(w0), 0.25*_sq3(*_curl_parts(bx, w0, 1, 2, 3, dx)))


def jz(bx, bcc, dx):
    return bx.full(len(bcc), _curl_z(bx, bcc, 0, 1, dx))


def j2(bx, bcc, dx):
    return bx.full(len(bcc), 0.25*_sq3(*_curl_parts(bx, bcc, 0, 1, 2, dx)))


def bmag(bx, bcc, dx=None):
    A = bx.act
    return bx.full(len(bcc), np.sqrt(_sq3(A(bcc[:, 0]), A(bcc[:, 1]), A(bcc[:, 2]))))


def _steps(bx):
    """index steps of the neighbours in x2 and x3: zero in a direction the mesh does not have"""
    return (1 if bx.multi_d else 0), (1 if bx.three_d else 0)


def curv(bx, bcc, dx):
    A = bx.act
    sj, sk = _steps(bx)
    B = [A(bcc[:, n]) for n in range(3)]
    B2 = _sq3(*B)
    g = []
    for n in range(3):
        d1 = (A(bcc[:, n], di=1) - A(bcc[:, n], di=-1))/(2.0*_dx(dx, 0))
        d2 = (A(bcc[:, n], dj=sj) - A(bcc[:, n], dj=-sj))/(2.0*_dx(dx, 1))
        d3 = (A(bcc[:, n], dk=sk) - A(bcc[:, n], dk=-sk))/(2.0*_dx(dx, 2))
        g.append((B[0]*d1 + B[1]*d2) + B[2]*d3)
    c = []
    for n in range(3):          # column n of (I - bhat bhat), rows x, y, z
        col = [(1.0 if r == n else 0.0) - B[r]*B[n]/B2 for r in range(3)]
        c.append((g[0]*col[0] + g[1]*col[1]) + g[2]*col[2])
    return bx.full(len(bcc), np.sqrt(_sq3(*c))/B2)


def _jxb(bx, bcc, dx):
    A = bx.act
    j1, j2_, j3 = _curl_parts(bx, bcc, 0, 1, 2, dx)
    Bx, By, Bz = (A(bcc[:, n]) for n in range(3))
    return (j2_*Bz - j3*By, j3*Bx - j1*Bz, j1*By - j2_*Bx), _sq3(Bx, By, Bz), (Bx, By, Bz)


def k_jxb(bx, bcc, dx):
    f, B2, _ = _jxb(bx, bcc, dx)
    return bx.full(len(bcc), np.sqrt(_sq3(*f))/B2)


def curv_perp(bx, bcc, dx):
    A = bx.act
    sj, sk = _steps(bx)
    f, B2, B = _jxb(bx, bcc, dx)
    f = [x/B2 for x in f]
    h = [x/np.sqrt(B2) for x in B]

    def unit(**s):
        v = [A(bcc[:, n], **s) for n in range(3)]
        mag = np.sqrt(_sq3(*v))
        return [x/mag for x in v]
    ip, im = unit(di=1), unit(di=-1)
    jp, jm = unit(dj=sj), unit(dj=-sj)
    kp, km = unit(dk=sk), unit(dk=-sk)
    t = []
    for n in range(3):
        d1 = (ip[n] - im[n])/(2.0*_dx(dx, 0))
        d2 = (jp[n] - jm[n])/(2.0*_dx(dx, 1))
        d3 = (kp[n] - km[n])/(2.0*_dx(dx, 2))
        c = (h[0]*d1 + h[1]*d2) + h[2]*d3
        t.append((f[n] - c)*(f[n] - c))
    return bx.full(len(bcc), np.sqrt((t[0] + t[1]) + t[2]))


def divb(bx, b1, b2, b3, dx):
    d = (b1[..., 1:] - b1[..., :-1])/_dx(dx, 0)
    if bx.multi_d:
        d = d + (b2[:, :, 1:, :] - b2[:, :, :-1, :])/_dx(dx, 1)
    if bx.three_d:
        d = d + (b3[:, 1:] - b3[:, :-1])/_dx(dx, 2)
    return d


def temperature(bx, w0, dx=None):
    return bx.full(len(w0), bx.act(w0[:, 4])/bx.act(w0[:, 0]))


def restate(key, bx, w0=None, bcc=None, faces=None, dx=None):
    """the variable `key` of athenak_amd.capi.DERIVED"""
    if key in ("wz", "w2", "temperature"):
        return globals()[key](bx, w0, dx)
    if key == "divb":
        return divb(bx, *faces, dx)
    return globals()[key](bx, bcc, dx)
