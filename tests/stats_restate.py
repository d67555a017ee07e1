"""numpy restatement of the run-time statistics, written from the formulas (no GPU, no product code).

turb_terms: the eleven per-cell terms of the turbulence history columns over the active cells, (11, nmb, nx3, nx2, nx1).
numpy evaluates one correctly rounded IEEE operation per ufunc call and fuses nothing, so the bits depend only on the
ASSOCIATION, which is written out here with explicit parentheses:

  Bx By Bz   the bare components (no cell volume)
  B^2        ((Bx*Bx + By*By) + Bz*Bz)*vol,              vol = (dx1*dx2)*dx3
  B^4        (B2*B2)*vol
  dB^2       ((sum of nine squares, left to right)/dx1^2)*vol: the three face differences d*d, then 0.25 times each of
             dyBx dzBx dxBy dzBy dxBz dyBz as (0.25*d)*d, where d is the difference over two cells (a[+1] - a[-1])
  BdB^2      bdb1 = (Bx*d1f + (0.5*By)*dyBx) + (0.5*Bz)*dzBx,  bdb2 = (By*d2f + (0.5*Bz)*dzBy) + (0.5*Bx)*dxBy,
             bdb3 = (Bz*d3f + (0.5*Bx)*dxBz) + (0.5*By)*dyBz;  (((b1*b1 + b2*b2) + b3*b3)/dx1^2)*vol
  J          Jx = 0.5*dyBz - 0.5*dzBy, Jy = 0.5*dzBx - 0.5*dxBz, Jz = 0.5*dxBy - 0.5*dyBx
  |BxJ|^2    (((c1*c1 + c2*c2) + c3*c3)/dx1^2)*vol, c1 = By*Jz - Bz*Jy, c2 = Bz*Jx - Bx*Jz, c3 = Bx*Jy - By*Jx
  |B.J|^2    ((s*s)/dx1^2)*vol, s = (Bx*Jx + By*Jy) + Bz*Jz
  U^2        ((vx*vx + vy*vy) + vz*vz)*vol
  dU         ((sum of nine (0.25*d)*d, left to right: dxUx dyUy dzUz dyUx dzUx dxUy dzUy dxUz dyUz)/dx1^2)*vol

A cell-centred difference across a direction the mesh does not have is the difference of the cell with itself (+0).

pdf_bins / pdf_index: the edges and the bin of a value, in Python floats (math.log10 and pow are the C library's).
"""
import math

import numpy as np

LABELS = ["Bx", "By", "Bz", "B^2", "B^4", "dB^2", "BdB^2", "|BxJ|^2", "|B.J|^2", "U^2", "dU"]


def _dxm(dx, n):
    return dx[:, n][:, None, None, None]


def turb_terms(bx, w0, bcc, faces, dx):
    A = bx.act
    dj, dk = (1 if bx.multi_d else 0), (1 if bx.three_d else 0)

    def d_i(q):
        return A(q, di=1) - A(q, di=-1)

    def d_j(q):
        return A(q, dj=dj) - A(q, dj=-dj)

    def d_k(q):
        return A(q, dk=dk) - A(q, dk=-dk)

    dx1, dx2, dx3 = _dxm(dx, 0), _dxm(dx, 1), _dxm(dx, 2)
    vol = (dx1*dx2)*dx3
    dxsq = dx1*dx1
    Bx, By, Bz = A(bcc[:, 0]), A(bcc[:, 1]), A(bcc[:, 2])
    f1, f2, f3 = faces
    d1f = A(f1, di=1) - A(f1)
    d2f = A(f2, dj=1) - A(f2)            # the face arrays have extent nx + 1 in their own direction, also when nx = 1
    d3f = A(f3, dk=1) - A(f3)
    dyBx, dzBx = d_j(bcc[:, 0]), d_k(bcc[:, 0])
    dxBy, dzBy = d_i(bcc[:, 1]), d_k(bcc[:, 1])
    dxBz, dyBz = d_i(bcc[:, 2]), d_j(bcc[:, 2])
    t = [Bx.copy(), By.copy(), Bz.copy()]
    B2 = (Bx*Bx + By*By) + Bz*Bz
    t.append(B2*vol)
    t.append((B2*B2)*vol)
    s = d1f*d1f
    s = s + d2f*d2f
    s = s + d3f*d3f
    for d in (dyBx, dzBx, dxBy, dzBy, dxBz, dyBz):
        s = s + (0.25*d)*d
    t.append((s/dxsq)*vol)
    b1 = (Bx*d1f + (0.5*By)*dyBx) + (0.5*Bz)*dzBx
    b2 = (By*d2f + (0.5*Bz)*dzBy) + (0.5*Bx)*dxBy
    b3 = (Bz*d3f + (0.5*Bx)*dxBz) + (0.5*By)*dyBz
    t.append((((b1*b1 + b2*b2) + b3*b3)/dxsq)*vol)
    Jx = 0.5*dyBz - 0.5*dzBy
    Jy = 0.5*dzBx - 0.5*dxBz
    Jz = 0.5*dxBy - 0.5*dyBx
    c1, c2, c3 = By*Jz - Bz*Jy, Bz*Jx - Bx*Jz, Bx*Jy - By*Jx
    t.append((((c1*c1 + c2*c2) + c3*c3)/dxsq)*vol)
    sdot = (Bx*Jx + By*Jy) + Bz*Jz
    t.append(((sdot*sdot)/dxsq)*vol)
    vx, vy, vz = A(w0[:, 1]), A(w0[:, 2]), A(w0[:, 3])
    t.append(((vx*vx + vy*vy) + vz*vz)*vol)
    ds = [d_i(w0[:, 1]), d_j(w0[:, 2]), d_k(w0[:, 3]), d_j(w0[:, 1]), d_k(w0[:, 1]), d_i(w0[:, 2]), d_k(w0[:, 2]),
          d_i(w0[:, 3]), d_j(w0[:, 3])]
    s = (0.25*ds[0])*ds[0]
    for d in ds[1:]:
        s = s + (0.25*d)*d
    t.append((s/dxsq)*vol)
    return np.stack(t)


def reduction_depth(ncell, nmb_total, nt=256, per=4):
    """number of additions on the longest path from a term to its sum in the reduction the library builds: `per` strided
    adds per thread (from 0.0), log2(nt) tree levels over a tile of nt*per cells, ceil(ntile/nt) strided adds per thread
    (from 0.0) and log2(nt) tree levels over the tiles of a MeshBlock, one add per MeshBlock on the host (from 0.0)"""
    ntile = -(-ncell//(nt*per))
    lev = int(math.log2(nt))
    return per + lev + (-(-ntile//nt)) + lev + nmb_total


def sum_bound(terms, depth):
    """|computed sum - exact sum| <= depth * 2^-53 * sum|terms| (1 + O(2^-53)): every addition on a path of `depth`
    additions rounds a partial sum whose magnitude is at most sum|terms|.  The factor 1.0000001 stands for the higher
    orders."""
    return 1.0000001*depth*2.0**-53*math.fsum(np.abs(terms).ravel().tolist())


def pdf_bins(bin_min, bin_max, nbin, logscale):
    """edges[nbin+1] and the step"""
    if logscale:
        lo, hi = math.log10(bin_min), math.log10(bin_max)
        edges = [math.pow(10.0, lo + i*(hi - lo)/nbin) for i in range(nbin + 1)]
        return edges, (math.log10(bin_max) - math.log10(bin_min))/nbin
    step = (bin_max - bin_min)/nbin
    return [bin_min + i*step for i in range(nbin + 1)], (bin_max - bin_min)/nbin


def pdf_index(x, edges, step, logscale):
    """bin of one value in 0 .. nbin+1, None for a NaN"""
    nbin = len(edges) - 1
    x = float(x)
    if x != x:
        return None
    if x < edges[0]:
        return 0
    if x >= edges[nbin]:
        return nbin + 1
    if logscale:
        return int(math.log10(x/edges[0])/step) + 1
    return int((x - edges[0])/step) + 1


def pdf_near_edge(x, edges, step, logscale, tol=1e-9):
    """True when q = log10(x/edges[0])/step of an in-range value lies within tol of an integer (log bins only): the
    device's log10 is not the C library's, so such a cell may fall on either side"""
    x = float(x)
    if not logscale or x != x or x < edges[0] or x >= edges[-1]:
        return False
    q = math.log10(x/edges[0])/step
    return abs(q - round(q)) < tol


def histogram(vals, weights, edges, step, logscale, vals2=None, edges2=None, step2=None, logscale2=None, skip_near=False):
    """counts, per-bin lists of weights, number of NaN cells dropped, number of cells left out near a log edge"""
    nb = len(edges) + 1
    nb2 = len(edges2) + 1 if vals2 is not None else 1
    counts = np.zeros((nb2, nb), dtype=np.int64)
    wl = [[[] for _ in range(nb)] for _ in range(nb2)]
    nan = near = 0
    v2 = vals2 if vals2 is not None else [0.0]*len(vals)
    for x, y, w in zip(vals, v2, weights):
        xb = pdf_index(x, edges, step, logscale)
        yb = 0 if vals2 is None else pdf_index(y, edges2, step2, logscale2)
        if xb is None or yb is None:
            nan += 1
            continue
        if skip_near and (pdf_near_edge(x, edges, step, logscale) or
                          (vals2 is not None and pdf_near_edge(y, edges2, step2, logscale2))):
            near += 1
            continue
        counts[yb, xb] += 1
        wl[yb][xb].append(float(w))
    return counts, wl, nan, near
