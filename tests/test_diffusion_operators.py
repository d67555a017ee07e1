"""Diffusion operators (csrc/akmi_diffusion.hip) one entry point at a time: viscous, heat, resistive and
ambipolar fluxes, resistive and ambipolar EMFs, the two reduced time steps.

not gpu: pins of the oracle's operators that need no second implementation --
  * uniform velocity and uniform p/d: viscous and heat fluxes leave the flux arrays bit-unchanged,
  * a linear shear v_y = a*x: the x1-face flux of IVY (and, in 2-D/3-D, the x2-face flux of IVX) is -nu*d*a and the
    energy flux the matching 0.5*nud*(ay*fvy) term,
  * a face field that is the discrete gradient of a scalar is discretely curl-free: resistive EMFs and energy
    fluxes vanish to rounding,
  * the two time steps are the numpy minimum of the same expression, bit for bit.
gpu: every entry point against its oracle twin, bit for bit over whole arrays (ghosts and untouched entries included),
at MeshBlock shapes that put more than one 64-lane tile along x1, a last x1 tile of one lane, rows off the tile of 4
along x2, nk and nmb that are no powers of two, ng = 2, 3, 4 and a different, non-dyadic dx for every block and
direction.  Flux and EMF arrays are prefilled with random values: the kernels accumulate."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import akref

FLT_MAX = float(np.finfo(np.float32).max)
EPS = float(np.finfo(np.float64).eps)
GAMMA = 1.4

# (nx1, nx2, nx3, nmb, ng): the smallest shapes at which each edge of the 64x4 thread mapping exists
SHAPES = [
    (12, 8, 8, 2, 2),      # one partial tile along x1: the regime of the whole-run diffusion tests
    (63, 1, 1, 3, 2),      # 64 faces: exactly one full x1 tile, no second one
    (64, 1, 1, 3, 2),      # 65 faces: a second tile of one lane; the cells fill one tile exactly
    (65, 5, 1, 3, 2),      # cells spill by one lane; 5 (cells) and 6 (faces) rows over tiles of 4
    (64, 3, 3, 3, 2),      # nx2 + 1 = 4 rows exactly; nk = 3 and 4 with nmb = 3 in the blockIdx.z decode
    (130, 7, 2, 2, 4),     # three x1 tiles, ng = 4, nx3 = 2
    (66, 6, 5, 2, 3),      # ng = 3, every extent off the tile grid
]
_id = lambda s: "x".join(str(q) for q in s[:3]) + "-nmb%d-ng%d" % s[3:]
shapes = pytest.mark.parametrize("shape", SHAPES, ids=_id)
MULTI_TILE = [s for s in SHAPES if s[0] > 62]


class Case:
    """index space of a pack and rough random input for it; the arrays are shared between tests and read-only"""

    def __init__(self, shape, nvar=5, ideal=1, dx=None):
        nx1, nx2, nx3, nmb, ng = shape
        self.shape, self.nmb, self.ng, self.nvar, self.ideal = shape, nmb, ng, nvar, ideal
        if dx is None:                           # different for every block and direction, not dyadic
            dx = [(0.013 + 0.002*m, 0.017 + 0.003*m, 0.023 + 0.005*m) for m in range(nmb)]
        self.pk, self.dx = akref.make_pack(nmb, nx1, nx2, nx3, ng, np.array(dx), GAMMA, nvar=nvar)
        self.pk.is_ideal = int(ideal)
        self.ndim = 1 + (nx2 > 1) + (nx3 > 1)
        self.N1, self.N2, self.N3 = nx1 + 2*ng, (nx2 + 2*ng if nx2 > 1 else 1), (nx3 + 2*ng if nx3 > 1 else 1)
        self.is_, self.ie = ng, ng + nx1 - 1
        self.js, self.je = (ng, ng + nx2 - 1) if nx2 > 1 else (0, 0)
        self.ks, self.ke = (ng, ng + nx3 - 1) if nx3 > 1 else (0, 0)
        self.active = (slice(None), slice(self.ks, self.ke + 1), slice(self.js, self.je + 1),
                       slice(self.is_, self.ie + 1))

    def random_fields(self, seed):
        rng = np.random.default_rng(seed)
        N1, N2, N3, nmb = self.N1, self.N2, self.N3, self.nmb
        self.w = rng.normal(size=(nmb, self.nvar, N3, N2, N1))
        self.w[:, 0] = np.abs(self.w[:, 0]) + 0.1
        if self.ideal:
            self.w[:, 4] = np.abs(self.w[:, 4]) + 0.1
        self.bcc = rng.normal(size=(nmb, 3, N3, N2, N1))
        self.b = [rng.normal(size=(nmb, N3, N2, N1 + 1)), rng.normal(size=(nmb, N3, N2 + 1, N1)),
                  rng.normal(size=(nmb, N3 + 1, N2, N1))]
        for x in [self.w, self.bcc] + self.b:
            x.setflags(write=False)
        return self

    def fluxes(self, fs, seed, fill="random"):
        """flux arrays of the three directions: face-shaped (fs = 1, MHD) or cell-shaped (fs = 0, hydro)"""
        N1, N2, N3 = self.N1, self.N2, self.N3
        shp = [(self.nmb, self.nvar, N3, N2, N1 + fs), (self.nmb, self.nvar, N3, N2 + fs, N1),
               (self.nmb, self.nvar, N3 + fs, N2, N1)]
        return self._fill(shp, seed, fill)

    def emfs(self, seed, fill="random"):
        N1, N2, N3 = self.N1, self.N2, self.N3
        shp = [(self.nmb, N3 + 1, N2 + 1, N1), (self.nmb, N3 + 1, N2, N1 + 1), (self.nmb, N3, N2 + 1, N1 + 1)]
        return self._fill(shp, seed, fill)

    @staticmethod
    def _fill(shp, seed, fill):
        if fill == "zero":
            return [np.zeros(s) for s in shp]
        rng = np.random.default_rng(seed)
        return [rng.normal(size=s) for s in shp]


@functools.lru_cache(maxsize=None)
def _case(shape, nvar=5, ideal=1):
    return Case(shape, nvar, ideal).random_fields(101 + sum(shape) + nvar)


def _P(c):
    return C.byref(c.pk)


def _ptrs(arrays):
    return [akref.ptr(x) for x in arrays]


# ---- numpy restatements of the two time steps: the oracle's expression in its operand order ------------------------
def _cond_dt_cells(c, alpha, w):
    """SQR(dx)/alpha*d/gm1 per active cell and direction: (ndim, nmb, nk, nj, ni)"""
    d = w[:, 0][c.active]
    gm1 = GAMMA - 1.0
    return np.stack([(c.dx[:, q]*c.dx[:, q])[:, None, None, None]/alpha*d/gm1 for q in range(c.ndim)])


def _resist_dt_cells(c, eta_o, eta_a, bcc):
    """SQR(dx)/(eta_o + eta_a*B^2) per active cell and direction"""
    b0, b1, b2 = (bcc[:, q][c.active] for q in range(3))
    eta = eta_o + eta_a*(b0*b0 + b1*b1 + b2*b2)
    assert np.all(eta > 0.0), "the oracle's `if (eta > 0)` branch is not what these tests compare"
    return np.stack([(c.dx[:, q]*c.dx[:, q])[:, None, None, None]/eta for q in range(c.ndim)])


def _planted(c, what, decoy):
    """the winning cell at (ke, je, ie) of the last block: the last valid lane of the last partial tile; with `decoy`,
    ghost cells next to that lane along every refined direction carry a value that would win if it were read"""
    last = (c.ke, c.je, c.ie)
    ghosts = [(c.ke, c.je, c.ie + 1)]
    if c.ndim > 1:
        ghosts.append((c.ke, c.je + 1, c.ie))
    if c.ndim > 2:
        ghosts.append((c.ke + 1, c.je, c.ie))
    src = _case(c.shape)
    if what == "density":
        w = src.w.copy()
        w[-1, 0][last] = 0.01                     # every other density is >= 0.1; dx^2 of the blocks differs by < 2.1
        if decoy:
            for g in ghosts:
                w[-1, 0][g] = 1e-5
        return w, last, ghosts
    bcc = src.bcc.copy()
    bcc[(-1, slice(None)) + last] = (12.0, -13.0, 14.0)
    if decoy:
        for g in ghosts:
            bcc[(-1, slice(None)) + g] = (60.0, 60.0, 60.0)
    return bcc, last, ghosts


# ---- not gpu: pins of the oracle's operators ------------------------------------------------------------------------
PIN_SHAPES = [(64, 1, 1, 3, 2), (65, 5, 1, 3, 2), (66, 6, 5, 2, 3)]
pin_shapes = pytest.mark.parametrize("shape", PIN_SHAPES, ids=_id)


@pin_shapes
@pytest.mark.parametrize("fs", [0, 1])
def test_uniform_state_adds_no_viscous_or_heat_flux(shape, fs):
    """velocity differences and p/d differences are exactly zero, so every increment is nud*0 (alpha*densf*0) and
    `-=` of it is exact: the prefilled arrays come back bit for bit.  The density is rough; p = 2*d keeps p/d exact."""
    R = akref.lib()
    c = Case(shape)
    rng = np.random.default_rng(3)
    w = np.empty((c.nmb, 5, c.N3, c.N2, c.N1))
    w[:, 0] = np.abs(rng.normal(size=w[:, 0].shape)) + 0.1
    w[:, 1], w[:, 2], w[:, 3] = 0.3, -0.7, 1.1
    w[:, 4] = 2.0*w[:, 0]
    for call, coeff in ((R.akref_viscous_fluxes, 0.01), (R.akref_heat_fluxes, 0.02)):
        flx = c.fluxes(fs, 5)
        keep = [x.copy() for x in flx]
        assert call(_P(c), C.c_double(coeff), akref.ptr(w), *_ptrs(flx), fs) == 0
        for x, y in zip(flx, keep):
            assert np.array_equal(x, y)


@pin_shapes
def test_linear_shear_gives_the_newtonian_stress(shape):
    """v_y = a*x with constant d, v_x, v_z.  dx, a and the cell index are dyadic, so v_y, its differences and the
    quotients by dx are exact: fvy = a on x1 faces, fvx = a on x2 faces, every other gradient 0.  What is left of the
    oracle's path is nud = (0.5*nu)*(d + d) [1 rounding; the halving and the doubling are exact] and nud*a [1], into a
    zero-filled array; numpy's nu*d*a rounds twice: k = 4 roundings between the two, each <= 2^-53 < 1.2e-16.
    Energy flux: ay*fvy [1], (0.5*nud)*(..) [1] on top of nud [1], against 0.5*(nu*d)*(ay*a) [3]: k = 6."""
    R = akref.lib()
    nmb = shape[3]
    dx = [(2.0**-(6 + m), 2.0**-(5 + m), 2.0**-(4 + m)) for m in range(nmb)]
    c = Case(shape, dx=dx)
    nu, d, a = 0.01, 1.3, 0.75
    w = np.empty((c.nmb, 5, c.N3, c.N2, c.N1))
    w[:, 0], w[:, 1], w[:, 3], w[:, 4] = d, 0.25, -0.5, 1.0
    x = np.arange(c.N1)[None, :]*c.dx[:, 0][:, None]                   # (nmb, N1), exact
    w[:, 2] = (a*x)[:, None, None, :]
    flx = c.fluxes(1, 0, fill="zero")
    assert R.akref_viscous_fluxes(_P(c), C.c_double(nu), akref.ptr(w), *_ptrs(flx), 1) == 0
    k, j = slice(c.ks, c.ke + 1), slice(c.js, c.je + 1)
    f1 = flx[0][:, :, k, j, c.is_:c.ie + 2]                            # the x1 faces [is, ie+1] the operator covers
    want = -(nu*d*a)
    assert np.all(f1[:, 1] == 0.0) and np.all(f1[:, 3] == 0.0) and np.all(f1[:, 0] == 0.0)
    assert np.allclose(f1[:, 2], want, rtol=4e-16*4, atol=0.0)
    ay = (w[:, 2, :, :, c.is_ - 1:c.ie + 1] + w[:, 2, :, :, c.is_:c.ie + 2])[:, k, j]      # v_y(i-1) + v_y(i), exact
    assert np.allclose(f1[:, 4], -(0.5*(nu*d)*(ay*a)), rtol=4e-16*6, atol=0.0)
    if c.ndim > 1:
        f2 = flx[1][:, :, k, c.js:c.je + 2, c.is_:c.ie + 1]
        assert np.allclose(f2[:, 1], want, rtol=4e-16*4, atol=0.0)         # the stress tensor is symmetric
        assert np.all(f2[:, 2] == 0.0) and np.all(f2[:, 3] == 0.0)
        ax = 0.25 + 0.25
        assert np.allclose(f2[:, 4], -(0.5*(nu*d)*(ax*a)), rtol=4e-16*6, atol=0.0)
    else:
        assert np.all(flx[1] == 0.0)
    assert np.all(flx[2] == 0.0)                                        # nothing varies along x3
    # and nothing outside the faces of the active cells was touched
    m1 = np.ones_like(flx[0], dtype=bool)
    m1[:, :, k, j, c.is_:c.ie + 2] = False
    assert np.all(flx[0][m1] == 0.0)


@pin_shapes
def test_gradient_field_has_no_resistive_emf_or_flux(shape):
    """B = discrete gradient of a random scalar phi (one value per cell, which is what makes a *face* field a gradient:
    B1(i) = (phi(i) - phi(i-1))/dx1 ...).  Then each edge current is a difference of two terms that cancel exactly in
    real arithmetic, e.g. J3 = (B2(i) - B2(i-1))/dx1 - (B1(j) - B1(j-1))/dx2.  In floating point every B carries two
    roundings (subtraction, division): |dB| <= eps*max|B| with eps = 2^-52.  One term: two such B [2], the rounding of
    their difference, u*|diff| <= eps*max|B| [1], the division on a quotient <= 2*max|B|/dx [1] -- 4*eps*max|B|/dx;
    a current has two terms: |J| <= c*eps*max|B|/min(dx) with c = 8 subtractions-and-quotients counted this way.
    EMF increment = eta*J.  Energy flux = 0.25*eta*(four currents, each times a sum of two B): <= eta*16*eps*max|B|^2/dx,
    i.e. c = 16.  Arrays are zero-filled so that the increments are read directly."""
    R = akref.lib()
    c = Case(shape)
    rng = np.random.default_rng(17)
    N1, N2, N3 = c.N1, c.N2, c.N3
    phi = rng.normal(size=(c.nmb, N3 + 2, N2 + 2, N1 + 2))             # cell (k,j,i) is phi[k+1, j+1, i+1]
    if c.ndim < 3:
        phi[:] = phi[:, :1]                      # nothing varies along a collapsed direction: its B component is 0,
    if c.ndim < 2:                               # as the reduced curl of the 1-D / 2-D branches assumes
        phi[:] = phi[:, :, :1]
    dxm = lambda q: c.dx[:, q][:, None, None, None]
    b1 = (phi[:, 1:-1, 1:-1, 1:] - phi[:, 1:-1, 1:-1, :-1])/dxm(0)
    b2 = (phi[:, 1:-1, 1:, 1:-1] - phi[:, 1:-1, :-1, 1:-1])/dxm(1)
    b3 = (phi[:, 1:, 1:-1, 1:-1] - phi[:, :-1, 1:-1, 1:-1])/dxm(2)
    b = [np.ascontiguousarray(x) for x in (b1, b2, b3)]
    assert b[0].shape == (c.nmb, N3, N2, N1 + 1) and b[2].shape == (c.nmb, N3 + 1, N2, N1)
    eta = 0.003
    maxb = max(np.abs(x).max() for x in b)
    dxmin = c.dx[:, :c.ndim].min()
    e = c.emfs(0, fill="zero")
    assert R.akref_resistive_emfs(_P(c), C.c_double(eta), *_ptrs(b), *_ptrs(e)) == 0
    for x in e:
        assert np.abs(x).max() <= eta*8*EPS*maxb/dxmin
    flx = c.fluxes(1, 0, fill="zero")
    assert R.akref_resistive_fluxes(_P(c), C.c_double(eta), *_ptrs(b), *_ptrs(flx)) == 0
    for x in flx:
        assert np.abs(x).max() <= eta*16*EPS*maxb*maxb/dxmin
    # the same operators on rough (not curl-free) data of the same size give increments of order eta*max|B|/dx
    rough = _case(shape)
    e = c.emfs(0, fill="zero")
    R.akref_resistive_emfs(_P(c), C.c_double(eta), *_ptrs(rough.b), *_ptrs(e))
    assert max(np.abs(x).max() for x in e) > eta*1.0/c.dx.max()


@shapes
def test_conduction_newdt_is_the_numpy_minimum(shape):
    R = akref.lib()
    c = _case(shape)
    alpha = 0.02
    dt = np.zeros(1)
    assert R.akref_conduction_newdt(_P(c), C.c_double(alpha), akref.ptr(c.w), akref.ptr(dt)) == 0
    assert dt[0] == min(FLT_MAX, _cond_dt_cells(c, alpha, c.w).min())


@shapes
@pytest.mark.parametrize("eta", [(0.003, 0.02), (0.0, 0.02)], ids=["ohm+ad", "ad"])
def test_resistive_newdt_is_the_numpy_minimum(shape, eta):
    R = akref.lib()
    c = _case(shape)
    dt = np.zeros(1)
    assert R.akref_resistive_newdt(_P(c), C.c_double(eta[0]), C.c_double(eta[1]), akref.ptr(c.bcc),
                                   akref.ptr(dt)) == 0
    assert dt[0] == min(FLT_MAX, _resist_dt_cells(c, eta[0], eta[1], c.bcc).min())


@pytest.mark.parametrize("shape", MULTI_TILE, ids=_id)
def test_planted_extrema_win_in_the_oracle(shape):
    """the inputs of the planted gpu cases do what they are meant to: the minimum comes from (ke, je, ie) of the last
    block, and the decoys in the ghost zone would undercut it if they were read"""
    R = akref.lib()
    c = _case(shape)
    alpha, eta = 0.02, (0.003, 0.02)
    for decoy in (False, True):
        w, last, ghosts = _planted(c, "density", decoy)
        dt = np.zeros(1)
        R.akref_conduction_newdt(_P(c), C.c_double(alpha), akref.ptr(w), akref.ptr(dt))
        cells = _cond_dt_cells(c, alpha, w)
        assert dt[0] == cells[:, -1, -1, -1, -1].min() and (cells == dt[0]).sum() == 1
        bcc, last, ghosts = _planted(c, "field", decoy)
        R.akref_resistive_newdt(_P(c), C.c_double(eta[0]), C.c_double(eta[1]), akref.ptr(bcc), akref.ptr(dt))
        cells = _resist_dt_cells(c, eta[0], eta[1], bcc)
        assert dt[0] == cells[:, -1, -1, -1, -1].min() and (cells == dt[0]).sum() == 1
    assert w[-1, 0][ghosts[0]] < w[-1, 0][last] and np.abs(bcc[-1, 0][ghosts[0]]) > np.abs(bcc[-1, 0][last])


# ---- gpu: the HIP kernels against the oracle, bit for bit -----------------------------------------------------------
class Dev:
    """device copies for one case: the pack with a device dx, tensors kept alive until the comparison"""

    def __init__(self, c):
        import torch
        from athenak_amd import capi
        self.torch, self.capi, self.L = torch, capi, capi.lib()
        self.dxd = self.t(c.dx)
        self.pk = capi.Pack.from_buffer_copy(bytes(c.pk))
        self.pk.dx = self.dxd.data_ptr()
        self.P = C.byref(self.pk)

    def t(self, x):
        return self.torch.from_numpy(np.array(x)).cuda()           # a copy: the shared inputs are read-only

    def ptrs(self, tensors):
        return [self.capi._p(x) for x in tensors]


def _same(host, dev):
    for q, (x, y) in enumerate(zip(host, dev)):
        assert np.array_equal(x, y.cpu().numpy()), "array %d differs" % q


@pytest.mark.gpu
@shapes
@pytest.mark.parametrize("ideal", [1, 0], ids=["ideal", "isothermal"])
@pytest.mark.parametrize("fs", [0, 1], ids=["cell-shaped", "face-shaped"])
def test_hip_viscous_fluxes_match_the_oracle(shape, fs, ideal):
    R = akref.lib()
    c = _case(shape, 5, 1) if ideal else _case(shape, 4, 0)
    D = Dev(c)
    nu = C.c_double(0.01)
    flx = c.fluxes(fs, 23)
    wd, fd = D.t(c.w), [D.t(x) for x in flx]
    assert R.akref_viscous_fluxes(_P(c), nu, akref.ptr(c.w), *_ptrs(flx), fs) == 0
    D.capi.check(D.L.akmi_viscous_fluxes(D.P, nu, D.capi._p(wd), *D.ptrs(fd), fs, None), "viscous_fluxes")
    _same(flx, fd)


@pytest.mark.gpu
@shapes
@pytest.mark.parametrize("fs", [0, 1], ids=["cell-shaped", "face-shaped"])
def test_hip_heat_fluxes_match_the_oracle(shape, fs):
    R = akref.lib()
    c = _case(shape)
    D = Dev(c)
    alpha = C.c_double(0.02)
    flx = c.fluxes(fs, 29)
    wd, fd = D.t(c.w), [D.t(x) for x in flx]
    assert R.akref_heat_fluxes(_P(c), alpha, akref.ptr(c.w), *_ptrs(flx), fs) == 0
    D.capi.check(D.L.akmi_heat_fluxes(D.P, alpha, D.capi._p(wd), *D.ptrs(fd), fs, None), "heat_fluxes")
    _same(flx, fd)


@pytest.mark.gpu
@shapes
def test_hip_resistive_emfs_match_the_oracle(shape):
    R = akref.lib()
    c = _case(shape)
    D = Dev(c)
    eta = C.c_double(0.003)
    e = c.emfs(31)
    bd, ed = [D.t(x) for x in c.b], [D.t(x) for x in e]
    assert R.akref_resistive_emfs(_P(c), eta, *_ptrs(c.b), *_ptrs(e)) == 0
    D.capi.check(D.L.akmi_resistive_emfs(D.P, eta, *D.ptrs(bd), *D.ptrs(ed), None), "resistive_emfs")
    _same(e, ed)


@pytest.mark.gpu
@shapes
def test_hip_resistive_fluxes_match_the_oracle(shape):
    R = akref.lib()
    c = _case(shape)
    D = Dev(c)
    eta = C.c_double(0.003)
    flx = c.fluxes(1, 37)
    bd, fd = [D.t(x) for x in c.b], [D.t(x) for x in flx]
    assert R.akref_resistive_fluxes(_P(c), eta, *_ptrs(c.b), *_ptrs(flx)) == 0
    D.capi.check(D.L.akmi_resistive_fluxes(D.P, eta, *D.ptrs(bd), *D.ptrs(fd), None), "resistive_fluxes")
    _same(flx, fd)


@pytest.mark.gpu
@shapes
def test_hip_ambipolar_emfs_match_the_oracle(shape):
    R = akref.lib()
    c = _case(shape)
    D = Dev(c)
    eta = C.c_double(0.02)
    e = c.emfs(41)
    ccd, bd, ed = D.t(c.bcc), [D.t(x) for x in c.b], [D.t(x) for x in e]
    assert R.akref_ambipolar_emfs(_P(c), eta, akref.ptr(c.bcc), *_ptrs(c.b), *_ptrs(e)) == 0
    D.capi.check(D.L.akmi_ambipolar_emfs(D.P, eta, D.capi._p(ccd), *D.ptrs(bd), *D.ptrs(ed), None),
                 "ambipolar_emfs")
    _same(e, ed)


@pytest.mark.gpu
@shapes
def test_hip_ambipolar_fluxes_match_the_oracle(shape):
    R = akref.lib()
    c = _case(shape)
    D = Dev(c)
    eta = C.c_double(0.02)
    flx = c.fluxes(1, 43)
    ccd, bd, fd = D.t(c.bcc), [D.t(x) for x in c.b], [D.t(x) for x in flx]
    assert R.akref_ambipolar_fluxes(_P(c), eta, akref.ptr(c.bcc), *_ptrs(c.b), *_ptrs(flx)) == 0
    D.capi.check(D.L.akmi_ambipolar_fluxes(D.P, eta, D.capi._p(ccd), *D.ptrs(bd), *D.ptrs(fd), None),
                 "ambipolar_fluxes")
    _same(flx, fd)


def _newdt_inputs(c, what, case):
    """random: the shared rough input; last-lane / decoy: the planted cases (multi-tile shapes)"""
    if case == "random":
        return (c.w if what == "density" else c.bcc), None
    arr, last, ghosts = _planted(c, what, case == "decoy")
    return arr, last


NEWDT_CASES = [(s, "random") for s in SHAPES] + [(s, k) for s in MULTI_TILE for k in ("last-lane", "decoy")]
newdt_cases = pytest.mark.parametrize("shape,case", NEWDT_CASES, ids=["%s-%s" % (_id(s), k) for s, k in NEWDT_CASES])


@pytest.mark.gpu
@newdt_cases
def test_hip_conduction_newdt_matches_the_oracle(shape, case):
    R = akref.lib()
    c = _case(shape)
    D = Dev(c)
    alpha = C.c_double(0.02)
    w, last = _newdt_inputs(c, "density", case)
    dt, dtd = np.zeros(1), D.torch.zeros(1, dtype=D.torch.float64, device="cuda")
    wd = D.t(w)
    assert R.akref_conduction_newdt(_P(c), alpha, akref.ptr(w), akref.ptr(dt)) == 0
    D.capi.check(D.L.akmi_conduction_newdt(D.P, alpha, D.capi._p(wd), D.capi._p(dtd), None), "conduction_newdt")
    got = dtd.cpu().numpy()
    print("conduction_newdt oracle %r hip %r" % (dt[0], got[0]))
    assert np.array_equal(dt, got)
    if last is not None:                # ... and it is the planted cell's value, not a ghost cell's
        assert got[0] == _cond_dt_cells(c, alpha.value, w)[:, -1, -1, -1, -1].min()


@pytest.mark.gpu
@newdt_cases
@pytest.mark.parametrize("eta", [(0.003, 0.02), (0.0, 0.02)], ids=["ohm+ad", "ad"])
def test_hip_resistive_newdt_matches_the_oracle(shape, case, eta):
    R = akref.lib()
    c = _case(shape)
    D = Dev(c)
    eo, ea = C.c_double(eta[0]), C.c_double(eta[1])
    bcc, last = _newdt_inputs(c, "field", case)
    dt, dtd = np.zeros(1), D.torch.zeros(1, dtype=D.torch.float64, device="cuda")
    ccd = D.t(bcc)
    assert R.akref_resistive_newdt(_P(c), eo, ea, akref.ptr(bcc), akref.ptr(dt)) == 0
    D.capi.check(D.L.akmi_resistive_newdt(D.P, eo, ea, D.capi._p(ccd), D.capi._p(dtd), None), "resistive_newdt")
    got = dtd.cpu().numpy()
    print("resistive_newdt oracle %r hip %r" % (dt[0], got[0]))
    assert np.array_equal(dt, got)
    if last is not None:
        assert got[0] == _resist_dt_cells(c, eta[0], eta[1], bcc)[:, -1, -1, -1, -1].min()
