"""Inputs, reference sequence and coverage census of the single-stage parity tests (test_stage_cases_host.py on the
CPU, test_gpu_stage_operators.py on the GPU): ONE call of a stage entry of the library on a state built to reach the
branches whole runs of the decks do not, against the oracle's task chain, bit for bit.

Nothing here touches the GPU or the HIP library: the states, the expected arrays and the census come from numpy and
the CPU oracle (oracle/akref) alone.
"""
import ctypes as C
import functools

import numpy as np

from oracle import akref

SENTINEL = -7.0                         # content of every array (or part of one) a stage must not write
DFLOOR, PFLOOR = 1.0e-3, 1.0e-4
FLT_MAX = float(np.finfo(np.float32).max)
BETA_RK4 = 1.193743905974738            # first-stage weight of RK4: beta*dt is a product that rounds
# (gam0, gam1, beta, dt): the first stage of a cycle and the last stage of RK2.  beta*dt ~ 1e-3: with 1e-4 and 1e-6 the
# floors bind in fewer than five cells for hydro DC / Roe and for every last stage (0.5*(u0 + u1) of two positive states
# leaves the flux term alone to reach a floor); at 1e-3 every reference is still finite.
WEIGHTS = {"first": (0.0, 1.0, BETA_RK4, 1.0e-3), "last": (0.5, 0.5, 0.5, 2.0e-3)}
# the density of one cell is 2**TINY_EXP times its neighbour's: the star density of the faces of that cell lies outside
# the exponent window of the short sqrt / reciprocal forms of the fused sweeps, so the wave that holds it falls back.
# The oracle's stage stays finite at -701 for every scheme of CASES but MHD HLLE, whose flux overflows once 1/d**2 does:
# there the exponent is raised to -510, the smallest power of two at which its reference is finite (-511 is not).  That
# cell is then inside the window -- HLLE has no star density -- and only keeps its jump of 150 decades.
# test_stage_cases_host.py asserts the finiteness of every reference.
TINY_EXP = -701
TINY_EXP_OF = {("mhd", "hlle"): -510}


def wild_prims(shape5, rng, mhd):
    """primitive states with jumps of many decades between neighbouring cells: exercises the
    supersonic branches, the HLLE/HLLC pressure estimates, Roe's negative-density fallback and
    the L/R floors of ppmx/wenoz/teno"""
    w = np.empty(shape5)
    w[:, 0] = 10.0**rng.uniform(-4, 2, size=w[:, 0].shape)
    w[:, 1:4] = rng.normal(0, 3.0, size=w[:, 1:4].shape)
    w[:, 4] = 10.0**rng.uniform(-5, 2, size=w[:, 4].shape)
    return w


# ---- shapes ---------------------------------------------------------------------------------------------------------
# name -> (nmb, (nx1, nx2, nx3)); nghost comes with the scheme.  Why these: test_gpu_stage_operators.py
SHAPES = {
    "3x12x10x9": (3, (12, 10, 9)),
    "11x9x10": (1, (11, 9, 10)),
    "132x6x5": (1, (132, 6, 5)),
    "6x40x5": (1, (6, 40, 5)),
    "8x12x10": (8, (12, 10, 1)),        # 2-D and 1-D: as many blocks as give ~1 000 active cells, so that the floors
    "64x16": (64, (16, 1, 1)),          # bind in at least five of them and every fan selection has faces
}


def _pow2_near(n):
    return 2.0**-int(round(np.log2(n)))


def block_dx(nmb, nx):
    """cell sizes per block: block 0 powers of two in every direction (12, 10, 9 cells: 1/16, 1/8, 1/8 -- the product
    branch of the kernels), block 1 1/n (the division branch), block 2 a power of two in x1 and x3 but not in x2; further
    blocks repeat the three.  A pack of one block takes 1/n."""
    dx = np.ones((nmb, 3))
    for m in range(nmb):
        kind = 1 if nmb == 1 else m % 3
        for q in range(3):
            if nx[q] == 1:
                continue
            p2 = kind == 0 or (kind == 2 and q != 1)
            dx[m, q] = _pow2_near(nx[q]) if p2 else 1.0/nx[q]
    return dx


def make_pack(nmb, nx, ng, mhd, nscalars=0, ideal=True, dfloor=DFLOOR, pfloor=PFLOOR, sigma_max=None, sfloor=0.0):
    """(akmi_pack for host arrays, its dx array) of a pack of nmb blocks of nx cells.  sfloor = None: the default entropy
    floor FLT_MIN, which the packs of the calm states keep (it binds in none of their cells: test_stage_cases_host.py).
    For the states with the tiny cell the entropy floor is off (0): it binds only where the cell 2**TINY_EXP below its neighbour has blown a density up to ~1e137,
    and its value gm1/pow(d, gm1) then compares the device's pow with the host's -- they differ by an ulp there
    (d = 2.24e137: w0[4] 1.456914187975195e+191 against 1.4569141879751954e+191), which no kernel of a stage can mend."""
    nvar = (5 if ideal else 4) + nscalars
    pk, dx = akref.make_pack(nmb, nx[0], nx[1], nx[2], ng, block_dx(nmb, nx), 5.0/3.0 if mhd else 1.4, nvar=nvar,
                             dfloor=dfloor, pfloor=pfloor, sfloor=sfloor, sigma_max=sigma_max)
    if not ideal:
        pk.is_ideal = 0
        pk.iso_cs = 0.7
    return pk, dx


class Geo:
    """index ranges of a pack, as make_geo of the library and mkG of the oracle have them"""

    def __init__(self, pk):
        self.nmb, self.nvar, self.ng = pk.nmb, pk.nvar, pk.ng
        self.nx = (pk.nx1, pk.nx2, pk.nx3)
        self.multi_d, self.three_d = pk.nx2 > 1, pk.nx3 > 1
        self.N1 = pk.nx1 + 2*pk.ng
        self.N2 = pk.nx2 + 2*pk.ng if self.multi_d else 1
        self.N3 = pk.nx3 + 2*pk.ng if self.three_d else 1
        self.is_, self.ie = pk.ng, pk.ng + pk.nx1 - 1
        self.js, self.je = (pk.ng, pk.ng + pk.nx2 - 1) if self.multi_d else (0, 0)
        self.ks, self.ke = (pk.ng, pk.ng + pk.nx3 - 1) if self.three_d else (0, 0)
        self.dims = 1 + int(self.multi_d) + int(self.three_d)

    def cells(self):
        return (self.nmb, self.nvar, self.N3, self.N2, self.N1)

    def faces(self, q):
        return (self.nmb, self.N3 + (q == 2), self.N2 + (q == 1), self.N1 + (q == 0))

    def active(self):
        """slices (k, j, i) of the active cells"""
        return (slice(self.ks, self.ke + 1), slice(self.js, self.je + 1), slice(self.is_, self.ie + 1))

    def ct_faces(self, q):
        """slices (k, j, i) of the faces of direction q that CT owns (mhd_ct.cpp:45-77)"""
        return (slice(self.ks, self.ke + 1 + (q == 2)), slice(self.js, self.je + 1 + (q == 1)),
                slice(self.is_, self.ie + 1 + (q == 0)))


BNAMES = ("x1f", "x2f", "x3f")


def _c2p(pack, mhd, u, b, w, bcc, rng_):
    """the oracle's ConsToPrim of the cells il..iu, jl..ju, kl..ku (rng_) of every block of the arrays, in place"""
    R, P = akref.lib(), akref.ptr
    if mhd:
        R.akref_mhd_c2p(C.byref(pack), P(u), *[P(x) for x in b], P(w), P(bcc), *rng_, None)
    else:
        R.akref_hydro_c2p(C.byref(pack), P(u), P(w), *rng_, None)


def _one_state(g, mhd, ideal, nscal, seed, pk, tiny_exp):
    """conserved state, face field and their conversion of one wild state (see wild_state)"""
    rng = np.random.default_rng(seed)
    nmb, N3, N2, N1 = g.nmb, g.N3, g.N2, g.N1
    w = np.empty((nmb, 5 + nscal, N3, N2, N1))
    w[:, :5] = wild_prims((nmb, 5, N3, N2, N1), rng, mhd)
    if nscal:
        w[:, 5:] = rng.uniform(0.0, 1.0, size=w[:, 5:].shape)
    b = None
    if mhd:
        b = [rng.normal(0, 2.0, size=g.faces(q)) for q in range(3)]
        b[0][:, :, :, ::3] = 0.0            # Bx = 0 faces (degenerate HLLD branches)
    # ---- the named cells: special s sits in block s % nmb, row js + s, plane ks + s (where those directions exist), at
    # i = is + 1, so that the cells i-1 .. i+2 it may touch are active ones
    def where(s):
        return (s % nmb, g.ks + (s % g.nx[2] if g.three_d else 0), g.js + (s % g.nx[1] if g.multi_d else 0), g.is_ + 1)
    _, k, j, i = where(0)                   # -0.0 momenta, in two identical neighbouring cells of every block: the contact
    for m in range(nmb):                    # speed of the x1 face between them is 0 and its mass flux +-0.0 or an ulp's worth
        w[m, 1:4, k, j, i] = -0.0           # (the sign byte of a zero)
        w[m, :, k, j, i + 1] = w[m, :, k, j, i]
        if mhd:
            b[0][m, k, j, i + 2] = b[0][m, k, j, i]
            b[1][m, k, j:j + 2, i + 1] = b[1][m, k, j:j + 2, i]
            b[2][m, k:k + 2, j, i + 1] = b[2][m, k:k + 2, j, i]
    if mhd:
        m, k, j, i = where(1)               # By exactly 0 in four cells in a row: 0 on both sides of x1 face i+1, slopes too
        b[1][m, k, j:j + 2, i - 1:i + 3] = 0.0
    m, k, j, i = where(2)                   # two neighbouring cells with identical states (zero slopes)
    w[m, :, k, j, i + 1] = w[m, :, k, j, i]
    if mhd:
        b[0][m, k, j, i + 2] = b[0][m, k, j, i]
        b[1][m, k, j:j + 2, i + 1] = b[1][m, k, j:j + 2, i]
        b[2][m, k:k + 2, j, i + 1] = b[2][m, k:k + 2, j, i]
    mt, kt, jt, it = where(3)               # one cell whose density is 2**TINY_EXP times its neighbour's
    w[mt, 0, kt, jt, it - 1] = 0.75         # (a neighbour below 1: the tiny density lies below 2**TINY_EXP whatever the seed)
    w[mt, 0, kt, jt, it] = 2.0**tiny_exp*w[mt, 0, kt, jt, it - 1]
    # ---- conserved variables, the cell-centred field the face average
    nv = g.nvar
    u = np.empty((nmb, nv, N3, N2, N1))
    u[:, 0] = w[:, 0]
    u[:, 1:4] = w[:, 0:1]*w[:, 1:4]
    e_m = 0.0
    if mhd:
        bcc = np.stack([0.5*(b[0][..., :-1] + b[0][..., 1:]), 0.5*(b[1][:, :, :-1] + b[1][:, :, 1:]),
                        0.5*(b[2][:, :-1] + b[2][:, 1:])], axis=1)
        e_m = 0.5*(bcc**2).sum(axis=1)
    if ideal:
        u[:, 4] = w[:, 4] + 0.5*w[:, 0]*(w[:, 1:4]**2).sum(axis=1) + e_m
    if nscal:
        u[:, nv - nscal:] = w[:, 0:1]*w[:, 5:]
    tiny = u[mt, :, kt, jt, it].copy()
    # ---- ConsToPrim of ALL cells with the floors of the pack: what a driver holds after Initialize
    wout = np.zeros_like(u)
    bcc0 = np.zeros((nmb, 3, N3, N2, N1)) if mhd else None
    _c2p(pk, mhd, u, b, wout, bcc0, (0, N1 - 1, 0, N2 - 1, 0, N3 - 1))
    if tiny_exp != 0:
        # the tiny cell alone is converted without a density floor (with one it would not be tiny); its pressure floor
        # holds.  Block mt is converted as a pack of one block, so that no other cell is converted twice.
        pk0, dx0 = make_pack(1, g.nx, g.ng, mhd, nscal, ideal, dfloor=0.0, sigma_max=float("inf"))
        u[mt, :, kt, jt, it] = tiny
        one = slice(mt, mt + 1)
        _c2p(pk0, mhd, u[one], [x[one] for x in b] if mhd else None, wout[one], bcc0[one] if mhd else None,
             (it, it, jt, jt, kt, kt))
    return u, wout, bcc0, b


@functools.lru_cache(maxsize=None)
def wild_state(nmb, nx, ng, mhd, nscalars, seed, ideal=True, tiny_exp=None):
    """A consistent stage input on the host: dict of u0, w0 (, bcc0, b0x1f, b0x2f, b0x3f) and u1 (, b1x1f, b1x2f, b1x3f),
    read-only arrays shared between the tests.

    Recipe of wild_prims (density 10**U(-4, 2), velocities N(0, 3), internal energy 10**U(-5, 2)), face fields N(0, 2)
    with every third x1 face column exactly 0, passive scalars U(0, 1); conserved state from it with the cell-centred
    field the face average; then ALL cells, ghost zones included, through the oracle's ConsToPrim with dfloor = 1e-3,
    pfloor = 1e-4.  So w0 == ConsToPrim(u0) in every cell with the floors applied: what a driver holds after Initialize
    and the precondition of the u0 / face forms of the MHD sweeps.  A handful of named cells (block s % nmb, row js + s,
    plane ks + s, i = is + 1 for s = 0..3) carry: -0.0 momenta; a transverse field component exactly 0 on both sides of
    an x1 face; two neighbouring cells with identical states; one cell whose density is 2**TINY_EXP times its
    neighbour's -- that cell alone is converted without a density floor, which would otherwise lift it (tiny_exp = 0: no
    such cell, the calm state).
    u1 and b1 are a second, independent wild state (seed + 1000): the second register of copy_u1 = 0 and 3."""
    tiny_exp = TINY_EXP if tiny_exp is None else tiny_exp
    pk, dx = make_pack(nmb, nx, ng, mhd, nscalars, ideal, sfloor=None if tiny_exp == 0 else 0.0)
    g = Geo(pk)
    st = {}
    for reg, sd in (("0", seed), ("1", seed + 1000)):
        u, w, bcc, b = _one_state(g, mhd, ideal, nscalars, sd, pk, tiny_exp)
        st["u" + reg] = u
        if reg == "0":
            st["w0"] = w
            if mhd:
                st["bcc0"] = bcc
        if mhd:
            for q in range(3):
                st["b" + reg + BNAMES[q]] = b[q]
    for v in st.values():
        v.setflags(write=False)
    return st


def stage_inputs(state, copy_u1, mhd):
    """fresh arrays a stage entry is called with: the second register is the sentinel for copy_u1 = 1 and 2"""
    a = {k: v.copy() for k, v in state.items()}
    if copy_u1 in (1, 2):
        a["u1"][...] = SENTINEL
        if mhd:
            for q in BNAMES:
                a["b1" + q][...] = SENTINEL
    return a


def oracle_stage(pack, scheme, weights, copy_u1, state, c2p, do_newdt):
    """The reference's sequence of one stage with the oracle's task entries (src/mhd/mhd_tasks.cpp:48-75,
    src/hydro/hydro_tasks.cpp:55-71): fluxes; CopyCons when copy_u1 is 1 or 2; RKUpdate; CornerE; CT; and, for the
    entries that convert (c2p), ConsToPrim of the ACTIVE cells plus NewTimeStep when do_newdt.

    pack: (akmi_pack, dx) for host arrays; scheme: (reconstruction, solver) names; weights: (gam0, gam1, beta_dt) with
    beta_dt the ROUNDED product beta*dt; state: wild_state(...).  Returns the expected content of every array of
    stage_inputs(state, copy_u1) after the call -- those the stage writes and those it must leave alone -- plus
    `counters` (from zero) and `dt3`, and `mass_flux_signs`: per direction the number of faces with a positive and with
    a negative mass flux.
      copy_u1 = 0: u0 / b0 updated in place from both registers.
      copy_u1 = 1: the same with u1 = u0, b1 = b0; the second register receives the old state in the cells and faces
                   the update owns (rk_store) and keeps the sentinel elsewhere.
      copy_u1 = 2: u0 / b0 untouched; the new state in the cells / faces the update owns of u1 / b1, sentinel elsewhere.
                   (1-D: CT does not own the x1 faces, Bx is constant; the register receives b0's all the same.)
      copy_u1 = 3: u0 untouched, the new cells in u1's buffer around u1's old ghost zones; b0 in place, b1 untouched."""
    pk, dx = pack
    g = Geo(pk)
    mhd = "bcc0" in state
    R = akref.lib()
    gam0, gam1, beta_dt = weights
    rc, rs = akref.RECON[scheme[0]], akref.RSOLVER[scheme[1]]
    P = akref.ptr
    a = stage_inputs(state, copy_u1, mhd)
    out = {k: v.copy() for k, v in a.items()}
    u0 = a["u0"].copy()
    u1 = u0.copy() if copy_u1 in (1, 2) else a["u1"].copy()                 # CopyCons
    nv = g.nvar
    flx = [np.zeros((g.nmb, nv) + g.faces(q)[1:]) for q in range(3)]
    if mhd:
        b0 = [a["b0" + q].copy() for q in BNAMES]
        b1 = [x.copy() for x in b0] if copy_u1 in (1, 2) else [a["b1" + q].copy() for q in BNAMES]
        efc = [np.zeros((g.nmb, g.N3, g.N2, g.N1)) for _ in range(6)]
        e = [np.zeros((g.nmb, g.N3 + 1, g.N2 + 1, g.N1)), np.zeros((g.nmb, g.N3 + 1, g.N2, g.N1 + 1)),
             np.zeros((g.nmb, g.N3, g.N2 + 1, g.N1 + 1))]
        assert R.akref_mhd_fluxes(C.byref(pk), rc, rs, P(a["w0"]), P(a["bcc0"]), *[P(x) for x in b0],
                                  *[P(x) for x in flx], *[P(x) for x in efc]) == 0
    else:
        assert R.akref_hydro_fluxes(C.byref(pk), rc, rs, P(a["w0"]), *[P(x) for x in flx], 1) == 0
    w = (C.c_double(gam0), C.c_double(gam1), C.c_double(beta_dt))
    R.akref_rk_update(C.byref(pk), *w, P(u0), P(u1), *[P(x) for x in flx], 1)
    if mhd:
        R.akref_mhd_corner_e(C.byref(pk), P(a["w0"]), P(a["bcc0"]), *[P(x) for x in efc], *[P(x) for x in flx],
                             *[P(x) for x in e])
        R.akref_mhd_ct(C.byref(pk), *w, *[P(x) for x in e], *[P(x) for x in b0], *[P(x) for x in b1])
    counters = np.zeros(3, dtype=np.int32)
    dt3 = np.full(3, FLT_MAX)
    if c2p:
        ck, cj, ci = g.active()
        rng_ = (ci.start, ci.stop - 1, cj.start, cj.stop - 1, ck.start, ck.stop - 1)
        w0n = a["w0"].copy()
        if mhd:
            bccn = a["bcc0"].copy()
            R.akref_mhd_c2p(C.byref(pk), P(u0), *[P(x) for x in b0], P(w0n), P(bccn), *rng_, P(counters))
            if do_newdt:
                R.akref_mhd_newdt(C.byref(pk), P(w0n), P(bccn), P(dt3))
            out["bcc0"] = bccn
        else:
            R.akref_hydro_c2p(C.byref(pk), P(u0), P(w0n), *rng_, P(counters))
            if do_newdt:
                R.akref_hydro_newdt(C.byref(pk), P(w0n), P(dt3))
        out["w0"] = w0n

    def place(new, old_first, second_in, sl):
        """(first register, second register) after the call; sl: the part of the arrays the update owns"""
        idx = (slice(None),)*(new.ndim - 3) + sl
        second = second_in.copy()
        if copy_u1 == 0:
            return new, second
        if copy_u1 == 1:
            second[idx] = old_first[idx]
            return new, second
        second[idx] = new[idx]
        return old_first.copy(), second
    out["u0"], out["u1"] = place(u0, a["u0"], a["u1"], g.active())
    if mhd:
        for q in range(3):
            n0, n1 = "b0" + BNAMES[q], "b1" + BNAMES[q]
            if copy_u1 == 3:                # the face field of a last stage out of place is updated in place
                out[n0], out[n1] = b0[q], a[n1].copy()
            else:
                out[n0], out[n1] = place(b0[q], a[n0], a[n1], g.ct_faces(q))
    out["counters"], out["dt3"] = counters, dt3
    ndir = g.dims
    out["mass_flux_signs"] = [(int((flx[q][:, 0] > 0).sum()), int((flx[q][:, 0] < 0).sum())) for q in range(ndir)]
    # faces of the x1 range a stage solves whose mass flux is exactly +-0.0 (elsewhere the arrays were never written)
    fk, fj, fi = _face_range(g, 0, mhd)
    out["mass_flux_zeros"] = int((flx[0][:, 0, fk, fj, fi] == 0.0).sum())
    return out


# ---- which Riemann fan the faces take ----------------------------------------------------------------------------
def _plm_lr(q, axis):
    """PLM left / right states (plm.hpp:20-37) at the faces between cells 1 .. n-2 along `axis`: face f of the result
    lies between cells f+1 and f+2 of q"""
    q = np.moveaxis(q, axis, -1)
    dql, dqr = q[..., 1:-1] - q[..., :-2], q[..., 2:] - q[..., 1:-1]
    dq2 = dql*dqr
    with np.errstate(all="ignore"):
        dqm = np.where(dq2 <= 0.0, 0.0, dq2/(dql + dqr))
    ql, qr = q[..., 1:-1] + dqm, q[..., 1:-1] - dqm             # at the high / low face of cells 1 .. n-2
    return np.moveaxis(ql[..., :-1], -1, axis), np.moveaxis(qr[..., 1:], -1, axis)


def _face_range(g, q, mhd):
    """(k, j, i) slices of the faces of direction q a stage solves: the active ones, CT-extended by one cell in the
    transverse directions that exist for MHD (hydro_fluxes.cpp:95-104, mhd_fluxes.cpp:117-248)"""
    lo = [g.ks, g.js, g.is_]
    hi = [g.ke, g.je, g.ie]
    ext = [g.three_d, g.multi_d, True]
    sl = []
    for ax in range(3):
        d = 2 - ax                          # direction of this axis
        if d == q:
            sl.append(slice(lo[ax], hi[ax] + 2))
        else:
            x = 1 if (mhd and ext[ax]) else 0
            sl.append(slice(lo[ax] - x, hi[ax] + 1 + x))
    return tuple(sl)


HLLD_SELECTIONS = ("sL >= 0", "sR <= 0", "sAL >= 0", "sM >= 0", "sAR > 0", "else")
HLLC_REGIONS = ("supersonic", "sM >= 0", "sM < 0")


def hlld_census(pack, state):
    """Per direction, how many faces of the ranges a stage solves take each selection of the Riemann fan, from PLM left /
    right states of state['w0'] (, 'bcc0' and the face field) -- a numpy restatement of the wave speeds of
    hlld_mhd.hpp:66-151 (the six selections HLLD_SELECTIONS) or, for hydro, of hllc_hyd.hpp:40-75 (HLLC_REGIONS).
    Returns a list of integer arrays, one per direction of the pack.  Ideal gas only."""
    pk, dx = pack
    g = Geo(pk)
    mhd = "bcc0" in state
    gamma = pk.gamma
    w = state["w0"]
    out = []
    for q in range(g.dims):
        axis = 4 - q                        # axis of direction q in (m, n, k, j, i)
        L, Rr = _plm_lr(w[:, :5], axis)
        # face index f of L / R is the face on the low side of cell f + 2 - 1 ... shift so that face f == array index f
        sl = _face_range(g, q, mhd)

        def at(x, nax=5):
            idx = [slice(None)]*(nax - 3) + list(sl)
            ax = nax - 1 - q
            idx[ax] = slice(sl[2 - q].start - 2, sl[2 - q].stop - 2)      # face f lies at index f - 2 of L / R
            return x[tuple(idx)]
        L, Rr = at(L), at(Rr)
        ivx = 1 + q
        dl, dr, vl, vr = L[:, 0], Rr[:, 0], L[:, ivx], Rr[:, ivx]
        pl, pr = (gamma - 1.0)*L[:, 4], (gamma - 1.0)*Rr[:, 4]
        with np.errstate(all="ignore"):
            if not mhd:
                al, ar = np.sqrt(gamma*pl/dl), np.sqrt(gamma*pr/dr)
                alpha = (gamma + 1.0)/(2.0*gamma)
                qc = 0.25*(dl + dr)*(al + ar)
                pm = 0.5*(pl + pr + (vl - vr)*qc)
                qe = np.where(pm <= pl, 1.0, np.sqrt(1.0 + alpha*(pm/pl - 1.0)))
                qf = np.where(pm <= pr, 1.0, np.sqrt(1.0 + alpha*(pm/pr - 1.0)))
                sl_, sr_ = vl - al*qe, vr + ar*qf
                ml, mr = dl*(vl - sl_), -(dr*(vr - sr_))
                am = ((pl + (vl - sl_)*dl*vl) - (pr + (vr - sr_)*dr*vr))/(ml + mr)
                sup = (sl_ >= 0.0) | (sr_ <= 0.0)
                out.append(np.array([sup.sum(), (~sup & (am >= 0.0)).sum(), (~sup & ~(am >= 0.0)).sum()]))
                continue
            bq = state["bcc0"]
            bl3, br3 = _plm_lr(bq, axis)
            bl3, br3 = at(bl3), at(br3)
            iby, ibz = (q + 1) % 3, (q + 2) % 3
            bx = state["b0" + BNAMES[q]][(slice(None),) + sl]
            byl, bzl, byr, bzr = bl3[:, iby], bl3[:, ibz], br3[:, iby], br3[:, ibz]

            def fast(d, p, by, bz):
                asq, ct2 = gamma*p, by*by + bz*bz
                qsq, tmp = bx*bx + ct2 + asq, bx*bx + ct2 - asq
                return np.sqrt(0.5*(qsq + np.sqrt(tmp*tmp + 4.0*asq*ct2))/d)
            cfl, cfr = fast(dl, pl, byl, bzl), fast(dr, pr, byr, bzr)
            s0, s4 = np.minimum(vl - cfl, vr - cfr), np.maximum(vl + cfl, vr + cfr)
            bxsq = bx*bx
            ptl, ptr = pl + 0.5*(bxsq + byl**2 + bzl**2), pr + 0.5*(bxsq + byr**2 + bzr**2)
            sdl, sdr = s0 - vl, s4 - vr
            s2 = (sdr*dr*vr - sdl*dl*vl + (ptl - ptr))/(sdr*dr - sdl*dl)
            dls, drs = dl*sdl/(s0 - s2), dr*sdr/(s4 - s2)
            s1, s3 = s2 - np.abs(bx)/np.sqrt(dls), s2 + np.abs(bx)/np.sqrt(drs)
            sel = np.select([s0 >= 0.0, s4 <= 0.0, s1 >= 0.0, s2 >= 0.0, s3 > 0.0], [0, 1, 2, 3, 4], default=5)
        out.append(np.bincount(sel.ravel(), minlength=6))
    return out


# ---- the cases of test_gpu_stage_operators.py ------------------------------------------------------------------
X3_U0, X12_U0, BCC_FACES = 0x100, 0x200, 0x400          # AKMI_COPY_* of include/akmi.h
FLAG_SETS = {"": 0, "x3": X3_U0, "x3+x12": X3_U0 | X12_U0, "x3+x12+bf": X3_U0 | X12_U0 | BCC_FACES}
FORMS_OF = {0: 0, X3_U0: 1, X3_U0 | X12_U0: 3, X3_U0 | X12_U0 | BCC_FACES: 11}      # AKMI_FORM_* the call must report
SEED = 20240


class Case:
    """one stage call: fluid 'mhd' | 'hydro', scheme (recon, solver), nghost, EOS, passive scalars, shape (key of SHAPES),
    copy_u1 (0..3), form flags (key of FLAG_SETS), weights (key of WEIGHTS), entry 'update' | 'fused' | 'fused_dt' | 'w'"""

    def __init__(self, fluid, recon, rs, shape, copy, weights, entry, flags="", ng=2, ideal=True, nscal=0, calm=False):
        self.fluid, self.recon, self.rs, self.shape, self.copy, self.weights = fluid, recon, rs, shape, copy, weights
        self.entry, self.flags, self.ng, self.ideal, self.nscal, self.calm = entry, flags, ng, ideal, nscal, calm
        # calm: the same state without the tiny cell (exponent 0: the density of its neighbour).  Round that cell a stage
        # leaves densities of 1e137 and speeds that overflow, which then fix the CFL minima alone (0 = dx/inf for MHD); the
        # calm companions are the cases whose dt3 is set by ordinary cells, and they keep the default entropy floor.
        self.tiny_exp = 0 if calm else TINY_EXP_OF.get((fluid, rs), TINY_EXP)

    mhd = property(lambda s: s.fluid == "mhd")

    def id(self):
        eos = "" if self.ideal else "-iso"
        sc = "-%dscal" % self.nscal if self.nscal else ""
        fl = "+" + self.flags if self.flags else ""
        return "%s-%s-%s%s%s-%s-copy%d%s-%s-%s%s" % (self.fluid, self.recon, self.rs, eos, sc, self.shape, self.copy, fl,
                                                      self.weights, self.entry, "-calm" if self.calm else "")

    def state_key(self):
        nmb, nx = SHAPES[self.shape]
        return (nmb, nx, self.ng, self.mhd, self.nscal, SEED, self.ideal, self.tiny_exp)

    def oracle_key(self):
        """what the expected arrays depend on (not the form flags, not how dt reaches the kernels)"""
        return self.state_key() + (self.recon, self.rs, self.weights, self.copy, self.entry != "update")


def _cases():
    A, B, C_, D = "3x12x10x9", "11x9x10", "132x6x5", "6x40x5"
    wof = {0: "last", 1: "first", 2: "first", 3: "last"}        # a first stage copies, a last one reads both registers
    cs = []
    # ---- MHD PLM + HLLD, ideal gas: k_sweep12s + x3 march + k_corner_ct<MFB>
    for copy in (0, 1, 2, 3):
        for wt in ("first", "last"):
            for entry in ("update", "fused") if wt == wof[copy] else ("fused",):
                cs.append(Case("mhd", "plm", "hlld", A, copy, wt, entry))
    for copy in (2, 3):
        for fl in ("x3", "x3+x12", "x3+x12+bf"):
            for entry in ("update", "fused"):
                cs.append(Case("mhd", "plm", "hlld", A, copy, wof[copy], entry, flags=fl))
    cs.append(Case("mhd", "plm", "hlld", A, 1, "first", "fused_dt"))
    for copy in (0, 1, 2, 3):
        for entry in ("update", "fused"):
            cs.append(Case("mhd", "plm", "hlld", B, copy, wof[copy], entry))
    for copy in (2, 3):
        cs.append(Case("mhd", "plm", "hlld", B, copy, wof[copy], "fused", flags="x3+x12+bf"))
    for shp in (C_, D):
        for copy in (1, 2, 3):
            cs.append(Case("mhd", "plm", "hlld", shp, copy, wof[copy], "fused"))
        cs.append(Case("mhd", "plm", "hlld", shp, 3, "last", "fused", flags="x3+x12+bf"))
        cs.append(Case("mhd", "plm", "hlld", shp, 1, "first", "update"))
    # ---- MHD generic sequence: x1 sweep + x2 / x3 marches
    for kw in (dict(recon="ppm4", rs="hlld", ng=3), dict(recon="plm", rs="hlle"), dict(recon="plm", rs="llf"),
               dict(recon="plm", rs="hlld", ideal=False), dict(recon="plm", rs="hlld", nscal=2)):
        for copy, entry in ((1, "update"), (1, "fused"), (2, "fused"), (0, "fused")):
            cs.append(Case("mhd", shape=A, copy=copy, weights=wof[copy], entry=entry, **kw))
    # ---- hydro one-kernel stage: k_hydro_stage3d2 (with ConsToPrim inside: entry 'w')
    for recon in ("dc", "plm"):
        for rs in ("llf", "hlle", "hllc", "roe"):
            for copy, entry in ((1, "update"), (1, "fused"), (2, "fused"), (0, "fused"), (1, "w")):
                cs.append(Case("hydro", recon, rs, A, copy, wof[copy], entry))
    for copy in (2, 0):
        cs.append(Case("hydro", "plm", "hllc", A, copy, wof[copy], "w"))
    # (isothermal: HLLE and LLF keep the density positive, its floor does not bind; Roe on first-stage weights does)
    for copy, entry in ((1, "update"), (1, "fused"), (2, "fused"), (0, "fused")):
        cs.append(Case("hydro", "plm", "roe", A, copy, "first", entry, ideal=False))
    for copy, entry in ((1, "update"), (1, "fused"), (2, "fused"), (0, "fused")):
        cs.append(Case("hydro", "plm", "hllc", A, copy, wof[copy], entry, nscal=2))
    for shp in (B, C_, D):
        for copy, entry in ((1, "update"), (1, "fused"), (2, "fused"), (1, "w")):
            cs.append(Case("hydro", "plm", "hllc", shp, copy, wof[copy], entry))
    # ---- hydro generic sequence
    for recon, rs in (("ppm4", "hllc"), ("wenoz", "hlle")):
        for copy, entry in ((1, "update"), (1, "fused"), (2, "fused"), (0, "fused")):
            cs.append(Case("hydro", recon, rs, A, copy, wof[copy], entry, ng=3))
    # ---- 2-D and 1-D
    for shp in ("8x12x10", "64x16"):
        for fluid, rs in (("mhd", "hlld"), ("hydro", "hllc")):
            for copy in (1, 2):
                for entry in ("update", "fused"):
                    cs.append(Case(fluid, "plm", rs, shp, copy, "first", entry))
    # ---- calm companions: the CFL scan (and the conversion) on states whose new speeds are ordinary numbers
    for shp in (A, B, C_, D, "8x12x10", "64x16"):
        cs.append(Case("mhd", "plm", "hlld", shp, 1, "first", "fused", calm=True))
    cs.append(Case("mhd", "plm", "hlld", A, 3, "last", "fused", flags="x3+x12+bf", calm=True))
    cs.append(Case("mhd", "plm", "hlld", A, 1, "first", "fused_dt", calm=True))
    for kw in (dict(recon="ppm4", rs="hlld", ng=3), dict(recon="plm", rs="hlle"), dict(recon="plm", rs="llf"),
               dict(recon="plm", rs="hlld", ideal=False), dict(recon="plm", rs="hlld", nscal=2)):
        cs.append(Case("mhd", shape=A, copy=1, weights="first", entry="fused", calm=True, **kw))
    for rs in ("llf", "hlle", "roe", "hllc"):
        cs.append(Case("hydro", "plm", rs, A, 1, "first", "fused", calm=True))
    cs.append(Case("hydro", "plm", "roe", A, 1, "first", "w", calm=True))
    return cs


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _pack_of(nmb, nx, ng, mhd, nscal, ideal, calm):
    return make_pack(nmb, nx, ng, mhd, nscal, ideal, sfloor=None if calm else 0.0)


def case_pack(case):
    nmb, nx = SHAPES[case.shape]
    return _pack_of(nmb, nx, case.ng, case.mhd, case.nscal, case.ideal, case.calm)


def case_state(case):
    return wild_state(*case.state_key())


def beta_dt_of(weights):
    g0, g1, beta, dt = WEIGHTS[weights]
    return g0, g1, beta*dt


@functools.lru_cache(maxsize=None)
def _expected(key):
    nmb, nx, ng, mhd, nscal, seed, ideal, tiny, recon, rs, weights, copy, c2p = key
    out = oracle_stage(_pack_of(nmb, nx, ng, mhd, nscal, ideal, tiny == 0), (recon, rs), beta_dt_of(weights), copy,
                       wild_state(nmb, nx, ng, mhd, nscal, seed, ideal, tiny), c2p, 1)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def case_expected(case):
    """oracle_stage of the case, computed once per distinct reference and shared (read-only)"""
    return _expected(case.oracle_key())
