"""ConsToPrim, the CFL scans and the two in-place / out-of-place pairs (csrc/akmi_c2p.hpp and its users) one entry point
at a time against the `akref_*` twin, bit for bit over whole arrays.

Packs: rows of 74 (more than a wave, no multiple of one) in 3-D, a 2-D pack with an odd N1, a 1-D pack of three 64-lane
tiles; every block has its own cell sizes.  Gases: ideal with and without passive scalars (some negative), ideal with a
temperature floor, isothermal with and without a scalar; hydro and MHD.  About a tenth of all cells (ghost cells
included) lie below the density floor and a tenth below the pressure floor, so that every floor counter that the case can
hit is above zero in the oracle alone -- asserted without a GPU, and again where the kernels are compared.
Arrays a call must not touch outside its box carry a sentinel there."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import akref

FLT_MAX = float(np.finfo(np.float32).max)
GAMMA = 1.4
DFLOOR, PFLOOR, ISO_CS, SIGMA_MAX = 0.05, 0.02, 0.8, 20.0
SENTINEL = -777.25

# (nmb, nx1, nx2, nx3, ng)
PACKS = [(2, 70, 6, 4, 2), (2, 33, 9, 1, 3), (3, 130, 1, 1, 2)]
_pid = lambda s: "%dx%dx%d-nmb%d-ng%d" % (s[1], s[2], s[3], s[0], s[4])
packs = pytest.mark.parametrize("pack", PACKS, ids=_pid)
# one seed per pack, chosen so that the few ghost cells of the small packs (twelve in the 1-D one) hold a cell below each
# floor in every gas: test_oracle_alone_hits_every_floor_the_case_can_hit
SEEDS = {PACKS[0]: 1, PACKS[1]: 1, PACKS[2]: 10}
# name -> (is_ideal, nvar, tfloor)
GASES = {"ideal": (1, 5, None), "ideal-2scalars": (1, 7, None), "ideal-tfloor": (1, 5, 0.5),
         "isothermal": (0, 4, None), "isothermal-1scalar": (0, 5, None)}
gases = pytest.mark.parametrize("gas", list(GASES))
fluids = pytest.mark.parametrize("mhd", [False, True], ids=["hydro", "mhd"])


def _dx(nmb, pow2=False):
    if pow2:
        return np.array([(2.0**-(6 + m), 2.0**-(5 + m), 2.0**-(4 + m)) for m in range(nmb)])
    return np.array([(0.013 + 0.002*m, 0.017 + 0.003*m, 0.023 + 0.005*m) for m in range(nmb)])


class Case:
    """a pack, its index space and a rough conserved state with cells below the floors; shared and read-only"""

    def __init__(self, pack, gas="ideal", mhd=False, pow2=False):
        nmb, nx1, nx2, nx3, ng = pack
        ideal, nvar, tfloor = GASES[gas]
        self.nmb, self.nvar, self.ideal, self.mhd, self.tfloor = nmb, nvar, ideal, mhd, tfloor
        self.pk, self.dx = akref.make_pack(nmb, nx1, nx2, nx3, ng, _dx(nmb, pow2), GAMMA, nvar=nvar, dfloor=DFLOOR,
                                           pfloor=PFLOOR, tfloor=tfloor, sigma_max=SIGMA_MAX if mhd else None)
        self.pk.is_ideal, self.pk.iso_cs = ideal, ISO_CS
        self.N1, self.N2, self.N3 = nx1 + 2*ng, (nx2 + 2*ng if nx2 > 1 else 1), (nx3 + 2*ng if nx3 > 1 else 1)
        self.is_, self.ie = ng, ng + nx1 - 1
        self.js, self.je = (ng, ng + nx2 - 1) if nx2 > 1 else (0, 0)
        self.ks, self.ke = (ng, ng + nx3 - 1) if nx3 > 1 else (0, 0)
        self.full = (0, self.N1 - 1, 0, self.N2 - 1, 0, self.N3 - 1)
        # strictly inside the arrays in every direction that exists
        self.sub = (1, self.N1 - 3) + ((1, self.N2 - 3) if nx2 > 1 else (0, 0)) + ((1, self.N3 - 3) if nx3 > 1 else (0, 0))
        N1, N2, N3 = self.N1, self.N2, self.N3
        rng = np.random.default_rng([SEEDS[pack], nvar, ideal, mhd])
        self.b = [0.5*rng.normal(size=s) for s in ((nmb, N3, N2, N1 + 1), (nmb, N3, N2 + 1, N1), (nmb, N3 + 1, N2, N1))]
        u = rng.normal(size=(nmb, nvar, N3, N2, N1))
        u[:, 0] = np.abs(u[:, 0]) + 0.1
        u[:, 1:4] *= 0.5
        low_d = rng.random(u[:, 0].shape) < 0.1
        u[:, 0][low_d] = 0.8*DFLOOR*rng.random(int(low_d.sum()))
        if ideal:
            e_other = 0.5*(u[:, 1]**2 + u[:, 2]**2 + u[:, 3]**2)/u[:, 0]
            if mhd:
                bx, by, bz = (0.5*(self.b[0][..., 1:] + self.b[0][..., :-1]), 0.5*(self.b[1][:, :, 1:] + self.b[1][:, :, :-1]),
                              0.5*(self.b[2][:, 1:] + self.b[2][:, :-1]))
                e_other = e_other + 0.5*(bx*bx + by*by + bz*bz)
            low_p = rng.random(e_other.shape) < 0.1
            u[:, 4] = e_other + np.where(low_p, 0.001, np.abs(u[:, 4]) + 0.1)     # efloor = PFLOOR/(GAMMA - 1) = 0.05
        self.u = u
        for x in [self.u] + self.b:
            x.setflags(write=False)

    def box_mask(self, box):
        il, iu, jl, ju, kl, ku = box
        m = np.zeros((self.N3, self.N2, self.N1), dtype=bool)
        m[kl:ku + 1, jl:ju + 1, il:iu + 1] = True
        return m

    def fresh(self, box=None):
        """u0 (a copy, the sentinel outside `box`), w0 and bcc0 full of the sentinel, counters that are not zero"""
        u = self.u.copy()
        if box is not None:
            u[:, :, ~self.box_mask(box)] = SENTINEL
        w = np.full_like(u, SENTINEL)
        bcc = np.full((self.nmb, 3, self.N3, self.N2, self.N1), SENTINEL)
        return u, w, bcc, np.array([3, 5, 7, 0], dtype=np.int32)

    def oracle_c2p(self, box, u, w, bcc, cnt):
        R = akref.lib()
        if self.mhd:
            rc = R.akref_mhd_c2p(C.byref(self.pk), akref.ptr(u), *[akref.ptr(x) for x in self.b], akref.ptr(w),
                                 akref.ptr(bcc), *box, akref.ptr(cnt))
        else:
            rc = R.akref_hydro_c2p(C.byref(self.pk), akref.ptr(u), akref.ptr(w), *box, akref.ptr(cnt))
        assert rc == 0

    def oracle_newdt(self, w, bcc):
        R, dt3 = akref.lib(), np.zeros(3)
        if self.mhd:
            assert R.akref_mhd_newdt(C.byref(self.pk), akref.ptr(w), akref.ptr(bcc), akref.ptr(dt3)) == 0
        else:
            assert R.akref_hydro_newdt(C.byref(self.pk), akref.ptr(w), akref.ptr(dt3)) == 0
        return dt3

    def floors_fired(self, cnt):
        """every counter the case can hit moved from its start value (fresh()), the others did not"""
        hit = (cnt[:3] - np.array([3, 5, 7])).tolist()
        want = [True, bool(self.ideal), bool(self.ideal and self.tfloor)]
        assert [h > 0 for h in hit] == want and min(hit) >= 0, (hit, want)

    def shell_slabs(self):
        """the partition of the ghost shell k_c2p_shell uses: k-ghost planes over all j, i; j-ghost rows of the active
        planes; i-ghost columns of the active rows"""
        N1, N2, N3 = self.N1, self.N2, self.N3
        s = []
        if N3 > 1:
            s += [(0, N1 - 1, 0, N2 - 1, 0, self.ks - 1), (0, N1 - 1, 0, N2 - 1, self.ke + 1, N3 - 1)]
        if N2 > 1:
            s += [(0, N1 - 1, 0, self.js - 1, self.ks, self.ke), (0, N1 - 1, self.je + 1, N2 - 1, self.ks, self.ke)]
        s += [(0, self.is_ - 1, self.js, self.je, self.ks, self.ke), (self.ie + 1, N1 - 1, self.js, self.je, self.ks, self.ke)]
        return s


@functools.lru_cache(maxsize=None)
def _case(pack, gas="ideal", mhd=False, pow2=False):
    return Case(pack, gas, mhd, pow2)


@functools.lru_cache(maxsize=None)
def _prims(pack, gas, mhd):
    """the oracle's conversion of the whole pack: input of the NewTimeStep entries, read-only"""
    c = _case(pack, gas, mhd)
    u, w, bcc, cnt = c.fresh()
    c.oracle_c2p(c.full, u, w, bcc, cnt)
    for x in (u, w, bcc, cnt):
        x.setflags(write=False)
    return u, w, bcc, cnt


# ---- not gpu: the inputs do what they are meant to ------------------------------------------------------------------
@packs
@gases
@fluids
def test_oracle_alone_hits_every_floor_the_case_can_hit(pack, gas, mhd):
    c = _case(pack, gas, mhd)
    c.floors_fired(_prims(pack, gas, mhd)[3])
    u, w, bcc, cnt = c.fresh(c.sub)
    c.oracle_c2p(c.sub, u, w, bcc, cnt)
    c.floors_fired(cnt)
    out = ~c.box_mask(c.sub)
    assert np.all(w[:, :, out] == SENTINEL) and np.all(u[:, :, out] == SENTINEL) and not np.any(w[:, :, ~out] == SENTINEL)
    u, w, bcc, cnt = c.fresh()
    for box in c.shell_slabs():
        c.oracle_c2p(box, u, w, bcc, cnt)
    c.floors_fired(cnt)
    below_d = (c.u[:, 0] < DFLOOR).mean()
    assert 0.07 < below_d < 0.13
    if c.nvar > (5 if c.ideal else 4):
        assert (c.u[:, -1] < 0.0).any()
    dt3 = c.oracle_newdt(*_prims(pack, gas, mhd)[1:3])
    assert np.all(dt3 > 0.0) and np.all(dt3 < 1.0)


# ---- gpu ------------------------------------------------------------------------------------------------------------
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
        self.b = [self.t(x) for x in c.b]

    def t(self, x):
        return self.torch.from_numpy(np.array(x)).cuda()           # a copy: the shared inputs are read-only

    def p(self, *tensors):
        return [self.capi._p(x) for x in tensors]


def _same(host, dev, names):
    for n, x, y in zip(names, host, dev):
        assert np.array_equal(x, y.cpu().numpy()), n


@pytest.mark.gpu
@packs
@gases
@fluids
@pytest.mark.parametrize("box", ["full", "sub"])
def test_hip_c2p_matches_the_oracle(pack, gas, mhd, box):
    c = _case(pack, gas, mhd)
    D = Dev(c)
    rng = c.full if box == "full" else c.sub
    host = c.fresh(rng)
    ud, wd, bd, cd = dev = [D.t(x) for x in host]
    c.oracle_c2p(rng, *host)
    c.floors_fired(host[3])
    if mhd:
        rc = D.L.akmi_mhd_c2p(D.P, *D.p(ud, *D.b, wd, bd), *rng, *D.p(cd), None)
    else:
        rc = D.L.akmi_hydro_c2p(D.P, *D.p(ud, wd), *rng, *D.p(cd), None)
    D.capi.check(rc, "c2p")
    print("counters oracle %r hip %r" % (host[3].tolist(), cd.cpu().numpy().tolist()))
    _same(host, dev, ("u0", "w0", "bcc0", "counters"))


@pytest.mark.gpu
@packs
@gases
@fluids
@pytest.mark.parametrize("do_newdt", [0, 1, 2])
def test_hip_c2p_newdt_matches_the_oracle(pack, gas, mhd, do_newdt):
    """do_newdt 0: dt3 is not touched; 1: the entry resets it first; 2: the caller has, and a slot that already holds
    less than any cell gives keeps its value"""
    c = _case(pack, gas, mhd)
    D = Dev(c)
    u, w, bcc, cnt = (x.copy() for x in _prims(pack, gas, mhd))
    if not mhd:
        bcc[:] = SENTINEL
    start = {0: [1.5, 2.5, 3.5], 1: [1e-30, -1.0, 0.0], 2: [FLT_MAX, 1e-30, FLT_MAX]}[do_newdt]
    want = c.oracle_newdt(w, bcc) if do_newdt else np.array(start)
    if do_newdt == 2:
        assert want[1] > 1e-30
        want[1] = 1e-30
    u0, w0, bcc0, cnt0 = c.fresh()
    ud, wd, bd, cd, dtd = [D.t(x) for x in (u0, w0, bcc0, cnt0, np.array(start))]
    if mhd:
        rc = D.L.akmi_mhd_c2p_newdt(D.P, *D.p(ud, *D.b, wd, bd), do_newdt, *D.p(cd, dtd), None)
    else:
        rc = D.L.akmi_hydro_c2p_newdt(D.P, *D.p(ud, wd), do_newdt, *D.p(cd, dtd), None)
    D.capi.check(rc, "c2p_newdt")
    print("dt3 oracle %r hip %r" % (want.tolist(), dtd.cpu().numpy().tolist()))
    c.floors_fired(cnt)
    _same((u, w, bcc, cnt, want), (ud, wd, bd, cd, dtd), ("u0", "w0", "bcc0", "counters", "dt3"))


@pytest.mark.gpu
@packs
@gases
@fluids
def test_hip_c2p_shell_matches_the_oracle_on_its_slabs(pack, gas, mhd):
    """the ghost shell, converted by the oracle slab by slab; the active cells keep the sentinel"""
    c = _case(pack, gas, mhd)
    D = Dev(c)
    act = c.box_mask((c.is_, c.ie, c.js, c.je, c.ks, c.ke))
    u0, w0, bcc0, cnt0 = c.fresh()
    u0[:, :, act] = SENTINEL
    host = [x.copy() for x in (u0, w0, bcc0, cnt0)]
    for box in c.shell_slabs():
        c.oracle_c2p(box, *host)
    c.floors_fired(host[3])
    assert np.all(host[1][:, :, act] == SENTINEL) and not np.any(host[1][:, :, ~act] == SENTINEL)
    ud, wd, bd, cd = dev = [D.t(x) for x in (u0, w0, bcc0, cnt0)]
    if mhd:
        rc = D.L.akmi_mhd_c2p_shell(D.P, *D.p(ud, *D.b, wd, bd, cd), None)
    else:
        rc = D.L.akmi_hydro_c2p_shell(D.P, *D.p(ud, wd, cd), None)
    D.capi.check(rc, "c2p_shell")
    _same(host, dev, ("u0", "w0", "bcc0", "counters"))


@pytest.mark.gpu
@packs
@pytest.mark.parametrize("gas", ["ideal", "ideal-2scalars", "isothermal", "isothermal-1scalar"])
@fluids
def test_hip_newdt_matches_the_oracle(pack, gas, mhd):
    c = _case(pack, gas, mhd)
    D = Dev(c)
    _, w, bcc, _ = _prims(pack, gas, mhd)
    want = c.oracle_newdt(w, bcc)
    wd, bd, dtd = D.t(w), D.t(bcc), D.t(np.array([1e-30, -1.0, 0.0]))      # the entry resets dt3 itself
    if mhd:
        rc = D.L.akmi_mhd_newdt(D.P, *D.p(wd, bd, dtd), None)
    else:
        rc = D.L.akmi_hydro_newdt(D.P, *D.p(wd, dtd), None)
    D.capi.check(rc, "newdt")
    print("dt3 oracle %r hip %r" % (want.tolist(), dtd.cpu().numpy().tolist()))
    assert np.array_equal(want, dtd.cpu().numpy())


@pytest.mark.gpu
@packs
@pytest.mark.parametrize("still", [0, 1, 2], ids=["vx=0", "vy=0", "vz=0"])
def test_hip_kinematic_newdt_matches_the_oracle(pack, still):
    """dx/|v| per cell; a direction without any motion keeps FLT_MAX"""
    c = _case(pack)
    D = Dev(c)
    w = _prims(pack, "ideal", False)[1].copy()
    w[:, 1 + still] = 0.0
    want = np.zeros(3)
    assert akref.lib().akref_kinematic_newdt(C.byref(c.pk), akref.ptr(w), akref.ptr(want)) == 0
    assert want[still] == FLT_MAX and np.all(np.delete(want, still) < 1.0)
    wd, dtd = D.t(w), D.t(np.array([1e-30, -1.0, 0.0]))
    D.capi.check(D.L.akmi_kinematic_newdt(D.P, *D.p(wd, dtd), None), "kinematic_newdt")
    assert np.array_equal(want, dtd.cpu().numpy())


RK = (0.5, 0.5, 0.0037)           # gam0, gam1, beta*dt


@pytest.mark.gpu
@packs
@pytest.mark.parametrize("pow2", [False, True], ids=["dx", "pow2-dx"])
@pytest.mark.parametrize("nvar_gas", ["ideal", "ideal-2scalars"])
@pytest.mark.parametrize("fs", [0, 1], ids=["cell-shaped", "face-shaped"])
def test_hip_rk_update_in_place_and_out_of_place(pack, pow2, nvar_gas, fs):
    """u1 == u0 (the state after CopyCons): the in-place entry, the out-of-place entry (+ swap) and the oracle agree"""
    c = _case(pack, nvar_gas, False, pow2)
    D = Dev(c)
    rng = np.random.default_rng(11)
    N1, N2, N3 = c.N1, c.N2, c.N3
    flx = [rng.normal(size=(c.nmb, c.nvar, N3, N2, N1 + fs)), rng.normal(size=(c.nmb, c.nvar, N3, N2 + fs, N1)),
           rng.normal(size=(c.nmb, c.nvar, N3 + fs, N2, N1))]
    want = c.u.copy()
    assert akref.lib().akref_rk_update(C.byref(c.pk), *[C.c_double(x) for x in RK], akref.ptr(want), akref.ptr(c.u),
                                       *[akref.ptr(x) for x in flx], fs) == 0
    assert not np.array_equal(want, c.u)
    fd = [D.t(x) for x in flx]
    u0d, u1d = D.t(c.u), D.t(c.u)
    D.capi.check(D.L.akmi_rk_update(D.P, *RK, *D.p(u0d, u1d, *fd), fs, None), "rk_update")
    src, dst = D.t(c.u), D.t(np.full_like(c.u, SENTINEL))
    D.capi.check(D.L.akmi_rk_update_oop(D.P, *RK, *D.p(src, dst, *fd), fs, None), "rk_update_oop")
    _same((want, c.u, want, c.u), (u0d, u1d, dst, src), ("u0 in place", "u1 in place", "dst", "src"))


@pytest.mark.gpu
@packs
@pytest.mark.parametrize("pow2", [False, True], ids=["dx", "pow2-dx"])
def test_hip_ct_in_place_and_out_of_place(pack, pow2):
    """b1 == b0: the in-place entry, the out-of-place entry (+ swap) and the oracle agree on all three face arrays"""
    c = _case(pack, "ideal", True, pow2)
    D = Dev(c)
    rng = np.random.default_rng(13)
    N1, N2, N3 = c.N1, c.N2, c.N3
    e = [rng.normal(size=(c.nmb, N3 + 1, N2 + 1, N1)), rng.normal(size=(c.nmb, N3 + 1, N2, N1 + 1)),
         rng.normal(size=(c.nmb, N3, N2 + 1, N1 + 1))]
    want = [x.copy() for x in c.b]
    assert akref.lib().akref_mhd_ct(C.byref(c.pk), *[C.c_double(x) for x in RK], *[akref.ptr(x) for x in e],
                                    *[akref.ptr(x) for x in want], *[akref.ptr(x) for x in c.b]) == 0
    assert not np.array_equal(want[2], c.b[2])
    ed = [D.t(x) for x in e]
    b0d, b1d = [D.t(x) for x in c.b], [D.t(x) for x in c.b]
    D.capi.check(D.L.akmi_mhd_ct(D.P, *RK, *D.p(*ed, *b0d, *b1d), None), "mhd_ct")
    dst = [D.t(np.full_like(x, SENTINEL)) for x in c.b]
    D.capi.check(D.L.akmi_mhd_ct_oop(D.P, *RK, *D.p(*ed, *D.b, *dst), None), "mhd_ct_oop")
    _same(want + c.b + want + c.b, b0d + b1d + dst + D.b, ["b0 in place"]*3 + ["b1 in place"]*3 + ["dst"]*3 + ["src"]*3)
