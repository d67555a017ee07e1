"""ShearingBoxCC / ShearingBoxFC / OrbitalAdvectionCC / OrbitalAdvectionFC -- the shearing box (src/shearing_box/): source
terms, shear-periodic x1 boundaries and orbital advection of a hydro or an MHD fluid on one rank and a uniform mesh.

The objects exist iff the deck holds <shearing_box> (hydro/hydro.cpp:135-142, mhd/mhd.cpp:182-192).  Hydro and MHD bind
them to the tasks the reference's lists name: InitRecv (the distance the x1 boundaries have sheared), HydroSrcTerms /
MHDSrcTerms (SourceTermsCC after the physical source terms), SendU_OA / RecvU_OA and SendB_OA / RecvB_OA (last stage,
3-D), SendU_Shr / RecvU_Shr and SendB_Shr / RecvB_Shr (every stage after the exchange, 3-D), EField (+ SourceTermsFC,
2-D).  In 2-D only the source terms act (their r-z branch) and a shear-periodic face is a periodic one.  Every operator
is one or two launches of csrc/akmi_sbox.hip.  One fluid per deck: <hydro> next to <mhd>, and everything else outside
this slice, is refused by name in shearing_box_deck_checks.
"""
import numpy as np
import torch

from . import capi
from .mesh import SHEAR_PERIODIC, CellCenterX, LeftEdgeX


def _fatal(msg):
    raise RuntimeError("### FATAL ERROR " + msg)


def shearing_box_deck_checks(pin, nranks=1, restart=False):
    """what a deck with <shearing_box> may not ask for; called by MeshBlockPack.AddPhysics before anything is allocated"""
    if not pin.DoesBlockExist("shearing_box"):
        return
    pin.GetReal("shearing_box", "qshear")          # both required, shearing_box.cpp:30-31
    pin.GetReal("shearing_box", "omega0")
    if pin.DoesBlockExist("mhd") and pin.DoesBlockExist("hydro"):
        _fatal("<shearing_box> with <mhd> next to <hydro> is not on this path: one fluid")
    if pin.DoesBlockExist("ion-neutral"):
        _fatal("<shearing_box> with <ion-neutral> is not on this path")
    if pin.DoesBlockExist("mesh_refinement") and pin.GetOrAddString("mesh_refinement", "refinement", "none") != "none":
        _fatal("<shearing_box> with <mesh_refinement>/refinement = %s is not on this path (uniform meshes)"
               % pin.GetString("mesh_refinement", "refinement"))
    if nranks > 1:
        _fatal("<shearing_box> runs on one rank on this path (nranks=%d)" % nranks)
    if pin.DoesBlockExist("turb_driving"):
        _fatal("<shearing_box> with <turb_driving> is not on this path")
    if pin.DoesBlockExist("gravity"):
        _fatal("<shearing_box> with <gravity> is not on this path")
    if restart:
        _fatal("-r of a deck with <shearing_box>: restarting a shearing-box run is not on this path")
    for blk in list(pin.blocks):
        if blk.startswith("output") and pin.GetString(blk, "file_type") == "rst":
            _fatal("<shearing_box> with rst outputs (<%s>/file_type = rst) is not on this path" % blk)


def shearing_box_native_refusal(pin):
    """the C++ host has none of this: it must not run such a deck as if the block were not there"""
    if pin.DoesBlockExist("shearing_box") or "shear_periodic" in (
            pin.GetOrAddString("mesh", "ix1_bc", "periodic"), pin.GetOrAddString("mesh", "ox1_bc", "periodic")):
        _fatal("<shearing_box> runs on the Python host only (--host python): the C++ host (--host native) has neither the "
               "shear-periodic boundary nor orbital advection")


def _block_bounds(ppack, device):
    """device double[nmb][6]: x1min, x1max, x2min, x2max, x3min, x3max of every MeshBlock (xlim of include/akmi.h)"""
    b = np.array([[s.x1min, s.x1max, s.x2min, s.x2max, s.x3min, s.x3max] for s in ppack.pmb.mb_size], dtype=np.float64)
    return torch.from_numpy(b).to(device)


class ShearingBox:
    """shearing_box.cpp:24-68: parameters of the block and the MeshBlocks on the shear-periodic x1 faces"""

    def __init__(self, ppack, pin):
        self.pmy_pack = ppack
        self.qshear = pin.GetReal("shearing_box", "qshear")
        self.omega0 = pin.GetReal("shearing_box", "omega0")
        self.is_stratified = pin.GetOrAddBoolean("shearing_box", "stratified", False)
        self.shearing_box_r_phi = False            # 2D r-phi not yet implemented (shearing_box.cpp:27)
        self.yshear = 0.0
        bcs = np.asarray(ppack.pmb.mb_bcs)
        self.x1bndry_mbgid = [[ppack.gids + m for m in range(ppack.nmb_thispack) if bcs[m, n] == SHEAR_PERIODIC]
                              for n in (0, 1)]
        self.nmb_x1bndry = [len(g) for g in self.x1bndry_mbgid]

    def _x1_table(self, dev):
        """table of the boundary MeshBlocks (tab of include/akmi.h)"""
        ppack = self.pmy_pack
        pm = ppack.pmesh
        self.nslot = max(1, *self.nmb_x1bndry)
        self.nmbx2 = pm.nmb_rootx2
        self.tab_stride = 2 + self.nmbx2
        tab = np.zeros((2, self.nslot, self.tab_stride), dtype=np.int32)
        for n in (0, 1):
            slot_of = {g: s for s, g in enumerate(self.x1bndry_mbgid[n])}
            for s, g in enumerate(self.x1bndry_mbgid[n]):
                l1, l2, l3 = pm.lloc_eachmb[g][:3]
                tab[n, s, 0], tab[n, s, 1] = g - ppack.gids, l2
                for bx in range(self.nmbx2):
                    tab[n, s, 2 + bx] = slot_of[pm.gid_of_lloc[(l1, bx, l3)]]
        self.tab = torch.from_numpy(tab).to(dev)

    def InitRecv(self, time):
        """shearing_box_tasks.cpp:25-30: the x2 distance the x1 boundaries have sheared"""
        ms = self.pmy_pack.pmesh.mesh_size
        lx = (ms.x1max - ms.x1min)
        self.yshear = (self.qshear*self.omega0)*lx*time
        if self.yshear < 0.0 and sum(self.nmb_x1bndry):
            # (the three cases of shearing_box_cc.cpp:139-264 are written for an offset that grows from zero)
            _fatal("<shearing_box>: the shear-periodic boundary needs qshear*omega0*time >= 0 (yshear = %r at time = %r)"
                   % (self.yshear, time))


class ShearingBoxCC(ShearingBox):
    """shearing_box_cc.cpp / shearing_box_srcterms.cpp for the cell-centred variables of a hydro or an MHD fluid"""

    def __init__(self, ppack, pin, nvar, fluid):
        super().__init__(ppack, pin)
        self.pmy_fluid = fluid
        self.nvar = nvar
        pm = ppack.pmesh
        dev = fluid.device
        self.xlim = _block_bounds(ppack, dev)
        if sum(self.nmb_x1bndry) and self.qshear*self.omega0 < 0.0 and pm.three_d:
            _fatal("<shearing_box>: shear-periodic boundaries need qshear*omega0 >= 0 (qshear = %r, omega0 = %r)"
                   % (self.qshear, self.omega0))
        self._x1_table(dev)
        self.buf = None
        if sum(self.nmb_x1bndry) and pm.three_d:
            n3, n2, n1 = pm.mb_indcs.ncells
            self.buf = torch.zeros((2, self.nslot, nvar, n3, pm.mb_indcs.nx2, pm.mb_indcs.ng), dtype=torch.float64,
                                   device=dev)

    def SourceTermsCC(self, w0, bdt, u0, bcc0=None):
        """shearing_box_srcterms.cpp:27-84, and :92-150 when the cell-centred field of an MHD fluid is given; the
        coefficients as the reference writes them"""
        f = self.pmy_fluid
        coef1 = 2.0*bdt*self.omega0
        coef2 = (2.0 - self.qshear)*bdt*self.omega0
        coef3 = bdt*(self.omega0*self.omega0)
        qo = self.qshear*self.omega0
        if bcc0 is not None:
            capi.check(f.L.akmi_sbox_srcterms_mhd(f.pack_c, coef1, coef2, coef3, bdt, qo, 1 if self.is_stratified else 0,
                                                  self.xlim, w0, bcc0, u0, capi._stream()), "sbox_srcterms_mhd")
            return
        capi.check(f.L.akmi_sbox_srcterms(f.pack_c, coef1, coef2, coef3, bdt, qo, 1 if self.is_stratified else 0, self.xlim,
                                          w0, u0, capi._stream()), "sbox_srcterms")

    def PackAndSendCC(self, u0, recon):
        """shearing_box_cc.cpp:48-116: the fractional remap of both x1 ghost slabs into the buffer"""
        if self.buf is None:
            return
        f = self.pmy_fluid
        capi.check(f.L.akmi_sbox_remap_x1(f.pack_c, recon, self.nmb_x1bndry[0], self.nmb_x1bndry[1], self.nslot, self.tab,
                                          self.tab_stride, self.yshear, u0, self.buf, capi._stream()), "sbox_remap_x1")

    def RecvAndUnpackCC(self, u0):
        """shearing_box_cc.cpp:118-266 and :359-388: the integer shift and the copy into the ghost zones, one gather"""
        if self.buf is None:
            return
        f = self.pmy_fluid
        dx2 = float(self.pmy_pack.pmb.mb_size[0].dx2)
        joffset = int(self.yshear/dx2)
        capi.check(f.L.akmi_sbox_shift_x1(f.pack_c, self.nmb_x1bndry[0], self.nmb_x1bndry[1], self.nslot, self.tab,
                                          self.tab_stride, self.nmbx2, joffset, self.buf, u0, capi._stream()),
                   "sbox_shift_x1")


class ShearingBoxFC(ShearingBox):
    """shearing_box_fc.cpp and SourceTermsFC of shearing_box_srcterms.cpp for the face-centred field.  The reference
    neither remaps nor corrects the EMFs at this boundary; neither does this."""

    def __init__(self, ppack, pin, fluid):
        super().__init__(ppack, pin)
        self.pmy_fluid = fluid
        pm = ppack.pmesh
        dev = fluid.device
        self.xlim = _block_bounds(ppack, dev)
        self._x1_table(dev)
        self.buf = None
        if sum(self.nmb_x1bndry) and pm.three_d:
            n3, n2, n1 = pm.mb_indcs.ncells
            self.buf = torch.zeros((2, self.nslot, 3, n3, pm.mb_indcs.nx2, pm.mb_indcs.ng), dtype=torch.float64, device=dev)

    def SourceTermsFC(self, b0, efld):
        """shearing_box_srcterms.cpp:159-200: E = -(v_K x B) of the background flow, 2-D r-z only"""
        f = self.pmy_fluid
        capi.check(f.L.akmi_sbox_efield_2d(f.pack_c, self.qshear*self.omega0, self.xlim, b0.x1f, b0.x2f, efld.x1e, efld.x2e,
                                           capi._stream()), "sbox_efield_2d")

    def PackAndSendFC(self, b0, recon):
        """shearing_box_fc.cpp:48-136: the fractional remap of the three components of both x1 ghost slabs"""
        if self.buf is None:
            return
        f = self.pmy_fluid
        capi.check(f.L.akmi_sbox_remap_x1_fc(f.pack_c, recon, self.nmb_x1bndry[0], self.nmb_x1bndry[1], self.nslot, self.tab,
                                             self.tab_stride, self.yshear, b0.x1f, b0.x2f, b0.x3f, self.buf, capi._stream()),
                   "sbox_remap_x1_fc")

    def RecvAndUnpackFC(self, b0):
        """shearing_box_fc.cpp:138-286 and :379-431: the integer shift and the copy into the ghost faces, one gather"""
        if self.buf is None:
            return
        f = self.pmy_fluid
        dx2 = float(self.pmy_pack.pmb.mb_size[0].dx2)
        joffset = int(self.yshear/dx2)
        capi.check(f.L.akmi_sbox_shift_x1_fc(f.pack_c, self.nmb_x1bndry[0], self.nmb_x1bndry[1], self.nslot, self.tab,
                                             self.tab_stride, self.nmbx2, joffset, self.buf, b0.x1f, b0.x2f, b0.x3f,
                                             capi._stream()), "sbox_shift_x1_fc")


class OrbitalAdvectionCC:
    """orbital_advection.cpp:30-58, orbital_advection_cc.cpp: the remap of all of u0 along x2 by -qshear*omega0*x1*dt,
    once per cycle.  One rank: the rows beyond an x2 edge are read from the x2 neighbour's active cells (its pack index
    is in the neighbour table), so nothing is packed and PackAndSendCC has no work."""

    def __init__(self, ppack, pin, nvar, fluid):
        self.pmy_pack = ppack
        self.pmy_fluid = fluid
        self.qshear = pin.GetReal("shearing_box", "qshear")
        self.omega0 = pin.GetReal("shearing_box", "omega0")
        self.shearing_box_r_phi = False
        pm = ppack.pmesh
        ind = pm.mb_indcs
        # orbital_advection.cpp:39-42
        xmin, xmax = abs(pm.mesh_size.x1min), abs(pm.mesh_size.x1max)
        self.maxjshift = int(pm.cfl_no*max(xmin, xmax)) + 1
        if pm.three_d:
            if ind.ng + self.maxjshift > ind.nx2:
                # (the reference packs ng + maxjshift rows of a block of nx2: it would read outside the block)
                _fatal("<shearing_box>: orbital advection needs nghost + maxjshift <= <meshblock>/nx2, but %d + %d > %d "
                       "(maxjshift = int(cfl_number*max(|x1min|, |x1max|)) + 1)" % (ind.ng, self.maxjshift, ind.nx2))
            per = capi.BC["periodic"]
            if pm.mesh_bcs[2] != per or pm.mesh_bcs[3] != per:
                # (the reference would remap from buffers that nothing has filled)
                _fatal("<shearing_box>: orbital advection in 3-D needs periodic x2 faces (<mesh>/ix2_bc, ox2_bc)")
        self.xlim = _block_bounds(ppack, fluid.device)
        sz = ppack.pmb.mb_size
        self._x1v = np.array([CellCenterX(np.arange(ind.nx1), ind.nx1, s.x1min, s.x1max) for s in sz])
        self._dx2 = np.array([[s.dx2] for s in sz])

    def max_joffset(self, dt):
        """max over the columns of |int(yshear/dx2)|, yshear = -qshear*omega0*x1v*dt (orbital_advection_cc.cpp:244-245)"""
        yshear = -(self.qshear*self.omega0)*self._x1v*dt
        return int(np.abs(np.trunc(yshear/self._dx2)).max())

    def RecvAndUnpackCC(self, u0, out, recon):
        """orbital_advection_cc.cpp:215-288: out's active cells = u0 shifted and remapped; the caller swaps the two"""
        f = self.pmy_fluid
        dt = self.pmy_pack.pmesh.dt
        jmax = self.max_joffset(dt)
        if jmax > self.maxjshift:
            _fatal("<shearing_box>: orbital advection over dt = %r shifts a column by %d cells, more than maxjshift = %d "
                   "(the reference reads outside its buffers); lower <time>/cfl_number or the time step"
                   % (dt, jmax, self.maxjshift))
        capi.check(f.L.akmi_sbox_orbital_cc(f.pack_c, recon, self.maxjshift, self.qshear*self.omega0, dt,
                                            f.pbval_u.nghbr, self.xlim, u0, out, capi._stream()), "sbox_orbital_cc")


class OrbitalAdvectionFC(OrbitalAdvectionCC):
    """orbital_advection_fc.cpp: the shift of the face-centred field along x2 by constrained transport with the
    effective EMFs of the shift of B3 (at x1 cell centres) and B1 (at x1 faces).  The two EMF arrays are this object's
    own (orbital_advection_fc.cpp:43-49), cell-shaped.  As for the cell-centred variables nothing is packed: the rows
    beyond an x2 edge are read from the x2 neighbour's active rows."""

    def __init__(self, ppack, pin, fluid):
        super().__init__(ppack, pin, 3, fluid)
        ind = ppack.pmesh.mb_indcs
        self._x1f = np.array([LeftEdgeX(np.arange(ind.nx1 + 1), ind.nx1, s.x1min, s.x1max) for s in ppack.pmb.mb_size])
        self.emfx = self.emfz = None
        if ppack.pmesh.three_d:
            n3, n2, n1 = ind.ncells
            self.emfx = torch.zeros((ppack.nmb_thispack, n3, n2, n1), dtype=torch.float64, device=fluid.device)
            self.emfz = torch.zeros_like(self.emfx)

    def max_joffset(self, dt):
        """the largest |joffset| over the pencils of B3 (cell centres) and of B1 (faces is..ie+1)"""
        yshear = -(self.qshear*self.omega0)*self._x1f*dt
        return max(super().max_joffset(dt), int(np.abs(np.trunc(yshear/self._dx2)).max()))

    def RecvAndUnpackFC(self, b0, recon):
        """orbital_advection_fc.cpp:223-358: the effective EMFs, then CT in place"""
        f = self.pmy_fluid
        dt = self.pmy_pack.pmesh.dt
        jmax = self.max_joffset(dt)
        if jmax > self.maxjshift:
            _fatal("<shearing_box>: orbital advection over dt = %r shifts a column by %d cells, more than maxjshift = %d "
                   "(the reference reads outside its buffers); lower <time>/cfl_number or the time step"
                   % (dt, jmax, self.maxjshift))
        capi.check(f.L.akmi_sbox_orbital_emf(f.pack_c, recon, self.maxjshift, self.qshear*self.omega0, dt, f.pbval_u.nghbr,
                                             self.xlim, b0.x1f, b0.x3f, self.emfx, self.emfz, capi._stream()),
                   "sbox_orbital_emf")
        capi.check(f.L.akmi_sbox_orbital_ct(f.pack_c, self.emfx, self.emfz, b0.x1f, b0.x2f, b0.x3f, capi._stream()),
                   "sbox_orbital_ct")
