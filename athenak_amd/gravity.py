"""Gravity / MGGravityDriver -- self-gravity by a multigrid Poisson solver, <gravity>
(src/gravity/gravity.cpp, mg_gravity.cpp:39-245; src/multigrid/multigrid.cpp, multigrid_driver.cpp, multigrid_tasks.cpp).

On this path: one rank, a uniform 3-D mesh, cubic MeshBlocks with a power-of-two edge, cubic cells, mg_nghost = 1.  The
faces of the mesh are periodic or, with <gravity>/mg_bc = zerofixed | zerograd | multipole written in the deck, physical
(mg_gravity.cpp:66-126).  Everything else stops in gravity_deck_checks with the name of the parameter.

The level structure is the reference's: the MeshBlock levels (edge n, n/2, ... 1) on top of the root-grid levels (the
grid of MeshBlocks, halved while all three extents stay even); SetupMultigrid, SolveFMG / SolveFMGCoarser /
FMGProlongate, SolveMG -> SolveIterative / SolveIterativeFixedTimes, SolveVCycle, OneStepToCoarser / OneStepToFiner and
SolveCoarsestGrid run inside akmi_mg_solve (csrc/akmi_mg.hip), which enqueues the several hundred small launches of
one Solve from C++; this module owns the parameters, the level bookkeeping, the workspace and phi, and prints what
the reference prints.  DESIGN section 19.
"""
import ctypes as C

import numpy as np
import torch

from . import capi


def root_levels(nrbx1, nrbx2, nrbx3):
    """multigrid.cpp:100-108: the root grid is halved while every extent divides"""
    nlevel = 0
    for l in range(20):
        if nrbx1 % (1 << l) == 0 and nrbx2 % (1 << l) == 0 and nrbx3 % (1 << l) == 0:
            nlevel = l + 1
    return nlevel


def block_levels(nx):
    """multigrid.cpp:133-138: 0 = not a power of two"""
    for l in range(20):
        if (1 << l) == nx:
            return l + 1
    return 0


def level_counts(mesh_n, block_n):
    """(nrootlevel, nmblevel, ntotallevel, ni): SetupMultigrid (multigrid_driver.cpp:239-256) and the sweep count of
    SolveCoarsestGrid (:869-870)"""
    nrb = tuple(mesh_n[q]//block_n[q] for q in range(3))
    nroot, nmb = root_levels(*nrb), block_levels(block_n[0])
    return nroot, nmb, nroot + nmb - 1, max(nrb) >> (nroot - 1)


def _fatal(msg):
    raise RuntimeError("### FATAL ERROR " + msg)


def gravity_deck_checks(pin, nranks=1, restart=False):
    """what a deck with <gravity> may not ask for; called by MeshBlockPack.AddPhysics before anything is allocated"""
    if not pin.DoesBlockExist("gravity"):
        return
    g = "gravity"
    if pin.DoesBlockExist("mesh_refinement") and pin.GetOrAddString("mesh_refinement", "refinement", "none") != "none":
        _fatal("<gravity> with <mesh_refinement>/refinement = %s is not on this path (uniform meshes: the octets of "
               "refined meshes are not built)" % pin.GetString("mesh_refinement", "refinement"))
    if nranks > 1:
        _fatal("<gravity> runs on one rank on this path (nranks=%d)" % nranks)
    if pin.DoesBlockExist("ion-neutral"):
        _fatal("<gravity> with <ion-neutral> is not on this path")
    if restart:
        _fatal("-r of a deck with <gravity>: restarting a self-gravitating run is not on this path")
    for blk in list(pin.blocks):
        if blk.startswith("output") and pin.GetString(blk, "file_type") == "rst":
            _fatal("<gravity> with rst outputs (<%s>/file_type = rst) is not on this path" % blk)
    faces = [(name, pin.GetOrAddString("mesh", name, "periodic"))
             for name in ("ix1_bc", "ox1_bc", "ix2_bc", "ox2_bc", "ix3_bc", "ox3_bc")]
    physical = [(name, v) for name, v in faces if v != "periodic"]
    mg_bc = pin.GetOrAddString(g, "mg_bc", "none")
    if physical and mg_bc == "none":
        # (the reference would silently take zerofixed; here the deck has to say which)
        _fatal("<gravity> needs periodic faces on this path unless <gravity>/mg_bc = zerofixed | zerograd | multipole "
               "says what the Poisson solver does at the others: <mesh>/%s = %s" % physical[0])
    if mg_bc != "none" and mg_bc not in capi.MGBC:
        _fatal("in MGGravityDriver\nUnknown mg_bc type: %s" % mg_bc)
    if mg_bc != "none" and not physical:
        _fatal("<gravity>/mg_bc = %s on a mesh with six periodic faces is not on this path (it would have no effect: "
               "none)" % mg_bc)
    if pin.GetOrAddReal(g, "mask_radius", -1.0) > 0.0 and not physical:
        _fatal("<gravity>/mask_radius > 0 on a strictly periodic mesh is not on this path")
    if mg_bc == "multipole":
        # the reference's own fatal errors, mg_gravity.cpp:99-117
        if pin.GetOrAddInteger(g, "mporder", 4) not in (2, 4):
            _fatal("in MGGravityDriver\nmporder must be 2 (quadrupole) or 4 (hexadecapole).")
        if pin.GetOrAddBoolean(g, "auto_mporigin", True):
            if pin.GetOrAddBoolean(g, "nodipole", False):
                _fatal("in MGGravityDriver\nauto_mporigin and nodipole cannot be used together.")
        else:
            for d in (1, 2, 3):
                if not pin.DoesParameterExist(g, "mporigin_x%d" % d):
                    _fatal("Parameter name 'mporigin_x%d' not found in block 'gravity'" % d)
    if pin.GetOrAddInteger(g, "mg_nghost", 1) != 1:
        _fatal("<gravity>/mg_nghost = %d is not on this path (1)" % pin.GetInteger(g, "mg_nghost"))
    if pin.GetOrAddBoolean(g, "root_on_host", False):
        _fatal("<gravity>/root_on_host = true is not on this path (the root grid is solved on the device)")
    nx = [pin.GetInteger("mesh", "nx%d" % d) for d in (1, 2, 3)]
    if nx[1] == 1 or nx[2] == 1:
        _fatal("in MultigridDriver::MultigridDriver\nCurrently the Multigrid solver works only in 3D.")
    mb = [pin.GetOrAddInteger("meshblock", "nx%d" % d, nx[d - 1]) for d in (1, 2, 3)]
    if mb[0] != mb[1] or mb[0] != mb[2]:
        _fatal("in Multigrid::Multigrid\nThe Multigrid solver requires logically cubic MeshBlock.")
    if block_levels(mb[0]) == 0:
        _fatal("in Multigrid::Multigrid\nThe MeshBlock size must be power of two.")
    dx = [(pin.GetReal("mesh", "x%dmax" % d) - pin.GetReal("mesh", "x%dmin" % d))/float(nx[d - 1]) for d in (1, 2, 3)]
    if dx[0] != dx[1] or dx[0] != dx[2]:
        _fatal("<gravity> needs cubic cells (dx1 == dx2 == dx3): dx = %r; the reference uses dx1 alone" % (dx,))
    # the reference's own fatal errors, mg_gravity.cpp:52-65
    if pin.GetOrAddReal(g, "threshold", -1.0) < 0.0 and pin.GetOrAddInteger(g, "niteration", -1) < 0:
        _fatal("in MGGravityDriver::MGGravityDriver\nEither \"threshold\" or \"niteration\" parameter must be set in "
               "the <gravity> block.\nWhen both parameters are specified, \"niteration\" is ignored.\nSet \"threshold "
               "= 0.0\" for automatic convergence control.")
    if pin.GetOrAddReal(g, "four_pi_G", -1.0) < 0.0:
        _fatal("in MGGravityDriver::MGGravityDriver\nGravitational constant must be set in the "
               "Mesh::InitUserMeshData using the SetGravitationalConstant or SetFourPiG function.")


class MGGravityDriver:
    """mg_gravity.cpp:39-138 (parameters) and :177-245 (Solve)"""

    def __init__(self, ppack, pin, device):
        g = "gravity"
        self.pmy_pack = ppack
        self.device = device
        self.four_pi_G_ = pin.GetOrAddReal(g, "four_pi_G", -1.0)
        self.omega_ = pin.GetOrAddReal(g, "omega", 1.15)
        self.eps_ = pin.GetOrAddReal(g, "threshold", -1.0)
        self.niter_ = pin.GetOrAddInteger(g, "niteration", -1)
        # (the reference reads these two with GetOrAddReal into ints; the MultigridDriver defaults are 1)
        self.npresmooth_ = int(pin.GetOrAddReal(g, "npresmooth", 1))
        self.npostsmooth_ = int(pin.GetOrAddReal(g, "npostsmooth", 1))
        self.full_multigrid_ = pin.GetOrAddBoolean(g, "full_multigrid", False)
        self.fmg_ncycle_ = pin.GetOrAddInteger(g, "fmg_ncycle", 1)
        self.fshowdef_ = pin.GetOrAddInteger(g, "show_defect", 0)
        self.mg_verbose_ = pin.GetOrAddInteger(g, "mg_verbose", 0)
        self.fsubtract_average_ = pin.GetOrAddBoolean(g, "subtract_average", True)
        pm = ppack.pmesh
        # mg_gravity.cpp:66-126: one type for every non-periodic face, the multipole settings, the mask
        self.mg_bc_ = pin.GetOrAddString(g, "mg_bc", "none")
        self.periodic_ = [int(b == capi.BC["periodic"]) for b in pm.mesh_bcs[:6]]
        if not pm.strictly_periodic:
            self.fsubtract_average_ = False
        self.mporder_, self.autompo_, self.nodipole_, self.mpo_ = -1, True, False, [0.0, 0.0, 0.0]
        if self.mg_bc_ == "multipole":
            self.mporder_ = pin.GetOrAddInteger(g, "mporder", 4)
            self.autompo_ = pin.GetOrAddBoolean(g, "auto_mporigin", True)
            self.nodipole_ = pin.GetOrAddBoolean(g, "nodipole", False)
            if not self.autompo_:
                self.mpo_ = [pin.GetReal(g, "mporigin_x%d" % d) for d in (1, 2, 3)]
            self.fsubtract_average_ = False
        self.mask_radius_ = pin.GetOrAddReal(g, "mask_radius", -1.0)
        self.mask_origin_ = [pin.GetOrAddReal(g, "mask_origin_x%d" % d, 0.0) for d in (1, 2, 3)]
        ind, ms = pm.mb_indcs, pm.mesh_size
        self.nrbx = (pm.nmb_rootx1, pm.nmb_rootx2, pm.nmb_rootx3)
        self.nrootlevel_, self.nmblevel_, self.ntotallevel_, self.ni_ = level_counts(
            (pm.mesh_indcs.nx1, pm.mesh_indcs.nx2, pm.mesh_indcs.nx3), (ind.nx1, ind.nx2, ind.nx3))
        self.coffset_ = 0
        self.nmb = ppack.nmb_thispack
        sz = ppack.pmb.mb_size[0]
        self.rdx_ = (sz.x1max - sz.x1min)/float(ind.nx1)                 # block_rdx, multigrid.cpp:87-92
        self.root_rdx_ = (ms.x1max - ms.x1min)/float(self.nrbx[0])       # rdx_ of the root Multigrid, :77
        self.vol_ = (ms.x1max - ms.x1min)*(ms.x2max - ms.x2min)*(ms.x3max - ms.x3min)
        lloc = np.array([tuple(pm.lloc_eachmb[int(gid)])[:3] for gid in ppack.pmb.mb_gid], dtype=np.int32)
        self.lloc_dev = torch.from_numpy(lloc.reshape(-1).copy()).to(device)
        self.nghbr_dev = torch.from_numpy(np.ascontiguousarray(ppack.pmb.nghbr_gid, dtype=np.int32).reshape(-1)).to(device)
        xlim = np.array([[s.x1min, s.x1max, s.x2min, s.x2max, s.x3min, s.x3max] for s in ppack.pmb.mb_size])
        self.xlim_dev = torch.from_numpy(xlim.reshape(-1).copy()).to(device)
        self.mesh_ext_ = [ms.x1min, ms.x1max, ms.x2min, ms.x2max, ms.x3min, ms.x3max]
        self.L = capi.lib()
        self.plan = capi.MgPlan()
        self.ws = None
        self.norms = (C.c_double*capi.MG_NNORMS)()
        self.ncycles = C.c_int(0)
        self.last_norms = []
        self.failed = False

    def SetFourPiG(self, four_pi_G):
        self.four_pi_G_ = four_pi_G

    def _fill_plan(self, fluid):
        p, ind = self.plan, self.pmy_pack.pmesh.mb_indcs
        p.nmb, p.nxb = self.nmb, ind.nx1
        p.nrx1, p.nrx2, p.nrx3 = self.nrbx
        p.nmblevel, p.nrootlevel = self.nmblevel_, self.nrootlevel_
        p.ng, p.nvar = ind.ng, fluid.nvars
        p.npresmooth, p.npostsmooth, p.niter = self.npresmooth_, self.npostsmooth_, self.niter_
        p.full_multigrid, p.fmg_ncycle = int(self.full_multigrid_), self.fmg_ncycle_
        p.subtract_average, p.show_defect = int(self.fsubtract_average_), self.fshowdef_
        p.rdx, p.root_dx, p.omega = self.rdx_, self.root_rdx_, self.omega_
        p.four_pi_G, p.eps, p.vol = self.four_pi_G_, self.eps_, self.vol_
        p.nghbr, p.lloc = self.nghbr_dev.data_ptr(), self.lloc_dev.data_ptr()
        p.mg_bc = capi.MGBC[self.mg_bc_]
        p.periodic[:], p.mesh_ext[:] = self.periodic_, self.mesh_ext_
        p.mporder, p.nodipole, p.auto_mporigin = max(self.mporder_, 0), int(self.nodipole_), int(self.autompo_)
        p.mporigin[:], p.mask_radius, p.mask_origin[:] = self.mpo_, self.mask_radius_, self.mask_origin_
        p.xlim = self.xlim_dev.data_ptr()
        if self.ws is None:
            n = int(self.L.akmi_mg_workspace_doubles(p))
            if n < 0:
                raise capi.AkmiError("mg_workspace_doubles: %s" % self.L.akmi_last_error().decode())
            self.ws = torch.zeros(n, dtype=torch.float64, device=self.device)
        p.ws = self.ws.data_ptr()

    def level_array(self, is_root, level, which):
        """a view of array `which` (0 u, 1 src, 2 def, 3 uold) of a level inside the workspace"""
        off = int(self.L.akmi_mg_level_offset(self.plan, int(is_root), level, which))
        if off < 0:
            raise capi.AkmiError("mg_level_offset: %s" % self.L.akmi_last_error().decode())
        s = self.nmblevel_ - 1 - level if not is_root else self.nrootlevel_ - 1 - level
        if is_root:
            sh = (1, 1, (self.nrbx[2] >> s) + 2, (self.nrbx[1] >> s) + 2, (self.nrbx[0] >> s) + 2)
        else:
            e = (self.plan.nxb >> s) + 2
            sh = (self.nmb, 1, e, e, e)
        return self.ws[off:off + int(np.prod(sh))].view(sh)

    def _multipole(self):
        """the 28 doubles the last Solve left in the workspace: 25 scaled coefficients, the origin"""
        if self.mg_bc_ != "multipole" or self.ws is None:
            raise RuntimeError("### FATAL ERROR the multipole coefficients need <gravity>/mg_bc = multipole and a Solve")
        off = int(self.L.akmi_mg_multipole_offset(self.plan))
        if off < 0:
            raise capi.AkmiError("mg_multipole_offset: %s" % self.L.akmi_last_error().decode())
        return self.ws[off:off + capi.MG_NMPCOEFF + 3].cpu().numpy()

    def mpcoeff(self):
        """mpcoeff_ after ScaleMultipoleCoefficients: 9 (mporder = 2) or 25 numbers; read back when asked for only"""
        return self._multipole()[:9 if self.mporder_ == 2 else capi.MG_NMPCOEFF].copy()

    def mporigin(self):
        """mpo_: the centre of mass under auto_mporigin, the deck's origin otherwise"""
        return self._multipole()[capi.MG_NMPCOEFF:].copy()

    def Solve(self, stage=0, pdriver=None):
        """MGGravityDriver::Solve, mg_gravity.cpp:177-245"""
        pk = self.pmy_pack
        fluid = pk.pmhd if pk.pmhd is not None else pk.phydro
        self._fill_plan(fluid)
        co = C.c_int(self.coffset_)
        capi.check(self.L.akmi_mg_solve(self.plan, fluid.u0, pk.pgrav.phi, C.byref(co), self.norms,
                                        C.byref(self.ncycles), capi._stream()), "mg_solve")
        self.coffset_ = co.value
        nrm = list(self.norms)
        self.last_norms = [v for v in nrm[:41] if v >= 0.0]
        if self.fshowdef_ >= 2 and self.last_norms:
            print("MG initial defect = %g" % self.last_norms[0])
            for n, v in enumerate(self.last_norms[1:]):
                print("MG iteration %d: defect = %g" % (n, v))
        if self.eps_ >= 0.0 and self.ncycles.value >= 40 and self.last_norms[-1] > self.eps_:
            # multigrid_driver.cpp:817-825: the run stops after this cycle
            print("### FATAL ERROR in MultigridDriver::SolveIterative\nFailed to converge after %d iterations (defect "
                  "= %g, threshold = %g)" % (self.ncycles.value, self.last_norms[-1], self.eps_))
            self.failed = True
            if pdriver is not None:
                pdriver.nlim = pk.pmesh.ncycle
        if self.fshowdef_ >= 1:
            print("MGGravityDriver::Solve: Final defect norm = %g" % nrm[41])


class Gravity:
    """gravity.cpp:33-66"""

    def __init__(self, ppack, pin, device=None):
        device = device or capi.DEVICE
        self.pmy_pack = ppack
        self.four_pi_G = pin.GetOrAddReal("gravity", "four_pi_G", -1.0)
        self.output_defect = pin.GetOrAddBoolean("gravity", "output_defect", False)
        self.fill_ghost = pin.GetOrAddBoolean("gravity", "fill_ghost", True)
        if self.four_pi_G == 0.0:
            _fatal("in Gravity::Gravity\nGravitational constant must be set in the Mesh::InitUserMeshData using the "
                   "SetGravitationalConstant or SetFourPiG function.")
        self.pmgd = MGGravityDriver(ppack, pin, device)
        n3, n2, n1 = ppack.pmesh.mb_indcs.ncells
        self.phi = torch.zeros((ppack.nmb_thispack, 1, n3, n2, n1), dtype=torch.float64, device=device)
