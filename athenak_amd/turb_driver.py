"""TurbulenceDriver -- driven turbulence, <turb_driving> (src/srcterms/turb_driver.cpp).

The random generator, the mode list, the amplitude table and the sin/cos tables are the host entries of
csrc/akmi_turb.hip (one implementation, shared with the C ABI); the force synthesis, the moments, the push and
the removal of the net momentum are its device entries.  Every global sum is the sum of per-MeshBlock partials
in gid order: each rank fills a K x nmb_total array with its blocks' partials at their gids and +inf elsewhere,
the array is reduced with all-reduce(min) (exact: min(x, +inf) = x), and every rank adds the same numbers in
the same order -- the result does not depend on the rank count.

Task placement (turb_driver.cpp:283-313, meshblock_pack.cpp:177-189): InitializeModes and AddForcing in
before_timeintegrator, and one more AddForcing in every stage between the fluxes and the RK update; each
AddForcing takes the OU step and pushes with the full pm.dt, as the reference does.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import capi
from .tasklist import TaskID, TaskStatus


def turb_deck_checks(pin):
    """what a deck with <turb_driving> may not combine it with (both hosts say the same)"""
    if not pin.DoesBlockExist("turb_driving"):
        return
    if pin.DoesBlockExist("mesh_refinement"):
        raise RuntimeError("### FATAL ERROR <turb_driving> is not available on refined meshes "
                           "(<mesh_refinement> in the input file)")
    if pin.DoesBlockExist("ion-neutral"):
        raise RuntimeError("### FATAL ERROR <turb_driving> with <ion-neutral> is not on this path")
    if pin.DoesBlockExist("hydro") and pin.DoesBlockExist("mhd"):
        raise RuntimeError("### FATAL ERROR <turb_driving> drives one fluid: <hydro> or <mhd>, not both")
    dtype = pin.GetOrAddInteger("turb_driving", "driving_type", 0)
    if dtype not in (0, 1):
        raise RuntimeError("### FATAL ERROR <turb_driving>/driving_type = %d: 0 (isotropic) or 1 "
                           "(anisotropic)" % dtype)


def gid_ordered_sums(partial, pack):
    """partial: (nmb_thispack, K) per-MeshBlock sums of this rank -> K Python floats, each the sum over all
    MeshBlocks of the mesh in gid order (sequential, from 0.0)"""
    pm = pack.pmesh
    part = np.asarray(partial, dtype=np.float64)
    K = part.shape[1]
    full = np.full((K, pm.nmb_total), np.inf)
    full[:, pack.gids:pack.gids + pack.nmb_thispack] = part.T
    if pm.nranks > 1:
        import torch.distributed as dist
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        t = torch.from_numpy(full).to(dev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        full = t.cpu().numpy()
    out = []
    for q in range(K):
        s = 0.0
        for g in range(pm.nmb_total):
            s += float(full[q, g])
        out.append(s)
    return out


def scale_factor(t0, t1, dedt, dt, gnx):
    """s of turb_driver.cpp:781-804 from the reduced sum rho|f|^2 (t0) and sum m.f (t1)"""
    t0 = max(t0, 1.0e-20)
    t1 = max(t1, 1.0e-20)
    m0, m1 = t0, t1
    dvol = 1.0/(gnx[0]*gnx[1]*gnx[2])
    m0 = 0.5*m0*dvol*dt
    m1 = m1*dvol
    if m1 >= 0:
        s = -m1/2./m0 + math.sqrt(m1*m1/4./m0/m0 + dedt/m0)
    else:
        s = m1/2./m0 + math.sqrt(m1*m1/4./m0/m0 + dedt/m0)
    if m0 == 0.0:
        s = 0.0
    return s


def ou_factors(dt, tcorr):
    """fcorr, gcorr of turb_driver.cpp:832-838"""
    if tcorr <= 1e-6:
        return 0.0, 1.0
    fcorr = math.exp(-dt/tcorr)
    return fcorr, math.sqrt(1.0 - fcorr*fcorr)


class TurbulenceDriver:
    """src/srcterms/turb_driver.hpp: force, force_tmp, rstate and the two task hooks"""

    def __init__(self, ppack, pin, device=None):
        """the deck has passed turb_deck_checks (MeshBlockPack.AddPhysics)"""
        self.pmy_pack = ppack
        self.device = device or capi.DEVICE
        self.L = capi.lib()
        g = "turb_driving"
        self.nlow = pin.GetOrAddInteger(g, "nlow", 1)
        self.nhigh = pin.GetOrAddInteger(g, "nhigh", 2)
        self.driving_type = pin.GetOrAddInteger(g, "driving_type", 0)
        self.expo = pin.GetOrAddReal(g, "expo", 5.0/3.0)
        self.exp_prp = pin.GetOrAddReal(g, "exp_prp", 5.0/3.0)
        self.exp_prl = pin.GetOrAddReal(g, "exp_prl", 0.0)
        self.dedt = pin.GetOrAddReal(g, "dedt", 0.0)
        self.tcorr = pin.GetOrAddReal(g, "tcorr", 0.0)
        pm = ppack.pmesh
        self.nmode = capi.check(self.L.akmi_turb_mode_count(self.nlow, self.nhigh, self.driving_type),
                                "turb_mode_count")
        ms = pm.mesh_size
        self.lens = (ms.x1max - ms.x1min, ms.x2max - ms.x2min, ms.x3max - ms.x3min)
        self.rstate = capi.RngState()
        self.rstate.idum = -1                         # Initialize(), turb_driver.cpp:167
        self.kvec = np.zeros((max(self.nmode, 1), 3))
        self._amplitudes(None, self.kvec)
        indcs = pm.mb_indcs
        nmb = ppack.nmb_thispack
        self.nmb = nmb
        nx = (indcs.nx1, indcs.nx2, indcs.nx3)
        bounds = np.array([[s.x1min, s.x1max, s.x2min, s.x2max, s.x3min, s.x3max] for s in ppack.pmb.mb_size],
                          dtype=np.float64)
        tabs = [np.zeros((nmb, max(self.nmode, 1), nx[d])) for d in (0, 0, 1, 1, 2, 2)]
        capi.check(self.L.akmi_turb_tables(nmb, self.nmode, nx[0], nx[1], nx[2], self.kvec.ctypes.data_as(C.c_void_p),
                                           bounds.ctypes.data_as(C.c_void_p),
                                           *[t.ctypes.data_as(C.c_void_p) for t in tabs]), "turb_tables")
        self.tables_host = tabs                       # xs, xc, ys, yc, zs, zc
        self.tables = [torch.from_numpy(t).to(self.device) for t in tabs]
        n3, n2, n1 = indcs.ncells
        self.force = torch.zeros((nmb, 3, n3, n2, n1), dtype=torch.float64, device=self.device)
        self.force_tmp = torch.zeros_like(self.force)
        self.partial = torch.zeros((nmb, 4), dtype=torch.float64, device=self.device)
        self.s = 0.0
        self.gnx = (pm.mesh_indcs.nx1, pm.mesh_indcs.nx2, pm.mesh_indcs.nx3)
        self.work = None

    # ---- pieces -------------------------------------------------------------------------
    def _amplitudes(self, amp, kvec=None):
        n = self.L.akmi_turb_amplitudes(
            self.nlow, self.nhigh, self.driving_type, self.expo, self.exp_prp, self.exp_prl, self.lens[0], self.lens[1],
            self.lens[2], C.byref(self.rstate), None if kvec is None else kvec.ctypes.data_as(C.c_void_p),
            None if amp is None else amp.ctypes.data_as(C.c_void_p))
        return capi.check(n, "turb_amplitudes")

    def _fluid(self):
        pk = self.pmy_pack
        return pk.phydro if pk.phydro is not None else pk.pmhd

    def _work(self, pack_c):
        if self.work is None:
            nbytes = int(self.L.akmi_turb_workspace_bytes(pack_c))
            self.work = torch.empty((nbytes + 7)//8, dtype=torch.float64, device=self.device)
        return self.work

    def _sums(self, K):
        # the entries write partial[m][K] contiguously
        return gid_ordered_sums(self.partial.flatten()[:self.nmb*K].reshape(self.nmb, K).cpu().numpy(), self.pmy_pack)

    # ---- tasks --------------------------------------------------------------------------
    def IncludeInitializeModesTask(self, tl, start):
        id_init = tl.AddTask(self.InitializeModes, start)
        tl.AddTask(self.AddForcing, id_init)

    def IncludeAddForcingTask(self, tl, start):
        f = self._fluid()
        return tl.InsertTask(self.AddForcing, f.id["flux"], f.id["rkupdt"])

    def InitializeModes(self, pdrive, stage):
        """turb_driver.cpp:320-814: new amplitudes, force_tmp, mean removed, scale s for dedt"""
        f = self._fluid()
        amp = np.zeros((max(self.nmode, 1), 24))
        self._amplitudes(amp)
        amp_dev = torch.from_numpy(amp).to(self.device)
        xs, xc, ys, yc, zs, zc = self.tables
        capi.check(self.L.akmi_turb_synthesize(
            f.pack_c, self.nmode, amp_dev, xs, xc, ys, yc, zs, zc, f.u0, self.force_tmp, self.partial,
            self._work(f.pack_c), capi._stream()), "turb_synthesize")
        t0, t1, t2, t3 = self._sums(4)
        capi.check(self.L.akmi_turb_moments(
            f.pack_c, t0, t1, t2, t3, f.u0, self.force_tmp, self.partial, self._work(f.pack_c), capi._stream()),
            "turb_moments")
        m0, m1 = self._sums(2)
        self.s = scale_factor(m0, m1, self.dedt, self.pmy_pack.pmesh.dt, self.gnx)
        return TaskStatus.complete

    def AddForcing(self, pdrive, stage):
        """turb_driver.cpp:819-1206, non-relativistic single-fluid branch"""
        f = self._fluid()
        dt = self.pmy_pack.pmesh.dt
        fcorr, gcorr = ou_factors(dt, self.tcorr)
        capi.check(self.L.akmi_turb_add_forcing(
            f.pack_c, fcorr, gcorr, self.s, dt, self.force_tmp, self.force, f.u0, self.partial, self._work(f.pack_c),
            capi._stream()), "turb_add_forcing")
        t0, t1, t2, t3 = self._sums(4)
        capi.check(self.L.akmi_turb_remove_net_mom(
            f.pack_c, t0, t1, t2, t3, f.u0, capi._stream()), "turb_remove_net_mom")
        return TaskStatus.complete


def add_turbulence_driver(ppack, pin):
    """MeshBlockPack::AddPhysics (6), meshblock_pack.cpp:177-189"""
    if not pin.DoesBlockExist("turb_driving"):
        return None
    pt = TurbulenceDriver(ppack, pin)
    none = TaskID(0)
    pt.IncludeInitializeModesTask(ppack.tl_map["before_timeintegrator"], none)
    pt.IncludeAddForcingTask(ppack.tl_map["stagen"], none)
    return pt
