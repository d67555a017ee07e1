"""ion_neutral::IonNeutral -- two-fluid (ion-neutral) MHD: an ion fluid (MHD) and a neutral fluid (hydro) on the same
mesh, coupled by a stiff drag term with optional ionization and recombination, integrated with the ImEx schemes
imex2, imex2+ and imex3.

Mirror of src/ion-neutral/ion-neutral.cpp:25-31 (the coefficients) and ion-neutral_tasks.cpp:30-292 (the task list,
FirstTwoImpRK, ImpRKUpdate).  The three passes of ImpRKUpdate are one launch of akmi_ionn_imp_update
(csrc/akmi_ionn.hip).
"""
import ctypes as C

from . import capi
from .tasklist import TaskID, TaskStatus

_DIFFUSION_KEYS = {"hydro": ("nu_iso", "nu_aniso", "alpha_iso", "alpha_aniso", "alpha_spitzer"),
                   "mhd": ("nu_iso", "nu_aniso", "alpha_iso", "alpha_aniso", "alpha_spitzer", "eta_ohm", "eta_ad")}


def ionn_deck_checks(pin, nranks=1):
    """what a deck with <ion-neutral> must hold and may not combine it with; called by MeshBlockPack.AddPhysics before
    any physics module is built.  Each message names the parameter."""
    if not pin.DoesBlockExist("ion-neutral"):
        return
    if not (pin.DoesBlockExist("hydro") and pin.DoesBlockExist("mhd")):          # meshblock_pack.cpp:150-155
        raise RuntimeError("### FATAL ERROR <ion-neutral> block detected in input file, but either <hydro> or <mhd> "
                           "also not specified")
    if nranks > 1:
        raise RuntimeError("### FATAL ERROR <ion-neutral> runs on one rank on this path (nranks=%d): the two-fluid task "
                           "list has not been run across ranks" % nranks)
    if pin.DoesBlockExist("mesh_refinement"):
        raise RuntimeError("### FATAL ERROR <ion-neutral> with <mesh_refinement> is not on this path: the implicit "
                           "update has not been carried through restriction, flux correction and prolongation")
    if pin.DoesBlockExist("turb_driving"):
        raise RuntimeError("### FATAL ERROR <ion-neutral> with <turb_driving> is not on this path")
    for blk in ("hydro", "mhd"):
        if pin.DoesBlockExist(blk + "_srcterms"):
            raise RuntimeError("### FATAL ERROR <ion-neutral> with <%s_srcterms> is not on this path" % blk)
        if pin.DoesParameterExist(blk, "fofc") and pin.GetBoolean(blk, "fofc"):
            raise RuntimeError("### FATAL ERROR <ion-neutral> with <%s>/fofc = true is not on this path: the first-order "
                               "flux correction reads the second register before FirstTwoImpRK has filled it" % blk)
        for key in _DIFFUSION_KEYS[blk]:
            if pin.DoesParameterExist(blk, key):
                raise RuntimeError("### FATAL ERROR <ion-neutral> with <%s>/%s is not on this path: the diffusion "
                                   "operators have not been run inside the two-fluid task list" % (blk, key))


class IonNeutral:
    def __init__(self, ppack, pin):
        self.pmy_pack = ppack
        self.drag_coeff = pin.GetReal("ion-neutral", "drag_coeff")
        self.ionization_coeff = pin.GetOrAddReal("ion-neutral", "ionization_coeff", 0.0)
        self.recombination_coeff = pin.GetOrAddReal("ion-neutral", "recombination_coeff", 0.0)
        self.L = capi.lib()
        self.id = {}

    # ---- task list assembly: ion-neutral_tasks.cpp:38-86 ---------------------------
    def AssembleIonNeutralTasks(self, tl):
        none = TaskID(0)
        pmhd, phyd = self.pmy_pack.pmhd, self.pmy_pack.phydro
        i = self.id
        b = tl["before_stagen"]
        i["i_irecv"] = b.AddTask(pmhd.InitRecv, none)
        i["n_irecv"] = b.AddTask(phyd.InitRecv, none)
        s = tl["stagen"]
        # FirstTwoImpRK does CopyCons
        i["impl_2x"] = s.AddTask(self.FirstTwoImpRK, none)
        i["i_flux"] = s.AddTask(pmhd.Fluxes, i["impl_2x"])
        i["i_sendf"] = s.AddTask(pmhd.SendFlux, i["i_flux"])
        i["i_recvf"] = s.AddTask(pmhd.RecvFlux, i["i_sendf"])
        i["i_rkupdt"] = s.AddTask(pmhd.RKUpdate, i["i_recvf"])
        i["i_srctrms"] = s.AddTask(pmhd.MHDSrcTerms, i["i_rkupdt"])
        i["n_flux"] = s.AddTask(phyd.Fluxes, i["i_srctrms"])
        i["n_sendf"] = s.AddTask(phyd.SendFlux, i["n_flux"])
        i["n_recvf"] = s.AddTask(phyd.RecvFlux, i["n_sendf"])
        i["n_rkupdt"] = s.AddTask(phyd.RKUpdate, i["n_recvf"])
        i["n_srctrms"] = s.AddTask(phyd.HydroSrcTerms, i["n_rkupdt"])
        i["impl"] = s.AddTask(self.ImpRKUpdate, i["n_srctrms"])
        i["i_restu"] = s.AddTask(pmhd.RestrictU, i["impl"])
        i["n_restu"] = s.AddTask(phyd.RestrictU, i["i_restu"])
        i["i_sendu"] = s.AddTask(pmhd.SendU, i["n_restu"])
        i["n_sendu"] = s.AddTask(phyd.SendU, i["n_restu"])
        i["i_recvu"] = s.AddTask(pmhd.RecvU, i["i_sendu"])
        i["n_recvu"] = s.AddTask(phyd.RecvU, i["n_sendu"])
        i["efld"] = s.AddTask(pmhd.EField, i["i_recvu"])
        i["sende"] = s.AddTask(pmhd.SendE, i["efld"])
        i["recve"] = s.AddTask(pmhd.RecvE, i["sende"])
        i["ct"] = s.AddTask(pmhd.CT, i["recve"])
        i["restb"] = s.AddTask(pmhd.RestrictB, i["ct"])
        i["sendb"] = s.AddTask(pmhd.SendB, i["restb"])
        i["recvb"] = s.AddTask(pmhd.RecvB, i["sendb"])
        i["i_bcs"] = s.AddTask(pmhd.ApplyPhysicalBCs, i["recvb"])
        i["n_bcs"] = s.AddTask(phyd.ApplyPhysicalBCs, i["n_recvu"])
        i["i_prol"] = s.AddTask(pmhd.Prolongate, i["i_bcs"])
        i["n_prol"] = s.AddTask(phyd.Prolongate, i["n_bcs"])
        i["i_c2p"] = s.AddTask(pmhd.ConToPrim, i["i_prol"])
        i["n_c2p"] = s.AddTask(phyd.ConToPrim, i["n_prol"])
        i["i_newdt"] = s.AddTask(pmhd.NewTimeStep, i["i_c2p"])
        i["n_newdt"] = s.AddTask(phyd.NewTimeStep, i["n_c2p"])
        a = tl["after_stagen"]
        i["i_clear"] = a.AddTask(pmhd.ClearSend, none)
        i["n_clear"] = a.AddTask(phyd.ClearSend, none)

    # ---- tasks ---------------------------------------------------------------------
    def FirstTwoImpRK(self, pdrive, stage):
        """ion-neutral_tasks.cpp:96-126: the first two, fully implicit stages; first task of the first stage only"""
        if stage != 1:
            return TaskStatus.complete
        pmhd, phyd = self.pmy_pack.pmhd, self.pmy_pack.phydro
        phyd.u1.copy_(phyd.u0)
        pmhd.u1.copy_(pmhd.u0)
        pmhd.b1.x1f.copy_(pmhd.b0.x1f)
        pmhd.b1.x2f.copy_(pmhd.b0.x2f)
        pmhd.b1.x3f.copy_(pmhd.b0.x3f)
        self.ImpRKUpdate(pdrive, -1)
        self.ImpRKUpdate(pdrive, 0)
        # primitives of both fluids over all cells (the ConToPrim tasks of a task-granular fluid do exactly that)
        phyd.ConToPrim(pdrive, 0)
        pmhd.ConToPrim(pdrive, 0)
        return TaskStatus.complete

    def imp_coefficients(self, pdrive, estage, dt):
        """the host side of ImpRKUpdate: (istage, do_solve, adt[istage-1], gamma_adt, xi_adt, alpha_adt), all in double
        (ion-neutral_tasks.cpp:147,171,189-203)"""
        istage = estage + 2
        adt = [pdrive.a_twid[istage - 2][s]*dt for s in range(istage - 1)]
        do_solve = estage < pdrive.nexp_stages
        if istage < 3 and pdrive.integrator == "imex2+":
            gamma_adt = xi_adt = alpha_adt = 0.0
        else:
            gamma_adt = self.drag_coeff*(pdrive.a_impl)*(dt)
            xi_adt = self.ionization_coeff*(pdrive.a_impl)*(dt)
            alpha_adt = self.recombination_coeff*(pdrive.a_impl)*(dt)
        return istage, do_solve, adt, gamma_adt, xi_adt, alpha_adt

    def ImpRKUpdate(self, pdrive, estage):
        """ion-neutral_tasks.cpp:144-292: estage = -1, 0 (FirstTwoImpRK), then the explicit stage 1 .. nexp_stages"""
        pmhd, phyd = self.pmy_pack.pmhd, self.pmy_pack.phydro
        n3, n2, n1 = self.pmy_pack.pmesh.mb_indcs.ncells
        istage, do_solve, adt, g_adt, xi_adt, al_adt = self.imp_coefficients(pdrive, estage, self.pmy_pack.pmesh.dt)
        ru = pdrive.impl_src
        if ru is None:
            raise RuntimeError("### FATAL ERROR ImpRKUpdate before Driver.Initialize has allocated impl_src")
        assert ru.shape[1] == self.pmy_pack.nmb_thispack, (ru.shape, self.pmy_pack.nmb_thispack)
        adt_c = (C.c_double*max(len(adt), 1))(*adt)
        capi.check(self.L.akmi_ionn_imp_update(
            self.pmy_pack.nmb_thispack, n3*n2*n1, pmhd.nvars, phyd.nvars, pdrive.nimp_stages, istage,
            1 if do_solve else 0, adt_c, g_adt, xi_adt, al_adt, self.drag_coeff, self.ionization_coeff,
            self.recombination_coeff, pmhd.u0, phyd.u0, ru, capi._stream()), "ionn_imp_update")
        return TaskStatus.complete
