"""Driver: RK stage tables and the main loop over task lists.

Mirror of src/driver/driver.cpp:93-162 (RK weights), :163-273 (ImEx tables), :290-307 (ExecuteTaskList), :314-371
(Initialize), :380-459 (Execute), :569-653 (InitBoundaryValuesAndPrimitives).
"""
import time as _time

from .tasklist import TaskListStatus


class Driver:
    def __init__(self, pin, pmesh):
        self.time_evolution = pin.GetOrAddString("time", "evolution", "dynamic")
        if self.time_evolution not in ("dynamic", "kinematic"):
            raise RuntimeError("### FATAL ERROR <time> evolution = '%s' is not on this path "
                               "(dynamic, kinematic)" % self.time_evolution)
        self.integrator = pin.GetOrAddString("time", "integrator", "rk2")
        self.tlim = pin.GetReal("time", "tlim")
        self.nlim = pin.GetOrAddInteger("time", "nlim", -1)
        self.ndiag = pin.GetOrAddInteger("time", "ndiag", 1)
        self.gam0, self.gam1, self.beta, self.delta = [0.0]*4, [0.0]*4, [0.0]*4, [0.0]*4
        self.nimp_stages, self.a_impl, self.gamma = 0, 0.0, 0.0
        self.a_twid = [[0.0]*4 for _ in range(4)]
        if self.integrator == "rk1":
            self.nexp_stages, self.cfl_limit = 1, 1.0
            self.gam0[0], self.gam1[0], self.beta[0] = 0.0, 1.0, 1.0
        elif self.integrator == "rk2":
            self.nexp_stages, self.cfl_limit = 2, 1.0
            self.gam0[0], self.gam1[0], self.beta[0] = 0.0, 1.0, 1.0
            self.gam0[1], self.gam1[1], self.beta[1] = 0.5, 0.5, 0.5
        elif self.integrator == "rk3":
            self.nexp_stages, self.cfl_limit = 3, 1.0
            self.gam0[0], self.gam1[0], self.beta[0] = 0.0, 1.0, 1.0
            self.gam0[1], self.gam1[1], self.beta[1] = 0.25, 0.75, 0.25
            self.gam0[2], self.gam1[2], self.beta[2] = 2.0/3.0, 1.0/3.0, 2.0/3.0
        elif self.integrator == "rk4":
            # RK4()4[2S] of Ketcheson (2010), driver.cpp:131-160
            self.nexp_stages, self.cfl_limit = 4, 1.3925
            self.gam0[0], self.gam1[0], self.beta[0] = 0.0, 1.0, 1.193743905974738
            self.gam0[1], self.gam1[1], self.beta[1] = (0.121098479554482, 0.721781678111411,
                                                        0.099279895495783)
            self.gam0[2], self.gam1[2], self.beta[2] = (-3.843833699660025, 2.121209265338722,
                                                        1.131678018054042)
            self.gam0[3], self.gam1[3], self.beta[3] = (0.546370891121863, 0.198653035682705,
                                                        0.310665766509336)
            self.delta = [1.0, 0.217683334308543, 1.065841341361089, 0.0]
        elif self.integrator in ("imex2", "imex2+", "imex3"):
            self._imex_tables()
        else:
            raise RuntimeError("### FATAL ERROR integrator=%s not implemented. Valid choices on "
                               "this path are [rk1,rk2,rk3,rk4,imex2,imex2+,imex3]." % self.integrator)
        # the ImEx integrators treat the stiff drag term of two-fluid MHD and nothing else (driver.cpp:352-368)
        ionn = pin.DoesBlockExist("ion-neutral")
        if self.nimp_stages > 0 and not ionn:
            raise RuntimeError("### FATAL ERROR integrator=%s is an ImEx integrator: it needs the <ion-neutral> block "
                               "(two-fluid MHD). Valid choices without it are [rk1,rk2,rk3,rk4]." % self.integrator)
        if ionn and self.nimp_stages == 0:
            raise RuntimeError("### FATAL ERROR IonNeutral MHD can only be run with ImEx integrators.")
        self.impl_src = None
        self.nmb_updated_ = 0
        self.run_time_ = 0.0

    def _imex_tables(self):
        """driver.cpp:163-273.  Stage 1 has gam0 = 1, gam1 = 0 (not the 0, 1 of rk*): u0 has been through the first two
        implicit stages by then and u1 has not."""
        at = self.a_twid
        if self.integrator == "imex2":
            # IMEX-SSP2(3,2,2): Pareschi & Russo (2005) Table III; explicit steps identical to RK2
            self.nimp_stages, self.nexp_stages, self.cfl_limit = 3, 2, 1.0
            self.gam0[0], self.gam1[0], self.beta[0] = 1.0, 0.0, 1.0
            self.gam0[1], self.gam1[1], self.beta[1] = 0.5, 0.5, 0.5
            at[0][0], at[0][1], at[0][2] = -1.0, 0.0, 0.0
            at[1][0], at[1][1], at[1][2] = 0.5, 0.0, 0.0
            at[2][0], at[2][1], at[2][2] = 0.0, 0.25, 0.25
            self.a_impl = 0.5
        elif self.integrator == "imex2+":
            # IMEX(4,3,2): Krapp et al. (2024, arXiv:2310.04435), Eq. 30
            self.nimp_stages, self.nexp_stages, self.cfl_limit = 4, 3, 1.0
            self.gamma = gamma = 1.707106781186547   # 1+1/sqrt(2)
            self.gam0[0], self.gam1[0], self.beta[0] = 1.0, 0.0, gamma
            self.gam0[1] = (2.0*gamma - 1.0)/(2.0*gamma*gamma)
            self.gam1[1] = (1.0 - (2.0*gamma - 1.0)/(2.0*gamma*gamma))
            self.beta[1] = 1.0/(2.0*gamma)
            self.gam0[2], self.gam1[2], self.beta[2] = 1.0, 0.0, 0.0
            at[2][2] = (1.0 - 2.0*gamma*gamma)/2.0/gamma         # every other entry is 0.0
            self.a_impl = gamma
        else:
            # IMEX-SSP3(4,3,3): Pareschi & Russo (2005) Table VI; explicit steps identical to RK3
            self.nimp_stages, self.nexp_stages, self.cfl_limit = 4, 3, 1.0
            self.gam0[0], self.gam1[0], self.beta[0] = 1.0, 0.0, 1.0
            self.gam0[1], self.gam1[1], self.beta[1] = 0.25, 0.75, 0.25
            self.gam0[2], self.gam1[2], self.beta[2] = 2.0/3.0, 1.0/3.0, 2.0/3.0
            a, b, e = 0.24169426078821, 0.06042356519705, 0.12915286960590
            at[0][0] = -2.0*a
            at[1][0], at[1][1] = a, 1.0 - 2.0*a
            at[2][0], at[2][1], at[2][2] = b, e - ((1.0 - a)/4.0), 0.5 - b - e - 1.25*a
            at[3][0], at[3][1] = (-2.0/3.0)*b, (1.0 - 4.0*e)/6.0
            at[3][2], at[3][3] = (4.0*(b + e + a) - 1.0)/6.0, 2.0*(1.0 - a)/3.0
            self.a_impl = a

    def ExecuteTaskList(self, pm, tl, stage):
        """driver.cpp:290-307 (one pack per rank)"""
        pmbp = pm.pmb_pack
        tlist = pmbp.tl_map[tl]
        if tlist.Empty():
            return
        tlist.Reset()
        while not tlist.IsComplete():
            if tlist.DoAvailable(self, stage) == TaskListStatus.complete:
                break

    def InitBoundaryValuesAndPrimitives(self, pm):
        """driver.cpp:569-653: one halo exchange + BCs + c2p everywhere"""
        self._begin_stage(pm)
        ph = pm.pmb_pack.phydro
        if ph is not None:
            ph.RestrictU(self, 0)
            ph.InitRecv(self, -1)
            ph.SendU(self, 0)
            ph.ClearSend(self, -1)
            ph.ClearRecv(self, -1)
            ph.RecvU(self, 0)
            ph.SendU_Shr(self, 0)              # driver.cpp:597-600: the shear-periodic x1 faces at the start time
            ph.RecvU_Shr(self, 0)
            ph.Prolongate(self, 0)
            ph.ApplyPhysicalBCs(self, 0)
            ph.ConToPrim(self, 0)
        pmhd = pm.pmb_pack.pmhd
        if pmhd is not None:
            pmhd.RestrictU(self, 0)
            pmhd.RestrictB(self, 0)
            pmhd.InitRecv(self, -1)
            pmhd.SendU(self, 0)
            pmhd.RecvU(self, 0)
            pmhd.SendB(self, 0)
            pmhd.RecvB(self, 0)
            pmhd.ClearSend(self, -1)
            pmhd.ClearRecv(self, -1)
            pmhd.SendU_Shr(self, 0)            # driver.cpp:620-625: the shear-periodic x1 faces at the start time
            pmhd.SendB_Shr(self, 0)
            pmhd.RecvU_Shr(self, 0)
            pmhd.RecvB_Shr(self, 0)
            pmhd.Prolongate(self, 0)
            pmhd.ApplyPhysicalBCs(self, 0)
            pmhd.ConToPrim(self, 0)

    def Initialize(self, pm, pin=None, pout=None, res_flag=False):
        """driver.cpp:314-371; with pout: the initial outputs (driver.cpp:340-346), which a restarted
        run does not repeat"""
        self.pout, self.pin_ = pout, pin
        self.InitBoundaryValuesAndPrimitives(pm)
        ph, pmhd = pm.pmb_pack.phydro, pm.pmb_pack.pmhd
        if ph is not None:
            ph.NewTimeStep(self, self.nexp_stages)
        if pmhd is not None:
            pmhd.NewTimeStep(self, self.nexp_stages)
        pm.NewTimeStep(self.tlim)
        self.nmb_updated_ = 0
        if pout is not None and not res_flag:
            pout.MakeOutputs(pm, pin)
        # stiff source terms of the ImEx integrators (driver.cpp:352-368): (nimp_stages, nmb, 8, n3, n2, n1)
        if getattr(pm.pmb_pack, "pionn", None) is not None and self.impl_src is None:
            import torch
            n3, n2, n1 = pm.mb_indcs.ncells
            nmb = max(pm.pmb_pack.nmb_thispack, pm.nmb_maxperrank)
            self.impl_src = torch.zeros((self.nimp_stages, nmb, 8, n3, n2, n1), dtype=torch.float64,
                                        device=pm.pmb_pack.pmhd.u0.device)

    @staticmethod
    def _begin_stage(pm):
        """FluidBase.BeginStage of every fluid: no hand-shake flag of one stage is left standing for the next"""
        for ph in (pm.pmb_pack.phydro, pm.pmb_pack.pmhd):
            if ph is not None:
                ph.BeginStage()

    def _cycle(self, pm):
        self.ExecuteTaskList(pm, "before_timeintegrator", 0)
        for stage in range(1, self.nexp_stages + 1):
            self._begin_stage(pm)
            self.ExecuteTaskList(pm, "before_stagen", stage)
            if pm.pmb_pack.pgrav is not None:                          # driver.cpp:403-411: every stage, not at t = 0
                pm.pmb_pack.pgrav.pmgd.Solve(stage, self)
            self.ExecuteTaskList(pm, "stagen", stage)
            self.ExecuteTaskList(pm, "after_stagen", stage)
        self.ExecuteTaskList(pm, "after_timeintegrator", 1)
        pm.time = pm.time + pm.dt
        pm.ncycle += 1
        self.nmb_updated_ += pm.nmb_total
        if getattr(self, "pout", None) is not None:
            self.pout.TestAndMakeOutputs(pm, self.pin_, self.tlim)     # driver.cpp:432-445
        if pm.adaptive:                                                # driver.cpp:447-450
            pm.pmr.AdaptiveMeshRefinement(self, getattr(self, "pin_", None))
        pm.NewTimeStep(self.tlim)

    def Finalize(self, pm, pin, pout=None):
        """driver.cpp:467-500: final outputs, then the problem generator's final work (the
        linear-wave error file)"""
        if pout is not None:
            pout.MakeOutputs(pm, pin)
        if pm.pgen is not None and pm.pgen.pgen_final_func is not None:
            pm.pgen.write_errors_file = True
            errs = pm.pgen.pgen_final_func()
            pm.pgen.write_errors_file = False
            return errs
        return None

    def Execute(self, pm, pin=None, max_cycles=None):
        """driver.cpp:380-459; returns cycles executed by this call"""
        n = 0
        t0 = _time.time()
        while (pm.time < self.tlim) and (pm.ncycle < self.nlim or self.nlim < 0):
            if max_cycles is not None and n >= max_cycles:
                break
            self._cycle(pm)
            n += 1
        self.run_time_ += _time.time() - t0
        return n

    def zone_cycles_per_second(self, pm):
        """driver.cpp:513-522"""
        return self.nmb_updated_*pm.NumberOfMeshBlockCells()/max(self.run_time_, 1e-30)
