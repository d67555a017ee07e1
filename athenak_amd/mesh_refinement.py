"""MeshRefinement: adaptive mesh refinement on one rank.

Host-side restatement of src/mesh/refinement_criteria.cpp:28-108,345-386 (the <amr_criterion*> blocks and the
location criterion) and of src/mesh/mesh_refinement.cpp: AdaptiveMeshRefinement :145-188, CheckForRefinement :196-267,
UpdateMeshBlockTree :274-416, RedistAndRefineMeshBlocks :427-687, RepairAMRFC :1189-1220.  The two device pieces are
csrc/akmi_amr.hip: akmi_amr_check (one launch per criterion, flags updated on the device, one read-back per check) and
akmi_amr_regrid_cc / _fc / akmi_amr_repair_fc.  The regrid is out of place, from the old arrays into those of the fluid
objects rebuilt for the new mesh, so the reference's move-left / move-right ordering of in-place copies (:817-910) has
no counterpart here.  Everything downstream of a regrid is the path of a statically refined mesh.
"""
import numpy as np
import torch

from . import capi
from .mesh import FLT_MAX, LoadBalance

_METHODS = ("min_max", "slope", "second_deriv", "location")
_VARIABLES = ("hydro_u_d", "hydro_w_d", "mhd_u_d", "mhd_w_d")


class RefCritData:
    """refinement_criteria.hpp: one <amr_criterion*> block"""

    def __init__(self, pin, blk):
        self.block = blk
        self.method = pin.GetString(blk, "method")
        if self.method == "user":
            raise RuntimeError("### FATAL ERROR <%s>/method = user: user-defined refinement functions are not on "
                               "this path (supported: %s)" % (blk, ", ".join(_METHODS)))
        if self.method not in _METHODS:
            raise RuntimeError("### FATAL ERROR Unknown refinement criterion '%s' in <%s> (supported: %s)"
                               % (self.method, blk, ", ".join(_METHODS)))
        self.variable = None
        if self.method != "location":
            self.variable = pin.GetString(blk, "variable")
            if self.variable not in _VARIABLES:
                raise RuntimeError("### FATAL ERROR Unknown refinement variable '%s' requested in <%s> (supported: %s)"
                                   % (self.variable, blk, ", ".join(_VARIABLES)))
        self.value_min = pin.GetOrAddReal(blk, "value_min", -FLT_MAX)
        self.value_max = pin.GetOrAddReal(blk, "value_max", FLT_MAX)
        self.loc = [pin.GetOrAddReal(blk, "location_x%d" % q, 0.0) for q in (1, 2, 3)]
        self.rad = pin.GetOrAddReal(blk, "location_rad", 0.0)


def old_to_new(newtoold, old_nmb, nleaf):
    """mesh_refinement.cpp:450-469: per old gid the new gid -- of the block itself, of the first child of a refined
    block, of the block a derefined group merged into"""
    new_nmb = len(newtoold)
    oldtonew = [0]*old_nmb
    idx = 1
    for n in range(1, new_nmb):
        if newtoold[n] == newtoold[n - 1] + 1:                     # normal
            oldtonew[idx] = n
            idx += 1
        elif newtoold[n] == newtoold[n - 1] + nleaf:               # derefined
            for _ in range(nleaf - 1):
                oldtonew[idx] = n - 1
                idx += 1
            oldtonew[idx] = n
            idx += 1
    while idx < old_nmb:                                           # fill the last block
        oldtonew[idx] = new_nmb - 1
        idx += 1
    return oldtonew


def level_change_flags(old_lloc, new_lloc, oldtonew, nleaf):
    """mesh_refinement.cpp:495-506: refine_flag reset from what happened to every old block (+1 refined, -nleaf
    derefined, 0 kept), whoever flagged it"""
    rf = np.zeros(len(old_lloc), dtype=np.int32)
    for oldm, l in enumerate(old_lloc):
        ol, nl = l.level, new_lloc[oldtonew[oldm]].level
        rf[oldm] = -nleaf if ol > nl else (1 if ol < nl else 0)
    return rf


def regrid_plan(newtoold, refine_flag, new_lloc):
    """(nmb_new, 3) int32 rows {kind, old, octant} of include/akmi.h from the new-to-old list and the flags reset from
    the level changes (+1 refined, -nleaf derefined, 0 kept)"""
    rows = np.zeros((len(newtoold), 3), dtype=np.int32)
    for newm, oldm in enumerate(newtoold):
        f = refine_flag[oldm]
        if f > 0:
            l = new_lloc[newm]
            rows[newm] = (1, oldm, (l.lx1 & 1) + 2*(l.lx2 & 1) + 4*(l.lx3 & 1))
        elif f < -1:
            rows[newm] = (-1, oldm, 0)
        else:
            rows[newm] = (0, oldm, 0)
    return rows


class MeshRefinement:
    def __init__(self, pm, pin):
        self.pmy_mesh = pm
        self.pin = pin
        pk = pm.pmb_pack
        self.ncyc_check_amr = pin.GetOrAddInteger("mesh_refinement", "ncycle_check", 1)
        self.refinement_interval = pin.GetOrAddInteger("mesh_refinement", "refinement_interval", 5)
        self.rcrit = [RefCritData(pin, b) for b in pin.blocks if b.startswith("amr_criterion")]
        if not self.rcrit:
            raise RuntimeError("### FATAL ERROR No <amr_criterion> blocks were found in input file")
        for c in self.rcrit:
            if c.variable and c.variable.startswith("hydro") and pk.phydro is None:
                raise RuntimeError("### FATAL ERROR Hydro refinement variable used but <hydro> not defined")
            if c.variable and c.variable.startswith("mhd") and pk.pmhd is None:
                raise RuntimeError("### FATAL ERROR MHD refinement variable used but <mhd> not defined")
        # what this path does not carry across a regrid, said before anything runs
        for b, d in pin.blocks.items():
            if b.startswith("output") and d.get("file_type") == "rst":
                raise RuntimeError("### FATAL ERROR <%s>/file_type = rst in a deck with refinement = adaptive: the "
                                   "restart reader rebuilds the mesh from the deck, not from the file" % b)
        self.nleaf = 1 << (3 if pm.three_d else (2 if pm.multi_d else 1))
        self.refine_flag = np.zeros(pm.nmb_total, dtype=np.int32)
        self.ncyc_since_ref = np.zeros(pm.nmb_total, dtype=np.int64)
        self.fc_amr_repair = np.zeros(pm.nmb_total, dtype=np.int32)
        self.nmb_created = 0
        self.nmb_deleted = 0
        self.newtoold = self.oldtonew = None

    # ---- criteria ------------------------------------------------------------------------------------------
    def _variable(self, pk, name):
        ph = pk.phydro if name.startswith("hydro") else pk.pmhd
        return ph, (ph.u0 if name.endswith("_u_d") else ph.w0)

    def _location_mask(self, pk, c):
        """refinement_criteria.cpp:345-386: any part of the MeshBlock within rad of the position"""
        pm = self.pmy_mesh
        mask = np.zeros(pk.nmb_thispack, dtype=bool)

        def near(lo, hi, x):
            return ((lo < x + c.rad and lo > x - c.rad) or (hi < x + c.rad and hi > x - c.rad)
                    or (hi > x + c.rad and lo < x - c.rad))
        for m, s in enumerate(pk.pmb.mb_size):
            mask[m] = (near(s.x1min, s.x1max, c.loc[0]) and (not pm.multi_d or near(s.x2min, s.x2max, c.loc[1]))
                       and (not pm.three_d or near(s.x3min, s.x3max, c.loc[2])))
        return mask

    def CheckForRefinement(self, pk):
        """mesh_refinement.cpp:196-267"""
        pm = self.pmy_mesh
        self.refine_flag = np.zeros(pm.nmb_total, dtype=np.int32)
        self.ncyc_since_ref += 1
        if pm.ncycle % self.ncyc_check_amr != 0:
            return
        ph0 = pk.phydro if pk.phydro is not None else pk.pmhd
        flags = torch.zeros(pk.nmb_thispack, dtype=torch.int32, device=ph0.device)
        for c in self.rcrit:                      # in the deck's order: a later criterion sees the earlier flags
            if c.method == "location":
                flags[torch.from_numpy(self._location_mask(pk, c)).to(flags.device)] = 1
                continue
            ph, q = self._variable(pk, c.variable)
            capi.check(ph.L.akmi_amr_check(ph.pack_c, capi.AMR_METHOD[c.method], q, q.stride(0), c.value_min,
                                           c.value_max, flags, capi._stream()), "amr_check")
        rf = flags.cpu().numpy()                  # the one device-to-host copy of a check
        for m in range(pk.nmb_thispack):
            lev = pm.lloc_eachmb[m + pk.gids].level
            if lev == pm.max_level and rf[m] > 0:
                rf[m] = 0
            if lev == pm.root_level and rf[m] < 0:
                rf[m] = 0
            if self.ncyc_since_ref[m + pk.gids] < self.refinement_interval:
                rf[m] = 0
        self.refine_flag[pk.gids:pk.gids + pk.nmb_thispack] = rf

    # ---- tree ----------------------------------------------------------------------------------------------
    def UpdateMeshBlockTree(self):
        """mesh_refinement.cpp:274-416 on one rank -> (nnew, ndel)"""
        pm = self.pmy_mesh
        nleaf = self.nleaf
        rf = self.refine_flag
        llref = [pm.lloc_eachmb[g] for g in range(pm.nmb_total) if rf[g] == 1]
        llderef = [pm.lloc_eachmb[g] for g in range(pm.nmb_total) if rf[g] == -1]
        if not llref and len(llderef) < nleaf:
            return 0, 0
        if len(llderef) < nleaf:
            llderef = []
        # sibling groups: found from the even-indexed block; all nleaf must follow it in the list, on its level
        cllderef = []
        lk, lj = (1 if pm.three_d else 0), (1 if pm.multi_d else 0)
        for n, l0 in enumerate(llderef):
            if (l0.lx1 & 1) or (l0.lx2 & 1) or (l0.lx3 & 1):
                continue
            r, rr = n, 0
            for k in range(lk + 1):
                for j in range(lj + 1):
                    for i in range(2):
                        if r < len(llderef):
                            l = llderef[r]
                            if (l0.lx1 + i == l.lx1 and l0.lx2 + j == l.lx2 and l0.lx3 + k == l.lx3
                                    and l0.level == l.level):
                                rr += 1
                            r += 1
            if rr == nleaf:
                cllderef.append(type(l0)(l0.lx1 >> 1, l0.lx2 >> 1, l0.lx3 >> 1, l0.level - 1))
        # deeper levels first -- but the reference's std::sort(cllderef, &cllderef[ctnd-1], GreaterLevel) takes its end
        # iterator one short, so the LAST coarse location keeps its place whatever its level; restated as it is.
        # (Among equal levels the order cannot matter: a derefinement is vetoed by leaves two levels below its own,
        # which no derefinement of the same level removes.)
        if len(cllderef) > 1:
            cllderef = sorted(cllderef[:-1], key=lambda l: -l.level) + cllderef[-1:]
        nnew, ndel = [0], [0]
        for l in llref:                                        # refinements first
            pm.ptree.Refine(pm.ptree.FindMeshBlock(l), nnew)
        for l in cllderef:                                     # derefinements second
            pm.ptree.Derefine(pm.ptree.FindMeshBlock(l), ndel)
        return nnew[0], ndel[0]

    # ---- regrid --------------------------------------------------------------------------------------------
    def RedistAndRefineMeshBlocks(self, pin, nnew, ndel):
        """mesh_refinement.cpp:427-687 on one rank"""
        pm = self.pmy_mesh
        pk = pm.pmb_pack
        nleaf = self.nleaf
        old_nmb = pm.nmb_total
        new_nmb = old_nmb + nnew - ndel
        newtoold = []
        new_lloc = pm.ptree.CreateZOrderedLLList(newtoold)
        if len(new_lloc) != new_nmb:
            raise RuntimeError("### FATAL ERROR Number of MeshBlocks in new tree = %d but expected value = %d"
                               % (len(new_lloc), new_nmb))
        oldtonew = old_to_new(newtoold, old_nmb, nleaf)
        cost = [1.0]*new_nmb
        rank_eachmb, gids_eachrank, nmb_eachrank = LoadBalance(cost, pm.nranks)
        if nmb_eachrank[pm.my_rank] > pm.nmb_maxperrank:
            raise RuntimeError("### FATAL ERROR Number of MeshBlocks in this rank on new tree = %d on rank = %d exceeds "
                               "<mesh_refinement>/max_nmb_per_rank = %d"
                               % (nmb_eachrank[pm.my_rank], pm.my_rank, pm.nmb_maxperrank))
        # the 2:1 rule refines blocks nobody flagged: reset the flags from what happened to every block
        rf = level_change_flags(pm.lloc_eachmb, new_lloc, oldtonew, nleaf)
        self.refine_flag = rf
        self.newtoold, self.oldtonew = newtoold, oldtonew
        plan = regrid_plan(newtoold, rf, new_lloc)
        ncyc = np.array([0 if rf[o] != 0 else self.ncyc_since_ref[o] for o in newtoold], dtype=np.int64)
        self.fc_amr_repair = np.array([1 if rf[o] != 0 else 0 for o in newtoold], dtype=np.int32)
        self.ncyc_since_ref = ncyc
        # the new mesh
        pm.lloc_eachmb = new_lloc
        pm.gid_of_lloc = {tuple(l): i for i, l in enumerate(new_lloc)}
        pm.rank_eachmb, pm.cost_eachmb = rank_eachmb, cost
        pm.gids_eachrank, pm.nmb_eachrank = gids_eachrank, nmb_eachrank
        pm.nmb_total = new_nmb
        pm.nmb_thisrank = nmb_eachrank[pm.my_rank]
        old_h, old_m = pk.phydro, pk.pmhd
        pk.RebuildAfterRegrid(pin)
        # the evolved arrays of the new mesh from those of the old one
        dev = (old_h or old_m).device
        plan_dev = torch.from_numpy(plan).to(dev)
        for old, new in ((old_h, pk.phydro), (old_m, pk.pmhd)):
            if old is None:
                continue
            capi.check(new.L.akmi_amr_regrid_cc(old.pack_c, new.pack_c, new.nvars, plan_dev, old.u0, new.u0,
                                                capi._stream()), "amr_regrid_cc")
            new.counters.copy_(old.counters)
            if getattr(old, "use_fofc", False):
                new.nfofc.copy_(old.nfofc)
        if old_m is not None:
            ob, nb = old_m.b0, pk.pmhd.b0
            capi.check(pk.pmhd.L.akmi_amr_regrid_fc(
                old_m.pack_c, pk.pmhd.pack_c, plan_dev, ob.x1f, ob.x2f, ob.x3f, nb.x1f, nb.x2f, nb.x3f, capi._stream()),
                "amr_regrid_fc")
        if dev != "cpu" and torch.cuda.is_available():
            torch.cuda.current_stream().synchronize()          # the old arrays and the plan are released on return

    def RepairAMRFC(self, pmhd):
        """mesh_refinement.cpp:1189-1220: internal faces of every refined or derefined block, from exterior faces the
        boundary exchange has finalized"""
        rep = torch.from_numpy(self.fc_amr_repair).to(pmhd.device)
        b = pmhd.b0
        capi.check(pmhd.L.akmi_amr_repair_fc(pmhd.pack_c, rep, b.x1f, b.x2f, b.x3f, capi._stream()), "amr_repair_fc")
        if pmhd.device != "cpu" and torch.cuda.is_available():
            torch.cuda.current_stream().synchronize()

    def AdaptiveMeshRefinement(self, pdriver, pin=None):
        """mesh_refinement.cpp:145-188; returns True when the mesh changed"""
        pm = self.pmy_mesh
        pin = pin or self.pin
        self.CheckForRefinement(pm.pmb_pack)
        nnew, ndel = self.UpdateMeshBlockTree()
        if nnew == 0 and ndel == 0:
            return False
        self.RedistAndRefineMeshBlocks(pin, nnew, ndel)
        pdriver.InitBoundaryValuesAndPrimitives(pm)
        pk = pm.pmb_pack
        if pk.pmhd is not None:
            self.RepairAMRFC(pk.pmhd)
            pdriver.InitBoundaryValuesAndPrimitives(pm)
        if pk.phydro is not None:
            pk.phydro.NewTimeStep(pdriver, pdriver.nexp_stages)
        if pk.pmhd is not None:
            pk.pmhd.NewTimeStep(pdriver, pdriver.nexp_stages)
        self.nmb_created += nnew
        self.nmb_deleted += ndel
        return True
