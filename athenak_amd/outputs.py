"""Outputs: the data formats on the far side of the hot path, written so that the reference's
own readers (vis/python/athena_read.py tab()/hst()/error_dat(), bin_convert.read_binary())
parse them unchanged.

Mirrors, for the file types a hydro/MHD run of this path uses:
  Outputs                src/outputs/outputs.cpp:47-304      (<outputN> blocks -> pout_list)
  BaseTypeOutput         src/outputs/basetype_output.cpp     (variable groups, slices, gather)
  FormattedTableOutput   src/outputs/formatted_table.cpp     (tab/<basename>.<id>.NNNNN.tab)
  HistoryOutput          src/outputs/history.cpp             (<basename>.hydro|mhd.hst, <basename>.user.hst)
  PDFOutput              src/outputs/pdf.cpp                 (pdf_<id>[_<variable_2>]/<basename>.bins.pdf, .NNNNN.pdf)
  MeshBinaryOutput       src/outputs/binary.cpp              (bin/<basename>.<id>.NNNNN.bin)
  CoarsenedBinaryOutput  src/outputs/coarsened_binary.cpp    (cbin_<id>_<f>/<basename>.<id>.NNNNN.cbin)
  RestartOutput          src/outputs/restart.cpp             (rst/<basename>.NNNNN.rst) + read_restart()
The volume sums of the history file (akmi_history_sums), the turbulence history columns of a driven MHD run with
<problem>/user_hist = true (akmi_turb_history), the histograms of the pdf outputs (akmi_pdf) and the cell averages and
moments of the cbin outputs (akmi_coarsen) are reduced on the device; everything else here is host-side formatting of
arrays copied from the device.  Other file types of the reference (vtk, cart, sph, log, trk) are rejected loudly.
"""
import ctypes as C
import os
import struct

import numpy as np

from . import capi
from .mesh import CellCenterX


def _fatal(msg):
    raise RuntimeError("### FATAL ERROR " + msg)


def _cfmt(fmt, val):
    """printf with a C format string (the decks carry C formats such as %12.5e)"""
    return fmt % val


def CellCenterIndex(x, n, xmin, xmax):
    """src/coordinates/cell_locations.hpp:48-50"""
    return int(((x - xmin)/(xmax - xmin))*float(n))


class OutputParameters:
    """src/outputs/outputs.hpp: OutputParameters"""

    def __init__(self):
        self.block_number = 0
        self.block_name = ""
        self.last_time = -1.0
        self.dt = 0.0
        self.dcycle = 0
        self.file_number = 0
        self.file_basename = ""
        self.file_type = ""
        self.variable = ""
        self.file_id = ""
        self.include_gzs = False
        self.gid = -1
        self.slice1 = self.slice2 = self.slice3 = False
        self.slice_x1 = self.slice_x2 = self.slice_x3 = 0.0
        self.data_format = " %12.5e"
        self.user_hist_only = False
        # pdf (outputs.cpp:252-271)
        self.bin_min = self.bin_max = 0.0
        self.nbin = 0
        self.logscale = True
        self.mass_weighted = False
        self.variable_2 = ""
        self.bin2_min, self.bin2_max = 0.0, 1.0
        self.nbin2 = 0
        self.logscale2 = True
        # cbin (outputs.cpp:247-249)
        self.coarsen_factor = 1
        self.compute_moments = False


class OutputMeshBlockInfo:
    def __init__(self, gid, ois, oie, ojs, oje, oks, oke, size):
        self.mb_gid = gid
        self.ois, self.oie, self.ojs, self.oje, self.oks, self.oke = ois, oie, ojs, oje, oks, oke
        self.x1min, self.x1max = size.x1min, size.x1max
        self.x2min, self.x2max = size.x2min, size.x2max
        self.x3min, self.x3max = size.x3min, size.x3max


# derived variables of derived_variables.cpp that this path computes (akmi_derived_var, csrc/akmi_derived.hip):
# output name -> (key of capi.DERIVED, label of basetype_output.cpp:486-559)
_DERIVED = {"hydro_wz": ("wz", "vorz"), "hydro_w2": ("w2", "vor2"), "mhd_wz": ("wz", "vorz"), "mhd_w2": ("w2", "vor2"),
            "mhd_jz": ("jz", "jz"), "mhd_j2": ("j2", "j2"), "mhd_curv": ("curv", "curv"),
            "mhd_k_jxb": ("k_jxb", "k_jxb"), "mhd_curv_perp": ("curv_perp", "curv_perp"),
            "mhd_bmag": ("bmag", "bmag"), "mhd_divb": ("divb", "divb")}

# names of the reference that stay refused, each with what it would need
_REFUSED = {"mhd_jcon": "it needs the saved state of SaveMHDState",
            "hydro_sgs": "the sub-grid-scale tensors are not on this path",
            "mhd_sgs": "the sub-grid-scale tensors are not on this path",
            "mhd_dynamo_ks": "the dynamo wavenumber scales are not on this path",
            "mhd_curv_alt": "the alternative curvature is not on this path",
            "mhd_t": "the temperature array of DynGRMHD does not exist on this path"}


def derived_which(name, is_mhd, is_ideal=True):
    """(which, ncomp, label) of a derived variable by output name or by plain key ("temperature", "wz", ...);
    the names this path does not compute stop here with a message that names them"""
    if name in _REFUSED or name.endswith("_moments") or name.startswith(("rad", "prtcl")):
        why = _REFUSED.get(name, "radiation, particle and moment outputs are not on this path")
        _fatal("Output variable '%s' is not implemented on this path: %s" % (name, why))
    if name in _DERIVED:
        key, label = _DERIVED[name]
        if name.startswith("mhd_" if not is_mhd else "hydro_"):
            _fatal("Output of %s variable '%s' requested but no %s object has been constructed"
                   % (("MHD", name, "MHD") if not is_mhd else ("Hydro", name, "Hydro")))
    elif name in capi.DERIVED:
        key, label = name, name
    else:
        _fatal("Derived variable '%s' is not a valid choice (%s)" % (name, ", ".join(sorted(_DERIVED))))
    if not is_mhd and key not in ("temperature", "wz", "w2"):
        _fatal("Derived variable '%s' needs the magnetic field: no MHD object has been constructed" % name)
    if key == "temperature" and not is_ideal:
        # derived_variables.cpp:98-115 divides w0(IEN) by w0(IDN); the block needs neither <units> nor gamma
        _fatal("Derived variable 'temperature' (derived_variables.cpp:98, eint/dens) needs the ideal-gas EOS: "
               "an isothermal fluid stores no internal energy")
    return capi.DERIVED[key], 1, label


def derived_array(phys, which):
    """the derived variable over the whole pack: (nmb, 1, N3, N2, N1) on the device of the state arrays"""
    import torch
    nmb, _, n3, n2, n1 = phys.w0.shape
    out = torch.empty((nmb, 1, n3, n2, n1), dtype=torch.float64, device=phys.w0.device)
    L = capi.lib()
    if not hasattr(L, "akmi_derived_var"):
        _fatal("derived output variables need akmi_derived_var of libakmi.so (a GPU): this backend has none")
    b0 = getattr(phys, "b0", None)
    b = (b0.x1f, b0.x2f, b0.x3f) if b0 is not None else (None, None, None)
    capi.check(L.akmi_derived_var(phys.pack_c, which, phys.w0, phys.u0, getattr(phys, "bcc0", None), *b, out, 1,
                                  capi._stream()), "derived_var")
    return out


def _scalars(nfluid, nscalars):
    """basetype_output.cpp:275-307: r_NN in u0, s_NN in w0, after the fluid variables"""
    us = [("r_%02d" % (n % 100), nfluid + n, "u0") for n in range(nscalars)]
    ws = [("s_%02d" % (n % 100), nfluid + n, "w0") for n in range(nscalars)]
    return us, ws


# variable groups of basetype_output.cpp:196-620 for Newtonian hydro/MHD:
# name -> list of (label, component, array); array "dv:<which>" is computed at output time
def _grav_phi_outvars(have_grav, block_name):
    """variable = grav_phi, basetype_output.cpp:172-178,620-623: Gravity::phi"""
    if not have_grav:
        _fatal("Output of gravity potential requested in <output> block '%s' but gravity object not constructed."
               "\nInput file is likely missing a <gravity> block" % block_name)
    return [("grav_phi", 0, "phi")]


def _outvars(variable, is_mhd, is_ideal=True, turb=False, nscalars=0):
    blk = "mhd" if is_mhd else "hydro"
    u = [("dens", 0, "u0"), ("mom1", 1, "u0"), ("mom2", 2, "u0"), ("mom3", 3, "u0"), ("ener", 4, "u0")]
    w = [("dens", 0, "w0"), ("velx", 1, "w0"), ("vely", 2, "w0"), ("velz", 3, "w0"), ("eint", 4, "w0")]
    if not is_ideal:                       # basetype_output.cpp:252-271: energies only if is_ideal
        u, w = u[:4], w[:4]
    us, ws = _scalars(len(u), nscalars)
    b = [("bcc1", 0, "bcc0"), ("bcc2", 1, "bcc0"), ("bcc3", 2, "bcc0")]
    table = {blk + "_u": u + us, blk + "_w": w + ws, blk + "_u_s": us, blk + "_w_s": ws}
    for sfx, (lab, n, arr) in zip(("d", "m1", "m2", "m3", "e"), u):
        table["%s_u_%s" % (blk, sfx)] = [(lab, n, arr)]
    for sfx, (lab, n, arr) in zip(("d", "vx", "vy", "vz", "e"), w):
        table["%s_w_%s" % (blk, sfx)] = [(lab, n, arr)]
    if is_mhd:
        # the scalars precede the cell-centred field in the combined groups (basetype_output.cpp:409-477)
        table.update({"mhd_bcc": b, "mhd_u_bcc": u + us + b, "mhd_w_bcc": w + ws + b, "mhd_bcc1": b[0:1],
                      "mhd_bcc2": b[1:2], "mhd_bcc3": b[2:3]})
    if turb:                               # basetype_output.cpp:614-617: TurbulenceDriver::force
        table["turb_force"] = [("force1", 0, "force"), ("force2", 1, "force"), ("force3", 2, "force")]
    if variable in table:
        return table[variable]
    if (variable in _DERIVED and variable.startswith(blk + "_")) or variable in _REFUSED \
            or variable.endswith("_moments") or variable.startswith(("rad", "prtcl")):
        which, _, label = derived_which(variable, is_mhd, is_ideal)
        return [(label, 0, "dv:%d" % which)]
    _fatal("Output variable '%s' not implemented on this path (choices: %s)"
           % (variable, ", ".join(sorted(list(table) + [k for k in _DERIVED if k.startswith(blk + "_")]))))


def _out_fluid(pk, variable=None):
    """(fluid, is_mhd) an output block reads.  With two fluids (<ion-neutral>) the hydro_* variables read the neutral
    fluid and the mhd_* variables the ion fluid, as the reference's groups do (basetype_output.cpp:196-477)."""
    if getattr(pk, "pionn", None) is not None and variable is not None and variable.startswith("hydro_"):
        return pk.phydro, False
    return (pk.pmhd, True) if pk.pmhd is not None else (pk.phydro, False)


class BaseTypeOutput:
    def __init__(self, pin, pm, op):
        self.out_params = op
        self.outvars = []
        self.outmbs = []
        self.outarray = None
        pk = pm.pmb_pack
        if op.file_type not in ("hst", "rst", "pdf"):
            two = getattr(pk, "pionn", None) is not None
            if two and op.file_type not in ("tab", "bin"):
                _fatal("%s output of a run with two fluids is not on this path yet (output block '%s'): tab, bin and hst"
                       % (op.file_type, op.block_name))
            phys, is_mhd = _out_fluid(pk, op.variable)
            if op.variable == "grav_phi":
                if op.file_type not in ("tab", "bin"):
                    _fatal("%s output of grav_phi is not on this path (output block '%s'): tab and bin"
                           % (op.file_type, op.block_name))
                self.outvars = _grav_phi_outvars(getattr(pk, "pgrav", None) is not None, op.block_name)
                return
            self.outvars = _outvars(op.variable, is_mhd, phys.peos.eos_data.is_ideal,
                                    getattr(pk, "pturb", None) is not None and not two, getattr(phys, "nscalars", 0))

    def LoadOutputData(self, pm):
        """basetype_output.cpp:729-862: per-block index ranges (ghost zones, slices) and a
        host copy of the selected components"""
        pk = pm.pmb_pack
        phys, _ = _out_fluid(pk, getattr(self.out_params, "variable", None))
        self._load_ranges(pm)
        self._load_outarray(pm, pk, phys)

    def _load_ranges(self, pm):
        """basetype_output.cpp:729-805: outmbs, the index ranges of the MeshBlocks this output writes"""
        op = self.out_params
        ind = pm.mb_indcs
        pk = pm.pmb_pack
        self.outmbs = []
        for m in range(pk.nmb_thispack):
            if op.gid >= 0 and (m + pk.gids) != op.gid:
                continue
            size = pk.pmb.mb_size[m]
            if op.include_gzs:
                n3, n2, n1 = ind.ncells
                ois, oie, ojs, oje, oks, oke = 0, n1 - 1, 0, n2 - 1, 0, n3 - 1
            else:
                ois, oie, ojs, oje, oks, oke = ind.is_, ind.ie, ind.js, ind.je, ind.ks, ind.ke
            if op.slice1:
                if op.slice_x1 < size.x1min or op.slice_x1 >= size.x1max:
                    continue
                ois = oie = CellCenterIndex(op.slice_x1, ind.nx1, size.x1min, size.x1max) + ind.is_
            if op.slice2:
                if op.slice_x2 < size.x2min or op.slice_x2 >= size.x2max:
                    continue
                ojs = oje = CellCenterIndex(op.slice_x2, ind.nx2, size.x2min, size.x2max) + ind.js
            if op.slice3:
                if op.slice_x3 < size.x3min or op.slice_x3 >= size.x3max:
                    continue
                oks = oke = CellCenterIndex(op.slice_x3, ind.nx3, size.x3min, size.x3max) + ind.ks
            self.outmbs.append(OutputMeshBlockInfo(int(pk.pmb.mb_gid[m]), ois, oie, ojs, oje, oks,
                                                   oke, size))

    def _load_outarray(self, pm, pk, phys):
        """basetype_output.cpp:807-862: a host copy of the selected components"""
        if not self.outmbs or not self.outvars:
            self.outarray = None
            return
        o = self.outmbs[0]
        shape = (len(self.outvars), len(self.outmbs), o.oke - o.oks + 1, o.oje - o.ojs + 1,
                 o.oie - o.ois + 1)
        out = np.empty(shape, dtype=np.float64)
        host = {}
        derived = {}              # one launch per output and derived variable, over all MeshBlocks of the pack
        for n, (_, comp, arr) in enumerate(self.outvars):
            if arr.startswith("dv:") and arr not in derived:
                derived[arr] = derived_array(phys, int(arr[3:]))
            for mi, o in enumerate(self.outmbs):
                m = o.mb_gid - pk.gids
                key = (arr, m, comp)
                if key not in host:
                    if arr in derived:
                        host[key] = _to_numpy(derived[arr][m, comp])
                    else:
                        src = pk.pturb if arr == "force" else (pk.pgrav if arr == "phi" else phys)
                        host[key] = _to_numpy(getattr(src, arr)[m, comp])
                out[n, mi] = host[key][o.oks:o.oke + 1, o.ojs:o.oje + 1, o.ois:o.oie + 1]
        self.outarray = out

    def _advance(self, pm, pin, numbered=True):
        op = self.out_params
        if numbered:
            op.file_number += 1
            pin.SetInteger(op.block_name, "file_number", op.file_number)
        if op.last_time < 0.0:
            op.last_time = pm.time
        else:
            op.last_time += op.dt
        pin.SetReal(op.block_name, "last_time", op.last_time)


def _to_numpy(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _barrier(pm):
    if pm.nranks > 1:
        import torch.distributed as dist
        dist.barrier()


class FormattedTableOutput(BaseTypeOutput):
    def __init__(self, pin, pm, op):
        super().__init__(pin, pm, op)
        if pm.multi_d and not (op.slice1 or op.slice2):
            _fatal("Formatted table outputs can only contain 1D slices\nPlease add additional slice planes")
        if pm.three_d and ((not op.slice2 and not op.slice3) or (not op.slice1 and not op.slice3)):
            _fatal("Formatted table outputs can only contain 1D slices\nPlease add additional slice planes")
        os.makedirs("tab", exist_ok=True)

    def WriteOutputFile(self, pm, pin):
        """formatted_table.cpp:52-195"""
        op = self.out_params
        fname = "tab/%s.%s.%05d.tab" % (op.file_basename, op.file_id, op.file_number)
        fmt = op.data_format
        if pm.my_rank == 0:
            with open(fname, "w") as f:
                f.write("# Athena++ data at time=%e" % pm.time)
                f.write("  cycle=%d \n" % pm.ncycle)
                f.write("# gid  ")
                if not op.slice1:
                    f.write(" i       x1v     ")
                if not op.slice2:
                    f.write(" j       x2v     ")
                if not op.slice3:
                    f.write(" k       x3v     ")
                for (label, _, _) in self.outvars:
                    f.write("    %s     " % label)
                f.write("\n")
        _barrier(pm)
        ind = pm.mb_indcs
        for r in range(pm.nranks):
            if r == pm.my_rank:
                with open(fname, "a") as f:
                    for mi, o in enumerate(self.outmbs):
                        for k in range(o.oks, o.oke + 1):
                            for j in range(o.ojs, o.oje + 1):
                                for i in range(o.ois, o.oie + 1):
                                    line = ["%05d" % o.mb_gid]
                                    if o.oie != o.ois:
                                        line.append(" %04d" % i)
                                        line.append(_cfmt(fmt, CellCenterX(i - ind.is_, ind.nx1, o.x1min, o.x1max)))
                                    if o.oje != o.ojs:
                                        line.append(" %04d" % j)
                                        line.append(_cfmt(fmt, CellCenterX(j - ind.js, ind.nx2, o.x2min, o.x2max)))
                                    if o.oke != o.oks:
                                        line.append(" %04d" % k)
                                        line.append(_cfmt(fmt, CellCenterX(k - ind.ks, ind.nx3, o.x3min, o.x3max)))
                                    for n in range(len(self.outvars)):
                                        line.append(_cfmt(fmt, self.outarray[n, mi, k - o.oks, j - o.ojs, i - o.ois]))
                                    f.write("".join(line) + "\n")
            _barrier(pm)
        self._advance(pm, pin)


class HistoryOutput(BaseTypeOutput):
    """history.cpp: volume sums of the conserved variables, kinetic and magnetic energies"""

    def __init__(self, pin, pm, op):
        super().__init__(pin, pm, op)
        pk = pm.pmb_pack
        self.is_mhd = pk.pmhd is not None
        self.labels = ["mass", "1-mom", "2-mom", "3-mom", "tot-E", "1-KE", "2-KE", "3-KE"]
        phys = pk.pmhd if self.is_mhd else pk.phydro
        if phys is None:
            # history.cpp:32-52 would build an empty list and write nothing; here a history block needs a fluid to sum
            _fatal("hst output block '%s': no Hydro or MHD object has been constructed on this Mesh, so neither the "
                   "history sums nor the turbulence history columns can be formed" % op.block_name)
        if not phys.peos.eos_data.is_ideal:
            self.labels.remove("tot-E")
        if self.is_mhd:
            self.labels += ["1-ME", "2-ME", "3-ME"]
        self.hdata = None
        self.header_written = False
        # two fluids (<ion-neutral>): <basename>.hydro.hst of the neutrals as well (history.cpp:32-52 builds one
        # HistoryData per physics module); self.labels / hdata / header_written above are the ion (MHD) fluid's
        self.neutral = None
        if getattr(pk, "pionn", None) is not None:
            nl = ["mass", "1-mom", "2-mom", "3-mom", "tot-E", "1-KE", "2-KE", "3-KE"]
            if not pk.phydro.peos.eos_data.is_ideal:
                nl.remove("tot-E")
            self.neutral = {"labels": nl, "hdata": None, "header_written": False}
        # history.cpp:35-47: the user-defined columns after the physics', or alone with user_hist_only
        self.user_hist = user_hist_of(pin)
        self.physics_hist = not (self.user_hist and op.user_hist_only)
        self.udata = None
        self.user_header_written = False

    def LoadOutputData(self, pm):
        """history.cpp:78-160,272-374: the sums run on the device (akmi_history_sums); the user columns of a turbulence
        run are TurbulentHistory (turb.cpp:247-396, akmi_turb_history)"""
        import torch
        pk = pm.pmb_pack
        if self.user_hist:
            enrolled = getattr(pm.pgen, "user_hist_func", None)      # ShwaveHistory (pgen_name = shwave, ipert = 3)
            if enrolled is not None:
                self.ulabels, self.udata = enrolled(pm)
            else:
                self.ulabels, self.udata = capi.TURB_HIST_LABELS, turb_history_sums(pk.pmhd, pk)
        if not self.physics_hist:
            return
        phys = pk.pmhd if self.is_mhd else pk.phydro
        out = torch.zeros(len(self.labels), dtype=torch.float64, device=phys.u0.device)
        L = capi.lib()
        if self.is_mhd:
            b = (phys.b0.x1f, phys.b0.x2f, phys.b0.x3f)
        else:
            b = (None, None, None)
        capi.check(L.akmi_history_sums(phys.pack_c, 1 if self.is_mhd else 0, phys.u0, *b, out, capi._stream()),
                   "history_sums")
        self.hdata = out
        if self.neutral is not None:
            ph = pk.phydro
            nout = torch.zeros(len(self.neutral["labels"]), dtype=torch.float64, device=ph.u0.device)
            capi.check(L.akmi_history_sums(ph.pack_c, 0, ph.u0, None, None, None, nout, capi._stream()), "history_sums")
            self.neutral["hdata"] = nout

    def WriteOutputFile(self, pm, pin):
        """history.cpp:381-457"""
        op = self.out_params
        if self.physics_hist:
            h = self.hdata
            if pm.nranks > 1:
                import torch.distributed as dist
                if dist.get_backend() != "nccl":
                    h = h.cpu()
                dist.all_reduce(h, op=dist.ReduceOp.SUM)      # MPI_Reduce(MPI_SUM) to rank 0
            h = h.cpu().numpy()
            if pm.my_rank == 0:
                fname = "%s.%s.hst" % (op.file_basename, "mhd" if self.is_mhd else "hydro")
                self.header_written = self._append(fname, pm, self.labels, h, self.header_written)
                if self.neutral is not None:              # (one rank: ionn_deck_checks)
                    nt = self.neutral
                    nt["header_written"] = self._append("%s.hydro.hst" % op.file_basename, pm, nt["labels"],
                                                        nt["hdata"].cpu().numpy(), nt["header_written"])
        if self.user_hist and pm.my_rank == 0:
            # the sums are already those of the whole mesh on every rank (turb_history_sums)
            self.user_header_written = self._append("%s.user.hst" % op.file_basename, pm, self.ulabels,
                                                    self.udata, self.user_header_written)
        self._advance(pm, pin, numbered=False)

    def _append(self, fname, pm, labels, values, header_written):
        """history.cpp:418-445: one line of one history file, after its header the first time"""
        op = self.out_params
        with open(fname, "a") as f:
            if not header_written:
                f.write("# Athena++ history data\n")
                f.write("#  [%d]=time      " % 1)
                f.write("[%d]=dt       " % 2)
                for n, lab in enumerate(labels):
                    f.write("[%d]=%.10s    " % (n + 3, lab))
                f.write("\n")
            f.write(_cfmt(op.data_format, pm.time))
            f.write(_cfmt(op.data_format, pm.dt))
            for v in values:
                f.write(_cfmt(op.data_format, float(v)))
            f.write("\n")
        return True


def user_hist_of(pin):
    """<problem>/user_hist (pgen.cpp:49; default false, read without adding it to the deck) and what this path enrols for it:
    TurbulentHistory of pgen_name = turb on an MHD run (turb.cpp:42), ShwaveHistory of pgen_name = shwave with ipert = 3 (hydro) or
    ipert = 4 (MHD)"""
    if not (pin.DoesParameterExist("problem", "user_hist") and pin.GetBoolean("problem", "user_hist")):
        return False
    name = pin.GetString("problem", "pgen_name") if pin.DoesParameterExist("problem", "pgen_name") else "none"
    if name == "shwave":
        # shwave.cpp:144: ShwaveHistory is enrolled for the compressible hydro wave, and :186 for the MHD wave (dByc)
        if pin.DoesBlockExist("hydro") and pin.GetInteger("problem", "ipert") == 3:
            return True
        if pin.DoesBlockExist("mhd") and not pin.DoesBlockExist("hydro"):
            if pin.GetInteger("problem", "ipert") == 4:
                return True
            _fatal("<problem>/user_hist = true with pgen_name = shwave: the user history function of an MHD run (dByc) is "
                   "enrolled for ipert = 4, the only MHD perturbation")
        _fatal("<problem>/user_hist = true with pgen_name = shwave: the user history function (dVyc) is enrolled for "
               "ipert = 3 of a hydro run only")
    if name == "mri3d":
        # mri3d.cpp:58: MRIHistory is enrolled whatever the deck holds; the generator itself needs an MHD run
        return True
    if name != "turb":
        # pgen.cpp:86-92 exits with "user history function not enrolled"; the other generators' functions are not on this path
        _fatal("<problem>/user_hist = true, but the user history function of pgen_name = '%s' is not enrolled on this "
               "path (only the turbulence history columns of pgen_name = turb are)" % name)
    if not pin.DoesBlockExist("mhd"):
        # the reference dereferences a null pmhd here (turb.cpp:262)
        _fatal("<problem>/user_hist = true with pgen_name = turb needs an MHD run: the turbulence history columns "
               "(turb.cpp:247-396) are sums of the magnetic field")
    return True


def turb_history_sums(phys, pack):
    """the eleven sums of TurbulentHistory over the whole mesh as Python floats: per-MeshBlock partials of akmi_turb_history,
    added in gid order (turb_driver.gid_ordered_sums), so that they do not depend on the rank count"""
    import torch
    from .turb_driver import gid_ordered_sums
    L = capi.lib()
    if not hasattr(L, "akmi_turb_history"):
        _fatal("the turbulence history columns need akmi_turb_history of libakmi.so (a GPU): this backend has none")
    if getattr(phys, "bcc0", None) is None:
        _fatal("the turbulence history columns need an MHD run")
    nmb = phys.w0.shape[0]
    partial = torch.zeros((nmb, capi.TURB_NHIST), dtype=torch.float64, device=phys.w0.device)
    nbytes = int(L.akmi_turb_history_workspace_bytes(phys.pack_c))
    work = torch.empty(nbytes//8 + 1, dtype=torch.float64, device=phys.w0.device)
    capi.check(L.akmi_turb_history(phys.pack_c, phys.w0, phys.bcc0, phys.b0.x1f, phys.b0.x2f, phys.b0.x3f, partial,
                                   work, capi._stream()), "turb_history")
    return gid_ordered_sums(partial.cpu().numpy(), pack)


def pdf_bins(bin_min, bin_max, nbin, logscale):
    """(edges[nbin+1], step) with the expressions of pdf.cpp:82-102"""
    import math
    if logscale:
        lmin, lmax = math.log10(bin_min), math.log10(bin_max)
        edges = [math.pow(10.0, lmin + i*(lmax - lmin)/nbin) for i in range(nbin + 1)]
        step = (math.log10(bin_max) - math.log10(bin_min))/nbin
    else:
        bin_step = (bin_max - bin_min)/nbin
        edges = [bin_min + i*bin_step for i in range(nbin + 1)]
        step = (bin_max - bin_min)/nbin
    return np.array(edges, dtype=np.float64), step


_PDF_GROUPS = ("mhd_w", "mhd_u", "hydro_w", "hydro_u")


def _pdf_group_check(block, variable):
    """outputs.cpp:190-203"""
    if variable in _PDF_GROUPS:
        _fatal("PDF output block '%s' cannot output variable '%s'. The variable must be a single variable not a "
               "variable group" % (block, variable))


def pdf_checks(block, variable, bin_min, bin_max, nbin, logscale, variable_2="", bin2_min=0.0, bin2_max=1.0, nbin2=0,
               logscale2=True):
    """what a pdf block may not ask for (outputs.cpp:190-203, pdf.cpp:62-74, and what this path refuses)"""
    _pdf_group_check(block, variable)
    if nbin < 1:
        _fatal("PDF output block '%s': nbin = %d, at least one bin is needed" % (block, nbin))
    if logscale and bin_min <= 0.0:
        _fatal("logscale is true but bin_min <= 0.0")
    if not bin_max > bin_min:
        _fatal("PDF output block '%s': bin_max = %g is not above bin_min = %g" % (block, bin_max, bin_min))
    if variable_2:
        if nbin2 == 1:
            # basetype_output.cpp:187-190 loads the second variable only if nbin2 > 1, pdf.cpp:47 makes the histogram 2-D
            # for every nbin2 != 0: with nbin2 = 1 the reference reads an array that was never loaded
            _fatal("PDF output block '%s': nbin2 = 1 is not on this path (the reference builds a 2-D histogram there "
                   "without loading the second variable)" % block)
        if nbin2 < 0:
            _fatal("PDF output block '%s': nbin2 = %d" % (block, nbin2))
        if nbin2 > 0:
            _pdf_group_check(block, variable_2)
            if logscale2 and bin2_min <= 0.0:
                _fatal("logscale2 is true but bin2_min <= 0.0")
            if not bin2_max > bin2_min:
                _fatal("PDF output block '%s': bin2_max = %g is not above bin2_min = %g" % (block, bin2_max, bin2_min))


def _single_var(variable, is_mhd, is_ideal, turb, nscalars):
    ov = _outvars(variable, is_mhd, is_ideal, turb, nscalars)
    if len(ov) != 1:
        _fatal("PDF output cannot output variable '%s'. The variable must be a single variable not a variable group"
               % variable)
    return ov[0]


def pdf_histogram(pack, axes, mass_weighted, force_global=False):
    """counts (int64), weights (float64) of shape [(nbin2+2)|1][nbin+2] and the number of NaN cells dropped, over the
    whole mesh (all-reduce(sum) with ranks).  axes: one or two of ((label, comp, arr), edges, step, logscale) with arr as in
    _outvars."""
    import torch
    phys = pack.pmhd if pack.pmhd is not None else pack.phydro
    L = capi.lib()
    if not hasattr(L, "akmi_pdf"):
        _fatal("pdf outputs need akmi_pdf of libakmi.so (a GPU): this backend has none")
    keep, cax = [], []
    for (label, comp, arr), edges, step, logscale in axes:
        if arr.startswith("dv:"):
            t, comp = derived_array(phys, int(arr[3:])), 0
        else:
            t = getattr(pack.pturb if arr == "force" else phys, arr)
        keep.append(t)
        cax.append(capi.PdfAxis(t.data_ptr(), t.shape[1], comp, len(edges) - 1, 1 if logscale else 0,
                                float(edges[0]), float(edges[-1]), float(step)))
    shape = ((cax[1].nbin + 2) if len(cax) == 2 else 1, cax[0].nbin + 2)
    dev = phys.u0.device
    counts = torch.zeros(shape, dtype=torch.int64, device=dev)        # the entry counts in uint64; the bits are the same
    weights = torch.zeros(shape, dtype=torch.float64, device=dev)
    nan = torch.zeros(1, dtype=torch.int64, device=dev)
    capi.check(L.akmi_pdf(phys.pack_c, cax[0], cax[1] if len(cax) == 2 else None, phys.u0 if mass_weighted else None,
                          counts, weights, nan, 1 if force_global else 0, capi._stream()), "pdf")
    return pdf_reduce_ranks(pack.pmesh, counts, weights, nan)


def pdf_reduce_ranks(pm, counts, weights, nan):
    """pdf.cpp:296-304: sum over ranks (every rank gets it); numpy arrays and the NaN count"""
    if pm.nranks > 1:
        import torch.distributed as dist
        if dist.get_backend() != "nccl":
            counts, weights, nan = counts.cpu(), weights.cpu(), nan.cpu()
        for t in (counts, weights, nan):
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return counts.cpu().numpy(), weights.cpu().numpy(), int(nan.cpu()[0])


def pdf_axes(pack, variable, bin_min, bin_max, nbin, logscale=True, variable_2=None, bin2_min=0.0, bin2_max=1.0, nbin2=0,
             logscale2=True):
    """the axes of pdf_histogram for one or two output variables by name, after the checks of a pdf block"""
    pdf_checks("(accessor)", variable, bin_min, bin_max, nbin, logscale, variable_2 or "", bin2_min, bin2_max, nbin2,
               logscale2)
    phys = pack.pmhd if pack.pmhd is not None else pack.phydro
    args = (pack.pmhd is not None, phys.peos.eos_data.is_ideal, getattr(pack, "pturb", None) is not None,
            getattr(phys, "nscalars", 0))
    axes = [(_single_var(variable, *args),) + pdf_bins(bin_min, bin_max, nbin, logscale) + (logscale,)]
    if variable_2 and nbin2 > 0:
        axes.append((_single_var(variable_2, *args),) + pdf_bins(bin2_min, bin2_max, nbin2, logscale2) + (logscale2,))
    return axes


class PdfResult:
    """what Simulation.pdf / NativeSimulation.pdf return: bins (edges[nbin+1]), bins2 (or None), counts and weights of
    shape [(nbin2+2)|1][nbin+2] (row 0 / column 0 below the first edge, the last at or above the last edge), and the
    number of cells dropped because a value is NaN"""

    def __init__(self, axes, counts, weights, nan_dropped):
        self.bins = axes[0][1]
        self.bins2 = axes[1][1] if len(axes) == 2 else None
        self.counts, self.weights, self.nan_dropped = counts, weights, nan_dropped


class PDFOutput(BaseTypeOutput):
    """pdf.cpp: volume- or mass-weighted 1-D / 2-D histogram of one (two) single output variable(s) over the active cells
    of the whole mesh; the bin edges once in <basename>.bins.pdf, the weights of every output in <basename>.NNNNN.pdf"""

    def __init__(self, pin, pm, op):
        pdf_checks(op.block_name, op.variable, op.bin_min, op.bin_max, op.nbin, op.logscale, op.variable_2, op.bin2_min,
                   op.bin2_max, op.nbin2, op.logscale2)
        super().__init__(pin, pm, op)
        pk = pm.pmb_pack
        phys = pk.pmhd if pk.pmhd is not None else pk.phydro
        args = (pk.pmhd is not None, phys.peos.eos_data.is_ideal, getattr(pk, "pturb", None) is not None,
                getattr(phys, "nscalars", 0))
        self.outvars = [_single_var(op.variable, *args)]
        self.pdf_dimension = 1 if op.nbin2 == 0 else 2
        self.bins, self.step_size = pdf_bins(op.bin_min, op.bin_max, op.nbin, op.logscale)
        self.axes = [(self.outvars[0], self.bins, self.step_size, op.logscale)]
        self.dir_name = "pdf_" + op.file_id
        if self.pdf_dimension == 2:
            self.outvars.append(_single_var(op.variable_2, *args))
            self.bins2, self.step_size2 = pdf_bins(op.bin2_min, op.bin2_max, op.nbin2, op.logscale2)
            self.axes.append((self.outvars[1], self.bins2, self.step_size2, op.logscale2))
            self.dir_name += "_" + op.variable_2
        if pm.my_rank == 0:
            os.makedirs(self.dir_name, exist_ok=True)
        self.bins_written = False
        self.counts = self.result = None
        self.nan_dropped = 0

    def LoadOutputData(self, pm):
        """pdf.cpp:162-305"""
        self.counts, self.result, self.nan_dropped = pdf_histogram(pm.pmb_pack, self.axes, self.out_params.mass_weighted)

    def WriteOutputFile(self, pm, pin):
        """pdf.cpp:311-423"""
        op = self.out_params
        if pm.my_rank == 0:
            if not self.bins_written:
                with open("%s/%s.bins.pdf" % (self.dir_name, op.file_basename), "a") as f:
                    f.write("# pdf bins \n")
                    f.write("# [1]= %.20s \n" % self.outvars[0][0])
                    if self.pdf_dimension == 2:
                        f.write("# [2]= %.20s \n" % self.outvars[1][0])
                    f.write("".join(_cfmt(op.data_format, float(b)) for b in self.bins) + "\n")
                    if self.pdf_dimension == 2:
                        f.write("".join(_cfmt(op.data_format, float(b)) for b in self.bins2) + "\n")
                self.bins_written = True
            with open("%s/%s.%05d.pdf" % (self.dir_name, op.file_basename, op.file_number), "a") as f:
                f.write("# time= ")
                f.write(_cfmt(op.data_format, pm.time))
                f.write("\n")
                for row in self.result:
                    f.write("".join(_cfmt(op.data_format, float(v)) for v in row) + "\n")
                f.write("\n")
        self._advance(pm, pin)


class MeshBinaryOutput(BaseTypeOutput):
    def __init__(self, pin, pm, op):
        super().__init__(pin, pm, op)
        if pin.GetOrAddBoolean(op.block_name, "single_file_per_rank", False):
            _fatal("bin output: single_file_per_rank is not implemented on this path")
        os.makedirs("bin", exist_ok=True)

    def WriteOutputFile(self, pm, pin):
        """binary.cpp:52-319: text pre-header, parameter dump, then per MeshBlock 10 int32
        (ois,oie,ojs,oje,oks,oke,lx1,lx2,lx3,level), 6 Real (block extent) and the variables as
        float32 [nvar][k][j][i]"""
        op = self.out_params
        fname = "bin/%s.%s.%05d.bin" % (op.file_basename, op.file_id, op.file_number)
        msg = ("Athena binary output version=1.1\n  size of preheader=5\n  time=%.16e\n  cycle=%d\n"
               "  size of location=8\n  size of variable=4\n  number of variables=%d\n  variables:  "
               % (pm.time, pm.ncycle, len(self.outvars)))
        msg += "".join("%s  " % lab for (lab, _, _) in self.outvars) + "\n"
        dump = pin.ParameterDump()
        hdr = (msg + "  header offset=%d\n" % len(dump) + dump).encode("ascii")
        if pm.my_rank == 0:
            with open(fname, "wb") as f:
                f.write(hdr)
        _barrier(pm)
        for r in range(pm.nranks):
            if r == pm.my_rank and self.outmbs:
                with open(fname, "ab") as f:
                    for mi, o in enumerate(self.outmbs):
                        l1, l2, l3 = pm.lloc_eachmb[o.mb_gid][:3]
                        # binary.cpp:192-193: loc.level - root_level (0 on uniform meshes, >0 inside refined regions)
                        f.write(struct.pack("<10i", o.ois, o.oie, o.ojs, o.oje, o.oks, o.oke, l1, l2, l3,
                                            pm.level_of(o.mb_gid) - pm.root_level))
                        f.write(struct.pack("<6d", o.x1min, o.x1max, o.x2min, o.x2max, o.x3min, o.x3max))
                        f.write(np.ascontiguousarray(self.outarray[:, mi], dtype="<f4").tobytes())
            _barrier(pm)
        self._advance(pm, pin)


# ---- coarsened binary outputs -------------------------------------------------------------------------------------
_MOMENT_SUFFIX = ("_1st", "_2nd", "_3rd", "_4th")          # coarsened_binary.cpp:354-357
_NATIVE_STORED = {"u0": 0, "w0": 1, "bcc0": 2}            # akmi_sim_coarsen / akmi_sim_pdf: a stored array by number


def coarsen_extents(ind, include_gzs, slices=(False, False, False)):
    """(n1, n2, n3): the fine cells per MeshBlock and direction of an output with these keys (the ranges of
    BaseTypeOutput._load_ranges: the active cells, the whole array with ghost_zones, one cell across a slice)"""
    n3, n2, n1 = ind.ncells if include_gzs else (ind.nx3, ind.nx2, ind.nx1)
    return tuple(1 if sl else n for sl, n in zip(slices, (n1, n2, n3)))


def coarsen_checks(block, factor, extents):
    """what a cbin block may not ask for, before anything is allocated: the reference exits at the first output
    (coarsened_binary.cpp:213-218), a missing dimension or a slice (extent 1) included"""
    if factor < 1:
        _fatal("cbin output block '%s': coarsen_factor = %d, at least 1 is needed" % (block, factor))
    for q, n in enumerate(extents):
        if n % factor != 0:
            _fatal("Full data dimensions are not divisible by coarsen_factor (output block '%s': %d cells in x%d, "
                   "coarsen_factor = %d)" % (block, n, q + 1, factor))


def coarsen_labels(outvars, moments):
    if not moments:
        return [lab for (lab, _, _) in outvars]
    return [lab + sfx for (lab, _, _) in outvars for sfx in _MOMENT_SUFFIX]


def coarsen_pack(pack, outvars, factor, moments, lo, nc, staged=None):
    """akmi_coarsen over every MeshBlock of the pack: (len(outvars)*nmom, nmb, nc3, nc2, nc1) in fp64 on the device of the
    state arrays.  outvars as in _outvars; lo = (ois, ojs, oks), nc = (nc1, nc2, nc3).  A derived variable is computed into
    its scratch array first.  staged: None (the library's default), False or True."""
    import torch
    phys = pack.pmhd if pack.pmhd is not None else pack.phydro
    native = getattr(phys, "native_sim", None)          # the C++ host names its stored arrays itself
    L = capi.lib()
    if not hasattr(L, "akmi_coarsen"):
        _fatal("cbin outputs need akmi_coarsen of libakmi.so (a GPU): this backend has none")
    keep = {}
    tab = (capi.CoarsenVar*len(outvars))()
    for n, (_, comp, arr) in enumerate(outvars):
        if arr.startswith("dv:"):
            if arr not in keep:
                keep[arr] = native.derived_by_number(int(arr[3:])) if native else derived_array(phys, int(arr[3:]))
            tab[n] = capi.CoarsenVar(keep[arr].data_ptr(), 1, 0)
        elif native is not None:
            tab[n] = capi.CoarsenVar(None, _NATIVE_STORED[arr], comp)
        else:
            t = getattr(pack.pturb if arr == "force" else phys, arr)
            tab[n] = capi.CoarsenVar(t.data_ptr(), t.shape[1], comp)
    nmb = phys.w0.shape[0]
    out = torch.empty((len(outvars)*(4 if moments else 1), nmb, nc[2], nc[1], nc[0]), dtype=torch.float64,
                      device=phys.w0.device)
    clo, cnc = (C.c_int*3)(*lo), (C.c_int*3)(*nc)
    st = -1 if staged is None else int(bool(staged))
    if native is not None:
        torch.cuda.synchronize()
        capi.check(L.akmi_sim_coarsen(native.h, tab, len(outvars), factor, 1 if moments else 0, clo, cnc, out, st),
                   "sim_coarsen")
    else:
        capi.check(L.akmi_coarsen(phys.pack_c, tab, len(outvars), factor, 1 if moments else 0, clo, cnc, out, st,
                                  capi._stream()), "coarsen")
    return out


def coarsen_variable(pack, variable, factor, moments=False, ghost_zones=False, staged=None):
    """(labels, tensor) of Simulation.coarsen / NativeSimulation.coarsen: what a cbin block with these keys holds for this
    rank's MeshBlocks"""
    pm = pack.pmesh
    phys = pack.pmhd if pack.pmhd is not None else pack.phydro
    ind = pm.mb_indcs
    ext = coarsen_extents(ind, ghost_zones)
    coarsen_checks("(accessor)", factor, ext)
    outvars = _outvars(variable, pack.pmhd is not None, phys.peos.eos_data.is_ideal,
                       getattr(pack, "pturb", None) is not None, getattr(phys, "nscalars", 0))
    lo = (0, 0, 0) if ghost_zones else (ind.is_, ind.js, ind.ks)
    return coarsen_labels(outvars, moments), coarsen_pack(pack, outvars, factor, moments, lo,
                                                          tuple(n//factor for n in ext), staged)


class CoarsenedBinaryOutput(BaseTypeOutput):
    """coarsened_binary.cpp: every output variable averaged over f x f x f cells per MeshBlock, with compute_moments also
    <q^2>, <q^3>, <q^4>; the averages are formed on the device (akmi_coarsen, one launch for all variables and
    MeshBlocks) and only the coarse array is copied to the host"""

    def __init__(self, pin, pm, op):
        coarsen_checks(op.block_name, op.coarsen_factor,
                       coarsen_extents(pm.mb_indcs, op.include_gzs, (op.slice1, op.slice2, op.slice3)))
        if pin.GetOrAddBoolean(op.block_name, "single_file_per_rank", False):
            _fatal("cbin output: single_file_per_rank is not implemented on this path")
        super().__init__(pin, pm, op)
        self.dir_name = "cbin_%s_%d" % (op.file_id, op.coarsen_factor)
        os.makedirs(self.dir_name, exist_ok=True)

    def LoadOutputData(self, pm):
        """coarsened_binary.cpp:60-291: the ranges of the base class, then the coarse array of the selected MeshBlocks"""
        op = self.out_params
        pk = pm.pmb_pack
        f = op.coarsen_factor
        self._load_ranges(pm)
        self.outarray = None
        if not self.outmbs:
            return
        o = self.outmbs[0]
        nc = ((o.oie - o.ois + 1)//f, (o.oje - o.ojs + 1)//f, (o.oke - o.oks + 1)//f)
        nout = len(self.outvars)*(4 if op.compute_moments else 1)
        out = np.empty((nout, len(self.outmbs), nc[2], nc[1], nc[0]), dtype=np.float64)
        # one launch over the pack per distinct first cell: one, unless a slice (f = 1) cuts MeshBlocks of different levels
        by_lo = {}
        for mi, o in enumerate(self.outmbs):
            by_lo.setdefault((o.ois, o.ojs, o.oks), []).append((mi, o.mb_gid - pk.gids))
        for lo, mbs in by_lo.items():
            coarse = coarsen_pack(pk, self.outvars, f, op.compute_moments, lo, nc)
            sel = coarse[:, [m for _, m in mbs]] if len(mbs) != coarse.shape[1] else coarse
            out[:, [mi for mi, _ in mbs]] = _to_numpy(sel)
        self.outarray = out

    def WriteOutputFile(self, pm, pin):
        """coarsened_binary.cpp:298-530: the pre-header of a bin file plus the number of moments and the factor, the
        parameter dump, then per MeshBlock 10 int32, 6 Real and the coarse variables as float32 [n][k][j][i].  The six
        indices are ois, ois+nc1-1, ... (:416-421): the reference's reader takes the coarse extents from them."""
        op = self.out_params
        f = op.coarsen_factor
        fname = "%s/%s.%s.%05d.cbin" % (self.dir_name, op.file_basename, op.file_id, op.file_number)
        labels = coarsen_labels(self.outvars, op.compute_moments)
        msg = ("Athena binary output version=1.1\n  size of preheader=7\n  time=%.16e\n  cycle=%d\n"
               "  number of moments=%d\n  coarsening factor=%d\n  size of location=8\n  size of variable=4\n"
               "  number of variables=%d\n  variables:  "
               % (pm.time, pm.ncycle, 4 if op.compute_moments else 1, f, len(labels)))
        msg += "".join("%s  " % lab for lab in labels) + "\n"
        dump = pin.ParameterDump()
        hdr = (msg + "  header offset=%d\n" % len(dump) + dump).encode("ascii")
        if pm.my_rank == 0:
            with open(fname, "wb") as fp:
                fp.write(hdr)
        _barrier(pm)
        for r in range(pm.nranks):
            if r == pm.my_rank and self.outmbs:
                nc3, nc2, nc1 = self.outarray.shape[2:]
                with open(fname, "ab") as fp:
                    for mi, o in enumerate(self.outmbs):
                        l1, l2, l3 = pm.lloc_eachmb[o.mb_gid][:3]
                        fp.write(struct.pack("<10i", o.ois, o.ois + nc1 - 1, o.ojs, o.ojs + nc2 - 1, o.oks, o.oks + nc3 - 1,
                                             l1, l2, l3, pm.level_of(o.mb_gid) - pm.root_level))
                        fp.write(struct.pack("<6d", o.x1min, o.x1max, o.x2min, o.x2max, o.x3min, o.x3max))
                        with np.errstate(over="ignore"):          # a moment beyond float32 is written as inf
                            fp.write(np.ascontiguousarray(self.outarray[:, mi]).astype("<f4").tobytes())
            _barrier(pm)
        self._advance(pm, pin)


class RestartOutput(BaseTypeOutput):
    """restart.cpp:37-560: one file rst/<basename>.<NNNNN>.rst holding the parameter dump, the mesh
    header, the logical locations and costs of all MeshBlocks and, per MeshBlock (in gid order,
    `data_size` bytes each), the full-precision dependent variables INCLUDING ghost zones:
    [hydro u0][mhd u0][b0.x1f][b0.x2f][b0.x3f].  read_restart() below is the inverse."""

    def __init__(self, pin, pm, op):
        super().__init__(pin, pm, op)
        if pin.GetOrAddBoolean(op.block_name, "single_file_per_rank", False):
            _fatal("single_file_per_rank restart files are not on this path")
        if pm.my_rank == 0:
            os.makedirs("rst", exist_ok=True)

    def LoadOutputData(self, pm):
        """restart.cpp:53-137: everything is taken from the physics arrays at write time"""

    def WriteOutputFile(self, pm, pin):
        op = self.out_params
        fname = os.path.join("rst", "%s.%05d.rst" % (op.file_basename, op.file_number))
        # counters advance first so that the values for the NEXT dump are in the file (restart.cpp:193-200)
        self._advance(pm, pin)
        sbuf = pin.ParameterDump().encode()
        pk = pm.pmb_pack
        arrays = []               # per physics: list of tensors whose [m] slices form one record
        if pk.phydro is not None:
            arrays.append(pk.phydro.u0)
        if pk.pmhd is not None:
            arrays += [pk.pmhd.u0, pk.pmhd.b0.x1f, pk.pmhd.b0.x2f, pk.pmhd.b0.x3f]
        data_size = sum(int(a[0].numel())*8 for a in arrays)
        header = bytearray()
        header += struct.pack("<ii", pm.nmb_total, _root_level(pm))
        header += _pack_region_size(pm.mesh_size, pm.mesh_indcs)
        header += _pack_region_indcs(pm.mesh_indcs, coarse=False)
        header += _pack_region_indcs(pm.mb_indcs, coarse=True)
        header += struct.pack("<ddi", pm.time, pm.dt, pm.ncycle)
        for gid, l in enumerate(pm.lloc_eachmb):              # LogicalLocation {lx1,lx2,lx3,level}: the block's own level
            header += struct.pack("<iiii", l[0], l[1], l[2], pm.level_of(gid))
        header += np.asarray(pm.cost_eachmb, dtype="<f4").tobytes()
        header += struct.pack("<Q", data_size)
        base = len(sbuf) + len(header)
        if pm.my_rank == 0:
            with open(fname, "wb") as f:
                f.write(sbuf)
                f.write(header)
                f.truncate(base + data_size*pm.nmb_total)
        _barrier(pm)
        with open(fname, "r+b") as f:
            for m in range(pk.nmb_thispack):
                f.seek(base + data_size*(pk.gids + m))
                for a in arrays:
                    f.write(np.ascontiguousarray(_to_numpy(a[m]), dtype="<f8").tobytes())
        _barrier(pm)


def _root_level(pm):
    """build_tree.cpp:43-44"""
    nmbmax = max(pm.nmb_rootx1, pm.nmb_rootx2, pm.nmb_rootx3)
    lev = 0
    while (1 << lev) < nmbmax:
        lev += 1
    return lev


def _pack_region_size(ms, ind):
    """struct RegionSize {x1min,x2min,x3min,x1max,x2max,x3max,dx1,dx2,dx3} (mesh.hpp:25-29)"""
    dx = ((ms.x1max - ms.x1min)/float(ind.nx1), (ms.x2max - ms.x2min)/float(ind.nx2),
          (ms.x3max - ms.x3min)/float(ind.nx3))
    return struct.pack("<9d", ms.x1min, ms.x2min, ms.x3min, ms.x1max, ms.x2max, ms.x3max, *dx)


def _pack_region_indcs(ind, coarse):
    """struct RegionIndcs (mesh.hpp:35-41): 19 ints; the coarse members are only set for MeshBlocks
    (mesh.cpp:286-330)"""
    v = [ind.ng, ind.nx1, ind.nx2, ind.nx3, ind.is_, ind.ie, ind.js, ind.je, ind.ks, ind.ke]
    if coarse:
        cjs = ind.ng if ind.nx2 > 1 else 0
        cks = ind.ng if ind.nx3 > 1 else 0
        v += [ind.cnx1, ind.cnx2, ind.cnx3, ind.ng, ind.ng + ind.cnx1 - 1,
              cjs, cjs + ind.cnx2 - 1 if ind.nx2 > 1 else 0, cks, cks + ind.cnx3 - 1 if ind.nx3 > 1 else 0]
    else:
        v += [0]*9
    return struct.pack("<19i", *v)


_RST_HEADER = 2*4 + 9*8 + 2*19*4 + 2*8 + 4          # restart.cpp:296-297 "step1size" without the dump


def read_restart(path):
    """Inverse of RestartOutput: returns (parameter text, header dict, per-gid record reader).
    Mirrors ParameterInput::LoadFromFile (stop at <par_end>), Mesh::BuildTreeFromRestart
    (build_tree.cpp:315-370) and the restart constructor of ProblemGenerator (pgen.cpp:97-330)."""
    with open(path, "rb") as f:
        blob = f.read(1 << 16)
    end = blob.find(b"<par_end>")
    if end < 0:
        _fatal("<par_end> is not found in the first 64KBytes of restart file " + path)
    end = blob.index(b"\n", end) + 1
    text = blob[:end].decode()
    with open(path, "rb") as f:
        f.seek(end)
        h = f.read(_RST_HEADER)
        nmb_total, root_level = struct.unpack_from("<ii", h, 0)
        mesh_size = struct.unpack_from("<9d", h, 8)
        mesh_indcs = struct.unpack_from("<19i", h, 80)
        mb_indcs = struct.unpack_from("<19i", h, 156)
        time, dt, ncycle = struct.unpack_from("<ddi", h, 232)
        lloc = np.frombuffer(f.read(16*nmb_total), dtype="<i4").reshape(nmb_total, 4).copy()
        cost = np.frombuffer(f.read(4*nmb_total), dtype="<f4").copy()
        (data_size,) = struct.unpack("<Q", f.read(8))
        base = f.tell()
    hdr = dict(nmb_total=nmb_total, root_level=root_level, mesh_size=mesh_size, mesh_indcs=mesh_indcs,
               mb_indcs=mb_indcs, time=time, dt=dt, ncycle=ncycle, lloc=lloc, cost=cost,
               data_size=data_size, data_offset=base)

    def record(gid):
        with open(path, "rb") as f:
            f.seek(base + data_size*gid)
            return np.frombuffer(f.read(data_size), dtype="<f8")
    return text, hdr, record


class Outputs:
    """outputs.cpp:47-304"""

    def __init__(self, pin, pm):
        self.pout_list = []
        num_hst = num_rst = 0
        user_hist_of(pin)          # a user history function this path cannot enrol stops the run, hst block or not
        for name in list(pin.blocks):
            if not name.startswith("output"):
                continue
            op = OutputParameters()
            op.block_number = int(name[6:] or 0)
            op.block_name = name
            op.last_time = pin.GetOrAddReal(name, "last_time", -1.0)
            if pin.DoesParameterExist(name, "dcycle"):
                op.dcycle = pin.GetInteger(name, "dcycle")
                op.dt = 0.0
            else:
                op.dt = pin.GetReal(name, "dt")
                op.dcycle = 0
            if op.dcycle == 0 and op.dt <= 0.0:
                continue
            op.file_number = pin.GetOrAddInteger(name, "file_number", 0)
            op.file_basename = pin.GetString("job", "basename")
            op.file_type = pin.GetString(name, "file_type")
            if op.file_type not in ("hst", "rst", "log", "trk"):
                op.variable = pin.GetString(name, "variable")
                op.file_id = pin.GetOrAddString(name, "id", op.variable)
            op.include_gzs = pin.GetOrAddBoolean(name, "ghost_zones", False)
            op.gid = pin.GetOrAddInteger(name, "gid", -1)
            if op.gid >= 0 and pm.nmb_total == 1:
                _fatal("Cannot specify MeshBlock ID in output block '%s' when there is only one" % name)
            if op.gid > pm.nmb_total - 1:
                _fatal("MeshBlock gid=%d in output block '%s' exceeds total number of MeshBlocks"
                       % (op.gid, name))
            ms = pm.mesh_size
            for q, lo, hi in ((1, ms.x1min, ms.x1max), (2, ms.x2min, ms.x2max), (3, ms.x3min, ms.x3max)):
                key = "slice_x%d" % q
                if pin.DoesParameterExist(name, key):
                    x = pin.GetReal(name, key)
                    if not (lo <= x < hi):
                        _fatal("Slice at x%d=%g in output block '%s' is out of range of Mesh" % (q, x, name))
                    setattr(op, key, x)
                    setattr(op, "slice%d" % q, True)
            if op.file_type == "pdf":
                _pdf_group_check(name, op.variable)
            if op.file_type == "pdf" and pin.DoesBlockExist("ion-neutral"):
                _fatal("pdf output of a run with two fluids (<ion-neutral>) is not on this path yet (output block '%s')"
                       % name)
            if op.file_type == "rst" and pin.DoesBlockExist("ion-neutral"):
                _fatal("rst output with <ion-neutral>: restart files of a two-fluid run (the stiff source terms of the "
                       "ImEx integrator) are not on this path yet (output block '%s')" % name)
            if op.file_type == "rst" and pin.DoesBlockExist("turb_driving"):
                _fatal("rst output with <turb_driving>: restarting a driven run (force array and RNG state) is "
                       "not on this path yet (output block '%s')" % name)
            if op.file_type == "hst":
                op.user_hist_only = pin.GetOrAddBoolean(name, "user_hist_only", False)
                if op.user_hist_only and not user_hist_of(pin):                  # outputs.cpp:209-213
                    _fatal("User-history file requested in output block '%s', but <problem>/user_hist is not true"
                           % name)
            op.data_format = " " + pin.GetOrAddString(name, "data_format", "%12.5e")
            if op.file_type == "tab":
                self.pout_list.insert(0, FormattedTableOutput(pin, pm, op))
            elif op.file_type == "hst":
                self.pout_list.insert(0, HistoryOutput(pin, pm, op))
                num_hst += 1
            elif op.file_type == "pdf":                                          # outputs.cpp:252-273
                op.bin_min = pin.GetReal(name, "bin_min")
                op.bin_max = pin.GetReal(name, "bin_max")
                op.nbin = pin.GetInteger(name, "nbin")
                op.logscale = pin.GetOrAddBoolean(name, "logscale", True)
                op.mass_weighted = pin.GetOrAddBoolean(name, "mass_weighted", False)
                if pin.DoesParameterExist(name, "variable_2"):
                    op.variable_2 = pin.GetString(name, "variable_2")
                    op.bin2_min = pin.GetOrAddReal(name, "bin2_min", 0.0)
                    op.bin2_max = pin.GetOrAddReal(name, "bin2_max", 1.0)
                    op.nbin2 = pin.GetOrAddInteger(name, "nbin2", 0)
                    op.logscale2 = pin.GetOrAddBoolean(name, "logscale2", True)
                self.pout_list.insert(0, PDFOutput(pin, pm, op))
            elif op.file_type == "bin":
                self.pout_list.insert(0, MeshBinaryOutput(pin, pm, op))
            elif op.file_type == "cbin":                                         # outputs.cpp:247-249
                op.coarsen_factor = pin.GetInteger(name, "coarsen_factor")
                op.compute_moments = pin.GetOrAddBoolean(name, "compute_moments", False)
                self.pout_list.insert(0, CoarsenedBinaryOutput(pin, pm, op))
            elif op.file_type == "rst":
                # tail end of the list, so that the file counters of the other output types are
                # up to date in the restart file (outputs.cpp:285-292)
                self.pout_list.append(RestartOutput(pin, pm, op))
                num_rst += 1
            else:
                _fatal("Unrecognized or unsupported file format = '%s' in output block '%s' "
                       "(tab, hst, bin, cbin, pdf, rst on this path)" % (op.file_type, name))
        if num_hst > 1 or num_rst > 1:
            _fatal("More than one history or restart output block found in input file")

    def MakeOutputs(self, pm, pin):
        for out in self.pout_list:
            out.LoadOutputData(pm)
            out.WriteOutputFile(pm, pin)

    def TestAndMakeOutputs(self, pm, pin, tlim):
        """driver.cpp:432-445 (comparison at 32-bit precision, as the reference)"""
        time_32 = np.float32(pm.time)
        tlim_32 = np.float32(tlim)
        for out in self.pout_list:
            op = out.out_params
            next_32 = np.float32(op.last_time + op.dt)
            if ((op.dt > 0.0 and time_32 >= next_32 and time_32 < tlim_32) or
                    (op.dcycle > 0 and pm.ncycle % op.dcycle == 0)):
                out.LoadOutputData(pm)
                out.WriteOutputFile(pm, pin)
