"""NativeSimulation: the C++ host driver (csrc/akmi_host.cpp) behind the same Python surface
as main.Simulation.  Mesh, MeshBlockPack, TaskList, Hydro/MHD tasks and the Driver loop run
in C++ (akmi_sim_*); Python only evaluates the closed-form initial conditions into the native
device arrays (aliased as torch tensors through __cuda_array_interface__)."""
import ctypes as C

import torch

from . import capi
from .mesh import Mesh
from .pgen import ProblemGenerator


class _DevAlias:
    """exposes a raw device pointer to torch (zero-copy)"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (ptr, False),
                                         "version": 3, "strides": None}


class _Face:
    pass


class _Eos:
    def __init__(self, pin, blk):
        ideal = pin.GetString(blk, "eos") == "ideal"
        self.eos_data = type("EOS_Data", (), {
            "gamma": pin.GetReal(blk, "gamma") if ideal else 0.0, "is_ideal": ideal,
            "iso_cs": 0.0 if ideal else pin.GetReal(blk, "iso_sound_speed")})()


class _PhysAlias:
    """the attributes ProblemGenerator needs, backed by the native arrays"""


class NativeSimulation:
    def __init__(self, pin, initialize=True):
        self.pin = pin
        if pin.DoesBlockExist("mesh_refinement") and pin.GetOrAddString("mesh_refinement", "refinement", "none") == "adaptive":
            # said here, before the C++ host parses the deck (it would end the process with its own message)
            raise RuntimeError("### FATAL ERROR <mesh_refinement>/refinement = adaptive runs on the Python host only "
                               "(--host python): the C++ host builds none or static refinement")
        if pin.DoesBlockExist("ion-neutral"):
            raise RuntimeError("### FATAL ERROR <ion-neutral> runs on the Python host only (--host python): the C++ host "
                               "(--host native) has neither the two-fluid task list nor the ImEx integrators")
        if pin.DoesBlockExist("gravity"):
            raise RuntimeError("### FATAL ERROR <gravity> runs on the Python host only (--host python): the C++ host "
                               "(--host native) has no multigrid driver")
        from .shearing_box import shearing_box_native_refusal
        shearing_box_native_refusal(pin)
        self.L = capi.lib()
        stream = capi._stream()
        h = self.L.akmi_sim_create(pin.Dump().encode(), stream)
        if not h:       # a run-time failure (device allocation, HIP); deck errors exit with "### FATAL ERROR" as the reference does
            raise capi.AkmiError("akmi_sim_create failed: %s" % self.L.akmi_last_error().decode())
        self.h = C.c_void_p(h)
        # a Python Mesh of the same deck gives the problem generators their coordinates; with a
        # communicator (akmi_comm_init_*) both sides cut the block list the same way
        # (tests/test_host_plan.py) and the arrays are those of this rank's pack
        self.pmesh = Mesh(pin, my_rank=self.L.akmi_comm_rank(), nranks=self.L.akmi_comm_nranks())
        assert self.pmesh.pmb_pack.gids == self.L.akmi_sim_gids(self.h)
        is_mhd = pin.DoesBlockExist("mhd")
        blk = "mhd" if is_mhd else "hydro"
        n3, n2, n1 = self.pmesh.mb_indcs.ncells
        nmb = self.pmesh.pmb_pack.nmb_thispack
        assert nmb == self.L.akmi_sim_nmb_thisrank(self.h)
        ph = _PhysAlias()
        ph.peos = _Eos(pin, blk)
        ph.nfluid = 5 if ph.peos.eos_data.is_ideal else 4
        ph.nscalars = pin.GetOrAddInteger(blk, "nscalars", 0)
        ph.nvars = nv = ph.nfluid + ph.nscalars
        self._shape = (is_mhd, nmb, nv, n3, n2, n1)
        self._phys = ph
        ph.native_sim = self          # outputs.coarsen_pack goes through akmi_sim_coarsen (close() drops the reference)
        self._refresh()
        if is_mhd:
            self.pmesh.pmb_pack.pmhd = ph
        else:
            self.pmesh.pmb_pack.phydro = ph
        self.pmesh.pgen = ProblemGenerator(pin, self.pmesh)
        if initialize:
            self.Initialize()

    def _refresh(self):
        """(re)alias the native arrays: the C++ host swaps its two registers (u0/u1, b0/b1) after an
        out-of-place first stage, so the pointers behind the names change from call to call"""
        is_mhd, nmb, nv, n3, n2, n1 = self._shape
        ph = self._phys
        ph.u0 = self._alias("u0", (nmb, nv, n3, n2, n1))
        ph.w0 = self._alias("w0", (nmb, nv, n3, n2, n1))
        ph.u1 = self._alias("u1", (nmb, nv, n3, n2, n1))
        if is_mhd:
            ph.bcc0 = self._alias("bcc0", (nmb, 3, n3, n2, n1))
            for reg in ("b0", "b1"):
                f = _Face()
                f.x1f = self._alias(reg + "x1f", (nmb, n3, n2, n1 + 1))
                f.x2f = self._alias(reg + "x2f", (nmb, n3, n2 + 1, n1))
                f.x3f = self._alias(reg + "x3f", (nmb, n3 + 1, n2, n1))
                setattr(ph, reg, f)

    def _alias(self, name, shape):
        cnt = C.c_longlong(0)
        p = self.L.akmi_sim_array(self.h, name.encode(), C.byref(cnt))
        n = 1
        for s in shape:
            n *= s
        assert p and cnt.value == n, (name, cnt.value, n)
        return torch.as_tensor(_DevAlias(p, shape), device="cuda")

    @property
    def phys(self):
        return self._phys

    def Initialize(self):
        torch.cuda.synchronize()
        capi.check(self.L.akmi_sim_initialize(self.h, self.pin.GetReal("time", "tlim")), "sim_initialize")

    def Execute(self, max_cycles=None):
        n = capi.check(self.L.akmi_sim_execute(self.h, -1 if max_cycles is None else int(max_cycles)), "sim_execute")
        self._refresh()
        self.pmesh.time = self.time
        self.pmesh.dt = self.dt
        self.pmesh.ncycle = self.ncycle
        return n

    def derived(self, name):
        """a derived output variable of the present state ("mhd_j2", "hydro_wz", ... or "temperature") as a
        (nmb, 1, N3, N2, N1) tensor: akmi_sim_derived runs the kernel of the outputs on the native arrays"""
        from .outputs import derived_which
        is_mhd, nmb, _, n3, n2, n1 = self._shape
        which, ncomp, _ = derived_which(name, is_mhd, self._phys.peos.eos_data.is_ideal)
        return self.derived_by_number(which, ncomp)

    def derived_by_number(self, which, ncomp=1):
        """the derived variable AKMI_DV_<which> as derived() returns it"""
        _, nmb, _, n3, n2, n1 = self._shape
        out = torch.empty((nmb, ncomp, n3, n2, n1), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        capi.check(self.L.akmi_sim_derived(self.h, which, out), "sim_derived")
        return out

    def coarsen(self, variable, factor, moments=False, ghost_zones=False, staged=None):
        """as Simulation.coarsen: akmi_sim_coarsen runs the kernel of the cbin outputs on the native arrays"""
        from .outputs import coarsen_variable
        return coarsen_variable(self.pmesh.pmb_pack, variable, factor, moments, ghost_zones, staged)

    _STORED = {"u0": 0, "w0": 1, "bcc0": 2}          # akmi_sim_pdf: a stored array by number

    def pdf(self, variable, bin_min, bin_max, nbin, logscale=True, mass_weighted=False, variable_2=None, bin2_min=0.0,
            bin2_max=1.0, nbin2=0, logscale2=True, force_global=False):
        """as Simulation.pdf: akmi_sim_pdf runs the kernel of the pdf outputs on the native arrays"""
        from .outputs import PdfResult, pdf_axes, pdf_reduce_ranks
        pk = self.pmesh.pmb_pack
        axes = pdf_axes(pk, variable, bin_min, bin_max, nbin, logscale, variable_2, bin2_min, bin2_max, nbin2, logscale2)
        keep, cax = [], []
        for (label, comp, arr), edges, step, log in axes:
            if arr.startswith("dv:"):
                name = variable if len(cax) == 0 else variable_2
                t = self.derived(name)
                keep.append(t)
                ptr, nv, comp = t.data_ptr(), 1, 0
            else:
                ptr, nv = None, self._STORED[arr]
            cax.append(capi.PdfAxis(ptr, nv, comp, len(edges) - 1, 1 if log else 0, float(edges[0]), float(edges[-1]),
                                    float(step)))
        shape = ((cax[1].nbin + 2) if len(cax) == 2 else 1, cax[0].nbin + 2)
        counts = torch.zeros(shape, dtype=torch.int64, device="cuda")
        weights = torch.zeros(shape, dtype=torch.float64, device="cuda")
        nan = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        capi.check(self.L.akmi_sim_pdf(self.h, cax[0], cax[1] if len(cax) == 2 else None, 1 if mass_weighted else 0,
                                       counts, weights, nan, 1 if force_global else 0), "sim_pdf")
        return PdfResult(axes, *pdf_reduce_ranks(self.pmesh, counts, weights, nan))

    def turb_history(self):
        """as Simulation.turb_history: akmi_sim_turb_history, the sums over the whole mesh in gid order"""
        if not self._shape[0]:
            raise RuntimeError("### FATAL ERROR the turbulence history columns need an MHD run")
        out = (C.c_double*capi.TURB_NHIST)()
        torch.cuda.synchronize()
        capi.check(self.L.akmi_sim_turb_history(self.h, out), "sim_turb_history")
        return [float(v) for v in out]

    def stage_forms(self, stage):
        """which forms (capi.FORM_*) stage `stage` (1-based) of the last cycle took: the x3 march from u0, k_sweep12s from
        u0, both from the face field, primitives that a lean conversion had left; -1 when no such stage has run"""
        return int(self.L.akmi_sim_stage_forms(self.h, int(stage)))

    def floor_counters(self):
        """(density, energy, temperature) floor counts of the conversions so far (EventCounters of the reference)"""
        out = (C.c_int*3)()
        capi.check(self.L.akmi_sim_counters(self.h, out), "sim_counters")
        return tuple(int(v) for v in out)

    time = property(lambda s: s.L.akmi_sim_time(s.h))
    dt = property(lambda s: s.L.akmi_sim_dt(s.h))
    tlim = property(lambda s: s.L.akmi_sim_tlim(s.h))
    ncycle = property(lambda s: s.L.akmi_sim_ncycle(s.h))

    def close(self):
        if self.h:
            self.L.akmi_sim_destroy(self.h)
            self.h = None
            self._phys.native_sim = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- ranks ------------------------------------------------------------------------------------------
_KEEP = []      # callbacks handed to C must outlive the communicator


def init_comm_from_torch_distributed():
    """Give the C++ host a communicator for the ranks of the initialised torch.distributed job.
    Backend nccl (= RCCL, one GPU per rank): rank 0 creates the RCCL id, a broadcast hands it to
    every rank, and from there on the C++ host calls RCCL itself (ncclSend/ncclRecv/ncclAllReduce).
    Any other backend: the C++ host stages its messages through pinned host memory and this
    module moves them with torch.distributed point-to-point operations (tests: gloo, two ranks
    sharing the only GPU of the box, which RCCL refuses)."""
    import numpy as np
    import torch.distributed as dist
    L = capi.lib()
    rank, world = dist.get_rank(), dist.get_world_size()
    if dist.get_backend() == "nccl":
        idb = C.create_string_buffer(128)
        if rank == 0:
            capi.check(L.akmi_comm_unique_id(idb), "comm_unique_id")
        t = torch.frombuffer(bytearray(idb.raw), dtype=torch.uint8).cuda()
        dist.broadcast(t, 0)
        capi.check(L.akmi_comm_init_rccl(rank, world, bytes(t.cpu().numpy().tobytes())), "comm_init_rccl")
        return "rccl"

    EX = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                     C.POINTER(C.c_longlong), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong))
    AR = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int)

    def view(ptr, n):
        return torch.from_numpy(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(n,)))

    def exchange(user, npeer, peers, sp, sc, rp, rc):
        try:
            ops = []
            for q in range(npeer):
                if rc[q] > 0:
                    ops.append(dist.P2POp(dist.irecv, view(rp[q], rc[q]), peers[q]))
            for q in range(npeer):
                if sc[q] > 0:
                    ops.append(dist.P2POp(dist.isend, view(sp[q], sc[q]), peers[q]))
            for w in (dist.batch_isend_irecv(ops) if ops else []):
                w.wait()
            return 0
        except Exception:      # never unwind through C
            import traceback
            traceback.print_exc()
            return 1

    def allreduce_min(user, vals, n):
        try:
            t = view(vals, n)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return 0
        except Exception:
            import traceback
            traceback.print_exc()
            return 1

    ex, ar = EX(exchange), AR(allreduce_min)
    _KEEP[:] = [ex, ar]
    capi.check(L.akmi_comm_init_callbacks(rank, world, ex, ar, None), "comm_init_callbacks")
    return "callbacks"


def finalize_comm():
    capi.lib().akmi_comm_finalize()
    _KEEP[:] = []
