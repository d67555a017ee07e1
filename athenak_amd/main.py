"""main(): deck -> Mesh -> physics -> ProblemGenerator -> Driver (src/main.cpp:61-420)."""
import os

from .driver import Driver
from .mesh import Mesh
from .parameter_input import ParameterInput
from .pgen import ProblemGenerator

_DECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "inputs")


class Simulation:
    """Steps 3-8 of the reference's main() (src/main.cpp:246-375)."""

    def __init__(self, pin, my_rank=0, nranks=1, initialize=True, restart=None):
        """restart = (header, record reader) of outputs.read_restart(): Mesh::BuildTreeFromRestart
        + the restart constructor of ProblemGenerator (main.cpp:329,355-360)"""
        self.pin = pin
        if restart is not None and pin.DoesBlockExist("ion-neutral"):
            raise RuntimeError("### FATAL ERROR -r of a deck with <ion-neutral>: restarting a two-fluid run is not on "
                               "this path yet")
        if restart is not None and pin.DoesBlockExist("gravity"):
            raise RuntimeError("### FATAL ERROR -r of a deck with <gravity>: restarting a self-gravitating run is not on "
                               "this path yet")
        if restart is not None:
            from .shearing_box import shearing_box_deck_checks
            shearing_box_deck_checks(pin, nranks, restart=True)
        self.pmesh = Mesh(pin, my_rank, nranks)
        if restart is not None and self.pmesh.adaptive:
            raise RuntimeError("### FATAL ERROR -r of a deck with <mesh_refinement>/refinement = adaptive: the restart "
                               "reader rebuilds the mesh from the deck, not from the file")
        self.pmesh.AddCoordinatesAndPhysics(pin)
        if restart is not None:
            self._load_restart(*restart)
        self.pmesh.pgen = ProblemGenerator(pin, self.pmesh, restart=restart is not None)
        self.pdriver = Driver(pin, self.pmesh)      # after pgen: linear_wave rescales tlim
        if initialize:
            self.pdriver.Initialize(self.pmesh, pin)

    def _load_restart(self, hdr, record):
        import numpy as np
        import torch
        pm = self.pmesh
        ind = pm.mb_indcs
        got = (hdr["nmb_total"], hdr["mb_indcs"][:4], hdr["mesh_indcs"][:4])
        want = (pm.nmb_total, (ind.ng, ind.nx1, ind.nx2, ind.nx3),
                (pm.mesh_indcs.ng, pm.mesh_indcs.nx1, pm.mesh_indcs.nx2, pm.mesh_indcs.nx3))
        if got != want:
            raise RuntimeError("### FATAL ERROR mesh in the restart file %r does not match the "
                               "parameters %r" % (got, want))
        lloc = [tuple(int(x) for x in l[:4]) for l in hdr["lloc"]]          # (lx1, lx2, lx3, level) per block
        if lloc != [tuple(l)[:3] + (pm.level_of(g),) for g, l in enumerate(pm.lloc_eachmb)]:
            raise RuntimeError("### FATAL ERROR MeshBlock order or refinement levels of the restart file differ")
        pm.time, pm.dt, pm.ncycle = hdr["time"], hdr["dt"], hdr["ncycle"]   # build_tree.cpp:365-369
        pk = pm.pmb_pack
        arrays = []
        if pk.phydro is not None:
            arrays.append(pk.phydro.u0)
        if pk.pmhd is not None:
            arrays += [pk.pmhd.u0, pk.pmhd.b0.x1f, pk.pmhd.b0.x2f, pk.pmhd.b0.x3f]
        if sum(int(a[0].numel())*8 for a in arrays) != hdr["data_size"]:
            raise RuntimeError("### FATAL ERROR CC data size read from restart file not equal to size "
                               "of Hydro and/or MHD arrays, restart file is broken.")
        for m in range(pk.nmb_thispack):
            rec = record(pk.gids + m)
            off = 0
            for a in arrays:
                n = int(a[m].numel())
                a[m].copy_(torch.from_numpy(np.array(rec[off:off + n])).reshape(a[m].shape))
                off += n

    @property
    def phys(self):
        pk = self.pmesh.pmb_pack
        return pk.phydro if pk.phydro is not None else pk.pmhd

    def phi(self):
        """the gravitational potential of the last Solve, (nmb, 1, N3, N2, N1); zero before the first cycle"""
        pg = self.pmesh.pmb_pack.pgrav
        if pg is None:
            raise RuntimeError("### FATAL ERROR the gravitational potential needs a <gravity> block")
        return pg.phi

    @property
    def psbox_u(self):
        """the ShearingBoxCC of the fluid (qshear, omega0, yshear); None without a <shearing_box> block"""
        return getattr(self.phys, "psbox_u", None)

    @property
    def porb_u(self):
        """the OrbitalAdvectionCC of the fluid (maxjshift); None without a <shearing_box> block"""
        return getattr(self.phys, "porb_u", None)

    @property
    def psbox_b(self):
        """the ShearingBoxFC of an MHD fluid; None for hydro or without a <shearing_box> block"""
        return getattr(self.phys, "psbox_b", None)

    @property
    def porb_b(self):
        """the OrbitalAdvectionFC of an MHD fluid; None for hydro or without a <shearing_box> block"""
        return getattr(self.phys, "porb_b", None)

    @property
    def omega_measured(self):
        """pgen_name = gravity: the frequency / growth rate its final function measured (None before it has run)"""
        return getattr(self.pmesh.pgen, "omega_measured", None)

    def binary_gravity_errors(self):
        """pgen_name = binary_gravity: (potential L2, acceleration L2, max potential error, max acceleration error) of
        the present potential against the analytic two-sphere solution, as the final function prints them"""
        pgen = self.pmesh.pgen
        if getattr(pgen, "pgen_name", None) != "binary_gravity":
            raise RuntimeError("### FATAL ERROR binary_gravity_errors needs <problem>/pgen_name = binary_gravity")
        pgen.BinaryGravityErrors()
        return pgen.binary_errors

    @property
    def omega_analytical(self):
        return getattr(self.pmesh.pgen, "omega_analytical", None)

    def derived(self, name):
        """a derived output variable of the present state ("mhd_j2", "hydro_wz", ... or "temperature") as a
        (nmb, 1, N3, N2, N1) tensor, as NativeSimulation.derived"""
        from .outputs import derived_array, derived_which
        ph = self.phys
        which, _, _ = derived_which(name, self.pmesh.pmb_pack.pmhd is not None, ph.peos.eos_data.is_ideal)
        return derived_array(ph, which)

    def pdf(self, variable, bin_min, bin_max, nbin, logscale=True, mass_weighted=False, variable_2=None, bin2_min=0.0,
            bin2_max=1.0, nbin2=0, logscale2=True, force_global=False):
        """the histogram a pdf output block with these keys writes, of the present state over the whole mesh
        (outputs.PdfResult: bins, counts, weights); force_global takes the global-atomic path of akmi_pdf"""
        from .outputs import PdfResult, pdf_axes, pdf_histogram
        pk = self.pmesh.pmb_pack
        axes = pdf_axes(pk, variable, bin_min, bin_max, nbin, logscale, variable_2, bin2_min, bin2_max, nbin2, logscale2)
        return PdfResult(axes, *pdf_histogram(pk, axes, mass_weighted, force_global))

    def turb_history(self):
        """the eleven sums of the turbulence history columns (capi.TURB_HIST_LABELS) of the present state of an MHD
        run, over the whole mesh"""
        from .outputs import turb_history_sums
        pk = self.pmesh.pmb_pack
        if pk.pmhd is None:
            raise RuntimeError("### FATAL ERROR the turbulence history columns need an MHD run")
        return turb_history_sums(pk.pmhd, pk)

    def coarsen(self, variable, factor, moments=False, ghost_zones=False, staged=None):
        """(labels, tensor) a cbin output block with these keys holds of the present state, for this rank's MeshBlocks:
        the tensor is (nvars*nmom, nmb, nc3, nc2, nc1), the mean over factor^3 cells of every variable of the group and,
        with moments, of its 2nd to 4th power (nmom = 4, adjacent).  staged picks the form of akmi_coarsen (None: the
        library's default); both give the same bits."""
        from .outputs import coarsen_variable
        return coarsen_variable(self.pmesh.pmb_pack, variable, factor, moments, ghost_zones, staged)

    def Execute(self, max_cycles=None):
        return self.pdriver.Execute(self.pmesh, self.pin, max_cycles)


def load_deck(name_or_path, overrides=()):
    path = name_or_path
    if not os.path.exists(path):
        path = os.path.join(_DECKS, name_or_path)
    pin = ParameterInput(filename=path)
    pin.ModifyFromCmdline(list(overrides))
    return pin


def load_restart(path, overrides=(), my_rank=0, nranks=1, initialize=True):
    """athena -r <file> [overrides]: main.cpp:248-293,329,355-365.  Outputs, if wanted, are created
    by the caller from sim.pin (their file_number/last_time continue from the file)."""
    from .outputs import read_restart
    text, hdr, record = read_restart(path)
    pin = ParameterInput(text=text)
    pin.ModifyFromCmdline(list(overrides))
    return Simulation(pin, my_rank, nranks, initialize=initialize, restart=(hdr, record))


def run_deck(name_or_path, overrides=(), my_rank=0, nranks=1, max_cycles=None):
    sim = Simulation(load_deck(name_or_path, overrides), my_rank, nranks)
    sim.Execute(max_cycles)
    return sim
