"""TEST INFRASTRUCTURE: whole adaptive runs of the Python host, on the GPU ("cuda") or on the CPU backend of
tests/amr_cases.py ("cpu"), recorded the same way so that the two can be compared bit for bit."""
import os

import numpy as np

import amr_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECKS = os.path.join(ROOT, "athenak_amd", "inputs")


def _region(level, lo, hi, ndim, n=1):
    s = "<refined_region%d>\nlevel = %d\n" % (n, level)
    for d in range(ndim):
        s += "x%dmin = %s\nx%dmax = %s\n" % (d + 1, lo, d + 1, hi)
    return s


# A blast refines at once (the slope of the density at the edge of the hot sphere).  The quiet corner starts refined
# by a <refined_region>, where the slope is zero: its blocks are merged as soon as refinement_interval allows -- so
# twelve cycles hold refinements and derefinements, on the 2:1 rule's terms (three levels in the 2-D run).
WHOLE_RUNS = {
    "blast_mhd_2d": ("blast_mhd_amr.athinput",
                     ["mesh/nx1=32", "mesh/nx2=32", "meshblock/nx1=8", "meshblock/nx2=8", "mesh_refinement/num_levels=3",
                      "mesh_refinement/refinement_interval=2"], _region(1, -0.45, -0.3, 2)),
    "blast_hydro_3d": ("blast_hydro_amr.athinput",
                       ["mesh/nx1=16", "mesh/nx2=16", "mesh/nx3=16", "meshblock/nx1=4", "meshblock/nx2=4",
                        "meshblock/nx3=4", "mesh_refinement/num_levels=2", "mesh_refinement/refinement_interval=2"],
                       _region(1, -0.45, -0.3, 3)),
}
_FROZEN_OV = ["mesh/nx1=32", "mesh/nx2=32", "meshblock/nx1=8", "meshblock/nx2=8", "mesh_refinement/num_levels=2",
              "amr_criterion0/value_max=1.0e30", "mesh_refinement/refinement_interval=1000000"]


def _text(deck, extra):
    return open(os.path.join(DECKS, deck)).read() + "\n" + extra


def _frozen(adaptive):
    """an adaptive deck with a <refined_region1> and a criterion that never fires (value_max far above the data), and
    the same deck under refinement = static.  A maximum below value_max asks for derefinement, which the blocks of the
    region would get; refinement_interval longer than the run keeps every block at rest, so the criteria kernel runs
    every cycle and the mesh stays what the region made it."""
    t = _text("blast_mhd_amr.athinput", _region(1, -0.1, 0.1, 2))
    if not adaptive:
        t = t.replace("refinement = adaptive", "refinement = static")
    return t


def _sim(case):
    from athenak_amd.main import Simulation
    from athenak_amd.parameter_input import ParameterInput
    if case in WHOLE_RUNS:
        deck, ov, extra = WHOLE_RUNS[case]
        pin = ParameterInput(text=_text(deck, extra))
        pin.ModifyFromCmdline(list(ov))
    else:
        pin = ParameterInput(text=_frozen(case == "frozen_adaptive"))
        pin.ModifyFromCmdline(list(_FROZEN_OV))
    return Simulation(pin)


def _record(sim, leaves):
    pm = sim.pmesh
    pk = pm.pmb_pack
    arrays = {}
    if pk.phydro is not None:
        arrays["hydro_u0"] = pk.phydro.u0.cpu().numpy().copy()
    if pk.pmhd is not None:
        arrays["mhd_u0"] = pk.pmhd.u0.cpu().numpy().copy()
        for n in ("x1f", "x2f", "x3f"):
            arrays["b0_" + n] = getattr(pk.pmhd.b0, n).cpu().numpy().copy()
    pmr = pm.pmr
    return dict(leaves=leaves, dt=pm.dt, time=pm.time, arrays=arrays, created=pmr.nmb_created if pmr else 0,
                deleted=pmr.nmb_deleted if pmr else 0)


def run(case, device, cycles=12):
    """device "cpu": in this process, with athenak_amd.capi switched to the CPU backend for the run and back after"""
    if device == "cpu":
        ac.install_cpu_backend()
    try:
        sim = _sim(case)
        leaves = []
        for _ in range(cycles):
            assert sim.Execute(max_cycles=1) == 1
            leaves.append([tuple(l) for l in sim.pmesh.lloc_eachmb])
        return _record(sim, leaves)
    finally:
        if device == "cpu":
            ac.uninstall_cpu_backend()


def outputs_across_regrid(rundir, device):
    """blast_mhd_2d with hst and bin every cycle, a few cycles across its first regrids -> the number of MeshBlock
    records per bin file (split by the version-1.1 layout of the reference's bin_convert.read_binary, restated in
    tests/derived_cases.read_bin: the reference's own module is not part of this repository), the hst mass column, and
    the bound of its jumps"""
    import derived_cases as dc
    from athenak_amd.main import Simulation
    from athenak_amd.outputs import Outputs
    from athenak_amd.parameter_input import ParameterInput
    if device == "cpu":
        ac.install_cpu_backend()
    cwd = os.getcwd()
    try:
        deck, ov, extra = WHOLE_RUNS["blast_mhd_2d"]
        more = "<output3>\nfile_type = tab\nvariable = mhd_w\nslice_x2 = 0.01\ndt = 1.0e-8\n"
        if device != "cpu":                 # a derived variable has its kernel on the device only
            more += "<output4>\nfile_type = bin\nvariable = mhd_divb\ndt = 1.0e-8\n"
        pin = ParameterInput(text=_text(deck, extra + more))
        pin.blocks["output1"]["data_format"] = "%24.16e"          # the history sums with all their digits
        pin.ModifyFromCmdline(list(ov) + ["output1/dt=1.0e-8", "output2/dt=1.0e-8", "time/nlim=4"])
        os.chdir(rundir)
        sim = Simulation(pin, initialize=False)
        pm, drv = sim.pmesh, sim.pdriver
        pout = Outputs(pin, pm)
        nmb_before = pm.nmb_total
        drv.Initialize(pm, pin, pout)
        drv.Execute(pm, pin)
        drv.Finalize(pm, pin, pout)
        nmb_after = pm.nmb_total
        files = sorted(f for f in os.listdir("bin") if f.endswith(".bin") and "mhd_w_bcc" in f)
        tabs = sorted(os.listdir("tab"))
        # one row per cell of every MeshBlock the slice x2 = 0.01 cuts (through the blast: refined later on)
        tab_rows = [sum(1 for l in open(os.path.join("tab", f)) if l.strip() and not l.startswith("#")) for f in tabs]
        divb = sorted(f for f in os.listdir("bin") if "mhd_divb" in f)
        divb_blocks = [len(dc.read_bin(os.path.join("bin", f))[1]) for f in divb]
        nmb_files = [len(dc.read_bin(os.path.join("bin", f))[1]) for f in files]
        hst = [f for f in os.listdir(".") if f.endswith(".hst")][0]
        rows = np.loadtxt(hst, comments="#", ndmin=2)
        mass, hst_time = rows[:, 2], rows[:, 0]
        # the bound of the conservation test (tests/test_amr_host.py derives it): 8 ulp of the largest term per coarse
        # cell.  The largest term is the mass of a root cell times nleaf (density 1 up to the blast's compression, which
        # the factor nleaf = 4 covers in these few cycles); every cell of the final mesh is counted as a coarse cell.
        # The history file carries the sum with all its digits (data_format = %24.16e), so nothing is added for it.
        ind = pm.mb_indcs
        vol = (1.0/32)**2
        ncoarse = pm.nmb_total*ind.nx1*ind.nx2
        bound = 8*np.spacing(1.0*vol*4)*ncoarse
        return dict(nmb_before=nmb_before, nmb_after=nmb_after, nmb_files=nmb_files, hst_mass=mass, mass_bound=bound,
                    tab_rows=tab_rows, divb_blocks=divb_blocks, nx1=ind.nx1,
                    bin_files=[os.path.join("bin", f) for f in files], hst_file=hst, hst_time=hst_time)
    finally:
        os.chdir(cwd)
        if device == "cpu":
            ac.uninstall_cpu_backend()
