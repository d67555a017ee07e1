"""Cost of the implicit update of two-fluid (ion-neutral) MHD, akmi_ionn_imp_update, at n^3 cells per fluid (one GPU).

python tools/ionn_profile.py kernel [n] [rounds]   the five calls of an imex3 cycle (istage = 1..5) on random states, `rounds`
                                                   times in that order after 3 warm-up rounds; HIP-event time per istage
python tools/ionn_profile.py host [n] [cycles]     a periodic two-fluid box of one MeshBlock through the whole host, imex3
python tools/ionn_profile.py parse <dir> [rounds]  the kernel times of a `rocprofv3 --kernel-trace --stats -d <dir> -- python
                                                   tools/ionn_profile.py kernel|host ...` run: per istage (kernel mode: the
                                                   launches of k_ionn_imp_update in trace order, warm-up dropped) beside the
                                                   counted bytes, and the share of all kernel time the implicit update takes

Counted traffic per cell: 8 + 8*(non-zero coefficients) doubles read; 16 written by a solving stage, 8 by the last."""
import csv
import ctypes as C
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM = 3
# imex3: non-zero coefficients of a_twid[istage-2][0..istage-2] and whether the stage solves
NONZERO = {1: 0, 2: 1, 3: 2, 4: 3, 5: 4}
SOLVES = {1: True, 2: True, 3: True, 4: True, 5: False}


def counted_bytes(istage, cells):
    return 8*cells*(8 + 8*NONZERO[istage] + (16 if SOLVES[istage] else 8))


def imex3_rows():
    from athenak_amd.driver import Driver
    from athenak_amd.parameter_input import ParameterInput
    d = Driver(ParameterInput(text="<time>\nintegrator = imex3\ntlim = 1.0\n<ion-neutral>\ndrag_coeff = 1.0\n"), None)
    return d


def run_kernel(n, rounds):
    import torch
    from athenak_amd import capi
    L = capi.lib()
    d = imex3_rows()
    cells = n*n*n
    g = torch.Generator(device="cuda").manual_seed(1)
    ui = torch.empty((1, 4, cells), dtype=torch.float64, device="cuda").normal_(generator=g)
    un = torch.empty((1, 4, cells), dtype=torch.float64, device="cuda").normal_(generator=g)
    ru = torch.empty((4, 1, 8, cells), dtype=torch.float64, device="cuda").normal_(generator=g).mul_(1e-3)
    ui[:, 0].uniform_(0.5, 1.5, generator=g)
    un[:, 0].uniform_(0.5, 1.5, generator=g)
    dt, drag = 1e-3, 1.0
    ev = {i: [] for i in range(1, 6)}
    for r in range(WARM + rounds):
        for istage in range(1, 6):
            adt = [d.a_twid[istage - 2][s]*dt for s in range(istage - 1)]
            adt_c = (C.c_double*max(len(adt), 1))(*adt)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            capi.check(L.akmi_ionn_imp_update(1, cells, 4, 4, 4, istage, 1 if SOLVES[istage] else 0, adt_c,
                                              drag*d.a_impl*dt, 0.0, 0.0, drag, 0.0, 0.0, ui, un, ru, capi._stream()),
                       "ionn_imp_update")
            b.record()
            if r >= WARM:
                ev[istage].append((a, b))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ui).all()) and bool(torch.isfinite(un).all())
    print("akmi_ionn_imp_update, imex3, %d^3 cells per fluid, %d rounds (HIP events round one launch)" % (n, rounds))
    for istage in range(1, 6):
        us = sorted(1e3*a.elapsed_time(b) for a, b in ev[istage])
        med = us[len(us)//2]
        by = counted_bytes(istage, cells)
        print("istage %d  median %8.1f us  min %8.1f  max %8.1f   counted %6.1f MB   %6.0f GB/s" % (
            istage, med, us[0], us[-1], by/1e6, by/med/1e3), flush=True)


_BOX = """
<job>
basename = ionn_profile
<mesh>
nghost = 2
nx1 = {n}
x1min = -0.5
x1max = 0.5
ix1_bc = periodic
ox1_bc = periodic
nx2 = {n}
x2min = -0.5
x2max = 0.5
ix2_bc = periodic
ox2_bc = periodic
nx3 = {n}
x3min = -0.5
x3max = 0.5
ix3_bc = periodic
ox3_bc = periodic
<meshblock>
nx1 = {n}
nx2 = {n}
nx3 = {n}
<time>
evolution = dynamic
integrator = imex3
cfl_number = 0.3
nlim = -1
tlim = 100.0
<ion-neutral>
drag_coeff = 1.0
<hydro>
eos = isothermal
reconstruct = plm
rsolver = hlle
iso_sound_speed = 1.0
<mhd>
eos = isothermal
reconstruct = plm
rsolver = hlle
iso_sound_speed = 1.0
<problem>
pgen_name = turb
d_i = 0.1
d_n = 1.0
beta = 4.0
"""


def run_host(n, cycles):
    import time
    import torch
    from athenak_amd.main import Simulation
    from athenak_amd.parameter_input import ParameterInput
    sim = Simulation(ParameterInput(text=_BOX.format(n=n)), initialize=False)
    pk = sim.pmesh.pmb_pack
    g = torch.Generator(device="cuda").manual_seed(2)
    for ph in (pk.pmhd, pk.phydro):                      # small random velocities, so that nothing is trivially zero
        for c in (1, 2, 3):
            ph.u0[:, c] = ph.u0[:, 0]*torch.empty_like(ph.u0[:, 0]).uniform_(-0.1, 0.1, generator=g)
    sim.pdriver.Initialize(sim.pmesh, sim.pin)
    sim.Execute(2)
    torch.cuda.synchronize()
    t0 = time.time()
    sim.Execute(cycles)
    torch.cuda.synchronize()
    el = time.time() - t0
    print("two-fluid box %d^3, imex3 + plm + hlle, %d cycles: %.2f ms per cycle (host clock, synchronised)" % (
        n, cycles, 1e3*el/cycles))


def parse(path, rounds):
    rows = []
    for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    total = sum(e - s for s, e, _ in rows)
    ionn = [(s, e) for s, e, name in rows if "k_ionn_imp_update" in name]
    t_ionn = sum(e - s for s, e in ionn)
    print("kernels in the trace: %d, total kernel time %.3f ms; k_ionn_imp_update: %d launches, %.3f ms = %.2f%% of it" % (
        len(rows), total/1e6, len(ionn), t_ionn/1e6, 100.0*t_ionn/max(total, 1)))
    if rounds and len(ionn) == 5*(WARM + rounds):
        print("per istage, trace order (warm-up rounds dropped):")
        for istage in range(1, 6):
            ns = sorted(e - s for q, (s, e) in enumerate(ionn) if q % 5 == istage - 1 and q >= 5*WARM)
            print("istage %d  median %8.1f us  min %8.1f  max %8.1f" % (istage, ns[len(ns)//2]/1e3, ns[0]/1e3, ns[-1]/1e3))


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "kernel":
        run_kernel(int(sys.argv[2]) if len(sys.argv) > 2 else 128, int(sys.argv[3]) if len(sys.argv) > 3 else 20)
    elif mode == "host":
        run_host(int(sys.argv[2]) if len(sys.argv) > 2 else 128, int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    elif mode == "parse":
        parse(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 0)
    else:
        sys.exit(__doc__)
