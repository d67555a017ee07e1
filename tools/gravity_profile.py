"""Cost of self-gravity: the multigrid Solve (akmi_mg_solve), its launch count, a gravity cycle against the same deck
without gravity, and the finest-level smoother against akmi_calib_copy on the same arrays (one GPU).

python tools/gravity_profile.py solve [n] [nb] [rounds]    one Solve (FMG + 4 V-cycles, 2+2 sweeps) of an n^3 Jeans-wave box
                                                           with nb^3 MeshBlocks: host clock, synchronised, `rounds` times
                                                           after 3 warm-up Solves; launches per Solve
python tools/gravity_profile.py cycle [n] [nb] [cycles]    ms per cycle of that box with <gravity> + self_gravity, and with
                                                           both removed (task-granular path both times)
python tools/gravity_profile.py smooth [n] [nb] [rounds]   one colour of the smoother on the finest level against
                                                           akmi_calib_copy of the same number of doubles (HIP events)
python tools/gravity_profile.py isolated [n] [nb] [rounds] the same Solve on inputs/binary_gravity.athinput (outflow faces) with
                                                           mg_bc = zerofixed and multipole, next to the periodic one
python tools/gravity_profile.py all                        the table of profiles/gravity_mg.txt

Counted traffic of one colour of the smoother: u read, src read, u written, whole cache lines: 24 bytes per cell of
the level arrays (ghosts included); of the copy: 16 bytes per double."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM = 3


def _sim(n, nb, gravity=True, init=True):
    from athenak_amd.main import Simulation, load_deck
    over = ["mesh/nx1=%d" % n, "mesh/nx2=%d" % n, "mesh/nx3=%d" % n, "mesh/x2max=1.0", "mesh/x3max=1.0",
            "meshblock/nx1=%d" % nb, "meshblock/nx2=%d" % nb, "meshblock/nx3=%d" % nb, "time/tlim=100.0",
            "gravity/niteration=4"]
    pin = load_deck("jeans_wave.athinput", over)
    for blk in [b for b in pin.blocks if b.startswith("output")]:
        del pin.blocks[blk]
    pin.blocks["hydro"]["fused_stage"] = "false"
    if not gravity:
        del pin.blocks["gravity"], pin.blocks["hydro_srcterms"]
        pin.blocks["problem"]["pgen_name"] = "turb"           # a uniform box: the cycle's cost does not depend on the data
    return Simulation(pin, initialize=init)


def _sim_isolated(n, nb, mg_bc):
    """the two-sphere deck at n^3 with the solver settings of _sim: FMG + 4 V-cycles, 2+2 sweeps"""
    from athenak_amd.main import Simulation, load_deck
    over = ["mesh/nx%d=%d" % (q, n) for q in (1, 2, 3)] + ["meshblock/nx%d=%d" % (q, nb) for q in (1, 2, 3)] + [
        "gravity/mg_bc=%s" % mg_bc, "gravity/threshold=-1.0", "gravity/npresmooth=2", "gravity/npostsmooth=2"]
    pin = load_deck("binary_gravity.athinput", over)
    for blk in [b for b in pin.blocks if b.startswith("output")]:
        del pin.blocks[blk]
    pin.blocks["gravity"]["niteration"] = "4"
    return Simulation(pin)


def _median(v):
    v = sorted(v)
    return v[len(v)//2], v[0], v[-1]


def run_solve(n, nb, rounds, mg_bc=None):
    import torch
    from athenak_amd import capi
    sim = _sim(n, nb) if mg_bc is None else _sim_isolated(n, nb, mg_bc)
    d = sim.pmesh.pmb_pack.pgrav.pmgd
    L = capi.lib()
    ms = []
    for r in range(WARM + rounds):
        torch.cuda.synchronize()
        L.akmi_mg_launch_count(1)
        t0 = time.perf_counter()
        d.Solve()
        torch.cuda.synchronize()
        if r >= WARM:
            ms.append(1e3*(time.perf_counter() - t0))
    launches = int(L.akmi_mg_launch_count(0))
    med, lo, hi = _median(ms)
    print("Solve %4d^3, blocks %2d^3 (%4d), levels %d+%d-1, FMG + 4 V-cycles, 2+2 sweeps" % (n, nb, d.nmb, d.nrootlevel_, d.nmblevel_)
          + (", %-9s" % mg_bc if mg_bc else "") + ": median %8.3f ms  min %8.3f  "
          "max %8.3f  (%d rounds)  %5d launches  %6.2f us per launch" % (
              med, lo, hi, rounds, launches, 1e3*med/launches), flush=True)


def run_cycle(n, nb, cycles):
    import torch
    for grav in (True, False):
        sim = _sim(n, nb, grav)
        sim.Execute(2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sim.Execute(cycles)
        torch.cuda.synchronize()
        print("cycle %4d^3, blocks %2d^3, isothermal hydro plm + hlle, rk2, %s: %8.2f ms per cycle (%d cycles, host clock)"
              % (n, nb, "with <gravity> + self_gravity" if grav else "without gravity            ",
                 1e3*(time.perf_counter() - t0)/cycles, cycles), flush=True)
        del sim


def run_smooth(n, nb, rounds):
    import torch
    from athenak_amd import capi
    L = capi.lib()
    nmb = (n//nb)**3
    cells = nmb*(nb + 2)**3
    g = torch.Generator(device="cuda").manual_seed(3)
    u = torch.empty(cells, dtype=torch.float64, device="cuda").normal_(generator=g)
    src = torch.empty(cells, dtype=torch.float64, device="cuda").normal_(generator=g)
    ev = {"smooth": [], "copy": []}
    for r in range(WARM + rounds):
        for what in ("smooth", "copy"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if what == "smooth":
                capi.check(L.akmi_mg_smooth(nmb, nb, nb, nb, 1.0/n, 1.15, r & 1, 0, u, src, capi._stream()),
                           "mg_smooth")
            else:
                capi.check(L.akmi_calib_copy(src, u, cells, capi._stream()), "calib_copy")
            b.record()
            if r >= WARM:
                ev[what].append((a, b))
    torch.cuda.synchronize()
    for what, by in (("smooth", 24*cells), ("copy", 16*cells)):
        med, lo, hi = _median([1e3*a.elapsed_time(b) for a, b in ev[what]])
        print("%-6s %4d^3, blocks %2d^3: median %8.1f us  min %8.1f  max %8.1f   counted %7.1f MB  %6.0f GB/s" % (
            what, n, nb, med, lo, hi, by/1e6, by/med/1e3), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    a = [int(x) for x in sys.argv[2:]]
    if mode == "solve":
        run_solve(*(a + [128, 32, 10][len(a):]))
    elif mode == "cycle":
        run_cycle(*(a + [128, 32, 5][len(a):]))
    elif mode == "smooth":
        run_smooth(*(a + [128, 32, 20][len(a):]))
    elif mode == "isolated":
        n, nb, rounds = a + [128, 32, 10][len(a):]
        for bc in (None, "zerofixed", "multipole"):
            run_solve(n, nb, rounds, bc)
    elif mode == "all":
        for n, nb in ((128, 64), (128, 32), (256, 64), (256, 32)):
            run_solve(n, nb, 10)
        run_smooth(256, 32, 20)
        run_smooth(128, 64, 20)
        run_cycle(128, 32, 5)
    else:
        sys.exit(__doc__)
