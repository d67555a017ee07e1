"""python -m athenak_amd (-i <deck> | -r <restart file>) [-d <run_dir>] [--host python|native] [block/name=value ...]

Command-line entry with the argument conventions of the reference's executable
(src/main.cpp:61-420: -i input file, -d run directory, trailing block/name=value overrides), so
that scripts written around `athena -i ...` (e.g. the reference's regression-test driver) can run
this implementation: reads the deck, builds Mesh/physics/ProblemGenerator/Outputs/Driver, runs
Initialize -> Execute -> Finalize and writes tab/hst/bin/-errs.dat files in the run directory.

--host native runs the C++ host driver (native.NativeSimulation: one process, from a deck) and writes the same files:
the output blocks work over its mesh, which aliases the native device arrays.
"""
import os
import sys
import time


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    deck, rundir, overrides, rstfile, host = None, None, [], None, "python"
    i = 0
    while i < len(argv):
        a = argv[i]
        if a == "-i":
            deck = argv[i + 1]; i += 2
        elif a == "-r":
            rstfile = argv[i + 1]; i += 2
        elif a == "-d":
            rundir = argv[i + 1]; i += 2
        elif a == "--host":
            host = argv[i + 1]; i += 2
        elif a in ("-h", "--help"):
            print(__doc__)
            return 0
        elif a.startswith("-"):
            sys.stderr.write("### FATAL ERROR unknown option %s (supported: -i -r -d --host -h)\n" % a)
            return 1
        else:
            overrides.append(a); i += 1
    if deck is None and rstfile is None:
        sys.stderr.write("### FATAL ERROR Either an input or restart file must be specified: "
                         "-i <deck> or -r <file>\n")
        return 1
    if host not in ("python", "native"):
        sys.stderr.write("### FATAL ERROR --host %s: python or native\n" % host)
        return 1
    if host == "native" and (rstfile is not None or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        sys.stderr.write("### FATAL ERROR --host native runs one process from a deck (-i): restarts and several "
                         "ranks take the Python host from the command line\n")
        return 1
    from .main import Simulation, load_deck, load_restart
    from .outputs import Outputs
    if deck is not None:
        deck = os.path.abspath(deck) if os.path.exists(deck) else deck
    if rstfile is not None:
        rstfile = os.path.abspath(rstfile)
    if rundir:
        os.makedirs(rundir, exist_ok=True)
        os.chdir(rundir)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if host == "native":
        return _run_native(deck, overrides)
    if world > 1:
        import torch
        import torch.distributed as dist
        if torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group(os.environ.get("AKMI_DIST_BACKEND", "nccl"))
    if rstfile is not None:
        sim = load_restart(rstfile, overrides, my_rank=rank, nranks=world, initialize=False)
        pin = sim.pin
    else:
        pin = load_deck(deck, overrides)
        sim = Simulation(pin, my_rank=rank, nranks=world, initialize=False)
    pm, drv = sim.pmesh, sim.pdriver
    pout = Outputs(pin, pm)
    drv.Initialize(pm, pin, pout, res_flag=rstfile is not None)
    t0 = time.time()
    drv.Execute(pm, pin)
    import torch
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    el = time.time() - t0
    drv.Finalize(pm, pin, pout)
    if rank == 0:
        _summary(pm, drv.tlim, drv.nlim, el, drv.nmb_updated_*pm.NumberOfMeshBlockCells())
    if world > 1:
        dist.destroy_process_group()
    return 0


def _summary(pm, tlim, nlim, el, zone_cycles):
    print("\ncycle=%d time=%.14e dt=%.14e" % (pm.ncycle, pm.time, pm.dt))
    print("Terminating on %s" % ("time limit" if pm.time >= tlim else "cycle limit"))
    print("time=%e cycle=%d\ntlim=%e nlim=%d" % (pm.time, pm.ncycle, tlim, nlim))
    print("cpu time used  = %e\nzone-cycles/cpu_second = %e" % (el, zone_cycles/max(el, 1e-30)))


def _run_native(deck, overrides):
    """the run of main() on the C++ host: akmi_sim_execute one cycle at a time, the outputs tested after each as
    Driver._cycle does.

    The C++ host reads its own copy of the deck and adds the defaults it takes to that copy, so the Python-side record
    would lack them and the parameter dump that heads bin, cbin and rst files would differ from the Python host's.  The
    record is therefore taken from the Python host, built once without initialising it and released before the C++ host
    allocates: one extra allocation of the state and one extra evaluation of the initial conditions at start-up."""
    import gc
    import torch
    from .driver import Driver
    from .main import Simulation, load_deck
    from .native import NativeSimulation
    from .outputs import Outputs
    record = load_deck(deck, overrides)
    for blk, d in record.blocks.items():
        # the other writers read objects of the Python host (its pack descriptor, its boundary values) that the mesh of
        # the C++ host does not carry; cbin goes through akmi_sim_coarsen
        if blk.startswith("output") and d.get("file_type") != "cbin":
            sys.stderr.write("### FATAL ERROR --host native writes cbin outputs only: output block '%s' has file_type = %s\n"
                             % (blk, d.get("file_type")))
            return 1
    py = Simulation(record, initialize=False)
    del py
    gc.collect()
    torch.cuda.empty_cache()
    pin = load_deck(deck, overrides)
    sim = NativeSimulation(pin, initialize=False)
    for blk, d in pin.blocks.items():                   # what both hosts read or set must agree
        for k, v in d.items():
            if record.blocks.get(blk, {}).get(k) != v:
                sys.stderr.write("### FATAL ERROR <%s>/%s = %s on the C++ host, %s on the Python host\n"
                                 % (blk, k, v, record.blocks.get(blk, {}).get(k)))
                return 1
    pin.blocks = record.blocks
    pm = sim.pmesh
    drv = Driver(pin, pm)                               # the limits of the loop and Finalize; the C++ host integrates
    pout = Outputs(pin, pm)
    sim.Initialize()
    pm.time, pm.dt, pm.ncycle = sim.time, sim.dt, sim.ncycle
    tlim = sim.tlim
    pout.MakeOutputs(pm, pin)
    t0 = time.time()
    n = 0
    while pm.time < tlim and (pm.ncycle < drv.nlim or drv.nlim < 0):
        dt_used = pm.dt
        if sim.Execute(max_cycles=1) != 1:
            break
        n += 1
        dt_next, pm.dt = pm.dt, dt_used                 # the outputs see the step just taken (Driver._cycle)
        pout.TestAndMakeOutputs(pm, pin, tlim)
        pm.dt = dt_next
    torch.cuda.synchronize()
    el = time.time() - t0
    drv.Finalize(pm, pin, pout)
    _summary(pm, tlim, drv.nlim, el, n*pm.nmb_total*pm.NumberOfMeshBlockCells())
    sim.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
