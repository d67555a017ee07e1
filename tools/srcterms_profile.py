"""Cost of the source-term pass: rt3d at n^3 in one MeshBlock on the C++ host, hydro and MHD, with and without the
<*_srcterms> block (the run without it is at rest in hydrostatic imbalance -- only its kernel times matter).

python tools/srcterms_profile.py [n] [cycles] [hydro|mhd] [src|nosrc]: prints ms/cycle per run (all four without the
last two arguments); under `rocprofv3 --kernel-trace --stats -- python tools/srcterms_profile.py 256 5 hydro src` the
per-kernel times of one configuration
(k_srcterms against the stage kernels; hydro without the block runs the stage kernel with ConsToPrim inside)."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from athenak_amd import native  # noqa: E402
from athenak_amd.parameter_input import ParameterInput  # noqa: E402


def deck(n, mhd, src):
    text = open(os.path.join(ROOT, "athenak_amd", "inputs", "rt3d.athinput")).read()
    text = text[:text.index("<output1>")]
    if mhd:
        text = text.replace("<hydro_srcterms>", "<mhd_srcterms>").replace("<hydro>", "<mhd>").replace("hllc", "hlld")
    pin = ParameterInput(text=text)
    blk = "mhd" if mhd else "hydro"
    for b in ("mesh", "meshblock"):
        for q in (1, 2, 3):
            pin.blocks[b]["nx%d" % q] = str(n)
    pin.blocks["mesh"]["x3min"], pin.blocks["mesh"]["x3max"] = "-0.2", "0.2"
    pin.blocks["time"]["tlim"] = "100.0"
    pin.blocks["time"]["run_ahead"] = "false"
    if mhd:
        pin.blocks["problem"]["b0"] = "0.05"
    if not src:      # the generator still needs g: the block stays, the term is switched off
        pin.blocks[blk + "_srcterms"]["const_accel"] = "false"
    return pin


def run(n, cycles, mhd, src):
    sim = native.NativeSimulation(deck(n, mhd, src))
    sim.Execute(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sim.Execute(cycles)
    torch.cuda.synchronize()
    ms = 1e3*(time.perf_counter() - t0)/cycles
    sim.close()
    return ms


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    fluids = [sys.argv[3] == "mhd"] if len(sys.argv) > 3 else [False, True]
    srcs = [sys.argv[4] == "src"] if len(sys.argv) > 4 else [False, True]
    for mhd in fluids:
        for src in srcs:
            print("%d^3 %-5s const_accel %-5s %.3f ms/cycle" % (n, "MHD" if mhd else "hydro", src, run(n, cycles, mhd, src)),
                  flush=True)
