"""Per-cycle time of the driven 256^3 MHD box against the same box undriven (Python host, one GPU).

python tools/turb_profile.py [n] [cycles]: prints one line per run with ms/cycle; run it under
`rocprofv3 --kernel-trace --stats -- python tools/turb_profile.py` for the per-kernel times.
Undriven runs are shown both on the fused stage (the default) and on the task-granular chain that a
driven run takes, so the cost of the forcing itself and the cost of the path are told apart."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from athenak_amd.main import Simulation, load_deck  # noqa: E402
from athenak_amd.parameter_input import ParameterInput  # noqa: E402


def deck(n, driven, fused):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "athenak_amd", "inputs",
                             "turb_mhd.athinput")).read()
    text = text[:text.index("<output1>")]
    if not driven:
        text = text[:text.index("<turb_driving>")]
    pin = ParameterInput(text=text)
    for b in ("mesh", "meshblock"):
        for q in (1, 2, 3):
            pin.blocks[b]["nx%d" % q] = str(n)
    pin.blocks["mhd"]["fused_stage"] = "true" if fused else "false"
    pin.blocks["time"]["tlim"] = "100.0"
    return pin


def run(n, cycles, driven, fused):
    sim = Simulation(deck(n, driven, fused))
    sim.Execute(2)                               # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sim.Execute(cycles)
    torch.cuda.synchronize()
    return 1e3*(time.perf_counter() - t0)/cycles


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    for driven, fused in ((False, True), (False, False), (True, False)):
        print("%d^3 MHD %-9s %-12s %.3f ms/cycle" % (n, "driven" if driven else "undriven",
                                                      "fused" if fused else "task-chain", run(n, cycles, driven, fused)),
              flush=True)
