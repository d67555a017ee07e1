"""Cost of the coarsened binary output at n^3 MHD (one GPU): akmi_coarsen against a device-to-device copy of the bytes
the kernel has to read.

python tools/cbin_profile.py [n] [repeats] [output file]: an Orszag-Tang box of one MeshBlock, a few cycles, then the entry
itself for mhd_w_bcc (eight variables, preallocated output, no read-back) timed by HIP events at coarsen_factor = 2, 4, 8,
with and without moments, in both forms (staged through LDS / direct), each next to a copy of as many bytes as the kernel
reads.  The lines are printed and written to the output file (default profiles/cbin_outputs.txt).  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/cbin_profile.py` (no counters) for the kernel rows the events bracket:
the tool does not start the profiler, so those rows land in the profiler's own output and are copied into the output
file by hand."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from athenak_amd import capi, outputs  # noqa: E402
from athenak_amd.main import Simulation, load_deck  # noqa: E402
from tools.derived_profile import timed  # noqa: E402

LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def coarsen_call(pack, outvars, f, moments, staged, n):
    """a closure that launches akmi_coarsen over the active cells on a preallocated output"""
    ph = pack.pmhd
    L = capi.lib()
    ind = pack.pmesh.mb_indcs
    tab = (capi.CoarsenVar*len(outvars))(*[capi.CoarsenVar(getattr(ph, arr).data_ptr(), getattr(ph, arr).shape[1], comp)
                                          for (_, comp, arr) in outvars])
    nc = n//f
    out = torch.empty((len(outvars)*(4 if moments else 1), 1, nc, nc, nc), dtype=torch.float64, device="cuda")
    lo, cnc = (C.c_int*3)(ind.is_, ind.js, ind.ks), (C.c_int*3)(nc, nc, nc)

    def call():
        capi.check(L.akmi_coarsen(ph.pack_c, tab, len(outvars), f, int(moments), lo, cnc, out, int(staged),
                                  capi._stream()), "coarsen")
    call.keep = (tab, out, lo, cnc)
    return call


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "cbin_outputs.txt")
    ov = ["mesh/nx%d=%d" % (q, n) for q in (1, 2, 3)] + ["meshblock/nx%d=%d" % (q, n) for q in (1, 2, 3)]
    sim = Simulation(load_deck("orszag_tang.athinput", ov))
    sim.Execute(2)
    pack = sim.pmesh.pmb_pack
    outvars = outputs._outvars("mhd_w_bcc", True)
    words = len(outvars)*n**3                        # the active cells of eight variables, each read once
    src = torch.empty(words, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    t_c = timed(lambda: dst.copy_(src), repeats)
    say("# tools/cbin_profile.py %d %d: akmi_coarsen of mhd_w_bcc timed by HIP events; a device-to-device copy reading the "
        "same %.0f MB takes %.1f us" % (n, repeats, 8e-6*words, t_c))
    for f in (2, 4, 8):
        for moments in (False, True):
            t = [timed(coarsen_call(pack, outvars, f, moments, staged, n), repeats) for staged in (0, 1)]
            say("%d^3 f=%d moments=%-5s  direct %9.1f us (%.2f x copy)   staged %9.1f us (%.2f x copy)   direct/staged %.2f"
                % (n, f, moments, t[0], t[0]/t_c, t[1], t[1]/t_c, t[0]/t[1]))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fp:
        fp.write("\n".join(LINES) + "\n")
