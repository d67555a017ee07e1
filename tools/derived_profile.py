"""Cost of the derived output variables at n^3 MHD (one GPU): the kernel against a device-to-device copy of the bytes
it has to read and write.

python tools/derived_profile.py [n] [repeats]: an Orszag-Tang box of one MeshBlock, a few cycles, then per variable
(mhd_j2, mhd_curv, mhd_divb, ...) the time of akmi_derived_var by HIP events and the time of a copy of as many bytes
(the arrays the variable reads once + the one it writes).  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/derived_profile.py` for the kernel times the events bracket."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from athenak_amd.main import Simulation, load_deck  # noqa: E402

# doubles per cell the kernel must move: components read (each once) + the one written
READS = {"mhd_wz": 2, "mhd_w2": 3, "mhd_jz": 2, "mhd_j2": 3, "mhd_curv": 3, "mhd_k_jxb": 3, "mhd_curv_perp": 3,
         "mhd_bmag": 3, "mhd_divb": 3}


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3*a.elapsed_time(b)/repeats        # microseconds


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    names = sys.argv[3].split(",") if len(sys.argv) > 3 else ["mhd_j2", "mhd_curv", "mhd_divb"]
    ov = ["mesh/nx%d=%d" % (q, n) for q in (1, 2, 3)] + ["meshblock/nx%d=%d" % (q, n) for q in (1, 2, 3)]
    sim = Simulation(load_deck("orszag_tang.athinput", ov))
    sim.Execute(2)
    cells = sim.phys.w0[0, 0].numel()
    for name in names:
        words = (READS[name] + 1)*cells
        src = torch.empty(words//2, dtype=torch.float64, device="cuda").normal_()
        dst = torch.empty_like(src)
        t_k = timed(lambda: sim.derived(name), repeats)
        t_c = timed(lambda: dst.copy_(src), repeats)
        print("%d^3 %-14s kernel+alloc %8.1f us   copy of %.0f MB (read + write) %8.1f us   ratio %.2f   %.0f GB/s" % (
            n, name, t_k, 8e-6*words, t_c, t_k/t_c, 8e-3*words/t_k), flush=True)
