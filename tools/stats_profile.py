"""Cost of the run-time statistics at n^3 MHD (one GPU): akmi_turb_history and akmi_pdf against a device-to-device copy
of the bytes each kernel has to read.

python tools/stats_profile.py [n] [repeats] [output file]: an Orszag-Tang box of one MeshBlock, a few cycles, then the
entries themselves (preallocated outputs, no read-back) timed by HIP events: the history sums and five histograms -- 1-D
100 bins (LDS path), the same with the global-atomic path forced, 2-D 100 x 100 (over the LDS limit: global path), and a
constant field (every cell in one bin) through both paths -- each next to a copy of as many bytes as the kernel reads.
The lines are printed and written to the output file (default profiles/stats_outputs.txt).  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/stats_profile.py` for the kernel rows the events bracket (the event
times of akmi_pdf include its three memsets, those of akmi_turb_history its second kernel)."""
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


def row(n, what, t_k, words, repeats):
    # the copy reads `words` doubles once (and writes as many)
    src = torch.empty(words, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    t_c = timed(lambda: dst.copy_(src), repeats)
    say("%d^3 %-36s %9.1f us   copy reading %6.0f MB %8.1f us   ratio %.2f" % (n, what, t_k, 8e-6*words, t_c, t_k/t_c))
    return t_k


def pdf_call(ph, axes, mass, force_global):
    """a closure that launches akmi_pdf on preallocated outputs"""
    L = capi.lib()
    cax = [capi.PdfAxis(t.data_ptr(), t.shape[1], comp, len(e) - 1, int(log), float(e[0]), float(e[-1]), float(step))
           for (t, comp, e, step, log) in axes]
    shape = ((cax[1].nbin + 2) if len(cax) == 2 else 1, cax[0].nbin + 2)
    counts = torch.zeros(shape, dtype=torch.int64, device="cuda")
    weights = torch.zeros(shape, dtype=torch.float64, device="cuda")
    nan = torch.zeros(1, dtype=torch.int64, device="cuda")
    y = cax[1] if len(cax) == 2 else None

    def call():
        capi.check(L.akmi_pdf(ph.pack_c, cax[0], y, ph.u0 if mass else None, counts, weights, nan, int(force_global),
                              capi._stream()), "pdf")
    call.keep = (cax, counts, weights, nan)
    return call


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "stats_outputs.txt")
    ov = ["mesh/nx%d=%d" % (q, n) for q in (1, 2, 3)] + ["meshblock/nx%d=%d" % (q, n) for q in (1, 2, 3)]
    sim = Simulation(load_deck("orszag_tang.athinput", ov))
    sim.Execute(2)
    ph = sim.phys
    cells = ph.w0[0, 0].numel()
    L = capi.lib()
    say("# tools/stats_profile.py %d %d: entries timed by HIP events, each against a device-to-device copy" % (n, repeats))
    partial = torch.zeros((1, capi.TURB_NHIST), dtype=torch.float64, device="cuda")
    work = torch.empty(int(L.akmi_turb_history_workspace_bytes(ph.pack_c))//8 + 1, dtype=torch.float64, device="cuda")

    def hist():
        capi.check(L.akmi_turb_history(ph.pack_c, ph.w0, ph.bcc0, ph.b0.x1f, ph.b0.x2f, ph.b0.x3f, partial, work,
                                       capi._stream()), "turb_history")
    # history: bcc0 (3), velocities (3), three face arrays
    row(n, "akmi_turb_history", timed(hist, repeats), 9*cells, repeats)
    e1, s1 = outputs.pdf_bins(0.01, 100.0, 100, True)
    e2, s2 = outputs.pdf_bins(-2.0, 2.0, 100, False)
    rho = (ph.w0, 0, e1, s1, True)
    bx = (ph.bcc0, 0, e2, s2, False)
    row(n, "akmi_pdf 1-D 100 bins (LDS)", timed(pdf_call(ph, [rho], False, False), repeats), cells, repeats)
    row(n, "akmi_pdf 1-D 100 bins, global forced", timed(pdf_call(ph, [rho], False, True), repeats), cells, repeats)
    row(n, "akmi_pdf 1-D mass-weighted (LDS)", timed(pdf_call(ph, [rho], True, False), repeats), 2*cells, repeats)
    row(n, "akmi_pdf 2-D 100 x 100 (global)", timed(pdf_call(ph, [rho, bx], False, False), repeats), 2*cells, repeats)
    ph.w0[:, 0] = 1.0                             # a constant field: every cell hits one bin
    t_l = row(n, "akmi_pdf constant field (LDS)", timed(pdf_call(ph, [rho], False, False), repeats), cells, repeats)
    t_g = row(n, "akmi_pdf constant field, global forced", timed(pdf_call(ph, [rho], False, True), repeats), cells, repeats)
    say("constant field: forced global / privatised = %.2f" % (t_g/t_l))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
