"""python tools/sbox_profile.py [--cycle] [output file]: the timings of profiles/sbox.txt on one GPU.

Device events round 20 launches after 5 of warm-up: the orbital-advection kernel at 128^3 and 256^3 (five variables)
next to akmi_calib_copy over the same bytes on the same arrays, the two launches of the shear-periodic boundary, and one
cycle of the hydro_shwave scheme at 128^3 with and without <shearing_box> on the task-granular chain (host clock round 20
cycles ending in a synchronise, two windows each, alternating).  --cycle: the last part alone.

--mhd: the timings of profiles/sbox_mhd.txt instead: at 128^3 the two launches of the orbital
advection of the face-centred field (akmi_sbox_orbital_emf, akmi_sbox_orbital_ct) for DC, PLM and PPMX, each next to
akmi_calib_copy moving the same bytes, and the two launches of the shear-periodic boundary of the field."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from athenak_amd import capi  # noqa: E402
from test_gpu_sbox import deck_text, make_sim  # noqa: E402

BOX = ((-0.25, -0.25, -0.25), (0.25, 0.25, 0.25))
SHWAVE = "pgen_name = shwave\nipert = 2\nd0 = 1.0\namp = 1.0e-4\nnwx = -8\nnwy = 2\nnwz = 0"
LINWAVE = ("pgen_name = linear_wave\nwave_flag = 0\namp = 1.0e-4\ndens = 1.0\npgas = 0.6\nvx0 = 0.0\nalong_x1 = false\n"
           "along_x2 = false\nalong_x3 = false")


def ev_time(fn, warm=5, rep=20):
    """microseconds per call"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rep):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)/rep*1e3


def cycles(sim, n=20):
    """milliseconds per cycle"""
    sim.Execute(max_cycles=3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sim.Execute(max_cycles=n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0)/n*1e3


def mhd_part(say):
    """orbital advection and the shear-periodic boundary of b0 at 128^3"""
    from test_gpu_sbox_mhd import deck_text as mhd_deck
    n = 128
    for recon, ng in (("ppmx", 3), ("plm", 2), ("dc", 2)):
        sim = make_sim(mhd_deck((n, n, n), (1, 1, 1), ng, BOX[0], BOX[1], recon=recon))
        ph, orb = sim.phys, sim.phys.porb_b
        for t in (ph.b0.x1f, ph.b0.x2f, ph.b0.x3f):
            t.normal_()
        sim.pmesh.dt = dt = 0.3*(0.5/n)
        L, pc, qo = ph.L, ph.pack_c, orb.qshear*orb.omega0
        b = ph.b0
        t_emf = ev_time(lambda: capi.check(L.akmi_sbox_orbital_emf(pc, ph.recon_method, orb.maxjshift, qo, dt, ph.pbval_u.nghbr,
                                                                   orb.xlim, b.x1f, b.x3f, orb.emfx, orb.emfz, capi._stream()),
                                           "sbox_orbital_emf"))
        t_ct = ev_time(lambda: capi.check(L.akmi_sbox_orbital_ct(pc, orb.emfx, orb.emfz, b.x1f, b.x2f, b.x3f, capi._stream()),
                                          "sbox_orbital_ct"))
        # bytes: emf reads two face arrays and writes two EMF arrays (4 doubles per cell); CT reads the two EMF arrays and
        # reads and writes three face arrays (8 doubles per cell)
        src, dst = ph.u0.view(-1), ph.u1.view(-1)
        c_emf, c_ct = 2*n**3, 4*n**3
        t_c1 = ev_time(lambda: capi.check(L.akmi_calib_copy(dst, src, c_emf, capi._stream()), "calib_copy"))
        t_c2 = ev_time(lambda: capi.check(L.akmi_calib_copy(dst, src, c_ct, capi._stream()), "calib_copy"))
        say("orbital_emf %d^3 %-4s ng=%d: %7.1f us = %5.0f GB/s (32 B per cell) | akmi_calib_copy, same bytes: %6.1f us | ratio %.2f"
            % (n, recon, ng, t_emf, 32.0*n**3/t_emf/1e3, t_c1, t_c1/t_emf))
        say("orbital_ct  %d^3 %-4s ng=%d: %7.1f us = %5.0f GB/s (64 B per cell) | akmi_calib_copy, same bytes: %6.1f us | ratio %.2f"
            % (n, recon, ng, t_ct, 64.0*n**3/t_ct/1e3, t_c2, t_c2/t_ct))
        del sim, ph, orb, b, src, dst
        torch.cuda.empty_cache()
    sim = make_sim(mhd_deck((64, 64, 128), (2, 2, 1), 3, BOX[0], BOX[1], recon="ppmx", tlim=100.0))
    ph, sb = sim.phys, sim.phys.psbox_b
    sb.yshear = 0.1234
    t_re = ev_time(lambda: sb.PackAndSendFC(ph.b0, ph.recon_method))
    t_sh = ev_time(lambda: sb.RecvAndUnpackFC(ph.b0))
    nb = sb.buf.numel()
    src, dst = ph.u0.view(-1), ph.u1.view(-1)
    t_c = ev_time(lambda: capi.check(ph.L.akmi_calib_copy(dst, src, nb, capi._stream()), "calib_copy"))
    say("shear boundary of b0 128^3 (2 x 2 x 1 blocks, ng = 3, both faces): remap_x1_fc %.1f us, shift_x1_fc %.1f us | "
        "akmi_calib_copy of the buffer's %d doubles: %.1f us" % (t_re, t_sh, nb, t_c))


def main(argv):
    only_cycle = "--cycle" in argv
    files = [a for a in argv if not a.startswith("--")]
    out = open(files[0], "w") if files else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    assert torch.cuda.is_available(), "needs a GPU"
    say(torch.cuda.get_device_name(0))
    if "--mhd" in argv:
        return mhd_part(say)
    for n in (() if only_cycle else (128, 256)):
        for recon, ng in (("ppmx", 3), ("plm", 2), ("dc", 2)):
            sim = make_sim(deck_text((n, n, n), (1, 1, 1), ng, BOX[0], BOX[1], recon=recon, eos="ideal", rsolver="hllc"))
            ph = sim.phys
            ph.u0.normal_()
            sim.pmesh.dt = dt = 0.3*(0.5/n)            # the time step of a sound speed of one at cfl_number = 0.3
            ncell = 5*n**3
            t_orb = ev_time(lambda: ph.porb_u.RecvAndUnpackCC(ph.u0, ph.u1, ph.recon_method))
            src, dst = ph.u0.view(-1), ph.u1.view(-1)
            t_cpy = ev_time(lambda: capi.check(ph.L.akmi_calib_copy(dst, src, ncell, capi._stream()), "calib_copy"))
            gb = 16.0*ncell/1e9
            say("orbital_cc %d^3 x 5 var %-4s ng=%d: %7.1f us = %5.0f GB/s (16 B per active cell) | akmi_calib_copy, same bytes: "
                "%6.1f us = %5.0f GB/s | ratio %.2f" % (n, recon, ng, t_orb, gb/t_orb*1e6, t_cpy, gb/t_cpy*1e6, t_cpy/t_orb))
            del sim, ph, src, dst
            torch.cuda.empty_cache()
    if not only_cycle:
        sim = make_sim(deck_text((64, 64, 128), (2, 2, 1), 3, BOX[0], BOX[1], recon="ppmx", problem=SHWAVE, tlim=100.0),
                       initialize=True)
        ph, sb = sim.phys, sim.phys.psbox_u
        sb.yshear = 0.1234
        t_re = ev_time(lambda: sb.PackAndSendCC(ph.u0, ph.recon_method))
        t_sh = ev_time(lambda: sb.RecvAndUnpackCC(ph.u0))
        say("shear boundary 128^3 (2 x 2 x 1 blocks, ng = 3, 4 var, both faces): remap_x1 %.1f us, shift_x1 %.1f us" % (t_re, t_sh))
        del sim, ph, sb
    a = make_sim(deck_text((64, 64, 128), (2, 2, 1), 3, BOX[0], BOX[1], recon="ppmx", problem=SHWAVE, tlim=100.0), initialize=True)
    b = make_sim(deck_text((64, 64, 128), (2, 2, 1), 3, BOX[0], BOX[1], recon="ppmx", problem=LINWAVE, tlim=100.0,
                           x1_bc="periodic", sbox=False, extra="<hydro>\nfused_stage = false\n"), initialize=True)
    ta, tb = cycles(a), cycles(b)
    ta2, tb2 = cycles(a), cycles(b)
    say("cycle 128^3 (2 x 2 x 1 blocks, isothermal, ppmx + hlle, rk2, task-granular chain): with <shearing_box> %.3f / %.3f ms, "
        "without %.3f / %.3f ms" % (ta, ta2, tb, tb2))


if __name__ == "__main__":
    main(sys.argv[1:])
