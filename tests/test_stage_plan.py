"""not gpu: which kernels a stage runs is one function of the pack, the scheme and the environment switches (plan_stage in
csrc/akmi_stage.hip, the unit of the fused stage that holds the plan and the entry points and no kernel).  Its two public answers, akmi_hydro_stage_w_eligible and akmi_mhd_u0_sweeps_eligible, read the pack
and the environment only -- no device call -- so they are compared here against a table written out by hand.  The switches
are read once per process: every set of rows runs in a process of its own, with exactly the switches it names."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="hipcc not available")

DC, PLM, PPM4 = 0, 1, 2
LLF, HLLE, HLLC, HLLD, ROE = 0, 1, 2, 3, 4
SWITCHES = ("AKMI_FUSE_C2P", "AKMI_HYDRO_ONE_KERNEL", "AKMI_HS_LDS", "AKMI_HS_MAXT", "AKMI_HS_TILE")


def answers(rows):
    """[(function, pack keywords, recon, rsolver)] -> the library's answers, in this process"""
    import __graft_entry__ as g
    from athenak_amd import capi
    g.build()
    lib = C.CDLL(g.LIB)
    out = []
    for fn, kw, recon, rs in rows:
        nx = kw.get("nx", (16, 16, 16))
        p = capi.Pack(nmb=1, nvar=kw.get("nvar", 5), nx1=nx[0], nx2=nx[1], nx3=nx[2], ng=kw.get("ng", 2), dx=None,
                      gamma=5.0/3.0, dfloor=1e-20, pfloor=1e-20, tfloor=1e-20, sfloor=1e-20, sigma_max=1e30, iso_cs=1.0,
                      is_ideal=kw.get("ideal", 1))
        out.append(int(getattr(lib, "akmi_" + fn + "_eligible")(C.byref(p), recon, rs)))
    return out


def check(env, table):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_stage_plan as t\n"
            "table = %r\n"
            "got = t.answers([row for row, _ in table])\n"
            "assert got == [want for _, want in table], [(r, w, g) for (r, w), g in zip(table, got) if w != g]\n"
            "print('ok')\n" % (ROOT, os.path.join(ROOT, "tests"), table))
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, "-c", code], env=dict(base, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def hyd_tile_fits(c1, c2, maxlds, maxt=256):
    """does any tile of k_hydro_stage3d2 satisfy the limits (the feasibility part of hyd_tile, written out again)?  tw x th
    positions, one halo entry per thread at most, two planes with halo + two face arrays of five doubles per entry in LDS"""
    for n1 in range(1, c1 + 1):
        tw = (c1 + n1 - 1)//n1 + 1
        if tw > 130:
            continue
        if tw < 8 and n1 > 1:
            break
        for th in range(3, 41):
            if tw*th > maxt:
                break
            if 3*(tw + 3) + 3*th <= tw*th and 8*5*(2*(tw + 3)*(th + 3) + 2*tw*th) <= maxlds:
                return True
    return False


W, U0 = "hydro_stage_w", "mhd_u0_sweeps"
W16, W3, W2 = (W, {}, PLM, HLLC), (W, dict(nx=(3, 16, 16)), PLM, HLLC), (W, dict(nx=(2, 16, 16)), PLM, HLLC)
U16 = (U0, {}, PLM, HLLD)
# ((function, pack, recon, rsolver), expected) with no switch set
TABLE = [
    (W16, 1),                                            # hydro 3-D 16^3 PLM + HLLC, ideal gas, nvar = 5
    ((W, {}, DC, LLF), 1),
    ((W, dict(nvar=6), PLM, HLLC), 0),                   # a passive scalar
    ((W, dict(nvar=4, ideal=0), PLM, HLLE), 0),          # isothermal
    ((W, dict(ng=3), PPM4, HLLC), 0),
    ((W, dict(nx=(16, 16, 1)), PLM, HLLC), 0),           # 2-D
    (W2, 0),                                             # no tile shape at any LDS size
    (W3, 1),                                             # 4 x 21 positions, 20 160 bytes of LDS
    (U16, 1),                                            # MHD 3-D 16^3 PLM + HLLD, ideal gas, nvar = 5
    ((U0, {}, PLM, LLF), 0),
    ((U0, dict(ng=3), PPM4, HLLD), 0),
    ((U0, dict(nvar=6), PLM, HLLD), 0),
    ((U0, dict(nvar=4, ideal=0), PLM, HLLD), 0),
    ((U0, dict(nx=(16, 16, 1)), PLM, HLLD), 0),          # 2-D
]


def test_tile_rows_are_what_fits():
    """the rows whose answer is "a tile fits", from the limits themselves: 53 KB of LDS by default, 20 000 bytes below"""
    assert [hyd_tile_fits(nx1, 16, 53*1024) for nx1 in (16, 3, 2)] == [True, True, False]
    assert [hyd_tile_fits(nx1, 16, 20000) for nx1 in (16, 3, 2)] == [True, False, False]


def test_eligibility_answers_match_the_table():
    check({}, TABLE)


@pytest.mark.parametrize("env,table", [
    ({"AKMI_FUSE_C2P": "0"}, [(W16, 0), (U16, 1)]),
    ({"AKMI_HYDRO_ONE_KERNEL": "0"}, [(W16, 0), (U16, 1)]),
    ({"AKMI_HS_LDS": "20000"}, [(W16, 1), (W3, 0), (W2, 0)]),                # a tile fits / fits no more / never did
], ids=["FUSE_C2P=0", "HYDRO_ONE_KERNEL=0", "HS_LDS=20000"])
def test_switched_eligibility_answers(env, table):
    check(env, table)
