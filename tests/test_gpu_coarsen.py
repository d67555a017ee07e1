"""gpu: the coarsened binary output (akmi_coarsen, csrc/akmi_coarsen.hip) on the device.

  * Simulation.coarsen on evolved states equals the numpy restatement (tests/coarsen_restate.py) bit for bit, in both forms
    of the kernel (staged through LDS / direct), with and without moments: uniform and refined meshes, 1-D to 3-D, ghost
    zones, stored, derived and forcing variables, factors 1, 2, 3, 4, 8, 16;
  * the entry on synthetic arrays of magnitude 1e-150 ... 1e150 with a NaN and a -0.0: NaN positions equal, every other
    value equal as bits; tiles along i, partial tiles, a variable table too long to pass by value;
  * independent checks: a constant field, the sum of the coarse cells against math.fsum of the fine ones, <x^2> >= <x>^2;
  * the C++ host through coarsen() and through `python -m athenak_amd --host native` (whole files against the Python
    host's), 2 and 4 ranks through the command line, and the deck inputs/turb_mhd_cbin.athinput.

Every test prints the figures it asserts on before it asserts."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import coarsen_cases as cc  # noqa: E402
import coarsen_restate as R  # noqa: E402
import derived_cases as dc  # noqa: E402
import parity_util as pu  # noqa: E402
from athenak_amd import capi  # noqa: E402
from athenak_amd.main import Simulation, load_deck  # noqa: E402

pytestmark = pytest.mark.gpu

_SIMS = {}


def _mesh(n, mb):
    ov = []
    for q in range(3):
        ov += ["mesh/nx%d=%d" % (q + 1, n[q]), "meshblock/nx%d=%d" % (q + 1, mb[q])]
    return ov


def _sim(key):
    """the evolved state of a case, computed once and left unchanged"""
    if key not in _SIMS:
        if key == "ot48":
            deck, ov, cycles = "orszag_tang.athinput", _mesh((48, 24, 12), (24, 12, 6)) + ["mesh/nghost=2"], 10
        elif key == "ot16":
            deck, ov, cycles = "orszag_tang.athinput", _mesh((16, 16, 16), (16, 16, 16)) + ["mesh/nghost=4"], 5
        elif key == "turb":
            deck, ov, cycles = "turb_mhd.athinput", _mesh((16, 16, 16), (8, 8, 8)), 5
        elif key == "hydro":
            (deck, ov), cycles = pu.deck_overrides("linear_wave_hydro", 16, 3, 8), 3
        elif key == "smr":
            (deck, ov), cycles = pu.deck_overrides("blast_smr", 32, 3, 8), 2
        elif key == "ot2d":
            deck, ov, cycles = "orszag_tang.athinput", _mesh((32, 16, 1), (16, 16, 1)), 5
        elif key == "rj1d":
            deck, ov, cycles = "rj2a.athinput", _mesh((96, 1, 1), (24, 1, 1)), 5
        sim = Simulation(load_deck(deck, list(ov) + ["time/nlim=-1"]))
        assert sim.Execute(max_cycles=cycles) == cycles
        _SIMS[key] = sim
    return _SIMS[key]


# (state, variable, factor, ghost_zones)
CASES = [
    ("ot48", "mhd_w_bcc", 2, False), ("ot48", "mhd_w_bcc", 3, False),
    ("ot48", "mhd_w_bcc", 2, True),                      # fine extents 28 x 16 x 10
    ("ot16", "mhd_u_bcc", 4, True), ("ot16", "mhd_u_bcc", 8, True),        # fine extents 24^3
    ("ot16", "mhd_w_bcc", 16, False),                    # one coarse cell, a 4096-term serial sum
    ("turb", "turb_force", 2, False), ("turb", "mhd_j2", 2, False), ("turb", "mhd_j2", 4, True),
    ("hydro", "hydro_w", 2, False), ("hydro", "hydro_w", 4, False),
    ("smr", "mhd_w_bcc", 2, False), ("smr", "mhd_divb", 4, False),
    ("ot2d", "mhd_w_bcc", 1, False), ("ot2d", "mhd_jz", 1, True),
    ("rj1d", "mhd_u_bcc", 1, False),
]


@pytest.mark.parametrize("state,variable,f,gz", CASES, ids=lambda v: str(v))
def test_coarsen_is_the_restatement_bit_for_bit_in_both_forms(state, variable, f, gz):
    sim = _sim(state)
    if state == "smr":
        assert sim.pmesh.multilevel
    for moments in (False, True):
        labels, want = cc.restated(sim, variable, f, moments, gz)
        for staged in (False, True):
            got_labels, t = sim.coarsen(variable, f, moments=moments, ghost_zones=gz, staged=staged)
            assert got_labels == labels and tuple(t.shape) == want.shape and t.dtype == torch.float64
            dc.assert_bits(t.cpu().numpy(), want, "%s %s f=%d gz=%s moments=%s staged=%s" % (state, variable, f, gz, moments, staged))
        print("%s %s f=%d gz=%s moments=%s: %s, both forms equal the restatement" % (state, variable, f, gz, moments, want.shape))
    # the default form (staged=None) is one of the two
    _, t = sim.coarsen(variable, f, moments=True, ghost_zones=gz)
    dc.assert_bits(t.cpu().numpy(), want, "default form")


# ---- the entry on synthetic arrays ---------------------------------------------------------------------------------
def _entry(arrays, nx, ng, f, moments, lo, nc, staged):
    """akmi_coarsen on device copies of [(host array (nmb, nvar, N3, N2, N1), comp)]"""
    nmb = arrays[0][0].shape[0]
    dxd = torch.ones((nmb, 3), dtype=torch.float64, device="cuda")
    pk = dc.pack_struct(nmb, 5, nx, ng, np.ones((nmb, 3)))
    pk.dx = dxd.data_ptr()
    dev = {}
    for a, _ in arrays:
        if id(a) not in dev:
            dev[id(a)] = torch.from_numpy(a).cuda()
    tab = (capi.CoarsenVar*len(arrays))(*[capi.CoarsenVar(dev[id(a)].data_ptr(), a.shape[1], comp) for a, comp in arrays])
    out = torch.full((len(arrays)*(4 if moments else 1), nmb, nc[2], nc[1], nc[0]), 7.0, dtype=torch.float64, device="cuda")
    capi.check(capi.lib().akmi_coarsen(C.byref(pk), tab, len(arrays), f, int(moments), (C.c_int*3)(*lo), (C.c_int*3)(*nc),
                                       capi._p(out), int(staged), capi._stream()), "coarsen")
    return out.cpu().numpy()


# (nx, ng, nmb, lo, factors): small odd boxes; rows wider than a workgroup (two tiles along i, the second partial: 320 and
# 80 coarse cells), several coarse rows per workgroup, a row segment of 20 x 32 doubles
SYN = [((23, 13, 9), 2, 3, (1, 0, 1), (1, 2, 3, 4)), ((640, 32, 32), 0, 2, (0, 0, 0), (2, 8, 32)),
       ((300, 3, 2), 1, 2, (2, 1, 0), (1,))]


@pytest.mark.parametrize("nx,ng,nmb,lo,factors", SYN, ids=["odd", "wide", "row"])
def test_entry_on_wide_range_arrays_nan_and_negative_zero(nx, ng, nmb, lo, factors):
    N = (nx[0] + 2*ng, nx[1] + 2*ng, nx[2] + 2*ng)
    a, at_nan, at_zero = cc.wide_field((nmb, 3, N[2], N[1], N[0]), seed=sum(nx))
    b, _, _ = cc.wide_field((nmb, 1, N[2], N[1], N[0]), seed=sum(nx) + 1)
    arrays = [(a, 0), (a, 1), (a, 2), (b, 0)]
    for f in factors:
        nc = tuple((n - l)//f for n, l in zip(N, lo))
        for moments in (False, True):
            want = R.restate_vars([x[:, c] for x, c in arrays], f, lo, nc, moments)
            for staged in (0, 1):
                got = _entry(arrays, nx, ng, f, moments, lo, nc, staged)
                cc.assert_same_bits(got, want, "%s f=%d moments=%s staged=%d" % (nx, f, moments, staged))
            print("%s f=%d moments=%s: %d values, %d NaN, %d inf: equal in both forms" % (
                nx, f, moments, want.size, int(np.isnan(want).sum()), int(np.isinf(want).sum())))


def test_variable_table_in_device_memory():
    """26 variables do not fit the by-value table of 24: the same bits through the table in device memory"""
    nx, ng, nmb = (23, 13, 9), 2, 2
    a, _, _ = cc.wide_field((nmb, 26, 13, 17, 27), seed=3)
    arrays = [(a, c) for c in range(26)]
    want = R.restate_vars([a[:, c] for c in range(26)], 2, (1, 0, 1), (13, 8, 6), True)
    for staged in (0, 1):
        cc.assert_same_bits(_entry(arrays, nx, ng, 2, True, (1, 0, 1), (13, 8, 6), staged), want, "26 variables")


def test_entry_refuses_ranges_outside_the_array():
    L = capi.lib()
    buf = torch.zeros(12**3, dtype=torch.float64, device="cuda")
    pk = dc.pack_struct(1, 5, (8, 8, 8), 2, np.ones((1, 3)))
    tab = (capi.CoarsenVar*1)(capi.CoarsenVar(buf.data_ptr(), 1, 0))

    def call(f, lo, nc, t=tab):
        return L.akmi_coarsen(C.byref(pk), t, 1, f, 0, (C.c_int*3)(*lo), (C.c_int*3)(*nc), capi._p(buf), 0, None)
    assert call(2, (2, 2, 2), (6, 4, 4)) < 0 and b"leave the array extent 12" in L.akmi_last_error()
    assert call(2, (-1, 2, 2), (4, 4, 4)) < 0
    assert call(0, (2, 2, 2), (4, 4, 4)) < 0 and b"coarsen_factor = 0" in L.akmi_last_error()
    assert call(2, (2, 2, 2), (4, 4, 4), (capi.CoarsenVar*1)(capi.CoarsenVar(buf.data_ptr(), 1, 1))) < 0
    assert L.akmi_coarsen_default_staged() in (0, 1)


# ---- independent checks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [2, 4])
def test_constant_field_gives_its_powers_exactly(f):
    """f^3 = 8 or 64 equal terms: every partial sum n*c^p and the division by f^3 are exact while n*c^p has few bits"""
    c = 1.375
    a = np.full((2, 1, 16, 16, 16), c)
    c2 = c*c
    c3 = c2*c
    c4 = c3*c
    for staged in (0, 1):
        got = _entry([(a, 0)], (16, 16, 16), 0, f, True, (0, 0, 0), (16//f,)*3, staged)
        for q, want in enumerate((c, c2, c3, c4)):
            assert np.all(got[q] == want), (f, staged, q, got[q].ravel()[0], want)
    print("constant %r, f=%d: %r %r %r %r exactly" % (c, f, c, c2, c3, c4))


@pytest.mark.parametrize("f", [2, 4])
def test_sum_of_the_coarse_cells_and_the_variance(f):
    """f^3 * fsum(coarse rho) against fsum(fine rho): every coarse cell carries n = f^3 + 1 roundings (f^3 - 1 additions,
    the first addition to +0.0 exact, one division; times f^3, a power of two, is exact), so the totals differ by at most
    n * 2^-53 * sum|rho|.  <rho^2> - <rho>^2 >= -(3 f^3 + 4) * 2^-53 * <rho^2>: <rho^2> carries a relative error of at most
    (f^3 + 1) u, <rho> an absolute one of at most f^3 u sqrt(<rho^2>), which enters the square twice, and the exact
    moments obey Jensen's inequality."""
    sim = _sim("ot48" if f == 2 else "ot16")
    _, t = sim.coarsen("mhd_w_d", f, moments=True)
    got = t.cpu().numpy()
    ind = sim.pmesh.mb_indcs
    rho = sim.phys.w0[:, 0].cpu().numpy()
    fine = rho[:, ind.ks:ind.ke + 1, ind.js:ind.je + 1, ind.is_:ind.ie + 1]
    n = f**3 + 1
    total = float(f**3)*math.fsum(got[0].ravel().tolist())
    want = math.fsum(fine.ravel().tolist())
    bound = n*cc.U*math.fsum(np.abs(fine).ravel().tolist())
    print("f=%d: f^3*fsum(coarse) %.17g, fsum(fine) %.17g, |diff| %.3e, bound %.3e" % (f, total, want, abs(total - want), bound))
    assert abs(total - want) <= bound
    m1, m2 = got[0], got[1]
    slack = (3*f**3 + 4)*cc.U*m2
    worst = float(((m1*m1 - m2)/slack).max())
    print("f=%d: worst (<x>^2 - <x^2>)/bound %.3f, min variance %.3e" % (f, worst, float((m2 - m1*m1).min())))
    assert np.all(m2 - m1*m1 >= -slack)
    assert np.all(got[3] >= 0.0) and np.all(m2 > 0.0)


# ---- hosts ---------------------------------------------------------------------------------------------------------
def test_native_host_gives_the_python_hosts_bits():
    from athenak_amd.native import NativeSimulation
    deck, ov = pu.deck_overrides("orszag_tang", (24, 12, 12), 3, (12, 12, 12), cfl=0.3)
    a, b = Simulation(load_deck(deck, ov)), NativeSimulation(load_deck(deck, ov))
    assert a.Execute(max_cycles=4) == 4 and b.Execute(max_cycles=4) == 4
    assert torch.equal(a.phys.u0, b.phys.u0)
    for var, f, mom, gz in (("mhd_w_bcc", 2, True, False), ("mhd_u", 4, False, True), ("mhd_j2", 3, True, False),
                            ("mhd_bcc", 6, True, False)):
        for staged in (False, True, None):
            la, ta = a.coarsen(var, f, moments=mom, ghost_zones=gz, staged=staged)
            lb, tb = b.coarsen(var, f, moments=mom, ghost_zones=gz, staged=staged)
            assert la == lb
            dc.assert_bits(tb.cpu().numpy(), ta.cpu().numpy(), "C++ host %s f=%d" % (var, f))
        dc.assert_bits(ta.cpu().numpy(), cc.restated(a, var, f, mom, gz)[1], "Python host %s f=%d" % (var, f))
    b.close()


# ---- ranks, through the command line -----------------------------------------------------------------------------------
RANK_ARGS = _mesh((32, 16, 16), (8, 8, 8)) + ["time/nlim=3", "time/cfl_number=0.3"]
RANK_OUTPUTS = """<output1>
file_type = cbin
variable = mhd_w_bcc
coarsen_factor = 2
compute_moments = true
dcycle = 1
<output2>
file_type = cbin
variable = mhd_j2
id = j2gz
coarsen_factor = 4
ghost_zones = true
dcycle = 3
"""


def _run_ranks(world, outdir, host="python"):
    """`python -m athenak_amd` once per rank (gloo, the ranks share the GPU), each process under its own time limit"""
    from test_distributed_gloo import _free_port
    deck = os.path.join(outdir, "ot_cbin.athinput")
    with open(deck, "w") as fp:
        fp.write(open(os.path.join(ROOT, "athenak_amd", "inputs", "orszag_tang.athinput")).read() + RANK_OUTPUTS)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), WORLD_SIZE=str(world),
               MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), AKMI_DIST_BACKEND="gloo", LOCAL_RANK="0")
    procs = [subprocess.Popen([sys.executable, "-m", "athenak_amd", "-i", deck, "-d", outdir, "--host", host] + RANK_ARGS,
                              env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    try:
        for r, p in enumerate(procs):
            out, _ = p.communicate(timeout=150)
            assert p.returncode == 0, "rank %d of %d:\n%s" % (r, world, out.decode()[-2000:])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return dc.files_of(outdir)


@pytest.fixture(scope="module")
def one_process_files():
    with tempfile.TemporaryDirectory() as d:
        return _run_ranks(1, d)


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_write_the_one_process_file_byte_for_byte(one_process_files, world):
    want = {k: v for k, v in one_process_files.items() if k.endswith(".cbin")}
    # the initial output, one per dcycle and the final one
    assert sorted(want) == sorted(["cbin_mhd_w_bcc_2/OrszagTang.mhd_w_bcc.%05d.cbin" % n for n in range(5)] +
                                  ["cbin_j2gz_4/OrszagTang.j2gz.%05d.cbin" % n for n in range(3)])
    with tempfile.TemporaryDirectory() as d:
        got = {k: v for k, v in _run_ranks(world, d).items() if k.endswith(".cbin")}
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], (world, k, len(got[k]), len(want[k]))
    p_blocks = 32*16*16//512
    print("%d ranks: %d files byte-identical, %d bytes in all, %d MeshBlocks each" % (world, len(want),
                                                                                      sum(len(v) for v in want.values()), p_blocks))


def test_command_line_on_the_native_host_writes_the_python_hosts_files_byte_for_byte(one_process_files):
    """`python -m athenak_amd --host native` against the default host: the complete files, pre-header, `header offset=` line
    and parameter dump included"""
    want = {k: v for k, v in one_process_files.items() if k.endswith(".cbin")}
    assert len(want) == 8
    with tempfile.TemporaryDirectory() as d:
        got = {k: v for k, v in _run_ranks(1, d, host="native").items() if k.endswith(".cbin")}
    assert sorted(got) == sorted(want)
    for k in want:
        print("%s: %d bytes, %d of them header" % (k, len(want[k]), want[k].index(b"<par_end>\n") + 10))
        assert got[k] == want[k], (k, len(got[k]), len(want[k]))


def test_one_process_files_hold_the_records_of_every_block(one_process_files):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.cbin")
        open(path, "wb").write(one_process_files["cbin_mhd_w_bcc_2/OrszagTang.mhd_w_bcc.00003.cbin"])
        p = R.parse_cbin(path)
    assert len(p["blocks"]) == 16 and p["preheader"]["cycle"] == "3" and p["preheader"]["number of moments"] == "4"
    assert len(p["names"]) == 32 and p["blocks"][0][3].shape == (32, 4, 4, 4)
    assert all(b[0] == (2, 5, 2, 5, 2, 5) for b in p["blocks"])
    assert all(np.isfinite(b[3]).all() for b in p["blocks"])


# ---- the deck --------------------------------------------------------------------------------------------------------
def test_cbin_deck_writes_its_files_and_the_parser_reads_the_restatement():
    from athenak_amd.outputs import Outputs
    pin = load_deck("turb_mhd_cbin.athinput", _mesh((16, 16, 16), (8, 8, 8)) + ["time/nlim=3"])
    for blk in ("output1", "output2"):
        pin.SetInteger(blk, "dcycle", 1)                  # the deck's dt = 0.01 would not come round in three cycles
    sim = Simulation(pin, initialize=False)
    pm, drv = sim.pmesh, sim.pdriver
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        try:
            pout = Outputs(pin, pm)
            drv.Initialize(pm, pin, pout)
            assert drv.Execute(pm, pin) == 3
            drv.Finalize(pm, pin, pout)
        finally:
            os.chdir(here)
        files = sorted(dc.files_of(d))
        assert files == sorted(["cbin_mhd_w_bcc_4/TurbMHDCbin.mhd_w_bcc.%05d.cbin" % n for n in range(5)] +
                               ["cbin_mhd_j2_2/TurbMHDCbin.mhd_j2.%05d.cbin" % n for n in range(5)])
        for dn, var, f, mom in (("cbin_mhd_w_bcc_4", "mhd_w_bcc", 4, True), ("cbin_mhd_j2_2", "mhd_j2", 2, False)):
            labels, want = cc.restated(sim, var, f, mom)
            for n in (3, 4):                                  # after the third cycle, and the final output of the same state
                p = R.parse_cbin(os.path.join(d, dn, "TurbMHDCbin.%s.%05d.cbin" % (var, n)))
                assert p["names"] == labels and p["preheader"]["coarsening factor"] == str(f) and p["preheader"]["cycle"] == "3"
                assert len(p["blocks"]) == 8
                for m, (idx, logical, geom, data) in enumerate(p["blocks"]):
                    assert idx == (2, 2 + 8//f - 1)*3 and logical[3] == 0
                    assert np.array_equal(data.view(np.uint32), want[:, m].astype(np.float32).view(np.uint32)), (var, n, m)
