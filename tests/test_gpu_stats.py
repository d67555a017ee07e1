"""gpu: the turbulence history columns (akmi_turb_history) and the pdf outputs (akmi_pdf), csrc/akmi_stats.hip.

  * the eleven history sums against math.fsum of the numpy restatement (tests/stats_restate.py), each within
    d * 2^-53 * sum|terms|, d the depth of the reduction the library builds (computed from the shape, printed);
    bit-identical between one process and 2 / 4 ranks and between the Python and the C++ host;
  * histogram counts EQUAL to the restatement (linear bins: no exclusions, with values below, above, on an edge and a
    NaN; log bins: cells within 1e-9 of an edge left out, at most 1 in 10^4); weights of every bin within
    n_b * 2^-53 * sum|w| of math.fsum; totals against the mesh volume / the mass column; both accumulation paths.

Every test prints the figures it asserts on (depth, worst err/bound, totals) before it asserts."""
import ctypes as C
import math
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import derived_cases as dc  # noqa: E402
import parity_util as pu  # noqa: E402
import stats_cases as sc  # noqa: E402
import stats_restate as S  # noqa: E402
from athenak_amd import capi  # noqa: E402
from athenak_amd.main import Simulation, load_deck  # noqa: E402

pytestmark = pytest.mark.gpu


def _mesh(n, mb):
    ov = []
    for q in range(3):
        ov += ["mesh/nx%d=%d" % (q + 1, n[q]), "meshblock/nx%d=%d" % (q + 1, mb[q])]
    return ov


def _evolved(deck, ov, cycles):
    sim = Simulation(load_deck(deck, ov))
    assert sim.Execute(max_cycles=cycles) == cycles
    return sim


# ---- 1. history against the restatement ------------------------------------------------------------------------
HIST_CASES = [
    ("orszag_tang.athinput", (16, 16, 16), (16, 16, 16), 10),
    ("orszag_tang.athinput", (48, 24, 20), (24, 12, 10), 10),          # 8 blocks, no cube, no multiple of a wave
    ("turb_mhd.athinput", (16, 16, 16), (16, 16, 16), 5),
    ("turb_mhd.athinput", (48, 24, 20), (24, 12, 10), 5),
    ("orszag_tang.athinput", (32, 16, 1), (32, 16, 1), 10),            # 2-D
    ("rj2a.athinput", (96, 1, 1), (24, 1, 1), 10),                     # 1-D
]


@pytest.mark.parametrize("ng", [2, 4])
@pytest.mark.parametrize("deck,n,mb,cycles", HIST_CASES, ids=lambda v: str(v).replace(".athinput", "").replace(" ", ""))
def test_history_sums_within_the_bound_of_the_reduction(deck, n, mb, cycles, ng):
    sim = _evolved(deck, _mesh(n, mb) + ["mesh/nghost=%d" % ng, "time/nlim=-1"], cycles)
    got = sim.turb_history()
    bx, a = dc.pack_arrays(sim)
    terms = S.turb_terms(bx, a["w0"], a["bcc"], a["faces"], a["dx"])
    depth = S.reduction_depth(mb[0]*mb[1]*mb[2], sim.pmesh.nmb_total)
    worst = 0.0
    for q, lab in enumerate(S.LABELS):
        want = math.fsum(terms[q].ravel().tolist())
        bound = S.sum_bound(terms[q], depth)
        err = abs(got[q] - want)
        worst = max(worst, err/bound if bound > 0 else 0.0)
        assert err <= bound, (lab, got[q], want, err, bound, depth)
    print("history %s %s ng=%d: depth d = %d, worst err/bound %.3f" % (deck, n, ng, depth, worst))
    assert all(np.isfinite(got)) and got[3] > 0.0 and got[9] >= 0.0


# ---- 2. ranks and hosts ------------------------------------------------------------------------------------------
RANK_CASE = ("orszag_tang", 32, 3, 16)
RANK_PDF = dict(variable="mhd_w_d", bin_min=0.05, bin_max=30.0, nbin=7, mass_weighted=True, variable_2="mhd_j2", bin2_min=1e-3, bin2_max=1e3, nbin2=9)


def _rank_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    deck, ov = pu.deck_overrides(*RANK_CASE, cfl=0.3)
    sim = Simulation(load_deck(deck, ov), my_rank=rank, nranks=world)
    sim.Execute(max_cycles=3)
    h = sim.turb_history()
    r = sim.pdf(**RANK_PDF)
    if rank == 0:
        np.savez(os.path.join(outdir, "w%d.npz" % world), hist=np.array(h), counts=r.counts, weights=r.weights)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def one_process():
    deck, ov = pu.deck_overrides(*RANK_CASE, cfl=0.3)
    sim = Simulation(load_deck(deck, ov))
    sim.Execute(max_cycles=3)
    return sim


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_give_the_one_process_sums_bit_for_bit_and_the_same_counts(one_process, world):
    import torch.multiprocessing as mp
    from test_distributed_gloo import _free_port
    sim = one_process
    h = np.array(sim.turb_history())
    r = sim.pdf(**RANK_PDF)
    want = _restated_pdf(sim, **RANK_PDF)
    sc.check_hist(r.counts, r.weights, want, "one process")
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_rank_worker, args=(world, _free_port(), d), nprocs=world, join=True)
        z = np.load(os.path.join(d, "w%d.npz" % world))
        dc.assert_bits(z["hist"], h, "history sums, %d ranks" % world)
        assert np.array_equal(z["counts"], r.counts) and int(r.counts.sum()) == 32**3
        sc.check_hist(z["counts"], z["weights"], want, "%d ranks" % world)


def _field(sim, bx, a, name):
    """the active cells of an output variable by name, from the arrays of the pack"""
    if name == "mhd_j2":
        return sc.active(bx, dc.restated("j2", bx, a))
    arr, comp = {"mhd_w_d": (a["w0"], 0), "mhd_bcc1": (a["bcc"], 0), "mhd_u_e": (sim.phys.u0.cpu().numpy(), 4)}[name]
    return sc.active(bx, arr[:, comp])


def _restated_pdf(sim, variable, bin_min, bin_max, nbin, logscale=True, mass_weighted=False, variable_2=None, bin2_min=0.0,
                  bin2_max=1.0, nbin2=0, logscale2=True, force_global=False):
    """what Simulation.pdf of these arguments has to return, restated from the arrays of the pack (every MeshBlock)"""
    bx, a = dc.pack_arrays(sim)
    w = sc.cell_volumes(bx, a["dx"], len(a["w0"]))
    if mass_weighted:
        w = w*sc.active(bx, sim.phys.u0.cpu().numpy()[:, 0])
    e1, s1 = S.pdf_bins(bin_min, bin_max, nbin, logscale)
    if variable_2 is None:
        return sc.restated_hist(_field(sim, bx, a, variable), w, e1, s1, logscale)
    e2, s2 = S.pdf_bins(bin2_min, bin2_max, nbin2, logscale2)
    return sc.restated_hist(_field(sim, bx, a, variable), w, e1, s1, logscale, _field(sim, bx, a, variable_2), e2, s2, logscale2)


def test_native_host_gives_the_python_hosts_statistics():
    from athenak_amd.native import NativeSimulation
    deck, ov = pu.deck_overrides("orszag_tang", (24, 12, 12), 3, (12, 12, 12), cfl=0.3)
    a = Simulation(load_deck(deck, ov))
    b = NativeSimulation(load_deck(deck, ov))
    assert a.Execute(max_cycles=4) == 4 and b.Execute(max_cycles=4) == 4
    assert torch.equal(a.phys.u0, b.phys.u0)
    dc.assert_bits(np.array(b.turb_history()), np.array(a.turb_history()), "history sums, C++ host")
    for kw in (dict(variable="mhd_w_d", bin_min=0.05, bin_max=30.0, nbin=7, mass_weighted=True),
               dict(variable="mhd_bcc1", bin_min=-2.0, bin_max=2.0, nbin=16, logscale=False, variable_2="mhd_j2",
                    bin2_min=1e-3, bin2_max=1e3, nbin2=9),
               dict(variable="mhd_u_e", bin_min=0.1, bin_max=10.0, nbin=5, force_global=True)):
        x, y = a.pdf(**kw), b.pdf(**kw)
        assert np.array_equal(x.counts, y.counts) and x.nan_dropped == y.nan_dropped == 0
        assert int(x.counts.sum()) == 24*12*12
        want = _restated_pdf(a, **kw)
        sc.check_hist(x.counts, x.weights, want, "Python host %s" % kw["variable"])
        sc.check_hist(y.counts, y.weights, want, "C++ host %s" % kw["variable"])
    b.close()


# ---- 3.-6. synthetic histograms through the entry ----------------------------------------------------------------
def _entry(vals, nx, ng, dx, edges, step, log, vals2=None, ax2=None, dens=None, force_global=False):
    """akmi_pdf on device copies of host arrays (nmb, N3, N2, N1); dens: (nmb, 5, N3, N2, N1) conserved array"""
    nmb = len(vals)
    dxd = torch.from_numpy(np.ascontiguousarray(dx)).cuda()
    pk = dc.pack_struct(nmb, 5, nx, ng, dx)
    pk.dx = dxd.data_ptr()
    v1 = torch.from_numpy(np.ascontiguousarray(vals)).cuda()
    x = capi.PdfAxis(v1.data_ptr(), 1, 0, len(edges) - 1, int(log), edges[0], edges[-1], step)
    y, v2 = None, None
    ny = 1
    if vals2 is not None:
        e2, s2, l2 = ax2
        v2 = torch.from_numpy(np.ascontiguousarray(vals2)).cuda()
        y = capi.PdfAxis(v2.data_ptr(), 1, 0, len(e2) - 1, int(l2), e2[0], e2[-1], s2)
        ny = len(e2) + 1
    u0 = torch.from_numpy(np.ascontiguousarray(dens)).cuda() if dens is not None else None
    counts = torch.full((ny, len(edges) + 1), 7, dtype=torch.int64, device="cuda")      # the entry clears them
    weights = torch.full((ny, len(edges) + 1), 7.0, dtype=torch.float64, device="cuda")
    nan = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    capi.check(capi.lib().akmi_pdf(C.byref(pk), C.byref(x), C.byref(y) if y is not None else None, capi._p(u0),
                                   capi._p(counts), capi._p(weights), capi._p(nan), int(force_global), capi._stream()), "pdf")
    return counts.cpu().numpy(), weights.cpu().numpy(), int(nan.cpu()[0])


def _box(nx, ng, nmb):
    bx = S_box(nx, ng)
    # cell sizes that are no powers of two and differ between blocks (as on a refined mesh)
    dx = np.array([[1.0/24/(1 + m % 2), 0.7/12/(1 + m % 2), 1.3/10/(1 + m % 2)] for m in range(nmb)])
    return bx, dx


def S_box(nx, ng):
    import derived_restate as R
    return R.Box(nx[0], nx[1], nx[2], ng)


SYN_SHAPES = [((24, 12, 10), 8), ((16, 16, 16), 1)]


@pytest.mark.parametrize("nx,nmb", SYN_SHAPES)
def test_linear_counts_equal_and_weights_within_the_bound(nx, nmb):
    bx, dx = _box(nx, 2, nmb)
    full = sc.linear_field((nmb, bx.N3, bx.N2, bx.N1), seed=11 + nmb, planted=False)
    sc.plant(bx.act(full), seed=3)                        # edge values, infinities and the NaN in ACTIVE cells
    rng = np.random.default_rng(5)
    u0 = rng.uniform(0.5, 1.5, (nmb, 5, bx.N3, bx.N2, bx.N1))
    vals = sc.active(bx, full)
    assert np.isnan(vals).sum() == 1 and (vals == 8.0).sum() == 1
    edges, step = S.pdf_bins(0.0, 8.0, 16, False)
    vol = sc.cell_volumes(bx, dx, nmb)
    for mass in (False, True):
        w = vol*sc.active(bx, u0[:, 0]) if mass else vol
        counts, wl, nan, _ = S.histogram(vals, w, edges, step, False)
        got_c, got_w, got_nan = _entry(full, nx, 2, dx, edges, step, False, dens=u0 if mass else None)
        assert np.array_equal(got_c, counts) and got_nan == nan == int(np.isnan(vals).sum())
        assert got_c[0, 0] > 0 and got_c[0, 17] > 0 and int(got_c.sum()) + nan == vals.size
        worst = sc.check_weights(got_w, wl, "linear, mass=%s" % mass)
        print("linear %s nmb=%d mass=%s: worst err/bound %.3f, %d NaN dropped" % (nx, nmb, mass, worst, got_nan))


@pytest.mark.parametrize("nbin,lo,hi", [(16, 1e-2, 1e2), (7, 0.05, 30.0), (100, 1e-3, 1e3)])
def test_log_counts_equal_away_from_the_edges(nbin, lo, hi):
    nx, nmb = (24, 12, 10), 8
    bx, dx = _box(nx, 2, nmb)
    full = sc.lognormal_field((nmb, bx.N3, bx.N2, bx.N1))
    vals = sc.active(bx, full)
    assert vals.size == 23040
    edges, step = S.pdf_bins(lo, hi, nbin, True)
    near = np.array([S.pdf_near_edge(v, edges, step, True) for v in vals])
    print("log %d bins: %d of %d cells within 1e-9 of an edge" % (nbin, int(near.sum()), vals.size))
    assert near.sum() <= vals.size/10**4
    # the cells left out are made NaN on both sides: dropped by the entry, counted apart
    act = bx.act(full)
    act[near.reshape(act.shape)] = np.nan
    vals = act.reshape(-1)
    vol = sc.cell_volumes(bx, dx, nmb)
    counts, wl, nan, _ = S.histogram(vals, vol, edges, step, True)
    got_c, got_w, got_nan = _entry(full, nx, 2, dx, edges, step, True)
    assert np.array_equal(got_c, counts) and got_nan == nan == int(near.sum())
    sc.check_weights(got_w, wl, "log %d" % nbin)
    # total volume of the pack
    sc.check_total(got_w, got_c, math.fsum(vol.tolist()), math.fsum(vol.tolist()), "log %d: volume" % nbin)


@pytest.mark.parametrize("nb", [(30, 40), (80, 70)], ids=["lds", "above_the_lds_limit"])
def test_both_accumulation_paths(nb):
    """a 2-D histogram through the LDS path and with the global path forced; (80+2)*(70+2) = 5904 entries exceed
    AKMI_PDF_LDS_BINS, so there the global path is taken unforced as well"""
    nx, nmb = (24, 12, 10), 8
    bx, dx = _box(nx, 2, nmb)
    f1 = sc.lognormal_field((nmb, bx.N3, bx.N2, bx.N1), seed=21)
    f2 = sc.linear_field((nmb, bx.N3, bx.N2, bx.N1), seed=22, planted=False)
    sc.plant(bx.act(f2), seed=4)
    e1, s1 = S.pdf_bins(0.05, 30.0, nb[0], True)
    e2, s2 = S.pdf_bins(0.0, 8.0, nb[1], False)
    limit = capi.lib().akmi_pdf_lds_bins()
    assert ((nb[0] + 2)*(nb[1] + 2) <= limit) == (nb == (30, 40)) and limit == 4096
    vol = sc.cell_volumes(bx, dx, nmb)
    v1, v2 = sc.active(bx, f1), sc.active(bx, f2)
    near = np.array([S.pdf_near_edge(v, e1, s1, True) for v in v1])
    assert near.sum() == 0
    counts, wl, nan, _ = S.histogram(v1, vol, e1, s1, True, v2, e2, s2, False)
    a = _entry(f1, nx, 2, dx, e1, s1, True, f2, (e2, s2, False))
    b = _entry(f1, nx, 2, dx, e1, s1, True, f2, (e2, s2, False), force_global=True)
    for got_c, got_w, got_nan in (a, b):
        assert np.array_equal(got_c, counts) and got_nan == nan == 1
        sc.check_weights(got_w, wl, "2-D %s" % (nb,))


def test_constant_field_hits_one_bin():
    nx, nmb = (16, 16, 16), 1
    bx, dx = _box(nx, 2, nmb)
    full = np.full((nmb, bx.N3, bx.N2, bx.N1), 1.0)
    edges, step = S.pdf_bins(1e-2, 1e2, 100, True)
    for fg in (False, True):
        c, w, nan = _entry(full, nx, 2, dx, edges, step, True, force_global=fg)
        assert c.sum() == 4096 and c.max() == 4096 and nan == 0 and c[0, S.pdf_index(1.0, edges, step, True)] == 4096
        vol = float((dx[0, 0]*dx[0, 1])*dx[0, 2])
        assert abs(w.sum() - 4096*vol) <= 4096*sc.U*4096*vol


def test_entry_refuses_what_it_cannot_bin():
    L = capi.lib()
    dx = np.ones((1, 3))
    pk = dc.pack_struct(1, 5, (8, 8, 8), 2, dx)
    buf = torch.zeros(12**3, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(64, dtype=torch.int64, device="cuda")
    x = capi.PdfAxis(buf.data_ptr(), 1, 0, 0, 0, 0.0, 1.0, 1.0)
    assert L.akmi_pdf(C.byref(pk), C.byref(x), None, None, capi._p(cnt), capi._p(buf), capi._p(cnt), 0, None) < 0
    assert b"nbin = 0" in L.akmi_last_error()
    x = capi.PdfAxis(buf.data_ptr(), 1, 0, 4, 1, 0.0, 1.0, 0.25)
    assert L.akmi_pdf(C.byref(pk), C.byref(x), None, None, capi._p(cnt), capi._p(buf), capi._p(cnt), 0, None) < 0
    assert b"positive first edge" in L.akmi_last_error()
    assert L.akmi_turb_history(C.byref(pk), capi._p(buf), None, None, None, None, capi._p(buf), capi._p(buf), None) < 0
    assert b"MHD" in L.akmi_last_error()


# ---- 5., 7. totals and derived variables on simulations ----------------------------------------------------------
def test_totals_and_the_pdf_of_a_derived_variable(one_process):
    sim = one_process
    bx, a = dc.pack_arrays(sim)
    nmb = len(a["w0"])
    vol = sc.cell_volumes(bx, a["dx"], nmb)
    # volume-weighted: the total is the mesh volume
    r = sim.pdf("mhd_w_d", 0.05, 30.0, 7)
    assert int(r.counts.sum()) == vol.size and r.nan_dropped == 0
    ms = sim.pmesh.mesh_size
    volume = (ms.x1max - ms.x1min)*(ms.x2max - ms.x2min)*(ms.x3max - ms.x3min)
    sc.check_total(r.weights, r.counts, volume, math.fsum(vol.tolist()), "volume-weighted total")
    # mass-weighted: the total is the mass column of akmi_history_sums
    r = sim.pdf("mhd_w_d", 0.05, 30.0, 7, mass_weighted=True)
    out = torch.zeros(11, dtype=torch.float64, device="cuda")
    ph = sim.phys
    capi.check(capi.lib().akmi_history_sums(C.byref(ph.pack_c), 1, capi._p(ph.u0), capi._p(ph.b0.x1f), capi._p(ph.b0.x2f),
                                            capi._p(ph.b0.x3f), capi._p(out), capi._stream()), "history_sums")
    w = vol*sc.active(bx, ph.u0.cpu().numpy()[:, 0])
    sc.check_total(r.weights, r.counts, float(out[0]), math.fsum(np.abs(w).tolist()), "mass-weighted total", device_sum=True)
    # a derived variable: the histogram of the array derived() returns
    e, s = S.pdf_bins(1e-3, 1e3, 12, True)
    r = sim.pdf("mhd_j2", 1e-3, 1e3, 12)
    j2 = sim.derived("mhd_j2").cpu().numpy()[:, 0]
    ind = sim.pmesh.mb_indcs
    c, wt, nan = _entry(j2, (ind.nx1, ind.nx2, ind.nx3), ind.ng, a["dx"], e, s, True)
    assert np.array_equal(r.counts, c) and r.nan_dropped == nan and np.array_equal(r.bins, np.array(e))
    vals = sc.active(bx, j2)
    near = np.array([S.pdf_near_edge(v, e, s, True) for v in vals])
    if near.sum() == 0:
        counts, wl, _, _ = S.histogram(vals, vol, e, s, True)
        assert np.array_equal(r.counts, counts)
        sc.check_weights(r.weights, wl, "mhd_j2")


def test_refined_mesh_volume_total():
    """two levels (blast_mhd_smr): fine and coarse blocks carry different weights; the total is the mesh volume"""
    deck, ov = pu.deck_overrides("blast_smr", 32, 3, 8)
    sim = _evolved(deck, ov + ["time/nlim=-1"], 2)
    assert sim.pmesh.multilevel
    r = sim.pdf("mhd_w_d", 0.01, 100.0, 20)
    bx, a = dc.pack_arrays(sim)
    vol = sc.cell_volumes(bx, a["dx"], len(a["w0"]))
    assert vol.max() > 7.0*vol.min() and int(r.counts.sum()) == vol.size        # two levels: volumes 8 : 1
    ms = sim.pmesh.mesh_size
    volume = (ms.x1max - ms.x1min)*(ms.x2max - ms.x2min)*(ms.x3max - ms.x3min)
    sc.check_total(r.weights, r.counts, volume, math.fsum(vol.tolist()), "refined mesh: volume")


def test_stats_deck_writes_its_files():
    from athenak_amd.outputs import Outputs
    pin = load_deck("turb_mhd_stats.athinput", ["mesh/nx1=16", "mesh/nx2=16", "mesh/nx3=16", "meshblock/nx1=8",
                                                 "meshblock/nx2=8", "meshblock/nx3=8"])
    sim = Simulation(pin)
    sim.Execute(max_cycles=2)
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        try:
            Outputs(pin, sim.pmesh).MakeOutputs(sim.pmesh, pin)
        finally:
            os.chdir(here)
        files = sorted(dc.files_of(d))
    assert files == ["TurbMHDStats.mhd.hst", "TurbMHDStats.user.hst", "pdf_mhd_w_d/TurbMHDStats.00000.pdf",
                     "pdf_mhd_w_d/TurbMHDStats.bins.pdf", "pdf_mhd_w_d_mhd_j2/TurbMHDStats.00000.pdf",
                     "pdf_mhd_w_d_mhd_j2/TurbMHDStats.bins.pdf"]
