"""gpu: derived output variables through the HIP entry (akmi_derived_var, csrc/akmi_derived.hip).

  * every variable equals the numpy restatement of tests/derived_restate.py BIT FOR BIT over the reference's index range
    and is +0 outside it, on evolved states (Orszag-Tang after 10 cycles, a driven box after 5, a 1-D Riemann problem),
    1-D / 2-D / 3-D, one block and eight blocks of 24 x 12 x 10, two and four ghost cells.  The restatement's docstring
    names the expression that fixes the order of every sum; no tolerance anywhere;
  * div B after 50 cycles, uniform and statically refined;
  * second-order convergence on an analytic field; the writers; both hosts; two ranks."""
import ctypes as C
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
from athenak_amd import capi, outputs  # noqa: E402
from athenak_amd.main import Simulation, load_deck  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0**-53


def _evolved(deck, ov, cycles):
    sim = Simulation(load_deck(deck, ov))
    assert sim.Execute(max_cycles=cycles) == cycles
    return sim


def _check_all(sim, names):
    bx, a = dc.pack_arrays(sim)
    for name, key in names.items():
        got = sim.derived(name).cpu().numpy()
        assert got.shape[1] == 1
        dc.assert_bits(got[:, 0], dc.restated(key, bx, a), name)
        dc.outside_is_fill(got[:, 0], bx, key)
        assert np.isfinite(got).all(), name
        if sim.pmesh.multi_d and key != "divb":          # (a 1-D hydro shock tube has no vorticity)
            assert np.abs(got).max() > 0.0, name
    return bx, a


def _mesh(n, mb):
    ov = []
    for q in range(3):
        ov += ["mesh/nx%d=%d" % (q + 1, n[q]), "meshblock/nx%d=%d" % (q + 1, mb[q])]
    return ov


MHD_CASES = [
    # deck, mesh, MeshBlock, cycles
    ("rj2a.athinput", (64, 1, 1), (64, 1, 1), 10),
    ("rj2a.athinput", (96, 1, 1), (24, 1, 1), 10),
    ("orszag_tang.athinput", (48, 24, 1), (48, 24, 1), 10),
    ("orszag_tang.athinput", (48, 48, 1), (24, 12, 1), 10),
    ("orszag_tang.athinput", (24, 12, 10), (24, 12, 10), 10),
    ("orszag_tang.athinput", (48, 24, 20), (24, 12, 10), 10),          # 8 blocks, no cube, x1 no multiple of 64
    ("turb_mhd.athinput", (48, 24, 20), (24, 12, 10), 5),
    ("turb_mhd.athinput", (24, 12, 10), (24, 12, 10), 5),
]


@pytest.mark.parametrize("ng", [2, 4])
@pytest.mark.parametrize("deck,n,mb,cycles", MHD_CASES, ids=lambda v: str(v).replace(".athinput", "").replace(" ", ""))
def test_mhd_variables_bit_identical_to_the_restatement(deck, n, mb, cycles, ng):
    sim = _evolved(deck, _mesh(n, mb) + ["mesh/nghost=%d" % ng, "time/nlim=-1"], cycles)
    names = dict(dc.MHD_NAMES)
    names["temperature"] = "temperature"
    _check_all(sim, names)


@pytest.mark.parametrize("ng", [2, 4])
@pytest.mark.parametrize("deck,n,mb,cycles", [("sod.athinput", (96, 1, 1), (24, 1, 1), 10),
                                              ("turb_hydro.athinput", (48, 24, 20), (24, 12, 10), 5),
                                              ("rt2d.athinput", (48, 48, 1), (24, 12, 1), 10)],
                         ids=lambda v: str(v).replace(".athinput", "").replace(" ", ""))
def test_hydro_variables_bit_identical_to_the_restatement(deck, n, mb, cycles, ng):
    # (rt2d.athinput asks for ppm4, which needs three ghost cells: PLM, so that the deck is valid with two as well)
    sim = _evolved(deck, _mesh(n, mb) + ["mesh/nghost=%d" % ng, "time/nlim=-1", "hydro/reconstruct=plm"], cycles)
    names = dict(dc.HYDRO_NAMES)
    names["temperature"] = "temperature"
    _check_all(sim, names)
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*mhd_j2"):
        sim.derived("mhd_j2")


def _divb_bound(sim, a, nupdates):
    """Bound of |div B| from its expression, ((x1f[i+1] - x1f[i])/dx1 + (x2f[j+1] - x2f[j])/dx2) + (x3f[k+1] - x3f[k])/dx3:
    constrained transport keeps the sum zero in exact arithmetic, so what is left is rounding.  Each of the six face
    values carries at most 8 roundings per stage update (the two EMF differences, their scaling by dt/dx, the sum, and the
    three operations of the Runge-Kutta average), each at most u*Bmax, u = 2^-53; each face value enters one difference
    that is divided by its dx; the three differences, three divisions and two additions of the expression itself add at
    most 8 u Bmax/dx.  bound = (6*8*nupdates + 8) u Bmax/dxmin."""
    bmax = max(np.abs(f).max() for f in a["faces"])
    ndim = 1 + int(sim.pmesh.multi_d) + int(sim.pmesh.three_d)
    dxmin = a["dx"][:, :ndim].min()
    return (6*8*nupdates + 8)*U*bmax/dxmin


def test_divb_after_50_cycles_uniform():
    sim = _evolved("orszag_tang.athinput", _mesh((32, 32, 32), (16, 16, 16)) + ["time/nlim=-1"], 50)
    bx, a = dc.pack_arrays(sim)
    got = sim.derived("mhd_divb").cpu().numpy()[:, 0]
    dc.assert_bits(got, dc.restated("divb", bx, a), "mhd_divb")
    bound = _divb_bound(sim, a, nupdates=50*2)
    print("divb uniform: max |divb| active %.3e, whole array %.3e, bound %.3e, |B|max/dx %.3e" % (
        np.abs(bx.act(got)).max(), np.abs(got).max(), bound, max(np.abs(f).max() for f in a["faces"])/a["dx"].min()))
    assert np.abs(got).max() <= bound          # ghost cells included: the loop of the reference covers them


def test_divb_after_50_cycles_refined_mesh():
    """two levels (blast_mhd_smr): every block, the cells along fine/coarse boundaries and the ghost cells included"""
    deck, ov = pu.deck_overrides("blast_smr", 32, 3, 8)
    sim = _evolved(deck, ov + ["time/nlim=-1"], 50)
    assert sim.pmesh.multilevel
    bx, a = dc.pack_arrays(sim)
    got = sim.derived("mhd_divb").cpu().numpy()[:, 0]
    dc.assert_bits(got, dc.restated("divb", bx, a), "mhd_divb")
    nst = {"rk1": 1, "rk2": 2, "rk3": 3}[sim.pin.GetString("time", "integrator")]
    bound = _divb_bound(sim, a, nupdates=50*nst)
    print("divb refined: max |divb| active %.3e, whole array %.3e, bound %.3e" % (
        np.abs(bx.act(got)).max(), np.abs(got).max(), bound))
    assert np.abs(got).max() <= bound


def _entry_eval(key, bx, n, a):
    """akmi_derived_var on device copies of host arrays"""
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
           (("w0", a["w0"]), ("bcc", a["bcc"]), ("f1", a["faces"][0]), ("f2", a["faces"][1]), ("f3", a["faces"][2]),
            ("dx", a["dx"]))}
    pk = dc.pack_struct(len(a["w0"]), a["w0"].shape[1], (n, n, n), bx.ng, a["dx"])
    pk.dx = dev["dx"].data_ptr()
    out = torch.full((len(a["w0"]), bx.N3, bx.N2, bx.N1), 7.0, dtype=torch.float64, device="cuda")
    capi.check(capi.lib().akmi_derived_var(C.byref(pk), capi.DERIVED[key], capi._p(dev["w0"]), None, capi._p(dev["bcc"]),
                                           capi._p(dev["f1"]), capi._p(dev["f2"]), capi._p(dev["f3"]), capi._p(out), 1,
                                           capi._stream()), "derived_var")
    return out.cpu().numpy()


def test_second_order_convergence_on_an_analytic_field():
    """B = v = (-sin y, sin x, 0): the error ratio between 32^3 and 64^3 is 4 for a second-order stencil (3.5 ... 4.5)"""
    from test_derived_host import analytic_errors
    errs = analytic_errors(_entry_eval)
    for key in ("jz", "j2", "wz", "w2"):
        ratio = errs[key, 32]/errs[key, 64]
        print("convergence %s: %.3e -> %.3e, ratio %.4f" % (key, errs[key, 32], errs[key, 64], ratio))
        assert 3.5 <= ratio <= 4.5, (key, ratio)


def test_entry_refuses_what_it_cannot_compute():
    L = capi.lib()
    dx = np.ones((1, 3))
    pk = dc.pack_struct(1, 5, (8, 8, 8), 2, dx)
    out = torch.zeros(12**3, dtype=torch.float64, device="cuda")
    assert L.akmi_derived_ncomp(capi.DERIVED["curv"]) == 1 and L.akmi_derived_ncomp(99) == -1
    assert L.akmi_derived_var(C.byref(pk), 99, None, None, None, None, None, None, capi._p(out), 1, None) < 0
    assert L.akmi_derived_var(C.byref(pk), capi.DERIVED["j2"], None, None, None, None, None, None, capi._p(out), 1, None) < 0
    assert b"bcc0" in L.akmi_last_error()
    assert L.akmi_derived_var(C.byref(pk), capi.DERIVED["wz"], capi._p(out), None, None, None, None, None, capi._p(out), 3, None) < 0
    pk.is_ideal, pk.nvar = 0, 4
    assert L.akmi_derived_var(C.byref(pk), 0, capi._p(out), None, None, None, None, None, capi._p(out), 1, None) < 0
    assert b"temperature" in L.akmi_last_error()


# ---- through the writers ---------------------------------------------------------------------------------------
def test_tab_and_bin_files_with_derived_variables():
    with tempfile.TemporaryDirectory() as d:
        sim = dc.run_and_write(dc.writer_deck(dc.WRITER_OUTPUTS), d)
        arr = dc.check_writer_files(sim, d)
        bx, a = dc.pack_arrays(sim)
        for name in arr:
            dc.assert_bits(arr[name], dc.restated(dc.MHD_NAMES[name], bx, a), name)


def test_files_without_scalars_are_those_of_the_stored_array_path(monkeypatch):
    with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2:
        dc.run_and_write(dc.writer_deck(dc.STORED_OUTPUTS), d1)
        monkeypatch.setattr(outputs, "_outvars", dc.parent_outvars)
        dc.run_and_write(dc.writer_deck(dc.STORED_OUTPUTS), d2)
        a, b = dc.files_of(d1), dc.files_of(d2)
        assert sorted(a) == sorted(b) and len(a) == 6
        for k in a:
            assert a[k] == b[k], k


def test_scalar_columns_are_written():
    text = dc.writer_deck("<output1>\nfile_type = bin\nvariable = mhd_w_bcc\ndcycle = 1\n<output2>\nfile_type = bin\n"
                          "variable = mhd_u_s\ndcycle = 1\n").replace("gamma = 1.666666667\n",
                                                                       "gamma = 1.666666667\nnscalars = 2\n")
    text = text.replace("fused_stage = false", "fused_stage = true")       # the fused stage carries the scalars along
    from athenak_amd.parameter_input import ParameterInput
    with tempfile.TemporaryDirectory() as d:
        pin = ParameterInput(text=text)
        sim = Simulation(pin)
        sim.Execute(max_cycles=2)
        ph, ng = sim.phys, sim.pmesh.mb_indcs.ng
        ph.w0[:, 5:7].normal_()                   # the generator leaves the scalars at zero: give the columns content
        os.chdir(d)
        try:
            outputs.Outputs(pin, sim.pmesh).MakeOutputs(sim.pmesh, pin)
        finally:
            os.chdir(ROOT)
        names, blocks = dc.read_bin(os.path.join(d, "bin", "OrszagTang.mhd_w_bcc.00000.bin"))
        assert names == ["dens", "velx", "vely", "velz", "eint", "s_00", "s_01", "bcc1", "bcc2", "bcc3"]
        w, b = ph.w0.cpu().numpy(), ph.bcc0.cpu().numpy()
        for m, (h, data) in enumerate(blocks):
            want = np.concatenate([w[m], b[m]])[:, ng:-ng, ng:-ng, ng:-ng].astype(np.float32)
            assert np.array_equal(data, want)
        names, _ = dc.read_bin(os.path.join(d, "bin", "OrszagTang.mhd_u_s.00000.bin"))
        assert names == ["r_00", "r_01"]


# ---- hosts and ranks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,names", [("orszag_tang", dc.MHD_NAMES), ("linear_wave_hydro", dc.HYDRO_NAMES)])
def test_native_host_gives_the_python_hosts_arrays(problem, names):
    from athenak_amd.native import NativeSimulation
    deck, ov = pu.deck_overrides(problem, (24, 12, 12), 3, (12, 12, 12), cfl=0.3)
    a = Simulation(load_deck(deck, ov))
    b = NativeSimulation(load_deck(deck, ov))
    assert a.Execute(max_cycles=4) == 4 and b.Execute(max_cycles=4) == 4
    assert torch.equal(a.phys.u0, b.phys.u0)
    for name in list(names) + ["temperature"]:
        x, y = a.derived(name).cpu().numpy(), b.derived(name).cpu().numpy()
        dc.assert_bits(y, x, name)
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*mhd_jcon"):
        b.derived("mhd_jcon")
    b.close()


def _rank_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    deck, ov = pu.deck_overrides("orszag_tang", 32, 3, 16, cfl=0.3)
    sim = Simulation(load_deck(deck, ov), my_rank=rank, nranks=world)
    sim.Execute(max_cycles=3)
    pk = sim.pmesh.pmb_pack
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), gids=pk.gids,
             **{n: sim.derived(n).cpu().numpy() for n in dc.MHD_NAMES})
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_give_the_one_process_arrays_block_by_block():
    import torch.multiprocessing as mp
    from test_distributed_gloo import _free_port
    deck, ov = pu.deck_overrides("orszag_tang", 32, 3, 16, cfl=0.3)
    one = Simulation(load_deck(deck, ov))
    one.Execute(max_cycles=3)
    want = {n: one.derived(n).cpu().numpy() for n in dc.MHD_NAMES}
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_rank_worker, args=(2, _free_port(), d), nprocs=2, join=True)
        seen = 0
        for r in range(2):
            z = np.load(os.path.join(d, "rank%d.npz" % r))
            g0 = int(z["gids"])
            for n in dc.MHD_NAMES:
                dc.assert_bits(z[n], want[n][g0:g0 + len(z[n])], "%s rank %d" % (n, r))
            seen += len(z["mhd_j2"])
        assert seen == len(want["mhd_j2"]) == 8
