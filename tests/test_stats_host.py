"""not gpu: the turbulence history columns and the pdf outputs on the host.

  * the arithmetic of the kernels (athenak_amd/csrc/akmi_stats.hpp, compiled for the CPU by tests/host_shim/) against
    the numpy restatement of tests/stats_restate.py: the eleven history terms bit for bit on random states (1-D, 2-D,
    3-D, two and four ghost cells), the bin indices on random values, on values exactly on an edge, below, above, NaN;
  * bin edges of outputs.pdf_bins against the restatement;
  * the files of a pdf block and of <problem>/user_hist = true through the product's host logic on CPU tensors: names,
    directories, header lines, counters;
  * every refusal, with its message; a turbulence deck with an hst block and no user_hist writes the ordinary file."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import derived_cases as dc  # noqa: E402
import stats_cases as sc  # noqa: E402
import stats_restate as S  # noqa: E402
from athenak_amd import capi, outputs  # noqa: E402
from test_derived_host import SHAPES, random_state  # noqa: E402


@pytest.fixture(scope="module")
def shim():
    return sc.build_shim()


@pytest.fixture
def cpu_backend_with_stats():
    sc.install_cpu_backend()
    yield
    sc.uninstall_cpu_backend()


# ---- arithmetic ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ng", [2, 4])
@pytest.mark.parametrize("nx,nmb", SHAPES)
def test_history_terms_are_the_restatement_bit_for_bit(shim, nx, nmb, ng):
    bx, a = random_state(nmb, nx, ng, seed=7 + nx[1]*100 + nx[2]*10 + ng + nmb)
    pk = dc.pack_struct(nmb, 5, nx, ng, a["dx"])
    got = np.zeros((11, nmb, nx[2], nx[1], nx[0]))
    assert shim.hs_turb_terms(C.byref(pk), sc.ptr(a["w0"]), sc.ptr(a["bcc"]), *[sc.ptr(f) for f in a["faces"]],
                              sc.ptr(got)) == 0
    want = S.turb_terms(bx, a["w0"], a["bcc"], a["faces"], a["dx"])
    for q, lab in enumerate(S.LABELS):
        dc.assert_bits(got[q], want[q], "%s %s nmb=%d ng=%d" % (lab, nx, nmb, ng))
    assert np.abs(got[5:9]).max() > 0.0
    # Bx, By, Bz are NOT weighted by the cell volume
    dc.assert_bits(got[0], bx.act(a["bcc"][:, 0]), "Bx")


def test_history_labels():
    assert capi.TURB_HIST_LABELS == S.LABELS and capi.TURB_NHIST == 11


def _shim_bins(shim, x, edges, step, log):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros(x.size, dtype=np.int32)
    shim.hs_pdf_bins(sc.ptr(x), C.c_longlong(x.size), len(edges) - 1, int(log), C.c_double(edges[0]),
                     C.c_double(edges[-1]), C.c_double(step), sc.ptr(out))
    return out


def test_linear_bin_indices_with_the_edge_cases(shim):
    edges, step = S.pdf_bins(0.0, 8.0, 16, False)
    assert edges == [0.5*i for i in range(17)] and step == 0.5
    x = sc.linear_field((23040,), seed=3)
    got = _shim_bins(shim, x, edges, step, False)
    want = [S.pdf_index(v, edges, step, False) for v in x]
    assert sum(w is None for w in want) == 1
    assert [(-1 if w is None else w) for w in want] == got.tolist()
    assert got[x == 8.0].tolist() == [17] and got[x == 0.0].tolist() == [1, 1] and set(got[x < 0.0]) == {0}   # (-0.0 == 0.0)
    assert got[x == 7.5].tolist() == [16] and got[x == np.inf].tolist() == [17] and got[x == -np.inf].tolist() == [0]


@pytest.mark.parametrize("nbin,lo,hi", [(16, 1e-2, 1e2), (7, 0.05, 30.0), (100, 1e-3, 1e3)])
def test_log_bin_indices(shim, nbin, lo, hi):
    """on the CPU the header's log10 IS the C library's: equal without exclusions; and no cell of this field lies within
    1e-9 of an edge (the condition of the GPU test)"""
    edges, step = S.pdf_bins(lo, hi, nbin, True)
    x = sc.lognormal_field((23040,))
    got = _shim_bins(shim, x, edges, step, True)
    assert got.tolist() == [S.pdf_index(v, edges, step, True) for v in x]
    assert sum(S.pdf_near_edge(v, edges, step, True) for v in x) == 0
    if nbin == 7:
        assert (got == 0).sum() > 0 and (got == 8).sum() > 0          # both overflow bins are populated


def test_bin_edges_of_the_product_are_the_restatements():
    for args in ((1e-2, 1e2, 16, True), (0.05, 30.0, 7, True), (0.0, 8.0, 16, False), (-3.0, 11.0, 9, False)):
        e, s = outputs.pdf_bins(*args)
        we, ws = S.pdf_bins(*args)
        assert e.tolist() == we and s == ws


# ---- files, on CPU tensors -------------------------------------------------------------------------------------
PDF_BLOCKS = """
<output1>
file_type = pdf
variable = mhd_w_d
bin_min = 0.01
bin_max = 100.0
nbin = 16
mass_weighted = true
dcycle = 1
<output2>
file_type = pdf
variable = mhd_w_d
id = rho
variable_2 = mhd_j2
bin_min = 0.0
bin_max = 2.0
nbin = 4
logscale = false
bin2_min = 1.0e-3
bin2_max = 1.0e3
nbin2 = 6
dcycle = 1
<output3>
file_type = hst
dcycle = 1
"""


def _turb_pin(text, user_hist=True):
    """the deck with its <problem> block naming the turbulence generator (what Outputs reads of it)"""
    from athenak_amd.parameter_input import ParameterInput
    head, tail = text.split("<problem>")
    tail = tail[tail.index("<output1>"):] if "<output1>" in tail else ""
    return ParameterInput(text=head + "<problem>\npgen_name = turb\n" + ("user_hist = true\n" if user_hist else "") + tail)


def _write_twice(pin, sim, d):
    here = os.getcwd()
    os.chdir(d)
    try:
        out = outputs.Outputs(pin, sim.pmesh)
        out.MakeOutputs(sim.pmesh, pin)
        out.MakeOutputs(sim.pmesh, pin)
    finally:
        os.chdir(here)
    return out


def test_pdf_and_user_history_files(cpu_backend_with_stats):
    from athenak_amd.main import Simulation
    from athenak_amd.parameter_input import ParameterInput
    text = dc.writer_deck(PDF_BLOCKS)
    sim = Simulation(ParameterInput(text=text))
    sim.Execute(max_cycles=2)
    pin = _turb_pin(text)
    with tempfile.TemporaryDirectory() as d:
        out = _write_twice(pin, sim, d)
        files = sorted(dc.files_of(d))
        assert files == ["OrszagTang.mhd.hst", "OrszagTang.user.hst",
                         "pdf_mhd_w_d/OrszagTang.00000.pdf", "pdf_mhd_w_d/OrszagTang.00001.pdf", "pdf_mhd_w_d/OrszagTang.bins.pdf",
                         "pdf_rho_mhd_j2/OrszagTang.00000.pdf", "pdf_rho_mhd_j2/OrszagTang.00001.pdf",
                         "pdf_rho_mhd_j2/OrszagTang.bins.pdf"]
        # bins, written once
        b = open(os.path.join(d, "pdf_mhd_w_d", "OrszagTang.bins.pdf")).read().split("\n")
        assert b[0] == "# pdf bins " and b[1] == "# [1]= dens " and len(b) == 4 and b[3] == ""
        edges, _ = S.pdf_bins(0.01, 100.0, 16, True)
        assert b[2] == "".join(" %12.5e" % e for e in edges)
        b = open(os.path.join(d, "pdf_rho_mhd_j2", "OrszagTang.bins.pdf")).read().split("\n")
        assert b[:3] == ["# pdf bins ", "# [1]= dens ", "# [2]= j2 "] and len(b) == 6
        assert len(b[3].split()) == 5 and len(b[4].split()) == 7
        # one histogram per file: "# time= ", rows of nbin+2 columns, a blank line
        p = open(os.path.join(d, "pdf_mhd_w_d", "OrszagTang.00001.pdf")).read().split("\n")
        assert p[0] == "# time= " + " %12.5e" % sim.pmesh.time and len(p[1].split()) == 18 and p[2:] == ["", ""]
        p = open(os.path.join(d, "pdf_rho_mhd_j2", "OrszagTang.00000.pdf")).read().split("\n")
        assert len(p) == 1 + 8 + 2 and all(len(r.split()) == 6 for r in p[1:9])
        # the numbers are those of the restatement on the same arrays
        bx, a = dc.pack_arrays(sim)
        vol = sc.cell_volumes(bx, a["dx"], len(a["w0"]))
        rho = sc.active(bx, a["w0"][:, 0])
        u_rho = sc.active(bx, sim.phys.u0.numpy()[:, 0])
        e1, s1 = S.pdf_bins(0.01, 100.0, 16, True)
        counts, wl, nan, _ = S.histogram(rho, vol*u_rho, e1, s1, True)
        po = [o for o in out.pout_list if o.out_params.file_type == "pdf" and o.pdf_dimension == 1][0]
        assert np.array_equal(po.counts, counts) and nan == 0 == po.nan_dropped
        sc.check_weights(po.result, wl, "mass-weighted density pdf")
        j2 = sc.active(bx, dc.restated("j2", bx, a))
        e1, s1 = S.pdf_bins(0.0, 2.0, 4, False)
        e2, s2 = S.pdf_bins(1e-3, 1e3, 6, True)
        counts, wl, nan, _ = S.histogram(rho, vol, e1, s1, False, j2, e2, s2, True)
        po = [o for o in out.pout_list if o.out_params.file_type == "pdf" and o.pdf_dimension == 2][0]
        assert po.counts.shape == (8, 6) and np.array_equal(po.counts, counts)
        sc.check_weights(po.result, wl, "density - j2 pdf")
        # counters advance, in the object and in the deck
        assert po.out_params.file_number == 2 and pin.GetInteger("output2", "file_number") == 2
        assert po.out_params.last_time == sim.pmesh.time          # dcycle: dt = 0, last_time stays at the first output's
        assert pin.GetReal("output2", "last_time") == pytest.approx(sim.pmesh.time, rel=1e-5)
        # user history: the header of history.cpp:426-445 with the eleven labels, 13 columns
        u = open(os.path.join(d, "OrszagTang.user.hst")).read().split("\n")
        assert u[0] == "# Athena++ history data"
        assert u[1] == "#  [1]=time      [2]=dt       " + "".join("[%d]=%.10s    " % (n + 3, l) for n, l in enumerate(S.LABELS))
        assert len(u) == 5 and all(len(r.split()) == 13 for r in u[2:4])
        terms = S.turb_terms(bx, a["w0"], a["bcc"], a["faces"], a["dx"])
        got = [float(x) for x in u[2].split()[2:]]
        for q in range(11):
            tot = float(np.sum(terms[q]))
            assert got[q] == pytest.approx(tot, rel=2e-5, abs=1e-5*float(np.abs(terms[q]).sum())), S.LABELS[q]
        m = open(os.path.join(d, "OrszagTang.mhd.hst")).read().split("\n")
        assert "[3]=mass" in m[1] and len(m[2].split()) == 13


def test_user_hist_only_writes_the_user_file_alone(cpu_backend_with_stats):
    from athenak_amd.main import Simulation
    from athenak_amd.parameter_input import ParameterInput
    text = dc.writer_deck("<output1>\nfile_type = hst\ndcycle = 1\nuser_hist_only = true\n")
    sim = Simulation(ParameterInput(text=text))
    with tempfile.TemporaryDirectory() as d:
        _write_twice(_turb_pin(text), sim, d)
        assert sorted(dc.files_of(d)) == ["OrszagTang.user.hst"]


def test_turbulence_deck_with_hst_and_no_user_hist_writes_the_ordinary_file(cpu_backend_with_stats):
    from athenak_amd.main import Simulation
    from athenak_amd.parameter_input import ParameterInput
    text = dc.writer_deck("<output1>\nfile_type = hst\ndcycle = 1\n")
    sim = Simulation(ParameterInput(text=text))
    with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2:
        _write_twice(_turb_pin(text, user_hist=False), sim, d1)
        _write_twice(ParameterInput(text=text), sim, d2)
        a, b = dc.files_of(d1), dc.files_of(d2)
        assert sorted(a) == ["OrszagTang.mhd.hst"] and a == b


def test_stats_deck_builds_its_outputs(monkeypatch):
    """inputs/turb_mhd_stats.athinput: host objects on CPU tensors, nothing is launched by building them"""
    monkeypatch.setattr(capi, "DEVICE", "cpu")
    from athenak_amd.main import load_deck
    from athenak_amd.mesh import Mesh
    pin = load_deck("turb_mhd_stats.athinput")
    pm = Mesh(pin)
    pm.AddCoordinatesAndPhysics(pin)
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        try:
            pout = outputs.Outputs(pin, pm)
            dirs = sorted(os.listdir(d))
        finally:
            os.chdir(here)
    kinds = sorted((o.out_params.file_type, getattr(o, "pdf_dimension", 0)) for o in pout.pout_list)
    assert kinds == [("hst", 0), ("pdf", 1), ("pdf", 2)]
    assert dirs == ["pdf_mhd_w_d", "pdf_mhd_w_d_mhd_j2"]
    h = [o for o in pout.pout_list if o.out_params.file_type == "hst"][0]
    assert h.user_hist and h.physics_hist
    p1 = [o for o in pout.pout_list if getattr(o, "pdf_dimension", 0) == 1][0]
    assert p1.out_params.mass_weighted and p1.out_params.logscale


# ---- refusals --------------------------------------------------------------------------------------------------
def _outputs_of(blocks, problem=None, fluid_mhd=True):
    from athenak_amd.main import Simulation
    from athenak_amd.parameter_input import ParameterInput
    import output_cases as oc
    text = dc.writer_deck(blocks) if fluid_mhd else (oc.SOD_DECK.replace("FUSED", "false").split("<output1>")[0] + blocks)
    pin = ParameterInput(text=text)
    sim = Simulation(pin, initialize=False)
    if problem is not None:
        head, tail = text.split("<problem>")
        tail = tail[tail.index("<output1>"):] if "<output1>" in tail else ""
        pin = ParameterInput(text=head + "<problem>\n" + problem + tail)
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        try:
            return outputs.Outputs(pin, sim.pmesh)
        finally:
            os.chdir(here)


PDF1 = "<output1>\nfile_type = pdf\ndcycle = 1\n"


@pytest.mark.parametrize("block,what", [
    (PDF1 + "variable = mhd_w_d\nbin_min = 0.0\nbin_max = 1.0\nnbin = 4\n", "logscale is true but bin_min <= 0.0"),
    (PDF1 + "variable = mhd_w_d\nbin_min = -1.0\nbin_max = 1.0\nnbin = 4\nlogscale = true\n", "logscale is true but bin_min <= 0.0"),
    (PDF1 + "variable = mhd_w_d\nbin_min = 1.0\nbin_max = 2.0\nnbin = 4\nvariable_2 = mhd_j2\nnbin2 = 3\nbin2_min = 0.0\n",
     "logscale2 is true but bin2_min <= 0.0"),
    (PDF1 + "variable = mhd_u\nbin_min = 1.0\nbin_max = 2.0\nnbin = 4\n",
     "PDF output block 'output1' cannot output variable 'mhd_u'. The variable must be a single variable not a variable group"),
    (PDF1 + "variable = mhd_w\nbin_min = 1.0\nbin_max = 2.0\nnbin = 4\n", "cannot output variable 'mhd_w'"),
    (PDF1 + "variable = mhd_w_d\nbin_min = 1.0\nbin_max = 2.0\nnbin = 4\nvariable_2 = mhd_j2\nnbin2 = 1\n", "nbin2 = 1 is not on this path"),
    (PDF1 + "variable = mhd_w_d\nbin_min = 1.0\nbin_max = 2.0\nnbin = 0\n", "nbin = 0"),
    (PDF1 + "variable = mhd_jcon\nbin_min = 1.0\nbin_max = 2.0\nnbin = 4\n", "mhd_jcon.*SaveMHDState"),
    (PDF1 + "variable = mhd_moments\nbin_min = 1.0\nbin_max = 2.0\nnbin = 4\n", "mhd_moments"),
    (PDF1 + "variable = mhd_bcc\nbin_min = 1.0\nbin_max = 2.0\nnbin = 4\n", "single variable"),
    ("<output1>\nfile_type = hst\ndcycle = 1\nuser_hist_only = true\n",
     "User-history file requested in output block 'output1', but <problem>/user_hist is not true"),
    ("<output1>\nfile_type = vtk\nvariable = mhd_w\ndcycle = 1\n", "Unrecognized or unsupported file format = 'vtk'"),
])
def test_refused_output_blocks(block, what, cpu_backend_with_stats):
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*" + what):
        _outputs_of(block)


def test_hydro_group_variables_and_user_hist_refusals(cpu_backend_with_stats):
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*cannot output variable 'hydro_u'"):
        _outputs_of(PDF1 + "variable = hydro_u\nbin_min = 1.0\nbin_max = 2.0\nnbin = 4\n", fluid_mhd=False)
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*cannot output variable 'hydro_w'"):
        _outputs_of(PDF1 + "variable = hydro_w\nbin_min = 1.0\nbin_max = 2.0\nnbin = 4\n", fluid_mhd=False)
    # user_hist on a hydro turbulence run, and with another problem generator
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*user_hist = true with pgen_name = turb needs an MHD run"):
        _outputs_of("<output1>\nfile_type = hst\ndcycle = 1\n", problem="pgen_name = turb\nuser_hist = true\n", fluid_mhd=False)
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*user history function of pgen_name = 'orszag_tang' is not enrolled"):
        _outputs_of("<output1>\nfile_type = hst\ndcycle = 1\n", problem="pgen_name = orszag_tang\nuser_hist = true\n")
    # ... also without an hst block
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*not enrolled"):
        _outputs_of("", problem="pgen_name = orszag_tang\nuser_hist = true\n")


def test_backend_without_the_entries_says_so():
    import cpu_backend
    cpu_backend.install()
    try:
        with tempfile.TemporaryDirectory() as d:
            with pytest.raises(RuntimeError, match="### FATAL ERROR.*akmi_pdf"):
                dc.run_and_write(dc.writer_deck(PDF1 + "variable = mhd_w_d\nbin_min = 0.1\nbin_max = 2.0\nnbin = 4\n"), d, cycles=0)
    finally:
        cpu_backend.uninstall()
