"""not gpu: derived output variables on the host.

  * the arithmetic of the kernel (athenak_amd/csrc/akmi_derived.hpp, compiled for the CPU by tests/host_shim/) against
    the numpy restatement of tests/derived_restate.py, bit for bit, on random states: 1-D, 2-D, 3-D, one block and eight
    blocks of 24 x 12 x 10, two and four ghost cells; everything outside the reference's loop range is +0;
  * second-order convergence on an analytic field, |B| to one ulp of the square root;
  * names, labels, scalar groups and refusals of outputs.py; tab and bin files with the new variables through the
    product's host logic on CPU tensors; a deck without scalars writes the files of the stored-array path as it was.
The restatement's docstring says which expression fixes the order of every sum."""
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
import derived_restate as R  # noqa: E402
from athenak_amd import capi, outputs  # noqa: E402

KEYS = ["temperature", "wz", "w2", "jz", "j2", "curv", "k_jxb", "curv_perp", "bmag", "divb"]


@pytest.fixture(scope="module")
def shim():
    return dc.build_shim()


@pytest.fixture
def cpu_backend_with_derived():
    dc.install_cpu_backend()
    yield
    dc.uninstall_cpu_backend()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def shim_eval(shim, key, bx, nx, ng, a):
    nmb = len(a["w0"])
    pk = dc.pack_struct(nmb, a["w0"].shape[1], nx, ng, a["dx"])
    out = np.full((nmb, bx.N3, bx.N2, bx.N1), 7.0)
    rc = shim.hd_derived_var(C.byref(pk), capi.DERIVED[key], _ptr(a["w0"]), None, _ptr(a["bcc"]),
                             *[_ptr(f) for f in a["faces"]], _ptr(out), 1)
    assert rc == 0
    return out


def random_state(nmb, nx, ng, seed):
    rng = np.random.default_rng(seed)
    bx = R.Box(nx[0], nx[1], nx[2], ng)
    sh = (bx.N3, bx.N2, bx.N1)
    w0 = rng.uniform(-1.0, 1.0, (nmb, 5) + sh)
    w0[:, 0] = 0.5 + rng.uniform(0, 1, (nmb,) + sh)
    w0[:, 4] = 0.5 + rng.uniform(0, 1, (nmb,) + sh)
    bcc = rng.uniform(-1.0, 1.0, (nmb, 3) + sh)
    faces = (rng.uniform(-1, 1, (nmb, bx.N3, bx.N2, bx.N1 + 1)), rng.uniform(-1, 1, (nmb, bx.N3, bx.N2 + 1, bx.N1)),
             rng.uniform(-1, 1, (nmb, bx.N3 + 1, bx.N2, bx.N1)))
    # cell sizes that are not powers of two and differ between blocks (as on a refined mesh)
    dx = np.array([[1.0/24/(1 + m % 2), 0.7/12/(1 + m % 2), 1.3/10/(1 + m % 2)] for m in range(nmb)])
    return bx, dict(w0=w0, bcc=bcc, faces=faces, dx=dx)


SHAPES = [((24, 1, 1), 1), ((24, 12, 1), 1), ((24, 12, 10), 1), ((24, 12, 10), 8), ((24, 12, 1), 8), ((24, 1, 1), 8)]


@pytest.mark.parametrize("ng", [2, 4])
@pytest.mark.parametrize("nx,nmb", SHAPES)
def test_kernel_arithmetic_is_the_restatement_bit_for_bit(shim, nx, nmb, ng):
    bx, a = random_state(nmb, nx, ng, seed=nx[1]*100 + nx[2]*10 + ng + nmb)
    for key in KEYS:
        got = shim_eval(shim, key, bx, nx, ng, a)
        dc.assert_bits(got, dc.restated(key, bx, a), "%s %s nmb=%d ng=%d" % (key, nx, nmb, ng))
        dc.outside_is_fill(got, bx, key)


def test_unknown_variable_and_component_count(shim):
    assert shim.hd_derived_ncomp(10) == -1 and shim.hd_derived_ncomp(-1) == -1
    assert [shim.hd_derived_ncomp(capi.DERIVED[k]) for k in KEYS] == [1]*10
    assert sorted(capi.DERIVED.values()) == list(range(10))


# ---- independent check: an analytic field with known curl -------------------------------------------------------
def _analytic(n, ng=2):
    """B = v = (-sin y, sin x, 0) on [0, 2 pi)^3, cell centres, ghost cells filled from the formula"""
    bx = R.Box(n, n, n, ng)
    h = 2.0*np.pi/n
    c = (np.arange(-ng, n + ng) + 0.5)*h
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    vec = np.stack([-np.sin(y), np.sin(x), np.zeros_like(x)])[None]
    w0 = np.concatenate([np.ones_like(vec[:, :1]), vec, np.ones_like(vec[:, :1])], axis=1)
    faces = tuple(np.zeros(s) for s in ((1, bx.N3, bx.N2, bx.N1 + 1), (1, bx.N3, bx.N2 + 1, bx.N1), (1, bx.N3 + 1, bx.N2, bx.N1)))
    a = dict(w0=np.ascontiguousarray(w0), bcc=np.ascontiguousarray(vec), faces=faces, dx=np.array([[h, h, h]]))
    curlz = bx.act(np.cos(x) + np.cos(y))
    return bx, a, curlz


def analytic_errors(evaluate):
    """max errors of jz, j2, wz, w2 at 32^3 and 64^3 for an evaluator (key, bx, n, a) -> array"""
    errs = {}
    for n in (32, 64):
        bx, a, cz = _analytic(n)
        for key in ("jz", "j2", "wz", "w2"):
            got = bx.act(evaluate(key, bx, n, a))[0]
            want = cz if key in ("jz", "wz") else cz*cz
            errs[key, n] = np.abs(got - want).max()
    return errs


def test_second_order_convergence_on_an_analytic_field(shim):
    """curl of (-sin y, sin x, 0) is (0, 0, cos x + cos y); centred differences give sin(h)/h times it, an error of
    h^2/6: the ratio between 32^3 and 64^3 is 4 (3.5 ... 4.5 asked)"""
    errs = analytic_errors(lambda key, bx, n, a: shim_eval(shim, key, bx, (n, n, n), 2, a))
    for key in ("jz", "j2", "wz", "w2"):
        ratio = errs[key, 32]/errs[key, 64]
        assert 3.5 <= ratio <= 4.5, (key, ratio, errs[key, 32], errs[key, 64])


def test_bmag_to_one_ulp(shim):
    """|B| against the square root of the exact sum of squares (Python fractions): one ulp of the sqrt"""
    from fractions import Fraction
    import math
    bx, a = random_state(1, (8, 6, 4), 2, seed=5)
    got = bx.act(shim_eval(shim, "bmag", bx, (8, 6, 4), 2, a))[0].ravel()
    B = [bx.act(a["bcc"][:, n])[0].ravel() for n in range(3)]
    for q in range(0, got.size, 7):
        s = sum(Fraction(float(B[n][q]))**2 for n in range(3))
        # exact value of sqrt(s) lies between the neighbours of the correctly rounded one
        g = float(got[q])
        lo, hi = Fraction(np.nextafter(g, 0.0)), Fraction(np.nextafter(g, math.inf))
        assert lo*lo <= s <= hi*hi, q


# ---- names, labels, refusals ------------------------------------------------------------------------------------
def test_names_and_labels():
    for name, key in dc.MHD_NAMES.items():
        assert outputs._outvars(name, True) == [(dc.LABELS[key], 0, "dv:%d" % capi.DERIVED[key])]
    for name, key in dc.HYDRO_NAMES.items():
        assert outputs._outvars(name, False) == [(dc.LABELS[key], 0, "dv:%d" % capi.DERIVED[key])]
    for name in dc.MHD_NAMES:
        with pytest.raises(RuntimeError, match="### FATAL ERROR.*" + name):
            outputs._outvars(name, False)                 # an MHD variable of a hydro run


def test_scalar_groups_and_labels():
    u = [l for l, _, _ in outputs._outvars("hydro_u", False, True, False, 2)]
    assert u == ["dens", "mom1", "mom2", "mom3", "ener", "r_00", "r_01"]
    assert outputs._outvars("hydro_w_s", False, True, False, 2) == [("s_00", 5, "w0"), ("s_01", 6, "w0")]
    assert outputs._outvars("mhd_u_s", True, False, False, 1) == [("r_00", 4, "u0")]            # isothermal: four fluid variables
    wb = [l for l, _, _ in outputs._outvars("mhd_w_bcc", True, True, False, 2)]
    assert wb == ["dens", "velx", "vely", "velz", "eint", "s_00", "s_01", "bcc1", "bcc2", "bcc3"]
    assert outputs._outvars("hydro_u_s", False) == []
    for name in ("hydro_u", "hydro_w", "hydro_u_d", "hydro_w_e"):
        assert outputs._outvars(name, False) == dc.parent_outvars(name, False)
    for name in ("mhd_u", "mhd_w", "mhd_bcc", "mhd_u_bcc", "mhd_w_bcc", "mhd_bcc3", "mhd_w_vx"):
        assert outputs._outvars(name, True) == dc.parent_outvars(name, True)


@pytest.mark.parametrize("name", dc.REFUSED + ["mhd_t"])
def test_refused_names_stop_both_hosts(name):
    """the output blocks of the Python host and the name table NativeSimulation.derived goes through"""
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*'%s'" % name):
        outputs._outvars(name, True)
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*'%s'" % name):
        outputs.derived_which(name, True)


def test_temperature_needs_the_energy_variable():
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*temperature.*derived_variables.cpp:98"):
        outputs.derived_which("temperature", True, is_ideal=False)
    assert outputs.derived_which("temperature", False, True) == (0, 1, "temperature")
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*mhd_j2"):
        outputs.derived_which("mhd_j2", False)


def test_output_block_with_a_refused_name_stops_the_run(cpu_backend_with_derived):
    from athenak_amd.main import Simulation
    from athenak_amd.parameter_input import ParameterInput
    pin = ParameterInput(text=dc.writer_deck("<output1>\nfile_type = bin\nvariable = mhd_jcon\ndcycle = 1\n"))
    sim = Simulation(pin, initialize=False)
    with pytest.raises(RuntimeError, match="### FATAL ERROR.*mhd_jcon.*SaveMHDState"):
        outputs.Outputs(pin, sim.pmesh)


# ---- through the writers, on CPU tensors -------------------------------------------------------------------------
def test_tab_and_bin_files_with_derived_variables(cpu_backend_with_derived):
    with tempfile.TemporaryDirectory() as d:
        sim = dc.run_and_write(dc.writer_deck(dc.WRITER_OUTPUTS), d)
        arr = dc.check_writer_files(sim, d)
        # and the arrays behind the files are the restatement's
        bx, a = dc.pack_arrays(sim)
        for name in arr:
            dc.assert_bits(arr[name], dc.restated(dc.MHD_NAMES[name], bx, a), name)


def test_backend_without_the_entry_says_so():
    """the plain oracle stand-in has no derived-variable entry: the output stops with a message, nothing is made up"""
    import cpu_backend
    cpu_backend.install()
    try:
        with tempfile.TemporaryDirectory() as d:
            with pytest.raises(RuntimeError, match="### FATAL ERROR.*akmi_derived_var"):
                dc.run_and_write(dc.writer_deck("<output1>\nfile_type = bin\nvariable = mhd_j2\ndcycle = 1\n"), d, cycles=0)
    finally:
        cpu_backend.uninstall()


def test_files_without_scalars_are_those_of_the_stored_array_path(cpu_backend_with_derived, monkeypatch):
    """every stored-array group of a deck with nscalars = 0, written with the variable table as it was before the derived
    variables and with the present one: the same bytes"""
    with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2:
        dc.run_and_write(dc.writer_deck(dc.STORED_OUTPUTS), d1)
        monkeypatch.setattr(outputs, "_outvars", dc.parent_outvars)
        dc.run_and_write(dc.writer_deck(dc.STORED_OUTPUTS), d2)
        a, b = dc.files_of(d1), dc.files_of(d2)
        assert sorted(a) == sorted(b) and len(a) == 6
        for k in a:
            assert a[k] == b[k], k


def test_scalar_columns_are_written(cpu_backend_with_derived):
    import output_cases as oc
    text = oc.SOD_DECK.replace("FUSED", "false")
    text = text[:text.index("<output1>")].replace("gamma = 1.4\n", "gamma = 1.4\nnscalars = 2\n")
    text += ("<output1>\nfile_type = tab\nvariable = hydro_w\ndata_format = %24.16e\ndcycle = 1\n"
             "<output2>\nfile_type = bin\nvariable = hydro_u_s\ndcycle = 1\n<output3>\nfile_type = bin\nvariable = hydro_u\ndcycle = 1\n")
    with tempfile.TemporaryDirectory() as d:
        sim = dc.run_and_write(text, d, cycles=2)
        head, rows = dc.read_tab(os.path.join(d, "tab", "Sod.hydro_w.00000.tab"))
        assert head[-7:] == ["dens", "velx", "vely", "velz", "eint", "s_00", "s_01"]
        w = sim.phys.w0.numpy()
        ng = sim.pmesh.mb_indcs.ng
        for r in rows:
            m, i = int(r[0]), int(r[1])
            assert [float(x) for x in r[3:]] == [float(w[m, n, 0, 0, i]) for n in range(7)]
        assert len(rows) == 64 and ng == 2
        names, blocks = dc.read_bin(os.path.join(d, "bin", "Sod.hydro_u_s.00000.bin"))
        assert names == ["r_00", "r_01"]
        u = sim.phys.u0.numpy()
        for m, (h, data) in enumerate(blocks):
            assert np.array_equal(data[:, 0, 0], u[m, 5:7, 0, 0, ng:-ng].astype(np.float32))
        names, _ = dc.read_bin(os.path.join(d, "bin", "Sod.hydro_u.00000.bin"))
        assert names == ["dens", "mom1", "mom2", "mom3", "ener", "r_00", "r_01"]


def test_diagnostics_deck_builds_its_outputs(monkeypatch):
    """inputs/turb_mhd_diag.athinput: a driven box with the four diagnostics as outputs (host objects on CPU tensors:
    nothing is launched by building them)"""
    monkeypatch.setattr(capi, "DEVICE", "cpu")
    from athenak_amd.main import load_deck
    from athenak_amd.mesh import Mesh
    pin = load_deck("turb_mhd_diag.athinput")
    assert pin.DoesBlockExist("turb_driving")
    pm = Mesh(pin)
    pm.AddCoordinatesAndPhysics(pin)
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        try:
            pout = outputs.Outputs(pin, pm)
        finally:
            os.chdir(here)
    got = sorted((o.out_params.file_type, o.out_params.variable, o.outvars[0][0]) for o in pout.pout_list)
    assert got == [("bin", "mhd_curv", "curv"), ("bin", "mhd_divb", "divb"), ("bin", "mhd_j2", "j2"),
                   ("bin", "mhd_wz", "vorz"), ("tab", "mhd_j2", "j2")]
