"""Shared by tests/test_derived_host.py (no GPU) and tests/test_gpu_derived.py: the CPU build of the derived-variable
arithmetic (tests/host_shim/derived_host.cpp), a CPU backend that adds it to the oracle-as-akmi stand-in, the arrays of
a pack as numpy, and the checks of the writers that both suites run (on CPU tensors / through the HIP entry)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import derived_restate as R  # noqa: E402

SHIM = os.path.join(ROOT, "tests", "host_shim")
SO = os.path.join(SHIM, "libderived_host.so")

# output name -> key of athenak_amd.capi.DERIVED, for the names of the issue's table
MHD_NAMES = {"mhd_wz": "wz", "mhd_w2": "w2", "mhd_jz": "jz", "mhd_j2": "j2", "mhd_curv": "curv", "mhd_k_jxb": "k_jxb",
             "mhd_curv_perp": "curv_perp", "mhd_bmag": "bmag", "mhd_divb": "divb"}
HYDRO_NAMES = {"hydro_wz": "wz", "hydro_w2": "w2"}
LABELS = {"wz": "vorz", "w2": "vor2", "jz": "jz", "j2": "j2", "curv": "curv", "k_jxb": "k_jxb",
          "curv_perp": "curv_perp", "bmag": "bmag", "divb": "divb"}
REFUSED = ["mhd_jcon", "hydro_sgs", "mhd_sgs", "mhd_dynamo_ks", "mhd_curv_alt", "hydro_moments", "mhd_moments",
           "rad_coord", "rad_hydro_u", "prtcl_all", "prtcl_d"]


def build_shim():
    src = os.path.join(SHIM, "derived_host.cpp")
    hdr = os.path.join(ROOT, "athenak_amd", "csrc", "akmi_derived.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        # -ffp-contract=off: products and sums rounded separately, as in the device build
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", SHIM, "-I",
                               os.path.join(ROOT, "athenak_amd", "csrc"), src, "-o", SO])
    return C.CDLL(SO)


def install_cpu_backend():
    """tests/cpu_backend.py plus akmi_derived_var / akmi_derived_ncomp from the CPU build of akmi_derived.hpp"""
    import cpu_backend
    from athenak_amd import capi
    H = build_shim()

    class Backend(cpu_backend.OracleAsAkmi):
        def akmi_derived_var(self, *args):
            return H.hd_derived_var(*args[:-1])          # last argument is the HIP stream

        def akmi_derived_ncomp(self, which):
            return H.hd_derived_ncomp(which)

    capi._LIB = Backend()
    capi.DEVICE = "cpu"


def uninstall_cpu_backend():
    import cpu_backend
    cpu_backend.uninstall()


def _np(t):
    return t.detach().cpu().numpy()


def pack_arrays(sim):
    """(Box, dict of the numpy arrays the restatement takes) of a Simulation / NativeSimulation"""
    ph, ind = sim.phys, sim.pmesh.mb_indcs
    bx = R.Box(ind.nx1, ind.nx2, ind.nx3, ind.ng)
    a = {"w0": _np(ph.w0), "dx": np.asarray(sim.pmesh.pmb_pack.pmb.dx, dtype=np.float64)[:len(ph.w0)]}
    if hasattr(ph, "bcc0"):
        a["bcc"] = _np(ph.bcc0)
        a["faces"] = (_np(ph.b0.x1f), _np(ph.b0.x2f), _np(ph.b0.x3f))
    return bx, a


def restated(key, bx, a):
    return R.restate(key, bx, a.get("w0"), a.get("bcc"), a.get("faces"), a["dx"])


def assert_bits(got, want, what):
    """bit identity of two float64 arrays (NaNs included: the bit patterns are compared)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    # +0 and -0 differ in bits and are kept apart on purpose: a reordered sum shows up there first
    assert not bad.any(), "%s: %d of %d values differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def outside_is_fill(got, bx, key):
    """everything outside the reference's loop range holds the fill of a freshly allocated array: +0"""
    if key == "divb":
        return          # the loop covers the whole array
    mask = np.ones(got.shape, dtype=bool)
    bx.act(mask)[...] = False
    assert np.all(got.view(np.uint64)[mask] == 0), key


# ---- the writers ------------------------------------------------------------------------------------------------
WRITER_OUTPUTS = """
<output1>
file_type = tab
variable = mhd_j2
data_format = %24.16e
dcycle = 1
slice_x2 = 0.1
slice_x3 = -0.2
<output2>
file_type = tab
variable = mhd_divb
id = divb_gz
data_format = %24.16e
dcycle = 1
ghost_zones = true
slice_x2 = 0.1
slice_x3 = -0.2
<output3>
file_type = bin
variable = mhd_curv
dcycle = 1
<output4>
file_type = bin
variable = mhd_divb
id = divb_gz
ghost_zones = true
dcycle = 1
<output5>
file_type = bin
variable = mhd_wz
slice_x3 = -0.2
dcycle = 1
<output6>
file_type = bin
variable = mhd_bmag
id = bmag_gz
ghost_zones = true
dcycle = 1
"""


def writer_deck(extra=""):
    import output_cases as oc
    text = oc.OT_DECK.replace("FUSED", "false")
    return text[:text.index("<output1>")] + extra


def run_and_write(deck_text, workdir, cycles=2):
    """Simulation of the deck advanced `cycles` cycles, then every <output> block written once into workdir"""
    from athenak_amd.main import Simulation
    from athenak_amd.outputs import Outputs
    from athenak_amd.parameter_input import ParameterInput
    pin = ParameterInput(text=deck_text)
    sim = Simulation(pin)
    sim.Execute(max_cycles=cycles)
    here = os.getcwd()
    os.makedirs(workdir, exist_ok=True)
    os.chdir(workdir)
    try:
        Outputs(pin, sim.pmesh).MakeOutputs(sim.pmesh, pin)
    finally:
        os.chdir(here)
    return sim


def read_bin(path):
    """(variable names, [(10-int header, float32 array [nvar][k][j][i])]) of a version-1.1 bin file, split with the
    readers of tests/test_outputs_formats.py"""
    from test_outputs_formats import _bin_block_headers, _bin_parts
    pre, _, payload = _bin_parts(path)
    names = pre.split(b"variables:")[1].split()
    hdrs = _bin_block_headers(path)
    out, pos = [], 0
    for h in hdrs:
        n = (h[5] - h[4] + 1, h[3] - h[2] + 1, h[1] - h[0] + 1)
        cnt = len(names)*n[0]*n[1]*n[2]
        pos += 40 + 48
        out.append((h, np.frombuffer(payload, dtype="<f4", count=cnt, offset=pos).reshape((len(names),) + n)))
        pos += 4*cnt
    assert pos == len(payload)
    return [x.decode() for x in names], out


def read_tab(path):
    """(labels after the coordinate columns, rows as lists of strings)"""
    lines = open(path).read().split("\n")
    head = lines[1].split()
    rows = [l.split() for l in lines[2:] if l.strip()]
    return head, rows


def check_writer_files(sim, workdir):
    """tab and bin files of WRITER_OUTPUTS against the entry's arrays: labels, index ranges, values"""
    ind = sim.pmesh.mb_indcs
    ng = ind.ng
    arr = {n: _np(sim.derived(n))[:, 0] for n in ("mhd_j2", "mhd_divb", "mhd_curv", "mhd_wz", "mhd_bmag")}
    size = sim.pmesh.pmb_pack.pmb.mb_size
    nmb = len(arr["mhd_j2"])
    # slice indices as CellCenterIndex gives them, restated: int((x - xmin)/(xmax - xmin)*n) + ng
    def sl(x, lo, hi, n):
        return int(((x - lo)/(hi - lo))*float(n)) + ng
    base = os.path.join(workdir, "tab", "OrszagTang.%s.00000.tab")
    for fid, name, gz in (("mhd_j2", "mhd_j2", False), ("divb_gz", "mhd_divb", True)):
        head, rows = read_tab(base % fid)
        assert head[-1] == LABELS[MHD_NAMES[name]] and head[1:5] == ["gid", "i", "x1v", LABELS[MHD_NAMES[name]]]
        want = []
        for m in range(nmb):
            s = size[m]
            if not (s.x2min <= 0.1 < s.x2max and s.x3min <= -0.2 < s.x3max):
                continue
            j, k = sl(0.1, s.x2min, s.x2max, ind.nx2), sl(-0.2, s.x3min, s.x3max, ind.nx3)
            irange = range(0, ind.nx1 + 2*ng) if gz else range(ng, ng + ind.nx1)
            want += [(m, i, arr[name][m, k, j, i]) for i in irange]
        assert len(rows) == len(want) and len(want) > 0
        for r, (m, i, v) in zip(rows, want):
            assert int(r[0]) == m and int(r[1]) == i
            assert np.float64(r[3]).view(np.uint64) == np.float64(v).view(np.uint64) or (v == 0.0 and float(r[3]) == 0.0), \
                (name, m, i, r[3], v)         # %24.16e round-trips a double exactly (the sign of a zero aside)
    binf = os.path.join(workdir, "bin", "OrszagTang.%s.00000.bin")
    for fid, name, gz, zslice in (("mhd_curv", "mhd_curv", False, False), ("divb_gz", "mhd_divb", True, False),
                                  ("mhd_wz", "mhd_wz", False, True), ("bmag_gz", "mhd_bmag", True, False)):
        names, blocks = read_bin(binf % fid)
        assert names == [LABELS[MHD_NAMES[name]]]
        assert len(blocks) == nmb
        for m, (h, data) in enumerate(blocks):
            s = size[m]
            lo = (0, 0, 0) if gz else (ng, ng, ng)
            n = (ind.nx3 + 2*ng, ind.nx2 + 2*ng, ind.nx1 + 2*ng) if gz else (ind.nx3, ind.nx2, ind.nx1)
            ks, ke = lo[0], lo[0] + n[0] - 1
            if zslice:
                ks = ke = sl(-0.2, s.x3min, s.x3max, ind.nx3)
            assert tuple(h[:6]) == (lo[2], lo[2] + n[2] - 1, lo[1], lo[1] + n[1] - 1, ks, ke)
            want = arr[name][m, ks:ke + 1, lo[1]:lo[1] + n[1], lo[2]:lo[2] + n[2]].astype(np.float32)
            assert np.array_equal(data[0].view(np.uint32), want.view(np.uint32)), (name, m)
    # the ghost cells of a variable the stencil cannot reach there are written as the fill, +0
    _, blocks = read_bin(binf % "bmag_gz")
    assert np.all(blocks[0][1][0, :ng] == 0.0) and np.any(blocks[0][1][0, ng:-ng, ng:-ng, ng:-ng] != 0.0)
    return arr


def parent_outvars(variable, is_mhd, is_ideal=True, turb=False, nscalars=0):
    """the variable table of the stored-array path as it was before the derived variables (no scalars, no derived
    names): what writes the files a deck with nscalars = 0 has to keep byte for byte"""
    blk = "mhd" if is_mhd else "hydro"
    u = [("dens", 0, "u0"), ("mom1", 1, "u0"), ("mom2", 2, "u0"), ("mom3", 3, "u0"), ("ener", 4, "u0")]
    w = [("dens", 0, "w0"), ("velx", 1, "w0"), ("vely", 2, "w0"), ("velz", 3, "w0"), ("eint", 4, "w0")]
    if not is_ideal:
        u, w = u[:4], w[:4]
    b = [("bcc1", 0, "bcc0"), ("bcc2", 1, "bcc0"), ("bcc3", 2, "bcc0")]
    table = {blk + "_u": u, blk + "_w": w}
    for sfx, v in zip(("d", "m1", "m2", "m3", "e"), u):
        table["%s_u_%s" % (blk, sfx)] = [v]
    for sfx, v in zip(("d", "vx", "vy", "vz", "e"), w):
        table["%s_w_%s" % (blk, sfx)] = [v]
    if is_mhd:
        table.update({"mhd_bcc": b, "mhd_u_bcc": u + b, "mhd_w_bcc": w + b, "mhd_bcc1": b[0:1], "mhd_bcc2": b[1:2],
                      "mhd_bcc3": b[2:3]})
    return table[variable]


STORED_OUTPUTS = "".join(
    "<output%d>\nfile_type = %s\nvariable = %s\ndcycle = 1\n%s" % (n + 1, ft, var, more)
    for n, (ft, var, more) in enumerate([
        ("bin", "mhd_w_bcc", ""), ("bin", "mhd_u", "ghost_zones = true\nid = u_gz\n"),
        ("tab", "mhd_w", "slice_x2 = 0.1\nslice_x3 = -0.2\n"), ("tab", "mhd_u_bcc", "slice_x1 = 0.1\nslice_x3 = -0.2\nid = ub\n"),
        ("bin", "mhd_bcc2", "slice_x3 = -0.2\n"), ("tab", "mhd_w_e", "slice_x2 = 0.1\nslice_x3 = -0.2\nghost_zones = true\n")]))


def files_of(workdir):
    out = {}
    for root, _, files in os.walk(workdir):
        for fn in files:
            out[os.path.relpath(os.path.join(root, fn), workdir)] = open(os.path.join(root, fn), "rb").read()
    return out


def pack_struct(nmb, nvar, nx, ng, dx):
    """capi.Pack of an ideal-gas pack over host arrays (dx: (nmb, 3) float64, kept alive by the caller)"""
    from athenak_amd import capi
    return capi.Pack(nmb, nvar, nx[0], nx[1], nx[2], ng, dx.ctypes.data, 5.0/3.0, 1e-37, 1e-37, 1e-37, 1e-37, 1e37, 1.0, 1)
