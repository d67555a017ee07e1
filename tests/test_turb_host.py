"""<turb_driving> on the host, no GPU: the random generator and the amplitude table of csrc/akmi_turb.hip against the
independent restatement of tests/turb_restate.py, bit for bit; incompressibility of every drawn mode; the deck errors
of both hosts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import turb_restate as R  # noqa: E402
from athenak_amd import capi  # noqa: E402


def _lib():
    return capi.lib()


def _state(idum=-1):
    st = capi.RngState()
    st.idum = idum
    return st


def test_rng_state_is_296_bytes():
    assert C.sizeof(capi.RngState) == 296
    assert _lib().akmi_rng_state_bytes() == 296


def test_uniform_deviates_bitwise():
    L, st, ref = _lib(), _state(), R.Ran2(-1)
    got = np.array([L.akmi_rng_uniform(C.byref(st)) for _ in range(10000)])
    want = np.array([ref.uniform() for _ in range(10000)])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert 0.0 < got.min() and got.max() < 1.0
    assert (st.idum, st.idum2, st.iy) == (ref.idum, ref.idum2, ref.iy) and list(st.iv) == ref.iv


def test_gaussian_deviates_bitwise():
    L, st, ref = _lib(), _state(), R.Ran2(-1)
    got = np.array([L.akmi_rng_gaussian(C.byref(st)) for _ in range(10000)])
    want = np.array([ref.gaussian() for _ in range(10000)])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert abs(got.mean()) < 0.05 and abs(got.std() - 1.0) < 0.05


def test_saved_state_continues_between_the_two_deviates_of_a_pair():
    L, st = _lib(), _state()
    for _ in range(7):                                    # odd: the second deviate of a pair is cached now
        L.akmi_rng_gaussian(C.byref(st))
    assert st.iset == 1
    saved = bytes(st)                                     # what a restart file holds
    straight = [L.akmi_rng_gaussian(C.byref(st)) for _ in range(5)]
    st2 = capi.RngState.from_buffer_copy(saved)
    again = [L.akmi_rng_gaussian(C.byref(st2)) for _ in range(5)]
    assert straight == again


@pytest.mark.parametrize("nlow,nhigh,dtype,count", [(1, 2, 0, 10), (1, 3, 0, 0), (0, 1, 0, 3), (1, 2, 1, 10),
                                                    (2, 4, 0, 0), (1, 1, 0, 3)])
def test_mode_counts(nlow, nhigh, dtype, count):
    want = len(R.mode_list(nlow, nhigh, dtype))
    if count:
        assert want == count
    assert _lib().akmi_turb_mode_count(nlow, nhigh, dtype) == want


def test_bad_driving_type_is_an_error():
    L = _lib()
    assert L.akmi_turb_mode_count(1, 2, 2) == capi.FAIL
    assert b"driving_type" in L.akmi_last_error()


@pytest.mark.parametrize("nlow,nhigh,dtype,lens", [(1, 2, 0, (1.0, 1.0, 1.0)), (1, 3, 0, (2.0, 1.0, 0.5)),
                                                   (1, 2, 1, (1.0, 1.0, 1.0)), (1, 3, 1, (1.0, 2.0, 3.0)),
                                                   (0, 2, 0, (1.0, 1.0, 1.0))])
def test_amplitudes_bitwise_and_divergence_free(nlow, nhigh, dtype, lens):
    L = _lib()
    st, ref = _state(), R.Ran2(-1)
    expo, exp_prp, exp_prl = 5.0/3.0, 5.0/3.0, 0.5
    n = L.akmi_turb_mode_count(nlow, nhigh, dtype)
    for draw in range(3):                                 # three cycles: the generator carries on
        kvec, amp = np.zeros((n, 3)), np.zeros((n, 24))
        got = L.akmi_turb_amplitudes(nlow, nhigh, dtype, C.c_double(expo), C.c_double(exp_prp), C.c_double(exp_prl),
                                     C.c_double(lens[0]), C.c_double(lens[1]), C.c_double(lens[2]), C.byref(st),
                                     kvec.ctypes.data_as(C.c_void_p), amp.ctypes.data_as(C.c_void_p))
        assert got == n
        kw, aw = R.amplitudes(ref, nlow, nhigh, dtype, expo, exp_prp, exp_prl, lens)
        assert np.array_equal(kvec.view(np.uint64), kw.view(np.uint64))
        assert np.array_equal(amp.view(np.uint64), aw.view(np.uint64)), draw
        assert np.count_nonzero(amp) > 0
        # k . A = 0 on every sin/cos combination of every mode (turb_driver.cpp:443-451,473-477,532-540)
        div, scale = R.divergence_coefficients(kvec, amp)
        assert np.all(np.abs(div) <= 1e-12*np.maximum(scale, 1e-300)[:, None]), np.abs(div).max()


def test_tables_match_the_restatement():
    L = _lib()
    kvec = np.array(R.amplitudes(R.Ran2(-1), 1, 2, 0, 5.0/3.0, 5.0/3.0, 0.0, (1.0, 1.0, 1.0))[0])
    nmb, nx = 2, (8, 4, 1)
    bounds = np.array([[-0.5, 0.0, -0.5, 0.5, -0.5, 0.5], [0.0, 0.5, -0.5, 0.5, -0.5, 0.5]])
    t = [np.zeros((nmb, len(kvec), nx[d])) for d in (0, 0, 1, 1, 2, 2)]
    assert L.akmi_turb_tables(nmb, len(kvec), *nx, kvec.ctypes.data_as(C.c_void_p), bounds.ctypes.data_as(C.c_void_p),
                              *[a.ctypes.data_as(C.c_void_p) for a in t]) == 0
    want = R.tables(kvec, bounds, nx)
    for d in range(3):
        assert np.array_equal(t[2*d], want[d][0]) and np.array_equal(t[2*d + 1], want[d][1])
    assert np.all(t[4] == 0.0) and np.all(t[5] == 1.0)     # collapsed x3: sin 0, cos 1


def test_scale_factor_solves_the_energy_equation():
    from athenak_amd.turb_driver import scale_factor
    t0, t1, dedt, dt, gnx = 3.7e3, 12.5, 0.1, 1e-3, (16, 16, 16)
    s = scale_factor(t0, t1, dedt, dt, gnx)
    dvol = 1.0/(16*16*16)
    m0, m1 = 0.5*t0*dvol*dt, t1*dvol
    assert abs(m0*s*s + m1*s - dedt) <= 1e-12*dedt


# ---- deck errors ---------------------------------------------------------------------
def _deck(extra):
    """the hydro turbulence deck with the blocks / parameters of `extra` ("block/name=value") added"""
    from athenak_amd.parameter_input import ParameterInput
    text = open(os.path.join(ROOT, "athenak_amd", "inputs", "turb_hydro.athinput")).read()
    text = text[:text.index("<output1>")]
    for e in extra:
        blk, rest = e.split("/", 1)
        text += "\n<%s>\n%s\n" % (blk, rest)
    return ParameterInput(text=text)


@pytest.mark.parametrize("extra,what", [
    (["mesh_refinement/refinement=static", "refined_region1/level=1"], "refined meshes"),
    (["turb_driving/driving_type=2"], "driving_type"),
    (["ion-neutral/gamma_ion=1.0"], "ion-neutral"),
])
def test_python_host_refuses(extra, what):
    from athenak_amd.mesh import MeshBlockPack
    from athenak_amd.turb_driver import turb_deck_checks
    pin = _deck(extra)
    with pytest.raises(RuntimeError, match=what):
        turb_deck_checks(pin)
    # AddPhysics says it before any physics module is built
    pk = MeshBlockPack.__new__(MeshBlockPack)
    pk.phydro = pk.pmhd = None
    with pytest.raises(RuntimeError, match=what):
        MeshBlockPack.AddPhysics(pk, pin)


def test_python_host_refuses_hst_and_rst_with_turb():
    from athenak_amd.mesh import Mesh
    from athenak_amd.outputs import Outputs
    pin = _deck(["output2/file_type=hst", "output2/dt=0.1"])
    pm = Mesh(pin)
    with pytest.raises(RuntimeError, match="turbulence history"):
        Outputs(pin, pm)
    pin = _deck(["output2/file_type=rst", "output2/dt=0.1"])
    with pytest.raises(RuntimeError, match="rst output with <turb_driving>"):
        Outputs(pin, Mesh(pin))


def test_cpp_host_refuses_turb_driving():
    """the C++ host does not run <turb_driving>: it stops with a message before anything is allocated"""
    body = r"""
import sys
sys.path.insert(0, %r)
from athenak_amd import capi
from athenak_amd.main import load_deck
L = capi.lib()
h = L.akmi_sim_create(load_deck("turb_hydro.athinput", ["time/nlim=1"]).Dump().encode(), None)
print(L.akmi_last_error().decode())
print("not refused")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", body], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "not refused" not in r.stdout
    assert "### FATAL ERROR" in r.stderr and "turb_driving" in r.stderr, r.stderr[-2000:]


# ---- the gid-ordered global sum on several ranks (gloo, CPU) ---------------------------
def _sums_worker(rank, world, port, outdir):
    import types
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from athenak_amd.mesh import LoadBalance
    from athenak_amd.turb_driver import gid_ordered_sums
    nmb_total, K = 11, 4
    rng = np.random.default_rng(7)
    allp = rng.standard_normal((nmb_total, K))*10.0**rng.integers(-8, 8, (nmb_total, K))   # wide range: order matters
    _, slist, nlist = LoadBalance([1.0]*nmb_total, world)
    pk = types.SimpleNamespace(pmesh=types.SimpleNamespace(nmb_total=nmb_total, nranks=world), gids=slist[rank],
                               nmb_thispack=nlist[rank])
    got = gid_ordered_sums(allp[slist[rank]:slist[rank] + nlist[rank]], pk)
    np.save(os.path.join(outdir, "r%d.npy" % rank), np.array(got))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_gid_ordered_sums_do_not_depend_on_the_rank_count(world, tmp_path):
    """every rank gets the sequential gid-order sum of all MeshBlocks' partials, bit for bit the one-rank result"""
    import types
    import torch.multiprocessing as mp
    from test_distributed_gloo import _free_port
    from athenak_amd.turb_driver import gid_ordered_sums
    mp.spawn(_sums_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    rng = np.random.default_rng(7)
    allp = rng.standard_normal((11, 4))*10.0**rng.integers(-8, 8, (11, 4))
    one = np.array(gid_ordered_sums(allp, types.SimpleNamespace(
        pmesh=types.SimpleNamespace(nmb_total=11, nranks=1), gids=0, nmb_thispack=11)))
    want = []
    for q in range(4):
        s = 0.0
        for g in range(11):
            s += float(allp[g, q])
        want.append(s)
    assert np.array_equal(one, np.array(want))
    for r in range(world):
        assert np.array_equal(np.load(str(tmp_path / ("r%d.npy" % r))).view(np.uint64), one.view(np.uint64))
