"""gpu: physical source terms (<hydro_srcterms> / <mhd_srcterms>: const_accel, ism_cooling) through the C ABI and both
hosts, against the restatement of tests/srcterms_restate.py.  The cases live in tests/srcterms_gpu_cases.py; every one
runs in a process of its own under a time limit and prints the figures it asserts on.

Tolerances.  The constant acceleration is compared bit for bit.  The cooling function goes through the device's log10 /
exp / pow: with the OpenCL-profile limits for double (log10 <= 3 ulp, exp <= 3 ulp, pow <= 16 ulp) the table branch gives
|d log Lambda| <= 25*max|lhd[i+1] - lhd[i]|*3 ulp(8.2) ~ 8e-14, i.e. d Lambda/Lambda <= ln 10*8e-14 + 16*2.2e-16 ~ 2e-13;
the tests allow 1e-12 relative on the cooling term (floor: one ulp of u0(IEN)) and leave out cells whose restated
log10 T lies within 1e-12 of a branch point (4.2, 8.15), at most 0.01 % of a sample.
The exact solution (uniform gas, constant g): v = g t and p = p0 to 1e-13 relative; E = E0 + rho (g t)^2/2 to 1e-13 of
E (one ulp of E is 3e-13 of the increment itself at g t < 0.1 c_s, so no double-precision code meets a bound relative
to the increment)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "srcterms_gpu_cases.py")
pytestmark = pytest.mark.gpu

# switches that are read when the package is imported: first stage in place
ENV = {"tasks_ip": {"AKMI_TASK_OOP": "0"}, "fused_ip": {"AKMI_OUT_OF_PLACE": "0"}}


def _run(*args, env=None, timeout=600):
    r = subprocess.run([sys.executable, CASES] + [str(a) for a in args], env=dict(os.environ, **(env or {})),
                       capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), "rc %d\n%s\n%s" % (
        r.returncode, r.stdout[-3000:], r.stderr[-5000:])
    return r.stdout


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(*args, world=2, timeout=600):
    """one process per rank, sharing the GPU; all of them have to end well"""
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, CASES] + [str(a) for a in args] + [str(r), str(world), str(port)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (o, e) in zip(procs, outs):
        print(o[-2000:])
        assert p.returncode == 0 and o.rstrip().endswith("OK"), "rc %d\n%s\n%s" % (p.returncode, o[-3000:], e[-5000:])


def test_const_accel_abi_bitwise():
    """akmi_srcterms_apply on random (w0, u0): dir 1/2/3, ideal and isothermal, hydro and MHD array shapes, 1 and 5
    MeshBlocks, blocks that are neither cubes nor multiples of a wave, dt by value and from device memory; ghost zones
    and every other variable untouched"""
    _run("abi_accel")


def test_cooling_abi_to_the_derived_tolerance(tmp_path):
    """2^20 temperatures log-uniform in [10, 1e9] K: the cooling term to 1e-12 relative, akmi_srcterms_newdt to 1e-12,
    (double)FLT_MAX exactly without cooling; both terms in one launch = the restated sequence"""
    _run("abi_cool", tmp_path)
    assert (tmp_path/"srcterms_coolfn.txt").exists()


@pytest.mark.parametrize("path", ["tasks", "tasks_ip", "fused", "fused_ip"])
@pytest.mark.parametrize("case", ["rt2d", "rt3d_mhd"])
def test_every_application_of_a_run_bitwise(case, path):
    """rt2d (RK3 / PPM4 / HLLC) and rt3d MHD (RK2 / PLM / HLLD), 20 cycles: w0, u0 before and after every srctrms call"""
    _run("run_snap", case, path, env=ENV.get(path))


def test_every_cooling_application_of_a_driven_run():
    _run("run_snap", "turb_cooling", "tasks")


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("mode", ["py_tasks", "py_fused", "cpp_sync", "cpp_runahead", "mb8", "smr"])
def test_uniform_gas_under_constant_acceleration(mode, d):
    """fails without the feature: the block is ignored and the gas stays at rest"""
    _run("uniform", mode, d)


def test_uniform_gas_cycle_graph_1d():
    _run("uniform", "graph", 1)


@pytest.mark.parametrize("mode", ["rank_py", "rank_cpp"])
def test_uniform_gas_two_ranks(mode):
    _run_ranks("uniform", mode, 3)


@pytest.mark.parametrize("case", ["rt3d", "rt3d_mhd"])
def test_paths_agree_bitwise(case, tmp_path):
    """task chain = fused stage = C++ host (synchronous, run-ahead) = 2 ranks (both hosts) on u0, b0, time, dt"""
    for path in ("tasks", "fused", "sync", "runahead"):
        _run("paths", case, path, tmp_path)
    _run_ranks("paths", case, "fused", tmp_path)
    _run_ranks("paths", case, "sync", tmp_path)
    ref = np.load(str(tmp_path/("%s_tasks_w1_r0.npz" % case)))
    assert np.isfinite(ref["u0"]).all()
    for path in ("fused", "sync", "runahead"):
        got = np.load(str(tmp_path/("%s_%s_w1_r0.npz" % (case, path))))
        for k in ref.files:
            assert np.array_equal(got[k].view(np.uint64), ref[k].view(np.uint64)), (path, k)
    for path in ("fused", "sync"):
        for r in range(2):
            got = np.load(str(tmp_path/("%s_%s_w2_r%d.npz" % (case, path, r))))
            g0 = int(got["gids"][0])
            for k in ref.files:
                if k == "gids":
                    continue
                want = ref[k] if k in ("time", "dt") else ref[k][g0:g0 + got[k].shape[0]]
                assert np.array_equal(got[k].view(np.uint64), want.view(np.uint64)), (path, r, k)


@pytest.mark.parametrize("path", ["tasks", "fused", "sync"])
def test_thermal_equilibrium(path):
    _run("equilibrium", path)
