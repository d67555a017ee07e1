"""The C entry points of the C++ host (csrc/akmi_host*.cpp: akmi_sim_*, akmi_comm_*, akmi_host_exchange_plan) return
AKMI_FAIL / NULL with the message in akmi_last_error() for RUN-TIME failures -- a device allocation, a HIP call, anything the
C++ runtime throws -- instead of letting an exception cross `extern "C"` and abort the caller (include/akmi.h:24-27; the
TaskStatus::fail of src/tasklist/task_list.hpp:30).  Errors of the input deck keep the reference's "### FATAL ERROR" + exit
(src/eos/eos.cpp:37-39).  Every case runs in a process of its own: the point is that the PROCESS survives."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROLOGUE = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
from athenak_amd import capi
from athenak_amd.main import load_deck
L = capi.lib()
def deck(n, extra=()):
    ov = ["time/nlim=2"]
    for q in (1, 2, 3):
        ov += ["mesh/nx%%d=%%d" %% (q, n), "meshblock/nx%%d=%%d" %% (q, n)]
    return load_deck("orszag_tang.athinput", ov + list(extra)).Dump().encode()
def create(text):
    h = L.akmi_sim_create(text, None)
    return h, L.akmi_last_error().decode()
""" % ROOT


def _run(body, env=None):
    r = subprocess.run([sys.executable, "-c", PROLOGUE + body], env=dict(os.environ, **(env or {})), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, "the process died (rc %d)\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="the machine has a device")
def test_create_without_a_device_is_an_error_return():
    out = _run(r"""
h, msg = create(deck(16))
assert not h and "akmi_sim_create" in msg and "hipMalloc" in msg, (h, msg)
print("alive:", msg)
""")
    assert "alive" in out


@pytest.mark.gpu
def test_injected_allocation_failure_is_an_error_return():
    """the 7th device allocation of the process fails (the Mesh and half of the physics exist by then)"""
    out = _run(r"""
h, msg = create(deck(16))
assert not h and "akmi_sim_create" in msg and "injected" in msg, (h, msg)
h2, msg2 = create(deck(16))                   # and again: nothing is left in a state that faults
assert not h2 and "injected" in msg2
print("alive:", msg)
""", env={"AKMI_FAIL_ALLOC_AFTER": "7"})
    assert "alive" in out


@pytest.mark.gpu
def test_failures_return_and_the_library_keeps_working():
    out = _run(r"""
import torch
torch.cuda.set_device(0)
# a MeshBlock no device holds: 6144^3 cells x 5 variables x 8 bytes = 9.3 TB for u0 alone
h, msg = create(deck(6144))
assert not h and "hipMalloc" in msg, (h, msg)
print("too large:", msg)
# an exception of the C++ runtime: std::stol on a digit string beyond long (std::out_of_range)
h, msg = create(deck(16, ["mhd/fused_stage=99999999999999999999999999"]))
assert not h and "akmi_sim_create" in msg, (h, msg)
print("runtime exception:", msg)
# execute before initialize
h, msg = create(deck(16))
assert h, msg
h = C.c_void_p(h)
assert L.akmi_sim_execute(h, 1) < 0 and "initialize" in L.akmi_last_error().decode()
L.akmi_sim_destroy(h)
# ... and an ordinary run still works in the same process
sys.path.insert(0, %r)
import parity_util as pu
r = pu.compare_run("orszag_tang", 16, 3, 16, cycles=2, native=True, fused=True)
assert r["bitwise_equal"], r
print("alive")
""" % os.path.join(ROOT, "tests"))
    assert "alive" in out and "too large" in out and "runtime exception" in out


# AKMI_FAIL_ALLOC_AFTER counts the allocations (DvceArray::Realloc) of each element type on their own.  ONE akmi_sim_create of
# the 16^3 Orszag-Tang deck makes 27, read off a build that printed them (gpu run of the knob at 26 and 27: 3 159 072 bytes
# held either way): 24 of doubles -- dx, u0 w0 u1, dt3, bcc0, b0 and b1 (3 faces each), and on the task path that small 3-D
# MHD packs take the flux faces (3), the edge fields (3) and the six sweep EMFs -- and 3 of ints (bcs, neighbours, counters)
NALLOC_REAL_CREATE_16 = 24


@pytest.mark.gpu
def test_failed_create_releases_device_memory():
    """a create that fails half-way gives back what it had allocated: the second simulation fails at its 5th array of doubles
    (dt3), with the MeshBlock tables, u0, w0, u1 (12 MB each at 64^3) and the counters in existence"""
    out = _run(r"""
h, msg = create(deck(16))
assert h, msg
L.akmi_sim_destroy(C.c_void_p(h))
assert L.akmi_host_device_bytes() == 0, L.akmi_host_device_bytes()
h, msg = create(deck(64))
held = L.akmi_host_device_bytes()
print("held after the failed create:", held)
assert not h and "akmi_sim_create" in msg and "injected" in msg, (h, msg)
assert held == 0, held
print("alive:", msg)
""", env={"AKMI_FAIL_ALLOC_AFTER": str(NALLOC_REAL_CREATE_16 + 4)})
    assert "alive" in out


@pytest.mark.gpu
@pytest.mark.parametrize("deck_name,extra", [("orszag_tang.athinput", ["mhd/fused_stage=true"]),     # run-ahead cycles: d_dt
                                             ("sod.athinput", [])])                                 # stage kernel writes w1
def test_destroy_releases_everything(deck_name, extra):
    """create, initialize, two cycles, destroy: no device array of the host outlives its simulation (the arrays are the
    zero-filled ones of the create: nothing is compared but the return codes and the counter)"""
    out = _run(r"""
ov = ["time/nlim=2"] + %r
for q in (1, 2, 3):
    ov += ["mesh/nx%%d=16" %% q, "meshblock/nx%%d=16" %% q]
h, msg = create(load_deck(%r, ov).Dump().encode())
assert h, msg
h = C.c_void_p(h)
assert L.akmi_host_device_bytes() > 0
rc = L.akmi_sim_initialize(h, C.c_double(-1.0))
assert rc == 0, (rc, L.akmi_last_error().decode())
rc = L.akmi_sim_execute(h, 2)
assert rc == 2, (rc, L.akmi_last_error().decode())
L.akmi_sim_destroy(h)
assert L.akmi_host_device_bytes() == 0, L.akmi_host_device_bytes()
print("alive")
""" % (extra, deck_name))
    assert "alive" in out
