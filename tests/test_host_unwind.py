"""CPU: a constructor of the C++ host that throws releases what it and its sub-objects had built (csrc/akmi_host.hpp: DvceArray,
std::unique_ptr, HipHandle).  On a machine without a device every akmi_sim_create fails at its first device allocation, with
the Mesh, the MeshBlockPack and the MeshBlock tables already built; the three host files are compiled under AddressSanitizer,
linked with tests/host_unwind_main.c (a program of its own: nothing is preloaded, nothing sanitised is loaded into Python) and
the kernels' objects of the ordinary build, and LeakSanitizer has nothing to report when the program exits."""
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOST_SOURCES = ["akmi_host.cpp", "akmi_host_smr.cpp", "akmi_host_comm.cpp"]


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _hipcc():
    return "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


@pytest.mark.skipif(_has_gpu(), reason="the machine has a device: akmi_sim_create would succeed")
@pytest.mark.skipif(_hipcc() is None, reason="needs hipcc")
def test_failed_creates_leak_nothing(tmp_path):
    import __graft_entry__ as g
    g.build()
    objdir = os.path.join(g.LIBDIR, "obj")
    kernels = [os.path.join(objdir, s + ".o") for s in g.HIP_SOURCES if s.endswith(".hip")]
    if not all(os.path.exists(o) for o in kernels):     # a library without its objects: compile them again
        g.build(force=True)
    hipcc, out = _hipcc(), str(tmp_path)
    asan = ["-Xarch_host", "-fsanitize=address"]        # the host side only: device code is compiled as in the ordinary build
    cflags = [f for f in g.HIPCC_FLAGS if f not in ("-shared", "-O3")] + ["-O1", "-g"] + asan

    def compile_one(src):
        obj = os.path.join(out, src + ".o")
        subprocess.check_call([hipcc] + cflags + ["-c", os.path.join(g.CSRC, src), "-o", obj], cwd=g.CSRC)
        return obj

    with ThreadPoolExecutor(max_workers=len(HOST_SOURCES)) as ex:
        objs = list(ex.map(compile_one, HOST_SOURCES))
    main = os.path.join(out, "host_unwind_main.o")
    subprocess.check_call([hipcc, "-x", "c", "-std=c99", "-O1", "-g"] + asan + ["-c",
                           os.path.join(ROOT, "tests", "host_unwind_main.c"), "-o", main])
    exe = os.path.join(out, "host_unwind")
    subprocess.check_call([hipcc, "--offload-arch=gfx950"] + asan + ["-o", exe, main] + objs + kernels + ["-ldl"])
    # two MeshBlocks per direction: the exchange plan for two ranks needs more than the deck's one block
    deck = open(os.path.join(ROOT, "athenak_amd", "inputs", "orszag_tang.athinput")).read()
    head, blk = deck.split("<meshblock>")
    blk = re.sub(r"(?m)^nx([12]) = \d+", r"nx\1 = 200", blk)
    assert blk.count("= 200") == 2
    path = os.path.join(out, "deck.athinput")
    with open(path, "w") as f:
        f.write(head + "<meshblock>" + blk)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "LSAN_OPTIONS")}
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=300)
    text = r.stdout + r.stderr
    sys.stdout.write(text[-4000:])
    assert r.returncode == 0, text[-4000:]
    assert text.count("akmi_sim_create") == 3 and "plan entries" in text, text[-4000:]
    assert "LeakSanitizer" not in text and "AddressSanitizer" not in text, text[-4000:]
