"""The library's stage entries are ONE call: akmi_X_stage_fused, akmi_X_stage_fused_dt, akmi_X_stage_phase with every
phase and akmi_X_stage_phase_dt with every phase fill the same StageCall, with dt either folded into beta (dt_dev = NULL)
or read from device memory.  The C++ host relies on it (FluidBase::LaunchStage reaches the library through the phase
entry that takes dt_dev alone), so from identical inputs every entry must leave every output array bit-identical.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import parity_util as pu  # noqa: E402
from athenak_amd import capi  # noqa: E402

FLT_MAX = float(np.finfo(np.float32).max)
# (fluid, reconstruct, rsolver, nghost): hydro's one-kernel tile and its generic sequence, MHD's k_sweep12s + x3 march
# and its generic sequence
SCHEMES = [("hydro", "plm", "hllc", 2), ("hydro", "ppm4", "hlle", 3), ("mhd", "plm", "hlld", 2), ("mhd", "plm", "hlle", 2)]
# mesh, MeshBlock, dimensions: two blocks of 16x8x8, one of 16x8(x1), one of 16(x1x1)
SHAPES = {"2x16x8x8": ((32, 8, 8), (16, 8, 8), 3), "16x8x1": ((16, 8), (16, 8), 2), "16x1x1": ((16,), (16,), 1)}
G0, G1, BETA = 0.0, 1.0, 1.193743905974738      # first-stage weights (RK4's beta: beta*dt is a product that rounds)


@functools.lru_cache(maxsize=None)
def _inputs(fluid, recon, rsolver, ng, shape):
    """a smooth, positive state (linear wave of amplitude 0.05) after Driver::Initialize: ghost zones filled, primitives
    converted in every cell; no floor binds"""
    n, mb, dims = SHAPES[shape]
    sim, _, is_mhd = pu.make_pair("linear_wave_" + fluid, n, dims, mb, fused=True, ng=ng, recon=recon, rsolver=rsolver,
                                  extra=["problem/amp=0.05"])
    ph = sim.phys
    arrs = {"u0": ph.u0, "w0": ph.w0}
    if is_mhd:
        arrs.update(bcc0=ph.bcc0, b0x1f=ph.b0.x1f, b0x2f=ph.b0.x2f, b0x3f=ph.b0.x3f)
    arrs = {k: v.clone() for k, v in arrs.items()}
    assert all(bool(torch.isfinite(v).all()) for v in arrs.values())
    assert float(arrs["w0"][:, 0].min()) > 0.5 and float(arrs["w0"][:, 4].min()) > 0.1      # density, internal energy
    return ph, arrs, float(sim.pmesh.dt), is_mhd


def _call(ph, arrs, dt, is_mhd, entry, phase, with_dt_dev, copy):
    """one stage call through `entry` on fresh copies of the inputs; every output array as host bytes"""
    L = capi.lib()
    a = {k: v.clone() for k, v in arrs.items()}
    a["u1"] = torch.full_like(a["u0"], -7.0)            # what a stage does not write must come out as it went in
    if is_mhd:
        for q in ("x1f", "x2f", "x3f"):
            a["b1" + q] = torch.full_like(a["b0" + q], -7.0)
    a["dt3"] = torch.full((3,), FLT_MAX, dtype=torch.float64, device="cuda")
    a["counters"] = torch.zeros(3, dtype=torch.int32, device="cuda")
    nbytes = int(L.akmi_stage_workspace_bytes(C.byref(ph.pack_c), 1 if is_mhd else 0))
    ws = torch.zeros((nbytes + 7)//8, dtype=torch.float64, device="cuda")
    dt_dev = torch.tensor([dt], dtype=torch.float64, device="cuda")
    p = lambda k: capi._p(a[k])
    args = [C.byref(ph.pack_c), ph.recon_method, ph.rsolver_method, capi.d(G0), capi.d(G1)]
    if entry.endswith("_dt"):
        args += [capi.d(BETA), capi._p(dt_dev)] if with_dt_dev else [capi.d(BETA*dt), None]
    else:
        args += [capi.d(BETA*dt)]
    args += [copy, p("w0")] + ([p("bcc0")] if is_mhd else []) + [p("u0"), p("u1")]
    if is_mhd:
        args += [p(b + q) for b in ("b0", "b1") for q in ("x1f", "x2f", "x3f")]
    args += [1, p("counters"), p("dt3")] + ([capi.PHASE_ALL] if phase else []) + [capi._p(ws), capi._stream()]
    capi.check(getattr(L, entry)(*args), entry)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().tobytes() for k, v in a.items()}


@pytest.mark.parametrize("copy", [1, 2])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("scheme", SCHEMES, ids=lambda s: "-".join(map(str, s[:3])))
def test_entries_are_one_call(scheme, shape, copy):
    """u0, u1, w0, (bcc0, b0*, b1*,) dt3 and counters after akmi_X_stage_fused against the other entries, do_newdt = 1"""
    fluid = scheme[0]
    ph, arrs, dt, is_mhd = _inputs(*scheme, shape)
    ref = _call(ph, arrs, dt, is_mhd, "akmi_%s_stage_fused" % fluid, False, False, copy)
    # (the call did run: copy 1 leaves the old state in u1 and the new one in u0, copy 2 writes the new one into u1)
    assert ref["u1"] != torch.full_like(arrs["u0"], -7.0).cpu().numpy().tobytes()
    assert (ref["u0"] == arrs["u0"].cpu().numpy().tobytes()) == (copy == 2)
    for entry, phase, with_dt_dev in [("stage_fused_dt", False, False), ("stage_fused_dt", False, True),
                                      ("stage_phase", True, False), ("stage_phase_dt", True, False),
                                      ("stage_phase_dt", True, True)]:
        out = _call(ph, arrs, dt, is_mhd, "akmi_%s_%s" % (fluid, entry), phase, with_dt_dev, copy)
        differ = [k for k in ref if out[k] != ref[k]]
        assert not differ, (entry, "dt_dev" if with_dt_dev else "NULL", differ)
