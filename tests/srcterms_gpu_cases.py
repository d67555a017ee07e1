"""TEST INFRASTRUCTURE: the GPU cases of tests/test_gpu_srcterms.py.  Each case is run as
`python srcterms_gpu_cases.py <case> [args]` in a process of its own under the caller's time limit; it prints the
figures it measures, then asserts.  Two-rank cases are started once per rank (`rank world port` at the end)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import srcterms_restate as R  # noqa: E402
from athenak_amd import capi  # noqa: E402
from athenak_amd.main import Simulation, load_deck  # noqa: E402

UNITS3 = R.cooling_units(R.Units(3.0856775809623245e+18, 6.83e+31, 3.15576e+13, 1.4))
GAMMA = 5.0/3.0
NEAR = 1e-12           # cells whose restated log10 T lies this close to a branch point may be left out ...
MAX_SHARE = 1e-4       # ... at most this share of the sample


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def pack_of(nmb, nvar, nx, ng, ideal, gamma, dx_dev):
    return capi.Pack(nmb, nvar, nx[0], nx[1], nx[2], ng, dx_dev.data_ptr(), gamma if ideal else 0.0, 1e-37, 1e-37, 1e-37,
                     1e-37, 3e38, 0.0 if ideal else 1.0, 1 if ideal else 0)


def shape_of(nmb, nvar, nx, ng):
    return (nmb, nvar, nx[2] + 2*ng if nx[2] > 1 else 1, nx[1] + 2*ng if nx[1] > 1 else 1, nx[0] + 2*ng)


def near_branch(logt):
    return (np.abs(logt - 4.2) <= NEAR) | (np.abs(logt - 8.15) <= NEAR)


# ---- 3: constant acceleration through the ABI, bit for bit ---------------------------------
def abi_accel():
    L = capi.lib()
    rng = np.random.default_rng(3)
    n = 0
    for nx, ng in (((16, 16, 16), 2), ((20, 6, 10), 3), ((37, 5, 3), 2), ((70, 9, 1), 2), ((33, 1, 1), 4), ((64, 64, 8), 2)):
        for nmb in (1, 5):
            for ideal in (True, False):
                for nvar in ((5, 7) if ideal else (4, 6)):        # hydro / MHD shapes, with passive scalars
                    for d in (1, 2, 3):
                        sh = shape_of(nmb, nvar, nx, ng)
                        w0 = rng.standard_normal(sh)
                        w0[:, 0] = rng.uniform(0.1, 10.0, w0[:, 0].shape)
                        u0 = rng.standard_normal(sh)*10.0**rng.integers(-3, 4, sh)
                        beta, dt, g = float(rng.choice([1.0, 0.5, 0.25, 2.0/3.0])), float(rng.uniform(1e-4, 1e-1)), \
                            float(rng.uniform(-3.0, 3.0))
                        dxd = torch.ones((nmb, 3), dtype=torch.float64, device="cuda")
                        pk = pack_of(nmb, nvar, nx, ng, ideal, 1.4, dxd)
                        sc = capi.SrcTerms(1, d, 0, 0, g, 0.0, 1.4, 1.0, 1.0, 1.0)
                        wd, ud = torch.from_numpy(w0).cuda(), torch.from_numpy(u0).cuda()
                        dtd = torch.tensor([dt, 0.0], dtype=torch.float64, device="cuda")
                        by_dev = (n % 2 == 1)             # dt by value / from device memory, alternately
                        capi.check(L.akmi_srcterms_apply(C.byref(pk), C.byref(sc), capi.d(beta), capi.d(float("nan") if by_dev else dt),
                                                         capi._p(dtd) if by_dev else None, capi._p(wd), capi._p(ud),
                                                         capi._stream()), "apply")
                        want = R.apply(w0, u0, nx, ng, beta*dt, ideal, accel=(g, d))
                        got = ud.cpu().numpy()
                        assert np.array_equal(bits(got), bits(want)), (nx, ng, nmb, ideal, nvar, d, np.abs(got - want).max())
                        assert not np.array_equal(got, u0)
                        assert np.array_equal(wd.cpu().numpy(), w0)
                        n += 1
    # nothing enabled: nothing changes; a bad direction is an error
    sc = capi.SrcTerms(0, 1, 0, 0, 1.0, 0.0, 1.4, 1.0, 1.0, 1.0)
    capi.check(L.akmi_srcterms_apply(C.byref(pk), C.byref(sc), capi.d(1.0), capi.d(1.0), None, capi._p(wd), capi._p(ud),
                                     capi._stream()), "apply")
    assert np.array_equal(ud.cpu().numpy(), got)
    sc = capi.SrcTerms(1, 4, 0, 0, 1.0, 0.0, 1.4, 1.0, 1.0, 1.0)
    assert L.akmi_srcterms_apply(C.byref(pk), C.byref(sc), capi.d(1.0), capi.d(1.0), None, capi._p(wd), capi._p(ud),
                                 capi._stream()) == capi.FAIL
    print("abi_accel: %d cases bit for bit" % n)


# ---- 4, 5: cooling through the ABI, to the derived tolerance -------------------------------
def _cool_state(rng, nx, ng, nmb, nvar=5):
    sh = shape_of(nmb, nvar, nx, ng)
    w0 = rng.standard_normal(sh)
    rho = rng.uniform(0.1, 10.0, w0[:, 0].shape)
    temp = 10.0**rng.uniform(1.0, 9.0, rho.shape)                     # K, log-uniform in [10, 1e9]
    w0[:, 0] = rho
    w0[:, 4] = temp*rho/(UNITS3[0]*(GAMMA - 1.0))
    u0 = np.abs(rng.standard_normal(sh)) + 1.0
    u0[:, 4] = w0[:, 4]*rng.uniform(1.0, 2.0, rho.shape)               # an energy of the size of the gas's own
    return w0, u0


def abi_cool(outdir=None):
    L = capi.lib()
    rng = np.random.default_rng(4)
    nx, ng, nmb = (64, 64, 32), 2, 8                  # 2^20 active cells
    w0, u0 = _cool_state(rng, nx, ng, nmb)
    hrate = 2.0e-26
    cooling = (GAMMA, UNITS3, hrate)
    dxd = torch.ones((nmb, 3), dtype=torch.float64, device="cuda")
    pk = pack_of(nmb, 5, nx, ng, True, GAMMA, dxd)
    sc = capi.SrcTerms(0, 1, 1, 0, 0.0, hrate, GAMMA, *UNITS3)
    wd, ud = torch.from_numpy(w0).cuda(), torch.from_numpy(u0).cuda()
    beta, dt = 0.5, 1.0e-3
    capi.check(L.akmi_srcterms_apply(C.byref(pk), C.byref(sc), capi.d(beta), capi.d(dt), None, capi._p(wd), capi._p(ud),
                                     capi._stream()), "apply")
    got = ud.cpu().numpy()
    ks, js, is_ = R._active(nx, ng)
    a = (slice(None), ks, js, is_)
    term, logt = R.cooling_term(w0, nx, ng, beta*dt, cooling)
    assert term.size == 2**20
    got_term = u0[:, 4][a] - got[:, 4][a]            # what the kernel subtracted (exact where it matters: see the floor)
    skip = near_branch(logt)
    share = skip.mean()
    floor = np.spacing(np.abs(u0[:, 4][a]))           # one ulp of u0(IEN)
    err = np.abs(got_term - term)
    rel = np.where(skip, 0.0, np.maximum(err - floor, 0.0)/np.abs(term))
    print("abi_cool: cells %d, left out near a branch point %d (share %.2e), max rel diff of the cooling term %.3e "
          "(beyond one ulp of u0(IEN))" % (term.size, skip.sum(), share, rel.max()))
    assert share <= MAX_SHARE
    assert rel.max() <= 1e-12, rel.max()
    # the function by itself: the same cells with u0(IEN) = 0, so that the result IS the (negated) term and no rounding of
    # the subtraction hides the difference.  The term is a difference, rho*Lambda/cu - Gamma/hu: where cooling and heating
    # nearly balance (cold gas: that is where the thermal equilibrium lies) the relative difference of the NET term is the
    # one of Lambda times the cancellation factor, so the function is judged against the size of the two parts, which is
    # what the derivation of the tolerance bounds; the net-relative figure is printed for the record.
    uz = u0.copy()
    uz[:, 4] = 0.0
    udz = torch.from_numpy(uz).cuda()
    capi.check(L.akmi_srcterms_apply(C.byref(pk), C.byref(sc), capi.d(beta), capi.d(dt), None, capi._p(wd), capi._p(udz),
                                     capi._stream()), "apply")
    diff = np.where(skip, 0.0, np.abs(-udz.cpu().numpy()[:, 4][a] - term))
    gross = R.cooling_gross(w0, nx, ng, beta*dt, cooling)
    pure, pure_net = diff/gross, diff/np.abs(term)
    cancel = float((gross/np.abs(term)).ravel()[pure_net.argmax()])       # of the cell with the largest net-relative figure
    rel_fn = float(pure.max())
    print("abi_cool: with u0(IEN) = 0: max diff relative to the parts of the term %.3e, relative to the net term %.3e "
          "(cancellation factor there %.1e)" % (rel_fn, pure_net.max(), cancel))
    for name, m in (("KI02", logt <= 4.2), ("table", (logt > 4.2) & (logt <= 8.15)), ("power law", logt > 8.15)):
        print("  branch %-9s cells %7d  max rel to parts %.3e  to net %.3e" % (name, m.sum(), pure[m].max(), pure_net[m].max()))
    assert rel_fn <= 1e-12, rel_fn
    # everything else untouched: ghost zones of the energy, every other variable
    chk = got.copy()
    chk[:, 4][a] = u0[:, 4][a]
    assert np.array_equal(bits(chk), bits(u0))
    # 5: the time step
    dtd = torch.zeros(1, dtype=torch.float64, device="cuda")
    capi.check(L.akmi_srcterms_newdt(C.byref(pk), C.byref(sc), capi._p(wd), capi._p(dtd), capi._stream()), "newdt")
    got_dt = float(dtd.cpu()[0])
    cells, logt2 = R.newdt_cells(w0, nx, ng, cooling)
    keep = ~near_branch(logt2)
    assert (~keep).mean() <= MAX_SHARE
    want_dt = float(min(R.FLT_MAX, cells[keep].min()))
    print("abi_cool: newdt got %.17g want %.17g rel %.3e" % (got_dt, want_dt, abs(got_dt - want_dt)/want_dt))
    assert abs(got_dt - want_dt) <= 1e-12*want_dt
    sc0 = capi.SrcTerms(1, 1, 0, 0, 1.0, 0.0, GAMMA, 1.0, 1.0, 1.0)
    capi.check(L.akmi_srcterms_newdt(C.byref(pk), C.byref(sc0), capi._p(wd), capi._p(dtd), capi._stream()), "newdt")
    assert bits(dtd.cpu().numpy())[0] == bits(np.array([R.FLT_MAX]))[0]
    # both terms in one launch == the restated sequence (acceleration exact, cooling to the tolerance)
    sc2 = capi.SrcTerms(1, 2, 1, 0, -0.7, hrate, GAMMA, *UNITS3)
    ud2 = torch.from_numpy(u0).cuda()
    capi.check(L.akmi_srcterms_apply(C.byref(pk), C.byref(sc2), capi.d(beta), capi.d(dt), None, capi._p(wd), capi._p(ud2),
                                     capi._stream()), "apply")
    g2 = ud2.cpu().numpy()
    w2 = R.apply(w0, u0, nx, ng, beta*dt, True, accel=(-0.7, 2), cooling=cooling)
    assert np.array_equal(bits(g2[:, :4]), bits(w2[:, :4]))
    e_err = np.abs(g2[:, 4][a] - w2[:, 4][a])
    ok = skip | (e_err <= 1e-12*np.abs(term) + 2.0*np.spacing(np.abs(w2[:, 4][a])))
    assert ok.all()
    if outdir:
        with open(os.path.join(outdir, "srcterms_coolfn.txt"), "w") as f:
            f.write("cooling term, device against numpy restatement, 2^20 temperatures log-uniform in [10, 1e9] K, u0(IEN) = 0\n"
                    "max diff relative to bdt*rho*(rho*Lambda/cu + Gamma/hu): %.3e\n"
                    "max diff relative to the net term: %.3e (cancellation factor of that cell %.1e)\n"
                    "with u0(IEN) of the gas's own size, beyond one ulp of u0(IEN): %.3e\n"
                    "left out near a branch point: %d\n"
                    % (rel_fn, pure_net.max(), cancel, rel.max(), skip.sum()))


# ---- runs ----------------------------------------------------------------------------------
def _set(pin, ov):
    """"block/name=value" into the deck, whether it holds the parameter already or not"""
    for o in ov:
        b, rest = o.split("/", 1)
        k, v = rest.split("=", 1)
        pin.blocks.setdefault(b, {})[k] = v
    return pin


def _path_overrides(blk, path):
    """path: tasks | tasks_ip (first stage in place) | fused | fused_ip | sync | runahead | graph -> deck overrides and
    the environment the CALLER has to start this process with (the switches are read when the package is imported)"""
    ov = ["%s/small_pack_tasks=false" % blk]
    env = {}
    if path.startswith("tasks"):
        ov.append("%s/fused_stage=false" % blk)
    else:
        ov.append("%s/fused_stage=true" % blk)
    if path == "tasks_ip":
        env["AKMI_TASK_OOP"] = "0"
    if path == "fused_ip":
        env["AKMI_OUT_OF_PLACE"] = "0"
    if path == "sync":
        ov += ["time/run_ahead=false", "time/cycle_graph=false"]
    if path == "runahead":
        ov += ["time/run_ahead=true", "time/cycle_graph=false"]
    if path == "graph":
        ov += ["time/run_ahead=false", "time/cycle_graph=true"]
    return ov, env


RT3D_MHD = ["mhd/eos=ideal", "mhd/reconstruct=plm", "mhd/rsolver=hlld", "mhd/gamma=1.4", "mhd_srcterms/const_accel=true",
            "mhd_srcterms/const_accel_val=-0.1", "mhd_srcterms/const_accel_dir=3", "problem/b0=0.05"]


def _rt3d_mhd_pin(ov):
    """rt3d.athinput with <hydro> / <hydro_srcterms> replaced by their MHD twins"""
    from athenak_amd.parameter_input import ParameterInput
    text = open(os.path.join(ROOT, "athenak_amd", "inputs", "rt3d.athinput")).read()
    text = text.replace("<hydro_srcterms>", "<mhd_srcterms>").replace("<hydro>", "<mhd>").replace("rsolver = hllc", "rsolver = hlld")
    text = text.replace("variable = hydro_w", "variable = mhd_w")
    pin = ParameterInput(text=text)
    pin.blocks.setdefault("problem", {})["b0"] = "0.05"
    return _set(pin, ov)


def _sim(case, path, rank=0, world=1):
    """case: rt2d | rt3d | rt3d_mhd | turb_cooling"""
    blk = "mhd" if case in ("rt3d_mhd", "turb_cooling") else "hydro"
    ov, _ = _path_overrides(blk, path)
    if case == "rt3d_mhd":
        pin = _rt3d_mhd_pin(ov)
    else:
        pin = _set(load_deck(case + ".athinput"), ov if case != "turb_cooling" else [])
    if path in ("sync", "runahead", "graph"):
        from athenak_amd import native
        if world > 1:
            assert native.init_comm_from_torch_distributed() == "callbacks"
        return native.NativeSimulation(pin), pin
    return Simulation(pin, my_rank=rank, nranks=world), pin


def run_snap(case, path):
    """6: every ApplySrcTerms of a 20-cycle run of the Python host against the restatement"""
    sim, pin = _sim(case, path)
    ph = sim.phys
    ind = sim.pmesh.mb_indcs
    nx, ng = (ind.nx1, ind.nx2, ind.nx3), ind.ng
    ps = ph.psrc
    calls = {"n": 0, "worst": 0.0, "skipped": 0, "cells": 0}
    inner = ps.ApplySrcTerms
    ideal = ph.peos.eos_data.is_ideal

    def wrapped(w0, beta, dt, u0):
        wb, ub = w0.cpu().numpy().copy(), u0.cpu().numpy().copy()
        inner(w0, beta, dt, u0)
        ua = u0.cpu().numpy()
        assert np.array_equal(w0.cpu().numpy(), wb)
        bdt = beta*dt
        if ps.ism_cooling:
            cooling = (ph.peos.eos_data.gamma, (ps.temp_unit, ps.cooling_unit, ps.heating_unit), ps.hrate)
            want = R.apply(wb, ub, nx, ng, bdt, ideal, cooling=cooling)
            term, logt = R.cooling_term(wb, nx, ng, bdt, cooling)
            ks, js, is_ = R._active(nx, ng)
            a = (slice(None), ks, js, is_)
            skip = near_branch(logt)
            err = np.abs(ua[:, 4][a] - want[:, 4][a])
            floor = np.spacing(np.abs(ub[:, 4][a]))
            rel = np.where(skip, 0.0, np.maximum(err - floor, 0.0)/np.maximum(np.abs(term), 1e-300))
            calls["worst"] = max(calls["worst"], float(rel.max()))
            calls["skipped"] += int(skip.sum())
            calls["cells"] += skip.size
            assert rel.max() <= 1e-12, rel.max()
            ua2 = ua.copy()
            ua2[:, 4][a] = want[:, 4][a]
            assert np.array_equal(bits(ua2), bits(want))
        else:
            want = R.apply(wb, ub, nx, ng, bdt, ideal, accel=(ps.const_accel_val, ps.const_accel_dir))
            assert np.array_equal(bits(ua), bits(want)), np.abs(ua - want).max()
            assert not np.array_equal(ua, ub)
        calls["n"] += 1
    ps.ApplySrcTerms = wrapped
    sim.Execute(max_cycles=20)
    nst = sim.pdriver.nexp_stages
    print("run_snap %s %s: %d calls, fused %s, worst rel %.3e, skipped %d of %d" % (
        case, path, calls["n"], ph.fused, calls["worst"], calls["skipped"], calls["cells"]))
    assert calls["n"] == 20*nst
    assert ph.fused == path.startswith("fused")
    if calls["cells"]:
        assert calls["skipped"] <= MAX_SHARE*calls["cells"]
    assert np.isfinite(ph.u0.cpu().numpy()).all()


# ---- 7: uniform gas under constant acceleration ----------------------------------------------
def _uniform_pin(mode, d, mhd=False):
    """turb problem generator without <turb_driving>: uniform gas at rest, rho = 1, p = 1/gamma (c_s = 1), periodic"""
    from athenak_amd.parameter_input import ParameterInput
    blk = "mhd" if mhd else "hydro"
    one_d = mode == "graph"
    n = 32
    mbn = n if mode not in ("mb8", "smr", "rank_py", "rank_cpp") else n//2
    nx23 = 1 if one_d else n
    mb23 = 1 if one_d else mbn
    text = """<job>
basename = uniform
<mesh>
nghost = 2
nx1 = %d
x1min = -0.5
x1max = 0.5
nx2 = %d
x2min = -0.5
x2max = 0.5
nx3 = %d
x3min = -0.5
x3max = 0.5
<meshblock>
nx1 = %d
nx2 = %d
nx3 = %d
<time>
integrator = rk2
cfl_number = 0.3
nlim = -1
tlim = 10.0
<%s>
eos = ideal
gamma = 1.4
reconstruct = plm
rsolver = %s
small_pack_tasks = false
<%s_srcterms>
const_accel = true
const_accel_val = 0.4
const_accel_dir = %d
<problem>
pgen_name = turb
""" % (n, nx23, nx23, mbn, mb23, mb23, blk, "hlld" if mhd else "hllc", blk, d)
    if mode == "smr":
        text += "<mesh_refinement>\nrefinement = static\n<refined_region1>\nlevel = 1\nx1min = -0.2\nx1max = 0.2\n" \
                "x2min = -0.2\nx2max = 0.2\nx3min = -0.2\nx3max = 0.2\n"
    pin = ParameterInput(text=text)
    ov, _ = _path_overrides(blk, {"py_tasks": "tasks", "py_fused": "fused", "cpp_sync": "sync", "cpp_runahead": "runahead",
                                    "graph": "graph", "mb8": "fused", "smr": "tasks", "rank_py": "fused",
                                    "rank_cpp": "sync"}[mode])
    return _set(pin, ov)


def uniform(mode, d, rank=0, world=1):
    d = int(d)
    pin = _uniform_pin(mode, d)
    cpp = mode in ("cpp_sync", "cpp_runahead", "graph", "rank_cpp")
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    if cpp:
        from athenak_amd import native
        if world > 1:
            assert native.init_comm_from_torch_distributed() == "callbacks"
        sim = native.NativeSimulation(pin)
    else:
        sim = Simulation(pin, my_rank=rank, nranks=world)
    ph = sim.phys
    ind = sim.pmesh.mb_indcs
    ks, js, is_ = R._active((ind.nx1, ind.nx2, ind.nx3), ind.ng)
    a = (slice(None), slice(None), ks, js, is_)
    u_init = ph.u0.cpu().numpy()[a].copy()
    E0, rho, g, gam = u_init[:, 4], 1.0, 0.4, 1.4
    ncyc = 20 if mode == "smr" else 10
    if mode == "cpp_runahead":
        sim.Execute(max_cycles=ncyc)
    else:
        for _ in range(ncyc):
            sim.Execute(max_cycles=1)
    torch.cuda.synchronize()
    t = sim.time if cpp else sim.pmesh.time
    u = ph.u0.cpu().numpy()[a]
    gt = g*t
    assert 0.01 < gt < 0.1, gt                    # below a tenth of the sound speed (c_s = 1)
    v = u[:, d]/u[:, 0]
    p = (gam - 1.0)*(u[:, 4] - 0.5*(u[:, 1]**2 + u[:, 2]**2 + u[:, 3]**2)/u[:, 0])
    fv = np.abs(v - gt).max()/gt
    # E - E0 = rho (g t)^2 / 2, measured against E: one ulp of E (2.2e-16 at E = 1.79) is already 3e-13 of an increment of
    # 7e-4, so a bound relative to the increment itself cannot be met by any double-precision code at g t < 0.1 c_s
    fe = (np.abs((u[:, 4] - E0) - 0.5*rho*gt*gt)/u[:, 4]).max()
    fp = np.abs(p - 1.0/gam).max()/(1.0/gam)
    print("uniform %s dir %d rank %d: t %.6f g*t %.5f  rel err v %.3e  E-E0 %.3e  p %.3e" % (mode, d, rank, t, gt, fv, fe, fp))
    assert np.all(u[:, 0] == rho)
    for q in (1, 2, 3):
        if q != d:
            assert np.all(u[:, q] == 0.0)
    assert fv <= 1e-13 and fe <= 1e-13 and fp <= 1e-13, (fv, fe, fp)
    if cpp:
        sim.close()
        if world > 1:
            from athenak_amd import native
            native.finalize_comm()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


# ---- 8: the paths agree ------------------------------------------------------------------------
def paths(case, path, outdir, rank=0, world=1):
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    sim, pin = _sim(case, path, rank, world)
    cpp = path in ("sync", "runahead", "graph")
    if path == "runahead":
        sim.Execute(max_cycles=20)
    else:
        for _ in range(20):
            sim.Execute(max_cycles=1)
    torch.cuda.synchronize()
    ph = sim.phys
    pk = sim.pmesh.pmb_pack
    out = {"u0": ph.u0.cpu().numpy(), "gids": np.array([pk.gids]),
           "time": np.array([sim.time if cpp else sim.pmesh.time]), "dt": np.array([sim.dt if cpp else sim.pmesh.dt])}
    if case.endswith("mhd"):
        for f in ("x1f", "x2f", "x3f"):
            out["b0" + f] = getattr(ph.b0, f).cpu().numpy()
    np.savez(os.path.join(outdir, "%s_%s_w%d_r%d.npz" % (case, path, world, rank)), **out)
    print("paths %s %s rank %d/%d: time %.17g dt %.17g" % (case, path, rank, world, out["time"][0], out["dt"][0]))
    if cpp:
        sim.close()
        if world > 1:
            from athenak_amd import native
            native.finalize_comm()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


# ---- 9: thermal equilibrium ----------------------------------------------------------------------
def equilibrium(path):
    """hrate with rho*Lambda(T0) = Gamma at the restated Lambda: a uniform box at T0 keeps its energy.  At equilibrium
    the net rate is the rounding residue of two equal numbers, so the source time step eint/(FLT_MIN + |net|) is compared
    through the net rates, to 1e-12 of the gross cooling rate rho^2 Lambda/cu (the tolerance of the cooling function)."""
    from athenak_amd.parameter_input import ParameterInput
    text = open(os.path.join(ROOT, "athenak_amd", "inputs", "turb_cooling.athinput")).read()
    text = text[:text.index("<turb_driving>")]
    pin = ParameterInput(text=text)
    gam = pin.GetReal("mhd", "gamma")
    p_over_rho = 1.0/gam                                   # the turb generator: rho = 1, p = 1/gamma
    eint = p_over_rho/(gam - 1.0)
    # T0 ~ 5.8e3 K on the table branch: the temperature unit is linear in mu, so mu carries the factor 60 and the state
    # of the problem generator stays as it is
    pin.blocks["units"]["mu"] = repr(1.4*60.0)
    un = R.Units(3.0856775809623245e+18, 6.83e+31, 3.15576e+13, 1.4*60.0)
    tu, cu, hu = R.cooling_units(un)
    lam = float(R.ism_cool_fn(np.array([tu*eint/1.0*(gam - 1.0)]))[0])
    hrate = 1.0*(lam/cu)*hu
    pin.blocks["mhd_srcterms"]["hrate"] = repr(hrate)
    ov, _ = _path_overrides("mhd", path)
    _set(pin, ov)
    cpp = path == "sync"
    if cpp:
        from athenak_amd import native
        sim = native.NativeSimulation(pin)
    else:
        sim = Simulation(pin)
    ph = sim.phys
    ind = sim.pmesh.mb_indcs
    nx, ng = (ind.nx1, ind.nx2, ind.nx3), ind.ng
    ks, js, is_ = R._active(nx, ng)
    a = (slice(None), ks, js, is_)
    cooling = (gam, (tu, cu, hu), hrate)
    w0 = ph.w0.cpu().numpy()
    want_dt = R.newdt(w0, nx, ng, cooling)
    if not cpp:
        got_dt = ph.psrc.dtnew
        print("equilibrium: T0 %.1f K  source dtnew got %.6e restated %.6e" % (tu*eint*(gam - 1.0), got_dt, want_dt))
        rate_scale = 1.0*(1.0*lam/cu)
        assert abs(eint/got_dt - eint/want_dt) <= 1e-12*rate_scale + 1e-12*eint/want_dt
    worst = 0.0
    e_prev = ph.u0.cpu().numpy()[:, 4][a].copy()
    for c in range(10):
        sim.Execute(max_cycles=1)
        torch.cuda.synchronize()
        e = ph.u0.cpu().numpy()[:, 4][a].copy()
        worst = max(worst, float(np.abs(e - e_prev).max()/np.abs(e_prev).max()))
        e_prev = e
    print("equilibrium %s: largest relative change of the energy per cycle %.3e over 10 cycles, dt %.4e" % (
        path, worst, sim.dt if cpp else sim.pmesh.dt))
    assert worst <= 1e-12
    if cpp:
        sim.close()


if __name__ == "__main__":
    case, args = sys.argv[1], sys.argv[2:]
    torch.cuda.set_device(0)
    fn = {"abi_accel": abi_accel, "abi_cool": abi_cool, "run_snap": run_snap, "uniform": uniform, "paths": paths,
          "equilibrium": equilibrium}[case]
    if case in ("uniform", "paths") and len(args) >= 3 and args[-1].isdigit() and args[-2].isdigit() and args[-3].isdigit():
        rank, world, port = int(args[-3]), int(args[-2]), args[-1]
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
        fn(*args[:-3], rank=rank, world=world)
    else:
        fn(*args)
    print("OK")
