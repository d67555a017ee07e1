"""GPU tests of the lean ConsToPrim and the sweeps that make it possible (<mhd>/lean_prims, C++ host): k_sweep12s takes
density and momentum from u0 and the cell-centred field from the faces, the x3 march takes the field from the faces too,
and the conversion before such a stage stores w0[4] alone; akmi_sim_execute still returns with every array complete.
Everything is compared bit for bit, ghost zones included: u0, the faces, w0, bcc0, the floor counters and (time, dt).
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity_util as pu  # noqa: E402

X3_U0, X12_U0, LEAN, FACES = 1, 2, 4, 8          # capi.FORM_*
FORMS = X3_U0 | X12_U0 | FACES                   # what lean_prims = true asks of an eligible stage
MESH = (24, 20, 28)      # cell sizes that are no powers of two, several chunks of both marches, 60-cell waves end inside rows
PAIRS = 156              # 160^3 allocated cells in one block: the smallest even-row mesh the pair conversion takes
FLOORS = {"dfloor": 25.0/(36.0*math.pi), "pfloor": 5.0/(12.0*math.pi)}     # as in test_gpu_mhd_u0_sweeps.py


class _Bare(str):
    """a deck value that parity_util's params (repr of the value) writes without quotes"""
    __repr__ = str.__str__


def _arrays(sim):
    ph = sim.phys
    d = pu.product_arrays(sim)
    d["w0"] = ph.w0.cpu().numpy()
    d["bcc0"] = ph.bcc0.cpu().numpy()
    return d


def _params(lean, floors):
    params = dict(FLOORS) if floors else {}
    if lean is not None:
        params["lean_prims"] = _Bare(lean)
    return params


def _nst(integrator):
    return {"rk1": 1, "rk2": 2, "rk3": 3}[integrator]


def _result(sim, integrator):
    out = dict(arrays=_arrays(sim), counters=sim.floor_counters(), clock=(sim.time, sim.dt),
               forms=[sim.stage_forms(s) for s in range(1, _nst(integrator) + 1)])
    sim.close()
    return out


@functools.lru_cache(maxsize=None)
def _run(lean, steps, integrator="rk2", floors=True, mesh=MESH, tlim=None, sentinel=False):
    """3-D Orszag-Tang through the C++ host; lean = deck value of <mhd>/lean_prims (None: key absent), steps = tuple of
    Execute(max_cycles) calls, each of which must run that many cycles unless tlim is given"""
    kw = {"extra": ("time/tlim=%r" % tlim,)} if tlim is not None else {}
    sim, _, _ = pu.make_pair("orszag_tang", mesh, 3, mesh, fused=True, native=True, params=_params(lean, floors),
                             cfl=0.3, integrator=integrator, **kw)
    if sentinel:         # a read of a dropped array would spread NaNs; an array left unwritten would keep them
        sim.phys.w0[:, 0:4] = float("nan")
        sim.phys.bcc0[:] = float("nan")
        import torch
        torch.cuda.synchronize()
    ran = []
    for n in steps:
        ran.append(sim.Execute(max_cycles=n))
        assert tlim is not None or ran[-1] == n
    out = _result(sim, integrator)
    out["ran"] = ran
    return out


def _expected_forms(integrator, lean_before_first):
    """lean_prims = true: every stage that does not write the array it reads takes all forms; LEAN where the conversion
    before it was a lean one -- always between the stages of a cycle, before a first stage only inside a call.  rk3's
    second stage is in place: old form, full conversion before it."""
    first = FORMS | (LEAN if lean_before_first else 0)
    return {"rk1": [first], "rk2": [first, FORMS | LEAN], "rk3": [first, 0, FORMS | LEAN]}[integrator]


ORACLE_CASES = [
    # id, mesh, meshblock, integrator, floors
    ("24x20x28", MESH, MESH, "rk2", False),
    ("32^3", 32, 32, "rk2", False),
    ("32x16x16-2blocks", (32, 16, 16), 16, "rk2", False),
    ("27x20x28", (27, 20, 28), (27, 20, 28), "rk2", False),
    ("rk1", MESH, MESH, "rk1", False),
    ("rk3", MESH, MESH, "rk3", False),
    ("floors", MESH, MESH, "rk2", True),
]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: c[0])
def test_against_oracle(case):
    """3 cycles in ONE Execute call (the conversions between its cycles are lean) against 3 steps of the oracle"""
    _, n, mb, integrator, floors = case
    sim, osim, _ = pu.make_pair("orszag_tang", n, 3, mb, fused=True, native=True, params=_params("true", floors),
                                cfl=0.3, integrator=integrator)
    assert sim.Execute(max_cycles=3) == 3
    for _ in range(3):
        assert osim.step()
    clock = (sim.time, sim.dt)
    res = _result(sim, integrator)
    assert clock == (osim.time, osim.dt), (clock, osim.time, osim.dt)
    want = pu.oracle_arrays(osim, True)
    want["w0"], want["bcc0"] = osim.array("w0"), osim.array("bcc0")
    for k, v in want.items():
        assert np.array_equal(res["arrays"][k], v), k
    assert res["forms"] == _expected_forms(integrator, True), res["forms"]
    if floors:
        # a lean conversion has written floored u0 back and the sweeps have read it
        assert res["counters"][0] > 0 and res["counters"][1] > 0, res["counters"]


def _same(a, b):
    assert a["clock"] == b["clock"], (a["clock"], b["clock"])
    assert a["counters"] == b["counters"], (a["counters"], b["counters"])
    for k in a["arrays"]:
        assert np.array_equal(a["arrays"][k], b["arrays"][k]), k


@pytest.mark.parametrize("integrator", ["rk2", "rk3"])
def test_new_against_old(integrator):
    """lean_prims = true against false in one process, with floors that bind"""
    new, old = _run("true", (3,), integrator), _run("false", (3,), integrator)
    assert new["forms"] == _expected_forms(integrator, True), new["forms"]
    assert all(f in (0, X3_U0) for f in old["forms"]), old["forms"]
    assert new["counters"][0] > 0 and new["counters"][1] > 0, new["counters"]
    _same(new, old)


def test_one_cycle_per_call():
    """Execute(1) three times == Execute(3): a call of one cycle converts fully at its end, so its first stage never runs
    on lean primitives"""
    for integrator in ("rk1", "rk2"):
        single = _run("true", (1, 1, 1), integrator)
        assert single["forms"] == _expected_forms(integrator, False), single["forms"]
        _same(single, _run("true", (3,), integrator))


def test_call_that_ends_by_tlim_fills():
    """the third cycle is clipped by tlim inside a call that may run ten: the host learns that the loop has ended only after
    the cycle's lean conversion is enqueued, and akmi_mhd_prims_fill completes the arrays before the call returns"""
    t2, dt2 = _run("false", (2,))["clock"]
    tlim = t2 + 0.5*dt2
    new, old = _run("true", (10,), tlim=tlim), _run("false", (10,), tlim=tlim)
    assert new["ran"] == old["ran"] and 3 <= new["ran"][0] < 10, (new["ran"], old["ran"])
    assert new["clock"][0] >= tlim
    _same(new, old)


def test_nothing_reads_the_dropped_arrays():
    """NaNs planted in w0[0..3] and bcc0 before Execute(3): the sweeps never read them and the call rewrites them"""
    _same(_run("true", (3,), sentinel=True), _run("false", (3,)))


def test_auto_follows_the_pair_conversion():
    """auto: off on a small mesh (the conversion is latency-bound there), on where the conversion takes its pair kernel"""
    small = _run(None, (2,), floors=False)
    assert small["forms"] == [X3_U0, X3_U0], small["forms"]
    new, old = _run(None, (2,), floors=False, mesh=PAIRS), _run("false", (2,), floors=False, mesh=PAIRS)
    assert all(f & LEAN for f in new["forms"]), new["forms"]
    assert not any(f & (LEAN | X12_U0 | FACES) for f in old["forms"]), old["forms"]
    _same(new, old)


def _direct_pack(nx, ng=2, ideal=True):
    import torch
    from athenak_amd import capi
    from oracle import akref
    pk, dx = akref.make_pack(1, nx[0], nx[1], nx[2], ng, np.array([[1.0/n for n in nx]]), 5.0/3.0,
                             dfloor=0.3, pfloor=0.2)
    pkd = capi.Pack.from_buffer_copy(bytes(pk))
    if not ideal:
        pkd.is_ideal = 0
    dxd = torch.from_numpy(dx.copy()).cuda()
    pkd.dx = dxd.data_ptr()
    return pkd, dxd


def _direct_state(nx, ng, seed):
    rng = np.random.default_rng(seed)
    n1, n2, n3 = (n + 2*ng for n in nx)
    u = rng.uniform(0.5, 2.0, size=(1, 5, n3, n2, n1))
    u[:, 1:4] = rng.normal(size=u[:, 1:4].shape)
    b = [rng.normal(size=(1, n3, n2, n1 + 1)), rng.normal(size=(1, n3, n2 + 1, n1)), rng.normal(size=(1, n3 + 1, n2, n1))]
    emag = 0.5*((0.5*(b[0][..., :-1] + b[0][..., 1:]))**2 + (0.5*(b[1][:, :, :-1] + b[1][:, :, 1:]))**2 +
                (0.5*(b[2][:, :-1] + b[2][:, 1:]))**2)
    u[:, 4] = 0.5*(u[:, 1]**2 + u[:, 2]**2 + u[:, 3]**2)/u[:, 0] + emag + rng.uniform(0.5, 3.0, size=u[:, 4].shape)
    low = rng.random(size=u[:, 0].shape)
    u[:, 0][low < 0.05] = 0.1                          # below the density floor
    u[:, 4][(low > 0.05) & (low < 0.1)] = 0.01         # below the pressure floor
    return u, b


@pytest.mark.parametrize("drop", [1, 2, 3])
def test_lean_conversion_plus_fill_is_the_full_conversion(drop):
    """akmi_mhd_c2p_newdt_lean + akmi_mhd_prims_fill == akmi_mhd_c2p_newdt in all eight arrays, u0, the counters and the CFL
    minima, with a tenth of the cells below a floor; the lean call alone leaves the dropped arrays untouched"""
    import torch
    from athenak_amd import capi
    L = capi.lib()
    pkd, keep = _direct_pack(MESH)
    u, b = _direct_state(MESH, 2, 43)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = []
    for lean in (False, True):
        ud, bd = t(u), [t(x) for x in b]
        wd = torch.full(u.shape, -7.0, dtype=torch.float64, device="cuda")
        bccd = torch.full((1, 3) + u.shape[2:], -7.0, dtype=torch.float64, device="cuda")
        cnt, dt3 = torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")
        fp = [capi._p(x) for x in bd]
        if lean:
            capi.check(L.akmi_mhd_c2p_newdt_lean(C.byref(pkd), capi._p(ud), *fp, capi._p(wd), capi._p(bccd), 1,
                                                 capi._p(cnt), capi._p(dt3), drop, None), "c2p_newdt_lean")
            if drop & 1:
                assert bool((wd[:, 0:4] == -7.0).all())
            if drop & 2:
                assert bool((bccd == -7.0).all())
            assert bool((wd[:, 4] != -7.0).all())
            capi.check(L.akmi_mhd_prims_fill(C.byref(pkd), capi._p(ud), *fp, capi._p(wd), capi._p(bccd), drop, None),
                       "prims_fill")
        else:
            capi.check(L.akmi_mhd_c2p_newdt(C.byref(pkd), capi._p(ud), *fp, capi._p(wd), capi._p(bccd), 1, capi._p(cnt),
                                            capi._p(dt3), None), "c2p_newdt")
        out.append([x.cpu().numpy() for x in (ud, wd, bccd, cnt, dt3)])
    assert out[0][3][0] > 100 and out[0][3][1] > 100, out[0][3]
    for name, a, c in zip(("u0", "w0", "bcc0", "counters", "dt3"), out[0], out[1]):
        assert np.array_equal(a, c), name


@pytest.mark.parametrize("why", ["isothermal", "ppm4"])
def test_stage_refuses_a_form_flag_where_the_sequence_does_not_apply(why):
    import torch
    from athenak_amd import capi
    L = capi.lib()
    ng = 3 if why == "ppm4" else 2
    pkd, keep = _direct_pack(MESH, ng=ng, ideal=why != "isothermal")
    u, b = _direct_state(MESH, ng, 44)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ud, u1d, wd = t(u), t(u), t(u)
    b0, b1 = [t(x) for x in b], [t(x) for x in b]
    bccd = torch.zeros((1, 3) + u.shape[2:], dtype=torch.float64, device="cuda")
    ws = torch.zeros(int(L.akmi_stage_workspace_bytes(C.byref(pkd), 1))//8 + 1, dtype=torch.float64, device="cuda")
    recon = 2 if why == "ppm4" else 1                   # AKMI_RECON_PPM4 / AKMI_RECON_PLM; rsolver 3: AKMI_RS_HLLD
    for flags in (capi.COPY_X3_U0 | capi.COPY_X12_U0, capi.COPY_X3_U0 | capi.COPY_BCC_FACES):
        rc = L.akmi_mhd_stage_update(C.byref(pkd), recon, 3, capi.d(0.0), capi.d(1.0), capi.d(1e-3), 2 | flags,
                                     capi._p(wd), capi._p(bccd), capi._p(ud), capi._p(u1d), *[capi._p(x) for x in b0],
                                     *[capi._p(x) for x in b1], capi._p(ws), None)
        assert rc < 0
        assert b"k_sweep12s" in L.akmi_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(u1d.cpu().numpy(), u)         # nothing ran
