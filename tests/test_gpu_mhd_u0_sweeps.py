"""GPU tests of the u0 form of the MHD stage (<mhd>/u0_sweeps, C++ host): the x3 march of a stage that does not write
the array it reads takes density and momentum from u0 instead of their copies in w0, and the last stage of a cycle is
made such a stage (result into u1's buffer, registers traded).  Everything is compared bit for bit, ghost zones included.
"""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import parity_util as pu  # noqa: E402

X3_U0 = 1        # capi.FORM_X3_U0; the other two forms (k_sweep12s from u0, lean ConsToPrim) are not built
MESH = (24, 20, 28)      # cell sizes that are no powers of two, several k-chunks of the x3 march
# 3-D Orszag-Tang starts from uniform density 25/(36 pi) and pressure 5/(12 pi): floors AT those values bind in every cell
# that a cycle leaves below them, i.e. in some cells but not in all
FLOORS = {"dfloor": 25.0/(36.0*math.pi), "pfloor": 5.0/(12.0*math.pi)}


class _Bare(str):
    """a deck value that parity_util's params (repr of the value) writes without quotes"""
    __repr__ = str.__str__


def _arrays(sim):
    ph = sim.phys
    d = pu.product_arrays(sim)
    d["w0"] = ph.w0.cpu().numpy()
    d["bcc0"] = ph.bcc0.cpu().numpy()
    return d


@functools.lru_cache(maxsize=None)
def _run(u0_sweeps, steps, integrator="rk2", floors=True):
    """3-D Orszag-Tang on MESH through the C++ host; steps = tuple of Execute(max_cycles) calls"""
    params = dict(FLOORS) if floors else {}
    if not u0_sweeps:
        params["u0_sweeps"] = _Bare("false")
    sim, _, _ = pu.make_pair("orszag_tang", MESH, 3, MESH, fused=True, native=True, params=params, cfl=0.3,
                             integrator=integrator)
    for n in steps:
        assert sim.Execute(max_cycles=n) == n
    nst = {"rk1": 1, "rk2": 2, "rk3": 3}[integrator]
    out = dict(arrays=_arrays(sim), counters=sim.floor_counters(), clock=(sim.time, sim.dt),
               forms=[sim.stage_forms(s) for s in range(1, nst + 1)])
    sim.close()
    return out


def _expected_forms(integrator):
    # the first stage is out of place anyway, the last one is made so; a stage in between keeps the old form
    # (rk3's stage 2: u1 has to survive it), with the full conversion before it as before every stage
    return {"rk1": [X3_U0], "rk2": [X3_U0, X3_U0], "rk3": [X3_U0, 0, X3_U0]}[integrator]


def test_identity_of_primitive_copies():
    """what the u0 form rests on: after a cycle in which the density and the energy floor bind, w0[dens] == u0[dens],
    w0[vel] == (1/u0[dens])*u0[mom] and bcc0 == the face averages, in every cell"""
    r = _run(True, (1,))
    assert r["counters"][0] > 0 and r["counters"][1] > 0, r["counters"]
    a = r["arrays"]
    u0, w0, bcc0 = a["u0"], a["w0"], a["bcc0"]
    assert np.array_equal(w0[:, 0], u0[:, 0])
    assert np.array_equal(w0[:, 1:4], (1.0/u0[:, 0])[:, None]*u0[:, 1:4])
    assert np.array_equal(bcc0[:, 0], 0.5*(a["b0x1f"][..., :-1] + a["b0x1f"][..., 1:]))
    assert np.array_equal(bcc0[:, 1], 0.5*(a["b0x2f"][..., :-1, :] + a["b0x2f"][..., 1:, :]))
    assert np.array_equal(bcc0[:, 2], 0.5*(a["b0x3f"][:, :-1] + a["b0x3f"][:, 1:]))


ORACLE_CASES = [
    # id, mesh, meshblock, integrator, floors
    ("24x20x28", MESH, MESH, "rk2", False),
    ("32^3", 32, 32, "rk2", False),
    ("32x16x16-2blocks", (32, 16, 16), 16, "rk2", False),
    ("rk1", MESH, MESH, "rk1", False),
    ("rk3", MESH, MESH, "rk3", False),
    ("floors", MESH, MESH, "rk2", True),
]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: c[0])
def test_against_oracle(case):
    _, n, mb, integrator, floors = case
    res = pu.compare_run("orszag_tang", n, 3, mb, cycles=3, fused=True, native=True, keep=True, cfl=0.3,
                         integrator=integrator, params=dict(FLOORS) if floors else None)
    sim = res["sim"]
    nst = len(_expected_forms(integrator))
    forms = [sim.stage_forms(s) for s in range(1, nst + 1)]
    counters = sim.floor_counters()
    sim.close()
    assert res["cycles"] == 3
    assert res["time"][0] == res["time"][1] and res["dt"][0] == res["dt"][1], (res["time"], res["dt"])
    assert res["bitwise_equal"], res["diffs"]
    assert forms == _expected_forms(integrator), forms
    if floors:
        assert counters[0] > 0 and counters[1] > 0, counters


def _same(a, b):
    assert a["clock"] == b["clock"], (a["clock"], b["clock"])
    assert a["counters"] == b["counters"], (a["counters"], b["counters"])
    for k in a["arrays"]:
        assert np.array_equal(a["arrays"][k], b["arrays"][k]), k


@pytest.mark.parametrize("integrator", ["rk2", "rk3"])
def test_new_against_old(integrator):
    """u0_sweeps = auto against false in one process: u0, b0, w0, bcc0, floor counters, (time, dt) after 3 cycles"""
    new, old = _run(True, (3,), integrator), _run(False, (3,), integrator)
    assert new["forms"] == _expected_forms(integrator), new["forms"]
    assert old["forms"] == [0]*len(old["forms"]), old["forms"]
    assert new["counters"][0] > 0 and new["counters"][1] > 0, new["counters"]
    _same(new, old)


def test_register_swaps_at_odd_count():
    """Execute(1) three times == Execute(3).  rk1 trades the registers once per cycle, so every call of one cycle ends on an
    odd number of trades and copies the state back; rk2 trades twice per cycle now (once before)"""
    for integrator in ("rk1", "rk2"):
        _same(_run(True, (1, 1, 1), integrator), _run(True, (3,), integrator))
