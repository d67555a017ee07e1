"""gpu: <turb_driving> through the Python host and the kernels of csrc/akmi_turb.hip, against the restatement of
tests/turb_restate.py.  Every case runs in a process of its own under a time limit."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

PROLOGUE = r"""
import math, sys
import numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import turb_restate as R
from athenak_amd.main import Simulation, load_deck
from athenak_amd import turb_driver as TD
def active(t, ind):
    return t[..., ind.ks:ind.ke + 1, ind.js:ind.je + 1, ind.is_:ind.ie + 1].cpu().numpy()
# every global sum of the driver, with the per-MeshBlock partials it was formed from
CALLS = []
_gsum = TD.gid_ordered_sums
def _recorded(partial, pack):
    out = _gsum(partial, pack)
    CALLS.append((np.array(partial), out))
    return out
TD.gid_ordered_sums = _recorded
def close(a, ref_terms, rel=1e-13):
    return abs(a - math.fsum(ref_terms)) <= rel*max(math.fsum(np.abs(ref_terms)), 1e-300)
""" % (ROOT, os.path.join(ROOT, "tests"))


def _run(body, env=None, timeout=600):
    r = subprocess.run([sys.executable, "-c", PROLOGUE + body], env=dict(os.environ, **(env or {})),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "rc %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-5000:])
    return r.stdout


SYNTH = r"""
ov = %r
sim = Simulation(load_deck("turb_hydro.athinput", ov))
pm, pk = sim.pmesh, sim.pmesh.pmb_pack
pt, ind = pk.pturb, pm.mb_indcs
pt.InitializeModes(sim.pdriver, 0)
kvec, amp = R.amplitudes(R.Ran2(-1), pt.nlow, pt.nhigh, pt.driving_type, pt.expo, pt.exp_prp, pt.exp_prl, pt.lens)
bounds = [[s.x1min, s.x1max, s.x2min, s.x2max, s.x3min, s.x3max] for s in pk.pmb.mb_size]
tabs = R.tables(kvec, bounds, (ind.nx1, ind.nx2, ind.nx3))
raw = R.synthesize(amp, tabs)
(p1, (t0, t1, t2, t3)), (p2, (m0s, m1s)) = CALLS[0], CALLS[1]
want = np.stack([raw[:, 0] - t1/t0, raw[:, 1] - t2/t0, raw[:, 2] - t3/t0], axis=1)
got = active(pt.force_tmp, ind)
assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.abs(got - want).max()
# ghost zones untouched
ft = pt.force_tmp.cpu().numpy().copy()
ft[..., ind.ks:ind.ke + 1, ind.js:ind.je + 1, ind.is_:ind.ie + 1] = 0.0
assert not ft.any()
# per-MeshBlock partials against math.fsum over the block's own cells, and the global sums
rho = active(sim.phys.u0[:, 0], ind)
mom0 = active(sim.phys.u0[:, 1:4], ind)
for m in range(pk.nmb_thispack):
    for q, ref in enumerate([rho[m]] + [rho[m]*raw[m, c] for c in range(3)]):
        assert close(p1[m, q], ref.ravel()), (m, q, p1[m, q])
    assert close(p2[m, 0], (rho[m]*(want[m, 0]*want[m, 0] + want[m, 1]*want[m, 1] + want[m, 2]*want[m, 2])).ravel())
    assert close(p2[m, 1], (mom0[m, 0]*want[m, 0] + mom0[m, 1]*want[m, 1] + mom0[m, 2]*want[m, 2]).ravel())
for q, ref in enumerate([rho] + [rho*raw[:, c] for c in range(3)]):
    assert close((t0, t1, t2, t3)[q], ref.ravel()), q
assert close(m0s, (rho*(want[:, 0]*want[:, 0] + want[:, 1]*want[:, 1] + want[:, 2]*want[:, 2])).ravel())
# the energy injection relation m0 s^2 + m1 s = dedt (turb_driver.cpp:781-804)
m0c = max(m0s, 1e-20); m1c = max(m1s, 1e-20)
dvol = 1.0/(pm.mesh_indcs.nx1*pm.mesh_indcs.nx2*pm.mesh_indcs.nx3)
M0, M1 = 0.5*m0c*dvol*pm.dt, m1c*dvol
assert abs(M0*pt.s*pt.s + M1*pt.s - pt.dedt) <= 1e-12*pt.dedt, (M0, M1, pt.s)
pt.AddForcing(sim.pdriver, 0)
mom = active(sim.phys.u0[:, 1:4], ind)
assert np.count_nonzero(mom) > 0
for c in range(3):
    assert abs(math.fsum(mom[:, c].ravel())) <= 1e-12*math.fsum(np.abs(mom).ravel())
print("ok", pt.nmode, pt.s)
"""


@pytest.mark.parametrize("ov", [
    ["mesh/nx1=64", "mesh/nx2=64", "mesh/nx3=64", "meshblock/nx1=32", "meshblock/nx2=32", "meshblock/nx3=32"],
    ["mesh/nx1=64", "mesh/nx2=64", "mesh/nx3=64", "meshblock/nx1=32", "meshblock/nx2=32", "meshblock/nx3=32",
     "turb_driving/driving_type=1"],
    ["mesh/nx1=64", "mesh/nx2=32", "mesh/nx3=1", "meshblock/nx1=32", "meshblock/nx2=16", "meshblock/nx3=1"],
    ["mesh/nx1=48", "mesh/nx2=32", "mesh/nx3=16", "meshblock/nx1=24", "meshblock/nx2=8", "meshblock/nx3=16",
     "turb_driving/driving_type=1", "turb_driving/nhigh=3"],
], ids=["3d_64_iso", "3d_64_aniso", "2d_nocube", "3d_nocube_aniso"])
def test_synthesis_reductions_and_scale(ov):
    assert "ok" in _run(SYNTH % (ov + ["time/nlim=1"],))


def test_physics_from_rest_one_cycle():
    """hydro at rest, white noise, RK1: the stage's update of u1 carries no flux (uniform state), so after one cycle the
    momentum is the push of before_timeintegrator with the net momentum removed.  Per-cell arithmetic bit for bit (with the
    driver's own global sums), the global sums within 1e-13 of math.fsum"""
    out = _run(r"""
sim = Simulation(load_deck("turb_hydro.athinput", ["turb_driving/tcorr=0.0", "time/integrator=rk1", "time/nlim=1"]))
pm, pk = sim.pmesh, sim.pmesh.pmb_pack
ind, pt = pm.mb_indcs, pk.pturb
dt = pm.dt
sim.Execute(1)
assert len(CALLS) == 4                  # synthesis, moments, AddForcing (before the stages), AddForcing (stage 1)
got = active(sim.phys.u0[:, 1:4], ind)
rho = np.ones_like(got[:, 0])
kvec, amp = R.amplitudes(R.Ran2(-1), 1, 2, 0, 5.0/3.0, 5.0/3.0, 0.0, pt.lens)
bounds = [[s.x1min, s.x1max, s.x2min, s.x2max, s.x3min, s.x3max] for s in pk.pmb.mb_size]
raw = R.synthesize(amp, R.tables(kvec, bounds, (ind.nx1, ind.nx2, ind.nx3)))
T = CALLS[0][1]
f = np.stack([raw[:, c] - T[c + 1]/T[0] for c in range(3)], axis=1)
m0, m1 = CALLS[1][1]
assert close(m0, (rho*(f[:, 0]*f[:, 0] + f[:, 1]*f[:, 1] + f[:, 2]*f[:, 2])).ravel()) and m1 == 0.0
s = TD.scale_factor(m0, m1, 0.1, dt, (32, 32, 32))
s_fsum = TD.scale_factor(math.fsum((rho*(f[:, 0]*f[:, 0] + f[:, 1]*f[:, 1] + f[:, 2]*f[:, 2])).ravel()), 0.0, 0.1, dt,
                         (32, 32, 32))
assert s == pt.s and abs(s - s_fsum) <= 1e-13*s
push = np.stack([0.0 + rho*(0.0*0.0 + 1.0*(f[:, c]*s))*dt for c in range(3)], axis=1)
P = CALLS[2][1]
assert close(P[0], rho.ravel()) and all(close(P[c + 1], push[:, c].ravel()) for c in range(3))
want = np.stack([push[:, c] - rho*P[c + 1]/P[0] for c in range(3)], axis=1)
assert np.count_nonzero(got) == got.size
assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.abs(got - want).max()
assert np.array_equal(active(sim.phys.u0[:, 0], ind), rho)
print("ok", np.abs(got).max())
""")
    assert "ok" in out


RUN = r"""
ov = %r
sim = Simulation(load_deck(%r, ov))
pk, ph = sim.pmesh.pmb_pack, sim.phys
# stage 1 must have copied u0 (b0) into the second register BEFORE the stage's AddForcing changes u0: the fused and the
# out-of-place first stages fold that copy into the update, and would leave u1 behind here
task = [t for t in pk.tl_map["stagen"].task_list_ if getattr(t.func_, "__func__", None) is TD.TurbulenceDriver.AddForcing]
assert len(task) == 1
orig, seen = task[0].func_, []
def bits(t):
    return t.contiguous().view(torch.int64)
def checked(d, stage):
    if stage == 1:
        ok = torch.equal(bits(ph.u1), bits(ph.u0))
        if pk.pmhd is not None:
            ok = ok and all(torch.equal(bits(getattr(ph.b1, a)), bits(getattr(ph.b0, a))) for a in ("x1f", "x2f", "x3f"))
        seen.append(ok)
    return orig(d, stage)
task[0].func_ = checked
sim.Execute(%d)
assert len(seen) == %d and all(seen), seen
np.save(%r, torch.cat([ph.u0.flatten().cpu()] + ([ph.b0.x1f.flatten().cpu(), ph.b0.x2f.flatten().cpu(),
        ph.b0.x3f.flatten().cpu()] if pk.pmhd is not None else [])).numpy())
print("ok", sim.pmesh.time)
"""


@pytest.mark.parametrize("deck", ["turb_hydro.athinput", "turb_mhd.athinput"])
def test_stage_one_copies_before_forcing(deck, tmp_path):
    """RK2: at every stage-1 AddForcing the second register holds u0 (and b0) as they were before it, whatever
    fused_stage says and with the first stage in place (AKMI_TASK_OOP=0, AKMI_OUT_OF_PLACE=0); the results agree"""
    blk = "mhd" if "mhd" in deck else "hydro"
    cases = [([], None), (["%s/fused_stage=true" % blk], None), (["%s/fused_stage=false" % blk],
                                                                  {"AKMI_TASK_OOP": "0", "AKMI_OUT_OF_PLACE": "0"})]
    res = []
    for n, (ov, env) in enumerate(cases):
        f = str(tmp_path / ("r%d.npy" % n))
        _run(RUN % (ov + ["time/nlim=20", "time/integrator=rk2"], deck, 5, 5, f), env=env)
        res.append(np.load(f))
    for r in res[1:]:
        assert np.array_equal(r.view(np.uint64), res[0].view(np.uint64))
    assert np.isfinite(res[0]).all()


def test_driven_mhd_run_stays_sound():
    """isothermal MHD 64^3 (2x2x2 MeshBlocks), dedt = 0.1, tcorr = 0.5 to t = 2: kinetic energy grows from zero, the
    density floor is never hit (the ConsToPrim counters), div B at round-off.  (Isothermal: the push changes the momentum
    and not the energy, as the reference's does, so with an ideal gas the kinetic energy it adds comes out of the internal
    energy, and at this dedt and tcorr the energy floor is hit within t = 2.)"""
    out = _run(r"""
sim = Simulation(load_deck("turb_mhd.athinput", ["mhd/eos=isothermal", "time/tlim=2.0", "mesh/nx1=64", "mesh/nx2=64", "mesh/nx3=64",
                                                "meshblock/nx1=32", "meshblock/nx2=32", "meshblock/nx3=32"]))
pm, ph = sim.pmesh, sim.phys
ind = pm.mb_indcs
def ke():
    u = active(ph.u0, ind)
    return float((0.5*(u[:, 1]**2 + u[:, 2]**2 + u[:, 3]**2)/u[:, 0]).sum())
assert ph.nvars == 4 and ke() == 0.0
sim.Execute(20)
k1 = ke()
sim.Execute()
k2 = ke()
assert abs(pm.time - 2.0) < 1e-12 and 0.0 < k1 < k2, (pm.time, k1, k2)
u = active(ph.u0, ind)
assert np.isfinite(u).all()
assert ph.counters.cpu().tolist() == [0, 0, 0], ph.counters.cpu().tolist()     # dfloor, efloor, tfloor
b1, b2, b3 = (x.cpu().numpy() for x in (ph.b0.x1f, ph.b0.x2f, ph.b0.x3f))
ks, js, is_ = slice(ind.ks, ind.ke + 1), slice(ind.js, ind.je + 1), slice(ind.is_, ind.ie + 1)
dx = 1.0/pm.mesh_indcs.nx1
div = ((b1[:, ks, js, ind.is_ + 1:ind.ie + 2] - b1[:, ks, js, is_]) + (b2[:, ks, ind.js + 1:ind.je + 2, is_] - b2[:, ks, js, is_])
       + (b3[:, ind.ks + 1:ind.ke + 2, js, is_] - b3[:, ks, js, is_]))/dx
assert np.abs(div).max() < 1e-11, np.abs(div).max()
print("ok", pm.time, pm.ncycle, k1, k2)
""", timeout=1200)
    assert "ok" in out


# ---- several ranks --------------------------------------------------------------------
RANKS = r"""
import os
import torch.distributed as dist
import torch.multiprocessing as mp

def worker(rank, world, port, deck, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    sim = Simulation(load_deck(deck, ["time/nlim=10"]), my_rank=rank, nranks=world)
    sim.Execute(10)
    pk, ph = sim.pmesh.pmb_pack, sim.phys
    arrs = [ph.u0, pk.pturb.force] + ([ph.b0.x1f, ph.b0.x2f, ph.b0.x3f] if pk.pmhd is not None else [])
    for n, a in enumerate(arrs):
        np.save("%s/a%d_g%d.npy" % (out, n, pk.gids), a.cpu().numpy())
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()

if __name__ == "__main__":
    world, port, deck, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    mp.spawn(worker, args=(world, port, deck, out), nprocs=world, join=True)
    print("ok")
"""


def _gather(d, nmb_total):
    """the arrays of all MeshBlocks in gid order from the per-rank files of directory d"""
    files = sorted(os.listdir(d))
    out = []
    for n in sorted({f.split("_")[0] for f in files}):
        parts = sorted((int(f.split("_g")[1][:-4]), f) for f in files if f.startswith(n + "_"))
        out.append(np.concatenate([np.load(os.path.join(d, f)) for _, f in parts]))
        assert out[-1].shape[0] == nmb_total
    return out


@pytest.mark.parametrize("deck,worlds", [("turb_mhd.athinput", (2, 4, 8)), ("turb_hydro.athinput", (2, 8))])
def test_ranks_match_single_process(deck, worlds, tmp_path):
    """2, 4 and 8 ranks sharing the GPU (halos and the driver's all-reduce over gloo) give the bits of one process: the
    global sums of the driver are the per-MeshBlock partials added in gid order whatever the rank layout"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_distributed_gloo import _free_port
    script = tmp_path / "ranks.py"
    script.write_text(PROLOGUE + RANKS)
    res = {}
    for world in (1,) + worlds:
        d = tmp_path / ("w%d" % world)
        d.mkdir()
        r = subprocess.run([sys.executable, str(script), str(world), str(_free_port()), deck, str(d)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "ok" in r.stdout, (world, r.stdout[-2000:], r.stderr[-4000:])
        res[world] = _gather(str(d), 8)
    for world in worlds:
        for a, b in zip(res[world], res[1]):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), world
    assert np.count_nonzero(res[1][1]) > 0
