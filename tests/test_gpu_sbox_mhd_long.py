"""gpu: the reference's regression of the MHD shearing box (tst/test_suite/sbox/test_sbox_mhdshwave_mpicpu.py): the
compressible MHD shearing wave of the deck inputs/mhd_shwave.athinput to t = 3 at 16^3 in one block and at 32^3 in eight
blocks of 16^3, the user history column dByc every 0.01 against the 301 values of the linear solution the reference's test
holds (tests/golden/mhd_shwave_dbyc.json, numbers only), with the reference's own bars; and the growth rate of the
magnetorotational instability of the deck inputs/mri3d.athinput against linear theory."""
import json
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_gpu_sbox import read_hst  # noqa: E402

pytestmark = pytest.mark.gpu

TABLE = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "mhd_shwave_dbyc.json")))["dbyc"])


def run_shwave4(res, rundir):
    from athenak_amd.__main__ import main
    t0 = time.time()
    assert main(["-i", "mhd_shwave.athinput", "-d", str(rundir), "job/basename=shwave4", "mesh/nx1=%d" % res,
                 "mesh/nx2=%d" % res, "mesh/nx3=%d" % res, "meshblock/nx1=16", "meshblock/nx2=16", "meshblock/nx3=16"]) == 0
    h = read_hst(os.path.join(str(rundir), "shwave4.user.hst"))
    return h, time.time() - t0


MRI_BETA = 128.0*np.pi**2/15.0          # 2 pi v_A/L_z = sqrt(15)/4 with v_A^2 = 2 p0/(beta d0), p0 = d0 = L_z = 1: 84.2


def run_mri(rundir, tlim):
    """inputs/mri3d.athinput in a unit box of 16^3 cells in 1 x 2 x 1 blocks, uniform Bz with the fastest-growing channel
    mode at the wavelength L_z (k_z = 4 pi/L_z is stable), a fixed seed; returns the user history"""
    from athenak_amd.__main__ import main
    args = ["mesh/nx1=16", "mesh/nx2=16", "mesh/nx3=16", "mesh/x2min=-0.5", "mesh/x2max=0.5", "meshblock/nx1=16", "meshblock/nx2=8",
            "meshblock/nx3=16", "problem/ifield=2", "problem/beta=%r" % MRI_BETA, "problem/amp=1.0e-4", "problem/rseed=1",
            "time/tlim=%r" % tlim, "output1/dt=0.1", "output1/data_format=%20.12e"]
    assert main(["-i", "mri3d.athinput", "-d", str(rundir)] + args) == 0
    return read_hst(os.path.join(str(rundir), "mri3d.user.hst"))


@pytest.mark.parametrize("res,bar", [(16, 2.1e-8), (32, 6.2e-9)])
def test_mhd_shearing_wave_regression(res, bar, tmp_path, monkeypatch):
    """err = mean |dByc - table| over the 301 history lines; the bars are the reference's: 2.1e-8 at 16^3, 6.2e-9 at 32^3.
    Measured: err(16) = 2.009e-8, err(32) = 6.090e-9; 325 and 649 cycles, 0.3 s and 0.5 s."""
    monkeypatch.chdir(tmp_path)
    h, secs = run_shwave4(res, tmp_path/("run%d" % res))
    assert len(TABLE) == 301 and len(h["dByc"]) == 301 and abs(h["time"][-1] - 3.0) <= 1e-4
    err = float(np.abs(h["dByc"] - TABLE).mean())
    print("mhd shwave %d^3: err = %.4e, bar %.1e, %.1f s" % (res, err, bar, secs))
    assert err <= bar


MRI_WINDOW = (14.0, 17.0)
MRI_DEFICIT = 2.56e-3


def test_mri_growth_rate(tmp_path, monkeypatch):
    """The channel mode of wavelength L_z grows at the maximum rate of the instability, gamma = q Omega/2 = 0.75
    (Balbus & Hawley 1991), and the Maxwell stress dBxBy = -int Bx By dV at 2 gamma.  The slope of ln(dBxBy) is fitted by
    least squares over t in [14, 17], chosen from the run: the rate measured over half time units rises from 0.43 at t = 6
    (many modes, the fastest has not taken over) through 0.7431 at t = 13 and 0.7458 at t = 14 to a plateau of 0.7484 at
    t = 16.5-17, and falls from t = 19 (0.7345 at t = 20, 0.67 at t = 22); at t = 17 the perturbed field is 0.18 B0, at
    t = 18 it is 0.38 B0.  Measured over the window: gamma = 0.74744, a numerical deficit of 2.56e-3 (0.34 % of 0.75) at
    16 cells per wavelength with PPM4 + HLLD, about 1 200 cycles in 1.8 s.  Nothing grows faster than the fastest mode (2 %
    for the fit); twice the measured deficit below."""
    monkeypatch.chdir(tmp_path)
    h = run_mri(tmp_path/"run", 18.0)
    t, s = h["time"], h["dBxBy"]
    m = (t >= MRI_WINDOW[0] - 1e-9) & (t <= MRI_WINDOW[1] + 1e-9)
    assert m.sum() >= 29 and (s[m] > 0.0).all()
    gamma = float(np.polyfit(t[m], np.log(s[m]), 1)[0])/2.0
    ratio = float(np.sqrt((h["1-ME"][m][-1] + h["2-ME"][m][-1])/h["3-ME"][m][-1]))
    print("mri3d 16^3: gamma = %.5f over t in [%g, %g], deficit %.3e, |dB|/B0 at the end of the window %.3f"
          % (gamma, MRI_WINDOW[0], MRI_WINDOW[1], 0.75 - gamma, ratio))
    assert MRI_DEFICIT <= 0.2*0.75
    assert gamma <= 0.75*(1.0 + 0.02)
    assert gamma >= 0.75 - 2.0*MRI_DEFICIT
