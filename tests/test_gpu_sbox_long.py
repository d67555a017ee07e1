"""gpu: LONG run -- the reference's own regression of the hydro shearing box
(tst/test_suite/sbox/test_sbox_hydroshwave_mpicpu.py): the incompressible shearing wave of Johnson & Gammie (2005) at
32 x 32 x 4 and 64 x 64 x 4 (blocks of 32 x 32 x 4) up to t = 5, about 1 070 and 2 100 cycles of the task-granular chain
with orbital advection and the shear-periodic boundary.  The error of sqrt(32 KE1) against amp 17/(1 + (1.5 t - 4)^2),
averaged over the history lines, has to converge at second order and to stay below the reference's bar for its own
code; nothing tighter is asked.  The short form (t <= 1) is in tests/test_gpu_sbox.py."""
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_sbox import run_shwave, shwave_error  # noqa: E402


def test_incompressible_shearing_wave_converges(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    err = {}
    for res in (32, 64):
        err[res], n, _ = shwave_error(run_shwave(res, 5.0, tmp_path/("run%d" % res)))
        assert n == 51
    print("hydro shwave: err(32) = %.6e  err(64) = %.6e  ratio = %.4f  (bars: ratio <= 0.25, err(64) <= 1.6e-5)"
          % (err[32], err[64], err[64]/err[32]))
    assert err[64]/err[32] <= 0.25
    assert err[64] <= 1.6e-5
