"""gpu: the two spellings of a call through the typed C ABI (athenak_amd/capi.py) launch the same kernel on the same
arguments: plain Python values as the product passes them, and C.byref / capi.d / capi._p as the tests spell them."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def test_rk_update_plain_and_explicit_arguments_agree_byte_for_byte():
    import torch
    from athenak_amd import capi
    L = capi.lib()
    nx, ng, nvar = 4, 2, 5
    n = nx + 2*ng
    gen = torch.Generator().manual_seed(20250)
    u0, u1, f1, f2, f3 = (torch.randn((1, nvar, n, n, n), dtype=torch.float64, generator=gen).cuda() for _ in range(5))
    dx = torch.full((1, 3), 1.0/nx, dtype=torch.float64).cuda()
    pack = capi.Pack(nmb=1, nvar=nvar, nx1=nx, nx2=nx, nx3=nx, ng=ng, dx=dx.data_ptr(), gamma=5.0/3.0, is_ideal=1)
    gam0, gam1, beta_dt = 0.25, 0.75, 0.0123

    plain = u0.clone()
    capi.check(L.akmi_rk_update(pack, gam0, gam1, beta_dt, plain, u1, f1, f2, f3, 0, capi._stream()), "rk_update")
    explicit = u0.clone()
    capi.check(L.akmi_rk_update(C.byref(pack), capi.d(gam0), capi.d(gam1), capi.d(beta_dt), capi._p(explicit), capi._p(u1),
                                capi._p(f1), capi._p(f2), capi._p(f3), 0, capi._stream()), "rk_update")
    torch.cuda.synchronize()
    assert not torch.equal(plain, u0)                       # the update ran
    assert torch.equal(plain.view(torch.int64), explicit.view(torch.int64))
