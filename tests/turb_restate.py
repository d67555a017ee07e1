"""CPU restatement of the turbulence driver (numpy + math), written from the published algorithms and the formulas of
src/srcterms/turb_driver.cpp, independent of csrc/akmi_turb.hip:
  Ran2          L'Ecuyer's combined generator with the Bays-Durham shuffle (Numerical Recipes ran2), Python integers
  gaussian      Marsaglia's polar Box-Muller on Ran2, the second deviate cached in the state
  modes         mode list and amplitude table of InitializeModes (turb_driver.cpp:389-604)
  tables        sin/cos of k*x at the cell centres (turb_driver.cpp:226-270)
  synthesize    force_tmp, each term ((amp*xt)*yt)*zt added in the reference's order from 0.0
"""
import math
import sys

import numpy as np

NTAB = 32
IM1, IM2 = 2147483563, 2147483399
IA1, IA2, IQ1, IQ2, IR1, IR2 = 40014, 40692, 53668, 52774, 12211, 3791
IMM1 = IM1 - 1
NDIV = 1 + IMM1//NTAB
AM = 1.0/IM1
RNMX = 1.0 - sys.float_info.epsilon


def _trunc_div(a, b):
    """C integer division (truncation toward zero)"""
    q = abs(a)//abs(b)
    return q if (a >= 0) == (b >= 0) else -q


class Ran2:
    def __init__(self, idum=-1):
        self.idum, self.idum2, self.iy, self.iv = idum, 123456789, 0, [0]*NTAB
        self.iset, self.gset = 0, 0.0

    def _schrage1(self, x):
        k = _trunc_div(x, IQ1)
        x = IA1*(x - k*IQ1) - k*IR1
        return x + IM1 if x < 0 else x

    def uniform(self):
        if self.idum <= 0:
            self.idum2, self.iy = 123456789, 0
            self.idum = 1 if -self.idum < 1 else -self.idum
            self.idum2 = self.idum
            for j in range(NTAB + 7, -1, -1):
                self.idum = self._schrage1(self.idum)
                if j < NTAB:
                    self.iv[j] = self.idum
            self.iy = self.iv[0]
        self.idum = self._schrage1(self.idum)
        k = _trunc_div(self.idum2, IQ2)
        self.idum2 = IA2*(self.idum2 - k*IQ2) - k*IR2
        if self.idum2 < 0:
            self.idum2 += IM2
        j = _trunc_div(self.iy, NDIV)
        self.iy = self.iv[j] - self.idum2
        self.iv[j] = self.idum
        if self.iy < 1:
            self.iy += IMM1
        t = AM*float(self.iy)
        return RNMX if t > RNMX else t

    def gaussian(self):
        if self.idum < 0:
            self.iset = 0
        if self.iset == 0:
            while True:
                v1 = 2.0*self.uniform() - 1.0
                v2 = 2.0*self.uniform() - 1.0
                rsq = v1*v1 + v2*v2
                if not (rsq >= 1.0 or rsq == 0.0):
                    break
            fac = math.sqrt(-2.0*math.log(rsq)/rsq)
            self.gset, self.iset = v1*fac, 1
            return v2*fac
        self.iset = 0
        return self.gset


def mode_list(nlow, nhigh, driving_type):
    out = []
    lo, hi = nlow*nlow, nhigh*nhigh
    for nkx in range(nhigh + 1):
        for nky in range(nhigh + 1):
            for nkz in range(nhigh + 1):
                if nkx == 0 and nky == 0 and nkz == 0:
                    continue
                if driving_type == 0:
                    ok = lo <= nkx*nkx + nky*nky + nkz*nkz <= hi
                else:
                    ok = lo <= nkx*nkx + nky*nky <= hi and lo <= nkz*nkz <= hi
                if ok:
                    out.append((nkx, nky, nkz))
    return out


NAMES = [c + t for c in "xyz" for t in ("ccc", "ccs", "csc", "css", "scc", "scs", "ssc", "sss")]


def amplitudes(rng, nlow, nhigh, driving_type, expo, exp_prp, exp_prl, lens):
    """one draw: (kvec [n,3], amp [n,24]) in the order NAMES"""
    dkx, dky, dkz = (2.0*math.pi/L for L in lens)
    ks, amps = [], []
    for nkx, nky, nkz in mode_list(nlow, nhigh, driving_type):
        kx, ky, kz = dkx*nkx, dky*nky, dkz*nkz
        a = dict.fromkeys(NAMES, 0.0)
        g = rng.gaussian
        if driving_type == 0:
            kiso = math.sqrt(kx*kx + ky*ky + kz*kz)
            norm = 1.0/math.pow(kiso, (expo + 2.0)/2.0) if kiso > 1e-16 else 0.0
            if nkz != 0:
                ikz = 1.0/(dkz*float(nkz))
                for c in "xy":
                    a[c + "ccc"] = g()
                    a[c + "ccs"] = g()
                    a[c + "csc"] = 0.0 if nky == 0 else g()
                    a[c + "css"] = 0.0 if nky == 0 else g()
                    a[c + "scc"] = 0.0 if nkx == 0 else g()
                    a[c + "scs"] = 0.0 if nkx == 0 else g()
                    a[c + "ssc"] = 0.0 if (nkx == 0 or nky == 0) else g()
                    a[c + "sss"] = 0.0 if (nkx == 0 or nky == 0) else g()
                a["zccc"] = ikz*(kx*a["xscs"] + ky*a["ycss"])
                a["zccs"] = -ikz*(kx*a["xscc"] + ky*a["ycsc"])
                a["zcsc"] = ikz*(kx*a["xsss"] - ky*a["yccs"])
                a["zcss"] = ikz*(-kx*a["xssc"] + ky*a["yccc"])
                a["zscc"] = ikz*(-kx*a["xccs"] + ky*a["ysss"])
                a["zscs"] = ikz*(kx*a["xccc"] - ky*a["yssc"])
                a["zssc"] = -ikz*(kx*a["xcss"] + ky*a["yscs"])
                a["zsss"] = ikz*(kx*a["xcsc"] + ky*a["yscc"])
            elif nky != 0:
                iky = 1.0/(dky*float(nky))
                for c in "xz":
                    a[c + "ccc"] = g()
                    a[c + "csc"] = g()
                    a[c + "scc"] = 0.0 if nkx == 0 else g()
                    a[c + "ssc"] = 0.0 if nkx == 0 else g()
                a["yccc"] = iky*kx*a["xssc"]
                a["ycsc"] = -iky*kx*a["xscc"]
                a["yscc"] = -iky*kx*a["xcsc"]
                a["yssc"] = iky*kx*a["xccc"]
            else:
                a["zccc"] = g()
                a["zscc"] = g()
                a["yccc"] = g()
                a["yscc"] = g()
        else:
            kprl = math.sqrt(kx*kx)
            kprp = math.sqrt(ky*ky + kz*kz)
            norm = (1.0/math.pow(kprp, (exp_prp + 1.0)/2.0)/math.pow(kprl, exp_prl/2.0)
                    if (kprl > 1e-16 and kprp > 1e-16) else 0.0)
            if nky != 0:
                iky = 1.0/(dky*float(nky))
                for t in ("ccc", "ccs", "csc", "css"):
                    a["x" + t] = g()
                for t in ("scc", "scs", "ssc", "sss"):
                    a["x" + t] = 0.0 if nkx == 0 else g()
                a["yccc"] = iky*(kx*a["xssc"])
                a["yccs"] = iky*(kx*a["xsss"])
                a["ycsc"] = -iky*(kx*a["xscc"])
                a["ycss"] = -iky*(kx*a["xscs"])
                a["yscc"] = -iky*(kx*a["xcsc"])
                a["yscs"] = -iky*(kx*a["xcss"])
                a["yssc"] = iky*(kx*a["xccc"])
                a["ysss"] = iky*(kx*a["xccs"])
            else:
                a["yccc"] = g()
                a["yscc"] = g()
        ks.append((kx, ky, kz))
        amps.append([a[n]*norm for n in NAMES])
    return np.array(ks, dtype=np.float64).reshape(-1, 3), np.array(amps, dtype=np.float64).reshape(-1, 24)


def cell_center(ith, n, xmin, xmax):
    x = (float(ith) + 0.5)/float(n)
    return (x*xmax - x*xmin) - (0.5*xmax - 0.5*xmin) + (0.5*xmin + 0.5*xmax)


def tables(kvec, bounds, nx):
    """[(sin, cos)] per direction, each [nmb, nmode, nx_d]"""
    nmb, nmode = len(bounds), len(kvec)
    out = []
    for d in range(3):
        s = np.zeros((nmb, nmode, nx[d]))
        c = np.ones((nmb, nmode, nx[d]))
        if d == 0 or nx[d] > 1:
            for m in range(nmb):
                for n in range(nmode):
                    for i in range(nx[d]):
                        x = cell_center(i, nx[d], bounds[m][2*d], bounds[m][2*d + 1])
                        s[m, n, i] = math.sin(kvec[n][d]*x)
                        c[m, n, i] = math.cos(kvec[n][d]*x)
        out.append((s, c))
    return out


def synthesize(amp, tabs):
    """force_tmp over the active cells: [nmb, 3, nx3, nx2, nx1]"""
    (xs, xc), (ys, yc), (zs, zc) = tabs
    nmb, nmode = xs.shape[0], xs.shape[1]
    nx1, nx2, nx3 = xs.shape[2], ys.shape[2], zs.shape[2]
    f = np.zeros((nmb, 3, nx3, nx2, nx1))
    for m in range(nmb):
        for n in range(nmode):
            xt = (xc[m, n][None, None, :], xs[m, n][None, None, :])
            yt = (yc[m, n][None, :, None], ys[m, n][None, :, None])
            zt = (zc[m, n][:, None, None], zs[m, n][:, None, None])
            for d in range(3):
                for t in range(8):
                    f[m, d] += ((amp[n, 8*d + t]*xt[t >> 2])*yt[(t >> 1) & 1])*zt[t & 1]
    return f


def divergence_coefficients(kvec, amp):
    """for each mode the 8 coefficients of div f on the trig basis (x-, y-, z-trig sin/cos): zero for an
    incompressible force.  d/dx cos(kx) = -k sin(kx), d/dx sin(kx) = k cos(kx)"""
    out = np.zeros((len(kvec), 8))
    scale = np.zeros(len(kvec))
    for n, (kx, ky, kz) in enumerate(kvec):
        for d, (k, bit) in enumerate(((kx, 4), (ky, 2), (kz, 1))):
            for t in range(8):
                a = amp[n, 8*d + t]
                sign = 1.0 if t & bit else -1.0
                out[n, t ^ bit] += sign*k*a
                scale[n] = max(scale[n], abs(k*a))
    return out, scale
