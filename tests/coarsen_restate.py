"""The coarsened binary output restated in numpy, and an independent parser of the .cbin layout.

restate(): the mean over f x f x f fine cells and, with moments, of x*x, (x*x)*x, ((x*x)*x)*x.  Explicit loops over the
offset (kk, jj, ii) inside a coarse cell, in that order with ii fastest, vectorised over the coarse cells: every
accumulator starts at +0.0, takes one term per step and is divided by float(f*f*f) at the end.  numpy rounds every
elementwise product and sum separately, so the result is the sequence of roundings the issue defines.

parse_cbin(): written from the description of the format (the text pre-header of nine "key=value" lines after the version
line, the variable list, "header offset=", the parameter dump; per MeshBlock 10 int32, 6 float64, then nvars*nmom arrays of
float32 [k][j][i] whose extents follow from the six indices), not from the writer."""
import struct

import numpy as np


def restate(a, f, lo, nc, moments):
    """a: (..., N3, N2, N1) float64; lo = (ois, ojs, oks); nc = (nc1, nc2, nc3).  Returns (nmom, ..., nc3, nc2, nc1)."""
    lead = a.shape[:-3]
    nmom = 4 if moments else 1
    acc = [np.zeros(lead + (nc[2], nc[1], nc[0])) for _ in range(nmom)]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for kk in range(f):
            for jj in range(f):
                for ii in range(f):
                    x = a[..., lo[2] + kk:lo[2] + kk + nc[2]*f:f, lo[1] + jj:lo[1] + jj + nc[1]*f:f,
                          lo[0] + ii:lo[0] + ii + nc[0]*f:f]
                    acc[0] = acc[0] + x
                    if moments:
                        x2 = x*x
                        x3 = x2*x
                        x4 = x3*x
                        acc[1] = acc[1] + x2
                        acc[2] = acc[2] + x3
                        acc[3] = acc[3] + x4
        cube = float(f*f*f)
        return np.stack([s/cube for s in acc])


def restate_vars(arrays, f, lo, nc, moments):
    """arrays: list of (nmb, N3, N2, N1), one per output variable -> (nvars*nmom, nmb, nc3, nc2, nc1), the moments of a
    variable adjacent"""
    r = restate(np.stack(arrays), f, lo, nc, moments)            # (nmom, nvars, nmb, nc3, nc2, nc1)
    return np.ascontiguousarray(np.moveaxis(r, 0, 1)).reshape((-1,) + r.shape[2:])


def parse_cbin(path):
    """dict: version line, the pre-header as {key: text}, names, dump (text), blocks = [(index[6], logical[4],
    geometry[6], data (nvars, n3, n2, n1) float32)]"""
    blob = open(path, "rb").read()
    pos = 0

    def line():
        nonlocal pos
        end = blob.index(b"\n", pos)
        text = blob[pos:end].decode("ascii")
        pos = end + 1
        return text
    out = {"version": line()}
    first = line()
    assert first.startswith("  size of preheader="), first
    npre = int(first.split("=")[1])
    pre = {}
    order = []
    for _ in range(npre - 1):
        key, val = line().split("=")
        assert key.startswith("  ")
        pre[key.strip()] = val
        order.append(key.strip())
    out["preheader"], out["preheader_order"] = pre, order
    nvline = line()
    assert nvline.startswith("  number of variables="), nvline
    out["nvars"] = int(nvline.split("=")[1])
    vline = line()
    assert vline.startswith("  variables:  "), vline
    out["variables_line"] = vline
    out["names"] = vline[len("  variables:  "):].split()
    off = line()
    assert off.startswith("  header offset="), off
    n = int(off.split("=")[1])
    out["dump"] = blob[pos:pos + n].decode("ascii")
    pos += n
    blocks = []
    while pos < len(blob):
        idx = struct.unpack_from("<6i", blob, pos)
        logical = struct.unpack_from("<4i", blob, pos + 24)
        geom = struct.unpack_from("<6d", blob, pos + 40)
        pos += 88
        n1, n2, n3 = idx[1] - idx[0] + 1, idx[3] - idx[2] + 1, idx[5] - idx[4] + 1
        cnt = out["nvars"]*n3*n2*n1
        data = np.frombuffer(blob, dtype="<f4", count=cnt, offset=pos).reshape(out["nvars"], n3, n2, n1)
        pos += 4*cnt
        blocks.append((idx, logical, geom, data))
    assert pos == len(blob)
    out["blocks"] = blocks
    return out
