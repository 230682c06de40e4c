"""What the ray-query tests share on the device (include/rt.h rt_trace_rays): the sentinel-filled output
buffers, one call helper and the bit comparison (tests/test_gpu_trace.py, tests/test_gpu_slab.py).  A
helper module, not a test: pytest does not rewrite its asserts, so every assert here carries its own
message."""
import math

import numpy as np
import torch

from gpu_support import DEV

INF, NAN = math.inf, math.nan
FIELDS = ("index", "t", "point", "normal", "front")
SENTINEL = dict(index=-7, t=12345.0, point=-54321.0, normal=777.0, front=0xAB)


class Out:
    """The five device outputs of `cap` rays, pre-filled with sentinels."""

    def __init__(self, cap):
        self.index = torch.full((cap,), SENTINEL["index"], dtype=torch.int32, device=DEV)
        self.t = torch.full((cap,), SENTINEL["t"], dtype=torch.float64, device=DEV)
        self.point = torch.full((cap, 3), SENTINEL["point"], dtype=torch.float64, device=DEV)
        self.normal = torch.full((cap, 3), SENTINEL["normal"], dtype=torch.float64, device=DEV)
        self.front = torch.full((cap,), SENTINEL["front"], dtype=torch.uint8, device=DEV)

    def ptrs(self, fields=FIELDS):
        return {"d_%s_ptr" % f: getattr(self, f).data_ptr() for f in fields}

    def host(self):
        return {f: getattr(self, f).cpu().numpy() for f in FIELDS}


def trace(r, O, D, t_min=1e-3, t_max=INF, iv=None, n=None, cap=None, stride=3, fields=FIELDS):
    """One rt_trace_rays call on the default stream: (outputs as numpy, [rays, scanned])."""
    n = len(O) if n is None else n
    o = np.zeros((len(O), stride or 3))  # stride 0 means 3
    d = np.zeros((len(O), stride or 3))
    o[:, :3], d[:, :3] = O, D
    if stride > 3:
        o[:, 3:], d[:, 3:] = NAN, NAN  # the padding lane of a Zig @Vector(3, f64) is never read
    d_o, d_d = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
    d_iv = torch.from_numpy(np.ascontiguousarray(iv)).to(DEV) if iv is not None else None
    out = Out(len(O) if cap is None else cap)
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)
    r.trace_rays(d_o.data_ptr(), d_d.data_ptr(), n, t_min, t_max, d_intervals_ptr=d_iv.data_ptr() if iv is not None else None,
                 d_stats_ptr=stats.data_ptr(), ray_stride=stride, **out.ptrs(fields))
    torch.cuda.synchronize()
    r.sync()  # reports a failure the kernel recorded
    return out.host(), stats.cpu().numpy().tolist()


def assert_equal(got, ref, n=None, fields=FIELDS, label=""):
    n = len(ref["index"]) if n is None else n
    for f in fields:
        assert np.array_equal(got[f][:n], ref[f][:n], equal_nan=(f == "normal")), \
            "%s: %s differs in %d of %d rays" % (label, f, int((got[f][:n] != ref[f][:n]).reshape(n, -1).any(axis=1).sum()), n)


def assert_sentinel(got, start, fields=FIELDS):
    for f in fields:
        assert (got[f][start:] == SENTINEL[f]).all(), "%s written past the last ray" % f
