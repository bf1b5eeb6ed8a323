"""include/mpcekf.h's limit-map rule (mpcekf_limit_map) restated in numpy: one numpy operation per
separately rounded fp64 operation, in the header's order.  Shared by the CPU property tests
(tests/test_limit_map_ref.py) and the GPU parity tests (tests/test_gpu_limit_map.py)."""
import numpy as np


def axis(a, lo, hi, m):
    """One axis of the lookup on a uniform grid of m >= 2 nodes: (j, f, clamped) per cell."""
    with np.errstate(all="ignore"):
        x = (a - lo) / (hi - lo)
        xc = np.where(x > 0.0, x, 0.0)      # NaN -> 0
        xc = np.where(xc < 1.0, xc, 1.0)
        s = xc * float(m - 1)
        j = np.minimum(s.astype(np.int64), m - 2)
        f = s - j.astype(np.float64)
        return j, f, ~((x >= 0.0) & (x <= 1.0))


def map_eval(z, T, z_lo, z_hi, T_lo, T_hi, tab, sets=None, interp_z=0):
    """tab [nz], [nt][nz] or [nsets][nt][nz] -> (val [n], clamped_z [n], clamped_T [n]).
    z [n]: the soc row of the previous step; T [n] (degC; ignored, may be None, with nt == 1)."""
    tab = np.asarray(tab, dtype=np.float64)
    tab = tab.reshape((1,) * (3 - tab.ndim) + tab.shape)
    _, nt, nz = tab.shape
    z = np.asarray(z, dtype=np.float64)
    n = z.shape[0]
    t = tab[np.zeros(n, dtype=int) if sets is None else np.asarray(sets)]     # [n][nt][nz]
    c = np.arange(n)
    with np.errstate(all="ignore"):
        if nz > 1:
            jz, fz, cz = axis(z, z_lo, z_hi, nz)
            if interp_z:
                fz = np.zeros(n)
        else:
            jz = np.zeros(n, dtype=np.int64)
            xz = (z - z_lo) / (z_hi - z_lo)
            cz = ~((xz >= 0.0) & (xz <= 1.0))
        if nt > 1:
            jt, ft, ct = axis(np.asarray(T, dtype=np.float64), T_lo, T_hi, nt)
        else:
            jt, ct = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)

        def along_z(j_t):
            a = t[c, j_t, jz]
            return a + fz * (t[c, j_t, jz + 1] - a) if nz > 1 else a

        a = along_z(jt)
        val = a + ft * (along_z(jt + 1) - a) if nt > 1 else a
    return val, cz, ct


class Record:
    """The map's per-cell record as the fused loop keeps it: z_last, neval, nclamp_z, nclamp_t."""

    def __init__(self, z0):
        z0 = np.asarray(z0, dtype=np.float64)
        self.z_last = z0.copy()
        self.neval = np.zeros(z0.shape[0])
        self.nclamp_z = np.zeros(z0.shape[0])
        self.nclamp_t = np.zeros(z0.shape[0])

    def evaluate(self, T, z_lo, z_hi, T_lo, T_hi, tabs, sets=None, interp_z=0):
        """One fused step's evaluation at z_last and T: {field: val [n]}; the counts advance once."""
        out = {}
        for k, tab in tabs.items():
            out[k], cz, ct = map_eval(self.z_last, T, z_lo, z_hi, T_lo, T_hi, tab, sets, interp_z)
        self.neval += 1.0
        self.nclamp_z += cz
        self.nclamp_t += ct
        return out

    def store(self, soc_row):
        """The end of a fused step: its soc row becomes z_last."""
        self.z_last = np.asarray(soc_row, dtype=np.float64).copy()

    def as_dict(self):
        return dict(z_last=self.z_last, neval=self.neval, nclamp_z=self.nclamp_z, nclamp_t=self.nclamp_t)
