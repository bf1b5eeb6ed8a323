"""Shared by tests/test_gpu_limits.py: the heterogeneous batches of the per-cell limits tests
(mpcekf_set_limits) and their C-oracle reference, run once per group of cells.

A group is a dict of oracle_c.run keywords (oracle_c.DEFAULTS' names) that differ from the
defaults; cell c of a batch gets group c % G, so every wave mixes groups.  The values were
checked on the CPU oracle (193 cells of batch_inputs at Np = 5 over 400 steps, 70 at Np = 20
over 200) to bind within the tests' horizons:

  phise_min 0.10   every cell differs from the defaults at Np = 5, 46 of 70 at Np = 20
  v_max 3.9        (4.0 does not bind at Np = 20 within 200 steps)
  Crate 3          u_min = -Q Crate: from step 0, and Hildreth into maxIter
  target_soc 80    from step 0 (mpcData.ref enters e and F)
  du_max 5         from step 0 (the rate rows and Ru)
  du_min -5        from step 0 (the first steps ramp the current down)
  u_max -55        u_min = -59.7 A: the current is boxed into [-59.7, -55] (-5 never binds)
  z_max 0.33       a few percent above the largest SOC0 (30 %): the SOC rows bind
  several          z_max 0.31 + z_tol 0.02 (zmax = 0.33; without z_tol the run differs:
                   test_oracle_floors), Crate 3, phise_min 0.09
"""
import functools

import numpy as np

import oracle_c
from conftest import batch_inputs

GROUPS = (
    dict(phise_min=0.10),
    dict(v_max=3.9),
    dict(Crate=3.0),
    dict(ref=80.0),
    dict(du_max=5.0),
    dict(du_min=-5.0),
    dict(u_max=-55.0),
    dict(z_max=0.33),
    dict(z_max=0.31, z_tol=0.02, Crate=3.0, phise_min=0.09),
)
G = len(GROUPS)
# oracle keyword -> Context.set_limits keyword / mpcekf_config field
FIELD = dict(ref="target_soc", Crate="Crate", u_max="u_max", du_min="du_min", du_max="du_max", v_max="v_max",
             phise_min="phise_min", z_max="z_max", z_tol="z_tol")
# the constraint block (bit of the mask: 0 useCurrent, 1 useVoltage, 2 useEta) a field enters the
# problem through; None: through e / F / Ru or the SOC rows, which no switch removes
BLOCK = dict(ref=None, du_max=None, z_max=None, z_tol=None, Crate=0, u_max=0, du_min=0, v_max=1, phise_min=2)
TRAJ = ("u", "v", "soc", "phise", "nexec", "J_unc", "J_fin", "norm_du", "nviol")


def pick(sel=None):
    return GROUPS if sel is None else tuple(GROUPS[i] for i in sel)


def active(group, mask):
    """Does any field the group changes enter the problem under the constraint mask?"""
    return any(BLOCK[k] is None or mask[BLOCK[k]] for k in group)


def group_of(n, groups=GROUPS):
    return np.arange(n) % len(groups)


def limit_arrays(n, groups=GROUPS):
    """{set_limits keyword: [n]} for cell c in group c % G: all nine fields, the defaults where
    the cell's group does not change one."""
    g = group_of(n, groups)
    out = {}
    for k, name in FIELD.items():
        vals = np.array([float(grp.get(k, oracle_c.DEFAULTS[k])) for grp in groups])
        out[name] = vals[g]
    return out


def uniform_arrays(n):
    """All nine fields as arrays constant at the defaults."""
    return {name: np.full(n, float(oracle_c.DEFAULTS[k])) for k, name in FIELD.items()}


def config_kwargs(group):
    """make_config keywords of a uniform context configured with the group's scalars."""
    return {FIELD[k]: v for k, v in group.items()}


@functools.lru_cache(maxsize=None)
def inputs(n):
    soc0, tc = batch_inputs(n)
    soc0.setflags(write=False)
    tc.setflags(write=False)
    return soc0, tc


def _freeze(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def oracle_default(kind, n, steps, Np=5, Nc=2, mask=(1, 1, 1), method="OB"):
    """The oracle under the default limits, all n cells (read-only, shared)."""
    soc0, tc = inputs(n)
    return _freeze(oracle_c.run(_rom(kind), soc0, tc, steps, nthreads=8, traj=True, Np=Np, Nc=Nc, constraints=mask,
                                method=method))


@functools.lru_cache(maxsize=None)
def oracle_groups(kind, n, steps, Np=5, Nc=2, mask=(1, 1, 1), method="OB", sel=None):
    """The oracle once per group on that group's cells, assembled into [steps, n] (status [n]).
    sel: indices into GROUPS (default all of them)."""
    soc0, tc = inputs(n)
    groups = pick(sel)
    g = group_of(n, groups)
    out = None
    for j, grp in enumerate(groups):
        idx = np.flatnonzero(g == j)
        o = oracle_c.run(_rom(kind), soc0[idx], tc[idx], steps, nthreads=8, traj=True, Np=Np, Nc=Nc, constraints=mask,
                         method=method, **grp)
        if out is None:
            out = {k: np.empty(v.shape[:-1] + (n,) if v.ndim == 2 else (n,), dtype=v.dtype)
                   for k, v in o.items() if k in TRAJ + ("status",)}
        for k in out:
            out[k][..., idx] = o[k]
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def _rom(kind):
    from importlib import import_module
    return import_module("mpc-ekf4fastcharge_amd").make_synth_rom(lookup=kind)


def bitwise(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} entries differ, first at {i}: {a[i]!r} vs {b[i]!r}")


def differs(a, b):
    """Per cell: does any compared output differ in a bit (NaN = NaN) between two oracle runs?"""
    d = np.zeros(a["status"].shape[0], dtype=bool)
    for k in TRAJ:
        x, y = a[k], b[k]
        same = (x == y) | (np.isnan(x) & np.isnan(y)) if x.dtype.kind == "f" else (x == y)
        d |= ~same.all(axis=0)
    return d | (a["status"] != b["status"])
