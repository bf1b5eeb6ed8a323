"""The per-cell charge summary (include/mpcekf.h, MPCEKF_SUM_*) restated in plain Python over
[nsteps][ncells] trajectories: an explicit step loop per cell, strict comparisons, the sum in
step order.  Shared by tests/test_summary_abi.py (hand-made rows) and tests/test_gpu_summary.py
(a twin context's trajectories); it never sees the code under test.

  reduce(traj, reach=None, obs=None, max_hild=100, state=None) -> {field: float64 [ncells]}

traj: dict with u, v, soc, phise (float64 [nsteps, n]) and nexec (int [nsteps, n]); reach:
None, a scalar or [n]; obs: None or [nsteps, n] (the plant's slot).  state: the result of an
earlier reduce to continue from (accumulation across calls); the step index t goes on from
its "seen".
"""
import numpy as np

FIELDS = ("seen", "steps", "err_step", "t_reach", "u_min", "u_min_step", "u_max", "v_max", "v_max_step", "v_min",
          "phise_min", "phise_min_step", "u_last", "v_last", "soc_last", "phise_last", "u_sum", "nexec_sum",
          "nexec_max", "nsat", "obs_min", "obs_min_step", "obs_max", "obs_max_step")
# reset values: counts, step indices and sums 0 (+0); extrema and last values NaN
ZERO = ("seen", "steps", "err_step", "t_reach", "u_min_step", "v_max_step", "phise_min_step", "u_sum", "nexec_sum",
        "nsat", "obs_min_step", "obs_max_step")


def reset(n):
    return {k: np.full(n, 0.0 if k in ZERO else np.nan) for k in FIELDS}


def _nan(x):
    return x != x


def reduce(traj, reach=None, obs=None, max_hild=100, state=None):
    u, v, soc, ph = (np.asarray(traj[k], dtype=np.float64) for k in ("u", "v", "soc", "phise"))
    ne = np.asarray(traj["nexec"])
    nsteps, n = u.shape
    thr = np.full(n, np.nan) if reach is None else np.broadcast_to(np.asarray(reach, dtype=np.float64), (n,))
    out = reset(n) if state is None else {k: np.array(state[k], dtype=np.float64) for k in FIELDS}
    for c in range(n):
        r = {k: float(out[k][c]) for k in FIELDS}
        for k in range(nsteps):
            r["seen"] += 1.0
            t = r["seen"]
            uk, vk, sk, pk = float(u[k, c]), float(v[k, c]), float(soc[k, c]), float(ph[k, c])
            if not (_nan(uk) or _nan(vk) or _nan(sk) or _nan(pk)):   # a counted step
                r["steps"] += 1.0
                if r["t_reach"] == 0.0 and sk >= thr[c]:
                    r["t_reach"] = t
                if _nan(r["u_min"]) or uk < r["u_min"]:
                    r["u_min"], r["u_min_step"] = uk, t
                if _nan(r["u_max"]) or uk > r["u_max"]:
                    r["u_max"] = uk
                if _nan(r["v_max"]) or vk > r["v_max"]:
                    r["v_max"], r["v_max_step"] = vk, t
                if _nan(r["v_min"]) or vk < r["v_min"]:
                    r["v_min"] = vk
                if _nan(r["phise_min"]) or pk < r["phise_min"]:
                    r["phise_min"], r["phise_min_step"] = pk, t
                r["u_last"], r["v_last"], r["soc_last"], r["phise_last"] = uk, vk, sk, pk
                r["u_sum"] = r["u_sum"] + uk
                x = float(int(ne[k, c]))
                r["nexec_sum"] += x
                if _nan(r["nexec_max"]) or x > r["nexec_max"]:
                    r["nexec_max"] = x
                if int(ne[k, c]) >= max_hild:
                    r["nsat"] += 1.0
            elif r["err_step"] == 0.0:
                r["err_step"] = t
            if obs is not None:
                ok = float(obs[k, c])
                if not _nan(ok):   # the slot's own NaN steps are skipped
                    if _nan(r["obs_min"]) or ok < r["obs_min"]:
                        r["obs_min"], r["obs_min_step"] = ok, t
                    if _nan(r["obs_max"]) or ok > r["obs_max"]:
                        r["obs_max"], r["obs_max_step"] = ok, t
        for k in FIELDS:
            out[k][c] = r[k]
    return out


def bits_equal(a, b, what=""):
    """np.array_equal on the uint64 views of two float64 arrays (NaNs and zero signs included)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
        i = int(np.flatnonzero(a.view(np.uint64).ravel() != b.view(np.uint64).ravel())[0])
        raise AssertionError(f"{what}: {int((a.view(np.uint64) != b.view(np.uint64)).sum())} of {a.size} entries differ "
                             f"in bits, first at {i}: {a.ravel()[i]!r} vs {b.ravel()[i]!r}")


def same_record(got, ref, what="", fields=FIELDS):
    for k in fields:
        bits_equal(got[k], ref[k], f"{what}: {k}")
