#!/usr/bin/env python3
"""Regenerates tests/golden/obs_batch8_40.npz: OB_step's obs output (OB_step.m:226-356) of
8 cells over 40 plant steps in handle mode (the closed-form cellData.function handles of
the synthetic ROM), from tests/obs_ref.ob_obs riding on oracle_np.ob_step.

The current is obs_ref.profile: a charge at -Q*Crate, a rest, a short discharge pulse --
fixed, independent of any controller.  Before writing, the table-mode ob_obs on the
quintic ROM is checked against the handle-mode values on all 8 x 40 entries of every field
to the documented handle-parity bound, 1e-6 relative to max(1, |field|).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import importlib  # noqa: E402

import obs_ref  # noqa: E402
import oracle_np as onp  # noqa: E402
from conftest import batch_inputs  # noqa: E402

N, STEPS, BOUND = 8, 40, 1e-6


def trajectory(rom, soc0, tc, u, handles):
    """{field: [STEPS, N, len]} (scalars [STEPS, N]) with the state advanced by ob_step."""
    out = {k: [] for k in obs_ref.OBS_FIELDS}
    for c in range(N):
        cs = onp.ob_step_init(rom, soc0[c], tc[c], handles=handles)
        rows = {k: [] for k in obs_ref.OBS_FIELDS}
        for k in range(STEPS):
            o = obs_ref.ob_obs(rom, cs["bigX"].T, cs["SOCnAvg"], cs["SOCpAvg"], cs["SOC0n"], cs["SOC0p"], u[k], tc[c],
                               handles=handles)
            onp.ob_step(u[k], tc[c], cs)
            for f in rows:
                rows[f].append(o[f])
        for f in rows:
            out[f].append(np.array(rows[f]))
    return {f: np.stack(v, axis=1) for f, v in out.items()}


def main():
    P = importlib.import_module("mpc-ekf4fastcharge_amd")
    rom = P.make_synth_rom(lookup="quintic")
    soc0, tc = batch_inputs(N, seed=113)
    u = obs_ref.profile(rom, STEPS)
    gold = trajectory(rom, soc0, tc, u, handles=True)
    tab = trajectory(rom, soc0, tc, u, handles=False)
    worst = 0.0
    for f in obs_ref.OBS_FIELDS:
        if gold[f].size:
            e = float(np.max(np.abs(tab[f] - gold[f]) / np.maximum(1.0, np.abs(gold[f]))))
            worst = max(worst, e)
            assert e <= BOUND, (f, e)
    path = os.path.join(ROOT, "tests", "golden", "obs_batch8_40.npz")
    np.savez_compressed(path, soc0=soc0, tc=tc, u=u, **{"obs_" + f: gold[f] for f in obs_ref.OBS_FIELDS})
    print(f"{path}: {os.path.getsize(path)} bytes; table mode within {worst:.3g} (bound {BOUND:g})")


if __name__ == "__main__":
    main()
