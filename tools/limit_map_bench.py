#!/usr/bin/env python3
"""Cost of the limit map over (SOC estimate, cell temperature) along the fused loop
(mpcekf_limit_map; k_map before a call's first step, then k_thermal_map in k_thermal's place with a
thermal model, or one k_map_step launch at the end of every step without one).

Milliseconds per fused step at 65,536 and at 1,024 cells, synthetic quintic ROM, timing off,
mpcekf_step with NULL outputs; a call of `--warmup` steps, then `--steps` timed steps in one call
(steps 10-110 of the charge by default), `--reps` times per case:

      step            (a) a context without a map and without a model
      limits          Crate and phise_min as uniform set_limits arrays: the per-cell route the map
                      also takes, without the map
      const           (b) a map on Crate and phise_min, 61 SOC nodes, constant at the configuration's
                      values: the problems of `limits`, bit for bit, with k_map_step at the end of
                      every step
      thermal         a context with the thermal model, no map
      limits_thermal  `limits` with the model
      const_thermal   (b) the constant map, 61 SOC x 4 temperature nodes, with the model:
                      k_thermal_map in k_thermal's place, no added launch
      mscc            (c) a hold-interpolated multi-stage constant-current staircase on Crate (2C to
                      10 % SOC, then 1.5C, 1C, 0.5C from 15 / 20 / 25 %) that binds on the cells
                      above 10 %, no model

step runs on this build and on the parent commit's (--parent-root: a checkout of it with its
library built; skipped without one).  Every case runs in a fresh child process, `--rounds` (3) per
case; per size and round the children run in an order that rotates by one each round, so this build
and the parent alternate and no case always follows the same one.  const - limits and
const_thermal - limits_thermal are the map's own cost; mscc - const is what limits that bind cost
the solver.  With --bench, (d) `python bench.py`'s default line is taken on this commit and on the
parent in `--bench-rounds` (6) alternated pairs, the parent first in the even pairs and this commit
first in the odd ones.  Nothing is tuned to a target: the figures are recorded with the parent's own
spread beside them.  Writes profiles/limit_map_bench.json stamped with mpcekf_build_id.

    python tools/limit_map_bench.py [--parent-root DIR] [--bench] [--cells 65536,1024] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("step", "limits", "const", "thermal", "limits_thermal", "const_thermal", "mscc")
SHARED = ("step",)          # the cases the parent commit, which has no map, runs too


def worker(a):
    """One case in this process: prints one JSON line."""
    import numpy as np
    sys.path.insert(0, a.root)
    P = importlib.import_module("mpc-ekf4fastcharge_amd")
    M = importlib.import_module("mpc-ekf4fastcharge_amd.mpcekf")
    rom = P.make_synth_rom(lookup="quintic")
    n = a.ncells
    rng = np.random.Generator(np.random.PCG64(0x5EED))
    soc0, tc = rng.uniform(5, 30, n), rng.uniform(20, 30, n)
    res = {"case": a.case, "ncells": n, "build_id": M._lib.load().mpcekf_build_id().decode()}
    ms = []
    cfg = M.make_config()
    model = a.case.endswith("thermal")
    with M.Context(rom, n) as ctx:
        if model:   # a few kelvins over the timed steps; half the cells adiabatic
            Cth, Rth = rng.uniform(40.0, 160.0, n), rng.uniform(2.0, 6.0, n)
            Rth[1::2] = np.inf
            ocv = M.thermal_ocv(rom)
        for _ in range(a.reps):
            ctx.init_cells(soc0, tc)                      # every rep: the same steps of the charge
            if model:
                ctx.thermal_begin(Cth, Rth, 25.0, ocv)
            if a.case.startswith("limits"):
                ctx.set_limits(Crate=np.full(n, cfg.Crate), phise_min=np.full(n, cfg.phise_min))
            if a.case == "const":
                ctx.limit_map(0.0, 1.0, Crate=np.full(61, cfg.Crate), phise_min=np.full(61, cfg.phise_min))
            if a.case == "const_thermal":
                ctx.limit_map(0.0, 1.0, T_lo=20.0, T_hi=40.0, Crate=np.full((4, 61), cfg.Crate),
                              phise_min=np.full((4, 61), cfg.phise_min))
            if a.case == "mscc":
                z_lo, z_hi, stair = M.mscc_map([0.0, 0.10, 0.15, 0.20, 0.25, 1.0], [2.0, 1.5, 1.0, 0.5, 0.5], 101)
                ctx.limit_map(z_lo, z_hi, interp_z="hold", Crate=stair)
            ctx.step_device(a.warmup)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.step_device(a.steps)                      # mpcekf_step, every output NULL
            ctx.sync()
            ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
        if a.case in ("const", "const_thermal", "mscc"):
            r = ctx.limit_map_get()
            lim = ctx.get_limits()["Crate"]
            res.update(neval=float(r["neval"][0]), nclamp_z_max=float(r["nclamp_z"].max()),
                       Crate_in_force_min_max=[float(lim.min()), float(lim.max())],
                       cells_below_2C=int((lim < cfg.Crate).sum()))
            ctx.limit_map_end()
    res.update(ms_per_step=ms, median_ms=statistics.median(ms), min_ms=min(ms))
    print(json.dumps(res), flush=True)


def child(a, case, root, n):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", case, "--root", root, "--ncells", str(n),
           "--steps", str(a.steps), "--warmup", str(a.warmup), "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    if r.returncode != 0:   # nothing more is started on the GPU after a failed child
        raise SystemExit(f"{case} ({root}): exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def bench_line(a, root):
    r = subprocess.run([sys.executable, "bench.py"], cwd=root, capture_output=True, text=True, timeout=a.bench_timeout)
    if r.returncode != 0:
        raise SystemExit(f"bench.py ({root}): exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--cells", default="65536,1024")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench", action="store_true", help="also bench.py's default line, this commit and the parent")
    ap.add_argument("--bench-rounds", type=int, default=6)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--bench-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "limit_map_bench.json"))
    ap.add_argument("--worker", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--ncells", type=int, default=65536)
    a = ap.parse_args()
    a.case = a.worker
    if a.worker:
        return worker(a)
    out = {"rom": "synthetic quintic", "steps": [a.warmup, a.warmup + a.steps], "reps": a.reps, "rounds": a.rounds,
           "what": "ms per fused step, wall clock of one call of `steps` steps after a warm-up call, timing off, no "
                   "trajectory output; per case the medians of its child processes (median of reps each); "
                   "parent_*: the parent commit's library and package, which has no map",
           "sizes": {}}

    def save():
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    for n in (int(x) for x in a.cells.split(",")):
        runs = {}
        order = [(c, ROOT) for c in CASES] + ([("parent_" + c, a.parent_root) for c in SHARED] if a.parent_root else [])
        # this build and the parent interleaved: step, parent_step, limits, ...
        order = sorted(order, key=lambda cr: (CASES.index(cr[0].replace("parent_", "")), cr[0].startswith("parent_")))
        for i in range(a.rounds):
            for j in range(len(order)):
                case, root = order[(i + j) % len(order)]
                r = child(a, case.replace("parent_", ""), root, n)
                r["case"] = case
                runs.setdefault(case, []).append(r)
                print(json.dumps({k: r[k] for k in ("case", "ncells", "build_id", "median_ms", "min_ms")}), flush=True)
        med = {c: [r["median_ms"] for r in v] for c, v in runs.items()}
        m = {c: statistics.median(v) for c, v in med.items()}
        size = {"median_ms_per_round": med, "median_ms": m, "range_ms": {c: [min(v), max(v)] for c, v in med.items()},
                "const_minus_limits_ms": m["const"] - m["limits"],
                "const_thermal_minus_limits_thermal_ms": m["const_thermal"] - m["limits_thermal"],
                "mscc_minus_const_ms": m["mscc"] - m["const"],
                "mscc": {k: runs["mscc"][0][k] for k in ("neval", "nclamp_z_max", "Crate_in_force_min_max", "cells_below_2C")}}
        out["build_id"] = runs["step"][0]["build_id"]
        if a.parent_root:
            out["parent_build_id"] = runs["parent_step"][0]["build_id"]
            for c in SHARED:
                lo, hi = min(med["parent_" + c]), max(med["parent_" + c])
                size[c + "_vs_parent"] = {"parent_min_ms": lo, "parent_max_ms": hi, "this_ms": med[c],
                                          "ranges_overlap": min(med[c]) <= hi and lo <= max(med[c])}
        out["sizes"][str(n)] = size
        print(json.dumps({"ncells": n, **{k: v for k, v in size.items() if k != "median_ms_per_round"}}), flush=True)
        save()
    if a.bench:
        lines = {"this": [], "parent": [], "first": []}
        for i in range(a.bench_rounds):
            order = ("parent", "this") if i % 2 == 0 else ("this", "parent")
            for who in order:
                if who == "this" or a.parent_root:
                    lines[who].append(bench_line(a, ROOT if who == "this" else a.parent_root))
            lines["first"].append(order[0])
            print(json.dumps({who: lines[who][-1]["value"] for who in order if lines[who]}), flush=True)
        out["bench_default_line"] = {k: v for k, v in lines.items() if v}
        out["bench_default_line"]["median_value"] = {k: statistics.median(x["value"] for x in lines[k])
                                                     for k in ("this", "parent") if lines[k]}
    save()


if __name__ == "__main__":
    main()
