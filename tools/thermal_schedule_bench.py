#!/usr/bin/env python3
"""Cost of the temperature schedule of the MPC limits along the fused loop
(mpcekf_thermal_schedule; k_sched before a call's first step, k_thermal_sched in k_thermal's place).

Milliseconds per fused step at 65,536 and at 1,024 cells, synthetic quintic ROM, timing off,
mpcekf_step with NULL outputs; a call of `--warmup` steps, then `--steps` timed steps in one call
(steps 10-110 of the charge by default), `--reps` times per case:

      step      a context without a model
      thermal   a context with the thermal model and no schedule
      limits    the thermal context with Crate and phise_min as uniform set_limits arrays: the
                split per-cell route the schedule also takes, without the schedule
      const     the thermal context with a schedule on Crate and phise_min whose tables are
                constant at the configuration's values: the problems of `limits`, bit for bit,
                with the schedule's kernels
      sched     the thermal context with a schedule on Crate and phise_min (two derating maps, 9
                knots over 20..40 degC, the cells alternating between the maps): limits that bind

step, thermal and limits run on this build and on the parent commit's (--parent-root: a checkout
of it with its library built; those cases are skipped without one).  Every case runs in a fresh
child process; per size and round the eight children run in an order that rotates by one each
round, so this build and the parent alternate and no case always follows the same one.
const - limits(parent) is the schedule's own cost; sched - const is what the derated limits cost
the solver (more rows of the QP active).  One more child (`timing`) takes mpcekf_set_timing's
buckets at the first size, ms per launch, for limits, const and sched.  With --bench,
`python bench.py`'s default line is taken on this commit and on the parent in `--bench-rounds`
alternated pairs, the parent first in the even pairs and this commit first in the odd ones.  Nothing is tuned to a target: the figures
are recorded with the parent's own spread beside them.  Writes
profiles/thermal_schedule_bench.json stamped with mpcekf_build_id.

    python tools/thermal_schedule_bench.py [--parent-root DIR] [--bench] [--cells 65536,1024] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("step", "thermal", "limits", "const", "sched")
SHARED = ("step", "thermal", "limits")          # the cases the parent commit runs too


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
    derated = dict(Crate=np.stack([np.linspace(2.0, 0.5, 9), np.linspace(2.0, 1.0, 9)]),
                   phise_min=np.stack([np.linspace(0.12, 0.08, 9), np.linspace(0.10, 0.08, 9)]))
    flat = dict(Crate=np.full((2, 9), M.make_config().Crate), phise_min=np.full((2, 9), M.make_config().phise_min))
    if a.case == "timing":
        return timing(a, M, rom, soc0, tc, rng, res, derated, flat)
    with M.Context(rom, n) as ctx:
        model = a.case != "step"
        if model:   # a few kelvins over the timed steps; half the cells adiabatic
            Cth, Rth = rng.uniform(40.0, 160.0, n), rng.uniform(2.0, 6.0, n)
            Rth[1::2] = np.inf
            ocv = M.thermal_ocv(rom)
        cfg = M.make_config()
        for _ in range(a.reps):
            ctx.init_cells(soc0, tc)                      # every rep: the same steps of the charge
            if model:
                ctx.thermal_begin(Cth, Rth, 25.0, ocv)
            if a.case == "limits":
                ctx.set_limits(Crate=np.full(n, cfg.Crate), phise_min=np.full(n, cfg.phise_min))
            if a.case in ("sched", "const"):
                ctx.thermal_schedule(20.0, 40.0, sets=(np.arange(n) % 2).astype(np.int32),
                                     **(derated if a.case == "sched" else flat))
            ctx.step_device(a.warmup)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.step_device(a.steps)                      # mpcekf_step, every output NULL
            ctx.sync()
            ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
        if model:
            r = ctx.thermal_get(("T", "steps", "nheld"))
            res["model_steps"] = float(r["steps"][0] + r["nheld"][0])
            res["T_rise_median"] = float(np.median(r["T"] - tc))
        if a.case in ("sched", "const"):
            res["Crate_in_force_min_max"] = [float(ctx.get_limits()["Crate"].min()), float(ctx.get_limits()["Crate"].max())]
    res.update(ms_per_step=ms, median_ms=statistics.median(ms), min_ms=min(ms))
    print(json.dumps(res), flush=True)


def timing(a, M, rom, soc0, tc, rng, res, derated, flat):
    """mpcekf_set_timing's buckets (ms per launch) over the timed steps: limits, const, sched, twice each."""
    import numpy as np
    n = a.ncells
    Cth, Rth = rng.uniform(40.0, 160.0, n), rng.uniform(2.0, 6.0, n)
    Rth[1::2] = float("inf")
    ocv = M.thermal_ocv(rom)
    cfg = M.make_config()
    res["buckets"] = []
    with M.Context(rom, n) as ctx:
        for case in ("limits", "const", "sched") * 2:
            ctx.init_cells(soc0, tc)
            ctx.thermal_begin(Cth, Rth, 25.0, ocv)
            if case == "limits":
                ctx.thermal_schedule_end()
                ctx.set_limits(Crate=np.full(n, cfg.Crate), phise_min=np.full(n, cfg.phise_min))
            else:
                ctx.thermal_schedule(20.0, 40.0, sets=(np.arange(n) % 2).astype(np.int32),
                                     **(derated if case == "sched" else flat))
            ctx.step_device(a.warmup)
            ctx.sync()
            ctx.set_timing(True)
            ctx.get_timing()
            ctx.step_device(a.steps)
            ctx.sync()
            t = ctx.get_timing()
            ctx.set_timing(False)
            res["buckets"].append({"case": case, **{k: v[0] / v[1] for k, v in t.items() if v[1]}})
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thermal_schedule_bench.json"))
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
                   "parent_*: the parent commit's library and package",
           "sizes": {}}

    def save():
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    for n in (int(x) for x in a.cells.split(",")):
        runs = {}
        order = [(c, ROOT) for c in CASES] + ([("parent_" + c, a.parent_root) for c in SHARED] if a.parent_root else [])
        # this build and the parent interleaved: step, parent_step, thermal, parent_thermal, ...
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
                "const_minus_limits_ms": m["const"] - m["limits"], "sched_minus_const_ms": m["sched"] - m["const"],
                "thermal_minus_step_ms": m["thermal"] - m["step"],
                "T_rise_median_K": runs["sched"][0]["T_rise_median"],
                "Crate_in_force_min_max": runs["sched"][0]["Crate_in_force_min_max"]}
        out["build_id"] = runs["step"][0]["build_id"]
        if a.parent_root:
            out["parent_build_id"] = runs["parent_step"][0]["build_id"]
            size["const_minus_parent_limits_ms"] = m["const"] - m["parent_limits"]
            size["sched_minus_parent_limits_ms"] = m["sched"] - m["parent_limits"]
            for c in SHARED:
                lo, hi = min(med["parent_" + c]), max(med["parent_" + c])
                size[c + "_vs_parent"] = {"parent_min_ms": lo, "parent_max_ms": hi, "this_ms": med[c],
                                          "inside_parent_spread": all(lo <= x <= hi for x in med[c])}
        if "timing_buckets" not in out:   # the first size only
            out["timing_buckets"] = {"ncells": n, "what": "mpcekf_set_timing, ms per launch over the timed steps (events "
                                     "on: not comparable with the wall-clock figures), one child process",
                                     "runs": child(a, "timing", ROOT, n)["buckets"]}
            print(json.dumps(out["timing_buckets"]["runs"]), flush=True)
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
