#!/usr/bin/env python3
"""Cost of the per-cell lumped thermal model along the fused loop (mpcekf_thermal_begin, k_thermal).

Milliseconds per fused step at 65,536 and at 1,024 cells, synthetic quintic ROM, timing off;
a call of `--warmup` steps, then `--steps` timed steps in one call (steps 10-110 of the charge by
default), `--reps` times per case:

  (a) parent    the parent commit's library, mpcekf_step with NULL outputs (--parent-root: a
                checkout of it with its library built; skipped without one)
      step      this build, mpcekf_step with NULL outputs on a context without a model
  (b) thermal   the same call on a context with a model: k_thermal after every step
  (c) rows      mpcekf_step_ex_thermal with temp + heat rows in device buffers

Every case runs in a fresh child process.  The children of parent and step alternate, `--rounds`
pairs; then step, thermal, rows rotate, each round starting one case later.  One more child
(`timing`) takes mpcekf_set_timing's buckets at the first size, ms per launch, over the same
steps on a context without and with the model, twice each, alternating.  With --bench,
`python bench.py`'s default line is taken on this commit and on the parent in `--bench-rounds`
alternated pairs, the parent first in the even pairs and this commit first in the odd ones.
Nothing is tuned to a target: the figures are recorded with the parent's own spread beside
them.  Writes profiles/thermal_bench.json stamped with mpcekf_build_id.

    python tools/thermal_bench.py [--parent-root DIR] [--bench] [--cells 65536,1024] [--out FILE]"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("step", "thermal", "rows")


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
    if a.case == "timing":
        return timing(a, M, rom, soc0, tc, rng, res)
    ms = []
    with M.Context(rom, n) as ctx:
        model = a.case in ("thermal", "rows")
        if model:   # a few kelvins over the timed steps; half the cells adiabatic
            Cth, Rth = rng.uniform(40.0, 160.0, n), rng.uniform(2.0, 6.0, n)
            Rth[1::2] = np.inf
            ocv = M.thermal_ocv(rom)
        bufs = [M.DeviceBuffer((max(a.steps, a.warmup), n), np.float64) for _ in range(2)] if a.case == "rows" else []

        def run(k):
            if a.case == "rows":
                M.check(ctx.L.mpcekf_step_ex_thermal(ctx.h, int(k), None, None, 0, None, C.c_void_p(bufs[0].ptr),
                                                     C.c_void_p(bufs[1].ptr), 1))
            else:
                ctx.step_device(k)                        # mpcekf_step, every output NULL

        for _ in range(a.reps):
            ctx.init_cells(soc0, tc)                      # every rep: the same steps of the charge
            if model:
                ctx.thermal_begin(Cth, Rth, 25.0, ocv)
            run(a.warmup)
            ctx.sync()
            t0 = time.perf_counter()
            run(a.steps)
            ctx.sync()
            ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
        if model:
            r = ctx.thermal_get(("T", "steps", "nheld"))
            res["model_steps"] = float(r["steps"][0] + r["nheld"][0])
            res["T_rise_median"] = float(np.median(r["T"] - tc))
        for b in bufs:
            b.free()
    res.update(ms_per_step=ms, median_ms=statistics.median(ms), min_ms=min(ms))
    print(json.dumps(res), flush=True)


def timing(a, M, rom, soc0, tc, rng, res):
    """mpcekf_set_timing's buckets (ms per launch) over the timed steps, without / with the model."""
    n = a.ncells
    Cth, Rth = rng.uniform(40.0, 160.0, n), rng.uniform(2.0, 6.0, n)
    Rth[1::2] = float("inf")
    ocv = M.thermal_ocv(rom)
    res["buckets"] = []
    with M.Context(rom, n) as ctx:
        for model in (False, True, False, True):
            ctx.init_cells(soc0, tc)
            if model:
                ctx.thermal_begin(Cth, Rth, 25.0, ocv)
            else:
                ctx.thermal_end()
            ctx.step_device(a.warmup)
            ctx.sync()
            ctx.set_timing(True)
            ctx.get_timing()
            ctx.step_device(a.steps)
            ctx.sync()
            t = ctx.get_timing()
            ctx.set_timing(False)
            res["buckets"].append({"model": model, **{k: v[0] / v[1] for k, v in t.items() if v[1]}})
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thermal_bench.json"))
    ap.add_argument("--worker", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--ncells", type=int, default=65536)
    a = ap.parse_args()
    a.case = a.worker
    if a.worker:
        return worker(a)
    out = {"rom": "synthetic quintic", "steps": [a.warmup, a.warmup + a.steps], "reps": a.reps, "rounds": a.rounds,
           "what": "ms per fused step, wall clock of one call of `steps` steps after a warm-up call, timing off, no "
                   "trajectory output (rows: temp + heat in device buffers); per case the medians of its child "
                   "processes (median of reps each)",
           "sizes": {}}
    for n in (int(x) for x in a.cells.split(",")):
        runs = {}

        def take(case, root=ROOT):
            r = child(a, "step" if case == "parent" else case, root, n)
            r["case"] = case
            runs.setdefault(case, []).append(r)
            print(json.dumps({k: r[k] for k in ("case", "ncells", "build_id", "median_ms", "min_ms")}), flush=True)

        for _ in range(a.rounds):
            if a.parent_root:
                take("parent", a.parent_root)
            take("step")
        for i in range(a.rounds):
            for j in range(len(CASES)):
                take(CASES[(i + j) % len(CASES)])
        med = {c: [r["median_ms"] for r in v] for c, v in runs.items()}
        m = {c: statistics.median(v) for c, v in med.items()}
        size = {"median_ms_per_round": med, "median_ms": m,
                "thermal_minus_step_ms": m["thermal"] - m["step"], "rows_minus_step_ms": m["rows"] - m["step"],
                "T_rise_median_K": runs["thermal"][0]["T_rise_median"]}
        out["build_id"] = runs["step"][0]["build_id"]
        if "parent" in m:
            out["parent_build_id"] = runs["parent"][0]["build_id"]
            lo, hi = min(med["parent"]), max(med["parent"])
            size["step_vs_parent"] = {"parent_min_ms": lo, "parent_max_ms": hi, "step_ms": med["step"][:a.rounds],
                                      "step_inside_parent_spread": all(lo <= x <= hi for x in med["step"][:a.rounds])}
        if "timing_buckets" not in out:   # the first size only
            out["timing_buckets"] = {"ncells": n, "what": "mpcekf_set_timing, ms per launch over the timed steps (events "
                                     "on: not comparable with the wall-clock figures), one child process",
                                     "runs": child(a, "timing", ROOT, n)["buckets"]}
            print(json.dumps(out["timing_buckets"]["runs"]), flush=True)
        out["sizes"][str(n)] = size
        print(json.dumps({"ncells": n, **{k: size[k] for k in ("median_ms", "thermal_minus_step_ms",
                                                                "rows_minus_step_ms")}}), flush=True)
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
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
