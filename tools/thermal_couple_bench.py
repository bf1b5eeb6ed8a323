#!/usr/bin/env python3
"""Cost of heat conduction between neighbouring cells along the fused loop (mpcekf_thermal_couple:
k_thermal_couple in k_thermal's place, k_couple_seed once per call).

Milliseconds per fused step at 65,568 cells (683 strings of 96) and at 1,056 cells (11 strings),
synthetic quintic ROM, timing off; a call of `--warmup` steps, then `--steps` timed steps in one
call (steps 10-110 of the charge by default), every output NULL, `--reps` times per case:

      parent    mpcekf_step on a thermal pack context, the parent commit's package and library
                (--parent-root: a checkout of it with its library built; skipped without one)
      plain     the same context and call on this build, no links
      coupled   the same with links (0.5-5 K/W, every fifth +inf)
      plain1    `--steps` calls of one step each on the plain context: ms per call
      coupled1  the same on the coupled context; every call launches k_couple_seed

  per step:  coupled - parent and coupled - plain
  per call:  (coupled1 - plain1) - (coupled - plain): what a call costs beyond its steps, the seed

Every case runs in a fresh child process; the cases rotate through `--rounds` rounds, the parent's
child and this build's alternating.  With --bench, `python bench.py`'s default line is taken on
this commit and on the parent in `--bench-rounds` alternated pairs, the parent first in the even
pairs and this commit first in the odd ones.  Nothing is tuned to a target: medians and ranges are
recorded as they come.  Writes profiles/thermal_couple_bench.json stamped with mpcekf_build_id.

    python tools/thermal_couple_bench.py [--parent-root DIR] [--bench] [--cells 65568,1056] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("parent", "plain", "coupled", "plain1", "coupled1")
SERIES = 96


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
    Cth, Rth = rng.uniform(40.0, 160.0, n), rng.uniform(2.0, 6.0, n)
    Rth[1::2] = np.inf
    links = rng.uniform(0.5, 5.0, n)
    links[4::5] = np.inf
    ocv = M.thermal_ocv(rom)
    res = {"case": a.case, "ncells": n, "build_id": M._lib.load().mpcekf_build_id().decode()}
    ms = []
    single = a.case.endswith("1")
    with M.Context(rom, n) as ctx:
        for _ in range(a.reps):
            ctx.init_cells(soc0, tc)                      # every rep: the same steps of the charge
            ctx.thermal_begin(Cth, Rth, 25.0, ocv)
            ctx.pack_begin(SERIES)
            if a.case.startswith("coupled"):
                ctx.thermal_couple(links)
            ctx.step_device(a.warmup)                     # mpcekf_step, every output NULL
            ctx.sync()
            t0 = time.perf_counter()
            if single:
                for _ in range(a.steps):
                    ctx.step_device(1)
            else:
                ctx.step_device(a.steps)
            ctx.sync()
            ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
        if a.case.startswith("coupled"):
            r = ctx.thermal_couple_get()
            res["dt_max_median_K"] = float(np.nanmedian(r["DT_MAX"]))
            res["linked_share"] = float(np.isfinite(r["DT_MAX"]).mean())
    res.update(ms_per_step=ms, median_ms=statistics.median(ms), min_ms=min(ms))
    print(json.dumps(res), flush=True)


def child(a, case, n):
    root = a.parent_root if case == "parent" else ROOT
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "plain" if case == "parent" else case, "--root", root,
           "--ncells", str(n), "--steps", str(a.steps), "--warmup", str(a.warmup), "--reps", str(a.reps)]
    env = dict(os.environ)
    if case == "parent":   # the parent's package on the parent's library
        env["MPCEKF_LIB"] = os.path.join(root, "mpc-ekf4fastcharge_amd", "_build", "libmpcekf.so")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout, env=env)
    if r.returncode != 0:   # nothing more is started on the GPU after a failed child
        raise SystemExit(f"{case} ({root}): exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    out = json.loads(r.stdout.strip().splitlines()[-1])
    out["case"] = case
    return out


def bench_line(a, root):
    r = subprocess.run([sys.executable, "bench.py"], cwd=root, capture_output=True, text=True, timeout=a.bench_timeout)
    if r.returncode != 0:
        raise SystemExit(f"bench.py ({root}): exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def span(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--cells", default="65568,1056")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench", action="store_true", help="also bench.py's default line, this commit and the parent")
    ap.add_argument("--bench-rounds", type=int, default=6)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--bench-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thermal_couple_bench.json"))
    ap.add_argument("--worker", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--ncells", type=int, default=65568)
    a = ap.parse_args()
    a.case = a.worker
    if a.worker:
        return worker(a)
    out = {"rom": "synthetic quintic", "series": SERIES, "steps": [a.warmup, a.warmup + a.steps], "reps": a.reps,
           "rounds": a.rounds,
           "what": "ms per fused step (plain1 / coupled1: per one-step call), wall clock after a warm-up call, timing "
                   "off, every output NULL; per case the medians of its child processes (median of reps each), with "
                   "their range",
           "sizes": {}}

    def flush():
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    cases = [c for c in CASES if c != "parent" or a.parent_root]
    for n in (int(x) for x in a.cells.split(",") if x):   # --cells "": the bench.py pairs only
        runs = {}
        for i in range(a.rounds):
            for j in range(len(cases)):
                r = child(a, cases[(i + j) % len(cases)], n)
                runs.setdefault(r["case"], []).append(r)
                print(json.dumps({k: r[k] for k in ("case", "ncells", "build_id", "median_ms", "min_ms")}), flush=True)
        med = {c: [r["median_ms"] for r in v] for c, v in runs.items()}
        m = {c: statistics.median(v) for c, v in med.items()}
        size = {"median_ms_per_child": med, "ms": {c: span(v) for c, v in med.items()},
                "coupled_minus_plain_ms_per_step": m["coupled"] - m["plain"],
                "seed_ms_per_call": (m["coupled1"] - m["plain1"]) - (m["coupled"] - m["plain"]),
                "coupled1_minus_plain1_ms_per_call": m["coupled1"] - m["plain1"],
                "dt_max_median_K": runs["coupled"][0]["dt_max_median_K"], "linked_share": runs["coupled"][0]["linked_share"]}
        out["build_id"] = runs["plain"][0]["build_id"]
        if a.parent_root:
            out["parent_build_id"] = runs["parent"][0]["build_id"]
            size["coupled_minus_parent_ms_per_step"] = m["coupled"] - m["parent"]
            size["plain_minus_parent_ms_per_step"] = m["plain"] - m["parent"]
        out["sizes"][str(n)] = size
        print(json.dumps({"ncells": n, **{k: v for k, v in size.items() if "_ms_" in k}}), flush=True)
        flush()
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
        for k in ("this", "parent"):
            if lines[k]:
                out["bench_default_line"][k + "_range"] = [min(x["value"] for x in lines[k]), max(x["value"] for x in lines[k])]
    flush()


if __name__ == "__main__":
    main()
