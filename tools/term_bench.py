#!/usr/bin/env python3
"""Cost and gain of charge termination along the fused loop (mpcekf_term_begin, k_term,
mpcekf_step_until).

The rule's own cost: milliseconds per fused step at 65,536 and 1,024 cells, synthetic quintic ROM,
timing off, outputs on the device (none asked for); a call of `--warmup` steps, then `--steps`
timed steps in one call (steps 10-110 of the charge by default), `--reps` times per case:

  parent    the parent commit's library, mpcekf_step with NULL outputs (--parent-root: a checkout
            of it with its library built; skipped without one)
  step      this build, the same call on a context without a rule
  term      the same call after term_begin with thresholds that never hold (soc_stop 2, i_taper -1,
            T_cut 1000): the same problems bit for bit, plus k_term after every step's Hildreth

Every case runs in a fresh child process; the cases rotate, each of `--rounds` rounds starting one
case later.  What the rule buys: run_summary over a `--cap`-step cap (3,000) at the first size with
per-cell C-rates 0.5..2 and SOC0 40..70 %, once with stop=dict(soc_stop=0.8) and once over the fixed
cap: steps_run and wall time of both.  With --bench, `python bench.py`'s default line is taken on
this commit and on the parent in `--bench-rounds` alternated pairs, the parent first in the even
pairs and this commit first in the odd ones.  No threshold is set: the figures are recorded with the
parent's own spread beside them.  Writes profiles/term_bench.json stamped with mpcekf_build_id.

    python tools/term_bench.py [--parent-root DIR] [--bench] [--cells 65536,1024] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(a):
    """One case in this process: prints one JSON line."""
    import numpy as np
    sys.path.insert(0, a.root)
    P = importlib.import_module("mpc-ekf4fastcharge_amd")
    M = importlib.import_module("mpc-ekf4fastcharge_amd.mpcekf")
    rom = P.make_synth_rom(lookup="quintic")
    n = a.ncells
    rng = np.random.Generator(np.random.PCG64(0x5EED))
    res = {"case": a.case, "ncells": n, "build_id": M._lib.load().mpcekf_build_id().decode()}
    if a.case in ("until", "fixed"):
        soc0, tc, crate = rng.uniform(40, 70, n), rng.uniform(20, 30, n), rng.uniform(0.5, 2.0, n)
        t0 = time.perf_counter()
        s = M.run_summary(rom, soc0, tc, a.cap, limits=dict(Crate=crate), reach=0.8, chunk=a.chunk,
                          stop=dict(soc_stop=0.8, chunk=a.chunk) if a.case == "until" else None)
        res.update(wall_s=time.perf_counter() - t0, steps_run=int(s.get("steps_run", a.cap)), cap=a.cap, chunk=a.chunk,
                   cells_reached=int((s["t_reach"] > 0).sum()), t_reach_max=float(s["t_reach"].max()),
                   soc_last_mean=float(np.nanmean(s["soc_last"])))
        if a.case == "until":
            res.update(open_left=int((s["term"]["state"] == 0).sum()), done_step_max=float(s["term"]["done_step"].max()))
        print(json.dumps(res), flush=True)
        return
    soc0, tc = rng.uniform(10, 60, n), rng.uniform(20, 30, n)
    ms = []
    with M.Context(rom, n) as ctx:
        for _ in range(a.reps):
            ctx.init_cells(soc0, tc)                      # every rep: the same steps of the charge
            if a.case == "term":
                ctx.term_begin(soc_stop=2.0, i_taper=-1.0, hold=1, T_cut=1000.0)
            ctx.step_device(a.warmup)                     # mpcekf_step, every output NULL
            ctx.sync()
            t0 = time.perf_counter()
            ctx.step_device(a.steps)
            ctx.sync()
            ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
        if a.case == "term":
            res["open_cells"] = ctx.term_open()
    res.update(ms_per_step=ms, median_ms=statistics.median(ms), min_ms=min(ms))
    print(json.dumps(res), flush=True)


def child(a, case, root, n):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", case, "--root", root, "--ncells", str(n),
           "--steps", str(a.steps), "--warmup", str(a.warmup), "--reps", str(a.reps), "--cap", str(a.cap),
           "--chunk", str(a.chunk)]
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
    ap.add_argument("--cap", type=int, default=3000)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--bench", action="store_true", help="also bench.py's default line, this commit and the parent")
    ap.add_argument("--bench-rounds", type=int, default=6)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--bench-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "term_bench.json"))
    ap.add_argument("--worker", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--ncells", type=int, default=65536)
    a = ap.parse_args()
    a.case = a.worker
    if a.worker:
        return worker(a)
    cases = (("parent",) if a.parent_root else ()) + ("step", "term")
    out = {"rom": "synthetic quintic", "steps": [a.warmup, a.warmup + a.steps], "reps": a.reps, "rounds": a.rounds,
           "what": "ms per fused step, wall clock of one call of `steps` steps after a warm-up call, timing off, no "
                   "trajectory output; per case the medians of its child processes (median of reps each); term: "
                   "thresholds that never hold",
           "sizes": {}}
    sizes = [int(x) for x in a.cells.split(",")]
    for n in sizes:
        runs = {}
        for i in range(a.rounds):
            for j in range(len(cases)):
                case = cases[(i + j) % len(cases)]
                r = child(a, "step" if case == "parent" else case, a.parent_root if case == "parent" else ROOT, n)
                r["case"] = case
                runs.setdefault(case, []).append(r)
                print(json.dumps({k: r[k] for k in ("case", "ncells", "build_id", "median_ms", "min_ms")}), flush=True)
        med = {c: [r["median_ms"] for r in v] for c, v in runs.items()}
        m = {c: statistics.median(v) for c, v in med.items()}
        size = {"ncells": n, "median_ms_per_round": med, "median_ms": m, "range_ms": {c: [min(v), max(v)] for c, v in med.items()},
                "term_minus_step_ms": m["term"] - m["step"], "open_cells_after": runs["term"][0]["open_cells"]}
        out["build_id"] = runs["step"][0]["build_id"]
        if "parent" in m:
            out["parent_build_id"] = runs["parent"][0]["build_id"]
            lo, hi = min(med["parent"]), max(med["parent"])
            size["term_minus_parent_ms"] = m["term"] - m["parent"]
            size["step_vs_parent"] = {"parent_min_ms": lo, "parent_max_ms": hi, "step_ms": med["step"],
                                      "step_minus_parent_ms": m["step"] - m["parent"],
                                      "step_inside_parent_spread": all(lo <= x <= hi for x in med["step"])}
        out["sizes"][str(n)] = size
        print(json.dumps({k: size[k] for k in ("ncells", "median_ms", "term_minus_step_ms")}), flush=True)
    # what the rule buys: the first size, the stopped run and the fixed one, the stopped one first
    out["stop_at_soc_0.8"] = {"what": "run_summary, per-cell Crate 0.5..2, SOC0 40..70 %: stop=dict(soc_stop=0.8) against "
                                      "the fixed cap; wall time of the whole call, context creation included",
                              "until": child(a, "until", ROOT, sizes[0]), "fixed": child(a, "fixed", ROOT, sizes[0])}
    print(json.dumps(out["stop_at_soc_0.8"]), flush=True)
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
        med = {k: statistics.median(x["value"] for x in lines[k]) for k in ("this", "parent") if lines[k]}
        out["bench_default_line"]["median_value"] = med
        if lines["parent"]:
            lo, hi = min(x["value"] for x in lines["parent"]), max(x["value"] for x in lines["parent"])
            out["bench_default_line"]["parent_range"] = [lo, hi]
            out["bench_default_line"]["this_range"] = [min(x["value"] for x in lines["this"]),
                                                       max(x["value"] for x in lines["this"])]
            out["bench_default_line"]["ranges_overlap"] = bool(out["bench_default_line"]["this_range"][0] <= hi and
                                                               lo <= out["bench_default_line"]["this_range"][1])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
