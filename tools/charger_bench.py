#!/usr/bin/env python3
"""Cost of the charger limits along the fused loop (mpcekf_charger_begin, k_charger in k_pack's or
k_pack_bal's place).

Milliseconds per fused step near 65,536 and near 1,024 cells (the nearest multiple of the string
length S: 65,568 and 1,056 for S = 96, the shared-block kernel; 66,000 and 1,000 for S = 1000, the
block-per-string kernel), with and without a balancer, synthetic quintic ROM, timing off, outputs
on the device (none asked for); a call of `--warmup` steps, then `--steps` timed steps in one call
(steps 10-110 of the charge by default), `--reps` times per case:

  parent    the parent commit's library on the same pack (or balancer) context (--parent-root: a
            checkout of it with its library built; skipped without one)
  pack      this build, the same context without a charger: k_pack / k_pack_bal
  chg0      the same context with a charger whose caps are both NaN: the same problems bit for
            bit, so the difference to `pack` is k_charger's own cost
  chg       binding caps (i_max 0.8 of the 1 C current, p_max 0.7 of S x 4 V x 1 C), for
            information: a change here is Hildreth's (other QPs), not the kernel's

Every case runs in a fresh child process; the cases rotate, each of `--rounds` rounds starting one
case later.  With --bench, `python bench.py`'s default line is taken on this commit and on the
parent in `--bench-rounds` alternated pairs, the parent first in the even pairs and this commit
first in the odd ones.  No threshold is set: the ranges are recorded and whether they overlap.
Writes profiles/charger_bench.json stamped with mpcekf_build_id.

    python tools/charger_bench.py [--parent-root DIR] [--bench] [--cells 65536,1024] [--series 96,1000] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I_1C = 30.0   # A: about the 1 C current of the synthetic ROM's cell


def inputs(np, n, S):
    """tools/pack_bench.py's population: SOC0 10..60 %, Crate 1 / 1.5 / 2 per cell, two cells per string at 70..90 %."""
    rng = np.random.Generator(np.random.PCG64(0x5EED))
    soc0, tc = rng.uniform(10, 60, n), rng.uniform(20, 30, n)
    crate = rng.choice(np.array([1.0, 1.5, 2.0]), n)
    high = np.arange(n) % S >= S - 2
    soc0[high] = rng.uniform(70, 90, int(high.sum()))
    return soc0, tc, crate


def worker(a):
    """One case in this process: prints one JSON line."""
    import numpy as np
    sys.path.insert(0, a.root)
    P = importlib.import_module("mpc-ekf4fastcharge_amd")
    M = importlib.import_module("mpc-ekf4fastcharge_amd.mpcekf")
    rom = P.make_synth_rom(lookup="quintic")
    n, S = a.ncells, a.s
    soc0, tc, crate = inputs(np, n, S)
    res = {"case": a.case, "ncells": n, "series": S, "balancer": bool(a.bal),
           "build_id": M._lib.load().mpcekf_build_id().decode()}
    ms = []
    with M.Context(rom, n) as ctx:
        for _ in range(a.reps):
            ctx.init_cells(soc0, tc)                      # every rep: the same steps of the charge
            ctx.set_limits(Crate=crate)
            ctx.pack_begin(S)
            if a.bal:
                ctx.balance_begin(0.1, 0.01, compensate=True)
            if a.case == "chg0":
                ctx.charger_begin()
            elif a.case == "chg":
                ctx.charger_begin(i_max=0.8 * I_1C, p_max=0.7 * S * 4.0 * I_1C)
            ctx.step_device(a.warmup)                     # mpcekf_step, every output NULL
            ctx.sync()
            t0 = time.perf_counter()
            ctx.step_device(a.steps)
            ctx.sync()
            ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
        if a.case in ("chg0", "chg"):
            r = ctx.charger_get()
            res["capped_share_of_string_steps"] = float((r["ncap_i"] + r["ncap_p"]).sum() / max(r["steps"].sum(), 1))
            res["ncap_i"], res["ncap_p"] = float(r["ncap_i"].sum()), float(r["ncap_p"].sum())
    res.update(ms_per_step=ms, median_ms=statistics.median(ms), min_ms=min(ms))
    print(json.dumps(res), flush=True)


def child(a, case, root, n, S, bal):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", case, "--root", root, "--ncells", str(n), "--s", str(S),
           "--bal", str(int(bal)), "--steps", str(a.steps), "--warmup", str(a.warmup), "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    if r.returncode != 0:   # nothing more is started on the GPU after a failed child
        raise SystemExit(f"{case} ({root}): exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def bench_line(a, root):
    r = subprocess.run([sys.executable, "bench.py"], cwd=root, capture_output=True, text=True, timeout=a.bench_timeout)
    if r.returncode != 0:
        raise SystemExit(f"bench.py ({root}): exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    # the fields this record quotes; the rest of the line (roofline, kernel tables) is bench.py's own business
    return {"value": line["value"], "unit": line["unit"], "ms_per_step": line["ms_per_step"],
            "build_id": line["checks"]["build_id"]}


def overlap(x, y):
    return bool(min(x) <= max(y) and min(y) <= max(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--cells", default="65536,1024")
    ap.add_argument("--series", default="96,1000")
    ap.add_argument("--balancer", default="0,1")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench", action="store_true", help="also bench.py's default line, this commit and the parent")
    ap.add_argument("--bench-rounds", type=int, default=6)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--bench-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "charger_bench.json"))
    ap.add_argument("--worker", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--ncells", type=int, default=65568)
    ap.add_argument("--s", type=int, default=96)
    ap.add_argument("--bal", type=int, default=0)
    a = ap.parse_args()
    a.case = a.worker
    if a.worker:
        return worker(a)
    cases = (("parent",) if a.parent_root else ()) + ("pack", "chg0", "chg")
    out = {"rom": "synthetic quintic", "steps": [a.warmup, a.warmup + a.steps], "reps": a.reps, "rounds": a.rounds,
           "what": "ms per fused step, wall clock of one call of `steps` steps after a warm-up call, timing off, no "
                   "trajectory output, per-cell Crate by set_limits, a pack context in every case; per case the medians "
                   "of its child processes (median of reps each)",
           "sizes": {}}

    def save():
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    for n0 in (int(x) for x in a.cells.split(",")):
        for S in (int(x) for x in a.series.split(",")):
            for bal in (int(x) for x in a.balancer.split(",")):
                n = max(S, int(round(n0 / S)) * S)     # the multiple of S nearest the size
                runs = {}
                for i in range(a.rounds):
                    for j in range(len(cases)):
                        case = cases[(i + j) % len(cases)]
                        r = child(a, "pack" if case == "parent" else case, a.parent_root if case == "parent" else ROOT, n, S,
                                  bal)
                        r["case"] = case
                        runs.setdefault(case, []).append(r)
                        print(json.dumps({k: r[k] for k in ("case", "ncells", "series", "balancer", "build_id", "median_ms",
                                                            "min_ms")}), flush=True)
                med = {c: [r["median_ms"] for r in v] for c, v in runs.items()}
                m = {c: statistics.median(v) for c, v in med.items()}
                size = {"ncells": n, "series": S, "balancer": bool(bal), "median_ms_per_round": med, "median_ms": m,
                        "range_ms": {c: [min(v), max(v)] for c, v in med.items()},
                        "chg0_minus_pack_ms": m["chg0"] - m["pack"],
                        "chg0_and_pack_ranges_overlap": overlap(med["chg0"], med["pack"]),
                        "chg_minus_pack_ms": m["chg"] - m["pack"],
                        "capped_share_of_string_steps": runs["chg"][0]["capped_share_of_string_steps"]}
                out["build_id"] = runs["pack"][0]["build_id"]
                if "parent" in m:
                    out["parent_build_id"] = runs["parent"][0]["build_id"]
                    size["pack_minus_parent_ms"] = m["pack"] - m["parent"]
                    size["pack_and_parent_ranges_overlap"] = overlap(med["pack"], med["parent"])
                out["sizes"][f"{n0}/S={S}/{'balancer' if bal else 'pack'}"] = size
                print(json.dumps({k: size[k] for k in ("ncells", "series", "balancer", "median_ms", "chg0_minus_pack_ms")}),
                      flush=True)
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
        if lines["parent"]:
            tv, pv = [x["value"] for x in lines["this"]], [x["value"] for x in lines["parent"]]
            out["bench_default_line"].update(parent_range=[min(pv), max(pv)], this_range=[min(tv), max(tv)],
                                             ranges_overlap=overlap(tv, pv))
    save()


if __name__ == "__main__":
    main()
