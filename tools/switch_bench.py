#!/usr/bin/env python3
"""Cost of the fused step with a constraint block switched off (mpcekf_switch.hip).

Milliseconds per fused step at 65,536 cells, synthetic quintic ROM, timing off, outputs on
the device; a call of `--warmup` steps, then `--steps` timed steps in one call, `--reps`
times per case.  Cases: the switch masks (1,1,1), (1,1,0), (1,0,0), (0,0,0) on this build,
and (1,1,1) on the parent commit's library (--parent-root: a checkout of it with its library
built; skipped without one).

Every case runs in a fresh child process.  The parent's and this build's (1,1,1) alternate,
`--rounds` pairs; then the switched masks, each beside another (1,1,1) run.  One gate is
recorded: this build's all-on median must fall inside the parent's own min-max of the
alternated rounds (the all-on kernels are the same code).  Writes
profiles/constraint_switches_bench.json stamped with mpcekf_build_id.

    python tools/switch_bench.py [--parent-root DIR] [--cells 65536] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKS = {"on_111": (1, 1, 1), "sw_110": (1, 1, 0), "sw_100": (1, 0, 0), "sw_000": (0, 0, 0), "parent_111": (1, 1, 1)}


def worker(a):
    """One case in this process: prints one JSON line."""
    import numpy as np
    sys.path.insert(0, a.root)
    P = importlib.import_module("mpc-ekf4fastcharge_amd")
    M = importlib.import_module("mpc-ekf4fastcharge_amd.mpcekf")
    rom = P.make_synth_rom(lookup="quintic")
    n = a.cells
    rng = np.random.Generator(np.random.PCG64(0x5EED))
    soc0, tc = rng.uniform(5, 30, n), rng.uniform(20, 30, n)
    mask = MASKS[a.case]
    cfg = M.make_config() if mask == (1, 1, 1) else M.make_config(constraints=mask)
    res = {"case": a.case, "mask": mask, "build_id": M._lib.load().mpcekf_build_id().decode()}
    ms = []
    with M.Context(rom, n, cfg) as ctx:
        res["ncon"] = ctx.ncon
        steps = max(a.steps, a.warmup)
        bufs = [M.DeviceBuffer((steps, n)) for _ in range(4)] + [M.DeviceBuffer((steps, n), np.int32)]
        for _ in range(a.reps):
            ctx.init_cells(soc0, tc)          # every rep: the same steps 1 .. warmup + steps of the charge
            ctx.step_device(a.warmup, *bufs)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.step_device(a.steps, *bufs)
            ctx.sync()
            ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
        ne = bufs[4].to_host()[:a.steps]
        res["qp_fraction"] = float((ne > 0).mean())   # cell-steps of the timed call that ran hildreth.m
        for b in bufs:
            b.free()
    res.update(ms_per_step=ms, median_ms=statistics.median(ms), min_ms=min(ms))
    print(json.dumps(res), flush=True)


def child(a, case, root):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", case, "--root", root, "--cells", str(a.cells),
           "--steps", str(a.steps), "--warmup", str(a.warmup), "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    if r.returncode != 0:   # nothing more is started on the GPU after a failed child
        raise SystemExit(f"{case} ({root}): exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--cells", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constraint_switches_bench.json"))
    ap.add_argument("--worker", default="")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    a.case = a.worker
    if a.worker:
        return worker(a)
    runs = {}

    def take(case, root=ROOT):
        r = child(a, case, root)
        runs.setdefault(case, []).append(r)
        print(json.dumps({k: r[k] for k in ("case", "build_id", "ncon", "median_ms", "min_ms", "qp_fraction")}),
              flush=True)

    for _ in range(a.rounds):
        if a.parent_root:
            take("parent_111", a.parent_root)
        take("on_111")
    for _ in range(a.rounds):
        for case in ("sw_110", "on_111", "sw_100", "sw_000"):
            take(case)
    med = {c: [r["median_ms"] for r in v] for c, v in runs.items()}
    m = {c: statistics.median(v) for c, v in med.items()}
    out = {"build_id": runs["on_111"][0]["build_id"], "ncells": a.cells, "rom": "synthetic quintic",
           "steps": [a.warmup, a.warmup + a.steps], "reps": a.reps, "rounds": a.rounds,
           "what": "ms per fused step, wall clock of one call of `steps` steps after a warm-up call, timing off, "
                   "outputs on the device; per case the medians of its child processes (median of reps each)",
           "masks": {c: MASKS[c] for c in runs}, "ncon": {c: v[0]["ncon"] for c, v in runs.items()},
           "qp_fraction": {c: v[0]["qp_fraction"] for c, v in runs.items()},
           "median_ms_per_round": med, "median_ms": m,
           "switched_minus_all_on_ms": {c: m[c] - m["on_111"] for c in m if c.startswith("sw_")}}
    if "parent_111" in m:
        out["parent_build_id"] = runs["parent_111"][0]["build_id"]
        lo, hi = min(med["parent_111"]), max(med["parent_111"])
        paired = med["on_111"][:a.rounds]
        out["all_on_vs_parent"] = {"parent_min_ms": lo, "parent_max_ms": hi, "all_on_paired_ms": paired,
                                   "all_on_paired_median_ms": statistics.median(paired),
                                   "all_on_median_inside_parent_min_max": lo <= statistics.median(paired) <= hi}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("median_ms", "switched_minus_all_on_ms")}), flush=True)
    if "all_on_vs_parent" in out:
        print(json.dumps(out["all_on_vs_parent"]), flush=True)


if __name__ == "__main__":
    main()
