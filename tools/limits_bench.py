#!/usr/bin/env python3
"""Cost of the fused step with per-cell limits (mpcekf_set_limits).

Milliseconds per fused step at 65,536 cells, synthetic quintic ROM, timing off, outputs on
the device; a call of `--warmup` steps, then `--steps` timed steps in one call, `--reps`
times per case.  Three lines:

  parent    the parent commit's library on a default context (--parent-root: a checkout of it
            with its library built; skipped without one)
  default   this build on a default context: the launches it had before
  percell   this build with all nine fields set to arrays constant at the configuration's
            values: the split route (k_cell<P_EKF | P_LIN>, k_mpc_pc<7>, k_hild, k_hild_slow) on
            the same trajectory, hence the same work

Every case runs in a fresh child process; the three alternate, `--rounds` rounds, their order
rotating from round to round.  One gate is recorded: the default line's median must fall inside
the parent's own min-max over the alternated rounds (it launches the same kernels).  The
per-cell line has no threshold.  Writes profiles/percell_limits_bench.json stamped with
mpcekf_build_id.

    python tools/limits_bench.py [--parent-root DIR] [--cells 65536] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("parent", "default", "percell")


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
    cfg = M.make_config()
    res = {"case": a.case, "build_id": M._lib.load().mpcekf_build_id().decode()}
    ms = []
    with M.Context(rom, n, cfg) as ctx:
        steps = max(a.steps, a.warmup)
        bufs = [M.DeviceBuffer((steps, n)) for _ in range(4)] + [M.DeviceBuffer((steps, n), np.int32)]
        for _ in range(a.reps):
            ctx.init_cells(soc0, tc)          # every rep: the same steps 1 .. warmup + steps of the charge
            if a.case == "percell":
                ctx.set_limits(**{k: np.full(n, getattr(cfg, k)) for k in ctx.LIMIT_FIELDS})
            ctx.step_device(a.warmup, *bufs)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.step_device(a.steps, *bufs)
            ctx.sync()
            ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
        ne = bufs[4].to_host()[:a.steps]
        res["qp_fraction"] = float((ne > 0).mean())   # cell-steps of the timed call that ran hildreth.m
        res["u_checksum"] = float(np.nansum(bufs[0].to_host()[:a.steps]))   # the same trajectory in all three
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "percell_limits_bench.json"))
    ap.add_argument("--worker", default="")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    a.case = a.worker
    if a.worker:
        return worker(a)
    runs = {}
    for rnd in range(a.rounds):
        k = rnd % len(CASES)            # the order rotates, so that no line always runs first (or last) of its round
        for case in CASES[k:] + CASES[:k]:
            if case == "parent" and not a.parent_root:
                continue
            r = child(a, case, a.parent_root if case == "parent" else ROOT)
            runs.setdefault(case, []).append(r)
            print(json.dumps({k: r[k] for k in ("case", "build_id", "median_ms", "min_ms", "qp_fraction", "u_checksum")}),
                  flush=True)
    med = {c: [r["median_ms"] for r in v] for c, v in runs.items()}
    m = {c: statistics.median(v) for c, v in med.items()}
    out = {"build_id": runs["default"][0]["build_id"], "ncells": a.cells, "rom": "synthetic quintic",
           "steps": [a.warmup, a.warmup + a.steps], "reps": a.reps, "rounds": a.rounds,
           "what": "ms per fused step, wall clock of one call of `steps` steps after a warm-up call, timing off, "
                   "outputs on the device; per case the medians of its child processes (median of reps each)",
           "qp_fraction": {c: v[0]["qp_fraction"] for c, v in runs.items()},
           "same_trajectory": len({v[0]["u_checksum"] for v in runs.values()}) == 1,
           "median_ms_per_round": med, "median_ms": m, "percell_minus_default_ms": m["percell"] - m["default"]}
    if "parent" in m:
        out["parent_build_id"] = runs["parent"][0]["build_id"]
        lo, hi = min(med["parent"]), max(med["parent"])
        out["default_vs_parent"] = {"parent_min_ms": lo, "parent_max_ms": hi, "default_median_ms": m["default"],
                                    "default_median_inside_parent_min_max": lo <= m["default"] <= hi}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("median_ms", "percell_minus_default_ms", "same_trajectory")}), flush=True)
    if "default_vs_parent" in out:
        print(json.dumps(out["default_vs_parent"]), flush=True)


if __name__ == "__main__":
    main()
