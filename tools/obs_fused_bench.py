#!/usr/bin/env python3
"""Cost of the obs trajectory along the fused loop (mpcekf_step_ex_obs, k_obs_traj).

Milliseconds per fused step at 65,536 cells, synthetic quintic ROM, timing off, outputs on
the device; a call of `--warmup` steps, then `--steps` timed steps in one call, `--reps`
times per case:

  (a) parent   the parent commit's library (--parent-root: a checkout of it with its library
               built; skipped without one)
  (b) nslots0  this build, no obs (mpcekf_step)
  (c) one      one slot, negPhise0
  (d) four     negPhise0, negThetass0, posThetass3, Vcell
  (e) full     the whole record
  and the stage pair mpcekf_plant_step / mpcekf_plant_step_obs(obs = NULL), whose difference
  is the cost of the stage route's full-record kernel k_plant_obs.

Every case runs in a fresh child process; the children of (a) and (b) alternate, `--rounds`
of each, then (c)-(e) and the stage pair alternate with (b) again.  Two comparisons are
recorded, not tuned: (b) against the spread of (a)'s own rounds, and (c) - (b) against the
stage pair's difference.  Writes profiles/obs_fused_bench.json stamped with mpcekf_build_id.

    python tools/obs_fused_bench.py [--parent-root DIR] [--cells 65536] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = ("negPhise0", "negThetass0", "posThetass3", "Vcell")


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
    lay = rom.obs_layout() if hasattr(rom, "obs_layout") else {}
    sel = {"parent": (), "nslots0": (), "one": ("negPhise0",), "four": FOUR, "full": tuple(lay)}.get(a.case, ())
    slots = [s for f in sel for s in range(lay[f].start, lay[f].stop)]
    res = {"case": a.case, "build_id": M._lib.load().mpcekf_build_id().decode(), "nslots": len(slots)}
    ms = []
    with M.Context(rom, n) as ctx:
        if a.case in ("plant_step", "plant_step_obs_null"):
            u = np.full(n, -2.0 * rom.Q)
            i, v = ctx._vec(u), np.empty(n)
            call = (lambda: M.check(ctx.L.mpcekf_plant_step(ctx.h, M.dptr(i), None, M.dptr(v)))) \
                if a.case == "plant_step" else \
                (lambda: M.check(ctx.L.mpcekf_plant_step_obs(ctx.h, M.dptr(i), None, M.dptr(v), None)))
            ctx.init_cells(soc0, tc)
            for _ in range(a.warmup):
                call()
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call()
                ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
        else:
            steps = max(a.steps, a.warmup)
            bufs = [M.DeviceBuffer((steps, n)) for _ in range(4)] + [M.DeviceBuffer((steps, n), np.int32)]
            ob = M.DeviceBuffer((steps, len(slots), n)) if slots else None
            kw = dict(obs=ob, obs_slots=slots) if slots else {}
            for _ in range(a.reps):
                ctx.init_cells(soc0, tc)          # every rep: the same steps 1 .. warmup + steps of the charge
                ctx.step_device(a.warmup, *bufs, **kw)
                ctx.sync()
                t0 = time.perf_counter()
                ctx.step_device(a.steps, *bufs, **kw)
                ctx.sync()
                ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
            for b in bufs + ([ob] if ob else []):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_fused_bench.json"))
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
        print(json.dumps({k: r[k] for k in ("case", "build_id", "nslots", "median_ms", "min_ms")}), flush=True)

    for _ in range(a.rounds):
        if a.parent_root:
            take("parent", a.parent_root)
        take("nslots0")
    for _ in range(a.rounds):
        for case in ("one", "nslots0", "four", "full", "plant_step", "plant_step_obs_null"):
            take(case)
    med = {c: [r["median_ms"] for r in v] for c, v in runs.items()}
    m = {c: statistics.median(v) for c, v in med.items()}
    out = {"build_id": runs["nslots0"][0]["build_id"], "ncells": a.cells, "rom": "synthetic quintic",
           "steps": [a.warmup, a.warmup + a.steps], "reps": a.reps, "rounds": a.rounds,
           "what": "ms per fused step, wall clock of one call of `steps` steps after a warm-up call, timing off, "
                   "outputs on the device; per case the medians of its child processes (median of reps each)",
           "median_ms_per_round": med, "median_ms": m}
    if "parent" in m:
        out["parent_build_id"] = runs["parent"][0]["build_id"]
        lo, hi = min(med["parent"]), max(med["parent"])
        out["b_vs_a"] = {"parent_min_ms": lo, "parent_max_ms": hi, "nslots0_ms": med["nslots0"][:a.rounds],
                         "nslots0_inside_parent_spread": all(lo <= x <= hi for x in med["nslots0"][:a.rounds])}
    stage = m["plant_step_obs_null"] - m["plant_step"]
    out["c_minus_b_vs_stage_pair"] = {
        "one_slot_minus_nslots0_ms": m["one"] - m["nslots0"], "four_slots_minus_nslots0_ms": m["four"] - m["nslots0"],
        "full_minus_nslots0_ms": m["full"] - m["nslots0"], "stage_pair_difference_ms": stage,
        "one_slot_at_or_below_stage_pair": m["one"] - m["nslots0"] <= stage}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["c_minus_b_vs_stage_pair"]), flush=True)


if __name__ == "__main__":
    main()
