"""Host-side mirror of the reference's operator interface, over the C-ABI.

The reference exposes MATLAB functions called by name from runMPC.m; this
module keeps those names and argument meanings, batched over cells:

  Context.OB_step(Iapp)              <- OB_step.m:1        (cellState lives in the context)
  Context.iterEKF(vk, ik)            <- iterEKF.m:30       (ekfData lives in the context)
  Context.EKFmatsHandler(zk, Xind)   <- EKFmatsHandler.m:1
  Context.iterMPC(lin, SOCk_1)       <- iterMPC.m:1        (mpcData lives in the context)
  predMat(a, C, D, Np, Nc)           <- predMat.m:1        (A = diag(a), B = ones)
  constraintsMPC(lin, uk_1, SOCk_1)  <- constraintsMPC.m:1
  hildreth(E, F, M, gamma, lambda0, maxIter) <- hildreth.m:1
  runMPC(rom, SOC0, TC, nsteps)      <- runMPC.m:72-112    (fused, batched)

Errors: MATLAB ``error()`` becomes :class:`MpcekfError`; per-cell soft failures
(EKF lock-out, thetae < 0) set ``status`` bits and make that cell's outputs NaN.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import LIN_SIZE, MpcekfError, check, dptr, iptr
from .rom import EL_TABLES, OBS_FIELDS, ROM, TF_CODE

__all__ = ["Context", "DeviceBuffer", "hip_runtimes", "tc_grid", "make_config", "predMat", "constraintsMPC", "constraint_rows", "hildreth", "runMPC", "run_summary", "thermal_ocv", "MpcekfError",
           "LIN_SIZE"]

LIN_FIELDS = dict(A=slice(0, 6), Csoc=slice(6, 12), Dsoc=12, Cv=slice(13, 19), Dv=19,
                  Cphi=slice(20, 26), Dphi=26, bv=27, bphi=28, xhat=slice(29, 35))


def make_config(**kw) -> _lib.Config:
    """mpcekf_config with the runMPC.m defaults, overridden by keyword."""
    L = _lib.load()
    c = _lib.Config()
    L.mpcekf_config_defaults(C.byref(c))
    alias = {"targetSOC": "target_soc", "maxHild": "max_hild"}
    for k, v in kw.items():
        k = alias.get(k, k)
        if k == "constraints":
            c.use_current, c.use_voltage, c.use_eta = (int(x) for x in v)
        elif k == "SigmaX0":
            for i in range(6):
                c.SigmaX0[i] = float(v[i])
        elif k == "method":
            # initKF.m:44-49 blend selector: 'OB'/'OutB' (runMPC.m:16) or 'MB'/'MdlB'
            m = str(v).upper()
            if m not in ("OB", "OUTB", "MB", "MDLB"):
                raise ValueError(f"method {v!r}: expected 'OB' or 'MB' (initKF.m:44-49)")
            c.method = _lib.METHOD_MB if m in ("MB", "MDLB") else _lib.METHOD_OB
        elif k == "bounds":
            c.flags = (c.flags | _lib.CF_BOUNDS) if v else (c.flags & ~_lib.CF_BOUNDS)
        else:
            if not hasattr(c, k):
                raise TypeError(f"unknown config field {k}")
            setattr(c, k, type(getattr(c, k))(v))
    return c


class _PackedRom:
    def __init__(self, rom: ROM):
        self.keep = []

        def arr(x, dt=np.float64):
            a = np.ascontiguousarray(x, dtype=dt)
            self.keep.append(a)
            return a

        r = _lib.Rom()
        r.nT, r.nZ, r.n, r.nz = rom.nT, rom.nZ, rom.n, rom.nz
        r.T_degC = dptr(arr(rom.T_degC))
        r.SOC_pct = dptr(arr(rom.SOC_pct))
        r.Ts = rom.Ts
        r.A = dptr(arr(rom.A))
        r.C = dptr(arr(rom.C))
        r.D = dptr(arr(rom.D))
        r.tf_code = iptr(arr([TF_CODE[n] for n in rom.names], np.int32))
        r.tf_xloc = dptr(arr(rom.xloc))
        r.F, r.R, r.Q, r.Rc, r.Tref = rom.F, rom.R, rom.Q, rom.Rc, rom.Tref
        r.tab_ntheta, r.tab_ntemp = rom.ntheta, rom.ntemp
        r.tab_T_K = dptr(arr(np.atleast_1d(rom.tab_T_K)))
        for side in ("neg", "pos"):
            e = getattr(rom, side)
            s = getattr(r, side)
            s.theta0, s.theta100 = e.theta0, e.theta100
            for k in ("soc0", "soc100", "Uocp", "dUocp", "k0", "Rf", "Cdleff", "Uocp1"):
                setattr(s, k, dptr(arr(getattr(e, k))))
            for k in EL_TABLES + ("Uocp1",):    # ABI v3 theta polynomials (NULL: v2 linear tables)
                has = bool(e.poly) and k in e.poly
                setattr(s, k + "_p", dptr(arr(e.poly[k])) if has else _lib._dp())
            for i, k in enumerate(EL_TABLES):  # ABI v3 Arrhenius energies (0: none)
                s.Ea[i] = float((e.Ea or {}).get(k, 0.0))
            for i, k in enumerate(EL_TABLES + ("Uocp1",)):  # ABI v4: functions on their own nodes
                if e.nodes and k in e.nodes:
                    x, c = e.nodes[k]
                    c = np.asarray(c, dtype=np.float64)
                    if c.shape[-1] < rom.npoly:   # one coefficient count (tab_npoly): zero-padded
                        c = np.concatenate([c, np.zeros(c.shape[:-1] + (rom.npoly - c.shape[-1],))], -1)
                    s.nnode[i] = int(np.asarray(x).size)
                    s.node[i] = dptr(arr(x))
                    s.node_p[i] = dptr(arr(c))
        r.tab_npoly = rom.npoly
        self.s = r


def tc_grid(tc, nsteps, ncells):
    """A temperature argument as the [nsteps, ncells] grid of per-step TC (degC): a scalar,
    a 1-D per-step profile [nsteps] or per-cell vector [ncells], [nsteps, 1], [1, ncells]
    or the full array.  A 1-D vector whose length is both nsteps and ncells is ambiguous
    and refused (oracle/oracle_c.py reads temperature arguments by the same rule)."""
    a = np.asarray(tc, dtype=np.float64)
    if a.ndim == 1 and a.size != 1:
        if a.size == nsteps and a.size == ncells:
            raise ValueError(f"tc: a 1-D vector of length {a.size} = nsteps = ncells is ambiguous; "
                             "pass [nsteps, 1] (per step) or [1, ncells] (per cell)")
        if a.size == nsteps:
            a = a.reshape(nsteps, 1)
        elif a.size == ncells:
            a = a.reshape(1, ncells)
        else:
            raise ValueError(f"tc: length {a.size} is neither nsteps ({nsteps}) nor ncells ({ncells})")
    return np.ascontiguousarray(np.broadcast_to(a, (nsteps, ncells)))


class DeviceBuffer:
    """A C-contiguous device array allocated by the library's own HIP runtime
    (mpcekf_dev_alloc), for outputs_on_device calls: the host process then holds one
    HIP runtime only, and no foreign runtime's pointers reach the kernels."""

    def __init__(self, shape, dtype=np.float64, device=0):
        self.L = _lib.load()
        self.shape = tuple(int(x) for x in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        check(self.L.mpcekf_dev_alloc(int(device), self.nbytes, C.byref(p)))
        self.ptr = p.value or 0

    def free(self):
        if getattr(self, "ptr", 0):
            self.L.mpcekf_dev_free(C.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()

    def row_bytes(self):
        return self.nbytes // self.shape[0] if self.shape and self.shape[0] else 0

    def to_host(self, rows=None):
        """The first ``rows`` leading-axis rows (default all) as a numpy array."""
        rows = self.shape[0] if rows is None else int(rows)
        if not 0 <= rows <= self.shape[0]:
            raise ValueError(f"to_host: rows = {rows} outside [0, {self.shape[0]}]")
        out = np.empty((rows,) + self.shape[1:], dtype=self.dtype)
        check(self.L.mpcekf_dev_copy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), out.nbytes,
                                     _lib.COPY_D2H))
        return out

    def sampled(self, rows, stride):
        """[rows, ncells] buffer -> its every ``stride``-th column of the first ``rows`` rows
        (a pitched device-to-host copy: only the sampled elements cross PCIe)."""
        if len(self.shape) != 2 or stride < 1 or self.shape[1] % stride:
            raise ValueError("sampled: 2-D buffer with ncells divisible by stride expected")
        n = self.shape[1]
        rows = int(rows)
        if not 0 <= rows <= self.shape[0]:
            raise ValueError(f"sampled: rows = {rows} outside [0, {self.shape[0]}]")
        it = self.dtype.itemsize
        out = np.empty((rows, n // stride), dtype=self.dtype)
        check(self.L.mpcekf_dev_copy2d(out.ctypes.data_as(C.c_void_p), it, C.c_void_p(self.ptr), stride * it, it,
                                       rows * (n // stride), _lib.COPY_D2H))
        return out

    def from_host(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if a.nbytes > self.nbytes:
            raise ValueError("from_host: array larger than the buffer")
        check(self.L.mpcekf_dev_copy(C.c_void_p(self.ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, _lib.COPY_H2D))


def hip_runtimes():
    """Paths of the HIP / HSA runtime libraries mapped into this process ({'hip': [...],
    'hsa': [...]}): one of each when the library's runtime is the only one."""
    out = {"hip": set(), "hsa": set()}
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                p = line.split()[-1] if line.split() else ""
                if "libamdhip64" in p:
                    out["hip"].add(p)
                elif "libhsa-runtime64" in p:
                    out["hsa"].add(p)
    except OSError:
        pass
    return {k: sorted(v) for k, v in out.items()}


class Context:
    """One device, one stream, ``ncells`` independent cells (mpcekf_ctx)."""

    def __init__(self, rom: ROM, ncells: int, cfg: _lib.Config | None = None, device: int = 0):
        self.L = _lib.load()
        self.rom = rom
        self.cfg = cfg if cfg is not None else make_config()
        self.device = device
        self._pr = _PackedRom(rom)
        h = C.c_void_p()
        check(self.L.mpcekf_ctx_create(C.byref(self._pr.s), C.byref(self.cfg), device, int(ncells), C.byref(h)))
        self.h = h
        n, nm, nz, nc = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
        check(self.L.mpcekf_ctx_info(h, C.byref(n), C.byref(nm), C.byref(nz), C.byref(nc)))
        self.n, self.NM, self.nz, self.ncon = n.value, nm.value, nz.value, nc.value
        # asynchronous = True: the stage functions below call the _async C-ABI twins (SURVEY.md
        # §8(b)): they return before their host outputs are written; sync() (or any synchronous
        # stage call) completes them.  The output arrays are held here until then.
        self.asynchronous = False
        self._pending = []

    def _stage(self, name, *args, keep=()):
        """One stage entry point: mpcekf_<name>, or mpcekf_<name>_async in asynchronous mode
        (its output arrays `keep` held until the synchronisation)."""
        if self.asynchronous:
            check(getattr(self.L, f"mpcekf_{name}_async")(self.h, *args))
            self._pending.append(keep)
        else:
            check(getattr(self.L, f"mpcekf_{name}")(self.h, *args))
            self._pending.clear()

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.L.mpcekf_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _vec(self, x, dtype=np.float64):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=dtype), (self.n,)))
        return a

    # -- initKF / initMPC / first OB_step --------------------------------
    def init_cells(self, soc0_pct, tc_degC):
        s = self._vec(soc0_pct)
        t = self._vec(tc_degC)
        check(self.L.mpcekf_init_cells(self.h, dptr(s), dptr(t)))
        self._soc0 = s / 100.0   # limit_map's default z0 (the unit of step()'s soc) until a fused step has run

    # -- fused loop (runMPC.m:83-112) ------------------------------------
    # runMPC.m stores per step: name -> (dtype, trailing shape); see mpcekf_traj
    TRAJ_FIELDS = dict(u=(np.float64, ()), v=(np.float64, ()), soc=(np.float64, ()), phise=(np.float64, ()),
                       nexec=(np.int32, ()), x=(np.float64, (6,)), zk=(np.float64, None),
                       zbk=(np.float64, None), J_unc=(np.float64, ()), J_fin=(np.float64, ()),
                       norm_du=(np.float64, ()), nviol=(np.int32, ()), poles=(np.float64, (7, 2)),
                       sv=(np.float64, (7,)))
    # the optional per-step rows of step(thermal=..., pack=...): name -> (one element per string and
    # step instead of per cell and step, dtype)
    STEP_ROWS = dict(temp=(False, np.float64), heat=(False, np.float64), cond=(False, np.float64),
                     ucmd=(False, np.float64), bleed=(False, np.float64), zmin=(True, np.float64),
                     vstr=(True, np.float64), istr=(True, np.float64), limiter=(True, np.int32),
                     capby=(True, np.int32))

    def step(self, nsteps, outputs=("u", "v", "soc", "phise", "nexec"), tc=None, obs=None, thermal=None, pack=None,
             aging=None, limit_map=None):
        """nsteps fused closed-loop steps (runMPC.m:83-112).  ``outputs`` names the per-step
        stores to return as [nsteps, ncells(, k)] arrays: u, v, soc, phise, nexec, and the
        diagnostics x (x_store), zk / zbk (zkEst / zkBound), J_unc, J_fin, norm_du, nviol
        (mpcData.cost), poles ([.., 7, 2] re/im of eig(CL)) and sv (svd(CL)), the stability
        diagnostics of iterMPC.m:53-60 (returned as complex [nsteps, ncells, 7] for poles).
        ``tc``: the TC of each step in degC (runMPC.m:85-92), see :func:`tc_grid`; None keeps
        every cell's current temperature.
        ``obs``: the plant's own observables of every step (OB_step's obs struct on the state
        each step starts from; ``phise`` above is the EKF's estimate): True for every field,
        or a field name / tuple of names as OB_step(obs=...) takes them.  Adds out["obs"], a
        dict field -> [nsteps, ncells] (scalar fields) or [nsteps, ncells, len] (vector
        fields); only the selected slots are computed and copied.  None: the call as it was.
        ``thermal``: on a context with a thermal model (thermal_begin), the model's per-step rows
        to return as [nsteps, ncells] arrays: "temp" (the temperature each step used) and / or
        "heat" (the heat it generated, W); mpcekf_step_ex_thermal.  On a context with links
        (thermal_couple) also "cond" (the heat the cell's neighbours conducted to it, W; +0.0 for a
        cell without a link); mpcekf_step_ex_couple.  None: the call as it was.
        ``pack``: on a pack context (pack_begin), the pack's per-step rows to return: "ucmd"
        [nsteps, ncells], each cell's own command before its string's reduction (``u`` holds the
        applied current), and / or "limiter" [nsteps, ncells // series] int32, each string's
        limiter as an in-string index or -1; mpcekf_step_ex_pack.  None: the call as it was (a
        pack context couples its strings all the same).  On a context with a balancer
        (balance_begin) also "bleed" [nsteps, ncells], each cell's bleed current (NaN for a cell
        with a NaN command), and / or "zmin" [nsteps, ncells // series], each string's smallest
        soc; mpcekf_step_ex_balance, which has no "cond" or "rate" row.  On a context with a charger
        (charger_begin) also "vstr", "istr" [nsteps, ncells // series], each string's voltage and
        its current after the charger's caps, and / or "capby" (int32: -1 no current, 0 not capped,
        1 the current cap, 2 the power cap); mpcekf_step_ex_charger, which has no "cond" or "rate"
        row either.
        ``aging``: on an aging context (aging_begin), ("rate",) returns out["rate"]
        [nsteps, nsrc * nreact, ncells], every step's side-reaction currents (A): the enabled
        sources in the order est, plant, the reactions inside; mpcekf_step_ex_aging.  None: the
        call as it was (an aging context accumulates its record all the same).
        ``limit_map``: on a context with a limit map (limit_map), ("lim",) returns out["lim"]
        [nsteps, nfields, ncells], the mapped fields' values the MPC stage of every step read, in
        the order the map named them; mpcekf_step_ex_map, which takes every thermal and pack row
        above but has no "cond" or "rate" row.  None: the call as it was (the map is evaluated all
        the same)."""
        n = self.n
        lm = () if limit_map is None else (limit_map,) if isinstance(limit_map, str) else tuple(limit_map)
        for k in lm:
            if k != "lim":
                raise KeyError(f"step: unknown limit_map row {k!r} (one of ('lim',))")
        if limit_map is not None and (aging is not None or (thermal is not None and "cond" in
                                                            ((thermal,) if isinstance(thermal, str) else tuple(thermal)))):
            raise ValueError("step: the map's row (lim) comes from mpcekf_step_ex_map, which has no cond or rate row")
        fields, slots = self._obs_select(obs, "step")   # KeyError before any library call
        th = () if thermal is None else (thermal,) if isinstance(thermal, str) else tuple(thermal)
        for k in th:
            if k not in ("temp", "heat", "cond"):
                raise KeyError(f"step: unknown thermal row {k!r} (one of ('temp', 'heat', 'cond'))")
        if thermal is not None and tc is not None:
            raise ValueError("step: thermal rows come from the model, which takes no tc")
        pk = () if pack is None else (pack,) if isinstance(pack, str) else tuple(pack)
        for k in pk:
            if k not in ("ucmd", "limiter", "bleed", "zmin", "vstr", "istr", "capby"):
                raise KeyError(f"step: unknown pack row {k!r} (one of ('ucmd', 'limiter', 'bleed', 'zmin', 'vstr', "
                               "'istr', 'capby'))")
        bal = "bleed" in pk or "zmin" in pk
        chg = "vstr" in pk or "istr" in pk or "capby" in pk
        if bal and not chg and ("cond" in th or aging is not None):
            raise ValueError("step: the balancer's rows (bleed, zmin) come from mpcekf_step_ex_balance, which has no "
                             "cond or rate row")
        if chg and ("cond" in th or aging is not None):
            raise ValueError("step: the charger's rows (vstr, istr, capby) come from mpcekf_step_ex_charger, which has "
                             "no cond or rate row")
        ag = () if aging is None else (aging,) if isinstance(aging, str) else tuple(aging)
        for k in ag:
            if k != "rate":
                raise KeyError(f"step: unknown aging row {k!r} (one of ('rate',))")
        tcs = None if tc is None else tc_grid(tc, nsteps, n)
        out = {}
        tr = _lib.Traj()
        for k in outputs:
            if k not in self.TRAJ_FIELDS:
                raise KeyError(f"unknown output {k}")
            dt, tail = self.TRAJ_FIELDS[k]
            tail = (self.nz + 2,) if tail is None else tail
            out[k] = np.empty((nsteps, n) + tail, dtype=dt)
            setattr(tr, k, out[k].ctypes.data_as(C.c_void_p).value)
        tcp = tcs.ctypes.data_as(C.c_void_p) if tcs is not None else None
        rec = None if fields is None else np.empty((nsteps, slots.size, n))
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        # the optional rows the call names, per cell or per string (STEP_ROWS); rate has a shape of its own
        series = getattr(self, "_pack_series", 0)   # 0: no begin, the library refuses the call
        for k in th + pk:
            per_string, dt = self.STEP_ROWS[k]
            out[k] = np.empty((nsteps, n // series if per_string and series else n), dtype=dt)
        if "rate" in ag:
            nreact, mask = getattr(self, "_aging", (0, 0))   # (0, 0): no begin, the library refuses the call
            out["rate"] = np.empty((nsteps, max(bin(mask).count("1") * nreact, 1), n))
        if "lim" in lm:
            out["lim"] = np.empty((nsteps, max(getattr(self, "_map_nf", 0), 1), n))   # 0: no map, the library refuses
        row = lambda *names: tuple(vp(out.get(k)) for k in names)
        ns = 0 if fields is None else int(slots.size)
        head, tail = (self.h, int(nsteps)), (C.byref(tr), iptr(slots) if ns else None, ns, vp(rec) if ns else None)
        call = head + (tcp,) + tail
        # the entry point, in this order: it decides which refusal of the library a misuse gets
        if limit_map is not None:   # a mapped context, whatever else it carries
            check(self.L.mpcekf_step_ex_map(*call, *row("temp", "heat", "ucmd", "limiter", "bleed", "zmin", "vstr",
                                                        "istr", "capby", "lim"), 0))
        elif chg:   # a pack context with a charger (and a balancer, for bleed / zmin)
            check(self.L.mpcekf_step_ex_charger(*call, *row("temp", "heat", "ucmd", "limiter", "bleed", "zmin", "vstr",
                                                            "istr", "capby"), 0))
        elif bal:   # a pack context with a balancer
            check(self.L.mpcekf_step_ex_balance(*call, *row("temp", "heat", "ucmd", "limiter", "bleed", "zmin"), 0))
        elif "cond" in th:   # every row of a coupled context: it has a model and a pack
            check(self.L.mpcekf_step_ex_couple(*call, *row("temp", "heat", "ucmd", "limiter", "rate", "cond"), 0))
        elif aging is not None:
            check(self.L.mpcekf_step_ex_aging(*call, *row("temp", "heat", "ucmd", "limiter", "rate"), 0))
        elif pack is not None:
            check(self.L.mpcekf_step_ex_pack(*call, *row("temp", "heat", "ucmd", "limiter"), 0))
        elif thermal is not None:   # the model takes no tc
            check(self.L.mpcekf_step_ex_thermal(*head, *tail, *row("temp", "heat"), 0))
        elif fields is None:
            check(self.L.mpcekf_step_ex(self.h, int(nsteps), tcp, C.byref(tr), 0))
        elif slots.size:
            check(self.L.mpcekf_step_ex_obs(self.h, int(nsteps), tcp, C.byref(tr), iptr(slots), int(slots.size),
                                            rec.ctypes.data_as(C.c_void_p), 0))
        else:
            check(self.L.mpcekf_step_ex(self.h, int(nsteps), tcp, C.byref(tr), 0))
        self._stepped(nsteps)
        if fields is not None:
            lay, pos, out["obs"] = self.rom.obs_layout(), 0, {}
            for k in fields:   # slot-major rows per step -> [nsteps, n] / [nsteps, n, len]
                m = lay[k].stop - lay[k].start
                out["obs"][k] = rec[:, pos] if k in self._OBS_SCALARS else rec[:, pos:pos + m].transpose(0, 2, 1)
                pos += m
        if "poles" in out:
            out["poles"] = _complex(out["poles"])
        return out

    def _stepped(self, nsteps):
        """After a fused call: once a step has run, the SOC given to init_cells is no longer the
        estimate, so limit_map's default z0 is mpcekf_limit_map's own (NaN for a first map)."""
        if nsteps:
            self._soc0 = None

    def _obs_select(self, obs, who):
        """obs=None / True / name / names -> (fields, int32 slots of the record), (None, None)
        for None; an unknown field raises KeyError (the spelling rules of OB_step(obs=...))."""
        if obs is None or obs is False:
            return None, None
        lay = self.rom.obs_layout()
        fields = OBS_FIELDS if obs is True else (obs,) if isinstance(obs, str) else tuple(obs)
        for k in fields:
            if k not in lay:
                raise KeyError(f"{who}: unknown obs field {k!r} (one of {OBS_FIELDS})")
        slots = np.ascontiguousarray(np.concatenate([np.arange(lay[k].start, lay[k].stop) for k in fields] or [[]]),
                                     dtype=np.int32)
        return tuple(fields), slots

    def step_device(self, nsteps, u=0, v=0, soc=0, phise=0, nexec=0, obs=0, obs_slots=()):
        """Fused steps writing [nsteps][ncells] outputs to device pointers (ints or
        DeviceBuffer; allocate them with DeviceBuffer / mpcekf_dev_alloc).  ``obs``: a device
        buffer [nsteps][len(obs_slots)][ncells] for the slots ``obs_slots`` of the plant's
        observable record at every step (mpcekf_step_ex_obs)."""
        p = [C.c_void_p(x.ptr if isinstance(x, DeviceBuffer) else x) if x else None for x in (u, v, soc, phise, nexec)]
        sl = np.ascontiguousarray(obs_slots, dtype=np.int32).ravel()
        if not obs and not sl.size:
            check(self.L.mpcekf_step(self.h, int(nsteps), None, *p, 1))
            self._stepped(nsteps)
            return
        tr = _lib.Traj()
        for k, x in zip(("u", "v", "soc", "phise", "nexec"), p):
            setattr(tr, k, x.value if x is not None else None)
        op = C.c_void_p(obs.ptr if isinstance(obs, DeviceBuffer) else obs) if obs else None
        check(self.L.mpcekf_step_ex_obs(self.h, int(nsteps), None, C.byref(tr), iptr(sl) if sl.size else None,
                                        int(sl.size), op, 1))
        self._stepped(nsteps)

    def sync(self):
        """Wait for every launch on the context's device and complete the asynchronous stage
        calls' host outputs (mpcekf_sync)."""
        check(self.L.mpcekf_sync(self.h))
        self._pending.clear()

    def set_graph(self, enable=True):
        """Replay repeated fused-call shapes from captured hipGraphs (mpcekf_set_graph)."""
        check(self.L.mpcekf_set_graph(self.h, int(bool(enable))))

    # -- per-cell limits and targets (runMPC.m:30-44 per cell) ------------
    LIMIT_FIELDS = _lib.LIMIT_FIELDS

    @classmethod
    def _limit_arrays(cls, n, fields):
        """set_limits' keywords -> (int32 field ids, float64 [len, n] values); ValueError for
        an unknown keyword, no keyword at all, or a value that is neither a scalar nor [n]."""
        if not fields:
            raise ValueError(f"set_limits: no field given (one of {cls.LIMIT_FIELDS})")
        alias = {"targetSOC": "target_soc"}
        ids, rows = [], []
        for k, v in fields.items():
            k = alias.get(k, k)
            if k not in cls.LIMIT_FIELDS:
                raise ValueError(f"set_limits: unknown field {k!r} (one of {cls.LIMIT_FIELDS})")
            if cls.LIMIT_FIELDS.index(k) in ids:
                raise ValueError(f"set_limits: field {k!r} given twice")
            a = np.asarray(v, dtype=np.float64)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n):
                raise ValueError(f"set_limits: {k} must be a scalar or a length-{n} array, got shape {a.shape}")
            ids.append(cls.LIMIT_FIELDS.index(k))
            rows.append(np.broadcast_to(a, (n,)))
        return np.asarray(ids, dtype=np.int32), np.ascontiguousarray(np.stack(rows), dtype=np.float64)

    def set_limits(self, **fields):
        """mpcData.ref / mpcData.const of runMPC.m:30-44 per cell (mpcekf_set_limits): keywords
        target_soc, Crate, u_max, du_min, du_max, v_max, phise_min, z_max, z_tol in make_config's
        units, each a scalar (broadcast) or a length-ncells array.  A field not named keeps what
        it had (the configuration's scalar, or an earlier set_limits).  Takes effect at the next
        MPC stage, mid-charge included."""
        ids, vals = self._limit_arrays(self.n, fields)   # ValueError before any library call
        check(self.L.mpcekf_set_limits(self.h, int(ids.size), iptr(ids), dptr(vals)))

    def get_limits(self):
        """{field: [ncells]} of the limits in force (mpcekf_get_limits): what set_limits stored,
        the configuration's scalar for a field never set."""
        ids = np.arange(len(self.LIMIT_FIELDS), dtype=np.int32)
        vals = np.empty((ids.size, self.n))
        check(self.L.mpcekf_get_limits(self.h, int(ids.size), iptr(ids), dptr(vals)))
        return {k: vals[i] for i, k in enumerate(self.LIMIT_FIELDS)}

    def clear_limits(self):
        """Back to the configuration's scalars and the launch sequence before the first
        set_limits (mpcekf_clear_limits)."""
        check(self.L.mpcekf_clear_limits(self.h))

    # -- per-cell charge summary along the fused loop ---------------------
    SUMMARY_FIELDS = _lib.SUMMARY_FIELDS

    def _summary_args(self, reach, obs):
        """summary_begin's arguments -> (float64 [n] thresholds or None, int32 slot or -1).  obs:
        a scalar field name of OB_step's obs, or (vector field, index).  KeyError for a field
        that is not one, ValueError for a bad shape or index: before any library call."""
        r = None
        if reach is not None:
            a = np.asarray(reach, dtype=np.float64)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != self.n):
                raise ValueError(f"summary_begin: reach must be a scalar or a length-{self.n} array, got shape {a.shape}")
            r = np.ascontiguousarray(np.broadcast_to(a, (self.n,)))
        slot = -1
        if obs is not None:
            name, idx = (obs, None) if isinstance(obs, str) else tuple(obs)
            lay = self.rom.obs_layout()
            if name not in lay:
                raise KeyError(f"summary_begin: unknown obs field {name!r} (one of {OBS_FIELDS})")
            m = lay[name].stop - lay[name].start
            if name in self._OBS_SCALARS:
                if idx not in (None, 0):
                    raise ValueError(f"summary_begin: obs field {name!r} is a scalar: no index {idx!r}")
                idx = 0
            elif idx is None or int(idx) != idx or not 0 <= int(idx) < m:
                raise ValueError(f"summary_begin: obs field {name!r} has {m} entries: give (field, index), 0-based")
            slot = lay[name].start + int(idx)
        return r, slot

    def summary_begin(self, reach=None, obs=None):
        """Start (or reset) the per-cell charge summary (mpcekf_summary_begin).  ``reach``: the
        SOC whose first crossing T_REACH records, a scalar or [ncells], in the unit of step()'s
        ``soc`` (zk(end): a fraction 0..1), None for none.  ``obs``: one slot of the plant's
        observables to track beside the EKF's outputs, e.g. "negPhise0" (the plant's own
        plating margin) or ("Thetae", 1); None for none."""
        r, slot = self._summary_args(reach, obs)   # KeyError / ValueError before any library call
        check(self.L.mpcekf_summary_begin(self.h, dptr(r), int(slot)))

    def step_summary(self, nsteps, tc=None):
        """nsteps fused steps (step()'s, tc as there) accumulated into the summary record; no
        trajectory is returned and none is kept (mpcekf_step_summary)."""
        tcs = None if tc is None else tc_grid(tc, nsteps, self.n)
        check(self.L.mpcekf_step_summary(self.h, int(nsteps), tcs.ctypes.data_as(C.c_void_p) if tcs is not None else None))
        self._stepped(nsteps)

    def get_summary(self, fields=None):
        """{name: [ncells] float64} of the summary record (mpcekf_get_summary): ``fields`` names
        of SUMMARY_FIELDS (default all).  Step indices and counts are exact integers."""
        names = self.SUMMARY_FIELDS if fields is None else (fields,) if isinstance(fields, str) else tuple(fields)
        for k in names:
            if k not in self.SUMMARY_FIELDS:
                raise KeyError(f"get_summary: unknown field {k!r} (one of {self.SUMMARY_FIELDS})")
        ids = np.asarray([self.SUMMARY_FIELDS.index(k) for k in names], dtype=np.int32)
        vals = np.empty((ids.size, self.n))
        check(self.L.mpcekf_get_summary(self.h, int(ids.size), iptr(ids), dptr(vals)))
        return {k: vals[i] for i, k in enumerate(names)}

    def summary_end(self):
        """Free the summary record and its window (mpcekf_summary_end)."""
        check(self.L.mpcekf_summary_end(self.h))

    # -- per-cell lumped thermal model along the fused loop ----------------
    THERMAL_PARAMS = _lib.THERMAL_PARAMS
    THERMAL_FIELDS = _lib.THERMAL_FIELDS

    @staticmethod
    def _per_cell(n, name, v, who="thermal_begin"):
        """A scalar or a length-n array -> float64 [n]; ValueError for any other shape."""
        a = np.asarray(v, dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n):
            raise ValueError(f"{who}: {name} must be a scalar or a length-{n} array, got shape {a.shape}")
        return np.broadcast_to(a, (n,))

    def thermal_begin(self, Cth, Rth, Tamb, ocv, T0=None):
        """Give the context a per-cell lumped thermal model (mpcekf_thermal_begin): heat capacity
        ``Cth`` (J/K), thermal resistance to the ambient ``Rth`` (K/W, np.inf: adiabatic) and
        ambient temperature ``Tamb`` (degC), each a scalar or [ncells]; ``ocv``: the open-circuit
        voltage on a uniform grid of cell SOC 0..1 (see :func:`thermal_ocv`); ``T0`` (degC,
        scalar or [ncells]): the temperature to start from, None keeps the cells' own.  From then
        on every fused call advances each cell's temperature after every step (and takes no
        ``tc``); a second call replaces the model and resets its record."""
        n = self.n
        par = np.ascontiguousarray(np.stack([self._per_cell(n, k, v) for k, v in
                                             zip(self.THERMAL_PARAMS, (Cth, Rth, Tamb))]), dtype=np.float64)
        tab = np.ascontiguousarray(ocv, dtype=np.float64)
        if tab.ndim != 1:
            raise ValueError(f"thermal_begin: ocv must be a 1-D table, got shape {tab.shape}")
        t0 = None if T0 is None else np.ascontiguousarray(self._per_cell(n, "T0", T0))
        check(self.L.mpcekf_thermal_begin(self.h, dptr(par), int(tab.size), dptr(tab), dptr(t0)))

    def thermal_get(self, fields=None):
        """{name: [ncells] float64} of the thermal record (mpcekf_thermal_get): ``fields`` names of
        THERMAL_FIELDS (default all).  Step indices and counts are exact integers."""
        names = self.THERMAL_FIELDS if fields is None else (fields,) if isinstance(fields, str) else tuple(fields)
        for k in names:
            if k not in self.THERMAL_FIELDS:
                raise KeyError(f"thermal_get: unknown field {k!r} (one of {self.THERMAL_FIELDS})")
        ids = np.asarray([self.THERMAL_FIELDS.index(k) for k in names], dtype=np.int32)
        vals = np.empty((ids.size, self.n))
        check(self.L.mpcekf_thermal_get(self.h, int(ids.size), iptr(ids), dptr(vals)))
        return {k: vals[i] for i, k in enumerate(names)}

    def thermal_end(self):
        """Drop the thermal model (mpcekf_thermal_end): the cells keep their temperature; a
        schedule over it ends too."""
        check(self.L.mpcekf_thermal_end(self.h))
        if getattr(self, "_map_nt", 1) > 1:   # a map with a temperature axis ended with the model
            self._map_nf, self._map_nt = 0, 1

    SCHEDULE_FIELDS = _lib.SCHEDULE_FIELDS

    @classmethod
    def _schedule_arrays(cls, n, T_lo, T_hi, sets, tables):
        """thermal_schedule's arguments -> (int32 ids [nf], float64 tables [nsets][nf][ntab],
        int32 set_of_cell [n] or None).  ValueError for an unknown, repeated or unschedulable
        field, no field at all, tables of different shapes, a table that is neither [ntab] nor
        [nsets][ntab], or a ``sets`` that is not a length-n integer array: before any library
        call.  The values themselves (grid ends, finiteness, set indices) are the library's to
        check."""
        if not tables:
            raise ValueError(f"thermal_schedule: no field given (one of {cls.SCHEDULE_FIELDS})")
        ids, tabs = [], []
        for k, v in tables.items():
            if k not in cls.LIMIT_FIELDS and k != "targetSOC":
                raise ValueError(f"thermal_schedule: unknown field {k!r} (one of {cls.SCHEDULE_FIELDS})")
            if k not in cls.SCHEDULE_FIELDS:
                raise ValueError(f"thermal_schedule: field {k!r} cannot be scheduled (one of {cls.SCHEDULE_FIELDS})")
            a = np.asarray(v, dtype=np.float64)
            if a.ndim not in (1, 2):
                raise ValueError(f"thermal_schedule: {k} must be a [ntab] or [nsets][ntab] table, got shape {a.shape}")
            ids.append(cls.LIMIT_FIELDS.index(k))
            tabs.append(a)
        two = [a for a in tabs if a.ndim == 2]
        nsets = two[0].shape[0] if two else 1
        ntab = tabs[0].shape[-1]
        for k, a in zip(tables, tabs):
            if a.shape[-1] != ntab or (a.ndim == 2 and a.shape[0] != nsets):
                raise ValueError(f"thermal_schedule: {k} has shape {a.shape}: every table is [{ntab}] or [{nsets}][{ntab}] here")
        if nsets < 1 or ntab < 1:
            raise ValueError(f"thermal_schedule: empty tables ({nsets} sets of {ntab} entries)")
        # [nf][nsets][ntab] -> [nsets][nf][ntab]; a [ntab] table serves every set
        tab = np.stack([np.broadcast_to(a, (nsets, ntab)) for a in tabs]).transpose(1, 0, 2)
        soc = None
        if sets is not None:
            soc = np.asarray(sets)
            if soc.shape != (n,) or not np.issubdtype(soc.dtype, np.integer):
                raise ValueError(f"thermal_schedule: sets must be a length-{n} integer array, got shape {soc.shape} "
                                 f"of {soc.dtype}")
            soc = np.ascontiguousarray(soc, dtype=np.int32)
        return np.asarray(ids, dtype=np.int32), np.ascontiguousarray(tab, dtype=np.float64), soc

    def thermal_schedule(self, T_lo, T_hi, sets=None, **tables):
        """Schedule MPC limits over the thermal model's temperature (mpcekf_thermal_schedule):
        each keyword is a limit field's name as in set_limits (Crate, u_max, du_min, du_max,
        v_max, phise_min; make_config's units) with a table over the uniform grid ``T_lo`` ..
        ``T_hi`` (degC), [ntab] or, for several derating maps in one batch, [nsets][ntab] with
        ``sets`` [ncells] naming each cell's map (None: map 0).  From then on the MPC stage of
        every fused step reads, per cell, the table value at the temperature the step used
        (clamped to the grid's ends, linear between knots); get_limits returns the values in
        force.  Needs thermal_begin; a second call replaces the schedule."""
        ids, tab, soc = self._schedule_arrays(self.n, T_lo, T_hi, sets, tables)   # ValueError before any library call
        check(self.L.mpcekf_thermal_schedule(self.h, int(ids.size), iptr(ids), int(tab.shape[2]), float(T_lo),
                                             float(T_hi), int(tab.shape[0]), dptr(tab), iptr(soc)))

    def thermal_schedule_end(self):
        """End the schedule (mpcekf_thermal_schedule_end): its fields go back to what set_limits
        or the configuration gave them."""
        check(self.L.mpcekf_thermal_schedule_end(self.h))

    # -- MPC limits mapped over the SOC estimate and the temperature ---------
    LIMIT_MAP_FIELDS = _lib.LIMIT_MAP_FIELDS

    @classmethod
    def _map_arrays(cls, n, sets, interp_z, z0, tables):
        """limit_map's arguments -> (int32 ids [nf], float64 tables [nsets][nf][nt][nz], int32
        set_of_cell [n] or None, interp_z 0 / 1, float64 z0 [n] or None).  A table is [nz] (no
        temperature axis), [nt][nz] or [nsets][nt][nz].  ValueError for an unknown, repeated or
        unmappable field, no field at all, tables of different shapes, a bad ``sets``, ``interp_z``
        or ``z0`` shape: before any library call.  The values themselves are the library's to
        check."""
        if not tables:
            raise ValueError(f"limit_map: no field given (one of {cls.SCHEDULE_FIELDS})")
        if interp_z not in ("linear", "hold", 0, 1):
            raise ValueError(f"limit_map: interp_z = {interp_z!r}: 'linear' or 'hold'")
        ids, tabs = [], []
        for k, v in tables.items():
            if k not in cls.SCHEDULE_FIELDS:
                raise ValueError(f"limit_map: field {k!r} cannot be mapped (one of {cls.SCHEDULE_FIELDS})")
            a = np.asarray(v, dtype=np.float64)
            if a.ndim not in (1, 2, 3):
                raise ValueError(f"limit_map: {k} must be a [nz], [nt][nz] or [nsets][nt][nz] table, got shape {a.shape}")
            ids.append(cls.LIMIT_FIELDS.index(k))
            tabs.append(a)
        three = [a for a in tabs if a.ndim == 3]
        two = [a for a in tabs if a.ndim >= 2]
        nsets = three[0].shape[0] if three else 1
        nt = two[0].shape[-2] if two else 1
        nz = tabs[0].shape[-1]
        for k, a in zip(tables, tabs):
            if a.shape[-1] != nz or (a.ndim >= 2 and a.shape[-2] != nt) or (a.ndim == 3 and a.shape[0] != nsets):
                raise ValueError(f"limit_map: {k} has shape {a.shape}: every table is [{nz}], [{nt}][{nz}] or "
                                 f"[{nsets}][{nt}][{nz}] here")
        if nsets < 1 or nt < 1 or nz < 1:
            raise ValueError(f"limit_map: empty tables ({nsets} sets of {nt} x {nz} entries)")
        # [nf][nsets][nt][nz] -> [nsets][nf][nt][nz]; a smaller table serves every set / temperature
        tab = np.stack([np.broadcast_to(a, (nsets, nt, nz)) for a in tabs]).transpose(1, 0, 2, 3)
        soc = None
        if sets is not None:
            soc = np.asarray(sets)
            if soc.shape != (n,) or not np.issubdtype(soc.dtype, np.integer):
                raise ValueError(f"limit_map: sets must be a length-{n} integer array, got shape {soc.shape} of {soc.dtype}")
            soc = np.ascontiguousarray(soc, dtype=np.int32)
        z = None if z0 is None else np.ascontiguousarray(cls._per_cell(n, "z0", z0, "limit_map"))
        return (np.asarray(ids, dtype=np.int32), np.ascontiguousarray(tab, dtype=np.float64), soc,
                int(interp_z in ("hold", 1)), z)

    def limit_map(self, z_lo, z_hi, T_lo=None, T_hi=None, sets=None, interp_z="linear", z0=None, **tables):
        """Map MPC limits over (SOC estimate, cell temperature) (mpcekf_limit_map): each keyword is
        a limit field's name as in set_limits (Crate, u_max, du_min, du_max, v_max, phise_min;
        make_config's units) with a table on the uniform grids ``z_lo`` .. ``z_hi`` (SOC fraction,
        the unit of step()'s ``soc``) and ``T_lo`` .. ``T_hi`` (degC): [nz] (no temperature axis:
        any context), [nt][nz] (needs thermal_begin) or, for several maps in one batch,
        [nsets][nt][nz] with ``sets`` [ncells] naming each cell's map (None: map 0).
        ``interp_z``: "linear", or "hold" for the left node's value (see :func:`mscc_map`); the
        temperature axis is linear.  From then on the MPC stage of every fused step reads, per
        cell, the table value at the previous step's ``soc`` and the temperature the step uses,
        clamped to the grids' ends.  ``z0`` (scalar or [ncells]): the SOC to evaluate at until a
        fused step has run.  None: when the call replaces an active map, the record's z_last as it
        stands; else the SOC given to init_cells if no fused step has run since; else NaN, the
        first column, as mpcekf_limit_map's NULL (a map set on a context that has stepped without
        one, after limit_map_end for instance: pass the last ``soc`` row as z0 to start from it).
        get_limits returns the values in force; a second call replaces the map."""
        ids, tab, soc, hold, z = self._map_arrays(self.n, sets, interp_z, z0, tables)   # ValueError before any library call
        nt = tab.shape[2]
        if nt > 1 and (T_lo is None or T_hi is None):
            raise ValueError("limit_map: tables with a temperature axis need T_lo and T_hi")
        if z is None and not getattr(self, "_map_nf", 0) and getattr(self, "_soc0", None) is not None:
            z = np.ascontiguousarray(self._soc0)
        check(self.L.mpcekf_limit_map(self.h, int(ids.size), iptr(ids), int(tab.shape[3]), float(z_lo), float(z_hi),
                                      int(nt), float(0.0 if T_lo is None else T_lo), float(1.0 if T_hi is None else T_hi),
                                      hold, int(tab.shape[0]), dptr(tab), iptr(soc), dptr(z)))
        self._map_nf, self._map_nt = int(ids.size), int(nt)

    def limit_map_get(self, fields=None):
        """{name: [ncells] float64} of the map's record (mpcekf_limit_map_get): ``fields`` names of
        LIMIT_MAP_FIELDS (default all).  Counts are exact integers."""
        names = self.LIMIT_MAP_FIELDS if fields is None else (fields,) if isinstance(fields, str) else tuple(fields)
        for k in names:
            if k not in self.LIMIT_MAP_FIELDS:
                raise KeyError(f"limit_map_get: unknown field {k!r} (one of {self.LIMIT_MAP_FIELDS})")
        ids = np.asarray([self.LIMIT_MAP_FIELDS.index(k) for k in names], dtype=np.int32)
        vals = np.empty((ids.size, self.n))
        check(self.L.mpcekf_limit_map_get(self.h, int(ids.size), iptr(ids), dptr(vals)))
        return {k: vals[i] for i, k in enumerate(names)}

    def limit_map_end(self):
        """End the map (mpcekf_limit_map_end): its fields go back to what set_limits or the
        configuration gave them."""
        check(self.L.mpcekf_limit_map_end(self.h))
        self._map_nf = 0

    # -- heat conduction between neighbouring cells of a pack string --------
    COUPLE_FIELDS = ("NB_SUM", "DT_MAX", "DT_MAX_STEP")   # include/mpcekf.h MPCEKF_TCR_*

    @staticmethod
    def _couple_links(n, R_link):
        """thermal_couple's argument -> float64 [n]; every check mpcekf_thermal_couple makes on
        the links, before the library is called."""
        r = np.asarray(R_link, dtype=np.float64)
        if r.ndim == 0:
            r = np.full(n, float(r))
        if r.shape != (n,):
            raise ValueError(f"thermal_couple: R_link must be a scalar or a length-{n} array, got shape {r.shape}")
        r = np.ascontiguousarray(r)
        if not np.all(r > 0):   # NaN fails the comparison
            raise ValueError("thermal_couple: R_link must be > 0 (K/W; np.inf: no link) and not NaN")
        return r

    def thermal_couple(self, R_link):
        """Link neighbouring cells of every pack string thermally (mpcekf_thermal_couple):
        ``R_link`` (K/W, a scalar or [ncells]) is the resistance between cell c and cell c + 1,
        used where both are in one string; np.inf: no link.  Needs thermal_begin and pack_begin.
        From then on every fused call conducts heat between the linked cells; a second call
        replaces the links and resets the coupling's record."""
        r = self._couple_links(self.n, R_link)
        check(self.L.mpcekf_thermal_couple(self.h, dptr(r)))

    def thermal_couple_get(self, fields=None):
        """{name: [ncells] float64} of the coupling's record (mpcekf_thermal_couple_get):
        ``fields`` names of COUPLE_FIELDS, None: all."""
        names = self.COUPLE_FIELDS if fields is None else (fields,) if isinstance(fields, str) else tuple(fields)
        for k in names:
            if k not in self.COUPLE_FIELDS:
                raise KeyError(f"thermal_couple_get: unknown field {k!r} (one of {self.COUPLE_FIELDS})")
        ids = np.array([self.COUPLE_FIELDS.index(k) for k in names], dtype=np.int32)
        vals = np.empty((ids.size, self.n))
        check(self.L.mpcekf_thermal_couple_get(self.h, int(ids.size), iptr(ids), dptr(vals)))
        return {k: vals[i] for i, k in enumerate(names)}

    def thermal_couple_end(self):
        """Drop the links and their record (mpcekf_thermal_couple_end): the model is per cell
        again.  thermal_end and pack_end do the same implicitly."""
        check(self.L.mpcekf_thermal_couple_end(self.h))

    # -- series strings: one current per pack string ------------------------
    PACK_FIELDS = _lib.PACK_FIELDS

    def pack_begin(self, series):
        """Make the context a pack of ncells // series strings of ``series`` cells in series
        (mpcekf_pack_begin): string g is the cells [g * series, (g + 1) * series).  From then on
        every fused step applies to each cell of a string the string's current, the largest
        (least charging) command among its cells; a second call replaces the first and resets
        the record.  series = 1 couples nothing."""
        series = int(series)
        check(self.L.mpcekf_pack_begin(self.h, series))
        self._pack_series = series

    def pack_get(self, fields=None):
        """{name: [ncells] float64} of the pack record (mpcekf_pack_get): ``fields`` names of
        PACK_FIELDS (default all): nlim, the steps the cell was its string's limiter; steps, the
        steps it had a command; headroom, the sum of applied current minus own command (A steps)."""
        names = self.PACK_FIELDS if fields is None else (fields,) if isinstance(fields, str) else tuple(fields)
        for k in names:
            if k not in self.PACK_FIELDS:
                raise KeyError(f"pack_get: unknown field {k!r} (one of {self.PACK_FIELDS})")
        ids = np.asarray([self.PACK_FIELDS.index(k) for k in names], dtype=np.int32)
        vals = np.empty((ids.size, self.n))
        check(self.L.mpcekf_pack_get(self.h, int(ids.size), iptr(ids), dptr(vals)))
        return {k: vals[i] for i, k in enumerate(names)}

    def pack_end(self):
        """Drop the pack (mpcekf_pack_end): every cell is on its own again."""
        check(self.L.mpcekf_pack_end(self.h))
        self._pack_series = 0

    # -- passive balancing: bleed currents around the cells that are ahead ---
    BALANCE_PARAMS = _lib.BALANCE_PARAMS
    BALANCE_FIELDS = _lib.BALANCE_FIELDS

    @classmethod
    def _balance_args(cls, n, i_bleed, dz_on, dz_off=None, compensate=True):
        """balance_begin's arguments -> (float64 [3, n] parameters, int compensate).  ValueError
        for a bad shape, a negative or NaN i_bleed, dz_on <= 0 or NaN, dz_off outside [0, dz_on]
        or a compensate that is no 0 / 1: before any library call."""
        ib = cls._per_cell(n, "i_bleed", i_bleed, who="balance_begin")
        on = cls._per_cell(n, "dz_on", dz_on, who="balance_begin")
        off = on / 2 if dz_off is None else cls._per_cell(n, "dz_off", dz_off, who="balance_begin")
        if not np.all(ib >= 0):
            raise ValueError("balance_begin: i_bleed: a current >= 0 (0: no bleeder), not NaN")
        if not np.all(on > 0):
            raise ValueError("balance_begin: dz_on: a SOC fraction > 0, not NaN")
        if not np.all((off >= 0) & (off <= on)):
            raise ValueError("balance_begin: dz_off: a SOC fraction in [0, dz_on]")
        if not isinstance(compensate, (bool, np.bool_)) and not (isinstance(compensate, (int, np.integer))
                                                                  and compensate in (0, 1)):
            raise ValueError(f"balance_begin: compensate = {compensate!r}: True / False (1 / 0)")
        return np.ascontiguousarray(np.stack([ib, on, off]), dtype=np.float64), int(compensate)

    def balance_begin(self, i_bleed, dz_on, dz_off=None, compensate=True):
        """Give the pack context a passive balancer (mpcekf_balance_begin), each parameter a scalar
        or [ncells]: ``i_bleed`` (A, >= 0; 0: the cell has no bleeder); a cell's bleeder switches
        on once its soc is ``dz_on`` (a fraction, > 0) above the smallest of its string and off at
        ``dz_off`` (default dz_on / 2) or below; ``compensate``: the charger adds a bleeding
        cell's bleed current to what the cell accepts.  From then on every fused step applies to a
        bleeding cell its string's current less its bleed current.  A second call resets."""
        # ValueError before any library call
        par, comp = self._balance_args(self.n, i_bleed, dz_on, dz_off, compensate)
        check(self.L.mpcekf_balance_begin(self.h, dptr(par), comp))

    def balance_get(self, fields=None):
        """{name: [ncells] float64} of the balance record (mpcekf_balance_get): ``fields`` names of
        BALANCE_FIELDS (default all): steps_on, the steps the cell was bleeding; q_bleed, the sum of
        its bleed current over them (A steps); switches, the times its bleeder went on; dz_max and
        dz_last, the largest and the latest distance to its string's smallest soc; steps, the
        steps it was valid."""
        names = self.BALANCE_FIELDS if fields is None else (fields,) if isinstance(fields, str) else tuple(fields)
        for k in names:
            if k not in self.BALANCE_FIELDS:
                raise KeyError(f"balance_get: unknown field {k!r} (one of {self.BALANCE_FIELDS})")
        ids = np.asarray([self.BALANCE_FIELDS.index(k) for k in names], dtype=np.int32)
        vals = np.empty((ids.size, self.n))
        check(self.L.mpcekf_balance_get(self.h, int(ids.size), iptr(ids), dptr(vals)))
        return {k: vals[i] for i, k in enumerate(names)}

    def balance_end(self):
        """Drop the balancer (mpcekf_balance_end): the pack couples its strings as before."""
        check(self.L.mpcekf_balance_end(self.h))

    # -- charger limits: string voltage, current and power caps ---------------
    CHARGER_PARAMS = _lib.CHARGER_PARAMS
    CHARGER_FIELDS = _lib.CHARGER_FIELDS

    @staticmethod
    def _charger_args(nstr, i_max=None, p_max=None):
        """charger_begin's arguments -> float64 [2, nstrings] parameters (None: NaN, the cap is
        off).  ValueError for a bad shape, a negative i_max or p_max <= 0: before any library
        call."""
        rows = []
        for name, a in (("i_max", i_max), ("p_max", p_max)):
            a = np.nan if a is None else a
            a = np.asarray(a, dtype=np.float64)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != nstr):
                raise ValueError(f"charger_begin: {name}: a scalar or [nstrings = {nstr}], not {a.shape}")
            rows.append(np.broadcast_to(a, (nstr,)))
        im, pm = rows
        if not np.all(np.isnan(im) | (im >= 0)):
            raise ValueError("charger_begin: i_max: a current >= 0 (A), or NaN / None for no current cap")
        if not np.all(np.isnan(pm) | (pm > 0)):
            raise ValueError("charger_begin: p_max: a power > 0 (W), or NaN / None for no power cap")
        return np.ascontiguousarray(np.stack([im, pm]), dtype=np.float64)

    def charger_begin(self, i_max=None, p_max=None):
        """Give the pack context a charger (mpcekf_charger_begin), each parameter a scalar or
        [nstrings]: ``i_max`` (A, >= 0) and ``p_max`` (W, > 0) bound every string's charging
        current and power; None or NaN: that cap is off, np.inf never binds.  From then on every
        fused step adds up each string's voltage and raises the string's (negative) current to
        -i_max and -p_max / V where those are larger.  A second call resets the record."""
        series = getattr(self, "_pack_series", 0)
        par = self._charger_args(self.n // series if series else self.n, i_max, p_max)   # ValueError before any library call
        check(self.L.mpcekf_charger_begin(self.h, dptr(par)))

    def charger_get(self, fields=None):
        """{name: [nstrings] float64} of the charger record (mpcekf_charger_get): ``fields`` names
        of CHARGER_FIELDS (default all): steps, the steps with a string current; ncap_i / ncap_p,
        the steps the current / power cap set it; q, the sum of the string current (A steps); e, the
        sum of voltage times current (W steps); curtail, the sum of capped minus uncapped current;
        p_min, the smallest (most charging) power; v_peak, the largest string voltage; nvalid_min,
        the smallest number of cells that contributed to a string voltage."""
        names = self.CHARGER_FIELDS if fields is None else (fields,) if isinstance(fields, str) else tuple(fields)
        for k in names:
            if k not in self.CHARGER_FIELDS:
                raise KeyError(f"charger_get: unknown field {k!r} (one of {self.CHARGER_FIELDS})")
        ids = np.asarray([self.CHARGER_FIELDS.index(k) for k in names], dtype=np.int32)
        series = getattr(self, "_pack_series", 0)
        vals = np.empty((ids.size, self.n // series if series else self.n))
        check(self.L.mpcekf_charger_get(self.h, int(ids.size), iptr(ids), dptr(vals)))
        return {k: vals[i] for i, k in enumerate(names)}

    def charger_end(self):
        """Drop the charger (mpcekf_charger_end): the pack's strings are bounded by their cells
        alone, as before."""
        check(self.L.mpcekf_charger_end(self.h))

    # -- charge termination: latch, rest, stop when done --------------------
    TERM_PARAMS = _lib.TERM_PARAMS
    TERM_FIELDS = _lib.TERM_FIELDS

    @classmethod
    def _term_args(cls, n, soc_stop, i_taper, hold, T_cut):
        """term_begin's arguments -> (float64 [3, n] thresholds with NaN for None, int hold).
        ValueError for a bad shape or a hold that is no count >= 1: before any library call."""
        par = np.full((len(cls.TERM_PARAMS), n), np.nan)
        for i, (name, v) in enumerate(zip(cls.TERM_PARAMS, (soc_stop, i_taper, T_cut))):
            if v is not None:
                par[i] = cls._per_cell(n, name, v, who="term_begin")
        if isinstance(hold, bool) or int(hold) != hold or int(hold) < 1:
            raise ValueError(f"term_begin: hold = {hold!r}: a step count >= 1")
        return par, int(hold)

    def term_begin(self, soc_stop=None, i_taper=None, hold=1, T_cut=None):
        """Give the context a termination rule (mpcekf_term_begin), each threshold a scalar or
        [ncells], None (or NaN) for a criterion that is off: ``soc_stop`` a SOC in the unit of
        step()'s ``soc`` (a fraction 0..1); ``i_taper`` (A) with ``hold``: the current has been at
        or under i_taper for ``hold`` steps in a row after having been above it; ``T_cut`` (degC).
        From then on every fused step latches the cells that meet a criterion and rests them at
        0 A; on a pack a string follows its first latched cell.  A second call resets."""
        par, hold = self._term_args(self.n, soc_stop, i_taper, hold, T_cut)   # ValueError before any library call
        check(self.L.mpcekf_term_begin(self.h, dptr(par), hold))

    def term_get(self, fields=None):
        """{name: [ncells] float64} of the termination record (mpcekf_term_get): ``fields`` names
        of TERM_FIELDS (default all): state (0 open, 1 latched, 2 dead), done_step, reason (bits:
        1 soc_stop, 2 taper, 4 T_cut, 8 string), soc_done, u_done, T_done, rest, steps."""
        names = self.TERM_FIELDS if fields is None else (fields,) if isinstance(fields, str) else tuple(fields)
        for k in names:
            if k not in self.TERM_FIELDS:
                raise KeyError(f"term_get: unknown field {k!r} (one of {self.TERM_FIELDS})")
        ids = np.asarray([self.TERM_FIELDS.index(k) for k in names], dtype=np.int32)
        vals = np.empty((ids.size, self.n))
        check(self.L.mpcekf_term_get(self.h, int(ids.size), iptr(ids), dptr(vals)))
        return {k: vals[i] for i, k in enumerate(names)}

    def term_open(self):
        """The number of cells still open (mpcekf_term_open): one 4-byte copy."""
        v = C.c_int64()
        check(self.L.mpcekf_term_open(self.h, C.byref(v)))
        return v.value

    def term_end(self):
        """Drop the termination rule (mpcekf_term_end): every cell steps on as it stands."""
        check(self.L.mpcekf_term_end(self.h))

    def step_until(self, max_steps, chunk=64, tc=None):
        """Fused steps in calls of ``chunk`` until no cell is open or ``max_steps`` are run
        (mpcekf_step_until); no trajectory is returned; with a summary begun the record folds as in
        step_summary.  ``tc``: None, or the temperature (degC, a scalar or [ncells]) of every
        step.  Returns (steps_run, open)."""
        if isinstance(max_steps, bool) or int(max_steps) != max_steps or int(max_steps) < 0:
            raise ValueError(f"step_until: max_steps = {max_steps!r}: a step count >= 0")
        if isinstance(chunk, bool) or int(chunk) != chunk or int(chunk) < 1:
            raise ValueError(f"step_until: chunk = {chunk!r}: a step count >= 1")
        t = None if tc is None else np.ascontiguousarray(self._per_cell(self.n, "tc", tc, who="step_until"))
        run, left = C.c_int32(), C.c_int64()
        check(self.L.mpcekf_step_until(self.h, int(max_steps), int(chunk), dptr(t), C.byref(run), C.byref(left)))
        self._stepped(run.value)
        return run.value, left.value

    # -- side-reaction losses per cell (plating, SEI) -----------------------
    AGING_PARAMS = _lib.AGING_PARAMS
    AGING_FIELDS = _lib.AGING_FIELDS
    AGING_SOURCES = _lib.AGING_SOURCES

    @classmethod
    def _aging_args(cls, n, reactions, sources):
        """aging_begin's arguments -> (float64 params [nreact][5][n], the sources' bit mask);
        every check mpcekf_aging_begin makes, before the library is called."""
        if isinstance(reactions, dict):
            reactions = (reactions,)
        reactions = tuple(reactions)
        if not 1 <= len(reactions) <= 4:
            raise ValueError(f"aging_begin: {len(reactions)} reactions: 1 to 4")
        src = (sources,) if isinstance(sources, str) else tuple(sources)
        mask = 0
        for k in src:
            if k not in cls.AGING_SOURCES:
                raise ValueError(f"aging_begin: unknown source {k!r} (of {tuple(cls.AGING_SOURCES)})")
            mask |= cls.AGING_SOURCES[k]
        if not mask:
            raise ValueError(f"aging_begin: no source given (of {tuple(cls.AGING_SOURCES)})")
        par = np.empty((len(reactions), len(cls.AGING_PARAMS), n))
        for r, d in enumerate(reactions):
            d = dict(d)
            d.setdefault("gate", np.inf)
            for k in d:
                if k not in cls.AGING_PARAMS:
                    raise ValueError(f"aging_begin: reaction {r}: unknown parameter {k!r} (of {cls.AGING_PARAMS})")
            for i, k in enumerate(cls.AGING_PARAMS):
                if k not in d:
                    raise ValueError(f"aging_begin: reaction {r}: {k} is missing")
                par[r, i] = cls._per_cell(n, k, d[k], who=f"aging_begin: reaction {r}")
            i0, U, al, Ea, gate = par[r]
            if not (np.isfinite(i0) & (i0 >= 0)).all():
                raise ValueError(f"aging_begin: reaction {r}: i0 must be finite and >= 0")
            if not (np.isfinite(U).all() and np.isfinite(Ea).all()):
                raise ValueError(f"aging_begin: reaction {r}: U and Ea must be finite")
            if not (np.isfinite(al) & (al > 0)).all():
                raise ValueError(f"aging_begin: reaction {r}: alpha must be finite and > 0")
            if np.isnan(gate).any():
                raise ValueError(f"aging_begin: reaction {r}: gate is NaN (inf: always on)")
        return np.ascontiguousarray(par), mask

    def aging_begin(self, reactions, sources=("est",)):
        """Give the context side reactions (mpcekf_aging_begin): ``reactions`` is one dict or up
        to four, each of i0 (A), U (V), alpha, Ea (J/mol) and gate (V, default inf: always on),
        each a scalar or [ncells].  After every fused step each reaction's Tafel current
        j = i0 exp(Ea/R (1/Tref - 1/T)) exp(-alpha F (phi - U) / (R T)) is added to the cell's
        record where phi - U < gate, with phi the EKF's phise ("est"), the plant's negPhise0
        ("plant"), or both (``sources``).  A second call replaces the first and resets the record."""
        par, mask = self._aging_args(self.n, reactions, sources)
        check(self.L.mpcekf_aging_begin(self.h, int(par.shape[0]), mask, dptr(par)))
        self._aging = (int(par.shape[0]), mask)

    def aging_get(self, source, react, fields=None):
        """{name: [ncells] float64} of the aging record (mpcekf_aging_get) of ``source`` ("est" or
        "plant") and reaction ``react``: ``fields`` names of AGING_FIELDS (default all).  Charge in
        Ah = q_sum * Ts / 3600; steps and nskip are per source."""
        if source not in self.AGING_SOURCES:
            raise KeyError(f"aging_get: unknown source {source!r} (of {tuple(self.AGING_SOURCES)})")
        names = self.AGING_FIELDS if fields is None else (fields,) if isinstance(fields, str) else tuple(fields)
        for k in names:
            if k not in self.AGING_FIELDS:
                raise KeyError(f"aging_get: unknown field {k!r} (one of {self.AGING_FIELDS})")
        ids = np.asarray([self.AGING_FIELDS.index(k) for k in names], dtype=np.int32)
        vals = np.empty((ids.size, self.n))
        check(self.L.mpcekf_aging_get(self.h, self.AGING_SOURCES[source], int(react), int(ids.size), iptr(ids), dptr(vals)))
        return {k: vals[i] for i, k in enumerate(names)}

    def aging_record(self):
        """{source: [one aging_get dict per reaction]} for every enabled source."""
        nreact, mask = getattr(self, "_aging", (0, 0))
        return {k: [self.aging_get(k, r) for r in range(nreact)] for k, b in self.AGING_SOURCES.items() if mask & b}

    def aging_end(self):
        """Drop the side reactions and their record (mpcekf_aging_end)."""
        check(self.L.mpcekf_aging_end(self.h))
        self._aging = (0, 0)

    def set_timing(self, enable=True):
        """enable: True/1 = every step; N > 1 = sample every N-th step (less perturbation)."""
        check(self.L.mpcekf_set_timing(self.h, int(enable)))

    def get_timing(self):
        """{kernel: (ms_sum, launches)} since the last call (HIP events on the ctx stream)."""
        names = ("plant", "flush", "cell", "hild", "bounds")  # MPCEKF_K_* order
        ms = np.zeros(len(names))
        nl = (C.c_int64 * len(names))()
        check(self.L.mpcekf_get_timing(self.h, dptr(ms), nl))
        return {k: (float(ms[i]), int(nl[i])) for i, k in enumerate(names)}

    def get_stamps(self):
        """k_cell section stamps of the last fused step [NSTAMPS][ncells] (profiling builds; else None)."""
        ns = C.c_int32(0)
        check(self.L.mpcekf_get_stamps(self.h, None, C.byref(ns)))
        if ns.value == 0:
            return None
        out = np.empty((ns.value, self.n), dtype=np.int64)
        check(self.L.mpcekf_get_stamps(self.h, out.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(ns)))
        return out

    def get_hild_problems(self):
        """(prob [51][ncells] field-major, hflag [ncells]) of the last fused step (diagnostic)."""
        prob = np.empty((51, self.n))
        hflag = np.empty(self.n, dtype=np.int32)
        check(self.L.mpcekf_get_hild_problems(self.h, dptr(prob), iptr(hflag)))
        return prob, hflag

    def get_zk(self):
        zk = np.empty((self.n, self.nz + 2))
        zb = np.empty((self.n, self.nz + 2))
        check(self.L.mpcekf_get_zk(self.h, dptr(zk), dptr(zb)))
        return zk, zb

    # -- MATLAB-named stage functions --------------------------------------
    def _tvec(self, T):
        return None if T is None else self._vec(T)

    def obs_layout(self):
        """{field: slice} of the observable record as the library lays it out
        (mpcekf_obs_layout); equals ROM.obs_layout()."""
        off = np.zeros(_lib.OBS_COUNT + 1, dtype=np.int32)
        check(self.L.mpcekf_obs_layout(self.h, iptr(off)))
        return {k: slice(int(off[f]), int(off[f + 1])) for f, k in enumerate(OBS_FIELDS)}

    _OBS_SCALARS = frozenset(("negSOC", "posSOC", "cellSOC", "negIfdl0", "posIfdl3", "negIf0", "posIf3",
                              "negThetass0", "posThetass3", "negPhise0", "Vcell"))

    def _obs_dict(self, rec, fields, slices):
        # views of the slot-major record: scalar fields [n], vector fields [n, len]
        return {k: rec[sl.start] if k in self._OBS_SCALARS else rec[sl].T for k, sl in zip(fields, slices)}

    def OB_step(self, Iapp, Tc=None, obs=False):
        """[Vcell, obs, cellState] = OB_step(Iapp, Tc, cellState, ROM)  (OB_step.m:1).
        Tc (degC, scalar or [n]) becomes the cell temperature; None keeps the current one.

        obs=False: Vcell [n].  obs=True: (Vcell, dict) with every field of the reference's obs
        struct (OB_step.m:226-228, 289-356; rom.OBS_FIELDS): scalar fields [n], vector fields
        [n, len] (len may be 0).  obs=("negPhise0", "Thetae"): only those fields cross PCIe
        (the record stays on the device, mpcekf_plant_obs_slots).  Vcell and the plant state
        are the same bits whichever way it is called."""
        i = self._vec(Iapp)
        t = self._tvec(Tc)
        v = np.empty(self.n)
        if obs is False or obs is None:
            self._stage("plant_step", dptr(i), dptr(t), dptr(v), keep=(v,))
            return v
        lay = self.rom.obs_layout()
        if obs is True:
            rec = np.empty((lay["Vcell"].stop, self.n))
            # the inputs stay alive until the synchronisation too (an input the library
            # cannot bounce is read in place)
            self._stage("plant_step_obs", dptr(i), dptr(t), dptr(v), dptr(rec), keep=(v, rec, i, t))
            return v, self._obs_dict(rec, OBS_FIELDS, [lay[k] for k in OBS_FIELDS])
        fields = (obs,) if isinstance(obs, str) else tuple(obs)
        for k in fields:
            if k not in lay:
                raise KeyError(f"OB_step: unknown obs field {k!r} (one of {OBS_FIELDS})")
        slots = np.ascontiguousarray(np.concatenate([np.arange(lay[k].start, lay[k].stop) for k in fields] or [[]]),
                                     dtype=np.int32)
        rec = np.empty((slots.size, self.n))
        self._stage("plant_step_obs", dptr(i), dptr(t), dptr(v), None, keep=(v, i, t))
        if slots.size:
            self._stage("plant_obs_slots", iptr(slots), int(slots.size), dptr(rec), keep=(rec, slots))
        pos, sl = 0, []
        for k in fields:
            m = lay[k].stop - lay[k].start
            sl.append(slice(pos, pos + m))
            pos += m
        return v, self._obs_dict(rec, fields, sl)

    def plant_obs_slots(self, slots):
        """Slots of the device-resident record of the last OB_step(obs=...) call, [len(slots), n]
        (mpcekf_plant_obs_slots); MpcekfError when there is no record since init_cells, the
        last fused step or set_state."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        out = np.empty((sl.size, self.n))
        self._stage("plant_obs_slots", iptr(sl), int(sl.size), dptr(out), keep=(out, sl))
        return out

    def iterEKF(self, vk, ik, Tk=None, bounds=True, xind=True):
        """[zk, boundzk, ekfData, Xind] = iterEKF(vk, ik, Tk, ekfData)  (iterEKF.m:30).

        Xind is returned as dict(model=[n,4] model index t*nZ+z, theT, theZ, gamma);
        xind=False: None (it stays on the device for EKFmatsHandler(None, None)).  vk = None:
        the last OB_step's Vcell on the device (the asynchronous route's hand-off)."""
        v = None if vk is None else self._vec(vk)
        i = self._vec(ik)
        t = self._tvec(Tk)
        zk = np.empty((self.n, self.nz + 2))
        zb = np.empty((self.n, self.nz + 2)) if bounds else None
        xm = np.empty((self.n, 4), dtype=np.int32) if xind else None
        xg = np.empty((self.n, 4)) if xind else None
        self._stage("ekf_step", dptr(v), dptr(i), dptr(t), dptr(zk), dptr(zb), iptr(xm), dptr(xg), keep=(zk, zb, xm, xg))
        if not xind:
            return zk, zb, None
        return zk, zb, _Xind(model=xm, gamma=xg, nZ=self.rom.nZ)

    def EKFmatsHandler(self, zk, Xind, Tk=None, keep=False):
        """[MPC, xhat] = EKFmatsHandler(ekfData, Xind, zk, Tk)  (EKFmatsHandler.m:1).

        Returns the packed linearisation records [n, 35] (fields: LIN_FIELDS).  zk = Xind =
        None: the device copies of the last iterEKF; keep=True: the records stay on the
        device only (None is returned; lin_fields reads slots, iterMPC / mpc_diag take
        lin=None) -- the stage route without host round trips."""
        t = self._tvec(Tk)
        lin = None if keep else np.empty((self.n, LIN_SIZE))
        if zk is None:
            self._stage("linearize", None, None, None, dptr(t), dptr(lin), keep=(lin,))
            return lin
        zk = np.ascontiguousarray(zk, dtype=np.float64)
        xm = np.ascontiguousarray(Xind["model"], dtype=np.int32)
        xg = np.ascontiguousarray(Xind["gamma"], dtype=np.float64)
        self._stage("linearize", dptr(zk), iptr(xm), dptr(xg), dptr(t), dptr(lin), keep=(lin,))
        return lin

    def lin_fields(self, slots, set=None, out=None):
        """Slots (MPCEKF_LIN_*) of the device-resident records of the last EKFmatsHandler:
        [n, len(slots)]; ``set`` [n, len(slots)] is written into them first.  ``out``: a
        C-contiguous float64 [n, len(slots)] array to fill instead of a new one."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        if out is None:
            out = np.empty((self.n, sl.size))
        elif out.shape != (self.n, sl.size) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError(f"lin_fields: out must be a C-contiguous float64 array of shape {(self.n, sl.size)}")
        st = None
        if set is not None:
            st = np.ascontiguousarray(set, dtype=np.float64)
            if st.size != self.n * sl.size:   # the C side reads n * len(slots) doubles from it
                raise ValueError(f"lin_fields: set must hold {(self.n, sl.size)} values, got shape {st.shape}")
            st = st.reshape(self.n, sl.size)
        self._stage("lin_fields", iptr(sl), int(sl.size), dptr(st), dptr(out), keep=(out,))
        return out

    def iterMPC(self, lin, SOCk_1, cost=False):
        """[uk, mpcData] = iterMPC(xk, cellState, mpcData)  (iterMPC.m:1). Returns uk, nexec;
        with cost=True also this call's mpcData.cost row (iterMPC.m:89-95) as a dict of
        J_uncon, J_final, norm_DU, viol, nexec per cell."""
        lin = None if lin is None else np.ascontiguousarray(lin, dtype=np.float64)   # None: the device record
        s = None if SOCk_1 is None else self._vec(SOCk_1)   # None: zk(end) of the last iterEKF, on the device
        uk = np.empty(self.n)
        ne = np.empty(self.n, dtype=np.int32)
        if not cost:
            self._stage("mpc_step", dptr(lin), dptr(s), dptr(uk), iptr(ne), keep=(uk, ne))
            return uk, ne
        ju, jf, nd = np.empty(self.n), np.empty(self.n), np.empty(self.n)
        nv = np.empty(self.n, dtype=np.int32)
        self._stage("mpc_step_ex", dptr(lin), dptr(s), dptr(uk), iptr(ne), dptr(ju), dptr(jf), dptr(nd), iptr(nv),
                    keep=(uk, ne, ju, jf, nd, nv))
        return uk, ne, dict(J_uncon=ju, J_final=jf, norm_DU=nd, viol=nv, nexec=ne)

    def mpc_diag(self, lin, uk_1=None):
        """mpcData.poles / mpcData.sv of the iterMPC that iterMPC(lin, ..) would run
        (iterMPC.m:53-60): (poles complex [n, 7], sv [n, 7]).  uk_1 None: the context's."""
        lin = None if lin is None else np.ascontiguousarray(lin, dtype=np.float64)   # None: the device record
        u = None if uk_1 is None else self._vec(uk_1)
        p = np.empty((self.n, 7, 2))
        sv = np.empty((self.n, 7))
        self._stage("mpc_diag", dptr(lin), dptr(u), dptr(p), dptr(sv), keep=(p, sv))
        return _complex(p), sv   # a view of p: asynchronously, its values arrive at the sync

    # -- state -----------------------------------------------------------
    def get_state(self):
        n, NM = self.n, self.NM
        st = dict(bigX=np.empty((n, NM, 6)), ekf=np.empty((n, NM, 20)), scal=np.empty((n, _lib.NSCAL)),
                  lam=np.empty((n, self.ncon)), warn=np.empty(n, np.int32), status=np.empty(n, np.int32))
        if self.cfg.method == _lib.METHOD_MB:
            st["mb"] = np.empty((n, _lib.MB_SIZE))
        s = _lib.State(dptr(st["bigX"]), dptr(st["ekf"]), dptr(st["scal"]), dptr(st["lam"]),
                       iptr(st["warn"]), iptr(st["status"]), dptr(st.get("mb")))
        check(self.L.mpcekf_get_state(self.h, C.byref(s)))
        return st

    SCALARS = ("SOCnAvg", "SOCpAvg", "x0", "SigmaX0", "priorI", "uk_1", "uk", "vk")  # MPCEKF_S_* order

    def get_scalars(self, names=("SOCnAvg", "SOCpAvg"), flags=False):
        """The named per-cell scalars ({name: [ncells]}; names from SCALARS) and, with
        flags=True, warn / status -- only these bytes cross PCIe (mpcekf_get_scalars)."""
        slots = np.array([self.SCALARS.index(k) for k in names], dtype=np.int32)
        sc = np.empty((self.n, len(slots)))
        warn = np.empty(self.n, np.int32) if flags else None
        status = np.empty(self.n, np.int32) if flags else None
        self._stage("get_scalars", iptr(slots), len(slots), dptr(sc), iptr(warn), iptr(status), keep=(sc, warn, status))
        out = {k: sc[:, j] for j, k in enumerate(names)}
        if flags:
            out.update(warn=warn, status=status)
        return out

    def set_state(self, st):
        a = {k: (np.ascontiguousarray(v, dtype=np.int32 if k in ("warn", "status") else np.float64)
                 if v is not None else None) for k, v in st.items()}
        s = _lib.State(dptr(a.get("bigX")), dptr(a.get("ekf")), dptr(a.get("scal")), dptr(a.get("lam")),
                       iptr(a.get("warn")), iptr(a.get("status")), dptr(a.get("mb")))
        check(self.L.mpcekf_set_state(self.h, C.byref(s)))


def _complex(p):
    """[..., 2] re / im float64 pairs as a complex128 [...] view (no copy, the exact pairs:
    re + 1j * im would turn a -0 real part into +0 and an infinite imaginary part's real
    part into NaN)."""
    return p.view(np.complex128)[..., 0]


class _Xind(dict):
    """iterEKF's Xind: model / gamma, and theT / theZ (model // nZ, model % nZ) formed when
    first read -- after an asynchronous iterEKF, model holds its values only after the sync."""

    def __init__(self, model, gamma, nZ):
        super().__init__(model=model, gamma=gamma)
        self._nZ = nZ

    def __missing__(self, key):
        if key == "theT":
            v = self["model"] // self._nZ
        elif key == "theZ":
            v = self["model"] % self._nZ
        else:
            raise KeyError(key)
        self[key] = v
        return v


# ---------------------------------------------------------------------------
# context-free batched functions
# ---------------------------------------------------------------------------
def predMat(a, Cr, D, Np=5, Nc=2, device=0):
    """predMat.m with A = diag(a) (a [n,6]), B = ones, C [n,6], D [n] -> Phi [n,Np,7], G [n,Np,Nc]."""
    L = _lib.load()
    a = np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64)
    Cr = np.ascontiguousarray(np.atleast_2d(Cr), dtype=np.float64)
    D = np.ascontiguousarray(np.atleast_1d(D), dtype=np.float64)
    n = a.shape[0]
    Phi = np.empty((n, Np, 7))
    G = np.empty((n, Np, Nc))
    check(L.mpcekf_predmat(device, n, Np, Nc, dptr(a), dptr(Cr), dptr(D), dptr(Phi), dptr(G)))
    return Phi, G


def constraint_rows(cfg):
    """nC of constraintsMPC.m:15-101 for cfg's switches: [Cu; -Cu; I; -I] (4 Nc rows) if
    useCurrent, G_v (Np) if useVoltage, -G_e (Np) if useEta, then always G_soc (Np)."""
    return (4 * cfg.Nc if cfg.use_current else 0) + (cfg.Np if cfg.use_voltage else 0) + \
           (cfg.Np if cfg.use_eta else 0) + cfg.Np


def constraintsMPC(lin, uk_1, SOCk_1, Q, cfg=None, device=0):
    """constraintsMPC.m: lin [n,35] -> M [n,ncon,Nc], gamma [n,ncon]; ncon = constraint_rows(cfg),
    the enabled blocks only (cfg = make_config(constraints=(cur, v, eta)))."""
    L = _lib.load()
    cfg = cfg if cfg is not None else make_config()
    lin = np.ascontiguousarray(np.atleast_2d(lin), dtype=np.float64)
    n = lin.shape[0]
    u = np.ascontiguousarray(np.broadcast_to(uk_1, (n,)), dtype=np.float64)
    s = np.ascontiguousarray(np.broadcast_to(SOCk_1, (n,)), dtype=np.float64)
    ncon = constraint_rows(cfg)
    M = np.empty((n, ncon, cfg.Nc))
    g = np.empty((n, ncon))
    check(L.mpcekf_constraints(device, C.byref(cfg), float(Q), n, dptr(lin), dptr(u), dptr(s), dptr(M), dptr(g)))
    return M, g


def hildreth(E, F, M, gamma, lambda0=None, maxIter=100, tol=1e-6, device=0):
    """hildreth.m batched: E [n,Nc,Nc], F [n,Nc], M [n,ncon,Nc], gamma [n,ncon]."""
    L = _lib.load()
    E = np.ascontiguousarray(E, dtype=np.float64)
    n, Nc = E.shape[0], E.shape[1]
    F = np.ascontiguousarray(F, dtype=np.float64)
    M = np.ascontiguousarray(M, dtype=np.float64)
    g = np.ascontiguousarray(gamma, dtype=np.float64)
    ncon = M.shape[1]
    lam = np.zeros((n, ncon)) if lambda0 is None else np.array(lambda0, dtype=np.float64, order="C")
    DU = np.empty((n, Nc))
    ne = np.empty(n, dtype=np.int32)
    check(L.mpcekf_hildreth(device, n, Nc, ncon, dptr(E), dptr(F), dptr(M), dptr(g), dptr(lam),
                            int(maxIter), float(tol), dptr(DU), iptr(ne)))
    return DU, lam, ne


def hildreth_structured(E, F, Hv, He, Hs, gamma, lambda0=None, maxIter=100, tol=1e-6, device=0):
    """hildreth.m on constraintsMPC.m-structured problems (the fused step's solver):
    E [n,2,2], F [n,2], Hv/He/Hs [n,5] Toeplitz columns, gamma [n,23]."""
    L = _lib.load()
    E = np.ascontiguousarray(E, dtype=np.float64)
    n = E.shape[0]
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (F, Hv, He, Hs, gamma)]
    lam = np.zeros((n, 23)) if lambda0 is None else np.array(lambda0, dtype=np.float64, order="C")
    DU = np.empty((n, 2))
    ne = np.empty(n, dtype=np.int32)
    check(L.mpcekf_hildreth_structured(device, n, dptr(E), *[dptr(x) for x in a], dptr(lam), int(maxIter),
                                       float(tol), dptr(DU), iptr(ne)))
    return DU, lam, ne


def structured_M(Hv, He, Hs):
    """The constraintsMPC.m matrix [Cu; -Cu; I; -I; G_v; -G_e; G_soc] (23 x 2) of
    Toeplitz columns, with the kernels' exact entries (signed zeros included)."""
    M = np.zeros((23, 2))
    for i in range(2):
        for k in range(2):
            M[i, k] = 1.0 if k <= i else 0.0
            M[2 + i, k] = -(1.0 if k <= i else 0.0)
            M[4 + i, k] = 1.0 if i == k else 0.0
            M[6 + i, k] = -(1.0 if i == k else 0.0)
    for r in range(5):
        for k in range(2):
            M[8 + r, k] = Hv[r - k] if k <= r else 0.0
            M[13 + r, k] = -(He[r - k] if k <= r else 0.0)
            M[18 + r, k] = Hs[r - k] if k <= r else 0.0
    return M


def thermal_ocv(rom, n=101, T_degC=25.0):
    """The cell's open-circuit voltage on a uniform grid of n cell-SOC points 0..1 at T_degC, from
    the ROM's own electrode handles: Uocp_pos(soc_pos(z, T), T) - Uocp_neg(soc_neg(z, T), T).
    Host numpy only; the table Context.thermal_begin takes."""
    T = float(T_degC) + 273.15
    pos, neg = rom.fn("pos"), rom.fn("neg")   # scalar functions, as the reference's handles are called
    return np.array([float(pos.Uocp(pos.soc(z, T), T)) - float(neg.Uocp(neg.soc(z, T), T))
                     for z in np.linspace(0.0, 1.0, int(n)).tolist()], dtype=np.float64)


def mscc_map(soc_breaks, crates, nz):
    """A multi-stage constant-current staircase as a hold-interpolated table: (z_lo, z_hi, table
    [nz]) for Context.limit_map(z_lo, z_hi, interp_z="hold", Crate=table).  ``crates`` [m]: the
    C-rate of each stage; ``soc_breaks`` [m + 1] ascending SOC fractions: stage i holds on
    [soc_breaks[i], soc_breaks[i + 1]), the first stage also below soc_breaks[0] and the last at
    and above soc_breaks[-1].  The grid is uniform with ``nz`` nodes over soc_breaks[0] ..
    soc_breaks[-1], and node j carries the stage its SOC lies in, so a break that is not a node
    takes effect at the next node above it: choose nz so that (nz - 1) * (break - z_lo) /
    (z_hi - z_lo) is an integer for an exact staircase.  Host numpy only."""
    b = np.asarray(soc_breaks, dtype=np.float64)
    c = np.asarray(crates, dtype=np.float64)
    if b.ndim != 1 or c.ndim != 1 or b.size != c.size + 1 or c.size < 1:
        raise ValueError(f"mscc_map: {c.size} stages need {c.size + 1} soc_breaks, got {b.size}")
    if not np.all(np.diff(b) > 0):
        raise ValueError("mscc_map: soc_breaks must ascend")
    if int(nz) != nz or int(nz) < 2:
        raise ValueError(f"mscc_map: nz = {nz!r}: 2 nodes or more")
    z = b[0] + (b[-1] - b[0]) * (np.arange(int(nz)) / (int(nz) - 1))
    # a node within rounding of a break belongs to the stage the break opens
    stage = np.searchsorted(b[1:-1], z + 1e-12 * (b[-1] - b[0]), side="right")
    return float(b[0]), float(b[-1]), c[stage]


def _limit_map(ctx, limit_map):
    """runMPC's / run_summary's limit_map dict: Context.limit_map's arguments."""
    if limit_map:
        ctx.limit_map(**limit_map)


def _thermal_begin(ctx, thermal):
    """runMPC's / run_summary's thermal dict: thermal_begin's keywords, plus an optional
    "schedule": a dict of thermal_schedule's (T_lo, T_hi, sets and the tables), and an optional
    "couple": thermal_couple's R_link, which the caller sets once the pack stands."""
    kw = dict(thermal)
    sched = kw.pop("schedule", None)
    kw.pop("couple", None)
    ctx.thermal_begin(**kw)
    if sched:
        ctx.thermal_schedule(**sched)


def _couple_links(n, thermal, pack, who):
    """thermal["couple"] checked before a context exists: None when the dict has none."""
    if not thermal or thermal.get("couple") is None:
        return None
    if not pack:
        raise ValueError(f"{who}: thermal['couple'] links the cells of a pack string: pass pack=dict(series=S)")
    return Context._couple_links(n, thermal["couple"])


def _charger_args(n, pack, who):
    """pack["charger"] checked before a context exists: (the pack dict without it, charger_begin's
    parameters [2, nstrings] or None).  KeyError for an unknown key, ValueError for a bad value."""
    if not pack or "charger" not in pack:
        return pack, None
    pack = dict(pack)
    c = pack.pop("charger")
    if not c:
        return pack, None
    for k in c:
        if k not in ("i_max", "p_max"):
            raise KeyError(f"{who}: unknown pack['charger'] key {k!r} (one of ('i_max', 'p_max'))")
    series = int(pack.get("series", 0))
    if series < 1 or n % series:
        raise ValueError(f"{who}: pack['charger'] needs a series that divides ncells = {n}, not {pack.get('series')!r}")
    return pack, Context._charger_args(n // series, **c)


def _pack_args(n, pack, who):
    """runMPC's / run_summary's pack dict checked before a context exists: (pack_begin's keywords,
    balance_begin's (parameters [3, n], compensate) or None).  KeyError for an unknown balance
    key, ValueError for a bad value."""
    if not pack or "balance" not in pack:
        return pack, None
    pack = dict(pack)
    b = pack.pop("balance")
    if not b:
        return pack, None
    known = ("i_bleed", "dz_on", "dz_off", "compensate")
    for k in b:
        if k not in known:
            raise KeyError(f"{who}: unknown pack['balance'] key {k!r} (one of {known})")
    for k in ("i_bleed", "dz_on"):
        if k not in b:
            raise KeyError(f"{who}: pack['balance'] needs {k!r}")
    return pack, Context._balance_args(n, **b)


def _stop_args(n, stop, who, chunk=False):
    """runMPC's / run_summary's stop dict checked before a context exists: (term_begin's
    thresholds [3, n], hold, chunk), or None when there is no dict.  KeyError for an unknown key,
    ValueError for a bad shape, hold or chunk."""
    if stop is None:
        return None
    known = ("soc_stop", "i_taper", "hold", "T_cut") + (("chunk",) if chunk else ())
    for k in stop:
        if k not in known:
            raise KeyError(f"{who}: unknown stop key {k!r} (one of {known})")
    par, hold = Context._term_args(n, stop.get("soc_stop"), stop.get("i_taper"), stop.get("hold", 1), stop.get("T_cut"))
    c = stop.get("chunk", 64)
    if isinstance(c, bool) or int(c) != c or int(c) < 1:
        raise ValueError(f"{who}: stop['chunk'] = {c!r}: a step count >= 1")
    return par, hold, int(c)


def runMPC(rom, SOC0, TC, nsteps, cfg=None, device=0, ncells=None, tc_traj=None, obs=None, limits=None,
           thermal=None, pack=None, aging=None, stop=None, limit_map=None):
    """runMPC.m:72-112 for a batch of cells; returns trajectories [nsteps, ncells].
    limit_map: a dict of Context.limit_map's arguments (z_lo, z_hi, T_lo, T_hi, sets, interp_z, z0,
    the tables): limits that follow each cell's SOC estimate and temperature, set after the
    extensions below; adds out["limits"], the values in force at the last step, out["limit_map"],
    the map's record, and (not with aging or thermal["couple"], whose calls have no such row)
    out["lim"], the values every step read.
    tc_traj [nsteps, ncells] (degC): a temperature profile (TC is the initial one).
    obs: the plant's observables of every step as out["obs"] (Context.step's obs=).
    limits: per-cell targets and limits, a dict of Context.set_limits' keywords (a protocol
    sweep: runMPC.m:30-44 per cell), set after init_cells and before the first step.
    thermal: a dict of Context.thermal_begin's keywords (Cth, Rth, Tamb, ocv, T0): the cells
    heat themselves (TC is the initial temperature; no tc_traj); adds out["temp"], out["heat"]
    and out["thermal"], the model's record.  thermal["schedule"]: a dict of
    Context.thermal_schedule's arguments (T_lo, T_hi, sets, the tables): limits that follow the
    cells' temperature; adds out["limits"], the values in force at the last step.
    pack: dict(series=S): the cells form ncells // S series strings, each charged with the one
    current its weakest cell accepts (Context.pack_begin); out["u"] is the applied current, and
    out["ucmd"], out["limiter"] and out["pack"], the pack's record, are added.
    pack["balance"]: a dict of Context.balance_begin's keywords (i_bleed, dz_on, dz_off,
    compensate): a passive balancer; adds out["bleed"], out["zmin"] (not with aging or
    thermal["couple"], whose calls have no such rows) and out["balance"], the balancer's record.
    pack["charger"]: a dict of Context.charger_begin's keywords (i_max, p_max): a charger's current
    and power rating per string; adds out["vstr"], out["istr"], out["capby"] (not with aging or
    thermal["couple"] either) and out["charger"], the charger's record.
    aging: a dict of Context.aging_begin's keywords (reactions, sources): adds out["rate"], every
    step's side-reaction currents, and out["aging"], the record (Context.aging_record).
    thermal["couple"] with a pack: Context.thermal_couple's R_link, heat conduction between
    neighbouring cells of a string; adds out["cond"] and out["couple"], the coupling's record.
    stop: a dict of Context.term_begin's keywords (soc_stop, i_taper, hold, T_cut): the termination
    rule over the fixed nsteps; a done cell rests at 0 A; adds out["term"], the rule's record."""
    SOC0 = np.atleast_1d(np.asarray(SOC0, dtype=np.float64))
    n = ncells or SOC0.shape[0]
    links = _couple_links(n, thermal, pack, "runMPC")
    pack, chg = _charger_args(n, pack, "runMPC")
    pack, bal = _pack_args(n, pack, "runMPC")
    term = _stop_args(n, stop, "runMPC")
    with Context(rom, n, cfg, device) as ctx:
        ctx.init_cells(SOC0, TC)
        if limits:
            ctx.set_limits(**limits)
        if thermal:
            _thermal_begin(ctx, thermal)
        if pack:
            ctx.pack_begin(**pack)
        if bal:
            check(ctx.L.mpcekf_balance_begin(ctx.h, dptr(bal[0]), bal[1]))
        if chg is not None:
            check(ctx.L.mpcekf_charger_begin(ctx.h, dptr(chg)))
        if links is not None:
            ctx.thermal_couple(links)
        if aging:
            ctx.aging_begin(**aging)
        if term:
            check(ctx.L.mpcekf_term_begin(ctx.h, dptr(term[0]), term[1]))
        _limit_map(ctx, limit_map)
        lm_rows = bool(limit_map) and not aging and links is None
        th_rows = ("temp", "heat", "cond") if links is not None else ("temp", "heat")
        pk_rows = ("ucmd", "limiter", "bleed", "zmin") if bal and not aging and links is None else ("ucmd", "limiter")
        if chg is not None and not aging and links is None:
            pk_rows += ("vstr", "istr", "capby")
        out = ctx.step(nsteps, tc=tc_traj, obs=obs, thermal=th_rows if thermal else None,
                       pack=pk_rows if pack else None, aging=("rate",) if aging else None,
                       limit_map=("lim",) if lm_rows else None)
        if limit_map:
            out["limits"] = ctx.get_limits()
            out["limit_map"] = ctx.limit_map_get()
        if aging:
            out["aging"] = ctx.aging_record()
        if term:
            out["term"] = ctx.term_get()
        if pack:
            out["pack"] = ctx.pack_get()
        if bal:
            out["balance"] = ctx.balance_get()
        if chg is not None:
            out["charger"] = ctx.charger_get()
        if links is not None:
            out["couple"] = ctx.thermal_couple_get()
        if thermal:
            out["thermal"] = ctx.thermal_get()
            if thermal.get("schedule"):
                out["limits"] = ctx.get_limits()
        out["status"] = ctx.get_state()["status"]
        return out


def run_summary(rom, SOC0, TC, nsteps, cfg=None, device=0, ncells=None, tc_traj=None, limits=None, reach=None,
                obs=None, chunk=None, thermal=None, pack=None, aging=None, stop=None, limit_map=None):
    """runMPC.m:72-112 for a batch of cells, read out as the per-cell charge summary instead of
    trajectories: {field: [ncells]} of Context.get_summary plus "status".  limits: as runMPC's
    (a protocol sweep); reach, obs: Context.summary_begin's; tc_traj [nsteps, ncells] (degC): a
    temperature profile; chunk: steps per step_summary call (default all at once; with tc_traj
    a chunk bounds the host array each call converts).  Neither host nor device memory grows
    with nsteps.  thermal: as runMPC's, its "schedule" included (no tc_traj); adds "thermal", the
    model's record.  pack: as runMPC's; adds "pack", the pack's record, beside the summary (whose
    currents are the applied ones), with pack["balance"] "balance", the balancer's record, and with
    pack["charger"] "charger", the charger's record.
    aging: as runMPC's; adds "aging", the side reactions' record.
    thermal["couple"] with a pack: as runMPC's; adds "couple", the coupling's record.
    stop: a dict of Context.term_begin's keywords plus chunk (default 64): the loop runs through
    Context.step_until with nsteps as the cap and ends when every cell is done (no tc_traj: TC
    holds); adds "steps_run", the steps run, and "term", the rule's record.
    limit_map: as runMPC's; adds "limit_map", the map's record."""
    SOC0 = np.atleast_1d(np.asarray(SOC0, dtype=np.float64))
    n = ncells or SOC0.shape[0]
    nsteps = int(nsteps)
    chunk = nsteps if not chunk else int(chunk)
    if chunk < 0 or (chunk == 0 and nsteps):
        raise ValueError(f"run_summary: chunk = {chunk}")
    tcs = None if tc_traj is None else tc_grid(tc_traj, nsteps, n)
    links = _couple_links(n, thermal, pack, "run_summary")
    pack, chg = _charger_args(n, pack, "run_summary")
    pack, bal = _pack_args(n, pack, "run_summary")
    term = _stop_args(n, stop, "run_summary", chunk=True)
    if term and tc_traj is not None:
        raise ValueError("run_summary: stop runs step_until, which takes one temperature row: no tc_traj")
    with Context(rom, n, cfg, device) as ctx:
        ctx.init_cells(SOC0, TC)
        if limits:
            ctx.set_limits(**limits)
        if thermal:
            _thermal_begin(ctx, thermal)
        if pack:
            ctx.pack_begin(**pack)
        if bal:
            check(ctx.L.mpcekf_balance_begin(ctx.h, dptr(bal[0]), bal[1]))
        if chg is not None:
            check(ctx.L.mpcekf_charger_begin(ctx.h, dptr(chg)))
        if links is not None:
            ctx.thermal_couple(links)
        if aging:
            ctx.aging_begin(**aging)
        _limit_map(ctx, limit_map)
        ctx.summary_begin(reach=reach, obs=obs)
        if term:
            check(ctx.L.mpcekf_term_begin(ctx.h, dptr(term[0]), term[1]))
            steps_run, _ = ctx.step_until(nsteps, chunk=term[2])
        else:
            for k in range(0, nsteps, max(chunk, 1)):
                m = min(chunk, nsteps - k)
                ctx.step_summary(m, tc=None if tcs is None else tcs[k:k + m])
        out = ctx.get_summary()
        if limit_map:
            out["limit_map"] = ctx.limit_map_get()
        if term:
            out["steps_run"] = steps_run
            out["term"] = ctx.term_get()
        if aging:
            out["aging"] = ctx.aging_record()
        if pack:
            out["pack"] = ctx.pack_get()
        if bal:
            out["balance"] = ctx.balance_get()
        if chg is not None:
            out["charger"] = ctx.charger_get()
        if links is not None:
            out["couple"] = ctx.thermal_couple_get()
        if thermal:
            out["thermal"] = ctx.thermal_get()
        out["status"] = ctx.get_state()["status"]
        return out


def cl_eig(a):
    """eig / svd of one small square matrix as the fused step computes mpcData.poles and
    mpcData.sv (iterMPC.m:57-60; mpcekf_cl_eig): (poles complex [n] sorted by descending
    real then imaginary part, sv [n] descending).  Host code, no device needed."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    n = a.shape[0]
    if a.shape != (n, n):
        raise ValueError("square matrix expected")
    re, im, sv = np.empty(n), np.empty(n), np.empty(n)
    L = _lib.load()
    check(L.mpcekf_cl_eig(n, dptr(a), dptr(re), dptr(im), dptr(sv)))
    return re + 1j * im, sv
