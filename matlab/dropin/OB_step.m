function [Vcell, obs, cellState] = OB_step(Iapp, Tc, cellState, ROM, initCfg)
% Drop-in for OB_step.m:1 over the MI355X library: the first call (empty cellState)
% creates the context from ROM and the recorded initKF / initMPC settings and runs
% mpcekf_init_cells; every call then runs the plant step (mpcekf_plant_step) at Tc for
% all cells.  cellState carries the handle.  By default obs holds Vcell and the pre-step
% electrode averages of OB_step.m:226-228 (negSOC, posSOC, cellSOC), which is all runMPC.m
% reads; the other observables of OB_step.m:289-356 are then not computed.
% initCfg.obsFields (first call) asks for more, at 8 bytes per cell and slot over PCIe
% every step: 'all' fills every field of the reference's obs (mpcekf_plant_step_obs, each
% field len x ncells), a cellstr such as {'negPhise0', 'Thetae'} only those fields
% (mpcekf_plant_obs_slots) beside the default four.
  if nargin < 3 || isempty(cellState) || ~isfield(cellState, 'initialized') || ~cellState.initialized
    if nargin < 5 || ~isfield(initCfg, 'SOC0')
      error('First call requires initCfg.SOC0 (in %).');
    end
    S = mpcekf_session('get');
    if isempty(S.kf) || isempty(S.mpc), error('mpcekf drop-in: call initKF and initMPC first'); end
    n = numel(initCfg.SOC0);
    cfg = S.mpc.mpcekf_cfg;
    cfg.SigmaV = S.kf.SigmaV;  cfg.SigmaW = S.kf.SigmaW;  cfg.SigmaX0 = S.kf.SigmaX0;
    cfg.flags = 1;                                         % MPCEKF_CF_BOUNDS: boundzk too
    if strcmp(S.kf.method, 'MB'), cfg.method = 1; end
    % the electrode tables hold the ROM set-points and the distinct Tc (mpcekf_rom_struct
    % keeps only their span when they do not fit its 8 table temperatures, e.g. a per-cell
    % Tc of thousands of distinct values), built as mpcekf_export_rom builds them
    % (mpcekf_build_tables: node tables for lookup-table handles, ntheta by the error
    % budget) with the budget checked at the distinct Tc this run uses.  A ROM whose tables
    % miss the budget there is refused ('mpcekf:budget'), unless initCfg.tabBudget = 'warn':
    % then it runs with a warning and cellState.tab_error says how far its lookups are off.
    Tu = unique(Tc(:)');
    [R, terr, tok] = mpcekf_build_tables(ROM, [], Tu, struct('Teval', Tu + 273.15, 'strict', false));
    if ~tok
      msg = sprintf(['OB_step drop-in: the electrode tables miss the error budget at the run''s ' ...
                     'temperatures (neg Uocp %.3g V, k0 %.3g; pos Uocp %.3g V, k0 %.3g)'], ...
                    terr.neg.Uocp, terr.neg.k0_rel, terr.pos.Uocp, terr.pos.k0_rel);
      if isfield(initCfg, 'tabBudget') && strcmpi(initCfg.tabBudget, 'warn')
        warning('mpcekf:budget', '%s', msg);
      else
        error('mpcekf:budget', '%s (initCfg.tabBudget = ''warn'' runs it anyway)', msg);
      end
    end
    h = mpcekf_mex('create', R, cfg, S.device, n);
    mpcekf_session('set', 'h', h);
    mpcekf_mex('init', h, reshape(initCfg.SOC0, 1, n), Tc .* ones(1, n));
    % initMPC's vector-valued targetSOC / Crate / limits: one entry per cell (runMPC.m:30-44)
    if isfield(S.mpc, 'mpcekf_limits') && ~isempty(S.mpc.mpcekf_limits.idx)
      mpcekf_mex('setlimits', h, S.mpc.mpcekf_limits.idx, S.mpc.mpcekf_limits.values);
    end
    fn = ROM.cellData.function.neg;
    cellState = struct('initialized', true, 'h', h, 'n', n, 'Ts', ROM.xraData.Tsamp, ...
                       'theta0n', fn.theta0(), 'theta100n', fn.theta100(), 'tab_error', terr);
    cellState.obsFields = {};                                % default: today's four fields
    if isfield(initCfg, 'obsFields') && ~isempty(initCfg.obsFields)
      names = {'negSOC', 'posSOC', 'cellSOC', 'negIfdl', 'posIfdl', 'negIfdl0', 'posIfdl3', 'negIf', 'posIf', ...
               'negIf0', 'posIf3', 'negIdl', 'posIdl', 'negThetass', 'posThetass', 'negThetass0', 'posThetass3', ...
               'negPhise', 'posPhise', 'negPhise0', 'Phie', 'Thetae', 'negPhis', 'posPhis', 'Vcell'};
      if ischar(initCfg.obsFields)
        if ~strcmpi(initCfg.obsFields, 'all'), error('initCfg.obsFields: ''all'' or a cellstr of obs field names'); end
        cellState.obsFields = 'all';
      else
        off = mpcekf_mex('obslayout', h);
        [known, f] = ismember(initCfg.obsFields, names);
        if ~all(known), error('initCfg.obsFields: unknown obs field %s', initCfg.obsFields{find(~known, 1)}); end
        cellState.obsFields = reshape(initCfg.obsFields, 1, []);
        cellState.obsSlots = arrayfun(@(k) off(k) + 1 : off(k + 1), f, 'UniformOutput', false);
      end
    end
  end
  n = cellState.n;
  iapp = reshape(Iapp .* ones(1, n), 1, n);
  tc = reshape(Tc .* ones(1, n), 1, n);
  if ischar(cellState.obsFields)                               % 'all': the reference's whole obs
    [Vcell, obs] = mpcekf_mex('plantobs', cellState.h, iapp, tc);
    return;
  elseif ~isempty(cellState.obsFields)                         % the default four and the named fields
    s = mpcekf_mex('scalars', cellState.h, [1 2]);
    obs = struct('negSOC', s(1, :), 'posSOC', s(2, :));
    obs.cellSOC = (obs.negSOC - cellState.theta0n) / (cellState.theta100n - cellState.theta0n);
    Vcell = mpcekf_mex('plantobs', cellState.h, iapp, tc);     % nargout 1: the record stays on the device
    rows = mpcekf_mex('obsslots', cellState.h, [cellState.obsSlots{:}]);
    at = 0;
    for k = 1:numel(cellState.obsFields)
      m = numel(cellState.obsSlots{k});
      obs.(cellState.obsFields{k}) = rows(at + 1 : at + m, :);
      at = at + m;
    end
    obs.Vcell = Vcell;
    return;
  end
  s = mpcekf_mex('scalars', cellState.h, [1 2]);             % pre-update averages (OB_step.m:226-228),
  obs = struct('negSOC', s(1, :), 'posSOC', s(2, :));         % 16 B per cell over PCIe
  obs.cellSOC = (obs.negSOC - cellState.theta0n) / (cellState.theta100n - cellState.theta0n);
  Vcell = mpcekf_mex('plant', cellState.h, iapp, tc);
  obs.Vcell = Vcell;
end
