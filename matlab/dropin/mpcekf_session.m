function [S, out] = mpcekf_session(op, name, value)
% MPCEKF_SESSION  State the drop-in wrappers share within one MATLAB session: the
% library context handle (one context for the batch, like the reference's one
% persistent iterEKF state per session, iterEKF.m:31) and the initKF / initMPC settings
% the context is created from on the first OB_step call.
%   S = mpcekf_session('get');  mpcekf_session('set', name, value);  mpcekf_session('reset')
%   [S, out] = mpcekf_session('step', nsteps, obsFields)
%     nsteps fused closed-loop steps (runMPC.m:84-111) on the session's context: out.u, v,
%     soc, phise, nexec are ncells x nsteps.  The optional obsFields -- 'all' or a cellstr
%     such as {'negPhise0', 'Thetae'}, the names of initCfg.obsFields -- adds out.obs, the
%     plant's own observables at every step: each field len x ncells x nsteps (len = 1 for
%     the scalar fields).  out.phise is the EKF's estimate; out.obs.negPhise0 the plant's.
%   mpcekf_session('termbegin', params, hold)
%     charge termination on the session's context (mpcekf_term_begin): params ncells x 3, columns
%     soc_stop (a fraction 0..1), i_taper (A), T_cut (degC), NaN: that criterion off; hold (default
%     1): the steps the current stays at or under i_taper.  From then on 'step' and 'stepuntil'
%     latch the cells that meet a criterion and rest them at 0 A.
%   [S, out] = mpcekf_session('termget')     out: the record, a struct of ncells x 1 vectors (state,
%     done_step, reason, soc_done, u_done, T_done, rest, steps)
%   mpcekf_session('termend')
%   [S, out] = mpcekf_session('stepuntil', max_steps, chunk)
%     fused steps in calls of chunk (default 64) until no cell is open or max_steps are run
%     (mpcekf_step_until): out.steps_run, out.open.
%   mpcekf_session('chargerbegin', params)
%     a charger's ratings on the session's pack context (mpcekf_charger_begin): params nstrings x 2,
%     columns i_max (A) and p_max (W), NaN: that cap off.  Without params the session's optional
%     field `charger` (mpcekf_session('set', 'charger', params)) is used; a begin stores its params there.
%   [S, out] = mpcekf_session('chargerget')  out: the record, a struct of nstrings x 1 vectors (steps,
%     ncap_i, ncap_p, q, e, curtail, p_min, v_peak, nvalid_min)
%   mpcekf_session('chargerend')
%   [S, out] = mpcekf_session('stepexcharger', nsteps)
%     out.u .. out.limiter as 'stepexpack' gives them, out.bal (bleed, zmin; [] without a balancer)
%     and out.chg (vstr, istr, capby), nstrings x nsteps each.
%   mpcekf_session('limitmap', map)
%     MPC limits over each cell's SOC estimate and temperature on the session's context
%     (mpcekf_limit_map): map is a struct with idx, z_lo, z_hi, tables (nz x nt x numel(idx) x nsets)
%     and the optional T_lo, T_hi, interp (0 linear, 1 hold), sets, z0, as mpcekf_mex('limitmap') takes them.
%   [S, out] = mpcekf_session('limitmapget')  out: the record, a struct of ncells x 1 vectors (z_last,
%     neval, nclamp_z, nclamp_t)
%   mpcekf_session('limitmapend')
%   [S, out] = mpcekf_session('stepexmap', nsteps)
%     out.u .. out.nexec as 'step' gives them and out.lim, ncells x numel(idx) x nsteps: the mapped
%     fields' values the MPC stage of every step read.
  persistent P
  % zk_last / ekf_tick: the zk the last iterEKF returned and a counter of iterEKF calls, so
  % EKFmatsHandler knows when the library's device copies of zk and Xind are the caller's
  % xhat_dev: the xhat the device-resident linearisation records hold (EKFmatsHandler's, or
  % the xk an iterMPC call wrote over it)
  if isempty(P), P = struct('h', [], 'kf', [], 'mpc', [], 'device', 0, 'zk_last', [], 'ekf_tick', 0, ...
                            'xhat_dev', [], 'charger', []); end
  out = [];
  switch op
    case 'set'
      P.(name) = value;
    case 'reset'
      if ~isempty(P.h), mpcekf_mex('destroy', P.h); end
      P.h = [];
    case 'get'
    case 'step'
      if isempty(P.h), error('mpcekf_session: step before the first OB_step call created the context'); end
      nsteps = name;
      if nargin < 3 || isempty(value)
        [u, v, soc, phise, nexec] = mpcekf_mex('step', P.h, nsteps);
        out = struct('u', u, 'v', v, 'soc', soc, 'phise', phise, 'nexec', nexec);
      else
        names = {'negSOC', 'posSOC', 'cellSOC', 'negIfdl', 'posIfdl', 'negIfdl0', 'posIfdl3', 'negIf', 'posIf', ...
                 'negIf0', 'posIf3', 'negIdl', 'posIdl', 'negThetass', 'posThetass', 'negThetass0', 'posThetass3', ...
                 'negPhise', 'posPhise', 'negPhise0', 'Phie', 'Thetae', 'negPhis', 'posPhis', 'Vcell'};
        if ischar(value)
          if ~strcmpi(value, 'all'), error('obsFields: ''all'' or a cellstr of obs field names'); end
          value = names;
        end
        [known, f] = ismember(value, names);
        if ~all(known), error('obsFields: unknown obs field %s', value{find(~known, 1)}); end
        off = mpcekf_mex('obslayout', P.h);
        slots = arrayfun(@(k) off(k) + 1 : off(k + 1), f, 'UniformOutput', false);
        keep = ~cellfun(@isempty, slots);                        % a field without rows in tfData.names
        out = struct('obs', struct());
        if any(keep)
          [u, v, soc, phise, nexec, rows] = mpcekf_mex('stepobs', P.h, nsteps, [slots{:}]);
        else
          [u, v, soc, phise, nexec] = mpcekf_mex('step', P.h, nsteps);
          rows = zeros(size(u, 1), 0, nsteps);
        end
        out.u = u; out.v = v; out.soc = soc; out.phise = phise; out.nexec = nexec;
        at = 0;
        for k = 1:numel(value)                                   % rows: ncells x nslots x nsteps
          m = numel(slots{k});
          out.obs.(value{k}) = permute(rows(:, at + 1 : at + m, :), [2 1 3]);
          at = at + m;
        end
      end
    case {'termbegin', 'termget', 'termend', 'stepuntil'}
      if isempty(P.h), error('mpcekf_session: %s before the first OB_step call created the context', op); end
      switch op
        case 'termbegin'
          if nargin < 3 || isempty(value), value = 1; end
          mpcekf_mex('termbegin', P.h, name, value);
        case 'termget'
          out = mpcekf_mex('termget', P.h);
        case 'termend'
          mpcekf_mex('termend', P.h);
        case 'stepuntil'
          if nargin < 3 || isempty(value), value = 64; end
          [run, left] = mpcekf_mex('stepuntil', P.h, name, value);
          out = struct('steps_run', run, 'open', left);
      end
    case {'balancebegin', 'balanceget', 'balanceend', 'stepexbalance'}
      if isempty(P.h), error('mpcekf_session: %s before the first OB_step call created the context', op); end
      switch op
        case 'balancebegin'
          if nargin < 3 || isempty(value), value = 1; end
          mpcekf_mex('balancebegin', P.h, name, value);
        case 'balanceget'
          out = mpcekf_mex('balanceget', P.h);
        case 'balanceend'
          mpcekf_mex('balanceend', P.h);
        case 'stepexbalance'
          [o.u, o.v, o.soc, o.phise, o.nexec, o.ucmd, o.limiter, o.bleed, o.zmin] = mpcekf_mex('stepexbalance', P.h, name);
          out = o;
      end
    case {'chargerbegin', 'chargerget', 'chargerend', 'stepexcharger'}
      if isempty(P.h), error('mpcekf_session: %s before the first OB_step call created the context', op); end
      switch op
        case 'chargerbegin'
          if nargin < 2 || isempty(name), name = P.charger; end
          if isempty(name), error('mpcekf_session: chargerbegin: no params and no charger field set'); end
          mpcekf_mex('chargerbegin', P.h, name);
          P.charger = name;
        case 'chargerget'
          out = mpcekf_mex('chargerget', P.h);
        case 'chargerend'
          mpcekf_mex('chargerend', P.h);
        case 'stepexcharger'
          [o.u, o.v, o.soc, o.phise, o.nexec, o.ucmd, o.limiter, o.bal, o.chg] = mpcekf_mex('stepexcharger', P.h, name);
          out = o;
      end
    case {'limitmap', 'limitmapget', 'limitmapend', 'stepexmap'}
      if isempty(P.h), error('mpcekf_session: %s before the first OB_step call created the context', op); end
      switch op
        case 'limitmap'
          m = name;
          opt = {'T_lo', 'T_hi', 'interp', 'sets', 'z0'};
          for k = 1:numel(opt)
            if ~isfield(m, opt{k}), m.(opt{k}) = []; end
          end
          mpcekf_mex('limitmap', P.h, m.idx, m.z_lo, m.z_hi, m.T_lo, m.T_hi, m.tables, m.interp, m.sets, m.z0);
        case 'limitmapget'
          out = mpcekf_mex('limitmapget', P.h);
        case 'limitmapend'
          mpcekf_mex('limitmapend', P.h);
        case 'stepexmap'
          [o.u, o.v, o.soc, o.phise, o.nexec, lim] = mpcekf_mex('stepexmap', P.h, name);
          o.lim = reshape(lim, size(lim, 1), size(lim, 2) / max(name, 1), name);   % explicit: [] cannot be inferred when nsteps = 0
          out = o;
      end
    otherwise
      error('mpcekf_session: unknown op %s', op);
  end
  S = P;
end
