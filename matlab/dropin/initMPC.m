function mpcData = initMPC(SOC0, Np, Nc, targetSOC, opts)
% Drop-in for initMPC.m:1 over the MI355X library: records the horizons, the
% constraint switches and the limits for the context the first OB_step call creates.
% targetSOC, opts.Crate and the fields of opts.limits (u_max, du_min, du_max, v_max,
% phise_min, z_max, z_tol) may each be a vector with one entry per cell (numel(SOC0)): a
% protocol sweep over the batch (runMPC.m:30-44 per cell).  The context is created from the
% first entries; the vectors go to it through mpcekf_mex('setlimits', ...) after 'init'
% (OB_step's first call).  Scalars behave as before.
  L = opts.limits;
  n = numel(SOC0);
  % mpcekf_mex('setlimits') field numbers (MPCEKF_LIM_* + 1) and this call's values
  names = {'target_soc', 'Crate', 'u_max', 'du_min', 'du_max', 'v_max', 'phise_min', 'z_max', 'z_tol'};
  vals = {targetSOC, opts.Crate, L.u_max, L.du_min, L.du_max, L.v_max, L.phise_min, L.z_max, L.z_tol};
  idx = [];
  percell = zeros(n, 0);
  for k = 1:numel(vals)
    if ~isscalar(vals{k})
      if numel(vals{k}) ~= n
        error('initMPC: %s has %d entries; expected a scalar or one per cell (%d)', names{k}, numel(vals{k}), n);
      end
      idx(end + 1) = k;                                      %#ok<AGROW>
      percell(:, end + 1) = vals{k}(:);                      %#ok<AGROW>  ncells x numel(idx)
      vals{k} = vals{k}(1);
    end
  end
  cfg = struct('Np', Np, 'Nc', Nc, 'target_soc', vals{1}, 'Crate', vals{2}, ...
               'u_max', vals{3}, 'du_min', vals{4}, 'du_max', vals{5}, 'v_min', L.v_min, ...
               'v_max', vals{6}, 'phise_min', vals{7}, 'z_max', vals{8}, 'z_tol', vals{9}, ...
               'use_current', opts.constraints(1), 'use_voltage', opts.constraints(2), ...
               'use_eta', opts.constraints(3));
  mpcData = struct('SOC0', SOC0, 'Np', Np, 'Nc', Nc, 'ref', targetSOC, 'uk_1', 0, 'limits', L, ...
                   'maxHild', 100, 'mpcekf_cfg', cfg, ...
                   'mpcekf_limits', struct('idx', idx, 'values', percell));
  mpcekf_session('set', 'mpc', mpcData);
end
