// Rule-based controllers on the device (include/pedn.h: pedn_ctrl_*): the reference's RuleBasedGaterAgent and
// RuleBasedSeparatorAgent (rl/agents/rule_based.py) for every env, computed by wave 0 of the observation block of an agent from the
// float32 observation it has just written -- no extra launch, no host round trip between env steps.
//
//   gater      avg = np.mean(densities) (float32: a sequential sum below 8 links, NumPy's 8-way pairwise sum at 8);
//              avg <= 2: every link's physical width; otherwise per link current_width + 1 / - 1 (float32) when the density is above /
//              below the threshold (float32), the link's width when equal
//   separator  x = obs[1] (the forward link's outflow; obs[4] does not exist, the reverse term is 0.0):
//              no smoothing  x + 0 == 0 ? width / 2 : width * x / (x + 0)   in float32 (binary64 when the width is a numpy float64)
//              smoothing     m = float(np.mean(last `window` values of x))  (float32 mean), then the same in binary64
// Every action is rounded to float32 and widened into the engine-owned action rows [R][A] (NaN = no action: agents without a controller).
// The moving-average buffers are [slot][RS] float32 rows per agent plus a count per (agent, replica); each value has one writer (the lane
// of its replica), so the two half-batch chains and any launch plan keep them consistent without atomics.
#pragma once

#define PEDN_CTRL_MAX_WINDOW 32   // longest moving-average window of a separator controller (pedn_ctrl_configure refuses longer)

template <bool CTRL>
__device__ __forceinline__ void ctrl_decide(const CtrlView& cv, const RlView& q, int ag, int type, int n, int r, const float* o,
                                            const float (*sD)[64], const float (*sG)[64], int lane, float reward_sum) {
  float* ep = cv.ep + (size_t)r * q.n_agents + ag;
  *ep = cv.ep_mode == 2 ? 0.0f : *ep + reward_sum;   // episode_true_rewards[a] += rewards[a] (rl_utils.py:1593-1599)
  const CtrlAgent C = cv.agent[ag];
  const int a0 = q.agent_act_off[ag];
  double* act = cv.actions + (size_t)r * q.A + a0;
  if (C.kind == 1 && type == 1) {
    const float avg = numpy_sum_f32(n, [&](int i) { return sD[i][lane]; }) / (float)n;
    if (avg <= 2.0f) {
      for (int i = 0; i < n; ++i) act[i] = (double)cv.open[a0 + i];
    } else {
      for (int i = 0; i < n; ++i) {
        const float d = sD[i][lane], cw = sG[i][lane];
        const float x = d > C.thr ? cw + 1.0f : (d < C.thr ? cw - 1.0f : cv.open[a0 + i]);
        act[i] = (double)x;
      }
    }
  } else if (C.kind == 2 && type == 0) {
    const float x = o[1];
    float a;
    if (C.window > 0) {   // _update_and_smooth_inflow: append, drop the oldest beyond the window, float(np.mean(buffer))
      const size_t RS = (size_t)cv.RS;
      int32_t* cnt = cv.count + (size_t)ag * RS + r;
      const int c = *cnt, w = C.window;
      const float* ring = cv.ring + (size_t)C.ring * RS + r;
      cv.ring[((size_t)C.ring + (size_t)(c % w)) * RS + r] = x;
      *cnt = c + 1;
      const int m = min(c + 1, w), first = c + 1 - m;   // values first .. c, oldest first
      const float mean = numpy_sum_f32(m, [&](int i) { return ring[(size_t)((first + i) % w) * RS]; }) / (float)m;
      const double li = (double)mean;
      a = li + 0.0 == 0.0 ? (float)(C.w64 / 2.0) : (float)(C.w64 * li / (li + 0.0));
    } else if (x + 0.0f == 0.0f) {
      a = (float)(C.w64 / 2.0);
    } else {
      a = C.wide ? (float)(C.w64 * (double)x / (double)(x + 0.0f)) : (C.w32 * x) / (x + 0.0f);
    }
    act[0] = (double)a;
  }
}

// rl_observe_kernel with the controllers (pedn_ctrl_observe, and pedn_ctrl_step when the observations are a launch of their own)
template <bool HIST>
__global__ __launch_bounds__(256) void ctrl_observe_kernel(DevView v, RlView q, int t, int accumulate, CtrlView cv) {
  __shared__ float lds[PEDN_CTRL_LDS_FLOATS];
  rl_observe_body<false, HIST, true>(v, q, t, accumulate, blockIdx.x, lds, &cv);
}

// link_turn_kernel<PR, true, HIST> with the controllers: the last sub-step of a controlled env step (pedn_ctrl_step)
template <bool PR, bool HIST>
__global__ __launch_bounds__(256, 4) void ctrl_link_turn_kernel(DevView v, int t, unsigned n_link_blocks, unsigned n_tp_blocks, unsigned n_tp_heavy,
                                                                RlView q, int accumulate, CtrlView cv) {
  __shared__ double lds[PEDN_TF_LDS_DOUBLES];
  static_assert(sizeof(double) * PEDN_TF_LDS_DOUBLES >= sizeof(float) * PEDN_CTRL_LDS_FLOATS, "observation rows must fit");
  link_turn_body<PR, true, HIST, false, true>(v, t, n_link_blocks, n_tp_blocks, n_tp_heavy, q, accumulate, lds, &cv);
}

// ---- host side: pedn_ctrl_* of include/pedn.h.  The core launches the twins above when handed a CtrlView (rl_observe, rl_step)
int pedn_ctrl_configure(pedn_sim* s, const int32_t* kind, const int32_t* window, const int32_t* wide, const float* threshold,
                        const double* width, const float* open) {
  if (!s || !kind || !window || !wide || !threshold || !width || !open) return fail(s, PEDN_E_ARG, "null argument");
  if (!s->rl_ready) return fail(s, PEDN_E_ARG, "pedn_rl_configure has not been called");
  if (s->norm.on) return fail(s, PEDN_E_ARG, "controllers and the running normalisation cannot be combined: switch the normalisation off first");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  const RlView& q = s->rl;
  std::vector<int32_t> type((size_t)q.n_agents);
  HIP_TRY(s, hipMemcpy(type.data(), q.agent_type, type.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<CtrlAgent> ag((size_t)q.n_agents);
  int rows = 0;
  bool any = false;
  for (int a = 0; a < q.n_agents; ++a) {
    CtrlAgent& c = ag[a];
    c.kind = kind[a];
    if (c.kind < 0 || c.kind > 2) return fail(s, PEDN_E_ARG, "controller kind must be 0 (none), 1 (gater rule) or 2 (separator rule)");
    if (c.kind == 1 && type[a] != 1) return fail(s, PEDN_E_ARG, "agent " + std::to_string(a) + " is not a gater");
    if (c.kind == 1 && q.obs_mode != 2) return fail(s, PEDN_E_ARG, "the gater rule reads densities: obs_mode must be option2");
    if (c.kind == 2 && type[a] != 0) return fail(s, PEDN_E_ARG, "agent " + std::to_string(a) + " is not a separator");
    c.window = c.kind == 2 ? window[a] : 0;
    if (c.window < 0 || c.window > PEDN_CTRL_MAX_WINDOW)
      return fail(s, PEDN_E_ARG, "moving-average window outside 0.." + std::to_string(PEDN_CTRL_MAX_WINDOW));
    c.wide = wide[a] != 0;
    c.ring = rows;
    rows += c.window;
    c.thr = threshold[a];
    c.w64 = width[a];
    c.w32 = (float)width[a];
    any = any || c.kind != 0;
  }
  const DevView& v = s->v;
  CtrlView& cv = s->ctrl.view;
  int rc;
  // (sizes depend only on the agent set: allocated once per pedn_rl_configure, the moving-average rows grow when a call needs more)
  static_assert(sizeof(CtrlAgent) == 32, "CtrlAgent is uploaded as bytes");
  if (!cv.actions || s->ctrl.ready == false) {
    CtrlAgent* d_ag;
    float* d_open;
    if ((rc = dalloc(s, (size_t)q.n_agents, &d_ag)) != PEDN_OK) return rc;
    if ((rc = dalloc(s, (size_t)q.A, &d_open)) != PEDN_OK) return rc;
    if ((rc = dalloc(s, (size_t)v.R * q.A, &cv.actions)) != PEDN_OK) return rc;
    if ((rc = dalloc(s, (size_t)v.R * q.n_agents, &cv.ep)) != PEDN_OK) return rc;
    if ((rc = dalloc(s, (size_t)q.n_agents * v.RS, &cv.count)) != PEDN_OK) return rc;
    cv.agent = d_ag;
    cv.open = d_open;
    cv.ring = nullptr;
    s->ctrl.rows = 0;
  }
  if (rows > s->ctrl.rows) {
    if ((rc = dalloc(s, (size_t)rows * v.RS, &cv.ring)) != PEDN_OK) return rc;
    s->ctrl.rows = rows;
  }
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  HIP_TRY(s, hipMemcpy(const_cast<CtrlAgent*>(cv.agent), ag.data(), ag.size() * sizeof(CtrlAgent), hipMemcpyHostToDevice));
  HIP_TRY(s, hipMemcpy(const_cast<float*>(cv.open), open, (size_t)q.A * sizeof(float), hipMemcpyHostToDevice));
  std::vector<double> nan((size_t)v.R * q.A, __builtin_nan(""));   // no action until the first observation decides one
  HIP_TRY(s, hipMemcpy(cv.actions, nan.data(), nan.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(s, hipMemset(cv.ep, 0, (size_t)v.R * q.n_agents * sizeof(float)));
  HIP_TRY(s, hipMemset(cv.count, 0, (size_t)q.n_agents * v.RS * sizeof(int32_t)));   // every moving-average buffer empty
  cv.RS = v.RS;
  cv.ep_mode = 1;
  s->ctrl.ready = true;
  s->ctrl.any = any;
  return PEDN_OK;
}

int pedn_ctrl_observe(pedn_sim* s, int32_t t) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->ctrl.ready) return fail(s, PEDN_E_ARG, "pedn_ctrl_configure has not been called");
  CtrlView cv = s->ctrl.view;
  cv.ep_mode = 2;
  return rl_observe(s, t, 0, nullptr, nullptr, &cv);
}

int pedn_ctrl_step(pedn_sim* s, int32_t t, int32_t action_gap, int32_t n_steps) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->ctrl.ready) return fail(s, PEDN_E_ARG, "pedn_ctrl_configure has not been called");
  if (n_steps < 0 || action_gap < 1 || t < 1 || t + (int64_t)n_steps * action_gap - 1 > s->v.T1 - 1)
    return fail(s, PEDN_E_ARG, "step range outside 1..T");
  CtrlView cv = s->ctrl.view;
  cv.ep_mode = 1;
  for (int i = 0; i < n_steps; ++i) {
    const int rc = rl_step(s, s->ctrl.any ? s->ctrl.view.actions : nullptr, 1, t + i * action_gap, action_gap, nullptr, nullptr, &cv);
    if (rc != PEDN_OK) return rc;
  }
  return PEDN_OK;
}

int pedn_ctrl_read(pedn_sim* s, double* actions, float* episode_rewards) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->ctrl.ready) return fail(s, PEDN_E_ARG, "pedn_ctrl_configure has not been called");
  HIP_TRY(s, hipSetDevice(s->device));
  join_forked(s);
  const size_t R = (size_t)s->v.R;
  if (actions) HIP_TRY(s, hipMemcpyAsync(actions, s->ctrl.view.actions, R * s->rl.A * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  if (episode_rewards)
    HIP_TRY(s, hipMemcpyAsync(episode_rewards, s->ctrl.view.ep, R * s->rl.n_agents * sizeof(float), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return PEDN_OK;
}

void* pedn_ctrl_device_ptr(pedn_sim* s, int32_t which) {
  if (!s || !s->ctrl.ready) return nullptr;
  return which == 0 ? (void*)s->ctrl.view.actions : which == 1 ? (void*)s->ctrl.view.ep : nullptr;
}
