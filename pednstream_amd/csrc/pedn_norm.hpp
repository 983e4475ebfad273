// Running observation / reward normalisation of the env batch (rl/rl_utils.py:57-300: RunningMeanStd, RunningNormalizeWrapper) -- one
// launch behind whichever launch wrote the observation and reward buffers.  The contract is DESIGN section 11; tests/norm_model.py
// restates it in numpy.
//
// Statistics are binary64 and live on the device.  Per observation column c: mean[c], var[c], count[c] (the reference keeps one count per
// agent; every tracked column of an agent carries the same value, so no workgroup waits for another one's store).  Batch moments over the
// env axis use ONE summation order S, a function of N = n_envs alone:
//   strand s (0 <= s < 64) adds the elements e = s, s + 64, s + 128, ... in increasing e, starting FROM its first element;
//   the min(N, 64) strand sums are the leaves, in order, of a binary tree that pairs neighbours: level 1 adds leaves (2i, 2i + 1),
//   level 2 adds nodes (2i, 2i + 1) of level 1, ...; a node whose right child has no leaf IS its left child (nothing is added).
// N = 1: S(x) = x[0], the batch mean is the row and the batch variance 0 -- the reference wrapper.
//
// norm_kernel, 1024 lanes per workgroup:
//   workgroups [0, ceil(O / 16))   16 observation columns each.  Lane = (column, row slot): the 16 lanes of a quarter wave read 64
//                                  consecutive bytes of one env's row, a wave four rows, the 16 waves 64 rows -- the 64 strands.  Strand
//                                  sums meet in LDS; every lane then walks the tree for its column (16 leaves in registers, two
//                                  cross-lane exchanges), so one barrier per moment and no broadcast of the result.  Merge
//                                  (_update_from_moments, :74-83) in every lane, stored by one; then the normalise pass.
//   the last workgroup             rewards: wave w takes agents w, w + 16, ...: discounted returns and their batch moments (lane = strand);
//                                  one lane merges them into the scalar triple in agent order (:251-267: agent a + 1 sees what agent a
//                                  left) and leaves the variance each agent divides by; all lanes normalise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PEDN_NORM_COLS 16
#define PEDN_NORM_STRANDS 64
#define PEDN_NORM_MAX_AGENTS (PEDN_NORM_COLS * PEDN_NORM_STRANDS)   // batch moments of the returns sit in the strand arrays

__device__ __forceinline__ double norm_clip(double x, double c) { return x < -c ? -c : (x > c ? c : x); }   // (NaN stays NaN, like np.clip)

// RunningMeanStd._update_from_moments, operation for operation
__device__ __forceinline__ void norm_merge(double& mean, double& var, double& count, double bm, double bv, double nd) {
  const double delta = bm - mean;
  const double tot = count + nd;
  mean = mean + delta * nd / tot;
  const double m2 = var * count + bv * nd + delta * delta * count * nd / tot;
  var = m2 / tot;
  count = tot;
}

// the two top levels of the tree for a lane that holds the node over leaves [16 sub, 16 sub + 16)
__device__ __forceinline__ double norm_tree_top(double x, int sub, int cnt) {
  double y = __shfl_xor(x, 16);
  double l = (sub & 1) ? y : x;
  x = ((sub | 1) * 16 < cnt) ? x + y : l;
  y = __shfl_xor(x, 32);
  l = (sub & 2) ? y : x;
  return (32 < cnt) ? x + y : l;
}

// S's tree over the strand sums p[leaf][col] for this lane's column
__device__ __forceinline__ double norm_tree_lds(const double (*p)[PEDN_NORM_COLS], int col, int sub, int cnt) {
  double a[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = p[sub * 16 + i][col];
#pragma unroll
  for (int w = 1; w < 16; w <<= 1)
#pragma unroll
    for (int i = 0; i < 16; i += 2 * w) {
      const double sum = a[i] + a[i + w];
      a[i] = (sub * 16 + i + w < cnt) ? sum : a[i];
    }
  return norm_tree_top(a[0], sub, cnt);
}

// S's tree with lane = leaf
__device__ __forceinline__ double norm_tree_wave(double x, int lane, int cnt) {
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) {
    const double y = __shfl_xor(x, w);
    const double l = (lane & w) ? y : x;
    x = ((lane | w) & ~(w - 1)) < cnt ? x + y : l;
  }
  return x;
}

__device__ __forceinline__ void norm_obs_block(const NormView& n, double (*sP)[PEDN_NORM_COLS], double (*sQ)[PEDN_NORM_COLS]) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int sub = lane >> 4, col = lane & 15;
  const int s = wave * 4 + sub;                              // strand = row slot of the workgroup
  const int c = (int)blockIdx.x * PEDN_NORM_COLS + col;
  const int N = n.R, O = n.O;
  const bool cin = c < O;
  const bool tr = cin && n.norm_obs && n.tracked[c] != 0;
  const int cnt = N < PEDN_NORM_STRANDS ? N : PEDN_NORM_STRANDS;
  const float* x = n.obs + (cin ? c : 0);
  double mean = 0.0, var = 1.0;
  if (tr) { mean = n.mean[c]; var = n.var[c]; }
  if (n.norm_obs && n.training) {   // (uniform over the launch)
    const double nd = (double)N;
    double count = tr ? n.count[c] : 1.0;
    double acc = 0.0;
    if (tr && s < N) {
      acc = (double)x[(size_t)s * O];
      for (int e = s + PEDN_NORM_STRANDS; e < N; e += PEDN_NORM_STRANDS) acc = acc + (double)x[(size_t)e * O];
    }
    sP[s][col] = acc;
    __syncthreads();
    const double bm = norm_tree_lds(sP, col, sub, cnt) / nd;
    acc = 0.0;
    if (tr && s < N) {
      double d = (double)x[(size_t)s * O] - bm;
      acc = d * d;
      for (int e = s + PEDN_NORM_STRANDS; e < N; e += PEDN_NORM_STRANDS) { d = (double)x[(size_t)e * O] - bm; acc = acc + d * d; }
    }
    sQ[s][col] = acc;
    __syncthreads();
    const double bv = norm_tree_lds(sQ, col, sub, cnt) / nd;
    norm_merge(mean, var, count, bm, bv, nd);
    if (tr && s == 0) { n.mean[c] = mean; n.var[c] = var; n.count[c] = count; }
  }
  if (!cin) return;
  float* o = n.obs_n + c;
  if (tr) {
    const double sd = sqrt(var + 1e-8);
    for (int e = s; e < N; e += PEDN_NORM_STRANDS) o[(size_t)e * O] = (float)norm_clip(((double)x[(size_t)e * O] - mean) / sd, n.clip_obs);
  } else
    for (int e = s; e < N; e += PEDN_NORM_STRANDS) o[(size_t)e * O] = x[(size_t)e * O];
}

__device__ __forceinline__ void norm_reward_block(const NormView& n, int rewards, int term, double* sBm, double* sBv) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = n.R, A = n.n_agents;
  const int total = N * A;
  if (!rewards || !n.norm_reward) {   // an observation without a step (reset), or rewards not normalised: the raw rows
    for (int i = tid; i < total; i += (int)blockDim.x) n.rew_n[i] = n.rew[i];
    return;
  }
  const int cnt = N < PEDN_NORM_STRANDS ? N : PEDN_NORM_STRANDS;
  const double nd = (double)N;
  const bool done = term < 0 ? n.clock[1] >= n.T : term != 0;
  const double keep = 1.0 - (done ? 1.0 : 0.0);
  for (int a = wave; a < A; a += (int)(blockDim.x >> 6)) {
    double acc = 0.0;
    for (int e = lane; e < N; e += PEDN_NORM_STRANDS) {
      const size_t i = (size_t)e * A + a;
      const double rt = (double)n.rew[i] + n.gamma * n.ret[i] * keep;
      n.ret[i] = rt;
      acc = e == lane ? rt : acc + rt;
    }
    if (n.training) {   // (uniform)
      const double bm = norm_tree_wave(acc, lane, cnt) / nd;
      acc = 0.0;
      for (int e = lane; e < N; e += PEDN_NORM_STRANDS) {
        const double d = n.ret[(size_t)e * A + a] - bm;   // (this lane's own store)
        acc = e == lane ? d * d : acc + d * d;
      }
      const double bv = norm_tree_wave(acc, lane, cnt) / nd;
      if (lane == 0) { sBm[a] = bm; sBv[a] = bv; }
    }
  }
  __syncthreads();
  if (tid == 0) {   // the agent loop of _normalize_rewards: sequential by contract
    double mean = n.ret_stats[0], var = n.ret_stats[1], count = n.ret_stats[2];
    for (int a = 0; a < A; ++a) {
      if (n.training) norm_merge(mean, var, count, sBm[a], sBv[a], nd);
      sBm[a] = var;   // what agent a's rewards are divided by
    }
    if (n.training) { n.ret_stats[0] = mean; n.ret_stats[1] = var; n.ret_stats[2] = count; }
  }
  __syncthreads();
  for (int i = tid; i < total; i += (int)blockDim.x)
    n.rew_n[i] = (float)norm_clip((double)n.rew[i] / sqrt(sBm[i % A] + 1e-8), n.clip_reward);
}

// rewards: 1 the launch follows an env step (returns, statistics, normalised rewards); 0 it follows an observation alone (raw rewards copied)
// term: the step's terminated flag, or -1: read it from the step clock
__global__ __launch_bounds__(1024) void norm_kernel(NormView n, int rewards, int term) {
  __shared__ double sP[PEDN_NORM_STRANDS][PEDN_NORM_COLS];
  __shared__ double sQ[PEDN_NORM_STRANDS][PEDN_NORM_COLS];
  if (blockIdx.x + 1 == gridDim.x) norm_reward_block(n, rewards, term, &sP[0][0], &sQ[0][0]);
  else norm_obs_block(n, sP, sQ);
}

// ---- host side: pedn_rl_norm_* of include/pedn.h; the core calls norm_launch (behind whatever wrote the raw rows) and norm_reset_returns
static void norm_launch(pedn_sim* s, hipStream_t st, int rewards, int term) {
  if (!s->norm.on) return;
  const unsigned blocks = (unsigned)((s->norm.view.O + PEDN_NORM_COLS - 1) / PEDN_NORM_COLS) + 1u;   // + the reward workgroup
  hipLaunchKernelGGL(norm_kernel, dim3(blocks), dim3(1024), 0, st, s->norm.view, rewards, term);
}

static int norm_reset_returns(pedn_sim* s) {   // a new episode: the discounted returns start again, the statistics stay
  if (!s->norm.alloc) return PEDN_OK;
  HIP_TRY(s, hipMemsetAsync(s->norm.view.ret, 0, (size_t)s->v.R * s->rl.n_agents * sizeof(double), s->stream));
  return PEDN_OK;
}

static int norm_init_stats(pedn_sim* s) {
  const int O = s->rl.O;
  std::vector<double> h((size_t)3 * O + 3);
  for (int c = 0; c < O; ++c) { h[c] = 0.0; h[(size_t)O + c] = 1.0; h[(size_t)2 * O + c] = 1e-4; }
  h[(size_t)3 * O] = 0.0; h[(size_t)3 * O + 1] = 1.0; h[(size_t)3 * O + 2] = 1e-4;
  HIP_TRY(s, hipMemcpy(s->norm.view.mean, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  return PEDN_OK;
}

int pedn_rl_norm_configure(pedn_sim* s, int32_t norm_obs, int32_t norm_reward, double clip_obs, double clip_reward, double gamma,
                           const int32_t* tracked_mask, const int32_t* agent_of_column) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->rl_ready) return fail(s, PEDN_E_ARG, "pedn_rl_configure has not been called");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);   // (ends a clocked section: a captured graph is checked against the signature before its next replay)
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  const RlView& q = s->rl;
  if (!norm_obs && !norm_reward) {   // off: the fetches hand out the raw rows again; the statistics are discarded
    s->norm.on = false;
    const NormView keep = s->norm.view;
    memset(&s->norm.view, 0, sizeof s->norm.view);
    if (s->norm.alloc) {   // (the buffers stay with the agent set)
      s->norm.view.obs_n = keep.obs_n; s->norm.view.rew_n = keep.rew_n; s->norm.view.mean = keep.mean; s->norm.view.var = keep.var; s->norm.view.count = keep.count;
      s->norm.view.ret = keep.ret; s->norm.view.ret_stats = keep.ret_stats; s->norm.view.tracked = keep.tracked;
    }
    store_sources(s);
    return PEDN_OK;
  }
  if (s->ctrl.ready) return fail(s, PEDN_E_ARG, "controllers and the running normalisation cannot be combined");
  if (!tracked_mask || !agent_of_column) return fail(s, PEDN_E_ARG, "null argument");
  if (!(clip_obs > 0.0) || !(clip_reward > 0.0)) return fail(s, PEDN_E_ARG, "clip_obs and clip_reward must be positive");
  if (q.n_agents > PEDN_NORM_MAX_AGENTS) return fail(s, PEDN_E_ARG, "more than 1024 agents");
  if ((int64_t)s->v.R * std::max(q.O, q.n_agents) > 0x7fffffff) return fail(s, PEDN_E_ARG, "observation buffer too large for the normalisation kernel");
  for (int c = 0; c < q.O; ++c)
    if (agent_of_column[c] < 0 || agent_of_column[c] >= q.n_agents) return fail(s, PEDN_E_ARG, "agent_of_column out of range");
  int rc;
  NormView n;
  memset(&n, 0, sizeof n);   // (padding too: the view is hashed as bytes, pedn_rl_clock_signature)
  if (!s->norm.alloc) {
    double* d = nullptr;
    float* f = nullptr;
    int32_t* m = nullptr;
    const size_t n_ret = (size_t)s->v.R * q.n_agents;
    if ((rc = dalloc(s, (size_t)3 * q.O + 3 + n_ret, &d)) != PEDN_OK) return rc;
    if ((rc = dalloc(s, (size_t)s->v.R * q.O + n_ret, &f)) != PEDN_OK) return rc;
    if ((rc = dalloc(s, (size_t)q.O, &m)) != PEDN_OK) return rc;
    n.mean = d; n.var = d + q.O; n.count = d + 2 * (size_t)q.O; n.ret_stats = d + 3 * (size_t)q.O; n.ret = n.ret_stats + 3;
    n.obs_n = f; n.rew_n = f + (size_t)s->v.R * q.O;
    n.tracked = m;
    HIP_TRY(s, hipMemset(f, 0, ((size_t)s->v.R * q.O + n_ret) * sizeof(float)));
  } else {
    const NormView& o = s->norm.view;
    n.mean = o.mean; n.var = o.var; n.count = o.count; n.ret_stats = o.ret_stats; n.ret = o.ret; n.obs_n = o.obs_n; n.rew_n = o.rew_n; n.tracked = o.tracked;
  }
  n.obs = q.obs; n.rew = q.rew; n.clock = s->d_clock;
  n.R = s->v.R; n.O = q.O; n.n_agents = q.n_agents; n.T = s->v.T1 - 1;
  n.norm_obs = norm_obs ? 1 : 0; n.norm_reward = norm_reward ? 1 : 0; n.training = 1;
  n.clip_obs = clip_obs; n.clip_reward = clip_reward; n.gamma = gamma;
  s->norm.view = n;
  s->norm.alloc = true;
  s->norm.tracked.assign(tracked_mask, tracked_mask + q.O);
  for (int32_t& t : s->norm.tracked) t = t ? 1 : 0;
  s->norm.agent.assign(agent_of_column, agent_of_column + q.O);
  HIP_TRY(s, hipMemcpy(const_cast<int32_t*>(n.tracked), s->norm.tracked.data(), (size_t)q.O * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(s, hipMemset(n.ret, 0, (size_t)s->v.R * q.n_agents * sizeof(double)));
  if ((rc = norm_init_stats(s)) != PEDN_OK) return rc;
  s->norm.on = true;
  store_sources(s);
  return PEDN_OK;
}

int pedn_rl_norm_set_training(pedn_sim* s, int32_t training) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->norm.on) return fail(s, PEDN_E_ARG, "pedn_rl_norm_configure has not switched the normalisation on");
  HIP_TRY(s, hipSetDevice(s->device));
  join_forked(s);   // (the flag travels in the launch's arguments: a clocked section ends, a captured graph is captured again)
  s->norm.view.training = training ? 1 : 0;
  return PEDN_OK;
}

int pedn_rl_norm_get_stats(pedn_sim* s, double* mean, double* var, double* count, double* ret_stats) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->norm.on) return fail(s, PEDN_E_ARG, "pedn_rl_norm_configure has not switched the normalisation on");
  HIP_TRY(s, hipSetDevice(s->device));
  join_forked(s);
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  const int O = s->norm.view.O;
  std::vector<double> h((size_t)3 * O + 3);
  HIP_TRY(s, hipMemcpy(h.data(), s->norm.view.mean, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (mean) memcpy(mean, h.data(), (size_t)O * sizeof(double));
  if (var) memcpy(var, h.data() + O, (size_t)O * sizeof(double));
  if (count) {   // per agent: the count of its tracked columns (they all carry the same one)
    for (int a = 0; a < s->norm.view.n_agents; ++a) count[a] = 1e-4;
    for (int c = O - 1; c >= 0; --c)
      if (s->norm.tracked[c]) count[s->norm.agent[c]] = h[(size_t)2 * O + c];
  }
  if (ret_stats) memcpy(ret_stats, h.data() + (size_t)3 * O, 3 * sizeof(double));
  return PEDN_OK;
}

int pedn_rl_norm_set_stats(pedn_sim* s, const double* mean, const double* var, const double* count, const double* ret_stats) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->norm.on) return fail(s, PEDN_E_ARG, "pedn_rl_norm_configure has not switched the normalisation on");
  HIP_TRY(s, hipSetDevice(s->device));
  join_forked(s);
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  const int O = s->norm.view.O;
  std::vector<double> h((size_t)3 * O + 3);
  HIP_TRY(s, hipMemcpy(h.data(), s->norm.view.mean, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (mean) memcpy(h.data(), mean, (size_t)O * sizeof(double));
  if (var) memcpy(h.data() + O, var, (size_t)O * sizeof(double));
  if (count)
    for (int c = 0; c < O; ++c) h[(size_t)2 * O + c] = count[s->norm.agent[c]];
  if (ret_stats) memcpy(h.data() + (size_t)3 * O, ret_stats, 3 * sizeof(double));
  HIP_TRY(s, hipMemcpy(s->norm.view.mean, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  return PEDN_OK;
}

void* pedn_rl_norm_device_ptr(pedn_sim* s, int32_t which) {
  if (!s || !s->norm.on) return nullptr;
  const NormView& n = s->norm.view;
  switch (which) {
    case 0: return n.obs_n;
    case 1: return n.rew_n;
    case 2: return n.mean;
    case 3: return n.var;
    case 4: return n.count;
    case 5: return n.ret;
    case 6: return n.ret_stats;
  }
  return nullptr;
}
