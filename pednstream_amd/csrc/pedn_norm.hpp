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

struct NormView {
  const float *obs, *rew;        // the raw rows: [R][O], [R][n_agents]
  float *obs_n, *rew_n;          // the normalised rows (rew_n right behind obs_n)
  double *mean, *var, *count;    // [O] each
  double *ret;                   // [R][n_agents] discounted returns
  double *ret_stats;             // mean, var, count of the returns
  const int32_t* tracked;        // [O] 1: normalised; 0: copied (a gater's gate width)
  const int32_t* clock;          // the device-resident step clock (a clocked launch takes `terminated` from it)
  int32_t R, O, n_agents, T;
  int32_t norm_obs, norm_reward, training, pad_;
  double clip_obs, clip_reward, gamma;
};

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
