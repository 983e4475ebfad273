// The gradient-free half of the reference's PPOAgent.update (rl/agents/PPO_org.py:543-577: value_net on states and next states with the
// StackedValueNetwork :175-197, the StackedPolicyNetwork on states and Normal.log_prob of the stored actions) for every row of a rollout,
// every env and every agent in ONE launch.  The contract is DESIGN section 16; tests/ppo_eval_model.py restates it in numpy.
//
// ppo_eval_kernel   grid (ceil((T + 1) * N / PEDN_PPO_TILE), n_agents, 2), 256 threads.  blockIdx.z = 0 is the value half over the
//                   (T + 1) * N rows r = t * N + e, blockIdx.z = 1 the actor half over the first T * N (its workgroups behind the last
//                   row leave before any barrier).  A workgroup evaluates one network of one agent for a tile of 32 consecutive rows
//                   with section 14's data path, pedn_mlp.hpp's mlp_layer: 4 waves, 8 rows each, a lane per neuron, chunks of 32
//                   inputs, hidden rows of 64 in LDS that only the row's own wave touches.  The first layer's inputs are put together
//                   on the fly (the kernel's gather): input i = f * S + s of row (t, e) is obs[max(t - (S - 1) + s, 0)][e][obs0 + f];
//                   a row's t and e are formed once per workgroup (the only 64-bit divisions), every offset into obs is 64-bit.
//                   The actor half calls what actor_forward_kernel calls (mlp_trunk with the LayerNorm, mlp_heads, mlp_softplus),
//                   so its mu and std are the bits that acted; its tail is normal_log_prob on a lane per (row, action).  The value
//                   half ends with value_head on a lane per row.
//                   LDS: 64 * 33 + 32 * 32 + 32 * 64 + 32 * 16 + 2 * 32 words = 23040 bytes, 7 workgroups per CU by LDS; the register
//                   budget is capped at 128 VGPRs (4 waves per SIMD: the compiler would take 136 and leave 3).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_actor.hpp"
#include "pedn_mlp.hpp"

#define PEDN_PPO_TILE PEDN_ACTOR_TILE             // rows per workgroup: mlp_layer's tile
#define PEDN_PPO_WAVE_ROWS PEDN_ACTOR_WAVE_ENVS    // rows per wave

struct PpoEvalArgs {
  const float* obs;        // [T + 1][N][n_obs]
  const void* actions;     // [T][N][n_actions], float or double
  const int32_t* table;    // [n_agents][PEDN_ACTOR_TABLE_COLS]: the actors' table
  const int32_t* vtable;   // [n_agents]: offsets (floats) in the value pack
  const float* actor;      // the actors' pack (PPO kind)
  const float* value;      // the value pack
  float* values;           // [T + 1][N][n_agents]
  float* logp;             // [T][N][n_actions]
  float *mu, *std;         // [T][N][n_actions] or null
  int64_t rows_v, rows_a;  // (T + 1) * N, T * N
  int32_t N, S, n_obs, n_actions, n_agents;
  int32_t act_f64;
  float min_std, max_std;
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void ppo_eval_kernel(PpoEvalArgs a) {
  __shared__ float sW[PEDN_ACTOR_HIDDEN * (PEDN_ACTOR_CHUNK + 1)];
  __shared__ __attribute__((aligned(16))) float sXc[PEDN_PPO_TILE * PEDN_ACTOR_CHUNK];
  __shared__ __attribute__((aligned(16))) float sH[PEDN_PPO_TILE * PEDN_ACTOR_HIDDEN];
  __shared__ float sOut[PEDN_PPO_TILE * 2 * PEDN_ACTOR_MAX_ACT];
  __shared__ int32_t sT[PEDN_PPO_TILE], sE[PEDN_PPO_TILE];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int H = PEDN_ACTOR_HIDDEN;
  const bool is_actor = blockIdx.z != 0;
  const int64_t n_rows = is_actor ? a.rows_a : a.rows_v;
  const int64_t row0 = (int64_t)blockIdx.x * PEDN_PPO_TILE;
  if (row0 >= n_rows) return;   // (the whole workgroup: the actor half has N rows fewer)
  const int agent = (int)blockIdx.y;
  const int32_t* t = a.table + (size_t)agent * PEDN_ACTOR_TABLE_COLS;
  const int obs0 = t[0], obs_w = t[1], act0 = t[2], act_w = t[3];
  if (threadIdx.x < PEDN_PPO_TILE) {
    const int64_t r = row0 + (int64_t)threadIdx.x;
    const int64_t tr = r / (int64_t)a.N;
    sT[threadIdx.x] = r < n_rows ? (int32_t)tr : -1;
    sE[threadIdx.x] = (int32_t)(r - tr * (int64_t)a.N);
  }
  // input i = f * S + s of row (t, e) is obs[max(t - (S - 1) + s, 0)][e][obs0 + f]; sT / sE hold the tile's t and e, -1 behind the last row
  const auto gather = [&](int c0, int kmax) {
    // a thread's column kk, and with it the frame s and the feature f, is the same in its 4 rows of the tile
    const int kk = (int)(threadIdx.x & (PEDN_ACTOR_CHUNK - 1));
    const unsigned k = (unsigned)(c0 + kk), f = k / (unsigned)a.S, s = k - f * (unsigned)a.S;
#pragma unroll
    for (int i = 0; i < PEDN_PPO_TILE * PEDN_ACTOR_CHUNK / 256; ++i) {
      const int r = (int)(threadIdx.x >> 5) + i * (256 / PEDN_ACTOR_CHUNK);
      const int t = sT[r];
      float x = 0.0f;
      if (kk < kmax && t >= 0) {
        int tt = t - (a.S - 1) + (int)s;
        tt = tt < 0 ? 0 : tt;
        x = a.obs[((size_t)tt * (size_t)a.N + (size_t)sE[r]) * (size_t)a.n_obs + (size_t)(obs0 + (int)f)];
      }
      sXc[r * PEDN_ACTOR_CHUNK + kk] = x;
    }
  };
  // both networks start with encoder.fc1, encoder.fc2 and fc; behind them the actor has its LayerNorm, fc_mu and fc_std (rest: fc_mu),
  // the value network its value_head (rest)
  float acc[PEDN_PPO_WAVE_ROWS];
  const float* rest = mlp_trunk(acc, is_actor ? a.actor + t[4] : a.value + a.vtable[agent], a.S * obs_w, is_actor, sW, sXc, sH, gather);
  if (!is_actor) {
    // value_head on a lane per row of the wave: v = b; v = v + w[k] * h[k], k ascending
    __syncthreads();   // (the wave's own rows; the barrier orders the LDS writes before the reads)
    if (lane < PEDN_PPO_WAVE_ROWS) {
      const int lr = wave * PEDN_PPO_WAVE_ROWS + lane;
      const float* h = sH + lr * H;
      float v = rest[H];
      for (int k = 0; k < H; ++k) v = v + rest[k] * h[k];
      const int64_t r = row0 + lr;
      if (r < n_rows) a.values[(size_t)r * (size_t)a.n_agents + (size_t)agent] = v;
    }
    return;
  }
  const float* so = mlp_heads(acc, rest, act_w, sW, sXc, sH, sOut, gather);
  const int lr = lane / act_w, j = lane - lr * act_w;
  const int64_t row = row0 + (int64_t)(wave * PEDN_PPO_WAVE_ROWS + lr);
  if (lr < PEDN_PPO_WAVE_ROWS && row < n_rows) {
    const float mu = so[lr * 2 * PEDN_ACTOR_MAX_ACT + j], z = so[lr * 2 * PEDN_ACTOR_MAX_ACT + PEDN_ACTOR_MAX_ACT + j];
    const size_t at = (size_t)row * (size_t)a.n_actions + (size_t)(act0 + j);
    const float sd = actor_clip(mlp_softplus(z), a.min_std, a.max_std);
    const float act = a.act_f64 ? (float)static_cast<const double*>(a.actions)[at] : static_cast<const float*>(a.actions)[at];
    a.logp[at] = (float)normal_log_prob(act, mu, sd);   // (rounded once)
    if (a.mu) a.mu[at] = mu;
    if (a.std) a.std[at] = sd;
  }
}

// ---- host side: pedn_ppo_evaluate of include/pedn.h; no state in the engine's handle
int pedn_ppo_evaluate(const float* obs, const void* actions, const int32_t* table, const int32_t* value_table, const float* actor_params,
                      const float* value_params, float* values, float* old_log_probs, float* mu, float* std, int32_t T, int32_t N,
                      int32_t stack_size, int32_t n_obs, int32_t n_actions, int32_t n_agents, int32_t hidden_size, int32_t actions_f64,
                      double min_std, double max_std, void* stream) {
  if (!obs || !actions || !table || !value_table || !actor_params || !value_params || !values || !old_log_probs)
    return fail(nullptr, PEDN_E_ARG, "null argument");
  if (hidden_size != PEDN_ACTOR_HIDDEN) return fail(nullptr, PEDN_E_ARG, "the PPO evaluation kernel is built for hidden_size 64");
  if (T < 1 || N < 1 || stack_size < 1 || n_obs < 1 || n_actions < 1 || n_agents < 1 || n_agents > 65535)
    return fail(nullptr, PEDN_E_ARG, "T, N, stack_size, n_obs, n_actions and n_agents must be positive (at most 65535 agents)");
  if (actions_f64 < 0 || actions_f64 > 1) return fail(nullptr, PEDN_E_ARG, "the actions' dtype flag is 0 (float32) or 1 (float64)");
  PpoEvalArgs a{};
  a.obs = obs; a.actions = actions; a.table = table; a.vtable = value_table; a.actor = actor_params; a.value = value_params;
  a.values = values; a.logp = old_log_probs; a.mu = mu; a.std = std;
  a.rows_a = (int64_t)T * (int64_t)N; a.rows_v = a.rows_a + N;
  a.N = N; a.S = stack_size; a.n_obs = n_obs; a.n_actions = n_actions; a.n_agents = n_agents; a.act_f64 = actions_f64;
  a.min_std = (float)min_std; a.max_std = (float)max_std;
  const int64_t tiles = (a.rows_v + PEDN_PPO_TILE - 1) / PEDN_PPO_TILE;
  if (tiles > 0x7fffffffLL) return fail(nullptr, PEDN_E_ARG, "(T + 1) * N is beyond the grid's 2^31 - 1 tiles of 32 rows");
  hipLaunchKernelGGL(ppo_eval_kernel, dim3((unsigned)tiles, (unsigned)n_agents, 2u), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}
