// The gradient-free half of the reference's PPOAgent.update (rl/agents/PPO_org.py:543-577: value_net on states and next states with the
// StackedValueNetwork :175-197, the StackedPolicyNetwork on states and Normal.log_prob of the stored actions) for every row of a rollout,
// every env and every agent in ONE launch.  The contract is DESIGN section 16; tests/ppo_eval_model.py restates it in numpy.
//
// ppo_eval_kernel   grid (ceil((T + 1) * N / PEDN_PPO_TILE), n_agents, 2), 256 threads.  blockIdx.z = 0 is the value half over the
//                   (T + 1) * N rows r = t * N + e, blockIdx.z = 1 the actor half over the first T * N (its workgroups behind the last
//                   row leave before any barrier).  A workgroup evaluates one network of one agent for a tile of 32 consecutive rows
//                   with section 14's data path: 4 waves, 8 rows each, a lane per neuron, chunks of 32 inputs whose weight rows
//                   (nn.Linear's [out][in]) are staged in LDS rows of 33 words, acc[r] = acc[r] + w * x[r][k], k ascending, one
//                   accumulator per (row, neuron); hidden rows of 64 in LDS that only the row's own wave touches.  The first layer's
//                   inputs are put together on the fly: input i = f * S + s of row (t, e) is obs[max(t - (S - 1) + s, 0)][e][obs0 + f];
//                   a row's t and e are formed once per workgroup (the only 64-bit divisions), every offset into obs is 64-bit.
//                   The actor half is actor_forward_kernel's arithmetic operation for operation (LayerNorm as the balanced tree,
//                   the heads as one layer of 2 * act_w rows, softplus in double), so its mu and std are the bits that acted; its tail
//                   is Normal.log_prob in double on a lane per (row, action).  The value half ends with value_head on a lane per row.
//                   LDS: 64 * 33 + 32 * 32 + 32 * 64 + 32 * 16 + 2 * 32 words = 23040 bytes, 7 workgroups per CU by LDS; the register
//                   budget is capped at 128 VGPRs (4 waves per SIMD: the compiler would take 136 and leave 3).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_actor.hpp"

#define PEDN_PPO_TILE 32          // rows per workgroup
#define PEDN_PPO_WAVE_ROWS 8      // rows per wave

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

// One layer for the wave's 8 rows: acc[r] = b[o]; acc[r] = acc[r] + w[o][k] * x[r][k], k = 0 .. K - 1.  Rows [0, n0) come from w0 / b0,
// rows [n0, rows) from w1 / b1.  first: x is gathered from the clamped time rows of obs (sXc, rows of PEDN_ACTOR_CHUNK; sT / sE hold the
// tile's t and e, -1 behind the last row); otherwise x is sH (rows of 64).  The arithmetic is actor_layer's.
__device__ __forceinline__ void ppo_layer(const PpoEvalArgs& a, float (&acc)[PEDN_PPO_WAVE_ROWS], const float* w0, const float* b0,
                                          const float* w1, const float* b1, int n0, int rows, int K, bool first, int obs0, float* sW,
                                          float* sXc, const float* sH, const int32_t* sT, const int32_t* sE) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const float bias = lane < rows ? (lane < n0 ? b0[lane] : b1[lane - n0]) : 0.0f;
#pragma unroll
  for (int r = 0; r < PEDN_PPO_WAVE_ROWS; ++r) acc[r] = bias;
  for (int c0 = 0; c0 < K; c0 += PEDN_ACTOR_CHUNK) {
    const int kmax = K - c0 < PEDN_ACTOR_CHUNK ? K - c0 : PEDN_ACTOR_CHUNK;
    __syncthreads();   // the chunk before has been consumed (and sH of the layer before, sT and sE are written)
    for (int idx = (int)threadIdx.x; idx < rows * PEDN_ACTOR_CHUNK; idx += 256) {
      const int o = idx / PEDN_ACTOR_CHUNK, kk = idx % PEDN_ACTOR_CHUNK;
      if (kk < kmax) sW[o * (PEDN_ACTOR_CHUNK + 1) + kk] = (o < n0 ? w0 + (size_t)o * K : w1 + (size_t)(o - n0) * K)[c0 + kk];
    }
    if (first) {
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
    }
    __syncthreads();
    if (lane < rows) {
      const float* wr = sW + lane * (PEDN_ACTOR_CHUNK + 1);
      const float* xr = first ? sXc + wave * PEDN_PPO_WAVE_ROWS * PEDN_ACTOR_CHUNK : sH + wave * PEDN_PPO_WAVE_ROWS * PEDN_ACTOR_HIDDEN + c0;
      const int xs = first ? PEDN_ACTOR_CHUNK : PEDN_ACTOR_HIDDEN;
      int kk = 0;
      for (; kk + 4 <= kmax; kk += 4) {
        const float wa = wr[kk], wb = wr[kk + 1], wc = wr[kk + 2], wd = wr[kk + 3];
#pragma unroll
        for (int r = 0; r < PEDN_PPO_WAVE_ROWS; ++r) {
          const float4 x = *reinterpret_cast<const float4*>(xr + r * xs + kk);   // (one address for the wave: a broadcast)
          acc[r] = acc[r] + wa * x.x;
          acc[r] = acc[r] + wb * x.y;
          acc[r] = acc[r] + wc * x.z;
          acc[r] = acc[r] + wd * x.w;
        }
      }
      for (; kk < kmax; ++kk) {
        const float w = wr[kk];
#pragma unroll
        for (int r = 0; r < PEDN_PPO_WAVE_ROWS; ++r) acc[r] = acc[r] + w * xr[r * xs + kk];
      }
    }
  }
}

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
  const int K1 = a.S * obs_w;
  if (threadIdx.x < PEDN_PPO_TILE) {
    const int64_t r = row0 + (int64_t)threadIdx.x;
    const int64_t tr = r / (int64_t)a.N;
    sT[threadIdx.x] = r < n_rows ? (int32_t)tr : -1;
    sE[threadIdx.x] = (int32_t)(r - tr * (int64_t)a.N);
  }
  // the network's tensors, in the order of its pack: both start with encoder.fc1, encoder.fc2 and fc
  const float* w1 = is_actor ? a.actor + t[4] : a.value + a.vtable[agent];
  const float* b1 = w1 + (size_t)H * K1;
  const float* w2 = b1 + H;
  const float* b2 = w2 + H * H;
  const float* w3 = b2 + H;
  const float* b3 = w3 + H * H;
  const float* rest = b3 + H;   // the actor: ln weight, ln bias, fc_mu, fc_std; the value network: value_head
  float* hrow = sH + wave * PEDN_PPO_WAVE_ROWS * H + lane;   // + r * H: this lane's neuron of the wave's row r

  float acc[PEDN_PPO_WAVE_ROWS];
  ppo_layer(a, acc, w1, b1, w1, b1, H, H, K1, true, obs0, sW, sXc, sH, sT, sE);
#pragma unroll
  for (int r = 0; r < PEDN_PPO_WAVE_ROWS; ++r) hrow[r * H] = acc[r] < 0.0f ? 0.0f : acc[r];
  ppo_layer(a, acc, w2, b2, w2, b2, H, H, H, false, obs0, sW, sXc, sH, sT, sE);
#pragma unroll
  for (int r = 0; r < PEDN_PPO_WAVE_ROWS; ++r) hrow[r * H] = acc[r] < 0.0f ? 0.0f : acc[r];
  ppo_layer(a, acc, w3, b3, w3, b3, H, H, H, false, obs0, sW, sXc, sH, sT, sE);
  if (is_actor) {   // LayerNorm(64), float32: actor_forward_kernel's
    const float g = rest[lane], b = rest[H + lane];
#pragma unroll
    for (int r = 0; r < PEDN_PPO_WAVE_ROWS; ++r) {
      const float mean = actor_tree_sum(acc[r]) / 64.0f;
      const float c = acc[r] - mean;
      const float var = actor_tree_sum(c * c) / 64.0f;
      acc[r] = c / sqrtf(var + 1e-5f) * g + b;
    }
  }
#pragma unroll
  for (int r = 0; r < PEDN_PPO_WAVE_ROWS; ++r) hrow[r * H] = acc[r] < 0.0f ? 0.0f : acc[r];
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
  const float* wmu = rest + 2 * H;
  const float* bmu = wmu + act_w * H;
  const float* wsd = bmu + act_w;
  const float* bsd = wsd + act_w * H;
  ppo_layer(a, acc, wmu, bmu, wsd, bsd, act_w, 2 * act_w, H, false, obs0, sW, sXc, sH, sT, sE);
  // rows [0, act_w): mu, rows [act_w, 2 act_w): the pre-softplus value; handed over to a lane per (row, action)
  float* so = sOut + wave * PEDN_PPO_WAVE_ROWS * 2 * PEDN_ACTOR_MAX_ACT;
  if (lane < 2 * act_w) {
    const int col = lane < act_w ? lane : PEDN_ACTOR_MAX_ACT + lane - act_w;
#pragma unroll
    for (int r = 0; r < PEDN_PPO_WAVE_ROWS; ++r) so[r * 2 * PEDN_ACTOR_MAX_ACT + col] = acc[r];
  }
  __syncthreads();
  const int lr = lane / act_w, j = lane - lr * act_w;
  const int64_t row = row0 + (int64_t)(wave * PEDN_PPO_WAVE_ROWS + lr);
  if (lr < PEDN_PPO_WAVE_ROWS && row < n_rows) {
    const float mu = so[lr * 2 * PEDN_ACTOR_MAX_ACT + j], z = so[lr * 2 * PEDN_ACTOR_MAX_ACT + PEDN_ACTOR_MAX_ACT + j];
    const size_t at = (size_t)row * (size_t)a.n_actions + (size_t)(act0 + j);
    float sd = z > 20.0f ? z : (float)log1p(exp((double)z));
    sd = actor_clip(sd, a.min_std, a.max_std);
    const float act = a.act_f64 ? (float)static_cast<const double*>(a.actions)[at] : static_cast<const float*>(a.actions)[at];
    // torch's Normal(mu, std).log_prob(act), in double from the float32 values, rounded once
    const double A = (double)act, M = (double)mu, Sd = (double)sd;
    a.logp[at] = (float)(-((A - M) * (A - M)) / (2.0 * (Sd * Sd)) - log(Sd) - 0.91893853320467267);
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
