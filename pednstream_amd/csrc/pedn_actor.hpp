// The reference's stacked actors (rl/agents/SAC.py:72-107 PolicyNetContinuous, rl/agents/PPO_org.py:145-172 StackedPolicyNetwork, and the
// take_action of both agents with the delta-action lines of their training loops) for every (env, agent) pair in ONE launch.  The
// contract is DESIGN section 14; tests/actor_model.py restates it in numpy.
//
// actor_forward_kernel   grid (ceil(n_envs / PEDN_ACTOR_TILE), n_agents), 256 threads.  A workgroup evaluates one agent for a tile of 32
//                        envs: 4 waves, 8 envs each, a lane per neuron, layer by layer with pedn_mlp.hpp's mlp_layer (mlp_trunk, then
//                        mlp_heads: the two heads are one layer of 2 * act_w rows).  The first layer's inputs are the kernel's gather:
//                        input i = f * S + s is stack[e][s][obs0 + f].  The double-precision tail (softplus, the Box-Muller draw, tanh)
//                        runs with a lane per (env, action) of the wave.  The last workgroup to finish advances the draw counter
//                        (ticket counter, vector atomics), when the launch drew noise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_mlp.hpp"

struct ActorArgs {
  const float* stack;      // [n_envs][S][n_obs]
  const int32_t* table;    // [n_agents][PEDN_ACTOR_TABLE_COLS]
  const float *low, *high; // [n_actions]
  const float* params;     // every agent's tensors, nn.Linear layout
  const float* noise;      // [n_envs][n_actions] (mode 1)
  float *mu, *std, *eps, *raw;   // [n_envs][n_actions]
  double* actions;         // [n_envs][n_actions]
  int64_t* state;          // 0 draw counter, 1 ticket (its low 32 bits)
  uint32_t k0, k1;         // key(seed)
  uint32_t replica_offset;
  int32_t n_envs, S, n_obs, n_actions;
  int32_t kind;            // 0 SAC, 1 PPO
  int32_t delta;           // delta actions
  int32_t mode;            // 0 draw the noise, 1 the caller's noise, 2 deterministic
  float max_delta, min_std, max_std;
};

__device__ __forceinline__ float actor_clip(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }   // (NaN stays)

__global__ __launch_bounds__(256) void actor_forward_kernel(ActorArgs a) {
  __shared__ float sW[PEDN_ACTOR_HIDDEN * (PEDN_ACTOR_CHUNK + 1)];
  __shared__ __attribute__((aligned(16))) float sXc[PEDN_ACTOR_TILE * PEDN_ACTOR_CHUNK];
  __shared__ __attribute__((aligned(16))) float sH[PEDN_ACTOR_TILE * PEDN_ACTOR_HIDDEN];
  __shared__ float sOut[PEDN_ACTOR_TILE * 2 * PEDN_ACTOR_MAX_ACT];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int32_t* t = a.table + (size_t)blockIdx.y * PEDN_ACTOR_TABLE_COLS;
  const int obs0 = t[0], obs_w = t[1], act0 = t[2], act_w = t[3];
  const unsigned env0 = blockIdx.x * PEDN_ACTOR_TILE;
  const int64_t d = a.state[0];
  // input i = f * S + s of the tile's env e is stack[env0 + e][s][obs0 + f]; dead envs read zeros
  const auto gather = [&](int c0, int kmax) {
    for (int idx = (int)threadIdx.x; idx < PEDN_ACTOR_TILE * PEDN_ACTOR_CHUNK; idx += 256) {
      const unsigned e = (unsigned)idx / PEDN_ACTOR_CHUNK, kk = (unsigned)idx % PEDN_ACTOR_CHUNK;
      float x = 0.0f;
      if ((int)kk < kmax && env0 + e < (unsigned)a.n_envs) {
        const unsigned k = (unsigned)c0 + kk, f = k / (unsigned)a.S, s = k - f * (unsigned)a.S;
        x = a.stack[((size_t)(env0 + e) * a.S + s) * a.n_obs + obs0 + f];
      }
      sXc[idx] = x;
    }
  };
  float acc[PEDN_ACTOR_WAVE_ENVS];
  const float* heads = mlp_trunk(acc, a.params + t[4], a.S * obs_w, a.kind != 0, sW, sXc, sH, gather);   // (LayerNorm: the PPO kind)
  const float* so = mlp_heads(acc, heads, act_w, sW, sXc, sH, sOut, gather);
  const int le = lane / act_w, j = lane - le * act_w;
  const unsigned env = env0 + (unsigned)(wave * PEDN_ACTOR_WAVE_ENVS + le);
  if (le < PEDN_ACTOR_WAVE_ENVS && env < (unsigned)a.n_envs) {
    const float mu = so[le * 2 * PEDN_ACTOR_MAX_ACT + j], z = so[le * 2 * PEDN_ACTOR_MAX_ACT + PEDN_ACTOR_MAX_ACT + j];
    const int col = act0 + j;
    const size_t at = (size_t)env * a.n_actions + col;
    float sd = mlp_softplus(z);
    if (a.kind) sd = actor_clip(sd, a.min_std, a.max_std);
    float eps = 0.0f;
    if (a.mode == 0)
      eps = philox_normal(a.k0, a.k1, a.replica_offset + env, d, 0x72u | ((uint32_t)col << 8));
    else if (a.mode == 1)
      eps = a.noise[at];
    const float u = a.mode == 2 ? mu : mu + sd * eps;
    const float lo = a.low[col], hi = a.high[col];
    float raw;
    if (a.kind == 0)
      raw = (float)tanh((double)u) * a.max_delta;
    else
      raw = a.delta ? actor_clip(u, -a.max_delta, a.max_delta) : actor_clip(u, lo, hi);
    double act = (double)raw;
    if (a.delta) {
      // the reference's obs.reshape(act_dim, -1)[:, -1] of the newest frame
      const float width = a.stack[((size_t)env * a.S + (a.S - 1)) * a.n_obs + obs0 + (j + 1) * (obs_w / act_w) - 1];
      act = (double)actor_clip(width + raw, lo, hi);
    }
    a.mu[at] = mu; a.std[at] = sd; a.eps[at] = eps; a.raw[at] = raw;
    a.actions[at] = act;
  }
  if (a.mode != 0) return;
  __syncthreads();   // (the workgroup has read the draw counter)
  if (threadIdx.x == 0) advance_draw_counter(a.state, d);
}

// ---- host side: pedn_actor_forward of include/pedn.h; no state in the engine's handle
int pedn_actor_forward(const float* stack, const int32_t* table, const float* low, const float* high, const float* params,
                       const float* noise, float* mu, float* std, float* eps, float* raw, double* actions, int64_t* state,
                       int32_t n_envs, int32_t stack_size, int32_t n_obs, int32_t n_actions, int32_t n_agents, int32_t hidden_size,
                       int32_t kind, int32_t delta_actions, int32_t mode, double max_delta, double min_std, double max_std, uint64_t seed,
                       uint32_t replica_offset, void* stream) {
  if (!stack || !table || !low || !high || !params || !mu || !std || !eps || !raw || !actions || !state)
    return fail(nullptr, PEDN_E_ARG, "null argument");
  if (hidden_size != PEDN_ACTOR_HIDDEN) return fail(nullptr, PEDN_E_ARG, "the actor kernel is built for hidden_size 64");
  if (n_envs < 1 || stack_size < 1 || n_obs < 1 || n_actions < 1 || n_agents < 1 || n_agents > 65535)
    return fail(nullptr, PEDN_E_ARG, "n_envs, stack_size, n_obs, n_actions and n_agents must be positive (at most 65535 agents)");
  if (kind < 0 || kind > 1 || mode < 0 || mode > 2) return fail(nullptr, PEDN_E_ARG, "kind is 0 (SAC) or 1 (PPO), mode 0, 1 or 2");
  if (mode == 1 && !noise) return fail(nullptr, PEDN_E_ARG, "mode 1 needs the noise");
  ActorArgs a{};
  a.stack = stack; a.table = table; a.low = low; a.high = high; a.params = params; a.noise = noise;
  a.mu = mu; a.std = std; a.eps = eps; a.raw = raw; a.actions = actions; a.state = state;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
  a.replica_offset = replica_offset;
  a.n_envs = n_envs; a.S = stack_size; a.n_obs = n_obs; a.n_actions = n_actions;
  a.kind = kind; a.delta = delta_actions != 0; a.mode = mode;
  a.max_delta = (float)max_delta; a.min_std = (float)min_std; a.max_std = (float)max_std;
  const dim3 grid((unsigned)((n_envs + PEDN_ACTOR_TILE - 1) / PEDN_ACTOR_TILE), (unsigned)n_agents);
  hipLaunchKernelGGL(actor_forward_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}
