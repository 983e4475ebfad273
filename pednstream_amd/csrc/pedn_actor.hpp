// The reference's stacked actors (rl/agents/SAC.py:72-107 PolicyNetContinuous, rl/agents/PPO_org.py:145-172 StackedPolicyNetwork, and the
// take_action of both agents with the delta-action lines of their training loops) for every (env, agent) pair in ONE launch.  The
// contract is DESIGN section 14; tests/actor_model.py restates it in numpy.
//
// actor_forward_kernel   grid (ceil(n_envs / PEDN_ACTOR_TILE), n_agents), 256 threads.  A workgroup evaluates one agent for a tile of 32
//                        envs: 4 waves, 8 envs each, a lane per neuron.  Every layer runs over chunks of 32 inputs: the workgroup copies
//                        the chunk of the weight rows (nn.Linear's [out][in], read with 128-byte row pieces) into LDS rows of 33 words,
//                        and for the first layer the chunk of the inputs too (input i = f * S + s is stack[e][s][obs0 + f]); then lane o
//                        reads its weight w[o][k] once per k (conflict-free: 33 is odd) and the 8 inputs of that k as broadcasts, and does
//                        acc[e] = acc[e] + w * x[e][k], k ascending, one accumulator per (env, neuron): the order depends on nothing but
//                        the layer's shape.  Hidden activations stay in LDS rows of 64 that only the env's own wave touches.  The two
//                        heads are one layer of 2 * act_w rows; the double-precision tail (softplus, the Box-Muller draw, tanh) runs
//                        with a lane per (env, action) of the wave.  The last workgroup to finish advances the draw counter (ticket
//                        counter, vector atomics), when the launch drew noise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_math.hpp"

#define PEDN_ACTOR_HIDDEN 64      // hidden_size of every layer (the reference's default; nothing else is built)
#define PEDN_ACTOR_TILE 32        // envs per workgroup
#define PEDN_ACTOR_WAVE_ENVS 8    // envs per wave
#define PEDN_ACTOR_CHUNK 32       // inputs per staged chunk
#define PEDN_ACTOR_MAX_ACT 8      // act_w of an agent
#define PEDN_ACTOR_TABLE_COLS 6   // obs0, obs_w, act0, act_w, parameter offset (floats), reserved

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

// One layer for the wave's 8 envs: acc[e] = b[o]; acc[e] = acc[e] + w[o][k] * x[e][k], k = 0 .. K - 1.  Rows [0, n0) come from w0 / b0,
// rows [n0, rows) from w1 / b1.  first: x is gathered from the stack (sXc, rows of PEDN_ACTOR_CHUNK); otherwise x is sH (rows of 64).
__device__ __forceinline__ void actor_layer(const ActorArgs& a, float (&acc)[PEDN_ACTOR_WAVE_ENVS], const float* w0, const float* b0,
                                            const float* w1, const float* b1, int n0, int rows, int K, bool first, int obs0, unsigned env0,
                                            float* sW, float* sXc, const float* sH) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const float bias = lane < rows ? (lane < n0 ? b0[lane] : b1[lane - n0]) : 0.0f;
#pragma unroll
  for (int e = 0; e < PEDN_ACTOR_WAVE_ENVS; ++e) acc[e] = bias;
  for (int c0 = 0; c0 < K; c0 += PEDN_ACTOR_CHUNK) {
    const int kmax = K - c0 < PEDN_ACTOR_CHUNK ? K - c0 : PEDN_ACTOR_CHUNK;
    __syncthreads();   // the chunk before has been consumed (and sH of the layer before is written)
    for (int idx = (int)threadIdx.x; idx < rows * PEDN_ACTOR_CHUNK; idx += 256) {
      const int o = idx / PEDN_ACTOR_CHUNK, kk = idx % PEDN_ACTOR_CHUNK;
      if (kk < kmax) sW[o * (PEDN_ACTOR_CHUNK + 1) + kk] = (o < n0 ? w0 + (size_t)o * K : w1 + (size_t)(o - n0) * K)[c0 + kk];
    }
    if (first) {
      for (int idx = (int)threadIdx.x; idx < PEDN_ACTOR_TILE * PEDN_ACTOR_CHUNK; idx += 256) {
        const unsigned e = (unsigned)idx / PEDN_ACTOR_CHUNK, kk = (unsigned)idx % PEDN_ACTOR_CHUNK;
        float x = 0.0f;
        if ((int)kk < kmax && env0 + e < (unsigned)a.n_envs) {
          const unsigned k = (unsigned)c0 + kk, f = k / (unsigned)a.S, s = k - f * (unsigned)a.S;
          x = a.stack[((size_t)(env0 + e) * a.S + s) * a.n_obs + obs0 + f];
        }
        sXc[idx] = x;
      }
    }
    __syncthreads();
    if (lane < rows) {
      const float* wr = sW + lane * (PEDN_ACTOR_CHUNK + 1);
      const float* xr = first ? sXc + wave * PEDN_ACTOR_WAVE_ENVS * PEDN_ACTOR_CHUNK : sH + wave * PEDN_ACTOR_WAVE_ENVS * PEDN_ACTOR_HIDDEN + c0;
      const int xs = first ? PEDN_ACTOR_CHUNK : PEDN_ACTOR_HIDDEN;
      int kk = 0;
      for (; kk + 4 <= kmax; kk += 4) {
        const float wa = wr[kk], wb = wr[kk + 1], wc = wr[kk + 2], wd = wr[kk + 3];
#pragma unroll
        for (int e = 0; e < PEDN_ACTOR_WAVE_ENVS; ++e) {
          const float4 x = *reinterpret_cast<const float4*>(xr + e * xs + kk);   // (one address for the wave: a broadcast)
          acc[e] = acc[e] + wa * x.x;
          acc[e] = acc[e] + wb * x.y;
          acc[e] = acc[e] + wc * x.z;
          acc[e] = acc[e] + wd * x.w;
        }
      }
      for (; kk < kmax; ++kk) {
        const float w = wr[kk];
#pragma unroll
        for (int e = 0; e < PEDN_ACTOR_WAVE_ENVS; ++e) acc[e] = acc[e] + w * xr[e * xs + kk];
      }
    }
  }
}

// sum of the wave's 64 values as a balanced tree: level m adds the partner 2^m lanes away.  Both partners add the same two numbers, so
// every lane holds the same bits at every level.
__device__ __forceinline__ float actor_tree_sum(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(256) void actor_forward_kernel(ActorArgs a) {
  __shared__ float sW[PEDN_ACTOR_HIDDEN * (PEDN_ACTOR_CHUNK + 1)];
  __shared__ __attribute__((aligned(16))) float sXc[PEDN_ACTOR_TILE * PEDN_ACTOR_CHUNK];
  __shared__ __attribute__((aligned(16))) float sH[PEDN_ACTOR_TILE * PEDN_ACTOR_HIDDEN];
  __shared__ float sOut[PEDN_ACTOR_TILE * 2 * PEDN_ACTOR_MAX_ACT];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int H = PEDN_ACTOR_HIDDEN;
  const int32_t* t = a.table + (size_t)blockIdx.y * PEDN_ACTOR_TABLE_COLS;
  const int obs0 = t[0], obs_w = t[1], act0 = t[2], act_w = t[3];
  const int K1 = a.S * obs_w;
  const unsigned env0 = blockIdx.x * PEDN_ACTOR_TILE;
  const int64_t d = a.state[0];
  // the agent's tensors, in the order of the pack
  const float* w1 = a.params + t[4];
  const float* b1 = w1 + (size_t)H * K1;
  const float* w2 = b1 + H;
  const float* b2 = w2 + H * H;
  const float* w3 = b2 + H;
  const float* b3 = w3 + H * H;
  const float* ln_g = b3 + H;
  const float* wmu = a.kind ? ln_g + 2 * H : ln_g;
  const float* bmu = wmu + act_w * H;
  const float* wsd = bmu + act_w;
  const float* bsd = wsd + act_w * H;
  float* hrow = sH + wave * PEDN_ACTOR_WAVE_ENVS * H + lane;   // + e * H: this lane's neuron of the wave's env e

  float acc[PEDN_ACTOR_WAVE_ENVS];
  actor_layer(a, acc, w1, b1, w1, b1, H, H, K1, true, obs0, env0, sW, sXc, sH);
#pragma unroll
  for (int e = 0; e < PEDN_ACTOR_WAVE_ENVS; ++e) hrow[e * H] = acc[e] < 0.0f ? 0.0f : acc[e];
  actor_layer(a, acc, w2, b2, w2, b2, H, H, H, false, obs0, env0, sW, sXc, sH);
#pragma unroll
  for (int e = 0; e < PEDN_ACTOR_WAVE_ENVS; ++e) hrow[e * H] = acc[e] < 0.0f ? 0.0f : acc[e];
  actor_layer(a, acc, w3, b3, w3, b3, H, H, H, false, obs0, env0, sW, sXc, sH);
  if (a.kind) {   // LayerNorm(64) of the PPO kind, float32
    const float g = ln_g[lane], b = ln_g[H + lane];
#pragma unroll
    for (int e = 0; e < PEDN_ACTOR_WAVE_ENVS; ++e) {
      const float mean = actor_tree_sum(acc[e]) / 64.0f;
      const float c = acc[e] - mean;
      const float var = actor_tree_sum(c * c) / 64.0f;
      acc[e] = c / sqrtf(var + 1e-5f) * g + b;
    }
  }
#pragma unroll
  for (int e = 0; e < PEDN_ACTOR_WAVE_ENVS; ++e) hrow[e * H] = acc[e] < 0.0f ? 0.0f : acc[e];
  actor_layer(a, acc, wmu, bmu, wsd, bsd, act_w, 2 * act_w, H, false, obs0, env0, sW, sXc, sH);
  // rows [0, act_w): mu, rows [act_w, 2 act_w): the pre-softplus value; handed over to a lane per (env, action)
  float* so = sOut + wave * PEDN_ACTOR_WAVE_ENVS * 2 * PEDN_ACTOR_MAX_ACT;
  if (lane < 2 * act_w) {
    const int col = lane < act_w ? lane : PEDN_ACTOR_MAX_ACT + lane - act_w;
#pragma unroll
    for (int e = 0; e < PEDN_ACTOR_WAVE_ENVS; ++e) so[e * 2 * PEDN_ACTOR_MAX_ACT + col] = acc[e];
  }
  __syncthreads();
  const int le = lane / act_w, j = lane - le * act_w;
  const unsigned env = env0 + (unsigned)(wave * PEDN_ACTOR_WAVE_ENVS + le);
  if (le < PEDN_ACTOR_WAVE_ENVS && env < (unsigned)a.n_envs) {
    const float mu = so[le * 2 * PEDN_ACTOR_MAX_ACT + j], z = so[le * 2 * PEDN_ACTOR_MAX_ACT + PEDN_ACTOR_MAX_ACT + j];
    const int col = act0 + j;
    const size_t at = (size_t)env * a.n_actions + col;
    float sd = z > 20.0f ? z : (float)log1p(exp((double)z));
    if (a.kind) sd = actor_clip(sd, a.min_std, a.max_std);
    float eps = 0.0f;
    if (a.mode == 0) {
      uint32_t w[4] = {a.replica_offset + env, (uint32_t)d, 0x72u | ((uint32_t)col << 8), (uint32_t)((uint64_t)d >> 32)};
      philox4x32_10(w, a.k0, a.k1);
      const double u1 = ((double)w[0] + 1.0) * 0x1p-32, u2 = (double)w[1] * 0x1p-32;
      eps = (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
    } else if (a.mode == 1)
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
  if (threadIdx.x == 0) {
    unsigned* ticket = reinterpret_cast<unsigned*>(a.state + 1);
    const unsigned mine = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (mine + 1u == gridDim.x * gridDim.y) {
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.state, d + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
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
