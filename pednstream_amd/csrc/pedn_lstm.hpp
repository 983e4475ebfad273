// The reference's stateful LSTM PPO agents (rl/agents/PPO_org.py:20-138 LSTMPolicyNetwork / LSTMValueNetwork, :470-516 take_action,
// :543-577 the gradient-free half of update) for every env and agent.  The contract is DESIGN section 17; tests/lstm_model.py restates it
// in numpy.  One nn.LSTM layer of 64 units, gate rows i, f, g, o; everything the stacked kernels also compute is pedn_mlp.hpp's.
//
// lstm_actor_kernel   grid (ceil(n_envs / 32), n_agents), 256 threads.  A workgroup steps one agent's LSTM for a tile of 32 envs: 4 waves,
//                     8 envs each, a lane per hidden unit that carries the unit's four gate accumulators of its 8 rows (lstm_gates), so
//                     the cell update needs no exchange between lanes.  h is staged into LDS and c into registers before anything is
//                     written back: lane j of a row's wave is the only reader and the only writer of unit j of (agent, env) in hc.
//                     Then mlp_heads on relu(h') and section 14's PPO tail on a lane per (env, action).
//                     LDS: 256 * 33 + 32 * 32 + 2 * 32 * 64 + 32 * 16 words = 56320 bytes, 2 workgroups per CU by LDS (160 KB).
// lstm_reset_kernel   zeroes h and c of the masked envs (mask NULL: all) of every agent, 16 bytes a thread.
// lstm_seq_kernel     grid (ceil(N / 32), n_agents, 3), 256 threads.  blockIdx.z is the role: 0 the value LSTM over obs[0 .. T - 1],
//                     1 the value LSTM over obs[1 .. T], 2 the actor LSTM over obs[0 .. T - 1] with Normal.log_prob of actions[t].
//                     Every role starts from a zero state and walks t inside the kernel with lstm_actor_kernel's step: c stays in
//                     registers, h in LDS; the weight chunks are staged again every step (from L2: a network is 4 * 64 *
//                     (obs_w + 64 + 2) floats).  Same LDS, so 2 waves per SIMD: both kernels declare that and with it a budget of 256 VGPRs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_actor.hpp"
#include "pedn_mlp.hpp"

#define PEDN_LSTM_GATES 4
#define PEDN_LSTM_ROWS (PEDN_LSTM_GATES * PEDN_ACTOR_HIDDEN)   // gate rows of weight_ih_l0 / weight_hh_l0
#define PEDN_LSTM_NOISE_SITE 0x74u                             // (0x72: the stacked actors, 0x73: the SAC targets)

// 1 / (1 + exp(-z)) in double from the float32 value, rounded once
__device__ __forceinline__ float lstm_sigmoid(float z) { return (float)(1.0 / (1.0 + pedn_exp(-(double)z))); }

// tanh in double from the float32 value, rounded once: (1 - e) / (1 + e) with e = exp(-2 |z|); below 2^-13 that quotient cancels, and
// the series' first two terms are exact to double there
__device__ __forceinline__ float lstm_tanh(float z) {
  const double a = fabs((double)z);
  double t;
  if (a < 0x1p-13)
    t = a - a * a * a / 3.0;
  else {
    const double e = pedn_exp(-2.0 * a);
    t = (1.0 - e) / (1.0 + e);
  }
  return (float)copysign(t, (double)z);
}

// value_head on relu(h) of one row: v = b; v = v + w[k] * h[k], k ascending (w: weight [64], then the bias)
__device__ __forceinline__ float lstm_value_head(const float* w, const float* h) {
  float v = w[PEDN_ACTOR_HIDDEN];
  for (int k = 0; k < PEDN_ACTOR_HIDDEN; ++k) v = v + w[k] * h[k];
  return v;
}

// bias[g] = bias_ih[o] + bias_hh[o] of this lane's gate rows o = g * 64 + lane (one float32 add; the same every step).  p: the
// network's lstm.* tensors: weight_ih [256][K], weight_hh [256][64], bias_ih [256], bias_hh [256].
__device__ __forceinline__ void lstm_bias(float (&bias)[PEDN_LSTM_GATES], const float* p, int K) {
  const int lane = (int)(threadIdx.x & 63);
  const float* bih = p + (size_t)PEDN_LSTM_ROWS * (K + PEDN_ACTOR_HIDDEN);
#pragma unroll
  for (int g = 0; g < PEDN_LSTM_GATES; ++g) bias[g] = bih[g * PEDN_ACTOR_HIDDEN + lane] + bih[PEDN_LSTM_ROWS + g * PEDN_ACTOR_HIDDEN + lane];
}

// The four gate pre-activations of this lane's unit for the wave's 8 rows: acc[g][r] = bias[g]; then + W_ih[o][k] * x[k] and
// + W_hh[o][k] * h[k], k ascending each, into the one accumulator (mlp_mac).  The workgroup copies a chunk of 32 inputs of the 256 rows
// into LDS rows of 33 words; gather(c0, kmax) fills sXc with inputs [c0, c0 + kmax) of the tile's rows; sHs holds the rows' h.
template <class Gather>
__device__ __forceinline__ void lstm_gates(float (&acc)[PEDN_LSTM_GATES][PEDN_ACTOR_WAVE_ENVS], const float (&bias)[PEDN_LSTM_GATES],
                                           const float* p, int K, float* sW, const float* sXc, const float* sHs, Gather gather) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int H = PEDN_ACTOR_HIDDEN;
  const float* wih = p;
  const float* whh = wih + (size_t)PEDN_LSTM_ROWS * K;
#pragma unroll
  for (int g = 0; g < PEDN_LSTM_GATES; ++g)
#pragma unroll
    for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) acc[g][r] = bias[g];
  // chunk ci < nx covers inputs [32 ci, ..) of x, the two behind them the halves of h
  const int nx = (K + PEDN_ACTOR_CHUNK - 1) / PEDN_ACTOR_CHUNK;
  for (int ci = 0; ci < nx + H / PEDN_ACTOR_CHUNK; ++ci) {
    const bool is_x = ci < nx;
    const int k0 = (is_x ? ci : ci - nx) * PEDN_ACTOR_CHUNK, kin = is_x ? K : H;
    const int kmax = kin - k0 < PEDN_ACTOR_CHUNK ? kin - k0 : PEDN_ACTOR_CHUNK;
    const float* w = is_x ? wih : whh;
    __syncthreads();   // the chunk before has been consumed (and what the caller wrote to LDS for this step is there)
    for (int idx = (int)threadIdx.x; idx < PEDN_LSTM_ROWS * PEDN_ACTOR_CHUNK; idx += 256) {
      const int o = idx / PEDN_ACTOR_CHUNK, kk = idx % PEDN_ACTOR_CHUNK;
      if (kk < kmax) sW[o * (PEDN_ACTOR_CHUNK + 1) + kk] = w[(size_t)o * kin + k0 + kk];
    }
    if (is_x) gather(k0, kmax);
    __syncthreads();
    const float* xr = is_x ? sXc + wave * PEDN_ACTOR_WAVE_ENVS * PEDN_ACTOR_CHUNK : sHs + wave * PEDN_ACTOR_WAVE_ENVS * H + k0;
    const int xs = is_x ? PEDN_ACTOR_CHUNK : H;
#pragma unroll
    for (int g = 0; g < PEDN_LSTM_GATES; ++g) mlp_mac(acc[g], sW + (g * H + lane) * (PEDN_ACTOR_CHUNK + 1), xr, xs, kmax);
  }
}

// c' = f * c + i * g, h' = o * tanh(c') of this lane's unit in the wave's rows.  c is updated in place, h' goes to hs (the state row in
// LDS, only the row's own wave touches it) and relu(h') to hr (what the heads read).  keep(r, i, f, g, o, c', h') is handed row r's
// activated gates and new state: the update's forward stores them (pedn_lstm_grad.hpp).
template <class Keep>
__device__ __forceinline__ void lstm_cell_keep(const float (&acc)[PEDN_LSTM_GATES][PEDN_ACTOR_WAVE_ENVS], float (&c)[PEDN_ACTOR_WAVE_ENVS],
                                               float* hs, float* hr, Keep keep) {
#pragma unroll
  for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) {
    const float i = lstm_sigmoid(acc[0][r]), f = lstm_sigmoid(acc[1][r]), g = lstm_tanh(acc[2][r]), o = lstm_sigmoid(acc[3][r]);
    const float fc = f * c[r], ig = i * g;
    c[r] = fc + ig;
    const float h = o * lstm_tanh(c[r]);
    hs[r * PEDN_ACTOR_HIDDEN] = h;
    hr[r * PEDN_ACTOR_HIDDEN] = h < 0.0f ? 0.0f : h;
    keep(r, i, f, g, o, c[r], h);
  }
}

__device__ __forceinline__ void lstm_cell(const float (&acc)[PEDN_LSTM_GATES][PEDN_ACTOR_WAVE_ENVS], float (&c)[PEDN_ACTOR_WAVE_ENVS],
                                          float* hs, float* hr) {
  lstm_cell_keep(acc, c, hs, hr, [](int, float, float, float, float, float, float) {});
}

struct LstmActorArgs {
  const float* obs;        // [n_envs][n_obs]
  const int32_t* table;    // [n_agents][PEDN_ACTOR_TABLE_COLS]
  const float *low, *high; // [n_actions]
  const float* params;     // every agent's lstm.*, mean_head.*, std_head.*
  const float* noise;      // [n_envs][n_actions] (mode 1)
  float* hc;               // [n_agents][n_envs][2][64]: h, then c
  float *mu, *std, *eps, *raw;   // [n_envs][n_actions]
  double* actions;         // [n_envs][n_actions]
  int64_t* state;          // 0 draw counter, 1 ticket (its low 32 bits)
  uint32_t k0, k1;         // key(seed)
  uint32_t replica_offset;
  int32_t n_envs, n_obs, n_actions;
  int32_t delta;           // delta actions
  int32_t mode;            // 0 draw the noise, 1 the caller's noise, 2 deterministic
  float max_delta, min_std, max_std;
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void lstm_actor_kernel(LstmActorArgs a) {
  __shared__ float sW[PEDN_LSTM_ROWS * (PEDN_ACTOR_CHUNK + 1)];
  __shared__ __attribute__((aligned(16))) float sXc[PEDN_ACTOR_TILE * PEDN_ACTOR_CHUNK];
  __shared__ __attribute__((aligned(16))) float sHs[PEDN_ACTOR_TILE * PEDN_ACTOR_HIDDEN];
  __shared__ __attribute__((aligned(16))) float sH[PEDN_ACTOR_TILE * PEDN_ACTOR_HIDDEN];
  __shared__ float sOut[PEDN_ACTOR_TILE * 2 * PEDN_ACTOR_MAX_ACT];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int H = PEDN_ACTOR_HIDDEN;
  const int32_t* t = a.table + (size_t)blockIdx.y * PEDN_ACTOR_TABLE_COLS;
  const int obs0 = t[0], obs_w = t[1], act0 = t[2], act_w = t[3];
  const unsigned env0 = blockIdx.x * PEDN_ACTOR_TILE;
  const int64_t d = a.state[0];
  // input k of the tile's env e is obs[env0 + e][obs0 + k]; dead envs read zeros
  const auto gather = [&](int c0, int kmax) {
    for (int idx = (int)threadIdx.x; idx < PEDN_ACTOR_TILE * PEDN_ACTOR_CHUNK; idx += 256) {
      const unsigned e = (unsigned)idx / PEDN_ACTOR_CHUNK, kk = (unsigned)idx % PEDN_ACTOR_CHUNK;
      float x = 0.0f;
      if ((int)kk < kmax && env0 + e < (unsigned)a.n_envs) x = a.obs[(size_t)(env0 + e) * a.n_obs + obs0 + c0 + (int)kk];
      sXc[idx] = x;
    }
  };
  // this lane's unit of the wave's rows: h into LDS, c into registers, before anything is written back
  float* hc = a.hc + ((size_t)blockIdx.y * a.n_envs + env0 + (unsigned)(wave * PEDN_ACTOR_WAVE_ENVS)) * (2 * H) + lane;
  float* hs = sHs + wave * PEDN_ACTOR_WAVE_ENVS * H + lane;
  float c[PEDN_ACTOR_WAVE_ENVS];
#pragma unroll
  for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) {
    const bool live = env0 + (unsigned)(wave * PEDN_ACTOR_WAVE_ENVS + r) < (unsigned)a.n_envs;
    hs[r * H] = live ? hc[(size_t)r * 2 * H] : 0.0f;
    c[r] = live ? hc[(size_t)r * 2 * H + H] : 0.0f;
  }
  const float* p = a.params + t[4];
  float acc[PEDN_LSTM_GATES][PEDN_ACTOR_WAVE_ENVS], bias[PEDN_LSTM_GATES];
  lstm_bias(bias, p, obs_w);
  lstm_gates(acc, bias, p, obs_w, sW, sXc, sHs, gather);
  lstm_cell(acc, c, hs, sH + wave * PEDN_ACTOR_WAVE_ENVS * H + lane);
#pragma unroll
  for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r)
    if (env0 + (unsigned)(wave * PEDN_ACTOR_WAVE_ENVS + r) < (unsigned)a.n_envs) {
      hc[(size_t)r * 2 * H] = hs[r * H];
      hc[(size_t)r * 2 * H + H] = c[r];
    }
  const float* heads = p + (size_t)PEDN_LSTM_ROWS * (obs_w + H + 2);
  const float* so = mlp_heads(acc[0], heads, act_w, sW, sXc, sH, sOut, gather);
  const int le = lane / act_w, j = lane - le * act_w;
  const unsigned env = env0 + (unsigned)(wave * PEDN_ACTOR_WAVE_ENVS + le);
  if (le < PEDN_ACTOR_WAVE_ENVS && env < (unsigned)a.n_envs) {
    const float mu = so[le * 2 * PEDN_ACTOR_MAX_ACT + j], z = so[le * 2 * PEDN_ACTOR_MAX_ACT + PEDN_ACTOR_MAX_ACT + j];
    const int col = act0 + j;
    const size_t at = (size_t)env * a.n_actions + col;
    const float sd = actor_clip(mlp_softplus(z), a.min_std, a.max_std);
    float eps = 0.0f;
    if (a.mode == 0)
      eps = philox_normal(a.k0, a.k1, a.replica_offset + env, d, PEDN_LSTM_NOISE_SITE | ((uint32_t)col << 8));
    else if (a.mode == 1)
      eps = a.noise[at];
    const float u = a.mode == 2 ? mu : mu + sd * eps;
    const float lo = a.low[col], hi = a.high[col];
    const float raw = a.delta ? actor_clip(u, -a.max_delta, a.max_delta) : actor_clip(u, lo, hi);
    double act = (double)raw;
    if (a.delta) {
      // the reference's obs.reshape(act_dim, -1)[:, -1]
      const float width = a.obs[(size_t)env * a.n_obs + obs0 + (j + 1) * (obs_w / act_w) - 1];
      act = (double)actor_clip(width + raw, lo, hi);
    }
    a.mu[at] = mu; a.std[at] = sd; a.eps[at] = eps; a.raw[at] = raw;
    a.actions[at] = act;
  }
  if (a.mode != 0) return;
  __syncthreads();   // (the workgroup has read the draw counter)
  if (threadIdx.x == 0) advance_draw_counter(a.state, d);
}

// hc as float4 [n_agents][n_envs][32]; mask u8 [n_envs] or null
__global__ __launch_bounds__(256) void lstm_reset_kernel(float4* hc, const uint8_t* mask, int64_t n_envs, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t env = (i / (2 * PEDN_ACTOR_HIDDEN / 4)) % n_envs;
  if (!mask || mask[env]) hc[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

struct LstmSeqArgs {
  const float* obs;        // [T + 1][N][n_obs]
  const void* actions;     // [T][N][n_actions], float or double
  const int32_t* table;    // [n_agents][PEDN_ACTOR_TABLE_COLS]: the actors' table
  const int32_t* vtable;   // [n_agents]: offsets (floats) in the value pack
  const float* actor;      // the actors' pack
  const float* value;      // the value pack
  float *values, *next_values;   // [T][N][n_agents]
  float* logp;             // [T][N][n_actions]
  float *mu, *std;         // [T][N][n_actions] or null
  int32_t T, N, n_obs, n_actions, n_agents;
  int32_t act_f64;
  float min_std, max_std;
};

// One role of lstm_seq_kernel for the workgroup's tile.  ACTOR: the actor's pack, heads and log-probabilities; else the value pack and
// value_head, over the frames from obs row `first` on, into out_v.
template <bool ACTOR>
__device__ __forceinline__ void lstm_seq_role(const LstmSeqArgs& a, int first, float* out_v, float* sW, float* sXc, float* sHs, float* sH,
                                              float* sOut) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int H = PEDN_ACTOR_HIDDEN;
  const int agent = (int)blockIdx.y;
  const int32_t* t = a.table + (size_t)agent * PEDN_ACTOR_TABLE_COLS;
  const int obs0 = t[0], obs_w = t[1], act0 = t[2], act_w = t[3];
  const unsigned env0 = blockIdx.x * PEDN_ACTOR_TILE;
  const size_t frame_words = (size_t)a.N * (size_t)a.n_obs;
  const float* frame = a.obs + (size_t)first * frame_words;   // row 0 of the role's sequence
  // input k of the tile's env e at the step is frame[env0 + e][obs0 + k]; rows behind N read zeros
  const auto gather = [&](int c0, int kmax) {
    for (int idx = (int)threadIdx.x; idx < PEDN_ACTOR_TILE * PEDN_ACTOR_CHUNK; idx += 256) {
      const unsigned e = (unsigned)idx / PEDN_ACTOR_CHUNK, kk = (unsigned)idx % PEDN_ACTOR_CHUNK;
      float x = 0.0f;
      if ((int)kk < kmax && env0 + e < (unsigned)a.N) x = frame[(size_t)(env0 + e) * (size_t)a.n_obs + (size_t)(obs0 + c0 + (int)kk)];
      sXc[idx] = x;
    }
  };
  const float* p = ACTOR ? a.actor + t[4] : a.value + a.vtable[agent];
  const float* rest = p + (size_t)PEDN_LSTM_ROWS * (obs_w + H + 2);   // mean_head (then std_head), or value_head
  float* hs = sHs + wave * PEDN_ACTOR_WAVE_ENVS * H + lane;
  float c[PEDN_ACTOR_WAVE_ENVS];
#pragma unroll
  for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) {
    hs[r * H] = 0.0f;
    c[r] = 0.0f;
  }
  // the tail's lane: (row le of the wave, action j) with the actor, row `lane` with a value network; `at` is its element of the step's
  // row in an output of `cols` columns, and each lane carries its own pointers (they are formed once, not kept per workgroup)
  const int le = ACTOR ? lane / act_w : lane, j = ACTOR ? lane - le * act_w : 0;
  const unsigned env = env0 + (unsigned)(wave * PEDN_ACTOR_WAVE_ENVS + le);
  const bool mine = le < PEDN_ACTOR_WAVE_ENVS && env < (unsigned)a.N;
  const size_t cols = (size_t)(ACTOR ? a.n_actions : a.n_agents), at = (size_t)env * cols + (size_t)(ACTOR ? act0 + j : agent);
  const size_t at_step = (size_t)a.N * cols;
  float* o_v = ACTOR ? nullptr : out_v + at;
  float* o_logp = ACTOR ? a.logp + at : nullptr;
  float* o_mu = ACTOR && a.mu ? a.mu + at : nullptr;
  float* o_std = ACTOR && a.std ? a.std + at : nullptr;
  const size_t act_size = a.act_f64 ? sizeof(double) : sizeof(float);
  const char* i_act = static_cast<const char*>(a.actions) + at * act_size;
  float acc[PEDN_LSTM_GATES][PEDN_ACTOR_WAVE_ENVS], bias[PEDN_LSTM_GATES];
  lstm_bias(bias, p, obs_w);
  for (int step = 0; step < a.T; ++step, frame += frame_words) {
    lstm_gates(acc, bias, p, obs_w, sW, sXc, sHs, gather);
    lstm_cell(acc, c, hs, sH + wave * PEDN_ACTOR_WAVE_ENVS * H + lane);
    if (!ACTOR) {
      __syncthreads();   // (the wave's own rows; the barrier orders the LDS writes before the reads)
      if (mine) *o_v = lstm_value_head(rest, sH + (wave * PEDN_ACTOR_WAVE_ENVS + lane) * H);
      o_v += at_step;
      continue;
    }
    const float* so = mlp_heads(acc[0], rest, act_w, sW, sXc, sH, sOut, gather);
    if (mine) {
      const float mu = so[le * 2 * PEDN_ACTOR_MAX_ACT + j], z = so[le * 2 * PEDN_ACTOR_MAX_ACT + PEDN_ACTOR_MAX_ACT + j];
      const float sd = actor_clip(mlp_softplus(z), a.min_std, a.max_std);
      const float act = a.act_f64 ? (float)*reinterpret_cast<const double*>(i_act) : *reinterpret_cast<const float*>(i_act);
      *o_logp = (float)normal_log_prob(act, mu, sd);   // (rounded once)
      if (o_mu) *o_mu = mu;
      if (o_std) *o_std = sd;
    }
    o_logp += at_step; i_act += at_step * act_size;
    if (o_mu) o_mu += at_step;
    if (o_std) o_std += at_step;
  }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void lstm_seq_kernel(LstmSeqArgs a) {
  __shared__ float sW[PEDN_LSTM_ROWS * (PEDN_ACTOR_CHUNK + 1)];
  __shared__ __attribute__((aligned(16))) float sXc[PEDN_ACTOR_TILE * PEDN_ACTOR_CHUNK];
  __shared__ __attribute__((aligned(16))) float sHs[PEDN_ACTOR_TILE * PEDN_ACTOR_HIDDEN];
  __shared__ __attribute__((aligned(16))) float sH[PEDN_ACTOR_TILE * PEDN_ACTOR_HIDDEN];
  __shared__ float sOut[PEDN_ACTOR_TILE * 2 * PEDN_ACTOR_MAX_ACT];
  if (blockIdx.z == 2)
    lstm_seq_role<true>(a, 0, nullptr, sW, sXc, sHs, sH, sOut);
  else
    lstm_seq_role<false>(a, (int)blockIdx.z, blockIdx.z == 0 ? a.values : a.next_values, sW, sXc, sHs, sH, sOut);
}

// ---- host side: pedn_lstm_* of include/pedn.h; no state in the engine's handle
static const char* lstm_sizes(int32_t n_rows, int32_t n_obs, int32_t n_actions, int32_t n_agents, int32_t hidden_size, int32_t num_layers) {
  if (hidden_size != PEDN_ACTOR_HIDDEN) return "the LSTM kernels are built for hidden_size 64";
  if (num_layers != 1) return "the LSTM kernels are built for one layer";
  if (n_rows < 1 || n_obs < 1 || n_actions < 1 || n_agents < 1 || n_agents > 65535)
    return "the env, observation, action and agent counts must be positive (at most 65535 agents)";
  return nullptr;
}

int pedn_lstm_actor_forward(const float* obs, const int32_t* table, const float* low, const float* high, const float* params,
                            const float* noise, float* hc, float* mu, float* std, float* eps, float* raw, double* actions, int64_t* state,
                            int32_t n_envs, int32_t n_obs, int32_t n_actions, int32_t n_agents, int32_t hidden_size, int32_t num_layers,
                            int32_t delta_actions, int32_t mode, double max_delta, double min_std, double max_std, uint64_t seed,
                            uint32_t replica_offset, void* stream) {
  if (!obs || !table || !low || !high || !params || !hc || !mu || !std || !eps || !raw || !actions || !state)
    return fail(nullptr, PEDN_E_ARG, "null argument");
  if (const char* why = lstm_sizes(n_envs, n_obs, n_actions, n_agents, hidden_size, num_layers)) return fail(nullptr, PEDN_E_ARG, why);
  if (mode < 0 || mode > 2) return fail(nullptr, PEDN_E_ARG, "mode is 0, 1 or 2");
  if (mode == 1 && !noise) return fail(nullptr, PEDN_E_ARG, "mode 1 needs the noise");
  LstmActorArgs a{};
  a.obs = obs; a.table = table; a.low = low; a.high = high; a.params = params; a.noise = noise; a.hc = hc;
  a.mu = mu; a.std = std; a.eps = eps; a.raw = raw; a.actions = actions; a.state = state;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
  a.replica_offset = replica_offset;
  a.n_envs = n_envs; a.n_obs = n_obs; a.n_actions = n_actions;
  a.delta = delta_actions != 0; a.mode = mode;
  a.max_delta = (float)max_delta; a.min_std = (float)min_std; a.max_std = (float)max_std;
  const dim3 grid((unsigned)((n_envs + PEDN_ACTOR_TILE - 1) / PEDN_ACTOR_TILE), (unsigned)n_agents);
  hipLaunchKernelGGL(lstm_actor_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}

int pedn_lstm_reset(float* hc, const uint8_t* mask, int32_t n_envs, int32_t n_agents, int32_t hidden_size, void* stream) {
  if (!hc) return fail(nullptr, PEDN_E_ARG, "null argument");
  if ((uintptr_t)hc & 15) return fail(nullptr, PEDN_E_ARG, "the recurrent state must be 16-byte aligned");
  if (hidden_size != PEDN_ACTOR_HIDDEN) return fail(nullptr, PEDN_E_ARG, "the LSTM kernels are built for hidden_size 64");
  if (n_envs < 1 || n_agents < 1 || n_agents > 65535) return fail(nullptr, PEDN_E_ARG, "n_envs and n_agents must be positive (at most 65535 agents)");
  const int64_t total = (int64_t)n_agents * n_envs * (2 * PEDN_ACTOR_HIDDEN / 4);
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return fail(nullptr, PEDN_E_ARG, "n_agents * n_envs is beyond the grid");
  hipLaunchKernelGGL(lstm_reset_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<float4*>(hc), mask,
                     (int64_t)n_envs, total);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}

int pedn_lstm_ppo_evaluate(const float* obs, const void* actions, const int32_t* table, const int32_t* value_table, const float* actor_params,
                           const float* value_params, float* values, float* next_values, float* old_log_probs, float* mu, float* std,
                           int32_t T, int32_t N, int32_t n_obs, int32_t n_actions, int32_t n_agents, int32_t hidden_size, int32_t num_layers,
                           int32_t actions_f64, double min_std, double max_std, void* stream) {
  if (!obs || !actions || !table || !value_table || !actor_params || !value_params || !values || !next_values || !old_log_probs)
    return fail(nullptr, PEDN_E_ARG, "null argument");
  if (const char* why = lstm_sizes(N, n_obs, n_actions, n_agents, hidden_size, num_layers)) return fail(nullptr, PEDN_E_ARG, why);
  if (T < 1) return fail(nullptr, PEDN_E_ARG, "T must be positive");
  if (actions_f64 < 0 || actions_f64 > 1) return fail(nullptr, PEDN_E_ARG, "the actions' dtype flag is 0 (float32) or 1 (float64)");
  LstmSeqArgs a{};
  a.obs = obs; a.actions = actions; a.table = table; a.vtable = value_table; a.actor = actor_params; a.value = value_params;
  a.values = values; a.next_values = next_values; a.logp = old_log_probs; a.mu = mu; a.std = std;
  a.T = T; a.N = N; a.n_obs = n_obs; a.n_actions = n_actions; a.n_agents = n_agents; a.act_f64 = actions_f64;
  a.min_std = (float)min_std; a.max_std = (float)max_std;
  const dim3 grid((unsigned)((N + PEDN_ACTOR_TILE - 1) / PEDN_ACTOR_TILE), (unsigned)n_agents, 3u);
  hipLaunchKernelGGL(lstm_seq_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}
