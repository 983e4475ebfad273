// The gradient-free half of the reference's SACAgent.update (rl/agents/SAC.py:296-318 calc_target and soft_update, with the critic
// QValueNetContinuous :109-125) for a whole-row minibatch and every agent.  The contract is DESIGN section 15; tests/sac_target_model.py
// restates it in numpy.
//
// sac_target_kernel   grid (ceil(B / PEDN_SAC_TILE), n_agents), 192 threads.  A workgroup evaluates one agent for a tile of 8 rows with a
//                     wave per network: wave 0 the actor, waves 1 and 2 the two target critics.  A wave runs its layers on its own: a lane
//                     per neuron, 8 accumulators (one per row), chunks of 32 inputs whose weight rows (nn.Linear's [out][in], read with
//                     128-byte row pieces) it copies into its OWN LDS rows of 33 words; within a wave the LDS unit serves reads behind the
//                     writes issued before them, so a wave's staging needs no workgroup barrier, only the compiler kept from reordering
//                     (sac_wave_sync).  The accumulation is pedn_mlp.hpp's mlp_mac, the one of section 14's mlp_layer.  The actor wave
//                     ends with the double-precision tail on a lane per (row, action): mlp_softplus, the noise (philox_normal), tanh,
//                     normal_log_prob; then the entropy on a lane per row.  ONE workgroup barrier hands next_action to the critic waves,
//                     which by then have their encoders behind them; they append it and the newest gate width to their 64 encoder outputs
//                     (an LDS row of 76 words), run fc (K = 65 + act_w, no ReLU) and fc_out (a lane per row).  A second barrier hands q1
//                     and q2 to the 8 lanes that form the target.  The last workgroup to finish advances the draw counter (ticket
//                     counter, vector atomics), when the launch drew noise.
// sac_polyak_kernel   target = target * (1 - tau) + online * tau over a whole pack, grid-stride, 16 bytes per access.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_mlp.hpp"

#define PEDN_SAC_TILE 8           // rows per workgroup (and per wave: every wave sees the whole tile)
#define PEDN_SAC_FEAT 76          // words of a critic's fc input row: 64 + act_w + 1 <= 73, rounded up to 16 bytes
#define PEDN_SAC_NOISE_SITE 0x73u

struct SacTargetArgs {
  const float* ns;             // [B][S][n_obs]
  const float* rewards;        // [B][n_agents]
  const float* dones;          // [B]
  const int32_t* table;        // [n_agents][PEDN_ACTOR_TABLE_COLS]: the actors' table
  const int32_t* ctable;       // [n_agents][2]: offsets (floats) of critic 1 and critic 2 in the critic packs
  const float* actor;          // the actors' pack (SAC kind)
  const float* critic;         // the target critics' pack
  const float* log_alpha;      // [n_agents]
  const float* noise;          // [B][n_actions] or null (draw)
  float* out_actions;          // [5][B][n_actions]: mu, std, eps, logp, next_actions
  float* out_agents;           // [4][B][n_agents]: entropy, q1, q2, td_target
  int64_t* state;              // 0 draw counter, 1 ticket (its low 32 bits)
  uint32_t k0, k1;             // key(seed)
  int32_t B, S, n_obs, n_actions, n_agents;
  float max_delta, gamma;
};

// Orders this wave's LDS writes before its later LDS reads of other lanes' words.  The hardware needs nothing (a wave's LDS instructions
// complete in order); the fences and the wave barrier keep the compiler from moving accesses across.
__device__ __forceinline__ void sac_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One layer of one wave for the tile's 8 rows: acc[r] = b[o]; then mlp_mac over chunks of 32 inputs, for lane o < rows.  Row
// o of the weights starts at w + o * K, behind `gap` more floats from row n0 on (the two heads with fc_mu's bias between them); the biases
// of rows [0, n0) lie behind row n0 - 1, the others behind the last row.  first: x is gathered from the next stacks (through sXc, rows of
// 32); otherwise x is the wave's LDS rows xin of stride xs (a multiple of 4 words).  sW, sXc: this wave's own.
__device__ __forceinline__ void sac_layer(const SacTargetArgs& a, float (&acc)[PEDN_SAC_TILE], const float* w, int n0, int gap, int rows, int K,
                                          bool first, int obs0, unsigned row0, float* sW, float* sXc, const float* xin, int xs) {
  const int lane = (int)(threadIdx.x & 63);
  const float bias = lane < rows ? w[(unsigned)(lane < n0 ? n0 * K + lane : rows * K + gap + lane - n0)] : 0.0f;
#pragma unroll
  for (int r = 0; r < PEDN_SAC_TILE; ++r) acc[r] = bias;
  for (int c0 = 0; c0 < K; c0 += PEDN_ACTOR_CHUNK) {
    const int kmax = K - c0 < PEDN_ACTOR_CHUNK ? K - c0 : PEDN_ACTOR_CHUNK;
    sac_wave_sync();   // the chunk before has been consumed (and the layer before has written its rows)
    {
      // half a wave per 128-byte row piece; 16 rows per pass, whose loads are all issued before the first LDS write waits for one.  A row
      // past the layer's last or a column past the chunk's last reads the last one in its place (no lane reads that LDS word).
      const int kk = lane & (PEDN_ACTOR_CHUNK - 1), half = lane >> 5;
      const int kc = c0 + (kk < kmax ? kk : kmax - 1);
#pragma unroll 1
      for (int p0 = 0; p0 < rows; p0 += 32) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          int o = p0 + 2 * i + half;
          o = o < rows ? o : rows - 1;
          v[i] = w[(unsigned)(o * K + (o < n0 ? 0 : gap) + kc)];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) sW[(p0 + 2 * i + half) * (PEDN_ACTOR_CHUNK + 1) + kk] = v[i];
      }
    }
    if (first) {   // rows past the batch's last read the last one in its place: nothing of them is stored
      const unsigned kk = (unsigned)lane & (PEDN_ACTOR_CHUNK - 1), half = (unsigned)lane >> 5;
      const unsigned k = (unsigned)c0 + ((int)kk < kmax ? kk : (unsigned)kmax - 1u), f = k / (unsigned)a.S, s = k - f * (unsigned)a.S;
      float x[PEDN_SAC_TILE / 2];
#pragma unroll
      for (unsigned i = 0; i < PEDN_SAC_TILE / 2; ++i) {
        unsigned row = row0 + 2 * i + half;
        row = row < (unsigned)a.B ? row : (unsigned)a.B - 1u;
        x[i] = a.ns[((size_t)row * a.S + s) * a.n_obs + obs0 + f];
      }
#pragma unroll
      for (unsigned i = 0; i < PEDN_SAC_TILE / 2; ++i) sXc[(2 * i + half) * PEDN_ACTOR_CHUNK + kk] = x[i];
    }
    sac_wave_sync();
    if (lane < rows) mlp_mac(acc, sW + lane * (PEDN_ACTOR_CHUNK + 1), first ? sXc : xin + c0, first ? PEDN_ACTOR_CHUNK : xs, kmax);
  }
}

__global__ __launch_bounds__(192) void sac_target_kernel(SacTargetArgs a) {
  // per wave: a weight chunk, an input chunk and hidden rows; per critic wave the fc input rows; the hand-overs
  __shared__ float sW[3][PEDN_ACTOR_HIDDEN * (PEDN_ACTOR_CHUNK + 1)];
  __shared__ __attribute__((aligned(16))) float sXc[3][PEDN_SAC_TILE * PEDN_ACTOR_CHUNK];
  __shared__ __attribute__((aligned(16))) float sH[3][PEDN_SAC_TILE * PEDN_ACTOR_HIDDEN];
  __shared__ __attribute__((aligned(16))) float sFeat[2][PEDN_SAC_TILE * PEDN_SAC_FEAT];
  __shared__ float sOut[PEDN_SAC_TILE * 2 * PEDN_ACTOR_MAX_ACT];   // mu | pre-softplus of the heads
  __shared__ float sAct[PEDN_SAC_TILE * PEDN_ACTOR_MAX_ACT];       // next_action
  __shared__ float sLogp[PEDN_SAC_TILE * PEDN_ACTOR_MAX_ACT];
  __shared__ float sEnt[PEDN_SAC_TILE];
  __shared__ float sQ[2][PEDN_SAC_TILE];
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int H = PEDN_ACTOR_HIDDEN;
  const int agent = (int)blockIdx.y;
  const int32_t* t = a.table + (size_t)agent * PEDN_ACTOR_TABLE_COLS;
  const int obs0 = t[0], obs_w = t[1], act0 = t[2], act_w = t[3];
  const int K1 = a.S * obs_w;
  const unsigned row0 = blockIdx.x * PEDN_SAC_TILE;
  float* mW = sW[wave];
  float* mX = sXc[wave];
  float* mH = sH[wave];
  float acc[PEDN_SAC_TILE];
  // the wave's network: the layers lie one behind the other, nn.Linear's weight then bias
  const float* net = wave == 0 ? a.actor + t[4] : a.critic + a.ctable[2 * agent + (wave - 1)];
  const int K3 = wave == 0 ? H : H + act_w + 1;
  const int at2 = H * K1 + H, at3 = at2 + H * H + H, at4 = at3 + H * K3 + H;   // fc2, fc, behind fc: the heads / fc_out
  float* feat = sFeat[wave == 0 ? 0 : wave - 1];

  // Layer li of the wave's network, up to the barrier: the actor's four, a critic's encoder.
  const int n_before = wave == 0 ? 4 : 2;
#pragma unroll 1
  for (int li = 0; li < n_before; ++li) {
    const bool heads = li == 3;
    const float* w = net + (li == 0 ? 0 : li == 1 ? at2 : li == 2 ? at3 : at4);
    const int n0 = heads ? act_w : H, rows = heads ? 2 * act_w : H;   // (the heads: fc_mu's rows, its bias, fc_std's rows, its bias)
    sac_layer(a, acc, w, n0, heads ? act_w : 0, rows, li == 0 ? K1 : H, li == 0, obs0, row0, mW, mX, mH, H);
    sac_wave_sync();   // (every lane has read the rows that are overwritten now)
    // ReLU into the next layer's input rows (a critic's encoder: into its fc input rows); the heads (mu | the pre-softplus value) as they are
    float* dst = heads ? sOut : (wave != 0 && li == 1 ? feat : mH);
    const int ds = heads ? 2 * PEDN_ACTOR_MAX_ACT : (wave != 0 && li == 1 ? PEDN_SAC_FEAT : H);
    if (lane < rows) {
      const int col = lane < n0 ? lane : PEDN_ACTOR_MAX_ACT + lane - n0;
#pragma unroll
      for (int r = 0; r < PEDN_SAC_TILE; ++r) dst[r * ds + col] = (!heads && acc[r] < 0.0f) ? 0.0f : acc[r];
    }
  }
  if (wave == 0) {
    sac_wave_sync();
    // the tail in double on a lane per (row, action)
    const int lr = lane / act_w, j = lane - lr * act_w;
    const unsigned row = row0 + (unsigned)lr;
    if (lr < PEDN_SAC_TILE) {
      const float mu = sOut[lr * 2 * PEDN_ACTOR_MAX_ACT + j], z = sOut[lr * 2 * PEDN_ACTOR_MAX_ACT + PEDN_ACTOR_MAX_ACT + j];
      const int col = act0 + j;
      const bool live = row < (unsigned)a.B;
      const size_t at = (size_t)row * a.n_actions + col;
      const float sd = mlp_softplus(z);
      float eps = 0.0f;
      if (a.noise) {
        if (live) eps = a.noise[at];
      } else
        eps = philox_normal(a.k0, a.k1, row, a.state[0], PEDN_SAC_NOISE_SITE | ((uint32_t)col << 8));
      const float u = mu + sd * eps;
      const float th = (float)tanh((double)u);
      const float na = th * a.max_delta;
      // Normal(mu, std).log_prob(u) - log(1 - tanh(tanh(u))^2 + 1e-7): the reference squashes the squashed action once more
      const double T2 = tanh((double)th);
      const double lp = normal_log_prob(u, mu, sd) - log(1.0 - T2 * T2 + 1e-7);
      const float logp = (float)lp;
      sAct[lr * PEDN_ACTOR_MAX_ACT + j] = na;
      sLogp[lr * PEDN_ACTOR_MAX_ACT + j] = logp;
      if (live) {
        float* o = a.out_actions + at;
        const size_t plane = (size_t)a.B * a.n_actions;
        o[0] = mu; o[plane] = sd; o[2 * plane] = eps; o[3 * plane] = logp; o[4 * plane] = na;
      }
    }
    sac_wave_sync();
    if (lane < PEDN_SAC_TILE) {
      float ent = 0.0f;
      for (int jj = 0; jj < act_w; ++jj) ent = ent - sLogp[lane * PEDN_ACTOR_MAX_ACT + jj];
      sEnt[lane] = ent;
      if (row0 + (unsigned)lane < (unsigned)a.B) a.out_agents[(size_t)(row0 + lane) * a.n_agents + agent] = ent;
    }
  } else if (lane < PEDN_SAC_TILE) {   // the newest frame's last column of the agent: the reference's s[:, -1, -1] behind its transpose
    const unsigned row = row0 + (unsigned)lane;
    feat[lane * PEDN_SAC_FEAT + H + act_w] = row < (unsigned)a.B ? a.ns[((size_t)row * a.S + (a.S - 1)) * a.n_obs + obs0 + obs_w - 1] : 0.0f;
  }
  __syncthreads();   // next_action is there
  if (wave != 0) {
    const int lr = lane / act_w, j = lane - lr * act_w;
    if (lr < PEDN_SAC_TILE) feat[lr * PEDN_SAC_FEAT + H + j] = sAct[lr * PEDN_ACTOR_MAX_ACT + j];
    sac_layer(a, acc, net + at3, H, 0, H, K3, false, obs0, row0, mW, mX, feat, PEDN_SAC_FEAT);
#pragma unroll
    for (int r = 0; r < PEDN_SAC_TILE; ++r) mH[r * H + lane] = acc[r];   // (no ReLU behind fc, as in the reference)
    const float* wo = net + at4;
    const float* bo = wo + H;
    sac_wave_sync();
    if (lane < PEDN_SAC_TILE) {   // fc_out on a lane per row
      float q = bo[0];
      for (int k = 0; k < H; ++k) q = q + wo[k] * mH[lane * H + k];
      sQ[wave - 1][lane] = q;
      if (row0 + (unsigned)lane < (unsigned)a.B) a.out_agents[((size_t)wave * a.B + row0 + lane) * a.n_agents + agent] = q;
    }
  }
  __syncthreads();   // q1 and q2 are there
  if (threadIdx.x < PEDN_SAC_TILE && row0 + threadIdx.x < (unsigned)a.B) {
    const unsigned row = row0 + threadIdx.x;
    const float q1 = sQ[0][threadIdx.x], q2 = sQ[1][threadIdx.x];
    const float q = (q2 < q1 || q2 != q2) ? q2 : q1;   // torch.min: NaN wins
    const float alpha = (float)exp((double)a.log_alpha[agent]);
    const float nv = q + alpha * sEnt[threadIdx.x];
    const size_t at = (size_t)row * a.n_agents + agent;
    a.out_agents[3 * (size_t)a.B * a.n_agents + at] = a.rewards[at] + (a.gamma * nv) * (1.0f - a.dones[row]);
  }
  if (a.noise) return;
  if (threadIdx.x == 0) advance_draw_counter(a.state, a.state[0]);   // (this lane's wave has read the draw counter)
}

// target[i] = target[i] * (1 - tau) + online[i] * tau; n4 = the pack's length in float4.
__global__ __launch_bounds__(256) void sac_polyak_kernel(float4* __restrict__ target, const float4* __restrict__ online, int64_t n4, float keep, float tau) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 t = target[i];
    const float4 o = online[i];
    t.x = t.x * keep + o.x * tau;
    t.y = t.y * keep + o.y * tau;
    t.z = t.z * keep + o.z * tau;
    t.w = t.w * keep + o.w * tau;
    target[i] = t;
  }
}

// ---- host side: pedn_sac_td_target and pedn_sac_soft_update of include/pedn.h; no state in the engine's handle
int pedn_sac_td_target(const float* next_states, const float* rewards, const float* dones, const int32_t* table, const int32_t* critic_table,
                       const float* actor_params, const float* target_params, const float* log_alpha, const float* noise,
                       float* out_actions, float* out_agents, int64_t* state, int32_t batch, int32_t stack_size, int32_t n_obs,
                       int32_t n_actions, int32_t n_agents, int32_t hidden_size, double max_delta, double gamma, uint64_t seed,
                       void* stream) {
  if (!next_states || !rewards || !dones || !table || !critic_table || !actor_params || !target_params || !log_alpha || !out_actions ||
      !out_agents || !state)
    return fail(nullptr, PEDN_E_ARG, "null argument");
  if (hidden_size != PEDN_ACTOR_HIDDEN) return fail(nullptr, PEDN_E_ARG, "the SAC target kernel is built for hidden_size 64");
  if (batch < 1 || stack_size < 1 || n_obs < 1 || n_actions < 1 || n_agents < 1 || n_agents > 65535)
    return fail(nullptr, PEDN_E_ARG, "batch, stack_size, n_obs, n_actions and n_agents must be positive (at most 65535 agents)");
  SacTargetArgs a{};
  a.ns = next_states; a.rewards = rewards; a.dones = dones; a.table = table; a.ctable = critic_table;
  a.actor = actor_params; a.critic = target_params; a.log_alpha = log_alpha; a.noise = noise;
  a.out_actions = out_actions; a.out_agents = out_agents; a.state = state;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
  a.B = batch; a.S = stack_size; a.n_obs = n_obs; a.n_actions = n_actions; a.n_agents = n_agents;
  a.max_delta = (float)max_delta; a.gamma = (float)gamma;
  const dim3 grid((unsigned)((batch + PEDN_SAC_TILE - 1) / PEDN_SAC_TILE), (unsigned)n_agents);
  hipLaunchKernelGGL(sac_target_kernel, grid, dim3(192), 0, (hipStream_t)stream, a);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}

int pedn_sac_soft_update(float* target, const float* online, int64_t n_floats, double tau, void* stream) {
  if (!target || !online) return fail(nullptr, PEDN_E_ARG, "null argument");
  if (n_floats < 4 || n_floats % 4) return fail(nullptr, PEDN_E_ARG, "the packs' length must be a positive multiple of 4 floats");
  if (((uintptr_t)target | (uintptr_t)online) & 15) return fail(nullptr, PEDN_E_ARG, "the packs must be 16-byte aligned");
  if (!(tau >= 0.0 && tau <= 1.0)) return fail(nullptr, PEDN_E_ARG, "tau must be in [0, 1]");
  const int64_t n4 = n_floats / 4;
  const int64_t blocks = (n4 + 255) / 256;
  hipLaunchKernelGGL(sac_polyak_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<float4*>(target), reinterpret_cast<const float4*>(online), n4, (float)(1.0 - tau), (float)tau);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}
