// The critic half of the reference's SACAgent.update (rl/agents/SAC.py:320-341: both critic forwards, the two MSE losses against the TD
// target, their backward passes and one Adam step of each critic) for a whole-row minibatch and every agent.  The contract is DESIGN
// section 18; tests/sac_critic_model.py restates it in numpy.
//
// critic_grad_kernel   grid (ceil(B / 32), n_agents), 512 threads.  A workgroup takes one agent and a tile of 32 rows; waves 0-3 run
//                      critic 1, waves 4-7 critic 2, each wave 8 rows with a lane per neuron.  Both critics have the same shapes, so all 8
//                      waves walk the same control flow and share the workgroup barriers and the gathered input chunk.  Forward: section
//                      15's layers (pedn_mlp.hpp's mlp_mac on weight chunks of 32 inputs staged in LDS rows of 33 words), with the
//                      activations kept in LDS: h1, feat = [zs, action, g], h3.  Backward with pedn_mlp_grad.hpp's pieces: a weight
//                      gradient has a lane per output neuron, a wave per 8 of a chunk's 32 input columns and ONE chain over the tile's
//                      rows, ascending; an input gradient has a lane per input column and a chain over the output neurons.  The chunk of a
//                      weight gradient goes to the workspace [tiles][pack + losses] through LDS as 128-byte row pieces.  Rows past B are
//                      not part of any chain.
// critic_adam_kernel   grid-stride over the pack, 16 bytes per access: adds the tiles' partials, tiles ascending, writes the gradient pack
//                      and the losses and, unless switched off, steps exp_avg, exp_avg_sq and the online pack in place.  The last
//                      workgroup to finish advances the step state (the counter and the running products of the betas).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_adam.hpp"
#include "pedn_mlp.hpp"
#include "pedn_mlp_grad.hpp"

struct CriticArgs {
  const float* s;              // [B][S][n_obs]
  const float* actions;        // [B][n_actions]
  const float* td;             // [B][n_agents]
  const int32_t* table;        // [n_agents][PEDN_ACTOR_TABLE_COLS]: the actors' table
  const int32_t* ctable;       // [n_agents][2]: offsets (floats) of critic 1 and critic 2 in the critic packs
  const float* online;         // the online critics' pack
  float* ws;                   // [tiles][ws_stride]: the tiles' partial gradients (the pack's layout), behind them [n_agents][2] partial losses
  float* q;                    // [2][B][n_agents]
  int64_t pack, ws_stride;     // floats
  int32_t B, S, n_obs, n_actions, n_agents;
  float scale;                 // (float)(2.0 / B)
};

__global__ __launch_bounds__(512) void critic_grad_kernel(CriticArgs a) {
  __shared__ float sW[2][PEDN_ACTOR_HIDDEN * PEDN_GRAD_PAD];
  __shared__ __attribute__((aligned(16))) float sXc[PEDN_GRAD_TILE * PEDN_ACTOR_CHUNK];
  __shared__ __attribute__((aligned(16))) float sH1[2][PEDN_GRAD_TILE * PEDN_ACTOR_HIDDEN];
  __shared__ __attribute__((aligned(16))) float sFeat[2][PEDN_GRAD_TILE * PEDN_GRAD_FEAT];
  __shared__ __attribute__((aligned(16))) float sD[2][PEDN_GRAD_TILE * PEDN_GRAD_DS];   // h3, then the output gradient of the layer at hand
  __shared__ float sE[2][PEDN_GRAD_TILE];    // q - td
  __shared__ float sDq[2][PEDN_GRAD_TILE];   // its gradient
  const int tid = (int)threadIdx.x, t = tid & 255, lane = tid & 63;
  const int c = __builtin_amdgcn_readfirstlane(tid >> 8), w4 = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
  const int H = PEDN_ACTOR_HIDDEN;
  const int agent = (int)blockIdx.y;
  const int32_t* tb = a.table + (size_t)agent * PEDN_ACTOR_TABLE_COLS;
  const int obs0 = tb[0], obs_w = tb[1], act0 = tb[2], act_w = tb[3];
  const int K1 = a.S * obs_w, K3 = H + act_w + 1;
  const int row0 = (int)blockIdx.x * PEDN_GRAD_TILE;
  const int nrows = a.B - row0 < PEDN_GRAD_TILE ? a.B - row0 : PEDN_GRAD_TILE;
  const int32_t at = a.ctable[2 * agent + c];
  const float* net = a.online + at;
  float* gws = a.ws + (size_t)blockIdx.x * a.ws_stride + at;
  const int at2 = H * K1 + H, at3 = at2 + H * H + H, at4 = at3 + H * K3 + H;   // fc2, fc, fc_out
  float* mW = sW[c];
  float* mH1 = sH1[c];
  float* mF = sFeat[c];
  float* mD = sD[c];
  const int myrow = w4 * PEDN_GRAD_WAVE_ROWS;
  float acc[PEDN_GRAD_WAVE_ROWS];

  // inputs [c0, c0 + kmax) of the tile's rows for both critics
  auto gather = [&](int c0, int kmax) { sac_gather_chunk(sXc, a.s, a.S, a.n_obs, obs0, row0, nrows, c0, kmax, tid, 512); };

  // ---- forward: section 15's critic on the sampled states and the stored actions
  mlp_group_layer(acc, true, net, net + H * K1, net, net + H * K1, H, H, K1, true, mW, sXc, nullptr, 0, t, gather);
#pragma unroll
  for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) mH1[(myrow + r) * H + lane] = acc[r] < 0.0f ? 0.0f : acc[r];
  mlp_group_layer(acc, true, net + at2, net + at2 + H * H, net + at2, net + at2 + H * H, H, H, H, false, mW, sXc, mH1 + myrow * H, H, t, gather);
#pragma unroll
  for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) mF[(myrow + r) * PEDN_GRAD_FEAT + lane] = acc[r] < 0.0f ? 0.0f : acc[r];
  if (t < PEDN_GRAD_TILE) {   // the stored action and the newest frame's last column of the agent; zeros in rows past B
    const bool live = t < nrows;
    const size_t row = (size_t)(row0 + t);
    for (int j = 0; j < act_w; ++j) mF[t * PEDN_GRAD_FEAT + H + j] = live ? a.actions[row * a.n_actions + act0 + j] : 0.0f;
    mF[t * PEDN_GRAD_FEAT + H + act_w] = live ? a.s[(row * a.S + (a.S - 1)) * a.n_obs + obs0 + obs_w - 1] : 0.0f;
    for (int j = K3; j < PEDN_GRAD_FEAT; ++j) mF[t * PEDN_GRAD_FEAT + j] = 0.0f;
  }
  mlp_group_layer(acc, true, net + at3, net + at3 + H * K3, net + at3, net + at3 + H * K3, H, H, K3, false, mW, sXc, mF + myrow * PEDN_GRAD_FEAT,
                  PEDN_GRAD_FEAT, t, gather);
#pragma unroll
  for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) mD[(myrow + r) * PEDN_GRAD_DS + lane] = acc[r];   // (no ReLU behind fc, as in the reference)
  const float* wo = net + at4;
  __syncthreads();
  if (lane < PEDN_GRAD_WAVE_ROWS) {   // fc_out on a lane per row, section 15's chain
    const int r = myrow + lane;
    float q = wo[H];
    for (int k = 0; k < H; ++k) q = q + wo[k] * mD[r * PEDN_GRAD_DS + k];
    float e = 0.0f;
    if (r < nrows) {
      const size_t row = (size_t)(row0 + r);
      a.q[((size_t)c * a.B + row) * a.n_agents + agent] = q;
      e = q - a.td[row * a.n_agents + agent];
    }
    sE[c][r] = e;
    sDq[c][r] = e * a.scale;
  }
  __syncthreads();

  // ---- backward.  fc_out: its weight (lane k of wave 1), its bias and the tile's sum of squares (wave 2); then h3's gradient in place
  if (w4 == 1) {
    float g = 0.0f;
    for (int r = 0; r < nrows; ++r) g = g + sDq[c][r] * mD[r * PEDN_GRAD_DS + lane];
    gws[at4 + lane] = g;
  } else if (w4 == 2 && lane < 2) {
    float g = 0.0f;
    if (lane == 0) {
      for (int r = 0; r < nrows; ++r) g = g + sDq[c][r];
      gws[at4 + H] = g;
    } else {
      for (int r = 0; r < nrows; ++r) g = g + sE[c][r] * sE[c][r];
      a.ws[(size_t)blockIdx.x * a.ws_stride + a.pack + 2 * agent + c] = g;
    }
  }
  __syncthreads();
  {
    const float wl = wo[lane];
#pragma unroll
    for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) mD[(myrow + r) * PEDN_GRAD_DS + lane] = sDq[c][myrow + r] * wl;
  }
  // fc: weight and bias; the 64 encoder columns of dfeat; the ReLU mask z > 0
  mlp_grad_dw_tile<8, false>(mD, PEDN_GRAD_DS, mF, PEDN_GRAD_FEAT, K3, nrows, gws + at3, gws + at3 + H * K3, mW, false, true, true, 0, t, 256, gather);
  mlp_grad_dx_tile(acc, true, mD + myrow * PEDN_GRAD_DS, PEDN_GRAD_DS, net + at3, K3, mW, t, 256);
  __syncthreads();   // every wave has read the output gradient that is overwritten now
#pragma unroll
  for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) mD[(myrow + r) * PEDN_GRAD_DS + lane] = mF[(myrow + r) * PEDN_GRAD_FEAT + lane] > 0.0f ? acc[r] : 0.0f;
  // encoder.fc2, then the mask, then encoder.fc1
  mlp_grad_dw_tile<8, false>(mD, PEDN_GRAD_DS, mH1, H, H, nrows, gws + at2, gws + at2 + H * H, mW, false, true, true, 0, t, 256, gather);
  mlp_grad_dx_tile(acc, true, mD + myrow * PEDN_GRAD_DS, PEDN_GRAD_DS, net + at2, H, mW, t, 256);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) mD[(myrow + r) * PEDN_GRAD_DS + lane] = mH1[(myrow + r) * H + lane] > 0.0f ? acc[r] : 0.0f;
  mlp_grad_dw_tile<8, false>(mD, PEDN_GRAD_DS, sXc, PEDN_ACTOR_CHUNK, K1, nrows, gws, gws + H * K1, mW, true, true, true, 0, t, 256, gather);
}

struct CriticAdamArgs {
  const float4* ws;            // the workspace, rows of ws_stride floats
  float4* grads;               // the gradient pack
  float4* m;                   // exp_avg
  float4* v;                   // exp_avg_sq
  float4* p;                   // the online pack
  float* losses;               // [n_agents][2]
  int64_t* state;              // pedn_adam.hpp's step state
  int64_t n4, ws_stride4;      // the pack's and a workspace row's length in float4
  int32_t tiles, n_agents, B, do_adam;
  double lr, beta1, beta2;
  AdamCoef coef;
};

__global__ __launch_bounds__(256) void critic_adam_kernel(CriticAdamArgs a) {
  const AdamStep st = adam_step_begin(a.state, a.beta1, a.beta2);
  const float nstep = adam_nstep(a.lr, st), s = st.s;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = gid; i < a.n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int tl = 0; tl < a.tiles; ++tl) {   // tiles ascending
      const float4 w = a.ws[(int64_t)tl * a.ws_stride4 + i];
      g.x = g.x + w.x; g.y = g.y + w.y; g.z = g.z + w.z; g.w = g.w + w.w;
    }
    a.grads[i] = g;
    if (a.do_adam) {
      float4 m = a.m[i], v = a.v[i], p = a.p[i];
      p.x = adam_one<false>(g.x, m.x, v.x, p.x, a.coef, nstep, s);
      p.y = adam_one<false>(g.y, m.y, v.y, p.y, a.coef, nstep, s);
      p.z = adam_one<false>(g.z, m.z, v.z, p.z, a.coef, nstep, s);
      p.w = adam_one<false>(g.w, m.w, v.w, p.w, a.coef, nstep, s);
      a.m[i] = m; a.v[i] = v; a.p[i] = p;
    }
  }
  if (gid < 2 * (int64_t)a.n_agents) {   // the mean of the squares: the tiles' sums, ascending, over B
    const float* wsf = reinterpret_cast<const float*>(a.ws);
    float l = 0.0f;
    for (int tl = 0; tl < a.tiles; ++tl) l = l + wsf[((int64_t)tl * a.ws_stride4 + a.n4) * 4 + gid];
    a.losses[gid] = l / (float)a.B;
  }
  if (!a.do_adam) return;
  __syncthreads();   // every wave of the workgroup has read the step state
  if (threadIdx.x == 0) adam_step_advance(a.state, st, gridDim.x);   // the last workgroup advances the state
}

// ---- host side: pedn_sac_critic_update of include/pedn.h; no state in the engine's handle
int pedn_sac_critic_update(const float* states, const float* actions, const float* td_target, const int32_t* table, const int32_t* critic_table,
                           float* online_params, float* grads, float* exp_avg, float* exp_avg_sq, float* workspace, float* q, float* losses,
                           int64_t* adam_state, int64_t pack_floats, int32_t batch, int32_t stack_size, int32_t n_obs, int32_t n_actions,
                           int32_t n_agents, int32_t hidden_size, double lr, double beta1, double beta2, double eps, int32_t do_adam,
                           void* stream) {
  if (!states || !actions || !td_target || !table || !critic_table || !online_params || !grads || !exp_avg || !exp_avg_sq || !workspace || !q ||
      !losses || !adam_state)
    return fail(nullptr, PEDN_E_ARG, "null argument");
  if (const char* why = update_refusal(
          hidden_size, "the critic kernels are built for hidden_size 64", batch >= 1 && stack_size >= 1 && n_obs >= 1 && n_actions >= 1, n_agents,
          "batch, stack_size, n_obs, n_actions and n_agents must be positive (at most 65535 agents)", nullptr, pack_floats >= 4 && pack_floats % 4 == 0,
          "the packs' length must be a positive multiple of 4 floats",
          (uintptr_t)online_params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)workspace, lr, lr, beta1, beta2, eps))
    return fail(nullptr, PEDN_E_ARG, why);
  const int tiles = (batch + PEDN_GRAD_TILE - 1) / PEDN_GRAD_TILE;
  const int64_t ws_stride = pack_floats + (2 * (int64_t)n_agents + 3) / 4 * 4;
  CriticArgs a{};
  a.s = states; a.actions = actions; a.td = td_target; a.table = table; a.ctable = critic_table; a.online = online_params;
  a.ws = workspace; a.q = q; a.pack = pack_floats; a.ws_stride = ws_stride;
  a.B = batch; a.S = stack_size; a.n_obs = n_obs; a.n_actions = n_actions; a.n_agents = n_agents;
  a.scale = (float)(2.0 / (double)batch);
  hipLaunchKernelGGL(critic_grad_kernel, dim3((unsigned)tiles, (unsigned)n_agents), dim3(512), 0, (hipStream_t)stream, a);
  HIP_TRY(nullptr, hipGetLastError());
  CriticAdamArgs b{};
  b.ws = reinterpret_cast<const float4*>(workspace); b.grads = reinterpret_cast<float4*>(grads); b.m = reinterpret_cast<float4*>(exp_avg);
  b.v = reinterpret_cast<float4*>(exp_avg_sq); b.p = reinterpret_cast<float4*>(online_params); b.losses = losses; b.state = adam_state;
  b.n4 = pack_floats / 4; b.ws_stride4 = ws_stride / 4; b.tiles = tiles; b.n_agents = n_agents; b.B = batch; b.do_adam = do_adam ? 1 : 0;
  b.lr = lr; b.beta1 = beta1; b.beta2 = beta2;
  b.coef = adam_coef(beta1, beta2, eps);
  int64_t blocks = (b.n4 + 255) / 256;
  const int64_t need = (2 * (int64_t)n_agents + 255) / 256;   // the losses have a thread each
  blocks = blocks < need ? need : blocks < 2048 ? blocks : 2048;
  hipLaunchKernelGGL(critic_adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, b);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}
