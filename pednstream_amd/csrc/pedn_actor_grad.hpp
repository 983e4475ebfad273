// The actor half of the reference's SACAgent.update (rl/agents/SAC.py:347-370: the actor loss, its backward pass through the actor and
// through both stepped online critics, the actor's Adam step, the temperature loss and its Adam step) for a whole-row minibatch and every
// agent.  The contract is DESIGN section 19; tests/sac_actor_model.py restates it in numpy.
//
// sacactor_grad_kernel   grid (ceil(B / 32), n_agents), 768 threads.  A workgroup takes one agent and a tile of 32 rows (section 18's tile).
//                        Three groups of 4 waves run the three networks side by side, 8 rows per wave, a lane per neuron: group 0 critic 1,
//                        group 1 critic 2, group 2 the actor.  fc1 and fc2 have the same shapes in all three, so the groups share the
//                        gathered input chunk and the workgroup barriers; the actor's fc and heads run while the critics wait, the
//                        critics' fc (which needs new_action) while the actor waits.  The tails (section 15's, then the backward's) run on
//                        a lane per (row, action) of the actor's group, in double from the float32 values, rounded once.  A critic is linear
//                        behind its encoder, so d q / d action_j is the vector sum_o fc_out[o] * fc[o][64 + j] of the critic: no critic
//                        backward.  The actor's backward is pedn_mlp_grad.hpp's: a weight gradient has a lane per output neuron, 8 waves with
//                        4 of a chunk's 32 columns each and ONE chain over the tile's rows; an input gradient has a lane per column, 8
//                        waves with 4 rows each and a chain over the output neurons.  The tile's partials go to the workspace
//                        [tiles][pack + per-agent sums].  Rows past B are in no chain.
// sacactor_adam_kernel   grid-stride over the actors' pack: adds the tiles' partials, tiles ascending, writes the gradient pack, the losses
//                        and alpha_grad and, unless switched off, takes section 18's Adam step (exp_avg_sq's multiply-add fused) on the pack
//                        and on every log_alpha.
// (The kernels are not called actor_*: tests/test_actor_kernel_resources.py counts every kernel of that prefix as pedn_actor.hpp's.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_adam.hpp"
#include "pedn_mlp.hpp"
#include "pedn_mlp_grad.hpp"

#define PEDN_AG_THREADS 768
#define PEDN_AG_NOISE_SITE 0x75u

struct ActorGradArgs {
  const float* s;              // [B][S][n_obs]
  const float* noise;          // [B][n_actions] or null (draw)
  const int32_t* table;        // [n_agents][PEDN_ACTOR_TABLE_COLS]: the actors' table
  const int32_t* ctable;       // [n_agents][2]: offsets (floats) of critic 1 and critic 2 in the critic packs
  const float* actor;          // the actors' pack (SAC kind)
  const float* online;         // the online critics' pack
  const float* log_alpha;      // [n_agents]
  const float* tent;           // [n_agents]: the target entropies
  float* ws;                   // [tiles][ws_stride]: the tiles' partial gradients (the actors' pack's layout), behind them [n_agents][2] partial sums
  float* out_actions;          // [9][B][n_actions]: mu, std, eps, logp, new_actions, z (the pre-softplus value), t = tanh(u), and the loss' gradients by mu and by z
  float* out_agents;           // [3][B][n_agents]: entropy, q1, q2
  int64_t* state;              // 0 draw counter, 1 ticket (its low 32 bits)
  int64_t pack4, ws_stride;    // floats: where a workspace row's sums start, and its length
  uint32_t k0, k1;             // key(seed)
  int32_t B, S, n_obs, n_actions, n_agents;
  float max_delta;
};

// The launch's arguments as the kernel argument segment holds them, for the fields that only the tails read: read there, a field is loaded
// where it is used and not held in SGPRs from the kernel's entry on (with every field live throughout the kernel spilled 43 SGPRs).  The
// empty asm keeps the compiler from merging the loads into the entry block's.
typedef const __attribute__((address_space(4))) ActorGradArgs* ActorGradLate;
__device__ __forceinline__ ActorGradLate ag_late_args() {
  ActorGradLate p = (ActorGradLate)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

__global__ __launch_bounds__(PEDN_AG_THREADS) void sacactor_grad_kernel(ActorGradArgs a) {
  __shared__ float sW[3][PEDN_ACTOR_HIDDEN * PEDN_GRAD_PAD];
  __shared__ __attribute__((aligned(16))) float sXc[PEDN_GRAD_TILE * PEDN_ACTOR_CHUNK];
  __shared__ __attribute__((aligned(16))) float sA[3][PEDN_GRAD_TILE * PEDN_ACTOR_HIDDEN];   // h1 of the three networks
  __shared__ __attribute__((aligned(16))) float sB[PEDN_GRAD_TILE * PEDN_ACTOR_HIDDEN];      // the actor's h2
  __shared__ __attribute__((aligned(16))) float sC[PEDN_GRAD_TILE * PEDN_ACTOR_HIDDEN];      // the actor's h3 behind its ReLU
  __shared__ __attribute__((aligned(16))) float sF[2][PEDN_GRAD_TILE * PEDN_GRAD_FEAT];    // the critics' fc input rows
  __shared__ __attribute__((aligned(16))) float sD[3][PEDN_GRAD_TILE * PEDN_GRAD_DS];      // 0, 1: the critics' fc output; 2: the heads' gradient
  __shared__ float sOut[PEDN_GRAD_TILE * 2 * PEDN_ACTOR_MAX_ACT];                            // mu | pre-softplus of the heads
  __shared__ float sAct[PEDN_GRAD_TILE * PEDN_ACTOR_MAX_ACT];                                // new_action
  __shared__ float sLogp[PEDN_GRAD_TILE * PEDN_ACTOR_MAX_ACT];
  __shared__ float sTail[3][PEDN_GRAD_TILE * PEDN_ACTOR_MAX_ACT];                         // std, eps and t = tanh(u), for the backward's tail
  __shared__ float sEnt[PEDN_GRAD_TILE];
  __shared__ float sQ[2][PEDN_GRAD_TILE];
  __shared__ float sWo[2][PEDN_ACTOR_HIDDEN];      // the critics' fc_out weights
  __shared__ double sV[2][PEDN_ACTOR_MAX_ACT];     // d q / d action of each critic
  __shared__ float sL[2][PEDN_GRAD_TILE];        // a row's -alpha * entropy - min_q, and its entropy - target_entropy
  const int tid = (int)threadIdx.x, t = tid & 255, lane = tid & 63;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 8), w4 = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
  const int H = PEDN_ACTOR_HIDDEN;
  const int agent = (int)blockIdx.y;
  const int32_t* tb = a.table + (size_t)agent * PEDN_ACTOR_TABLE_COLS;
  const int obs0 = tb[0], obs_w = tb[1], act0 = tb[2], act_w = tb[3];
  const int K1 = a.S * obs_w, K3 = H + act_w + 1;
  const int row0 = (int)blockIdx.x * PEDN_GRAD_TILE;
  const int nrows = a.B - row0 < PEDN_GRAD_TILE ? a.B - row0 : PEDN_GRAD_TILE;
  const bool is_actor = g == 2;
  const float* anet = a.actor + tb[4];
  const float* net = is_actor ? anet : a.online + a.ctable[2 * agent + g];
  const int at2 = H * K1 + H, at3 = at2 + H * H + H;                 // fc2, fc
  const int at4 = at3 + H * (is_actor ? H : K3) + H;                 // the actor's heads / a critic's fc_out
  const int ah = at3 + H * H + H;                                    // the actor's heads, for every thread
  float* mW = sW[g];
  float* mA = sA[g];
  const int myrow = w4 * PEDN_GRAD_WAVE_ROWS;
  // the wave's first row once more, as a vector value, for the stores of its rows: from the scalar the compiler forms every row's LDS
  // address in SGPRs and holds them through the forward, which spilled
  const int vrow = ((tid >> 6) & 3) * PEDN_GRAD_WAVE_ROWS;
  const bool given = a.noise != nullptr;
  float acc[PEDN_GRAD_WAVE_ROWS];

  // inputs [c0, c0 + kmax) of the tile's rows for all three networks
  auto gather = [&](int c0, int kmax) { sac_gather_chunk(sXc, a.s, a.S, a.n_obs, obs0, row0, nrows, c0, kmax, tid, PEDN_AG_THREADS); };

  // ---- forward: the encoders of the three networks side by side
  mlp_group_layer(acc, true, net, net + H * K1, net, net + H * K1, H, H, K1, true, mW, sXc, nullptr, 0, t, gather);
#pragma unroll
  for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) mA[(vrow + r) * H + lane] = acc[r] < 0.0f ? 0.0f : acc[r];
  mlp_group_layer(acc, true, net + at2, net + at2 + H * H, net + at2, net + at2 + H * H, H, H, H, false, mW, sXc, mA + myrow * H, H, t, gather);
  if (is_actor) {
#pragma unroll
    for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) sB[(vrow + r) * H + lane] = acc[r] < 0.0f ? 0.0f : acc[r];
  } else {
#pragma unroll
    for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) sF[g][(vrow + r) * PEDN_GRAD_FEAT + lane] = acc[r] < 0.0f ? 0.0f : acc[r];
  }
  // the actor's fc and heads (section 14's SAC kind); the critics' groups take the barriers
  mlp_group_layer(acc, is_actor, anet + at3, anet + at3 + H * H, anet + at3, anet + at3 + H * H, H, H, H, false, mW, sXc, sB + myrow * H, H, t, gather);
  if (is_actor) {
#pragma unroll
    for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) sC[(vrow + r) * H + lane] = acc[r] < 0.0f ? 0.0f : acc[r];
  }
  const float* wmu = anet + ah;
  const float* bmu = wmu + act_w * H;
  const float* wsd = bmu + act_w;
  const float* bsd = wsd + act_w * H;
  mlp_group_layer(acc, is_actor, wmu, bmu, wsd, bsd, act_w, 2 * act_w, H, false, mW, sXc, sC + myrow * H, H, t, gather);
  if (is_actor && lane < 2 * act_w) {
    const int col = lane < act_w ? lane : PEDN_ACTOR_MAX_ACT + lane - act_w;
#pragma unroll
    for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) sOut[(vrow + r) * 2 * PEDN_ACTOR_MAX_ACT + col] = acc[r];
  }
  __syncthreads();

  // (the group once more, behind an empty asm: what the tails and the critics' fc derive from it is formed here, not held in SGPRs through
  // the forward, where they spilled)
  int g2 = g;
  asm volatile("" : "+s"(g2));
  const bool actor2 = g2 == 2;
  float* mW2 = sW[g2];
  // ---- section 15's tail on a lane per (row, action) of the actor's group; what the backward's tail needs of it waits in LDS
  const int tr = t / act_w, tj = t - tr * act_w;
  const bool pair = actor2 && tr < PEDN_GRAD_TILE;
  const bool live = tr < nrows;
  if (pair) {
    const float mu = sOut[tr * 2 * PEDN_ACTOR_MAX_ACT + tj], z = sOut[tr * 2 * PEDN_ACTOR_MAX_ACT + PEDN_ACTOR_MAX_ACT + tj];
    float eps = 0.0f;
    const int col = act0 + tj;
    ActorGradLate la = ag_late_args();
    const size_t at = (size_t)(row0 + tr) * la->n_actions + col;
    const float sd = mlp_softplus(z);
    if (given) {
      if (live) eps = la->noise[at];
    } else
      eps = philox_normal(la->k0, la->k1, (uint32_t)(row0 + tr), la->state[0], PEDN_AG_NOISE_SITE | ((uint32_t)col << 8));
    const float u = mu + sd * eps;
    __builtin_amdgcn_sched_barrier(0);   // (one double-precision function at a time: interleaved, their temporaries cost a VGPR too many)
    const float th = (float)tanh((double)u);
    __builtin_amdgcn_sched_barrier(0);
    const float na = th * la->max_delta;
    // Normal(mu, std).log_prob(u) - log(1 - tanh(tanh(u))^2 + 1e-7): the reference squashes the squashed action once more (SAC.py:353)
    const double T2 = tanh((double)th);
    __builtin_amdgcn_sched_barrier(0);
    const float logp = (float)(normal_log_prob(u, mu, sd) - log(1.0 - T2 * T2 + 1e-7));
    sAct[tr * PEDN_ACTOR_MAX_ACT + tj] = na;
    sLogp[tr * PEDN_ACTOR_MAX_ACT + tj] = logp;
    sTail[0][tr * PEDN_ACTOR_MAX_ACT + tj] = sd;
    sTail[1][tr * PEDN_ACTOR_MAX_ACT + tj] = eps;
    sTail[2][tr * PEDN_ACTOR_MAX_ACT + tj] = th;
    if (live) {
      float* o = la->out_actions + at;
      const size_t plane = (size_t)a.B * la->n_actions;
      o[0] = mu; o[plane] = sd; o[2 * plane] = eps; o[3 * plane] = logp; o[4 * plane] = na;
      o[5 * plane] = z; o[6 * plane] = th;
    }
  }
  if (!actor2) {
    if (t < PEDN_GRAD_TILE) {   // the newest frame's last column of the agent; zeros in rows past B and behind the row's end
      const size_t row = (size_t)(row0 + t);
      sF[g2][t * PEDN_GRAD_FEAT + H + act_w] = t < nrows ? a.s[(row * a.S + (a.S - 1)) * a.n_obs + obs0 + obs_w - 1] : 0.0f;
      for (int j = K3; j < PEDN_GRAD_FEAT; ++j) sF[g2][t * PEDN_GRAD_FEAT + j] = 0.0f;
    }
    if (w4 == 3) sWo[g2][lane] = net[at4 + lane];
  }
  __syncthreads();   // new_action and logp are there
  if (actor2) {
    if (t < PEDN_GRAD_TILE) {
      float ent = 0.0f;
      for (int j = 0; j < act_w; ++j) ent = ent - sLogp[t * PEDN_ACTOR_MAX_ACT + j];
      sEnt[t] = ent;
      if (t < nrows) {
        ActorGradLate la = ag_late_args();
        la->out_agents[(size_t)(row0 + t) * la->n_agents + agent] = ent;
      }
    }
  } else if (tr < PEDN_GRAD_TILE)
    sF[g2][tr * PEDN_GRAD_FEAT + H + tj] = sAct[tr * PEDN_ACTOR_MAX_ACT + tj];
  // ---- the critics' fc and fc_out on (states, new_action): section 15's arithmetic, section 18's q
  mlp_group_layer(acc, !actor2, net + at3, net + at3 + H * K3, net + at3, net + at3 + H * K3, H, H, K3, false, mW2, sXc,
           sF[actor2 ? 0 : g2] + myrow * PEDN_GRAD_FEAT, PEDN_GRAD_FEAT, t, gather);
  if (!actor2) {
#pragma unroll
    for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) sD[g2][(vrow + r) * PEDN_GRAD_DS + lane] = acc[r];   // (no ReLU behind fc, as in the reference)
  }
  __syncthreads();
  if (!actor2) {
    if (lane < PEDN_GRAD_WAVE_ROWS) {   // fc_out on a lane per row, section 15's chain
      const int r = myrow + lane;
      float q = net[at4 + H];
      for (int k = 0; k < H; ++k) q = q + sWo[g2][k] * sD[g2][r * PEDN_GRAD_DS + k];
      sQ[g2][r] = q;
      if (r < nrows) {
        ActorGradLate la = ag_late_args();
        la->out_agents[((size_t)(1 + g2) * a.B + row0 + r) * la->n_agents + agent] = q;
      }
    } else if (w4 == 1 && lane - PEDN_GRAD_WAVE_ROWS < act_w) {
      // d q / d action_j = sum over o ascending of fc_out[o] * fc[o][64 + j], from +0.0, in double (64 terms that cancel: in float32 this
      // sum alone carried the gradient's error); fc's last chunk (columns 64 ..) is still staged
      const int j = lane - PEDN_GRAD_WAVE_ROWS;
      double v = 0.0;
      for (int o = 0; o < H; ++o) v = v + (double)sWo[g2][o] * (double)mW2[o * PEDN_GRAD_PAD + j];
      sV[g2][j] = v;
    }
  }
  __syncthreads();   // q1, q2 and the critics' vectors are there
  float* mD = sD[2];
  if (actor2) {
    ActorGradLate la = ag_late_args();
    const int B = la->B;
    const float alpha = (float)exp((double)la->log_alpha[agent]);
    if (t < PEDN_GRAD_TILE) {
      const float q1 = sQ[0][t], q2 = sQ[1][t];
      const float q = (q2 < q1 || q2 != q2) ? q2 : q1;   // torch.min: NaN wins
      sL[0][t] = -(alpha * sEnt[t]) - q;
      sL[1][t] = sEnt[t] - la->tent[agent];
    }
    if (pair) {
      // the backward's tail: d actor_loss / d mu and / d (the pre-softplus value) of this (row, action), in double, rounded once
      float gmu = 0.0f, gz = 0.0f;
      if (live) {
        const float q1 = sQ[0][tr], q2 = sQ[1][tr];
        const float z = sOut[tr * 2 * PEDN_ACTOR_MAX_ACT + PEDN_ACTOR_MAX_ACT + tj];
        const float sd = sTail[0][tr * PEDN_ACTOR_MAX_ACT + tj], eps = sTail[1][tr * PEDN_ACTOR_MAX_ACT + tj], th = sTail[2][tr * PEDN_ACTOR_MAX_ACT + tj];
        // torch.minimum's backward: the smaller one takes the gradient, equal ones half each (and both all of it beside a NaN)
        const double w1 = q1 > q2 ? 0.0 : (q1 == q2 ? 0.5 : 1.0), w2 = q1 < q2 ? 0.0 : (q1 == q2 ? 0.5 : 1.0);
        const double G = 1.0 / (double)B;
        const double dqa = w1 * sV[0][tj] + w2 * sV[1][tj];
        const double Dt = 1.0 - (double)th * (double)th;
        __builtin_amdgcn_sched_barrier(0);
        const double T = tanh((double)th), omT = 1.0 - T * T;
        __builtin_amdgcn_sched_barrier(0);
        const double dlp = (double)alpha * G;
        const double gu = (dlp * (2.0 * T * omT / (omT + 1e-7)) - G * dqa * (double)la->max_delta) * Dt;
        const double gsd = gu * (double)eps - dlp / (double)sd;   // Normal's paths via u and mu cancel; via std they leave -1 / std
        __builtin_amdgcn_sched_barrier(0);
        const double sp = z > 20.0f ? 1.0 : 1.0 / (1.0 + exp(-(double)z));
        gmu = (float)gu;
        gz = (float)(gsd * sp);
      }
      mD[tr * PEDN_GRAD_DS + tj] = gmu;
      mD[tr * PEDN_GRAD_DS + act_w + tj] = gz;
      if (live) {
        const size_t plane = (size_t)B * la->n_actions;
        float* o = la->out_actions + (size_t)(row0 + tr) * la->n_actions + act0 + tj;
        o[7 * plane] = gmu; o[8 * plane] = gz;
      }
    }
  }
  __syncthreads();
  // the tile's row of the workspace, and the actor's heads again: formed here, behind the forward, which has no SGPRs to hold them
  ActorGradLate lb = ag_late_args();
  float* wrow = lb->ws + (size_t)blockIdx.x * lb->ws_stride;
  float* gws = wrow + lb->table[(size_t)agent * PEDN_ACTOR_TABLE_COLS + 4];
  if (tid < 2) {   // the tile's two sums, rows ascending
    float v = 0.0f;
    for (int r = 0; r < nrows; ++r) v = v + sL[tid][r];
    wrow[lb->pack4 + 2 * agent + tid] = v;
  }
  int ahb = ah;
  asm volatile("" : "+s"(ahb));
  const float* hmu = anet + ahb;
  const float* hsd = hmu + act_w * H + act_w;

  // ---- backward through the actor, all waves.  The heads: a thread per weight, then h3's gradient behind the ReLU mask into sD[0]
  mlp_grad_heads_tile<false>(mD, PEDN_GRAD_DS, sC, act_w, nrows, gws + ah, true, tid, PEDN_AG_THREADS);
  float* dD = sD[0];
  for (int idx = tid; idx < PEDN_GRAD_TILE * H; idx += PEDN_AG_THREADS) {
    const int r = idx >> 6, k = idx & 63;
    float v = 0.0f;
    for (int o = 0; o < 2 * act_w; ++o) v = v + mD[r * PEDN_GRAD_DS + o] * (o < act_w ? hmu[o * H + k] : hsd[(o - act_w) * H + k]);
    dD[r * PEDN_GRAD_DS + k] = sC[idx] > 0.0f ? v : 0.0f;
  }
  // fc, the mask, encoder.fc2, the mask, encoder.fc1
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  float dx[4];
  mlp_grad_dw_tile<4, false>(dD, PEDN_GRAD_DS, sB, H, H, nrows, gws + at3, gws + at3 + H * H, sW[0], false, true, wv < 8, 8, tid, PEDN_AG_THREADS, gather);
  mlp_grad_dx_tile(dx, wv < 8, dD + 4 * wv * PEDN_GRAD_DS, PEDN_GRAD_DS, anet + at3, H, sW[1], tid, PEDN_AG_THREADS);
  __syncthreads();   // every wave has read the output gradient that is overwritten now
  if (wv < 8) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dD[(4 * wv + r) * PEDN_GRAD_DS + lane] = sB[(4 * wv + r) * H + lane] > 0.0f ? dx[r] : 0.0f;
  }
  mlp_grad_dw_tile<4, false>(dD, PEDN_GRAD_DS, sA[2], H, H, nrows, gws + at2, gws + at2 + H * H, sW[0], false, true, wv < 8, 8, tid, PEDN_AG_THREADS, gather);
  mlp_grad_dx_tile(dx, wv < 8, dD + 4 * wv * PEDN_GRAD_DS, PEDN_GRAD_DS, anet + at2, H, sW[1], tid, PEDN_AG_THREADS);
  __syncthreads();
  if (wv < 8) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dD[(4 * wv + r) * PEDN_GRAD_DS + lane] = sA[2][(4 * wv + r) * H + lane] > 0.0f ? dx[r] : 0.0f;
  }
  mlp_grad_dw_tile<4, false>(dD, PEDN_GRAD_DS, sXc, PEDN_ACTOR_CHUNK, K1, nrows, gws, gws + H * K1, sW[0], true, true, wv < 8, 8, tid, PEDN_AG_THREADS, gather);
  if (given) return;
  __syncthreads();   // the tail's lanes have read the draw counter
  if (tid == 0) {
    int64_t* state = ag_late_args()->state;
    advance_draw_counter(state, state[0]);
  }
}

struct ActorAdamArgs {
  const float* ws;             // the workspace, rows of ws_stride floats
  float* grads;                // the gradient pack
  float* m;                    // exp_avg
  float* v;                    // exp_avg_sq
  float* p;                    // the actors' pack
  float* log_alpha;            // [n_agents]
  float* alpha_mv;             // [2][n_agents]: exp_avg and exp_avg_sq of log_alpha
  float* scalars;              // [3][n_agents]: actor_loss, alpha_loss, alpha_grad
  int64_t* state;              // pedn_adam.hpp's step state
  int64_t n, pack4, ws_stride; // floats: the pack's length, where a workspace row's sums start, a workspace row's length
  int32_t tiles, n_agents, B, do_adam;
  double lr, alpha_lr, beta1, beta2;
  AdamCoef coef;
};

__global__ __launch_bounds__(256) void sacactor_adam_kernel(ActorAdamArgs a) {
  const AdamStep st = adam_step_begin(a.state, a.beta1, a.beta2);
  const float nstep = adam_nstep(a.lr, st), nstep_alpha = adam_nstep(a.alpha_lr, st), s = st.s;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = gid; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    float g = 0.0f;
    for (int tl = 0; tl < a.tiles; ++tl) g = g + a.ws[(int64_t)tl * a.ws_stride + i];   // tiles ascending
    a.grads[i] = g;
    if (a.do_adam) {
      float m = a.m[i], v = a.v[i];
      const float p = adam_one<true>(g, m, v, a.p[i], a.coef, nstep, s);
      a.m[i] = m; a.v[i] = v; a.p[i] = p;
    }
  }
  if (gid < (int64_t)a.n_agents) {   // the two means, the temperature's loss and gradient, and its step
    float l = 0.0f, e = 0.0f;
    for (int tl = 0; tl < a.tiles; ++tl) {
      l = l + a.ws[(int64_t)tl * a.ws_stride + a.pack4 + 2 * gid];
      e = e + a.ws[(int64_t)tl * a.ws_stride + a.pack4 + 2 * gid + 1];
    }
    const float alpha = (float)exp((double)a.log_alpha[gid]);
    const float ga = alpha * (e / (float)a.B);
    a.scalars[gid] = l / (float)a.B;
    a.scalars[a.n_agents + gid] = ga;       // alpha_loss = mean((entropy - target) * alpha): the same number as its gradient
    a.scalars[2 * a.n_agents + gid] = ga;
    if (a.do_adam) {
      float m = a.alpha_mv[gid], v = a.alpha_mv[a.n_agents + gid];
      const float p = adam_one<true>(ga, m, v, a.log_alpha[gid], a.coef, nstep_alpha, s);
      a.alpha_mv[gid] = m; a.alpha_mv[a.n_agents + gid] = v; a.log_alpha[gid] = p;
    }
  }
  if (!a.do_adam) return;
  __syncthreads();   // every wave of the workgroup has read the step state
  if (threadIdx.x == 0) adam_step_advance(a.state, st, gridDim.x);   // the last workgroup advances the state
}

// ---- host side: pedn_sac_actor_update of include/pedn.h; no state in the engine's handle
int pedn_sac_actor_update(const float* states, const float* noise, const int32_t* table, const int32_t* critic_table, float* actor_params,
                          const float* online_params, float* log_alpha, const float* target_entropy, float* grads, float* exp_avg,
                          float* exp_avg_sq, float* alpha_moments, float* workspace, float* out_actions, float* out_agents, float* scalars,
                          int64_t* adam_state, int64_t* draw_state, int64_t pack_floats, int32_t batch, int32_t stack_size, int32_t n_obs,
                          int32_t n_actions, int32_t n_agents, int32_t hidden_size, double max_delta, double actor_lr, double alpha_lr,
                          double beta1, double beta2, double eps, uint64_t seed, int32_t do_adam, void* stream) {
  if (!states || !table || !critic_table || !actor_params || !online_params || !log_alpha || !target_entropy || !grads || !exp_avg || !exp_avg_sq ||
      !alpha_moments || !workspace || !out_actions || !out_agents || !scalars || !adam_state || !draw_state)
    return fail(nullptr, PEDN_E_ARG, "null argument");
  if (const char* why = update_refusal(
          hidden_size, "the SAC actor kernels are built for hidden_size 64", batch >= 1 && stack_size >= 1 && n_obs >= 1 && n_actions >= 1, n_agents,
          "batch, stack_size, n_obs, n_actions and n_agents must be positive (at most 65535 agents)", nullptr, pack_floats >= 1,
          "the actors' pack is empty",
          (uintptr_t)actor_params | (uintptr_t)online_params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)workspace,
          actor_lr, alpha_lr, beta1, beta2, eps))
    return fail(nullptr, PEDN_E_ARG, why);
  const int tiles = (batch + PEDN_GRAD_TILE - 1) / PEDN_GRAD_TILE;
  const int64_t pack4 = (pack_floats + 3) / 4 * 4;
  const int64_t ws_stride = pack4 + (2 * (int64_t)n_agents + 3) / 4 * 4;
  ActorGradArgs a{};
  a.s = states; a.noise = noise; a.table = table; a.ctable = critic_table; a.actor = actor_params; a.online = online_params;
  a.log_alpha = log_alpha; a.tent = target_entropy; a.ws = workspace; a.out_actions = out_actions; a.out_agents = out_agents;
  a.state = draw_state; a.pack4 = pack4; a.ws_stride = ws_stride;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
  a.B = batch; a.S = stack_size; a.n_obs = n_obs; a.n_actions = n_actions; a.n_agents = n_agents;
  a.max_delta = (float)max_delta;
  hipLaunchKernelGGL(sacactor_grad_kernel, dim3((unsigned)tiles, (unsigned)n_agents), dim3(PEDN_AG_THREADS), 0, (hipStream_t)stream, a);
  HIP_TRY(nullptr, hipGetLastError());
  ActorAdamArgs b{};
  b.ws = workspace; b.grads = grads; b.m = exp_avg; b.v = exp_avg_sq; b.p = actor_params; b.log_alpha = log_alpha; b.alpha_mv = alpha_moments;
  b.scalars = scalars; b.state = adam_state; b.n = pack_floats; b.pack4 = pack4; b.ws_stride = ws_stride;
  b.tiles = tiles; b.n_agents = n_agents; b.B = batch; b.do_adam = do_adam ? 1 : 0;
  b.lr = actor_lr; b.alpha_lr = alpha_lr; b.beta1 = beta1; b.beta2 = beta2;
  b.coef = adam_coef(beta1, beta2, eps);
  int64_t blocks = (b.n + 255) / 256;
  const int64_t need = ((int64_t)n_agents + 255) / 256;   // the agents' scalars have a thread each
  blocks = blocks < need ? need : blocks < 2048 ? blocks : 2048;
  hipLaunchKernelGGL(sacactor_adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, b);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}
