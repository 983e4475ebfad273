// One epoch of the reference's PPOAgent.update loop (rl/agents/PPO_org.py:579-629) for its recurrent agents (LSTMPolicyNetwork /
// LSTMValueNetwork, use_stacked_obs=False): both forwards over every env's whole sequence, the clipped surrogate and the MSE value loss,
// back-propagation through time, clip_grad_norm_ of each network, two Adam steps and the KL early stop, for a whole rollout and every
// agent.  The contract is DESIGN section 21; tests/lstm_update_model.py restates it in numpy.  The work is split at its only sequential
// dependency, the walk through time:
//
// lstmgrad_seq_fwd_kernel grid (ceil(N / 32), n_agents, 2), 256 threads.  blockIdx.z = 0 is the value network, 1 the actor.  A workgroup
//                         takes one agent, one network and a tile of PEDN_LG_ENV_TILE = 32 envs and walks t ascending from a zero state
//                         in lstm_seq_kernel's arrangement (a wave per 8 envs, a lane per hidden unit, c in registers, h in LDS, section
//                         17's step operation for operation); it writes log_probs / values, the loss' tail (pedn_ppo_loss.hpp: std, d_mu,
//                         d_z, -min(surr1, surr2)) and per row h', c' and the four activated gates into the workspace.
//                         LDS: lstm_seq_kernel's 256 * 33 + 32 * 32 + 2 * 32 * 64 + 32 * 16 words = 56320 bytes: 2 workgroups per CU, 2
//                         waves per SIMD.
// lstmgrad_seq_bwd_kernel the same grid, t descending.  W_hh is staged once, transposed, and stays in LDS; a step is the cell's lines on
//                         a lane per unit, which overwrite the row's gates with the pre-activation gradients a[t] (256 floats), and
//                         dh_rec = a W_hh as one chain over the 256 gate rows (mlp_mac with the operands' roles exchanged).  No weight
//                         gradient is in the loop.  (One kernel for both directions carried the forward's scalars through the
//                         backward: 69 SGPRs spilled, and 3 to 9 under every arrangement tried; apart, neither spills.)
//                         LDS: 32 * 260 + 64 * 257 + 32 * 16 words = 101120 bytes: one workgroup per CU, 1 wave per SIMD (the grid is
//                         N / 32 * n_agents * 2 workgroups: 128 for one agent at 2048 envs).
// lstmgrad_dw_kernel      grid (G, n_agents, 2), 256 threads, G = min(tiles, groups): section 20's row-tile arrangement over all R = T * N
//                         rows r = t * N + e.  Per tile of 32 rows it stages a, h[t - 1] (+0.0 at t = 0) and relu(h'), gathers x, and forms
//                         dW_ih, dW_hh, db_ih, db_hh (mlp_grad_dw_tile, a gate's 64 rows at a time), the heads' gradients
//                         (mlp_grad_heads_tile / section 20's value-loss lines) and the tile's three sums in double into the group's slab.
//                         LDS: 32 * 260 + 32 * 32 + 2 * 32 * 64 + 64 * 33 + 32 * 16 + 2 * 32 * 8 + 2 * 32 words = 66560 bytes: 2 workgroups
//                         per CU, 2 waves per SIMD.
// lstmgrad_reduce_kernel  grid (16, n_agents, 2): pedn_ppo_loss.hpp's pg_reduce_body on the recurrent networks' ranges.
// lstmgrad_adam_kernel    grid (16, n_agents, 2): pedn_ppo_loss.hpp's pg_adam_body.
// The stop flags are cleared by section 20's ppograd_begin_kernel.  A workgroup of an agent whose stop flag is set leaves at once, in all five.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_lstm.hpp"
#include "pedn_mlp_grad.hpp"
#include "pedn_ppo_grad.hpp"
#include "pedn_ppo_loss.hpp"

#define PEDN_LG_ENV_TILE PEDN_ACTOR_TILE              // envs per workgroup of the sequential launch (not part of the order of any sum yet)
#define PEDN_LG_ROW (6 * PEDN_ACTOR_HIDDEN)           // floats per (network, agent, row) of the activations: h', c', i, f, g, o (then a_i .. a_o)
#define PEDN_LG_A (2 * PEDN_ACTOR_HIDDEN)             // where the gates (and a) start in a row
#define PEDN_LG_AS (PEDN_LSTM_ROWS + 4)               // words of a staged row of a: 16-byte aligned rows, 8 rows on 8 banks
#define PEDN_LG_WT (PEDN_LSTM_ROWS + 1)               // words of a row of the transposed W_hh: odd, so that a lane per row reads conflict-free
#define PEDN_LG_TAIL 4                                // planes [R][n_actions] of the tail: std, d_mu, d_z, -min(surr1, surr2)
#define PEDN_LG_DS 16                                 // words of a row of the heads' output gradient: d_mu[act_w], d_z[act_w]; a value network's dv

struct LstmGradArgs {
  const float* obs;        // [T + 1][N][n_obs]
  const void* actions;     // [T][N][n_actions], float or double
  const float* old_logp;   // [T][N][n_actions]
  const float* adv;        // [T][N][n_agents]
  const float* td;         // [T][N][n_agents]
  const int32_t* table;    // [n_agents][PEDN_ACTOR_TABLE_COLS]: the actors' table
  const int32_t* vtable;   // [n_agents]: offsets (floats) in the value pack
  const float* actor;      // the actors' pack
  const float* value;      // the value pack
  const int32_t* flags;    // [n_agents]: the stop flags
  float* act;              // [2][n_agents][R][PEDN_LG_ROW]: the activations (0: the value networks', 1: the actors')
  float* tail;             // [PEDN_LG_TAIL][R][n_actions]
  float* ws;               // [G][ws_stride]: section 20's slabs in the layout of the two packs
  float* logp;             // [T][N][n_actions]
  float* values;           // [T][N][n_agents]
  int64_t rows, tiles;     // R = T * N and ceil(R / 32)
  int64_t apack4, vpack, ws_stride;
  int32_t T, N, n_obs, n_actions, n_agents, act_f64;
  float min_std, max_std, clip_lo, clip_hi;
  float vscale;            // (float)(2.0 / R)
};

// The launch's arguments as the kernel argument segment holds them, taken again behind an empty asm where they are used: what is derived
// from them is formed there and not held in scalar registers through the loops over t.  This reads the segment as ONE LstmGradArgs at
// offset 0: a kernel that uses it takes the struct as its only parameter (ppograd_kernel's PpoGradLate is the same arrangement).
typedef const __attribute__((address_space(4))) LstmGradArgs* LstmGradLate;
#define PEDN_LG_LATE(name)                                                   \
  LstmGradLate name = (LstmGradLate)__builtin_amdgcn_kernarg_segment_ptr(); \
  asm volatile("" : "+s"(name))

// where a recurrent network lies in its pack and how long it is: lstm.weight_ih, weight_hh, bias_ih, bias_hh, then the heads
__device__ __forceinline__ void lg_net_range(const int32_t* table, const int32_t* vtable, int agent, bool is_actor, int& off, int& len) {
  const int32_t* tb = table + (size_t)agent * PEDN_ACTOR_TABLE_COLS;
  const int H = PEDN_ACTOR_HIDDEN, lstm = PEDN_LSTM_ROWS * (tb[1] + H + 2);
  off = is_actor ? tb[4] : vtable[agent];
  len = is_actor ? lstm + 2 * (tb[3] * H + tb[3]) : lstm + H + 1;
}

// What a thread of the two sequential kernels is: lane k owns unit k of every slot of its wave's 8 rows in the activations, in both
// directions; the tail's lane is (row le of the wave, action j) with the actor, row `lane` with a value network.
template <bool ACTOR>
struct LstmGradLane {
  int wenv0;       // the wave's first env, a scalar value: which of its rows are under N is a scalar comparison, not a mask per row in an SGPR pair
  float* actw;     // this lane's unit of the wave's row 0 at step 0; a row is PEDN_LG_ROW floats, a step N rows
  int le, j;
  unsigned env;
  bool mine;
  size_t at;       // the tail lane's element of step 0's row in log_probs / values
  __device__ __forceinline__ LstmGradLane(const LstmGradArgs& a, int act0, int act_w) {
    const int lane = (int)(threadIdx.x & 63), agent = (int)blockIdx.y;
    wenv0 = (int)(blockIdx.x * PEDN_LG_ENV_TILE) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * PEDN_ACTOR_WAVE_ENVS;
    actw = a.act + (((size_t)(ACTOR ? 1 : 0) * (size_t)a.n_agents + (size_t)agent) * (size_t)a.rows + (size_t)wenv0) * PEDN_LG_ROW + lane;
    le = ACTOR ? lane / act_w : lane;
    j = ACTOR ? lane - le * act_w : 0;
    env = (unsigned)(wenv0 + le);
    mine = le < PEDN_ACTOR_WAVE_ENVS && env < (unsigned)a.N;
    at = (size_t)env * (size_t)(ACTOR ? a.n_actions : a.n_agents) + (size_t)(ACTOR ? act0 + j : agent);
  }
};

// One network of lstmgrad_seq_fwd_kernel for the workgroup's tile of envs: section 17's step over t ascending from a zero state, with what
// the backward needs kept.
template <bool ACTOR>
__device__ __forceinline__ void lstmgrad_fwd_role(const LstmGradArgs& a, float* sW, float* sXc, float* sHs, float* sH, float* sOut) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int H = PEDN_ACTOR_HIDDEN;
  const int agent = (int)blockIdx.y;
  const int32_t* t = a.table + (size_t)agent * PEDN_ACTOR_TABLE_COLS;
  const int obs0 = t[0], obs_w = t[1], act0 = t[2], act_w = t[3];
  const unsigned env0 = blockIdx.x * PEDN_LG_ENV_TILE;
  const float* p = ACTOR ? a.actor + t[4] : a.value + a.vtable[agent];
  const float* rest = p + (size_t)PEDN_LSTM_ROWS * (obs_w + H + 2);   // mean_head (then std_head), or value_head
  const LstmGradLane<ACTOR> me(a, act0, act_w);
  const float* frame = a.obs;
  // input k of the tile's env e at the step is frame[env0 + e][obs0 + k]; rows behind N read zeros
  const auto gather = [&](int c0, int kmax) {
    for (int idx = (int)threadIdx.x; idx < PEDN_ACTOR_TILE * PEDN_ACTOR_CHUNK; idx += 256) {
      const unsigned e = (unsigned)idx / PEDN_ACTOR_CHUNK, kk = (unsigned)idx % PEDN_ACTOR_CHUNK;
      float x = 0.0f;
      PEDN_LG_LATE(lg);
      if ((int)kk < kmax && env0 + e < (unsigned)lg->N) x = frame[(size_t)(env0 + e) * (size_t)lg->n_obs + (size_t)(obs0 + c0 + (int)kk)];
      sXc[idx] = x;
    }
  };
  float* hs = sHs + wave * PEDN_ACTOR_WAVE_ENVS * H + lane;
  float c[PEDN_ACTOR_WAVE_ENVS];
#pragma unroll
  for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) {
    hs[r * H] = 0.0f;
    c[r] = 0.0f;
  }
  float acc[PEDN_LSTM_GATES][PEDN_ACTOR_WAVE_ENVS], bias[PEDN_LSTM_GATES];
  lstm_bias(bias, p, obs_w);
  const int T = a.T;
  for (int step = 0; step < T; ++step) {
    {
      PEDN_LG_LATE(lf);
      frame = lf->obs + (size_t)step * (size_t)lf->N * (size_t)lf->n_obs;   // row 0 of the step's frame
    }
    lstm_gates(acc, bias, p, obs_w, sW, sXc, sHs, gather);
    {
      PEDN_LG_LATE(lk);
      const int live = (int)lk->N - me.wenv0;   // rows of the wave under N (not positive: none)
      float* keep_at = me.actw + (size_t)step * (size_t)lk->N * PEDN_LG_ROW;
      lstm_cell_keep(acc, c, hs, sH + wave * PEDN_ACTOR_WAVE_ENVS * H + lane, [&](int r, float gi, float gf, float gg, float go, float cc, float hh) {
        if (r < live) {
          float* w = keep_at + (size_t)r * PEDN_LG_ROW;
          w[0] = hh; w[H] = cc; w[2 * H] = gi; w[3 * H] = gf; w[4 * H] = gg; w[5 * H] = go;
        }
      });
    }
    if (!ACTOR) {
      __syncthreads();   // (the wave's own rows; the barrier orders the LDS writes before the reads)
      PEDN_LG_LATE(lv);
      if (me.mine)
        lv->values[me.at + (size_t)step * (size_t)lv->N * (size_t)lv->n_agents] = lstm_value_head(rest, sH + (wave * PEDN_ACTOR_WAVE_ENVS + lane) * H);
      continue;
    }
    const float* so = mlp_heads(acc[0], rest, act_w, sW, sXc, sH, sOut, gather);
    if (me.mine) {
      PEDN_LG_LATE(lt);
      const size_t o_at = me.at + (size_t)step * (size_t)lt->N * (size_t)lt->n_actions, plane = (size_t)lt->rows * (size_t)lt->n_actions;
      const float mu = so[me.le * 2 * PEDN_ACTOR_MAX_ACT + me.j], z = so[me.le * 2 * PEDN_ACTOR_MAX_ACT + PEDN_ACTOR_MAX_ACT + me.j];
      const float act = lt->act_f64 ? (float)static_cast<const double*>(lt->actions)[o_at] : static_cast<const float*>(lt->actions)[o_at];
      const float A = lt->adv[((size_t)step * (size_t)lt->N + (size_t)me.env) * (size_t)lt->n_agents + (size_t)agent];
      const PpoTailElem te = ppo_loss_tail(mu, z, act, lt->old_logp[o_at], A, lt->min_std, lt->max_std, lt->clip_lo, lt->clip_hi,
                                           -1.0 / ((double)lt->rows * (double)act_w));
      lt->logp[o_at] = te.lp;
      float* o = lt->tail + o_at;
      o[0] = te.sd; o[plane] = te.gmu; o[2 * plane] = te.gz; o[3 * plane] = te.el;
    }
  }
}

// (LstmGradArgs is the ONLY parameter of the three kernels below, at offset 0 of the kernel argument segment: PEDN_LG_LATE reads it there)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void lstmgrad_seq_fwd_kernel(LstmGradArgs a) {
  __shared__ float sW[PEDN_LSTM_ROWS * (PEDN_ACTOR_CHUNK + 1)];
  __shared__ __attribute__((aligned(16))) float sXc[PEDN_ACTOR_TILE * PEDN_ACTOR_CHUNK];
  __shared__ __attribute__((aligned(16))) float sHs[PEDN_ACTOR_TILE * PEDN_ACTOR_HIDDEN];
  __shared__ __attribute__((aligned(16))) float sH[PEDN_ACTOR_TILE * PEDN_ACTOR_HIDDEN];
  __shared__ float sOut[PEDN_ACTOR_TILE * 2 * PEDN_ACTOR_MAX_ACT];
  if (a.flags[blockIdx.y] != 0) return;   // the agent has stopped: before any barrier, nothing is written
  if (blockIdx.z != 0)
    lstmgrad_fwd_role<true>(a, sW, sXc, sHs, sH, sOut);
  else
    lstmgrad_fwd_role<false>(a, sW, sXc, sHs, sH, sOut);
}

// One network of lstmgrad_seq_bwd_kernel for the workgroup's tile of envs: back through time, t descending.  sA: a of the tile's 32 rows at
// the step; sT: W_hh transposed, sT[k * 257 + q] = W_hh[q][k], staged once; sD: the heads' output gradient of the tile's rows.
template <bool ACTOR>
__device__ __forceinline__ void lstmgrad_bwd_role(const LstmGradArgs& a, float* sA, float* sT, float* sD) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int H = PEDN_ACTOR_HIDDEN;
  const int agent = (int)blockIdx.y;
  const int32_t* t = a.table + (size_t)agent * PEDN_ACTOR_TABLE_COLS;
  const int obs_w = t[1], act0 = t[2], act_w = t[3];
  const float* p = ACTOR ? a.actor + t[4] : a.value + a.vtable[agent];
  const float* rest = p + (size_t)PEDN_LSTM_ROWS * (obs_w + H + 2);   // mean_head (then std_head), or value_head
  const LstmGradLane<ACTOR> me(a, act0, act_w);
  {
    const float* whh = p + (size_t)PEDN_LSTM_ROWS * obs_w;
    for (int idx = (int)threadIdx.x; idx < PEDN_LSTM_ROWS * H; idx += 256) {
      const int q = idx >> 6, k = idx & 63;
      sT[k * PEDN_LG_WT + q] = whh[idx];
    }
  }
  float dh_rec[PEDN_ACTOR_WAVE_ENVS], dc_rec[PEDN_ACTOR_WAVE_ENVS];
#pragma unroll
  for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) dh_rec[r] = dc_rec[r] = 0.0f;
  int cnt = PEDN_LSTM_ROWS;
  asm volatile("" : "+s"(cnt));   // (no instruction: the count stays a run-time value, see mlp_grad_dx)
  const float* hmu = rest;
  const float* hsd = hmu + act_w * H + act_w;
  const float* sDw = sD + wave * PEDN_ACTOR_WAVE_ENVS * PEDN_LG_DS;
  for (int step = a.T - 1; step >= 0; --step) {
    __syncthreads();   // the step before is done with sA and sD (the first time: W_hh is staged)
    if (me.le < PEDN_ACTOR_WAVE_ENVS) {
      PEDN_LG_LATE(lb);
      const size_t o_at = me.at + (size_t)step * (size_t)lb->N * (size_t)(ACTOR ? lb->n_actions : lb->n_agents);
      const size_t plane = (size_t)lb->rows * (size_t)lb->n_actions;
      float* d = sD + (wave * PEDN_ACTOR_WAVE_ENVS + me.le) * PEDN_LG_DS;
      if (ACTOR) {
        d[me.j] = me.mine ? lb->tail[plane + o_at] : 0.0f;
        d[act_w + me.j] = me.mine ? lb->tail[2 * plane + o_at] : 0.0f;
      } else {
        d[0] = me.mine ? (lb->values[o_at] - lb->td[o_at]) * lb->vscale : 0.0f;   // dv = (v - td) * (float)(2 / R)
      }
    }
    __syncthreads();
    // the gradient that reaches h' from the heads, before the ReLU's mask
    float dy[PEDN_ACTOR_WAVE_ENVS];
    if (ACTOR) {
#pragma unroll
      for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) dy[r] = 0.0f;
      for (int o = 0; o < 2 * act_w; ++o) {
        const float w = o < act_w ? hmu[o * H + lane] : hsd[(o - act_w) * H + lane];
#pragma unroll
        for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) dy[r] = dy[r] + sDw[r * PEDN_LG_DS + o] * w;
      }
    } else {
      const float wl = rest[lane];
#pragma unroll
      for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) dy[r] = sDw[r * PEDN_LG_DS] * wl;
    }
    PEDN_LG_LATE(lc);
    const size_t act_step = (size_t)lc->N * PEDN_LG_ROW;
    float* row = me.actw + (size_t)step * act_step;
    const int live = (int)lc->N - me.wenv0;   // rows of the wave under N (not positive: none)
#pragma unroll
    for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) {
      float a_i = 0.0f, a_f = 0.0f, a_g = 0.0f, a_o = 0.0f;
      if (r < live) {
        float* w = row + (size_t)r * PEDN_LG_ROW;
        const float hp = w[0], cc = w[H], gi = w[2 * H], gf = w[3 * H], gg = w[4 * H], go = w[5 * H];
        const float c_prev = step > 0 ? (w - act_step)[H] : 0.0f;
        const float tc = lstm_tanh(cc);
        const float dhh = hp > 0.0f ? dy[r] : 0.0f;
        const float dh = dhh + dh_rec[r];
        const float d_o = dh * tc;
        const float dtc = dh * go;
        const float u = 1.0f - tc * tc;
        float dc = dtc * u;
        dc = dc + dc_rec[r];
        const float d_i = dc * gg;
        const float d_g = dc * gi;
        const float d_f = dc * c_prev;
        dc_rec[r] = dc * gf;
        a_i = d_i * (gi * (1.0f - gi));
        a_f = d_f * (gf * (1.0f - gf));
        a_g = d_g * (1.0f - gg * gg);
        a_o = d_o * (go * (1.0f - go));
        w[2 * H] = a_i; w[3 * H] = a_f; w[4 * H] = a_g; w[5 * H] = a_o;
      }
      float* s = sA + (wave * PEDN_ACTOR_WAVE_ENVS + r) * PEDN_LG_AS + lane;
      s[0] = a_i; s[H] = a_f; s[2 * H] = a_g; s[3 * H] = a_o;
    }
    if (step == 0) break;
    __syncthreads();   // a of the wave's rows is there
    // dh_rec[k] = sum over the 256 gate rows q ascending of a[q] * W_hh[q][k], from +0.0: one chain
#pragma unroll
    for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) dh_rec[r] = 0.0f;
    mlp_grad_dx(dh_rec, sT + lane * PEDN_LG_WT, sA + wave * PEDN_ACTOR_WAVE_ENVS * PEDN_LG_AS, PEDN_LG_AS, cnt);
  }
}

__global__ __launch_bounds__(256) void lstmgrad_seq_bwd_kernel(LstmGradArgs a) {   // (the only parameter: PEDN_LG_LATE)
  __shared__ __attribute__((aligned(16))) float sA[PEDN_ACTOR_TILE * PEDN_LG_AS];
  __shared__ float sT[PEDN_ACTOR_HIDDEN * PEDN_LG_WT];
  __shared__ __attribute__((aligned(16))) float sD[PEDN_ACTOR_TILE * PEDN_LG_DS];
  if (a.flags[blockIdx.y] != 0) return;   // the agent has stopped: before any barrier, nothing is written
  if (blockIdx.z != 0)
    lstmgrad_bwd_role<true>(a, sA, sT, sD);
  else
    lstmgrad_bwd_role<false>(a, sA, sT, sD);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void lstmgrad_dw_kernel(LstmGradArgs a) {   // (the only parameter: PEDN_LG_LATE)
  __shared__ __attribute__((aligned(16))) float sA[PEDN_GRAD_TILE * PEDN_LG_AS];          // a of the tile's rows
  __shared__ __attribute__((aligned(16))) float sXc[PEDN_GRAD_TILE * PEDN_ACTOR_CHUNK];   // the gathered chunk of x
  __shared__ __attribute__((aligned(16))) float sHp[PEDN_GRAD_TILE * PEDN_ACTOR_HIDDEN];  // h[t - 1], +0.0 at t = 0
  __shared__ __attribute__((aligned(16))) float sC[PEDN_GRAD_TILE * PEDN_ACTOR_HIDDEN];   // relu(h')
  __shared__ float sG[PEDN_ACTOR_HIDDEN * PEDN_GRAD_PAD];                                   // a chunk of a weight gradient
  __shared__ __attribute__((aligned(16))) float sD[PEDN_GRAD_TILE * PEDN_LG_DS];          // the heads' output gradient
  __shared__ float sEl[2][PEDN_GRAD_TILE * PEDN_ACTOR_MAX_ACT];                           // -min(surr1, surr2) and logp - old; value: v - td
  __shared__ int32_t sT[PEDN_GRAD_TILE], sE[PEDN_GRAD_TILE];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = PEDN_ACTOR_HIDDEN;
  const int agent = (int)blockIdx.y;
  if (a.flags[agent] != 0) return;   // the agent has stopped: before any barrier, nothing is written
  const bool is_actor = blockIdx.z != 0;
  const int32_t* tb = a.table + (size_t)agent * PEDN_ACTOR_TABLE_COLS;
  const int obs0 = tb[0], K = tb[1], act0 = tb[2], act_w = tb[3];
  const int at_hh = PEDN_LSTM_ROWS * K, at_bih = at_hh + PEDN_LSTM_ROWS * H, at_bhh = at_bih + PEDN_LSTM_ROWS, ah = at_bhh + PEDN_LSTM_ROWS;
  const int pack_at = is_actor ? tb[4] : a.vtable[agent];
  int Hk = H;
  asm volatile("" : "+s"(Hk));   // (no instruction: the layers' input count stays a run-time value, so that no chunk loop is unrolled whole)
  // input k of row (t, e) is obs[t][e][obs0 + k]; sT / sE hold the tile's t and e, -1 behind the last row
  const auto gather = [&](int c0, int kmax) {
    const int kk = tid & (PEDN_ACTOR_CHUNK - 1);
    PEDN_LG_LATE(lg);
#pragma unroll
    for (int i = 0; i < PEDN_GRAD_TILE * PEDN_ACTOR_CHUNK / 256; ++i) {
      const int r = (tid >> 5) + i * (256 / PEDN_ACTOR_CHUNK);
      const int t = sT[r];
      float x = 0.0f;
      if (kk < kmax && t >= 0) x = lg->obs[((size_t)t * (size_t)lg->N + (size_t)sE[r]) * (size_t)lg->n_obs + (size_t)(obs0 + c0 + kk)];
      sXc[r * PEDN_ACTOR_CHUNK + kk] = x;
    }
  };
  const int n_tiles = (int)a.tiles;   // (the host refuses more than 2^31 - 1 tiles)
  for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
    PEDN_LG_LATE(la);   // (per tile, see ppograd_kernel)
    float* gws = la->ws + (size_t)blockIdx.x * (size_t)la->ws_stride + (is_actor ? (int64_t)pack_at : la->apack4 + (int64_t)pack_at);
    const float* actn = la->act + ((size_t)(is_actor ? 1 : 0) * (size_t)la->n_agents + (size_t)agent) * (size_t)la->rows * PEDN_LG_ROW;
    const size_t plane = (size_t)la->rows * (size_t)la->n_actions;
    const bool fresh = tile == (int)blockIdx.x;
    const int64_t row0 = (int64_t)tile * PEDN_GRAD_TILE;
    const int nrows = la->rows - row0 < PEDN_GRAD_TILE ? (int)(la->rows - row0) : PEDN_GRAD_TILE;
    __syncthreads();   // the tile before is done with the LDS
    if (tid < PEDN_GRAD_TILE) {
      const int64_t r = row0 + (int64_t)tid;
      const int64_t tr = r / (int64_t)la->N;
      sT[tid] = r < la->rows ? (int32_t)tr : -1;
      sE[tid] = (int32_t)(r - tr * (int64_t)la->N);
    }
    // ---- stage the tile: a, h[t - 1] and relu(h'); rows at or beyond R are zeros and in no chain
    for (int idx = tid; idx < PEDN_GRAD_TILE * PEDN_LSTM_ROWS; idx += 256) {
      const int r = idx >> 8, q = idx & (PEDN_LSTM_ROWS - 1);
      sA[r * PEDN_LG_AS + q] = r < nrows ? actn[(size_t)(row0 + r) * PEDN_LG_ROW + PEDN_LG_A + q] : 0.0f;
    }
    for (int idx = tid; idx < PEDN_GRAD_TILE * H; idx += 256) {
      const int r = idx >> 6, k = idx & 63;
      float hp = 0.0f, hc = 0.0f;
      if (r < nrows) {
        const int64_t row = row0 + r;
        hc = actn[(size_t)row * PEDN_LG_ROW + k];
        if (row >= (int64_t)la->N) hp = actn[(size_t)(row - (int64_t)la->N) * PEDN_LG_ROW + k];   // (t > 0)
      }
      sHp[idx] = hp;
      sC[idx] = hc < 0.0f ? 0.0f : hc;
    }
    if (is_actor) {
      const int r = tid >> 3, j = tid & 7;
      if (j < act_w) {
        float gmu = 0.0f, gz = 0.0f, el = 0.0f, ek = 0.0f;
        if (r < nrows) {
          const size_t at = (size_t)(row0 + r) * (size_t)la->n_actions + (size_t)(act0 + j);
          gmu = la->tail[plane + at]; gz = la->tail[2 * plane + at]; el = la->tail[3 * plane + at];
          ek = la->logp[at] - la->old_logp[at];
        }
        sD[r * PEDN_LG_DS + j] = gmu;
        sD[r * PEDN_LG_DS + act_w + j] = gz;
        sEl[0][r * PEDN_ACTOR_MAX_ACT + j] = el;
        sEl[1][r * PEDN_ACTOR_MAX_ACT + j] = ek;
      }
    } else if (tid < PEDN_GRAD_TILE) {
      float e = 0.0f;
      if (tid < nrows) {
        const size_t at = (size_t)(row0 + tid) * (size_t)la->n_agents + (size_t)agent;
        e = la->values[at] - la->td[at];
      }
      sEl[0][tid] = e;
      sD[tid * PEDN_LG_DS] = e * la->vscale;
    }
    // ---- the LSTM's weights and biases, a gate's 64 rows at a time: section 18's piece (its first barrier orders the staging above)
#pragma unroll 1
    for (int g = 0; g < PEDN_LSTM_GATES; ++g) {
      mlp_grad_dw_tile<8, true>(sA + g * H, PEDN_LG_AS, sXc, PEDN_ACTOR_CHUNK, K, nrows, gws + g * H * K, gws + at_bih + g * H, sG, true, fresh, true,
                                0, tid, 256, gather);
      mlp_grad_dw_tile<8, true>(sA + g * H, PEDN_LG_AS, sHp, H, Hk, nrows, gws + at_hh + g * H * H, gws + at_bhh + g * H, sG, false, fresh, true, 0,
                                tid, 256, gather);
    }
    // ---- the heads and the tile's sums
    double* sums = reinterpret_cast<double*>(la->ws + (size_t)blockIdx.x * (size_t)la->ws_stride + la->apack4 + la->vpack + (int64_t)PEDN_PG_SUMS * agent);
    if (is_actor) {
      mlp_grad_heads_tile<true>(sD, PEDN_LG_DS, sC, act_w, nrows, gws + ah, fresh, tid, 256);
      if (tid == 64 || tid == 128) {   // one chain in double over the tile's (row, action) elements, rows ascending, actions ascending within
        const int which = tid >> 7;
        double v = 0.0;
        for (int r = 0; r < nrows; ++r)
          for (int jj = 0; jj < act_w; ++jj) v = v + (double)sEl[which][r * PEDN_ACTOR_MAX_ACT + jj];
        sums[which] = fresh ? v : sums[which] + v;
      }
    } else if (wave == 1) {
      float g = 0.0f;
      for (int r = 0; r < nrows; ++r) g = g + sD[r * PEDN_LG_DS] * sC[r * H + lane];
      mlp_grad_put<true>(gws + ah + lane, g, fresh);
    } else if (wave == 2 && lane == 0) {
      float g = 0.0f;
      for (int r = 0; r < nrows; ++r) g = g + sD[r * PEDN_LG_DS];
      mlp_grad_put<true>(gws + ah + H, g, fresh);
    } else if (wave == 2 && lane == 1) {   // the sum of squares in double (a float32 square is exact there)
      double q = 0.0;
      for (int r = 0; r < nrows; ++r) q = q + (double)sEl[0][r] * (double)sEl[0][r];
      sums[2] = fresh ? q : sums[2] + q;
    }
  }
}

__global__ __launch_bounds__(256) void lstmgrad_reduce_kernel(PpoReduceArgs a) {
  __shared__ double sRed[256];
  const int agent = (int)blockIdx.y;
  if (a.flags[agent] != 0) return;
  int off, len;
  lg_net_range(a.table, a.vtable, agent, blockIdx.z != 0, off, len);
  pg_reduce_body(a, off, len, sRed);
}

__global__ __launch_bounds__(256) void lstmgrad_adam_kernel(PpoAdamArgs a) {
  const int agent = (int)blockIdx.y;
  if (a.flags[agent] != 0) return;
  int off, len;
  lg_net_range(a.table, a.vtable, agent, blockIdx.z != 0, off, len);
  pg_adam_body(a, off, len);
}

// ---- host side: pedn_lstm_ppo_epoch_update and pedn_lstm_ppo_begin_update of include/pedn.h; no state in the engine's handle
int pedn_lstm_ppo_begin_update(int32_t* stop_flags, int32_t n_agents, void* stream) { return pedn_ppo_begin_update(stop_flags, n_agents, stream); }

int pedn_lstm_ppo_epoch_update(const float* obs, const void* actions, const float* old_log_probs, const float* advantages, const float* td_target,
                               const int32_t* table, const int32_t* value_table, float* actor_params, float* value_params, float* actor_grads,
                               float* value_grads, float* actor_raw_grads, float* value_raw_grads, float* actor_exp_avg, float* value_exp_avg,
                               float* actor_exp_avg_sq, float* value_exp_avg_sq, float* workspace, float* activations, float* tail,
                               double* norm_parts, float* log_probs, float* values, float* scalars, int64_t* adam_state, int32_t* stop_flags,
                               int64_t actor_pack_floats, int64_t value_pack_floats, int32_t T, int32_t N, int32_t n_obs, int32_t n_actions,
                               int32_t n_agents, int32_t hidden_size, int32_t num_layers, int32_t actions_f64, int32_t groups, double min_std,
                               double max_std, double actor_lr, double critic_lr, double clip_eps, double max_grad_norm, double kl_tolerance,
                               double beta1, double beta2, double eps, int32_t do_adam, void* stream) {
  if (!obs || !actions || !old_log_probs || !advantages || !td_target || !table || !value_table || !actor_params || !value_params ||
      !actor_grads || !value_grads || !actor_raw_grads || !value_raw_grads || !actor_exp_avg || !value_exp_avg || !actor_exp_avg_sq ||
      !value_exp_avg_sq || !workspace || !activations || !tail || !norm_parts || !log_probs || !values || !scalars || !adam_state || !stop_flags)
    return fail(nullptr, PEDN_E_ARG, "null argument");
  if (const char* why = update_refusal(
          hidden_size, "the LSTM kernels are built for hidden_size 64", T >= 1 && N >= 1 && n_obs >= 1 && n_actions >= 1, n_agents,
          "T, N, n_obs, n_actions and n_agents must be positive (at most 65535 agents)",
          num_layers != 1                     ? "the LSTM kernels are built for one layer"
          : actions_f64 < 0 || actions_f64 > 1 ? "the actions' dtype flag is 0 (float32) or 1 (float64)"
          : groups < 1 || groups > 65535      ? "groups must be in 1 .. 65535"
                                              : nullptr,
          actor_pack_floats >= 1 && value_pack_floats >= 4 && value_pack_floats % 4 == 0,
          "the actors' pack is empty or the value pack's length is no positive multiple of 4 floats",
          (uintptr_t)actor_params | (uintptr_t)value_params | (uintptr_t)actor_grads | (uintptr_t)value_grads | (uintptr_t)actor_raw_grads |
              (uintptr_t)value_raw_grads | (uintptr_t)actor_exp_avg | (uintptr_t)value_exp_avg | (uintptr_t)actor_exp_avg_sq |
              (uintptr_t)value_exp_avg_sq | (uintptr_t)workspace | (uintptr_t)activations,
          actor_lr, critic_lr, beta1, beta2, eps))
    return fail(nullptr, PEDN_E_ARG, why);
  if (!(clip_eps > 0.0 && clip_eps < INFINITY)) return fail(nullptr, PEDN_E_ARG, "clip_eps must be finite and positive");
  if (!(max_grad_norm > 0.0 && max_grad_norm < INFINITY)) return fail(nullptr, PEDN_E_ARG, "max_grad_norm must be finite and positive");
  if (kl_tolerance != kl_tolerance) return fail(nullptr, PEDN_E_ARG, "kl_tolerance must not be NaN");
  const int64_t rows = (int64_t)T * (int64_t)N;
  const int64_t tiles = (rows + PEDN_GRAD_TILE - 1) / PEDN_GRAD_TILE;
  if (tiles > 0x7fffffffLL) return fail(nullptr, PEDN_E_ARG, "T * N is beyond 2^31 - 1 tiles of 32 rows");
  const int G = (int)(tiles < (int64_t)groups ? tiles : (int64_t)groups);
  const int64_t apack4 = (actor_pack_floats + 3) / 4 * 4;
  const int64_t ws_stride = apack4 + value_pack_floats + (int64_t)PEDN_PG_SUMS * n_agents;
  LstmGradArgs a{};
  a.obs = obs; a.actions = actions; a.old_logp = old_log_probs; a.adv = advantages; a.td = td_target; a.table = table; a.vtable = value_table;
  a.actor = actor_params; a.value = value_params; a.flags = stop_flags; a.act = activations; a.tail = tail; a.ws = workspace;
  a.logp = log_probs; a.values = values;
  a.rows = rows; a.tiles = tiles; a.apack4 = apack4; a.vpack = value_pack_floats; a.ws_stride = ws_stride;
  a.T = T; a.N = N; a.n_obs = n_obs; a.n_actions = n_actions; a.n_agents = n_agents; a.act_f64 = actions_f64;
  a.min_std = (float)min_std; a.max_std = (float)max_std; a.clip_lo = (float)(1.0 - clip_eps); a.clip_hi = (float)(1.0 + clip_eps);
  a.vscale = (float)(2.0 / (double)rows);
  const dim3 seq_grid((unsigned)((N + PEDN_LG_ENV_TILE - 1) / PEDN_LG_ENV_TILE), (unsigned)n_agents, 2u);
  hipLaunchKernelGGL(lstmgrad_seq_fwd_kernel, seq_grid, dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(nullptr, hipGetLastError());
  hipLaunchKernelGGL(lstmgrad_seq_bwd_kernel, seq_grid, dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(nullptr, hipGetLastError());
  hipLaunchKernelGGL(lstmgrad_dw_kernel, dim3((unsigned)G, (unsigned)n_agents, 2u), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(nullptr, hipGetLastError());
  PpoReduceArgs b{};
  b.ws = workspace; b.table = table; b.vtable = value_table; b.flags = stop_flags; b.raw_a = actor_raw_grads; b.raw_v = value_raw_grads;
  b.parts = norm_parts; b.scalars = scalars; b.rows = rows; b.apack4 = apack4; b.vpack = value_pack_floats; b.ws_stride = ws_stride;
  b.G = G; b.S = 1; b.n_agents = n_agents;
  hipLaunchKernelGGL(lstmgrad_reduce_kernel, dim3(PEDN_PG_BLOCKS, (unsigned)n_agents, 2u), dim3(256), 0, (hipStream_t)stream, b);
  HIP_TRY(nullptr, hipGetLastError());
  PpoAdamArgs c{};
  c.table = table; c.vtable = value_table; c.flags = stop_flags; c.raw_a = actor_raw_grads; c.raw_v = value_raw_grads; c.parts = norm_parts;
  c.g_a = actor_grads; c.g_v = value_grads; c.m_a = actor_exp_avg; c.m_v = value_exp_avg; c.v_a = actor_exp_avg_sq; c.v_v = value_exp_avg_sq;
  c.p_a = actor_params; c.p_v = value_params; c.scalars = scalars; c.state = adam_state;
  c.S = 1; c.n_agents = n_agents; c.do_adam = do_adam ? 1 : 0; c.max_norm = (float)max_grad_norm;
  c.lr_a = actor_lr; c.lr_v = critic_lr; c.beta1 = beta1; c.beta2 = beta2; c.kl_stop = 1.5 * kl_tolerance;
  c.coef = adam_coef(beta1, beta2, eps);
  hipLaunchKernelGGL(lstmgrad_adam_kernel, dim3(PEDN_PG_BLOCKS, (unsigned)n_agents, 2u), dim3(256), 0, (hipStream_t)stream, c);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}
