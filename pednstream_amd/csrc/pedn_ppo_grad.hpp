// One epoch of the reference's PPOAgent.update loop (rl/agents/PPO_org.py:579-629: both forwards, the clipped surrogate and the MSE value
// loss, two backward passes, clip_grad_norm_ of each network, two Adam steps, and the KL early stop) for a whole rollout and every agent.
// The contract is DESIGN section 20; tests/ppo_update_model.py restates it in numpy.
//
// ppograd_kernel          grid (G, n_agents, 2), 256 threads, G = min(tiles, groups).  blockIdx.z = 0 is the value network, 1 the actor.  A
//                         workgroup takes one agent, one network and the tiles g, g + G, g + 2 G, ... of 32 consecutive rows r = t * N + e,
//                         ascending.  Per tile: section 16's forward with section 14's data path (pedn_mlp.hpp's mlp_layer: 4 waves, 8 rows
//                         each, a lane per neuron, the stacks gathered on the fly) with the hidden rows kept in LDS, the loss' tail on a lane
//                         per (row, action) in double, rounded once per result, and the backward with pedn_mlp_grad.hpp's pieces (a weight
//                         gradient: a lane per output neuron, a wave per 8 of a chunk's 32 columns, ONE chain over the tile's rows; an input
//                         gradient: a lane per column, a chain over the output neurons; the LayerNorm's: a lane per neuron, the forward's tree).
//                         The workgroup owns one slab of the workspace in the layout of the packs: it stores its first tile's partial and
//                         adds every later one (slab = slab + partial; every address has one thread that reads and writes it).  Rows at or
//                         beyond T * N are in no chain.
//                         LDS: 64 * 33 + 32 * 32 + 4 * 32 * 64 + 32 * 68 + 32 * 16 + 2 * 32 * 8 + 4 * 32 words = 58624 bytes.
// ppograd_reduce_kernel   grid (16, n_agents, 2), 256 threads: adds the slabs from +0.0, g ascending, into the unclipped gradient packs, forms
//                         the losses and approx_kl, and each workgroup's part of sum g^2 in double (a thread's elements ascending, then a
//                         halving tree over the 256 threads).
// ppograd_adam_kernel     grid (16, n_agents, 2), 256 threads: total_norm = (float)sqrt(the 16 parts, ascending), clip_grad_norm_'s
//                         coefficient, the clipped gradient packs and, unless switched off, section 19's Adam step with the agent's own step
//                         count; the last workgroup of an agent (section 14's ticket) advances its count and sets its stop flag.
// ppograd_begin_kernel    clears the stop flags.
// A workgroup of an agent whose stop flag is set leaves at once, in all three.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_actor.hpp"
#include "pedn_adam.hpp"
#include "pedn_mlp.hpp"
#include "pedn_mlp_grad.hpp"
#include "pedn_ppo_loss.hpp"   // the loss' tail and the reduce and Adam launches' bodies, shared with pedn_lstm_grad.hpp

struct PpoGradArgs {
  const float* obs;        // [T + 1][N][n_obs]
  const void* actions;     // [T][N][n_actions], float or double
  const float* old_logp;   // [T][N][n_actions]
  const float* adv;        // [T][N][n_agents]
  const float* td;         // [T][N][n_agents]
  const int32_t* table;    // [n_agents][PEDN_ACTOR_TABLE_COLS]: the actors' table
  const int32_t* vtable;   // [n_agents]: offsets (floats) in the value pack
  const float* actor;      // the actors' pack (PPO kind)
  const float* value;      // the value pack
  const int32_t* flags;    // [n_agents]: the stop flags
  float* ws;               // [G][ws_stride]: a slab = the actors' pack's layout (rounded up to 4), the value pack's, [n_agents][PEDN_PG_SUMS]
  float* logp;             // [T][N][n_actions]
  float* values;           // [T][N][n_agents]
  float* tail;             // [3][T][N][n_actions] or null: std and the loss' gradients by mu and by the pre-softplus value
  int64_t rows, tiles;     // T * N and ceil(rows / 32)
  int64_t apack4, vpack, ws_stride;
  int32_t N, S, n_obs, n_actions, n_agents, act_f64;
  float min_std, max_std, clip_lo, clip_hi;   // (float)(1 - clip_eps), (float)(1 + clip_eps)
  float vscale;            // (float)(2.0 / rows)
};

typedef const __attribute__((address_space(4))) PpoGradArgs* PpoGradLate;

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void ppograd_kernel(PpoGradArgs a) {
  __shared__ float sW[PEDN_ACTOR_HIDDEN * PEDN_GRAD_PAD];
  __shared__ __attribute__((aligned(16))) float sXc[PEDN_GRAD_TILE * PEDN_ACTOR_CHUNK];
  __shared__ __attribute__((aligned(16))) float sA[PEDN_GRAD_TILE * PEDN_ACTOR_HIDDEN];   // h1
  __shared__ __attribute__((aligned(16))) float sB[PEDN_GRAD_TILE * PEDN_ACTOR_HIDDEN];   // h2
  __shared__ __attribute__((aligned(16))) float sC[PEDN_GRAD_TILE * PEDN_ACTOR_HIDDEN];   // h3 behind its ReLU
  __shared__ __attribute__((aligned(16))) float sX[PEDN_GRAD_TILE * PEDN_ACTOR_HIDDEN];   // the LayerNorm's normalised rows
  __shared__ __attribute__((aligned(16))) float sD[PEDN_GRAD_TILE * PEDN_GRAD_DS];          // the output gradient of the layer at hand
  __shared__ float sOut[PEDN_GRAD_TILE * 2 * PEDN_ACTOR_MAX_ACT];                         // mu | pre-softplus of the heads
  __shared__ float sEl[2][PEDN_GRAD_TILE * PEDN_ACTOR_MAX_ACT];                           // -min(surr1, surr2) and logp - old; value: v - td
  __shared__ float sSd[PEDN_GRAD_TILE], sDv[PEDN_GRAD_TILE];                                // the LayerNorm's sqrt(var + eps); the value's gradient
  __shared__ int32_t sT[PEDN_GRAD_TILE], sE[PEDN_GRAD_TILE];
  const int tid0 = (int)threadIdx.x;
  const int H = PEDN_ACTOR_HIDDEN;
  const int agent = (int)blockIdx.y;
  if (a.flags[agent] != 0) return;   // the agent has stopped: before any barrier, nothing is written
  const bool is_actor = blockIdx.z != 0;
  const int n_tiles = (int)a.tiles;   // (the host refuses more than 2^31 - 1 tiles)

  for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
    // The launch's arguments as the kernel argument segment holds them, taken again for every tile behind an empty asm: what is derived
    // from them (the networks' and the slab's addresses, the shapes) is formed per tile and not hoisted out of this loop, whose body is the
    // whole kernel (hoisted, those values were held in registers throughout: 68 SGPRs and 91 VGPRs spilled)
    PpoGradLate la = (PpoGradLate)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(la));
    // (the thread's number likewise: the predicates on its lane and wave are formed where they are used, not once before the loop and
    // held as masks in SGPR pairs, which spilled)
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int vrow = (tid >> 6) * PEDN_GRAD_WAVE_ROWS;   // the wave's first row (a vector value: the stores of its rows index with it)
    const int32_t* tb = la->table + (size_t)agent * PEDN_ACTOR_TABLE_COLS;
    const int act_w = tb[3];
    const int K1 = la->S * tb[1];
    const float* net = is_actor ? la->actor + tb[4] : la->value + la->vtable[agent];
    float* slab = la->ws + (size_t)blockIdx.x * (size_t)la->ws_stride;
    float* gws = slab + (is_actor ? (int64_t)tb[4] : la->apack4 + (int64_t)la->vtable[agent]);
    const int at2 = H * K1 + H, at3 = at2 + H * H + H, at4 = at3 + H * H + H;   // fc2, fc, the LayerNorm / value_head
    const int ah = at4 + 2 * H;                                                 // the actor's heads
    int Hk = H;
    asm volatile("" : "+s"(Hk));   // (no instruction: the layers' input count stays a run-time value, so that no chunk loop is unrolled whole)

    // input i = f * S + s of row (t, e) is obs[max(t - (S - 1) + s, 0)][e][obs0 + f]; sT / sE hold the tile's t and e, -1 behind the last row
    const auto gather = [&](int c0, int kmax) {
      const int kk = (int)(threadIdx.x & (PEDN_ACTOR_CHUNK - 1));
      const int S = la->S, obs0 = la->table[(size_t)agent * PEDN_ACTOR_TABLE_COLS];
      const unsigned k = (unsigned)(c0 + kk), f = k / (unsigned)S, s = k - f * (unsigned)S;
#pragma unroll
      for (int i = 0; i < PEDN_GRAD_TILE * PEDN_ACTOR_CHUNK / 256; ++i) {
        const int r = (int)(threadIdx.x >> 5) + i * (256 / PEDN_ACTOR_CHUNK);
        const int t = sT[r];
        float x = 0.0f;
        if (kk < kmax && t >= 0) {
          int tt = t - (S - 1) + (int)s;
          tt = tt < 0 ? 0 : tt;
          x = la->obs[((size_t)tt * (size_t)la->N + (size_t)sE[r]) * (size_t)la->n_obs + (size_t)(obs0 + (int)f)];
        }
        sXc[r * PEDN_ACTOR_CHUNK + kk] = x;
      }
    };
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
    // ---- forward: section 16's, with h1, h2, h3 (and the LayerNorm's rows) kept
    float acc[PEDN_GRAD_WAVE_ROWS];
    mlp_layer(acc, net, net + H * K1, net, net + H * K1, H, H, K1, true, sW, sXc, sA, gather);
    mlp_relu_store(sA + vrow * H + lane, acc);
    mlp_layer(acc, net + at2, net + at2 + H * H, net + at2, net + at2 + H * H, H, H, Hk, false, sW, sXc, sA, gather);
    mlp_relu_store(sB + vrow * H + lane, acc);
    mlp_layer(acc, net + at3, net + at3 + H * H, net + at3, net + at3 + H * H, H, H, Hk, false, sW, sXc, sB, gather);
    if (is_actor) {
      float xh[PEDN_GRAD_WAVE_ROWS], sd[PEDN_GRAD_WAVE_ROWS];
      mlp_layer_norm_keep(acc, xh, sd, net[at4 + lane], net[at4 + H + lane]);
#pragma unroll
      for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) {
        sX[(vrow + r) * H + lane] = xh[r];
        if (lane == 0) sSd[vrow + r] = sd[r];
      }
    }
    mlp_relu_store(sC + vrow * H + lane, acc);

    if (is_actor) {
      const float* so = mlp_heads(acc, net + ah, act_w, sW, sXc, sC, sOut, gather);
      // ---- the loss' tail on a lane per (row, action): forward in section 16's arithmetic, backward in double, rounded once per result
      // (the arguments once more behind an empty asm: the tail's fields are loaded here, not at the loop's top and held through the forward)
      PpoGradLate lt = la;
      asm volatile("" : "+s"(lt));
      const int lr = lane / act_w, j = lane - lr * act_w;
      if (lr < PEDN_GRAD_WAVE_ROWS) {
        const int tr = vrow + lr;
        float gmu = 0.0f, gz = 0.0f, el = 0.0f, ek = 0.0f;
        if (tr < nrows) {
          const int64_t row = row0 + tr;
          const float mu = so[lr * 2 * PEDN_ACTOR_MAX_ACT + j], z = so[lr * 2 * PEDN_ACTOR_MAX_ACT + PEDN_ACTOR_MAX_ACT + j];
          const size_t at = (size_t)row * (size_t)lt->n_actions + (size_t)(lt->table[(size_t)agent * PEDN_ACTOR_TABLE_COLS + 2] + j);
          const float act = lt->act_f64 ? (float)static_cast<const double*>(lt->actions)[at] : static_cast<const float*>(lt->actions)[at];
          const float old = lt->old_logp[at], A = lt->adv[(size_t)row * (size_t)lt->n_agents + (size_t)agent];
          const PpoTailElem te = ppo_loss_tail(mu, z, act, old, A, lt->min_std, lt->max_std, lt->clip_lo, lt->clip_hi,
                                               -1.0 / ((double)lt->rows * (double)act_w));
          lt->logp[at] = te.lp;
          gmu = te.gmu; gz = te.gz; el = te.el; ek = te.ek;
          const float sd = te.sd;
          if (lt->tail) {
            const size_t plane = (size_t)lt->rows * (size_t)lt->n_actions;
            float* o = lt->tail + at;
            o[0] = sd; o[plane] = gmu; o[2 * plane] = gz;
          }
        }
        sD[tr * PEDN_GRAD_DS + j] = gmu;
        sD[tr * PEDN_GRAD_DS + act_w + j] = gz;
        sEl[0][tr * PEDN_ACTOR_MAX_ACT + j] = el;
        sEl[1][tr * PEDN_ACTOR_MAX_ACT + j] = ek;
      }
      __syncthreads();
      // ---- the heads: a thread per weight; the tile's two sums; h3's gradient behind the ReLU mask, a lane per neuron
      mlp_grad_heads_tile<true>(sD, PEDN_GRAD_DS, sC, act_w, nrows, gws + ah, fresh, tid, 256);
      if (tid == 64 || tid == 128) {   // one chain over the tile's (row, action) elements, rows ascending, actions ascending within
        const int which = tid >> 7;
        // IN DOUBLE: the elements cancel (the advantages are normalised to mean 0), and as a float32 chain this sum alone carried the
        // forward's error against the reference's recorded update (24 times its float32 error in actor_loss)
        double v = 0.0;
        for (int r = 0; r < nrows; ++r)
          for (int jj = 0; jj < act_w; ++jj) v = v + (double)sEl[which][r * PEDN_ACTOR_MAX_ACT + jj];
        double* p = reinterpret_cast<double*>(la->ws + (size_t)blockIdx.x * (size_t)la->ws_stride + la->apack4 + la->vpack + (int64_t)PEDN_PG_SUMS * agent) + which;
        *p = fresh ? v : *p + v;
      }
      float dy[PEDN_GRAD_WAVE_ROWS];
#pragma unroll
      for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) dy[r] = 0.0f;
      {
        const float* hmu = net + ah;
        const float* hsd = hmu + act_w * H + act_w;
        for (int o = 0; o < 2 * act_w; ++o) {
          const float w = o < act_w ? hmu[o * H + lane] : hsd[(o - act_w) * H + lane];
#pragma unroll
          for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) dy[r] = dy[r] + sD[(vrow + r) * PEDN_GRAD_DS + o] * w;
        }
      }
#pragma unroll
      for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) dy[r] = sC[(vrow + r) * H + lane] > 0.0f ? dy[r] : 0.0f;
      __syncthreads();   // every thread has read the heads' gradient
#pragma unroll
      for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) sD[(vrow + r) * PEDN_GRAD_DS + lane] = dy[r];
      __syncthreads();
      // ---- the LayerNorm: its weight (wave 0) and bias (wave 1), rows ascending; then its input's gradient, the wave's own rows
      if (wave < 2) {
        float v = 0.0f;
        if (wave == 0)
          for (int r = 0; r < nrows; ++r) v = v + sD[r * PEDN_GRAD_DS + lane] * sX[r * H + lane];
        else
          for (int r = 0; r < nrows; ++r) v = v + sD[r * PEDN_GRAD_DS + lane];
        float* p = gws + at4 + wave * H + lane;
        *p = fresh ? v : *p + v;
      }
      {
        float xh[PEDN_GRAD_WAVE_ROWS], sd[PEDN_GRAD_WAVE_ROWS];
#pragma unroll
        for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) {
          xh[r] = sX[(vrow + r) * H + lane];
          sd[r] = sSd[vrow + r];
        }
        mlp_layer_norm_grad(dy, xh, sd, net[at4 + lane]);
      }
      __syncthreads();   // waves 0 and 1 have read the LayerNorm's output gradient
#pragma unroll
      for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) sD[(vrow + r) * PEDN_GRAD_DS + lane] = dy[r];
    } else {
      // ---- value_head on a lane per row (section 16's chain), e = v - td, dv = e * (float)(2 / R)
      const float* wo = net + at4;
      PpoGradLate lv = la;
      asm volatile("" : "+s"(lv));
      __syncthreads();   // h3 is there
      if (lane < PEDN_GRAD_WAVE_ROWS) {
        const int r = vrow + lane;
        float v = wo[H];
        for (int k = 0; k < H; ++k) v = v + wo[k] * sC[r * H + k];
        float e = 0.0f;
        if (r < nrows) {
          const size_t at = (size_t)(row0 + r) * (size_t)lv->n_agents + (size_t)agent;
          lv->values[at] = v;
          e = v - lv->td[at];
        }
        sEl[0][r] = e;
        sDv[r] = e * lv->vscale;
      }
      __syncthreads();
      if (wave == 1) {
        float g = 0.0f;
        for (int r = 0; r < nrows; ++r) g = g + sDv[r] * sC[r * H + lane];
        float* p = gws + at4 + lane;
        *p = fresh ? g : *p + g;
      } else if (wave == 2 && lane == 0) {
        float g = 0.0f;
        for (int r = 0; r < nrows; ++r) g = g + sDv[r];
        float* p = gws + at4 + H;
        *p = fresh ? g : *p + g;
      } else if (wave == 2 && lane == 1) {   // the sum of squares in double, like the actor's two sums (a float32 square is exact in double)
        double q = 0.0;
        for (int r = 0; r < nrows; ++r) q = q + (double)sEl[0][r] * (double)sEl[0][r];
        double* p = reinterpret_cast<double*>(lv->ws + (size_t)blockIdx.x * (size_t)lv->ws_stride + lv->apack4 + lv->vpack + (int64_t)PEDN_PG_SUMS * agent) + 2;
        *p = fresh ? q : *p + q;
      }
      {
        const float wl = wo[lane];
#pragma unroll
        for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) sD[(vrow + r) * PEDN_GRAD_DS + lane] = sC[(vrow + r) * H + lane] > 0.0f ? sDv[vrow + r] * wl : 0.0f;
      }
    }
    // ---- fc, the mask, encoder.fc2, the mask, encoder.fc1: section 18's pieces
    mlp_grad_dw_tile<8, true>(sD, PEDN_GRAD_DS, sB, H, Hk, nrows, gws + at3, gws + at3 + H * H, sW, false, fresh, true, 0, tid, 256, gather);
    mlp_grad_dx_tile(acc, true, sD + vrow * PEDN_GRAD_DS, PEDN_GRAD_DS, net + at3, H, sW, tid, 256);
    __syncthreads();   // every wave has read the output gradient that is overwritten now
#pragma unroll
    for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) sD[(vrow + r) * PEDN_GRAD_DS + lane] = sB[(vrow + r) * H + lane] > 0.0f ? acc[r] : 0.0f;
    mlp_grad_dw_tile<8, true>(sD, PEDN_GRAD_DS, sA, H, Hk, nrows, gws + at2, gws + at2 + H * H, sW, false, fresh, true, 0, tid, 256, gather);
    mlp_grad_dx_tile(acc, true, sD + vrow * PEDN_GRAD_DS, PEDN_GRAD_DS, net + at2, H, sW, tid, 256);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PEDN_GRAD_WAVE_ROWS; ++r) sD[(vrow + r) * PEDN_GRAD_DS + lane] = sA[(vrow + r) * H + lane] > 0.0f ? acc[r] : 0.0f;
    mlp_grad_dw_tile<8, true>(sD, PEDN_GRAD_DS, sXc, PEDN_ACTOR_CHUNK, K1, nrows, gws, gws + H * K1, sW, true, fresh, true, 0, tid, 256, gather);
  }
}

// where a network lies in its pack and how long it is
__device__ __forceinline__ void pg_net_range(const int32_t* table, const int32_t* vtable, int agent, bool is_actor, int S, int& off, int& len) {
  const int32_t* tb = table + (size_t)agent * PEDN_ACTOR_TABLE_COLS;
  const int H = PEDN_ACTOR_HIDDEN, K1 = S * tb[1], trunk = H * K1 + H + 2 * (H * H + H);
  off = is_actor ? tb[4] : vtable[agent];
  len = is_actor ? trunk + 2 * H + 2 * (tb[3] * H + tb[3]) : trunk + H + 1;
}

__global__ __launch_bounds__(256) void ppograd_reduce_kernel(PpoReduceArgs a) {
  __shared__ double sRed[256];
  const int agent = (int)blockIdx.y;
  if (a.flags[agent] != 0) return;
  int off, len;
  pg_net_range(a.table, a.vtable, agent, blockIdx.z != 0, a.S, off, len);
  pg_reduce_body(a, off, len, sRed);
}

__global__ __launch_bounds__(256) void ppograd_adam_kernel(PpoAdamArgs a) {
  const int agent = (int)blockIdx.y;
  if (a.flags[agent] != 0) return;
  int off, len;
  pg_net_range(a.table, a.vtable, agent, blockIdx.z != 0, a.S, off, len);
  pg_adam_body(a, off, len);
}

// stop_flags[0 .. n) = 0: a launch like the others, so that a captured update is one chain of kernel nodes
__global__ __launch_bounds__(256) void ppograd_begin_kernel(int32_t* flags, int32_t n) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) flags[i] = 0;
}

// ---- host side: pedn_ppo_epoch_update and pedn_ppo_begin_update of include/pedn.h; no state in the engine's handle
int pedn_ppo_begin_update(int32_t* stop_flags, int32_t n_agents, void* stream) {
  if (!stop_flags) return fail(nullptr, PEDN_E_ARG, "null argument");
  if (n_agents < 1 || n_agents > 65535) return fail(nullptr, PEDN_E_ARG, "n_agents must be in 1 .. 65535");
  hipLaunchKernelGGL(ppograd_begin_kernel, dim3((unsigned)((n_agents + 255) / 256)), dim3(256), 0, (hipStream_t)stream, stop_flags, n_agents);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}

int pedn_ppo_epoch_update(const float* obs, const void* actions, const float* old_log_probs, const float* advantages, const float* td_target,
                          const int32_t* table, const int32_t* value_table, float* actor_params, float* value_params, float* actor_grads,
                          float* value_grads, float* actor_raw_grads, float* value_raw_grads, float* actor_exp_avg, float* value_exp_avg,
                          float* actor_exp_avg_sq, float* value_exp_avg_sq, float* workspace, double* norm_parts, float* log_probs, float* values,
                          float* tail_out, float* scalars, int64_t* adam_state, int32_t* stop_flags, int64_t actor_pack_floats, int64_t value_pack_floats,
                          int32_t T, int32_t N, int32_t stack_size, int32_t n_obs, int32_t n_actions, int32_t n_agents, int32_t hidden_size,
                          int32_t actions_f64, int32_t groups, double min_std, double max_std, double actor_lr, double critic_lr,
                          double clip_eps, double max_grad_norm, double kl_tolerance, double beta1, double beta2, double eps, int32_t do_adam,
                          void* stream) {
  if (!obs || !actions || !old_log_probs || !advantages || !td_target || !table || !value_table || !actor_params || !value_params ||
      !actor_grads || !value_grads || !actor_raw_grads || !value_raw_grads || !actor_exp_avg || !value_exp_avg || !actor_exp_avg_sq ||
      !value_exp_avg_sq || !workspace || !norm_parts || !log_probs || !values || !scalars || !adam_state || !stop_flags)
    return fail(nullptr, PEDN_E_ARG, "null argument");
  if (const char* why = update_refusal(
          hidden_size, "the PPO update kernels are built for hidden_size 64", T >= 1 && N >= 1 && stack_size >= 1 && n_obs >= 1 && n_actions >= 1,
          n_agents, "T, N, stack_size, n_obs, n_actions and n_agents must be positive (at most 65535 agents)",
          actions_f64 < 0 || actions_f64 > 1 ? "the actions' dtype flag is 0 (float32) or 1 (float64)"
          : groups < 1 || groups > 65535  ? "groups must be in 1 .. 65535"
                                          : nullptr,
          actor_pack_floats >= 1 && value_pack_floats >= 4 && value_pack_floats % 4 == 0,
          "the actors' pack is empty or the value pack's length is no positive multiple of 4 floats",
          (uintptr_t)actor_params | (uintptr_t)value_params | (uintptr_t)actor_grads | (uintptr_t)value_grads | (uintptr_t)actor_raw_grads |
              (uintptr_t)value_raw_grads | (uintptr_t)actor_exp_avg | (uintptr_t)value_exp_avg | (uintptr_t)actor_exp_avg_sq |
              (uintptr_t)value_exp_avg_sq | (uintptr_t)workspace,
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
  PpoGradArgs a{};
  a.obs = obs; a.actions = actions; a.old_logp = old_log_probs; a.adv = advantages; a.td = td_target; a.table = table; a.vtable = value_table;
  a.actor = actor_params; a.value = value_params; a.flags = stop_flags; a.ws = workspace; a.logp = log_probs; a.values = values; a.tail = tail_out;
  a.rows = rows; a.tiles = tiles; a.apack4 = apack4; a.vpack = value_pack_floats; a.ws_stride = ws_stride;
  a.N = N; a.S = stack_size; a.n_obs = n_obs; a.n_actions = n_actions; a.n_agents = n_agents; a.act_f64 = actions_f64;
  a.min_std = (float)min_std; a.max_std = (float)max_std; a.clip_lo = (float)(1.0 - clip_eps); a.clip_hi = (float)(1.0 + clip_eps);
  a.vscale = (float)(2.0 / (double)rows);
  hipLaunchKernelGGL(ppograd_kernel, dim3((unsigned)G, (unsigned)n_agents, 2u), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(nullptr, hipGetLastError());
  PpoReduceArgs b{};
  b.ws = workspace; b.table = table; b.vtable = value_table; b.flags = stop_flags; b.raw_a = actor_raw_grads; b.raw_v = value_raw_grads;
  b.parts = norm_parts; b.scalars = scalars; b.rows = rows; b.apack4 = apack4; b.vpack = value_pack_floats; b.ws_stride = ws_stride;
  b.G = G; b.S = stack_size; b.n_agents = n_agents;
  hipLaunchKernelGGL(ppograd_reduce_kernel, dim3(PEDN_PG_BLOCKS, (unsigned)n_agents, 2u), dim3(256), 0, (hipStream_t)stream, b);
  HIP_TRY(nullptr, hipGetLastError());
  PpoAdamArgs c{};
  c.table = table; c.vtable = value_table; c.flags = stop_flags; c.raw_a = actor_raw_grads; c.raw_v = value_raw_grads; c.parts = norm_parts;
  c.g_a = actor_grads; c.g_v = value_grads; c.m_a = actor_exp_avg; c.m_v = value_exp_avg; c.v_a = actor_exp_avg_sq; c.v_v = value_exp_avg_sq;
  c.p_a = actor_params; c.p_v = value_params; c.scalars = scalars; c.state = adam_state;
  c.S = stack_size; c.n_agents = n_agents; c.do_adam = do_adam ? 1 : 0; c.max_norm = (float)max_grad_norm;
  c.lr_a = actor_lr; c.lr_v = critic_lr; c.beta1 = beta1; c.beta2 = beta2; c.kl_stop = 1.5 * kl_tolerance;
  c.coef = adam_coef(beta1, beta2, eps);
  hipLaunchKernelGGL(ppograd_adam_kernel, dim3(PEDN_PG_BLOCKS, (unsigned)n_agents, 2u), dim3(256), 0, (hipStream_t)stream, c);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}
