// What the clipped-loss epochs of the stacked agents (pedn_ppo_grad.hpp) and of the recurrent agents (pedn_lstm_grad.hpp,
// section 21) share, each written once: the loss' tail on one (row, action) element, the launch that adds the slabs and forms the losses and
// the parts of sum g^2, and the launch that clips and takes the Adam step and the early stop.  The two bodies take the network's range in its
// pack from the kernel that calls them: only that differs between the two layouts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_actor.hpp"
#include "pedn_adam.hpp"
#include "pedn_mlp.hpp"

#define PEDN_PG_BLOCKS 16                  // workgroups per (agent, network) of the reduce and Adam launches: part of the norm's order
#define PEDN_PG_SUMS 8                     // floats per agent and slab: three DOUBLES, the sums of -min(surr1, surr2), of logp - old, of (v - td)^2; 2 unused
#define PEDN_PG_SCALARS 7                  // actor_loss, critic_loss, approx_kl, actor_norm, value_norm, actor_coef, value_coef

// One (row, action) element of the loss: forward in section 16's arithmetic, backward in double, rounded once per result.
struct PpoTailElem {
  float lp, sd;     // Normal.log_prob(act) and the clamped std
  float gmu, gz;    // the loss' gradients by mu and by the pre-softplus value
  float el, ek;     // -min(surr1, surr2) and logp - old
};

// G = -1 / (rows * act_w): the mean's weight of the element.
__device__ __forceinline__ PpoTailElem ppo_loss_tail(float mu, float z, float act, float old, float A, float min_std, float max_std, float clip_lo,
                                                     float clip_hi, double G) {
  PpoTailElem e;
  const float sp = mlp_softplus(z);
  const float sd = actor_clip(sp, min_std, max_std);
  const float lp = (float)normal_log_prob(act, mu, sd);
  e.lp = lp; e.sd = sd;
  const float dl = lp - old;
  const float lrc = dl < -20.0f ? -20.0f : (dl > 20.0f ? 20.0f : dl);
  const float ratio = (float)exp((double)lrc);
  const float rc = ratio < clip_lo ? clip_lo : (ratio > clip_hi ? clip_hi : ratio);
  const float s1 = ratio * A, s2 = rc * A;
  e.el = -((s2 < s1 || s2 != s2) ? s2 : s1);   // torch.min: NaN wins
  e.ek = dl;
  // torch.minimum's backward: the smaller one takes the gradient, equal ones half each (inside the range the two halves add up);
  // clamp passes inside and on its bounds
  const double w1 = s1 > s2 ? 0.0 : (s1 == s2 ? 0.5 : 1.0), w2 = s1 < s2 ? 0.0 : (s1 == s2 ? 0.5 : 1.0);
  const double pr = (ratio >= clip_lo && ratio <= clip_hi) ? 1.0 : 0.0;
  const double pl = (dl >= -20.0f && dl <= 20.0f) ? 1.0 : 0.0;
  const double dlp = (G * (double)A * (w1 + w2 * pr)) * (double)ratio * pl;
  const double dm = (double)act - (double)mu, S = (double)sd;
  e.gmu = (float)(dlp * dm / (S * S));
  __builtin_amdgcn_sched_barrier(0);   // (one double-precision quotient chain at a time, section 19's remedy: interleaved, their temporaries cost registers)
  const double gsd = dlp * (dm * dm / (S * S * S) - 1.0 / S);
  const double ps = (sp >= min_std && sp <= max_std) ? 1.0 : 0.0;
  const double sg = z > 20.0f ? 1.0 : 1.0 / (1.0 + exp(-(double)z));
  e.gz = (float)(gsd * ps * sg);
  return e;
}

struct PpoReduceArgs {
  const float* ws;
  const int32_t* table;
  const int32_t* vtable;
  const int32_t* flags;
  float* raw_a;            // the unclipped gradient packs
  float* raw_v;
  double* parts;           // [n_agents][2][PEDN_PG_BLOCKS]: the workgroups' parts of sum g^2
  float* scalars;          // [PEDN_PG_SCALARS][n_agents]
  int64_t rows, apack4, vpack, ws_stride;
  int32_t G, S, n_agents;
};

// The reduce launch's workgroup (grid (16, n_agents, 2), 256 threads) for the network at [off, off + len) of its pack: the slabs added from
// +0.0, g ascending, into the unclipped gradient pack; the losses and approx_kl; the workgroup's part of sum g^2 in double (a thread's
// elements ascending, then a halving tree over the 256 threads in sRed).
__device__ __forceinline__ void pg_reduce_body(const PpoReduceArgs& a, int off, int len, double* sRed) {
  const int tid = (int)threadIdx.x, agent = (int)blockIdx.y;
  const bool is_actor = blockIdx.z != 0;
  const float* src = a.ws + (is_actor ? (int64_t)off : a.apack4 + (int64_t)off);
  float* raw = (is_actor ? a.raw_a : a.raw_v) + off;
  double sq = 0.0;
  for (int i = (int)blockIdx.x * 256 + tid; i < len; i += PEDN_PG_BLOCKS * 256) {
    float g = 0.0f;
    for (int s = 0; s < a.G; ++s) g = g + src[(int64_t)s * a.ws_stride + i];   // slabs ascending
    raw[i] = g;
    sq = sq + (double)g * (double)g;
  }
  sRed[tid] = sq;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) sRed[tid] = sRed[tid] + sRed[tid + h];
    __syncthreads();
  }
  if (tid == 0) a.parts[((size_t)agent * 2 + (is_actor ? 1 : 0)) * PEDN_PG_BLOCKS + blockIdx.x] = sRed[0];
  if (blockIdx.x == 0 && tid == 0) {
    // the three sums are doubles: slabs ascending from +0.0, the mean in double, rounded once
    const float* sums = a.ws + a.apack4 + a.vpack + (int64_t)PEDN_PG_SUMS * agent;
    if (is_actor) {
      double l = 0.0, k = 0.0;
      for (int s = 0; s < a.G; ++s) {
        const double* d = reinterpret_cast<const double*>(sums + (int64_t)s * a.ws_stride);
        l = l + d[0];
        k = k + d[1];
      }
      const double cnt = (double)a.rows * (double)a.table[(size_t)agent * PEDN_ACTOR_TABLE_COLS + 3];
      a.scalars[agent] = (float)(l / cnt);
      a.scalars[2 * a.n_agents + agent] = (float)(k / cnt);
    } else {
      double q = 0.0;
      for (int s = 0; s < a.G; ++s) q = q + reinterpret_cast<const double*>(sums + (int64_t)s * a.ws_stride)[2];
      a.scalars[a.n_agents + agent] = (float)(q / (double)a.rows);
    }
  }
}

struct PpoAdamArgs {
  const int32_t* table;
  const int32_t* vtable;
  int32_t* flags;
  const float* raw_a;
  const float* raw_v;
  const double* parts;
  float *g_a, *g_v, *m_a, *m_v, *v_a, *v_v, *p_a, *p_v;   // per network: the clipped gradients, exp_avg, exp_avg_sq, the parameters
  float* scalars;
  int64_t* state;          // [n_agents][4]: pedn_adam.hpp's step state of every agent
  int32_t S, n_agents, do_adam;
  float max_norm;
  double lr_a, lr_v, beta1, beta2, kl_stop;   // kl_stop = 1.5 * kl_tolerance
  AdamCoef coef;
};

// The Adam launch's workgroup (grid (16, n_agents, 2), 256 threads) for the network at [off, off + len) of its pack: total_norm =
// (float)sqrt(the 16 parts, ascending), clip_grad_norm_'s coefficient, the clipped gradients and, unless switched off, section 19's Adam
// step with the agent's own step count; the last workgroup of an agent (section 14's ticket) advances its count and sets its stop flag.
__device__ __forceinline__ void pg_adam_body(const PpoAdamArgs& a, int off, int len) {
  const int tid = (int)threadIdx.x, agent = (int)blockIdx.y;
  const bool is_actor = blockIdx.z != 0;
  int64_t* st = a.state + 4 * (size_t)agent;
  const AdamStep step = adam_step_begin(st, a.beta1, a.beta2);
  const float nstep = adam_nstep(is_actor ? a.lr_a : a.lr_v, step), s = step.s;
  // clip_grad_norm_: total_norm over the network's tensors, coef = min(max_norm / (total_norm + 1e-6), 1), g = g * coef
  const double* parts = a.parts + ((size_t)agent * 2 + (is_actor ? 1 : 0)) * PEDN_PG_BLOCKS;
  double total = 0.0;
  for (int b = 0; b < PEDN_PG_BLOCKS; ++b) total = total + parts[b];
  const float norm = (float)sqrt(total);
  float coef = a.max_norm / (norm + 1e-6f);
  coef = coef > 1.0f ? 1.0f : coef;   // (NaN stays, as torch's clamp leaves it)
  const float* raw = (is_actor ? a.raw_a : a.raw_v) + off;
  float* gr = (is_actor ? a.g_a : a.g_v) + off;
  float* mm = (is_actor ? a.m_a : a.m_v) + off;
  float* vv = (is_actor ? a.v_a : a.v_v) + off;
  float* pp = (is_actor ? a.p_a : a.p_v) + off;
  for (int i = (int)blockIdx.x * 256 + tid; i < len; i += (int)gridDim.x * 256) {
    const float g = raw[i] * coef;
    gr[i] = g;
    if (a.do_adam) {
      float m = mm[i], v = vv[i];
      const float p = adam_one<true>(g, m, v, pp[i], a.coef, nstep, s);
      mm[i] = m; vv[i] = v; pp[i] = p;
    }
  }
  if (blockIdx.x == 0 && tid == 0) {
    a.scalars[(3 + (is_actor ? 0 : 1)) * a.n_agents + agent] = norm;
    a.scalars[(5 + (is_actor ? 0 : 1)) * a.n_agents + agent] = coef;
  }
  if (!a.do_adam) return;
  __syncthreads();   // every wave of the workgroup has read the flag and the step state
  // the last workgroup of the agent's two networks advances its state and takes the reference's early stop: behind the step of an epoch
  // whose approx_kl > 1.5 * kl_tolerance (this epoch's reduce launch wrote it)
  if (tid == 0 && adam_step_advance(st, step, 2u * gridDim.x) && (double)a.scalars[2 * a.n_agents + agent] > a.kl_stop)
    __hip_atomic_store(a.flags + agent, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
