// On-policy rollout store of the env batch and the reference's advantage estimates (rl/agents/PPO_org.py:201-354, 518-567:
// store_transition, td_target / td_delta, rl/rl_utils.py:1754-1773 compute_gae, advantage normalisation).  The contract is DESIGN
// section 12; tests/rollout_model.py restates it in numpy.
//
// The store is device-resident, every array [row][env][...]: actions f64 [cap][N][n_actions], values f32 [cap + 1][N][A], rewards f32
// [cap][N][A], done f32 [cap][N], observations f32 [cap + 1][N][n_obs] (optional).  state[0] is the row cursor, state[1] a ticket counter,
// state[2] the overflow flag.
//
// rollout_record_kernel   one launch per policy step with constant arguments (it is captured with the step): row k = state[0] of every
//                         array is written from the caller's action / value rows and the engine's observation / reward buffers; the last
//                         workgroup to finish (ticket counter, vector atomics) advances the cursor.  k >= cap: nothing is written,
//                         state[2] = 1.
// rollout_gae_kernel      lane = one (env, agent) trajectory, walked backwards in time.  IEEE binary32, nothing fused:
//                           td_target[t] = r[t] + (g * v[t + 1]) * (1 - done[t]);  delta = td_target[t] - v[t]
//                           carry = c * carry + delta;  adv[t] = carry            (carry starts at +0.0, it is NOT masked by done)
//                         The loads of a block of PEDN_GAE_UNROLL rows are issued one block ahead of the chain that consumes them.
// rollout_advnorm_kernel  (x - mean) / (std + 1e-8) per agent over all T * N entries in binary64, three launches (pass 0, 1, 2): row sums
//                         over the env axis in the order S of pedn_norm.hpp, the T row sums added in increasing t.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_norm.hpp"

#define PEDN_GAE_UNROLL 8

struct RolloutView {
  const float *obs_src, *rew_src;   // what the fetches hand out: the normalised rows while the running normalisation is on
  double* actions;
  float *values, *rewards, *done, *obs;   // obs: NULL when observations are not kept
  float *td_target, *adv, *adv_n;         // [cap][N][A] each
  double* rowsum;                         // [2][cap][A]: row sums of the two normalisation passes
  int32_t* state;                         // cursor, ticket, overflow, (unused)
  const int32_t* clock;                   // the device-resident step clock
  int32_t cap, N, A, n_actions, n_obs, T, pad_[2];
};

__device__ __forceinline__ void rollout_copy_f32(float* dst, const float* src, size_t n, size_t tid, size_t nth) {
  if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0 && (n & 3) == 0) {   // (uniform over the launch)
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (size_t i = tid; i < n / 4; i += nth) d4[i] = s4[i];
  } else
    for (size_t i = tid; i < n; i += nth) dst[i] = src[i];
}

// obs[0] = the current observation, cursor / ticket / overflow back to 0
__global__ __launch_bounds__(256) void rollout_begin_kernel(RolloutView r) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  if (tid < 4) r.state[tid] = 0;
  if (r.obs) rollout_copy_f32(r.obs, r.obs_src, (size_t)r.N * r.n_obs, tid, nth);
}

// term: the step's terminated flag, or -1: read it from the step clock (the convention of norm_kernel)
__global__ __launch_bounds__(256) void rollout_record_kernel(RolloutView r, const double* actions, const float* values, int term) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  const int k = r.state[0];
  if (k < r.cap) {   // (uniform over the launch: the cursor moves only after every workgroup has taken its ticket)
    const size_t N = (size_t)r.N, na = N * r.n_actions, nv = N * r.A, no = N * r.n_obs;
    const float done = (term < 0 ? r.clock[1] >= r.T : term != 0) ? 1.0f : 0.0f;
    double* da = r.actions + (size_t)k * na;
    for (size_t i = tid; i < na; i += nth) da[i] = actions ? actions[i] : 0.0;
    float* dv = r.values + (size_t)k * nv;
    if (values) rollout_copy_f32(dv, values, nv, tid, nth);
    else
      for (size_t i = tid; i < nv; i += nth) dv[i] = 0.0f;
    rollout_copy_f32(r.rewards + (size_t)k * nv, r.rew_src, nv, tid, nth);
    for (size_t i = tid; i < N; i += nth) r.done[(size_t)k * N + i] = done;
    if (r.obs) rollout_copy_f32(r.obs + (size_t)(k + 1) * no, r.obs_src, no, tid, nth);
  } else if (tid == 0)
    r.state[2] = 1;
  // every lane's stores are addressed through k, so the workgroup has read the cursor by the time its ticket is taken
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned* ticket = reinterpret_cast<unsigned*>(r.state + 1);
    const unsigned mine = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (mine + 1u == gridDim.x) {   // the last one: nobody reads the cursor any more
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(r.state, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

struct GaeRows { float r[PEDN_GAE_UNROLL], v[PEDN_GAE_UNROLL], d[PEDN_GAE_UNROLL]; };

// rows t - 1, t - 2, ..., t - PEDN_GAE_UNROLL of one lane
template <bool DELTA>
__device__ __forceinline__ void gae_load(GaeRows& b, const float* rew, const float* val, const float* done, int t, size_t L, size_t DL) {
#pragma unroll
  for (int j = 0; j < PEDN_GAE_UNROLL; ++j) {
    const size_t row = (size_t)(t - 1 - j);
    b.r[j] = rew[row * L];
    b.v[j] = DELTA ? 0.0f : val[row * L];
    b.d[j] = DELTA ? 0.0f : done[row * DL];
  }
}

// DELTA: `r` is td_delta itself (compute_gae's own argument): no TD target, v / d / vnext are not used
template <bool DELTA>
__device__ __forceinline__ float gae_row(float r, float v, float d, float vnext, float g, float c, float& carry, float* td, float* adv) {
  float delta = r;
  if (!DELTA) {
    const float tt = __fadd_rn(r, __fmul_rn(__fmul_rn(g, vnext), __fsub_rn(1.0f, d)));
    delta = __fsub_rn(tt, v);
    *td = tt;
  }
  carry = __fadd_rn(__fmul_rn(c, carry), delta);
  *adv = carry;
  return v;
}

// rew, td, adv [T][lanes]; val [T + 1][lanes]; done [T][lanes / done_div], read at lane / done_div (1: a flag per lane; the store keeps
// one per env: done_div = n_agents).  DELTA: rew holds td_delta; val, done and td are not touched.
template <bool DELTA>
__global__ __launch_bounds__(256) void rollout_gae_kernel(const float* rew, const float* val, const float* done, int T, int lanes, int done_div,
                                                          float g, float c, float* td, float* adv) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= lanes) return;
  const size_t L = (size_t)lanes, DL = (size_t)(lanes / done_div);
  rew += i; adv += i;
  if (!DELTA) { val += i; td += i; done += i / done_div; }
  float carry = 0.0f;
  float vnext = DELTA ? 0.0f : val[(size_t)T * L];
  int t = T;
  if (t >= PEDN_GAE_UNROLL) {
    GaeRows cur, nxt;
    gae_load<DELTA>(cur, rew, val, done, t, L, DL);
    nxt = cur;
    while (t >= PEDN_GAE_UNROLL) {
      const int tn = t - PEDN_GAE_UNROLL;
      if (tn >= PEDN_GAE_UNROLL) gae_load<DELTA>(nxt, rew, val, done, tn, L, DL);   // in flight while the chain below runs
#pragma unroll
      for (int j = 0; j < PEDN_GAE_UNROLL; ++j) {
        const size_t row = (size_t)(t - 1 - j);
        vnext = gae_row<DELTA>(cur.r[j], cur.v[j], cur.d[j], vnext, g, c, carry, td + row * L, adv + row * L);
      }
      cur = nxt;
      t = tn;
    }
  }
  for (; t >= 1; --t) {   // the rows that do not fill a block
    const size_t row = (size_t)(t - 1);
    vnext = gae_row<DELTA>(rew[row * L], DELTA ? 0.0f : val[row * L], DELTA ? 0.0f : done[row * DL], vnext, g, c, carry, td + row * L, adv + row * L);
  }
}

// x, out [T][N][A]; rs [2][T][A].  Grid (ceil(A / 16), T): a workgroup owns 16 agent columns of one time row, lanes laid out as in
// norm_kernel (16 lanes = 64 consecutive bytes of one env's row, 64 row slots = the strands of S).
//   pass 0  rs[0][t][a] = S(x[t][:][a])                        pass 1  mean from rs[0]; rs[1][t][a] = S((x[t][:][a] - mean)^2)
//   pass 2  mean, std from rs; out = f32((x - mean) / (std + 1e-8))
__global__ __launch_bounds__(1024) void rollout_advnorm_kernel(const float* x, float* out, double* rs, int T, int N, int A, int pass) {
  __shared__ double sP[PEDN_NORM_STRANDS][PEDN_NORM_COLS];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int sub = lane >> 4, col = lane & 15;
  const int s = wave * 4 + sub;
  const int c = (int)blockIdx.x * PEDN_NORM_COLS + col, t = (int)blockIdx.y;
  const bool cin = c < A;
  const int cc = cin ? c : 0;
  const int cnt = N < PEDN_NORM_STRANDS ? N : PEDN_NORM_STRANDS;
  const double n = (double)T * (double)N;
  const size_t TA = (size_t)T * A;
  const float* xr = x + (size_t)t * N * A + cc;
  double mean = 0.0;
  if (pass >= 1) {   // (uniform) the T row sums in increasing t
    double tot = rs[cc];
    for (int u = 1; u < T; ++u) tot = tot + rs[(size_t)u * A + cc];
    mean = tot / n;
  }
  if (pass == 2) {
    double q = rs[TA + cc];
    for (int u = 1; u < T; ++u) q = q + rs[TA + (size_t)u * A + cc];
    const double sd = sqrt(q / (n - 1.0)) + 1e-8;
    if (cin) {
      float* o = out + (size_t)t * N * A + c;
      for (int e = s; e < N; e += PEDN_NORM_STRANDS) o[(size_t)e * A] = (float)(((double)xr[(size_t)e * A] - mean) / sd);
    }
    return;
  }
  double acc = 0.0;
  if (cin && s < N) {
    if (pass == 0) {
      acc = (double)xr[(size_t)s * A];
      for (int e = s + PEDN_NORM_STRANDS; e < N; e += PEDN_NORM_STRANDS) acc = acc + (double)xr[(size_t)e * A];
    } else {
      double d = (double)xr[(size_t)s * A] - mean;
      acc = d * d;
      for (int e = s + PEDN_NORM_STRANDS; e < N; e += PEDN_NORM_STRANDS) { d = (double)xr[(size_t)e * A] - mean; acc = acc + d * d; }
    }
  }
  sP[s][col] = acc;
  __syncthreads();
  const double sum = norm_tree_lds(sP, col, sub, cnt);
  if (cin && s == 0) rs[(size_t)pass * TA + (size_t)t * A + c] = sum;
}
