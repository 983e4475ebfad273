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

struct GaeRows { float r[PEDN_GAE_UNROLL], v[PEDN_GAE_UNROLL], d[PEDN_GAE_UNROLL], n[PEDN_GAE_UNROLL]; };

// rows t - 1, t - 2, ..., t - PEDN_GAE_UNROLL of one lane; nx: the rows' next values where they are an array of their own (pedn_gae_next)
template <bool DELTA>
__device__ __forceinline__ void gae_load(GaeRows& b, const float* rew, const float* val, const float* done, const float* nx, int t, size_t L, size_t DL) {
#pragma unroll
  for (int j = 0; j < PEDN_GAE_UNROLL; ++j) {
    const size_t row = (size_t)(t - 1 - j);
    b.r[j] = rew[row * L];
    b.v[j] = DELTA ? 0.0f : val[row * L];
    b.d[j] = DELTA ? 0.0f : done[row * DL];
    b.n[j] = !DELTA && nx ? nx[row * L] : 0.0f;
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
// one per env: done_div = n_agents).  nx (or null) [T][lanes]: row t's next value is nx[t] instead of val[t + 1], and val has T rows
// (pedn_gae_next).  DELTA: rew holds td_delta; val, done, nx and td are not touched.
template <bool DELTA>
__global__ __launch_bounds__(256) void rollout_gae_kernel(const float* rew, const float* val, const float* done, const float* nx, int T, int lanes,
                                                          int done_div, float g, float c, float* td, float* adv) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= lanes) return;
  const size_t L = (size_t)lanes, DL = (size_t)(lanes / done_div);
  rew += i; adv += i;
  if (!DELTA) { val += i; td += i; done += i / done_div; }
  if (!DELTA && nx) nx += i;   // (uniform over the launch)
  float carry = 0.0f;
  float vnext = DELTA || nx ? 0.0f : val[(size_t)T * L];
  int t = T;
  if (t >= PEDN_GAE_UNROLL) {
    GaeRows cur, nxt;
    gae_load<DELTA>(cur, rew, val, done, nx, t, L, DL);
    nxt = cur;
    while (t >= PEDN_GAE_UNROLL) {
      const int tn = t - PEDN_GAE_UNROLL;
      if (tn >= PEDN_GAE_UNROLL) gae_load<DELTA>(nxt, rew, val, done, nx, tn, L, DL);   // in flight while the chain below runs
#pragma unroll
      for (int j = 0; j < PEDN_GAE_UNROLL; ++j) {
        const size_t row = (size_t)(t - 1 - j);
        vnext = gae_row<DELTA>(cur.r[j], cur.v[j], cur.d[j], !DELTA && nx ? cur.n[j] : vnext, g, c, carry, td + row * L, adv + row * L);
      }
      cur = nxt;
      t = tn;
    }
  }
  for (; t >= 1; --t) {   // the rows that do not fill a block
    const size_t row = (size_t)(t - 1);
    vnext = gae_row<DELTA>(rew[row * L], DELTA ? 0.0f : val[row * L], DELTA ? 0.0f : done[row * DL], !DELTA && nx ? nx[row * L] : vnext, g, c, carry, td + row * L, adv + row * L);
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

// ---- host side: pedn_rollout_* and pedn_gae of include/pedn.h.  State: pedn_sim::ro (store_drop, store_sources: pedn_host.hpp)
static unsigned rollout_blocks(size_t elems) { return (unsigned)std::min<size_t>(std::max<size_t>((elems + 1023) / 1024, 1), 2048); }

int pedn_rollout_free(pedn_sim* s) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);   // (ends a clocked section: a captured record launch is not replayed over freed rows, pedn_rl_clock_signature)
  HIP_TRY(s, hipDeviceSynchronize());
  store_drop(s->ro);
  return PEDN_OK;
}

int pedn_rollout_configure(pedn_sim* s, int32_t capacity, int32_t store_obs) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->rl_ready) return fail(s, PEDN_E_ARG, "pedn_rl_configure has not been called");
  if (capacity < 1) return fail(s, PEDN_E_ARG, "capacity < 1");
  int rc = pedn_rollout_free(s);
  if (rc != PEDN_OK) return rc;
  const RlView& q = s->rl;
  const size_t N = (size_t)s->v.R, cap = (size_t)capacity, nv = N * q.n_agents;
  if (nv > 0x7fffffffull) return fail(s, PEDN_E_ARG, "more than 2^31 trajectories");   // (a lane index is an int; rows are addressed in 64 bits)
  RolloutView r;
  memset(&r, 0, sizeof r);   // (padding too: the view is hashed as bytes, pedn_rl_clock_signature)
  DevicePool& mem = s->ro.mem;
  if ((rc = mem.take(s, cap * N * q.A * sizeof(double), (void**)&r.actions)) != PEDN_OK || (rc = mem.take(s, (cap + 1) * nv * sizeof(float), (void**)&r.values)) != PEDN_OK ||
      (rc = mem.take(s, cap * nv * sizeof(float), (void**)&r.rewards)) != PEDN_OK || (rc = mem.take(s, cap * N * sizeof(float), (void**)&r.done)) != PEDN_OK ||
      (rc = mem.take(s, cap * nv * sizeof(float), (void**)&r.td_target)) != PEDN_OK || (rc = mem.take(s, cap * nv * sizeof(float), (void**)&r.adv)) != PEDN_OK ||
      (rc = mem.take(s, cap * nv * sizeof(float), (void**)&r.adv_n)) != PEDN_OK || (rc = mem.take(s, 2 * cap * q.n_agents * sizeof(double), (void**)&r.rowsum)) != PEDN_OK ||
      (rc = mem.take(s, 4 * sizeof(int32_t), (void**)&r.state)) != PEDN_OK ||
      (store_obs && (rc = mem.take(s, (cap + 1) * N * q.O * sizeof(float), (void**)&r.obs)) != PEDN_OK)) {
    const std::string keep = s->err;
    store_drop(s->ro);
    return fail(s, rc, keep);
  }
  r.clock = s->d_clock;
  r.cap = capacity; r.N = s->v.R; r.A = q.n_agents; r.n_actions = q.A; r.n_obs = q.O; r.T = s->v.T1 - 1;
  s->ro.view = r;
  s->ro.on = true;
  store_sources(s);
  return PEDN_OK;
}

int pedn_rollout_begin(pedn_sim* s) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->ro.on) return fail(s, PEDN_E_ARG, "pedn_rollout_configure has not been called");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);   // (ends a clocked section: the cursor goes back behind everything recorded so far)
  const RolloutView& r = s->ro.view;
  hipLaunchKernelGGL(rollout_begin_kernel, dim3(rollout_blocks(r.obs ? (size_t)r.N * r.n_obs : 1)), dim3(256), 0, s->stream, r);
  HIP_TRY(s, hipGetLastError());
  s->ro.begun = true;
  s->ro.finished = false;
  s->ro.rows = 0;
  return PEDN_OK;
}

// (no allocation, no synchronisation, no event query: safe under stream capture)
int pedn_rollout_record(pedn_sim* s, const double* actions, const float* values, int32_t term, void* stream) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->ro.on || !s->ro.begun) return fail(s, PEDN_E_ARG, "pedn_rollout_begin has not been called");
  HIP_TRY(s, hipSetDevice(s->device));
  const RolloutView& r = s->ro.view;
  hipStream_t st = stream ? (hipStream_t)stream : s->stream;
  const size_t widest = (size_t)r.N * std::max(std::max(r.obs ? r.n_obs : 0, 2 * r.n_actions), r.A);
  hipLaunchKernelGGL(rollout_record_kernel, dim3(rollout_blocks(widest)), dim3(256), 0, st, r, actions, values, s->clocked ? -1 : (term ? 1 : 0));
  HIP_TRY(s, hipGetLastError());
  s->ro.finished = false;
  return PEDN_OK;
}

int pedn_rollout_finish(pedn_sim* s, const float* last_values, int32_t* rows, int32_t* overflow) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->ro.on || !s->ro.begun) return fail(s, PEDN_E_ARG, "pedn_rollout_begin has not been called");
  HIP_TRY(s, hipSetDevice(s->device));
  join_forked(s);   // (ends a clocked section)
  HIP_TRY(s, hipDeviceSynchronize());   // records may sit on a caller's stream
  const RolloutView& r = s->ro.view;
  int32_t h[4] = {0, 0, 0, 0};
  HIP_TRY(s, hipMemcpy(h, r.state, sizeof h, hipMemcpyDeviceToHost));
  const int n = std::min(h[0], r.cap);
  const size_t nv = (size_t)r.N * r.A;
  if (last_values) HIP_TRY(s, hipMemcpy(r.values + (size_t)n * nv, last_values, nv * sizeof(float), hipMemcpyDeviceToDevice));
  else HIP_TRY(s, hipMemset(r.values + (size_t)n * nv, 0, nv * sizeof(float)));
  HIP_TRY(s, hipDeviceSynchronize());
  s->ro.rows = n;
  s->ro.finished = true;
  if (rows) *rows = n;
  if (overflow) *overflow = h[2];
  return PEDN_OK;
}

static void gae_launch(const float* rew, const float* val, const float* done, const float* nx, int T, int lanes, int done_div, double gamma, double lmbda,
                       float* td, float* adv, hipStream_t st) {
  const float g = (float)gamma, c = (float)(gamma * lmbda);   // (the product in binary64, rounded once)
  const dim3 grid((unsigned)((lanes + 255) / 256));
  if (val) hipLaunchKernelGGL(rollout_gae_kernel<false>, grid, dim3(256), 0, st, rew, val, done, nx, T, lanes, done_div, g, c, td, adv);
  else hipLaunchKernelGGL(rollout_gae_kernel<true>, grid, dim3(256), 0, st, rew, val, done, nx, T, lanes, done_div, g, c, td, adv);
}

int pedn_rollout_compute(pedn_sim* s, double gamma, double lmbda, int32_t normalize) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->ro.on || !s->ro.finished) return fail(s, PEDN_E_ARG, "pedn_rollout_finish has not been called");
  const RolloutView& r = s->ro.view;
  const int T = s->ro.rows;
  if (T < 1) return fail(s, PEDN_E_ARG, "the store is empty");
  if (normalize && (int64_t)T * r.N < 2) return fail(s, PEDN_E_ARG, "advantage normalisation needs at least two entries per agent");
  HIP_TRY(s, hipSetDevice(s->device));
  gae_launch(r.rewards, r.values, r.done, nullptr, T, r.N * r.A, r.A, gamma, lmbda, r.td_target, r.adv, s->stream);
  if (normalize) {
    const dim3 grid((unsigned)((r.A + PEDN_NORM_COLS - 1) / PEDN_NORM_COLS), (unsigned)T);
    for (int pass = 0; pass < 3; ++pass)   // (a launch per pass: each needs every workgroup's row sums of the one before)
      hipLaunchKernelGGL(rollout_advnorm_kernel, grid, dim3(1024), 0, s->stream, r.adv, r.adv_n, r.rowsum, T, r.N, r.A, pass);
  }
  HIP_TRY(s, hipGetLastError());
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return PEDN_OK;
}

void* pedn_rollout_device_ptr(pedn_sim* s, int32_t which) {
  if (!s || !s->ro.on) return nullptr;
  const RolloutView& r = s->ro.view;
  switch (which) {
    case 0: return r.actions;
    case 1: return r.values;
    case 2: return r.rewards;
    case 3: return r.done;
    case 4: return r.obs;
    case 5: return r.td_target;
    case 6: return r.adv;
    case 7: return r.adv_n;
    case 8: return r.state;
  }
  return nullptr;
}

int pedn_gae(const float* rewards, const float* values, const float* dones, int32_t T, int32_t lanes, double gamma, double lmbda,
             float* td_target, float* adv, void* stream) {
  if (!rewards || !adv || (values && (!dones || !td_target))) return fail(nullptr, PEDN_E_ARG, "null argument");
  if (T < 1 || lanes < 1) return fail(nullptr, PEDN_E_ARG, "T and lanes must be positive");
  gae_launch(rewards, values, dones, nullptr, T, lanes, 1, gamma, lmbda, td_target, adv, (hipStream_t)stream);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}

int pedn_gae_next(const float* rewards, const float* values, const float* next_values, const float* dones, int32_t T, int32_t lanes,
                  double gamma, double lmbda, float* td_target, float* adv, void* stream) {
  if (!rewards || !values || !next_values || !dones || !td_target || !adv) return fail(nullptr, PEDN_E_ARG, "null argument");
  if (T < 1 || lanes < 1) return fail(nullptr, PEDN_E_ARG, "T and lanes must be positive");
  gae_launch(rewards, values, dones, next_values, T, lanes, 1, gamma, lmbda, td_target, adv, (hipStream_t)stream);
  HIP_TRY(nullptr, hipGetLastError());
  return PEDN_OK;
}
