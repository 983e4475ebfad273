// Off-policy replay buffer of the env batch (rl/rl_utils.py:37-50 ReplayBuffer under rl/agents/SAC.py:127-225
// train_off_policy_multi_agent): a device-resident ring of transitions that keeps every observation ONCE, and a gather of sampled
// minibatches as stacks of the last `stack` observations.  The contract is DESIGN section 13; tests/replay_model.py restates it in numpy.
//
// Every begin / push takes the next serial s (int64, device memory) and writes slot s mod R of the ring: frames f32 [R][N][n_obs],
// actions f64 [R][N][n_actions], rewards f32 [R][N][A], done f32 [R], first i64 [R] (the serial of the row's RESET row; -1: the row is a
// RESET row itself).  step_serial i64 [cap] maps the running STEP count j (slot j mod cap) to its serial.
// state (i64): 0 head (the next serial), 1 jhead (STEP rows so far), 2 size_rows, 3 first of the running episode (-1 before the first
// begin), 4 draw counter, 5 error flag, 6 push ticket, 7 sample ticket (the low 32 bits of each), 8 head mod R, 9 jhead mod cap (kept
// by the push launch, so that no kernel divides: the slot of serial x is state[8] - (head - x), plus R when that is negative).
//
// replay_push_kernel     one launch per begin / policy step with constant arguments (it is captured with the step): the slot of serial
//                        head is written from the caller's action rows and the engine's observation / reward buffers, and `stacked`
//                        [N][stack][n_obs] gets the next state of the new row (older frames are read back from the ring: no launch
//                        of this kernel writes them).  The last workgroup to finish (ticket counter, vector atomics) writes the two
//                        tables' entries, advances head / jhead and brings size_rows up to date -- nothing this lane reads is written
//                        by another lane of the same launch.
// replay_sample_kernel   a workgroup takes PEDN_REPLAY_GROUP samples at a time: one lane per sample draws (or reads) its (serial, env),
//                        validates it against the ring and leaves the row's slot, env and stack depth in LDS; then a wave per sample copies the
//                        stack + 1 distinct frame slices (each loaded once, stored into the state and / or the next state), the action,
//                        reward and done entries.  A sample that is not sampleable writes nothing and raises state[5].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_math.hpp"

#define PEDN_REPLAY_GROUP 8   // samples per workgroup pass (4 waves: two samples each)

// n 4-byte words; 16-byte accesses when both ends allow (uniform over the caller's lanes)
__device__ __forceinline__ void replay_copy_words(uint32_t* dst, const uint32_t* src, size_t n, size_t tid, size_t nth) {
  if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0 && (n & 3) == 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (size_t i = tid; i < n / 4; i += nth) d4[i] = s4[i];
  } else
    for (size_t i = tid; i < n; i += nth) dst[i] = src[i];
}

__device__ __forceinline__ int64_t replay_max(int64_t a, int64_t b) { return a > b ? a : b; }

// reset != 0: a RESET row (the frame only; the running episode starts here).  term: the step's terminated flag, or -1: read it from
// the step clock (the convention of rollout_record_kernel).  Grid: blockIdx.y = 0 copies the row, blockIdx.y = 1 writes `stacked`.
__global__ __launch_bounds__(256) void replay_push_kernel(ReplayView r, const double* actions, int reset, int term) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  const int64_t s = r.state[0], j = r.state[1];
  const size_t slot = (size_t)r.state[8];
  const int64_t q = reset ? s : r.state[3];   // (uniform over the launch: the state moves only after every workgroup has taken its ticket)
  const size_t N = (size_t)r.N, no = N * r.n_obs;
  if (blockIdx.y == 0) {
    replay_copy_words(reinterpret_cast<uint32_t*>(r.frames + slot * no), reinterpret_cast<const uint32_t*>(r.obs_src), no, tid, nth);
    if (!reset) {
      const size_t na = N * r.n_actions, nr = N * r.A;
      replay_copy_words(reinterpret_cast<uint32_t*>(r.actions + slot * na), reinterpret_cast<const uint32_t*>(actions), 2 * na, tid, nth);
      replay_copy_words(reinterpret_cast<uint32_t*>(r.rewards + slot * nr), reinterpret_cast<const uint32_t*>(r.rew_src), nr, tid, nth);
      if (tid == 0) r.done[slot] = (term < 0 ? r.clock[1] >= r.T : term != 0) ? 1.0f : 0.0f;
    }
  } else {
    // stacked[e][i] = frame max(s - stack + 1 + i, q) of env e; i = stack - 1 is the new observation, the others sit in the ring,
    // min(stack - 1 - i, s - q) slots behind this one.  A lane per 16 bytes (4 bytes when a row is no multiple of 16), 32-bit indices.
    const unsigned w = (unsigned)r.n_obs, S = (unsigned)r.stack;
    const bool v4 = (w & 3) == 0;   // (every row of every array then starts on 16 bytes)
    const unsigned wq = v4 ? w / 4 : w, total = (unsigned)r.N * S * wq;
    const int64_t back = s - q;
    for (unsigned x = (unsigned)tid; x < total; x += (unsigned)nth) {
      const unsigned p = x / wq, c = x - p * wq, e = p / S, i = p - e * S;
      const int64_t m = back < (int64_t)(S - 1 - i) ? back : (int64_t)(S - 1 - i);
      const int64_t fs = (int64_t)slot - m + ((int64_t)slot < m ? r.R : 0);
      const float* src = m == 0 ? r.obs_src + (size_t)e * w : r.frames + ((size_t)fs * N + e) * w;
      float* dst = r.stacked + (size_t)p * w;
      if (v4) reinterpret_cast<uint4*>(dst)[c] = reinterpret_cast<const uint4*>(src)[c];
      else reinterpret_cast<uint32_t*>(dst)[c] = reinterpret_cast<const uint32_t*>(src)[c];
    }
  }
  // every lane's stores are addressed through s, so the workgroup has read the state by the time its ticket is taken
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned* ticket = reinterpret_cast<unsigned*>(r.state + 6);
    const unsigned mine = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (mine + 1u == gridDim.x * gridDim.y) {   // the last one: nobody reads the state any more
      const int64_t head = s + 1, nslot = (int64_t)slot + 1 == r.R ? 0 : (int64_t)slot + 1;
      int64_t size = r.state[2], njslot = r.state[9];
      r.first[slot] = reset ? -1 : q;
      if (!reset) {
        r.step_serial[njslot] = s;
        njslot = njslot + 1 == r.cap ? 0 : njslot + 1;
        size = size < r.cap ? size + 1 : r.cap;
      }
      const int64_t jhead = reset ? j : j + 1;
      // rows whose oldest frame has left the ring go: they are the oldest ones (the bound is monotone in the serial), and one launch
      // evicts one frame, which at most `stack` rows share as their oldest (the rows behind a RESET row)
      for (int it = 0; it <= r.stack && size > 0; ++it) {
        const int64_t jo = jhead - size;
        int64_t so = s, qo = q;
        if (jo != j) {   // (rank j is the row of this launch: its entries are this lane's own, taken from registers)
          so = r.step_serial[njslot - size + (njslot < size ? r.cap : 0)];
          const int64_t ago = head - so;   // (<= R: the row was sampleable after the launch before)
          if (ago > r.R) { --size; continue; }
          qo = r.first[nslot - ago + (nslot < ago ? r.R : 0)];
        }
        if (replay_max(so - r.stack, qo) >= head - r.R) break;
        --size;
      }
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(r.state + 2, size, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(r.state + 8, nslot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(r.state + 9, njslot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(r.state + 1, jhead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (reset) __hip_atomic_store(r.state + 3, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(r.state, head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Which columns a sample hands out and where: observation columns [obs0, obs0 + obs_w), action columns [act0, act0 + act_w), reward
// columns [rew0, rew0 + rew_w); states / next_states [B][stack][obs_w], actions [B][act_w], rewards [B][rew_w], dones [B], idx [B][2].
struct ReplayOut {
  float *states, *next_states, *rewards, *dones;
  double* actions;
  int64_t* idx;
  int32_t obs0, obs_w, act0, act_w, rew0, rew_w;
};

// given: [B][2] (serial, env) pairs to gather, or NULL: draw them (draw d = state[4], advanced by the last workgroup)
// Grid: ceil(B / PEDN_REPLAY_GROUP) workgroups.
__global__ __launch_bounds__(256) void replay_sample_kernel(ReplayView r, ReplayOut o, const int64_t* given, uint32_t B) {
  __shared__ int64_t sSlot[PEDN_REPLAY_GROUP];   // the row's slot (-1: nothing to copy)
  __shared__ int32_t sBack[PEDN_REPLAY_GROUP], sE[PEDN_REPLAY_GROUP];   // min(serial - first, stack); env
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int64_t d = r.state[4];
  const size_t N = (size_t)r.N;
  const int S = r.stack;
  const uint32_t k0 = blockIdx.x * PEDN_REPLAY_GROUP;
  if (threadIdx.x < PEDN_REPLAY_GROUP) {
    const int64_t head = r.state[0], size = r.state[2], nslot = r.state[8], njslot = r.state[9];
    const uint32_t k = k0 + threadIdx.x;
    int64_t sv = -1, q = -1, e = 0, slot = -1;
    if (k < B) {
      bool ok = size > 0;
      if (ok) {
        if (given) {
          sv = given[2 * (size_t)k];
          e = given[2 * (size_t)k + 1];
          // inside the ring, a STEP row, and not older than the oldest sampleable row
          ok = e >= 0 && e < (int64_t)N && sv >= 0 && sv < head && sv >= head - r.R;
          if (ok) {
            slot = nslot - (head - sv) + (nslot < head - sv ? r.R : 0);
            q = r.first[slot];
            ok = q >= 0 && sv >= r.step_serial[njslot - size + (njslot < size ? r.cap : 0)];
          }
        } else {
          uint32_t w[4] = {k, (uint32_t)d, 0x71u, (uint32_t)((uint64_t)d >> 32)};
          philox4x32_10(w, r.k0, r.k1);
          const int64_t ago = 1 + (int64_t)(((uint64_t)w[0] * (uint64_t)size) >> 32);   // STEP count jhead - ago
          e = (int64_t)(((uint64_t)w[1] * (uint64_t)N) >> 32);
          sv = r.step_serial[njslot - ago + (njslot < ago ? r.cap : 0)];
          slot = nslot - (head - sv) + (nslot < head - sv ? r.R : 0);
          q = r.first[slot];
        }
      }
      if (!ok) {
        slot = -1;
        __hip_atomic_store(r.state + 5, (int64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else if (o.idx && o.idx != given) {
        o.idx[2 * (size_t)k] = sv;
        o.idx[2 * (size_t)k + 1] = e;
      }
    }
    const int64_t back = sv - q;
    sSlot[threadIdx.x] = slot; sBack[threadIdx.x] = (int32_t)(back < S ? back : S); sE[threadIdx.x] = (int32_t)e;
  }
  __syncthreads();
  for (int u = wave; u < PEDN_REPLAY_GROUP; u += 4) {
    const int64_t slot = sSlot[u];
    if (slot < 0) continue;   // (uniform over the wave)
    const int back = sBack[u];
    const size_t k = (size_t)k0 + u, e = (size_t)sE[u];
    float* st = o.states + k * S * o.obs_w;
    float* nx = o.next_states + k * S * o.obs_w;
    // frame f = 0 .. stack: serial max(sv - stack + f, first), min(stack - f, sv - first) slots behind the row's own; it is state row f
    // (f < stack) and next-state row f - 1 (f >= 1).  A lane takes 4 floats of one frame: every frame's loads are in flight together,
    // each slice is loaded once; one 16-byte access where the source and the destinations allow, 4-byte accesses otherwise.
    const int groups = (o.obs_w + 3) / 4, items = (S + 1) * groups;
    for (int x = lane; x < items; x += 64) {
      const int f = x / groups, c = (x - f * groups) * 4;
      const int m = S - f < back ? S - f : back;
      const int64_t fs = slot - m + (slot < m ? r.R : 0);
      const uint32_t* src = reinterpret_cast<const uint32_t*>(r.frames + ((size_t)fs * N + e) * r.n_obs + o.obs0) + c;
      uint32_t* d0 = reinterpret_cast<uint32_t*>(st + (size_t)(f < S ? f : 0) * o.obs_w) + c;        // (stored only when f < S)
      uint32_t* d1 = reinterpret_cast<uint32_t*>(nx + (size_t)(f >= 1 ? f - 1 : 0) * o.obs_w) + c;   // (stored only when f >= 1)
      const int n = o.obs_w - c < 4 ? o.obs_w - c : 4;
      uint4 v = {0u, 0u, 0u, 0u};
      if (n == 4 && (((uintptr_t)src | (uintptr_t)d0 | (uintptr_t)d1) & 15) == 0) {
        v = *reinterpret_cast<const uint4*>(src);
        if (f < S) *reinterpret_cast<uint4*>(d0) = v;
        if (f >= 1) *reinterpret_cast<uint4*>(d1) = v;
      } else {
        v.x = src[0];
        if (n > 1) v.y = src[1];
        if (n > 2) v.z = src[2];
        if (n > 3) v.w = src[3];
        if (f < S) { d0[0] = v.x; if (n > 1) d0[1] = v.y; if (n > 2) d0[2] = v.z; if (n > 3) d0[3] = v.w; }
        if (f >= 1) { d1[0] = v.x; if (n > 1) d1[1] = v.y; if (n > 2) d1[2] = v.z; if (n > 3) d1[3] = v.w; }
      }
    }
    const double* as = r.actions + ((size_t)slot * N + e) * r.n_actions + o.act0;
    for (int c = lane; c < o.act_w; c += 64) o.actions[k * o.act_w + c] = as[c];
    const float* rs = r.rewards + ((size_t)slot * N + e) * r.A + o.rew0;
    for (int c = lane; c < o.rew_w; c += 64)
      reinterpret_cast<uint32_t*>(o.rewards)[k * o.rew_w + c] = reinterpret_cast<const uint32_t*>(rs)[c];
    if (lane == 0) o.dones[k] = r.done[slot];
  }
  if (given) return;
  __syncthreads();   // (the workgroup has read the draw counter)
  if (threadIdx.x == 0) {
    unsigned* ticket = reinterpret_cast<unsigned*>(r.state + 7);
    const unsigned mine = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (mine + 1u == gridDim.x) {
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(r.state + 4, d + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- host side: pedn_replay_* of include/pedn.h.  State: pedn_sim::rp (store_drop, store_sources: pedn_host.hpp)
int pedn_replay_free(pedn_sim* s) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);   // (ends a clocked section: a captured push launch is not replayed over freed rows, pedn_rl_clock_signature)
  HIP_TRY(s, hipDeviceSynchronize());
  store_drop(s->rp);
  return PEDN_OK;
}

int pedn_replay_configure(pedn_sim* s, int64_t capacity, int32_t stack_size, int32_t episode_steps, uint64_t seed) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->rl_ready) return fail(s, PEDN_E_ARG, "pedn_rl_configure has not been called");
  if (capacity < 1) return fail(s, PEDN_E_ARG, "capacity < 1");
  if (stack_size < 1) return fail(s, PEDN_E_ARG, "stack_size < 1");
  if (episode_steps < 1) return fail(s, PEDN_E_ARG, "episode_steps < 1");
  if (capacity > (int64_t)1 << 40) return fail(s, PEDN_E_ARG, "capacity too large");
  if ((int64_t)s->v.R * stack_size * s->rl.O > 0x7fffffff) return fail(s, PEDN_E_ARG, "more than 2^31 entries in the stacked observation");
  int rc = pedn_replay_free(s);
  if (rc != PEDN_OK) return rc;
  const RlView& q = s->rl;
  ReplayView r;
  memset(&r, 0, sizeof r);   // (padding too: the view is hashed as bytes, pedn_rl_clock_signature)
  r.cap = capacity;
  r.R = capacity + stack_size + (capacity + episode_steps - 1) / episode_steps + 1;
  const size_t N = (size_t)s->v.R, R = (size_t)r.R;
  DevicePool& mem = s->rp.mem;
  if ((rc = mem.take(s, R * N * q.O * sizeof(float), (void**)&r.frames)) != PEDN_OK || (rc = mem.take(s, R * N * q.A * sizeof(double), (void**)&r.actions)) != PEDN_OK ||
      (rc = mem.take(s, R * N * q.n_agents * sizeof(float), (void**)&r.rewards)) != PEDN_OK || (rc = mem.take(s, R * sizeof(float), (void**)&r.done)) != PEDN_OK ||
      (rc = mem.take(s, N * stack_size * q.O * sizeof(float), (void**)&r.stacked)) != PEDN_OK || (rc = mem.take(s, R * sizeof(int64_t), (void**)&r.first)) != PEDN_OK ||
      (rc = mem.take(s, (size_t)capacity * sizeof(int64_t), (void**)&r.step_serial)) != PEDN_OK || (rc = mem.take(s, 16 * sizeof(int64_t), (void**)&r.state)) != PEDN_OK) {
    const std::string keep = s->err;
    store_drop(s->rp);
    return fail(s, rc, keep);
  }
  const int64_t no_episode = -1;
  HIP_TRY(s, hipMemcpy(r.state + 3, &no_episode, sizeof no_episode, hipMemcpyHostToDevice));
  r.clock = s->d_clock;
  r.k0 = (uint32_t)(seed & 0xffffffffu); r.k1 = (uint32_t)(seed >> 32);
  r.N = s->v.R; r.A = q.n_agents; r.n_actions = q.A; r.n_obs = q.O; r.stack = stack_size; r.T = s->v.T1 - 1;
  s->rp.view = r;
  s->rp.on = true;
  store_sources(s);
  return PEDN_OK;
}

// both roles of replay_push_kernel get the same number of workgroups: a lane takes about four 16-byte accesses of the wider role (few
// workgroups: every one of them takes a ticket from one counter)
static dim3 replay_push_grid(const ReplayView& r) {
  const size_t row = (size_t)r.N * std::max(std::max(r.n_obs, 2 * r.n_actions), r.A) / 4 + 1;
  const size_t stack = (size_t)r.N * r.stack * r.n_obs / ((r.n_obs & 3) ? 1 : 4);
  return dim3((unsigned)std::min<size_t>((std::max(row, stack) + 1023) / 1024, 512), 2);
}

int pedn_replay_begin(pedn_sim* s) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->rp.on) return fail(s, PEDN_E_ARG, "pedn_replay_configure has not been called");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);   // (ends a clocked section: the RESET row takes the observation the eager reset left)
  hipLaunchKernelGGL(replay_push_kernel, replay_push_grid(s->rp.view), dim3(256), 0, s->stream, s->rp.view, (const double*)nullptr, 1, 0);
  HIP_TRY(s, hipGetLastError());
  s->rp.begun = true;
  return PEDN_OK;
}

// (no allocation, no synchronisation, no event query: safe under stream capture)
int pedn_replay_push(pedn_sim* s, const double* actions, int32_t term, void* stream) {
  if (!s || !actions) return fail(s, PEDN_E_ARG, "null argument");
  if (!s->rp.on || !s->rp.begun) return fail(s, PEDN_E_ARG, "pedn_replay_begin has not been called");
  HIP_TRY(s, hipSetDevice(s->device));
  hipStream_t st = stream ? (hipStream_t)stream : s->stream;
  hipLaunchKernelGGL(replay_push_kernel, replay_push_grid(s->rp.view), dim3(256), 0, st, s->rp.view, actions, 0, s->clocked ? -1 : (term ? 1 : 0));
  HIP_TRY(s, hipGetLastError());
  return PEDN_OK;
}

// (the same: safe under stream capture)
int pedn_replay_sample(pedn_sim* s, int64_t batch, const int64_t* indices, int32_t obs0, int32_t obs_w, int32_t act0, int32_t act_w,
                       int32_t rew0, int32_t rew_w, float* states, double* actions, float* rewards, float* next_states, float* dones,
                       int64_t* idx, void* stream) {
  if (!s || !states || !actions || !rewards || !next_states || !dones) return fail(s, PEDN_E_ARG, "null argument");
  if (!s->rp.on) return fail(s, PEDN_E_ARG, "pedn_replay_configure has not been called");
  const ReplayView& r = s->rp.view;
  if (batch < 1 || batch > 0x7fffffffll) return fail(s, PEDN_E_ARG, "batch size out of range");
  if (obs0 < 0 || obs_w < 1 || obs0 + obs_w > r.n_obs || act0 < 0 || act_w < 1 || act0 + act_w > r.n_actions || rew0 < 0 || rew_w < 1 ||
      rew0 + rew_w > r.A)
    return fail(s, PEDN_E_ARG, "column range outside the row");
  HIP_TRY(s, hipSetDevice(s->device));
  ReplayOut o;
  memset(&o, 0, sizeof o);
  o.states = states; o.next_states = next_states; o.rewards = rewards; o.dones = dones; o.actions = actions; o.idx = idx;
  o.obs0 = obs0; o.obs_w = obs_w; o.act0 = act0; o.act_w = act_w; o.rew0 = rew0; o.rew_w = rew_w;
  const int64_t groups = (batch + PEDN_REPLAY_GROUP - 1) / PEDN_REPLAY_GROUP;
  hipStream_t st = stream ? (hipStream_t)stream : s->stream;
  hipLaunchKernelGGL(replay_sample_kernel, dim3((unsigned)groups), dim3(256), 0, st, r, o, indices, (uint32_t)batch);
  HIP_TRY(s, hipGetLastError());
  return PEDN_OK;
}

int pedn_replay_size(pedn_sim* s, int64_t* state) {
  if (!s || !state) return fail(s, PEDN_E_ARG, "null argument");
  if (!s->rp.on) return fail(s, PEDN_E_ARG, "pedn_replay_configure has not been called");
  HIP_TRY(s, hipSetDevice(s->device));
  HIP_TRY(s, hipDeviceSynchronize());   // pushes and samples may sit on a caller's stream
  HIP_TRY(s, hipMemcpy(state, s->rp.view.state, 6 * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (state[5]) HIP_TRY(s, hipMemset(s->rp.view.state + 5, 0, sizeof(int64_t)));   // reported once
  return PEDN_OK;
}

void* pedn_replay_device_ptr(pedn_sim* s, int32_t which) {
  if (!s || !s->rp.on) return nullptr;
  const ReplayView& r = s->rp.view;
  switch (which) {
    case 0: return r.frames;
    case 1: return r.actions;
    case 2: return r.rewards;
    case 3: return r.done;
    case 4: return r.first;
    case 5: return r.step_serial;
    case 6: return r.stacked;
    case 7: return r.state;
  }
  return nullptr;
}
