// What the kernels of the reference's stacked 64-wide networks share (DESIGN sections 14-16: actor_forward_kernel, sac_target_kernel,
// ppo_eval_kernel): the layer's accumulation order, the LayerNorm, the double-precision pieces of the tails and the draw counter.  The
// sections require the kernels to agree operation for operation; they do because each operation is written once, here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pedn_math.hpp"

#define PEDN_ACTOR_HIDDEN 64      // hidden_size of every layer (the reference's default; nothing else is built)
#define PEDN_ACTOR_TILE 32        // rows (envs) per workgroup of mlp_layer
#define PEDN_ACTOR_WAVE_ENVS 8    // rows per wave
#define PEDN_ACTOR_CHUNK 32       // inputs per staged chunk
#define PEDN_ACTOR_MAX_ACT 8      // act_w of an agent
#define PEDN_ACTOR_TABLE_COLS 6   // obs0, obs_w, act0, act_w, parameter offset (floats), reserved

// acc[r] = acc[r] + w[k] * x[r][k], k = 0 .. kmax - 1 ascending, one accumulator per (row, neuron): the order depends on nothing but the
// layer's shape.  wr: this lane's weights of the chunk; xr: the wave's R input rows of stride xs words (16-byte aligned), every lane
// reads one address: a broadcast.
template <int R>
__device__ __forceinline__ void mlp_mac(float (&acc)[R], const float* wr, const float* xr, int xs, int kmax) {
  int kk = 0;
  for (; kk + 4 <= kmax; kk += 4) {
    const float wa = wr[kk], wb = wr[kk + 1], wc = wr[kk + 2], wd = wr[kk + 3];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float4 x = *reinterpret_cast<const float4*>(xr + r * xs + kk);
      acc[r] = acc[r] + wa * x.x;
      acc[r] = acc[r] + wb * x.y;
      acc[r] = acc[r] + wc * x.z;
      acc[r] = acc[r] + wd * x.w;
    }
  }
  for (; kk < kmax; ++kk) {
    const float w = wr[kk];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = acc[r] + w * xr[r * xs + kk];
  }
}

// One layer of a workgroup of 4 waves for its tile of 32 rows, 8 per wave, a lane per neuron: acc[r] = b[o]; then mlp_mac over chunks
// of 32 inputs.  Rows [0, n0) of the layer come from w0 / b0, rows [n0, rows) from w1 / b1 (nn.Linear's [out][in]).  The workgroup
// copies the chunk of the weight rows (read with 128-byte row pieces) into LDS rows of 33 words, which lane o then reads conflict-free
// (33 is odd).  first: gather(c0, kmax) fills sXc (rows of PEDN_ACTOR_CHUNK) with inputs [c0, c0 + kmax) of the tile's rows, zeros
// behind them; otherwise x is sH (rows of 64, which only the row's own wave touches).
template <class Gather>
__device__ __forceinline__ void mlp_layer(float (&acc)[PEDN_ACTOR_WAVE_ENVS], const float* w0, const float* b0, const float* w1,
                                          const float* b1, int n0, int rows, int K, bool first, float* sW, const float* sXc, const float* sH,
                                          Gather gather) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const float bias = lane < rows ? (lane < n0 ? b0[lane] : b1[lane - n0]) : 0.0f;
#pragma unroll
  for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) acc[r] = bias;
  for (int c0 = 0; c0 < K; c0 += PEDN_ACTOR_CHUNK) {
    const int kmax = K - c0 < PEDN_ACTOR_CHUNK ? K - c0 : PEDN_ACTOR_CHUNK;
    __syncthreads();   // the chunk before has been consumed (and what the caller wrote to LDS for this layer is there)
    for (int idx = (int)threadIdx.x; idx < rows * PEDN_ACTOR_CHUNK; idx += 256) {
      const int o = idx / PEDN_ACTOR_CHUNK, kk = idx % PEDN_ACTOR_CHUNK;
      if (kk < kmax) sW[o * (PEDN_ACTOR_CHUNK + 1) + kk] = (o < n0 ? w0 + (size_t)o * K : w1 + (size_t)(o - n0) * K)[c0 + kk];
    }
    if (first) gather(c0, kmax);
    __syncthreads();
    if (lane < rows)
      mlp_mac(acc, sW + lane * (PEDN_ACTOR_CHUNK + 1),
              first ? sXc + wave * PEDN_ACTOR_WAVE_ENVS * PEDN_ACTOR_CHUNK : sH + wave * PEDN_ACTOR_WAVE_ENVS * PEDN_ACTOR_HIDDEN + c0,
              first ? PEDN_ACTOR_CHUNK : PEDN_ACTOR_HIDDEN, kmax);
  }
}

// sum of the wave's 64 values as a balanced tree: level m adds the partner 2^m lanes away.  Both partners add the same two numbers, so
// every lane holds the same bits at every level.
__device__ __forceinline__ float mlp_tree_sum(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}

// LayerNorm(64) over the wave's lanes, float32; g, b: this lane's weight and bias
template <int R>
__device__ __forceinline__ void mlp_layer_norm(float (&acc)[R], float g, float b) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float mean = mlp_tree_sum(acc[r]) / 64.0f;
    const float c = acc[r] - mean;
    const float var = mlp_tree_sum(c * c) / 64.0f;
    acc[r] = c / sqrtf(var + 1e-5f) * g + b;
  }
}

// ReLU into hrow + r * 64: this lane's neuron of the wave's row r
template <int R>
__device__ __forceinline__ void mlp_relu_store(float* hrow, const float (&acc)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) hrow[r * PEDN_ACTOR_HIDDEN] = acc[r] < 0.0f ? 0.0f : acc[r];
}

// encoder.fc1, encoder.fc2 and fc of the network whose pack starts at p (each nn.Linear's weight, then its bias), with a ReLU behind
// each; ln: LayerNorm(64) between fc and its ReLU, weight and bias behind fc's.  Leaves the rows in sH and returns what follows in the pack.
template <class Gather>
__device__ __forceinline__ const float* mlp_trunk(float (&acc)[PEDN_ACTOR_WAVE_ENVS], const float* p, int K1, bool ln, float* sW,
                                                  const float* sXc, float* sH, Gather gather) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int H = PEDN_ACTOR_HIDDEN;
  const float* w1 = p;
  const float* b1 = w1 + (size_t)H * K1;
  const float* w2 = b1 + H;
  const float* b2 = w2 + H * H;
  const float* w3 = b2 + H;
  const float* b3 = w3 + H * H;
  const float* rest = b3 + H;
  float* hrow = sH + wave * PEDN_ACTOR_WAVE_ENVS * H + lane;
  mlp_layer(acc, w1, b1, w1, b1, H, H, K1, true, sW, sXc, sH, gather);
  mlp_relu_store(hrow, acc);
  mlp_layer(acc, w2, b2, w2, b2, H, H, H, false, sW, sXc, sH, gather);
  mlp_relu_store(hrow, acc);
  mlp_layer(acc, w3, b3, w3, b3, H, H, H, false, sW, sXc, sH, gather);
  if (ln) mlp_layer_norm(acc, rest[lane], rest[H + lane]);
  mlp_relu_store(hrow, acc);
  return ln ? rest + 2 * H : rest;
}

// fc_mu and fc_std (at p, one behind the other) as one layer of 2 * act_w rows on the trunk's sH, handed over through sOut to a lane
// per (row, action).  Returns the wave's rows so: so[r * 16 + j] is mu, so[r * 16 + 8 + j] the pre-softplus value of its row r.
// gather is the trunk's and is not called: one instantiation of mlp_layer per kernel (with a second one the compiler unrolls the
// layers differently: 20 % more instructions).
template <class Gather>
__device__ __forceinline__ const float* mlp_heads(float (&acc)[PEDN_ACTOR_WAVE_ENVS], const float* p, int act_w, float* sW, const float* sXc,
                                                  const float* sH, float* sOut, Gather gather) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int H = PEDN_ACTOR_HIDDEN;
  const float* wmu = p;
  const float* bmu = wmu + act_w * H;
  const float* wsd = bmu + act_w;
  const float* bsd = wsd + act_w * H;
  mlp_layer(acc, wmu, bmu, wsd, bsd, act_w, 2 * act_w, H, false, sW, sXc, sH, gather);
  float* so = sOut + wave * PEDN_ACTOR_WAVE_ENVS * 2 * PEDN_ACTOR_MAX_ACT;
  if (lane < 2 * act_w) {
    const int col = lane < act_w ? lane : PEDN_ACTOR_MAX_ACT + lane - act_w;
#pragma unroll
    for (int r = 0; r < PEDN_ACTOR_WAVE_ENVS; ++r) so[r * 2 * PEDN_ACTOR_MAX_ACT + col] = acc[r];
  }
  __syncthreads();
  return so;
}

// torch's softplus (threshold 20), in double from the float32 value, rounded once
__device__ __forceinline__ float mlp_softplus(float z) { return z > 20.0f ? z : (float)log1p(exp((double)z)); }

// torch's Normal(mu, sd).log_prob(a), in double from the float32 values
__device__ __forceinline__ double normal_log_prob(float a, float mu, float sd) {
  const double A = (double)a, M = (double)mu, Sd = (double)sd;
  return -((A - M) * (A - M)) / (2.0 * (Sd * Sd)) - log(Sd) - 0.91893853320467267;
}

// A standard normal by Box-Muller from the Philox block of counter (w0, d, site_col) under key (k0, k1): d is the draw counter,
// site_col the stream's site byte | the action column << 8.
__device__ __forceinline__ float philox_normal(uint32_t k0, uint32_t k1, uint32_t w0, int64_t d, uint32_t site_col) {
  uint32_t w[4] = {w0, (uint32_t)d, site_col, (uint32_t)((uint64_t)d >> 32)};
  philox4x32_10(w, k0, k1);
  const double u1 = ((double)w[0] + 1.0) * 0x1p-32, u2 = (double)w[1] * 0x1p-32;
  return (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
}

// One thread per workgroup, behind the workgroup's read of the draw counter d = state[0]: the last workgroup of the grid to take a
// ticket (state[1], its low 32 bits) resets the tickets and advances the counter (vector atomics).
__device__ __forceinline__ void advance_draw_counter(int64_t* state, int64_t d) {
  unsigned* ticket = reinterpret_cast<unsigned*>(state + 1);
  const unsigned mine = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (mine + 1u == gridDim.x * gridDim.y) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(state, d + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
