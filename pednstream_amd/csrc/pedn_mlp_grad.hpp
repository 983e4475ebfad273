// The backward pieces of a 64-wide nn.Linear layer for a tile of rows, each written once for critic_grad_kernel, sacactor_grad_kernel and
// ppograd_kernel.  Like pedn_mlp.hpp's forward they fix the order of every sum by the layer's shape alone: every
// accumulator starts at +0.0, rows ascend in a weight gradient, output neurons ascend in an input gradient.  A group of `n` threads (a
// multiple of 64; thread t of it is lane t & 63 of its wave t >> 6) shares the staging; no piece reads threadIdx.  The innermost loops
// come first, then the tile's pieces with the workgroup barriers they need: every wave of the workgroup calls those, whatever group it
// is in.
#pragma once
#include <hip/hip_runtime.h>

#include "pedn_mlp.hpp"

#define PEDN_GRAD_PAD (PEDN_ACTOR_CHUNK + 1)   // words of a staged row: odd, so that a lane per row reads conflict-free
#define PEDN_GRAD_TILE 32        // rows of a tile: what a workgroup holds in LDS at a time
#define PEDN_GRAD_WAVE_ROWS 8    // rows per wave of a group of 4 waves
#define PEDN_GRAD_DS 68          // words of a row of the output gradients (and of h3): 16-byte aligned rows, 8 rows on 8 banks
#define PEDN_GRAD_FEAT 96        // words of a critic's fc input row: 64 + act_w + 1 <= 73, rounded up to whole chunks

// Stage rows [o0, o0 + 32) of the weights w ([out][K], nn.Linear's layout), columns [0, 64), TRANSPOSED: sT[k * 33 + oo] = w[o0 + oo][k].
// The global reads are 256-byte row pieces; lane k then reads its 32 weights conflict-free.
__device__ __forceinline__ void mlp_grad_stage_wt(float* sT, const float* w, int K, int o0, int t, int n) {
  for (int idx = t; idx < PEDN_ACTOR_CHUNK * PEDN_ACTOR_HIDDEN; idx += n) {
    const int oo = idx >> 6, k = idx & 63;
    sT[k * PEDN_GRAD_PAD + oo] = w[(unsigned)((o0 + oo) * K + k)];
  }
}

// dX[r][k] = dX[r][k] + d[r][o] * w[o][k] for the n <= 32 staged o, ascending, lane k: wt = sT + k * 33 (mlp_grad_stage_wt), d = the
// wave's R rows of the output gradient from column o0 on (stride ds words, 16-byte aligned: a broadcast).  It IS the forward's
// accumulation with the roles of the operands exchanged, so it is the forward's code.  n is a run-time value on purpose: with a constant
// the compiler unrolls the chunk whole and hoists its 288 LDS loads into registers (89 spills in critic_grad_kernel).
template <int R>
__device__ __forceinline__ void mlp_grad_dx(float (&acc)[R], const float* wt, const float* d, int ds, int n) {
  mlp_mac(acc, wt, d, ds, n);
}

// dW[o][k0 + j] = dW[o][k0 + j] + d[r][o] * x[r][k0 + j], r = 0 .. nrows - 1 ascending, lane o, J a multiple of 4: dcol = d + o (stride ds),
// x = the tile's input rows from column k0 on (stride xs words, 16-byte aligned: a broadcast).
template <int J>
__device__ __forceinline__ void mlp_grad_dw(float (&g)[J], const float* dcol, int ds, const float* x, int xs, int nrows) {
  for (int r = 0; r < nrows; ++r) {
    const float dv = dcol[r * ds];
#pragma unroll
    for (int j = 0; j < J; j += 4) {
      const float4 xv = *reinterpret_cast<const float4*>(x + r * xs + j);
      g[j] = g[j] + dv * xv.x;
      g[j + 1] = g[j + 1] + dv * xv.y;
      g[j + 2] = g[j + 2] + dv * xv.z;
      g[j + 3] = g[j + 3] + dv * xv.w;
    }
  }
}

// *p = v, or with ACC and not fresh *p = *p + v: a partial joins the workgroup's slab.  The caller sees to it that an
// address has ONE thread that reads and writes it, the same in every tile.
template <bool ACC>
__device__ __forceinline__ void mlp_grad_put(float* p, float v, bool fresh) {
  *p = (!ACC || fresh) ? v : *p + v;
}

// Put columns [c0, c0 + kmax) of a weight gradient of 64 rows, staged in sG as rows of 33 words, to gw ([64][K]) as 128-byte row
// pieces: the mirror of the forward's weight staging.
template <bool ACC>
__device__ __forceinline__ void mlp_grad_store(const float* sG, float* gw, int K, int c0, int kmax, bool fresh, int t, int n) {
  for (int idx = t; idx < PEDN_ACTOR_HIDDEN * PEDN_ACTOR_CHUNK; idx += n) {
    const int o = idx / PEDN_ACTOR_CHUNK, kk = idx % PEDN_ACTOR_CHUNK;
    if (kk < kmax) mlp_grad_put<ACC>(gw + (unsigned)(o * K + c0 + kk), sG[o * PEDN_GRAD_PAD + kk], fresh);
  }
}

// LayerNorm(64) over the wave's lanes as pedn_mlp.hpp's mlp_layer_norm computes it, operation for operation, with what its backward needs
// kept: xh[r] = (x - mean) / sd[r], sd[r] = sqrt(var + 1e-5); acc[r] = xh[r] * g + b.
template <int R>
__device__ __forceinline__ void mlp_layer_norm_keep(float (&acc)[R], float (&xh)[R], float (&sd)[R], float g, float b) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float mean = mlp_tree_sum(acc[r]) / 64.0f;
    const float c = acc[r] - mean;
    const float var = mlp_tree_sum(c * c) / 64.0f;
    sd[r] = sqrtf(var + 1e-5f);
    xh[r] = c / sd[r];
    acc[r] = xh[r] * g + b;
  }
}

// LayerNorm's backward, a lane per neuron, the 64 lanes summed with the forward's balanced tree: from d[r] = dL / dy of this lane's
// neuron, dxh = d * g, m1 = tree(dxh) / 64, m2 = tree(dxh * xh) / 64, dL / dx = ((dxh - m1) - xh * m2) / sd, every product, difference
// and quotient one rounded float32 operation in that order.  (The weight's and the bias' gradients are sums over rows: dW[k] += d[r][k] *
// xh[r][k], db[k] += d[r][k], rows ascending, which the caller forms like any bias gradient.)
template <int R>
__device__ __forceinline__ void mlp_layer_norm_grad(float (&d)[R], const float (&xh)[R], const float (&sd)[R], float g) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float dxh = d[r] * g;
    const float m1 = mlp_tree_sum(dxh) / 64.0f;
    const float m2 = mlp_tree_sum(dxh * xh[r]) / 64.0f;
    d[r] = ((dxh - m1) - xh[r] * m2) / sd[r];
  }
}

// ---- the tile's pieces

// One forward layer of a group of 4 waves (thread t of 256) for the tile, pedn_mlp.hpp's mlp_layer with a group's own staging rows sW: acc[r]
// = b[o]; then mlp_mac over chunks of 32 inputs, lane o < rows.  Rows [0, n0) of the layer come from w0 / b0, the others from w1 / b1.  A
// group that is not active takes the barriers only.  first: gather(c0, kmax) fills sXc (32 rows of 32, zeros behind kmax and in rows past
// the last) for every group; otherwise x is this wave's rows xin of stride xs.
template <int R, class Gather>
__device__ __forceinline__ void mlp_group_layer(float (&acc)[R], bool active, const float* w0, const float* b0, const float* w1, const float* b1,
                                                int n0, int rows, int K, bool first, float* sW, const float* sXc, const float* xin, int xs, int t,
                                                Gather gather) {
  const int lane = t & 63, w4 = t >> 6;
  const float bias = active && lane < rows ? (lane < n0 ? b0[lane] : b1[lane - n0]) : 0.0f;
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = bias;
  for (int c0 = 0; c0 < K; c0 += PEDN_ACTOR_CHUNK) {
    const int kmax = K - c0 < PEDN_ACTOR_CHUNK ? K - c0 : PEDN_ACTOR_CHUNK;
    __syncthreads();   // the chunk before has been consumed (and what the caller wrote to LDS for this layer is there)
    if (active)
      for (int idx = t; idx < rows * PEDN_ACTOR_CHUNK; idx += 256) {
        const int o = idx / PEDN_ACTOR_CHUNK, kk = idx % PEDN_ACTOR_CHUNK;
        if (kk < kmax) sW[o * PEDN_GRAD_PAD + kk] = (o < n0 ? w0 + (unsigned)(o * K) : w1 + (unsigned)((o - n0) * K))[c0 + kk];
      }
    if (first) gather(c0, kmax);
    __syncthreads();
    if (active && lane < rows)
      mlp_mac(acc, sW + lane * PEDN_GRAD_PAD, first ? sXc + w4 * R * PEDN_ACTOR_CHUNK : xin + c0, first ? PEDN_ACTOR_CHUNK : xs, kmax);
  }
}

// The tile's input gradient: acc[r] = sum over o ascending of d[r][o] * w[o][k] from +0.0, lane k < 64 (of thread t), the wave's R rows
// drows of the output gradient (stride ds).  The n threads of the staging group (thread t of them) stage w ([64][K]) into sT; a wave that
// is not active takes the barriers only.
template <int R>
__device__ __forceinline__ void mlp_grad_dx_tile(float (&acc)[R], bool active, const float* drows, int ds, const float* w, int K, float* sT, int t,
                                                 int n) {
  const int lane = t & 63;
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0f;
  int cnt = PEDN_ACTOR_CHUNK;
  asm volatile("" : "+s"(cnt));   // (no instruction: the count stays a run-time value, see mlp_grad_dx)
  for (int o0 = 0; o0 < PEDN_ACTOR_HIDDEN; o0 += PEDN_ACTOR_CHUNK) {
    __syncthreads();   // the staging rows are free
    mlp_grad_stage_wt(sT, w, K, o0, t, n);
    __syncthreads();
    if (active) mlp_grad_dx(acc, sT + lane * PEDN_GRAD_PAD, drows + o0, ds, cnt);
  }
}

// The tile's gradients of one layer's weight [64][K] and bias from its output gradient d (rows of ds words) and its input x (rows of xs
// words that cover whole chunks; first: x is the gathered chunk, which gather(c0, kmax) fills), put to gw and gb (ACC and not fresh: added
// to them): wave t >> 6 of the group of n threads takes columns J * wave .. + J - 1 of every chunk if it is active (the first 32 / J waves
// are), wave bias_wave the bias.  Thread t puts the same addresses in every tile.  sG: staging rows.  (The wave is formed here from t and is
// no argument: handed in, as a vector or as a scalar value, it cost critic_grad_kernel 2 VGPRs more than its 132.)
template <int J, bool ACC, class Gather>
__device__ __forceinline__ void mlp_grad_dw_tile(const float* d, int ds, const float* x, int xs, int K, int nrows, float* gw, float* gb, float* sG,
                                                 bool first, bool fresh, bool active, int bias_wave, int t, int n, Gather gather) {
  const int lane = t & 63, wave = t >> 6;
  __syncthreads();   // d is there
  if (wave == bias_wave) {
    float b = 0.0f;
    for (int r = 0; r < nrows; ++r) b = b + d[r * ds + lane];
    mlp_grad_put<ACC>(gb + lane, b, fresh);
  }
  for (int c0 = 0; c0 < K; c0 += PEDN_ACTOR_CHUNK) {
    const int kmax = K - c0 < PEDN_ACTOR_CHUNK ? K - c0 : PEDN_ACTOR_CHUNK;
    if (first) {
      gather(c0, kmax);
      __syncthreads();
    }
    if (active) {
      float g[J];
#pragma unroll
      for (int j = 0; j < J; ++j) g[j] = 0.0f;
      mlp_grad_dw(g, d + lane, ds, (first ? x : x + c0) + J * wave, xs, nrows);
#pragma unroll
      for (int j = 0; j < J; ++j) sG[lane * PEDN_GRAD_PAD + J * wave + j] = g[j];
    }
    __syncthreads();
    mlp_grad_store<ACC>(sG, gw, K, c0, kmax, fresh, t, n);
    __syncthreads();   // sG and the gathered chunk are free
  }
}

// The tile's gradients of the two heads fc_mu and fc_std (at gh as in the pack: weight, bias, weight, bias) from their output gradient d
// (rows of ds words: mu's act_w columns, then the pre-softplus value's) and h3 (rows of 64): a thread per weight, rows ascending, then a
// thread per bias.  Thread t of n puts the same addresses in every tile.
template <bool ACC>
__device__ __forceinline__ void mlp_grad_heads_tile(const float* d, int ds, const float* h3, int act_w, int nrows, float* gh, bool fresh, int t,
                                                    int n) {
  const int H = PEDN_ACTOR_HIDDEN;
  for (int idx = t; idx < 2 * act_w * H; idx += n) {
    const int o = idx >> 6, k = idx & 63;
    float v = 0.0f;
    for (int r = 0; r < nrows; ++r) v = v + d[r * ds + o] * h3[r * H + k];
    mlp_grad_put<ACC>(gh + (o < act_w ? 0 : act_w) + idx, v, fresh);
  }
  if (t < 2 * act_w) {
    float v = 0.0f;
    for (int r = 0; r < nrows; ++r) v = v + d[r * ds + t];
    mlp_grad_put<ACC>(gh + (t < act_w ? act_w * H + t : 2 * act_w * H + t), v, fresh);
  }
}

// Inputs [c0, c0 + kmax) of a SAC minibatch's tile (rows row0 .. + nrows - 1 of s, [B][S][n_obs]) into sXc for every network of the
// workgroup, thread t of its n: input f * S + s of a row is s[row][s][obs0 + f]; zeros elsewhere.
__device__ __forceinline__ void sac_gather_chunk(float* sXc, const float* s, int S, int n_obs, int obs0, int row0, int nrows, int c0, int kmax,
                                                 int t, int n) {
  for (int idx = t; idx < PEDN_GRAD_TILE * PEDN_ACTOR_CHUNK; idx += n) {
    const int r = idx / PEDN_ACTOR_CHUNK, kk = idx % PEDN_ACTOR_CHUNK;
    float v = 0.0f;
    if (kk < kmax && r < nrows) {
      const unsigned k = (unsigned)(c0 + kk), f = k / (unsigned)S, st = k - f * (unsigned)S;
      v = s[((size_t)(row0 + r) * S + st) * n_obs + obs0 + f];
    }
    sXc[idx] = v;
  }
}
