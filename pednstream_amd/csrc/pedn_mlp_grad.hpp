// The backward pieces of a 64-wide nn.Linear layer for a tile of rows, each written once (critic_grad_kernel; the actor
// and PPO gradients will use the same ones).  Like pedn_mlp.hpp's forward they fix the order of every sum by the layer's shape alone:
// every accumulator starts at +0.0, rows ascend in a weight gradient, output neurons ascend in an input gradient.  A group of `n` threads
// (a multiple of 64, thread t of it) shares the staging; the caller places the workgroup barriers between the pieces.
#pragma once
#include <hip/hip_runtime.h>

#include "pedn_mlp.hpp"

#define PEDN_GRAD_PAD (PEDN_ACTOR_CHUNK + 1)   // words of a staged row: odd, so that a lane per row reads conflict-free

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

// Store columns [c0, c0 + kmax) of a weight gradient of 64 rows, staged in sG as rows of 33 words, to gw ([64][K]) as 128-byte row
// pieces: the mirror of the forward's weight staging.
__device__ __forceinline__ void mlp_grad_store(const float* sG, float* gw, int K, int c0, int kmax, int t, int n) {
  for (int idx = t; idx < PEDN_ACTOR_HIDDEN * PEDN_ACTOR_CHUNK; idx += n) {
    const int o = idx / PEDN_ACTOR_CHUNK, kk = idx % PEDN_ACTOR_CHUNK;
    if (kk < kmax) gw[(unsigned)(o * K + c0 + kk)] = sG[o * PEDN_GRAD_PAD + kk];
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
