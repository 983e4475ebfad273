// torch.optim.Adam's step as the device-side updates take it (the step, its state and what the entry points refuse;
// section 19: the fused exp_avg_sq), written once for critic_adam_kernel, sacactor_adam_kernel and ppograd_adam_kernel.  The step state
// is four int64 words: 0 the step count, 1 the ticket (its low 32 bits), 2 and 3 the doubles beta1^t and beta2^t.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pedn_mlp.hpp"

struct AdamCoef {
  float b2, omb1, omb2, eps;   // (float)beta2, (float)(1 - beta1), (float)(1 - beta2), (float)eps
};

// One element's step: m = m + (1 - beta1) * (g - m), v = v * beta2 + (1 - beta2) * g * g, p = p + (nstep * m) / (sqrt(v) / s + eps).
// FUSED: exp_avg_sq's last product is fused into its sum, v = fma((1 - beta2) * g, g, v * beta2), one rounding fewer.  torch's own step fuses
// it too, and with every product rounded one element of a recorded actor update lay 1.26 ulp from the float64 step where the reference
// lay 0.26.  An explicit fmaf: the library is built with -ffp-contract=off.  The critic's step is section 18's, every
// product rounded; the two are different contracts and stay apart.
template <bool FUSED>
__device__ __forceinline__ float adam_one(float g, float& m, float& v, float p, const AdamCoef& c, float nstep, float s) {
  m = m + c.omb1 * (g - m);
  v = FUSED ? fmaf(c.omb2 * g, g, v * c.b2) : v * c.b2 + (c.omb2 * g) * g;
  const float den = sqrtf(v) / s + c.eps;
  return p + (nstep * m) / den;
}

// What a step reads of its state: the count and the products behind this step, in double, and s = (float)sqrt(1 - beta2^t)
struct AdamStep {
  int64_t steps;
  double b1t, b2t;
  float s;
};

__device__ __forceinline__ AdamStep adam_step_begin(const int64_t* state, double beta1, double beta2) {
  const double* pw = reinterpret_cast<const double*>(state + 2);
  AdamStep st;
  st.steps = state[0];
  st.b1t = pw[0] * beta1;
  st.b2t = pw[1] * beta2;
  st.s = (float)sqrt(1.0 - st.b2t);
  return st;
}

// -lr / (1 - beta1^t) of a learning rate, rounded once
__device__ __forceinline__ float adam_nstep(double lr, const AdamStep& st) { return -(float)(lr / (1.0 - st.b1t)); }

// One thread per workgroup, behind the workgroup's reads of the state: the last of `tickets` callers resets the tickets and advances the
// state (nobody reads it any more), and is told so.
__device__ __forceinline__ bool adam_step_advance(int64_t* state, const AdamStep& st, unsigned tickets) {
  unsigned* ticket = reinterpret_cast<unsigned*>(state + 1);
  const unsigned mine = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (mine + 1u != tickets) return false;
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(state, st.steps + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(state + 2, (int64_t)__double_as_longlong(st.b1t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(state + 3, (int64_t)__double_as_longlong(st.b2t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// ---- host side
static AdamCoef adam_coef(double beta1, double beta2, double eps) {
  return AdamCoef{(float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps};
}

// What every update entry point refuses behind its null pointers, in the order all three keep: the networks' width, the counts (dims_ok: the
// entry point's own positive ones; the agents are a grid dimension), what only this entry point refuses (own_msg, or null), its packs' lengths
// (packs_ok), the alignment of what is read 16 bytes at a time (ptrs: those addresses ORed) and Adam's hyper-parameters (lr_b: a second
// learning rate, or lr_a again).  Returns the message, or null when there is nothing to refuse.
static const char* update_refusal(int32_t hidden_size, const char* hidden_msg, bool dims_ok, int32_t n_agents, const char* dims_msg,
                                  const char* own_msg, bool packs_ok, const char* pack_msg, uintptr_t ptrs, double lr_a, double lr_b,
                                  double beta1, double beta2, double eps) {
  if (hidden_size != PEDN_ACTOR_HIDDEN) return hidden_msg;
  if (!dims_ok || n_agents < 1 || n_agents > 65535) return dims_msg;
  if (own_msg) return own_msg;
  if (!packs_ok) return pack_msg;
  if (ptrs & 15) return "the packs and the workspace must be 16-byte aligned";
  if (!(lr_a >= 0.0 && lr_a < INFINITY && lr_b >= 0.0 && lr_b < INFINITY)) return "lr must be finite and not negative";
  if (!(eps >= 0.0 && eps < INFINITY)) return "eps must be finite and not negative";
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return "the betas must be in [0, 1)";
  return nullptr;
}
