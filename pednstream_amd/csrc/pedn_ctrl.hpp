// Rule-based controllers on the device (include/pedn.h: pedn_ctrl_*): the reference's RuleBasedGaterAgent and
// RuleBasedSeparatorAgent (rl/agents/rule_based.py) for every env, computed by wave 0 of the observation block of an agent from the
// float32 observation it has just written -- no extra launch, no host round trip between env steps.
//
//   gater      avg = np.mean(densities) (float32: a sequential sum below 8 links, NumPy's 8-way pairwise sum at 8);
//              avg <= 2: every link's physical width; otherwise per link current_width + 1 / - 1 (float32) when the density is above /
//              below the threshold (float32), the link's width when equal
//   separator  x = obs[1] (the forward link's outflow; obs[4] does not exist, the reverse term is 0.0):
//              no smoothing  x + 0 == 0 ? width / 2 : width * x / (x + 0)   in float32 (binary64 when the width is a numpy float64)
//              smoothing     m = float(np.mean(last `window` values of x))  (float32 mean), then the same in binary64
// Every action is rounded to float32 and widened into the engine-owned action rows [R][A] (NaN = no action: agents without a controller).
// The moving-average buffers are [slot][RS] float32 rows per agent plus a count per (agent, replica); each value has one writer (the lane
// of its replica), so the two half-batch chains and any launch plan keep them consistent without atomics.
#pragma once

#define PEDN_CTRL_MAX_WINDOW 32   // longest moving-average window of a separator controller (pedn_ctrl_configure refuses longer)

struct CtrlAgent {
  int32_t kind;     // 0 no controller, 1 gater rule, 2 separator rule
  int32_t window;   // separator: moving-average window (0: no smoothing)
  int32_t wide;     // separator without smoothing: the width is a binary64 numpy scalar (binary64 arithmetic instead of float32)
  int32_t ring;     // separator with smoothing: first row of its window in CtrlView::ring
  float thr;        // gater: threshold rounded to float32
  float w32;        // separator: road width rounded to float32
  double w64;       // separator: road width
};

struct CtrlView {
  const CtrlAgent* agent;   // [n_agents]
  const float* open;        // [A] gater slots: float32 physical width of the slot's link
  double* actions;          // [R][A] next actions
  float* ep;                // [R][n_agents] episode reward sums
  float* ring;              // [rows][RS] moving-average values
  int32_t* count;           // [n_agents][RS] values appended to each buffer so far
  int32_t ep_mode;          // 1: add this step's reward; 2: start from 0 (the reset observation)
  int32_t RS;               // replica stride of ring / count rows
};

template <bool CTRL>
__device__ __forceinline__ void ctrl_decide(const CtrlView& cv, const RlView& q, int ag, int type, int n, int r, const float* o,
                                            const float (*sD)[64], const float (*sG)[64], int lane, float reward_sum) {
  float* ep = cv.ep + (size_t)r * q.n_agents + ag;
  *ep = cv.ep_mode == 2 ? 0.0f : *ep + reward_sum;   // episode_true_rewards[a] += rewards[a] (rl_utils.py:1593-1599)
  const CtrlAgent C = cv.agent[ag];
  const int a0 = q.agent_act_off[ag];
  double* act = cv.actions + (size_t)r * q.A + a0;
  if (C.kind == 1 && type == 1) {
    const float avg = numpy_sum_f32(n, [&](int i) { return sD[i][lane]; }) / (float)n;
    if (avg <= 2.0f) {
      for (int i = 0; i < n; ++i) act[i] = (double)cv.open[a0 + i];
    } else {
      for (int i = 0; i < n; ++i) {
        const float d = sD[i][lane], cw = sG[i][lane];
        const float x = d > C.thr ? cw + 1.0f : (d < C.thr ? cw - 1.0f : cv.open[a0 + i]);
        act[i] = (double)x;
      }
    }
  } else if (C.kind == 2 && type == 0) {
    const float x = o[1];
    float a;
    if (C.window > 0) {   // _update_and_smooth_inflow: append, drop the oldest beyond the window, float(np.mean(buffer))
      const size_t RS = (size_t)cv.RS;
      int32_t* cnt = cv.count + (size_t)ag * RS + r;
      const int c = *cnt, w = C.window;
      const float* ring = cv.ring + (size_t)C.ring * RS + r;
      cv.ring[((size_t)C.ring + (size_t)(c % w)) * RS + r] = x;
      *cnt = c + 1;
      const int m = min(c + 1, w), first = c + 1 - m;   // values first .. c, oldest first
      const float mean = numpy_sum_f32(m, [&](int i) { return ring[(size_t)((first + i) % w) * RS]; }) / (float)m;
      const double li = (double)mean;
      a = li + 0.0 == 0.0 ? (float)(C.w64 / 2.0) : (float)(C.w64 * li / (li + 0.0));
    } else if (x + 0.0f == 0.0f) {
      a = (float)(C.w64 / 2.0);
    } else {
      a = C.wide ? (float)(C.w64 * (double)x / (double)(x + 0.0f)) : (C.w32 * x) / (x + 0.0f);
    }
    act[0] = (double)a;
  }
}

// rl_observe_kernel with the controllers (pedn_ctrl_observe, and pedn_ctrl_step when the observations are a launch of their own)
template <bool HIST>
__global__ __launch_bounds__(256) void ctrl_observe_kernel(DevView v, RlView q, int t, int accumulate, CtrlView cv) {
  __shared__ float lds[PEDN_CTRL_LDS_FLOATS];
  rl_observe_body<false, HIST, true>(v, q, t, accumulate, blockIdx.x, lds, &cv);
}

// link_turn_kernel<PR, true, HIST> with the controllers: the last sub-step of a controlled env step (pedn_ctrl_step)
template <bool PR, bool HIST>
__global__ __launch_bounds__(256, 4) void ctrl_link_turn_kernel(DevView v, int t, unsigned n_link_blocks, unsigned n_tp_blocks, unsigned n_tp_heavy,
                                                                RlView q, int accumulate, CtrlView cv) {
  __shared__ double lds[PEDN_TF_LDS_DOUBLES];
  static_assert(sizeof(double) * PEDN_TF_LDS_DOUBLES >= sizeof(float) * PEDN_CTRL_LDS_FLOATS, "observation rows must fit");
  link_turn_body<PR, true, HIST, false, true>(v, t, n_link_blocks, n_tp_blocks, n_tp_heavy, q, accumulate, lds, &cv);
}
