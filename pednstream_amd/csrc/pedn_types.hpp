// pedn_types.hpp -- device-visible data structures of the HIP engine: the per-link parameter record, the scalar records
// one wave reads, and the view of all HBM arrays that every kernel receives by value.  See DESIGN.md section 4 for the layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pedn.h"

// ------------------------------------------------------------------------------------------------- device view
enum { F_IN = 0, F_OUT, F_CI, F_CO, F_S, F_R, F_GATE };
enum { G_TT = 0, G_ATT, G_N, G_K, G_V, G_LF };
// History rows that node_step(t) addresses at a row index every wave of the launch shares (DevView.rb; t' = t - 1, t'' = t - 2 wrapped
// as wrap_idx does): RB_<field>_<T: row t, P: row t', Q: row t'', W: row t' - W>
enum {
  RB_IN_P = 0, RB_IN_T, RB_OUT_P, RB_OUT_T, RB_CI_P, RB_CI_T, RB_CO_P, RB_CO_T, RB_S_Q, RB_S_P, RB_R_Q, RB_R_P, RB_GATE_P,
  RB_N_Q, RB_N_P, RB_K_P, RB_V_P, RB_TT_P, RB_LF_P, RB_ATT_P, RB_TT_W, RB_COUNT
};

struct LinkP {  // static per-link parameters, wave-uniform on the device
  double length, width, vf, kc, kj, gamma, act, bi, noise;
  double kjA;                                  // kj * (length * width): jam capacity of an unseparated link (link.py:386)
  float tt0;
  float kc32, kj32, dk32, area32, gamma32;     // (float)kc, (float)kj, (float)(kj - kc), (float)(length * width), (float)gamma:
                                               // the float32 casts the formulas take of wave-uniform doubles, made once on the host
  int32_t rev, sep, fd, tau_sw, fft;
  int32_t pad;
  __host__ __device__ void derive() {
    kjA = kj * (length * width);
    kc32 = (float)kc; kj32 = (float)kj; dk32 = (float)(kj - kc); area32 = (float)(length * width); gamma32 = (float)gamma;
  }
};

// Per-replica scenario parameters of one (link, replica): ONE 32-byte record -- two 16-byte loads per lane -- instead of six arrays
// (randomised ensembles / RL resets, env_loader.py:363-424).  The look-backs fit 16 bits (pedn_set_link_params checks).
struct alignas(16) LinkPR {
  double kc, kj, vf;      // k_critical, k_jam, free_flow_speed
  float tt0;              // travel_time[0] (link.py:83)
  int16_t fft, tau_sw;    // free_flow_tau (link.py:86), shock-wave look-back (link.py:380)
};
static_assert(sizeof(LinkPR) == 32, "LinkPR must stay two 16-byte loads");

struct SlotRec {  // one wave of node_kernel: a (node, slot) with everything static it needs, fetched by ONE scalar load burst (filled by pedn_compile::pack)
  // dyn: where the slot's row of turning fractions comes from -- 0 tf / tf_u (default or imposed), 1 tfd[t & 1] (turn_frac_kernel),
  // 2 turn_tab[t] / turn_tab_r (every product constant: replica-independent, tabulated and renormalised on the host)
  // act: action slot of the batched RL step that sets this slot's gate (back gate of lout = front gate of lin), -1 none
  // lp: index of the node among those that solve the node LP (assign_flows_type 'optimal'), on the node's slot 0, else -1
  // trow: the slot's row record in trow_words when the row's turning fractions are computed on the device (dyn == 1), else -1
  // mirror: position (block * 8 + wave) of the slot at the corridor's other end -- the one whose incoming link is this slot's
  // outgoing link -- for the quiet-corridor words (DevView.quiet); -1 for a virtual pair
  int32_t node, slot, base, m, kind, dyn, lin, lout, turn0, demand_row, act, lp, trow, mirror;
  LinkP Pin, Pout;  // parameters of the incoming / outgoing link of the slot (unused for a virtual pair)
};

// One wave of dead_link_kernel: what the step of a slot that no pedestrian reaches has left once every operand that is a literal +0.0, a
// field of the slot's SlotRec, a shared gate or a launch constant has been evaluated -- by dead_prep_kernel, on the device, through the
// device functions the step itself calls (pedn_kernels.hpp), whenever dl_refresh runs.  One scalar load burst at the top of the wave.
// A virtual pair (lin >= L) uses lin and lout only.
enum { DEAD_IS64 = 1u, DEAD_GATE_REC = 2u };
struct alignas(16) DeadRec {
  int32_t lin, lout;
  float ka, kb;               // density[t'] of the incoming link and of its reverse: +0.0 / area
  double v64, length, noise;  // speed_base of (ka, kb) in its binary64 form (DEAD_IS64), Pin.length, Pin.noise
  double send;                // sending flow of the incoming link once t' >= fft (send_flow on +0.0 inputs and the shared front gate)
  double rr0, rr1;            // receiving bound of the outgoing link before smoothing: t' + 1 - tau_sw < 0, otherwise (recv_flow)
  double gate;                // shared back gate of the outgoing link; DEAD_GATE_REC: it differs from Pout.width (the gate-record rule)
  float v32, tt0;             // speed_base in its float32 form, Pin.tt0
  int32_t fft, tau_sw;        // Pin.fft, Pout.tau_sw
  uint32_t bits;              // DEAD_IS64 | DEAD_GATE_REC
  uint32_t fl_send, fl_rr0, fl_rr1;   // error flags that send (but for the per-lane same-step flag) / rr0 / rr1 raise
};
static_assert(sizeof(DeadRec) <= 128, "DeadRec must stay one short scalar load burst");

struct CorrRec {  // one lane group of link_kernel: both directions of a corridor
  int32_t a, b, pad0, pad1;
  LinkP Pa, Pb;
};

// ---- route choice (path_finder.py:561-737), organised per row (= incoming slot) of a dynamic node: one wave of
// turn_frac_kernel owns (row, 64 replicas).  Its static data are int32 word records fetched with vector loads (lane k holds
// word k) and broadcast with v_readlane -- see turn_frac_body.
#define PEDN_TF_LDS_ROWS 64    // LDS rows (64 lanes x 8 bytes) of one workgroup = 4 rows of dynamic nodes, shared out by the compiler (pedn_compile.hpp)
#define PEDN_TROW_WORDS 128
#define PEDN_TF_INL_ROWS 8     // LDS rows a slot wave of node_kernel<.., TF> has for the probabilities of its own row (single-launch plan)
#define PEDN_TF_COOP_GROUPS 8   // rows with more multi-entry groups get a workgroup of their own (see turn_frac_body)
// row record, PEDN_TROW_WORDS words (m = -1: padding), written by pedn_compile::compile:
//   [0] m  [1] first turn of the row  [2] first group (index into tgrp_words / 32)  [3] number of multi-entry groups
//   [4] Q0  [5] Q1: the row's (turn, od) products  [6] n_used outgoing links below  [7] some of them is a separator
//   entries e = 0..4 at 8 + 10 e, e = 5, 6 at 64 + 10 (e - 5): link, reverse link, separator flag, float32(length * width),
//       free-flow speed (2 words), k_critical (2), length (2); entries >= n_used repeat entry 0
//   turns jj = 0..6 at 84 + 3 jj: q0, q1 (absolute product indices), mode (1: every product is the constant 1 -> the raw
//       fraction is tabulated per step on the host)
//   [107] 1: some probability of the row lives in ent_p instead of LDS
//   [108] 1: coop -- the four records of this workgroup are the same row; its groups and turns are shared out over the waves
//   [109] first LDS row of this row inside its workgroup (the inline variant rebases to it)
// group record, 32 words (softmax group (od, up) with more than one downstream, update_node_turn_probs :561-589):
//   [0] n  [1] allphys  [2 + e] entry of the row record the downstream link is (-1: virtual link, density 0, capacity 100)
//   [9 + e] where P(down | up, od) goes: < 0 nowhere, < PEDN_TF_LDS_ROWS that LDS row of the workgroup, else row
//   (value - PEDN_TF_LDS_ROWS) of ent_p   [16 + 2 e] alpha * distance / (sum of the group's distances + 1e-6) (2 words)

struct DevView {
  double* f64[7];
  float* f32[6];
  float* rsum;
  double *front, *back, *sepw, *sepnp, *tf, *demand, *ent_p;
  double* tfd[2];  // [n_turns][RS] x 2: fractions of dynamic nodes; step t reads tfd[t & 1], the fractions of t + 1 are
                   // written into the other buffer while the host can still read those of t
  // replica-uniform shortcuts (NaN = the value differs between replicas, read the per-replica row instead): a value every
  // replica shares is one scalar load per wave instead of 8 bytes per lane
  const double *front_u, *back_u;  // [L]
  const double* tf_u;              // [n_turns]
  // per-replica scenario parameters (randomised ensembles / RL resets, env_loader.py:363-424); used when pr != 0
  const LinkPR* prm;                  // [L][RS] k_critical, k_jam, free_flow_speed, free_flow_tau, shock-wave look-back, travel_time[0]
  const double *pair_pod_r, *turn_tab_r;  // [n_pair][RS], [n_turns][RS]: P(od | up) with per-replica, time-constant OD weights
  int32_t pr, pod_pr;
  const double* od_w;
  uint32_t* flags;
  const LinkP* lp;
  const SlotRec* slot_rec;
  const CorrRec* corr_rec;
  const int32_t *node_kind, *node_slot_ptr, *node_turn_ptr, *node_demand_row, *node_dyn, *slot_in, *slot_out;
  const int32_t* pair_row;      // [n_pair] where the product's P(down | up, od) is: -1 the constant 1 (single-entry group), else as word 9 + e of a group record
  const int32_t* trow_words;    // [n_trow][PEDN_TROW_WORDS] rows of dynamic nodes, heaviest first
  const int32_t* tgrp_words;    // [n_multi + 8][32] groups with more than one downstream entry (single-entry groups have P = 1 exactly)
  const double* turn_tab;       // [T+1][n_turns] tabulated raw fractions of such turns
  const double* pair_pod;  // [T+1][n_pair] P(od | up) of the pair's upstream group, replica independent
  int32_t L, Lall, T1, RS, R, W, n_grp, n_multi, n_trow, n_pairs_corr, n_pair, n_turns;
  double dt, pf_temp, pf_alpha, pf_beta, pf_omega, pf_eps;
  uint32_t k0, k1, replica_offset;
  int32_t meanfield;
  int32_t tf_general;  // diagnostics (PEDN_TF_GENERAL): 1 the any-size softmax path, 2 the general row-sum path of turn_frac_body
  // history rows: time index t lives in row (t & mask).  Full-record mode: every mask is 0x7fffffff (row = t, T+1 rows, the
  // reference's own footprint).  Recent-history mode (hist = 1): inflow and cumulative_inflow keep all rows (the sending
  // flow looks back an unbounded, data-dependent number of steps into them), the others are rings of mask + 1 rows.
  int32_t m64[7], m32[6];
  int32_t hist;
  // Lazy reset (pedn_reset_lazy, full-record mode): rows above valid_hi have neither been written nor cleared since the last reset and
  // hold the previous episode's values.  The only reads that can land there are the wrapped (negative) indices of get_outflow's
  // look-backs (link.py:205-212: Python's inflow[-k] = the untouched tail = 0): answered with the initial value instead of the row.
  // 0x7fffffff after an ordinary reset.
  int32_t valid_hi;
  // Device-resident step clock (pedn_rl_clock_begin / pedn_rl_step_clocked): a launch whose step argument is negative takes its step --
  // and the node kernel its valid_hi -- from here, see node_clock in pedn_kernels.hpp.  [0] node_kernel's step, [1] the step of the
  // launch behind it, [2] valid_hi.
  int32_t* clock;
  int32_t tf_lds_off;   // node_kernel<.., TF>: first double of the waves' private LDS rows for their own turning fractions (PEDN_TF_INL_ROWS each)
  int32_t pairs_adj;  // 1: corridor p is the links (2p, 2p + 1) -- the reference creates the two directions of an edge one after the other --
                      // so the link update forms its row addresses from p alone, without waiting for the corridor's record
  int32_t sub0, subRS;  // replicas [sub0, sub0 + subRS) are this launch's share (the whole batch, or one half of it per stream)
  // gater actions applied inside node_kernel (pedn_rl_step, gater-only agent sets): row-major [R][rl_A] widths, NaN = no action
  const double* rl_actions;
  int32_t rl_A;
  double rl_max_delta_gate;
  // node LP (PEDN_NODE_OPTIMAL): per (LP node, replica group) a tableau of lp_stride doubles x 64 lanes and lp_bstride basis ids
  double* lp_ws;
  int32_t* lp_basis;
  size_t lp_stride, lp_bstride;
  // Quiet corridors (owner-wave plan, node_kernel<LU>; PEDN_QUIET): words [2][quiet_npos][RS / 64][2] -- [step & 1][slot position
  // (block * 8 + wave)][replica group][own | inbox].  Launch t stores t + 1 into its own word and into its mirror's inbox word when,
  // in all 64 replicas, everything it wrote for its end of the corridor is +0.0, else 0 (see node_step).  quiet_use: the host vouches
  // that launch t - 1 on this chain was such a launch and nothing has changed a history row since (launch_step); nullptr: neither
  // loaded nor stored.
  uint32_t* quiet;
  int32_t quiet_use, quiet_npos;
  // Zero elision (full-record mode; PEDN_ZERO_ELIDE): the host vouches that the row this launch writes of inflow / outflow /
  // cumulative_inflow / cumulative_outflow (zg64: row t) and of num_pedestrians / density (zg32: row t - 1, node_kernel<LU>) holds +0.0
  // -- not written since the last full reset but by zeros (pedn_sim.zhw64 / zhw32).  A wave then skips a pair of stores whose values
  // are +0.0 in all 64 lanes (node_step).  0 in the engine's own view: set only in the copy a step launch carries.
  // zg32 covers link_flow too: its quiet value ks * speed is +0.0 wherever num_pedestrians is.
  int32_t zg64, zg32;
  // Lean quiet step (PEDN_QUIET_LEAN; set with DevView.quiet): a slot wave whose column / row of the node's products P * s holds +0.0 in
  // all 64 lanes skips its column pass / row sums, whose results that fixes (node_step)
  int32_t quiet_lean;
  // Row bases (node_step, every node kernel but the clocked one): first byte of the history row RB_k of this launch's step, through the same
  // full-record / ring mapping as R64 / R32 -- the same for every wave of the grid, so the host forms them once per launch (row_bases in
  // pedn_hip.hip) and a wave adds only its column's element offset.  quiet_rd / quiet_wr: the halves of DevView.quiet that launch t reads
  // (step t - 1) and writes (step t).  Unset in the engine's own view: set only in the copy a node-kernel launch carries.
  char* rb[RB_COUNT];
  uint32_t *quiet_rd, *quiet_wr;
};

// ---- views of the training-side subsystems (pedn_ctrl / norm / rollout / replay.hpp): what their launches carry by value.  Here, not with
// their kernels, because the engine's handle embeds them (pedn_host.hpp); pedn_rl_clock_signature hashes them as bytes.
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

struct NormView {
  const float *obs, *rew;        // the raw rows: [R][O], [R][n_agents]
  float *obs_n, *rew_n;          // the normalised rows (rew_n right behind obs_n)
  double *mean, *var, *count;    // [O] each
  double *ret;                   // [R][n_agents] discounted returns
  double *ret_stats;             // mean, var, count of the returns
  const int32_t* tracked;        // [O] 1: normalised; 0: copied (a gater's gate width)
  const int32_t* clock;          // the device-resident step clock (a clocked launch takes `terminated` from it)
  int32_t R, O, n_agents, T;
  int32_t norm_obs, norm_reward, training, pad_;
  double clip_obs, clip_reward, gamma;
};

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

struct ReplayView {
  const float *obs_src, *rew_src;   // what the fetches hand out: the normalised rows while the running normalisation is on
  float* frames;
  double* actions;
  float *rewards, *done, *stacked;
  int64_t *first, *step_serial, *state;
  const int32_t* clock;             // the device-resident step clock
  int64_t cap, R;
  uint32_t k0, k1;                  // key(seed)
  int32_t N, A, n_actions, n_obs, stack, T;
};
