// pedn_plan.hpp -- the step planner: which launches a step consists of, and the host's bookkeeping that this decision reads and advances.
// Pure host C++ (no HIP API call, no engine handle): included by pedn_hip.hip, whose launch_step / launch_split_step perform what a plan
// names, and by tests/plan_prog.cpp on its own (host sanitizers).
//
//   StepState    the marks: what the host knows of the device's state between two launches (ONE member of pedn_sim, `marks`)
//   StepCaps     what a plan reads and a step never changes (pedn_sim fills it: step_caps in pedn_host.hpp)
//   StepRequest  what a caller asks for: the step, the plan family, the chain
//   plan_step / commit_step, plan_split_step / commit_split_step
//                pure decision from (caps, state, request); the commit advances every mark, once per step
//   transitions  one per event outside a step that touches the marks; nothing else assigns them
#pragma once
#include <algorithm>

struct CtrlView;   // (pedn_types.hpp) a request only carries the pointer

namespace pedn_plan {

constexpr int ALL_ROWS = 0x7fffffff;   // valid_hi: no lazy reset in effect; zhw64 / zhw32: no gate until the next full reset

struct StepState {
  int valid_hi = ALL_ROWS;   // lazy reset: history rows above this index are neither written nor cleared (mirrored into DevView.valid_hi by the launcher)
  int link_pending = -1;     // owner-wave plan: step whose link update has not been performed yet, -1 none
  // Quiet corridors (DevView.quiet): quiet_valid = the step whose words every replica group has, from a node_kernel<LU> launch on each
  // chain with no change of a history row since -- the next LU launch may use them; -1 none.  Cleared by everything that could break that
  // (touch).  quiet_pack: which packing's words quiet_valid speaks of: 0 the full bin set (d_quiet), 1 the live bins (d_quiet_live).
  int quiet_valid = -1;
  int quiet_pack = 0;
  // Zero elision (DevView.zg64 / zg32): zhw64 = the highest row of inflow / outflow / cumulative_inflow / cumulative_outflow, zhw32 = of
  // num_pedestrians / density / link_flow, that may hold anything but +0.0 -- -1 after a full reset (which leaves every row at +0.0), kept
  // by the lazy reset (the old episode's rows stay), ALL_ROWS when something the host does not follow may write them (a zero-copy pointer,
  // the clocked steps) until the next full reset.  A launch that writes row x of a group gets the gate iff x > the group's mark; the mark
  // is raised to x when the step commits (both chains of a step decide from the marks before it).  Only zeros are ever written below the
  // marks' back (clear_rows, catch_up), so they need not raise them.
  int zhw64 = ALL_ROWS, zhw32 = ALL_ROWS;
  int zgated = 0;            // node-kernel launches with a gate open since the last reset of either kind (pedn_plan_info info[7])
  // Dead links (pedn_partition.hpp):
  //   dl_grow   nothing has run since the last FULL reset: a recomputed dead set replaces the old one; otherwise it is intersected with it
  //             (rows above valid_hi may hold a previous episode's values, and a link that ever carried someone holds them anywhere)
  //   dl_off    something the host does not follow may have written a state or history field (a zero-copy pointer, the clocked steps):
  //             no split until the next full reset -- the events that set zhw64 / zhw32 to ALL_ROWS
  bool dl_grow = true, dl_off = false;
  int split_steps = 0;       // steps launched by launch_split_step since the last reset of either kind (pedn_plan_info info[10])
  int tp_ready = -1;         // step whose turning fractions are in tfd[step & 1] (written by link_turn_kernel of the step before, or inline), -1: none
  int last_t = -1;           // last step launched (pedn_get_turning_fractions: which buffer holds a dynamic node's fractions)
  long step_epoch = 1;       // counts launched steps; h_tf_set_epoch[node] == step_epoch: fractions imposed since the last step
  int second_launch = 0;     // the last launch_step: a launch followed node_kernel (the profiling entry points)
  int tp_ran = 0;            // a launch_step launched the stand-alone turn_frac_kernel since the caller cleared this (the profiling entry points)
};

struct StepCaps {
  bool node_lp = false;      // PEDN_NODE_OPTIMAL: no owner-wave plan
  bool inline_tf = false;    // single-launch plan: node_kernel<LU, TF> computes the device-computed rows
  bool inline_help = false;  // ... by helper waves (node_kernel_h)
  bool quiet = false, quiet_lean = false;
  bool fuse_tp = false;      // the fractions of t + 1 ride in the launch behind node_kernel(t)
  bool fuse_obs = false, rl_ready = false;   // ... and so do the observations of an env step
  bool zero_elide = false, hist = false;     // (recent-history mode: ring rows are reused, never a gate)
  bool pr = false;           // per-replica link parameters
  bool trow = false;         // rows of fractions computed on the device (n_trow > 0)
  bool links = false;        // physical links (n_pairs_corr > 0)
  bool live = false;         // the live packing of the dead-link plan has a block (n_live_blocks > 0)
  int T1 = 0;
};

struct StepRequest {
  int t = 0;
  bool lazy = false;            // owner-wave family: leave the link update of t to node_kernel<LU>(t + 1) or to a flush
  int observe = -1;             // >= 0: an env step's observations of t, the value is rl_observe's accumulate flag
  const double* fold = nullptr; // gater actions that node_kernel applies itself (the first sub-step of an env step)
  const CtrlView* ctrl = nullptr;   // the observing launch is the controller twin
  int chain = -1;               // -1: the whole batch on the engine's stream; else this chain's share of the replicas on its stream
  int n_chains = 1;             // chains of the step (a split step: its lean launches, pedn_sim.dead_streams)
  bool profiled = false;        // the launches are bracketed by the caller's events
};

enum Second { SECOND_NONE = 0, SECOND_LINK = 1, SECOND_LINK_TURN = 2 };   // link_kernel_1r alone / link_turn_kernel or its controller twin

struct StepPlan {
  int t = 0;
  bool lazy = false;         // the request's, where the owner-wave family exists at all
  bool flush = false;        // the pending link update first, as a launch of its own
  bool tf_alone = false;     // then the stand-alone turning fractions of t
  // the node launch
  bool lu = false, inl = false, helpers = false;
  bool quiet = false, quiet_use = false, quiet_lean = false;
  int zg64 = 0, zg32 = 0;
  // the launch behind it
  Second second = SECOND_NONE;
  bool link = false, fused = false, obs = false, ctrl = false;   // its parts: link update of t, fractions of t + 1, observations (controller twin)
  bool one_r = false;        // its link update runs one replica per lane
  bool commits = false;      // the step's last chain: the marks advance
};

struct SplitPlan {
  int t = 0, lean_launches = 1;
  bool live = false, quiet_use = false, quiet_lean = false;
  int zg64 = 0, zg32 = 0;
};

// zero elision: may a launch that writes row `row` of a group whose mark is `hw` skip its +0.0 stores?
static inline int zero_gate(const StepCaps& c, int hw, int row) { return c.zero_elide && !c.hist && row > hw ? 1 : 0; }

// One step = [flush] [turn_frac_kernel(t)] node_kernel(t) [second launch].  Every chain of a step gets the same plan: only the last
// one commits, and a flush in front of an earlier chain's launches leaves link_pending as it is.
static inline StepPlan plan_step(const StepCaps& c, const StepState& st, const StepRequest& rq) {
  StepPlan p;
  const int t = p.t = rq.t;
  p.commits = rq.chain < 0 || rq.chain == rq.n_chains - 1;
  p.lazy = rq.lazy && !c.node_lp && c.links;
  // single-launch plan (inline_tf): node_kernel<LU, TF> computes the device-computed rows itself -- wherever it can be the LU kernel
  const bool inl_plan = p.lazy && c.inline_tf && c.trow;
  const bool can_inl = inl_plan && st.link_pending == t - 1 && t >= 2;
  p.tf_alone = c.trow && st.tp_ready != t && !can_inl;   // first step of an episode, a repeated or an out-of-order step
  // a pending link update is flushed when this is not the step it waits for, or when this step starts with the stand-alone turning
  // fractions (they read num_pedestrians[t - 1] as stored)
  p.flush = st.link_pending >= 0 && (!(p.lazy && st.link_pending == t - 1) || p.tf_alone);
  p.lu = p.lazy && st.link_pending == t - 1 && t >= 2 && !p.flush;
  p.inl = can_inl && p.lu;
  p.helpers = p.inl && c.inline_help;
  // quiet corridors: every node_kernel<LU> launch (not the single-launch plan's <LU, TF>) stores the words of step t; it uses those of
  // t - 1 when the launch of t - 1 was one of them and nothing has touched the history since (the words of a split step belong to the
  // live packing)
  p.quiet = p.lu && !p.inl && c.quiet;
  p.quiet_use = p.quiet && st.quiet_valid == t - 1 && st.quiet_pack == 0;
  p.quiet_lean = p.quiet && c.quiet_lean;
  // zero elision: node_kernel(t) writes row t of the flows and cumulative counts, node_kernel<LU>(t) also row t - 1 of num_pedestrians /
  // density (the link update behind an ordinary node kernel writes row t of those, ungated).  The marks as they are before this step: a
  // flush raises zhw32 first, but then this node kernel is not the LU one and writes no row of num_pedestrians / density.
  p.zg64 = zero_gate(c, st.zhw64, t);
  p.zg32 = p.lu ? zero_gate(c, st.zhw32, t - 1) : 0;
  // the turning fractions of t + 1 ride in the launch behind node_kernel(t) -- except behind the last step of the horizon, where
  // pair_pod / turn_tab have no row T + 1 to read (they hold T + 1 rows, 0..T) and nothing would consume the result
  // (and not under the single-launch plan, where the next step computes its own rows)
  p.fused = c.trow && c.fuse_tp && t + 1 <= c.T1 - 1 && !inl_plan;
  p.obs = rq.observe >= 0 && c.rl_ready && c.fuse_obs;
  p.ctrl = p.obs && rq.ctrl != nullptr;
  // link update: one replica per lane as a launch of its own and with per-replica parameters, two inside link_turn_kernel (link_body);
  // lazy: no link-update workgroups in this step's second launch
  p.one_r = c.pr || (!p.fused && !p.obs);
  p.link = !p.lazy && c.links;
  p.second = p.fused || p.obs ? SECOND_LINK_TURN : p.link ? SECOND_LINK : SECOND_NONE;
  return p;
}

// One step t >= 2 of a split range (launch_split_step): rq.n_chains launches of dead_link_kernel and, where the live packing has a block,
// node_kernel<LU> over it.
static inline SplitPlan plan_split_step(const StepCaps& c, const StepState& st, const StepRequest& rq) {
  SplitPlan p;
  p.t = rq.t;
  p.lean_launches = rq.n_chains;
  p.zg64 = zero_gate(c, st.zhw64, rq.t);
  p.zg32 = zero_gate(c, st.zhw32, rq.t - 1);
  p.live = c.live;
  p.quiet_use = st.quiet_valid == rq.t - 1 && st.quiet_pack == 1;
  p.quiet_lean = c.quiet_lean;
  return p;
}

// ---- commits
// what every committed step leaves behind: node launches of t on every replica [lu: they performed the link update of t - 1], the link
// update of t pending or not, quiet words of t in packing `pack` or none
static inline void step_done(StepState& st, int t, bool lu, bool pending, bool quiet, int pack) {
  st.link_pending = pending ? t : -1;
  st.quiet_valid = quiet ? t : -1;
  st.quiet_pack = pack;
  st.zhw64 = std::max(st.zhw64, t);
  if (lu) st.zhw32 = std::max(st.zhw32, t - 1);
  if (st.valid_hi != ALL_ROWS && t > st.valid_hi) st.valid_hi = t;   // rows <= t are written once this step's launches are
  st.last_t = t;
  ++st.step_epoch;
}

// behind the launches of one chain of a step (after `flushed`, where the plan flushed)
static inline void commit_step(StepState& st, const StepPlan& p) {
  if (p.tf_alone) st.tp_ran = 1;
  if (p.zg64 || p.zg32) ++st.zgated;
  st.second_launch = p.second != SECOND_NONE;
  if (!p.commits) return;   // the other chains of this step still have to see the old marks
  step_done(st, p.t, p.lu, p.lazy, p.quiet, 0);
  st.dl_grow = false;   // something has run since the last full reset
  if (p.link) st.zhw32 = std::max(st.zhw32, p.t);   // the link update of t in the second launch
  // the stand-alone launch of t wrote tfd[t & 1]: fractions of another step that were kept there are gone (a step that jumps and leaves
  // no fractions behind -- the single-launch plan, PEDN_FUSE_TP=0, the horizon's last step -- would else leave tp_ready naming them)
  if (p.tf_alone && st.tp_ready >= 0 && ((st.tp_ready ^ p.t) & 1) == 0) st.tp_ready = -1;
  if (p.inl) st.tp_ready = p.t;   // the fractions of t are in tfd[t & 1] (a following step that cannot inline computes its own)
  if (p.fused) st.tp_ready = p.t + 1;
}

static inline void commit_split_step(StepState& st, const SplitPlan& p) {
  if (p.zg64 || p.zg32) st.zgated += p.lean_launches + (p.live ? 1 : 0);
  ++st.split_steps;
  st.second_launch = 0;
  step_done(st, p.t, true, true, p.live, 1);
}

// ---- transitions: the events outside a step
// something may change a history row or break the chain of node_kernel<LU> launches: the quiet words of the last step may not be used
static inline void touch(StepState& st) { st.quiet_valid = -1; }
// the pending link update was performed as a launch of its own on every replica (num_pedestrians / density of that row written)
static inline void flushed(StepState& st) {
  touch(st);
  st.zhw32 = std::max(st.zhw32, st.link_pending);
  st.link_pending = -1;
}
// a setter changed something the fractions in tfd were computed from (or imposed other fractions)
static inline void fractions_invalid(StepState& st) { st.tp_ready = -1; }
// a changed input of the dead-link proof gave another dead set: the quiet words were stored under the old work lists
static inline void dead_set_changed(StepState& st) { touch(st); }
// a profiling entry point is about to launch a step and look at tp_ran / second_launch behind it
static inline void profile_begin(StepState& st) { st.tp_ran = 0; }
// both resets: the bookkeeping back to "nothing has run" (a pending link update is discarded: the state it would complete is cleared)
static inline void episode_reset(StepState& st) {
  st.tp_ready = st.last_t = st.link_pending = -1;
  touch(st);
  st.zgated = st.split_steps = 0;
}
static inline void reset_full(StepState& st) {
  episode_reset(st);
  st.valid_hi = ALL_ROWS;
  st.zhw64 = st.zhw32 = -1;   // every row of the six fields is +0.0 once the rows are cleared
  st.dl_grow = true;          // dead links: proven afresh from here
  st.dl_off = false;
}
// (the zero-elision marks stay: the rows above row 0 still hold the old episode's values)
static inline void reset_lazy(StepState& st) {
  episode_reset(st);
  st.valid_hi = 0;
}
// rows (valid_hi, upto] were cleared (upto = ALL_ROWS: every row there is, no lazy reset in effect any more)
static inline void caught_up(StepState& st, int upto) {
  touch(st);
  if (upto > st.valid_hi) st.valid_hi = upto;
}
// something the host does not follow may write the 64-bit / 32-bit zero-elided fields (a zero-copy pointer, a clocked section: both)
static inline void foreign_write(StepState& st, bool f64, bool f32) {
  st.dl_off = true;
  if (f64) st.zhw64 = ALL_ROWS;
  if (f32) st.zhw32 = ALL_ROWS;
}
// a clocked section that began at step t0 ended with the device's clock at t_now (steps t0 .. t_now - 1 ran) and its valid_hi
static inline void clock_ended(StepState& st, const StepCaps& c, int t0, int t_now, int valid_hi) {
  touch(st);
  if (t_now > t0) {
    st.last_t = t_now - 1;
    st.step_epoch += t_now - t0;
    st.tp_ready = (c.trow && t_now <= c.T1 - 1) ? t_now : -1;   // link_turn_kernel(t_now - 1) left the fractions of t_now
    st.link_pending = -1;
  }
  st.valid_hi = valid_hi;
}

}  // namespace pedn_plan
