// pedn_plan.hpp -- the step planner: which launches a step consists of, and the host's bookkeeping that this decision reads and advances.
// Pure host C++ (no HIP API call, no engine handle): included by pedn_hip.hip, whose launch_step / launch_split_step perform what a plan
// names, and by tests/plan_prog.cpp on its own (host sanitizers).
//
//   StepState    the marks: what the host knows of the device's state between two launches (ONE member of pedn_sim, `marks`)
//   StepCaps     what a plan reads and a step never changes (static_caps of the engine's plan + what pedn_sim adds: step_caps in pedn_host.hpp)
//   StepRequest  what a caller asks for: the step, the plan family, the chain
//   plan_step / commit_step, plan_split_step / commit_split_step
//                pure decision from (caps, state, request); the commit advances every mark, once per step
//   transitions  one per event outside a step that touches the marks; nothing else assigns them
//   Knobs / PlanInputs / EnginePlan, choose, static_caps, report
//                the plan chooser: which plan an engine steps under at all, decided once at creation (ONE member of pedn_sim, `plan`)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

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

struct StepCaps {   // (what the engine's plan fixes: static_caps(EnginePlan); rl_ready, pr, trow, links, live, T1: step_caps in pedn_host.hpp)
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
  int n_chains = 1;             // chains of the step (a split step: its lean launches, EnginePlan.dead_streams)
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

// The block cutter of a split range (launch_split_block): how many of the steps [t, t1) that are left the lean stream takes in its next
// launch.  K: EnginePlan.dead_block; W: the window of the running average (DevView.W).  Never more than W: step t' of a block reads
// travel_time[t' - 1 - W], and with at most W steps per block the highest such row, (t + n - 1) - 1 - W, lies below the lowest row the
// block writes, t - 1 -- every row a block reads W back was written by an EARLIER launch.  At least one step (W < 1: single steps, which
// dead_link_kernel performs).
constexpr int DEAD_BLOCK_MAX = 16;   // = PEDN_DEAD_BLOCK_MAX of lean_block_kernel: one bit per step in two 32-bit gate masks, one register per step
constexpr int DEAD_BLOCK_DEFAULT = 4, DEAD_BLOCK_WAVES_DEFAULT = 2;   // (profiles/dead_block_settings.txt)
static inline int dead_block_len(int t, int t1, int K, int W) { return std::max(1, std::min(std::min(K, W), std::min(DEAD_BLOCK_MAX, t1 - t))); }

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

// ---- the plan chooser: which plan an engine steps under at all.  pedn_create calls it once (twice where a device fact turns out
// false: choose is a pure function, calling it again with a fact turned off changes nothing but what hangs on that fact), the result is
// pedn_sim::plan and nothing assigns it afterwards.  What moves after creation lives beside it: pedn_sim::chains / warmed_chains (the
// stream probe, pedn_set_streams), rl_fold (pedn_rl_configure).

// The PEDN_* knobs of the step plan as the environment gives them when an engine is created; -1: unset (which is not 0: the default of
// some depends on the model or on an earlier decision).
struct Knobs {
  int fuse_tp = -1;        // PEDN_FUSE_TP=0|1
  int fuse_obs = -1;       // PEDN_FUSE_OBS=0|1
  int streams = -1;        // PEDN_STREAMS=1|2 (anything but 2 is 1)
  int link_owner = -1;     // PEDN_LINK_OWNER=0|1
  int inline_tf = -1;      // PEDN_INLINE_TF=0|1|2 (any other value is 1)
  int quiet = -1;          // PEDN_QUIET=0|1
  int quiet_lean = -1;     // PEDN_QUIET_LEAN=0|1
  int zero_elide = -1;     // PEDN_ZERO_ELIDE=0|1
  int rl_chains = -1;      // PEDN_RL_CHAINS=1|2 (anything but 2 is 1)
  int dead_links = -1;     // PEDN_DEAD_LINKS=0|1
  int dead_waves = -1;     // PEDN_DEAD_WAVES, clamped to 3..8
  int dead_streams = -1;   // PEDN_DEAD_STREAMS=1|2 (anything but 1 is 2)
  int dead_block = -1;     // PEDN_DEAD_BLOCK, clamped to 1..DEAD_BLOCK_MAX
  int dead_block_waves = -1;   // PEDN_DEAD_BLOCK_WAVES, clamped to 2..8
  int stream_probe = -1;   // PEDN_STREAM_PROBE=0|1
};

// the one place that reads them
static inline Knobs knobs_from_env() {
  Knobs k;
  const auto flag = [](const char* name, int* out) { if (const char* f = getenv(name)) *out = atoi(f) != 0; };
  flag("PEDN_FUSE_TP", &k.fuse_tp); flag("PEDN_FUSE_OBS", &k.fuse_obs); flag("PEDN_LINK_OWNER", &k.link_owner);
  flag("PEDN_QUIET", &k.quiet); flag("PEDN_QUIET_LEAN", &k.quiet_lean); flag("PEDN_ZERO_ELIDE", &k.zero_elide);
  flag("PEDN_DEAD_LINKS", &k.dead_links); flag("PEDN_STREAM_PROBE", &k.stream_probe);
  if (const char* f = getenv("PEDN_STREAMS")) k.streams = atoi(f) == 2 ? 2 : 1;
  if (const char* f = getenv("PEDN_INLINE_TF")) k.inline_tf = atoi(f) == 2 ? 2 : atoi(f) != 0;
  if (const char* f = getenv("PEDN_RL_CHAINS")) k.rl_chains = atoi(f) == 2 ? 2 : 1;
  if (const char* f = getenv("PEDN_DEAD_WAVES")) k.dead_waves = std::max(3, std::min(atoi(f), 8));
  if (const char* f = getenv("PEDN_DEAD_STREAMS")) k.dead_streams = atoi(f) == 1 ? 1 : 2;
  if (const char* f = getenv("PEDN_DEAD_BLOCK")) k.dead_block = std::max(1, std::min(atoi(f), DEAD_BLOCK_MAX));
  if (const char* f = getenv("PEDN_DEAD_BLOCK_WAVES")) k.dead_block_waves = std::max(2, std::min(atoi(f), 8));
  return k;
}

// What the decision reads of the description and of the compiled tables (pedn_compile::Tables), and two facts of the device.
struct PlanInputs {
  int RS = 128;            // replicas rounded up to a multiple of 128
  int N = 0, L = 0;        // nodes, physical links
  int n_trow = 0;          // rows of turning fractions computed on the device
  bool node_lp = false;    // the node model is PEDN_NODE_OPTIMAL
  bool hist = false;       // recent-history mode
  bool inline_tf_ok = false;   // every device-computed row is short enough for ONE wave and its probabilities fit PEDN_TF_INL_ROWS LDS rows
  int n_blocks = 0;        // workgroups per replica group of the full packing
  int tiles = 0;           // doubles / 64 of the m * m tiles of its fullest block
  int n_rec = 0;           // its slot records (the idle block included)
  int tf_wave_lds = 0;     // doubles of LDS that each of the eight slot waves of node_kernel<.., TF> has for its own row (PEDN_TF_INL_LDS)
  // The device facts: was the request for more dynamic LDS than a kernel gets by default (64 KB; gfx950 has 160 KB per CU) granted for
  // node_kernel<LU, TF>, and for node_kernel_h?  pedn_create asks (hipFuncSetAttribute) only where the answer can matter -- lds_tf where
  // inline_candidate and node_lds_tf > 64 KB, lds_h where the plan chosen with lds_h = true has inline_help and node_lds_tf > 64 KB -- and
  // leaves the fact at true otherwise: choose reads neither anywhere else.
  bool lds_tf = true, lds_h = true;
};

struct EnginePlan {
  bool node_lp = false;    // PEDN_NODE_OPTIMAL: the node LP instead of the classic rule; no owner-wave plan
  bool hist = false;       // recent-history mode (of the inputs): ring rows are reused -- no zero gate, no dead-link plan
  bool fuse_tp = true;     // the link update and the next step's turn probabilities share one launch (launch_step)
  bool fuse_obs = true;    // pedn_rl_step: observations / rewards ride in the link update's launch (PEDN_FUSE_OBS=0: own launch)
  int chains = 1;          // chains of launches WANTED for long ranges of pedn_run, 1 or 2; pedn_sim::chains is what the stream probe left of it
  bool link_owner = false; // pedn_run: node_kernel(t + 1)'s slot waves perform the link update of t (one launch per step)
  // Single-launch plan of small batches with dynamic turning fractions: every device-computed row is short enough for ONE wave
  // (inline_tf_ok) and the whole node_kernel grid is one generation: the slot waves of node_kernel<LU, TF> compute their own rows, a
  // step is one launch.
  bool inline_tf = false;
  bool inline_help = false;   // ... with helper waves: node_kernel_h, sixteen waves per workgroup
  bool quiet = false;      // quiet corridors (DevView.quiet): node_kernel<LU> launches store the words; which step's may be used: marks.quiet_valid
  bool quiet_lean = true;  // ... and skip the node work that all-zero flows fix (DevView.quiet_lean)
  bool zero_elide = true;  // zero elision (DevView.zg64 / zg32): the marks are marks.zhw64 / zhw32
  int rl_chains = 0;       // pedn_rl_step steps the two halves of the envs as two chains that stay forked ACROSS calls: 0 by batch, 1 | 2 forced
  size_t node_lds = 0;     // dynamic LDS bytes of node_kernel
  size_t node_lds_tf = 0;  // ... of node_kernel<.., TF> and node_kernel_h
  int32_t tf_lds_off = 0;  // DevView.tf_lds_off: node_lds in doubles
  // Dead links (pedn_partition.hpp): in a two-chain range of pedn_run the nodes that provably never see a pedestrian are stepped by
  // dead_link_kernel -- one launch per step for the whole batch on the engine's stream (dead_streams = 2: one per half on the two chain
  // streams) -- and node_kernel<LU> runs over a second packing of the other (live) nodes only, for the whole batch, on a third stream
  // (launch_split_step).
  bool dead_links = true;
  // The live launch is a chain of latencies whose waves share the CUs with the lean kernel's: beside 8 lean waves per SIMD it took 20 us,
  // against 12 us alone (profiles/EXPERIMENTS.md #84; what the lean waves take from it is cache more than issue slots, #85).
  // dead_waves = workgroups of four waves per CU = waves per SIMD the lean kernel may hold (3..8; 8: no limit), through dynamic LDS that
  // it does not use (dead_lds_bytes in pedn_hip.hip: the size leaves the rest of the CU's LDS to the live workgroups).
  int dead_waves = 5;
  int dead_streams = 1;    // 1 | 2: one lean launch per step for the whole batch, or one per half on the chain streams
  // Blocks of steps (lean_block_kernel, launch_split_block in pedn_hip.hip): the lean stream steps up to dead_block steps of a split range
  // per launch, the running sum and the previous receiving flow in registers (1: dead_link_kernel, one launch per step; at run time never
  // more than W steps: dead_block_len).  dead_block_waves: the block kernel's OWN share of the wave places, as dead_waves (2..8).
  int dead_block = DEAD_BLOCK_DEFAULT;
  int dead_block_waves = DEAD_BLOCK_WAVES_DEFAULT;
  bool dead_capable = false;   // the dead-link plan can be taken at all: its buffers are allocated (pedn_sim::d_live_rec and what goes with it)
  // 32-bit words of [2][slot positions][RS / 64][own | inbox] for the full packing (0: no quiet words; melbourne x 1024 ~ 0.3 MB) and
  // for the live packing at its capacity (0: not dead_capable)
  size_t quiet_words = 0, quiet_words_live = 0;
  bool stream_probe = true;   // PEDN_STREAM_PROBE=0: the chains' streams are taken to overlap without being timed (warm_chain_streams)
};

constexpr size_t LDS_DEFAULT = 64 * 1024, LDS_PER_CU = 160 * 1024;

// LDS of node_kernel: 8 (LP: 16) rows of 64 doubles + the m * m tiles of the fullest block; <.., TF>: + the eight slot waves' own rows
// (register budget of the node kernels: node_kernel_waves() in pedn_kernels.hpp)
static inline size_t node_lds_bytes(const PlanInputs& in) { return (size_t)((in.node_lp ? 16 : 8) + in.tiles) * 64 * sizeof(double); }
static inline size_t node_lds_tf_bytes(const PlanInputs& in) { return node_lds_bytes(in) + (size_t)8 * in.tf_wave_lds * sizeof(double); }
// could the single-launch plan be taken if the device grants the LDS it needs?
static inline bool inline_candidate(const PlanInputs& in) { return in.inline_tf_ok && !in.node_lp && node_lds_tf_bytes(in) <= LDS_PER_CU; }
// slot records the live packing of the dead-link plan may need: at most one bin per node, one idle block behind them
static inline size_t live_rec_capacity(int n_nodes) { return ((size_t)n_nodes + 1) * 8; }

static inline EnginePlan choose(const PlanInputs& in, const Knobs& k) {
  EnginePlan p;
  p.node_lp = in.node_lp;
  p.hist = in.hist;
  p.node_lds = node_lds_bytes(in);
  p.node_lds_tf = node_lds_tf_bytes(in);
  p.tf_lds_off = (int32_t)(p.node_lds / sizeof(double));
  // The link update of t and the turning fractions of t+1 share one launch (both only read what node_kernel(t) and earlier
  // launches wrote); PEDN_FUSE_TP=0 gives the fractions a launch of their own in front of node_kernel(t+1).
  if (k.fuse_tp >= 0) p.fuse_tp = k.fuse_tp != 0;
  if (k.fuse_obs >= 0) p.fuse_obs = k.fuse_obs != 0;
  // two chains of launches (one per half of the replicas) in pedn_run; PEDN_STREAMS=1|2, pedn_set_streams.  Default from 640
  // replicas: one chain's launch leaves wave places empty while it fills and drains, and the other half's launches use them
  // (delft x 1024: 51.7 -> 45.3 us per step in round 2; round 5, melbourne / delft: x 640 25.8 -> 23.6 / 36.2 -> 34.3, x 768 27.1 -> 24.8,
  // x 896 31.3 -> 27.5 / 45.3 -> 40.7; x 512 19.2 either way).  The halves are whole 128-replica segments (view_of): 640 = 384 + 256.
  p.chains = k.streams >= 0 ? k.streams : in.RS >= 640 ? 2 : 1;
  // Owner-wave plan of pedn_run (launch_step: lazy): node_kernel<LU>(t + 1) performs the link update of t, one launch per step.  The
  // default for models whose second launch is the link update alone (no turning fractions computed on the device): melbourne x 1024
  // 37.4 -> 32.7-33.7 us per step on one chain, 34.6 -> 30.3 on two (profiles/r04_owner_wave.txt).  With dynamic rows the second launch
  // stays (node_kernel(t + 1) needs the fractions that need node_kernel(t)'s flows) and the longer node_kernel costs more than the
  // link-update workgroups that leave it save (delft x 1024: 42.1-42.6 -> 44.2).  PEDN_LINK_OWNER=0|1 overrides.
  p.link_owner = k.link_owner >= 0 ? k.link_owner != 0 : in.n_trow == 0 && !in.node_lp;
  // Single-launch plan with dynamic turning fractions: the rows computed inside node_kernel<LU, TF> by the slot waves themselves.  That
  // instantiation is built for 2 waves per SIMD (1 block per CU): only where the whole grid is one generation of them -- small
  // batches, which are chains of latencies and gain a whole launch (nine_intersections x 256: 17.2 -> ... us per step).
  const bool large = p.node_lds_tf > LDS_DEFAULT;
  const bool possible = inline_candidate(in) && (!large || in.lds_tf);
  // ... by HELPER waves (node_kernel_h: sixteen waves per workgroup at 128 VGPRs, still one workgroup per CU): the row (~5 us) and the
  // slot wave's own chain (~5 us) side by side -- nine_intersections x 256 16.2 -> 12.5 us per step, 45_intersections x 1024 (272
  // workgroups) 17.9 -> 13.6, x 1280 (340) 20.4 -> 14.7 under pedn_run's two chains and 20.5 -> 19.1 step by step; x 1536 (408) still
  // wins under pedn_run (21.3 -> 17.5) but not step by step (22.3 -> 23.1), at 544 (x 2048) two launches per step are faster either
  // way (22.9 against 23.7).  The default up to 352 workgroups; PEDN_INLINE_TF=0 two launches, 1 the slot waves' own rows, 2 helper
  // waves (forced whatever the grid).  profiles/r04_inline_helpers.txt
  p.inline_tf = possible && (size_t)(in.RS / 64) * (size_t)in.n_blocks <= 352;
  p.inline_help = p.inline_tf;
  if (k.inline_tf >= 0) { p.inline_tf = k.inline_tf != 0 && possible; p.inline_help = k.inline_tf == 2 && possible; }
  if (large && !in.lds_h) p.inline_help = false;
  if (p.inline_tf) p.link_owner = true;
  // quiet corridors: the owner-wave launches skip the loads of corridors that are empty in all 64 replicas of a group (node_step)
  p.quiet = k.quiet >= 0 ? k.quiet != 0 : p.link_owner && !in.node_lp;
  if (k.quiet_lean >= 0) p.quiet_lean = k.quiet_lean != 0;
  // zero elision: the node kernels skip +0.0 stores into rows that hold +0.0 since the last full reset (zero_gate)
  if (k.zero_elide >= 0) p.zero_elide = k.zero_elide != 0;
  // 0 = by batch: two chains where the step is not a pure chain of latencies any more -- from 4096 envs, and from 1024 with per-env
  // scenarios (45_intersections: 2048 envs plain 24.8-25.2 -> 24.7-25.7 us per env step, randomised 27.5-27.9 -> 25.6-26.0;
  // 4096 envs 40.6 -> 35.9; profiles/r04_rl_chains.txt); PEDN_RL_CHAINS=1|2 forces
  if (k.rl_chains >= 0) p.rl_chains = k.rl_chains;
  if (k.dead_links >= 0) p.dead_links = k.dead_links != 0;
  if (k.dead_waves >= 0) p.dead_waves = k.dead_waves;
  if (k.dead_streams >= 0) p.dead_streams = k.dead_streams;
  // Blocks of steps for the lean stream.  Up to 1024 replicas the live launches are the step and the lean stream has time to spare: short
  // blocks at the smallest share of the wave places (melbourne x 1024: 15.8-16.0 -> 14.8-15.0 us per step in the driver's window, 16.0-16.4
  // -> 15.6-15.8 in the default one; share 5: no gain).  Above, the lean stream is the longer one and a share of 2 starves it (x 4096: 41.4-
  // 42.6 -> 45.3-46.2): the share of dead_waves and longer blocks (x 4096 31.9-32.6, x 2048 21.7-22.4 -> 20.9-21.3).
  // profiles/dead_block_settings.txt
  const bool lean_bound = in.RS > 1024;
  p.dead_block = k.dead_block >= 0 ? k.dead_block : lean_bound ? 8 : DEAD_BLOCK_DEFAULT;
  p.dead_block_waves = k.dead_block_waves >= 0 ? k.dead_block_waves : lean_bound ? 5 : DEAD_BLOCK_WAVES_DEFAULT;
  if (k.stream_probe >= 0) p.stream_probe = k.stream_probe != 0;
  const size_t groups = (size_t)(in.RS / 64);
  if (p.quiet) p.quiet_words = (size_t)2 * (size_t)in.n_rec * groups * 2;
  // dead links: room for a packing of the live nodes alone, its quiet words (node_step indexes the words of one step, half of them, in
  // 32 bits), and the records of every slot dead_link_kernel may step
  const size_t live_words = (size_t)2 * live_rec_capacity(in.N) * groups * 2;
  p.dead_capable = p.dead_links && p.quiet && p.link_owner && !p.inline_tf && !in.hist && !in.node_lp && in.n_trow == 0 && in.L > 0 &&
                   live_words / 2 < ((size_t)1 << 31);
  if (p.dead_capable) p.quiet_words_live = live_words;
  return p;
}

// the part of StepCaps that the engine's plan fixes
static inline StepCaps static_caps(const EnginePlan& p) {
  StepCaps c;
  c.node_lp = p.node_lp; c.inline_tf = p.inline_tf; c.inline_help = p.inline_help;
  c.quiet = p.quiet; c.quiet_lean = p.quiet_lean;
  c.fuse_tp = p.fuse_tp; c.fuse_obs = p.fuse_obs;
  c.zero_elide = p.zero_elide; c.hist = p.hist;
  return c;
}

// What pedn_plan_info reports of the plan; links: the model has physical links (n_pairs_corr > 0).
struct PlanReport {
  int owner_wave;    // [1] steps take the owner-wave family (with device-computed rows: the single-launch plan, inline_tf)
  int quiet;         // [5] ... and its launches keep and use the quiet-corridor words
  int zero_elide;    // [6] the node kernels may skip +0.0 stores into clean rows
  int quiet_lean;    // [8] the quiet-corridor launches take the lean path
  int dead_links;    // [9] may be other than 0: the split plan is not ruled out for good (the rest: dl_split_ok, pedn_hip.hip)
};
static inline PlanReport report(const EnginePlan& p, bool links) {
  PlanReport r;
  r.owner_wave = p.link_owner && !p.node_lp && links;
  r.quiet = p.quiet && r.owner_wave;
  r.zero_elide = p.zero_elide && !p.hist;
  r.quiet_lean = p.quiet_lean && r.quiet;
  r.dead_links = p.dead_capable && links;
  return r;
}

}  // namespace pedn_plan
