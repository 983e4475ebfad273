// pedn_host.hpp -- the engine's handle (pedn_sim) and the host helpers that the core (pedn_hip.hip) and the host sections of the subsystem
// headers share: error reporting, device allocations, host <-> device staging, and the declarations of the core services a subsystem may
// call.  Included by pedn_hip.hip behind pedn_kernels.hpp and in front of the subsystem headers.
#pragma once
#include <hip/hip_ext.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pedn_kernels.hpp"
#include "pedn_plan.hpp"

static thread_local std::string g_last_error;

struct pedn_sim;
// Device allocations with an owner of their own (a store that is freed while the engine lives on); what lives as long as the engine goes
// into pedn_sim::allocs (upload / dalloc).
namespace {   // (internal to the library's one translation unit, like the static helpers)
struct DevicePool : std::vector<void*> {
  int take(pedn_sim* s, size_t bytes, void** out);   // hipMalloc + hipMemset to 0 of max(bytes, 16), registered here
  void drop();                                       // hipFree of everything taken
};
}  // namespace

// Per-subsystem state of the handle: the view the subsystem's launches carry by value (zeroed while there is none; hashed as bytes by
// pedn_rl_clock_signature) and the host's flags.
// rule-based controllers (pedn_ctrl.hpp); any: some agent has a controller (else a controlled step applies no actions at all), rows: the
// moving-average rows allocated in view.ring
struct CtrlState { CtrlView view{}; bool ready = false, any = false; int rows = 0; };
// running normalisation (pedn_norm.hpp): its buffers belong to the agent set (pedn_sim::allocs); [O] tracked mask, agent of every column
struct NormState { NormView view = {}; bool on = false, alloc = false; std::vector<int32_t> tracked, agent; };
// rollout store (pedn_rollout.hpp) and replay store (pedn_replay.hpp), each with its own allocations; the two may live side by side
struct RolloutState { RolloutView view = {}; bool on = false, begun = false, finished = false; int rows = 0; DevicePool mem; };
struct ReplayState { ReplayView view = {}; bool on = false, begun = false; DevicePool mem; };

struct pedn_sim {
  DevView v{};
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int device = 0;
  int n_nodes = 0, n_turns = 0, n_demand = 0, n_od = 0, n_blocks = 0, n_ent = 0;
  // The static plan: which plan the engine steps under at all (pedn_plan.hpp: choose).  Assigned by pedn_create and by nothing else.
  pedn_plan::EnginePlan plan;
  int packed_by = 1;   // (from the model compiler, pedn_compile.hpp) how nodes were binned into node_kernel's blocks: 0 by degree, 1 by the static load estimate, 2 by measured cost
  // A caller that looks at the state after EVERY step (a controller reading densities, an output handler) makes every pending link
  // update a launch of its own and every next step start from stand-alone turning fractions: three launches per step where the plain plan
  // has two.  pedn_step notices (touched: something settled the pending state since the last step) and steps such a caller under the
  // plain plan until two steps in a row go untouched (nine_intersections, step + two reads: 76.0 -> 71 us per step).
  int touched = 0, touch_streak = 0;
  int step_streak = 0;   // consecutive pedn_step(t), pedn_step(t + 1), ... calls with nothing looking at the state in between (see pedn_step)
  std::vector<int32_t> h_slot_trow;
  int forked = 0;      // stream2 holds work of a chain of pedn_rl_step / pedn_step that the engine's stream does not order yet (join_forked)
  // Device-resident step clock (DevView.clock; pedn_rl_clock_begin .. pedn_rl_clock_end): while `clocked`, env steps are enqueued with
  // constant arguments (pedn_rl_step_clocked) and the host does not know the step the device is at -- every other entry point that
  // steps, reads or changes state first ends the clocked section (clock_end: synchronises and takes the bookkeeping back).
  int32_t* d_clock = nullptr;
  bool clocked = false;
  int clock_t0 = 0;   // step the clock was set to by pedn_rl_clock_begin
  // The marks: what the host knows of the device's state between two launches.  Read by the step planner, advanced by its commits and
  // transitions alone (pedn_plan.hpp); marks.valid_hi is mirrored into v.valid_hi (mirror_marks).
  pedn_plan::StepState marks;
  uint32_t* d_quiet = nullptr;   // the quiet-corridor words of the full packing (plan.quiet)
  // Dead links (pedn_partition.hpp; plan.dead_capable): the host's side of the split plan of launch_split_step.
  //   dl_dirty  an input of the proof has changed (or nothing was computed yet): dl_refresh recomputes before the next split range
  //   (marks.dl_grow, marks.dl_off: whether a recomputed set may grow, whether the plan is off until the next full reset)
  bool dl_dirty = true;
  std::vector<char> dl_node;           // [nodes] 1: stepped by dead_link_kernel
  // what the earlier proofs since the last full reset took for sources and found reachable: pedestrians that entered under them are
  // still walking when a demand row is zeroed or a turn closed behind them, so both stay sources of every later proof (dl_refresh)
  std::vector<char> dl_src;            // [demand rows] h_demand_nz, OR-ed over those proofs
  std::vector<char> dl_reach;          // [links] REACH, OR-ed over those proofs
  std::vector<char> h_demand_nz;       // [demand rows] the row may hold something else than +0.0
  std::vector<char> h_tab_nz;          // [turns] a host-tabulated fraction that is not +-0.0 at some step (tabulate_pair_pod)
  std::vector<int32_t> h_pack_order;   // nodes in the order the bins were packed in (pedn_compile::Tables::pack_order; dl_refresh repacks in it)
  std::vector<int32_t> h_link_sep, h_link_tau_sw, h_link_rev, h_node_kind, h_slot_in, h_slot_out;
  int n_dead_links = 0, n_dead_pos = 0, n_live_blocks = 0, live_npos = 0;
  size_t node_lds_live = 0;
  SlotRec* d_live_rec = nullptr;       // the live packing's slot records (capacity: the full packing's)
  SlotRec* d_dead_rec = nullptr;       // the records of the slots dead_link_kernel steps (copies, in work-list order): dead_prep_kernel's input
  DeadRec* d_dead_drec = nullptr;      // ... and what the lean waves read: their slot-uniform results (dead_prep_kernel, launched by dl_refresh)
  uint32_t* d_quiet_live = nullptr;
  hipStream_t stream3 = nullptr;       // the live bins' stream; null: not seen to overlap with the chains (no split)
  hipEvent_t ev_join3 = nullptr;
  // (The link update as a launch of its own runs one replica per lane -- link_kernel_1r: 42-47 VGPRs, 8 waves per SIMD; melbourne x 1024
  // 12.3-12.6 against 12.7-13.1 us with two replicas per lane, profiles/r03_link_kernel_variants.txt; inside link_turn_kernel, whose
  // budget is set by the turning fractions, it keeps two replicas per lane: half the workgroups.)
  int max_degree = 0;     // largest number of incident corridors of a node
  hipStream_t stream2 = nullptr;   // second half of the replicas in pedn_run (chains > 1)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int warmed_chains = 1;  // chains whose streams exist and were probed to overlap
  int chains = 1;         // plan of pedn_run for long ranges: 1 or 2 chains of launches (plan.chains, as far as the streams were seen to overlap; pedn_set_streams)
  int stream_probe_attempts = 0;   // warm_chain_streams: probes run until the chains' streams were seen to overlap
  float stream_probe_ms = 0.0f;
  std::vector<int32_t> node_turn_ptr, node_demand_row;
  std::vector<int32_t> h_up_od_ptr, h_upod_od, h_pair_upod;  // route-choice tables needed to re-tabulate P(od | up)
  std::vector<double> h_od_w;
  std::vector<int32_t> h_turn_pair_ptr, h_pair_const, h_turn_mode;
  double* d_pair_pod = nullptr;
  double* d_turn_tab = nullptr;
  RlView rl{};
  // rule-based controllers (pedn_ctrl_*, pedn_ctrl.hpp): device rows of next actions and episode sums, moving-average buffers
  CtrlState ctrl;
  bool rl_ready = false;
  bool rl_fold = false;   // gater-only agent set: pedn_rl_step lets node_kernel apply the actions (no launch of rl_apply_kernel)
  std::vector<SlotRec> h_slot_rec;
  SlotRec* d_slot_rec = nullptr;
  std::vector<double> h_front_u, h_back_u, h_tf_u;
  double *d_front_u = nullptr, *d_back_u = nullptr, *d_tf_u = nullptr;
  std::vector<int32_t> h_node_dyn, h_slot_dyn;  // per node: dynamic; per slot: SlotRec.dyn (0 static, 1 turn_frac_kernel, 2 tabulated)
  std::vector<int32_t> h_node_slot_ptr;
  std::vector<double> h_ttab, h_ttab_r;         // host copies of turn_tab [T+1][n_turns] / turn_tab_r [n_turns][R] (tabulated rows: final values)
  std::vector<char> h_rl_link;
  LinkPR* d_prm = nullptr;           // per-replica link parameters [L][RS] (pedn_set_link_params, pedn_randomize_scenarios)
  LinkPR* d_prm_draw = nullptr;      // recent-history mode: where pedn_randomize_scenarios draws before the result is accepted
  double *d_pair_pod_r = nullptr, *d_turn_tab_r = nullptr;
  // per-replica OD weights and the tables derived from them on the device (scenario_pod_tables)
  double *d_od_w_r = nullptr, *d_pod_tot = nullptr;     // [n_od][RS], [n_up][RS]
  const int32_t *d_up_od_ptr = nullptr, *d_upod_od = nullptr, *d_upod_up = nullptr, *d_pair_upod = nullptr, *d_turn_pair_ptr = nullptr,
                *d_turn_mode = nullptr, *d_tab_rows = nullptr;
  int n_tab_rows = 0, n_upod = 0;
  bool pod_tables_uploaded = false, ttab_r_stale = false;   // h_ttab_r is older than turn_tab_r on the device
  int* d_max_tau = nullptr;
  int n_pair = 0, n_up = 0, n_over = 0;
  int n_tf_heavy_quads = 0;  // leading workgroups of turn_frac_body with long chains (more than PEDN_TF_HEAVY_GROUPS softmax groups in a row)
  std::vector<long> h_tf_set_epoch;   // [nodes] marks.step_epoch when fractions were last imposed on the node
  int rows64[7], rows32[6];  // history rows of every field (T+1, or the size of its ring in recent-history mode)
  std::vector<void*> allocs;
  // host <-> device staging: two slots used in turn, each a pinned host buffer + a device buffer + the event recorded behind
  // the slot's last consumer, so that an upload neither waits for the stream nor borrows caller memory beyond the call
  struct Stage { void* pin = nullptr; void* dev = nullptr; size_t bytes = 0; hipEvent_t done = nullptr; };
  Stage stage[2];
  int stage_next = 0;
  void* rl_pin = nullptr;      // pinned landing buffer of the RL step's observations + rewards (rl_fetch)
  size_t rl_pin_bytes = 0;
  std::string err;
  struct MetricsState* metrics = nullptr;   // evaluation metrics (pedn_metrics.hpp)
  NormState norm;
  RolloutState ro;
  ReplayState rp;
};

// what the step planner reads of the handle (pedn_plan.hpp)
static inline pedn_plan::StepCaps step_caps(const pedn_sim* s) {
  pedn_plan::StepCaps c = pedn_plan::static_caps(s->plan);
  c.rl_ready = s->rl_ready; c.pr = s->v.pr != 0;
  c.trow = s->v.n_trow > 0; c.links = s->v.n_pairs_corr > 0; c.live = s->n_live_blocks > 0;
  c.T1 = s->v.T1;
  return c;
}
// DevView.valid_hi follows the marks: behind every commit or transition that may move marks.valid_hi
static inline void mirror_marks(pedn_sim* s) { s->v.valid_hi = s->marks.valid_hi; }

static int fail(pedn_sim* s, int code, const std::string& msg) {
  g_last_error = msg;
  if (s) s->err = msg;
  return code;
}

#define HIP_TRY(sim, expr)                                                                     \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return fail(sim, PEDN_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));      \
  } while (0)

template <typename T>
static int upload(pedn_sim* s, const T* src, size_t n, const T** dst) {
  void* p = nullptr;
  size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
  HIP_TRY(s, hipMalloc(&p, bytes));
  s->allocs.push_back(p);
  if (n) HIP_TRY(s, hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
  *dst = (const T*)p;
  return PEDN_OK;
}

template <typename T>
static int dalloc(pedn_sim* s, size_t n, T** dst) {
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T));
  if (e != hipSuccess) return fail(s, PEDN_E_NOMEM, std::string("hipMalloc of ") + std::to_string(n * sizeof(T)) + " bytes: " + hipGetErrorString(e));
  s->allocs.push_back(p);
  *dst = (T*)p;
  return PEDN_OK;
}

// A staging slot of at least `bytes` whose previous use has completed (the other slot may still be in flight).
#define PEDN_DIRECT_READ_BYTES 65536     // pedn_read_block: up to this size the gather kernel writes into the pinned buffer itself
#define PEDN_IN_PLACE_BYTES (4u << 20)   // host rows up to this size are read in place by their consuming kernel (stage_in_place; measured up to 256 KB)
static int stage_acquire(pedn_sim* s, size_t bytes, pedn_sim::Stage** out) {
  pedn_sim::Stage& st = s->stage[s->stage_next];
  s->stage_next ^= 1;
  if (!st.done) HIP_TRY(s, hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
  else HIP_TRY(s, hipEventSynchronize(st.done));
  if (bytes > st.bytes) {
    if (st.dev) HIP_TRY(s, hipFree(st.dev));
    if (st.pin) HIP_TRY(s, hipHostFree(st.pin));
    st.dev = st.pin = nullptr;
    st.bytes = 0;
    const size_t want = std::max<size_t>(bytes, 1 << 20);
    HIP_TRY(s, hipMalloc(&st.dev, want));
    HIP_TRY(s, hipHostMalloc(&st.pin, want, hipHostMallocDefault));
    st.bytes = want;
  }
  *out = &st;
  return PEDN_OK;
}

// host values -> the slot's device buffer (through its pinned buffer: the caller's memory is not touched after the return)
static int stage_upload(pedn_sim* s, pedn_sim::Stage* st, const void* src, size_t bytes, size_t offset = 0) {
  memcpy((char*)st->pin + offset, src, bytes);
  HIP_TRY(s, hipMemcpyAsync((char*)st->dev + offset, (char*)st->pin + offset, bytes, hipMemcpyHostToDevice, s->stream));
  return PEDN_OK;
}

// call after the last launch that reads or writes the slot
static int stage_commit(pedn_sim* s, pedn_sim::Stage* st) {
  HIP_TRY(s, hipEventRecord(st->done, s->stream));
  return PEDN_OK;
}

// Host rows that ONE kernel reads once (the action rows of a host-driven env step): copied into a pinned slot and read by the kernel IN
// PLACE over the bus -- no copy command in front of the launch (a DMA costs ~20 us of stream latency, a copy from pageable memory waits
// for the stream; the consuming wave's bus read costs it ~2 us).  The caller records the slot's event behind the consuming launch
// (stage_commit).  2048 envs: 93-96 -> 81 us per host-driven step, 48 -> 29 without a fetch.
static int stage_in_place(pedn_sim* s, const void* src, size_t bytes, pedn_sim::Stage** out) {
  int rc = stage_acquire(s, bytes, out);
  if (rc != PEDN_OK) return rc;
  memcpy((*out)->pin, src, bytes);
  return PEDN_OK;
}

// host bytes -> a device buffer of the engine; the caller's memory is borrowed for the call only, so the copy is waited for (rows beyond
// PEDN_IN_PLACE_BYTES; what was measured instead for smaller ones -- a copy COMMAND from a pinned slot, a copy KERNEL from it -- lost to
// reading them in place, profiles/r05_host_step_time.txt)
static int upload_through_stage(pedn_sim* s, void* dst, const void* src, size_t bytes) {
  HIP_TRY(s, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return PEDN_OK;
}

inline int DevicePool::take(pedn_sim* s, size_t bytes, void** out) {
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 16));
  if (e != hipSuccess) return fail(s, PEDN_E_NOMEM, std::string("hipMalloc of ") + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
  push_back(p);
  const hipError_t z = hipMemset(p, 0, std::max<size_t>(bytes, 16));
  if (z != hipSuccess) return fail(s, PEDN_E_DEVICE, std::string("hipMemset: ") + hipGetErrorString(z));
  *out = p;
  return PEDN_OK;
}
inline void DevicePool::drop() {
  for (void* p : *this) (void)hipFree(p);
  clear();
}

// a store (pedn_sim::ro / rp) goes: its arrays are freed, its view is zeroed (padding too: it is hashed as bytes), its flags are cleared
template <typename Store>
static void store_drop(Store& st) {
  st.mem.drop();
  st = Store();
  memset(&st.view, 0, sizeof st.view);
}

// the rows the fetches hand out: the normalised pair while the running normalisation is on, else (or raw) the raw one; rew right behind
// obs in both (pedn_rl_configure, pedn_rl_norm_configure)
struct FetchRows { float *obs, *rew; };
static inline FetchRows fetch_rows(const pedn_sim* s, bool raw = false) {
  if (s->norm.on && !raw) return {s->norm.view.obs_n, s->norm.view.rew_n};
  return {s->rl.obs, s->rl.rew};
}

// ... and they are the rows that a record launch of the rollout store and a push launch of the replay store copy
static void store_sources(pedn_sim* s) {
  const FetchRows f = fetch_rows(s);
  if (s->ro.on) { s->ro.view.obs_src = f.obs; s->ro.view.rew_src = f.rew; }
  if (s->rp.on) { s->rp.view.obs_src = f.obs; s->rp.view.rew_src = f.rew; }
}

// ---- core services, defined in pedn_hip.hip: what a subsystem's host section may call of the engine proper
static inline void join_forked(pedn_sim* s);           // ends a clocked section, joins the chains pedn_rl_step left forked
static inline void pending_links_first(pedn_sim* s);   // ... and performs a pending link update: in front of whatever reads or changes the state
static int clock_end(pedn_sim* s);
static int catch_up(pedn_sim* s, int upto);
static int rl_observe(pedn_sim* s, int32_t t, int32_t accumulate, float* obs, float* rewards, const CtrlView* cv, int norm = 0, int term = 0);
static int rl_step(pedn_sim* s, const double* actions, int32_t on_device, int32_t t, int32_t action_gap, float* obs, float* rewards,
                   const CtrlView* cv);
