/* pedn.h -- C-ABI of the MI355X engine for PedNStream's per-timestep network_loading hot path.
 *
 * The reference is pure Python and has no FFI; this header is the boundary a maintainer binds with ctypes
 * (see INTEGRATION.md).  Every entry point names the reference interface it replaces
 * (paths relative to the reference tree):
 *
 *   pedn_create                  Network.__init__ / init_nodes_and_links          src/LTM/network.py:56-121,194-248
 *                                Link.__init__ / Separator.__init__ state arrays   src/LTM/link.py:12-17,32-100,420-425
 *   pedn_step / pedn_run         Network.network_loading(t)                        src/LTM/network.py:266-287
 *                                (Node.assign_flows src/LTM/node.py:164-221, Link.cal_sending_flow src/LTM/link.py:216-370,
 *                                 Link.cal_receiving_flow[_with_reverse] :372-416, Network.update_link_states
 *                                 src/LTM/network.py:257-264, PathFinder.calculate_node_turning_fractions
 *                                 src/LTM/path_finder.py:717-737)
 *   pedn_set_demand              node.demand (origin arrays)                       src/LTM/network.py:130-139, node.py:176
 *   pedn_set_od_weights          ODManager.od_flows / get_od_flow                  src/LTM/od_manager.py:22-54
 *   pedn_set_turning_fractions   Network.update_turning_fractions_per_node         src/LTM/network.py:250-255
 *   pedn_get_turning_fractions   node.turning_fractions                            src/LTM/node.py:11
 *   pedn_set_width[s]            Link.front/back_gate_width, Separator.separator_width setters
 *                                                                                   src/LTM/link.py:110-126,462-478
 *   pedn_read                    the per-link history arrays read by callers       src/LTM/link.py:12-17,56,82-97
 *   pedn_error_flags             raise ValueError / Warning sites                  src/LTM/link.py:345-346,365-366; node.py:192-194,218-219,237-238
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success and a negative PEDN_E_* code on
 * failure, with a message retrievable through pedn_last_error().  Host pointers are borrowed for the duration of the
 * call.  All device work of one handle is enqueued on one HIP stream; pedn_step/pedn_run are asynchronous, the
 * read/flag calls synchronise.  Replicas are independent copies of the scenario stepped together; `replica` arguments
 * accept PEDN_ALL (-1) for "every replica".
 */
#ifndef PEDN_H
#define PEDN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PEDN_ABI_VERSION 4
#define PEDN_ALL (-1)
#define PEDN_MAX_DEGREE 8 /* incident corridor slots per node handled by the node kernel */

/* return codes */
#define PEDN_OK 0
#define PEDN_E_ARG (-1)     /* bad argument / inconsistent model description */
#define PEDN_E_DEVICE (-2)  /* HIP runtime error */
#define PEDN_E_MODEL (-3)   /* sticky per-replica model error, see pedn_error_flags */
#define PEDN_E_NOMEM (-4)

/* per-replica sticky error bits (pedn_error_flags) */
#define PEDN_F_NEG_SENDING 1u /* negative sending flow            (link.py:345-346,365-366 ValueError) */
#define PEDN_F_NEG_FLOW 2u    /* negative s / r / q at a node      (node.py:192-194,218-219,237-238 Warning) */
#define PEDN_F_INDEX 4u       /* history index outside [-(T+1), T] (IndexError in the reference) */
#define PEDN_F_NEG_BINOM 8u   /* binomial with n < 0               (numpy ValueError at link.py:382) */
#define PEDN_F_SAME_STEP 16u  /* look-back of 0 steps: the reference result depends on node iteration order */
#define PEDN_F_LP 32u         /* node LP (assign_flows_type 'optimal') did not terminate: `res.success` false, node.py:267 */
/* (bit 64u is reserved: it belonged to the persistent plan of ABI 3, removed as a measured negative) */

/* RNG modes (oracle/rng_contract.py) */
#define PEDN_RNG_PHILOX 0
#define PEDN_RNG_MEANFIELD 1 /* binomial -> floor(n*p), normal -> 0 */

#define PEDN_NODE_CLASSIC 0
#define PEDN_NODE_OPTIMAL 1
#define PEDN_LP_PENALTY 1e-2 /* Node.w, node.py:14 */
#define PEDN_HIST_FULL 0
#define PEDN_HIST_RECENT 1

/* width selectors */
#define PEDN_W_FRONT 0
#define PEDN_W_BACK 1
#define PEDN_W_SEP 2
/* 0/1 per (separator link, replica): the separator width is held as a numpy float64 scalar in the reference (it is after
 * ActionApplier's np.clip, rl/builders.py:295), which makes `num_pedestrians / area` (link.py:136) a binary64 division
 * rounded to float32 instead of a float32 division.  pedn_rl_apply_actions sets it; the plain setters clear it. */
#define PEDN_W_SEP_NUMPY 3

/* history fields; f64 fields 0..6 have n_links + n_vlinks columns for ids 0..3 (virtual links keep only those) */
enum {
  PEDN_FIELD_INFLOW = 0,
  PEDN_FIELD_OUTFLOW = 1,
  PEDN_FIELD_CUM_INFLOW = 2,
  PEDN_FIELD_CUM_OUTFLOW = 3,
  PEDN_FIELD_SENDING = 4,
  PEDN_FIELD_RECEIVING = 5,
  PEDN_FIELD_GATE_REC = 6, /* back_gate_width_data (separator_width_data for separators) */
  PEDN_FIELD_TRAVEL_TIME = 7,
  PEDN_FIELD_AVG_TRAVEL_TIME = 8,
  PEDN_FIELD_NUM_PED = 9,
  PEDN_FIELD_DENSITY = 10,
  PEDN_FIELD_SPEED = 11,
  PEDN_FIELD_LINK_FLOW = 12,
  PEDN_N_FIELDS = 13
};

/* Static, replica-independent description of one scenario (built by pednstream_amd/flatten.py).
 * Node n owns slots node_slot_ptr[n] .. node_slot_ptr[n+1]-1; slot k of a node holds the incoming link
 * slot_in_link[] and the outgoing link slot_out_link[] towards the same neighbour (reverse pair); a link index
 * >= n_links denotes a virtual link (origin/destination side, always slot 0 of its node).
 * Turning fractions of node n are node_turn_ptr[n] .. +m(m-1), source-major, destinations ascending skipping the
 * source's own slot (node.py:274-280). */
typedef struct pedn_model_desc {
  int32_t abi_version;
  int32_t n_nodes, n_links, n_vlinks, n_turns, n_demand, n_od;
  int32_t T;      /* simulation_steps; histories have T+1 entries */
  int32_t window; /* moving-average window W = round(100/dt)  (link.py:89) */
  double dt;      /* unit_time */

  const int32_t* node_kind;       /* [n_nodes] 0 one-to-one, 1 regular                 (network.py:141-167) */
  const int32_t* node_slot_ptr;   /* [n_nodes+1] */
  const int32_t* node_turn_ptr;   /* [n_nodes+1] */
  const int32_t* node_demand_row; /* [n_nodes] row of `demand`, or -1 */
  const int32_t* node_dyn;        /* [n_nodes] 1: turning fractions recomputed every step (path_finder.py:731-737) */
  const int32_t* slot_in_link;    /* [n_slots] */
  const int32_t* slot_out_link;   /* [n_slots] */

  const int32_t* link_rev;    /* [n_links] reverse link */
  const int32_t* link_sep;    /* [n_links] 1: Separator */
  const int32_t* link_fd;     /* [n_links] 0 yperman, 1 greenshields, 2 smulders */
  const int32_t* link_tau_sw; /* [n_links] round(length/(shockwave_speed*dt))  (link.py:380) */
  const int32_t* link_fft;    /* [n_links] free_flow_tau                        (link.py:86) */
  const float* link_tt0;      /* [n_links] travel_time[0]                       (link.py:83) */
  const double *link_length, *link_width, *link_vf, *link_kc, *link_kj, *link_gamma, *link_act, *link_bi, *link_noise;
  const double *front_gate0, *back_gate0, *sep_width0; /* [n_links] initial widths */

  const double* tf_init; /* [n_turns] */
  const double* demand;  /* [n_demand][T+1] */
  const double* od_w;    /* [n_od][T+1] */

  /* route-choice tables (all index ranges are global, CSR per node) */
  double pf_temp, pf_alpha, pf_beta, pf_omega, pf_eps;
  int32_t n_up, n_upod, n_grp, n_ent, n_pair;
  const int32_t* node_up_ptr;   /* [n_nodes+1] -> upstream groups of the node              (up_od_probs, :599-615) */
  const int32_t* up_slot;       /* [n_up]      incoming slot (local index) the upstream group belongs to */
  const int32_t* up_od_ptr;     /* [n_up+1]    -> upod entries of one upstream */
  const int32_t* upod_od;       /* [n_upod]    OD row in od_w */
  const int32_t* node_grp_ptr;  /* [n_nodes+1] -> (od, up) softmax groups of the node       (turns_distances, :563) */
  const int32_t* grp_ent_ptr;   /* [n_grp+1]   -> downstream entries of one group */
  const int32_t* grp_allphys;   /* [n_grp]     1: every downstream is a physical link (f32 density branch, :581) */
  const int32_t* grp_node;      /* [n_grp]     node index the group belongs to */
  const int32_t* ent_link;      /* [n_ent]     outgoing link of the entry, -1 = virtual     (:577-579) */
  const double* ent_dist;       /* [n_ent]     remaining distance */
  const int32_t* turn_pair_ptr; /* [n_turns+1] -> (entry, upod) products summed into one turning fraction (:668-686) */
  const int32_t* pair_ent;      /* [n_pair] */
  const int32_t* pair_upod;     /* [n_pair] */

  /* PEDN_HIST_FULL: all 13 arrays keep their T+1 entries like the reference's (80 B per link, time index and replica).
   * PEDN_HIST_RECENT: only what the recurrence itself looks far back into is kept whole -- inflow and cumulative_inflow
   * (link.py:199-214,284-288: data-dependent look-back); cumulative_outflow keeps max(tau_shockwave) + 2 entries, travel_time
   * the moving-average window + 2, everything else the last 4.  Same numbers step for step (the batched RL environment
   * reads nothing older); pedn_read of an entry that has left its ring fails, and so does one of an entry not written yet whose
   * ring slot still holds an older one (sending_flow / receiving_flow of step t are entries t-1, node.py:206, link.py:367: after
   * step t their newest entry is t-1).  16 B + a few rows instead of 80 B. */
  int32_t history_mode;

  /* PEDN_NODE_CLASSIC: RegularNode.solve('classic') (node.py:272-300).  PEDN_NODE_OPTIMAL: assign_flows_type 'optimal', the
   * linear programme of node.py:249-271 (maximise the total flow minus 0.01 x the deviation from the turning fractions under
   * the sending / receiving constraints) solved per (node, replica) by a dense primal simplex with Bland's rule.  The
   * reference hands the same programme to scipy/HiGHS; the optimum is degenerate, so the two agree in the objective value,
   * not necessarily in the vertex: parity for this mode is objective-level only (unpinned). */
  int32_t node_model;

  /* [n_nodes] or NULL: measured cost of every node's slowest slot wave (any unit; ticks from kernel entry to the node kernel's first
   * block barrier, tools/pack_calibrate.py -> <scenario>/pack_cost.json).  Nodes are binned into the node kernel's blocks of eight
   * waves; a block lasts as long as its slowest wave, so nodes of similar cost should share a block.  Without it the bins are packed
   * by a static estimate (the number of (turn, od) products of a node). */
  const float* node_cost;
} pedn_model_desc;

typedef struct pedn_sim pedn_sim;

int pedn_abi_version(void);
/* message of the last failing call on this thread (handle may be NULL for pedn_create failures) */
const char* pedn_last_error(const pedn_sim* sim);

int pedn_create(const pedn_model_desc* model, int32_t n_replicas, int32_t replica_offset, uint64_t seed,
                int32_t rng_mode, int32_t device, pedn_sim** out);
int pedn_destroy(pedn_sim* sim);

/* values[n] -> demand[node][0..n-1] (rest zero); node is the model's node index, replica may be PEDN_ALL */
int pedn_set_demand(pedn_sim* sim, int32_t node, int32_t replica, const double* values, int32_t n);
/* demand[node][0..n-1] of one replica back to the host (what pedn_set_demand* / pedn_draw_demand left on the device) */
int pedn_get_demand(pedn_sim* sim, int32_t node, int32_t replica, double* values, int32_t n);
/* the same for every replica in one call: values[r * n + i] = demand of replica r at time index i (n <= T+1, rest zero) */
int pedn_set_demand_matrix(pedn_sim* sim, int32_t node, const double* values, int32_t n);
/* the same for a subset: values[k * n + i] = demand of replica replicas[k] at time index i, k < n_rep; one upload */
int pedn_set_demand_rows(pedn_sim* sim, int32_t node, const int32_t* replicas, int32_t n_rep, const double* values, int32_t n);
/* values[T+1] -> OD weight row `od` (shared by all replicas) */
int pedn_set_od_weights(pedn_sim* sim, int32_t od, const double* values, int32_t n);
int pedn_set_turning_fractions(pedn_sim* sim, int32_t node, int32_t replica, const double* tf, int32_t n);
int pedn_get_turning_fractions(pedn_sim* sim, int32_t node, int32_t replica, double* tf, int32_t n);
int pedn_set_width(pedn_sim* sim, int32_t which, int32_t link, int32_t replica, double value);
/* values[n_links][n_replicas] */
int pedn_set_widths(pedn_sim* sim, int32_t which, const double* values);
/* every replica back to the same widths (an episode reset): front[n_links], back[n_links], sep[n_links] broadcast, the
 * "separator width is an np.float64" marks (PEDN_W_SEP_NUMPY) cleared */
int pedn_reset_widths(pedn_sim* sim, const double* front, const double* back, const double* sep);
/* current widths -> values[n_links][n_replicas] (the device may have changed them through pedn_rl_apply_actions) */
int pedn_get_widths(pedn_sim* sim, int32_t which, double* values);

/* one step t in 1..T for every replica; asynchronous.  (The reference's loops run t = 1 .. T-1, network.py:266-287 callers; its
 * arrays have T+1 entries like these, so t = T is a valid step -- the batched RL env takes it.  Behind step T no turning fractions
 * of T+1 are prepared: the per-step tables end at T.) */
int pedn_step(pedn_sim* sim, int32_t t);
/* steps t0 .. t1-1 enqueued back to back, t1 <= T+1; asynchronous.  Same results as t1 - t0 calls of pedn_step, under the launch
 * plan the engine picked for the model (pedn_plan_info): for a model without device-computed turning fractions the slot waves of
 * step t + 1's node kernel perform Network.update_link_states(t) (network.py:257-264) themselves -- ONE launch per step; small batches
 * of models with short dynamic rows step the same way, the slot waves computing their own rows of turning fractions too.  The link
 * update of the last step launched stays pending until the next step or the first call that looks at or changes the state. */
int pedn_run(pedn_sim* sim, int32_t t0, int32_t t1);
int pedn_synchronize(pedn_sim* sim);
/* synchronises; flags[n_replicas] may be NULL; returns the OR over replicas (>= 0) or a negative code */
int pedn_error_flags(pedn_sim* sim, uint32_t* flags);

/* out[(t1-t0)][(link1-link0)][(rep1-rep0)] of the field's element type (f64 for ids 0..6, f32 otherwise) */
int pedn_read(pedn_sim* sim, int32_t field, int32_t t0, int32_t t1, int32_t link0, int32_t link1, int32_t rep0,
              int32_t rep1, void* out);

/* number of time indices field `field` keeps: T+1, or the size of its ring in PEDN_HIST_RECENT mode (time index t lives in
 * row t mod that size) */
int pedn_history_rows(pedn_sim* sim, int32_t field);

/* ---- evaluation metrics of every replica (rl/rl_utils.py:770-1512 of the reference, on what save_network_state would write) ----------
 * Every history is read over its T+1 rows; rows no step has written read as zero (the hi rule of pedn_read).  The f32 fields
 * travel_time, num_pedestrians and density are widened to f64 before any arithmetic; k_critical, k_jam and free_flow_speed are
 * per replica, length and width the static ones.  Sums over (link, time) are per-link serial partial sums folded in link order:
 * within rounding of the reference's single serial sum, bit-identical from run to run and for any split into windows.
 *   pedn_metrics_begin        static set-up, accumulators zeroed.  link_flags[n_links]: bit 0 the link starts at an origin node,
 *                             bit 1 it ends at a destination node, bit 2 it lies on some od path (all links when there is no path
 *                             finder).  origin_rows / origin_len [n_origins]: demand row (-1 none) and the number of demand values of
 *                             each origin node in the order of origin_nodes.  agent_ptr[n_agents + 1] / agent_links: the links of each
 *                             agent (gater: real incoming, then real outgoing links; separator: forward, reverse).
 *   pedn_metrics_accumulate   folds rows t0 <= t < t1 into the accumulators.  Windows must increase and must not overlap; rows that
 *                             no window covers read as zero.  PEDN_E_ARG with pedn_read's message when a row has left a field's ring.
 *   pedn_metrics_read         out[n_replicas][PEDN_N_METRICS] (indices below), agent_links[n_replicas][len(agent_links)][2] = per-link
 *                             mean density and mean density / k_jam (NaN: no valid row), agents[n_replicas][n_agents][3] = mean of
 *                             those over the agent's links and their number.  Either agent array may be NULL. */
enum {
  PEDN_M_THROUGHPUT = 0, PEDN_M_COMPLETED_DEMAND, PEDN_M_TOTAL_DEMAND,
  PEDN_M_AVG_TRAVEL_TIME, PEDN_M_TT_NUM_LINKS,
  PEDN_M_TOTAL_DELAY, PEDN_M_DELAY_INTENSITY, PEDN_M_DELAY_PERSON_TIME, PEDN_M_DELAY_NUM_LINKS,
  PEDN_M_AVG_TIME_SPENT, PEDN_M_PERSON_TIME, PEDN_M_TOTAL_TRIPS, PEDN_M_NUM_ORIGIN_LINKS,
  PEDN_M_SERVED_RATE, PEDN_M_TOTAL_INFLOW, PEDN_M_TOTAL_OUTFLOW, PEDN_M_NUM_DEST_LINKS,
  PEDN_M_CONGESTION_TIME, PEDN_M_AVG_CONGESTION_DENSITY, PEDN_M_CONGESTION_FRACTION, PEDN_M_TOTAL_AREA_TIME,
  PEDN_M_CONGESTED_ROWS, PEDN_M_COUNTED_ROWS,
  PEDN_N_METRICS
};
int pedn_metrics_begin(pedn_sim* sim, const int32_t* link_flags, const int32_t* origin_rows, const int32_t* origin_len, int32_t n_origins,
                       const int32_t* agent_ptr, const int32_t* agent_links, int32_t n_agents, double unit_time);
int pedn_metrics_accumulate(pedn_sim* sim, int32_t t0, int32_t t1);
int pedn_metrics_read(pedn_sim* sim, double* out, double* agent_links, double* agents);

/* Everything the engine still owes the histories is enqueued on pedn_stream(): a link update left pending by the last pedn_step /
 * pedn_run (the next step's node kernel would have performed it), chains that are still forked, the rows a lazy reset declared
 * unwritten (cleared now).  Asynchronous.  After it, work ordered behind pedn_stream() sees every row of every field complete. */
int pedn_flush(pedn_sim* sim);
/* zero-copy access for on-device consumers: HBM base pointer of a history field laid out
 * [pedn_history_rows][columns][replica_stride]; columns/replica_stride may be NULL.  The call itself performs pedn_flush, so the
 * view is complete for a consumer that orders itself behind pedn_stream() NOW.  The pointer stays valid for the handle's life, but
 * what it shows is complete only up to the last pedn_flush / pedn_device_ptr / pedn_synchronize: after a later pedn_step / pedn_run
 * (last step's density / speed / travel time / num_pedestrians rows pending) or pedn_reset_lazy (rows above the current step hold the
 * previous episode) a consumer that kept the pointer calls pedn_flush before it orders itself behind the stream again. */
void* pedn_device_ptr(pedn_sim* sim, int32_t field, int64_t* columns, int64_t* replica_stride);
/* hipStream_t the engine launches on (a pure getter: it enqueues nothing -- see pedn_flush) */
void* pedn_stream(pedn_sim* sim);

/* HIP-event timing on the engine's stream: begin records an event, end records + synchronises and returns the
 * elapsed milliseconds in *ms */
int pedn_timer_begin(pedn_sim* sim);
int pedn_timer_end(pedn_sim* sim, float* ms);

/* One step with every kernel bracketed by HIP events on the engine's stream (synchronises).  ms[0] = turning-probability
 * kernel, ms[1] = node kernel, ms[2] = link kernel (0 when a kernel is not launched for this scenario). */
int pedn_profile_step(pedn_sim* sim, int32_t t, float ms[3]);

/* Steps t0 <= t < t1 under the launch plan pedn_run uses for such a range, every launch bracketed by its own dispatch
 * timestamps (synchronises).  ms[0..2] = mean duration of a launch of {stand-alone turning fractions, node kernel, the launch
 * behind it (link update and / or turning fractions of t + 1)}; *chains = 1 or 2: how many chains of launches ran side by
 * side (2: the two halves of the replicas on two streams -- a launch then covers n_replicas / 2 and overlaps the other
 * chain's launches, so per-launch bandwidths of the two chains add up). */
int pedn_profile_run(pedn_sim* sim, int32_t t0, int32_t t1, float ms[3], int32_t* chains);
/* The same range, not averaged: out[5 * row + {0..4}] = {step, chain (0 / 1), kind (0 stand-alone turning fractions, 1 node kernel,
 * 2 the launch behind it), start, end} with start / end in milliseconds after the start of the range's first launch; at most
 * `capacity` rows (3 per step and chain), *n_rows of them written.  Shows how the launches of the two chains overlap. */
int pedn_profile_timeline(pedn_sim* sim, int32_t t0, int32_t t1, float* out, int32_t capacity, int32_t* n_rows, int32_t* chains);

/* launch plan of pedn_run for long ranges: 1 = one chain of launches on the engine's stream, 2 = the halves of the replicas as two
 * chains on two streams (the default from 640 replicas -- the halves are whole 128-replica segments, 640 = 384 + 256; replicas are independent, results are the same).  The two streams are probed
 * to run side by side (pedn_plan_info); when the runtime cannot provide two independent queues the plan falls back to one chain. */
int pedn_set_streams(pedn_sim* sim, int32_t n);
/* The launch plan of pedn_run: info[0] = chains (1 | 2), info[1] = 1 when the link update is performed by the next step's node kernel
 * (one launch per step), info[2] = streams created until one was found that overlaps with the engine's stream (0: not probed yet;
 * the runtime may map two streams onto one hardware queue, which would serialise the chains), info[3] = duration in microseconds of
 * the probe's two concurrent 300 us kernels on the pair kept (~300: they overlap, ~600: they do not); n = entries of info (>= 4);
 * with n >= 5: info[4] = how nodes were packed into the node kernel's workgroups: 0 by degree, 1 by the static load estimate, 2 by
 * the measured cost pedn_model_desc.node_cost; with n >= 6: info[5] = 1 when those one-launch steps skip the loads of corridors that were
 * empty in all 64 replicas of a group at the step before (quiet corridors, PEDN_QUIET=0|1; results are the same either way); with
 * n >= 7: info[6] = 1 when the node kernels skip the stores of +0.0 into rows of inflow / outflow / cumulative_inflow /
 * cumulative_outflow / num_pedestrians / density / link_flow that have held +0.0 since the last pedn_reset (zero elision, PEDN_ZERO_ELIDE=0|1,
 * full-record mode only; results are the same either way; pedn_device_ptr on one of those fields, and the clocked steps, turn it
 * off until the next pedn_reset); with n >= 8: info[7] = node-kernel launches that could skip such stores since the last reset of
 * either kind; with n >= 9: info[8] = 1 when the quiet-corridor launches of info[5] also skip the column pass / row sums of a node
 * slot whose flows are +0.0 in all 64 replicas of a group (PEDN_QUIET_LEAN=0|1, default on; results are the same either way); with
 * n >= 10: info[9] = the links that a two-chain range of pedn_run steps in the lean dead-link kernel because no pedestrian can ever
 * reach them -- proven on the host from the demand rows, turning fractions and gates -- while the node kernel runs over the other
 * nodes only, on a third stream (PEDN_DEAD_LINKS=0|1, default on; results are the same either way); 0 when that plan is off; with
 * n >= 11: info[10] = the steps launched under that plan since the last reset of either kind. */
int pedn_plan_info(pedn_sim* sim, int32_t* info, int32_t n);

/* reset all histories and dynamic state to t = 0 (widths, turning fractions and demand are kept) */
int pedn_reset(pedn_sim* sim);
/* The same for a caller that resets every episode (rl/pz_pednet_env.py:143-193 rebuilds the Network instead): in full-record mode only
 * what a new episode reads before it writes is restored -- row 0 of every field, avg_travel_time below the moving-average window
 * (link.py:91), the gate record (link.py:56) -- and every other row counts as unwritten until its step runs: pedn_read answers such
 * rows with the field's initial value (what the reference's fresh arrays hold), the kernels do the same for the only reads that can
 * land there (get_outflow's negative indices, link.py:205-212), an out-of-order step or observation clears the rows it skips first,
 * and pedn_device_ptr clears the rest, because a zero-copy consumer may look anywhere.  Recent-history mode: the same as pedn_reset. */
int pedn_reset_lazy(pedn_sim* sim);

/* ---- per-replica scenarios on one topology (reference: NetworkEnvGenerator.create_network with
 * link_params_overrides / od_flows / demand_params_overrides, src/utils/env_loader.py:81-158, as produced by
 * generate_random_link_params :363-424, generate_random_od_flows :224-259, generate_random_demand_params :183-222).
 * Demand per replica is pedn_set_demand(node, replica, ...).  Call pedn_reset afterwards: travel_time[0] depends on them. */
/* matrices [n_links][n_replicas]: k_critical, k_jam, free_flow_speed and the host-derived free_flow_tau (link.py:86),
 * shock-wave look-back (link.py:380) and travel_time[0] (link.py:83).  kc == NULL returns to the shared parameters. */
int pedn_set_link_params(pedn_sim* sim, const double* kc, const double* kj, const double* vf, const int32_t* free_flow_tau,
                         const int32_t* tau_sw, const float* tt0);
/* the per-replica link parameters back to the host, matrices [n_links][n_replicas]; any pointer may be NULL */
int pedn_get_link_params(pedn_sim* sim, double* kc, double* kj, double* vf, int32_t* free_flow_tau, int32_t* tau_sw, float* tt0);
/* w[n_od][n_replicas]: time-constant OD weights per replica (the randomiser's np.full(T+1, weight)); NULL returns to the
 * shared, time-varying weights of pedn_set_od_weights */
int pedn_set_od_weights_per_replica(pedn_sim* sim, const double* w);
int pedn_get_od_weights_per_replica(pedn_sim* sim, double* w);
/* A new scenario for EVERY replica drawn on the device, in place -- what NetworkEnvGenerator.randomize_network draws per env
 * (src/utils/env_loader.py:160-181) without the host: `what` bit 0 link parameters (generate_random_link_params :363-424: exactly
 * int(corridors * link_fraction) corridors per replica without replacement; with probability 1/2 k_critical and k_jam x U(0.6, 1.2)
 * with the floors max(0.5, .) / max(2 k_c, .); with probability 1/2 free_flow_speed x U(0.6, 0.9); look-backs and travel_time[0]
 * re-derived, link.py:58-63,83-86,380), bit 1 OD weights (generate_random_od_flows :224-259: U(1, 10) per OD pair, constant over
 * the episode), bit 2 origin demand (generate_random_demand_params :183-222 + the series of od_manager.py:92-155 as pedn_draw_demand)
 * for the n_origins nodes listed.  Philox4x32-10 keyed by (seed, global replica id): a function of the seed, independent of how the
 * ensemble is sharded; the same distributions as the reference's randomisers, NOT numpy's stream: pinned bit for bit by
 * the CPU restatement oracle/rand_contract.py and distribution-tested against the numpy generator it replaces.
 * Asynchronous; call pedn_reset afterwards. */
int pedn_randomize_scenarios(pedn_sim* sim, uint64_t seed, double link_fraction, int32_t what, const int32_t* origin_nodes,
                             int32_t n_origins);

/* ---- batched RL environment step around the hot path ------------------------------------------------
 * Replaces, for every replica at once, the per-env Python glue of the reference's PettingZoo wrapper:
 *   pedn_rl_apply_actions   ActionApplier.apply_all_actions / clip_*_action_value     rl/builders.py:264-352
 *   pedn_rl_observe         ObservationBuilder.build_observation                       rl/builders.py:68-177 (+ :179-238 normalisation)
 *                           PedNetParallelEnv._compute_rewards                          rl/pz_pednet_env.py:548-581
 * Agents are listed in the reference's order (separators, then gaters; rl/discovery.py:121-123).  An action row holds,
 * agent after agent, one width per separator and one width per outgoing link of a gater; an observation row holds 4
 * features per separator and features_per_link x outdegree per gater (no padding, discovery.py:176-178). */
typedef struct pedn_rl_desc {
  int32_t n_agents;
  const int32_t* agent_type;     /* [n_agents] 0 separator, 1 gater */
  const int32_t* agent_link_ptr; /* [n_agents+1] */
  const int32_t* agent_links;    /* gater: controlled outgoing links; separator: forward link, reverse link */
  int32_t obs_mode;              /* 1..5 = "option1".."option5" (builders.py:47-58) */
  int32_t normalize;             /* builders.py:179-238 */
  int32_t reward_mode;           /* 0: as the reference runs (its `return` sits inside the agent loop, pz_pednet_env.py:581,
                                       so only the first agent is ever rewarded); 1: every gater agent */
  double max_delta_sep, max_delta_gate, min_sep; /* pz_pednet_env.py:84-86 */
} pedn_rl_desc;

/* validates the description and allocates the device buffers; returns the row lengths */
int pedn_rl_configure(pedn_sim* sim, const pedn_rl_desc* desc, int32_t* n_actions, int32_t* n_obs);
/* actions[n_replicas][n_actions] (binary64, widths in metres); on_device != 0: `actions` is a device pointer.  A NaN entry
 * means "no action for this slot": the widths it controls stay exactly as they are (apply_all_actions only touches the agents
 * it is given, rl/builders.py:343-352) */
int pedn_rl_apply_actions(pedn_sim* sim, const double* actions, int32_t on_device);
/* observations and rewards of step t (after pedn_step(t)) into the device buffers; accumulate != 0 adds the rewards to
 * the buffer (float32, like the reference's cumulative_rewards) instead of overwriting.  obs / rewards may be NULL;
 * otherwise they receive host copies [n_replicas][n_obs] / [n_replicas][n_agents] (synchronises). */
int pedn_rl_observe(pedn_sim* sim, int32_t t, int32_t accumulate, float* obs, float* rewards);
/* The observation / reward buffers as the last pedn_rl_step / pedn_rl_observe left them -> host (either pointer may be NULL); waits
 * for the engine's work.  For callers that step SEVERAL engines before they look at any of them: pedn_rl_step(..., NULL, NULL) on every
 * engine, then one fetch each -- the engines' launches overlap instead of alternating with host waits (MultiScenarioVecEnv: one engine
 * per randomised topology, rl/pz_pednet_env.py:143-193 rebuilds the network per reset). */
int pedn_rl_fetch(pedn_sim* sim, float* obs, float* rewards);
/* pedn_rl_step(.., NULL, NULL) on every engine of sims[0 .. n), then pedn_rl_fetch of each, in ONE call: the engines' launches overlap and
 * the per-engine cost of a host-side loop over handles is gone (MultiScenarioVecEnv: 32 engines x 64 envs).  actions / obs / rewards are the
 * engines' rows one after the other (engine k: its n_replicas rows); all engines step the same t with the same agent layout. */
int pedn_rl_step_many(pedn_sim** sims, int32_t n, const double* actions, int32_t t, int32_t action_gap, float* obs, float* rewards);
/* apply -> action_gap x (pedn_step(t+k), observe) in one call (pz_pednet_env.py:195-254).  obs / rewards NULL: asynchronous, the
 * results stay in the device buffers (pedn_rl_device_ptr), complete after pedn_synchronize.  With on_device actions and nothing
 * fetched, large batches step as two chains on two streams that stay forked across calls (the halves of the envs are independent);
 * every call that needs the whole batch joins them first, so callers see the same ordering as on one stream.  on_device = 2: device
 * actions as with 1, and every launch of the call goes to pedn_stream() -- for a caller that orders the call between its own streams
 * and the engine's with events instead of host synchronisation (VecPedNetEnv.step_device(sync=False)). */
int pedn_rl_step(pedn_sim* sim, const double* actions, int32_t on_device, int32_t t, int32_t action_gap, float* obs,
                 float* rewards);
/* ---- env steps with CONSTANT launch arguments: a captured graph of (policy -> env step -> reward bookkeeping) can be replayed ------
 * (rl/pz_pednet_env.py:195-254 is called once per policy step, rl/train_ppo_sb3.py:246 wraps one env; here the step index lives in
 * device memory, so the launches of a step do not change from step to step.)
 *   pedn_rl_clock_begin(t)    everything pending is settled on pedn_stream(), the device clock is set to step t.  The turning fractions
 *                             of step t must be in place already (they are after pedn_rl_step(t - 1)): the first step of an episode
 *                             runs through pedn_rl_step, whose stand-alone fractions read the gate widths behind that step's actions.
 *   pedn_rl_step_clocked      ONE env step (apply -> action_gap x (network_loading, observe)) enqueued on `stream` (a hipStream_t; NULL =
 *                             pedn_stream()) without touching the host's bookkeeping: no allocation, no synchronisation, no event query --
 *                             safe under stream capture.  `actions` is a device pointer [n_replicas][n_actions] (or NULL) read when
 *                             the launch RUNS: a replayed graph reads whatever the buffer holds then.  The step's last launch advances
 *                             the clock; a step enqueued beyond the horizon T does nothing.  Observations / rewards: pedn_rl_device_ptr.
 *                             The caller orders `stream` behind pedn_stream() once after pedn_rl_clock_begin.
 *   pedn_rl_clock_end(&t)     synchronises the DEVICE, reads the clock back (t = the next step to run) and restores the host's
 *                             bookkeeping; every other entry point that steps, reads or changes the state does this implicitly first. */
int pedn_rl_clock_begin(pedn_sim* sim, int32_t t);
int pedn_rl_step_clocked(pedn_sim* sim, const double* actions, int32_t action_gap, void* stream);
int pedn_rl_clock_end(pedn_sim* sim, int32_t* t);
/* 1 while a clocked section is open (pedn_rl_clock_begin .. the next call that ends it), else 0: a caller that replays a captured
 * graph checks this before every replay -- another entry point may have ended the section -- and begins it again if need be */
int pedn_rl_clocked(pedn_sim* sim);
/* A hash of everything the launches of pedn_rl_step_clocked carry by value (device pointers, sizes, whether replicas have their own
 * scenarios, the agent set) and of what selects their kernels and grids.  A captured graph is valid as long as this value is the one
 * it was captured under: e.g. the first reset(options={'randomize': True}) switches the step to the per-replica-parameter kernels. */
uint64_t pedn_rl_clock_signature(pedn_sim* sim);
/* device buffers for zero-copy consumers: 0 actions (f64 [R][n_actions]), 1 observations (f32 [R][n_obs]), 2 rewards (f32 [R][n_agents]) */
void* pedn_rl_device_ptr(pedn_sim* sim, int32_t which);

/* ---- running observation / reward normalisation on the device (rl/rl_utils.py:57-300: RunningMeanStd, RunningNormalizeWrapper) -----
 * Off by default.  While on, ONE more launch follows whichever launch wrote the observation and reward buffers -- in pedn_rl_observe,
 * pedn_rl_step (host and device actions) and pedn_rl_step_clocked (on the caller's stream, constant arguments: it is captured with the
 * step) -- and writes normalised rows into two buffers of their own; the raw buffers stay as they are.  The contract (DESIGN section 11,
 * restated in numpy by tests/norm_model.py): binary64 statistics that live on the device and survive pedn_reset; per tracked observation
 * column the batch mean and variance over the env axis, summed in one fixed order that depends on n_envs alone (pedn_norm.hpp), merged
 * with the operation order of RunningMeanStd._update_from_moments; out = f32(clip((x - mean) / sqrt(var + 1e-8), +-clip_obs)) with the
 * statistics AFTER the update; untracked columns are copied.  Rewards: ret[e][a] = r + gamma * ret[e][a] * (1 - terminated), agent after
 * agent merged into one scalar triple, out = f32(clip(r / sqrt(ret_var + 1e-8), +-clip_reward)); pedn_reset zeroes ret.  With one env
 * this is the reference wrapper bit for bit.
 *   pedn_rl_norm_configure   tracked_mask [n_obs]: 1 = normalise the column, 0 = copy it (the gate width of every link of a gater);
 *                            agent_of_column [n_obs]: the agent a column belongs to (the per-agent count of get/set_stats).  Switches
 *                            the normalisation on with fresh statistics (mean 0, var 1, count 1e-4), training on; norm_obs = norm_reward
 *                            = 0 switches it off (the two arrays may then be NULL).  Refused together with pedn_ctrl_configure;
 *                            pedn_rl_step_many refuses engines that normalise.  pedn_rl_configure switches it off.
 *   pedn_rl_norm_set_training  0: the statistics are frozen (rows are still normalised, returns still discounted)
 *   pedn_rl_norm_get_stats / pedn_rl_norm_set_stats   mean [n_obs], var [n_obs] (entries of untracked columns are not used), count
 *                            [n_agents], ret_stats [3] = mean, var, count of the returns; NULL skips an array
 *   pedn_rl_norm_device_ptr  0 normalised observations (f32 [R][n_obs]), 1 normalised rewards (f32 [R][n_agents]), 2 / 3 / 4 mean / var /
 *                            count per column (f64 [n_obs]), 5 returns (f64 [R][n_agents]), 6 ret_stats (f64 [3]); NULL while off
 * While on, pedn_rl_fetch and the obs / rewards arguments of pedn_rl_observe / pedn_rl_step hand out the NORMALISED rows (after
 * pedn_rl_observe the rewards are the raw ones: no step, nothing to discount); pedn_rl_fetch_raw and pedn_rl_device_ptr keep handing out
 * the raw ones.  pedn_rl_clock_signature covers the switch and the launch's arguments. */
int pedn_rl_norm_configure(pedn_sim* sim, int32_t norm_obs, int32_t norm_reward, double clip_obs, double clip_reward, double gamma,
                           const int32_t* tracked_mask, const int32_t* agent_of_column);
int pedn_rl_norm_set_training(pedn_sim* sim, int32_t training);
int pedn_rl_norm_get_stats(pedn_sim* sim, double* mean, double* var, double* count, double* ret_stats);
int pedn_rl_norm_set_stats(pedn_sim* sim, const double* mean, const double* var, const double* count, const double* ret_stats);
void* pedn_rl_norm_device_ptr(pedn_sim* sim, int32_t which);
int pedn_rl_fetch_raw(pedn_sim* sim, float* obs, float* rewards);

/* ---- on-policy rollout store and advantage estimates on the device (rl/agents/PPO_org.py:201-354,518-567; rl/rl_utils.py:1754-1773) ----
 * A device-resident store of `capacity` transitions of every env, filled by ONE launch per policy step, and the reference's TD targets,
 * GAE and advantage normalisation for all n_envs x n_agents trajectories.  The contract (restated in numpy by
 * tests/rollout_model.py), IEEE binary32, nothing fused:
 *   td_target[t] = r[t] + (f32(gamma) * v[t + 1]) * (1 - done[t]),  td_delta[t] = td_target[t] - v[t]
 *   c = f32(gamma * lmbda) (the product in binary64); carry = +0; t = T - 1 .. 0: carry = c * carry + td_delta[t], adv[t] = carry
 * (the carry is not masked by done: a fill is one episode, or a prefix of one).  With one env this is the reference's compute_gae bit
 * for bit.  Normalised advantages: per agent over all T * n_envs entries in binary64, (x - mean) / (std + 1e-8) with the unbiased std;
 * sums over the env axis in the fixed order of the running normalisation, the T row sums added in increasing t.
 * Arrays, every one [row][env][...]: 0 actions f64 [cap][R][n_actions], 1 values f32 [cap + 1][R][n_agents] (row t = V(s_t) as given to
 * the record of row t; row `rows` = the bootstrap value of pedn_rollout_finish), 2 rewards f32 [cap][R][n_agents], 3 done f32 [cap][R],
 * 4 observations f32 [cap + 1][R][n_obs] (NULL unless store_obs; row 0 = the observation at pedn_rollout_begin, row k + 1 = the one
 * behind step k), 5 td_target, 6 advantages, 7 normalised advantages f32 [cap][R][n_agents], 8 state int32 [4] = cursor, ticket,
 * overflow.  Observations and rewards are read from the buffers pedn_rl_fetch hands out (the normalised rows while pedn_rl_norm_configure
 * has the normalisation on).
 *   pedn_rollout_configure   allocates the store (a previous one is freed).  pedn_rl_configure drops it; pedn_rl_clock_signature covers it.
 *   pedn_rollout_begin       cursor = 0, overflow = 0, observation row 0 = the current observation; on pedn_stream()
 *   pedn_rollout_record      one launch on `stream` (NULL = pedn_stream()); actions f64 [R][n_actions] and values f32 [R][n_agents] are
 *                            device pointers (NULL = zeros).  done = term, or, inside a clocked section, whether the device clock stands
 *                            at the horizon.  No allocation, no synchronisation, no event query: safe under stream capture, and the
 *                            arguments are constant, so a captured record is replayed with the step.  A record beyond the capacity
 *                            writes nothing and raises the overflow flag.
 *   pedn_rollout_finish      synchronises the device; rows = min(cursor, capacity); values[rows] = last_values (device, NULL = zeros)
 *   pedn_rollout_compute     td_target and advantages of rows [0, rows) (one launch), normalised advantages when `normalize` (three more)
 *   pedn_gae                 the same arithmetic on plain device pointers, no handle: rewards / dones / td_target / adv [T][lanes],
 *                            values [T + 1][lanes]; one launch on `stream`.  values = NULL: `rewards` holds td_delta itself (the argument
 *                            of the reference's compute_gae), only adv is written */
int pedn_rollout_configure(pedn_sim* sim, int32_t capacity, int32_t store_obs);
int pedn_rollout_free(pedn_sim* sim);
int pedn_rollout_begin(pedn_sim* sim);
int pedn_rollout_record(pedn_sim* sim, const double* actions, const float* values, int32_t term, void* stream);
int pedn_rollout_finish(pedn_sim* sim, const float* last_values, int32_t* rows, int32_t* overflow);
int pedn_rollout_compute(pedn_sim* sim, double gamma, double lmbda, int32_t normalize);
void* pedn_rollout_device_ptr(pedn_sim* sim, int32_t which);
int pedn_gae(const float* rewards, const float* values, const float* dones, int32_t T, int32_t lanes, double gamma, double lmbda,
             float* td_target, float* adv, void* stream);
/* pedn_gae with the next values in an array of their own: values and next_values f32 [T][lanes], td_target[t] = r[t] + (f32(gamma) *
 * next_values[t]) * (1 - done[t]), everything else (the kernel, the order, the roundings) pedn_gae's; with next_values[t] = values[t + 1]
 * the results are pedn_gae's bit for bit.  For recurrent critics, whose next_values are a run of their own (pedn_lstm_ppo_evaluate).  No
 * pointer may be NULL. */
int pedn_gae_next(const float* rewards, const float* values, const float* next_values, const float* dones, int32_t T, int32_t lanes,
                  double gamma, double lmbda, float* td_target, float* adv, void* stream);

/* ---- the reference's stacked actors for all envs and agents in one launch (rl/agents/SAC.py:72-107,277-293; PPO_org.py:145-172,470-516) --
 * Handle-free, on plain device pointers; the arithmetic contract is DESIGN section 14 (tests/actor_model.py restates it in numpy).
 *   stack    f32 [n_envs][stack_size][n_obs], oldest frame first (e.g. array 6 of pedn_replay_device_ptr); input i = f * stack_size + s of
 *            an agent is stack[e][s][obs0 + f]
 *   table    int32 [n_agents][6]: obs0, obs_w, act0, act_w, the offset of the agent's tensors in `params` (floats), 0.  The caller
 *            guarantees obs0 + obs_w <= n_obs, act0 + act_w <= n_actions, 1 <= act_w <= 8, disjoint action columns, and with
 *            delta_actions that act_w divides obs_w
 *   low, high  f32 [n_actions]: the bounds of the absolute actions
 *   params   f32: per agent, in nn.Linear's [out][in] layout, encoder.fc1 weight [64][stack_size * obs_w] and bias [64], encoder.fc2
 *            [64][64] + [64], fc [64][64] + [64], for kind 1 ln weight [64] and bias [64], fc_mu [act_w][64] + [act_w], fc_std the same
 *   noise    f32 [n_envs][n_actions], read with mode 1 (may be NULL otherwise)
 *   mu, std, eps, raw  f32 [n_envs][n_actions], actions f64 [n_envs][n_actions]: written for every column some agent owns
 *   state    int64 [2], zeroed by the caller once: 0 the draw counter d, 1 the ticket of the launch's workgroups
 * kind 0 (SAC): std = softplus, raw = tanh(mu + std * eps) * max_delta.  kind 1 (PPO): LayerNorm behind fc, std clamped to
 * [min_std, max_std], raw = mu + std * eps clamped to +-max_delta (delta_actions) or to [low, high].  actions = clip(width + raw, low,
 * high) with delta_actions (width: the newest frame's column obs0 + (j + 1) * obs_w / act_w - 1), else raw.  mode 0: eps of (env, column
 * c) is drawn from Philox4x32-10((replica_offset + env, d lo, 0x72 | c << 8, d hi), seed) and the launch's last workgroup advances d;
 * mode 1: eps = noise; mode 2 (deterministic): eps = 0 and raw comes from mu alone.  hidden_size must be 64.
 * One launch on `stream` (NULL = the default stream); no allocation, no synchronisation, no event query, constant arguments: safe under
 * stream capture, and a captured launch is replayed with the step (the draw counter lives in device memory). */
int pedn_actor_forward(const float* stack, const int32_t* table, const float* low, const float* high, const float* params,
                       const float* noise, float* mu, float* std, float* eps, float* raw, double* actions, int64_t* state,
                       int32_t n_envs, int32_t stack_size, int32_t n_obs, int32_t n_actions, int32_t n_agents, int32_t hidden_size,
                       int32_t kind, int32_t delta_actions, int32_t mode, double max_delta, double min_std, double max_std, uint64_t seed,
                       uint32_t replica_offset, void* stream);

/* ---- SAC TD targets and Polyak updates of all agents (rl/agents/SAC.py:109-125 QValueNetContinuous, :296-318 calc_target, soft_update) ----
 * Handle-free, on plain device pointers; the arithmetic contract is DESIGN section 15 (tests/sac_target_model.py restates it in numpy).
 *   next_states  f32 [batch][stack_size][n_obs], rewards f32 [batch][n_agents], dones f32 [batch]: a whole-row minibatch (pedn_replay_sample)
 *   table        the int32 [n_agents][6] table of pedn_actor_forward, with the same guarantees; actor_params its SAC-kind pack
 *   critic_table int32 [n_agents][2]: the offsets (floats, multiples of 4) of the agent's critic 1 and critic 2 in a critic pack
 *   target_params  f32: per critic, in nn.Linear's [out][in] layout, encoder.fc1 [64][stack_size * obs_w] + [64], encoder.fc2 [64][64] +
 *                [64], fc [64][64 + act_w + 1] + [64], fc_out [1][64] + [1]; its input row is the 64 encoder outputs, next_action and the
 *                newest frame's column obs0 + obs_w - 1; no ReLU between fc and fc_out
 *   log_alpha    f32 [n_agents]
 *   noise        f32 [batch][n_actions] used as eps, or NULL: eps of (row b, column c) is drawn from Philox4x32-10((b, d lo, 0x73 | c << 8,
 *                d hi), seed) and the launch's last workgroup advances d
 *   out_actions  f32 [5][batch][n_actions]: mu, std, eps, logp, next_actions; out_agents f32 [4][batch][n_agents]: entropy, q1, q2,
 *                td_target.  Written for every column some agent owns, for inspection; td_target is the result
 *   state        int64 [2], zeroed by the caller once: 0 the draw counter d, 1 the ticket of the launch's workgroups
 * next_action = tanh(mu + std * eps) * max_delta, logp = Normal(mu, std).log_prob(u) - log(1 - tanh(tanh(u))^2 + 1e-7) (the reference's
 * second tanh is mirrored), entropy = -sum logp, q = min(q1, q2) with NaN winning, td_target = r + gamma * (q + exp(log_alpha) * entropy) *
 * (1 - done).  hidden_size must be 64.  One launch on `stream` (NULL = the default stream); no allocation, no synchronisation, no event
 * query, constant arguments: safe under stream capture. */
int pedn_sac_td_target(const float* next_states, const float* rewards, const float* dones, const int32_t* table, const int32_t* critic_table,
                       const float* actor_params, const float* target_params, const float* log_alpha, const float* noise,
                       float* out_actions, float* out_agents, int64_t* state, int32_t batch, int32_t stack_size, int32_t n_obs,
                       int32_t n_actions, int32_t n_agents, int32_t hidden_size, double max_delta, double gamma, uint64_t seed,
                       void* stream);
/* target[i] = target[i] * (float)(1 - tau) + online[i] * (float)tau for i < n_floats (a positive multiple of 4; both packs 16-byte aligned;
 * 0 <= tau <= 1): the reference's soft_update of every target critic at once.  One launch on `stream`, capturable like the above. */
int pedn_sac_soft_update(float* target, const float* online, int64_t n_floats, double tau, void* stream);

/* ---- SAC critic gradients and Adam steps of all agents (rl/agents/SAC.py:320-341, the critic half of SACAgent.update) -----------------------
 * Handle-free, on plain device pointers; the arithmetic contract is DESIGN section 18 (tests/sac_critic_model.py restates it in numpy).
 *   states       f32 [batch][stack_size][n_obs], actions f32 [batch][n_actions] (what the critics see: the stored actions), td_target f32
 *                [batch][n_agents] (pedn_sac_td_target's)
 *   table, critic_table   as for pedn_sac_td_target
 *   online_params, grads, exp_avg, exp_avg_sq   f32 [pack_floats] each, one layout (pedn_sac_td_target's target_params), 16-byte aligned;
 *                pack_floats a multiple of 4; the padding between the critics is +0.0 and stays so
 *   workspace    f32 [ceil(batch / 32)][pack_floats + 2 * n_agents rounded up to 4], zeroed by the caller once, 16-byte aligned
 *   q            f32 [2][batch][n_agents]: q1, q2; losses f32 [n_agents][2]: mean((q - td_target)^2) of critic 1 and critic 2
 *   adam_state   int64 [4], set by the caller once: 0 the step count (0), 1 the ticket of the launch's workgroups (0), 2 and 3 the
 *                doubles beta1^t and beta2^t (1.0)
 * Two launches on `stream`: the tiles' partial gradients of both MSE losses (tiles of 32 rows, rows ascending), then their sum (tiles
 * ascending) into grads and losses and, if do_adam is not 0, one torch.optim.Adam step (no weight decay, no amsgrad) of exp_avg, exp_avg_sq
 * and online_params in place, which advances adam_state.  With do_adam = 0 nothing but grads, losses, q and the workspace is written.
 * 0 <= lr, eps < inf, 0 <= beta < 1; hidden_size must be 64.  No allocation, no synchronisation, no event query, constant arguments: safe
 * under stream capture. */
int pedn_sac_critic_update(const float* states, const float* actions, const float* td_target, const int32_t* table, const int32_t* critic_table,
                           float* online_params, float* grads, float* exp_avg, float* exp_avg_sq, float* workspace, float* q, float* losses,
                           int64_t* adam_state, int64_t pack_floats, int32_t batch, int32_t stack_size, int32_t n_obs, int32_t n_actions,
                           int32_t n_agents, int32_t hidden_size, double lr, double beta1, double beta2, double eps, int32_t do_adam,
                           void* stream);

/* ---- SAC actor and temperature gradients and Adam steps of all agents (rl/agents/SAC.py:347-370, the actor half of SACAgent.update) -------
 * Handle-free, on plain device pointers; the arithmetic contract is DESIGN section 19 (tests/sac_actor_model.py restates it in numpy).
 *   states       f32 [batch][stack_size][n_obs]; noise f32 [batch][n_actions] used as eps, or NULL: drawn (Philox stream 0x75, counter
 *                draw_state[0], row = the batch row)
 *   table, critic_table   as for pedn_sac_td_target
 *   actor_params, grads, exp_avg, exp_avg_sq   f32 [pack_floats] each, pedn_actor_forward's SAC-kind pack and three of its layout, 16-byte
 *                aligned; the padding between the actors is +0.0 and stays so.  online_params: the online critics' pack, read only
 *   log_alpha    f32 [n_agents], stepped in place; target_entropy f32 [n_agents]; alpha_moments f32 [2][n_agents]: exp_avg, exp_avg_sq
 *   workspace    f32 [ceil(batch / 32)][pack_floats rounded up to 4 + 2 * n_agents rounded up to 4], zeroed by the caller once
 *   out_actions  f32 [9][batch][n_actions]: mu, std, eps, logp, new_actions, z (the pre-softplus value), t = tanh(mu + std * eps), d_mu and
 *                d_z (the loss' gradients by mu and by z); out_agents f32 [3][batch][n_agents]: entropy, q1, q2
 *   scalars      f32 [3][n_agents]: actor_loss = mean(-alpha * entropy - min(q1, q2)), alpha_loss, alpha_grad = alpha * mean(entropy -
 *                target_entropy)
 *   adam_state   int64 [4] as for pedn_sac_critic_update, the actor's and the temperature's own; draw_state int64 [2] (zeros)
 * Two launches on `stream`: the tiles' partial gradients (tiles of 32 rows, rows ascending), then their sum (tiles ascending) into grads
 * and scalars and, if do_adam is not 0, one torch.optim.Adam step of actor_params with actor_lr and of log_alpha with alpha_lr, in
 * place, which advances adam_state.  With do_adam = 0 nothing but grads, scalars, the outputs, the workspace and (drawing) draw_state is
 * written.  0 <= lr, eps < inf, 0 <= beta < 1; hidden_size must be 64.  No allocation, no synchronisation, constant arguments: safe under
 * stream capture. */
int pedn_sac_actor_update(const float* states, const float* noise, const int32_t* table, const int32_t* critic_table, float* actor_params,
                          const float* online_params, float* log_alpha, const float* target_entropy, float* grads, float* exp_avg,
                          float* exp_avg_sq, float* alpha_moments, float* workspace, float* out_actions, float* out_agents, float* scalars,
                          int64_t* adam_state, int64_t* draw_state, int64_t pack_floats, int32_t batch, int32_t stack_size, int32_t n_obs,
                          int32_t n_actions, int32_t n_agents, int32_t hidden_size, double max_delta, double actor_lr, double alpha_lr,
                          double beta1, double beta2, double eps, uint64_t seed, int32_t do_adam, void* stream);

/* ---- PPO's value critics and old log-probabilities of a whole rollout (rl/agents/PPO_org.py:175-197 StackedValueNetwork, :543-577) -------
 * Handle-free, on plain device pointers; the arithmetic contract is DESIGN section 16 (tests/ppo_eval_model.py restates it in numpy).
 *   obs          f32 [T + 1][N][n_obs]: every observation once (array 4 of pedn_rollout_device_ptr behind pedn_rollout_finish).  The state
 *                of row t, 0 <= t <= T, of env e is the frames obs[max(t - (stack_size - 1) + s, 0)][e], s = 0 .. stack_size - 1, oldest
 *                first; input i = f * stack_size + s of an agent is that frame's column obs0 + f
 *   actions      [T][N][n_actions], f32 (actions_f64 = 0) or f64 (1, read as (float)x): the actions whose log-probability is wanted
 *   table        the int32 [n_agents][6] table of pedn_actor_forward, with the same guarantees; actor_params its PPO-kind pack
 *   value_table  int32 [n_agents]: the offset (floats, a multiple of 4) of the agent's value network in value_params
 *   value_params f32: per agent, in nn.Linear's [out][in] layout, encoder.fc1 [64][stack_size * obs_w] + [64], encoder.fc2 [64][64] + [64],
 *                fc [64][64] + [64], value_head [1][64] + [1]; v = value_head(relu(fc(encoder))), no LayerNorm
 *   values       f32 [T + 1][N][n_agents]: V of every state, row T the bootstrap value; values[t + 1] is the reference's next_values[t]
 *   old_log_probs  f32 [T][N][n_actions]: Normal(mu, std).log_prob(action) with mu, std of pedn_actor_forward's kind 1 (std clamped to
 *                [min_std, max_std]), evaluated in double from the float32 values and rounded once
 *   mu, std      f32 [T][N][n_actions], or NULL: not written
 * Written for every column some agent owns.  hidden_size must be 64.  One launch on `stream` (NULL = the default stream); no allocation,
 * no synchronisation, no event query, constant arguments: safe under stream capture. */
int pedn_ppo_evaluate(const float* obs, const void* actions, const int32_t* table, const int32_t* value_table, const float* actor_params,
                      const float* value_params, float* values, float* old_log_probs, float* mu, float* std, int32_t T, int32_t N,
                      int32_t stack_size, int32_t n_obs, int32_t n_actions, int32_t n_agents, int32_t hidden_size, int32_t actions_f64,
                      double min_std, double max_std, void* stream);

/* ---- one epoch of PPO's clipped-loss update of all agents (rl/agents/PPO_org.py:579-629 and the KL early stop) ---------------------------
 * Handle-free, on plain device pointers; the arithmetic contract is DESIGN section 20 (tests/ppo_update_model.py restates it in numpy).
 *   obs, actions, table, value_table, actor_params, value_params, min_std, max_std   as for pedn_ppo_evaluate; both packs are stepped in place
 *   old_log_probs  f32 [T][N][n_actions]; advantages, td_target f32 [T][N][n_agents] (an agent's advantage serves its act_w columns)
 *   *_grads, *_raw_grads, *_exp_avg, *_exp_avg_sq   f32, the layout of their network's pack: the clipped and the unclipped gradients and
 *                Adam's moments; 16-byte aligned like the packs; the padding is +0.0 and stays so
 *   workspace    f32 [min(ceil(T * N / 32), groups)][actor_pack_floats rounded up to 4 + value_pack_floats + 8 * n_agents]: a slab per group of
 *                tiles, bounded by `groups` whatever T * N is; need not be zeroed
 *   norm_parts   f64 [n_agents][2][16]; log_probs f32 [T][N][n_actions]; values f32 [T][N][n_agents]
 *   tail_out     f32 [3][T][N][n_actions], or NULL: not written: std and the actor loss' gradients by mu and by the pre-softplus value
 *   scalars      f32 [7][n_agents]: actor_loss, critic_loss, approx_kl = mean(log_probs - old_log_probs), the actor's and the value network's
 *                total gradient norm, and their clip coefficients min(max_grad_norm / (norm + 1e-6), 1)
 *   adam_state   int64 [n_agents][4], set by the caller once: per agent the step count (0), a ticket (0), the doubles beta1^t, beta2^t (1.0)
 *   stop_flags   int32 [n_agents]: an agent whose flag is not 0 is skipped whole (nothing of it is read or written).  With do_adam the
 *                flag is set behind the step of an epoch whose approx_kl > 1.5 * kl_tolerance; pedn_ppo_begin_update clears the flags
 * Three launches on `stream`: the groups' partial gradients (tiles of 32 rows, rows ascending; group g takes tiles g, g + G, ..), their sum
 * (g ascending) with the losses and the norms' parts, then clip_grad_norm_ and, if do_adam is not 0, one torch.optim.Adam step of each
 * network (actor_lr, critic_lr).  With do_adam = 0 no parameter, moment, count or flag changes.  0 <= lr, eps < inf, 0 <= beta < 1, 0 <
 * clip_eps, max_grad_norm < inf, kl_tolerance not NaN, 1 <= groups <= 65535; hidden_size must be 64.  No allocation, no synchronisation,
 * constant arguments: safe under stream capture. */
int pedn_ppo_epoch_update(const float* obs, const void* actions, const float* old_log_probs, const float* advantages, const float* td_target,
                          const int32_t* table, const int32_t* value_table, float* actor_params, float* value_params, float* actor_grads,
                          float* value_grads, float* actor_raw_grads, float* value_raw_grads, float* actor_exp_avg, float* value_exp_avg,
                          float* actor_exp_avg_sq, float* value_exp_avg_sq, float* workspace, double* norm_parts, float* log_probs, float* values,
                          float* tail_out, float* scalars, int64_t* adam_state, int32_t* stop_flags, int64_t actor_pack_floats, int64_t value_pack_floats,
                          int32_t T, int32_t N, int32_t stack_size, int32_t n_obs, int32_t n_actions, int32_t n_agents, int32_t hidden_size,
                          int32_t actions_f64, int32_t groups, double min_std, double max_std, double actor_lr, double critic_lr,
                          double clip_eps, double max_grad_norm, double kl_tolerance, double beta1, double beta2, double eps, int32_t do_adam,
                          void* stream);
/* stop_flags[0 .. n_agents) = 0, one small launch on `stream`: capturable. */
int pedn_ppo_begin_update(int32_t* stop_flags, int32_t n_agents, void* stream);

/* ---- the reference's stateful LSTM PPO agents (rl/agents/PPO_org.py:20-138 LSTMPolicyNetwork / LSTMValueNetwork, :470-516, :543-577) ----
 * Handle-free, on plain device pointers; the arithmetic contract is DESIGN section 17 (tests/lstm_model.py restates it in numpy).  One
 * nn.LSTM layer of 64 units (hidden_size must be 64, num_layers 1), gate rows i, f, g, o; an agent's input is the single frame's columns
 * obs0 .. obs0 + obs_w - 1.
 *   table    the int32 [n_agents][6] table of pedn_actor_forward, with the same guarantees; the offset is the agent's in `params`
 *   params   f32: per agent lstm.weight_ih_l0 [256][obs_w], lstm.weight_hh_l0 [256][64], lstm.bias_ih_l0 [256], lstm.bias_hh_l0 [256],
 *            mean_head [act_w][64] + [act_w], std_head the same
 *   hc       f32 [n_agents][n_envs][2][64], 16-byte aligned: h, then c, of every (agent, env); read and updated in place, one writer per
 *            (agent, env, unit).  The caller zeroes it once (pedn_lstm_reset)
 *   obs      f32 [n_envs][n_obs]; low, high, noise, mu, std, eps, raw, actions, state as in pedn_actor_forward
 * pedn_lstm_actor_forward: one step of every agent's actor for every env: (h, c) <- LSTM(obs, (h, c)), mu = mean_head(relu(h)), std =
 * softplus(std_head(relu(h))) clamped to [min_std, max_std], then pedn_actor_forward's kind-1 tail (raw, actions, the three modes); the
 * drawn noise uses site byte 0x74.  One launch on `stream` (NULL = the default stream); no allocation, no synchronisation, no event query,
 * constant arguments: safe under stream capture, and a captured launch is replayed with the step.
 * pedn_lstm_reset: h = c = +0.0 for the envs whose mask byte is not 0 (mask u8 [n_envs] on the device, NULL: every env), of every agent:
 * the reference's reset_buffer().  One launch, capturable like the above. */
int pedn_lstm_actor_forward(const float* obs, const int32_t* table, const float* low, const float* high, const float* params,
                            const float* noise, float* hc, float* mu, float* std, float* eps, float* raw, double* actions, int64_t* state,
                            int32_t n_envs, int32_t n_obs, int32_t n_actions, int32_t n_agents, int32_t hidden_size, int32_t num_layers,
                            int32_t delta_actions, int32_t mode, double max_delta, double min_std, double max_std, uint64_t seed,
                            uint32_t replica_offset, void* stream);
int pedn_lstm_reset(float* hc, const uint8_t* mask, int32_t n_envs, int32_t n_agents, int32_t hidden_size, void* stream);
/* What PPOAgent.update computes under no_grad with the LSTM networks, for every env and agent in ONE launch; each of the three runs
 * starts from a zero state and steps t inside the kernel:
 *   obs          f32 [T + 1][N][n_obs] (array 4 of pedn_rollout_device_ptr behind pedn_rollout_finish); actions as in pedn_ppo_evaluate
 *   value_params f32: per agent lstm.* as above, value_head [1][64] + [1]; value_table int32 [n_agents]: its offsets (multiples of 4)
 *   values       f32 [T][N][n_agents]: the value LSTM over obs[0 .. T - 1]
 *   next_values  f32 [T][N][n_agents]: the value LSTM over obs[1 .. T], a run of its own (NOT values[t + 1]: forward_all_steps of the
 *                next states with hidden = None)
 *   old_log_probs  f32 [T][N][n_actions]: Normal(mu, std).log_prob(action) of the actor LSTM over obs[0 .. T - 1]; mu, std f32 [T][N][n_actions]
 *                or NULL: not written
 * Written for every column some agent owns.  Capturable like the above. */
int pedn_lstm_ppo_evaluate(const float* obs, const void* actions, const int32_t* table, const int32_t* value_table, const float* actor_params,
                           const float* value_params, float* values, float* next_values, float* old_log_probs, float* mu, float* std,
                           int32_t T, int32_t N, int32_t n_obs, int32_t n_actions, int32_t n_agents, int32_t hidden_size, int32_t num_layers,
                           int32_t actions_f64, double min_std, double max_std, void* stream);

/* ---- replay store of the off-policy trainers on the device (rl/rl_utils.py:37-50 ReplayBuffer; rl/agents/SAC.py:127-225) ----------
 * A device-resident ring of transitions of every env that keeps each observation ONCE, filled by ONE launch per policy step, and a
 * gather of sampled minibatches as stacks of the last `stack_size` observations.  The contract (restated in numpy by
 * tests/replay_model.py): every begin / push takes the next serial s = 0, 1, ... and writes slot s mod R of the ring, R = capacity +
 * stack_size + ceil(capacity / episode_steps) + 1.  A RESET row (begin) holds the observation; a STEP row (push) the observation behind
 * the step, the actions, the rewards, done and `first`, the serial of its episode's RESET row.  State of STEP row s = the frames
 * max(s - stack_size + i, first), i = 0 .. stack_size - 1; next state = the frames max(s - stack_size + 1 + i, first).  Sampleable: the
 * newest `capacity` STEP rows whose oldest frame max(s - stack_size, first) is still in the ring (>= head - R): size_rows of them, a
 * suffix of the STEP rows.  Everything is copied bit for bit.
 * Arrays: 0 frames f32 [R][envs][n_obs], 1 actions f64 [R][envs][n_actions], 2 rewards f32 [R][envs][n_agents], 3 done f32 [R],
 * 4 first i64 [R] (-1: a RESET row), 5 step_serial i64 [capacity] (STEP count j mod capacity -> serial), 6 the stacked observation f32
 * [envs][stack_size][n_obs] (the next state of the newest row, written by the begin / push launch itself), 7 state i64 [10] = head (the
 * next serial), STEP rows so far, size_rows, first of the running episode, draw counter, error flag, two ticket counters, head mod R, STEP
 * rows mod capacity.
 * Observations and rewards are read from the buffers pedn_rl_fetch hands out (the normalised rows while the normalisation is on).
 *   pedn_replay_configure    allocates the store (a previous one is freed); capacity in rows (one row = one policy step of all envs).
 *                            pedn_rl_configure drops it; pedn_rl_clock_signature covers it.  It lives beside a rollout store.
 *   pedn_replay_begin        a RESET row from the current observation; on pedn_stream()
 *   pedn_replay_push         a STEP row: one launch on `stream` (NULL = pedn_stream()); actions f64 [envs][n_actions] is a device
 *                            pointer.  done = term, or, inside a clocked section, whether the device clock stands at the horizon.  No
 *                            allocation, no synchronisation, no event query, constant arguments: a captured push is replayed with the step.
 *   pedn_replay_sample       one launch on `stream`, capturable like the push.  indices = NULL: `batch` (row, env) pairs drawn with
 *                            replacement, draw d (the draw counter, advanced by the launch) and sample k from
 *                            w = philox4x32_10((k, d & 0xffffffff, 0x71, d >> 32), (seed & 0xffffffff, seed >> 32)): STEP count
 *                            j = (STEP rows so far) - 1 - ((w[0] * size_rows) >> 32), env (w[1] * envs) >> 32.  indices = device i64
 *                            [batch][2] (serial, env): those pairs, the draw counter stays.  Outputs (device): states / next_states f32
 *                            [batch][stack_size][obs_w], actions f64 [batch][act_w], rewards f32 [batch][rew_w], dones f32 [batch], idx
 *                            i64 [batch][2] (NULL: not wanted) -- the observation columns [obs0, obs0 + obs_w) and so on.  A sample that
 *                            is not sampleable (an empty store, an evicted or RESET serial, an env out of range) writes nothing, reads
 *                            nothing outside the ring and raises the error flag.
 *   pedn_replay_size         synchronises the device; state[6] = the first six state words; the error flag is cleared once reported */
int pedn_replay_configure(pedn_sim* sim, int64_t capacity, int32_t stack_size, int32_t episode_steps, uint64_t seed);
int pedn_replay_free(pedn_sim* sim);
int pedn_replay_begin(pedn_sim* sim);
int pedn_replay_push(pedn_sim* sim, const double* actions, int32_t term, void* stream);
int pedn_replay_sample(pedn_sim* sim, int64_t batch, const int64_t* indices, int32_t obs0, int32_t obs_w, int32_t act0, int32_t act_w,
                       int32_t rew0, int32_t rew_w, float* states, double* actions, float* rewards, float* next_states, float* dones,
                       int64_t* idx, void* stream);
int pedn_replay_size(pedn_sim* sim, int64_t* state);
void* pedn_replay_device_ptr(pedn_sim* sim, int32_t which);

/* ---- rule-based controllers on the device (rl/agents/rule_based.py, evaluated by rl/rl_utils.py:1513-1750) ----------------------
 * A controller per agent of the pedn_rl_configure agent set computes the agent's next action from the float32 observation the step has
 * just written, inside the observation part of the step's second launch (no extra launch, no host round trip between env steps):
 *   kind 1  RuleBasedGaterAgent(outgoing_links, "option2", threshold): needs obs_mode 2; `threshold` is rounded to float32, `open[slot]`
 *           is the float32 physical width of the slot's link (the "open" action and the action at a density equal to the threshold)
 *   kind 2  RuleBasedSeparatorAgent(width, use_smoothing, buffer_size): window[a] = buffer_size with smoothing, 0 without (at most
 *           PEDN_CTRL_MAX_WINDOW = 32); wide[a] != 0: the width is a binary64 numpy scalar (binary64 arithmetic without smoothing)
 *   kind 0  no controller: the agent's action slots stay NaN (no action)
 * Arrays are [n_agents], `open` is [n_actions].  Configuring empties every moving-average buffer and the episode sums, and fills the
 * action rows with NaN; pedn_reset and pedn_ctrl_observe keep the buffers (they belong to the agent, not to the episode).
 *   pedn_ctrl_observe(t)             the reset observation (pedn_rl_observe(t, 0)) through the controllers: episode sums back to 0,
 *                                    the actions of the first env step into the action rows
 *   pedn_ctrl_step(t, gap, n)        n env steps t, t + gap, ... (pedn_rl_step with the action rows as device actions) enqueued without a
 *                                    host wait; on the last sub-step of each the controllers decide the next actions and every agent's
 *                                    summed reward is added to its float32 episode sum.  Results: pedn_rl_device_ptr / pedn_rl_fetch
 *   pedn_ctrl_read                   host copies of the action rows [R][n_actions] (f64) / episode sums [R][n_agents] (f32); NULL skips
 *   pedn_ctrl_device_ptr(which)      0 action rows, 1 episode sums */
int pedn_ctrl_configure(pedn_sim* sim, const int32_t* kind, const int32_t* window, const int32_t* wide, const float* threshold,
                        const double* width, const float* open);
int pedn_ctrl_observe(pedn_sim* sim, int32_t t);
int pedn_ctrl_step(pedn_sim* sim, int32_t t, int32_t action_gap, int32_t n_steps);
int pedn_ctrl_read(pedn_sim* sim, double* actions, float* episode_rewards);
void* pedn_ctrl_device_ptr(pedn_sim* sim, int32_t which);

/* Origin demand drawn on the device for every replica at once -- the arrays DemandGenerator builds on the host
 * (src/LTM/od_manager.py:92-155) for the patterns generate_random_demand_params picks (src/utils/env_loader.py:183-222):
 *   pattern 0 gaussian_peaks: Poisson(base + peak * (bump(T/4) + bump(3T/4))), bump(c)(t) = exp(-(t-c)^2 / (2 (T/20)^2)), t < T
 *   pattern 1 constant:       base for t <= T
 *   pattern 2 sudden_demand:  pattern 0 plus `spike_height` for spike_start <= t < spike_start + spike_len
 * Arrays are [n_replicas] for ONE origin node.  The Poisson draws are keyed (seed, global replica id, node, t) with
 * Philox4x32-10 and inverted by sequential search; this is a generator of its own (same distributions as the reference,
 * not numpy's stream), pinned bit for bit by oracle/rand_contract.py (glibc's exp on both sides). */
int pedn_draw_demand(pedn_sim* sim, int32_t node, uint64_t seed, const int32_t* pattern, const double* base, const double* peak,
                     const int32_t* spike_start, const int32_t* spike_len, const double* spike_height);

/* Diagnostic: evaluate the device-side arithmetic primitives on the GPU so that tests can compare them bit for bit
 * with the oracle.  op 0: powf(a[i], b[i]) -> out (f32 in a/b/out as doubles); 1: exp(a[i]); 2: sqrt(a[i]);
 * 3: a[i]/b[i] (f64); 4: (float)a[i]/(float)b[i]; 5: binomial(n=a[i], p=b[i]) keyed (seed, replica=i, link=7, t=11,
 * site=0); 6: normal(sigma=a[i]) keyed (seed, replica=i, link=7, t=11); 7 / 8: a[i] + b[i] with 8- / 16-byte accesses
 * (streaming launches of known byte count for calibrating the HBM counters and the practical bandwidth ceiling); 9: the same
 * with chunks of `seed` doubles visited in a scrambled order (n and seed powers of two). */
int pedn_device_math(int32_t device, int32_t op, int32_t n, const double* a, const double* b, uint64_t seed, double* out);

/* ---- one epoch of PPO's clipped-loss update of the recurrent agents (rl/agents/PPO_org.py:579-629 with use_stacked_obs=False) -------------
 * Handle-free, on plain device pointers; the arithmetic contract is DESIGN section 21 (tests/lstm_update_model.py restates it in numpy).
 *   obs, actions, table, value_table, actor_params, value_params, min_std, max_std   as for pedn_lstm_ppo_evaluate; both packs are stepped
 *                in place.  Env e is one sequence obs[0 .. T - 1][e] from a zero state; done flags inside it do not reset the state
 *   old_log_probs, advantages, td_target, *_grads, *_raw_grads, *_exp_avg, *_exp_avg_sq, workspace, norm_parts, log_probs, values, scalars,
 *   adam_state, stop_flags, groups and the hyper-parameters   as for pedn_ppo_epoch_update, with the recurrent networks' packs
 *   activations  f32 [2][n_agents][T * N][384], 16-byte aligned: per network (0 the value networks, 1 the actors), agent and row r = t * N + e
 *                the forward's h', c' and activated gates i, f, g, o (64 each); the backward overwrites the gates with the pre-activation
 *                gradients a_i, a_f, a_g, a_o.  Need not be zeroed
 *   tail         f32 [4][T][N][n_actions]: std, the actor loss' gradients by mu and by the pre-softplus value, and -min(surr1, surr2)
 * Five launches on `stream`: every env's sequence forward through time, then backward (each a workgroup per 32 envs, agent and network),
 * the weight gradients over tiles of 32 rows into the groups' slabs, their sum with the losses and the norms' parts, then clip_grad_norm_
 * and, if do_adam is not 0, one torch.optim.Adam step of each network.  hidden_size must be 64 and num_layers 1.  No allocation, no
 * synchronisation, constant arguments: safe under stream capture. */
int pedn_lstm_ppo_epoch_update(const float* obs, const void* actions, const float* old_log_probs, const float* advantages, const float* td_target,
                               const int32_t* table, const int32_t* value_table, float* actor_params, float* value_params, float* actor_grads,
                               float* value_grads, float* actor_raw_grads, float* value_raw_grads, float* actor_exp_avg, float* value_exp_avg,
                               float* actor_exp_avg_sq, float* value_exp_avg_sq, float* workspace, float* activations, float* tail,
                               double* norm_parts, float* log_probs, float* values, float* scalars, int64_t* adam_state, int32_t* stop_flags,
                               int64_t actor_pack_floats, int64_t value_pack_floats, int32_t T, int32_t N, int32_t n_obs, int32_t n_actions,
                               int32_t n_agents, int32_t hidden_size, int32_t num_layers, int32_t actions_f64, int32_t groups, double min_std,
                               double max_std, double actor_lr, double critic_lr, double clip_eps, double max_grad_norm, double kl_tolerance,
                               double beta1, double beta2, double eps, int32_t do_adam, void* stream);
/* stop_flags[0 .. n_agents) = 0, one small launch on `stream`: capturable. */
int pedn_lstm_ppo_begin_update(int32_t* stop_flags, int32_t n_agents, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEDN_H */
