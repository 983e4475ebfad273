// pedn_hip.hip -- the core of the host side of the MI355X (gfx950) engine for PedNStream's network_loading hot path: uploads of the compiled model
// (pedn_compile.hpp) and the choice of the static plan (pedn_create, through pedn_plan.hpp: choose), the setters and reads, the step path (launch_step, pedn_step, pedn_run, rl_step and the clocked step) and
// the agent set (pedn_rl_configure) of the C-ABI of include/pedn.h.  The kernels live in pedn_kernels.hpp, the device data structures in
// pedn_types.hpp, the bit-exact arithmetic primitives in pedn_math.hpp, the handle and the shared host helpers in pedn_host.hpp.
// Every training-side feature (controllers, running normalisation, rollout and replay stores, stacked actors, SAC targets, PPO evaluation, evaluation
// metrics) lives entirely in its own header, kernels first and host section behind them; this file knows them by a few named functions
// (norm_launch, norm_reset_returns, store_drop, metrics_free), they know it by the services declared at the end of pedn_host.hpp.
//
// Data layout in HBM: every history field is one array [T+1][columns][RS] with the replica index
// fastest (RS = replicas rounded up to a multiple of 128).  A wavefront owns 64 consecutive replicas of ONE link or node:
// topology and link parameters are wave-uniform (scalar loads), every history access of a wave is one coalesced row
// segment, and the data-dependent look-backs gather between rows of the same column.
//
// Compile with -ffp-contract=off: results must match the reference bit for bit.
#include <memory>

#include "pedn_kernels.hpp"
#include "pedn_host.hpp"
#include "pedn_partition.hpp"
#include "pedn_compile.hpp"
#include "pedn_ctrl.hpp"
#include "pedn_norm.hpp"
#include "pedn_rollout.hpp"
#include "pedn_replay.hpp"
#include "pedn_actor.hpp"
#include "pedn_sac.hpp"
#include "pedn_critic.hpp"
#include "pedn_actor_grad.hpp"
#include "pedn_ppo.hpp"
#include "pedn_ppo_grad.hpp"
#include "pedn_lstm.hpp"
#include "pedn_lstm_grad.hpp"
#include "pedn_metrics.hpp"

// The first launch on a stream and the first cross-stream wait cost the runtime ~0.2 ms (queue creation, signal set-up): pay
// that when the two-chain plan is chosen, not inside the first pedn_run that uses it.
// The two chains only pay off when the two streams are served by DIFFERENT hardware queues.  The runtime maps streams onto a few
// queues (GPU_MAX_HW_QUEUES, 4 by default) and, in a process that holds other streams already -- torch + RCCL under the launcher --
// handed both of the engine's streams the same one: the chains then run one behind the other (melbourne x 1024 30.3 -> 39.0 us per
// step, delft 42.8 -> 64.8, profiles/r04_stream_queues.txt).  So the pairing is probed, not assumed: a 300 us spin on each stream,
// timed together; while they do not overlap another candidate for stream2 is created (the rejected ones stay alive until the
// search ends, so that the runtime moves on to its other queues).
// (chain 2: the stream of the live bins under the dead-link plan, launch_split_step)
static hipStream_t chain_stream(const pedn_sim* s, int c) { return c <= 0 ? s->stream : c == 1 ? s->stream2 : s->stream3; }

// a 300 us spin on the engine's stream and on stream2 (n = 3: and on stream3) at once; *ms = how long all took together
static int probe_overlap(pedn_sim* s, float* ms, int n = 2) {
  HIP_TRY(s, hipEventRecord(s->ev_fork, s->stream));
  for (int c = 1; c < n; ++c) HIP_TRY(s, hipStreamWaitEvent(chain_stream(s, c), s->ev_fork, 0));
  HIP_TRY(s, hipEventRecord(s->ev0, s->stream));
  for (int c = 0; c < n; ++c) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, chain_stream(s, c), 30000ull);   // ticks of the constant 100 MHz clock
  for (int c = 1; c < n; ++c) {
    hipEvent_t ev = c == 1 ? s->ev_join : s->ev_join3;
    HIP_TRY(s, hipEventRecord(ev, chain_stream(s, c)));
    HIP_TRY(s, hipStreamWaitEvent(s->stream, ev, 0));
  }
  HIP_TRY(s, hipEventRecord(s->ev1, s->stream));
  HIP_TRY(s, hipEventSynchronize(s->ev1));
  HIP_TRY(s, hipEventElapsedTime(ms, s->ev0, s->ev1));
  return PEDN_OK;
}
// The second chain's stream, probed to overlap with the engine's; *got = 2 when the two really run side by side, else 1 (the plan
// falls back to one chain).  (Four chains were built and measured no faster: profiles/r04_four_chains.txt.)
static int warm_chain_streams(pedn_sim* s, int* got) {
  *got = 1;
  if (!s->plan.stream_probe) { *got = 2; return PEDN_OK; }
  std::vector<hipStream_t> rejected;
  int rc = PEDN_OK, attempts = 0;
  for (int attempt = 0; attempt < 10 && rc == PEDN_OK; ++attempt) {
    float ms = 0.0f;
    rc = probe_overlap(s, &ms);   // the first pass pays for whatever the runtime sets up lazily (queue creation: ~0.2 ms)
    if (rc == PEDN_OK) rc = probe_overlap(s, &ms);
    if (rc != PEDN_OK) break;
    ++attempts;
    s->stream_probe_ms = ms;
    if (ms < 0.45f) { *got = 2; break; }        // overlapped: 0.3 ms + overheads; one behind another: >= 0.6 ms
    hipStream_t next = nullptr;
    if (hipStreamCreateWithFlags(&next, hipStreamNonBlocking) != hipSuccess) break;   // keep what we have
    rejected.push_back(s->stream2);
    s->stream2 = next;
  }
  s->stream_probe_attempts = attempts;
  for (hipStream_t x : rejected) hipStreamDestroy(x);
  return rc;
}

// The third stream (the live bins of the dead-link plan, launch_split_step), probed to run beside BOTH chains' streams as stream2 was
// probed against the engine's; left null when no candidate does: the plan then stays off (the live launch behind a chain's launches
// would only lengthen that chain).
static int warm_third_stream(pedn_sim* s) {
  if (s->stream3 || !s->plan.dead_links || s->chains < 2) return PEDN_OK;
  const bool probe = s->plan.stream_probe;
  std::vector<hipStream_t> rejected;
  int rc = PEDN_OK;
  bool ok = false;
  for (int attempt = 0; attempt < 6 && rc == PEDN_OK && !ok; ++attempt) {
    // at the highest stream priority: the live launch is a one-generation chain of latencies (3-4 bins x the replica groups) beside
    // two streams that keep every wave place taken -- its workgroups must not queue behind theirs for a place
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = greatest = 0;
    if (hipStreamCreateWithPriority(&s->stream3, hipStreamNonBlocking, greatest) != hipSuccess) { s->stream3 = nullptr; break; }
    if (!probe) { ok = true; break; }
    float ms = 0.0f;
    rc = probe_overlap(s, &ms, 3);
    if (rc == PEDN_OK) rc = probe_overlap(s, &ms, 3);
    if (rc == PEDN_OK && ms < 0.45f) ok = true;
    else { rejected.push_back(s->stream3); s->stream3 = nullptr; }
  }
  for (hipStream_t x : rejected) hipStreamDestroy(x);
  (void)hipGetLastError();
  return rc;
}

// rows [row0, row1) of every history field back to their initial values (`what` as in init_state_kernel; 1 = everything)
static int clear_rows(pedn_sim* s, int row0, int row1, int what) {
  DevView& v = s->v;
  if (row1 <= row0) return PEDN_OK;
  if (what & 1)
    for (int f = 0; f < 4; ++f) {
      const int a = std::min(row0, s->rows64[f]), b = std::min(row1, s->rows64[f]);
      if (b > a) HIP_TRY(s, hipMemsetAsync(v.f64[f] + (size_t)a * v.Lall * v.RS, 0, (size_t)(b - a) * v.Lall * v.RS * sizeof(double), s->stream));
    }
  if (v.L > 0) {
    int max_rows = 0;  // over the fields init_state_kernel fills (all of them have L columns)
    for (int f = 4; f < 7; ++f) max_rows = std::max(max_rows, s->rows64[f]);
    for (int g = 0; g < 6; ++g) max_rows = std::max(max_rows, s->rows32[g]);
    const int a = std::min(row0, max_rows), b = std::min(row1, max_rows);
    if (b > a) {
      const size_t n_l = (size_t)(b - a) * v.L * v.RS;
      hipLaunchKernelGGL(init_state_kernel, dim3((unsigned)((n_l + 255) / 256)), dim3(256), 0, s->stream, v, a, b - a, what);
      HIP_TRY(s, hipGetLastError());
    }
  }
  return PEDN_OK;
}

static int reset_state(pedn_sim* s) {
  DevView& v = s->v;
  HIP_TRY(s, hipMemsetAsync(v.flags, 0, (size_t)v.RS * sizeof(uint32_t), s->stream));
  pedn_plan::reset_full(s->marks);
  mirror_marks(s);
  s->dl_dirty = true;
  return clear_rows(s, 0, v.T1, 1);
}

// Lazy reset (full-record mode): only what a fresh episode reads before it writes is restored -- row 0 of every field, the rows of
// avg_travel_time below the window (link.py:91: never written by the link update), the gate record (stored only where it differs from
// the width) -- and every other row is declared unwritten (valid_hi = 0): 19.5 GB -> 2.5 GB for 45_intersections x 2048 envs.
static int reset_state_lazy(pedn_sim* s) {
  DevView& v = s->v;
  if (v.hist) return reset_state(s);    // the rings are small: nothing to save
  HIP_TRY(s, hipMemsetAsync(v.flags, 0, (size_t)v.RS * sizeof(uint32_t), s->stream));
  int rc;
  if ((rc = clear_rows(s, 0, 1, 1)) || (rc = clear_rows(s, 1, std::min(v.W, v.T1), 2)) || (rc = clear_rows(s, 1, v.T1, 4))) return rc;
  pedn_plan::reset_lazy(s->marks);
  mirror_marks(s);
  return PEDN_OK;
}

// Rows (valid_hi, upto] cleared now: something is about to read them from memory (an out-of-order step, an observation of a step that
// has not run, a zero-copy consumer).
static int catch_up(pedn_sim* s, int upto) {
  if (s->marks.valid_hi >= upto) return PEDN_OK;
  upto = std::min(upto, s->v.T1 - 1);
  DevView view = s->v;
  int rc = PEDN_OK;
  if (upto > s->marks.valid_hi) {
    // everything but the gate record and the low rows of avg_travel_time, which the lazy reset restored already
    DevView& v = s->v;
    const int a = s->marks.valid_hi + 1, b = upto + 1;
    for (int f = 0; f < 4; ++f) HIP_TRY(s, hipMemsetAsync(v.f64[f] + (size_t)a * v.Lall * v.RS, 0, (size_t)(b - a) * v.Lall * v.RS * sizeof(double), s->stream));
    if (v.L > 0) {
      // sending / receiving flow of step t are entries t - 1: entry valid_hi belongs to the step that is being skipped
      const size_t n_1 = (size_t)v.L * v.RS;
      hipLaunchKernelGGL(init_state_kernel, dim3((unsigned)((n_1 + 255) / 256)), dim3(256), 0, s->stream, view, s->marks.valid_hi, 1, 16);
      HIP_TRY(s, hipGetLastError());
      const size_t n_l = (size_t)(b - a) * v.L * v.RS;
      hipLaunchKernelGGL(init_state_kernel, dim3((unsigned)((n_l + 255) / 256)), dim3(256), 0, s->stream, view, a, b - a, 8);
      rc = hipGetLastError() == hipSuccess ? PEDN_OK : fail(s, PEDN_E_DEVICE, "init_state_kernel");
    }
  }
  pedn_plan::caught_up(s->marks, upto);
  mirror_marks(s);
  return rc;
}

static int push_uniform(pedn_sim* s) {
  for (size_t l = 0; l < s->h_rl_link.size(); ++l)
    if (s->h_rl_link[l]) s->h_front_u[l] = s->h_back_u[l] = __builtin_nan("");
  if (!s->h_front_u.empty()) {
    HIP_TRY(s, hipMemcpyAsync(s->d_front_u, s->h_front_u.data(), s->h_front_u.size() * 8, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, hipMemcpyAsync(s->d_back_u, s->h_back_u.data(), s->h_back_u.size() * 8, hipMemcpyHostToDevice, s->stream));
  }
  if (!s->h_tf_u.empty())
    HIP_TRY(s, hipMemcpyAsync(s->d_tf_u, s->h_tf_u.data(), s->h_tf_u.size() * 8, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));  // the host vectors may change right after
  return PEDN_OK;
}

// check_fractions (path_finder.py:691-715) for the rows whose fractions are tabulated on the host (SlotRec.dyn == 2): the
// same binary64 operations the device applies to the other rows.  tab[turn * stride] holds the raw sums.
static void finish_tabulated_rows(const pedn_sim* s, double* tab, size_t stride) {
  for (int n = 0; n < s->n_nodes; ++n) {
    const int s0 = s->h_node_slot_ptr[n], d = s->h_node_slot_ptr[n + 1] - s0;
    for (int i = 0; i < d; ++i) {
      if (s->h_slot_dyn[s0 + i] != 2) continue;
      const int ta = s->node_turn_ptr[n] + i * (d - 1);
      double rowsum = 0.0;
      for (int jj = 0; jj < d - 1; ++jj) rowsum = (jj == 0) ? tab[(size_t)(ta + jj) * stride] : rowsum + tab[(size_t)(ta + jj) * stride];
      if (fabs(rowsum - 1) > 1e-3)
        for (int jj = 0; jj < d - 1; ++jj) {
          double& f = tab[(size_t)(ta + jj) * stride];
          f = rowsum > 1e-6 ? f / rowsum : 1.0 / (double)(d - 1);
        }
    }
  }
}

// P(od | up)[t] = w_od[t] / sum over the upstream's ODs (uniform when the sum is 0), path_finder.py:599-615; the sum runs in
// table order.  Replica independent, so it is tabulated once per (step, product) on the host with the same binary64 operations.
static int tabulate_pair_pod(pedn_sim* s) {
  const int T1 = s->v.T1, np = s->n_pair;
  if (np == 0 || s->d_turn_tab == nullptr) return PEDN_OK;
  std::vector<double> upod((size_t)s->h_upod_od.size());
  std::vector<double> table((size_t)T1 * np);
  for (int t = 0; t < T1; ++t) {
    for (int u = 0; u < s->n_up; ++u) {
      const int a = s->h_up_od_ptr[u], b = s->h_up_od_ptr[u + 1];
      double tot = 0.0;
      for (int q = a; q < b; ++q) tot += s->h_od_w[(size_t)s->h_upod_od[q] * T1 + t];
      for (int q = a; q < b; ++q)
        upod[q] = tot > 0.0 ? s->h_od_w[(size_t)s->h_upod_od[q] * T1 + t] / tot : (b - a > 0 ? 1.0 / (double)(b - a) : 0.0);
    }
    for (int q = 0; q < np; ++q) table[(size_t)t * np + q] = upod[s->h_pair_upod[q]];
  }
  // turns whose products all have the constant probability 1: the fraction is the plain sequential sum of P(od | up)
  const int nt = s->n_turns;
  std::vector<double> ttab((size_t)T1 * std::max(nt, 1), 0.0);
  for (int t = 0; t < T1; ++t)
    for (int tn = 0; tn < nt; ++tn) {
      if (!s->h_turn_mode[tn]) continue;
      double acc = 0.0;
      for (int q = s->h_turn_pair_ptr[tn]; q < s->h_turn_pair_ptr[tn + 1]; ++q) acc += 1.0 * table[(size_t)t * np + q];
      ttab[(size_t)t * nt + tn] = acc;
    }
  for (int t = 0; t < T1; ++t) finish_tabulated_rows(s, &ttab[(size_t)t * nt], 1);
  s->h_ttab = ttab;
  s->h_tab_nz.assign(std::max(nt, 1), 0);   // dead links: can a tabulated fraction ever be anything but +-0.0?
  for (int t = 0; t < T1; ++t)
    for (int tn = 0; tn < nt; ++tn)
      if (!pedn_part::is_zero(ttab[(size_t)t * nt + tn])) s->h_tab_nz[tn] = 1;
  s->dl_dirty = true;
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  HIP_TRY(s, hipMemcpy(s->d_pair_pod, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(s, hipMemcpy(s->d_turn_tab, ttab.data(), ttab.size() * sizeof(double), hipMemcpyHostToDevice));
  return PEDN_OK;
}

// rows[n_rows][R] (host) -> dst[n_rows][RS]
template <typename T>
static int push_matrix(pedn_sim* s, T* dst, const T* src, int n_rows) {
  DevView& v = s->v;
  if (n_rows == 0) return PEDN_OK;
  HIP_TRY(s, hipMemcpy2D(dst, (size_t)v.RS * sizeof(T), src, (size_t)v.R * sizeof(T), (size_t)v.R * sizeof(T), n_rows, hipMemcpyHostToDevice));
  return PEDN_OK;
}

// per-replica link-parameter records, allocated at the first use; padding lanes hold valid numbers and stay idle
static int ensure_link_records(pedn_sim* s) {
  if (s->d_prm) return PEDN_OK;
  const DevView& v = s->v;
  const size_t n = (size_t)v.L * v.RS;
  int rc = dalloc(s, n, &s->d_prm);
  if (rc != PEDN_OK) return rc;
  LinkPR fill;
  fill.kc = 1.0; fill.kj = 2.0; fill.vf = 1.0; fill.tt0 = 1.0f; fill.fft = 32767; fill.tau_sw = 1;
  std::vector<LinkPR> h(n, fill);
  HIP_TRY(s, hipMemcpy(s->d_prm, h.data(), n * sizeof(LinkPR), hipMemcpyHostToDevice));
  return PEDN_OK;
}

// device copies of the route-choice tables that P(od | up) per replica is derived from, and its buffers
static int ensure_pod_tables(pedn_sim* s) {
  if (s->pod_tables_uploaded) return PEDN_OK;
  DevView& v = s->v;
  const int np = s->n_pair, nt = s->n_turns;
  int rc;
  std::vector<int32_t> upod_up(std::max<size_t>(s->h_upod_od.size(), 1), 0), rows;
  for (int u = 0; u < s->n_up; ++u)
    for (int q = s->h_up_od_ptr[u]; q < s->h_up_od_ptr[u + 1]; ++q) upod_up[q] = u;
  for (int n = 0; n < s->n_nodes; ++n) {   // the rows finish_tabulated_rows visits
    const int s0 = s->h_node_slot_ptr[n], d = s->h_node_slot_ptr[n + 1] - s0;
    for (int i = 0; i < d; ++i)
      if (s->h_slot_dyn[s0 + i] == 2) { rows.push_back(s->node_turn_ptr[n] + i * (d - 1)); rows.push_back(d - 1); }
  }
  s->n_tab_rows = (int)rows.size() / 2;
  s->n_upod = (int)s->h_upod_od.size();
  if ((rc = upload(s, s->h_up_od_ptr.data(), s->h_up_od_ptr.size(), &s->d_up_od_ptr)) || (rc = upload(s, s->h_upod_od.data(), s->h_upod_od.size(), &s->d_upod_od)) ||
      (rc = upload(s, upod_up.data(), upod_up.size(), &s->d_upod_up)) || (rc = upload(s, s->h_pair_upod.data(), s->h_pair_upod.size(), &s->d_pair_upod)) ||
      (rc = upload(s, s->h_turn_pair_ptr.data(), s->h_turn_pair_ptr.size(), &s->d_turn_pair_ptr)) ||
      (rc = upload(s, s->h_turn_mode.data(), s->h_turn_mode.size(), &s->d_turn_mode)) || (rc = upload(s, rows.data(), rows.size(), &s->d_tab_rows)))
    return rc;
  if ((rc = dalloc(s, (size_t)std::max(s->n_od, 1) * v.RS, &s->d_od_w_r)) || (rc = dalloc(s, (size_t)std::max(s->n_up, 1) * v.RS, &s->d_pod_tot)) ||
      (rc = dalloc(s, (size_t)np * v.RS, &s->d_pair_pod_r)) || (rc = dalloc(s, (size_t)std::max(nt, 1) * v.RS, &s->d_turn_tab_r)))
    return rc;
  HIP_TRY(s, hipMemset(s->d_od_w_r, 0, (size_t)std::max(s->n_od, 1) * v.RS * 8));
  HIP_TRY(s, hipMemset(s->d_pair_pod_r, 0, (size_t)np * v.RS * 8));
  HIP_TRY(s, hipMemset(s->d_turn_tab_r, 0, (size_t)std::max(nt, 1) * v.RS * 8));
  s->pod_tables_uploaded = true;
  return PEDN_OK;
}

// P(od | up) and the tabulated rows of every replica from d_od_w_r (path_finder.py:599-615, :691-715), on the device
static int scenario_pod_tables(pedn_sim* s) {
  DevView& v = s->v;
  const int np = s->n_pair, nt = s->n_turns, RS = v.RS;
  auto blocks = [&](size_t rows) { return dim3((unsigned)((rows * (size_t)RS + 255) / 256)); };
  if (s->n_up > 0)
    hipLaunchKernelGGL(pod_tot_kernel, blocks(s->n_up), dim3(256), 0, s->stream, (const double*)s->d_od_w_r, s->d_up_od_ptr, s->d_upod_od, s->n_up, RS, s->d_pod_tot);
  hipLaunchKernelGGL(pod_pair_kernel, blocks(np), dim3(256), 0, s->stream, (const double*)s->d_od_w_r, s->d_up_od_ptr, s->d_upod_od, s->d_upod_up,
                     s->d_pair_upod, (const double*)s->d_pod_tot, np, RS, s->d_pair_pod_r);
  if (nt > 0)
    hipLaunchKernelGGL(pod_turn_kernel, blocks(nt), dim3(256), 0, s->stream, (const double*)s->d_pair_pod_r, s->d_turn_pair_ptr, s->d_turn_mode, nt, RS, s->d_turn_tab_r);
  if (s->n_tab_rows > 0)
    hipLaunchKernelGGL(pod_finish_kernel, blocks(s->n_tab_rows), dim3(256), 0, s->stream, s->d_turn_tab_r, s->d_tab_rows, s->n_tab_rows, RS);
  HIP_TRY(s, hipGetLastError());
  v.pair_pod_r = s->d_pair_pod_r; v.turn_tab_r = s->d_turn_tab_r;
  v.pod_pr = 1;
  s->ttab_r_stale = true;
  return PEDN_OK;
}

// (the entry points below have C linkage from their declarations in include/pedn.h)
static int push_rows(pedn_sim* s, double* dst, const double* values, int n_rows, size_t row0, size_t row_stride, int replica);
static void flush_links(pedn_sim* s, int half, hipEvent_t* ev, bool last = true);
typedef void (*step_kernel_fn)(DevView, int);   // node_kernel, turn_frac_kernel, link_kernel_1r
static step_kernel_fn node_kernel_for(const pedn_sim* s, bool lu, bool tf);
static void prewarm_chains(pedn_sim* s);
static int fork_chains(pedn_sim* s, int n, int idle = -1);
static int dl_refresh(pedn_sim* s);

int pedn_abi_version(void) { return PEDN_ABI_VERSION; }

const char* pedn_last_error(const pedn_sim* sim) { return sim ? sim->err.c_str() : g_last_error.c_str(); }

// the half-built handle of pedn_create: every early return destroys it (streams, events, every device allocation made so far); the
// message of the failure stays the thread's last error
namespace {
struct UnbuiltSim {
  void operator()(pedn_sim* s) const {
    const std::string keep = g_last_error;
    pedn_destroy(s);
    g_last_error = keep;
  }
};
}  // namespace

// was a request for `bytes` of dynamic LDS granted for the single-launch node kernel the handle selects, with / without per-replica
// link parameters?  (which of node_kernel<LU, TF> and node_kernel_h that is: s->plan.inline_help)
static bool node_tf_lds_granted(pedn_sim* s, int pr, size_t bytes) {
  const int keep = s->v.pr;
  s->v.pr = pr;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(node_kernel_for(s, true, true)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  s->v.pr = keep;
  return e == hipSuccess;
}

int pedn_create(const pedn_model_desc* m, int32_t n_replicas, int32_t replica_offset, uint64_t seed, int32_t rng_mode,
                int32_t device, pedn_sim** out) {
  if (!m || !out) return fail(nullptr, PEDN_E_ARG, "null argument");
  *out = nullptr;
  // ---- 1. the model compiler (pedn_compile.hpp): every refusal of the description itself, and the static tables; no device, no handle yet
  pedn_compile::Tables tab;
  {
    std::string err;
    int rc = pedn_compile::validate(*m, n_replicas, &err);
    if (rc == PEDN_OK) rc = pedn_compile::compile(*m, pedn_compile::options_from_env(), &tab, &err);
    if (rc != PEDN_OK) return fail(nullptr, rc, err);
  }
  const int N = m->n_nodes, L = m->n_links;
  const int n_slots = m->node_slot_ptr[N];

  HIP_TRY(nullptr, hipSetDevice(device));
  std::unique_ptr<pedn_sim, UnbuiltSim> guard(new pedn_sim());
  pedn_sim* const s = guard.get();
  s->device = device;
  DevView& v = s->v;
  v.L = L;
  v.Lall = L + m->n_vlinks;
  v.T1 = m->T + 1;
  v.R = n_replicas;
  v.RS = (n_replicas + 127) / 128 * 128;  // a link_kernel wave covers 128 replicas (2 per lane), a node_kernel wave 64
  v.sub0 = 0;
  v.subRS = v.RS;
  v.W = m->window;
  v.dt = m->dt;
  v.hist = m->history_mode == PEDN_HIST_RECENT;
  std::copy(tab.m64, tab.m64 + 7, v.m64);
  std::copy(tab.m32, tab.m32 + 6, v.m32);
  std::copy(tab.rows64, tab.rows64 + 7, s->rows64);
  std::copy(tab.rows32, tab.rows32 + 6, s->rows32);
  v.pf_temp = m->pf_temp; v.pf_alpha = m->pf_alpha; v.pf_beta = m->pf_beta; v.pf_omega = m->pf_omega; v.pf_eps = m->pf_eps;
  v.k0 = (uint32_t)seed; v.k1 = (uint32_t)(seed >> 32);
  v.replica_offset = (uint32_t)replica_offset;
  v.meanfield = rng_mode == PEDN_RNG_MEANFIELD;
  v.n_grp = m->n_grp;
  if (const char* d = getenv("PEDN_TF_GENERAL")) v.tf_general = atoi(d);  // diagnostics: 1 general softmax path, 2 general row-sum path
  v.n_pair = m->n_pair;
  v.n_multi = tab.n_multi;
  v.n_trow = tab.n_trow;
  v.n_turns = m->n_turns;
  v.n_pairs_corr = (int)tab.corr.size();
  v.pairs_adj = tab.pairs_adj;
  if (const char* f = getenv("PEDN_PAIRS_ADJ")) if (atoi(f) == 0) v.pairs_adj = 0;   // diagnostic: always through the record
  s->n_nodes = N; s->n_turns = m->n_turns; s->n_demand = m->n_demand; s->n_od = m->n_od; s->n_ent = m->n_ent;
  s->n_pair = m->n_pair;
  s->n_up = m->n_up;
  s->n_over = tab.n_over;
  s->n_tf_heavy_quads = tab.n_tf_heavy_quads;
  s->packed_by = tab.packed_by;
  s->n_blocks = tab.full.n_blocks;
  s->max_degree = tab.max_degree;
  s->node_turn_ptr.assign(m->node_turn_ptr, m->node_turn_ptr + N + 1);
  s->h_node_slot_ptr.assign(m->node_slot_ptr, m->node_slot_ptr + N + 1);
  s->h_tf_set_epoch.assign(N, 0);
  s->node_demand_row.assign(m->node_demand_row, m->node_demand_row + N);
  s->h_up_od_ptr.assign(m->up_od_ptr, m->up_od_ptr + m->n_up + 1);
  s->h_upod_od.assign(m->upod_od, m->upod_od + m->n_upod);
  s->h_pair_upod.assign(m->pair_upod, m->pair_upod + m->n_pair);
  s->h_od_w.assign(m->od_w, m->od_w + (size_t)m->n_od * v.T1);
  s->h_turn_pair_ptr.assign(m->turn_pair_ptr, m->turn_pair_ptr + m->n_turns + 1);
  {  // dead links (pedn_partition.hpp): the host's copy of what the proof reads
    s->h_node_kind.assign(m->node_kind, m->node_kind + N);
    s->h_slot_in.assign(m->slot_in_link, m->slot_in_link + n_slots);
    s->h_slot_out.assign(m->slot_out_link, m->slot_out_link + n_slots);
    s->h_link_rev.assign(m->link_rev, m->link_rev + L);
    s->h_link_sep.assign(m->link_sep, m->link_sep + L);
    s->h_link_tau_sw.assign(m->link_tau_sw, m->link_tau_sw + L);
    s->h_demand_nz = std::move(tab.demand_nz);
  }

  // ---- 2. the plan (pedn_plan.hpp: choose -- the rules, the PEDN_* knobs and the numbers behind each default are there).  Its two device
  // facts are asked for only where they can matter; a request that is refused turns the fact off and the plan is chosen again.
  {
    pedn_plan::PlanInputs in;
    in.RS = v.RS; in.N = N; in.L = L; in.n_trow = v.n_trow;
    in.node_lp = m->node_model == PEDN_NODE_OPTIMAL; in.hist = v.hist != 0;
    in.inline_tf_ok = tab.inline_tf_ok; in.n_blocks = tab.full.n_blocks; in.tiles = tab.full.tiles; in.n_rec = (int)tab.full.rec.size();
    in.tf_wave_lds = PEDN_TF_INL_LDS;
    const pedn_plan::Knobs knobs = pedn_plan::knobs_from_env();
    const size_t lds_tf = pedn_plan::node_lds_tf_bytes(in);
    if (pedn_plan::inline_candidate(in) && lds_tf > pedn_plan::LDS_DEFAULT) {   // (s->plan.inline_help is still off: node_kernel<LU, TF>)
      in.lds_tf = node_tf_lds_granted(s, 0, lds_tf) && node_tf_lds_granted(s, 1, lds_tf);
      (void)hipGetLastError();
    }
    s->plan = pedn_plan::choose(in, knobs);
    if (s->plan.inline_help && lds_tf > pedn_plan::LDS_DEFAULT) {   // node_kernel_h
      in.lds_h = node_tf_lds_granted(s, 0, lds_tf) && node_tf_lds_granted(s, 1, lds_tf);
      (void)hipGetLastError();
      if (!in.lds_h) s->plan = pedn_plan::choose(in, knobs);
    }
    s->chains = s->plan.chains;
    v.tf_lds_off = s->plan.tf_lds_off;
  }
  const pedn_plan::EnginePlan& plan = s->plan;

  // ---- 3. streams and events
  {
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(nullptr, PEDN_E_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    // a null stream2 would be the legacy default stream (it synchronises with everything): every handle is checked
    e = hipStreamCreateWithFlags(&s->stream2, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_join3, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&s->ev0);
    if (e == hipSuccess) e = hipEventCreate(&s->ev1);
    if (e != hipSuccess) return fail(nullptr, PEDN_E_DEVICE, std::string("second stream / events: ") + hipGetErrorString(e));
  }
  // ---- 4. memory budget
  {
    size_t RS = v.RS, T1 = v.T1;
    size_t need = (size_t)(m->n_demand) * T1 * RS * 8 + (size_t)(3 * m->n_turns + 3 * L) * RS * 8;
    for (int f = 0; f < 7; ++f) need += (size_t)s->rows64[f] * (f < 4 ? v.Lall : L) * RS * 8;
    for (int g = 0; g < 6; ++g) need += (size_t)s->rows32[g] * L * RS * 4;
    size_t free_b = 0, total_b = 0;
    const hipError_t mi = hipMemGetInfo(&free_b, &total_b);
    if (mi != hipSuccess) return fail(nullptr, PEDN_E_DEVICE, std::string("hipMemGetInfo: ") + hipGetErrorString(mi));
    if (need + (256u << 20) > free_b)
      return fail(nullptr, PEDN_E_NOMEM, "not enough HBM: need " + std::to_string(need >> 20) + " MiB, free " + std::to_string(free_b >> 20) + " MiB");
  }
  // ---- 5. uploads and allocations: the static tables, what the plan names, the dynamic state; then reset and warm
  int rc;
  if ((rc = upload(s, tab.lp.data(), tab.lp.size(), &v.lp)) || (rc = upload(s, m->node_kind, N, &v.node_kind)) ||
      (rc = upload(s, m->node_slot_ptr, N + 1, &v.node_slot_ptr)) || (rc = upload(s, m->node_turn_ptr, N + 1, &v.node_turn_ptr)) ||
      (rc = upload(s, m->node_demand_row, N, &v.node_demand_row)) || (rc = upload(s, m->node_dyn, N, &v.node_dyn)) ||
      (rc = upload(s, m->slot_in_link, n_slots, &v.slot_in)) || (rc = upload(s, m->slot_out_link, n_slots, &v.slot_out)) ||
      (rc = upload(s, tab.trow_words.data(), tab.trow_words.size(), &v.trow_words)) ||
      (rc = upload(s, tab.tgrp_words.data(), tab.tgrp_words.size(), &v.tgrp_words)) ||
      (rc = upload(s, tab.pair_row.data(), tab.pair_row.size(), &v.pair_row)) || (rc = upload(s, m->od_w, (size_t)m->n_od * v.T1, &v.od_w)) ||
      (rc = upload(s, tab.corr.data(), tab.corr.size(), &v.corr_rec)))
    return rc;
  s->h_pair_const = std::move(tab.pair_const);
  s->h_turn_mode = std::move(tab.turn_mode);
  s->h_slot_dyn = std::move(tab.slot_dyn);
  s->h_slot_trow = std::move(tab.slot_trow);
  s->h_pack_order = std::move(tab.pack_order);
  s->h_slot_rec = std::move(tab.full.rec);
  {  // what the plan names
    const std::vector<SlotRec>& rec = s->h_slot_rec;
    if (plan.node_lp) {  // tableau workspace: one per (regular node, replica group), sized for the largest such node
      const int n_lp = tab.full.n_lp, max_m = tab.full.lp_max_m;
      const int E = max_m * (max_m - 1), rows = 2 * max_m + E, cols = 3 * E + 2 * max_m;
      v.lp_stride = (size_t)(rows + 1) * (cols + 1) * 64;
      v.lp_bstride = (size_t)rows * 64;
      const size_t waves = (size_t)std::max(n_lp, 1) * (v.RS / 64);
      if ((rc = dalloc(s, waves * v.lp_stride, &v.lp_ws)) || (rc = dalloc(s, waves * v.lp_bstride, &v.lp_basis))) return rc;
    }
    if ((rc = upload(s, rec.data(), rec.size(), &v.slot_rec))) return rc;
    s->d_slot_rec = const_cast<SlotRec*>(v.slot_rec);
    v.quiet_npos = (int32_t)rec.size();
    if (plan.quiet) {
      // (node_step indexes the words of one step, half of them, in 32 bits)
      if (plan.quiet_words / 2 >= ((size_t)1 << 31)) return fail(s, PEDN_E_ARG, "too many quiet words");
      if ((rc = dalloc(s, plan.quiet_words, &s->d_quiet))) return rc;
      HIP_TRY(s, hipMemset(s->d_quiet, 0, plan.quiet_words * sizeof(uint32_t)));
    }
    if (plan.dead_capable) {   // the live packing at its capacity, its quiet words, the records of every slot dead_link_kernel may step (dl_refresh fills them)
      if ((rc = dalloc(s, pedn_plan::live_rec_capacity(N), &s->d_live_rec)) || (rc = dalloc(s, rec.size(), &s->d_dead_rec)) ||
          (rc = dalloc(s, rec.size(), &s->d_dead_drec)) || (rc = dalloc(s, plan.quiet_words_live, &s->d_quiet_live)))
        return rc;
      HIP_TRY(s, hipMemset(s->d_quiet_live, 0, plan.quiet_words_live * sizeof(uint32_t)));
    }
  }
  {  // dynamic state
    size_t RS = v.RS, T1 = v.T1;
    for (int f = 0; f < 7; ++f)
      if ((rc = dalloc(s, (size_t)s->rows64[f] * (f < 4 ? v.Lall : L) * RS, &v.f64[f]))) return rc;
    for (int g = 0; g < 6; ++g)
      if ((rc = dalloc(s, (size_t)s->rows32[g] * L * RS, &v.f32[g]))) return rc;
    if ((rc = dalloc(s, (size_t)L * RS, &v.rsum)) || (rc = dalloc(s, (size_t)L * RS, &v.front)) || (rc = dalloc(s, (size_t)L * RS, &v.back)) ||
        (rc = dalloc(s, (size_t)L * RS, &v.sepw)) || (rc = dalloc(s, (size_t)L * RS, &v.sepnp)))
      return rc;
    HIP_TRY(s, hipMemset(v.sepnp, 0, std::max<size_t>((size_t)L * RS, 1) * sizeof(double)));
    if ((rc = dalloc(s, (size_t)m->n_turns * RS, &v.tf)) || (rc = dalloc(s, (size_t)m->n_demand * T1 * RS, &v.demand)) ||
        (rc = dalloc(s, (size_t)std::max(s->n_over, 1) * RS, &v.ent_p)))  // probabilities that do not fit a node's LDS rows
      return rc;
    for (int k = 0; k < 2; ++k)
      if ((rc = dalloc(s, (size_t)std::max(m->n_turns, 1) * RS, &v.tfd[k]))) return rc;
    if ((rc = dalloc(s, (size_t)m->n_pair * T1, &s->d_pair_pod))) return rc;
    v.pair_pod = s->d_pair_pod;
    if ((rc = dalloc(s, (size_t)std::max(m->n_turns, 1) * T1, &s->d_turn_tab))) return rc;
    v.turn_tab = s->d_turn_tab;
    HIP_TRY(s, hipMemset(s->d_turn_tab, 0, (size_t)std::max(m->n_turns, 1) * T1 * sizeof(double)));
    if ((rc = dalloc(s, RS, &v.flags)) || (rc = dalloc(s, 4, &s->d_clock))) return rc;
    HIP_TRY(s, hipMemset(s->d_clock, 0, 4 * sizeof(int32_t)));
    v.clock = s->d_clock;
  }
  {  // initial widths, turning fractions, demand (broadcast to every replica)
    const double* w0[3] = {m->front_gate0, m->back_gate0, m->sep_width0};
    double* dst[3] = {v.front, v.back, v.sepw};
    for (int k = 0; k < 3; ++k)
      if ((rc = push_rows(s, dst[k], w0[k], L, 0, 1, PEDN_ALL))) return rc;
    if ((rc = push_rows(s, v.tf, m->tf_init, m->n_turns, 0, 1, PEDN_ALL)) || (rc = push_rows(s, v.demand, m->demand, m->n_demand * v.T1, 0, 1, PEDN_ALL)))
      return rc;
    HIP_TRY(s, hipMemsetAsync(v.ent_p, 0, (size_t)std::max(s->n_over, 1) * v.RS * 8, s->stream));
    for (int k = 0; k < 2; ++k) HIP_TRY(s, hipMemsetAsync(v.tfd[k], 0, (size_t)std::max(m->n_turns, 1) * v.RS * 8, s->stream));
    // replica-uniform shortcuts: everything starts uniform; dynamic nodes always use their per-replica rows
    const double qnan = __builtin_nan("");
    s->h_front_u.assign(m->front_gate0, m->front_gate0 + L);
    s->h_back_u.assign(m->back_gate0, m->back_gate0 + L);
    s->h_tf_u.assign(m->tf_init, m->tf_init + m->n_turns);
    s->h_node_dyn.assign(m->node_dyn, m->node_dyn + N);
    for (int n = 0; n < N; ++n)
      if (m->node_dyn[n])
        for (int k = m->node_turn_ptr[n]; k < m->node_turn_ptr[n + 1]; ++k) s->h_tf_u[k] = qnan;
    if ((rc = dalloc(s, (size_t)L, &s->d_front_u)) || (rc = dalloc(s, (size_t)L, &s->d_back_u)) || (rc = dalloc(s, (size_t)m->n_turns, &s->d_tf_u))) return rc;
    v.front_u = s->d_front_u; v.back_u = s->d_back_u; v.tf_u = s->d_tf_u;
    if ((rc = push_uniform(s)) || (rc = tabulate_pair_pod(s))) return rc;
  }
  if ((rc = reset_state(s))) return rc;
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  if (s->chains > 1) {   // the chains the plan wants: as far as their streams are seen to overlap
    int got = 1;
    if ((rc = warm_chain_streams(s, &got))) return rc;
    s->chains = s->warmed_chains = got;
    if (s->d_live_rec && (rc = warm_third_stream(s))) return rc;
    prewarm_chains(s);
  }
  *out = guard.release();
  return PEDN_OK;
}

int pedn_destroy(pedn_sim* s) {
  if (!s) return PEDN_OK;
  hipSetDevice(s->device);
  if (s->clocked) hipDeviceSynchronize();   // clocked steps may still run on a caller's stream (or in a graph being replayed there)
  if (s->stream3) hipStreamSynchronize(s->stream3);
  if (s->stream2) hipStreamSynchronize(s->stream2);
  if (s->stream) hipStreamSynchronize(s->stream);
  metrics_free(s);
  store_drop(s->ro);
  store_drop(s->rp);
  for (void* p : s->allocs) hipFree(p);
  if (s->rl_pin) hipHostFree(s->rl_pin);
  for (pedn_sim::Stage& st : s->stage) {
    if (st.dev) hipFree(st.dev);
    if (st.pin) hipHostFree(st.pin);
    if (st.done) hipEventDestroy(st.done);
  }
  if (s->ev0) hipEventDestroy(s->ev0);
  if (s->ev1) hipEventDestroy(s->ev1);
  if (s->stream2) hipStreamDestroy(s->stream2);
  if (s->stream3) hipStreamDestroy(s->stream3);
  if (s->ev_join3) hipEventDestroy(s->ev_join3);
  if (s->ev_fork) hipEventDestroy(s->ev_fork);
  if (s->ev_join) hipEventDestroy(s->ev_join);
  if (s->stream) hipStreamDestroy(s->stream);
  delete s;
  return PEDN_OK;
}

// what both resets do in front of clearing the state (which takes the marks back to "nothing has run": reset_full / reset_lazy)
static int reset_bookkeeping(pedn_sim* s) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  HIP_TRY(s, hipSetDevice(s->device));
  join_forked(s);
  return norm_reset_returns(s);
}

int pedn_reset(pedn_sim* s) {
  const int rc = reset_bookkeeping(s);
  return rc != PEDN_OK ? rc : reset_state(s);
}
int pedn_reset_lazy(pedn_sim* s) {
  const int rc = reset_bookkeeping(s);
  return rc != PEDN_OK ? rc : reset_state_lazy(s);
}

// dead links: an upload into demand row `row` -- the host looks at the values (outside any step): a row that may now hold anything but
// +0.0 is a source of the proof; all = the upload replaces the whole row in every replica
static void dl_demand_upload(pedn_sim* s, int row, const double* values, size_t n, bool all) {
  char nz = 0;
  for (size_t i = 0; i < n && !nz; ++i) nz = pedn_part::not_plus_zero(values[i]);
  const char now = all ? nz : (char)(s->h_demand_nz[row] | nz);
  if (now != s->h_demand_nz[row]) { s->h_demand_nz[row] = now; s->dl_dirty = true; }
}

// values (host) -> rows of a [rows][RS] device array, one replica or all
static int push_rows(pedn_sim* s, double* dst, const double* values, int n_rows, size_t row0, size_t row_stride, int replica) {
  if (n_rows <= 0) return PEDN_OK;
  DevView& v = s->v;
  if (replica != PEDN_ALL && (replica < 0 || replica >= v.R)) return fail(s, PEDN_E_ARG, "replica out of range");
  HIP_TRY(s, hipSetDevice(s->device));
  join_forked(s);       // every setter that goes through here (demand, turning fractions, widths) is ordered behind both chains
  pedn_sim::Stage* st;
  int rc = stage_acquire(s, (size_t)n_rows * 8, &st);
  if (rc != PEDN_OK || (rc = stage_upload(s, st, values, (size_t)n_rows * 8)) != PEDN_OK) return rc;
  int r0 = replica == PEDN_ALL ? 0 : replica, r1 = replica == PEDN_ALL ? v.RS : replica + 1;
  size_t n = (size_t)n_rows * (r1 - r0);
  hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, dst, (const double*)st->dev, n_rows,
                     row0, row_stride, v.RS, r0, r1, 0, 1);
  HIP_TRY(s, hipGetLastError());
  return stage_commit(s, st);
}

int pedn_set_demand(pedn_sim* s, int32_t node, int32_t replica, const double* values, int32_t n) {
  if (!s || !values) return fail(s, PEDN_E_ARG, "null argument");
  if (node < 0 || node >= s->n_nodes) return fail(s, PEDN_E_ARG, "node out of range");
  int row = s->node_demand_row[node];
  if (row < 0) return fail(s, PEDN_E_ARG, "node has no virtual (origin/destination) link");
  std::vector<double> full(s->v.T1, 0.0);  // copied into the pinned staging buffer before push_rows returns
  for (int i = 0; i < n && i < s->v.T1; ++i) full[i] = values[i];
  dl_demand_upload(s, row, full.data(), full.size(), replica == PEDN_ALL);
  return push_rows(s, s->v.demand, full.data(), s->v.T1, (size_t)row * s->v.T1, 1, replica);
}

int pedn_get_demand(pedn_sim* s, int32_t node, int32_t replica, double* values, int32_t n) {
  if (!s || !values) return fail(s, PEDN_E_ARG, "null argument");
  if (node < 0 || node >= s->n_nodes) return fail(s, PEDN_E_ARG, "node out of range");
  const int row = s->node_demand_row[node];
  if (row < 0) return fail(s, PEDN_E_ARG, "node has no virtual (origin/destination) link");
  DevView& v = s->v;
  if (replica < 0 || replica >= v.R) return fail(s, PEDN_E_ARG, "replica out of range");
  if (n < 0 || n > v.T1) return fail(s, PEDN_E_ARG, "more values than time indices");
  if (n == 0) return PEDN_OK;
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  HIP_TRY(s, hipMemcpy2D(values, 8, v.demand + (size_t)row * v.T1 * v.RS + replica, (size_t)v.RS * 8, 8, n, hipMemcpyDeviceToHost));
  return PEDN_OK;
}

int pedn_set_demand_matrix(pedn_sim* s, int32_t node, const double* values, int32_t n) {
  if (!s || !values) return fail(s, PEDN_E_ARG, "null argument");
  if (node < 0 || node >= s->n_nodes) return fail(s, PEDN_E_ARG, "node out of range");
  const int row = s->node_demand_row[node];
  if (row < 0) return fail(s, PEDN_E_ARG, "node has no virtual (origin/destination) link");
  DevView& v = s->v;
  if (n < 0 || n > v.T1) return fail(s, PEDN_E_ARG, "more demand values than time indices");
  if (n == 0) return PEDN_OK;
  dl_demand_upload(s, row, values, (size_t)v.R * n, false);
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  const size_t bytes = (size_t)v.R * n * 8;
  pedn_sim::Stage* st;
  int rc = stage_acquire(s, bytes, &st);
  if (rc != PEDN_OK || (rc = stage_upload(s, st, values, bytes)) != PEDN_OK) return rc;
  const size_t lanes = (size_t)v.T1 * v.RS;
  hipLaunchKernelGGL(demand_matrix_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s->stream, v.demand, (const double*)st->dev,
                     (size_t)row, n, v.T1, v.R, v.RS);
  HIP_TRY(s, hipGetLastError());
  return stage_commit(s, st);
}

int pedn_set_demand_rows(pedn_sim* s, int32_t node, const int32_t* replicas, int32_t n_rep, const double* values, int32_t n) {
  if (!s || !values || !replicas) return fail(s, PEDN_E_ARG, "null argument");
  if (node < 0 || node >= s->n_nodes) return fail(s, PEDN_E_ARG, "node out of range");
  const int row = s->node_demand_row[node];
  if (row < 0) return fail(s, PEDN_E_ARG, "node has no virtual (origin/destination) link");
  DevView& v = s->v;
  if (n < 0 || n > v.T1) return fail(s, PEDN_E_ARG, "more demand values than time indices");
  for (int k = 0; k < n_rep; ++k)
    if (replicas[k] < 0 || replicas[k] >= v.R) return fail(s, PEDN_E_ARG, "replica out of range");
  if (n == 0 || n_rep <= 0) return PEDN_OK;
  dl_demand_upload(s, row, values, (size_t)n_rep * n, false);
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  // staging layout: values [n_rep][n] (f64), then the replica ids (int32)
  const size_t vbytes = (size_t)n_rep * n * 8, bytes = vbytes + (size_t)n_rep * 4;
  pedn_sim::Stage* st;
  int rc = stage_acquire(s, bytes, &st);
  if (rc != PEDN_OK || (rc = stage_upload(s, st, values, vbytes)) != PEDN_OK || (rc = stage_upload(s, st, replicas, (size_t)n_rep * 4, vbytes)) != PEDN_OK)
    return rc;
  const size_t lanes = (size_t)v.T1 * n_rep;
  hipLaunchKernelGGL(demand_rows_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s->stream, v.demand, (const double*)st->dev,
                     (const int32_t*)((const char*)st->dev + vbytes), n_rep, (size_t)row, n, v.T1, v.RS);
  HIP_TRY(s, hipGetLastError());
  return stage_commit(s, st);
}

int pedn_draw_demand(pedn_sim* s, int32_t node, uint64_t seed, const int32_t* pattern, const double* base, const double* peak,
                     const int32_t* spike_start, const int32_t* spike_len, const double* spike_height) {
  if (!s || !pattern || !base || !peak || !spike_start || !spike_len || !spike_height) return fail(s, PEDN_E_ARG, "null argument");
  if (node < 0 || node >= s->n_nodes) return fail(s, PEDN_E_ARG, "node out of range");
  const int row = s->node_demand_row[node];
  if (row < 0) return fail(s, PEDN_E_ARG, "node has no virtual (origin/destination) link");
  DevView& v = s->v;
  for (int r = 0; r < v.R; ++r) {
    if (pattern[r] < 0 || pattern[r] > 2) return fail(s, PEDN_E_ARG, "demand pattern outside 0..2");
    if (!(base[r] >= 0.0) || !(peak[r] >= 0.0) || base[r] + 2.0 * peak[r] > 500.0) return fail(s, PEDN_E_ARG, "demand rate outside [0, 500]");
  }
  if (!s->h_demand_nz[row]) { s->h_demand_nz[row] = 1; s->dl_dirty = true; }   // dead links: a row drawn on the device counts as non-zero
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  // staging layout: pattern, spike_start, spike_len (int32 [R] each, padded to 8 bytes), then base, peak, spike_height (f64 [R])
  const size_t R = (size_t)v.R, ioff = ((3 * R * 4 + 7) / 8) * 8, bytes = ioff + 3 * R * 8;
  pedn_sim::Stage* st;
  int rc = stage_acquire(s, bytes, &st);
  if (rc != PEDN_OK) return rc;
  unsigned char* h = (unsigned char*)st->pin;
  memcpy(h, pattern, R * 4);
  memcpy(h + R * 4, spike_start, R * 4);
  memcpy(h + 2 * R * 4, spike_len, R * 4);
  memcpy(h + ioff, base, R * 8);
  memcpy(h + ioff + R * 8, peak, R * 8);
  memcpy(h + ioff + 2 * R * 8, spike_height, R * 8);
  HIP_TRY(s, hipMemcpyAsync(st->dev, st->pin, bytes, hipMemcpyHostToDevice, s->stream));
  const unsigned char* d = (const unsigned char*)st->dev;
  const size_t lanes = (size_t)v.T1 * v.RS;
  hipLaunchKernelGGL(draw_demand_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s->stream, v.demand, (size_t)row, v.T1, v.R,
                     v.RS, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), v.replica_offset, (uint32_t)node,
                     (const int32_t*)d, (const double*)(d + ioff), (const double*)(d + ioff + R * 8), (const int32_t*)(d + R * 4),
                     (const int32_t*)(d + 2 * R * 4), (const double*)(d + ioff + 2 * R * 8));
  HIP_TRY(s, hipGetLastError());
  return stage_commit(s, st);
}

int pedn_set_od_weights(pedn_sim* s, int32_t od, const double* values, int32_t n) {
  if (!s || !values) return fail(s, PEDN_E_ARG, "null argument");
  if (od < 0 || od >= s->n_od || n != s->v.T1) return fail(s, PEDN_E_ARG, "od index or length out of range");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  HIP_TRY(s, hipMemcpy((void*)(s->v.od_w + (size_t)od * s->v.T1), values, (size_t)n * 8, hipMemcpyHostToDevice));
  std::copy(values, values + n, s->h_od_w.begin() + (size_t)od * s->v.T1);
  pedn_plan::fractions_invalid(s->marks);  // fractions of the next step may already sit in tfd, computed with the old weights
  return tabulate_pair_pod(s);
}

int pedn_set_turning_fractions(pedn_sim* s, int32_t node, int32_t replica, const double* tf, int32_t n) {
  if (!s || !tf) return fail(s, PEDN_E_ARG, "null argument");
  if (node < 0 || node >= s->n_nodes) return fail(s, PEDN_E_ARG, "node out of range");
  int a = s->node_turn_ptr[node], b = s->node_turn_ptr[node + 1];
  if (n != b - a) return fail(s, PEDN_E_ARG, "turning-fraction count does not match m(m-1)");
  int rc = push_rows(s, s->v.tf, tf, n, (size_t)a, 1, replica);
  if (rc != PEDN_OK) return rc;
  s->dl_dirty = true;
  // a dynamic node recomputes its fractions every step (network.py:272-275); until then a read returns what was imposed
  s->h_tf_set_epoch[node] = s->marks.step_epoch;
  // (the imposed values go into the buffer of the last step too, see below: a REPEAT of that step must recompute them, not take them
  // for its own -- under the single-launch plan tp_ready names that very step; found by tools/gpu_fuzz_plans.py)
  if (s->h_node_dyn[node]) pedn_plan::fractions_invalid(s->marks);
  if (s->h_node_dyn[node] && s->marks.last_t >= 0 && (rc = push_rows(s, s->v.tfd[s->marks.last_t & 1], tf, n, (size_t)a, 1, replica)) != PEDN_OK) return rc;
  for (int k = 0; k < n; ++k)
    s->h_tf_u[a + k] = (replica == PEDN_ALL && !s->h_node_dyn[node]) ? tf[k] : __builtin_nan("");
  return push_uniform(s);
}

int pedn_get_turning_fractions(pedn_sim* s, int32_t node, int32_t replica, double* tf, int32_t n) {
  if (!s || !tf) return fail(s, PEDN_E_ARG, "null argument");
  if (node < 0 || node >= s->n_nodes) return fail(s, PEDN_E_ARG, "node out of range");
  if (replica < 0 || replica >= s->v.R) return fail(s, PEDN_E_ARG, "replica out of range");
  int a = s->node_turn_ptr[node], b = s->node_turn_ptr[node + 1];
  if (n != b - a) return fail(s, PEDN_E_ARG, "turning-fraction count does not match m(m-1)");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  const double* src = (s->h_node_dyn[node] && s->marks.last_t >= 0) ? s->v.tfd[s->marks.last_t & 1] : s->v.tf;
  HIP_TRY(s, hipMemcpy2D(tf, 8, src + (size_t)a * s->v.RS + replica, (size_t)s->v.RS * 8, 8, n, hipMemcpyDeviceToHost));
  if (s->v.pod_pr && s->ttab_r_stale) {  // the per-replica tables were derived on the device: fetch the host copy once
    s->h_ttab_r.assign((size_t)std::max(s->n_turns, 1) * s->v.R, 0.0);
    HIP_TRY(s, hipMemcpy2D(s->h_ttab_r.data(), (size_t)s->v.R * 8, s->d_turn_tab_r, (size_t)s->v.RS * 8, (size_t)s->v.R * 8, std::max(s->n_turns, 1), hipMemcpyDeviceToHost));
    s->ttab_r_stale = false;
  }
  if (s->h_node_dyn[node] && s->marks.last_t >= 0 && s->h_tf_set_epoch[node] != s->marks.step_epoch) {  // rows tabulated on the host (SlotRec.dyn == 2)
    const int s0 = s->h_node_slot_ptr[node], d = s->h_node_slot_ptr[node + 1] - s0;
    for (int i = 0; i < d; ++i)
      if (s->h_slot_dyn[s0 + i] == 2)
        for (int jj = 0; jj < d - 1; ++jj) {
          const int tn = a + i * (d - 1) + jj;
          tf[tn - a] = s->v.pod_pr ? s->h_ttab_r[(size_t)tn * s->v.R + replica] : s->h_ttab[(size_t)s->marks.last_t * s->n_turns + tn];
        }
  }
  return PEDN_OK;
}

int pedn_set_width(pedn_sim* s, int32_t which, int32_t link, int32_t replica, double value) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (link < 0 || link >= s->v.L || which < 0 || which > 3) return fail(s, PEDN_E_ARG, "link or selector out of range");
  if (replica != PEDN_ALL && (replica < 0 || replica >= s->v.R)) return fail(s, PEDN_E_ARG, "replica out of range");
  double* dst = which == PEDN_W_FRONT ? s->v.front : which == PEDN_W_BACK ? s->v.back : which == PEDN_W_SEP ? s->v.sepw : s->v.sepnp;
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);     // the link update records the gate / reads the separator width of its own step
  s->dl_dirty = true;
  if (which == PEDN_W_BACK) pedn_plan::fractions_invalid(s->marks);  // capacity fallback of the turn probabilities (path_finder.py:575-576)
  join_forked(s);   // (as every setter: ordered behind both chains)
  // one launch, its values as kernel arguments: the row's replicas and the link's entry of the replica-uniform shortcut (front_u / back_u:
  // NaN = "differs between replicas"; a link the RL agents write per replica keeps NaN, push_uniform)
  double* uni = nullptr;
  double uval = 0.0;
  if (which <= PEDN_W_BACK) {
    std::vector<double>& hu = which == PEDN_W_FRONT ? s->h_front_u : s->h_back_u;
    hu[link] = replica == PEDN_ALL ? value : __builtin_nan("");
    uval = (link < (int)s->h_rl_link.size() && s->h_rl_link[link]) ? __builtin_nan("") : hu[link];
    uni = (which == PEDN_W_FRONT ? s->d_front_u : s->d_back_u) + link;
  }
  const int r0 = replica == PEDN_ALL ? 0 : replica, n = replica == PEDN_ALL ? s->v.RS : 1;
  hipLaunchKernelGGL(set_width_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, dst + (size_t)link * s->v.RS, r0, n, value, uni, uval);
  HIP_TRY(s, hipGetLastError());
  return PEDN_OK;
}

int pedn_set_widths(pedn_sim* s, int32_t which, const double* values) {
  if (!s || !values) return fail(s, PEDN_E_ARG, "null argument");
  if (which < 0 || which > 3) return fail(s, PEDN_E_ARG, "selector out of range");
  DevView& v = s->v;
  if (which == PEDN_W_BACK) pedn_plan::fractions_invalid(s->marks);
  if (v.L == 0) return PEDN_OK;
  double* dst = which == PEDN_W_FRONT ? v.front : which == PEDN_W_BACK ? v.back : which == PEDN_W_SEP ? v.sepw : v.sepnp;
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  s->dl_dirty = true;
  size_t bytes = (size_t)v.L * v.R * 8;
  pedn_sim::Stage* st;
  int rc = stage_acquire(s, bytes, &st);
  if (rc != PEDN_OK || (rc = stage_upload(s, st, values, bytes)) != PEDN_OK) return rc;
  size_t n = (size_t)v.L * v.R;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, dst, (const double*)st->dev, v.L,
                     (size_t)0, (size_t)1, v.RS, 0, v.R, 1, v.R);
  HIP_TRY(s, hipGetLastError());
  if ((rc = stage_commit(s, st)) != PEDN_OK) return rc;
  if (which <= PEDN_W_BACK) {
    std::vector<double>& u = which == PEDN_W_FRONT ? s->h_front_u : s->h_back_u;
    for (int l = 0; l < v.L; ++l) {
      bool same = true;
      for (int r = 1; r < v.R && same; ++r) same = values[(size_t)l * v.R + r] == values[(size_t)l * v.R];
      u[l] = same ? values[(size_t)l * v.R] : __builtin_nan("");
    }
    return push_uniform(s);
  }
  return PEDN_OK;
}

int pedn_reset_widths(pedn_sim* s, const double* front, const double* back, const double* sep) {
  if (!s || !front || !back || !sep) return fail(s, PEDN_E_ARG, "null argument");
  DevView& v = s->v;
  pedn_plan::fractions_invalid(s->marks);
  if (v.L == 0) return PEDN_OK;
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  s->dl_dirty = true;
  int rc;
  if ((rc = push_rows(s, v.front, front, v.L, 0, 1, PEDN_ALL)) || (rc = push_rows(s, v.back, back, v.L, 0, 1, PEDN_ALL)) ||
      (rc = push_rows(s, v.sepw, sep, v.L, 0, 1, PEDN_ALL)))
    return rc;
  HIP_TRY(s, hipMemsetAsync(v.sepnp, 0, (size_t)v.L * v.RS * sizeof(double), s->stream));
  s->h_front_u.assign(front, front + v.L);
  s->h_back_u.assign(back, back + v.L);
  return push_uniform(s);
}

int pedn_get_widths(pedn_sim* s, int32_t which, double* values) {
  if (!s || !values) return fail(s, PEDN_E_ARG, "null argument");
  if (which < 0 || which > 3) return fail(s, PEDN_E_ARG, "selector out of range");
  DevView& v = s->v;
  if (v.L == 0) return PEDN_OK;
  const double* src = which == PEDN_W_FRONT ? v.front : which == PEDN_W_BACK ? v.back : which == PEDN_W_SEP ? v.sepw : v.sepnp;
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  HIP_TRY(s, hipMemcpy2D(values, (size_t)v.R * 8, src, (size_t)v.RS * 8, (size_t)v.R * 8, v.L, hipMemcpyDeviceToHost));
  return PEDN_OK;
}

// Row bases of a node-kernel launch of step t (DevView.rb, node_step): the rows of t, t - 1, t - 2 (wrapped as wrap_idx does) and
// t - 1 - W of the fields node_step addresses at a row every wave shares, mapped to their place in a full record or a ring as R64 / R32
// do in the kernels.  A row the step cannot touch (t - 1 - W < 0: the window has not filled, t - 2 of a step the LU kernel never runs) gets
// the field's first row.  Called when vn.quiet is what the launch will carry: quiet_rd / quiet_wr are the halves of steps t - 1 and t.
static void row_bases(DevView& vn, int t) {
  const size_t n64 = (size_t)vn.L * vn.RS, n64a = (size_t)vn.Lall * vn.RS;   // elements of a row: inflow .. cumulative_outflow hold the virtual links too
  auto wrap = [&](int i) { if (i < 0) i += vn.T1; return i < 0 || i >= vn.T1 ? 0 : i; };
  auto r64 = [&](int F, int i) { return (char*)(vn.f64[F] + (size_t)(vn.hist ? (i & vn.m64[F]) : i) * (F < F_S ? n64a : n64)); };
  auto r32 = [&](int G, int i) { return (char*)(vn.f32[G] + (size_t)(vn.hist ? (i & vn.m32[G]) : i) * n64); };
  const int tp = wrap(t - 1), tq = wrap(t - 2), tw = t - 1 - vn.W >= 0 ? wrap(t - 1 - vn.W) : 0, tt = wrap(t);
  vn.rb[RB_IN_P] = r64(F_IN, tp); vn.rb[RB_IN_T] = r64(F_IN, tt);
  vn.rb[RB_OUT_P] = r64(F_OUT, tp); vn.rb[RB_OUT_T] = r64(F_OUT, tt);
  vn.rb[RB_CI_P] = r64(F_CI, tp); vn.rb[RB_CI_T] = r64(F_CI, tt);
  vn.rb[RB_CO_P] = r64(F_CO, tp); vn.rb[RB_CO_T] = r64(F_CO, tt);
  vn.rb[RB_S_Q] = r64(F_S, tq); vn.rb[RB_S_P] = r64(F_S, tp);
  vn.rb[RB_R_Q] = r64(F_R, tq); vn.rb[RB_R_P] = r64(F_R, tp);
  vn.rb[RB_GATE_P] = r64(F_GATE, tp);
  vn.rb[RB_N_Q] = r32(G_N, tq); vn.rb[RB_N_P] = r32(G_N, tp);
  vn.rb[RB_K_P] = r32(G_K, tp); vn.rb[RB_V_P] = r32(G_V, tp); vn.rb[RB_TT_P] = r32(G_TT, tp);
  vn.rb[RB_LF_P] = r32(G_LF, tp); vn.rb[RB_ATT_P] = r32(G_ATT, tp);
  vn.rb[RB_TT_W] = r32(G_TT, tw);
  const size_t half = (size_t)vn.quiet_npos * (size_t)(vn.RS / 64) * 2;   // [slot position][replica group][own | inbox] of one step
  vn.quiet_rd = vn.quiet ? vn.quiet + (size_t)((t - 1) & 1) * half : nullptr;
  vn.quiet_wr = vn.quiet ? vn.quiet + (size_t)(t & 1) * half : nullptr;
}

// lu: the instantiation whose slot waves perform the link update of step t-1 themselves (node_kernel<..., LU = true>)
// tf: ... and compute their own rows of turning fractions (node_kernel<.., TF> / with helper waves node_kernel_h)
static step_kernel_fn node_kernel_for(const pedn_sim* s, bool lu, bool tf) {
  const bool h = s->v.hist != 0;  // recent-history mode: the instantiations that mask the history rows
  const bool d6 = s->max_degree <= 6;  // loops and the row of turning fractions unrolled for 6 instead of 8 corridors per node
#define PEDN_NK(PR_, LP_, LU_, TF_) (h ? (d6 ? node_kernel<PR_, LP_, true, 6, LU_, TF_> : node_kernel<PR_, LP_, true, 8, LU_, TF_>) \
                                       : (d6 ? node_kernel<PR_, LP_, false, 6, LU_, TF_> : node_kernel<PR_, LP_, false, 8, LU_, TF_>))
  if (s->plan.node_lp) return s->v.pr ? PEDN_NK(true, true, false, false) : PEDN_NK(false, true, false, false);
  if (lu && tf && s->plan.inline_help) {   // helper waves compute the rows: sixteen waves per workgroup
    if (s->v.pr) return h ? (d6 ? node_kernel_h<true, true, 6> : node_kernel_h<true, true, 8>) : (d6 ? node_kernel_h<true, false, 6> : node_kernel_h<true, false, 8>);
    return h ? (d6 ? node_kernel_h<false, true, 6> : node_kernel_h<false, true, 8>) : (d6 ? node_kernel_h<false, false, 6> : node_kernel_h<false, false, 8>);
  }
  if (lu && tf) return s->v.pr ? PEDN_NK(true, false, true, true) : PEDN_NK(false, false, true, true);
  if (lu) return s->v.pr ? PEDN_NK(true, false, true, false) : PEDN_NK(false, false, true, false);
  return s->v.pr ? PEDN_NK(true, false, false, false) : PEDN_NK(false, false, false, false);
#undef PEDN_NK
}

// the node kernel of a clocked env step (pedn_rl_step_clocked): the step index comes from DevView.clock
static step_kernel_fn clocked_node_kernel_for(const pedn_sim* s) {
  const bool h = s->v.hist != 0, d6 = s->max_degree <= 6;
#define PEDN_NKC(PR_) (h ? (d6 ? node_kernel<PR_, false, true, 6, false, false, true> : node_kernel<PR_, false, true, 8, false, false, true>) \
                         : (d6 ? node_kernel<PR_, false, false, 6, false, false, true> : node_kernel<PR_, false, false, 8, false, false, true>))
  return s->v.pr ? PEDN_NKC(true) : PEDN_NKC(false);   // (not built for the node LP: pedn_rl_clock_begin refuses)
#undef PEDN_NKC
}

// the other step kernels, by the view's per-replica link parameters (pr) and recent-history mode (hist)
static step_kernel_fn turn_frac_kernel_for(const DevView& v) {
  if (v.pr) return v.hist ? turn_frac_kernel<true, true> : turn_frac_kernel<true, false>;
  return v.hist ? turn_frac_kernel<false, true> : turn_frac_kernel<false, false>;
}
static step_kernel_fn link_kernel_1r_for(const DevView& v) {
  if (v.pr) return v.hist ? link_kernel_1r<true, true> : link_kernel_1r<true, false>;
  return v.hist ? link_kernel_1r<false, true> : link_kernel_1r<false, false>;
}
// obs: the observations ride in the launch; clk: the launch of a clocked env step (it always observes)
typedef void (*link_turn_kernel_fn)(DevView, int, unsigned, unsigned, unsigned, RlView, int);
static link_turn_kernel_fn link_turn_kernel_for(const DevView& v, bool obs, bool clk) {
#define PEDN_LTK(OBS_, CLK_) (v.pr ? (v.hist ? link_turn_kernel<true, OBS_, true, CLK_> : link_turn_kernel<true, OBS_, false, CLK_>) \
                                   : (v.hist ? link_turn_kernel<false, OBS_, true, CLK_> : link_turn_kernel<false, OBS_, false, CLK_>))
  if (clk) return PEDN_LTK(true, true);
  return obs ? PEDN_LTK(true, false) : PEDN_LTK(false, false);
#undef PEDN_LTK
}
// the controller twins (pedn_ctrl.hpp)
typedef void (*ctrl_link_turn_kernel_fn)(DevView, int, unsigned, unsigned, unsigned, RlView, int, CtrlView);
static ctrl_link_turn_kernel_fn ctrl_link_turn_kernel_for(const DevView& v) {
  if (v.pr) return v.hist ? ctrl_link_turn_kernel<true, true> : ctrl_link_turn_kernel<true, false>;
  return v.hist ? ctrl_link_turn_kernel<false, true> : ctrl_link_turn_kernel<false, false>;
}
// (the observations as a launch of their own: the plain kernel and its twin differ in their arguments, so a selector each)
typedef void (*rl_observe_kernel_fn)(DevView, RlView, int, int);
static rl_observe_kernel_fn rl_observe_kernel_for(const DevView& v) { return v.hist ? rl_observe_kernel<true> : rl_observe_kernel<false>; }
typedef void (*ctrl_observe_kernel_fn)(DevView, RlView, int, int, CtrlView);
static ctrl_observe_kernel_fn ctrl_observe_kernel_for(const DevView& v) { return v.hist ? ctrl_observe_kernel<true> : ctrl_observe_kernel<false>; }

// The link update of step t as a launch of its own (the second launch of a step of a model without dynamic turning fractions, and
// the flush of a pending update under the owner-wave plan): one replica per lane.  e >= 0: start / stop events ev[e], ev[e + 1].
static unsigned link_blocks(const DevView& v, bool one_r) {
  return v.n_pairs_corr > 0 ? (unsigned)(((size_t)v.n_pairs_corr * (one_r ? v.subRS : v.subRS / 2) + 255) / 256) : 0u;
}
static void launch_link_update(pedn_sim* s, const DevView& v, hipStream_t stream, int t, hipEvent_t* ev, int e) {
  auto launch = [&](auto kernel, dim3 grid, dim3 block, auto... args) {
    if (ev) hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, ev[e], ev[e + 1], 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
  };
  const unsigned nlb = link_blocks(v, true);
  if (nlb == 0) return;
  launch(link_kernel_1r_for(v), dim3(nlb), dim3(256), v, t);
}

// Workgroups of a step's launches for the share of the batch that v is (view_of): rgroups groups of 64 replicas; tf_blocks: a wave per (row
// of a dynamic node, 64 replicas), four to a workgroup.  The second launch (link_turn_kernel and its twins) is nlb workgroups of link update,
// ntb of the turning fractions of t + 1 (fused; nth of them heavy rows, run in front of the link update), nob of observations (one per agent).
struct StepGrid {
  unsigned rgroups, nlb, ntb, nth, nob;
  StepGrid(const pedn_sim* s, const DevView& v, unsigned link_blocks_, bool fused, bool obs)
      : rgroups((unsigned)(v.subRS / 64)), nlb(link_blocks_), ntb(fused ? tf_blocks(v) : 0u),
        nth(fused ? (unsigned)s->n_tf_heavy_quads * rgroups : 0u), nob(obs ? (unsigned)s->rl.n_agents * rgroups : 0u) {}
  unsigned tf_blocks(const DevView& v) const { return (unsigned)((v.n_trow + 3) / 4) * rgroups; }
  dim3 second() const { return dim3(nlb + ntb + nob); }
};

// this launch's share of the batch: the whole of it on the engine's stream (half = -1) or one half of the replicas per stream
// (half = index of the chain, 0 or 1: each steps its share of the replicas on its own stream)
static DevView view_of(const pedn_sim* s, int half, hipStream_t* stream) {
  DevView v = s->v;
  *stream = s->stream;
  if (half >= 0) {
    // RS is a multiple of 128 (a wave of link_body covers 128 replicas): when the 128-replica segments do not halve, chain 0 takes one more
    const int a = ((s->v.RS / 128 + 1) / 2) * 128;
    v.sub0 = half ? a : 0;
    v.subRS = half ? s->v.RS - a : a;
    *stream = chain_stream(s, half);
  }
  return v;
}

// Owner-wave plan: the link update of the last step launched is still to be done (link_pending); do it now.  last: on the last of the
// chains (the others still see the update as pending).
static void flush_links(pedn_sim* s, int half, hipEvent_t* ev, bool last) {
  if (s->marks.link_pending < 0) return;
  hipStream_t stream;
  const DevView v = view_of(s, half, &stream);
  launch_link_update(s, v, stream, s->marks.link_pending, ev, 4);
  if (last) pedn_plan::flushed(s->marks);
  else pedn_plan::touch(s->marks);
}

// Every entry point that looks at or changes what a link update reads or writes calls pending_links_first: under the owner-wave plan the
// link update of the last step launched may still be pending (link_pending) -- the next step's node kernel would perform it.
static int join_chains(pedn_sim* s, int n, int idle = -1);
// (also: pedn_rl_step may have left the two halves of the batch stepping as two chains on two streams across calls -- `forked` -- so
// that the engine's stream does not order stream2's work yet: joined first.  Anything that enqueues on the engine's stream or reads
// device memory calls this, i.e. every entry point but the stepping calls themselves and the pure host getters.)
static inline void join_forked(pedn_sim* s) {
  if (s->clocked) clock_end(s);   // whoever needs the host's view of the state ends a clocked section first (synchronises)
  if (s->forked) {
    s->forked = 0;
    join_chains(s, 2);
  }
}
static inline void pending_links_first(pedn_sim* s) {
  s->touched = 1;
  pedn_plan::touch(s->marks);   // whatever comes next may change a history row or break the chain of node_kernel<LU> launches
  join_forked(s);
  if (s->marks.link_pending >= 0) flush_links(s, -1, nullptr);
}

// The first launch of a kernel on a stream that has not run it yet costs the runtime several tens of microseconds (measured: the first
// two-chain range of a process took 32.6-33.9 us per step over 20 steps, the following ones 29.0-29.3): pay that when the plan is
// chosen.  Every step kernel is launched once on every chain's stream over NOTHING -- node_kernel on the block of idle slot records
// behind the bins (its waves meet at the two barriers and leave), the link update with zero corridors.
static void prewarm_chains(pedn_sim* s) {
  if (s->chains < 2) return;
  DevView v = s->v;
  v.slot_rec = s->d_slot_rec + (size_t)s->n_blocks * 8;   // the idle block
  row_bases(v, 2);
  DevView vl = s->v;
  vl.n_pairs_corr = 0;
  vl.n_trow = 0;
  RlView q{};
  DevView sel = vl;
  sel.pr = 0;   // (what is warmed are the instantiations without per-replica parameters, whatever the engine holds)
  for (int c = 0; c < s->chains; ++c) {
    hipStream_t st = chain_stream(s, c);
    for (int lu = 0; lu < 2; ++lu) hipLaunchKernelGGL(node_kernel_for(s, lu != 0, false), dim3(1, 1), dim3(512), s->plan.node_lds, st, v, 2);
    if (s->plan.inline_tf) hipLaunchKernelGGL(node_kernel_for(s, true, true), dim3(1, 1), dim3(s->plan.inline_help ? 1024 : 512), s->plan.node_lds_tf, st, v, 2);
    hipLaunchKernelGGL(link_turn_kernel_for(sel, false, false), dim3(1), dim3(256), 0, st, vl, 1, 0u, 0u, 0u, q, 0);
    hipLaunchKernelGGL(link_kernel_1r_for(sel), dim3(1), dim3(256), 0, st, vl, 1);
    if (s->stream3) hipLaunchKernelGGL(dead_link_kernel, dim3(1), dim3(256), 0, st, v, 2, (const DeadRec*)s->d_dead_drec, 0);   // (no slot: its waves leave)
    if (s->stream3) hipLaunchKernelGGL(lean_block_kernel, dim3(1), dim3(256), 0, st, v, 2, 1, 0u, 0u, (const DeadRec*)s->d_dead_drec, 0);
  }
  if (s->stream3) {   // the live bins' stream of the dead-link plan
    hipLaunchKernelGGL(node_kernel_for(s, true, false), dim3(1, 1), dim3(512), s->plan.node_lds, s->stream3, v, 2);
    hipStreamSynchronize(s->stream3);
  }
  for (int c = s->chains - 1; c >= 0; --c) hipStreamSynchronize(chain_stream(s, c));
}

// ---- Dead links (pedn_partition.hpp, dead_link_kernel; EnginePlan.dead_links in pedn_plan.hpp)
// The proof, from what the host knows now, and the two things built from it: the records of the dead nodes' slots (dead_link_kernel's
// work list) and a second packing of the live nodes alone for node_kernel<LU>.  Between full resets the set only
// shrinks (dl_grow), and the proof's sources only grow (dl_src, dl_reach).  A live slot whose corridor's other end is a dead slot mirrors ITSELF: its own quiet word fills its inbox -- the
// dead end writes +0.0 only, has no separator and a shock-wave look-back >= 1 (eligibility), which is all the inbox vouches for.
// The lean waves' records (DeadRec) from the slots' SlotRec copies and the shared gates as they stand on the device now: one launch of
// dead_prep_kernel on the engine's stream, behind every setter's launch and in front of the fork of the next split range.  Every run of
// dl_refresh ends here, whether the set of dead nodes changed or not: a shared gate set to another valid width leaves the set as it is.
static int dl_prep(pedn_sim* s) {
  if (s->n_dead_pos <= 0) return PEDN_OK;
  hipLaunchKernelGGL(dead_prep_kernel, dim3((unsigned)((s->n_dead_pos + 63) / 64)), dim3(64), 0, s->stream, s->v, (const SlotRec*)s->d_dead_rec,
                     s->d_dead_drec, s->n_dead_pos);
  HIP_TRY(s, hipGetLastError());
  return PEDN_OK;
}

static int dl_refresh(pedn_sim* s) {
  s->dl_dirty = false;
  if (!s->d_live_rec) return PEDN_OK;
  const DevView& v = s->v;
  const int N = s->n_nodes, L = v.L;
  std::vector<char> tab(std::max(s->n_turns, 1), 1);
  if (!v.pod_pr && (int)s->h_tab_nz.size() >= s->n_turns) tab.assign(s->h_tab_nz.begin(), s->h_tab_nz.end());
  pedn_part::Model pm;
  pm.n_nodes = N; pm.n_links = L;
  pm.node_slot_ptr = s->h_node_slot_ptr.data(); pm.node_turn_ptr = s->node_turn_ptr.data(); pm.node_kind = s->h_node_kind.data();
  pm.node_demand_row = s->node_demand_row.data(); pm.slot_in = s->h_slot_in.data(); pm.slot_out = s->h_slot_out.data();
  pm.link_rev = s->h_link_rev.data(); pm.slot_dyn = s->h_slot_dyn.data(); pm.node_lp = s->plan.node_lp;
  // once a step has run, the sources of the earlier proofs stay sources: their pedestrians may still be on the way
  if (s->marks.dl_grow || s->dl_src.size() != s->h_demand_nz.size() || s->dl_reach.size() != (size_t)std::max(L, 1)) {
    s->dl_src = s->h_demand_nz;
    s->dl_reach.assign(std::max(L, 1), 0);
  } else {
    for (size_t i = 0; i < s->dl_src.size(); ++i) s->dl_src[i] |= s->h_demand_nz[i];
  }
  // A link whose free_flow_tau is 0 is a source of its own: its sending flow of step 1 is smoothed against entry -1 of the history, the
  // untouched tail's -1.0 (link.py:364: floor(0.8 * 0 + 0.2 * -1) = -1 on an empty link), the node hands the negative flow on, and the
  // pedestrians it invents walk on from there (tests/test_gpu_dead_record.py: the oracle of such a link).  A seed of every proof.
  for (const SlotRec& R : s->h_slot_rec)
    if (R.node >= 0 && R.lin < L && R.Pin.fft < 1) s->dl_reach[R.lin] = 1;
  pm.demand_nz = s->dl_src.data(); pm.tf_u = s->h_tf_u.data(); pm.tab_nz = tab.data();
  pm.seed_links = s->dl_reach.data();
  pm.link_sep = s->h_link_sep.data(); pm.link_tau_sw = s->h_link_tau_sw.data();
  pm.front_u = s->h_front_u.data(); pm.back_u = s->h_back_u.data();
  pm.link_rl = s->h_rl_link.size() >= (size_t)L ? s->h_rl_link.data() : nullptr;
  pm.per_replica_params = v.pr != 0 || s->rl_ready;   // (an agent set: its action slots and controllers stay with the node kernel)
  const pedn_part::Result proof = pedn_part::partition(pm);
  std::copy(proof.reach.begin(), proof.reach.end(), s->dl_reach.begin());   // (a superset of the seeds)
  std::vector<char> dead = proof.node_dead;
  if (!s->marks.dl_grow && s->dl_node.size() == dead.size())
    for (int n = 0; n < N; ++n) dead[n] = dead[n] && s->dl_node[n];
  else if (!s->marks.dl_grow) dead.assign(N, 0);
  // the lean waves take both gates of a slot from the replica-uniform shortcuts: a node with a slot whose gates are not shared stays with
  // the node kernel (the proof's eligibility rule says as much for every corridor of a dead node; this is the kernel's own condition)
  for (int n = 0; n < N; ++n)
    for (int k = s->h_node_slot_ptr[n]; dead[n] && k < s->h_node_slot_ptr[n + 1]; ++k) {
      const int lin = s->h_slot_in[k], lout = s->h_slot_out[k];
      if (lin < L && lout < L && (s->h_front_u[lin] != s->h_front_u[lin] || s->h_back_u[lout] != s->h_back_u[lout])) dead[n] = 0;
    }
  if (dead == s->dl_node) return dl_prep(s);
  s->dl_node = dead;
  pedn_plan::dead_set_changed(s->marks);
  // the work list of dead_link_kernel, and the live packing: the full packing's records of the live nodes, first-fit in its order
  const std::vector<SlotRec>& full = s->h_slot_rec;
  std::vector<SlotRec> pos;
  std::vector<int32_t> first(N, -1);
  int n_links = 0;
  for (size_t i = 0; i < full.size(); ++i) {
    if (full[i].node < 0) continue;
    if (full[i].slot == 0) first[full[i].node] = (int32_t)i;
    if (dead[full[i].node]) { pos.push_back(full[i]); n_links += full[i].lin < L; }
  }
  const pedn_compile::Packing live = pedn_compile::pack(s->h_pack_order, s->h_node_slot_ptr.data(), dead.data(), L, true, false,
                                                        [&](int n, int k) { return full[first[n] + k]; });   // (a node's slots are consecutive waves of one block)
  const std::vector<SlotRec>& rec = live.rec;
  s->n_dead_links = n_links;
  s->n_dead_pos = (int)pos.size();
  s->n_live_blocks = live.n_blocks;
  s->live_npos = (int)rec.size();
  s->node_lds_live = (size_t)(8 + live.tiles) * 64 * sizeof(double);
  // every launch that read the old lists was joined into the engine's stream by the pedn_run that made it
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  HIP_TRY(s, hipMemcpy(s->d_live_rec, rec.data(), rec.size() * sizeof(SlotRec), hipMemcpyHostToDevice));
  if (!pos.empty()) HIP_TRY(s, hipMemcpy(s->d_dead_rec, pos.data(), pos.size() * sizeof(SlotRec), hipMemcpyHostToDevice));
  return dl_prep(s);
}

// Does a two-chain range of pedn_run take the split plan now?  Everything the proof and dead_link_kernel do not cover keeps the plan
// off: recent-history mode, the node LP, rows of fractions computed on the device (all three: plan.dead_capable, pedn_plan.hpp),
// per-replica link parameters, an agent set, no third stream that overlaps, a state the host does not follow (dl_off) -- and a model
// without a dead link.
static bool dl_split_ok(pedn_sim* s) {
  if (!s->plan.dead_capable || !s->stream3 || s->marks.dl_off || s->chains < 2 || s->v.pr || s->rl_ready || s->v.n_pairs_corr == 0) return false;
  if (s->dl_dirty && dl_refresh(s) != PEDN_OK) return false;
  return s->n_dead_links > 0;
}

// Dynamic LDS per workgroup (four waves) of dead_link_kernel such that exactly n of them fit a CU's 160 KB, n = 3..7: the SMALLEST such
// size, so that the rest stays free for the live workgroups of node_kernel<LU> (n = 5: 28 160 B each, 23 040 B left; the live packing of
// melbourne asks for 20 480).  In units of 2 560 B, a multiple of both LDS allocation granules in use on CDNA (512 and 1 280 B), so the
// count does not depend on which one the device rounds to: k units with n k <= 64 < (n + 1) k.
static size_t dead_lds_bytes(int n) {
  if (n >= 8) return 0;   // the register budget's own 8 waves per SIMD
  return (size_t)(64 / (n + 1) + 1) * 2560;
}

// a step of the whole batch, or chain c of n, under the plain (lazy = false) or the owner-wave family
static inline pedn_plan::StepRequest step_request(int t, bool lazy, int chain = -1, int n_chains = 1) {
  pedn_plan::StepRequest rq;
  rq.t = t; rq.lazy = lazy; rq.chain = chain; rq.n_chains = n_chains;
  return rq;
}

// One step t >= 2 of a split range: dead_link_kernel for the whole batch on the engine's stream (dead_streams = 2: for each half of the
// replicas on the two chain streams), node_kernel<LU> over the live bins for the whole batch on the third stream; the host's marks
// advance once, as in launch_step.  Proof obligations -- why the
// three launches of a step, and the launches of successive steps on different streams, need no order between them:
//   * the two kinds of wave write disjoint elements: a slot wave of either kernel writes the rows of ITS incoming link (link update,
//     sending flow, outflow / cumulative_outflow), the receiving flow, gate record and inflow / cumulative_inflow of ITS outgoing link,
//     and every physical link is the incoming link of exactly one slot, which one of the two work lists holds;
//   * every element that one kind reads of what the other kind writes is +0.0 in every row since the last full reset: a live slot
//     next to a dead node reads outflow / cumulative_outflow / num_pedestrians of its outgoing link (written by the dead slot: +0.0 by
//     construction), a dead slot takes the inflow / cumulative_inflow that a live slot writes into it as +0.0 without reading them --
//     the link is outside REACH (pedn_partition.hpp), so the node model can only produce +0.0 for it;
//   * the error flags are OR-ed atomically by both; the live waves read them only to decide their quiet word, which selects between
//     two paths that give the same bits;
//   * a block of steps in one lean launch (launch_split_block) reads of its own stream's earlier output only rows that EARLIER launches
//     wrote -- the running sum and receiving_flow[t0 - 2] of the launch before it on its stream (or of the full step in front of the
//     fork), travel_time[t - 1 - W] of a launch before it because a block has at most W steps (pedn_plan::dead_block_len) -- so nothing
//     here depends on which step either stream is in: neither list of obligations above names a step.
static void launch_split_live(pedn_sim* s, const pedn_plan::SplitPlan& p, int t) {
  if (!p.live) return;
  DevView vn = s->v;
  vn.slot_rec = s->d_live_rec;
  vn.quiet = s->d_quiet_live;
  vn.quiet_npos = s->live_npos;
  vn.quiet_use = p.quiet_use;
  vn.quiet_lean = p.quiet_lean ? 1 : 0;
  vn.rl_actions = nullptr;
  vn.zg64 = p.zg64; vn.zg32 = p.zg32;
  row_bases(vn, t);
  hipLaunchKernelGGL(node_kernel_for(s, true, false), dim3((unsigned)(vn.RS / 64), (unsigned)s->n_live_blocks), dim3(512), s->node_lds_live, s->stream3, vn, t);
}
static void launch_split_step(pedn_sim* s, int t) {
  const pedn_plan::SplitPlan p = pedn_plan::plan_split_step(step_caps(s), s->marks, step_request(t, true, -1, s->plan.dead_streams));
  const size_t lds = dead_lds_bytes(s->plan.dead_waves);   // the lean kernel's share of the wave places
  for (int c = 0; c < p.lean_launches; ++c) {
    hipStream_t stream;
    DevView vd = view_of(s, p.lean_launches == 1 ? -1 : c, &stream);
    vd.zg64 = p.zg64; vd.zg32 = p.zg32;
    row_bases(vd, t);
    const unsigned waves = (unsigned)s->n_dead_pos * (unsigned)(vd.subRS / 64);
    if (waves > 0) hipLaunchKernelGGL(dead_link_kernel, dim3((waves + 3) / 4), dim3(256), lds, stream, vd, t, (const DeadRec*)s->d_dead_drec, s->n_dead_pos);
  }
  launch_split_live(s, p, t);
  pedn_plan::commit_split_step(s->marks, p);
  mirror_marks(s);
}

// Steps t .. t + n - 1 of a split range (2 <= n <= min(dead_block, W, PEDN_DEAD_BLOCK_MAX)): ONE launch of lean_block_kernel for all of
// them (dead_streams = 2: one per half) in front of the block's n live launches, which go out step by step exactly as launch_split_step
// sends them.  The planner still plans and commits every STEP: the gates of the lean launch -- bit k: those of step t + k -- are the
// plans' own, taken from a dry run of the same plan / commit pair on a copy of the marks, so that the lean launch can go out first.
static void launch_split_block(pedn_sim* s, int t, int n) {
  const pedn_plan::StepCaps caps = step_caps(s);
  uint32_t zg64m = 0, zg32m = 0;
  int lean_launches = 1;
  pedn_plan::StepState dry = s->marks;
  for (int k = 0; k < n; ++k) {
    const pedn_plan::SplitPlan p = pedn_plan::plan_split_step(caps, dry, step_request(t + k, true, -1, s->plan.dead_streams));
    zg64m |= (uint32_t)(p.zg64 != 0) << k;
    zg32m |= (uint32_t)(p.zg32 != 0) << k;
    lean_launches = p.lean_launches;
    pedn_plan::commit_split_step(dry, p);
  }
  const size_t lds = dead_lds_bytes(s->plan.dead_block_waves);   // the block kernel's own share of the wave places
  for (int c = 0; c < lean_launches; ++c) {
    hipStream_t stream;
    DevView vd = view_of(s, lean_launches == 1 ? -1 : c, &stream);
    row_bases(vd, t);
    const unsigned waves = (unsigned)s->n_dead_pos * (unsigned)(vd.subRS / 64);
    if (waves > 0) hipLaunchKernelGGL(lean_block_kernel, dim3((waves + 3) / 4), dim3(256), lds, stream, vd, t, n, zg64m, zg32m, (const DeadRec*)s->d_dead_drec, s->n_dead_pos);
  }
  for (int k = 0; k < n; ++k) {
    const pedn_plan::SplitPlan p = pedn_plan::plan_split_step(step_caps(s), s->marks, step_request(t + k, true, -1, s->plan.dead_streams));
    launch_split_live(s, p, t + k);
    pedn_plan::commit_split_step(s->marks, p);
    mirror_marks(s);
  }
}

// One chain's launches of a step, as the planner names them (pedn_plan::plan_step: the flush of a pending link update, the stand-alone
// turning fractions, node_kernel(t), the launch behind it), then the commit.  rq.chain = -1: the whole batch on the engine's stream; 0 / 1:
// the first / second half of the replicas on stream / stream2 (the caller launches every chain of a step; the last one commits).
// rq.profiled: every launch between the caller's start / stop events ev = {turn_prob, node, link} x 2.  *observed: the observations were part
// of the second launch.
static int launch_step(pedn_sim* s, const pedn_plan::StepRequest& rq, hipEvent_t* ev = nullptr, bool* observed = nullptr) {
  const int t = rq.t;
  if (s->dl_dirty && rq.chain <= 0) dl_refresh(s);   // dead links: an input of the proof has changed since the last step
  if (rq.chain < 0 && t - 1 > s->marks.valid_hi) {   // a step that skips ahead after a lazy reset (chains: their callers do this before the fork)
    const int rc = catch_up(s, t - 1);
    if (rc != PEDN_OK) return rc;
  }
  hipStream_t stream;
  DevView v = view_of(s, rq.chain, &stream);
  const pedn_plan::StepPlan p = pedn_plan::plan_step(step_caps(s), s->marks, rq);
  if (p.flush) flush_links(s, rq.chain, nullptr, p.commits);
  DevView vn = v;                 // node_kernel's view: with the action rows when it applies the gater actions itself
  vn.rl_actions = rq.fold;
  vn.quiet = p.quiet ? s->d_quiet : nullptr;
  vn.quiet_use = p.quiet_use;
  vn.quiet_lean = p.quiet_lean ? 1 : 0;
  vn.zg64 = p.zg64;
  vn.zg32 = p.zg32;
  row_bases(vn, t);
  auto launch = [&](auto kernel, dim3 grid, dim3 block, int e, auto... args) {
    if (rq.profiled) hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, ev[e], ev[e + 1], 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
  };
  const StepGrid g(s, v, p.link ? link_blocks(v, p.one_r) : 0u, p.fused, p.obs);
  if (p.tf_alone) launch(turn_frac_kernel_for(v), dim3(g.tf_blocks(v)), dim3(256), 0, v, t);
  const size_t nlds = p.inl ? s->plan.node_lds_tf : s->plan.node_lds;
  const dim3 nblock(p.helpers ? 1024 : 512);   // helper waves: sixteen per workgroup
  if (rq.profiled) hipExtLaunchKernelGGL(node_kernel_for(s, p.lu, p.inl), dim3(g.rgroups, (unsigned)s->n_blocks), nblock, nlds, stream, ev[2], ev[3], 0, vn, t);
  else hipLaunchKernelGGL(node_kernel_for(s, p.lu, p.inl), dim3(g.rgroups, (unsigned)s->n_blocks), nblock, nlds, stream, vn, t);
  if (p.second == pedn_plan::SECOND_LINK_TURN) {
    RlView q = s->rl;
    if (!p.obs) q.n_agents = 0;
    const int acc = rq.observe > 0 ? 1 : 0;
    const dim3 block(256);
    if (p.ctrl) launch(ctrl_link_turn_kernel_for(v), g.second(), block, 4, v, t, g.nlb, g.ntb, g.nth, q, acc, *rq.ctrl);
    else launch(link_turn_kernel_for(v, p.obs, false), g.second(), block, 4, v, t, g.nlb, g.ntb, g.nth, q, acc);
  } else if (p.second == pedn_plan::SECOND_LINK) {
    launch_link_update(s, v, stream, t, rq.profiled ? ev : nullptr, 4);
  }
  if (observed) *observed = p.obs;
  pedn_plan::commit_step(s->marks, p);
  mirror_marks(s);
  return PEDN_OK;
}

int pedn_step(pedn_sim* s, int32_t t) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (t < 1 || t > s->v.T1 - 1) return fail(s, PEDN_E_ARG, "time step outside 1..T");
  HIP_TRY(s, hipSetDevice(s->device));
  int rc = clock_end(s);
  if (rc != PEDN_OK) return rc;
  // The reference's own calling sequence -- for t in range(1, T): network_loading(t) -- on a batch that pedn_run would step as two chains:
  // from the third consecutive step that nothing looked at, the halves of the replicas step on two streams and STAY forked across the
  // calls (like pedn_rl_step's chains); whatever reads or changes the state next joins them (join_forked, as after an RL step).
  // melbourne x 1024 in a Python loop: 32.6 -> 28.9 us per step, delft 48.9 -> 43.9 (pedn_run: 28.6 / 43.4).
  const bool in_sequence = !s->touched && t == s->marks.last_t + 1 && s->chains > 1 && s->warmed_chains >= 2 && s->v.RS >= 256;
  s->step_streak = in_sequence ? std::min(s->step_streak + 1, 2) : 0;
  const bool two = s->step_streak >= 2;
  if (!two) join_forked(s);
  // owner-wave plan: this step's link update stays pending -- the next step's node kernel performs it, or whatever call looks at
  // or changes the state first (pending_links_first)
  bool lazy = s->plan.link_owner;
  if (lazy && s->plan.inline_tf) {   // (without device-computed rows both plans are two launches per step for such a caller)
    s->touch_streak = s->touched ? std::min(s->touch_streak + 1, 2) : std::max(s->touch_streak - 1, 0);
    if (s->touch_streak >= 2) lazy = false;
  }
  s->touched = 0;
  if (two) {
    if (!s->forked) {
      if (s->marks.link_pending >= 0 && s->marks.link_pending != t - 1) { pending_links_first(s); s->touched = 0; }   // a stale pending update: whole batch, before the fork
      if (t - 1 > s->marks.valid_hi && (rc = catch_up(s, t - 1)) != PEDN_OK) return rc;
      if ((rc = fork_chains(s, 2)) != PEDN_OK) return rc;
      s->forked = 1;
    }
    for (int c = 0; c < 2 && rc == PEDN_OK; ++c) rc = launch_step(s, step_request(t, lazy, c, 2));
    if (rc != PEDN_OK) return rc;
  } else if ((rc = launch_step(s, step_request(t, lazy))) != PEDN_OK) return rc;
  HIP_TRY(s, hipGetLastError());
  return PEDN_OK;
}

int pedn_profile_step(pedn_sim* s, int32_t t, float ms[3]) {
  if (!s || !ms) return fail(s, PEDN_E_ARG, "null argument");
  if (t < 1 || t > s->v.T1 - 1) return fail(s, PEDN_E_ARG, "time step outside 1..T");
  HIP_TRY(s, hipSetDevice(s->device));
  join_forked(s);   // (a pending link update is left to the first step of the range, as in pedn_run)
  // hipExtLaunchKernelGGL start/stop events carry the dispatch's own begin/end timestamps (what rocprofv3 reports),
  // not the enqueue-to-completion interval an ordinary hipEventRecord bracket would measure.
  hipEvent_t ev[6];
  for (int i = 0; i < 6; ++i) HIP_TRY(s, hipEventCreate(&ev[i]));
  pedn_plan::profile_begin(s->marks);
  pedn_plan::StepRequest rq = step_request(t, false);
  rq.profiled = true;
  launch_step(s, rq, ev);
  HIP_TRY(s, hipGetLastError());
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  ms[0] = ms[1] = ms[2] = 0.0f;
  if (s->marks.tp_ran) HIP_TRY(s, hipEventElapsedTime(&ms[0], ev[0], ev[1]));  // stand-alone turn probabilities (normally fused into [2])
  HIP_TRY(s, hipEventElapsedTime(&ms[1], ev[2], ev[3]));
  if (s->marks.second_launch) HIP_TRY(s, hipEventElapsedTime(&ms[2], ev[4], ev[5]));
  for (int i = 0; i < 6; ++i) hipEventDestroy(ev[i]);
  return PEDN_OK;
}

// pedn_run's plan for the range [t0, t1): how many chains of launches (each a share of the replicas on its own stream)?
static int chains_for(const pedn_sim* s, int t0, int t1) {
  if (s->chains < 2 || t1 - t0 < 8) return 1;
  return s->v.RS >= 256 ? 2 : 1;   // (every chain at least one 128-replica segment, view_of)
}

// Fork: every other chain's stream waits for what the engine's stream holds so far (idle: a chain that gets no work in this range).
static int fork_chains(pedn_sim* s, int n, int idle) {
  HIP_TRY(s, hipEventRecord(s->ev_fork, s->stream));
  for (int c = 1; c < n; ++c)
    if (c != idle) HIP_TRY(s, hipStreamWaitEvent(chain_stream(s, c), s->ev_fork, 0));
  return PEDN_OK;
}
// Join of the chains of launches: the engine's stream waits for everything enqueued on the other streams.  If the event path fails
// the streams are drained instead, so that no call ever returns with work on them that the engine's stream does not order.
static int join_chains(pedn_sim* s, int n, int idle) {
  hipError_t e = hipSuccess;
  for (int c = 1; c < n && e == hipSuccess; ++c) {
    if (c == idle) continue;
    hipEvent_t ev = c == 1 ? s->ev_join : s->ev_join3;
    e = hipEventRecord(ev, chain_stream(s, c));
    if (e == hipSuccess) e = hipStreamWaitEvent(s->stream, ev, 0);
  }
  if (e != hipSuccess) {
    for (int c = n - 1; c >= 0; --c) hipStreamSynchronize(chain_stream(s, c));
    return fail(s, PEDN_E_DEVICE, std::string("joining the chains of launches: ") + hipGetErrorString(e));
  }
  return PEDN_OK;
}

int pedn_run(pedn_sim* s, int32_t t0, int32_t t1) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (t0 < 1 || t1 > s->v.T1 || t0 > t1) return fail(s, PEDN_E_ARG, "step range outside 1..T");
  HIP_TRY(s, hipSetDevice(s->device));
  // Replicas are independent, so the two halves of the batch can run as two chains of launches on two streams: while one
  // half is in its link update (few, long waves) the other half's node_kernel fills the machine, and the ramp and the tail of
  // every launch overlap the other chain's work.  Forking and joining costs two cross-stream waits per CALL, so only ranges of
  // several steps take this plan; everything else (single steps, RL steps, profiling) stays on the one stream.
  // Owner-wave plan (link_owner): one launch per step for models without dynamic turning fractions -- node_kernel<LU>(t) performs the
  // link update of t - 1 -- plus one link_kernel for the last step of the range.
  const bool lazy = s->plan.link_owner;
  int rc = clock_end(s);
  if (rc != PEDN_OK) return rc;
  join_forked(s);
  const int nch = chains_for(s, t0, t1);
  if (nch > 1) {
    if (s->marks.link_pending >= 0 && s->marks.link_pending != t0 - 1) pending_links_first(s);   // a stale pending update: on the whole batch, before the fork
    if (t0 - 1 > s->marks.valid_hi && (rc = catch_up(s, t0 - 1)) != PEDN_OK) return rc;
    // Dead-link plan: the first node launch of the range on the whole batch and the full bin set, in front of the fork; every later one
    // is a node_kernel<LU> launch with quiet words and is split (launch_split_step) -- no event between the streams inside the range; with
    // one lean launch per step (dead_streams = 1) the second chain's stream has no work and is neither forked nor joined
    const bool split = nch == 2 && lazy && dl_split_ok(s);
    int t = t0;
    if (split && (rc = launch_step(s, step_request(t++, lazy))) != PEDN_OK) return rc;
    const int idle = split && s->plan.dead_streams == 1 ? 1 : -1;
    if ((rc = fork_chains(s, split ? 3 : nch, idle)) != PEDN_OK) return rc;
    while (t < t1) {
      if (split) {   // the steps that are left, in blocks of the lean stream (a block of one step: dead_link_kernel, as without blocks)
        const int n = pedn_plan::dead_block_len(t, t1, s->plan.dead_block, s->v.W);
        if (n > 1) launch_split_block(s, t, n);
        else launch_split_step(s, t);
        t += n;
      } else {
        for (int c = 0; c < nch; ++c) launch_step(s, step_request(t, lazy, c, nch));
        ++t;
      }
    }
    rc = join_chains(s, split ? 3 : nch, idle);    // the last step's link update stays pending on the joined stream (pending_links_first)
    if (rc != PEDN_OK) return rc;
  } else {
    for (int t = t0; t < t1; ++t)
      if ((rc = launch_step(s, step_request(t, lazy))) != PEDN_OK) return rc;
  }
  HIP_TRY(s, hipGetLastError());
  return PEDN_OK;
}

int pedn_plan_info(pedn_sim* s, int32_t* info, int32_t n) {
  if (!s || !info || n < 4) return fail(s, PEDN_E_ARG, "pedn_plan_info: null argument or fewer than 4 entries");
  const pedn_plan::PlanReport r = pedn_plan::report(s->plan, s->v.n_pairs_corr > 0);
  info[0] = s->chains;
  info[1] = r.owner_wave;   // (with device-computed rows: the single-launch plan, inline_tf)
  info[2] = s->stream_probe_attempts;
  info[3] = (int32_t)(s->stream_probe_ms * 1000.0f + 0.5f);
  if (n >= 5) info[4] = s->packed_by;   // bins of node_kernel packed by 0 degree, 1 the static load estimate, 2 measured node cost
  if (n >= 6) info[5] = r.quiet;   // the owner-wave launches keep and use the quiet-corridor words (PEDN_QUIET)
  if (n >= 7) info[6] = r.zero_elide;   // the node kernels may skip +0.0 stores into clean rows (PEDN_ZERO_ELIDE)
  if (n >= 8) info[7] = s->marks.zgated;   // ... and this many node-kernel launches had a gate open since the last reset
  if (n >= 9) info[8] = r.quiet_lean;   // the quiet-corridor launches take the lean path (PEDN_QUIET_LEAN)
  if (n >= 10) info[9] = r.dead_links && dl_split_ok(s) ? s->n_dead_links : 0;   // links that dead_link_kernel steps in a two-chain range (PEDN_DEAD_LINKS)
  if (n >= 11) info[10] = s->marks.split_steps;   // ... and the steps that were launched that way since the last reset
  return PEDN_OK;
}

int pedn_set_streams(pedn_sim* s, int32_t n) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (n != 1 && n != 2) return fail(s, PEDN_E_ARG, "1 or 2 chains of launches");
  HIP_TRY(s, hipSetDevice(s->device));
  int rc = clock_end(s);
  if (rc != PEDN_OK) return rc;
  if (n > s->warmed_chains) {
    pending_links_first(s);
    int got = 1;
    if ((rc = warm_chain_streams(s, &got)) != PEDN_OK) return rc;
    s->warmed_chains = got;
  }
  const int before = s->chains;
  s->chains = n > 1 ? std::min<int>(n, std::max(s->warmed_chains, 1)) : 1;
  if (s->chains > 1 && s->d_live_rec && (rc = warm_third_stream(s)) != PEDN_OK) return rc;
  if (s->chains > before) prewarm_chains(s);   // (every chain's stream: hipSetDevice above)
  return PEDN_OK;
}

// Steps [t0, t1) under pedn_run's plan with every launch bracketed by its dispatch timestamps.  rows: one per launch,
// {step, chain, kind (0 stand-alone turning fractions, 1 node_kernel, 2 the launch behind it), start, end} in ms after the start of
// the first launch of the range.
struct ProfRow { int t, chain, kind; float start, end; };
static int profile_range(pedn_sim* s, int t0, int t1, std::vector<ProfRow>& rows, int* chains) {
  const int halves = chains_for(s, t0, t1), n = (t1 - t0) * halves;
  const bool two = halves > 1;
  const bool lazy = s->plan.link_owner;   // pedn_run's plan
  struct Events {  // destroyed on every way out of the function
    std::vector<hipEvent_t> e;
    ~Events() { for (hipEvent_t x : e) if (x) hipEventDestroy(x); }
  } evs;
  evs.e.assign((size_t)(n + halves) * 6, nullptr);   // the last `halves` sets: the trailing link update of the owner-wave plan
  std::vector<hipEvent_t>& ev = evs.e;
  for (auto& e : ev) HIP_TRY(s, hipEventCreate(&e));
  std::vector<int> tp_ran((size_t)n, 0), second((size_t)n, 0);
  if (two) {
    if (s->marks.link_pending >= 0 && s->marks.link_pending != t0 - 1) pending_links_first(s);
    int rc = PEDN_OK;
    if (t0 - 1 > s->marks.valid_hi && (rc = catch_up(s, t0 - 1)) != PEDN_OK) return rc;
    if ((rc = fork_chains(s, halves)) != PEDN_OK) return rc;
  }
  for (int t = t0, k = 0; t < t1; ++t)
    for (int h = 0; h < halves; ++h, ++k) {
      pedn_plan::profile_begin(s->marks);
      pedn_plan::StepRequest rq = step_request(t, lazy, two ? h : -1, halves);
      rq.profiled = true;
      launch_step(s, rq, &ev[(size_t)k * 6]);
      tp_ran[k] = s->marks.tp_ran;
      second[k] = s->marks.second_launch;
    }
  const bool flushed = s->marks.link_pending >= 0;
  for (int h = 0; h < halves; ++h) flush_links(s, two ? h : -1, &ev[(size_t)(n + h) * 6], h == halves - 1);
  if (two) {
    const int rc = join_chains(s, halves);
    if (rc != PEDN_OK) return rc;
  }
  HIP_TRY(s, hipGetLastError());
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  // the first launch of the range (chain 0): its node_kernel, or the stand-alone turning fractions in front of it
  hipEvent_t origin = tp_ran[0] ? ev[0] : ev[2];
  rows.clear();
  for (int k = 0; k < n; ++k) {
    const int t = t0 + k / halves, chain = k % halves;
    for (int kind = 0; kind < 3; ++kind) {
      if ((kind == 0 && !tp_ran[k]) || (kind == 2 && !second[k])) continue;
      ProfRow r{t, chain, kind, 0.0f, 0.0f};
      HIP_TRY(s, hipEventElapsedTime(&r.start, origin, ev[(size_t)k * 6 + 2 * kind]));
      HIP_TRY(s, hipEventElapsedTime(&r.end, origin, ev[(size_t)k * 6 + 2 * kind + 1]));
      rows.push_back(r);
    }
  }
  for (int h = 0; h < halves && flushed; ++h) {   // the trailing link update: the second launch of the range's last step
    ProfRow r{t1 - 1, h, 2, 0.0f, 0.0f};
    HIP_TRY(s, hipEventElapsedTime(&r.start, origin, ev[(size_t)(n + h) * 6 + 4]));
    HIP_TRY(s, hipEventElapsedTime(&r.end, origin, ev[(size_t)(n + h) * 6 + 5]));
    rows.push_back(r);
  }
  *chains = halves;
  return PEDN_OK;
}

int pedn_profile_run(pedn_sim* s, int32_t t0, int32_t t1, float ms[3], int32_t* chains) {
  if (!s || !ms || !chains) return fail(s, PEDN_E_ARG, "null argument");
  if (t0 < 1 || t1 > s->v.T1 || t0 >= t1) return fail(s, PEDN_E_ARG, "step range outside 1..T");
  HIP_TRY(s, hipSetDevice(s->device));
  join_forked(s);   // (a pending link update is left to the first step of the range, as in pedn_run)
  std::vector<ProfRow> rows;
  int ch = 1;
  const int rc = profile_range(s, t0, t1, rows, &ch);
  if (rc != PEDN_OK) return rc;
  double sum[3] = {0, 0, 0};
  int cnt[3] = {0, 0, 0};
  for (const ProfRow& r : rows) { sum[r.kind] += (double)r.end - (double)r.start; ++cnt[r.kind]; }
  for (int i = 0; i < 3; ++i) ms[i] = cnt[i] ? (float)(sum[i] / cnt[i]) : 0.0f;
  *chains = ch;
  return PEDN_OK;
}

int pedn_profile_timeline(pedn_sim* s, int32_t t0, int32_t t1, float* out, int32_t capacity, int32_t* n_rows, int32_t* chains) {
  if (!s || !out || !n_rows || !chains) return fail(s, PEDN_E_ARG, "null argument");
  if (t0 < 1 || t1 > s->v.T1 || t0 >= t1) return fail(s, PEDN_E_ARG, "step range outside 1..T");
  HIP_TRY(s, hipSetDevice(s->device));
  join_forked(s);   // (a pending link update is left to the first step of the range, as in pedn_run)
  std::vector<ProfRow> rows;
  int ch = 1;
  const int rc = profile_range(s, t0, t1, rows, &ch);
  if (rc != PEDN_OK) return rc;
  if ((int)rows.size() > capacity) return fail(s, PEDN_E_ARG, "timeline buffer too small: " + std::to_string(rows.size()) + " rows");
  for (size_t i = 0; i < rows.size(); ++i) {
    out[5 * i] = (float)rows[i].t; out[5 * i + 1] = (float)rows[i].chain; out[5 * i + 2] = (float)rows[i].kind;
    out[5 * i + 3] = rows[i].start; out[5 * i + 4] = rows[i].end;
  }
  *n_rows = (int32_t)rows.size();
  *chains = ch;
  return PEDN_OK;
}

int pedn_synchronize(pedn_sim* s) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return PEDN_OK;
}

int pedn_error_flags(pedn_sim* s, uint32_t* flags) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  std::vector<uint32_t> h(s->v.RS);
  HIP_TRY(s, hipMemcpy(h.data(), s->v.flags, (size_t)s->v.RS * 4, hipMemcpyDeviceToHost));
  uint32_t any = 0;
  for (int r = 0; r < s->v.R; ++r) {
    any |= h[r];
    if (flags) flags[r] = h[r];
  }
  return (int)any;
}

int pedn_read(pedn_sim* s, int32_t field, int32_t t0, int32_t t1, int32_t c0, int32_t c1, int32_t r0, int32_t r1, void* out) {
  if (!s || !out) return fail(s, PEDN_E_ARG, "null argument");
  DevView& v = s->v;
  if (field < 0 || field >= PEDN_N_FIELDS) return fail(s, PEDN_E_ARG, "unknown field");
  int cols = field < 4 ? v.Lall : v.L;
  if (t0 < 0 || t1 > v.T1 || t0 >= t1 || c0 < 0 || c1 > cols || c0 >= c1 || r0 < 0 || r1 > v.R || r0 >= r1)
    return fail(s, PEDN_E_ARG, "read range out of bounds");
  const int rows = field < 7 ? s->rows64[field] : s->rows32[field - 7], mask = field < 7 ? v.m64[field] : v.m32[field - 7];
  if (rows < v.T1) {  // recent-history mode: only the newest `rows` time indices of this field exist
    // sending_flow / receiving_flow of step t are entries t - 1 (node.py:206, link.py:367): their newest entry is one behind
    const int newest = std::max((field == F_S || field == F_R) ? s->marks.last_t - 1 : s->marks.last_t, 0);
    if (t1 - 1 > newest || t0 <= newest - rows)
      return fail(s, PEDN_E_ARG, "time index outside the field's ring (recent-history mode keeps the last " + std::to_string(rows) +
                                 " entries of this field; the newest is " + std::to_string(newest) + ")");
  }
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  // (no wait here: everything the gather reads was written by earlier work on this stream)
  size_t n = (size_t)(t1 - t0) * (c1 - c0) * (r1 - r0);
  size_t esz = field < 7 ? 8 : 4;
  pedn_sim::Stage* st;
  int rc = stage_acquire(s, n * esz, &st);
  if (rc != PEDN_OK) return rc;
  unsigned blocks = (unsigned)((n + 255) / 256);
  // lazy reset: rows that were neither written nor cleared since the reset read as their initial value.  sending / receiving flow of
  // step t are entries t - 1; the gate record and avg_travel_time below the window were restored by the reset itself.
  int hi = 0x7fffffff;
  if (s->marks.valid_hi != 0x7fffffff) {
    hi = s->marks.valid_hi;
    if (field == F_S || field == F_R) hi = std::max(hi - 1, 0);
    else if (field == F_GATE) hi = 0x7fffffff;
    else if (field == 7 + G_ATT) hi = std::max(hi, v.W - 1);
  }
  // small reads (a controller looking at a few values after every step): the gather writes STRAIGHT into the pinned buffer over the bus --
  // no copy command behind the kernel (its ~10 us of stream latency were half of such a read)
  const bool direct = n * esz <= PEDN_DIRECT_READ_BYTES;
  void* const dst = direct ? st->pin : st->dev;
  if (field < 7)
    hipLaunchKernelGGL(gather_kernel<double>, dim3(blocks), dim3(256), 0, s->stream, (const double*)v.f64[field], (double*)dst, t0,
                       t1 - t0, c0, c1 - c0, r0, r1 - r0, cols, v.RS, mask, hi, (field == F_S || field == F_R) ? -1.0 : 0.0);
  else
    hipLaunchKernelGGL(gather_kernel<float>, dim3(blocks), dim3(256), 0, s->stream, (const float*)v.f32[field - 7], (float*)dst, t0,
                       t1 - t0, c0, c1 - c0, r0, r1 - r0, cols, v.RS, mask, hi, 0.0f);
  HIP_TRY(s, hipGetLastError());
  if (!direct) HIP_TRY(s, hipMemcpyAsync(st->pin, st->dev, n * esz, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  memcpy(out, st->pin, n * esz);
  return stage_commit(s, st);
}

int pedn_flush(pedn_sim* s) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);   // joins forked chains, ends a clocked section, performs a pending link update -- all on pedn_stream()
  if (s->marks.valid_hi != 0x7fffffff) {   // a zero-copy consumer may look at any row: finish what a lazy reset left out
    const int rc = catch_up(s, s->v.T1 - 1);
    if (rc != PEDN_OK) return rc;
    pedn_plan::caught_up(s->marks, pedn_plan::ALL_ROWS);
    mirror_marks(s);
  }
  return PEDN_OK;
}

void* pedn_device_ptr(pedn_sim* s, int32_t field, int64_t* columns, int64_t* replica_stride) {
  if (!s || field < 0 || field >= PEDN_N_FIELDS) return nullptr;
  if ((s->marks.link_pending >= 0 || s->forked || s->clocked || s->marks.valid_hi != 0x7fffffff) && pedn_flush(s) != PEDN_OK) return nullptr;
  // zero elision: a zero-copy consumer may write any row of the field -- no gate on its group until the next full reset
  // (dead links: ... and no split plan either)
  pedn_plan::foreign_write(s->marks, field <= F_CO, field == 7 + G_N || field == 7 + G_K || field == 7 + G_LF);
  if (columns) *columns = field < 4 ? s->v.Lall : s->v.L;
  if (replica_stride) *replica_stride = s->v.RS;
  return field < 7 ? (void*)s->v.f64[field] : (void*)s->v.f32[field - 7];
}

int pedn_history_rows(pedn_sim* s, int32_t field) {
  if (!s || field < 0 || field >= PEDN_N_FIELDS) return fail(s, PEDN_E_ARG, "unknown field");
  return field < 7 ? s->rows64[field] : s->rows32[field - 7];
}

void* pedn_stream(pedn_sim* s) { return s ? (void*)s->stream : nullptr; }

int pedn_timer_begin(pedn_sim* s) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  HIP_TRY(s, hipEventRecord(s->ev0, s->stream));
  return PEDN_OK;
}

int pedn_timer_end(pedn_sim* s, float* ms) {
  if (!s || !ms) return fail(s, PEDN_E_ARG, "null argument");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  HIP_TRY(s, hipEventRecord(s->ev1, s->stream));
  HIP_TRY(s, hipEventSynchronize(s->ev1));
  HIP_TRY(s, hipEventElapsedTime(ms, s->ev0, s->ev1));
  return PEDN_OK;
}

int pedn_set_link_params(pedn_sim* s, const double* kc, const double* kj, const double* vf, const int32_t* fft, const int32_t* tau_sw,
                         const float* tt0) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  pedn_plan::fractions_invalid(s->marks);
  s->dl_dirty = true;
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  DevView& v = s->v;
  if (!kc) {  // back to the shared parameters
    v.pr = 0;
    return PEDN_OK;
  }
  if (!kj || !vf || !fft || !tau_sw || !tt0) return fail(s, PEDN_E_ARG, "all six parameter matrices are required");
  for (size_t i = 0; i < (size_t)v.L * v.R; ++i) {
    if (!(kj[i] > kc[i]) || !(kc[i] > 0.0) || !(vf[i] > 0.0)) return fail(s, PEDN_E_ARG, "need 0 < k_critical < k_jam and free_flow_speed > 0");
    if (fft[i] < 0 || tau_sw[i] < 0) return fail(s, PEDN_E_ARG, "negative look-back");
    if (v.hist && tau_sw[i] + 2 > s->rows64[F_CO]) return fail(s, PEDN_E_ARG, "shock-wave look-back longer than the cumulative_outflow ring (recent-history mode)");
  }
  for (size_t i = 0; i < (size_t)v.L * v.R; ++i)
    if (fft[i] > 32767 || tau_sw[i] > 32767) return fail(s, PEDN_E_ARG, "look-back beyond 32767 steps");
  int rc;
  if ((rc = ensure_link_records(s)) != PEDN_OK) return rc;
  // the six matrices through one staging slot, packed into the 32-byte records on the device
  const size_t n = (size_t)v.L * v.R, bytes = n * (3 * 8 + 2 * 4 + 4);
  pedn_sim::Stage* st;
  if ((rc = stage_acquire(s, bytes, &st)) != PEDN_OK) return rc;
  unsigned char* h = (unsigned char*)st->pin;
  memcpy(h, kc, n * 8); memcpy(h + n * 8, kj, n * 8); memcpy(h + 2 * n * 8, vf, n * 8);
  memcpy(h + 3 * n * 8, fft, n * 4); memcpy(h + 3 * n * 8 + n * 4, tau_sw, n * 4); memcpy(h + 3 * n * 8 + 2 * n * 4, tt0, n * 4);
  HIP_TRY(s, hipMemcpyAsync(st->dev, st->pin, bytes, hipMemcpyHostToDevice, s->stream));
  const unsigned char* d = (const unsigned char*)st->dev;
  const size_t lanes = (size_t)v.L * v.RS;
  hipLaunchKernelGGL(pack_link_params_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s->stream, s->d_prm, (const double*)d,
                     (const double*)(d + n * 8), (const double*)(d + 2 * n * 8), (const int32_t*)(d + 3 * n * 8),
                     (const int32_t*)(d + 3 * n * 8 + n * 4), (const float*)(d + 3 * n * 8 + 2 * n * 4), v.L, v.R, v.RS);
  HIP_TRY(s, hipGetLastError());
  if ((rc = stage_commit(s, st)) != PEDN_OK) return rc;
  v.prm = s->d_prm;
  v.pr = 1;
  return PEDN_OK;
}

int pedn_get_link_params(pedn_sim* s, double* kc, double* kj, double* vf, int32_t* fft, int32_t* tau_sw, float* tt0) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->v.pr || !s->d_prm) return fail(s, PEDN_E_ARG, "no per-replica link parameters are set");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  const DevView& v = s->v;
  const size_t n = (size_t)v.L * v.R, bytes = n * (3 * 8 + 2 * 4 + 4);
  pedn_sim::Stage* st;
  int rc = stage_acquire(s, bytes, &st);
  if (rc != PEDN_OK) return rc;
  unsigned char* d = (unsigned char*)st->dev;
  hipLaunchKernelGGL(unpack_link_params_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, (const LinkPR*)s->d_prm,
                     (double*)d, (double*)(d + n * 8), (double*)(d + 2 * n * 8), (int32_t*)(d + 3 * n * 8), (int32_t*)(d + 3 * n * 8 + n * 4),
                     (float*)(d + 3 * n * 8 + 2 * n * 4), v.L, v.R, v.RS);
  HIP_TRY(s, hipGetLastError());
  HIP_TRY(s, hipMemcpyAsync(st->pin, st->dev, bytes, hipMemcpyDeviceToHost, s->stream));
  if ((rc = stage_commit(s, st)) != PEDN_OK) return rc;
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  const unsigned char* h = (const unsigned char*)st->pin;
  if (kc) memcpy(kc, h, n * 8);
  if (kj) memcpy(kj, h + n * 8, n * 8);
  if (vf) memcpy(vf, h + 2 * n * 8, n * 8);
  if (fft) memcpy(fft, h + 3 * n * 8, n * 4);
  if (tau_sw) memcpy(tau_sw, h + 3 * n * 8 + n * 4, n * 4);
  if (tt0) memcpy(tt0, h + 3 * n * 8 + 2 * n * 4, n * 4);
  return PEDN_OK;
}

int pedn_set_od_weights_per_replica(pedn_sim* s, const double* w) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  DevView& v = s->v;
  pedn_plan::fractions_invalid(s->marks);
  s->dl_dirty = true;
  if (!w) {
    v.pod_pr = 0;
    return PEDN_OK;
  }
  if (s->n_pair == 0) return PEDN_OK;
  int rc;
  if ((rc = ensure_pod_tables(s)) != PEDN_OK) return rc;
  if ((rc = push_matrix(s, s->d_od_w_r, w, s->n_od)) != PEDN_OK) return rc;
  return scenario_pod_tables(s);
}

int pedn_get_od_weights_per_replica(pedn_sim* s, double* w) {
  if (!s || !w) return fail(s, PEDN_E_ARG, "null argument");
  if (!s->v.pod_pr || !s->d_od_w_r) return fail(s, PEDN_E_ARG, "no per-replica OD weights are set");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  HIP_TRY(s, hipMemcpy2D(w, (size_t)s->v.R * 8, s->d_od_w_r, (size_t)s->v.RS * 8, (size_t)s->v.R * 8, s->n_od, hipMemcpyDeviceToHost));
  return PEDN_OK;
}

int pedn_randomize_scenarios(pedn_sim* s, uint64_t seed, double link_fraction, int32_t what, const int32_t* origin_nodes, int32_t n_origins) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!(link_fraction >= 0.0 && link_fraction <= 1.0)) return fail(s, PEDN_E_ARG, "link_fraction outside [0, 1]");
  if ((what & 4) && n_origins > 0 && !origin_nodes) return fail(s, PEDN_E_ARG, "origin nodes missing");
  HIP_TRY(s, hipSetDevice(s->device));
  DevView& v = s->v;
  pending_links_first(s);
  pedn_plan::fractions_invalid(s->marks);
  s->dl_dirty = true;
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
  int rc;
  if ((what & 1) && v.n_pairs_corr > 0) {
    const int k = (int)((double)v.n_pairs_corr * link_fraction);   // int(len(valid_links) * 0.2), env_loader.py:393
    if ((rc = ensure_link_records(s)) != PEDN_OK) return rc;
    if (!s->d_max_tau && (rc = dalloc(s, 1, &s->d_max_tau)) != PEDN_OK) return rc;
    HIP_TRY(s, hipMemsetAsync(s->d_max_tau, 0, sizeof(int), s->stream));
    // recent-history mode: the cumulative_outflow ring must cover the longest shock-wave look-back drawn -- checked BEFORE the draw
    // replaces the scenario in use: the records are drawn into a second buffer and copied over only when the check has passed (a copy,
    // not a swap of the two pointers: DevView.prm stays what captured launches carry, pedn_rl_clock_signature)
    LinkPR* dst = s->d_prm;
    if (v.hist) {
      if (!s->d_prm_draw && (rc = dalloc(s, (size_t)v.L * v.RS, &s->d_prm_draw)) != PEDN_OK) return rc;
      dst = s->d_prm_draw;
    }
    hipLaunchKernelGGL(rand_links_kernel, dim3((unsigned)((v.RS + 63) / 64)), dim3(64), 0, s->stream, v, dst, k, k0, k1, s->d_max_tau);
    HIP_TRY(s, hipGetLastError());
    if (v.hist) {
      int mt = 0;
      HIP_TRY(s, hipMemcpyAsync(&mt, s->d_max_tau, sizeof(int), hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(s, hipStreamSynchronize(s->stream));
      if (mt + 2 > s->rows64[F_CO])   // the engine keeps the scenario it had
        return fail(s, PEDN_E_ARG, "a drawn shock-wave look-back (" + std::to_string(mt) + ") is longer than the cumulative_outflow ring (recent-history mode)");
      HIP_TRY(s, hipMemcpyAsync(s->d_prm, s->d_prm_draw, (size_t)v.L * v.RS * sizeof(LinkPR), hipMemcpyDeviceToDevice, s->stream));
    }
    v.prm = s->d_prm;
    v.pr = 1;
  }
  if ((what & 2) && s->n_pair > 0) {
    if ((rc = ensure_pod_tables(s)) != PEDN_OK) return rc;
    const size_t lanes = (size_t)s->n_od * v.RS;
    hipLaunchKernelGGL(rand_od_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s->stream, s->d_od_w_r, s->n_od, v.RS, k0, k1, v.replica_offset);
    if ((rc = scenario_pod_tables(s)) != PEDN_OK) return rc;
  }
  if ((what & 4) && n_origins > 0) {
    std::vector<int32_t> hn((size_t)2 * n_origins);
    for (int i = 0; i < n_origins; ++i) {
      const int node = origin_nodes[i];
      if (node < 0 || node >= s->n_nodes || s->node_demand_row[node] < 0) return fail(s, PEDN_E_ARG, "origin node without a virtual link");
      hn[i] = s->node_demand_row[node];
      s->h_demand_nz[hn[i]] = 1;   // dead links: a row drawn on the device counts as non-zero
      hn[n_origins + i] = node;
    }
    pedn_sim::Stage* st;
    if ((rc = stage_acquire(s, hn.size() * 4, &st)) != PEDN_OK) return rc;
    if ((rc = stage_upload(s, st, hn.data(), hn.size() * 4)) != PEDN_OK) return rc;
    const size_t lanes = (size_t)v.T1 * v.RS;
    hipLaunchKernelGGL(rand_demand_kernel, dim3((unsigned)((lanes + 255) / 256), (unsigned)n_origins), dim3(256), 0, s->stream, v.demand,
                       (const int32_t*)st->dev, (const int32_t*)st->dev + n_origins, v.T1, v.R, v.RS, k0, k1, v.replica_offset);
    HIP_TRY(s, hipGetLastError());
    if ((rc = stage_commit(s, st)) != PEDN_OK) return rc;
  }
  return PEDN_OK;
}

int pedn_rl_configure(pedn_sim* s, const pedn_rl_desc* d, int32_t* n_actions, int32_t* n_obs) {
  if (!s || !d) return fail(s, PEDN_E_ARG, "null argument");
  if (d->n_agents < 1) return fail(s, PEDN_E_ARG, "no agents");
  if (d->obs_mode < 1 || d->obs_mode > 5) return fail(s, PEDN_E_ARG, "obs_mode must be 1..5");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  static const int fpl_of[6] = {0, 3, 4, 5, 2, 7};  // builders.py:47-58
  const int fpl = fpl_of[d->obs_mode];
  DevView& v = s->v;
  std::vector<int32_t> act_off(d->n_agents), obs_off(d->n_agents), slot_agent, slot_idx;
  int A = 0, O = 0;
  for (int a = 0; a < d->n_agents; ++a) {
    const int n = d->agent_link_ptr[a + 1] - d->agent_link_ptr[a];
    act_off[a] = A; obs_off[a] = O;
    for (int k = d->agent_link_ptr[a]; k < d->agent_link_ptr[a + 1]; ++k) {
      int l = d->agent_links[k];
      if (l < 0 || l >= v.L) return fail(s, PEDN_E_ARG, "agent link out of range");
    }
    if (d->agent_type[a] == 0) {
      if (n != 2) return fail(s, PEDN_E_ARG, "separator agent needs (forward, reverse)");
      if (d->normalize && (d->obs_mode == 3 || d->obs_mode == 4))
        return fail(s, PEDN_E_ARG, "normalised separator observations index out of range for option3/option4 (IndexError in the reference, builders.py:189-198)");
      slot_agent.push_back(a); slot_idx.push_back(0);
      A += 1; O += 4;
    } else if (d->agent_type[a] == 1) {
      if (n < 1 || n > PEDN_MAX_DEGREE) return fail(s, PEDN_E_ARG, "gater outdegree outside 1..8");
      if (d->normalize && d->obs_mode == 4)
        return fail(s, PEDN_E_ARG, "normalised gater observations index out of range for option4 (IndexError in the reference, builders.py:229-236)");
      for (int i = 0; i < n; ++i) { slot_agent.push_back(a); slot_idx.push_back(i); }
      A += n; O += n * fpl;
    } else return fail(s, PEDN_E_ARG, "agent_type must be 0 or 1");
  }
  RlView& q = s->rl;
  int rc;
#define UP(src, n, dst) if ((rc = upload(s, src, n, dst)) != PEDN_OK) return rc
  UP(d->agent_type, (size_t)d->n_agents, &q.agent_type);
  UP(d->agent_link_ptr, (size_t)d->n_agents + 1, &q.agent_link_ptr);
  UP(d->agent_links, (size_t)d->agent_link_ptr[d->n_agents], &q.agent_links);
  UP(act_off.data(), act_off.size(), &q.agent_act_off);
  UP(obs_off.data(), obs_off.size(), &q.agent_obs_off);
  UP(slot_agent.data(), slot_agent.size(), &q.slot_agent);
  UP(slot_idx.data(), slot_idx.size(), &q.slot_idx);
#undef UP
  if ((rc = dalloc(s, (size_t)v.R * A, &q.actions)) != PEDN_OK) return rc;
  // observations and rewards in ONE allocation, rewards right behind the observations: a fetch of both is one copy (rl_fetch)
  if ((rc = dalloc(s, (size_t)v.R * O + (size_t)v.R * d->n_agents, &q.obs)) != PEDN_OK) return rc;
  q.rew = q.obs + (size_t)v.R * O;
  HIP_TRY(s, hipMemset(q.obs, 0, (size_t)v.R * O * sizeof(float)));
  HIP_TRY(s, hipMemset(q.rew, 0, (size_t)v.R * d->n_agents * sizeof(float)));
  q.n_agents = d->n_agents; q.A = A; q.O = O; q.obs_mode = d->obs_mode; q.normalize = d->normalize; q.reward_mode = d->reward_mode;
  q.fpl = fpl; q.max_delta_sep = d->max_delta_sep; q.max_delta_gate = d->max_delta_gate; q.min_sep = d->min_sep;
  // widths of controlled links are written per replica by rl_apply_kernel: never take the uniform shortcut for them
  s->h_rl_link.assign((size_t)v.L, 0);
  for (int a = 0; a < d->n_agents; ++a)
    for (int k = d->agent_link_ptr[a]; k < d->agent_link_ptr[a + 1]; ++k) s->h_rl_link[d->agent_links[k]] = 1;
  {
    std::vector<LinkP> lp((size_t)v.L);
    HIP_TRY(s, hipMemcpy(lp.data(), v.lp, lp.size() * sizeof(LinkP), hipMemcpyDeviceToHost));
    for (int a = 0; a < d->n_agents; ++a)
      for (int k = d->agent_link_ptr[a]; k < d->agent_link_ptr[a + 1]; ++k) {
        s->h_rl_link[lp[d->agent_links[k]].rev] = 1;
      }
  }
  if ((rc = push_uniform(s)) != PEDN_OK) return rc;
  {  // a gater action (back gate of outgoing link l of the gater node = front gate of its reverse) is consumed by exactly one
     // wave of node_kernel, the slot (lin = reverse(l), lout = l): that wave can apply it.  A separator's width is read at both
     // ends of its corridor, so agent sets with a separator keep the separate rl_apply_kernel launch.
    bool only_gaters = true;
    for (SlotRec& R : s->h_slot_rec) R.act = -1;
    for (int a = 0, slot = 0; a < d->n_agents; ++a) {
      const int n = d->agent_link_ptr[a + 1] - d->agent_link_ptr[a];
      if (d->agent_type[a] == 0) { only_gaters = false; slot += 1; continue; }
      for (int i = 0; i < n; ++i, ++slot) {
        const int l = d->agent_links[d->agent_link_ptr[a] + i];
        int hits = 0;
        for (SlotRec& R : s->h_slot_rec)
          if (R.node >= 0 && R.lout == l && R.lin < v.L) { R.act = slot; ++hits; }
        if (hits != 1) only_gaters = false;
      }
    }
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    HIP_TRY(s, hipMemcpy(s->d_slot_rec, s->h_slot_rec.data(), s->h_slot_rec.size() * sizeof(SlotRec), hipMemcpyHostToDevice));
    s->rl_fold = only_gaters;
    if (const char* f = getenv("PEDN_RL_FOLD")) s->rl_fold = s->rl_fold && atoi(f) != 0;
    v.rl_A = A;
    v.rl_max_delta_gate = d->max_delta_gate;
    v.rl_actions = nullptr;
  }
  s->rl_ready = true;
  s->dl_dirty = true;
  s->ctrl.ready = s->ctrl.any = false;   // controllers belong to an agent set: configure them again
  s->norm.on = s->norm.alloc = false;    // so does the running normalisation
  memset(&s->norm.view, 0, sizeof s->norm.view);
  store_drop(s->ro);                     // and a rollout store (its rows have the agent set's widths)
  store_drop(s->rp);                     // and a replay store
  if (n_actions) *n_actions = A;
  if (n_obs) *n_obs = O;
  return PEDN_OK;
}

int pedn_rl_apply_actions(pedn_sim* s, const double* actions, int32_t on_device) {
  if (!s || !actions) return fail(s, PEDN_E_ARG, "null argument");
  if (!s->rl_ready) return fail(s, PEDN_E_ARG, "pedn_rl_configure has not been called");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  DevView& v = s->v;
  RlView& q = s->rl;
  const size_t bytes = (size_t)v.R * q.A * sizeof(double);
  RlView qq = q;
  if (on_device) qq.actions = const_cast<double*>(actions);  // read the caller's rows in place: no staging copy
  pedn_sim::Stage* st = nullptr;
  if (!on_device) {   // the host buffer is borrowed for the call only
    int rc;
    if (bytes <= PEDN_IN_PLACE_BYTES) {
      if ((rc = stage_in_place(s, actions, bytes, &st)) != PEDN_OK) return rc;
      qq.actions = (double*)st->pin;
    } else if ((rc = upload_through_stage(s, q.actions, actions, bytes)) != PEDN_OK) return rc;
  }
  size_t n = (size_t)q.A * v.RS;
  hipLaunchKernelGGL(rl_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, v, qq);
  HIP_TRY(s, hipGetLastError());
  if (st) return stage_commit(s, st);
  return PEDN_OK;
}

// observations / rewards -> the caller's buffers: both copies land in ONE pinned buffer, one wait for the stream, then two memcpys (into
// pageable memory each copy is staged and waited for by the runtime on its own)
static int rl_fetch(pedn_sim* s, float* obs, float* rewards, bool raw = false) {
  if (!obs && !rewards) return PEDN_OK;
  const RlView& q = s->rl;
  const FetchRows rows = fetch_rows(s, raw);
  const size_t nb_obs = (size_t)s->v.R * q.O * sizeof(float), nb_rew = (size_t)s->v.R * q.n_agents * sizeof(float);
  if (s->rl_pin_bytes < nb_obs + nb_rew) {
    if (s->rl_pin) HIP_TRY(s, hipHostFree(s->rl_pin));
    s->rl_pin = nullptr;
    s->rl_pin_bytes = 0;
    HIP_TRY(s, hipHostMalloc(&s->rl_pin, nb_obs + nb_rew, hipHostMallocDefault));
    s->rl_pin_bytes = nb_obs + nb_rew;
  }
  char* pin = (char*)s->rl_pin;
  if (obs && rewards) HIP_TRY(s, hipMemcpyAsync(pin, rows.obs, nb_obs + nb_rew, hipMemcpyDeviceToHost, s->stream));   // (contiguous: pedn_rl_configure)
  else if (obs) HIP_TRY(s, hipMemcpyAsync(pin, rows.obs, nb_obs, hipMemcpyDeviceToHost, s->stream));
  else HIP_TRY(s, hipMemcpyAsync(pin + nb_obs, rows.rew, nb_rew, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  if (obs) memcpy(obs, pin, nb_obs);
  if (rewards) memcpy(rewards, pin + nb_obs, nb_rew);
  return PEDN_OK;
}

// (cv: the controller twin, see launch_step)
// norm: 0 no normalisation launch (a sub-step inside an env step), 1 behind an observation alone, 2 behind an env step (term: its terminated flag)
static int rl_observe(pedn_sim* s, int32_t t, int32_t accumulate, float* obs, float* rewards, const CtrlView* cv, int norm, int term) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->rl_ready) return fail(s, PEDN_E_ARG, "pedn_rl_configure has not been called");
  if (t < 0 || t > s->v.T1 - 1) return fail(s, PEDN_E_ARG, "time step outside 0..T");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);
  if (t > s->marks.valid_hi) catch_up(s, t);   // observations of a step that has not run read its rows as they were initialised
  DevView& v = s->v;
  RlView& q = s->rl;
  const dim3 grid((unsigned)q.n_agents * (unsigned)(v.RS / 64));
  if (cv) hipLaunchKernelGGL(ctrl_observe_kernel_for(v), grid, dim3(256), 0, s->stream, v, q, t, accumulate, *cv);
  else hipLaunchKernelGGL(rl_observe_kernel_for(v), grid, dim3(256), 0, s->stream, v, q, t, accumulate);
  if (norm) norm_launch(s, s->stream, norm == 2, term);
  HIP_TRY(s, hipGetLastError());
  return rl_fetch(s, obs, rewards);
}

int pedn_rl_observe(pedn_sim* s, int32_t t, int32_t accumulate, float* obs, float* rewards) {
  return rl_observe(s, t, accumulate, obs, rewards, nullptr, 1);
}

static int fetch_entry(pedn_sim* s, float* obs, float* rewards, bool raw) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->rl_ready) return fail(s, PEDN_E_ARG, "pedn_rl_configure has not been called");
  HIP_TRY(s, hipSetDevice(s->device));
  join_forked(s);   // (ends a clocked section; both chains' work in front of the copies)
  return rl_fetch(s, obs, rewards, raw);
}

int pedn_rl_fetch(pedn_sim* s, float* obs, float* rewards) { return fetch_entry(s, obs, rewards, false); }
int pedn_rl_fetch_raw(pedn_sim* s, float* obs, float* rewards) { return fetch_entry(s, obs, rewards, true); }

int pedn_rl_step(pedn_sim* s, const double* actions, int32_t on_device, int32_t t, int32_t action_gap, float* obs, float* rewards) {
  return rl_step(s, actions, on_device, t, action_gap, obs, rewards, nullptr);
}

// cv: a controlled env step (pedn_ctrl_step) -- its last sub-step observes through the controller twins
static int rl_step(pedn_sim* s, const double* actions, int32_t on_device, int32_t t, int32_t action_gap, float* obs, float* rewards,
                   const CtrlView* cv) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (action_gap < 1 || t < 1 || t + action_gap - 1 > s->v.T1 - 1) return fail(s, PEDN_E_ARG, "step range outside 1..T");
  int rc = PEDN_OK;
  if (!s->rl_ready) return fail(s, PEDN_E_ARG, "pedn_rl_configure has not been called");
  if (s->clocked) {   // back to host-side step indices (the fold decision below reads tp_ready)
    HIP_TRY(s, hipSetDevice(s->device));
    if ((rc = clock_end(s)) != PEDN_OK) return rc;
  }
  RlView& q = s->rl;
  // gater-only agent sets: node_kernel of the first sub-step applies the actions (one launch less).  Not when the turning
  // fractions of step t still have to be computed by their own launch in front of node_kernel: their capacity fallback reads
  // the gate widths the actions are about to change (path_finder.py:575-576).
  const double* fold = nullptr;
  pedn_sim::Stage* fold_stage = nullptr;   // host actions read in place by node_kernel of the first sub-step (stage_in_place)
  if (actions) {
    const bool stand_alone_tf = s->v.n_trow > 0 && s->marks.tp_ready != t;
    if (s->rl_fold && !stand_alone_tf) {
      HIP_TRY(s, hipSetDevice(s->device));
      if (on_device) fold = actions;
      else {
        const size_t bytes = (size_t)s->v.R * q.A * sizeof(double);
        if (bytes <= PEDN_IN_PLACE_BYTES) {
          if ((rc = stage_in_place(s, actions, bytes, &fold_stage)) != PEDN_OK) return rc;
          fold = (const double*)fold_stage->pin;
        } else {
          if ((rc = upload_through_stage(s, q.actions, actions, bytes)) != PEDN_OK) return rc;
          fold = q.actions;
        }
      }
    } else if ((rc = pedn_rl_apply_actions(s, actions, on_device)) != PEDN_OK) return rc;   // (performs a pending link update first)
  }
  // Two chains that stay forked ACROSS calls (rl_chains): the two halves of the envs step on two streams, call after call, and are
  // joined only when something needs the whole batch (join_forked: an observation fetch, a setter, a read, a synchronise).  A step is two
  // dependent launches whose durations barely depend on the batch size, so the two half-batch chains run side by side almost for free
  // (45_intersections x 2048: 25.0 -> 22.x us per env step).  Only when nothing of this call runs on the engine's stream alone: the
  // actions are applied inside node_kernel (or there are none) and the observations ride in the second launch.
  // (actions from the host go through the engine's own action buffer, which the other chain's previous step may still be reading)
  if (t - 1 > s->marks.valid_hi) {   // skipping ahead after a lazy reset
    join_forked(s);
    if ((rc = catch_up(s, t - 1)) != PEDN_OK) return rc;
  }
  const bool by_batch = s->v.RS >= 4096 || (s->v.pr && s->v.RS >= 1024);
  // on_device == 2: the caller chains this call between its own streams and pedn_stream() with events (no host synchronisation):
  // everything must then be ordered by the engine's stream alone
  const int term = t + action_gap - 1 >= s->v.T1 - 1 ? 1 : 0;   // pz_pednet_env.py:592
  const bool two = !s->norm.on && on_device != 2 && (s->plan.rl_chains == 2 || (s->plan.rl_chains == 0 && by_batch)) && s->warmed_chains >= 2 && s->v.RS >= 256 && s->plan.fuse_obs && (!actions || (fold != nullptr && on_device)) && !obs && !rewards &&
                   s->marks.link_pending < 0 && !(s->v.n_trow > 0 && !s->plan.fuse_tp);
  if (!two) join_forked(s);
  else if (!s->forked) {
    if ((rc = fork_chains(s, 2)) != PEDN_OK) return rc;
    s->forked = 1;
  }
  for (int k = 0; k < action_gap; ++k) {
    const bool last = k == action_gap - 1;
    bool observed = false;
    // (always two launches per env step: the observations are a second launch either way, and with the rows of t + 1 riding in it the
    // two launches are shorter than the single-launch / owner-wave plans -- profiles/r04_rl_small_batches.txt, r04_rl_owner.txt)
    const CtrlView* ck = last ? cv : nullptr;
    pedn_plan::StepRequest rq = step_request(t + k, false, -1, two ? 2 : 1);
    rq.observe = k > 0 ? 1 : 0;
    rq.fold = k == 0 ? fold : nullptr;
    rq.ctrl = ck;
    if (two) {
      for (rq.chain = 0; rq.chain < 2; ++rq.chain) launch_step(s, rq, nullptr, &observed);
      if ((last && (obs || rewards)) || !observed) join_forked(s);
    } else {
      if ((rc = launch_step(s, rq, nullptr, &observed)) != PEDN_OK) return rc;
    }
    if (k == 0 && fold_stage && (rc = stage_commit(s, fold_stage)) != PEDN_OK) return rc;   // its only reader has been launched
    HIP_TRY(s, hipGetLastError());
    if (!observed) {
      if ((rc = rl_observe(s, t + k, k > 0, last ? obs : nullptr, last ? rewards : nullptr, ck, last ? 2 : 0, term)) != PEDN_OK) return rc;
    } else if (last) {
      norm_launch(s, s->stream, 1, term);
      HIP_TRY(s, hipGetLastError());
      if ((obs || rewards) && (rc = rl_fetch(s, obs, rewards)) != PEDN_OK) return rc;
    }
  }
  return PEDN_OK;
}

// ---- device-resident step clock: env steps whose launches have constant arguments (a captured graph of them can be replayed)
static int clock_end(pedn_sim* s) {
  if (!s->clocked) return PEDN_OK;
  s->clocked = false;
  // the clocked steps may sit on a caller's stream (or in a graph replayed on one): everything on the device first
  HIP_TRY(s, hipDeviceSynchronize());
  int32_t h[4] = {0, 0, 0, 0};
  HIP_TRY(s, hipMemcpy(h, s->d_clock, sizeof(h), hipMemcpyDeviceToHost));
  pedn_plan::clock_ended(s->marks, step_caps(s), s->clock_t0, h[0], h[2]);
  mirror_marks(s);
  return PEDN_OK;
}

int pedn_rl_clock_begin(pedn_sim* s, int32_t t) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->rl_ready) return fail(s, PEDN_E_ARG, "pedn_rl_configure has not been called");
  if (t < 1 || t > s->v.T1 - 1) return fail(s, PEDN_E_ARG, "time step outside 1..T");
  if (!s->plan.fuse_obs || !s->plan.fuse_tp || s->v.n_pairs_corr == 0 || s->plan.node_lp)
    return fail(s, PEDN_E_ARG, "the clocked step needs the fused second launch (PEDN_FUSE_OBS / PEDN_FUSE_TP), physical links and the classic node model");
  HIP_TRY(s, hipSetDevice(s->device));
  pending_links_first(s);   // (ends a clocked section that is still open)
  int rc;
  if (t - 1 > s->marks.valid_hi && (rc = catch_up(s, t - 1)) != PEDN_OK) return rc;
  // The fractions of step t must be in place: the stand-alone launch that would compute them reads the gate widths AFTER the actions of
  // step t are applied (capacity fallback, path_finder.py:575-576) -- only the ordinary pedn_rl_step can order that.  True for every
  // step but the first one after a reset or a setter.
  if (s->v.n_trow > 0 && s->marks.tp_ready != t)
    return fail(s, PEDN_E_ARG, "turning fractions of step " + std::to_string(t) + " are not prepared: run this step with pedn_rl_step first");
  hipLaunchKernelGGL(set_clock_kernel, dim3(1), dim3(64), 0, s->stream, s->d_clock, t, s->marks.valid_hi);
  HIP_TRY(s, hipGetLastError());
  s->clocked = true;
  s->clock_t0 = t;
  pedn_plan::foreign_write(s->marks, true, true);   // the host does not see which rows the clocked steps write: no zero gate, no dead-link plan
  return PEDN_OK;
}

int pedn_rl_step_clocked(pedn_sim* s, const double* actions, int32_t action_gap, void* stream) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  if (!s->clocked) return fail(s, PEDN_E_ARG, "pedn_rl_clock_begin has not been called (or the clocked section was ended by another call)");
  if (action_gap < 1) return fail(s, PEDN_E_ARG, "action_gap < 1");
  HIP_TRY(s, hipSetDevice(s->device));
  hipStream_t st = stream ? (hipStream_t)stream : s->stream;
  const DevView& v = s->v;
  RlView q = s->rl;
  const double* fold = nullptr;
  if (actions) {
    if (s->rl_fold) fold = actions;   // gater-only agent set: the consuming node_kernel wave clips and applies the action
    else {
      RlView qq = q;
      qq.actions = const_cast<double*>(actions);
      const size_t n = (size_t)q.A * v.RS;
      hipLaunchKernelGGL(rl_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, v, qq);
    }
  }
  // the fractions of t + 1 ride in the second launch (its workgroups idle behind the last step); it always observes
  const StepGrid g(s, v, link_blocks(v, v.pr != 0), v.n_trow > 0, true);
  for (int k = 0; k < action_gap; ++k) {
    DevView vn = v;
    vn.rl_actions = k == 0 ? fold : nullptr;
    hipLaunchKernelGGL(clocked_node_kernel_for(s), dim3(g.rgroups, (unsigned)s->n_blocks), dim3(512), s->plan.node_lds, st, vn, -1);
    const int acc = k > 0 ? 1 : 0;
    hipLaunchKernelGGL(link_turn_kernel_for(v, true, true), g.second(), dim3(256), 0, st, v, -1, g.nlb, g.ntb, g.nth, q, acc);
  }
  norm_launch(s, st, 1, -1);   // (constant arguments: `terminated` comes from the clock)
  HIP_TRY(s, hipGetLastError());
  return PEDN_OK;
}

int pedn_rl_clocked(pedn_sim* s) { return s && s->clocked ? 1 : 0; }

// What the launches of pedn_rl_step_clocked are made of: the device view they carry BY VALUE (pointers, sizes, per-replica-scenario
// switches -- not valid_hi, which a clocked launch takes from the clock), the RL view, and what selects kernels and grids.
uint64_t pedn_rl_clock_signature(pedn_sim* s) {
  if (!s) return 0;
  DevView v;
  memcpy(&v, &s->v, sizeof v);   // byte image, padding included (see below)
  v.valid_hi = 0;
  v.rl_actions = nullptr;
  uint64_t h = 1469598103934665603ull;   // FNV-1a
  auto mix = [&](const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  };
  static_assert(std::is_trivially_copyable<DevView>::value && std::is_trivially_copyable<RlView>::value, "hashed as bytes");
  // (hashed as bytes, padding included: s->v lives in the value-initialised pedn_sim and is only ever changed field by field, so
  // its padding keeps the image it was created with; a spurious difference would cost one more capture, never a stale graph)
  mix(&v, sizeof v);
  mix(&s->rl, sizeof s->rl);
  const int64_t sel[8] = {s->rl_fold, s->n_tf_heavy_quads, s->n_blocks, (int64_t)s->plan.node_lds, s->max_degree, s->plan.node_lp, s->plan.fuse_tp, s->plan.fuse_obs};
  mix(sel, sizeof sel);
  const int64_t on = s->norm.on;   // the normalisation launch and its view (zeroed while off; configure fills every byte it hashes)
  mix(&on, sizeof on);
  mix(&s->norm.view, sizeof s->norm.view);
  const int64_t store = s->ro.on;   // a record launch captured with the step carries the store's view (zeroed while there is none)
  mix(&store, sizeof store);
  mix(&s->ro.view, sizeof s->ro.view);
  const int64_t replay = s->rp.on;   // the same for a captured push launch of the replay store
  mix(&replay, sizeof replay);
  mix(&s->rp.view, sizeof s->rp.view);
  return h;
}

int pedn_rl_clock_end(pedn_sim* s, int32_t* t) {
  if (!s) return fail(nullptr, PEDN_E_ARG, "null handle");
  HIP_TRY(s, hipSetDevice(s->device));
  const int rc = clock_end(s);
  if (rc != PEDN_OK) return rc;
  if (t) *t = s->marks.last_t + 1;
  return PEDN_OK;
}

int pedn_rl_step_many(pedn_sim** sims, int32_t n, const double* actions, int32_t t, int32_t action_gap, float* obs, float* rewards) {
  if (!sims || n < 1) return fail(nullptr, PEDN_E_ARG, "no engines");
  for (int k = 0; k < n; ++k)
    if (!sims[k] || !sims[k]->rl_ready) return fail(sims[k], PEDN_E_ARG, "null handle or pedn_rl_configure has not been called");
  for (int k = 0; k < n; ++k)
    if (sims[k]->norm.on) return fail(sims[k], PEDN_E_ARG, "pedn_rl_step_many does not run the running normalisation (statistics are per engine)");
  size_t row = 0;
  for (int k = 0; k < n; ++k) {   // every engine's launches first (own stream each: they overlap) ...
    pedn_sim* s = sims[k];
    const int rc = pedn_rl_step(s, actions ? actions + row * (size_t)s->rl.A : nullptr, 0, t, action_gap, nullptr, nullptr);
    if (rc != PEDN_OK) return rc;
    row += (size_t)s->v.R;
  }
  row = 0;
  for (int k = 0; k < n; ++k) {   // ... then one fetch each
    pedn_sim* s = sims[k];
    const int rc = pedn_rl_fetch(s, obs ? obs + row * (size_t)s->rl.O : nullptr, rewards ? rewards + row * (size_t)s->rl.n_agents : nullptr);
    if (rc != PEDN_OK) return rc;
    row += (size_t)s->v.R;
  }
  return PEDN_OK;
}

void* pedn_rl_device_ptr(pedn_sim* s, int32_t which) {
  if (!s || !s->rl_ready) return nullptr;
  return which == 0 ? (void*)s->rl.actions : which == 1 ? (void*)s->rl.obs : which == 2 ? (void*)s->rl.rew : nullptr;
}

int pedn_device_math(int32_t device, int32_t op, int32_t n, const double* a, const double* b, uint64_t seed, double* out) {
  if (n <= 0 || !a || !out) return fail(nullptr, PEDN_E_ARG, "bad argument");
  HIP_TRY(nullptr, hipSetDevice(device));
  struct Buf {   // freed on every way out
    double* p = nullptr;
    ~Buf() { if (p) (void)hipFree(p); }
  } da, db, dout;
  HIP_TRY(nullptr, hipMalloc((void**)&da.p, (size_t)n * 8));
  HIP_TRY(nullptr, hipMalloc((void**)&dout.p, (size_t)n * 8));
  HIP_TRY(nullptr, hipMemcpy(da.p, a, (size_t)n * 8, hipMemcpyHostToDevice));
  if (b) {
    HIP_TRY(nullptr, hipMalloc((void**)&db.p, (size_t)n * 8));
    HIP_TRY(nullptr, hipMemcpy(db.p, b, (size_t)n * 8, hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(device_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, n, (const double*)da.p, (const double*)db.p,
                     (uint32_t)seed, (uint32_t)(seed >> 32), dout.p);
  HIP_TRY(nullptr, hipGetLastError());
  HIP_TRY(nullptr, hipDeviceSynchronize());
  HIP_TRY(nullptr, hipMemcpy(out, dout.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return PEDN_OK;
}

#ifdef PEDN_PHASE_PROFILE
// profiling build only (make phase-profile): read (zero = 0) or clear (zero = 1) the 16 phase accumulators of node_kernel
extern "C" int pedn_debug_tphases(unsigned long long* out, int zero) {
  void* dev = nullptr;
  if (hipGetSymbolAddress(&dev, HIP_SYMBOL(g_tphase)) != hipSuccess) return -1;
  if (zero) return (int)hipMemset(dev, 0, sizeof(unsigned long long) * 4096 * 8);
  return (int)hipMemcpy(out, dev, sizeof(unsigned long long) * 4096 * 8, hipMemcpyDeviceToHost);
}
// [workgroup][role 0 long turning-fraction rows / 1 link update / 2 short rows / 3 observations, start, end, 0] of the LAST launch of
// link_turn_kernel (zero = 1 clears)
extern "C" int pedn_debug_lt_timeline(unsigned long long* out, int n_blocks, int zero) {
  void* dev = nullptr;
  if (hipGetSymbolAddress(&dev, HIP_SYMBOL(g_lt_time)) != hipSuccess) return -1;
  if (zero) return (int)hipMemset(dev, 0, sizeof(unsigned long long) * PEDN_LT_BLOCKS * 4);
  if (n_blocks > PEDN_LT_BLOCKS) n_blocks = PEDN_LT_BLOCKS;
  return (int)hipMemcpy(out, dev, sizeof(unsigned long long) * (size_t)n_blocks * 4, hipMemcpyDeviceToHost);
}
// raw accumulators of the first n_waves waves of the grid, quiet and non-quiet launches together: [wave][12] = 9 phase sums, -, count,
// lifetime (tools/pack_analysis.py)
extern "C" int pedn_debug_phase_waves(unsigned long long* out, int n_waves) {
  void* dev = nullptr;
  if (hipGetSymbolAddress(&dev, HIP_SYMBOL(g_phase)) != hipSuccess) return -1;
  if (n_waves > PEDN_PHASE_WAVES) n_waves = PEDN_PHASE_WAVES;
  std::vector<unsigned long long> h((size_t)n_waves * 24);
  if (hipMemcpy(h.data(), dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  for (size_t w = 0; w < (size_t)n_waves; ++w)
    for (int i = 0; i < 12; ++i) out[w * 12 + i] = h[w * 24 + i] + h[w * 24 + 12 + i];
  return 0;
}
extern "C" int pedn_debug_phases(unsigned long long* out, int zero) {
  const size_t n = (size_t)PEDN_PHASE_WAVES * 24;   // out[0..11]: non-quiet waves, out[12..23]: quiet ones (g_phase)
  void* dev = nullptr;
  if (hipGetSymbolAddress(&dev, HIP_SYMBOL(g_phase)) != hipSuccess) return -1;
  if (zero) return (int)hipMemset(dev, 0, n * sizeof(unsigned long long));
  std::vector<unsigned long long> h(n);
  if (hipMemcpy(h.data(), dev, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  for (int i = 0; i < 24; ++i) out[i] = 0;
  for (size_t w = 0; w < (size_t)PEDN_PHASE_WAVES; ++w)
    for (int i = 0; i < 24; ++i) out[i] += h[w * 24 + i];
  return 0;
}
#endif
