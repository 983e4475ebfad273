// pedn_partition.hpp -- which links can ever hold a pedestrian?  Pure host C++ (no HIP call, no engine type): included by pedn_hip.hip
// for the dead-link plan of pedn_run, and by tests/partition_prog.cpp on its own.
//
// A pedestrian enters the network through the virtual in-link of a node whose demand row is not all +0.0 and moves from the incoming
// link of slot i of a node to the outgoing link of slot j only if the node's turning fraction (i, j) can be non-zero.  REACH is the
// closure of that relation over the directed physical links, decided from inputs the HOST knows -- which demand rows hold anything but
// +0.0, the shared turning fractions, the host-tabulated rows -- and assuming "possible" wherever it does not know (per-replica rows,
// rows computed on the device, the node LP).  A link outside REACH has inflow = outflow = +0.0 at every step, whatever the random draws:
// a zero sending flow times a finite fraction is +-0.0 or NaN, the node model floors and clamps that to +0.0 (node_step in
// pedn_kernels.hpp), and a fraction that is exactly +-0.0 turns any finite sending flow into +-0.0 the same way.
// Two more sources, both found by tests/test_gpu_dead_links_random.py:
//   * a link whose front gate may be negative (a negative shared value, or per-replica values the host does not follow): its sending
//     flow is min(gate * capacity, ...) < 0 even while it is empty, and a one-to-one node hands min(s, r) on unclamped -- the link fills
//     with the pedestrians its negative outflow invents and its neighbour gets a negative inflow;
//   * a link that an EARLIER state of the inputs has reached since the histories were last cleared (Model::seed_links): its pedestrians
//     are still walking when a demand row is zeroed or a turn is closed behind them, and a turn opened in front of them lets them on.
//   LIVE  the nodes incident to a link of REACH, and the nodes whose own demand row is non-zero
//   DEAD  the physical links whose head node (the node whose slot owns the link as its incoming link) is not in LIVE -- then no link at
//         that node, in either direction, is in REACH -- narrowed to whole nodes all of whose corridors the lean kernel can step
//         (eligibility, below): dead_link_kernel steps those, node_kernel<LU> the rest.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

namespace pedn_part {

// exactly +-0.0: the only fractions through which nothing can pass (a NaN means "differs between replicas": possible)
static inline bool is_zero(double x) {
  uint64_t b;
  memcpy(&b, &x, 8);
  return (b << 1) == 0;
}
// anything but +0.0, by the bits (-0.0 and NaN count as a value)
static inline bool not_plus_zero(double x) {
  uint64_t b;
  memcpy(&b, &x, 8);
  return b != 0;
}

struct Model {
  // topology as in pedn_model_desc: slots [node_slot_ptr[n], node_slot_ptr[n + 1]) of node n, slot k pairs the incoming link slot_in[k]
  // with the outgoing link slot_out[k] (both >= n_links: a virtual pair); turn (i, jj) of node n is node_turn_ptr[n] + i * (m - 1) + jj,
  // jj counting the out-slots j != i in ascending order
  int32_t n_nodes = 0, n_links = 0;
  const int32_t *node_slot_ptr = nullptr, *node_turn_ptr = nullptr, *node_kind = nullptr, *node_demand_row = nullptr;
  const int32_t *slot_in = nullptr, *slot_out = nullptr, *link_rev = nullptr;
  const int32_t* slot_dyn = nullptr;   // per slot: its row of fractions is 0 shared / per-replica static, 1 computed on the device, 2 tabulated on the host
  bool node_lp = false;                // the LP node model: every turn is possible
  // what the host knows of the run-time inputs
  const char* demand_nz = nullptr;     // [demand rows] 1: the row may hold something else than +0.0 (as created, uploaded, or drawn on the device)
  const double* tf_u = nullptr;        // [turns] the fraction every replica shares, NaN: per-replica rows
  const char* tab_nz = nullptr;        // [turns] rows tabulated on the host: 1 unless the entry is +-0.0 at every step and no per-replica OD weights are set
  // eligibility of a corridor for the lean kernel
  const int32_t *link_sep = nullptr, *link_tau_sw = nullptr;
  const double *front_u = nullptr, *back_u = nullptr;   // [links] the gate every replica shares, NaN: per-replica
  const char* seed_links = nullptr;    // [links] links that may hold pedestrians already: REACH of the earlier proofs since the last full reset (nullptr: none)
  const char* link_rl = nullptr;       // [links] an RL action slot or a controller drives the link's gate (nullptr: none)
  bool per_replica_params = false;     // per-replica link parameters are in use (DevView.pr)
};

struct Result {
  std::vector<char> reach;       // [links]
  std::vector<char> live;        // [nodes]
  std::vector<char> dead_raw;    // [links] head node not in LIVE
  std::vector<char> node_dead;   // [nodes] not in LIVE and every corridor eligible: its slots are stepped by dead_link_kernel
  std::vector<char> dead;        // [links] head node in node_dead
  int n_dead = 0;
};

// can a pedestrian pass from in-slot i to out-slot j (j != i) of node n?
static inline bool turn_possible(const Model& m, int n, int i, int j) {
  const int s0 = m.node_slot_ptr[n], d = m.node_slot_ptr[n + 1] - s0;
  if (m.node_kind[n] == 0 || m.node_lp) return true;   // one-to-one node: everything goes on; LP: not decided here
  const int dyn = m.slot_dyn[s0 + i];
  if (dyn == 1) return true;
  const int tn = m.node_turn_ptr[n] + i * (d - 1) + (j < i ? j : j - 1);
  if (dyn == 2) return m.tab_nz[tn] != 0;
  return !is_zero(m.tf_u[tn]);
}

static inline bool gate_ok(double g) { return g == g && g >= 0.0 && g < __builtin_inf(); }
// a front gate that is, or in some replica may be, below zero: the link sends a negative flow (send_flow: min(gate * capacity, ...))
static inline bool front_may_be_negative(double g) { return !(g >= 0.0); }

// both directions of the corridor whose one direction is l
static inline bool corridor_eligible(const Model& m, int l) {
  if (m.per_replica_params) return false;
  const int pair[2] = {l, m.link_rev[l]};
  for (int l2 : pair) {
    if (m.link_sep[l2] || m.link_tau_sw[l2] < 1) return false;
    if (!gate_ok(m.front_u[l2]) || !gate_ok(m.back_u[l2])) return false;
    if (m.link_rl && m.link_rl[l2]) return false;
  }
  return true;
}

static inline Result partition(const Model& m) {
  const int N = m.n_nodes, L = m.n_links;
  Result out;
  out.reach.assign(L, 0);
  out.live.assign(N, 0);
  out.dead_raw.assign(L, 0);
  out.node_dead.assign(N, 0);
  out.dead.assign(L, 0);
  std::vector<int32_t> head(L, -1), head_slot(L, -1);   // the node and slot that own link l as their incoming link
  for (int n = 0; n < N; ++n)
    for (int k = m.node_slot_ptr[n]; k < m.node_slot_ptr[n + 1]; ++k)
      if (m.slot_in[k] < L) { head[m.slot_in[k]] = n; head_slot[m.slot_in[k]] = k - m.node_slot_ptr[n]; }
  std::vector<int32_t> todo;
  auto spread = [&](int n, int i) {   // in-slot i of node n carries pedestrians
    const int s0 = m.node_slot_ptr[n], d = m.node_slot_ptr[n + 1] - s0;
    for (int j = 0; j < d; ++j) {
      const int lo = m.slot_out[s0 + j];
      if (j == i || lo >= L || out.reach[lo] || !turn_possible(m, n, i, j)) continue;
      out.reach[lo] = 1;
      todo.push_back(lo);
    }
  };
  for (int n = 0; n < N; ++n) {
    const int row = m.node_demand_row[n];
    if (row < 0 || !m.demand_nz[row]) continue;
    for (int k = m.node_slot_ptr[n]; k < m.node_slot_ptr[n + 1]; ++k)
      if (m.slot_in[k] >= L) { out.live[n] = 1; spread(n, k - m.node_slot_ptr[n]); }
  }
  for (int l = 0; l < L; ++l)
    if (!out.reach[l] && ((m.seed_links && m.seed_links[l]) || front_may_be_negative(m.front_u[l]))) {
      out.reach[l] = 1;
      todo.push_back(l);
    }
  while (!todo.empty()) {
    const int l = todo.back();
    todo.pop_back();
    if (head[l] >= 0) spread(head[l], head_slot[l]);
  }
  for (int l = 0; l < L; ++l)
    if (out.reach[l]) {
      if (head[l] >= 0) out.live[head[l]] = 1;
      if (head[m.link_rev[l]] >= 0) out.live[head[m.link_rev[l]]] = 1;
    }
  for (int n = 0; n < N; ++n) {
    bool ok = !out.live[n], any = false;
    for (int k = m.node_slot_ptr[n]; k < m.node_slot_ptr[n + 1] && ok; ++k)
      if (m.slot_in[k] < L) { any = true; ok = corridor_eligible(m, m.slot_in[k]); }
    out.node_dead[n] = ok && any;
  }
  for (int l = 0; l < L; ++l) {
    out.dead_raw[l] = head[l] >= 0 && !out.live[head[l]];
    out.dead[l] = head[l] >= 0 && out.node_dead[head[l]];
    out.n_dead += out.dead[l];
  }
  return out;
}

}  // namespace pedn_part
