// pedn_compile.hpp -- the model compiler: everything pedn_create derives from a pedn_model_desc before it touches the device.  Pure host
// C++ (no HIP API call, no engine handle): included by pedn_hip.hip, whose pedn_create uploads the tables and chooses the launch plan from
// them, and by tests/compile_prog.cpp on its own (host sanitizers).
//
//   validate   every refusal that needs neither a device nor a compiled table
//   compile    the static tables (Tables) and the refusals found while building them
//   pack       first-fit of an ordered node list into node_kernel's blocks of eight waves: compile packs every node (Tables::full),
//              dl_refresh in pedn_hip.hip packs the live nodes from the full packing's records
// Every failure returns PEDN_E_ARG with its message in *err.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pedn_partition.hpp"
#include "pedn_types.hpp"

namespace pedn_compile {

// The diagnostics knobs the compiler reads (the knobs that choose a launch plan are pedn_create's own).
struct Options {
  int tf_lds_limit = PEDN_TF_LDS_ROWS;   // PEDN_TF_LDS_LIMIT=n: a row gets at most n LDS rows (the rest goes to ent_p)
  int tf_heavy_groups = 2;               // PEDN_TF_HEAVY_GROUPS: a quad whose first row has more groups is dispatched in front of the link update
  int pack_by_load = 2;                  // PEDN_PACK_BY_LOAD=0: bins ordered by degree only, =1: by the static estimate even when a measured cost is given
  bool general_degree = false;           // PEDN_NODE_MD=8: report max_degree 8 (the general instantiation of the node kernels)
};

static inline Options options_from_env() {
  Options o;
  if (const char* d = getenv("PEDN_TF_LDS_LIMIT")) o.tf_lds_limit = std::max(0, std::min(atoi(d), PEDN_TF_LDS_ROWS));
  if (const char* d = getenv("PEDN_TF_HEAVY_GROUPS")) o.tf_heavy_groups = atoi(d);
  if (const char* f = getenv("PEDN_PACK_BY_LOAD")) o.pack_by_load = std::min(atoi(f), 2);
  if (const char* f = getenv("PEDN_NODE_MD")) o.general_degree = atoi(f) == 8;
  return o;
}

static inline int refuse(std::string* err, const std::string& msg) {
  if (err) *err = msg;
  return PEDN_E_ARG;
}

// ---- packing: slot records of node_kernel, block b = records [8 b, 8 b + 8)
struct Packing {
  std::vector<SlotRec> rec;   // (n_blocks + 1) x 8: one block of idle records behind the bins (prewarm_chains launches it)
  int n_blocks = 0;
  int tiles = 1;              // m * m LDS tiles of the fullest block, at least 1
  int n_lp = 0, lp_max_m = 0;   // nodes numbered for the node LP and the largest of them (number_lp)
};

static inline SlotRec idle_record() {
  SlotRec R{};
  R.node = -1; R.trow = -1; R.act = -1; R.lp = -1; R.mirror = -1;
  return R;
}

// First-fit of the nodes of `order` (but those with skip[n] != 0; skip may be null) into bins of 8 waves, a node's slots consecutive
// waves of one block.  rec_of(n, k) gives the record of slot k of node n; base, mirror and (number_lp) lp are set here.
//   base    running sum of d * d inside the block: the node's first LDS tile (<= 64 tiles because sum(d) <= 8)
//   mirror  of a physical slot: the position whose incoming link is its outgoing link; absent_mirrors_self (the live packing of the
//           dead-link plan): a slot whose corridor's other end is not in this packing mirrors itself.  -1 for virtual pairs and idle records.
//   lp      regular nodes numbered in position order on their slot 0 (the node LP's workspace)
template <class RecOf>
static inline Packing pack(const std::vector<int32_t>& order, const int32_t* node_slot_ptr, const char* skip, int L, bool absent_mirrors_self,
                           bool number_lp, RecOf rec_of) {
  auto deg = [&](int n) { return node_slot_ptr[n + 1] - node_slot_ptr[n]; };
  std::vector<std::vector<int>> bins;
  std::vector<int> fill;
  for (int n : order) {
    if (skip && skip[n]) continue;
    int d = deg(n), chosen = -1;
    for (size_t b = 0; b < bins.size(); ++b)
      if (fill[b] + d <= 8) { chosen = (int)b; break; }
    if (chosen < 0) { bins.emplace_back(); fill.push_back(0); chosen = (int)bins.size() - 1; }
    bins[chosen].push_back(n);
    fill[chosen] += d;
  }
  Packing P;
  P.n_blocks = (int)bins.size();
  P.rec.assign((bins.size() + 1) * 8, idle_record());
  for (size_t b = 0; b < bins.size(); ++b) {
    int wave = 0, base = 0;
    for (int n : bins[b]) {
      const int d = deg(n);
      for (int k = 0; k < d; ++k) {
        SlotRec& R = P.rec[b * 8 + wave++];
        R = rec_of(n, k);
        R.base = base;
      }
      base += d * d;
    }
    P.tiles = std::max(P.tiles, base);
  }
  std::vector<int32_t> pos_of(std::max(L, 1), -1);   // every physical link is the incoming link of one slot
  for (size_t i = 0; i < P.rec.size(); ++i)
    if (P.rec[i].node >= 0 && P.rec[i].lin < L) pos_of[P.rec[i].lin] = (int32_t)i;
  for (size_t i = 0; i < P.rec.size(); ++i) {
    SlotRec& R = P.rec[i];
    const bool physical = R.node >= 0 && R.lin < L && R.lout < L;
    R.mirror = !physical ? -1 : pos_of[R.lout] >= 0 || !absent_mirrors_self ? pos_of[R.lout] : (int32_t)i;
    if (number_lp && R.node >= 0 && R.kind == 1 && R.slot == 0) { R.lp = P.n_lp++; P.lp_max_m = std::max(P.lp_max_m, R.m); }
  }
  return P;
}

// ---- what compile produces
struct Tables {
  std::vector<LinkP> lp;          // [max(L, 1)]
  std::vector<CorrRec> corr;      // corridors: one lane of link_kernel updates both directions
  int pairs_adj = 1;              // DevView.pairs_adj
  // history rows (DevView.m64 / m32): the masks and the rows each field keeps (T + 1, or the size of its ring in recent-history mode)
  int32_t m64[7], m32[6];
  int rows64[7], rows32[6];
  // route choice: [n_pair] the product is the constant 1; [n_turns] every product of the turn is; per slot SlotRec.dyn and SlotRec.trow
  std::vector<int32_t> pair_const, turn_mode, slot_dyn, slot_trow;
  std::vector<int32_t> trow_words;   // [n_trow][PEDN_TROW_WORDS] (pedn_types.hpp)
  std::vector<int32_t> tgrp_words;   // [n_multi + 8][32]: turn_frac_body reads a chunk of four records ahead; padding has n = 0
  std::vector<int32_t> pair_row;     // [n_pair] DevView.pair_row
  int n_multi = 0, n_trow = 0, n_over = 0;   // n_over: rows of ent_p, for probabilities beyond a workgroup's LDS rows
  int n_tf_heavy_quads = 0;
  bool inline_tf_ok = false;         // every device-computed row is short enough for the single-launch plan (pedn_plan::PlanInputs.inline_tf_ok)
  std::vector<char> demand_nz;       // [max(n_demand, 1)] the row holds something else than +0.0
  std::vector<int32_t> pack_order;   // nodes in the order the bins were packed in
  int packed_by = 1;                 // 0 by degree, 1 by the static load estimate, 2 by measured cost
  int max_degree = 0;
  Packing full;                      // every node
};

static inline int validate(const pedn_model_desc& md, int n_replicas, std::string* err) {
  const pedn_model_desc* m = &md;
  if (m->abi_version != PEDN_ABI_VERSION) return refuse(err, "pedn_model_desc.abi_version mismatch");
  if (n_replicas < 1 || m->n_nodes < 1 || m->n_links < 0 || m->T < 2 || m->window < 1) return refuse(err, "bad sizes in model description");
  const int N = m->n_nodes, L = m->n_links;
  // ---- the topology against what the kernels assume
  for (int n = 0; n < N; ++n) {
    int deg = m->node_slot_ptr[n + 1] - m->node_slot_ptr[n];
    if (deg < 2 || deg > PEDN_MAX_DEGREE)
      return refuse(err, "node degree " + std::to_string(deg) + " outside 2.." + std::to_string(PEDN_MAX_DEGREE));
    if (m->node_kind[n] == 0 && deg != 2) return refuse(err, "one-to-one node with degree != 2");
    if (m->node_turn_ptr[n + 1] - m->node_turn_ptr[n] != deg * (deg - 1)) return refuse(err, "node_turn_ptr inconsistent");
    for (int k = m->node_slot_ptr[n]; k < m->node_slot_ptr[n + 1]; ++k) {
      int li = m->slot_in_link[k], lo = m->slot_out_link[k];
      if (li < 0 || lo < 0 || li >= L + m->n_vlinks || lo >= L + m->n_vlinks) return refuse(err, "slot link index out of range");
      if ((li >= L) != (lo >= L)) return refuse(err, "virtual/physical mismatch in a slot");
      if (li < L && m->link_rev[li] != lo) return refuse(err, "slot does not hold a reverse pair");
      if (li >= L && (m->node_demand_row[n] < 0 || m->node_demand_row[n] >= m->n_demand)) return refuse(err, "virtual slot without demand row");
    }
  }
  for (int l = 0; l < L; ++l) {
    int rv = m->link_rev[l];
    if (rv < 0 || rv >= L || rv == l || m->link_rev[rv] != l) return refuse(err, "link_rev is not an involution");
    if (m->link_fd[l] < 0 || m->link_fd[l] > 2) return refuse(err, "unknown fundamental diagram type");
  }
  for (int g = 0; g < m->n_grp; ++g)
    if (m->grp_ent_ptr[g + 1] - m->grp_ent_ptr[g] > PEDN_MAX_DEGREE - 1) return refuse(err, "softmax group too large");

  if (m->history_mode != PEDN_HIST_FULL && m->history_mode != PEDN_HIST_RECENT) return refuse(err, "unknown history_mode");
  if (m->node_model != PEDN_NODE_CLASSIC && m->node_model != PEDN_NODE_OPTIMAL) return refuse(err, "unknown node_model");
  // node_step forms the element offset of a column inside a history row, col * RS + r0, and the elements of a row in 32 bits (rowq / rowd in
  // pedn_kernels.hpp).  A row of 2^31 elements would be 16 GB of every binary64 field per step: no full-record or ring allocation that fits a
  // device comes near it, so such a batch is refused here instead of being given a 64-bit path of its own.
  if (((size_t)L + (size_t)m->n_vlinks) * (((size_t)n_replicas + 127) / 128 * 128) >= ((size_t)1 << 31))
    return refuse(err, "links x replicas must stay below 2^31 (one history row)");
  return PEDN_OK;
}

// of a model that validate accepts
static inline int compile(const pedn_model_desc& md, const Options& opt, Tables* out, std::string* err) {
  const pedn_model_desc* m = &md;
  Tables& t = *out;
  const int N = m->n_nodes, L = m->n_links, T1 = m->T + 1;
  const int n_slots = m->node_slot_ptr[N];
  {  // history rows
    const int FULL = 0x7fffffff;
    auto ring = [&](int need) {  // power-of-two ring of at least `need` rows, or all rows when that is no saving
      int p = 1;
      while (p < need) p <<= 1;
      return p >= T1 ? FULL : p - 1;
    };
    for (int f = 0; f < 7; ++f) t.m64[f] = FULL;
    for (int g = 0; g < 6; ++g) t.m32[g] = FULL;
    if (m->history_mode == PEDN_HIST_RECENT) {
      int max_sw = 0;
      for (int l = 0; l < L; ++l) max_sw = std::max(max_sw, m->link_tau_sw[l]);
      // cumulative_outflow[t' + 1 - tau_shockwave] (link.py:380-390) and [t'], with room for the per-replica scenarios of the
      // randomisers: free_flow_speed x U(0.6, 0.9) stretches the shock-wave look-back by up to 1 / 0.6 (env_loader.py:410-412; the
      // k_critical / k_jam factor cancels in the shock-wave speed unless a floor binds -- then pedn_set_link_params /
      // pedn_randomize_scenarios refuse the scenario)
      // (a look-back of x.5 before rounding divided by 0.6 can round one further up than max_sw / 0.6: sized for that)
      t.m64[F_CO] = ring((int)ceil(((double)max_sw + 0.5) / 0.6) + 2);
      t.m64[F_OUT] = t.m64[F_S] = t.m64[F_R] = t.m64[F_GATE] = ring(4);   // [t], [t-1], [t-2] at most
      t.m32[G_TT] = ring(m->window + 2);        // travel_time[t - W] leaves the moving average (link.py:183-186)
      t.m32[G_ATT] = t.m32[G_N] = t.m32[G_K] = t.m32[G_V] = t.m32[G_LF] = ring(4);
    }
    for (int f = 0; f < 7; ++f) t.rows64[f] = t.m64[f] == FULL ? T1 : t.m64[f] + 1;
    for (int g = 0; g < 6; ++g) t.rows32[g] = t.m32[g] == FULL ? T1 : t.m32[g] + 1;
  }
  t.demand_nz.assign(std::max(m->n_demand, 1), 0);
  for (int row = 0; row < m->n_demand; ++row)
    for (int k = 0; k < T1 && !t.demand_nz[row]; ++k) t.demand_nz[row] = pedn_part::not_plus_zero(m->demand[(size_t)row * T1 + k]);
  std::vector<LinkP>& lp = t.lp;
  lp.assign(std::max(L, 1), LinkP{});
  for (int l = 0; l < L; ++l) {
    LinkP& P = lp[l];
    P.length = m->link_length[l]; P.width = m->link_width[l]; P.vf = m->link_vf[l]; P.kc = m->link_kc[l]; P.kj = m->link_kj[l];
    P.gamma = m->link_gamma[l]; P.act = m->link_act[l]; P.bi = m->link_bi[l]; P.noise = m->link_noise[l];
    P.tt0 = m->link_tt0[l]; P.rev = m->link_rev[l]; P.sep = m->link_sep[l]; P.fd = m->link_fd[l];
    P.tau_sw = m->link_tau_sw[l]; P.fft = m->link_fft[l]; P.pad = 0;
    P.derive();
  }
  {  // every softmax entry feeds exactly one (turn, od) product: store probabilities in product order
    std::vector<int32_t> ent_pair(std::max(m->n_ent, 1), -1);
    for (int q = 0; q < m->n_pair; ++q) {
      int e = m->pair_ent[q];
      if (e < 0 || e >= m->n_ent || ent_pair[e] != -1) return refuse(err, "pair_ent is not injective");
      ent_pair[e] = q;
    }
    // exp(x)/exp(x) == 1 exactly as long as exp(x) is finite and non-zero; |x| <= temp * (|alpha| + |beta|*k_max/8 + |omega| + |eps|)
    const double xmax = fabs(m->pf_temp) * (fabs(m->pf_alpha) + fabs(m->pf_beta) * 16.0 + fabs(m->pf_omega) + fabs(m->pf_eps));
    const bool shortcut = xmax < 600.0;
    std::vector<int32_t>& pconst = t.pair_const;
    pconst.assign(std::max(m->n_pair, 1), 0);
    for (int g = 0; g < m->n_grp; ++g)
      if (m->grp_ent_ptr[g + 1] - m->grp_ent_ptr[g] == 1 && shortcut && ent_pair[m->grp_ent_ptr[g]] >= 0) pconst[ent_pair[m->grp_ent_ptr[g]]] = 1;
    t.turn_mode.assign(std::max(m->n_turns, 1), 0);
    for (int tn = 0; tn < m->n_turns; ++tn) {
      bool all_const = true;   // a turn without products is the constant 0
      for (int q = m->turn_pair_ptr[tn]; q < m->turn_pair_ptr[tn + 1]; ++q) all_const = all_const && pconst[q];
      t.turn_mode[tn] = all_const ? 1 : 0;
    }
    // row (incoming slot) of its node every softmax group belongs to, read off its products: the product (od, up, down) is
    // summed into the turn (up, down) (path_finder.py:668-686); a group none of whose entries feeds a product is never needed
    std::vector<int> grp_row(std::max(m->n_grp, 1), -1);
    for (int g = 0; g < m->n_grp; ++g) {
      const int n = m->grp_node[g];
      if (n < 0 || n >= N || g < m->node_grp_ptr[n] || g >= m->node_grp_ptr[n + 1]) return refuse(err, "grp_node / node_grp_ptr inconsistent");
      const int d = m->node_slot_ptr[n + 1] - m->node_slot_ptr[n];
      for (int e = m->grp_ent_ptr[g]; e < m->grp_ent_ptr[g + 1]; ++e) {
        if (ent_pair[e] < 0) continue;
        const int tn = (int)(std::upper_bound(m->turn_pair_ptr, m->turn_pair_ptr + m->n_turns + 1, ent_pair[e]) - m->turn_pair_ptr) - 1;
        const int row = (tn - m->node_turn_ptr[n]) / (d - 1);
        if (tn < m->node_turn_ptr[n] || tn >= m->node_turn_ptr[n + 1] || (grp_row[g] >= 0 && grp_row[g] != row))
          return refuse(err, "products of one softmax group lie in different rows");
        grp_row[g] = row;
      }
    }
    // Rows (incoming slots) of dynamic nodes.  A row whose turns are all mode 1 (every product constant) has fractions that
    // depend on the OD weights only: tabulated and renormalised on the host (tabulate_pair_pod), SlotRec.dyn = 2.  The others
    // get one record each for turn_frac_kernel -- see pedn_types.hpp for the word layout -- and SlotRec.dyn = 1.
    struct Row { int node, i, cost, need, groups; };
    std::vector<Row> rows;
    t.slot_dyn.assign(n_slots, 0);
    for (int n = 0; n < N; ++n) {
      if (m->node_kind[n] != 1 || !m->node_dyn[n]) continue;
      const int d = m->node_slot_ptr[n + 1] - m->node_slot_ptr[n];
      for (int i = 0; i < d; ++i) {
        const int ta = m->node_turn_ptr[n] + i * (d - 1), tb = ta + d - 1;
        int need = 0;
        for (int q = m->turn_pair_ptr[ta]; q < m->turn_pair_ptr[tb]; ++q) need += pconst[q] ? 0 : 1;
        t.slot_dyn[m->node_slot_ptr[n] + i] = need ? 1 : 2;
        if (!need) continue;
        int cost = m->turn_pair_ptr[tb] - m->turn_pair_ptr[ta], groups = 0;
        for (int g = m->node_grp_ptr[n]; g < m->node_grp_ptr[n + 1]; ++g)
          if (grp_row[g] == i && (m->grp_ent_ptr[g + 1] - m->grp_ent_ptr[g] > 1 || !shortcut)) ++groups;
        cost += 16 * groups;  // a group costs two divisions and an exp per downstream
        rows.push_back(Row{n, i, cost, need, groups});
      }
    }
    // workgroups of four rows, heaviest first (they start first); the rows of a workgroup share its PEDN_TF_LDS_ROWS LDS rows
    std::stable_sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) { return a.cost > b.cost; });
    std::vector<Row> packed;
    std::vector<int> lds_base;
    const int coop_groups = PEDN_TF_COOP_GROUPS;  // rows with more multi-entry groups get a workgroup of their own (2..12 measured: 8 best)
    const int lds_limit = opt.tf_lds_limit;
    {
      std::vector<char> taken(rows.size(), 0);
      for (size_t a0 = 0; a0 < rows.size(); ++a0) {
        if (taken[a0]) continue;
        if (rows[a0].groups > coop_groups) {  // a workgroup of its own: four records of the same row (coop)
          taken[a0] = 1;
          for (int k = 0; k < 4; ++k) { packed.push_back(rows[a0]); lds_base.push_back(0); }
          continue;
        }
        int fill = 0, cnt = 0;
        for (size_t k = a0; k < rows.size() && cnt < 4; ++k) {
          if (taken[k] || rows[k].groups > coop_groups) continue;
          const int need = std::min(rows[k].need, lds_limit);
          if (k != a0 && fill + need > PEDN_TF_LDS_ROWS) continue;
          taken[k] = 1;
          packed.push_back(rows[k]);
          lds_base.push_back(fill);
          fill += need;
          ++cnt;
        }
        for (; cnt < 4; ++cnt) { packed.push_back(Row{-1, 0, 0, 0, 0}); lds_base.push_back(0); }
      }
    }
    t.slot_trow.assign(n_slots, -1);
    t.inline_tf_ok = !packed.empty();
    std::vector<int32_t>& rwords = t.trow_words;
    std::vector<int32_t>& gwords = t.tgrp_words;
    std::vector<int32_t>& prow = t.pair_row;   // product -> where its probability is, -1: the constant 1
    rwords.assign(std::max<size_t>(packed.size(), 1) * PEDN_TROW_WORDS, 0);
    gwords.clear();
    prow.assign(std::max(m->n_pair, 1), -1);
    int n_over = 0, n_multi = 0;
    auto put_d = [](int32_t* w, double x) { memcpy(w, &x, 8); };
    auto put_f = [](int32_t* w, float x) { memcpy(w, &x, 4); };
    for (size_t ri = 0; ri < packed.size(); ++ri) {
      const int n = packed[ri].node, i = packed[ri].i;
      int32_t* w = &rwords[ri * PEDN_TROW_WORDS];
      if (n < 0) { w[0] = -1; continue; }
      if (ri % 4 != 0 && packed[ri - 1].node == n && packed[ri - 1].i == i) {  // coop: copy of the workgroup's first record
        std::copy(w - PEDN_TROW_WORDS, w, w);
        continue;
      }
      const int s0 = m->node_slot_ptr[n], d = m->node_slot_ptr[n + 1] - s0;
      const int ta = m->node_turn_ptr[n] + i * (d - 1);
      w[0] = d; w[1] = ta; w[2] = n_multi; w[4] = m->turn_pair_ptr[ta]; w[5] = m->turn_pair_ptr[ta + d - 1];
      for (int jj = 0; jj < d - 1; ++jj) {
        w[84 + 3 * jj] = m->turn_pair_ptr[ta + jj]; w[85 + 3 * jj] = m->turn_pair_ptr[ta + jj + 1]; w[86 + 3 * jj] = t.turn_mode[ta + jj];
      }
      std::vector<int> used;  // outgoing slots this row's multi-entry groups refer to
      int n_prob = 0, n_g = 0, any_sep = 0, over = 0;
      const int lds_rows = std::min(packed[ri].need, lds_limit);
      for (int g = m->node_grp_ptr[n]; g < m->node_grp_ptr[n + 1]; ++g) {
        const int a = m->grp_ent_ptr[g], b = m->grp_ent_ptr[g + 1];
        if (grp_row[g] != i || b - a < 1 || (b - a == 1 && shortcut)) continue;
        double sumd = 0.0;
        for (int e = a; e < b; ++e) sumd = (e == a) ? m->ent_dist[e] : sumd + m->ent_dist[e];
        gwords.resize(gwords.size() + 32, 0);
        int32_t* G = &gwords[gwords.size() - 32];
        G[0] = b - a; G[1] = m->grp_allphys[g];
        for (int k = 0; k < PEDN_MAX_DEGREE - 1; ++k) G[2 + k] = G[9 + k] = -1;
        for (int e = a; e < b; ++e) {
          const int k = e - a, l = m->ent_link[e];
          if (l >= 0) {
            int slot = -1;
            for (int j = 0; j < d; ++j)
              if (l < L && m->slot_out_link[s0 + j] == l) slot = j;
            if (slot < 0) return refuse(err, "softmax entry is not an outgoing link of its node");
            size_t u = std::find(used.begin(), used.end(), slot) - used.begin();
            if (u == used.size()) used.push_back(slot);
            G[2 + k] = (int)u;
          }
          if (ent_pair[e] >= 0) {
            if (n_prob < lds_rows) G[9 + k] = lds_base[ri] + n_prob;
            else { G[9 + k] = PEDN_TF_LDS_ROWS + n_over++; over = 1; }
            ++n_prob;
            prow[ent_pair[e]] = G[9 + k];
          }
          put_d(&G[16 + 2 * k], (m->pf_alpha * m->ent_dist[e]) / (sumd + 1e-6));
        }
        ++n_g; ++n_multi;
      }
      if (used.size() > (size_t)(PEDN_MAX_DEGREE - 1)) return refuse(err, "a row refers to more than 7 downstream links");
      for (int e = 0; e < PEDN_MAX_DEGREE - 1; ++e) {
        const int slot = used.empty() ? -1 : used[e < (int)used.size() ? e : 0];
        int32_t* E = e < 5 ? &w[8 + 10 * e] : &w[64 + 10 * (e - 5)];
        const int l = slot >= 0 ? m->slot_out_link[s0 + slot] : 0;  // only rows with groups come here, and L > 0 then
        E[0] = l; E[1] = m->link_rev[l]; E[2] = m->link_sep[l];
        put_f(&E[3], (float)(m->link_length[l] * m->link_width[l]));
        put_d(&E[4], m->link_vf[l]); put_d(&E[6], m->link_kc[l]); put_d(&E[8], m->link_length[l]);
        if (slot >= 0 && E[2]) any_sep = 1;
      }
      w[3] = n_g; w[6] = (int)used.size(); w[7] = any_sep; w[107] = over; w[108] = packed[ri].groups > coop_groups;
      w[109] = lds_base[ri];
      t.slot_trow[s0 + i] = (int)ri;
      if (over || packed[ri].groups > coop_groups || lds_rows > PEDN_TF_INL_ROWS) t.inline_tf_ok = false;
    }
    gwords.resize(gwords.size() + 8 * 32, 0);
    // the workgroups (quads of rows, heaviest first) whose dependent chains are longer than a link-update workgroup lasts: inside
    // link_turn_kernel they are dispatched in front of the link update, the short ones behind it (launch_step)
    t.n_tf_heavy_quads = 0;
    for (size_t q = 0; q * 4 < packed.size(); ++q)
      if (packed[q * 4].groups > opt.tf_heavy_groups) t.n_tf_heavy_quads = (int)q + 1;
    t.n_multi = n_multi;
    t.n_trow = (int)packed.size();
    t.n_over = n_over;
    for (int q = 0; q < m->n_pair; ++q)
      if (!pconst[q] && prow[q] < 0) return refuse(err, "(turn, od) product without a softmax entry on a dynamic node");
  }
  t.corr.clear();
  for (int l = 0; l < L; ++l)
    if (l < m->link_rev[l]) {
      CorrRec c{};
      c.a = l; c.b = m->link_rev[l]; c.Pa = lp[c.a]; c.Pb = lp[c.b];
      t.corr.push_back(c);
    }
  t.pairs_adj = 1;
  for (size_t p = 0; p < t.corr.size(); ++p)
    if (t.corr[p].a != 2 * (int)p || t.corr[p].b != 2 * (int)p + 1) t.pairs_adj = 0;
  {  // bin nodes into blocks of 8 waves: first-fit over the nodes ordered by (expected load, slot count) decreasing, so that
    // every block is full regardless of node degree.  The 8 waves of a block meet at two barriers, so a block lasts as long
    // as its slowest wave, and the slow waves are those of busy links (look-backs, diffusion, binomial draws).  The junctions
    // that many OD routes pass -- those with many (turn, od) products -- are the likely ones and go first (delft: 32.3 ->
    // 31.6 us; PEDN_PACK_BY_LOAD=0 orders by slot count only).  Re-packing at run time by the cost the waves measure
    // themselves (ticks up to the first barrier, sampled every 100 / 250 steps) was tried and changed nothing (30.5 us either
    // way): the spread inside a block comes from step-to-step variation, not from which junctions share it.
    // Better than the estimate: the MEASURED cost of every node's slowest wave (pedn_model_desc.node_cost, from a calibration run of
    // the profiling build, tools/pack_calibrate.py).  tools/pack_analysis.py: the wait at the first barrier is static (92 % of it is
    // explained by the waves' mean arrival times); half of it is a node's waves waiting for each other -- inherent --, the other half is
    // the packing's, and packing by measured cost removes at most half of that: 3.4-3.9 % of a wave's life.
    std::vector<int32_t>& order = t.pack_order;
    order.resize(N);
    std::vector<double> load(N, 0.0);
    for (int n = 0; n < N; ++n) order[n] = n;
    auto deg = [&](int n) { return m->node_slot_ptr[n + 1] - m->node_slot_ptr[n]; };
    const int by_load = std::min(opt.pack_by_load, m->node_cost ? 2 : 1);
    if (by_load == 2)
      for (int n = 0; n < N; ++n) load[n] = (double)m->node_cost[n];
    else if (by_load == 1)
      for (int n = 0; n < N; ++n) load[n] = m->turn_pair_ptr[m->node_turn_ptr[n + 1]] - m->turn_pair_ptr[m->node_turn_ptr[n]];
    t.packed_by = by_load;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return load[a] != load[b] ? load[a] > load[b] : deg(a) > deg(b); });
    t.full = pack(order, m->node_slot_ptr, nullptr, L, false, m->node_model == PEDN_NODE_OPTIMAL, [&](int n, int k) {
      const int sk = m->node_slot_ptr[n] + k;
      SlotRec R = idle_record();
      R.node = n; R.slot = k; R.m = deg(n);
      R.kind = m->node_kind[n]; R.dyn = t.slot_dyn[sk]; R.trow = t.slot_trow[sk];
      R.lin = m->slot_in_link[sk]; R.lout = m->slot_out_link[sk];
      R.turn0 = m->node_turn_ptr[n];
      R.demand_row = m->node_demand_row[n];
      if (R.lin < L) { R.Pin = lp[R.lin]; R.Pout = lp[R.lout]; }
      return R;
    });
    t.max_degree = 0;
    for (int n = 0; n < N; ++n) t.max_degree = std::max(t.max_degree, deg(n));
    if (opt.general_degree) t.max_degree = 8;
  }
  return PEDN_OK;
}

}  // namespace pedn_compile
