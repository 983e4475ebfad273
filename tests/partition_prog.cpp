// Stand-alone driver of pedn_partition.hpp (the host proof behind the dead-link plan); built by tests/test_partition_host.py with the
// host compiler and -fsanitize=address,undefined.
//   partition_prog selftest        hand-made models, exits non-zero on the first wrong answer
//   partition_prog model <file>    a model as written by tests/partition_model.py; prints reach / live / dead_raw / node_dead / dead
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <utility>
#include <vector>

#include "../pednstream_amd/csrc/pedn_partition.hpp"

using pedn_part::Model;
using pedn_part::Result;

// a small network: undirected edges become the directed links (2e, 2e + 1); node n owns one slot per incident corridor, in edge order,
// and a virtual pair behind them when it is an origin / destination
struct Net {
  int N = 0, L = 0, n_demand = 0;
  std::vector<int32_t> slot_ptr{0}, turn_ptr{0}, kind, demand_row, slot_in, slot_out, rev, slot_dyn, sep, tau_sw;
  std::vector<char> demand_nz, tab_nz, rl;
  std::vector<double> tf_u, front, back;
  bool node_lp = false, pr = false;
  Net(int n_nodes, const std::vector<std::pair<int, int>>& edges, const std::vector<int>& virt, const std::vector<int>& one_to_one) {
    N = n_nodes;
    L = 2 * (int)edges.size();
    int vl = L;
    for (size_t e = 0; e < edges.size(); ++e) { rev.push_back(2 * (int)e + 1); rev.push_back(2 * (int)e); }
    for (int n = 0; n < N; ++n) {
      for (size_t e = 0; e < edges.size(); ++e) {
        if (edges[e].second == n) { slot_in.push_back(2 * (int)e); slot_out.push_back(2 * (int)e + 1); }      // u -> v is link 2e
        else if (edges[e].first == n) { slot_in.push_back(2 * (int)e + 1); slot_out.push_back(2 * (int)e); }
      }
      bool v = false;
      for (int x : virt) v = v || x == n;
      if (v) { slot_in.push_back(vl); slot_out.push_back(vl + 1); vl += 2; demand_row.push_back(n_demand++); }
      else demand_row.push_back(-1);
      const int d = (int)slot_in.size() - slot_ptr.back();
      slot_ptr.push_back((int)slot_in.size());
      turn_ptr.push_back(turn_ptr.back() + d * (d - 1));
      bool o = false;
      for (int x : one_to_one) o = o || x == n;
      kind.push_back(o ? 0 : 1);
    }
    slot_dyn.assign(slot_in.size(), 0);
    sep.assign(L, 0);
    tau_sw.assign(L, 3);
    rl.assign(L, 0);
    front.assign(L, 2.0);
    back.assign(L, 2.0);
    demand_nz.assign(n_demand, 0);
    tf_u.assign(turn_ptr.back(), 0.5);
    tab_nz.assign(turn_ptr.back(), 1);
  }
  int link(int u, int v, const std::vector<std::pair<int, int>>& edges) const {
    for (size_t e = 0; e < edges.size(); ++e) {
      if (edges[e].first == u && edges[e].second == v) return 2 * (int)e;
      if (edges[e].first == v && edges[e].second == u) return 2 * (int)e + 1;
    }
    return -1;
  }
  // turn index of (incoming link lin -> outgoing link lout) at node n
  int turn(int n, int lin, int lout) const {
    const int s0 = slot_ptr[n], d = slot_ptr[n + 1] - s0;
    int i = -1, j = -1;
    for (int k = 0; k < d; ++k) { if (slot_in[s0 + k] == lin) i = k; if (slot_out[s0 + k] == lout) j = k; }
    return turn_ptr[n] + i * (d - 1) + (j < i ? j : j - 1);
  }
  int slot_of(int n, int lin) const {
    for (int k = slot_ptr[n]; k < slot_ptr[n + 1]; ++k) if (slot_in[k] == lin) return k;
    return -1;
  }
  Model model() const {
    Model m;
    m.n_nodes = N; m.n_links = L;
    m.node_slot_ptr = slot_ptr.data(); m.node_turn_ptr = turn_ptr.data(); m.node_kind = kind.data(); m.node_demand_row = demand_row.data();
    m.slot_in = slot_in.data(); m.slot_out = slot_out.data(); m.link_rev = rev.data(); m.slot_dyn = slot_dyn.data(); m.node_lp = node_lp;
    m.demand_nz = demand_nz.data(); m.tf_u = tf_u.data(); m.tab_nz = tab_nz.data();
    m.link_sep = sep.data(); m.link_tau_sw = tau_sw.data(); m.front_u = front.data(); m.back_u = back.data(); m.link_rl = rl.data();
    m.per_replica_params = pr;
    return m;
  }
};

static int failures = 0;
static std::string ones(const std::vector<char>& v) {
  std::string s;
  for (size_t i = 0; i < v.size(); ++i) if (v[i]) s += (s.empty() ? "" : " ") + std::to_string(i);
  return s;
}
static void expect(const char* what, const std::vector<char>& got, const std::vector<int>& want) {
  std::vector<char> w(got.size(), 0);
  for (int x : want) w[x] = 1;
  if (w != got) { printf("FAIL %s: got {%s}, expected {%s}\n", what, ones(got).c_str(), ones(w).c_str()); ++failures; }
}

static int selftest() {
  {  // a line 0 - 1 - 2 - 3 with the origin at 0: every node sees pedestrians, nothing is dead
    const std::vector<std::pair<int, int>> E{{0, 1}, {1, 2}, {2, 3}};
    Net n(4, E, {0, 3}, {1, 2});
    n.demand_nz[0] = 1;
    const Result r = pedn_part::partition(n.model());
    expect("line reach", r.reach, {0, 2, 4});
    expect("line live", r.live, {0, 1, 2, 3});
    expect("line dead", r.dead, {});
    if (r.n_dead != 0) { printf("FAIL line n_dead\n"); ++failures; }
  }
  // a Y: origin 0 - junction 1; 1 - 2 (destination); 1 - 3 - 4 (destination behind a one-to-one node).  Links: 0->1 = 0, 1->0 = 1,
  // 1->2 = 2, 2->1 = 3, 1->3 = 4, 3->1 = 5, 3->4 = 6, 4->3 = 7
  const std::vector<std::pair<int, int>> Y{{0, 1}, {1, 2}, {1, 3}, {3, 4}};
  auto y = [&]() { Net n(5, Y, {0, 2, 4}, {3}); n.demand_nz[0] = 1; return n; };
  const double values[] = {0.0, -0.0, __builtin_nan(""), 1e-300};
  for (int k = 0; k < 4; ++k) {   // the fraction 0->1 -> 1->3: exactly +-0.0 closes the branch, NaN (per-replica rows) and 1e-300 do not
    Net n = y();
    n.tf_u[n.turn(1, 0, 4)] = values[k];
    const Result r = pedn_part::partition(n.model());
    if (k < 2) {
      expect("Y zero reach", r.reach, {0, 2});
      expect("Y zero live", r.live, {0, 1, 2});
      expect("Y zero dead_raw", r.dead_raw, {4, 6, 7});
      expect("Y zero node_dead", r.node_dead, {3, 4});
      expect("Y zero dead", r.dead, {4, 6, 7});
    } else {
      expect("Y open reach", r.reach, {0, 2, 4, 6});
      expect("Y open dead", r.dead, {});
    }
  }
  {  // the junction's row computed on the device: every turn possible, whatever the shared fraction says
    Net n = y();
    n.tf_u[n.turn(1, 0, 4)] = 0.0;
    n.slot_dyn[n.slot_of(1, 0)] = 1;
    expect("Y device row", pedn_part::partition(n.model()).dead, {});
    n.slot_dyn[n.slot_of(1, 0)] = 2;   // tabulated on the host: by the table, not by tf_u
    expect("Y table open", pedn_part::partition(n.model()).dead, {});
    n.tab_nz[n.turn(1, 0, 4)] = 0;
    expect("Y table closed", pedn_part::partition(n.model()).dead, {4, 6, 7});
    n.node_lp = true;
    expect("Y node LP", pedn_part::partition(n.model()).dead, {});
  }
  {  // a dynamic node UPSTREAM of the closed branch does not open it; a second demand row switched on only shrinks DEAD
    Net n = y();
    n.tf_u[n.turn(1, 0, 4)] = 0.0;
    n.slot_dyn[n.slot_of(0, n.slot_in[n.slot_ptr[0] + 1])] = 1;   // the origin's virtual slot
    const Result a = pedn_part::partition(n.model());
    expect("Y upstream dynamic", a.dead, {4, 6, 7});
    n.demand_nz[1] = 1;   // node 2 becomes an origin: 2->1, then 1->0 and 1->3, 3->4
    const Result b = pedn_part::partition(n.model());
    expect("Y second origin reach", b.reach, {0, 1, 2, 3, 4, 6});
    expect("Y second origin dead", b.dead, {});
    for (size_t l = 0; l < b.dead.size(); ++l) if (b.dead[l] && !a.dead[l]) { printf("FAIL DEAD grew\n"); ++failures; }
    n.demand_nz[1] = 0; n.demand_nz[2] = 1;   // node 4 instead: 4->3, 3->1, 1->0 and 1->2
    expect("Y origin behind the branch", pedn_part::partition(n.model()).dead, {});
  }
  for (int k = 0; k < 7; ++k) {   // what the lean kernel does not step goes back to the node kernel: corridor 1 - 3 fails, node 3 with it
    Net n = y();
    n.tf_u[n.turn(1, 0, 4)] = 0.0;
    const char* what = "";
    switch (k) {
      case 0: n.sep[5] = 1; what = "separator"; break;
      case 1: n.front[4] = -0.5; what = "negative gate"; break;
      case 2: n.rl[5] = 1; what = "action slot"; break;
      case 3: n.back[5] = __builtin_nan(""); what = "per-replica gate"; break;
      case 4: n.tau_sw[4] = 0; what = "zero shock-wave look-back"; break;
      case 5: n.front[5] = __builtin_inf(); what = "infinite gate"; break;
      default: n.pr = true; what = "per-replica parameters"; break;
    }
    const Result r = pedn_part::partition(n.model());
    if (k == 1) {   // a negative front gate makes 1->3 a source: it sends a negative flow through the one-to-one node 3 into 3->4
      expect("negative front gate reach", r.reach, {0, 2, 4, 6});
      expect("negative front gate dead", r.dead, {});
      continue;
    }
    expect(what, r.dead_raw, {4, 6, 7});
    if (k < 6) { expect(what, r.node_dead, {4}); expect(what, r.dead, {6}); }
    else expect(what, r.dead, {});
  }
  {  // a per-replica front gate may be negative somewhere; a negative BACK gate only closes the link (recv_flow clamps at 0)
    Net n = y();
    n.tf_u[n.turn(1, 0, 4)] = 0.0;
    n.back[4] = -1.0;
    expect("negative back gate", pedn_part::partition(n.model()).dead, {6});
    n.front[7] = __builtin_nan("");   // 4->3: through node 3 into 3->1, and on from junction 1
    const Result r = pedn_part::partition(n.model());
    expect("per-replica front gate reach", r.reach, {0, 1, 2, 5, 7});
    expect("per-replica front gate dead", r.dead, {});
  }
  {  // what an earlier proof has reached stays a source: the branch was open, pedestrians are on 1->3, then the turn into it is closed
    Net n = y();
    n.tf_u[n.turn(1, 0, 4)] = 0.0;
    std::vector<char> seen(n.L, 0);
    seen[4] = 1;
    Model m = n.model();
    m.seed_links = seen.data();
    const Result r = pedn_part::partition(m);
    expect("seeded reach", r.reach, {0, 2, 4, 6});
    expect("seeded dead", r.dead, {});
    n.demand_nz[0] = 0;   // ... and with the origin's row zeroed as well
    m = n.model();
    m.seed_links = seen.data();
    expect("seeded, no demand: reach", pedn_part::partition(m).reach, {4, 6});
    expect("seeded, no demand: dead", pedn_part::partition(m).dead, {1, 2});   // 1->0 and 1->2: nodes 0 and 2 see nobody
  }
  if (!failures) printf("selftest ok\n");
  return failures ? 1 : 0;
}

static int from_file(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { perror(path); return 2; }
  auto rd = [&]() { long long x = 0; if (fscanf(f, "%lld", &x) != 1) { fprintf(stderr, "short model file\n"); exit(2); } return x; };
  auto ints = [&](size_t n) { std::vector<int32_t> v(n); for (auto& x : v) x = (int32_t)rd(); return v; };
  auto flags = [&](size_t n) { std::vector<char> v(n); for (auto& x : v) x = (char)rd(); return v; };
  auto dbls = [&](size_t n) {   // bit patterns, so that NaN and -0.0 survive
    std::vector<double> v(n);
    for (auto& x : v) { unsigned long long b = 0; if (fscanf(f, "%llx", &b) != 1) { fprintf(stderr, "short model file\n"); exit(2); } memcpy(&x, &b, 8); }
    return v;
  };
  const int N = (int)rd(), L = (int)rd(), S = (int)rd(), NT = (int)rd(), ND = (int)rd(), lp = (int)rd(), pr = (int)rd();
  const auto slot_ptr = ints(N + 1), turn_ptr = ints(N + 1), kind = ints(N), drow = ints(N), sin = ints(S), sout = ints(S), rev = ints(L), sdyn = ints(S);
  const auto dnz = flags(ND > 0 ? ND : 0);
  const auto tfu = dbls(NT);
  const auto tab = flags(NT);
  const auto sep = ints(L), tsw = ints(L);
  const auto front = dbls(L), back = dbls(L);
  const auto rl = flags(L), seen = flags(L);
  fclose(f);
  Model m;
  m.n_nodes = N; m.n_links = L;
  m.node_slot_ptr = slot_ptr.data(); m.node_turn_ptr = turn_ptr.data(); m.node_kind = kind.data(); m.node_demand_row = drow.data();
  m.slot_in = sin.data(); m.slot_out = sout.data(); m.link_rev = rev.data(); m.slot_dyn = sdyn.data(); m.node_lp = lp != 0;
  m.demand_nz = dnz.data(); m.tf_u = tfu.data(); m.tab_nz = tab.data();
  m.link_sep = sep.data(); m.link_tau_sw = tsw.data(); m.front_u = front.data(); m.back_u = back.data(); m.link_rl = rl.data();
  m.per_replica_params = pr != 0;
  m.seed_links = seen.data();
  const Result r = pedn_part::partition(m);
  printf("reach: %s\nlive: %s\ndead_raw: %s\nnode_dead: %s\ndead: %s\n", ones(r.reach).c_str(), ones(r.live).c_str(), ones(r.dead_raw).c_str(),
         ones(r.node_dead).c_str(), ones(r.dead).c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "selftest") return selftest();
  if (argc == 3 && std::string(argv[1]) == "model") return from_file(argv[2]);
  fprintf(stderr, "usage: %s selftest | model <file>\n", argv[0]);
  return 2;
}
