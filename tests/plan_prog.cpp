// plan_prog.cpp -- stand-alone driver of the step planner (pednstream_amd/csrc/pedn_plan.hpp) for tests/test_step_plan_host.py: built with the
// host compiler and the host sanitizers, no HIP library, never loaded into Python.
//
//   plan_prog SCRIPT      first line `caps k=v ...`, then one event per line; prints one line per planned launch and, behind every event,
//                         `state k=v ...`
//
// Events (what the library does around the planner at that point is restated here in the library's order):
//   step t=.. lazy=.. observe=.. fold=.. ctrl=.. chain=.. n=..   launch_step of one chain
//   split t=.. n=..       launch_split_step with n lean launches
//   stale t=..            a pending link update that is not the one of t - 1 is performed first (in front of a fork)
//   catchup t=..          catch_up(t) where t is above valid_hi
//   flush                 pending_links_first: whatever reads or changes the state (touch, then the pending link update)
//   flush_all             pedn_flush: ... and every row a lazy reset left out
//   invalidate | deadset | reset | reset_lazy | profile_begin
//   foreign f64=.. f32=.. a zero-copy pointer was handed out (pedn_device_ptr: behind flush_all)
//   clock t=.. k=..       pedn_rl_clock_begin(t), k clocked steps, clock_end -- `refused` where the fractions of t are not prepared
//   set k=v ...           marks set directly
//
//   plan_prog --choose SPEC   the plan chooser (choose / static_caps / report) over a grid.  SPEC has one `key=v1,v2,...` per line: the
//                         cross product of all lines is enumerated, the first line slowest; a line `~key=v1,v2,...` is not crossed -- each
//                         point draws its value from a hash of the point's index.  Keys: the fields of PlanInputs, `links`, the fields of
//                         Knobs as k_<name> (-1: unset), and two that stand for an input they set from the others:
//                           grid=G           n_blocks = the fewest blocks whose (RS / 64) * n_blocks is at least G
//                           lds_tf_min=B     tiles = the fewest tiles whose node_lds_tf is at least B bytes
//                         Prints a header line of column names, then one line of integers per point: the inputs, the knobs, the plan,
//                         static_caps as c_<name>, report as r_<name>.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../pednstream_amd/csrc/pedn_plan.hpp"

using namespace pedn_plan;
typedef std::map<std::string, long> Args;

static Args parse(std::istringstream& in) {
  Args a;
  std::string tok;
  while (in >> tok) {
    const size_t eq = tok.find('=');
    if (eq == std::string::npos) { fprintf(stderr, "bad token %s\n", tok.c_str()); exit(2); }
    a[tok.substr(0, eq)] = atol(tok.c_str() + eq + 1);
  }
  return a;
}
static long get(const Args& a, const char* k, long dflt) { auto it = a.find(k); return it == a.end() ? dflt : it->second; }

static StepCaps g_caps;
static StepState g_st;

static void print_state() {
  const StepState& s = g_st;
  printf("state valid_hi=%d link_pending=%d quiet_valid=%d quiet_pack=%d zhw64=%d zhw32=%d zgated=%d dl_grow=%d dl_off=%d split_steps=%d tp_ready=%d "
         "last_t=%d step_epoch=%ld second_launch=%d tp_ran=%d\n", s.valid_hi, s.link_pending, s.quiet_valid, s.quiet_pack, s.zhw64, s.zhw32, s.zgated,
         (int)s.dl_grow, (int)s.dl_off, s.split_steps, s.tp_ready, s.last_t, s.step_epoch, s.second_launch, s.tp_ran);
}

// catch_up of pedn_hip.hip
static void catch_up(int upto) {
  if (g_st.valid_hi >= upto) return;
  upto = std::min(upto, g_caps.T1 - 1);
  if (upto > g_st.valid_hi) printf("clear from=%d upto=%d\n", g_st.valid_hi + 1, upto);
  caught_up(g_st, upto);
}
// flush_links
static void flush_links(int chain, bool last) {
  if (g_st.link_pending < 0) return;
  printf("flush t=%d chain=%d\n", g_st.link_pending, chain);
  if (last) flushed(g_st);
  else touch(g_st);
}
static void pending_links_first() {
  touch(g_st);
  flush_links(-1, true);
}

static void step(const Args& a) {
  static const double some_actions[1] = {0.0};
  StepRequest rq;
  rq.t = (int)get(a, "t", 1); rq.lazy = get(a, "lazy", 0) != 0; rq.observe = (int)get(a, "observe", -1);
  rq.fold = get(a, "fold", 0) ? some_actions : nullptr;
  rq.ctrl = get(a, "ctrl", 0) ? reinterpret_cast<const CtrlView*>(some_actions) : nullptr;   // (never dereferenced: the planner tests it for null)
  rq.chain = (int)get(a, "chain", -1); rq.n_chains = (int)get(a, "n", 1); rq.profiled = get(a, "profiled", 0) != 0;
  if (rq.chain < 0 && rq.t - 1 > g_st.valid_hi) catch_up(rq.t - 1);
  const StepPlan p = plan_step(g_caps, g_st, rq);
  if (p.flush) flush_links(rq.chain, p.commits);
  if (p.tf_alone) printf("tf t=%d chain=%d\n", p.t, rq.chain);
  printf("node t=%d chain=%d lu=%d inl=%d helpers=%d quiet=%d use=%d lean=%d zg64=%d zg32=%d fold=%d vhi=%d\n", p.t, rq.chain, (int)p.lu, (int)p.inl,
         (int)p.helpers, (int)p.quiet, (int)p.quiet_use, (int)p.quiet_lean, p.zg64, p.zg32, rq.fold != nullptr, g_st.valid_hi);
  if (p.second != SECOND_NONE)
    printf("second t=%d chain=%d kind=%d link=%d fused=%d obs=%d ctrl=%d one_r=%d\n", p.t, rq.chain, (int)p.second, (int)p.link,
           (int)(p.second == SECOND_LINK_TURN && p.fused), (int)(p.second == SECOND_LINK_TURN && p.obs), (int)p.ctrl, (int)p.one_r);
  printf("commits last=%d\n", (int)p.commits);
  commit_step(g_st, p);
}

static void split(const Args& a) {
  StepRequest rq;
  rq.t = (int)get(a, "t", 2); rq.lazy = true; rq.n_chains = (int)get(a, "n", 1);
  const SplitPlan p = plan_split_step(g_caps, g_st, rq);
  for (int c = 0; c < p.lean_launches; ++c) printf("lean t=%d chain=%d zg64=%d zg32=%d vhi=%d\n", p.t, p.lean_launches == 1 ? -1 : c, p.zg64, p.zg32, g_st.valid_hi);
  if (p.live) printf("live t=%d use=%d lean=%d zg64=%d zg32=%d vhi=%d\n", p.t, (int)p.quiet_use, (int)p.quiet_lean, p.zg64, p.zg32, g_st.valid_hi);
  commit_split_step(g_st, p);
}

// pedn_rl_clock_begin(t), k steps of pedn_rl_step_clocked (the step index and valid_hi live on the device: node_clock), clock_end
static void clocked(const Args& a) {
  const int t = (int)get(a, "t", 1), k = (int)get(a, "k", 1);
  pending_links_first();
  if (t - 1 > g_st.valid_hi) catch_up(t - 1);
  if (g_caps.trow && g_st.tp_ready != t) { printf("refused\n"); return; }
  foreign_write(g_st, true, true);
  int vhi = g_st.valid_hi;
  for (int i = 0; i < k; ++i) {
    printf("node t=%d chain=-1 lu=0 inl=0 helpers=0 quiet=0 use=0 lean=0 zg64=0 zg32=0 fold=0 vhi=%d\n", t + i, vhi);
    printf("second t=%d chain=-1 kind=2 link=1 fused=%d obs=1 ctrl=0 one_r=%d\n", t + i, (int)(g_caps.trow && t + i + 1 <= g_caps.T1 - 1), (int)g_caps.pr);
    if (vhi != ALL_ROWS && t + i > vhi) vhi = t + i;
  }
  clock_ended(g_st, g_caps, t, t + k, vhi);
}

// ---- the plan chooser over a grid
static const char* const CHOOSE_KEYS[] = {"RS", "N", "L", "n_trow", "node_lp", "hist", "inline_tf_ok", "n_blocks", "tiles", "n_rec", "tf_wave_lds", "lds_tf", "lds_h", "links",
                                          "k_fuse_tp", "k_fuse_obs", "k_streams", "k_link_owner", "k_inline_tf", "k_quiet", "k_quiet_lean", "k_zero_elide", "k_rl_chains",
                                          "k_dead_links", "k_dead_waves", "k_dead_streams", "k_stream_probe", "grid", "lds_tf_min"};
enum { K_RS, K_N, K_L, K_TROW, K_LP, K_HIST, K_OK, K_BLOCKS, K_TILES, K_REC, K_WAVE_LDS, K_LDS_TF, K_LDS_H, K_LINKS, K_KNOB0, K_GRID = K_KNOB0 + 13, K_LDS_MIN, K_COUNT };
struct Dim { int key; std::vector<long> values; bool crossed; };

static int choose_grid(const char* path) {
  std::ifstream f(path);
  if (!f) { fprintf(stderr, "cannot read %s\n", path); return 2; }
  std::vector<Dim> dims;
  std::string line;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] == '#') continue;
    Dim d;
    d.crossed = line[0] != '~';
    const size_t eq = line.find('='), k0 = d.crossed ? 0 : 1;
    if (eq == std::string::npos) { fprintf(stderr, "bad line %s\n", line.c_str()); return 2; }
    for (d.key = 0; d.key < K_COUNT && line.compare(k0, eq - k0, CHOOSE_KEYS[d.key]) != 0; ++d.key) {}
    if (d.key == K_COUNT) { fprintf(stderr, "unknown key in %s\n", line.c_str()); return 2; }
    std::istringstream vals(line.substr(eq + 1));
    std::string tok;
    while (std::getline(vals, tok, ',')) d.values.push_back(atol(tok.c_str()));
    if (d.values.empty()) { fprintf(stderr, "no value in %s\n", line.c_str()); return 2; }
    dims.push_back(d);
  }
  size_t n_points = 1;
  for (const Dim& d : dims) if (d.crossed) n_points *= d.values.size();
  for (int k = 0; k < K_GRID; ++k) printf("%s ", CHOOSE_KEYS[k]);
  printf("fuse_tp fuse_obs chains link_owner inline_tf inline_help quiet quiet_lean zero_elide rl_chains node_lds node_lds_tf tf_lds_off "
         "dead_links dead_waves dead_streams dead_capable quiet_words quiet_words_live stream_probe inline_candidate "
         "c_node_lp c_inline_tf c_inline_help c_quiet c_quiet_lean c_fuse_tp c_fuse_obs c_zero_elide c_hist "
         "r_owner_wave r_quiet r_zero_elide r_quiet_lean r_dead_links\n");
  std::string out;
  const auto put = [&out](long long x) { char b[24]; out.append(b, (size_t)snprintf(b, sizeof b, "%lld ", x)); };
  for (size_t i = 0; i < n_points; ++i) {
    long a[K_COUNT];
    const long dflt[K_COUNT] = {128, 0, 0, 0, 0, 0, 0, 0, 0, 8, 0, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    std::copy(dflt, dflt + K_COUNT, a);
    size_t rest = i;
    for (size_t j = dims.size(); j-- > 0;) {
      const Dim& d = dims[j];
      if (d.crossed) { a[d.key] = d.values[rest % d.values.size()]; rest /= d.values.size(); }
      else {   // (splitmix64 of the point and the line)
        uint64_t z = (uint64_t)i * 64 + j + 0x9e3779b97f4a7c15ull;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; z ^= z >> 31;
        a[d.key] = d.values[z % d.values.size()];
      }
    }
    PlanInputs in;
    in.RS = (int)a[K_RS]; in.N = (int)a[K_N]; in.L = (int)a[K_L]; in.n_trow = (int)a[K_TROW];
    in.node_lp = a[K_LP] != 0; in.hist = a[K_HIST] != 0; in.inline_tf_ok = a[K_OK] != 0;
    in.n_blocks = (int)a[K_BLOCKS]; in.tiles = (int)a[K_TILES]; in.n_rec = (int)a[K_REC];
    in.tf_wave_lds = (int)a[K_WAVE_LDS]; in.lds_tf = a[K_LDS_TF] != 0; in.lds_h = a[K_LDS_H] != 0;
    if (a[K_GRID] >= 0) in.n_blocks = (int)((a[K_GRID] + in.RS / 64 - 1) / (in.RS / 64));
    while ((long)node_lds_tf_bytes(in) < a[K_LDS_MIN]) ++in.tiles;
    a[K_BLOCKS] = in.n_blocks; a[K_TILES] = in.tiles;
    Knobs k;
    int* const knob[13] = {&k.fuse_tp, &k.fuse_obs, &k.streams, &k.link_owner, &k.inline_tf, &k.quiet, &k.quiet_lean, &k.zero_elide, &k.rl_chains, &k.dead_links,
                           &k.dead_waves, &k.dead_streams, &k.stream_probe};
    for (int j = 0; j < 13; ++j) *knob[j] = (int)a[K_KNOB0 + j];
    const EnginePlan p = choose(in, k);
    const StepCaps c = static_caps(p);
    const PlanReport r = report(p, a[K_LINKS] != 0);
    for (int j = 0; j < K_GRID; ++j) put(a[j]);
    const long long plan[] = {p.fuse_tp, p.fuse_obs, p.chains, p.link_owner, p.inline_tf, p.inline_help, p.quiet, p.quiet_lean, p.zero_elide, p.rl_chains, (long long)p.node_lds,
                              (long long)p.node_lds_tf, p.tf_lds_off, p.dead_links, p.dead_waves, p.dead_streams, p.dead_capable, (long long)p.quiet_words,
                              (long long)p.quiet_words_live, p.stream_probe, inline_candidate(in), c.node_lp, c.inline_tf, c.inline_help, c.quiet, c.quiet_lean, c.fuse_tp,
                              c.fuse_obs, c.zero_elide, c.hist, r.owner_wave, r.quiet, r.zero_elide, r.quiet_lean, r.dead_links};
    for (long long x : plan) put(x);
    out += '\n';
    if (out.size() > (1 << 20) || i + 1 == n_points) { fwrite(out.data(), 1, out.size(), stdout); out.clear(); }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 3 && strcmp(argv[1], "--choose") == 0) return choose_grid(argv[2]);
  if (argc < 2) { fprintf(stderr, "usage: plan_prog SCRIPT | plan_prog --choose SPEC\n"); return 2; }
  std::ifstream f(argv[1]);
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    std::string ev;
    if (!(in >> ev) || ev[0] == '#') continue;
    const Args a = parse(in);
    if (ev == "caps") {
      StepCaps& c = g_caps;
      c.node_lp = get(a, "node_lp", 0); c.inline_tf = get(a, "inline_tf", 0); c.inline_help = get(a, "inline_help", 0);
      c.quiet = get(a, "quiet", 0); c.quiet_lean = get(a, "quiet_lean", 0); c.fuse_tp = get(a, "fuse_tp", 1); c.fuse_obs = get(a, "fuse_obs", 1);
      c.rl_ready = get(a, "rl_ready", 0); c.zero_elide = get(a, "zero_elide", 0); c.hist = get(a, "hist", 0); c.pr = get(a, "pr", 0);
      c.trow = get(a, "trow", 0); c.links = get(a, "links", 1); c.live = get(a, "live", 0); c.T1 = (int)get(a, "T1", 25);
      g_st = StepState();
      printf("script\n");
      continue;
    }
    if (ev == "step") step(a);
    else if (ev == "split") split(a);
    else if (ev == "stale") { if (g_st.link_pending >= 0 && g_st.link_pending != get(a, "t", 1) - 1) pending_links_first(); }
    else if (ev == "catchup") { if (get(a, "t", 0) > g_st.valid_hi) catch_up((int)get(a, "t", 0)); }
    else if (ev == "flush") pending_links_first();
    else if (ev == "flush_all") {
      pending_links_first();
      if (g_st.valid_hi != ALL_ROWS) { catch_up(g_caps.T1 - 1); caught_up(g_st, ALL_ROWS); }
    }
    else if (ev == "invalidate") fractions_invalid(g_st);
    else if (ev == "deadset") dead_set_changed(g_st);
    else if (ev == "reset") reset_full(g_st);
    else if (ev == "reset_lazy") { if (g_caps.hist) reset_full(g_st); else reset_lazy(g_st); }
    else if (ev == "profile_begin") profile_begin(g_st);
    else if (ev == "foreign") foreign_write(g_st, get(a, "f64", 0) != 0, get(a, "f32", 0) != 0);
    else if (ev == "clock") clocked(a);
    else if (ev == "set") {
      StepState& s = g_st;
      s.valid_hi = (int)get(a, "valid_hi", s.valid_hi); s.link_pending = (int)get(a, "link_pending", s.link_pending);
      s.quiet_valid = (int)get(a, "quiet_valid", s.quiet_valid); s.quiet_pack = (int)get(a, "quiet_pack", s.quiet_pack);
      s.zhw64 = (int)get(a, "zhw64", s.zhw64); s.zhw32 = (int)get(a, "zhw32", s.zhw32); s.tp_ready = (int)get(a, "tp_ready", s.tp_ready);
      s.last_t = (int)get(a, "last_t", s.last_t); s.dl_grow = get(a, "dl_grow", s.dl_grow); s.dl_off = get(a, "dl_off", s.dl_off);
    }
    else { fprintf(stderr, "unknown event %s\n", ev.c_str()); return 2; }
    print_state();
  }
  return 0;
}
