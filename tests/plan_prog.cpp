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
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <map>
#include <sstream>
#include <string>

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

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: plan_prog SCRIPT\n"); return 2; }
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
