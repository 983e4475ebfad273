"""Plumbing of tests/test_step_plan_host.py, tests/test_gpu_step_plan.py and tests/test_gpu_engine_plan.py: the stand-alone driver of the step
planner and the plan chooser (tests/plan_prog.cpp over pednstream_amd/csrc/pedn_plan.hpp), the grids the chooser is run over, the event scripts
the planner reads -- the library's entry points restated as the events they make of a call --
and Shadow, a restatement of what the KERNELS need of a sequence of launches: a shadow of device memory per half of the replicas, written
from the kernels' reads and writes, not from the planner's text."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_ROWS = 0x7FFFFFFF
CAPS = ("node_lp", "inline_tf", "inline_help", "quiet", "quiet_lean", "fuse_tp", "fuse_obs", "rl_ready", "zero_elide", "hist", "pr", "trow", "links",
        "live", "T1")


def build_prog(out_dir):
    """tests/plan_prog.cpp with the host compiler and ASan + UBSan, no HIP library; the executable's path."""
    exe = os.path.join(str(out_dir), "plan_prog")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "plan_prog.cpp")], check=True)
    return exe


def _kv(tokens):
    return {k: int(v) for k, v in (tok.split("=") for tok in tokens)}


def run_prog(exe, scripts, path):
    """scripts: [(caps, [event lines])].  Per script a list with one entry per event: (launch lines as (kind, {key: int}), state dict)."""
    with open(path, "w") as f:
        for caps, events in scripts:
            f.write("caps " + " ".join(f"{k}={int(caps[k])}" for k in CAPS) + "\n" + "\n".join(events) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]          # the sanitizers stayed silent
    out, launches = [], []
    for line in r.stdout.splitlines():
        tok = line.split()
        if tok[0] == "script":
            out.append([])
        elif tok[0] == "state":
            out[-1].append((launches, _kv(tok[1:])))
            launches = []
        else:
            launches.append((tok[0], _kv(tok[1:])))
    assert len(out) == len(scripts) and all(len(o) == len(s[1]) for o, s in zip(out, scripts))
    return out


# ---------------------------------------------------------------------------------------------------------------- the plan chooser
TF_WAVE_LDS = (8 + 8 - 1) * 64          # PEDN_TF_INL_LDS (pedn_kernels.hpp): (PEDN_TF_INL_ROWS + PEDN_MAX_DEGREE - 1) rows of 64 doubles
KNOBS = dict(fuse_tp=(-1, 0, 1), fuse_obs=(-1, 0, 1), streams=(-1, 1, 2), link_owner=(-1, 0, 1), inline_tf=(-1, 0, 1, 2), quiet=(-1, 0, 1),
             quiet_lean=(-1, 0, 1), zero_elide=(-1, 0, 1), rl_chains=(-1, 1, 2), dead_links=(-1, 0, 1), dead_waves=(-1, 3, 5, 8), dead_streams=(-1, 1, 2),
             stream_probe=(-1, 0, 1))          # every knob unset (-1) and at each value knobs_from_env can give it (dead_waves: the ends and the default)
# The knobs that another decision reads (link_owner: the default of quiet, dead_capable; inline_tf: link_owner; quiet and dead_links:
# dead_capable) are crossed with each other and with every input; each of the others only sets its own field of the plan, so a point
# draws their values from a hash of its index (all 13 crossed with the inputs would be 10^10 points).
CROSSED_KNOBS = ("link_owner", "inline_tf", "quiet", "dead_links")
# The inputs at their edges.  grid: n_blocks such that (RS / 64) * n_blocks is 352, and the smallest product above it that RS allows (353
# itself only for RS / 64 = 1); lds_tf_min: tiles such that node_lds_tf is exactly 64 KB / 160 KB, and one tile (512 B, the formula's
# step) above.  inline_tf_ok comes with n_trow > 0 only (pedn_compile.hpp: no row, nothing to inline), so that half is left out below.
GRID_INPUTS = dict(RS=(128, 576, 640, 704), grid=(352, 353), lds_tf_min=(64 << 10, (64 << 10) + 8, 160 << 10, (160 << 10) + 8), lds_tf=(0, 1), lds_h=(0, 1),
                   inline_tf_ok=(0, 1), node_lp=(0, 1), hist=(0, 1), n_trow=(0, 4), L=(0, 5))
GRID_FIXED = dict(N=10, n_rec=24, tf_wave_lds=TF_WAVE_LDS)


def run_choose(exe, spec, path):
    """spec: [(key, values)] in the driver's order (a key that starts with ~ is drawn, not crossed); {column: int64 array over the points}"""
    with open(path, "w") as f:
        f.write("".join(f"{k}={','.join(str(int(v)) for v in (vals if isinstance(vals, (tuple, list)) else (vals,)))}\n" for k, vals in spec))
    r = subprocess.run([exe, "--choose", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]          # the sanitizers stayed silent
    header, _, body = r.stdout.partition("\n")
    cols = header.split()
    table = np.fromstring(body, dtype=np.int64, sep=" ").reshape(-1, len(cols))
    return {c: table[:, i] for i, c in enumerate(cols)}


def grid_spec():
    return (list(GRID_FIXED.items()) + list(GRID_INPUTS.items()) + [("k_" + k, KNOBS[k]) for k in CROSSED_KNOBS]
            + [("~k_" + k, v) for k, v in KNOBS.items() if k not in CROSSED_KNOBS] + [("~links", (0, 1))])          # (links: only the report reads it)


def choose_one(exe, inputs, knobs, path):
    """the plan, static caps (c_*) and report (r_*) of one engine: {column: int}"""
    out = run_choose(exe, list(inputs.items()) + [("k_" + k, v) for k, v in knobs.items()], path)
    assert len(out["RS"]) == 1
    return {k: int(v[0]) for k, v in out.items()}


def compiled_inputs(compiled, model, n_replicas):
    """PlanInputs from what tests/compile_prog.cpp printed for the model (compile_model.run_prog) -- and, beside them, `links` and `packed_by`"""
    info, full = compiled["info"][0], compiled["full_info"][0]
    inputs = dict(RS=(n_replicas + 127) // 128 * 128, N=int(model["n_nodes"]), L=int(model["n_links"]), n_trow=int(info[1]),
                  node_lp=int(model.get("node_model", 0)), hist=int(model.get("history_mode", 0)), inline_tf_ok=int(info[4]), n_blocks=int(full[0]),
                  tiles=int(full[1]), n_rec=int(full[4]), tf_wave_lds=TF_WAVE_LDS, links=int(len(compiled["corr"][0]) > 0))
    return inputs, int(info[5])


def knobs_of(environ):
    """knobs_from_env restated for the values the tests set: 0 / 1 / 2 as text, unset"""
    return {k: int(environ["PEDN_" + k.upper()]) for k in KNOBS if "PEDN_" + k.upper() in environ}


def caps_of(plan, **runtime):
    """the StepCaps of an engine under `plan` (a row of run_choose): static_caps + the run-time entries"""
    return dict({k: plan["c_" + k] for k in ("node_lp", "inline_tf", "inline_help", "quiet", "quiet_lean", "fuse_tp", "fuse_obs", "zero_elide", "hist")}, **runtime)


# ---------------------------------------------------------------------------------------------------------------- the library's calls as events
def ev_step(t, lazy, chain=-1, n=1, observe=-1, fold=0, ctrl=0):
    return f"step t={t} lazy={int(lazy)} observe={observe} fold={int(fold)} ctrl={int(ctrl)} chain={chain} n={n}"


def ev_fork(t):
    """in front of a fork: a stale pending update on the whole batch, the rows a lazy reset left out below t"""
    return [f"stale t={t}", f"catchup t={t - 1}"]


def ev_run(t0, t1, lazy, chains=1, split=False, lean=1):
    """pedn_run(t0, t1) as the plan it was given"""
    if chains == 1:
        return [ev_step(t, lazy) for t in range(t0, t1)]
    out = ev_fork(t0)
    if split:
        return out + [ev_step(t0, lazy)] + [f"split t={t} n={lean}" for t in range(t0 + 1, t1)]
    return out + [ev_step(t, lazy, c, chains) for t in range(t0, t1) for c in range(chains)]


def ev_single(t, lazy, forked=None):
    """pedn_step(t); forked: None one stream, False the call that forks the two chains, True a later one"""
    if forked is None:
        return [ev_step(t, lazy)]
    return ([] if forked else ev_fork(t)) + [ev_step(t, lazy, c, 2) for c in range(2)]


def ev_rl(caps, t, gap, fold, ctrl, two):
    """pedn_rl_step(t, gap): actions applied by their own launch (behind a pending update) or folded into the first node launch"""
    out = [f"catchup t={t - 1}"] + ([] if fold else ["flush"])
    for k in range(gap):
        last = k == gap - 1
        kw = dict(observe=int(k > 0), fold=fold and k == 0, ctrl=ctrl and last)
        out += [ev_step(t + k, False, c, 2, **kw) for c in range(2)] if two else [ev_step(t + k, False, **kw)]
        if not (caps["rl_ready"] and caps["fuse_obs"]):          # rl_observe: a launch of its own
            out += ["flush", f"catchup t={t + k}"]
    return out


def split_possible(caps):
    return bool(caps["quiet"] and caps["links"] and not (caps["inline_tf"] or caps["hist"] or caps["node_lp"] or caps["trow"] or caps["pr"] or caps["rl_ready"]))


def fits(out, max_events):
    return len(out) <= max_events - 1


def random_script(caps, owner, seed, max_events=40):
    """at most max_events events over the horizon caps['T1'] - 1: single steps in sequence, repeated and jumping, ranges as 1 and 2 chains
    and split, RL steps, reads, setters, both resets, a foreign write, a clocked section, a change of the dead set"""
    rng = np.random.default_rng([seed, 0x504C414E])
    T = caps["T1"] - 1
    out, cur, foreign, forked, mark = ["reset"], 0, False, False, 1
    kinds = ["step", "step", "step", "run", "run", "read", "setter", "reset", "reset_lazy", "foreign", "deadset", "chains"]
    if caps["rl_ready"]:
        kinds += ["rl", "rl", "clock"]
    while True:
        if not fits(out, max_events):
            return out[:mark] + ["flush"]          # a reset-free end: whatever reads the result
        mark = len(out)
        kind = kinds[int(rng.integers(len(kinds)))]
        lazy = bool(owner) and rng.random() < 0.9          # (pedn_step steps a caller that looks after every step under the plain plan)
        if kind not in ("step", "chains"):
            forked = False
        if kind == "step" or kind == "chains":
            t = min(cur + 1, T) if rng.random() < 0.6 else max(cur, 1) if rng.random() < 0.5 else int(rng.integers(1, T + 1))
            if kind == "chains" and t == cur + 1:
                out += ev_single(t, lazy, forked)
                forked = True
            else:
                out += ev_single(t, lazy)
                forked = False
            cur = t
        elif kind == "run":
            t0 = min(cur + 1, T) if rng.random() < 0.7 else int(rng.integers(1, T + 1))
            t1 = min(T + 1, t0 + int(rng.integers(1, 7)))
            plan = int(rng.integers(3))
            split = plan >= 1 and owner and split_possible(caps) and not foreign and rng.random() < 0.8
            out += ev_run(t0, t1, bool(owner), 1 if plan == 0 else 2, split, int(rng.integers(1, 3)))
            cur = t1 - 1
        elif kind == "rl":
            gap = int(rng.integers(1, 4))
            t = min(cur + 1, T)
            gap = min(gap, T - t + 1)
            fold = bool(rng.integers(2))
            two = fold and caps["fuse_obs"] and rng.random() < 0.3
            out += (["flush"] if two else []) + ev_rl(caps, t, gap, fold, bool(rng.integers(2)), two)
            cur = t + gap - 1
        elif kind == "clock":
            if caps["fuse_obs"] and caps["fuse_tp"] and caps["links"] and not caps["node_lp"] and cur + 1 <= T:
                k = min(int(rng.integers(1, 4)), T - cur)
                out.append(f"clock t={cur + 1} k={k}")          # (refused where the fractions are not prepared: nothing runs)
                foreign = True
        elif kind == "read":
            out.append("flush")
        elif kind == "setter":
            out += ["flush", "invalidate"]
        elif kind == "deadset":
            out.append("deadset")
        elif kind == "foreign":
            out += ["flush_all", f"foreign f64={int(rng.integers(2))} f32={int(rng.integers(2))}"]
            foreign = True
        else:
            out.append(kind)
            cur, foreign = 0, foreign and kind == "reset_lazy" and not caps["hist"]


def all_caps():
    """owner-wave on / off, device rows yes / no, inline on / off, recent history, node LP, agent set, quiet and zero elision on / off"""
    out = []
    for bits in range(1 << 8):
        owner, trow, inline, hist, node_lp, rl, quiet, ze = ((bits >> i) & 1 for i in range(8))
        if inline and (not trow or node_lp or not owner):          # the single-launch plan is chosen for device rows, the classic node model
            continue
        out.append((dict(node_lp=node_lp, inline_tf=inline, inline_help=inline and bits % 3 == 0, quiet=quiet, quiet_lean=bits % 5 != 0, fuse_tp=bits % 7 != 0,
                         fuse_obs=bits % 11 != 0, rl_ready=rl, zero_elide=ze, hist=hist, pr=bits % 13 == 0, trow=trow, links=bits % 17 != 0, live=bits % 4 != 3,
                         T1=25 - bits % 3), owner))
    return out


# ---------------------------------------------------------------------------------------------------------------- the shadow of device memory
class Shadow:
    """What the launches of one script leave in device memory, per half of the replicas, and what each launch needs to find there.
      node      last node-launched step and how often its link update has run since (rule A)
      tfd       per buffer (step & 1): the step whose fractions it holds; emptied by an invalidation (rule B)
      words     (step, packing) of the quiet words stored by the last node launch covering the half, None once something may have changed a
                history row since or that launch stored none (rule C)
      dirty64 / dirty32  rows of the zero-elided fields that may hold something other than +0.0 since the last full reset; ANY: every row
                may, after a write that the host does not follow (rule D)"""
    ANY = "any row"

    def __init__(self, caps):
        self.caps = caps
        self.node = [None, None]
        self.tfd = [dict(), dict()]
        self.words = [None, None]
        self.dirty64, self.dirty32 = [set(), set()], [set(), set()]

    @staticmethod
    def cover(chain):
        return (0, 1) if chain < 0 else (chain,)

    def no_words(self, halves=(0, 1)):
        for h in halves:
            self.words[h] = None

    def pending(self):
        return [h for h in (0, 1) if self.node[h] is not None and self.node[h][1] != 1]

    def link_update(self, t, h, why):
        assert self.node[h] is not None and self.node[h][0] == t, f"A: {why}: link update of {t}, but the last node launch of half {h} was {self.node[h]}"
        self.node[h] = (t, self.node[h][1] + 1)
        assert self.node[h][1] == 1, f"A: {why}: link update of {t} performed twice on half {h}"
        self.dirty32[h].add(t)

    def gates(self, a, h):
        """(the launches of one step on different streams are not ordered: each sees the rows as they were before the step)"""
        for gate, dirty, row in ((a["zg64"], self.before64[h], a["t"]), (a["zg32"], self.before32[h], a["t"] - 1)):
            assert not gate or not (self.caps["hist"] or self.ANY in dirty or row in dirty), f"D: gate open on row {row}, half {h}"

    def node_launch(self, a, lu, inl):
        """node_kernel(t) or dead_link_kernel(t) on the halves of a['chain']: everything but the quiet words"""
        t = a["t"]
        for h in self.cover(a["chain"]):
            if lu:
                self.link_update(t - 1, h, "an LU launch")
            assert self.node[h] is None or self.node[h][1] == 1, f"A: node launch of {t} on half {h}, link update of {self.node[h][0]} not performed"
            self.node[h] = (t, 0 if self.caps["links"] else 1)          # (a model without physical links has no link update to perform)
            if self.caps["trow"] and inl:
                self.tfd[h][t & 1] = t
            elif self.caps["trow"]:
                assert self.tfd[h].get(t & 1) == t, f"B: node launch of {t} on half {h} finds the fractions of {self.tfd[h].get(t & 1)}"
            assert lu or not a["zg32"], "D: a 32-bit gate on a launch that writes no such row"
            self.gates(a, h)
            self.dirty64[h].add(t)
            assert a["vhi"] >= t - 1, f"F: node launch of {t} with valid_hi {a['vhi']}"

    def launch(self, kind, a):
        if kind == "flush":
            for h in self.cover(a["chain"]):
                self.link_update(a["t"], h, "flush")
            self.no_words(self.cover(a["chain"]))
        elif kind == "tf":
            for h in self.cover(a["chain"]):
                assert h not in self.pending(), f"A: stand-alone fractions of {a['t']} with a link update pending on half {h}"
                self.tfd[h][a["t"] & 1] = a["t"]
        elif kind == "node":
            self.node_launch(a, a["lu"], a["inl"])
            for h in self.cover(a["chain"]):
                if a["use"]:
                    assert a["lu"] and not a["inl"] and self.words[h] == (a["t"] - 1, 0), f"C: words {self.words[h]} used by step {a['t']}, half {h}"
                self.words[h] = (a["t"], 0) if a["quiet"] and a["lu"] and not a["inl"] else None
        elif kind == "lean":          # writes +0.0 only into its links, reads no words; the full packing's words are not stored
            self.node_launch(a, 1, 0)
            self.no_words(self.cover(a["chain"]))
        elif kind == "live":          # the live bins' share of the step that the lean launches have entered, on the whole batch
            for h in (0, 1):
                assert self.node[h] == (a["t"], 0)
                assert not a["use"] or self.before_words[h] == (a["t"] - 1, 1), f"C: live words {self.before_words[h]} used by step {a['t']}, half {h}"
                self.gates(a, h)
                self.words[h] = (a["t"], 1)
        elif kind == "second":
            assert not a["fused"] or a["t"] + 1 <= self.caps["T1"] - 1, f"B: fractions of row {a['t'] + 1} planned, the tables end at row {self.caps['T1'] - 1}"
            for h in self.cover(a["chain"]):
                if a["link"]:
                    self.link_update(a["t"], h, "second launch")
                if a["fused"]:
                    self.tfd[h][(a["t"] + 1) & 1] = a["t"] + 1
        elif kind == "clear":          # rows that a lazy reset left out are zeroed: a history row changes
            self.no_words()

    def event(self, name, args, launches):
        """the launches of one event, then what the event itself does to the memory"""
        self.before_words, self.before64, self.before32 = list(self.words), [set(x) for x in self.dirty64], [set(x) for x in self.dirty32]
        refused = any(kind == "refused" for kind, _ in launches)
        for kind, a in launches:
            if kind not in ("commits", "refused"):
                self.launch(kind, a)
        if name in ("flush", "flush_all", "invalidate", "deadset", "clock", "foreign") or (name == "stale" and launches):
            self.no_words()
        if name in ("flush", "flush_all", "clock"):
            assert not self.pending(), f"A: a touch leaves the link update of half {self.pending()} unperformed"
        if name == "invalidate":
            self.tfd = [dict(), dict()]
        if name in ("reset", "reset_lazy"):
            self.node, self.tfd = [None, None], [dict(), dict()]          # (a pending update is discarded with the state it would complete)
            self.no_words()
            if name == "reset" or self.caps["hist"]:
                self.dirty64, self.dirty32 = [set(), set()], [set(), set()]
        for h in (0, 1):
            if (name == "foreign" and args["f64"]) or (name == "clock" and not refused):
                self.dirty64[h].add(self.ANY)
            if (name == "foreign" and args["f32"]) or (name == "clock" and not refused):
                self.dirty32[h].add(self.ANY)


def check_script(caps, events, result):
    """rules A-F over one script's launches and states; returns the number of node launches checked"""
    sh, n, i = Shadow(caps), 0, 0
    prev = dict(step_epoch=1)
    while i < len(events):
        name, args = events[i].split()[0], _kv(events[i].split()[1:])
        launches, state = result[i]
        sh.event(name, args, launches)
        if name == "step":
            group = [i]
            while args["n"] > 1 and len(group) < args["n"]:          # E: the chains of one step
                group.append(group[-1] + 1)
                assert events[group[-1]].split()[0] == "step"
                sh.event("step", args, result[group[-1]][0])
            plans = [[(k, {x: v for x, v in a.items() if x != "chain"}) for k, a in result[g][0] if k != "commits"] for g in group]
            assert all(p == plans[0] for p in plans), f"E: the chains of step {args['t']} differ: {plans}"
            commits = [a["last"] for g in group for k, a in result[g][0] if k == "commits"]
            assert commits == [0] * (len(group) - 1) + [1], f"E: {commits}"
            state = result[group[-1]][1]
            assert state["step_epoch"] == prev["step_epoch"] + 1, "E: the step committed other than once"
            i = group[-1]
        if name in ("step", "split"):
            n += 1
            assert state["valid_hi"] >= args["t"], f"F: valid_hi {state['valid_hi']} behind step {args['t']}"
        prev = state
        i += 1
    assert not sh.pending(), "A: the script ends with a link update unperformed"
    return n


# ---------------------------------------------------------------------------------------------------------------- a library session
def session_events(chains, owner, dead_links, calls, lean=1, rs=256):
    """The events of a sequence of library calls on a model without device-computed rows: ("reset",), ("run", t0, t1), ("read",),
    ("step", t) -- pedn_run's chains_for and split decision and pedn_step's streaks restated from the plan the library reports."""
    out, touched, streak, last_t, forked = [], 0, 0, -1, False
    for call in calls:
        if call[0] == "reset":
            out.append("reset")
            touched, last_t, forked = touched, -1, False
        elif call[0] == "read":
            out.append("flush")
            touched, forked = 1, False
        elif call[0] == "run":
            t0, t1 = call[1:]
            nch = 2 if chains >= 2 and t1 - t0 >= 8 and rs >= 256 else 1
            out += ev_run(t0, t1, owner, nch, nch == 2 and owner and dead_links > 0, lean)
            last_t, forked = t1 - 1, False
        elif call[0] == "step":
            t = call[1]
            in_sequence = not touched and t == last_t + 1 and chains > 1 and rs >= 256
            streak = min(streak + 1, 2) if in_sequence else 0
            touched = 0
            out += ev_single(t, owner, (forked if streak >= 2 else None))
            forked, last_t = streak >= 2, t
    return out
