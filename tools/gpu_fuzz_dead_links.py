"""The dead-link plan under random calls on many random networks: tests/test_gpu_dead_links_random.py's case for every seed of a range
that has a dead link and no row of fractions computed on the device -- PEDN_DEAD_LINKS=1 against PEDN_DEAD_LINKS=0 against the CPU
oracle by bits, and plan_info()'s dead-link count and lean-kernel steps against the test's own copy of the proof's inputs after every
call (tests/dead_link_cases.py).  A failed comparison is reported with its seed and the campaign goes on; any other error ends it.

    python tools/gpu_fuzz_dead_links.py 4000 5000
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import dead_link_cases as dl
import partition_model as pm

lo, hi = int(sys.argv[1]), int(sys.argv[2])
n = len(dl.KINDS)
ran = dropped = plain = calls_total = lean_steps = 0
failed, kinds = [], {}
t_start = time.time()
for seed in range(lo, hi):
    case = dl.mutated_case(seed)
    if case is None:
        dropped += 1
        continue
    case, m, rec = case
    inp = pm.proof_inputs(m)
    if (inp["slot_dyn"] == 1).any() or not pm.partition(inp)["dead"]:
        plain += 1
        continue
    R = 330 if seed % 4 == 0 else 320
    calls, expect = dl.call_sequence(m, R, seed, (dl.KINDS[seed % n], dl.KINDS[(seed + n // 2) % n]))
    p = dl.start(case, m, rec, R, seed, ("create", "setters")[seed % 2])
    try:
        dl.run_calls(p, calls, expect, f"seed {seed} x {R}")
        lean_steps += p.split_steps()
    except AssertionError as e:
        failed.append(seed)
        print(f"FAILED seed {seed}: {str(e)[:600]}", flush=True)
    p.close()
    ran += 1
    calls_total += sum(c[0] != "check" for c in calls)
    for c in calls:
        kinds[c[0]] = kinds.get(c[0], 0) + 1
    if ran % 25 == 0:
        print(f"#   ... seed {seed} of {lo}..{hi}: {ran} networks, {len(failed)} failed, {time.time() - t_start:.0f} s", flush=True)
print(f"dead-link plan on == off == oracle, dead-link count and lean-kernel steps as tracked: {ran} random networks of seeds {lo}..{hi} (320 or 330 replicas), "
      f"{calls_total} calls {dict(sorted(kinds.items()))}, {lean_steps} steps on the lean kernel at the end of the last episodes; {plain} seeds without a dead link or with "
      f"device-computed rows and {dropped} dropped seeds not run; FAILED: {failed or 'none'}")
sys.exit(1 if failed else 0)
