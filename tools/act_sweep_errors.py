"""Measure, for every case of the acting sweep (tests/act_reference.py CASES) and for the two shifted cases of
tests/test_gpu_act.py, e_kernel = max|flock_sc_act - f64| and e_chain = max|f32 torch chain - f64|, and derive M: the
smallest power of two that is at least twice the largest e_kernel / e_chain. Needs the MI355X.

    python tools/act_sweep_errors.py [OUT.json]     (default: profiles/act_sweep/errors.json)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from act_reference import CASES, case_id, case_obs, case_seed, sc_act_path  # noqa: E402
import test_gpu_act as T  # noqa: E402


def main(out):
    dev = torch.device("cuda", 0)
    rec = {"sweep": [], "shifted": []}

    def one(key, name, L, obs, path):
        print("run", name, path, flush=True)
        act, _ = T._launch(L, obs)
        e_kernel, e_chain, _ = T._errors(L, obs, act)
        r = {"case": name, "path": list(path), "e_kernel": e_kernel, "e_chain": e_chain,
             "ratio": e_kernel / e_chain if e_chain > 0 else None}
        print(json.dumps(r), flush=True)
        rec[key].append(r)

    for c in CASES:
        A, R, n_in, fc1, fc2 = c
        L = T._learner(A, n_in, fc1, fc2, dev, fill=case_seed(c), fused=False)
        one("sweep", case_id(c), L, case_obs(R, A, n_in, case_seed(c)).to(dev), sc_act_path(n_in, fc1, fc2))
    for A, R, n_in, fc1, fc2 in ((4, 65, 4, 400, 300), (3, 65, 3, 40, 100)):
        L = T._learner(A, n_in, fc1, fc2, dev, fill=5, b1_shift=100.0)
        one("shifted", f"shift100_in{n_in}_{fc1}x{fc2}", L, case_obs(R, A, n_in, 5).to(dev),
            sc_act_path(n_in, fc1, fc2))
    worst = max(r["ratio"] for r in rec["sweep"] + rec["shifted"] if r["ratio"] is not None)
    m = 1
    while m < 2 * worst:
        m *= 2
    rec["worst_ratio"], rec["M"] = worst, m
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("worst ratio", worst, "M", m)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "act_sweep", "errors.json"))
