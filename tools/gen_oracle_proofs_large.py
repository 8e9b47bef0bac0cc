#!/usr/bin/env python3
"""Generates tests/golden/oracle_proofs_large.json: the ORACLE prover's proofs (oracle/plonk_prover.py) of the chain circuit at
group orders above 2^12, in the format of tests/golden/oracle_proofs.json (tools/gen_oracle_proofs.py), which this tool never
touches.  Both cases run on oracle.srs.Setup.from_tau(TEST_TAU, group_order): the committed .ptau stops at 2^11 powers.

A case already in the file is kept as it stands; --all proves everything again.  Minutes per case on one core: the recorded
"oracle_seconds" of each case say how many."""
import json
import os
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
from oracle.circuit import Program  # noqa: E402
from oracle.plonk_prover import Prover  # noqa: E402
from oracle.srs import TEST_TAU, Setup  # noqa: E402

ORDERS = (8192, 16384)


def chain_lines(n):
    return ["x0 public"] + ["x%d <== x%d * x%d" % (i + 1, i, i) for i in range(n - 1)]


def main():
    path = os.path.join(REPO, "tests", "golden", "oracle_proofs_large.json")
    out = {"source": "oracle/plonk_prover.py (CPU restatement, pinned by K6)", "cases": []}
    if os.path.exists(path) and "--all" not in sys.argv[1:]:
        with open(path) as f:
            out = json.load(f)
    have = {c["name"] for c in out["cases"]}
    for n in ORDERS:
        name, start = "chain_%d_x0_3" % n, {"x0": 3}
        if name in have:
            print(name, "kept", flush=True)
            continue
        setup = Setup.from_tau(TEST_TAU, n)
        prog = Program(chain_lines(n), n)
        wit = prog.fill_variable_assignments(start)
        t0 = time.time()
        prover = Prover(setup, prog)
        proof = prover.prove(dict(wit)).flatten()
        dt = time.time() - t0
        enc = {k: ([str(v[0]), str(v[1])] if isinstance(v, tuple) else str(v)) for k, v in proof.items()}
        out["cases"].append({"name": name, "group_order": n, "start": start, "proof": enc,
                             "challenges": {k: str(v) for k, v in prover.challenges.items()}, "oracle_seconds": round(dt, 1),
                             "srs_tau": str(TEST_TAU), "program": "chain"})
        print(name, "%.1fs" % dt, flush=True)
        with open(path, "w") as f:  # after every case: a later one takes minutes more
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
