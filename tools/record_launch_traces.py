#!/usr/bin/env python3
"""Record tests/golden/launch_traces.json: the [tag, cost] list of every case of
tests/launch_cases.py (one forward and one backward each, core.PROF on). Needs the GPU.

  python tools/record_launch_traces.py [--out PATH] [--hashes PATH]

--hashes also writes {case: {tensor name: sha256}} of every output and gradient, for a bitwise A/B of
two versions of the host layer (run it on each and compare the files). Record the traces from the
version whose behaviour is the reference; tests/test_gpu_launch_trace.py then holds later versions to it.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "aero-gnn_amd"), os.path.join(ROOT, "tests")]

import launch_cases  # noqa: E402


def _sha(t):
    import torch
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "launch_traces.json"))
    ap.add_argument("--hashes", default=None)
    args = ap.parse_args()
    traces, hashes = {}, {}
    for name, (_, _, env) in launch_cases.CASES.items():
        old = {k: os.environ.get(k) for k in env}
        try:
            trace, tensors = launch_cases.run_case(name, os.environ.__setitem__)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        traces[name] = trace
        hashes[name] = {k: _sha(t) for k, t in tensors.items()}
        print(f"{name}: {len(trace)} launches, {len(tensors)} tensors", flush=True)
    for path, obj in ((args.out, traces), (args.hashes, hashes)):
        if path:
            with open(path, "w") as f:
                json.dump(obj, f, indent=1, sort_keys=True)
                f.write("\n")


if __name__ == "__main__":
    main()
