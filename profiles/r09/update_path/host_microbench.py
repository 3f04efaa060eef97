"""Host cost of one update call, CPU only: microseconds per call of
``bucket.sgd_from`` and ``FusedAdamW.step_from`` with a stub allreduce (the
round is a constant, so what is timed is the update path's Python plus the
1,410-element torch operations behind it).  ``--root``: the tree to import.

    python profiles/r09/update_path/host_microbench.py --root <tree>
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))))
ap.add_argument("--calls", type=int, default=2000)
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))

import torch  # noqa: E402

from akka_allreduce_amd.data import AllReduceOutput, Geometry  # noqa: E402
from akka_allreduce_amd.models.mlp import MLP  # noqa: E402
from akka_allreduce_amd.parallel import FusedAdamW  # noqa: E402
from akka_allreduce_amd.parallel.dp import GradientBucket  # noqa: E402

torch.set_num_threads(1)
torch.manual_seed(0)
bucket = GradientBucket(list(MLP(24, 40, 10).parameters()), flatten_params=True)
assert bucket.numel == 1410
bucket.flat.normal_()
geo, counts = Geometry(bucket.numel, 1, bucket.numel), torch.ones((1, 1), dtype=torch.int32)


def stub(t, out=None):
    return AllReduceOutput(t, counts_per_chunk=counts, geometry=geo)


opt = FusedAdamW(bucket)
res = {"root": os.path.abspath(a.root)}
for name, call in (("sgd_from", lambda: bucket.sgd_from(stub, 1e-3)), ("adamw_step_from", lambda: opt.step_from(stub, 1e-3))):
    for _ in range(200):
        call()
    reps = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for _ in range(a.calls):
            call()
        reps.append((time.perf_counter() - t0) / a.calls * 1e6)
    res[name + "_us"] = {"median": round(statistics.median(reps), 2), "min": round(min(reps), 2),
                         "max": round(max(reps), 2)}
print(json.dumps(res))
