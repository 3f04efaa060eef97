"""Two ranks on the one-sided lane with a guarded fused AdamW update: rank 1's
batch is bad at steps 2 and 4, the exact round delivers the same non-finite
sum to both ranks, and both skip -- eager and as the whole step in one graph
replay.  Parameters, moments and shadow are bitwise the same on both ranks and
equal the unguarded run over the four clean batches."""
import os
import socket
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_both_ranks_skip_the_bad_rounds_eager_and_fully_graphed():
    n, steps = 2, 6
    with tempfile.TemporaryDirectory() as out:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
               "--master-addr", "127.0.0.1", "--master-port", str(_port()),
               os.path.join(ROOT, "tests", "skip_nonfinite_ranks.py"), "--out-dir", out, "--steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        rows = [torch.load(os.path.join(out, f"rank{i}.pt"), weights_only=True) for i in range(n)]
    for d in rows:
        assert d["replays"] == steps and d["error"] == 0
        assert d["after_capture_t"] == 0 and d["after_capture_record"] == [0, 0, 0, 0]
        assert d["clean_t"] == 4
        for run in ("eager", "graphed"):
            assert d[run + "_t"] == 4 and d[run + "_record"] == [1, 2, 0, 0], run
            for k in ("", "_m", "_v", "_shadow"):
                a, b = d[run + k], d["clean" + k]
                it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
                assert torch.equal(a.view(it), b.view(it)), (run, k)
        assert bool(torch.isfinite(d["eager"]).all()) and float(d["eager_m"].abs().max()) > 0
        assert torch.equal(d["eager_shadow"], d["eager"].to(torch.bfloat16))
    for k in ("eager", "eager_m", "eager_v", "eager_shadow", "graphed", "graphed_m", "graphed_v", "graphed_shadow"):
        assert torch.equal(rows[0][k], rows[1][k]), k  # every rank holds the same model
