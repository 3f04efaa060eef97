"""One bf16 rounding for every kernel that sums: a bf16 round on an exact ipc
lane (the compile-time-N vector body of csrc/kernels/ipc.hip) and one on the
one-sided lane (csrc/kernels/onesided.hip), 2 ranks on the box's one GPU, each
compared bit for bit with the standalone reduce kernels (csrc/kernels/reduce.hip:
vec, lds, scalar) over the same inputs.  A job's lanes are picked by tune() at
run time and a lane's bf16 sum is read by kernels of the other files
(count_mean<float, bf16> reads a one-sided round's sum), so all of them must
round alike: csrc/kernels/elem.h.  What this pins is the agreement between
the files; the rounding itself is checked against torch by the kernels' own
tests (test_kernels_gpu, test_ipc_gpu, test_onesided_gpu).

The inputs tile a table of rounding edges (exact ties both ways, overflow of
the fp32 sum, a finite sum that rounds to inf, subnormals, -0 + -0, inf - inf,
NaN) between randn at scales from 2^-120 to 2^120.  Two sizes: 8192 elements,
where every block passes the lanes' 16-B alignment test (reduce_span /
masked_sum: pointers, offsets and byte lengths all multiples of 16) and takes
the vector body; 8198 elements, blocks of 4099: rank 1's block starts 8198
bytes into the buffer and rank 0's ends in a part of odd length, so those take
the scalar body."""
import json
import os
import socket
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SIZES = (1 << 13, (1 << 13) + 6)
LANES = ("ipc_fused_lite", "onesided")


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def rounds():
    """One 2-rank job for the whole module: {(rank, size, lane): record}."""
    with tempfile.TemporaryDirectory() as out:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
               os.path.join(ROOT, "tests", "codec_ranks.py"), "--out-dir", out,
               "--sizes", ",".join(str(s) for s in SIZES), "--lanes", ",".join(LANES)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=180, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        recs = {}
        for rank in range(2):
            with open(os.path.join(out, f"rank{rank}.json")) as f:
                d = json.load(f)
            assert d["ipc_error"] == 0, d
            for rec in d["rounds"]:
                recs[(rank, rec["size"], rec["lane"])] = rec
    return recs


@pytest.mark.parametrize("lane", LANES)
@pytest.mark.parametrize("size", SIZES)
def test_lane_sum_has_the_standalone_kernels_bits(rounds, size, lane):
    for rank in range(2):
        rec = rounds[(rank, size, lane)]
        print(rank, rec)
        assert rec["state_lane"] == ("ipc" if lane.startswith("ipc") else lane), rec
        assert rec["counts_ok"], rec
        assert rec["nan"] > 0 and rec["inf"] > 0, rec  # the edges are in the output
        assert rec["equal"] == {"vec": True, "lds": True, "scalar": True}, rec
