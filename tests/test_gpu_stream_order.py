"""The stream order of the sequence-parallel drivers (ulysses.CommStreams: UlyssesAttention, UlyssesHunyuanAttention, ring.RingAttention) and of
wan.CfgBranchStreams, on one GPU, in a state where every wait decides a result: one side is slowed on purpose (device-side delays, collectives
replaced by stand-ins on the current stream), the result must stay bit-equal to the driver without streams, and with the waits of one role made
no-ops it must NOT (tests/_dist_gpu_worker_stream_order.py, tests/stream_order.py).  One short child process per case, one at a time."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# case -> (time limit of the child in seconds, negative controls it must report)
CASES = {
    "wan-blocked": (120, 2),
    "wan-cfg": (120, 4),
    "row-major": (90, 2),
    "hunyuan": (120, 2),
    "ring": (120, 6),
    "cfg-single": (90, 2),
}


def launch(case, port, limit):
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", X2V_STREAM_ORDER_CASE=case, GPU_MAX_HW_QUEUES="8")
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "_dist_gpu_worker_stream_order.py")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit + 30, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


@pytest.mark.parametrize("case", list(CASES))
def test_every_stream_wait_decides_a_result(case):
    """Positives bit-equal under slow communication and slow compute, no host synchronisation inside a driver call, and every negative control
    (one role of waits made a no-op under the regime aimed at it) differs from its positive; the worker asserts, this prints its figures."""
    limit, controls = CASES[case]
    out = launch(case, 29581 + list(CASES).index(case), limit)
    lines = [ln for ln in out.splitlines() if ln.startswith("STREAM_ORDER ")]
    print("\n".join(lines))
    assert f"STREAM_ORDER_OK {case}" in out
    assert sum(": control, " in ln for ln in lines) == controls
    assert sum(": positive, " in ln for ln in lines) >= (1 if case == "cfg-single" else 2)
