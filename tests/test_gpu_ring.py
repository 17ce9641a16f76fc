"""Ring attention on the GPU: the ranks share cuda:0 (one-GPU box) under gloo with host-staged point-to-point transfers (a shim that lives in
tests/_dist_gpu_worker_ring.py only), and one world-1 leg over real RCCL."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def launch(world, worker, port):
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", worker)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


@pytest.mark.parametrize("world", [2, 4])
def test_ring_wan_forward_on_one_gpu(world):
    """wan-tiny with 4 heads at world 2 (45 rows per rank) and 4 (36 rows per rank), and with 3 heads at world 2 — a head count Ulysses refuses: the ring
    forward against the CPU oracle and the single-GPU HIP forward, N carry launches per attention, the last one writing bf16, no host synchronisation in
    the driver's loop."""
    out = launch(world, "_dist_gpu_worker_ring.py", 29571 + 10 * (world > 2))
    assert "DIST_GPU_RING_OK" in out
    print("\n".join(ln for ln in out.splitlines() if ln.startswith("RING_GPU")))
    assert sum(ln.startswith("RING_GPU H=") for ln in out.splitlines()) == (2 if world == 2 else 1)


def test_ring_over_rccl_world1():
    assert "DIST_GPU_RING_RCCL1_OK" in launch(1, "_dist_gpu_worker_ring_rccl1.py", 29573)
