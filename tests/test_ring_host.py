"""Ring attention without a GPU: the carry formula in float64 (tests/attn_carry_ref.py: a chain over any chunking is dense attention), the argument
checks of x2v_attn_fwd_bf16_vt_carry, WanModel's `parallel_attn_type="ring"`, and gloo runs of ring.RingAttention at world 2 and 3 with the restated
carry step as its attention (tests/_dist_worker_ring.py)."""
import ctypes
import os
import subprocess
import sys
import types

import pytest
import torch

from tests import attn_carry_ref as C
from tests import attn_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("family,spike", [("R", "none"), ("R", "first"), ("R", "middle"), ("R", "last"), ("N", "none"), ("H", "none"), ("U", "none")])
def test_float64_chain_over_any_chunking_is_dense_attention(family, spike):
    """The formula itself: (A, L) after a chain equals float64 attention over the concatenated keys and its log-sum-exp to ~1e-12, whichever chunk
    dominates (spike first / middle / last; family H: one key decides a row and sits in any chunk) and for single-key chunks."""
    Sq, Sk, H = 37, 585, 2
    inp = A.Inputs(family, Sq, Sk, H, spike)
    s = A.scores(inp.q, inp.k, q_rounded=True)
    o, lse = C.dense(s, inp.v)
    for chunks in ((585,), (320, 65, 200), (1, 583, 1), (64,) * 9 + (9,), (200, 65, 320), (1,) * 5 + (580,)):
        Ac, Lc = C.chain(s, inp.v, chunks)
        assert float((Ac - o).abs().max()) <= 1e-12 * max(1.0, float(o.abs().max())), (family, spike, chunks)
        assert float((Lc - lse).abs().max()) <= 1e-12 * max(1.0, float(lse.abs().max())), (family, spike, chunks)


def test_carry_argument_validation_needs_no_gpu():
    from lightx2v_amd import lib

    L = lib._lib
    a, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4104)
    IN, OUT = lib.ATTN_CARRY_IN, lib.ATTN_CARRY_OUT
    assert (IN, OUT) == (8, 16)
    fn = L.x2v_attn_fwd_bf16_vt_carry
    # (q, ldq, k, ldk, vt, ldvt, o, ldo, acc, ldacc, lse, ldlse, Sq, Sk, H, head_dim, scale, flags, stream)
    for flags in (IN, OUT, IN | OUT):
        assert fn(a, 128, a, 128, a, 64, a, 128, None, 128, a, 64, 4, 4, 1, 128, 0.0, flags, None) == -5  # null acc with a carry bit
        assert b"acc / lse" in L.x2v_last_error()
        assert fn(a, 128, a, 128, a, 64, a, 128, a, 128, None, 64, 4, 4, 1, 128, 0.0, flags, None) == -5  # null lse
        assert fn(a, 128, a, 128, a, 64, a, 128, odd, 128, a, 64, 4, 4, 1, 128, 0.0, flags, None) == -2  # misaligned acc
        assert fn(a, 128, a, 128, a, 64, a, 128, a, 130, a, 64, 4, 4, 1, 128, 0.0, flags, None) == -2  # acc rows not 16-byte aligned
        assert fn(a, 128, a, 128, a, 64, a, 128, a, 128, a, 3, 4, 4, 1, 128, 0.0, flags, None) == -1  # ldlse < Sq
        assert b"ldlse=3" in L.x2v_last_error()
        assert fn(a, 128, a, 128, a, 64, a, 128, a, 124, a, 64, 4, 4, 1, 128, 0.0, flags, None) == -1  # ldacc < H * 128
        assert fn(a, 128, a, 128, a, 64, a, 128, a, 128, a, 64, 4, 4, 1, 64, 0.0, flags, None) == -1  # head_dim
        assert fn(a, 128, a, 128, a, 64, a, 128, a, 128, a, 64, 4, 0, 1, 128, 0.0, flags, None) == -1  # no keys
        assert fn(a, 128, a, 128, a, 64, a, 128, a, 128, a, 64, 4, 4, 1, 128, 0.0, flags | 2, None) == -5  # X2V_ATTN_VT_STAGGER is not a flag of this entry
        assert fn(a, 128, a, 128, a, 64, a, 128, a, 128, a, 64, 0, 4, 1, 128, 0.0, flags, None) == 0  # no query rows: nothing to do
    assert fn(a, 128, a, 128, a, 64, None, 128, a, 128, a, 64, 4, 4, 1, 128, 0.0, IN, None) == -5  # o is written without CARRY_OUT
    assert fn(a, 128, a, 128, a, 64, None, 128, None, 0, None, 0, 4, 4, 1, 128, 0.0, 0, None) == -5
    assert fn(a, 128, None, 128, a, 64, None, 0, a, 128, a, 64, 4, 4, 1, 128, 0.0, OUT, None) == -5  # o may be null under CARRY_OUT, k may not
    assert fn(a, 128, a, 128, a, 64, odd, 128, a, 128, a, 64, 4, 4, 1, 128, 0.0, IN, None) == -2


def test_wan_model_builds_with_ring_and_keeps_its_refusals(monkeypatch):
    from lightx2v_amd import ring, synth, wan

    dims = synth.WAN_DIMS["wan-tiny"]
    wd = synth.synth_wan_weights(dims, seed=3)
    base = dict(target_shape=(16, 3, 8, 8), target_video_length=9, infer_steps=3)
    model = wan.WanModel(wan.default_config(dims, parallel_attn_type="ring", cfg_pair=True, cfg_branch_streams=True, **base), wd, device="cpu")
    tr = model.transformer_infer
    assert isinstance(tr.parallel_attention, ring.RingAttention) and (tr.sp_rank, tr.sp_world) == (0, 1)
    assert not hasattr(tr.parallel_attention, "attend_blocked") and not hasattr(tr.parallel_attention, "begin_exchange")
    assert tr._self_attn_route(None, torch.zeros(1)) == "single"
    assert getattr(model, "_cfg_interleave", None) is None
    for kind in ("hip_radial", "hip_mxfp8"):
        with pytest.raises(NotImplementedError, match=kind + ".*ring"):
            wan.WanModel(wan.default_config(dims, self_attn_1_type=kind, parallel_attn_type="ring", **base), wd, device="cpu")
    with pytest.raises(NotImplementedError, match="parallel_attn_type=ring2d"):
        wan.WanModel(wan.default_config(dims, parallel_attn_type="ring2d", **base), wd, device="cpu")

    # a CFG step under ring: neither the pair pass nor the single-GPU branch streams, even when the config asks for both — two forwards, one after the other
    def no_streams(*a, **k):
        raise AssertionError("the single-GPU CfgBranchStreams was picked up under ring attention")

    monkeypatch.setattr(wan, "CfgBranchStreams", no_streams)
    model.scheduler = types.SimpleNamespace(seq_len=48, latents=types.SimpleNamespace(is_cuda=True))
    assert model._pair_ok({}) is False
    order = []
    model._forward = lambda inputs, positive: (order.append(positive), torch.full((2,), 1.0 if positive else 0.5))[1]
    model.infer({})
    assert order == [True, False]
    g = model.config["sample_guide_scale"]
    assert torch.equal(model.scheduler.noise_pred, torch.full((2,), 0.5 + g * 0.5))


@pytest.mark.parametrize("world", [2, 3])
def test_ring_gloo(world):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1", "--master-port", str(29561 + world),
           os.path.join(ROOT, "tests", "_dist_worker_ring.py")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "RING_DIST_OK" in p.stdout
