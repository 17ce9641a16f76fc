"""wan.cfg_front_form, the gate of the CFG-shared front, on the host: which forms of a CFG step share block 0's front and which keep both halves."""
import types

import torch


def test_gate_picks_shared_only_for_the_plain_pair_pass_on_one_tensor():
    from lightx2v_amd import synth, wan

    dims = synth.WAN_DIMS["wan-tiny"]
    cfg = wan.default_config(dims)
    assert cfg["cfg_shared_front"] is True
    tr = wan.WanTransformerInfer(cfg)
    x = torch.zeros(4, dims["dim"], dtype=torch.bfloat16)
    form = wan.cfg_front_form

    def block0(accepts):
        op = types.SimpleNamespace(accepts_resid_period=True) if accepts else types.SimpleNamespace()
        return types.SimpleNamespace(compute_phases=[None, None, types.SimpleNamespace(cross_attn_o=op), None])

    assert form(cfg, tr, x, x) == "shared"
    assert form(cfg, tr, x, x, block0(True)) == "shared"
    # the forms that keep computing both halves
    assert form(cfg, tr, x, x, form="separate") == "unshared"
    assert form(cfg, tr, x, x, form="streams") == "unshared"
    assert form(dict(cfg, cfg_shared_front=False), tr, x, x) == "unshared"
    assert form(cfg, tr, x, x.clone()) == "unshared"  # equal values, another tensor: a pre-infer hook may have made them differ
    assert form(cfg, tr, x, x + 1) == "unshared"
    assert form(cfg, tr, x, x, block0(False)) == "unshared"  # an operator class whose epilogue has no residual row period (mxfp8)
    tea_cfg = wan.default_config(dims, feature_caching="Tea", teacache_thresh=0.2, use_ret_steps=False, coefficients=[[0, 0, 0, 1.0, 0], [0, 0, 0.5, 1.0, 0]])
    assert form(tea_cfg, wan.WanTransformerInferTeaCaching(tea_cfg), x, x) == "unshared"  # skipped / residual-replay steps are per branch
    ulysses = wan.WanTransformerInfer(cfg)
    ulysses.parallel_attention = lambda **kw: None
    assert form(cfg, ulysses, x, x) == "unshared"
    # a config without the key (one written before it existed) shares: default on
    assert form({k: v for k, v in cfg.items() if k != "cfg_shared_front"}, tr, x, x) == "shared"


def test_operator_classes_declare_the_residual_row_period():
    from lightx2v_amd import ops

    assert ops.MMWeightHip.accepts_resid_period and ops.MMWeightFp8Hip.accepts_resid_period
    assert not getattr(ops.MMWeightMxfp8Hip, "accepts_resid_period", False)
