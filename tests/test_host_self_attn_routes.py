"""WanTransformerInfer's self-attention call path on the host: which route a call takes, where the "single" route's V operand comes from, and which
combinations are refused.  The expected values are the tables below, typed in from the conditions the driver documents, not computed from the driver."""
import itertools
import types

import pytest


def infer(**attrs):
    from lightx2v_amd import synth, wan

    tr = wan.WanTransformerInfer(wan.default_config(synth.WAN_DIMS["wan-tiny"]))
    for k, v in attrs.items():
        setattr(tr, k, v)
    return tr


def weights(blocked_ok=True, apply_vt=True):
    v = types.SimpleNamespace(accepts_blocked=blocked_ok)
    if apply_vt:
        v.apply_vt = lambda n1, heads: None
    return types.SimpleNamespace(self_attn_v=v, self_attn_o=types.SimpleNamespace(accepts_blocked=blocked_ok))


PA = {"none": lambda: None, "blocked": lambda: types.SimpleNamespace(attend_blocked=lambda *a, **kw: None), "callable": lambda: (lambda **kw: None)}

# (pa, x.is_cuda, blocked_exchange, _blocked_ok, _pair set) -> route: "ulysses_blocked" needs all of a parallel-attention object with attend_blocked, a
# device tensor, the blocked_exchange switch and operator classes that take block-strided operands; otherwise the pair pass where _pair is set; else
# "single" (one GPU, or Ulysses in its row-major form)
ROUTES = {
    ("none", False, False, False, False): "single",
    ("none", False, False, False, True): "pair",
    ("none", False, False, True, False): "single",
    ("none", False, False, True, True): "pair",
    ("none", False, True, False, False): "single",
    ("none", False, True, False, True): "pair",
    ("none", False, True, True, False): "single",
    ("none", False, True, True, True): "pair",
    ("none", True, False, False, False): "single",
    ("none", True, False, False, True): "pair",
    ("none", True, False, True, False): "single",
    ("none", True, False, True, True): "pair",
    ("none", True, True, False, False): "single",
    ("none", True, True, False, True): "pair",
    ("none", True, True, True, False): "single",
    ("none", True, True, True, True): "pair",
    ("blocked", False, False, False, False): "single",
    ("blocked", False, False, False, True): "pair",
    ("blocked", False, False, True, False): "single",
    ("blocked", False, False, True, True): "pair",
    ("blocked", False, True, False, False): "single",
    ("blocked", False, True, False, True): "pair",
    ("blocked", False, True, True, False): "single",
    ("blocked", False, True, True, True): "pair",
    ("blocked", True, False, False, False): "single",
    ("blocked", True, False, False, True): "pair",
    ("blocked", True, False, True, False): "single",
    ("blocked", True, False, True, True): "pair",
    ("blocked", True, True, False, False): "single",
    ("blocked", True, True, False, True): "pair",
    ("blocked", True, True, True, False): "ulysses_blocked",
    ("blocked", True, True, True, True): "ulysses_blocked",
    ("callable", False, False, False, False): "single",
    ("callable", False, False, False, True): "pair",
    ("callable", False, False, True, False): "single",
    ("callable", False, False, True, True): "pair",
    ("callable", False, True, False, False): "single",
    ("callable", False, True, False, True): "pair",
    ("callable", False, True, True, False): "single",
    ("callable", False, True, True, True): "pair",
    ("callable", True, False, False, False): "single",
    ("callable", True, False, False, True): "pair",
    ("callable", True, False, True, False): "single",
    ("callable", True, False, True, True): "pair",
    ("callable", True, True, False, False): "single",
    ("callable", True, True, False, True): "pair",
    ("callable", True, True, True, False): "single",
    ("callable", True, True, True, True): "pair",
}


def test_route_truth_table():
    assert set(ROUTES) == set(itertools.product(PA, (False, True), (False, True), (False, True), (False, True)))
    for (pa, is_cuda, blocked_exchange, blocked_ok, pair), want in ROUTES.items():
        tr = infer(parallel_attention=PA[pa](), blocked_exchange=blocked_exchange, _pair=(48, 64) if pair else None)
        before = dict(vars(tr))
        got = tr._self_attn_route(weights(blocked_ok=blocked_ok), types.SimpleNamespace(is_cuda=is_cuda))
        assert got == want, (pa, is_cuda, blocked_exchange, blocked_ok, pair)
        assert vars(tr) == before, "the route decision changed the driver"
        assert callable(getattr(tr, "_self_attn_" + got))


# (fast, radial, mx_attn, mmkw non-empty, apply_vt present, pa set) -> V source of the "single" route.  V^T comes from the v projection's epilogue iff
# pa is None and (fast or radial) and not mx_attn and not mmkw and apply_vt exists; otherwise v is row-major, and it is transposed after norm+RoPE
# iff pa is None and not mx_attn and (fast or radial).
V_SOURCES = {
    (False, False, False, False, False, False): "row_major",
    (False, False, False, False, False, True): "row_major",
    (False, False, False, False, True, False): "row_major",
    (False, False, False, False, True, True): "row_major",
    (False, False, False, True, False, False): "row_major",
    (False, False, False, True, False, True): "row_major",
    (False, False, False, True, True, False): "row_major",
    (False, False, False, True, True, True): "row_major",
    (False, False, True, False, False, False): "row_major",
    (False, False, True, False, False, True): "row_major",
    (False, False, True, False, True, False): "row_major",
    (False, False, True, False, True, True): "row_major",
    (False, False, True, True, False, False): "row_major",
    (False, False, True, True, False, True): "row_major",
    (False, False, True, True, True, False): "row_major",
    (False, False, True, True, True, True): "row_major",
    (False, True, False, False, False, False): "vt_transposed",
    (False, True, False, False, False, True): "row_major",
    (False, True, False, False, True, False): "vt_epilogue",
    (False, True, False, False, True, True): "row_major",
    (False, True, False, True, False, False): "vt_transposed",
    (False, True, False, True, False, True): "row_major",
    (False, True, False, True, True, False): "vt_transposed",
    (False, True, False, True, True, True): "row_major",
    (False, True, True, False, False, False): "row_major",
    (False, True, True, False, False, True): "row_major",
    (False, True, True, False, True, False): "row_major",
    (False, True, True, False, True, True): "row_major",
    (False, True, True, True, False, False): "row_major",
    (False, True, True, True, False, True): "row_major",
    (False, True, True, True, True, False): "row_major",
    (False, True, True, True, True, True): "row_major",
    (True, False, False, False, False, False): "vt_transposed",
    (True, False, False, False, False, True): "row_major",
    (True, False, False, False, True, False): "vt_epilogue",
    (True, False, False, False, True, True): "row_major",
    (True, False, False, True, False, False): "vt_transposed",
    (True, False, False, True, False, True): "row_major",
    (True, False, False, True, True, False): "vt_transposed",
    (True, False, False, True, True, True): "row_major",
    (True, False, True, False, False, False): "row_major",
    (True, False, True, False, False, True): "row_major",
    (True, False, True, False, True, False): "row_major",
    (True, False, True, False, True, True): "row_major",
    (True, False, True, True, False, False): "row_major",
    (True, False, True, True, False, True): "row_major",
    (True, False, True, True, True, False): "row_major",
    (True, False, True, True, True, True): "row_major",
    (True, True, False, False, False, False): "vt_transposed",
    (True, True, False, False, False, True): "row_major",
    (True, True, False, False, True, False): "vt_epilogue",
    (True, True, False, False, True, True): "row_major",
    (True, True, False, True, False, False): "vt_transposed",
    (True, True, False, True, False, True): "row_major",
    (True, True, False, True, True, False): "vt_transposed",
    (True, True, False, True, True, True): "row_major",
    (True, True, True, False, False, False): "row_major",
    (True, True, True, False, False, True): "row_major",
    (True, True, True, False, True, False): "row_major",
    (True, True, True, False, True, True): "row_major",
    (True, True, True, True, False, False): "row_major",
    (True, True, True, True, False, True): "row_major",
    (True, True, True, True, True, False): "row_major",
    (True, True, True, True, True, True): "row_major",
}


def test_v_source_truth_table():
    assert set(V_SOURCES) == set(itertools.product((False, True), repeat=6))
    for (fast, radial, mx_attn, mmkw, apply_vt, pa), want in V_SOURCES.items():
        tr = infer(radial=radial, mx_attn=mx_attn, parallel_attention=PA["callable"]() if pa else None)
        before = dict(vars(tr))
        got = tr._v_source(weights(apply_vt=apply_vt), {"x_scale": None} if mmkw else {}, fast)
        assert got == want, (fast, radial, mx_attn, mmkw, apply_vt, pa)
        assert vars(tr) == before, "the operand choice changed the driver"


def test_refusals_per_call():
    """Checked on every call, since radial, _pair and parallel_attention are set on live objects; what is built raises nothing."""
    ulysses = PA["callable"]()
    for attrs, pattern in (
        (dict(mx_attn=True, parallel_attention=ulysses), "hip_mxfp8.*Ulysses"),
        (dict(mx_attn=True, _pair=(48, 64)), "hip_mxfp8.*pair"),
        (dict(mx_attn=True, radial=True), "hip_mxfp8.*radial"),
        (dict(radial=True, parallel_attention=ulysses), "hip_radial.*Ulysses"),
        (dict(radial=True, _pair=(48, 64)), "hip_radial.*pair"),
    ):
        with pytest.raises(NotImplementedError, match=pattern):
            infer(**attrs)._refuse_unbuilt_self_attn()
    for attrs in (dict(), dict(radial=True), dict(mx_attn=True), dict(parallel_attention=ulysses), dict(_pair=(48, 64)), dict(parallel_attention=ulysses, _pair=(48, 64))):
        infer(**attrs)._refuse_unbuilt_self_attn()


def test_refusals_at_construction():
    """WanModel refuses the Ulysses combinations before it wraps the driver, and the pair-pass gate answers False for radial and mxfp8 without raising."""
    from lightx2v_amd import synth, wan

    dims = synth.WAN_DIMS["wan-tiny"]
    wd = synth.synth_wan_weights(dims, seed=3)
    for kind in ("hip_radial", "hip_mxfp8"):
        cfg = wan.default_config(dims, target_shape=(16, 3, 8, 8), target_video_length=9, infer_steps=3, self_attn_1_type=kind, parallel_attn_type="ulysses")
        with pytest.raises(NotImplementedError, match=kind + ".*ulysses"):
            wan.WanModel(cfg, wd, device="cpu")
        model = wan.WanModel(dict(cfg, parallel_attn_type=None, cfg_pair=True), wd, device="cpu")
        model.scheduler = types.SimpleNamespace(seq_len=48, latents=types.SimpleNamespace(is_cuda=True))
        assert model._pair_ok({}) is False
    dense = wan.WanModel(wan.default_config(dims, target_shape=(16, 3, 8, 8), target_video_length=9, infer_steps=3, cfg_pair=True), wd, device="cpu")
    dense.scheduler = types.SimpleNamespace(seq_len=48, latents=types.SimpleNamespace(is_cuda=True))
    assert dense._pair_ok({}) is True
