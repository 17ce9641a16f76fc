"""x2v_attn_frames_fwd_bf16 (per-frame cross-attention, include/x2v.h) on the GPU against tests/attn_frames_ref.py at attn_ref.Case.check's bar: the
smallest shapes that can break (rows per frame below one 64-row tile, no multiple of one, just above 256; 2 and 8 key tiles; 1 and 3 heads), ranges
with partial first / last frames, padded strides, o inside a poisoned buffer; and the entry's contracts."""
import itertools

import pytest
import torch

from tests import attn_frames_ref as R
from tests import attn_ref as A

pytestmark = pytest.mark.gpu
POISON = 24576.0  # exact in bf16
N_FRAMES = 3


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    return L


def padded(t, pad):
    """t [H, rows, 128] (CPU) -> a device view [rows, H*128] with token stride H*128 + pad."""
    H, rows, _ = t.shape
    buf = torch.zeros(rows, H * 128 + pad, dtype=torch.bfloat16, device="cuda")
    buf[:, : H * 128] = t.permute(1, 0, 2).reshape(rows, H * 128).cuda()
    return buf[:, : H * 128]


def run(lib, inp, row0, Sq, pre, k=None, v=None):
    """One launch on rows [row0, row0 + Sq): (output window, the poisoned buffer around it)."""
    W = inp.H * 128
    q = padded(inp.q_for(pre)[:, row0 : row0 + Sq], 8)
    k = padded(inp.k.reshape(inp.H, -1, 128), 16) if k is None else k
    v = padded(inp.v.reshape(inp.H, -1, 128), 24) if v is None else v
    big = torch.full((Sq + 4, W + 8), POISON, dtype=torch.bfloat16, device="cuda")
    out = big[2 : Sq + 2, :W]
    assert lib.attention_frames(q, k, v, inp.H, inp.rpf, row0=row0, keys_per_frame=inp.Kf, prescaled=pre, out=out) is out
    torch.cuda.synchronize()
    return out, big


def intact(big, Sq, W):
    return bool((big[:2] == POISON).all() and (big[Sq + 2 :] == POISON).all() and (big[:, W:] == POISON).all())


@pytest.mark.parametrize("H,Kf,rpf,pre", list(itertools.product((1, 3), (32, 128), (40, 200, 264), (False, True))))
def test_attn_frames_vs_float64(lib, H, Kf, rpf, pre):
    inp, case = R.FrameInputs(H, Kf, N_FRAMES, rpf), A.Case("attn_frames", record=False)
    for row0, Sq in R.ranges(rpf):
        exp = R.Expect(inp, row0, Sq, pre)
        if Sq > 1:  # the inputs separate the frames: the reference of the WRONG frame is outside the bar by orders of magnitude
            wrong = R.Expect(inp, row0, Sq, pre, shift=1).o
            assert float(((wrong - exp.o).abs() / exp.tol()).median()) > 20
            with pytest.raises(A.Reject):
                case.check(wrong.to(torch.bfloat16), exp)
        out, big = run(lib, inp, row0, Sq, pre)
        assert intact(big, Sq, H * 128), f"{inp.name} rows [{row0}, {row0 + Sq}): bytes outside the output window changed"
        rel, Y, worst = case.check(out.cpu().view(Sq, H, 128).permute(1, 0, 2), exp, f"row0={row0} Sq={Sq} pre={pre}")
        print(f"{inp.name} row0={row0} Sq={Sq} pre={pre}: relL2 {rel:.3e} Y {Y:.3e} worst d/tol {worst:.3f}")


def test_attn_frames_contracts(lib):
    H, Kf, rpf = 3, 128, 200
    inp = R.FrameInputs(H, Kf, N_FRAMES, rpf)
    row0, Sq = rpf + 5, rpf - 9  # inside frame 1
    out, _ = run(lib, inp, row0, Sq, False)
    # rows of k / v outside the attended frame are never read: NaN there leaves every bit as it was
    k, v = inp.k.clone(), inp.v.clone()
    k[:, 0], k[:, 2], v[:, 0], v[:, 2] = float("nan"), float("nan"), float("nan"), float("nan")
    out2, big = run(lib, inp, row0, Sq, False, padded(k.reshape(H, -1, 128), 16), padded(v.reshape(H, -1, 128), 24))
    assert torch.equal(out, out2) and intact(big, Sq, H * 128)
    # Sq == 0: no launch, nothing written
    kd, vd = padded(inp.k.reshape(H, -1, 128), 0), padded(inp.v.reshape(H, -1, 128), 0)
    big = torch.full((4, H * 128), POISON, dtype=torch.bfloat16, device="cuda")
    lib.attention_frames(kd[:0], kd, vd, H, rpf, row0=17, out=big[:0])
    torch.cuda.synchronize()
    assert (big == POISON).all()
    # every shape / alignment condition is an error code, raised without a launch: the output stays poisoned
    W, q = H * 128, padded(inp.q[:, :64], 0)
    big.fill_(POISON)
    o = torch.full((64, W), POISON, dtype=torch.bfloat16, device="cuda")
    P = lambda t, off=0: t.data_ptr() + off
    ok = dict(q=P(q), ldq=W, k=P(kd), ldk=W, v=P(vd), ldv=W, o=P(o), ldo=W, Sq=64, row0=0, rpf=rpf, n_frames=N_FRAMES, Kf=Kf, H=H, hd=128, scale=0.0, flags=0, stream=None)
    call = lambda **kw: lib._lib.x2v_attn_frames_fwd_bf16(*{**ok, **kw}.values())
    shape = [dict(hd=64), dict(Kf=48), dict(Kf=0), dict(Kf=160), dict(rpf=0), dict(row0=-1), dict(row0=3 * rpf - 63), dict(Sq=3 * rpf + 1), dict(H=0), dict(H=65536),
             dict(ldq=W - 8), dict(ldk=W - 8), dict(ldv=W - 8), dict(ldo=W - 8)]
    align = [dict(ldq=W + 4), dict(ldk=W + 4), dict(ldv=W + 4), dict(ldo=W + 4), dict(q=P(q, 8)), dict(k=P(kd, 8)), dict(v=P(vd, 8)), dict(o=P(o, 8))]
    for kw in shape:
        assert call(**kw) == -1, f"{kw}: expected X2V_E_SHAPE"
    for kw in align:
        assert call(**kw) == -2, f"{kw}: expected X2V_E_ALIGN"
    assert call(flags=2) == -5
    torch.cuda.synchronize()
    assert (o == POISON).all()
    assert call() == 0  # the same arguments, unmodified, launch
    torch.cuda.synchronize()
    assert not (o == POISON).any()
    with pytest.raises(lib.X2VError):
        lib.attention_frames(q, kd[:100], vd[:100], H, rpf)  # k / v are not whole frames
