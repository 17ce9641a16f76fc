"""The V^T cache append on the GPU (x2v_transpose_heads_append_bf16: include/x2v.h) and what the causal Wan driver builds on it: exactness of the append
at every edge of the 64-key tile and the 16-byte word (tests/kv_append_ref.check_append: the touched range is v's bits, every other element is
untouched), a chain of appends against the whole-sequence transpose, attention over a partly filled cache against attention over exactly its keys, and
the norm + RoPE kernel's token offset against one call over the whole sequence.  Everything here is a bit comparison; shapes are the smallest at which
each path of the kernel runs (first / interior / last tile, aligned and straddling words, one and several heads, spare tiles behind the range)."""
import numpy as np
import pytest
import torch

from tests import kv_append_ref as R

pytestmark = pytest.mark.gpu

CASES = [
    (0, 64),  # whole first tile
    (0, 45),  # partial tile from key 0
    (45, 45),  # odd start, crosses one tile boundary
    (90, 45),  # even non-multiple-of-8 start
    (135, 45),  # odd start, crosses a boundary
    (5, 3),  # range inside one tile
    (63, 2),  # crosses a boundary with two keys
    (64, 1),  # one key at a tile start
    (8, 200),  # aligned path with interior tiles
    (7, 201),  # merge path with interior tiles
    (56, 8),  # aligned range ending on a tile boundary
]
POISON = 0x7FC1  # a NaN pattern: rows, columns and tiles outside the operands' windows


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    return L


def _u16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _bf16(a, device="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.bfloat16).to(device)


@pytest.mark.parametrize("spare_tiles", [0, 2])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("key0,S", CASES)
def test_append_is_a_bit_copy_that_touches_nothing_else(lib, key0, S, H, spare_tiles):
    tiles = (key0 + S + 63) // 64 + spare_tiles
    n = H * tiles * 128 * 64
    guard = 128 * 64  # one tile of poison in front of and behind the cache
    big_vt = torch.from_numpy(np.full(n + 2 * guard, POISON, dtype=np.uint16).view(np.int16)).view(torch.bfloat16).cuda()
    before = R.cache_pattern(H, tiles)
    vt = big_vt[guard : guard + n].view(H, tiles, 128, 64)
    vt.copy_(_bf16(before))
    ldv = H * 128 + 8
    v_bits = R.v_pattern(S, H, seed=key0 + S)
    big_v = np.full((S + 4, ldv), POISON, dtype=np.uint16)
    big_v[2 : S + 2, : H * 128] = v_bits
    v = _bf16(big_v)[2 : S + 2, : H * 128]
    assert v.stride(0) == ldv and v.data_ptr() % 16 == 0 and vt.data_ptr() % 16 == 0 and vt.is_contiguous()
    assert lib.transpose_heads_append(v, vt, key0) is vt
    torch.cuda.synchronize()
    R.check_append(before, _u16(vt), v_bits, key0)
    big = _u16(big_vt)
    assert (big[:guard] == POISON).all() and (big[guard + n :] == POISON).all(), "wrote outside the cache"


@pytest.mark.parametrize("H", [1, 3])
def test_chain_of_appends_is_the_whole_sequence_transpose(lib, H):
    v = _bf16(R.v_pattern(180, H))
    vt = torch.zeros((H, 3, 128, 64), dtype=torch.bfloat16, device="cuda")
    for j in range(4):
        lib.transpose_heads_append(v[45 * j : 45 * j + 45], vt, 45 * j)
    assert torch.equal(vt.view(torch.int16), lib.transpose_heads(v, H).view(torch.int16))
    lib.transpose_heads_append(v[:0], vt, 17)  # no rows: nothing happens
    assert torch.equal(vt.view(torch.int16), lib.transpose_heads(v, H).view(torch.int16))


@pytest.fixture(scope="module")
def qkv():
    g = torch.Generator().manual_seed(20)
    H = 2
    q, k, v = (torch.randn(180, H * 128, generator=g).to(torch.bfloat16).cuda() for _ in range(3))
    return H, q[:45].contiguous(), k, v


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("kv_end", [45, 90, 135, 180])
def test_attention_over_the_cache_equals_attention_over_its_keys(lib, qkv, kv_end, prescaled):
    """Capacity 256; the cache's bytes behind kv_end hold a finite non-zero pattern (a masked key's probability is 0 and is still multiplied with the
    V^T entry).  The last tile is partly valid at 45, 90 and 135."""
    H, q, k, v = qkv
    if prescaled:
        q = (q.float() * lib.ATTN_PRESCALE).to(torch.bfloat16)
    k_cache = _bf16(R.v_pattern(256, H, seed=3))
    k_cache[:kv_end].copy_(k[:kv_end])
    vt_cache = _bf16(R.cache_pattern(H, 4))
    for s in range(0, kv_end, 45):
        lib.transpose_heads_append(v[s : s + 45], vt_cache, s)
    got = lib.attention_cached(q, k_cache, vt_cache, kv_end, H, prescaled=prescaled)
    want = lib.attention(q, k[:kv_end], None, H, vt=lib.transpose_heads(v[:kv_end], H), variant=lib.ATTN_FAST | (lib.ATTN_Q_PRESCALED if prescaled else 0))
    assert torch.isfinite(want.float()).all()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    with pytest.raises(lib.X2VError):
        lib.attention_cached(q, k_cache, vt_cache, 257, H)


@pytest.mark.parametrize("round_mode", [0, 1])
def test_rope_offset_of_a_block_equals_its_rows_of_the_whole_sequence(lib, round_mode):
    """Block j of 4 x 45 tokens on the grid (12, 5, 3): s0 = 45 j on the grid ((j + 1) * 3, 5, 3) gives the bits of rows [45 j, 45 j + 45) of one call
    over all 180 rows — the frame offset of compute_freqs_causvid as the kernel's token offset."""
    from lightx2v_amd import wan

    H = 2
    g = torch.Generator().manual_seed(21)
    q0, k0 = (torch.randn(180, H * 128, generator=g).to(torch.bfloat16).cuda() for _ in range(2))
    wq, wk = ((1 + 0.1 * torch.randn(H * 128, generator=g)).to(torch.bfloat16).cuda() for _ in range(2))
    cs = wan.rope_cos_sin_table(128, "cuda")
    kw = dict(round_mode=round_mode, q_out_scale=lib.ATTN_PRESCALE if round_mode == 0 else 1.0)
    qa, ka = q0.clone(), k0.clone()
    lib.rmsnorm_rope_(qa, ka, wq, wk, cs, (12, 5, 3), H, s0=0, **kw)
    for j in range(4):
        rows = slice(45 * j, 45 * j + 45)
        qb, kb = q0[rows].clone(), k0[rows].clone()
        lib.rmsnorm_rope_(qb, kb, wq, wk, cs, ((j + 1) * 3, 5, 3), H, s0=45 * j, **kw)
        assert torch.equal(qb.view(torch.int16), qa[rows].view(torch.int16)) and torch.equal(kb.view(torch.int16), ka[rows].view(torch.int16)), j
