"""The fused fp16 wide-head attention of the HunyuanVideo VAE mid block (lightx2v_amd/csrc/vae_attn.hip, lib.vae_attention16) against the float64
reference of tests/vae_attn16_ref.py at the edges of its key walk: a frame boundary on a 64-key tile edge and one key either side of it, pure causal
rows (every row its own limit), one frame (only the tail from n on is masked), blocks that span frames, last blocks of 4 and 6 rows, and the lazy
reference maximum moving at every tile, at every second or third, at different tiles for the rows of one block, and by so much that the rescale
factor underflows.

Acceptance is vae_attn16_ref.Case.check on every call: |got - o| <= 1.05 * 2^-10 * A + 2^-22 |o| on EVERY element, relL2 <= 1.5 * Y (Y from the CPU
emulations, never from the kernel), and family U read out to 2^-21: a prefix limit off by one key in any row fails it.
tests/test_vae_attn16_ref_host.py shows which subtly wrong kernels this rejects.

Every call reads qkv as the window [:, :3C] of a [n + 2, 3C + 8] buffer whose padding is NaN, through operand buffers filled with NaN beforehand, and
writes the window [1 : n + 1, 4 : 4 + C] of a poisoned [n + 3, C + 8] buffer whose surroundings are checked afterwards; a second call into fresh poison
must give the same bits."""
import os

import pytest
import torch

from tests import vae_attn16_ref as V

pytestmark = pytest.mark.gpu
POISON = -1984.0  # no output of these cases comes near it
CASE = V.Case("vae_attention16")


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    yield L
    path = os.environ.get("X2V_VAE_ATTN16_PARITY_TABLE")  # where to write the table of measured ratios (profiles/vae_attn16_fp64_parity.txt is one run's)
    if not path:
        return
    try:
        with open(path, "w") as f:
            f.write(f"# {CASE.name}: {len(CASE.rows)} checks, largest relL2 / Y = {CASE.max_ratio:.3f}, largest d/tol = {CASE.max_worst:.3f}\n")
            f.write("\n".join(CASE.table()) + "\n")
    except OSError:
        pass


def run(lib, inp):
    n, C = inp.n, inp.C
    src = torch.full((n + 2, 3 * C + 8), float("nan"), device="cuda")
    src[:n, : 3 * C] = inp.qkv.cuda()
    outs = []
    for _ in range(2):
        bufs = lib.vae_attention16_buffers(n, C, "cuda")
        for b in bufs:
            b.fill_(float("nan"))
        big = torch.full((n + 3, C + 8), POISON, device="cuda")
        out = big[1 : n + 1, 4 : 4 + C]
        lib.vae_attention16(src[:, : 3 * C], n, C, inp.hw, inp.scale, out, buffers=bufs)
        outs.append(out.clone())
        out.fill_(POISON)
        assert bool((big == POISON).all()), f"{inp.name}: a store outside out[{n}, {C}]"
    assert torch.equal(outs[0], outs[1]), f"{inp.name}: two calls on the same inputs differ"
    return outs[0].cpu()


@pytest.mark.parametrize("C,hw,frames", V.CASES)
def test_vae_attention16_vs_float64_at_every_walk_edge(lib, C, hw, frames):
    for inp in V.case_inputs(C, hw, frames, V.gpu_families(C, hw, frames)):
        rel, Y, worst = CASE.check(run(lib, inp), V.expect(inp))
        print(f"vae_attention16 {inp.name}: relL2 {rel:.3e} Y {Y:.3e} worst d/tol {worst:.3f}")
