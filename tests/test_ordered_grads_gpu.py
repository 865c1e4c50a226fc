"""GPU: the parameter-gradient sums of the training backward are added in a fixed order (nm_layernorm_bwd_ordered, nm_col_sum_ordered):
the same bits on every run, at sizes where many workgroups contribute to one output element."""
import ctypes as C

import pytest
import torch

from nerfmatch_amd import _lib, ops


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim", [(7200, 256), (1601, 128), (3, 64)])
def test_layernorm_bwd_parameter_gradients_are_reproducible(gpu, built_lib, rows, dim):
    x, g, dy = rnd(rows, dim, seed=1).to(gpu), (1 + 0.1 * rnd(dim, seed=2)).to(gpu), rnd(rows, dim, seed=3).to(gpu)
    runs = [ops.layernorm_bwd(x, g, dy) for _ in range(4)]
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, runs[0]))
    xh = torch.nn.functional.layer_norm(x.double(), (dim,))
    ref_g, ref_b = (dy.double() * xh).sum(0), dy.double().sum(0)
    assert (runs[0][1].double() - ref_g).abs().max() < 1e-5 * ref_g.abs().max().clamp_min(1.0)
    assert (runs[0][2].double() - ref_b).abs().max() < 1e-5 * ref_b.abs().max().clamp_min(1.0)
    assert torch.equal(runs[0][0], ops.layernorm_bwd(x, g, dy, param_grads=False)[0])  # dx does not depend on the form


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", [(100000, 128), (4800, 256), (50, 96), (1000, 70)])
def test_col_sum_is_reproducible(gpu, built_lib, M, N):
    dy = rnd(M, N, seed=4).to(gpu)
    runs = [ops.col_sum(dy) for _ in range(4)]
    assert all(torch.equal(r, runs[0]) for r in runs[1:])
    ref = dy.double().sum(0)
    assert (runs[0].double() - ref).abs().max() < 2e-6 * ref.abs().max()


def test_ordered_forms_check_their_workspace(built_lib):
    h = _lib.lib()
    buf = (C.c_char * 64)()
    p, null = C.cast(buf, C.c_void_p), C.c_void_p(0)
    assert h.nm_col_sum_workspace_bytes(100000, 128) == 256 * 128 * 4 and h.nm_col_sum_workspace_bytes(50, 96) == 96 * 4
    assert h.nm_col_sum_ordered(p, 4800, 256, 0, p, null, 0, null) == 4 and h.nm_col_sum_ordered(p, 4800, 256, 0, p, p, 64, null) == 4
    assert h.nm_col_sum_ordered(null, 4800, 256, 0, p, p, 1 << 20, null) == 1
    assert h.nm_layernorm_bwd_workspace_bytes(3, 64) == 2 * 64 * 4
    assert h.nm_layernorm_bwd_ordered(p, p, p, 8, 256, 1e-5, p, p, p, null, 0, null) == 4
    assert h.nm_layernorm_bwd_ordered(p, p, p, 8, 256, 1e-5, p, null, null, p, 1 << 20, null) == 1
    assert h.nm_layernorm_bwd_ordered(p, p, p, 8, 100, 1e-5, p, p, p, p, 1 << 20, null) == 2
