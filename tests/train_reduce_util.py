"""Shared helper of the row-reduction tests (csrc/train.hip): exact probes, fp64 references and Python mirrors of the host's slicing.

Exact probes.  The kernels under test sum over rows.  Operands whose every partial sum is representable in fp32 give the same bits in any
summation order -- across row slices, wavefront quarters, LDS trees and float atomics -- so a test can ask `torch.equal` against fp64 and a
single misplaced element of a ragged tile shows, however small it is.
  * integer probe: integers in [-4, 4] (bf16 holds them exactly: hi = v, lo = 0); |sum| <= 16 M < 2^24 up to M = 10^6.
  * split-term probes (split-bf16 kernel, M <= 512): ONE operand is +-(1 + 2^-12), the other an integer.  Then hi = +-1 and lo = +-2^-12, every
    product and partial sum is a multiple of 2^-12 below 2^12, and the truth contains the hi.lo (probe "a": x split) resp. lo.hi (probe "b": dy
    split) term: a kernel that dropped it would be off by 2^-12 sum(integer operand).  Never both operands split: lo.lo is dropped by design.
  * LayerNorm probe: rows of +-1 with as many of each, integer gamma in [1, 3], integer dy in [-4, 4], eps = 0: mean 0, variance 1, rstd 1 and
    xh = x exactly; the two row means divide by dim, a power of two.

Mirrors.  `wgrad_plan_fp32`, `wgrad_plan_bf16x3`, `col_sum_plan` and `ln_bwd_grid` repeat the arithmetic of nm_linear_wgrad, wb_slices /
nm_linear_wgrad_bf16x3, nm_col_sum(_ordered) and ln_bwd_grid, so that every GPU case can assert the edge it is meant to hit; the CPU test pins them
to the library's workspace queries.
"""
from collections import namedtuple

import torch

WG_TARGET, WG_MAX_SPLITS, WG_CHUNK = 512, 16, 32  # nm_linear_wgrad
WB_TARGET, WB_MAX_SLICES, WB_PART_BYTES = 384, 128, 16 << 20  # wb_slices
MIN_ROWS_PER_SLICE = 256
COL_SUM_MAX_CHUNKS, COL_SUM_MIN_ROWS = 256, 64
SPLIT_LO = 2.0**-12


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------ mirrors
PlanFp32 = namedtuple("PlanFp32", "tiles splits rows_per first_guess")
PlanBf16x3 = namedtuple("PlanBf16x3", "tiles slices rows_per rpw last_wave_rows first_guess")
PlanColSum = namedtuple("PlanColSum", "chunks rows_per parts")


def wgrad_plan_fp32(M, N, K):
    """nm_linear_wgrad: 64x64 tiles; rows in `splits` slices of `rows_per` (a multiple of the 32-row chunk); first_guess: the slice count
    before rows_per was rounded up."""
    tiles = cdiv(N, 64) * cdiv(K, 64)
    s0 = max(1, min(cdiv(WG_TARGET, tiles), WG_MAX_SPLITS, cdiv(M, MIN_ROWS_PER_SLICE)))
    rows_per = cdiv(cdiv(M, s0), WG_CHUNK) * WG_CHUNK
    return PlanFp32(tiles, cdiv(M, rows_per), rows_per, s0)


def wgrad_plan_bf16x3(M, N, K):
    """nm_linear_wgrad_bf16x3: 64x128 tiles; `slices` of `rows_per` rows, each cut into four wavefront quarters of `rpw` rows;
    last_wave_rows: the rows held by wavefronts 0..3 of the LAST slice."""
    tiles = cdiv(N, 64) * cdiv(K, 128)
    s = max(1, min(cdiv(WB_TARGET, tiles), WB_MAX_SLICES, cdiv(M, MIN_ROWS_PER_SLICE), WB_PART_BYTES // (4 * N * K)))
    rows_per = cdiv(cdiv(M, s), 64) * 64
    slices = cdiv(M, rows_per)
    rpw = cdiv(cdiv(rows_per, 4), 16) * 16
    lo = (slices - 1) * rows_per
    hi = min(M, lo + rows_per)
    last = tuple(max(0, min(hi, lo + (w + 1) * rpw) - (lo + w * rpw)) for w in range(4))
    return PlanBf16x3(tiles, slices, rows_per, rpw, last, s)


def wgrad_workspace_bytes(M, N, K):
    """nm_linear_wgrad_workspace_bytes: room for the larger of the two kernels' partial tiles, sized by the FIRST guess of the slice count
    (rounding rows_per up can only lower it)."""
    return max(WG_MAX_SPLITS, wgrad_plan_bf16x3(M, N, K).first_guess) * N * K * 4


def col_sum_plan(M):
    """nm_col_sum / nm_col_sum_ordered: `chunks` is the first guess (it sizes the workspace), `parts` the row chunks actually launched."""
    chunks = max(1, min(COL_SUM_MAX_CHUNKS, M // COL_SUM_MIN_ROWS))
    rows_per = cdiv(M, chunks)
    return PlanColSum(chunks, rows_per, cdiv(M, rows_per))


def ln_bwd_grid(rows, cus, param_grads):
    """workgroups (of four one-row wavefronts) of layernorm_bwd_kernel = partial rows of the ordered form when param_grads."""
    return max(1, min(cdiv(rows, 4), (1 if param_grads else 2) * cus))


# ------------------------------------------------------------------------------------------------------------ probes
def gen(seed):
    return torch.Generator().manual_seed(seed)


def int_probe(shape, seed, lo=-4, hi=4):
    """fp32 tensor of integers in [lo, hi]."""
    return torch.randint(lo, hi + 1, tuple(shape) if not isinstance(shape, int) else (shape,), generator=gen(seed)).float()


def split_probe(shape, seed):
    """+-(1 + 2^-12) with random signs: bf16 hi = +-1, lo = +-2^-12, both exact."""
    sign = torch.randint(0, 2, tuple(shape), generator=gen(seed)).float() * 2 - 1
    return sign * (1.0 + SPLIT_LO)


def wgrad_operands(M, N, K, probe, seed=0):
    """(dy, x) of one probe: "int", "a" (x split: the hi.lo term) or "b" (dy split: the lo.hi term)."""
    if probe == "int":
        return int_probe((M, N), seed + 1), int_probe((M, K), seed + 2)
    if probe == "a":
        return int_probe((M, N), seed + 1), split_probe((M, K), seed + 2)
    if probe == "b":
        return split_probe((M, N), seed + 1), int_probe((M, K), seed + 2)
    raise ValueError(probe)


def bf16_split(v):
    """(hi, lo) of the kernels' on-the-fly split: hi = bf16(v), lo = bf16(v - hi), as fp32 tensors."""
    hi = v.to(torch.bfloat16).float()
    return hi, (v - hi).to(torch.bfloat16).float()


def layernorm_probe(rows, dim, seed=0):
    """(x, gamma, dy): rows of a balanced random permutation of +-1, integer gamma in [1, 3], integer dy in [-4, 4]."""
    g = gen(seed)
    base = torch.cat([torch.ones(dim // 2), -torch.ones(dim // 2)])
    x = torch.stack([base[torch.randperm(dim, generator=g)] for _ in range(rows)])
    gamma = torch.randint(1, 4, (dim,), generator=g).float()
    dy = torch.randint(-4, 5, (rows, dim), generator=g).float()
    return x, gamma, dy


# ------------------------------------------------------------------------------------------------------------ fp64 references
def wgrad_ref(dy, x):
    return dy.double().T @ x.double()


def col_sum_ref(dy):
    return dy.double().sum(0)


def layernorm_bwd_ref(x, gamma, dy, eps):
    """(dx, dgamma, dbeta) of nn.LayerNorm (biased variance, eps inside the square root) in fp64."""
    x, gamma, dy = x.double(), gamma.double(), dy.double()
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    xh = xc * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def l2norm_bwd_ref(f, dy, e=1e-6):
    """d f of y = f / (|f| + e):  dy / (r + e) - f (f . dy) / (r (r + e)^2), the second term zero at r = 0; also returns r."""
    f, dy = f.double(), dy.double()
    r = f.norm(dim=-1, keepdim=True)
    second = f * (f * dy).sum(-1, keepdim=True) / (r * (r + e) ** 2).clamp_min(1e-300)
    return dy / (r + e) - torch.where(r > 0, second, torch.zeros_like(second)), r
