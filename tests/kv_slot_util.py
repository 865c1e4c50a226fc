"""The K / V operand slots of the head-dim-32 split-bf16 attention kernel, stated in plain torch on the CPU (test_kv_slot_util_cpu.py,
test_attention_projected_gpu.py).  Written from the layout comments of csrc/attention_tile.h, as index tables and not as a copy of a device
writer; nothing here touches the GPU or the package.

    slot index ((b H + h) nt + t), SLOT_BYTES each, nt = S / 32 tiles of 32 keys
    slot = 8 pieces of 64 lanes x 8 bf16; piece = which * 4 + ks * 2 + hl   (which: K = 0, V^T = 1; ks: k-step 0, 1; hl: hi = 0, lo = 1)
    K piece:   element i of lane (r = lane & 31, half = lane >> 5) = key 32 t + r,  dim 16 ks + 8 half + i  of head h
    V^T piece: element i of lane (r, half)                         = dim r,  key 32 t + (i & 3) + 16 ks + 8 (i >> 2) + 4 half

Split: hi = bf16(v), lo = bf16(v - hi), both round-to-nearest-even.  SPLIT_REL bounds what the pair loses:
    v in [2^e, 2^(e+1)): bf16 keeps 8 significant bits, so |v - hi| <= 2^(e-8) (half a unit in the last place).  The remainder r = v - hi is
    exact in fp32.  |r| = 2^(e-8) is a power of two and survives the second cast unchanged; otherwise |r| < 2^(e-8) lies in a binade
    [2^f, 2^(f+1)) with f <= e - 9 and its cast loses at most 2^(f-8) <= 2^(e-17):   |v - (hi + lo)| <= 2^-17 |v|.
(2^-18 does not hold: v = 1 + 2^-8 - 2^-17 has hi = 1 and r = 2^-8 - 2^-17, nine significant bits and a tie of the second cast, so it
loses 2^-17; random N(0, 1) values come close to 2^-17 as well -- test_kv_slot_util_cpu.py checks the example and prints the largest ratio.)"""
import functools

import torch

SLOT_BYTES = 8192
K, VT, HI, LO = 0, 1, 0, 1
SPLIT_REL = 2.0 ** -17


def piece(which, ks, hl):
    return which * 4 + ks * 2 + hl


@functools.lru_cache(maxsize=None)
def tables():
    """{K, VT} -> (key, dim): int64 tensors (2 k-steps, 64 lanes, 8 elements) with the key inside the 32-key tile and the dim inside the head
    that each element of a piece holds."""
    ks, lane, i = torch.meshgrid(torch.arange(2), torch.arange(64), torch.arange(8), indexing="ij")
    r, half = lane & 31, lane >> 5
    return {K: (r, 16 * ks + 8 * half + i), VT: ((i & 3) + 16 * ks + 8 * (i >> 2) + 4 * half, r)}


def split(v):
    """fp32 -> (hi, lo) as torch.bfloat16 (torch's cast rounds to nearest even)."""
    v = v.float()
    hi = v.to(torch.bfloat16)
    return hi, (v - hi.float()).to(torch.bfloat16)


def _pieces(buf, B, H, S):
    """The byte buffer as int16 (B, H, nt, which, ks, hl, lane, element): the piece index written out as its three digits."""
    assert S % 32 == 0 and buf.dtype == torch.uint8 and buf.is_contiguous() and buf.numel() == B * H * (S // 32) * SLOT_BYTES
    return buf.view(torch.int16).view(B, H, S // 32, 2, 2, 2, 64, 8)


def _tiles(t, H):
    """(B, S, 32 H) -> (B, nt, 32 keys, H, 32 dims), a view."""
    B, S, C = t.shape
    assert C == 32 * H and S % 32 == 0
    return t.view(B, S // 32, 32, H, 32)


def encode_slots(k, v, out=None):
    """k, v (B, S, 32 H) fp32 -> uint8 (B H (S / 32) SLOT_BYTES,), written piece by piece into `out` when given (a prefilled buffer shows
    what the eight pieces leave untouched)."""
    B, S, C = k.shape
    H = C // 32
    assert v.shape == k.shape
    if out is None:
        out = torch.zeros(B * H * (S // 32) * SLOT_BYTES, dtype=torch.uint8)
    p = _pieces(out, B, H, S)
    for which, src in ((K, k), (VT, v)):
        key, dim = tables()[which]
        el = _tiles(src.float().contiguous(), H)[:, :, key, :, dim]  # (ks, lane, i, B, nt, H): the indexed axes come first
        for hl, part in zip((HI, LO), split(el.permute(3, 5, 4, 0, 1, 2))):  # (B, H, nt, ks, lane, i)
            for ks in range(2):
                p[:, :, :, which, ks, hl] = part[:, :, :, ks].contiguous().view(torch.int16)
    return out


def decode_slots(buf, B, H, S):
    """-> k_hi, k_lo, v_hi, v_lo, each (B, S, 32 H) fp32: the values the bf16 elements hold, every one put where the tables say."""
    p = _pieces(buf.contiguous(), B, H, S)
    res = []
    for which in (K, VT):
        key, dim = tables()[which]
        for hl in (HI, LO):
            vals = p[:, :, :, which, :, hl].contiguous().view(torch.bfloat16).float()  # (B, H, nt, ks, lane, i)
            t = torch.full((B, S, 32 * H), float("nan"))
            _tiles(t, H)[:, :, key, :, dim] = vals.permute(3, 4, 5, 0, 2, 1)  # (ks, lane, i, B, nt, H)
            res.append(t)
    return tuple(res)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def inputs(M, K_, n_q, heads, seed=0):
    """x (M, K) ~ N(0, 1), stacked weights [Wq; Wk; Wv] (n_q + 64 heads, K) ~ N(0, 1 / K) -- the scaling of linear_family_worker.inputs, so
    its BARS apply -- and the float64 products of the same fp32 values per role.  Made once per shape, shared, never written to."""
    inner = 32 * heads
    x, w = rnd(M, K_, seed=seed + 1), rnd(n_q + 2 * inner, K_, seed=seed + 2, scale=K_ ** -0.5)
    y64 = x.double() @ w.double().T
    return {"x": x, "w": w, "q64": y64[:, :n_q], "k64": y64[:, n_q:n_q + inner], "v64": y64[:, n_q + inner:]}
