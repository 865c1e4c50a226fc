"""kv_slot_util.py holds what test_attention_projected_gpu.py relies on: the slot layout of csrc/attention_tile.h as a bijection, an encoder
that fills whole slots, a decoder that inverts it, and the bound on what the bf16 hi / lo split loses.  No GPU."""
import pytest
import torch

import kv_slot_util as su

SHAPES = [(1, 1, 32), (2, 3, 96), (3, 4, 160)]  # (B, H, S)


def tagged(B, H, S):
    """Inputs that say where they came from and that hi + lo holds exactly: (256 key + dim) 2^-b in K, its negative in V.  key < 256 and
    dim = 0 .. 32 H - 1 < 256 make an integer below 2^16: hi keeps its upper 8 significant bits, the rest is an integer of at most 8 bits and
    exact in lo; the batch element scales by a power of two."""
    assert S <= 256 and 32 * H <= 256
    key = torch.arange(S).view(1, S, 1).expand(B, S, 32 * H)
    dim = torch.arange(32 * H).view(1, 1, 32 * H).expand(B, S, 32 * H)
    tag = (256 * key + dim).float() * torch.exp2(-torch.arange(B).float()).view(B, 1, 1)
    return tag.contiguous(), (-tag).contiguous()


@pytest.mark.parametrize("B,H,S", SHAPES)
def test_decode_inverts_encode(B, H, S):
    k, v = tagged(B, H, S)
    buf = su.encode_slots(k, v)
    assert buf.dtype == torch.uint8 and buf.shape == (B * H * (S // 32) * su.SLOT_BYTES,)
    k_hi, k_lo, v_hi, v_lo = su.decode_slots(buf, B, H, S)
    for got_hi, got_lo, src in ((k_hi, k_lo, k), (v_hi, v_lo, v)):
        hi, lo = su.split(src)
        assert torch.equal(got_hi, hi.float()) and torch.equal(got_lo, lo.float())
        assert torch.equal(got_hi + got_lo, src)  # (the tags fit into 16 significant bits: nothing is lost)
    # random values: the decoder returns the two splits bit for bit, no NaN of its prefill left
    k, v = su.rnd(B, S, 32 * H, seed=1), su.rnd(B, S, 32 * H, seed=2)
    for got, want in zip(su.decode_slots(su.encode_slots(k, v), B, H, S), su.split(k) + su.split(v)):
        assert torch.equal(got, want.float())


def test_tagged_values_sit_where_the_layout_says():
    """Straight from the sentences of attention_tile.h, one element at a time, on the raw bytes."""
    B, H, S = 2, 3, 96
    nt = S // 32
    k, v = tagged(B, H, S)
    words = su.encode_slots(k, v).view(torch.int16).view(B * H * nt, 8, 64, 8)  # (slot, piece, lane, element)
    as_float = lambda w: w.view(torch.bfloat16).float()
    for b, h, t, ks, lane, i in ((0, 0, 0, 0, 0, 0), (1, 2, 2, 1, 63, 7), (0, 1, 1, 0, 37, 5), (1, 0, 2, 1, 31, 3), (1, 1, 0, 1, 32, 4)):
        slot, r, half = (b * H + h) * nt + t, lane & 31, lane >> 5
        got_k = as_float(words[slot, su.piece(su.K, ks, su.HI), lane, i]) + as_float(words[slot, su.piece(su.K, ks, su.LO), lane, i])
        assert got_k == k[b, 32 * t + r, 32 * h + 16 * ks + 8 * half + i]
        got_v = as_float(words[slot, su.piece(su.VT, ks, su.HI), lane, i]) + as_float(words[slot, su.piece(su.VT, ks, su.LO), lane, i])
        assert got_v == v[b, 32 * t + (i & 3) + 16 * ks + 8 * (i >> 2) + 4 * half, 32 * h + r]
    assert [su.piece(w, ks, hl) for w in (su.K, su.VT) for ks in (0, 1) for hl in (su.HI, su.LO)] == list(range(8))


def test_every_key_dim_pair_once_per_piece_kind():
    for which in (su.K, su.VT):
        key, dim = su.tables()[which]
        assert key.shape == dim.shape == (2, 64, 8)
        assert int(key.min()) == 0 and int(key.max()) == 31 and int(dim.min()) == 0 and int(dim.max()) == 31
        hits = torch.bincount((key * 32 + dim).flatten(), minlength=1024)
        assert hits.shape == (1024,) and bool((hits == 1).all())
    # and through the decoder: every (b, h, key, dim) of the four outputs is written (NaN prefill), from a buffer of distinct words
    B, H, S = 2, 3, 64
    n = B * H * (S // 32) * su.SLOT_BYTES // 2
    words = (torch.arange(n) % 0x7F00).to(torch.int16)  # (below the bf16 infinities / NaNs)
    outs = su.decode_slots(words.view(torch.uint8), B, H, S)
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    # each (slot, piece) holds 512 consecutive words: the multiset of values of an output is that of its pieces
    p = words.view(B * H * (S // 32), 8, 512)
    for o, (which, hl) in zip(outs, ((su.K, su.HI), (su.K, su.LO), (su.VT, su.HI), (su.VT, su.LO))):
        want = torch.cat([p[:, su.piece(which, ks, hl)].reshape(-1) for ks in (0, 1)]).view(torch.bfloat16).float()
        assert torch.equal(o.flatten().sort().values, want.sort().values)


@pytest.mark.parametrize("B,H,S", SHAPES)
def test_encoder_fills_every_byte(B, H, S):
    """From a 0xA5 prefill, with inputs whose bf16 words contain no 0xA5 byte: all-zero inputs (words 0x0000) and all-one inputs (hi
    0x3F80, lo 0x0000)."""
    for fill in (0.0, 1.0):
        k = torch.full((B, S, 32 * H), fill)
        out = torch.full((B * H * (S // 32) * su.SLOT_BYTES + 64,), 0xA5, dtype=torch.uint8)
        ret = su.encode_slots(k, k, out=out[:-64])
        assert ret.data_ptr() == out.data_ptr()
        assert not bool((out[:-64] == 0xA5).any()) and bool((out[-64:] == 0xA5).all())


def test_split_bound():
    """|v - (hi + lo)| <= SPLIT_REL |v| = 2^-17 |v| (derivation in kv_slot_util.py), on random fp32 values over 40 binades, and the example
    that shows 2^-18 is too small."""
    g = torch.Generator().manual_seed(7)
    v = torch.randn(1 << 20, generator=g) * torch.exp2(torch.randint(-20, 20, (1 << 20,), generator=g).float())
    hi, lo = su.split(v)
    assert hi.dtype == lo.dtype == torch.bfloat16
    assert torch.equal(hi, v.to(torch.bfloat16))
    ratio = ((v.double() - (hi.double() + lo.double())).abs() / v.double().abs()).max().item()
    print(f"split: largest |v - (hi + lo)| / |v| = {ratio:.4e} = 2^-17 x {ratio * 2**17:.4f}")
    assert 2.0 ** -18 < ratio <= su.SPLIT_REL == 2.0 ** -17
    e = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -17])
    hi, lo = su.split(e)
    assert hi.item() == 1.0 and lo.item() == 2.0 ** -8 and abs(e.double().item() - 1.0 - 2.0 ** -8) == 2.0 ** -17


def test_inputs():
    t = su.inputs(96, 136, 128, 8)
    assert t is su.inputs(96, 136, 128, 8)
    assert t["x"].shape == (96, 136) and t["w"].shape == (128 + 512, 136) and t["x"].dtype == t["w"].dtype == torch.float32
    assert t["q64"].shape == (96, 128) and t["k64"].shape == t["v64"].shape == (96, 256) and t["k64"].dtype == torch.float64
    assert (t["v64"] - t["x"].double() @ t["w"][384:].double().T).abs().max().item() < 1e-12
    assert abs(t["x"].std().item() - 1.0) < 0.05 and abs(t["w"].std().item() * 136 ** 0.5 - 1.0) < 0.05
    assert su.inputs(96, 136, 0, 8)["q64"].shape == (96, 0)
