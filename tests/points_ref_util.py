"""fp64 reference of one NeRF MLP's pointwise forward / backward with GIVEN ReLU gates, and the readers of what the fused pointwise kernels
(csrc/nerf_points_bf16.hip) leave between their passes (imported by name, like nerf_kernel_util).  Plain torch on the CPU, built from the
state-dict weights (`nerf_fine.state_dict()`: keys without the network prefix), never from a packed blob.  No fixture, no hook, no test;
nothing here touches a GPU unless it is handed GPU tensors.

Given the gates the backward pass is a linear map g4 -> (g_xi0, g_xi5, g_xd): with the gates a GPU route used itself, the fp64 result is the
exact answer for every row and column -- no sub-gradient ambiguity of a ReLU whose pre-activation is within rounding of zero is left."""
from types import SimpleNamespace

import torch

IPE, DIRS, TILE = 90, 27, 128  # xi columns that carry the encoding, xd columns of the direction encoding, samples per workgroup tile
# per-row bars of the shared-gate backward, of the tensor's largest reference entry, required of EVERY row (tests/test_points_shared_gates_gpu.py)
SPLIT_BAR = 2e-4  # the fused pair and the bf16x3 GEMM chain: the per-row bar test_tapped_points_kernels_vs_gemm_chain asks of 99.5 % of rows
FP32_BAR = 2e-5  # the fp32 GEMM chain: ten chained products at the 2e-6 single-GEMM bar of test_linear_wgrad_and_col_sum


def fine_state_dict(sd, net="nerf_fine"):
    """the entries of one network of a renderer's state dict, prefix stripped"""
    return {k[len(net) + 1:]: v for k, v in sd.items() if k.startswith(net + ".")}


def _p(sd, name):
    return sd[name].detach().to("cpu", torch.float64)


def _d(x):
    return x.detach().to("cpu", torch.float64)


def views_width(sd_fine):
    """27 direction columns + 16 appearance columns when the network has an appearance embedding"""
    return sd_fine["views_linears.0.weight"].shape[1] - 256


def pts_layer64(sd_fine, l, xi, h_prev):
    """post-ReLU activations of pts layer l from the previous layer's (layer 5 reads cat(xi[:, :90], h[4]); layer 0 reads xi[:, :90])"""
    x = _d(xi)[:, :IPE] if l == 0 else (torch.cat([_d(xi)[:, :IPE], _d(h_prev)], 1) if l == 5 else _d(h_prev))
    return torch.relu(x @ _p(sd_fine, f"pts_linears.{l}.weight").T + _p(sd_fine, f"pts_linears.{l}.bias"))


def heads64(sd_fine, h7, xd):
    """(views pre-activation u (n,128), hv = relu(u), rgb logits (n,3), raw sigma (n,1)) from layer 7's activations and the xd rows"""
    h7 = _d(h7)
    feat = h7 @ _p(sd_fine, "feature_linear.weight").T + _p(sd_fine, "feature_linear.bias")
    u = torch.cat([feat, _d(xd)[:, : views_width(sd_fine)]], 1) @ _p(sd_fine, "views_linears.0.weight").T + _p(sd_fine, "views_linears.0.bias")
    hv = torch.relu(u)
    logit = hv @ _p(sd_fine, "rgb_linear.weight").T + _p(sd_fine, "rgb_linear.bias")
    sigma = h7 @ _p(sd_fine, "alpha_linear.weight").T + _p(sd_fine, "alpha_linear.bias")
    return u, hv, logit, sigma


def field_forward64(sd_fine, xi, xd):
    """xi (n, >= 90), xd (n, >= 27 [+ 16]) -> h[0..7] (post-ReLU), the views layer's pre-activation u, hv = relu(u), rgb logits (n,3), raw
    sigma (n,1); every column past the encodings is ignored (the padding of the GEMM operands)."""
    h = []
    for l in range(8):
        h.append(pts_layer64(sd_fine, l, xi, h[-1] if h else None))
    u, hv, logit, sigma = heads64(sd_fine, h[7], xd)
    return SimpleNamespace(h=h, u=u, hv=hv, logit=logit, sigma=sigma)


def split_matmul(a, b):
    """a @ b in the split arithmetic's own terms: both operands rounded to bf16 hi + bf16 lo, hi.hi + hi.lo + lo.hi summed in fp64 (the
    lo.lo product and every rounding of an fp32 accumulator left out): the CPU model the bars of the split routes are judged against"""
    def parts(x):
        hi = x.float().bfloat16().double()
        return hi, (x - hi).float().bfloat16().double()
    (ah, al), (bh, bl) = parts(a), parts(b)
    return ah @ bh + ah @ bl + al @ bh


def field_backward64(sd_fine, g4, gates, gates_v, tap=None, mm=torch.matmul):
    """g4 (n,4) = d loss / d (rgb logits, raw sigma), gates[0..7] (n,256) and gates_v (n,128) 0/1 (or bool) -> g_xi0 (n,90), g_xi5 (n,90),
    g_xd (n, 27 [+ 16]): g_xi0 = g_0 @ W0 is the path through all eight layers, g_xi5 = g_5 @ W5[:, :90] the skip connection's.
    tap = (layer, g_h (n,256)) adds g_h to d loss / d h[layer] BEFORE that layer's gate is applied (layer 7: together with the density
    head's share).  mm: the matrix product (split_matmul for the arithmetic model)."""
    g4 = _d(g4)
    gate = [_d(g).double() for g in gates]
    tl, g_h = (tap[0], _d(tap[1])) if tap is not None else (-1, None)
    g_hv = mm(g4[:, :3], _p(sd_fine, "rgb_linear.weight")) * _d(gates_v).double()
    g_vin = mm(g_hv, _p(sd_fine, "views_linears.0.weight"))
    g_xd = g_vin[:, 256:]
    g = mm(g_vin[:, :256], _p(sd_fine, "feature_linear.weight")) + g4[:, 3:4] * _p(sd_fine, "alpha_linear.weight")
    if tl == 7:
        g = g + g_h
    g = g * gate[7]
    g_xi5 = None
    for l in range(7, 0, -1):
        gin = mm(g, _p(sd_fine, f"pts_linears.{l}.weight"))
        if l == 5:
            g_xi5, gin = gin[:, :IPE], gin[:, IPE:]
        if tl == l - 1:
            gin = gin + g_h
        g = gin * gate[l - 1]
    g_xi0 = mm(g, _p(sd_fine, "pts_linears.0.weight"))
    return g_xi0, g_xi5, g_xd


def decode_views_gates(gates_bytes, n):
    """Row 8 of the gate table (the views layer's 128 ReLU gates per sample) -> (n, 128) bool.

    Derivation, from csrc/nerf_points_bf16.hip (points_fwd_body): the table is u32x4 [ntiles][9][256], i.e. int32 [tiles][9][256][4]; a
    thread writes `cx.gptr[8 * 256]` with `cx.gptr = gates + bid * 9 * 256 + tid`, so cell [tile][8][tid].  Its sample is
    `bid * TILE + wave * 32 + s` with wave = tid >> 6, s = tid & 31, and hh = (tid & 63) >> 5 is the half-wavefront: thread
    tid = 64 wave + 32 hh + s holds sample 128 tile + 32 wave + s, two threads per sample.  In the loop over (ob, q, e) the value read is
    register 4 q + e of output block ob, whose bias is `bv[ob * 32 + 8 * q + e]` with bv offset by 4 hh: views unit 32 ob + 8 q + 4 hh + e.
    Its bit is `min(bits(hv), 1) << (16 * (ob & 1) + 4 * q + e)`, OR-ed into gv0 for ob < 2 and gv1 otherwise, stored as
    u32x4{gv0, gv1, 0, 0}: bit 16 (ob & 1) + 4 q + e of word ob >> 1.  Words 2 and 3 are zero (asserted here).  The backward kernel reads
    the same cell and the same bit (points_bwd_body: `gv[ob >> 1]`, bit 16 (ob & 1) + 4 q + e, for hv[ob * 16 + 4 q + e])."""
    ntiles = (n + TILE - 1) // TILE
    tab = gates_bytes.detach().cpu().contiguous().view(torch.int32).reshape(ntiles, 9, 256, 4)[:, 8].to(torch.int64) & 0xFFFFFFFF
    assert not tab[..., 2:].any(), "words 2 and 3 of the views row are not zero"
    tab = tab.reshape(ntiles, 4, 2, 32, 4).permute(0, 1, 3, 2, 4).reshape(ntiles * TILE, 2, 4)  # [sample][hh][word]
    out = torch.zeros(ntiles * TILE, 128, dtype=torch.bool)
    for hh in range(2):
        for ob in range(4):
            for q in range(4):
                for e in range(4):
                    out[:, 32 * ob + 8 * q + 4 * hh + e] = ((tab[:, hh, ob >> 1] >> (16 * (ob & 1) + 4 * q + e)) & 1).bool()
    return out[:n]


def tapped_gates(fused, rays, z, Sa, app_row):
    """Eight launches of nm_nerf_points_fwd_rays_bf16x3 (inerf.FusedField.forward_rays), tap = 0 .. 7: the same out4 and the same gate bytes
    from every one of them, and the tapped activations feats[l] (n, 256) of every pts layer; gates[l] = feats[l] > 0.

    Why feats[l] > 0 IS the gate bit the backward kernel reads: the tap dump (dump_tap_rows) stores max(acc + b, 0) from the raw
    accumulators in cx.hv and the bias row of layer l; the K-loop's re-packing (nerf_split_chain.h, UnitWork::act) forms the same
    max(cx.hv + b, 0) from the same registers and bias row (unit u: registers 8 (u & 1) .. + 7 of block u >> 1 = the columns dump_tap_rows
    assigns them), rounds it to its bf16 hi half and sets the bit where that half is non-zero (UnitWork::gates, gate_byte).  bf16 has
    fp32's exponent range and nothing is negative after the ReLU, so the hi half of a positive value is non-zero: one fp32 expression
    computed twice, not one value stored twice -- equal for every normal float."""
    runs = [fused.forward_rays(rays, z, Sa, app_row, tap) for tap in range(8)]
    out4, gates = runs[0][0], runs[0][1]
    for tap, (o, g, f) in enumerate(runs):
        assert torch.equal(o, out4) and torch.equal(g, gates), f"tap {tap} changes out4 or the gate bytes"
        assert f.shape == (out4.shape[0], 256)
    feats = [f for _, _, f in runs]
    return out4, gates, feats, [(f > 0).cpu() for f in feats]


def row_errors(got, want):
    """per-row maximum |got - want| in units of the reference TENSOR's largest entry (every row; want in fp64)"""
    want = _d(want)
    return (_d(got) - want).abs().max(1).values / want.abs().max().item()


# ----------------------------------------------------------------------------------------------- inputs without a GPU
def cpu_bundle(R, seed, S=128):
    """nerf_kernel_util.points_bundle's rays and fence posts, kept on the CPU"""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(R, 3, generator=g) * 0.2
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    rays = torch.cat([o, d, torch.full((R, 1), 0.01), torch.ones(R, 1), d, torch.full((R, 1), 0.002)], -1)
    z = torch.sort(torch.rand(R, S + 1, generator=g) * 0.9 + 0.05, dim=-1).values
    return rays, z, g


def oracle_rows(rays, z, Sa, app_row=None):
    """xi (n, 90), xd (n, 27 [+ 16]) of the first Sa intervals of every ray from the oracle's encoders, in fp64 (what nm_inerf_encode writes)"""
    from oracle import nerf_oracle as no

    rays, z = rays.double(), z.double()
    R = rays.shape[0]
    mean, var = no.frustum_gaussians(z[:, : Sa + 1], rays[:, :3], rays[:, 3:6], rays[:, 11:12])
    xi = no.ipe(mean.reshape(-1, 3), var.reshape(-1, 3), 15)
    xd = no.dir_pe(rays[:, 8:11], 4).repeat_interleave(Sa, 0)
    if app_row is not None:
        xd = torch.cat([xd, app_row.double()[None].expand(R * Sa, 16)], 1)
    return xi, xd
