"""The third door into the head-dim-32 attention kernel, the one MultiHeadAttention.forward takes at inference: nm_linear_qkv_bf16x3 writes
the keys and values from the projection GEMM's accumulators into the kernel's operand slots, already split into bf16 hi / lo, and
nm_attention_presplit reads them (ops.attention_projected).  On every form the GEMM can take -- the one-launch small-grid form at K = 256 and
K = 128, the ring kernels with the K % 16 == 8 tail, the separate small-grid launches of the q|key and the value chunks -- at 1, 2, 3 and 5 key
tiles, 1, 2 and 3 head chunks, M no multiple of 128, and n_q != 32 heads.

The slots are decoded by tests/kv_slot_util.py (the layout of csrc/attention_tile.h in plain torch) and held against
  * the plain GEMM's output (ops.linear, pinned to float64 by test_linear_family_gpu.py) split and encoded on the CPU: byte for byte;
  * the slots kv_presplit_kernel writes from that output (the other device writer): byte for byte;
  * the float64 projections: linear_family_worker.BARS["bf16x3"] + kv_slot_util.SPLIT_REL max|v|.
The attention output is held against attention_util.reference in float64 on the kernel's actual operands (q_out and the decoded hi + lo), at the
2e-5 of test_attention_routes_gpu.py::test_forward_against_float64."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import types
from pathlib import Path

import pytest
import torch

import attention_projected_worker as pw
import attention_util as au
import kv_slot_util as su
from attention_projected_worker import Case
from linear_family_worker import BARS
from nerfmatch_amd import _lib, ops
from nerfmatch_amd._lib import dptr

pytestmark = pytest.mark.gpu
WORKER = Path(pw.__file__).resolve()
SCALE = 32 ** -0.5
ATT_BAR = 2e-5

# (case, the forms its launches take).  B in {1, 3, 5}, S in {32, 64, 96, 160} (1, 2, 3, 5 tiles against the 4-slot ring), heads in {4, 8, 12},
# cross L in {65, 97, 129}; K = 256 / 128: one small-grid launch with 16 / 8 K-steps; K = 264 / 136: ring kernels, zero-filled half K-step.
# M = B S is a multiple of 128 nowhere: every launch has a last row tile with idle wavefronts, most have a batch boundary inside a tile.
SMALL_CASES = [
    (Case(1, 32, 4, 256, "self", 32), ("small<3>",)),      # one wavefront of keys, three idle
    (Case(3, 96, 8, 128, "self", 96), ("small<3>",)),
    (Case(5, 96, 4, 256, "self", 96), ("small<3>",)),
    (Case(5, 160, 12, 136, "self", 160), ("ring<1>", "ring<2>")),
    (Case(3, 64, 12, 264, "self", 64), ("ring<1>", "ring<2>")),
    (Case(1, 160, 8, 264, "self", 160), ("ring<1>", "ring<2>")),
    (Case(3, 32, 8, 128, "cross", 65), ("small<3>",)),
    (Case(1, 96, 12, 256, "cross", 129), ("small<3>",)),
    (Case(5, 32, 12, 128, "cross", 129), ("small<3>",)),
    (Case(5, 64, 4, 136, "cross", 97), ("ring<1>", "ring<2>")),
    (Case(3, 160, 8, 264, "cross", 65), ("ring<1>", "ring<2>")),
    (Case(3, 96, 8, 256, "self", 96, n_q=128), ("small<3>",)),   # n_q != 32 heads: q_out's row stride is n_q (GEMM outputs only)
    (Case(3, 96, 8, 136, "self", 96, n_q=128), ("ring<1>", "ring<2>")),
]


@functools.lru_cache(maxsize=None)
def big_cases():
    """Sized from the CU count so that the one-launch form (4 or 6 column chunks) exceeds 2 x CU count workgroups and a launch of 2 chunks does
    not: row tiles come in groups of 8, 2 CUs // 32 + 1 groups do it, and B batch elements of 864 keys (27 tiles) are the fewest rows that
    reach the last of these groups.  256 CUs: B = 19, M = 16416, 129 row tiles in 17 groups -- 544 and 816 workgroups against 512, 272 for 2
    chunks.  Cross, K = 128: the key and the value chunks as one small-grid launch each.  Self, K = 256: q|key are 4 chunks, the ring kernel,
    the values the small-grid form.  The attention checks look at batch element 0 (the float64 reference of all would be ~1 GB)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = 2 * cus // 32 + 1
    B = (groups - 1) * 8 * 128 // 864 + 1
    assert (groups - 1) * 8 < -(-B * 864 // 128) <= groups * 8
    assert groups * 8 * 4 > 2 * cus >= groups * 8 * 2
    return [(Case(B, 864, 8, 128, "cross", 65, B_att=1), ("small<1>", "small<2>")), (Case(B, 864, 8, 256, "self", 864, B_att=1), ("ring<1>", "small<2>"))]


ALL_IDS = [c.id for c, _ in SMALL_CASES] + ["big-cross-K128", "big-self-K256"]
ATT_IDS = [c.id for c, _ in SMALL_CASES if c.n_q < 0] + ["big-cross-K128", "big-self-K256"]


def lookup(case_id):
    if case_id.startswith("big"):
        return big_cases()[case_id == "big-self-K256"]
    return next(cf for cf in SMALL_CASES if cf[0].id == case_id)


class precisions:
    """bf16x3 linear and attention arithmetic inside the block (run() is cached across tests, so it cannot lean on monkeypatch)."""

    def __enter__(self):
        self.keep = ops.LINEAR_PRECISION, ops.ATTENTION_PRECISION
        ops.LINEAR_PRECISION = ops.ATTENTION_PRECISION = "bf16x3"

    def __exit__(self, *exc):
        ops.LINEAR_PRECISION, ops.ATTENTION_PRECISION = self.keep


def bits(t):
    return t.contiguous().view(torch.int32)


def col_ptr(t, col):
    return C.c_void_p(t.data_ptr() + 4 * col)


@functools.lru_cache(maxsize=None)
def run(case_id):
    """One case through nm_linear_qkv_bf16x3 and through the plain GEMM; computed once, shared by the tests below, never written to."""
    c, want_forms = lookup(case_id)
    dev = torch.device("cuda:0")
    t = pw.inputs(c)
    inner = 32 * c.heads
    rc, slots, q_out = pw.project(dev, t["x"], t["w"], c)
    with precisions():
        y = ops.linear(t["x"].to(dev), t["w"].to(dev))  # (M, n_q + 64 heads): q | k | v
    yk, yv = (y[:, c.nq + i * inner:c.nq + (i + 1) * inner].cpu().reshape(c.B, c.S, inner) for i in (0, 1))
    return types.SimpleNamespace(c=c, forms=want_forms, t=t, inner=inner, rc=rc, slots=slots, q_out=q_out, y=y, expected=su.encode_slots(yk, yv),
                                 need=slots.numel() - su.SLOT_BYTES)


def presplit(r, q, ldq, B, L):
    """nm_attention_presplit over r's slots into a NaN-prefilled output; q: a device pointer."""
    out = torch.full((B * L, r.inner), float("nan"), device=r.slots.device)
    rc = _lib.lib().nm_attention_presplit(q, ldq, dptr(r.slots, torch.uint8), B, L, r.c.S, r.c.heads, SCALE, dptr(out), _lib.stream())
    assert rc == 0, rc
    return out


# ------------------------------------------------------------------------------------------------------------ the GEMM's outputs
@pytest.mark.parametrize("case_id", ALL_IDS)
def test_gemm_outputs_exact(gpu, built_lib, case_id):
    """Checks 1, 3, 4.  The slot buffer equals, byte for byte, kv_slot_util.encode_slots of the plain GEMM's key and value columns -- the key
    pieces, and the value pieces too although their product runs with the MFMA operands swapped (measured on the MI355X: identical on every
    form) -- and the buffer kv_presplit_kernel writes from those columns.  So no byte inside keeps the 0xA5 prefill; the slot behind the buffer
    still holds it.  q_out[:M] has the bits of the plain GEMM's first n_q columns, the four rows behind M are still NaN."""
    r = run(case_id)
    c = r.c
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert pw.forms(c.M, c.K, c.nq, c.heads, cus) == r.forms, "the shape no longer reaches the kernel form it was chosen for"
    assert r.rc == 0
    got = r.slots.cpu()
    g8, e8 = got[:r.need].view(-1, 8, 1024), r.expected.view(-1, 8, 1024)
    assert torch.equal(g8[:, :4], e8[:, :4]), f"key pieces: {int((g8[:, :4] != e8[:, :4]).sum())} bytes differ from the encoded plain GEMM output"
    assert torch.equal(g8[:, 4:], e8[:, 4:]), f"value pieces: {int((g8[:, 4:] != e8[:, 4:]).sum())} bytes differ from the encoded plain GEMM output"
    assert bool((got[r.need:] == 0xA5).all()), "the slot behind the buffer was written"
    # the other device writer: nm_attention's kv_presplit_kernel on the fp32 columns (65 zero queries: the tiled kernel whatever S is)
    N = r.y.shape[1]
    ws2 = torch.full_like(r.slots, 0xA5)
    qd, od = torch.zeros(c.B * 65, r.inner, device=gpu), torch.empty(c.B * 65, r.inner, device=gpu)
    rc = _lib.lib().nm_attention(dptr(qd), col_ptr(r.y, c.nq), col_ptr(r.y, c.nq + r.inner), r.inner, N, N, c.B, 65, c.S, c.heads, 32, SCALE,
                                 _lib.NM_ATTN_BF16X3, dptr(ws2, torch.uint8), dptr(od), None, _lib.stream())
    assert rc == 0
    assert torch.equal(ws2, r.slots), f"{int((ws2 != r.slots).sum())} bytes differ from kv_presplit_kernel's slots"
    if c.nq:
        assert r.q_out.shape == (c.M + 4, c.nq)
        assert torch.equal(bits(r.q_out[:c.M]), bits(r.y[:, :c.nq])), "q rows"
        assert bool(torch.isnan(r.q_out[c.M:]).all()), "rows behind M were written"


@pytest.mark.parametrize("case_id", ALL_IDS)
def test_slots_against_float64(gpu, built_lib, case_id):
    """Check 2: hi + lo of the decoded slots against the float64 projections of the same fp32 inputs -- every (batch, key, head, dim) in its
    place.  Bar: BARS["bf16x3"] (5e-5, the project's bar for this GEMM at this input scaling) + SPLIT_REL max|v| (what hi + lo loses).
    q_out against its float64 projection at the GEMM's bar alone.
    Measured on the MI355X: keys and values <= 3.9e-5 on the small cases, <= 4.1e-5 on the two 16416-row ones (bars 7.7e-5 .. 9.5e-5, max|v| up
    to 5.9); q_out <= 3.1e-5."""
    r = run(case_id)
    c = r.c
    k_hi, k_lo, v_hi, v_lo = su.decode_slots(r.slots[:r.need].cpu(), c.B, c.heads, c.S)
    for name, hi, lo, ref in (("keys", k_hi, k_lo, r.t["k64"]), ("values", v_hi, v_lo, r.t["v64"])):
        err = ((hi.double() + lo.double()).reshape(c.M, r.inner) - ref).abs().max().item()
        bar = BARS["bf16x3"] + su.SPLIT_REL * ref.abs().max().item()
        print(f"{case_id} {name}: max |hi + lo - fp64| = {err:.3e} (bar {bar:.3e})")
        assert err <= bar, name
    if c.nq:
        err = (r.q_out[:c.M].cpu().double() - r.t["q64"]).abs().max().item()
        print(f"{case_id} q: max |q_out - fp64| = {err:.3e} (bar {BARS['bf16x3']:g})")
        assert err <= BARS["bf16x3"]


# ------------------------------------------------------------------------------------------------------------ attention over the slots
@pytest.mark.parametrize("case_id", ATT_IDS)
def test_attention_over_projected_slots(gpu, built_lib, case_id):
    """Checks 5 and 6.  nm_attention_presplit over the slots above, against attention_util.reference in float64 on the operands the kernel
    actually reads (q_out -- in cross mode the plain GEMM's projection of the queries -- and the decoded hi + lo): 2e-5, the bar
    test_forward_against_float64 holds for this kernel.  The same bits with the queries inside a wider NaN-filled buffer (ldq = 32 heads
    + 36), the bits of ops.attention_fused on the unfused buffers wherever that door reaches the same kernel (not the <= 64-token windows),
    and the bits ops.attention_projected returns wherever ops.projected_attention_supported lets the module take it.
    Measured on the MI355X: <= 1.6e-5 (cross, 32 keys, 129 queries, 12 heads: few keys, outputs of magnitude ~1); 2.5e-6 and 5.9e-6 at 864 keys."""
    r = run(case_id)
    c = r.c
    B, L, S, inner = c.B_att or c.B, c.L, c.S, r.inner
    with precisions():
        if c.mode == "self":
            q = r.q_out  # (row stride n_q = 32 heads)
        else:
            xq, wq = su.rnd(c.B * L, c.K, seed=11).to(gpu), su.rnd(inner, c.K, seed=12, scale=c.K ** -0.5).to(gpu)
            q = ops.linear(xq, wq)
        out = presplit(r, dptr(q), inner, B, L)
        assert bool(torch.isfinite(out).all())
        wide = torch.full((B * L, inner + 36), float("nan"), device=gpu)
        wide[:, 4:4 + inner] = q[:B * L]
        assert torch.equal(bits(presplit(r, col_ptr(wide, 4), inner + 36, B, L)), bits(out)), "ldq = 32 heads + 36"

        k_hi, k_lo, v_hi, v_lo = (t[:B].double() for t in su.decode_slots(r.slots[:r.need].cpu(), c.B, c.heads, S))
        q64 = q[:B * L].cpu().double().reshape(B, L, inner)
        ref = au.reference(q64, k_hi + k_lo, v_hi + v_lo, torch.zeros_like(q64), c.heads, SCALE)[0]
        err = (out.cpu().double().reshape(B, L, inner) - ref).abs().max().item()
        print(f"{case_id} attention: max |out - fp64 on the kernel's operands| = {err:.3e} (bar {ATT_BAR:g})")
        assert err <= ATT_BAR

        if not (L <= 64 and S <= 64):
            if c.mode == "self":
                fused = ops.attention_fused(r.y, (0, inner), (inner, 2 * inner), (2 * inner, 3 * inner), c.B, L, S, c.heads, SCALE)
            else:
                fused = ops.attention_fused(q, (0, inner), (0, inner), (inner, 2 * inner), c.B, L, S, c.heads, SCALE, kv=r.y)
            assert torch.equal(bits(fused[:B].reshape(B * L, inner)), bits(out)), "ops.attention_fused on the unfused buffers"
        assert ops.projected_attention_supported(c.K, c.heads, 32, L, S) == (not (L <= 64 and S <= 64))
        if ops.projected_attention_supported(c.K, c.heads, 32, L, S):
            x, w = r.t["x"].to(gpu), r.t["w"].to(gpu)
            got = ops.attention_projected(x, None, None, w, c.B, L, S, c.heads, SCALE) if c.mode == "self" else \
                ops.attention_projected(xq, wq, x, w, c.B, L, S, c.heads, SCALE)
            assert got.shape == (c.B, L, inner)
            assert torch.equal(bits(got[:B].reshape(B * L, inner)), bits(out)), "ops.attention_projected"


# ------------------------------------------------------------------------------------------------------------ the A/B arm
def test_ring_kernels_in_the_small_grid_forms_place(gpu, built_lib):
    """NM_GEMM_SMALL=0 is read once per process: ONE fresh child runs the K = 128 and K = 256 small cases with the ring kernels <1> and <2> in
    the place of the one-launch small-grid form; slot bytes and q_out bits equal this process's.  The products and their order are the same on
    every form, so the bits cannot show that the arm was taken: the child reports the NM_GEMM_SMALL it ran under, and that is all this
    test can show of it."""
    res = subprocess.run([sys.executable, str(WORKER)], env=dict(os.environ, NM_GEMM_SMALL="0"), capture_output=True, text=True,
                         timeout=180)  # (interpreter + torch + HIP start-up and 4 small launches: seconds)
    assert res.returncode == 0, res.stderr[-2000:]
    rep = json.loads(res.stdout.strip().splitlines()[-1])
    assert rep["NM_GEMM_SMALL"] == "0" and os.environ.get("NM_GEMM_SMALL") != "0"
    assert set(rep["cases"]) == {c.id for c in pw.AB_CASES}
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    for c in pw.AB_CASES:
        assert pw.forms(c.M, c.K, c.nq, c.heads, cus) == ("small<3>",)
        r = run(c.id)
        mine = pw.digests(r.slots, r.q_out)
        assert rep["cases"][c.id] == dict(mine, rc=0), c.id


# ------------------------------------------------------------------------------------------------------------ refusals and gating
REFUSED = {"K=132": dict(K=132), "n_q=64": dict(n_q=64), "heads=3": dict(heads=3), "S=40": dict(S=40, M=120), "M=S+32": dict(M=96 + 32)}


@pytest.mark.parametrize("what", REFUSED)
def test_refusals_leave_the_buffers_alone(gpu, built_lib, what):
    """K % 8, n_q % 128, 32 heads % 128, S % 32, M % S: NM_ERR_UNSUPPORTED before anything is launched -- prefills intact."""
    c = Case(3, 96, 8, 256, "self", 96)
    t = pw.inputs(c)
    rc, slots, q_out = pw.project(gpu, t["x"], t["w"], c, **REFUSED[what])
    assert rc == _lib.NM_ERR_UNSUPPORTED
    assert bool((slots == 0xA5).all()) and bool(torch.isnan(q_out).all())


def test_projected_attention_supported_agrees_with_the_refusals(gpu, built_lib, monkeypatch):
    """(K, heads, head_dim, L, S) as the module asks: n_q = 32 heads there and M = B S, so n_q = 64 reads heads = 2 and M % S cannot occur."""
    monkeypatch.setattr(ops, "LINEAR_PRECISION", "bf16x3")
    monkeypatch.setattr(ops, "ATTENTION_PRECISION", "bf16x3")
    assert ops.projected_attention_supported(256, 8, 32, 96, 96) and ops.projected_attention_supported(136, 12, 32, 65, 32)
    for K, heads, L, S in ((132, 8, 96, 96), (256, 2, 96, 96), (256, 3, 96, 96), (256, 8, 96, 40), (256, 8, 64, 64), (256, 8, 32, 64)):
        assert not ops.projected_attention_supported(K, heads, 32, L, S), (K, heads, L, S)
    assert not ops.projected_attention_supported(256, 8, 16, 96, 96)
    monkeypatch.setattr(ops, "LINEAR_PRECISION", "fp32")
    assert not ops.projected_attention_supported(256, 8, 32, 96, 96)


@pytest.mark.parametrize("mode", ["self", "cross"])
def test_module_takes_the_door_when_supported_and_falls_back_otherwise(gpu, built_lib, monkeypatch, mode):
    """MultiHeadAttention(128, head_num=4, head_dim=32) at inference: one call of ops.attention_projected for 96 keys; none with 3 heads or
    with 40 keys (no whole 32-key tiles), where it takes the unfused sequence.  Finite output either way."""
    from nerfmatch_amd.modules.attention import MultiHeadAttention

    monkeypatch.setattr(ops, "LINEAR_PRECISION", "bf16x3")
    monkeypatch.setattr(ops, "ATTENTION_PRECISION", "bf16x3")
    calls = []
    real = ops.attention_projected
    monkeypatch.setattr(ops, "attention_projected", lambda *a, **kw: (calls.append(a[4:8]), real(*a, **kw))[1])
    torch.manual_seed(3)
    for heads, S, want in ((4, 96, 1), (3, 96, 0), (4, 40, 0)):
        mha = MultiHeadAttention(128, head_num=heads, head_dim=32).to(gpu).eval()
        ctx = su.rnd(2, S, 128, seed=1).to(gpu)
        x = ctx if mode == "self" else su.rnd(2, 65, 128, seed=2).to(gpu)
        del calls[:]
        y = mha(x, ctx, ctx, residual=x)
        assert len(calls) == want, (heads, S, calls)
        assert not want or calls[0] == (2, x.shape[1], S, heads)
        assert y.shape == x.shape and bool(torch.isfinite(y).all()), (heads, S)


def test_precision_globals_restored(gpu):
    """Last in the file: what the tests above switched is back at the defaults for the rest of the suite."""
    assert ops.ATTENTION_PRECISION == "fp32" and ops.LINEAR_PRECISION == "fp32"
