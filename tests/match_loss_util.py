"""Drivers, float64 reference, dispatch restatement and case table of the coarse-match loss route tests (test_match_loss_util_cpu.py,
test_match_routes_gpu.py).  csrc/match.hip picks its kernels by shape and pointer alignment; the cases below reach every choice.

The reference is plain torch on the CPU; only run_pair / focal_count touch the GPU (ctypes over nerfmatch_amd._lib.lib(), as autograd.py)."""
import collections
import functools

import torch
import torch.nn.functional as F

from oracle import matcher_oracle as mo

NM_MATCH_BF16X3 = 1  # (= nerfmatch_amd._lib.NM_MATCH_BF16X3; restated so that the CPU tests need not import the package)

# ----------------------------------------------------------------------------------------------- bounds
# From the project's tests of the same quantities: conf / loss / gradients of test_train_gpu.test_coarse_match_loss_and_gradients (the loss
# relative to the loss itself, as test_training_step_mid_size_vs_oracle takes it); for the split-bf16 similarity GEMM the loss and gradient
# bounds of test_training_step_mid_size_vs_oracle and the conf bound of test_matcher_gpu.test_dual_softmax_full_size_vs_oracle.
TOL_FP32 = dict(conf=1e-5, loss=1e-5, grad=1e-4, dscale=1e-4)
TOL_BF16X3 = dict(conf=1e-4, loss=1e-5, grad=5e-3, dscale=5e-3)


def tolerances(flags):
    return TOL_BF16X3 if flags & NM_MATCH_BF16X3 else TOL_FP32


def rel(a, b, floor=1e-3):
    """max |a - b| relative to the largest reference entry (at least `floor`): the measure of test_train_gpu.py."""
    a, b = a.detach().cpu().double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(floor)).item()


def rel_scalar(a, b, floor=0.0):
    return abs(float(a) - float(b)) / max(abs(float(b)), floor, 1e-300)


# ----------------------------------------------------------------------------------------------- dispatch of csrc/match.hip
ROW_NREG = 20     # row_stats / row_select keep a row of up to 64 * 4 * ROW_NREG columns in registers
COL_CHUNKS = 64


def _align256(v):
    return (v + 255) & ~255


def route(M, N, gt_aligned=True, pt_mask_aligned=True):
    """The kernels nm_dual_softmax_match, nm_match_focal_loss and nm_match_focal_loss_bwd launch for an M x N pair, as three names.
    gt_aligned: conf_gt (of this pair) is 4-byte aligned; pt_mask_aligned: pt_mask is NULL or 4-byte aligned.  The three dispatch sites of
    csrc/match.hip point here: keep them in step."""
    vec = N % 4 == 0
    stats = "stats:vec-cached" if vec and N <= 64 * 4 * ROW_NREG else "stats:vec-uncached" if vec else "stats:scalar"
    nx = (N + 255) // 256
    fits = _align256(nx * M * 4) + nx * COL_CHUNKS * 16 <= COL_CHUNKS * N * 4
    loss = "loss:tile" if vec and gt_aligned and fits else "loss:two-kernel"
    bwd = "bwd:vec4" if vec and gt_aligned and pt_mask_aligned else "bwd:vec1"
    return stats, loss, bwd


ROUTE_NAMES = (("stats:vec-cached", "stats:vec-uncached", "stats:scalar"), ("loss:tile", "loss:two-kernel"), ("bwd:vec4", "bwd:vec1"))


# ----------------------------------------------------------------------------------------------- float64 reference
def focal_loss(conf, conf_gt, alpha=0.25, gamma=2.0, clamp=True):
    """oracle.train_oracle.matching_loss over alpha, gamma and clamp; conf_gt holds bytes: 1 = positive, 0 = negative, anything else belongs
    to neither mean (and to neither count)."""
    if clamp:
        conf = torch.clamp(conf, 1e-6, 1 - 1e-6)
    pos, neg = conf_gt == 1, conf_gt == 0
    loss_pos = -alpha * torch.pow(1 - conf[pos], gamma) * conf[pos].log()
    loss_neg = -alpha * torch.pow(conf[neg], gamma) * (1 - conf[neg]).log()
    return loss_pos.mean() + loss_neg.mean()


def reference(im, pt, scale, im_mask, pt_mask, conf_gt, alpha, gamma, clamp, grad_loss=1.0, dtype=torch.float64):
    """im (B,M,C), pt (B,N,C), masks (B,M) / (B,N) or None, conf_gt (B,M,N) uint8 (2-D inputs: one pair) -> dict of `dtype` CPU tensors:
      conf (B,M,N)  oracle.matcher_oracle.coarse_matching (mask fill -1e9, as the kernels)
      loss          focal_loss over the whole batch
      t, row_t, col_t   t = conf * d loss / d conf, its row and column sums
      ddot (B,M,N)  grad_loss * d loss / d (im_n . pt_n): autograd through the same expression with the dot products of the normalised
                    features as the leaf (torch.clamp passes the gradient on the closed interval, as focal_t does; masked_fill none)
      dscale (B,)   each pair's share of grad_loss * d loss / d scale;  dscale_total: the same by autograd
      conf_leaf     the confidence of the differentiated expression (equal to conf bit for bit: test_match_loss_util_cpu.py)."""
    if im.dim() == 2:
        im, pt, conf_gt = im[None], pt[None], conf_gt[None]
        im_mask = None if im_mask is None else im_mask[None]
        pt_mask = None if pt_mask is None else pt_mask[None]
    im, pt = im.detach().cpu().to(dtype), pt.detach().cpu().to(dtype)
    conf_gt = conf_gt.cpu()
    im_m = None if im_mask is None else im_mask.cpu().bool()
    pt_m = None if pt_mask is None else pt_mask.cpu().bool()
    with torch.enable_grad():
        conf, imn, ptn = mo.coarse_matching(im, pt, torch.tensor(float(scale), dtype=dtype), im_m, pt_m)
        dot = torch.einsum("bmd,bnd->bmn", imn, ptn).detach().requires_grad_()
        s = torch.tensor(float(scale), dtype=dtype, requires_grad=True)
        sim = dot * s
        ki = torch.ones_like(im[..., 0]) if im_m is None else im_m
        kp = torch.ones_like(pt[..., 0]) if pt_m is None else pt_m
        sim = sim.masked_fill(~(ki[..., None] * kp[:, None]).bool(), -1e9)
        conf_leaf = F.softmax(sim, 1) * F.softmax(sim, 2)
        conf_leaf.retain_grad()
        loss = focal_loss(conf_leaf, conf_gt, alpha, gamma, clamp)
        loss.backward()
    t = conf_leaf.detach() * conf_leaf.grad
    ddot = grad_loss * dot.grad
    return dict(conf=conf.detach(), conf_leaf=conf_leaf.detach(), loss=loss.detach(), t=t, row_t=t.sum(2), col_t=t.sum(1), ddot=ddot,
                dscale=(ddot * dot.detach()).sum((1, 2)) / float(scale), dscale_total=grad_loss * s.grad)


# ----------------------------------------------------------------------------------------------- ctypes drivers
def focal_count(conf_gt, acc=None):
    """nm_focal_count over `conf_gt` (a contiguous uint8 device tensor or view) onto acc[2:4]; a fresh zeroed acc when none is given."""
    from nerfmatch_amd._lib import check, dptr, lib, stream
    if acc is None:
        acc = torch.zeros(4, device=conf_gt.device, dtype=torch.float64)
    check(lib().nm_focal_count(dptr(conf_gt, torch.uint8), conf_gt.numel(), dptr(acc, torch.float64), stream()), "nm_focal_count")
    return acc


def run_pair(im, pt, scale, im_mask, pt_mask, conf_gt, alpha, gamma, clamp, mutual, threshold, flags, grad_loss=None, acc=None):
    """One pair through the C entry points, on fresh NaN-filled outputs: nm_focal_count (skipped when the caller hands in the `acc` of a
    batch it has counted already), nm_dual_softmax_match, nm_match_focal_loss, nm_match_focal_loss_bwd.  im (M,C), pt (N,C) float32,
    im_mask (M) / pt_mask (N) / conf_gt (M,N) uint8, all on the device; the uint8 ones may be views (misaligned on purpose).
    Returns CPU tensors: acc (4, float64, as it stands after this pair's loss), loss (from that acc), row_t, col_t, conf, i_ids, j_ids,
    mconf, ddot, and dscale (float)."""
    from nerfmatch_amd._lib import check, dptr, lib, stream
    L = lib()
    u8, f64, dev = torch.uint8, torch.float64, im.device
    (M, Cc), N = im.shape, pt.shape[0]
    assert conf_gt.shape == (M, N) and pt.shape[1] == Cc
    if acc is None:
        acc = focal_count(conf_gt)
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev, dtype=torch.float32)
    need = L.nm_match_workspace_bytes(M, N, Cc)
    ws = torch.empty(need, device=dev, dtype=u8)
    conf, imn, ptn, mconf, row_t, col_t, ddot = nan(M, N), nan(M, Cc), nan(N, Cc), nan(M), nan(M), nan(N), nan(M, N)
    oi, oj = (torch.full((M,), -7, device=dev, dtype=torch.int64) for _ in range(2))
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)
    check(L.nm_dual_softmax_match(dptr(im), dptr(pt), M, N, Cc, float(scale), dptr(im_mask, u8), dptr(pt_mask, u8), float(threshold),
                                  int(bool(mutual)), int(flags), dptr(conf), dptr(imn), dptr(ptn), dptr(oi, torch.int64), dptr(oj, torch.int64),
                                  dptr(mconf), dptr(cnt, torch.int32), dptr(ws, u8), need, stream()), "nm_dual_softmax_match")
    check(L.nm_match_focal_loss(dptr(conf_gt, u8), M, N, Cc, float(alpha), float(gamma), int(bool(clamp)), dptr(ws, u8), need, dptr(acc, f64),
                                dptr(row_t), dptr(col_t), stream()), "nm_match_focal_loss")
    acc_now = acc.clone()
    g = None if grad_loss is None else torch.tensor([grad_loss], device=dev, dtype=torch.float32)
    dscale = torch.zeros(1, device=dev, dtype=f64)
    check(L.nm_match_focal_loss_bwd(dptr(conf_gt, u8), dptr(im_mask, u8), dptr(pt_mask, u8), M, N, Cc, float(alpha), float(gamma),
                                    int(bool(clamp)), float(scale), dptr(g), dptr(ws, u8), need, dptr(acc, f64), dptr(row_t), dptr(col_t),
                                    dptr(ddot), dptr(dscale, f64), stream()), "nm_match_focal_loss_bwd")
    torch.cuda.synchronize()
    n = int(cnt.item())
    a = acc_now.cpu()
    return dict(acc=a, loss=(a[0] / a[2] + a[1] / a[3]).item(), row_t=row_t.cpu(), col_t=col_t.cpu(), conf=conf.cpu(), i_ids=oi[:n].cpu(),
                j_ids=oj[:n].cpu(), mconf=mconf[:n].cpu(), ddot=ddot.cpu(), dscale=dscale.item())


def offset_view(t, off):
    """A copy of the uint8 tensor `t` (any shape) that starts `off` bytes behind an allocation boundary."""
    buf = torch.empty(t.numel() + 16, device=t.device, dtype=torch.uint8)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ----------------------------------------------------------------------------------------------- cases
# Inputs follow test_train_gpu.test_coarse_match_loss_and_gradients: randn features, k planted positives pt[perm] = im[:k] + noise * randn,
# scale 10.  One seed per shape.  `special`:
#   ignored    bytes 2 and 255 over ~5 % of conf_gt and over three planted positives: in neither mean, neither count, no t
#   clamp-low  ten entries (planted row, ANOTHER planted column) labelled positive: conf ~ (row soft-max tail) x (column soft-max tail) < 1e-7
#   peaked     noise 0, scale 50: the planted entries saturate (conf > 1 - 1e-6); two of them are relabelled negative
# gt_off / pm_off: byte offset of conf_gt / pt_mask behind an allocation boundary (pm_off None: no view, the mask as allocated).
# loose: (quantity, recorded error of the float32 evaluation) pairs: bound 4 x that error instead of TOL_*, see "measured bounds" below.
Case = collections.namedtuple("Case", "name M N C k noise scale seed B masked gt_off pm_off alpha gamma clamp selections flags special expect loose")

_SEEDS = {(40, 5124): 41, (300, 8): 42, (1100, 8): 43, (90, 70): 44, (100, 72): 45, (64, 64): 46, (130, 264): 47, (48, 64): 48}
_TILE4 = ("stats:vec-cached", "loss:tile", "bwd:vec4")
_TWO1 = ("stats:scalar", "loss:two-kernel", "bwd:vec1")
_E_LOSS_FP32 = {(0.25, 2.0): 5.43e-6, (0.4, 2.0): 5.33e-6, (0.25, 1.5): 5.03e-6, (0.25, 3.0): 5.23e-6}  # ("measured bounds" below)


def _case(name, M, N, expect, C=256, k=None, noise=0.3, scale=10.0, B=1, masked=False, gt_off=0, pm_off=None, alpha=0.25, gamma=2.0, clamp=1,
          selections=((False, 0.0),), flags=0, special=None, loose=()):
    return Case(name, M, N, C, min(M, N) // 2 if k is None else k, noise, scale, _SEEDS[(M, N)], B, masked, gt_off, pm_off, alpha, gamma, clamp,
                tuple(selections), flags, special, tuple(expect), tuple(loose))


def _cases():
    c = []
    # a: the <4,0> statistics and selection; tile loss with 21 column chunks, vectorised backward
    c.append(_case("a-40x5124", 40, 5124, ("stats:vec-uncached", "loss:tile", "bwd:vec4"), k=20,
                   selections=((True, 0.0), (True, 0.3), (False, 0.0), (False, 0.3))))
    # b: tall and narrow: N % 4 == 0 but the partial sums do not fit -> two-kernel loss, then the vectorised backward
    c.append(_case("b-300x8", 300, 8, ("stats:vec-cached", "loss:two-kernel", "bwd:vec4"), k=4))
    c.append(_case("b-1100x8", 1100, 8, ("stats:vec-cached", "loss:two-kernel", "bwd:vec4"), k=6))
    # c: VEC = 1 everywhere, focal_bwd_kernel<1> included
    c.append(_case("c-90x70", 90, 70, _TWO1, k=30))
    c.append(_case("c-90x70-masked", 90, 70, _TWO1, k=30, masked=True))
    c.append(_case("c-90x70-B2", 90, 70, _TWO1, k=30, masked=True, B=2))
    # d: misaligned conf_gt / pt_mask (the aligned run of the same data is d-aligned)
    c.append(_case("d-aligned", 100, 72, _TILE4, masked=True, pm_off=0))
    c.append(_case("d-gt+1", 100, 72, ("stats:vec-cached", "loss:two-kernel", "bwd:vec1"), masked=True, gt_off=1, pm_off=0))
    c.append(_case("d-ptmask+1", 100, 72, ("stats:vec-cached", "loss:tile", "bwd:vec1"), masked=True, pm_off=1))
    c.append(_case("d-both+1", 100, 72, ("stats:vec-cached", "loss:two-kernel", "bwd:vec1"), masked=True, gt_off=1, pm_off=1))
    # e: alpha, gamma (the powf branches) and clamp
    for alpha, gamma in ((0.25, 2.0), (0.4, 2.0), (0.25, 1.5), (0.25, 3.0), (1.0, 1.0)):
        for clamp in (0, 1):
            c.append(_case(f"e-alpha{alpha:g}-gamma{gamma:g}-clamp{clamp}", 100, 72, _TILE4, alpha=alpha, gamma=gamma, clamp=clamp,
                           loose=(("loss", _E_LOSS_FP32[(alpha, gamma)]),) if (alpha, gamma) in _E_LOSS_FP32 else ()))
    # f: ignored bytes, in the tile kernel + focal_bwd<4> and in focal_rows / focal_cols + focal_bwd<1>
    c.append(_case("f-100x72", 100, 72, _TILE4, special="ignored"))
    c.append(_case("f-90x70", 90, 70, _TWO1, k=30, special="ignored"))
    # g: the lower clamp bound
    for clamp in (0, 1):
        c.append(_case(f"g-100x72-clamp{clamp}", 100, 72, _TILE4, special="clamp-low", clamp=clamp))
        c.append(_case(f"g-90x70-clamp{clamp}", 90, 70, _TWO1, k=30, special="clamp-low", clamp=clamp))
    # h: the upper clamp bound (clamp = 0 would be log 0, in the reference too)
    c.append(_case("h-64x64-peaked", 64, 64, _TILE4, C=128, k=32, noise=0.0, scale=50.0, special="peaked", loose=(("loss", 6.08e-4),)))
    # i: the other feature widths, both similarity GEMMs
    for M, N, C in ((130, 264, 512), (100, 72, 64), (48, 64, 128)):
        for flags in (0, NM_MATCH_BF16X3):
            c.append(_case(f"i-{M}x{N}-C{C}-{'bf16x3' if flags else 'fp32'}", M, N, _TILE4, C=C, flags=flags))
    return c


CASES = _cases()
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

# ---- measured bounds (a case that does not meet TOL_* is allowed 4 x the error of the SAME reference expression evaluated in float32 with
# torch on the CPU, reference(dtype=float32), against float64; both numbers are recorded here and the recorded one makes the bound) ------
# Only the loss of nine cases needs it; everything else meets TOL_* (the figures are in the docstring of test_match_routes_gpu.test_case).
#   case                     loss (float64)   torch fp32 vs float64   bound = 4 x   kernels vs float64 (MI355X)
#   e alpha 0.25 gamma 2     7.25e-07         5.43e-06                2.17e-05      1.27e-05      (clamp 0 and 1 alike: no entry is clamped)
#   e alpha 0.4  gamma 2     1.16e-06         5.33e-06                2.13e-05      1.27e-05
#   e alpha 0.25 gamma 1.5   6.05e-06         5.03e-06                2.01e-05      1.04e-05
#   e alpha 0.25 gamma 3     1.05e-08         5.23e-06                2.09e-05      1.75e-05
#   h-64x64-peaked           2.66e-03         6.08e-04                2.43e-03      6.09e-04
# The float32 column depends on the CPU that evaluates it (vector width, maths library): the host of the MI355X the kernels were measured on
# gives 3.70e-06 for gamma 2 and 2.87e-06 for gamma 3, under which the gamma 3 pair would miss (1.75e-05 against 1.15e-05).  That is why the
# bound is the recorded number and not a fresh evaluation, and why the cause matters more than the factor:
# e: the positives carry these losses (the negatives' share is below 1e-3): -alpha (1 - c)^gamma log c ~ alpha (1 - c)^(gamma + 1) at
#   c = 0.982 .. 0.988, so the relative error of the loss is (gamma + 1) dc / (1 - c) -- and an fp32 conf next to 1 is a multiple of 2^-24, which
#   alone is 4e-6 of 1 - c.  Evaluating the loss in float64 on the kernels' own fp32 conf gives their error to three digits (1.747e-05 of
#   1.750e-05 for gamma 3); the four figures are (gamma + 1) x 4.2e-06, one fp32 step in conf, which is 4.3e-07 from float64 at worst.  The
#   kernels evaluate conf of such an entry as (1 * 1/csum) * 1/rsum, three roundings, like softmax * softmax in torch.  No defect: the loss of
#   a nearly solved pair cannot be had to 1e-5 from an fp32 confidence.  (alpha 1 gamma 1: 2 x 4.1e-06 = 8.2e-06 meets 1e-5.)
# h: 64 % of the loss is the two relabelled negatives' term at the clamped c, and 1 - 1e-6 is not an fp32 number: fp32 clamps to 1 - 17 * 2^-24,
#   so log(1 - c) is log(1.0133e-6) instead of log(1e-6), 9.5e-4 relative on those terms -- in torch fp32 and in the kernels to the same digits.


def fp32_error(case, what):
    """Error of reference(dtype=float32) against float64 for `case`, in the measure the tests use for `what`."""
    r64, r32 = reference_of(case), reference_of(case, torch.float32)
    if what == "loss":
        return rel_scalar(r32["loss"], r64["loss"])
    if what == "dscale":
        return max(rel_scalar(a, b, 1e-3) for a, b in zip(r32["dscale"], r64["dscale"]))
    if what == "conf":
        return (r32["conf"].double() - r64["conf"]).abs().max().item()
    return rel(r32[what], r64[what])


def bound(case, what):
    """The bound of quantity `what` (conf, loss, row_t, col_t, ddot, dscale) for `case`."""
    if what in dict(case.loose):
        return 4.0 * dict(case.loose)[what]
    return tolerances(case.flags)["grad" if what in ("row_t", "col_t", "ddot") else what]


@functools.lru_cache(maxsize=None)
def inputs_of(case):
    """CPU tensors of a case: im (B,M,C), pt (B,N,C) float32, gt (B,M,N) uint8, im_mask / pt_mask (B,M) / (B,N) uint8 or None,
    perm (B,k) planted columns (row i <-> column perm[b, i]), marked (n,3) int64 [b, i, j] entries of `special`.  Shared: do not modify."""
    B, M, N, C, k = case.B, case.M, case.N, case.C, case.k
    g = torch.Generator().manual_seed(case.seed)
    im, pt = torch.randn(B, M, C, generator=g), torch.randn(B, N, C, generator=g)
    gt = torch.zeros(B, M, N, dtype=torch.uint8)
    perms = []
    for b in range(B):
        perm = torch.randperm(N, generator=g)[:k]
        gt[b, torch.arange(k), perm] = 1
        pt[b, perm] = im[b, :k] + case.noise * torch.randn(k, C, generator=g)
        perms.append(perm)
    im_mask = pt_mask = None
    if case.masked:  # the last 9 image tokens of the first pair, points 4..16 of the last
        im_mask, pt_mask = torch.ones(B, M, dtype=torch.uint8), torch.ones(B, N, dtype=torch.uint8)
        im_mask[0, -9:] = 0
        pt_mask[B - 1, 4:17] = 0
    marked = []
    gs = torch.Generator().manual_seed(1000 + case.seed)
    if case.special == "ignored":
        planted = [(0, i, int(perms[0][i])) for i in range(3)]
        flat = [(0, int(f) // N, int(f) % N) for f in torch.randperm(M * N, generator=gs)]
        marked = [e for e in flat if e not in planted][: (M * N) // 20] + planted
        for n, (b, i, j) in enumerate(marked):
            gt[b, i, j] = (2, 255)[n % 2]
    elif case.special == "clamp-low":
        marked = [(0, i, int(perms[0][(i + 1) % k])) for i in range(10)]
        for b, i, j in marked:
            gt[b, i, j] = 1
    elif case.special == "peaked":
        marked = [(0, i, int(perms[0][i])) for i in range(2)]
        for b, i, j in marked:
            gt[b, i, j] = 0
    return dict(im=im, pt=pt, gt=gt, im_mask=im_mask, pt_mask=pt_mask, perm=torch.stack(perms), marked=torch.tensor(marked, dtype=torch.int64).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def reference_of(case, dtype=torch.float64):
    """reference() of a case's inputs, computed once and shared: do not modify."""
    x = inputs_of(case)
    return reference(x["im"], x["pt"], case.scale, x["im_mask"], x["pt_mask"], x["gt"], case.alpha, case.gamma, case.clamp, dtype=dtype)


def band_counts(conf, gt):
    """(labelled positives with conf in [5e-7, 2e-6], labelled negatives with conf in [1 - 2e-6, 1 - 5e-7]): entries whose t jumps by a large
    amount when fp32 rounding puts conf on the other side of a clamp bound.  Both must be 0 for every case."""
    low = ((gt == 1) & (conf >= 5e-7) & (conf <= 2e-6)).sum().item()
    high = ((gt == 0) & (conf >= 1 - 2e-6) & (conf <= 1 - 5e-7)).sum().item()
    return low, high


def check_input_conditions(case):
    """The conditions the comparisons rest on, on the float64 reference; asserted without a GPU and again in front of every GPU case."""
    x, r = inputs_of(case), reference_of(case)
    conf, gt = r["conf"], x["gt"]
    assert band_counts(conf, gt) == (0, 0), (case.name, band_counts(conf, gt))
    m = x["marked"]
    cm = conf[m[:, 0], m[:, 1], m[:, 2]]
    if case.special == "clamp-low":
        assert len(m) == 10 and bool((gt[m[:, 0], m[:, 1], m[:, 2]] == 1).all()) and cm.max().item() < 1e-7, (case.name, cm.max().item())
        assert int((gt == 1).sum()) == case.k + 10  # none of the ten is a planted entry
    elif case.special == "peaked":
        assert int((conf > 1 - 1e-6).sum()) == case.k and bool((cm > 1 - 1e-6).all()) and bool((gt[m[:, 0], m[:, 1], m[:, 2]] == 0).all())
        assert int((gt == 1).sum()) == case.k - 2
    elif case.special == "ignored":
        assert bool((gt[m[:, 0], m[:, 1], m[:, 2]] > 1).all()) and int((gt > 1).sum()) == len(m) == (case.M * case.N) // 20 + 3
        assert int((gt == 1).sum()) <= case.k - 3  # three planted positives are among the ignored
    if case.clamp == 0:  # log 0 in the kernels and in the reference alike
        assert conf[gt == 1].min().item() > 0 and conf[gt == 0].max().item() < 1


# nm_focal_count alone: sizes around one 16-byte vector, a ragged tail, and one past the 512-workgroup cap (9 000 001 / 16 vectors over
# 256 * 4 per workgroup = 550 workgroups asked for, 512 launched: the grid stride runs)
COUNT_SIZES = (1, 15, 16, 17, 4097, 9_000_001)
COUNT_OFFSETS = (0, 1, 7, 15)


def count_bytes(total, seed=0):
    """`total` bytes drawn from {0, 1, 2, 255} (CPU uint8 tensor)."""
    g = torch.Generator().manual_seed(seed)
    return torch.tensor([0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 4, (total,), generator=g)]
