"""Driver, float64 oracle, feature builder and case table of the fused dual-softmax matcher tests (test_match_fused_util_cpu.py,
test_match_fused_routes_gpu.py).  csrc/match_fused.hip is driven through its C entry points on buffers the caller fills; the cases below are
the smallest shapes at which each edge of its tile map, tie handling, masks, batch indexing, threshold and scale range still exists.

Everything but run() and run_fresh() is plain torch on the CPU."""
import collections
import functools

import numpy as np
import torch

from conftest import TIE_REL
from nerfmatch_amd import synth
from oracle import matcher_oracle as mo

NM_OK, NM_ERR_ARG, NM_ERR_UNSUPPORTED, NM_ERR_WORKSPACE = 0, 1, 2, 4  # (include/nerfmatch_amd.h; restated so that the table imports no binding)
FT = 128                  # tile edge of csrc/match_fused.hip
SENTINEL_ID = -7          # what the tests put into out_i / out_j before a call
SENTINEL_CONF = -3.0      # ... and into out_conf
MARGIN = 50 * TIE_REL     # 1e-3: how far, relatively, every decision of the float64 oracle is from flipping (exact designed ties aside)
TOL = 1e-4                # returned confidence against the oracle, absolute: the bar of test_matcher_gpu.py
LOG2E_F32 = np.float32(1.44269504088896340736)


# ----------------------------------------------------------------------------------------------- ctypes driver
def workspace_bytes(P, M, N, C):
    from nerfmatch_amd._lib import lib
    return lib().nm_match_fused_workspace_bytes(P, M, N, C)


def run(im, pt, scale, im_mask, pt_mask, threshold, mutual, ws, out_i, out_j, out_conf, counts, ws_bytes=None):
    """nm_dual_softmax_match_fused on the caller's buffers: im (P,M,C), pt (P,N,C) float32, im_mask (P,M) / pt_mask (P,N) uint8 or None,
    ws uint8 (its size is passed unless ws_bytes says otherwise), out_i / out_j (P,M) int64, out_conf (P,M) float32, counts (P,) int32, all on
    the device.  Returns (return code, out_i, out_j, out_conf, counts) as CPU tensors: the raw buffers, whatever they hold."""
    from nerfmatch_amd._lib import dptr, lib, stream
    (P, M, C), N = im.shape, pt.shape[1]
    assert pt.shape == (P, N, C) and out_i.shape == out_j.shape == out_conf.shape == (P, M) and counts.shape == (P,)
    assert (im_mask is None or im_mask.shape == (P, M)) and (pt_mask is None or pt_mask.shape == (P, N))
    u8 = torch.uint8
    rc = lib().nm_dual_softmax_match_fused(dptr(im), dptr(pt), P, M, N, C, float(scale), dptr(im_mask, u8), dptr(pt_mask, u8), float(threshold),
                                           int(bool(mutual)), dptr(out_i, torch.int64), dptr(out_j, torch.int64), dptr(out_conf),
                                           dptr(counts, torch.int32), dptr(ws, u8), ws.numel() if ws_bytes is None else ws_bytes, stream())
    torch.cuda.synchronize()
    return rc, out_i.cpu(), out_j.cpu(), out_conf.cpu(), counts.cpu()


def run_fresh(x, scale, threshold, mutual, fill=0, pairs=None):
    """One call on a workspace of exactly nm_match_fused_workspace_bytes bytes, every byte `fill`, and sentinel-filled outputs.  x: inputs_of()
    dict on the CPU; pairs: a slice of the batch (None: all of it)."""
    sl = slice(None) if pairs is None else pairs
    dev = torch.device("cuda:0")
    g = lambda t: None if t is None else t[sl].contiguous().to(dev)
    im, pt, imm, ptm = g(x["im"]), g(x["pt"]), g(x["im_mask"]), g(x["pt_mask"])
    P, M, C = im.shape
    ws = torch.full((workspace_bytes(P, M, pt.shape[1], C),), fill, device=dev, dtype=torch.uint8)
    oi, oj = (torch.full((P, M), SENTINEL_ID, device=dev, dtype=torch.int64) for _ in range(2))
    oc = torch.full((P, M), SENTINEL_CONF, device=dev, dtype=torch.float32)
    cnt = torch.full((P,), SENTINEL_ID, device=dev, dtype=torch.int32)
    return run(im, pt, scale, imm, ptm, threshold, mutual, ws, oi, oj, oc, cnt)


# ----------------------------------------------------------------------------------------------- geometry of the tile map
Geometry = collections.namedtuple("Geometry", "tiles_m tiles_n rpx grid early groups live_waves_last")


def geometry(M, N):
    """The tile grid match_tile_kernel is launched on: 8 * rpx * tiles_n workgroups (rpx = ceil(tiles_m / 8) row tiles per XCD), of which `early`
    have row_tile >= tiles_m and return at once; groups = 32-row groups of the image side, live_waves_last = how many of the four wavefronts of
    the last row tile have a group of their own (sim_tile's `live`)."""
    tiles_m, tiles_n = -(-M // FT), -(-N // FT)
    rpx = -(-tiles_m // 8)
    groups = -(-M // 32)
    return Geometry(tiles_m, tiles_n, rpx, 8 * rpx * tiles_n, (8 * rpx - tiles_m) * tiles_n, groups, groups - 4 * (tiles_m - 1))


def column_class(col):
    """Which of the two register classes of column_reduce's third halving step (lane bit 2 <-> value-index bit 2 <-> column bit 3) sums
    column `col`."""
    return (col >> 3) & 1


def lane_half(col):
    """Which half of the wavefront holds column `col` of a tile (columns c and c + 4 of an 8-column group sit in lanes l and l + 32)."""
    return (col >> 2) & 1


def max_scale():
    """The largest float32 s with s * log2(e) <= 60 as the entry point evaluates it (float32 product), and the next float above it."""
    s = np.float32(60.0 / 1.44269504088896340736)
    while np.float32(s * LOG2E_F32) <= np.float32(60.0):
        s = np.nextafter(s, np.float32(np.inf))
    while not np.float32(s * LOG2E_F32) <= np.float32(60.0):
        s = np.nextafter(s, np.float32(0.0))
    return float(s), float(np.nextafter(s, np.float32(np.inf)))


# ----------------------------------------------------------------------------------------------- float64 oracle
def oracle(im, pt, scale, im_mask, pt_mask, mutual, threshold, same_cols=(), same_rows=()):
    """One pair: oracle.matcher_oracle.coarse_matching (mask fill -1e9) and mutual_matches (`conf == conf.max()` on equal bits, first column)
    on float64 copies of im (M,C), pt (N,C); masks (M,) / (N,) or None.  Returns conf (M,N) float64, i_ids, j_ids, mconf.
    same_cols / same_rows: groups of columns / rows whose inputs are bit-identical (and equally masked).  The oracle's GEMM is a blocked BLAS
    routine whose summation order depends on where in the matrix a row sits, so such copies come out one float64 step apart now and then;
    they are checked to agree to 1e-12 and then given the bits of the group's first member: equal inputs, equal confidence."""
    imm = None if im_mask is None else im_mask.bool()[None]
    ptm = None if pt_mask is None else pt_mask.bool()[None]
    conf, _, _ = mo.coarse_matching(im.double()[None], pt.double()[None], torch.tensor(float(scale), dtype=torch.float64), imm, ptm)
    for g in same_cols:
        g = [c for c in g if pt_mask is None or pt_mask[c]]
        for c in g[1:]:
            assert torch.equal(pt[c], pt[g[0]]) and bool(((conf[0, :, c] - conf[0, :, g[0]]).abs() <= 1e-12 * conf[0, :, g[0]]).all())
            conf[0, :, c] = conf[0, :, g[0]]
    for g in same_rows:
        for r in g[1:]:
            assert torch.equal(im[r], im[g[0]]) and bool(((conf[0, r] - conf[0, g[0]]).abs() <= 1e-12 * conf[0, g[0]]).all())
            assert im_mask is None or im_mask[r] == im_mask[g[0]]
            conf[0, r] = conf[0, g[0]]
    ids, mconf = mo.mutual_matches(conf, mutual=bool(mutual), threshold=float(threshold))
    return conf[0], ids[1], ids[2], mconf


def undecided_rows(conf, mutual, threshold, margin=MARGIN):
    """Rows of the float64 confidence matrix whose selection an fp32 kernel could decide differently: the row maximum is closer than `margin`
    (relative) to the largest entry of the row that is NOT the same bits, or to the threshold; for mutual matching the same for the column of
    the chosen entry (it is the column maximum by that margin over every entry of other bits, or below it by that margin).  Entries of equal
    bits are exact ties: what the first-column rule is for, and not a matter of rounding.  Rows whose maximum is 0 (masked) are never selected."""
    assert threshold >= 0.0
    top = conf.max(dim=1).values
    runner = conf.masked_fill(conf == top[:, None], -1.0).max(dim=1).values
    bad = (top - runner < margin * top) | ((top - threshold).abs() < margin * top)
    if mutual:
        j = (conf == top[:, None]).float().argmax(dim=1)  # any tied column stands for its group: bit-identical points give bit-identical columns
        col = conf[:, j]  # (M, M): column of row i's entry in [:, i]
        cmax = col.max(dim=0).values
        crun = col.masked_fill(col == cmax[None], -1.0).max(dim=0).values
        is_max = top == cmax
        bad |= torch.where(is_max, cmax - crun < margin * cmax, cmax - top < margin * cmax)
    return torch.nonzero(bad & (top > 0))[:, 0].tolist()


# ----------------------------------------------------------------------------------------------- cases
# design (all optional):
#   dups       groups of columns holding ONE bit-identical point row; the first column of a group is planted as the match of an image row of its
#              own (rows 0, 1, ... in group order), so that row's maximum is attained in every column of the group
#   hide       pt_mask hides the first (lowest) column of every dups group: the reference's answer moves to the next copy
#   dup_rows   groups of bit-identical image rows (the first is a planted row): both rows attain the column maximum of the planted column
#   zero_row / zero_col   an all-zero image token / point: f / (0 + 1e-6) = 0, a whole row / column of equal sim
#   anti       (row, col): pt[col] = -sign(scale) im[row]: sim = -|scale|
#   masks      per pair one of "none", "part" (image tokens 20..30 and points 3..8 masked), "pt-all", "im-all", "first1024" (image tokens 0..1023)
#   plant      how many rows get a planted correspondence (default min(M, N) // 2); thr: a float, or ("between", k): halfway between the k-th and
#              the (k+1)-th largest oracle confidence of the matches at threshold 0
Case = collections.namedtuple("Case", "name group P M N C scale mutual thr seed plant dups hide dup_rows zero_row zero_col anti masks")


def _case(name, group, M, N, mutual, P=1, C=64, scale=10.0, thr=0.0, seed=None, plant=None, dups=(), hide=False, dup_rows=(), zero_row=None,
          zero_col=None, anti=None, masks=None):
    seed = (M * 7919 + N * 104729 + C + P) % 100003 if seed is None else seed
    return Case(name, group, P, M, N, C, float(scale), bool(mutual), thr, seed, min(M, N) // 2 if plant is None else plant,
                tuple(tuple(g) for g in dups), hide, tuple(tuple(g) for g in dup_rows), zero_row, zero_col, anti, masks or ("none",) * P)


TILE_SHAPES = ((1, 1), (31, 33), (128, 128), (129, 127), (897, 130), (1025, 130), (2049, 70), (130, 641))
# the duplicate-column layouts, as (name, N, groups): every group's columns hold one point row
_SWEEP8 = tuple((c, c + 8) for c in range(8)) + tuple((40 + c, 48 + c) for c in range(8))  # class 0 -> 1 in columns 0..15, 1 -> 0 in 40..55
TIE_LAYOUTS = (
    ("same-half", 170, ((7, 23), (34, 35))),                      # same tile, same lane half, same class
    ("other-half", 170, ((8, 12), (99, 103), (1, 5))),            # c and c + 4 of one 8-column group: the two lane halves
    ("other-class", 130, _SWEEP8),                                # c and c + 8: the two register classes of the column sums
    ("tiles-same-class", 300, ((7, 135), (40, 296))),             # tiles 0 / 1, 0 / 2
    ("tiles-other-class", 300, ((7, 143), (24, 257), (9, 129))),  # tiles 0 / 1, 0 / 2
    ("three-tiles", 641, ((21, 130, 640), (3, 139, 520))),        # tiles 0, 1 and 5 (N = 641: tile 5 holds the one column 640); 0, 1 and 4
)


def _cases():
    c = []
    for M, N in TILE_SHAPES:
        for mutual in (True, False):
            c.append(_case(f"tile-{M}x{N}-{'mutual' if mutual else 'rowmax'}", "tile", M, N, mutual))
    # compaction: more than 1024 matches, none, and all of them behind the first 1024-row sweep
    c.append(_case("compact-1153-all", "compact", 1153, 1160, False, plant=1153))
    c.append(_case("compact-1153-none", "compact", 1153, 1160, False, plant=1153, thr=2.0))
    c.append(_case("compact-1153-second-sweep", "compact", 1153, 1160, False, plant=1153, masks=("first1024",)))
    # batch: three different pairs and mask pairs; the evaluator's batch of 16
    for mutual in (True, False):
        c.append(_case(f"batch-P3-{'mutual' if mutual else 'rowmax'}", "batch", 200, 170, mutual, P=3, masks=("none", "pt-all", "part")))
        c.append(_case(f"batch-P3-im-all-{'mutual' if mutual else 'rowmax'}", "batch", 200, 170, mutual, P=3, masks=("part", "im-all", "none"), seed=77))
    c.append(_case("batch-P16", "batch", 96, 140, True, P=16, masks=("none", "part") * 8))
    # exact ties from bit-identical point rows
    for lay, N, groups in TIE_LAYOUTS:
        for M in ((130, 1025) if lay == "other-class" else (130,)):
            for mutual in (True, False):
                for hide in (False, True):
                    c.append(_case(f"tie-{lay}-M{M}-{'mutual' if mutual else 'rowmax'}{'-hidden' if hide else ''}", "tie", M, N, mutual,
                                   dups=groups, hide=hide, seed=500 + M + N))
    for mutual in (True, False):
        c.append(_case(f"tie-rows-{'mutual' if mutual else 'rowmax'}", "tie", 300, 170, mutual, dup_rows=((5, 260), (40, 41, 170))))
        c.append(_case(f"tie-zero-{'mutual' if mutual else 'rowmax'}", "tie", 200, 170, mutual, zero_row=150, zero_col=160))
    # threshold between two oracle confidences
    for mutual in (True, False):
        c.append(_case(f"thr-between-{'mutual' if mutual else 'rowmax'}", "thr", 200, 170, mutual, thr=("between", 40)))
    # scale: negative, and the largest admitted with an anti-aligned point (sim = -|scale|)
    smax, _ = max_scale()
    for mutual in (True, False):
        c.append(_case(f"scale-neg10-{'mutual' if mutual else 'rowmax'}", "scale", 130, 70, mutual, scale=-10.0, anti=(100, 60)))
        c.append(_case(f"scale-max-{'mutual' if mutual else 'rowmax'}", "scale", 130, 70, mutual, scale=smax, anti=(100, 60)))
        c.append(_case(f"scale-negmax-{'mutual' if mutual else 'rowmax'}", "scale", 130, 70, mutual, scale=-smax, anti=(100, 60)))
    # the other feature widths, ragged
    for C in (128, 256, 512):
        c.append(_case(f"C{C}-139x133", "C", 139, 133, True, C=C))
    return c


CASES = _cases()
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
GROUPS = ("tile", "compact", "batch", "tie", "thr", "scale", "C")


def _masks(kind, M, N):
    imm, ptm = torch.ones(M, dtype=torch.uint8), torch.ones(N, dtype=torch.uint8)
    if kind == "part":
        imm[20:31] = 0
        ptm[3:9] = 0
    elif kind == "pt-all":
        ptm[:] = 0
    elif kind == "im-all":
        imm[:] = 0
    elif kind == "first1024":
        imm[:1024] = 0
    else:
        assert kind == "none", kind
    return imm, ptm


def _base_pair(case, p):
    """synth.separated_features + planted correspondences (row i <-> column perm[i], on the side of the sign of the scale), then the design."""
    M, N, C = case.M, case.N, case.C
    g = torch.Generator().manual_seed(case.seed * 31 + p)
    im, pt = synth.separated_features(M, N, C, seed=case.seed + 1000 * p)
    sign = 1.0 if case.scale > 0 else -1.0
    perm = torch.randperm(N, generator=g)
    firsts = [grp[0] for grp in case.dups]
    taken = {col for grp in case.dups for col in grp} | ({case.zero_col} if case.zero_col is not None else set()) | ({case.anti[1]} if case.anti else set())
    perm = firsts + [int(j) for j in perm if int(j) not in taken]  # rows 0.. take the duplicate groups' first columns, then free columns
    k = min(max(case.plant, len(firsts)), len(perm), M)
    perm = torch.tensor(perm[:k], dtype=torch.int64)
    pt[perm] = sign * im[:k] + 0.02 * torch.randn(k, C, generator=g)
    for grp in case.dups:
        for col in grp[1:]:
            pt[col] = pt[grp[0]]
    for grp in case.dup_rows:
        for row in grp[1:]:
            im[row] = im[grp[0]]
    if case.zero_row is not None:
        im[case.zero_row] = 0.0
    if case.zero_col is not None:
        pt[case.zero_col] = 0.0
    if case.anti is not None:
        pt[case.anti[1]] = -sign * im[case.anti[0]]
    return im, pt, perm, g


def designed_rows(case):
    """Image rows the builder must not touch (bit-identical or all-zero by design)."""
    return {r for grp in case.dup_rows for r in grp} | ({case.zero_row} if case.zero_row is not None else set())


@functools.lru_cache(maxsize=None)
def inputs_of(case):
    """CPU tensors of a case: im (P,M,C), pt (P,N,C) float32, im_mask (P,M) / pt_mask (P,N) uint8 (None when no pair of the case is masked),
    perm (list of P index tensors: row i of pair p is planted on column perm[p][i]), thr (float), reseeded (rows perturbed per pair).
    Every row outside a designed exact tie is decisive in the float64 oracle (undecided_rows is empty): rows that are not are perturbed, on the
    image side only, until they are.  Shared: do not modify."""
    ims, pts, perms, imms, ptms, moved = [], [], [], [], [], []
    thr = 0.0 if isinstance(case.thr, tuple) else float(case.thr)
    for p in range(case.P):
        im, pt, perm, g = _base_pair(case, p)
        imm, ptm = _masks(case.masks[p], case.M, case.N)
        if case.hide:
            for grp in case.dups:
                ptm[grp[0]] = 0
        keep = designed_rows(case)
        n_moved = 0
        for _ in range(40):
            conf = oracle(im, pt, case.scale, imm, ptm, case.mutual, thr, case.dups, case.dup_rows)[0]
            if isinstance(case.thr, tuple) and p == 0:  # halfway between two neighbouring match confidences that are far enough apart
                mc = torch.sort(oracle(im, pt, case.scale, imm, ptm, case.mutual, 0.0, case.dups, case.dup_rows)[3], descending=True).values
                k = case.thr[1]
                while (mc[k - 1] - mc[k]) < 4 * MARGIN * mc[k - 1]:
                    k += 1
                thr = float((mc[k - 1] + mc[k]) / 2)
            bad = undecided_rows(conf, case.mutual, thr)
            if not bad:
                break
            assert not set(bad) & keep, (case.name, p, sorted(set(bad) & keep))
            for r in bad:
                im[r] = im[r] + 0.05 * torch.randn(case.C, generator=g)
            n_moved += len(bad)
        else:
            raise AssertionError(f"{case.name} pair {p}: rows {bad[:8]} stay undecided")
        ims.append(im); pts.append(pt); perms.append(perm); imms.append(imm); ptms.append(ptm); moved.append(n_moved)
    masked = any(k != "none" for k in case.masks) or case.hide
    return dict(im=torch.stack(ims), pt=torch.stack(pts), im_mask=torch.stack(imms) if masked else None, pt_mask=torch.stack(ptms) if masked else None,
                perm=perms, thr=thr, reseeded=moved)


@functools.lru_cache(maxsize=None)
def oracle_of(case):
    """Per pair (conf, i_ids, j_ids, mconf) of the float64 oracle at the case's threshold, computed once and shared: do not modify."""
    x = inputs_of(case)
    pick = lambda t, p: None if t is None else t[p]
    return [oracle(x["im"][p], x["pt"][p], case.scale, pick(x["im_mask"], p), pick(x["pt_mask"], p), case.mutual, x["thr"], case.dups, case.dup_rows) for p in range(case.P)]


def tie_rows(conf):
    """{row: columns attaining the row maximum} for the rows of a float64 confidence matrix where more than one column does (maximum > 0)."""
    top = conf.max(dim=1).values
    hit = (conf == top[:, None]) & (top[:, None] > 0)
    return {int(r): torch.nonzero(hit[r])[:, 0].tolist() for r in torch.nonzero(hit.sum(1) > 1)[:, 0]}
