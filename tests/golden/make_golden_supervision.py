#!/usr/bin/env python3
"""Golden vectors of the coarse match supervision (tests/golden/supervision.npz), from the REFERENCE's own project_points3d.

    python tests/golden/make_golden_supervision.py        # rewrites tests/golden/supervision.npz (NM_GOLDEN_OUT=<dir>: elsewhere)

Needs the reference tree (make_golden.py's REF and stub modules).  The projections are the reference's numpy function
(nerfmatch/utils/geometry.py:119-136) on fp32 inputs, with the world-to-camera matrix the reference's datasets use (`qc2w.inverse()` in fp32,
nerfmatch/datasets/nerfmatch_dataset.py:261-262), and the same function on fp64 inputs (inverse taken in fp64).  Cell ids, the dense
matrix and the np.where triple restate nerfmatch_dataset.py:329-351 (= :562-583) line by line in `reference_supervision` below.

Cases (all at ds = 8)
  A  48 x 64 px (M = 48), B = 2 poses, N = 200: several points per cell, empty cells, and hand-placed points in cell row 0, in cell
     column 0, outside each of the four borders, behind the camera with the flipped projection inside the image, with pt_mask false,
     and on a cell whose im_mask is false;
  B1, B129  the same camera, N = 1 and N = 129;
  C  B = 2, element 0 sees nothing (for the fallback), element 1 does; with and without the fallback pairs C_fallback;
  D  480 x 640 px (M = 4800), one pose, k = 2 frames of 2400 points: cell ids and triple only;
  P  480 x 640 px, 4096 points WITHOUT the margin below (property test): fp64 projections and cells.

Boundary condition (asserted here for A-D): every fp64 projection is >= 0.01 px away from every multiple of ds in x and in y, and the
reference's fp32 cell equals its fp64 cell -- for those points the cell is not a rounding question, the tests demand identical integers.
`max_err_px` = max |fp32 - fp64| of the reference's projections over A-D; the tests' bar for pt2d_proj is 4 x that.
For P the generator asserts that the reference's own fp32 cells differ from the fp64 ones only within that bar of a cell boundary, and on
at most 1 % of the points.  Only arrays are written."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_golden as mg  # noqa: E402

DS = 8
MARGIN = 0.01


def camera(seed, H, W, focal):
    """fp32 intrinsics and a fp32 camera-to-world matrix (4 x 4) rounded from a fp64 rigid transform."""
    g = np.random.default_rng(seed)
    rv = g.uniform(-0.4, 0.4, 3)
    ang = np.linalg.norm(rv)
    ax = rv / ang
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = R, g.uniform(-1.0, 1.0, 3)
    K = np.array([[focal, 0, W / 2], [0, focal * 1.01, H / 2], [0, 0, 1]])
    return K.astype(np.float32), c2w.astype(np.float32)


def lift(K, c2w, uv, depth):
    """World points (fp32) whose projection under (K, c2w) is uv (n, 2) at camera depth `depth` (n,; negative: behind the camera)."""
    K, c2w = K.astype(np.float64), c2w.astype(np.float64)
    rays = np.concatenate([uv, np.ones((len(uv), 1))], -1) @ np.linalg.inv(K).T
    cam = rays * depth[:, None]
    return (cam @ c2w[:3, :3].T + c2w[:3, 3]).astype(np.float32)


def cell_pixels(g, cells_xy):
    """A pixel inside each cell (cx, cy), at least 0.5 px from the cell's borders."""
    return (np.asarray(cells_xy, np.float64) + g.uniform(0.0625, 0.9375, (len(cells_xy), 2))) * DS


def project_ref(K, c2w, pt3d, f64=False):
    """The reference's projection of one sample (nerfmatch_dataset.py:261-262, :303-308)."""
    from nerfmatch.utils.geometry import project_points3d

    dt = torch.float64 if f64 else torch.float32
    qK, qc2w = torch.tensor(K, dtype=dt), torch.tensor(c2w, dtype=dt)
    qw2c = qc2w.inverse()
    return project_points3d(qK.numpy(), qw2c[:3, :3].numpy(), qw2c[:3, 3].numpy(), pt3d.astype(np.float64 if f64 else np.float32))


def reference_supervision(qpt2d_proj, h, w, qmask, rmask, ds=DS, fallback=None):
    """nerfmatch_dataset.py:329-351 for one sample: -> match_gt (M, N) float32, gt_cell (N,) (-1 where the column is empty before the fallback)."""
    M, N = len(qmask), len(rmask)
    with np.errstate(invalid="ignore"):
        qpt2d_proj_ds = np.floor(qpt2d_proj / ds).astype(np.int64)                                     # :329
    rpt3d_visible = (qpt2d_proj_ds.min(-1) > 0) & (qpt2d_proj_ds[:, 0] < (w // ds)) & (qpt2d_proj_ds[:, 1] < (h // ds))  # :330-334
    qpt2d_ids = qpt2d_proj_ds[:, 0] + qpt2d_proj_ds[:, 1] * (w // ds)                                # :335
    qpt2d_ids = qpt2d_ids.clip(0, M - 1)                                                             # :338
    rpt3d_ids = np.arange(N)                                                                         # :341
    match_gt = np.zeros((M, N)).astype(np.float32)                                                   # :342
    match_gt[qpt2d_ids, rpt3d_ids] = 1.0                                                             # :343
    match_gt = qmask[:, None] * rmask[None, :] * rpt3d_visible[None, :] * match_gt                   # :344-346
    gt_cell = np.where(match_gt.sum(0) > 0, qpt2d_ids, -1).astype(np.int32)
    if match_gt.sum() < 1 and fallback is not None:                                                  # :347-351 (the caller's draw instead of random.random())
        match_gt[int(fallback[0]), int(fallback[1])] = 1.0
    return match_gt.astype(np.float32), gt_cell


def batch_case(tag, Ks, c2ws, pt3d, im_mask, pt_mask, H, W, fallback=None, dense=True, check=True):
    """Runs the reference per sample; returns the arrays of one case and the sample's max |fp32 - fp64| projection error."""
    B = len(pt3d)
    proj32, proj64, cells, dense_m = [], [], [], []
    for b in range(B):
        p32, p64 = project_ref(Ks[b], c2ws[b], pt3d[b]), project_ref(Ks[b], c2ws[b], pt3d[b], f64=True)
        m32, c32 = reference_supervision(p32, H, W, im_mask[b], pt_mask[b], fallback=None if fallback is None else fallback[b])
        _, c64 = reference_supervision(p64, H, W, im_mask[b], pt_mask[b])
        if check:
            frac = np.abs(p64 / DS - np.round(p64 / DS)) * DS
            assert frac.min() >= MARGIN, (tag, b, frac.min())
            assert np.array_equal(c32, c64), (tag, b)
        proj32.append(p32.astype(np.float32)); proj64.append(p64); cells.append(c32); dense_m.append(m32)
    dm = np.stack(dense_m)
    bi, ii, ji = np.where(dm)
    out = {f"{tag}_K": np.stack(Ks), f"{tag}_c2w": np.stack(c2ws), f"{tag}_pt3d": np.stack(pt3d), f"{tag}_im_mask": np.stack(im_mask),
           f"{tag}_pt_mask": np.stack(pt_mask), f"{tag}_hw": np.array([H, W], np.int64), f"{tag}_pt2d_proj": np.stack(proj32),
           f"{tag}_pt2d_proj64": np.stack(proj64), f"{tag}_gt_cell": np.stack(cells), f"{tag}_b_ids": bi.astype(np.int64),
           f"{tag}_i_ids": ii.astype(np.int64), f"{tag}_j_ids": ji.astype(np.int64)}
    if dense:
        out[f"{tag}_conf_gt"] = dm.astype(np.uint8)
    err = np.abs(np.stack(proj32).astype(np.float64) - np.stack(proj64))
    return out, float(err[np.isfinite(err)].max())


def case_a_points(g, K, c2w, H, W, N, pt_mask, im_mask):
    """Hand-placed points first (their roles in the comments), then random cells with an empty band (cell row 3 is never drawn)."""
    Wc, Hc = W // DS, H // DS
    hand = [(3, 0), (5, 0),            # cell row 0: excluded by the strict `> 0`
            (0, 2), (0, 4),            # cell column 0: excluded likewise
            (-1, 2), (Wc, 3),          # outside the left / right border
            (2, -1), (4, Hc),          # outside the top / bottom border
            (2, 2), (5, 4),            # behind the camera, flipped projection inside the image
            (3, 2),                    # pt_mask false
            (6, 1),                    # lands on a cell whose im_mask is false
            (2, 2), (2, 2), (2, 2)]    # three more in cell (2, 2)
    depth = np.full(len(hand), 2.0)
    depth[8:10] = -1.5
    pt_mask[10] = False
    im_mask[6 + 1 * Wc] = False
    rest = N - len(hand)
    cx = g.integers(1, Wc, rest)
    cy = g.choice([1, 2, 4, 5], rest)
    uv = cell_pixels(g, hand + list(zip(cx, cy)))
    depth = np.concatenate([depth, g.uniform(1.0, 4.0, rest)])
    return lift(K, c2w, uv, depth)


def random_cells(g, K, c2w, H, W, N, spill=1):
    Wc, Hc = W // DS, H // DS
    cx, cy = g.integers(-spill, Wc + spill, N), g.integers(-spill, Hc + spill, N)
    return lift(K, c2w, cell_pixels(g, list(zip(cx, cy))), g.uniform(1.0, 4.0, N))


def supervision_fixture():
    out, errs = {}, []
    # ---- A
    H, W, N = 48, 64, 200
    M = (H // DS) * (W // DS)
    g = np.random.default_rng(100)
    cams = [camera(1, H, W, 60.0), camera(2, H, W, 60.0)]
    pt3d, ims, pms = [], [], []
    for K, c2w in cams:
        pm, im = np.ones(N, np.bool_), np.ones(M, np.bool_)
        pt3d.append(case_a_points(g, K, c2w, H, W, N, pm, im))
        pm[g.integers(15, N, 10)] = False
        im[g.integers(0, M, 3)] = False
        ims.append(im); pms.append(pm)
    o, e = batch_case("A", [c[0] for c in cams], [c[1] for c in cams], pt3d, ims, pms, H, W)
    out.update(o); errs.append(e)
    assert (o["A_conf_gt"].sum(1).max() == 1) and (o["A_conf_gt"].sum(2).max() > 1) and (o["A_conf_gt"].sum(2).min() == 0)
    # ---- B: N = 1 and N = 129
    K, c2w = cams[0]
    for n in (1, 129):
        gb = np.random.default_rng(200 + n)
        p = lift(K, c2w, cell_pixels(gb, [(3, 2)]), np.array([2.0])) if n == 1 else random_cells(gb, K, c2w, H, W, n)
        o, e = batch_case(f"B{n}", [K], [c2w], [p], [np.ones(M, np.bool_)], [np.ones(n, np.bool_)], H, W)
        out.update(o); errs.append(e)
    # ---- C: element 0 sees nothing
    gc = np.random.default_rng(300)
    n = 70
    Wc, Hc = W // DS, H // DS
    outside = [(int(x), int(y)) for x, y in zip(gc.choice([-2, -1, 0, Wc, Wc + 1], n), gc.integers(-1, Hc + 1, n))]
    p0 = lift(cams[0][0], cams[0][1], cell_pixels(gc, outside), gc.uniform(1.0, 4.0, n))
    p1 = random_cells(gc, cams[1][0], cams[1][1], H, W, n)
    fb = np.array([[5, 7], [9, 11]], np.int32)
    args = ([c[0] for c in cams], [c[1] for c in cams], [p0, p1], [np.ones(M, np.bool_)] * 2, [np.ones(n, np.bool_)] * 2, H, W)
    o, e = batch_case("C", *args)
    out.update(o); errs.append(e)
    assert not (o["C_b_ids"] == 0).any() and (o["C_b_ids"] == 1).any()
    o, _ = batch_case("Cfb", *args, fallback=fb)
    for k in ("b_ids", "i_ids", "j_ids", "conf_gt"):
        out[f"C_fb_{k}"] = o[f"Cfb_{k}"]
    out["C_fallback"] = fb
    # ---- D: 480 x 640, k = 2 frames of 2400
    H, W, kf, nf = 480, 640, 2, 2400
    M = (H // DS) * (W // DS)
    gd = np.random.default_rng(400)
    K, c2w = camera(3, H, W, 600.0)
    p = random_cells(gd, K, c2w, H, W, kf * nf, spill=2)
    pm, im = gd.uniform(size=kf * nf) > 0.1, gd.uniform(size=M) > 0.05
    o, e = batch_case("D", [K], [c2w], [p], [im], [pm], H, W, dense=False)
    o["D_pt3d"] = o["D_pt3d"].reshape(1, kf, nf, 3)
    o["D_pt_mask"] = o["D_pt_mask"].reshape(1, kf, nf)
    out.update(o); errs.append(e)
    max_err = max(errs)
    out["max_err_px"] = np.float64(max_err)
    print(f"supervision: max |fp32 - fp64| of the reference's projections over A-D = {max_err:.3e} px; bar = 4x = {4 * max_err:.3e} px")
    # ---- P: 4096 points without the margin
    gp = np.random.default_rng(500)
    n = 4096
    uv = np.stack([gp.uniform(-16, W + 16, n), gp.uniform(-16, H + 16, n)], -1)
    p = lift(K, c2w, uv, gp.uniform(1.0, 4.0, n))
    ones_m, ones_n = np.ones(M, np.bool_), np.ones(n, np.bool_)
    p32, p64 = project_ref(K, c2w, p), project_ref(K, c2w, p, f64=True)
    _, c32 = reference_supervision(p32, H, W, ones_m, ones_n)
    _, c64 = reference_supervision(p64, H, W, ones_m, ones_n)
    diff = c32 != c64
    near = (np.abs(p64 / DS - np.round(p64 / DS)) * DS).min(-1) <= 4 * max_err
    assert not (diff & ~near).any() and diff.sum() <= n // 100, (int(diff.sum()), int((diff & ~near).sum()))
    print(f"supervision: property case, the reference's fp32 cells differ from fp64 on {int(diff.sum())} of {n} points, all within the bar of a boundary")
    out.update(P_K=K[None], P_c2w=c2w[None], P_pt3d=p[None], P_pt2d_proj64=p64[None], P_gt_cell64=c64[None], P_hw=np.array([H, W], np.int64))
    np.savez_compressed(mg.OUT / "supervision.npz", **out)
    print("wrote", mg.OUT / "supervision.npz")


if __name__ == "__main__":
    assert mg.REF.exists(), "the reference is only present in the build container"
    mg.install_stubs()
    torch.set_num_threads(8)
    supervision_fixture()
