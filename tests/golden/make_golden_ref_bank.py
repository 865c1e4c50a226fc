#!/usr/bin/env python3
"""Golden vectors of the reference point bank (tests/golden/ref_bank.npz), from the REFERENCE's own load_ref_pts.

    python tests/golden/make_golden_ref_bank.py        # rewrites tests/golden/ref_bank.npz (NM_GOLDEN_OUT=<dir>: elsewhere)

Needs the reference tree (make_golden.py's REF and stub modules).  nerfmatch.datasets.nerfmatch_dataset imports under those stubs, so BOTH
of the following are done for every case:
  * the reference's own NeRFMatchMultiPair.load_ref_pts (nerfmatch_dataset.py:441-518) is called on cache files written to a temporary
    directory in the reference's format (split "test": rids[:k]), once with sample_mode None -- the stacked rows and the FIRST frame's
    rc2w -- and once with sample_mode "rand", sample_pts -1 -- every visible row once, in randperm order, and the LAST frame's rc2w;
  * because that call returns neither the visible set in candidate order nor the per-step counts, :478-502 are restated line by line in
    `trace_ref` around the reference's project_points3d and `rc2w.inverse()`; the generator asserts that the restated visible rows are,
    as a multiset, exactly the rows the reference's call returned.
torch.randperm is not reproduced: what is recorded is `visible`, Nv, the per-step (I, V, union) and both rc2w.

Fixture condition (asserted for every case): every fp64 projection of every candidate into every camera of its row is at least 0.01 px
from each of the four image borders, |depth| >= 1e-3, and the reference's fp32 visibility bits equal its fp64 bits -- for such points
visibility is not a rounding question and the tests demand identical sets.  Also asserted on every step: the reference's float32
comparison `I < V / 3` agrees with the integer test 3 I < V.

Cases, all at 48 x 64 px (img_wh = (64, 48)), D = 4 features whose first column is the row's id (frame * n + row):
  k1       k = 1; some points behind the camera whose flipped projection lands inside the image (they count as visible);
  k3       k = 3, cameras turned so that the sequence is intersect, union, intersect;
  tie      k = 2, N = 60 with exactly 20 points inside camera 0: 3 I == V, the intersection is taken;
  tie_m1   k = 2, N = 40 with exactly 13 points inside camera 0: 3 I == V - 1, the union is taken;
  k10      k = 10 over 6 frames: a frame id occurs more than once;
  scaled   k = 2, one frame cached at 96 x 80 px (width / height differ from img_wh).
Only arrays are written."""
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_golden as mg  # noqa: E402
from make_golden_supervision import lift  # noqa: E402

W, H = 64, 48
D = 4
MARGIN = 0.01
MIN_DEPTH = 1e-3


def look(yaw, pitch, pos, focal=60.0, wh=(W, H)):
    """fp32 (K at resolution wh, c2w 4 x 4): a camera at `pos` turned by yaw (about y) and pitch (about x)."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = Ry @ Rx, pos
    s = wh[0] / W
    K = np.array([[focal * s, 0, wh[0] / 2], [0, focal * s * 1.01, wh[1] / 2], [0, 0, 1]])
    return K.astype(np.float32), c2w.astype(np.float32)


def frame_dict(i, K, c2w, wh):
    return dict(file_path=f"seq1/frame_{i:03d}.color.png", transform_matrix=c2w.tolist(), intrinsics=K.tolist(), width=int(wh[0]), height=int(wh[1]))


def project_ref(frame, pts, dt):
    """:481-496 for one frame: the reference's projection of `pts` (numpy fp32) at the target resolution, computed in dtype dt."""
    from nerfmatch.utils.geometry import project_points3d

    rc2w = torch.tensor(frame["transform_matrix"], dtype=dt)                                       # :482
    rw2c = rc2w.inverse()                                                                          # :483
    WH = torch.tensor((W, H), dtype=dt)                                                            # :486
    sK = torch.from_numpy(np.diag([WH[0] / frame["width"], WH[1] / frame["height"], 1])).to(dt)    # :487-489
    rK = torch.tensor(frame["intrinsics"], dtype=dt)                                               # :490
    return project_points3d(sK @ rK, rw2c[:3, :3], rw2c[:3, 3], torch.tensor(pts).to(dt), ret_depth=True), WH


def trace_ref(frames, rids, rpt3d, check=True):
    """:478-502 restated: -> visible (N,) bool, steps (k, 3) = (I, V, union), the last rc2w.  Asserts the fixture condition."""
    visible = torch.ones(len(rpt3d)).bool()                                                        # :478
    steps = []
    for i, rid in enumerate(rids):                                                                 # :480
        rframe = frames[rid]
        rc2w = torch.tensor(rframe["transform_matrix"], dtype=torch.float32)
        (rpt2d, depth), WH = project_ref(rframe, rpt3d, torch.float32)
        i_visible = (rpt2d >= 0).all(-1) & (rpt2d < WH).all(-1)                                    # :498
        (p64, d64), WH64 = project_ref(rframe, rpt3d, torch.float64)
        if check:
            dist = torch.stack([p64[:, 0].abs(), p64[:, 1].abs(), (p64[:, 0] - W).abs(), (p64[:, 1] - H).abs()]).min()
            assert float(dist) >= MARGIN, (rid, float(dist))
            assert float(d64.abs().min()) >= MIN_DEPTH and float(depth.abs().min()) >= MIN_DEPTH
            assert torch.equal(i_visible, (p64 >= 0).all(-1) & (p64 < WH64).all(-1)), rid
        intersect = visible & i_visible                                                            # :499
        union = visible | i_visible                                                                # :500
        take_union = bool(intersect.sum() < visible.sum() / 3)                                     # :502
        I, V = int(intersect.sum()), int(visible.sum())
        assert take_union == (3 * I < V), (I, V)
        steps.append((I, V, int(take_union)))
        visible = union if take_union else intersect
    return visible, np.array(steps, np.int64), rc2w


def call_ref(frames, rids, cache, sample_mode):
    """The reference's own load_ref_pts on the cache files of `frames`."""
    from nerfmatch.datasets.nerfmatch_dataset import NeRFMatchMultiPair

    me = SimpleNamespace(split="test", pair_topk=len(rids), rframes=frames, scene_dir=str(cache), use_msk=None, sample_mode=sample_mode,
                         img_wh=(W, H), sample_pts=-1)
    return NeRFMatchMultiPair.load_ref_pts(me, list(rids))


def case(tag, cams, whs, pts, rids, out, expect=None):
    """cams: [(K, c2w)] per frame, whs: the frames' own (width, height), pts (F, n, 3) fp32, rids: the query's frame ids."""
    F, n, _ = pts.shape
    frames = [frame_dict(i, K, c2w, wh) for i, ((K, c2w), wh) in enumerate(zip(cams, whs))]
    feat = np.random.default_rng(len(tag)).standard_normal((F, n, D)).astype(np.float32)
    feat[..., 0] = np.arange(F * n).reshape(F, n)
    unnorm = np.diag([2.0, 2.0, 2.0, 1.0]).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        for fr, p, f in zip(frames, pts, feat):
            name = fr["file_path"].replace("/", "_").replace(".color", "").replace(".png", "")
            np.save(Path(tmp) / f"{name}.npy", dict(pt3d=p, unnorm_scene=unnorm, pt_feat=f, pt_color=np.zeros((n, 3), np.float32)))
        s3, sf, sm, su, rc2w_none = call_ref(frames, rids, tmp, None)
        r3, rf, rm, ru, rc2w_rand = call_ref(frames, rids, tmp, "rand")
    visible, steps, rc2w_last = trace_ref(frames, rids, s3)
    assert torch.equal(rc2w_last, rc2w_rand) and torch.equal(rc2w_none, torch.tensor(frames[rids[0]]["transform_matrix"], dtype=torch.float32))
    vis = visible.numpy()
    # the rows the reference returned are the restated visible rows, each once
    assert len(r3) == vis.sum() >= 1 and sorted(rf[:, 0].tolist()) == sorted(sf[vis, 0].tolist())
    order = np.argsort(rf[:, 0], kind="stable"), np.argsort(sf[vis, 0], kind="stable")
    assert np.array_equal(r3[order[0]], s3[vis][order[1]]) and np.array_equal(rf[order[0]], sf[vis][order[1]]) and rm.all() and sm.all()
    if expect is not None:
        assert steps[:, 2].tolist() == expect, (tag, steps.tolist())
    print(f"ref_bank {tag}: k = {len(rids)}, N = {len(s3)}, Nv = {int(vis.sum())}, steps (I, V, union) = {steps.tolist()}")
    out.update({f"{tag}_pt3d": pts, f"{tag}_pt_feat": feat, f"{tag}_c2w": np.stack([c[1] for c in cams]), f"{tag}_K": np.stack([c[0] for c in cams]),
                f"{tag}_frame_wh": np.array(whs, np.float32), f"{tag}_ref_ids": np.array(rids, np.int64), f"{tag}_unnorm_scene": su,
                f"{tag}_stacked_pt3d": s3.astype(np.float32), f"{tag}_stacked_pt_feat": sf.astype(np.float32), f"{tag}_stacked_pt_mask": sm,
                f"{tag}_visible": vis, f"{tag}_n_visible": np.int64(vis.sum()), f"{tag}_steps": steps, f"{tag}_rc2w_none": rc2w_none.numpy(),
                f"{tag}_rc2w_rand": rc2w_rand.numpy()})
    return vis, steps


def pixels(g, m, inside, spill=30.0):
    """m pixels at least 1 px inside the image, or (inside=False) 1 .. spill px outside it."""
    if inside:
        return np.stack([g.uniform(1, W - 1, m), g.uniform(1, H - 1, m)], -1)
    uv = np.stack([g.uniform(-spill, W + spill, m), g.uniform(-spill, H + spill, m)], -1)
    side = g.integers(0, 4, m)
    uv[side == 0, 0] = g.uniform(-spill, -1, (side == 0).sum())
    uv[side == 1, 0] = g.uniform(W + 1, W + spill, (side == 1).sum())
    uv[side == 2, 1] = g.uniform(-spill, -1, (side == 2).sum())
    uv[side == 3, 1] = g.uniform(H + 1, H + spill, (side == 3).sum())
    return uv


def clear_of_borders(frames_cams, whs, pts):
    """which points keep the margin to every border of every camera (fp64)"""
    ok = np.ones(len(pts), bool)
    for (K, c2w), wh in zip(frames_cams, whs):
        (p, d), _ = project_ref(frame_dict(0, K, c2w, wh), pts, torch.float64)
        p, d = p.numpy(), d.numpy()
        dist = np.minimum(np.minimum(np.abs(p[:, 0]), np.abs(p[:, 1])), np.minimum(np.abs(p[:, 0] - W), np.abs(p[:, 1] - H)))
        ok &= (dist >= 10 * MARGIN) & (np.abs(d) >= 10 * MIN_DEPTH)
    return ok


def scattered(g, cams, whs, total, spill=12.0):
    """`total` points, each lifted from a random camera at a random pixel in or around its image, all clear of every camera's borders"""
    got = []
    while sum(len(a) for a in got) < total:
        j = int(g.integers(0, len(cams)))
        uv = np.stack([g.uniform(-spill, W + spill, 64), g.uniform(-spill, H + spill, 64)], -1) * (whs[j][0] / W)
        p = lift(cams[j][0], cams[j][1], uv, g.uniform(1.5, 4.0, 64))
        got.append(p[clear_of_borders(cams, whs, p)])
    return np.concatenate(got)[:total]


def ref_bank_fixture():
    out = {}
    full = (W, H)
    # ---- k1: one camera; 5 points behind it with the flipped projection inside
    g = np.random.default_rng(11)
    cam = look(0.2, -0.1, [0.1, 0.0, -0.2])
    n = 33
    uv = np.concatenate([pixels(g, 14, True), pixels(g, 14, False), pixels(g, 5, True)])
    depth = np.concatenate([g.uniform(1.5, 4.0, 28), -g.uniform(1.5, 4.0, 5)])
    p = lift(cam[0], cam[1], uv, depth)
    assert clear_of_borders([cam], [full], p).all()
    vis, steps = case("k1", [cam], [full], p[None], [0], out)
    assert vis[28:].all() and steps[0].tolist() == [19, 33, 0]
    # ---- k3: camera 0 sees over a third of the points (intersect), camera 1 looks elsewhere (union), camera 2 sees both halves (intersect)
    g = np.random.default_rng(12)
    cams = [look(0.0, 0.0, [0, 0, 0]), look(0.95, 0.0, [0.05, 0, 0]), look(0.47, 0.02, [0.02, 0.01, 0])]
    n = 50
    parts = []
    for j, m in ((0, 60), (1, 50), (2, 40)):
        pj = lift(cams[j][0], cams[j][1], pixels(g, 2 * m, True), g.uniform(2.0, 4.0, 2 * m))
        parts.append(pj[clear_of_borders(cams, [full] * 3, pj)][:m])
    p = np.concatenate(parts)
    assert p.shape == (3 * n, 3)
    case("k3", cams, [full] * 3, p[g.permutation(3 * n)].reshape(3, n, 3), [0, 1, 2], out, expect=[0, 1, 0])
    # ---- the ties of round 0, decided by camera 0 alone
    for tag, n, inside, expect0 in (("tie", 30, 20, 0), ("tie_m1", 20, 13, 1)):
        g = np.random.default_rng(13 + n)
        cams = [look(-0.1, 0.05, [0, 0.1, 0]), look(0.3, 0.0, [0.2, 0, 0.1])]
        uv = np.concatenate([pixels(g, inside, True), pixels(g, 2 * n - inside, False)])
        p = lift(cams[0][0], cams[0][1], uv, g.uniform(1.5, 4.0, 2 * n))
        assert clear_of_borders(cams, [full] * 2, p).all(), tag
        vis, steps = case(tag, cams, [full] * 2, p[g.permutation(2 * n)].reshape(2, n, 3), [0, 1], out)
        assert steps[0].tolist() == [inside, 2 * n, expect0] and (3 * inside == 2 * n - expect0)
    # ---- k10 over 6 frames
    g = np.random.default_rng(15)
    cams = [look(0.12 * f - 0.3, 0.05 * (f % 3) - 0.05, [0.05 * f, 0.02 * f, 0.0]) for f in range(6)]
    n = 24
    p = scattered(g, cams, [full] * 6, 6 * n)
    case("k10", cams, [full] * 6, p.reshape(6, n, 3), [3, 0, 5, 2, 2, 1, 4, 0, 3, 5], out)
    # ---- scaled: frame 0 cached at 96 x 80 px
    g = np.random.default_rng(16)
    whs = [(96, 80), full]
    cams = [look(0.1, 0.0, [0, 0, 0], focal=70.0, wh=whs[0]), look(-0.15, 0.05, [0.1, 0, 0])]
    n = 40
    p = scattered(g, cams, whs, 2 * n)
    case("scaled", cams, whs, p.reshape(2, n, 3), [0, 1], out)
    out["img_wh"] = np.array([W, H], np.int64)
    np.savez_compressed(mg.OUT / "ref_bank.npz", **out)
    print("wrote", mg.OUT / "ref_bank.npz")


if __name__ == "__main__":
    assert mg.REF.exists(), "the reference is only present in the build container"
    mg.install_stubs()
    torch.set_num_threads(8)
    ref_bank_fixture()
