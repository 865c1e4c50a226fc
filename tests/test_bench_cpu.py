"""CPU: bench.py's command line (a plain run is region A alone) and the files of --dump-outputs, no GPU involved."""
import importlib.util
from pathlib import Path

import numpy as np
import torch


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", Path(__file__).resolve().parents[1] / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_is_region_a_alone(monkeypatch):
    import sys

    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_files(tmp_path):
    """What one region-A step returns at the bench's default size: float32 arrays under 64 MB, pt_feat as a seeded sample of rows
    (the same rows in every run), pt3d and im_pred whole; past 16 MB the last two are sampled on the same rows."""
    bench = _bench()
    g = torch.Generator().manual_seed(0)
    Q, R = 16, 4800
    out = dict(im_pred=torch.rand(Q, 60, 80, 3, generator=g), pt3d=torch.rand(Q, R, 3, generator=g), pt_feat=torch.rand(Q, R, 256, generator=g))
    bench.dump_outputs(out, tmp_path / "a")
    got = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(got) == {"im_pred", "pt3d", "pt_feat", "pt_feat_rows"}
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    rows = got["pt_feat_rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_ROWS and len(np.unique(rows)) == len(rows)
    assert np.array_equal(got["pt_feat"], out["pt_feat"].reshape(-1, 256).numpy()[rows])
    assert np.array_equal(got["pt3d"], out["pt3d"].numpy()) and np.array_equal(got["im_pred"], out["im_pred"].numpy())
    bench.dump_outputs(out, tmp_path / "b")
    assert np.array_equal(np.load(tmp_path / "b" / "pt_feat_rows.npy"), got["pt_feat_rows"])
    big = dict(im_pred=torch.rand(200, 60, 80, 3, generator=g), pt3d=torch.rand(200, R, 3, generator=g), pt_feat=torch.zeros(200, R, 256))
    bench.dump_outputs(big, tmp_path / "c")
    rows = np.load(tmp_path / "c" / "pt_feat_rows.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "c" / "pt3d.npy"), big["pt3d"].reshape(-1, 3).numpy()[rows])
    assert np.array_equal(np.load(tmp_path / "c" / "im_pred.npy"), big["im_pred"].reshape(-1, 3).numpy()[rows])
    assert sum(p.stat().st_size for p in (tmp_path / "c").glob("*.npy")) <= 64 << 20
