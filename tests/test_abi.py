"""CPU: the C-ABI library loads and exports every symbol include/nerfmatch_amd.h declares (no compute calls)."""
import re
from pathlib import Path

from nerfmatch_amd import _lib

ROOT = Path(__file__).resolve().parents[1]


def header_symbols():
    txt = (ROOT / "include" / "nerfmatch_amd.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nm_[a-z0-9_]+)\s*\(", txt)))


def test_every_declared_symbol_is_exported_and_bound(built_lib):
    h = _lib.lib()
    syms = header_symbols()
    assert len(syms) >= 20
    assert h._nm_missing == [], f"declared in _lib.SIGNATURES but not exported: {h._nm_missing}"
    for s in syms:
        assert s in _lib.SIGNATURES, f"{s} is declared in the header but has no ctypes signature"
        assert getattr(h, s) is not None
    assert set(_lib.SIGNATURES) == set(syms)


def test_host_only_entry_points(built_lib):
    h = _lib.lib()
    assert h.nm_abi_version() == _lib.ABI_VERSION == 3  # (the literal: a bump is a conscious edit here too)
    assert h.nm_error_string(0) == b"ok" and b"supported" in h.nm_error_string(2)
    assert h.nm_raygen_count(480, 640, 8) == 4800 and h.nm_raygen_count(480, 480, 8) == 3600
    assert h.nm_nerf_blob_floats() == 611856 and h.nm_nerf_blob_bytes_bf16x3() == 16384 + (143 + 4) * 16384  # 143 K-step slots (feature_linear folded into the views layer) + 4 zero slots of run-ahead padding
    assert h.nm_match_workspace_bytes(4800, 4800, 256) > 4800 * 4800 * 4


def test_argument_validation_without_gpu(built_lib):
    """Bad arguments are rejected before anything is enqueued, so this is safe without a device."""
    import ctypes as C
    h = _lib.lib()
    null = C.c_void_p(0)
    assert h.nm_sample_coarse(null, null, 4, 32, null, null) == 1
    assert h.nm_nerf_fwd(null, null, null, null, 1, 32, 0, 0, -1.0, 0, null, null, null, null, null, null, null, null, null) == 1
    assert h.nm_linear(null, null, null, null, null, null, 4, 4, 8, 0, null, null) == 1
    # the weight-gradient kernels move 16-byte row pieces (the split-bf16 one 8-byte pieces of dy): misaligned operands are refused
    buf = (C.c_char * 256)()
    base = (C.addressof(buf) + 15) & ~15
    p, off4, off8 = C.c_void_p(base), C.c_void_p(base + 4), C.c_void_p(base + 8)
    for dy, x, dw in ((off4, p, p), (p, off4, p), (p, p, off4), (off8, p, p), (p, off8, p), (p, p, off8)):
        assert h.nm_linear_wgrad(dy, x, 8, 4, 4, 0, dw, null, 0, null) == _lib.NM_ERR_UNSUPPORTED
    assert h.nm_linear_wgrad(p, p, 8, 6, 4, 0, p, null, 0, null) == _lib.NM_ERR_UNSUPPORTED  # N not a multiple of 4
    assert h.nm_linear_wgrad(null, p, 8, 4, 4, 0, p, null, 0, null) == 1
    assert h.nm_linear_wgrad(p, p, 8, 4, 4, 1, p, null, 0, null) == 4  # aligned: the next check in line (accumulate needs a workspace)
    for dy, x, dw in ((off4, p, p), (p, off8, p), (p, p, off8)):
        assert h.nm_linear_wgrad_bf16x3(dy, x, 8, 4, 4, 0, dw, null, null, 0, null) == _lib.NM_ERR_UNSUPPORTED
    assert h.nm_linear_wgrad_bf16x3(off8, p, 8, 4, 4, 1, p, null, null, 0, null) == 4  # dy needs 8 bytes only


def test_library_of_another_abi_version_is_refused(built_lib, monkeypatch):
    """A stale build may export re-signed symbols under the same names: lib() must not hand it out."""
    import pytest

    monkeypatch.setattr(_lib, "_lib", None)  # (force a fresh load; the loaded handle comes back when the test ends)
    monkeypatch.setattr(_lib, "ABI_VERSION", _lib.ABI_VERSION + 1)
    with pytest.raises(_lib.NerfmatchAmdError, match="ABI version 3"):
        _lib.lib()
